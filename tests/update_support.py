"""What the tests of the one-call update share (test_learn_update_cpu.py, test_gpu_learner_update.py): the numpy reference of the permutation
that include/so100_learn.h specifies, written from the header's text over oracle.so100_oracle.philox4x32_np -- it shares no line with
csrc/so100_learn.hpp -- and the host twin of that header's shuffle_index, tests/_shufflecheck/libshufflecheck.so, built and loaded here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from oracle.so100_oracle import philox4x32_np

HERE = os.path.dirname(os.path.abspath(__file__))
SHUFFLE_STREAM = 0x53484633
ROUNDS = 6

_twin = None


def shufflecheck():
    """the host twin: sc_shuffle(seed, epoch, n, out int64[n]), sc_shuffle_epochs(seed, epoch0, epochs, n, out int32[epochs][n])"""
    global _twin
    if _twin is None:
        d = os.path.join(HERE, "_shufflecheck")
        subprocess.check_call(["make", "-C", d, "-s"])
        lib = C.CDLL(os.path.join(d, "libshufflecheck.so"))
        lib.sc_shuffle.restype, lib.sc_shuffle.argtypes = None, [C.c_ulonglong, C.c_uint, C.c_long, C.c_void_p]
        lib.sc_shuffle_epochs.restype, lib.sc_shuffle_epochs.argtypes = None, [C.c_ulonglong, C.c_uint, C.c_int, C.c_int, C.c_void_p]
        _twin = lib
    return _twin


def twin_perm(seed, epoch, n):
    out = np.empty(n, np.int64)
    shufflecheck().sc_shuffle(seed, epoch, n, out.ctypes.data_as(C.c_void_p))
    return out


def twin_perms(seed, epoch0, epochs, n):
    out = np.empty((epochs, n), np.int32)
    shufflecheck().sc_shuffle_epochs(seed, epoch0, epochs, n, out.ctypes.data_as(C.c_void_p))
    return out


def _feistel(x, h, mask, seed, epoch, rounds):
    """one pass of the network over an array of domain elements"""
    left, right = x >> np.uint64(h), x & mask
    for r in range(rounds):
        f = philox4x32_np(right, r, epoch, SHUFFLE_STREAM, seed & 0xFFFFFFFF, seed >> 32)[..., 0] & mask
        left, right = right, left ^ f
    return (left << np.uint64(h)) | right


def ref_perm(seed, epoch, n, rounds=ROUNDS):
    """perm(i) for every i in [0, n) as int64, from the header: all positions walk at once, each until it lands below n"""
    if n == 1:
        return np.zeros(1, np.int64)
    bits = max(1, int(n - 1).bit_length())
    h = (bits + 1) // 2
    mask = np.uint64((1 << h) - 1)
    seed, epoch = int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF
    x = _feistel(np.arange(n, dtype=np.uint64), h, mask, seed, epoch, rounds)
    walking = np.nonzero(x >= n)[0]
    while walking.size:
        x[walking] = _feistel(x[walking], h, mask, seed, epoch, rounds)
        walking = walking[x[walking] >= n]
    return x.astype(np.int64)


@functools.lru_cache(maxsize=None)
def ref_perm_cached(seed, epoch, n):
    p = ref_perm(seed, epoch, n)
    p.setflags(write=False)
    return p
