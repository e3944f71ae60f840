"""What the tests of the one-call update share (test_learn_update_cpu.py, test_gpu_learner_update.py): the numpy reference of the permutation
that include/so100_learn.h specifies, written from the header's text over oracle.so100_oracle.philox4x32_np -- it shares no line with
csrc/so100_learn.hpp -- and the calls into the host twin of that header's shuffle_index (tests/_learncheck/shufflecheck.cpp in hostlibs.learncheck())."""
import functools

import numpy as np

import hostlibs
from hostlibs import ptr
from oracle.so100_oracle import philox4x32_np

SHUFFLE_STREAM = 0x53484633
ROUNDS = 6


def twin_perm(seed, epoch, n):
    """sc_shuffle(seed, epoch, n, out int64[n])"""
    out = np.empty(n, np.int64)
    hostlibs.learncheck().sc_shuffle(seed, epoch, n, ptr(out))
    return out


def twin_perms(seed, epoch0, epochs, n):
    """sc_shuffle_epochs(seed, epoch0, epochs, n, out int32[epochs][n])"""
    out = np.empty((epochs, n), np.int32)
    hostlibs.learncheck().sc_shuffle_epochs(seed, epoch0, epochs, n, ptr(out))
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
