"""The one-call update without a device: the permutation of include/so100_learn.h -- csrc/so100_learn.hpp's shuffle_index instantiated on
the host (tests/_shufflecheck) against the numpy reference of update_support.py, for every index -- its uniformity, and the new interface:
struct mirror, argument errors that need no handle, no CPU fallback, the option errors of FusedPPO and of the command line.  CPU only.

Uniformity bounds.  They are conditions on the construction, set before the twin was run: a uniform permutation gives a chi-square z of
order 1, a spread of pair frequencies of 1 x the binomial sigma with a relative standard error of 1/sqrt(2 x pairs) (1.7 % for the 1770
pairs of n = 60, 0.4 % for the 32 896 of n = 257), and a largest deviation over that many pairs of 3.5 to 4.5 sigma.  Four Feistel rounds
on 3-bit halves give a spread of 1.11 and fail; six give 1.02."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import update_support as US

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 5, 17, 63, 64, 65, 257, 780, 4097, 262144, 262145]
SEEDS = [0, 99, 0xDEADBEEF12345678]
EPOCHS = [0, 7, 2 ** 32 - 1]


# ---- 1. the twin against numpy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_twin_equals_the_numpy_reference_for_every_index(n):
    seen = {}
    for seed in SEEDS:
        for epoch in EPOCHS:
            got = US.twin_perm(seed, epoch, n)
            assert np.array_equal(got, US.ref_perm(seed, epoch, n)), (seed, epoch)
            assert np.array_equal(np.sort(got), np.arange(n)), (seed, epoch)             # a permutation of range(n)
            seen[(seed, epoch)] = got
    if n >= 64:                                                                            # another epoch or seed: another permutation
        keys = list(seen)
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert not np.array_equal(seen[a], seen[b]), (a, b)


def test_the_reference_with_four_rounds_is_another_permutation():
    """the round count is part of the contract: the reference run with four rounds does not reproduce the twin"""
    assert not np.array_equal(US.ref_perm(99, 0, 257, rounds=4), US.twin_perm(99, 0, 257))


# ---- 2. uniformity ------------------------------------------------------------------------------------------------------------------------------
def _pair_counts(perms, mb):
    """[n, n] how often two rows shared a minibatch, and the probability of that under a uniform permutation"""
    epochs, n = perms.shape
    k = (n + mb - 1) // mb
    member = np.zeros((epochs, n, k), np.float32)                                          # member[e, row, minibatch]
    e_idx = np.repeat(np.arange(epochs), n)
    member[e_idx, perms.reshape(-1), np.tile(np.arange(n) // mb, epochs)] = 1.0
    counts = np.einsum("enk,emk->nm", member, member).astype(np.float64)
    sizes = np.bincount(np.arange(n) // mb).astype(np.float64)
    return counts, float((sizes * (sizes - 1)).sum() / (n * (n - 1)))


def _pair_figures(perms, mb):
    epochs, n = perms.shape
    counts, p = _pair_counts(perms, mb)
    c = counts[np.triu_indices(n, 1)]
    sigma = np.sqrt(epochs * p * (1 - p))
    dev = (c - epochs * p) / sigma
    return float(np.sqrt((dev ** 2).mean())), float(np.abs(dev).max())


@pytest.mark.parametrize("seed", [99, 5, 0xDEADBEEF12345678])
def test_small_permutations_are_uniform(seed):
    n, mb, epochs = 60, 15, 4000
    perms = US.twin_perms(seed, 0, epochs, n)
    assert np.array_equal(np.sort(perms, axis=1), np.tile(np.arange(n), (epochs, 1)))
    table = np.zeros((n, n))                                                               # table[position, row]
    np.add.at(table, (np.tile(np.arange(n), epochs), perms.reshape(-1)), 1.0)
    expect = epochs / n
    chi2 = ((table - expect) ** 2 / expect).sum()
    dof = (n - 1) ** 2
    z = (chi2 - dof) / np.sqrt(2 * dof)
    spread, worst = _pair_figures(perms, mb)
    print(f"[shuffle] n {n} seed {seed:#x}: chi-square z {z:+.2f}  pair spread {spread:.4f}  worst pair {worst:.2f} sigma")
    assert abs(z) <= 4
    assert spread <= 1.06
    assert worst <= 5.5


@pytest.mark.parametrize("seed", [99, 5, 0xDEADBEEF12345678])
def test_odd_sized_permutations_are_uniform(seed):
    n, mb, epochs = 257, 64, 1500                                                          # four minibatches of 64 and one of a single row
    perms = US.twin_perms(seed, 0, epochs, n)
    spread, worst = _pair_figures(perms, mb)
    print(f"[shuffle] n {n} seed {seed:#x}: pair spread {spread:.4f}  worst pair {worst:.2f} sigma")
    assert 0.97 <= spread <= 1.03
    assert worst <= 6


# ---- 3. the interface ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib.load()


def test_update_struct_matches_the_header():
    """field names and order of so100_update_io as the header declares them; the size of its output block"""
    from so100_mujoco_rl_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "so100_learn.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} so100_update_io;", src).group(1)
    names = []
    for decl in body.split(";"):
        names += [w.strip(" *") for w in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip(), count=1).split(",") if w.strip()]
    assert names == [f[0] for f in lib.UpdateIO._fields_]
    assert int(re.search(r"#define SO100_UPDATE_OUT (\d+)", src).group(1)) == lib.UPDATE_OUT == 15
    # x86-64 layout: 3 pointers, 2 int32, 7 pointers, 4 x 32 bit, one 64 bit, 3 pointers
    assert C.sizeof(lib.UpdateIO) == 3 * 8 + 8 + 7 * 8 + 16 + 8 + 3 * 8
    assert "so100_learner_shuffle" in lib.LEARN_EXPORTS and "so100_learner_update" in lib.LEARN_EXPORTS
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_null_arguments_are_refused_without_a_device(L):
    from so100_mujoco_rl_amd import lib
    assert L.so100_learner_shuffle(None, 0, 0, 8, None, None) == -1
    assert L.so100_last_error() == b"so100_learner_shuffle: null argument"
    assert L.so100_learner_update(None, C.byref(lib.UpdateIO()), None) == -1
    assert L.so100_last_error() == b"so100_learner_update: null argument"
    assert L.so100_learner_update(None, None, None) == -1
    assert L.so100_last_error() == b"so100_learner_update: null argument"


def test_device_shuffle_has_no_cpu_fallback_and_refuses_injected_permutations():
    from so100_mujoco_rl_amd import lib
    from so100_mujoco_rl_amd.ppo import FusedPPO
    od = 15
    b = {"obs": torch.zeros(2, 3, od), "actions": torch.zeros(2, 3, 6), "rewards": torch.zeros(2, 3), "dones": torch.zeros(2, 3),
         "values": torch.zeros(2, 3), "log_probs": torch.zeros(2, 3), "last_obs": torch.zeros(3, od)}
    f = FusedPPO(od, "cpu", seed=4, shuffle="device")
    assert (f.shuffle, f.shuffle_seed, f.shuffle_epoch) == ("device", 4, 0)
    with pytest.raises(ValueError, match="perms"):
        f.update(b, perms=[torch.arange(6)])
    with pytest.raises(lib.So100Error, match="no CPU fallback"):
        f.update(b)
    assert f.shuffle_epoch == 0
    assert FusedPPO(od, "cpu").shuffle == "torch"
    with pytest.raises(ValueError, match="shuffle"):
        FusedPPO(od, "cpu", shuffle="host")


@pytest.mark.parametrize("learner", [[], ["--learner", "torch"]])
def test_cli_device_shuffle_needs_the_fused_learner(tmp_path, monkeypatch, learner):
    from so100_mujoco_rl_amd import main as drv
    monkeypatch.chdir(tmp_path)
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "-e", "Env01-v1", "--shuffle", "device"] + learner)
    assert r.exit_code != 0 and isinstance(r.exception, RuntimeError) and "--learner fused" in str(r.exception)
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "--help"])
    assert r.exit_code == 0 and "--shuffle" in r.output
