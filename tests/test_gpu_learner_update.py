"""The whole PPO update in one C-ABI call (so100_learner_shuffle, so100_learner_update, ppo.FusedPPO(shuffle="device"), examples/train_ppo.cpp,
`train --shuffle device`) on the GPU: the device permutation against the numpy reference of update_support.py, one call against the same
launches made by hand (to the bit), the result against the fp64 reference of learn_support.py fed the NUMPY permutations, the Python learner
against manual calls and against the PyTorch learner, the argument errors that need a handle, the plain C++ trainer and the command line.

Tolerances.  The fp64 comparisons use the bounds the project already holds for the same quantities: PARAM_REF_TOL / MOMENT_TOL of
test_gpu_learner.py for the plain step, PARAM_TOL / MOMENT_TOL of test_gpu_learner_terms.py for the extended one, E2E_STAT_TOL for the diagnostics
against the fp32 PyTorch learner.  Each figure is printed as `[update-tol] name value` before it is asserted.  The reference is the fp64 one on
the numpy permutations, never the stepwise kernels and never the device's permutation."""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import learn_support as LS
import update_support as US
from learn_support import make_learner, state_dict
from test_gpu_learner import MOMENT_TOL as PLAIN_MOMENT_TOL, PARAM_REF_TOL as PLAIN_PARAM_TOL
from test_gpu_learner_terms import E2E_STAT_TOL, MOMENT_TOL, PARAM_TOL, chunk, reference_advantages, update_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CT, CN = 6, 130                                   # the chunk of learn_support.make_chunk: 780 rows
ROWS = CT * CN
EPOCHS, MB = 3, 257                               # three full minibatches and one of 9 rows per epoch: 12 steps
STOP_LR = 3e-3
# (shuffle seed, first epoch) per observation width: under these the fp64 reference's approx_kl has a step inside the SECOND epoch that
# exceeds every earlier one by 20 % or more (kl_stop_step asserts it), so a target between the two stops there in fp32 as well
STOP_SHUFFLE = {15: (11, 4), 8: (14, 0)}


def report(name, value):
    print(f"[update-tol] {name} {value:.3e}")
    return value


def ref_perms(seed, e0, epochs=EPOCHS, n=ROWS):
    return [torch.from_numpy(US.ref_perm_cached(seed, (e0 + e) & 0xFFFFFFFF, n).copy()) for e in range(epochs)]


def minibatches(perms, mb):
    return [p[i:i + mb] for p in perms for i in range(0, len(p), mb)]


# ---- so100_learner_shuffle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 4097, 262144, 262145])
def test_device_shuffle_equals_the_numpy_reference(n):
    """wave and block edges, odd and even bit counts, 4^9 (no walk) and 4^9 + 1 (a domain of four times n)"""
    L = make_learner(15, 64)
    for seed, epoch in ((99, 0), (0xDEADBEEF12345678, 2 ** 32 - 1)):
        out = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        L.shuffle(seed, epoch, n, out)
        assert np.array_equal(out.cpu().numpy(), US.ref_perm_cached(seed, epoch, n)), (seed, epoch)


# ---- one call against the same launches by hand ---------------------------------------------------------------------------------------------------
class Buffers:
    """the caller-owned tensors of one update from the shared initial weights; out and state start from values no launch writes"""

    def __init__(self, L, od, extended):
        P = L.num_params
        self.params = LS.flat_params(state_dict(od), od, DEV); self.m = torch.zeros(P, device=DEV); self.v = torch.zeros(P, device=DEV)
        self.adv = torch.full((CT, CN), 3.0, device=DEV); self.ret = torch.full((CT, CN), 3.0, device=DEV); self.adv_stats = torch.full((2,), 3.0, device=DEV)
        self.perm = torch.full((ROWS,), -1, dtype=torch.int64, device=DEV)
        self.out = torch.full((15,), 7.0, device=DEV)
        self.state = torch.full((2,), 7, dtype=torch.int32, device=DEV) if extended else None

    def everything(self):
        return [self.params, self.m, self.v, self.adv, self.ret, self.adv_stats, self.perm, self.out] + ([self.state] if self.state is not None else [])


def by_hand(L, od, b, tobs, terms, mb, seed, e0, step0, epochs=EPOCHS):
    """what so100_learner_update documents, through the stepwise entry points: advantages, explained variance, the zeroed state, per epoch the
    shuffle and the steps over perm[k mb:(k+1) mb], log_std copied before the last step"""
    from so100_mujoco_rl_amd import lib
    B = Buffers(L, od, terms is not None)
    off = lib.learner_layout(od)[0]["log_std"][0]
    L.advantages(b["packed"], b["last_obs"], B.params, B.adv, B.ret, B.adv_stats, terminal_obs=tobs)
    L.explained_variance(b["packed"], B.ret, B.out[8:9])
    if B.state is not None:
        B.state.zero_()
    step, last = step0, step0 + epochs * math.ceil(ROWS / mb)
    for e in range(epochs):
        L.shuffle(seed, e0 + e, ROWS, B.perm)
        for i in range(0, ROWS, mb):
            step += 1
            if step == last:
                B.out[9:15].copy_(B.params[off:off + 6])
            if terms is None:
                L.minibatch_step(b["packed"], B.perm[i:i + mb], B.adv, B.ret, B.adv_stats, B.params, B.m, B.v, step, B.out[0:4])
            else:
                L.minibatch_step_ex(b["packed"], B.perm[i:i + mb], B.adv, B.ret, B.adv_stats, B.params, B.m, B.v, step, B.out[0:8], update_state=B.state, **terms)
    return B


def one_call(L, od, b, tobs, terms, mb, seed, e0, step0, epochs=EPOCHS):
    B = Buffers(L, od, terms is not None)
    L.update(b["packed"], b["last_obs"], B.params, B.m, B.v, B.adv, B.ret, B.adv_stats, B.perm, B.out, epochs=epochs, mb=mb, adam_step0=step0,
             shuffle_seed=seed, shuffle_epoch0=e0, terminal_obs=tobs, terms=terms, update_state=B.state)
    return B


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


PLAIN, ALL = None, LS.ALL_TERMS
BIT_CASES = [(15, PLAIN, 257, 0, True), (15, ALL, 257, 0, True), (8, PLAIN, 257, 5, False), (8, ALL, 257, 5, True),
             (15, ALL, 780, 0, False), (15, PLAIN, 780, 5, True), (15, PLAIN, 1, 5, True), (8, ALL, 1, 0, True)]


@pytest.mark.parametrize("od,terms,mb,step0,with_tobs", BIT_CASES, ids=lambda v: "all" if v is ALL else "plain" if v is None else str(v))
def test_one_call_equals_the_steps_by_hand_to_the_bit(od, terms, mb, step0, with_tobs):
    L = make_learner(od, 780)
    b = update_batch(od)
    tobs = b["terminal_obs"] if with_tobs else None
    seed, e0 = 5, 2 ** 32 - 2                                      # the epoch counter wraps inside the update
    H = by_hand(L, od, b, tobs, terms, mb, seed, e0, step0)
    U = one_call(L, od, b, tobs, terms, mb, seed, e0, step0)
    names = ["params", "adam_m", "adam_v", "adv", "ret", "adv_stats", "perm", "out", "state"]
    for name, h, u in zip(names, H.everything(), U.everything()):
        assert same_bits(h, u), name
    steps = EPOCHS * math.ceil(ROWS / mb)
    if terms is not None:
        assert U.state.tolist() == [0, steps]
    assert np.array_equal(U.perm.cpu().numpy(), US.ref_perm_cached(seed, (e0 + EPOCHS - 1) & 0xFFFFFFFF, ROWS))      # the last epoch's permutation
    assert float((U.params - LS.flat_params(state_dict(od), od, DEV)).abs().max()) > 2e-4      # the net moved: Adam's first step alone is lr = 3e-4
    out = U.out.tolist()
    assert out[4:8] == [7.0] * 4 if terms is None else all(math.isfinite(x) for x in out[4:8])                      # the plain step writes four
    assert all(math.isfinite(x) for x in out[0:4] + out[8:15])


@functools.lru_cache(maxsize=None)
def reference_run(od, extended, target_kl, seed, e0):
    """the fp64 reference over the NUMPY permutations: (learner, the diagnostics of the steps evaluated)"""
    buf = chunk(od)[0]
    kw = dict(lr=STOP_LR, target_kl=target_kl, **LS.ALL_TERMS) if extended else {}
    ref = LS.RefLearner(od, state_dict(od), **kw)
    adv, ret, mean, std = reference_advantages(od)
    steps = [ref.step(buf, idx, adv, ret, mean, std)[0] for idx in minibatches(ref_perms(seed, e0), MB)]
    return ref, [st for st in steps if st is not None]


def kl_stop_step(od):
    """(s, target_kl): the first step s of the second epoch whose fp64 approx_kl is at least 1.2 x every earlier one, and 1.5 target_kl at
    the geometric mean of the two -- 9.5 % away from either side, which fp32 (1.5e-5 on approx_kl) cannot cross"""
    k = [st["approx_kl"] for st in reference_run(od, True, None, *STOP_SHUFFLE[od])[1]]
    assert len(k) == 12
    picks = [s for s in range(5, 9) if k[s - 1] >= 1.2 * max(k[:s - 1])]
    assert picks, k
    s = picks[0]
    return s, math.sqrt(k[s - 1] * max(k[:s - 1])) / 1.5


@pytest.mark.parametrize("od", [15, 8])
def test_a_kl_stop_inside_the_second_epoch_is_the_same_in_one_call(od):
    s, target = kl_stop_step(od)
    seed, e0 = STOP_SHUFFLE[od]
    terms = dict(target_kl=target, lr=STOP_LR, **LS.ALL_TERMS)
    L = make_learner(od, 780)
    b = update_batch(od)
    H = by_hand(L, od, b, b["terminal_obs"], terms, MB, seed, e0, 0)
    U = one_call(L, od, b, b["terminal_obs"], terms, MB, seed, e0, 0)
    for name, h, u in zip(["params", "adam_m", "adam_v", "adv", "ret", "adv_stats", "perm", "out", "state"], H.everything(), U.everything()):
        assert same_bits(h, u), name
    assert U.state.tolist() == [1, s - 1]                          # stopped; the steps before s were applied and nothing after
    # a run that was simply given s - 1 steps ends with the same parameters and moments: nothing after the stop was applied
    B = Buffers(L, od, True)
    L.advantages(b["packed"], b["last_obs"], B.params, B.adv, B.ret, B.adv_stats, terminal_obs=b["terminal_obs"])
    for step, idx in enumerate(minibatches(ref_perms(seed, e0), MB)[:s - 1], 1):
        L.minibatch_step_ex(b["packed"], idx.to(DEV), B.adv, B.ret, B.adv_stats, B.params, B.m, B.v, step, B.out[0:8], lr=STOP_LR, **LS.ALL_TERMS)
    assert same_bits(B.params, U.params) and same_bits(B.m, U.m) and same_bits(B.v, U.v)


# ---- against the fp64 reference on the numpy permutations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("od,kind", [(15, "plain"), (8, "plain"), (15, "stop"), (8, "stop"), (15, "free")])
def test_one_call_matches_the_fp64_reference(od, kind):
    """plain: the default step, 12 steps at lr 3e-4.  stop / free: every option on at lr 3e-3, with the stop above / without one (12 steps)."""
    seed, e0 = STOP_SHUFFLE[od]
    extended = kind != "plain"
    s, target = kl_stop_step(od) if kind == "stop" else (13, None)
    ref, steps = reference_run(od, extended, target, seed, e0)
    assert ref.applied == s - 1 and ref.stopped == (kind == "stop")
    L = make_learner(od, 780, lr=STOP_LR if extended else LS.HYPER["lr"])
    b = update_batch(od)
    terms = dict(target_kl=target, **LS.ALL_TERMS) if extended else None
    U = one_call(L, od, b, b["terminal_obs"], terms, MB, seed, e0, 0)
    if extended:
        assert U.state.tolist() == [int(kind == "stop"), s - 1]
    want = ref.net.state_dict(); mom = ref.moments()
    got_p, got_m, got_v = LS.split_flat(U.params, od), LS.split_flat(U.m, od), LS.split_flat(U.v, od)
    ep = report(f"params od{od} {kind}", max(LS.rel_err(got_p[n], want[n]) for n in want))
    em = report(f"exp_avg od{od} {kind}", max(LS.rel_err(got_m[n], mom[n][0]) for n in want))
    ev = report(f"exp_avg_sq od{od} {kind}", max(LS.rel_err(got_v[n], mom[n][1]) for n in want))
    p_tol, m_tol = (PARAM_TOL, MOMENT_TOL) if extended else (PLAIN_PARAM_TOL, PLAIN_MOMENT_TOL)
    assert ep <= p_tol and em <= m_tol and ev <= m_tol
    assert max(float((got_p[n] - state_dict(od)[n].double()).abs().max()) for n in want) > 1e-3


# ---- ppo.FusedPPO(shuffle="device") ---------------------------------------------------------------------------------------------------------------
def fused(od, shuffle, **kw):
    from so100_mujoco_rl_amd.ppo import FusedPPO
    f = FusedPPO(od, DEV, epochs=EPOCHS, minibatch=MB, seed=21, shuffle=shuffle, **kw)
    f.net.load_state_dict({k: v.to(DEV) for k, v in state_dict(od).items()})
    return f


@pytest.mark.parametrize("od,terms", [(15, PLAIN), (8, ALL)], ids=["od15-plain", "od8-all"])
def test_fused_ppo_device_updates_equal_manual_update_calls(od, terms):
    f = fused(od, "device", **(terms or {}))
    b = update_batch(od)
    s1 = f.update(b); s2 = f.update(b)
    assert (f.shuffle_epoch, f.adam_step, s1["n_updates"], s2["n_updates"]) == (2 * EPOCHS, 24, 12, 12)
    L = make_learner(od, MB)
    B = Buffers(L, od, terms is not None)
    for k in range(2):
        L.update(b["packed"], b["last_obs"], B.params, B.m, B.v, B.adv, B.ret, B.adv_stats, B.perm, B.out, epochs=EPOCHS, mb=MB, adam_step0=12 * k,
                 shuffle_seed=21, shuffle_epoch0=EPOCHS * k, terminal_obs=b["terminal_obs"], terms=terms, update_state=B.state)
    assert same_bits(f.params, B.params) and same_bits(f.adam_m, B.m) and same_bits(f.adam_v, B.v) and same_bits(f._perm, B.perm)
    out = B.out.tolist()
    assert [s2[k] for k in ("policy_loss", "value_loss", "clip_fraction", "grad_norm", "explained_variance")] == out[0:4] + [out[8]]
    assert s1["value_loss"] != s2["value_loss"]


def test_device_shuffle_does_not_depend_on_the_torch_generator():
    """the point of the feature: one seed, the same bits, whatever else drew from torch in between; with shuffle="torch" the same pair differs"""
    od = 15
    b = update_batch(od)
    got = {}
    for shuffle in ("device", "torch"):
        for torch_seed in (123, 456):
            f = fused(od, shuffle)
            torch.manual_seed(torch_seed)
            f.update(b)
            got[shuffle, torch_seed] = f.params.clone()
    assert same_bits(got["device", 123], got["device", 456])
    assert not torch.equal(got["torch", 123], got["torch", 456])


def test_fused_ppo_device_diagnostics_against_the_torch_learner(monkeypatch):
    """ppo.PPO (fp32 PyTorch autograd) on the numpy permutations, FusedPPO on the device's; every option on, a target_kl that never fires.
    The batch carries no terminal observations: ppo.PPO takes the rewards as they are, and so then does the advantage kernel."""
    from so100_mujoco_rl_amd.ppo import PPO
    od = 15
    opts = dict(target_kl=5.0, **LS.ALL_TERMS)
    b = update_batch(od)
    del b["terminal_obs"]
    f = fused(od, "device", **opts)
    s_f = f.update(b)
    t = PPO(od, DEV, epochs=EPOCHS, minibatch=MB, seed=21, **opts)
    t.net.load_state_dict({k: v.to(DEV) for k, v in state_dict(od).items()})
    perms = iter(ref_perms(21, 0))
    monkeypatch.setattr(torch, "randperm", lambda n, device=None: next(perms).to(device))
    s_t = t.update(b)
    monkeypatch.undo()
    assert s_f["n_updates"] == s_t["n_updates"] == 12 and not s_f["early_stop"] and not s_t["early_stop"]
    errs = {k: report(f"fused-device vs torch {k}", abs(s_f[k] - s_t[k]) / max(abs(s_t[k]), 1e-2))
            for k in ("value_loss", "approx_kl", "entropy_loss", "loss", "explained_variance", "std", "mean_reward")}
    assert all(e <= E2E_STAT_TOL for e in errs.values()), (errs, s_f, s_t)


# ---- argument errors that need a live handle ------------------------------------------------------------------------------------------------------
def test_rejected_update_calls_leave_code_message_and_a_working_handle():
    import ctypes as C
    from so100_mujoco_rl_amd import lib
    od, T, n = 15, 2, 16
    learner = lib.So100Learner(od, max_minibatch=64)
    L, stream = learner.L, learner._stream()
    f = dict(dtype=torch.float32, device=DEV)
    buf = torch.zeros(T, n, od + 10, **f); last_obs = torch.zeros(n, od, **f)
    params = torch.zeros(learner.num_params, **f); adam_m, adam_v = torch.zeros_like(params), torch.zeros_like(params)
    adv, ret, adv_stats, out = torch.zeros(T, n, **f), torch.zeros(T, n, **f), torch.zeros(2, **f), torch.zeros(15, **f)
    perm = torch.zeros(T * n, dtype=torch.int64, device=DEV)
    p = lambda t: t.data_ptr()
    kl = lib.PpoTerms(0.0, 0.0, 0, 0.01, -1.0)
    nan_terms = lib.PpoTerms(float("nan"), 0.0, 0, 0.0, -1.0)

    def io(**over):
        kw = dict(rollout_dev=p(buf), last_obs_dev=p(last_obs), T=T, N=n, params_dev=p(params), adam_m_dev=p(adam_m), adam_v_dev=p(adam_v), adv_dev=p(adv),
                  ret_dev=p(ret), adv_stats_dev=p(adv_stats), perm_dev=p(perm), epochs=1, mb=T * n, adam_step0=0, shuffle_seed=1, out_dev=p(out))
        kw.update(over)
        return lib.UpdateIO(**kw)

    upd = lambda **over: (lambda: L.so100_learner_update(learner.h, C.byref(io(**over)), stream))
    shf = lambda n_, ptr: (lambda: L.so100_learner_shuffle(learner.h, 1, 0, n_, ptr, stream))
    calls = [
        (lambda: L.so100_learner_update(learner.h, None, stream), b"so100_learner_update: null argument"),
        (upd(T=0), b"so100_learner_update: T must be >= 1, got 0"),
        (upd(N=-3), b"so100_learner_update: N must be >= 1, got -3"),
        (upd(epochs=0), b"so100_learner_update: epochs must be >= 1, got 0"),
        (upd(mb=0), b"so100_learner_update: mb must be in 1..max_minibatch, got 0"),
        (upd(mb=65), b"so100_learner_update: mb must be in 1..max_minibatch, got 65"),
        (upd(adam_step0=-1), b"so100_learner_update: adam_step0 must be >= 0, got -1"),
        (upd(T=4097, N=4096), b"so100_learner_update: T*N must be <= 16777216, got 16781312"),
        (upd(adam_step0=2 ** 31 - 1), b"so100_learner_update: adam_step0 + epochs*ceil(T*N/mb) must fit 31 bits"),
        (upd(perm_dev=None), b"so100_learner_update: rollout/last_obs/params/adam_m/adam_v/adv/ret/adv_stats/perm/out pointers are required"),
        (upd(out_dev=None), b"so100_learner_update: rollout/last_obs/params/adam_m/adam_v/adv/ret/adv_stats/perm/out pointers are required"),
        (upd(terms=C.pointer(kl)), b"so100_learner_update: target_kl needs the update-state pointer"),
        (upd(terms=C.pointer(nan_terms)), b"so100_learner_update: ent_coef must be >= 0"),
        (shf(0, p(perm)), b"so100_learner_shuffle: n must be in 1..1073741824, got 0"),
        (shf(2 ** 30 + 1, p(perm)), b"so100_learner_shuffle: n must be in 1..1073741824, got 1073741825"),
        (shf(T * n, None), b"so100_learner_shuffle: the perm pointer is required"),
    ]
    current = torch.cuda.current_device()
    for call, msg in calls:
        adv.fill_(5.0)
        assert call() == -1, msg
        assert L.so100_last_error() == msg
        torch.cuda.synchronize()
        assert bool((adv == 5.0).all())                            # a rejected call enqueued nothing
        learner.update(buf, last_obs, params, adam_m, adam_v, adv, ret, adv_stats, perm, out, epochs=1, mb=T * n, adam_step0=0, shuffle_seed=1)
        assert torch.cuda.current_device() == current
    torch.cuda.synchronize()
    assert torch.isfinite(adv).all() and sorted(perm.tolist()) == list(range(T * n))
    learner.close()


# ---- the plain C++ trainer and the command line ---------------------------------------------------------------------------------------------------
TRAINER_SCALE = [0.25, 0.0, 0.125, 0.0, 0.01, 0.0, 0.0, 0.25, 0.0, 0.125, 0.0, 0.125, 0.0]      # kScale of examples/train_ppo.cpp, in POLICY_TENSORS order


def test_plain_cpp_trainer_matches_the_same_loop_in_python(tmp_path):
    """examples/train_ppo.cpp: so100_rollout + so100_learner_update from C++ with raw hipMalloc'ed buffers, no Python and no torch.  The same
    loop through So100Sim.rollout and So100Learner.update ends with the same parameters; their fp64 sum is compared as printed."""
    from so100_mujoco_rl_amd import lib
    exe = str(tmp_path / "train_ppo")
    libdir = os.path.join(ROOT, "so100_mujoco_rl_amd")
    hipdir = os.path.join(os.path.dirname(torch.__file__), "lib")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-o", exe, os.path.join(ROOT, "examples", "train_ppo.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + libdir, "-lso100sim", "-Wl,-rpath," + libdir, "-Wl,-rpath," + hipdir])
    n, iters, seed, T, epochs = 64, 3, 7, 64, 4
    text = subprocess.check_output([exe, str(n), str(iters), str(seed)], text=True, timeout=120)
    lines = text.strip().splitlines()
    assert len(lines) == iters + 1 and all(l.startswith("iter") for l in lines[:iters]), text
    printed = float(re.fullmatch(r"param_checksum (\S+)", lines[-1]).group(1))

    sim = lib.So100Sim(lib.ENV01, n, flags=lib.F_REFERENCE, seed=seed)
    od = sim.obs_dim
    layout, P = lib.learner_layout(od)
    host = np.zeros(P, np.float32)
    for t, name in enumerate(lib.POLICY_TENSORS):
        off, shape = layout[name]
        i = np.arange(int(np.prod(shape)), dtype=np.uint64)
        u = ((i * np.uint64(2654435761) + np.uint64(t * 40503)) % np.uint64(2001)).astype(np.float32) / np.float32(1000.0) - np.float32(1.0)
        host[off:off + i.size] = u * np.float32(TRAINER_SCALE[t])
    params = torch.from_numpy(host).to(DEV)
    sim.set_policy({name: params[off:off + int(np.prod(shape))].view(shape) for name, (off, shape) in layout.items()})
    rows = T * n; mb = min(rows // 4, 32768); per_epoch = -(-rows // mb)
    learner = lib.So100Learner(od, max_minibatch=mb)
    f = dict(dtype=torch.float32, device=DEV)
    buf = torch.zeros(T, n, od + 10, **f); tobs = torch.zeros(T, n, od, **f)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    adv, ret, adv_stats, out = torch.zeros(T, n, **f), torch.zeros(T, n, **f), torch.zeros(2, **f), torch.zeros(15, **f)
    perm = torch.zeros(rows, dtype=torch.int64, device=DEV)
    sim.reset()
    for it in range(iters):
        sim.rollout(buf, it * T, terminal_obs_chunk=tobs)
        learner.update(buf, sim.obs, params, m, v, adv, ret, adv_stats, perm, out, epochs=epochs, mb=mb, adam_step0=it * epochs * per_epoch,
                       shuffle_seed=seed, shuffle_epoch0=it * epochs, terminal_obs=tobs)
    want = params.double().sum().item()
    assert float(np.abs(params.cpu().numpy() - host).max()) > 1e-3               # the three updates moved the parameters
    assert abs(printed - want) <= 1e-6 * abs(want), (printed, want)
    m_out = re.search(r"value_loss (\S+)", lines[iters - 1])
    assert abs(float(m_out.group(1)) - out[1].item()) <= 1e-5 * max(abs(out[1].item()), 1.0)      # the last line shows that update's out_dev
    sim.close(); learner.close()


def test_cli_train_with_the_device_shuffle(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from so100_mujoco_rl_amd import main as drv
    monkeypatch.chdir(tmp_path)
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "-e", "Env01-v1", "--envs", "64", "--iters", "2", "--learner", "fused", "--shuffle", "device"],
                           catch_exceptions=False)
    assert r.exit_code == 0
    d = tmp_path / "models" / "Env01-v1_PPO"
    assert (d / "best_model.pt").is_file() and (d / "last_model.pt").is_file()
