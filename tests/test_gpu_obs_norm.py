"""Observation normalisation on the GPU (so100_learner_obs_norm_update / _fold, so100_learner_set_obs_norm, both Python learners,
`train --normalize-obs`), through the C ABI: the moment kernels and the fold kernel against the numpy reference of obs_norm_support.py, the
learner with a normaliser set on raw chunks against the same calls without one on chunks normalised beforehand (to the bit), the folded weights
in so100_policy_forward against an fp64 evaluation of the normalised network, FusedPPO against the fp64 reference learner of learn_support.py
fed the reference-normalised chunks, the argument errors and the command line.

Tolerances.  The kernels: obs_norm_support.py (1e-10 on the moments, 1 fp32 ulp on the fold; derived there).  The learner: PARAM_REF_TOL /
MOMENT_TOL of test_gpu_learner.py, the bounds the project holds for the same comparison without the normalisation (the reward normalisation's
test of the same construction uses them).  The fold's accuracy in the policy kernel: three times the measured error (FOLD_* below)."""
import ctypes as C
import functools
import logging
import math
import os

import numpy as np
import pytest
import torch

import learn_support as LS
import obs_norm_support as OS
import reward_norm_support as RS
import update_support as US
from learn_support import make_learner, state_dict
from test_gpu_learner import MOMENT_TOL, PARAM_REF_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def packed(obs, seed=0):
    """a [T, N, od+10] chunk on the device whose observation columns are the given ones; the other columns hold noise"""
    T, N, od = obs.shape
    buf = torch.randn(T, N, od + 10, generator=torch.Generator().manual_seed(60 + seed))
    buf[..., :od] = torch.from_numpy(np.array(obs))
    return buf.to(DEV)


def device_state(st):
    return torch.from_numpy(np.array(st, np.float64)).to(DEV)


def run_update(L, buf, state):
    T, N = buf.shape[0], buf.shape[1]
    ws = torch.full((L.obs_norm_workspace_bytes(T, N) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    L.obs_norm_update(buf, state, ws)


# ---- 1. the moment kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", OS.OBS_DIMS)
@pytest.mark.parametrize("T,N", OS.SHAPES)
def test_moment_kernels_match_the_reference(T, N, od):
    L = make_learner(od, 64)
    obs = OS.make_obs(T, N, od)
    buf = packed(obs); before = buf.clone()
    st = torch.full((2 * od + 1,), 5.0, dtype=torch.float64, device=DEV)
    L.obs_norm_init(st)
    assert st.tolist() == OS.fresh_state(od).tolist()
    run_update(L, buf, st)
    rel = OS.check_state(st.cpu().numpy(), OS.reference(T, N, od))
    print(f"[obsnorm] gpu ({T}, {N}) od {od}: mean {rel[0]:.2e} var {rel[1]:.2e}")
    assert same_bits(buf, before)                                              # the chunk is read only
    # the same call from the same state: the same bits
    st2 = device_state(OS.fresh_state(od))
    run_update(L, buf, st2)
    assert same_bits(st, st2)
    # a second chunk continues from the first's state and stays within the bound of one chunk of 2T
    other = OS.make_obs(T, N, od, seed=2)
    run_update(L, packed(other, seed=1), st)
    both = np.concatenate([obs, other])
    want = OS.ref_update(both, OS.fresh_state(od))
    OS.check_state(st.cpu().numpy(), want, exact_count=False)
    whole = device_state(OS.fresh_state(od))
    run_update(L, packed(both), whole)
    OS.check_state(whole.cpu().numpy(), want)


def test_moment_kernels_over_several_groups():
    """20 000 rows: 79 blocks, so two groups in the merge's second level, and a last block of 32 rows"""
    T, N, od = 50, 400, 8
    L = make_learner(od, 64)
    obs = OS.make_obs(T, N, od)
    st = device_state(OS.fresh_state(od))
    run_update(L, packed(obs), st)
    OS.check_state(st.cpu().numpy(), OS.ref_update(obs, OS.fresh_state(od)))
    OS.check_state(st.cpu().numpy(), OS.twin_update(obs, OS.fresh_state(od)))      # the twin runs the kernels' order (fused multiply-adds aside)


# ---- 2. the fold kernel ---------------------------------------------------------------------------------------------------------------------------
ENV_OF_OD = {15: "Env01-v1", 8: "Env05-v1"}
FN = 67


def fold_on_device(L, od, state, params):
    folded = torch.full_like(params, 7.0); norm = torch.full((2 * od,), 7.0, device=DEV)
    L.obs_norm_fold(device_state(state), params, folded, norm)
    return folded, norm


def views(flat, od):
    """{tensor name: view into the flat block}: what so100_policy_weights may point at"""
    lay, _ = OS.layout(od)
    return {k: flat[off:off + math.prod(shape)].view(shape) for k, (off, shape) in lay.items()}


def fp64_policy(od, sd, obs64, noise):
    """action sample, value and log-prob of the network on (already normalised) float64 observations, the noise given"""
    net = LS.RefNet(od, sd)
    with torch.no_grad():
        mean, value = net.mean_action(obs64), net.value(obs64)
        nz = noise.double().cpu()
        logp = (-0.5 * nz ** 2 - net.log_std - 0.5 * math.log(2 * math.pi)).sum(1)
        return mean + net.log_std.exp() * nz, value, logp


# Measured on an MI355X, max |kernel - fp64| over 67 envs (action sample, value, log-prob), observations at obs_norm_support.scales():
# FOLD_MEASURED the folded weights on raw observations, PLAIN_MEASURED the unfolded weights on observations normalised in fp32 beforehand.
# Each is bounded at three times its figure.  The log-prob is formed from the noise alone, so the fold does not reach it; at |mean|/std up
# to 5 the fold costs the action and the value no more than the fp32 normalisation itself does.
FOLD_MEASURED = {15: (5.815e-7, 6.833e-7, 1.374e-6), 8: (5.485e-7, 4.669e-7, 1.289e-6)}
PLAIN_MEASURED = {15: (4.340e-7, 7.118e-7, 1.374e-6), 8: (4.527e-7, 3.766e-7, 1.289e-6)}


@pytest.mark.parametrize("od", OS.OBS_DIMS)
def test_fold_kernel_matches_the_reference_and_feeds_the_policy_kernel(od):
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    L = make_learner(od, 64)
    tensors = OS.policy_tensors(od)
    state = OS.reference(64, 300, od)
    params = LS.flat_params(state_dict(od), od, DEV); keep = params.clone()
    folded, norm = fold_on_device(L, od, state, params)
    worst = OS.check_fold(OS.unflatten(folded.cpu().numpy(), od), norm.cpu().numpy(), tensors, state)
    assert same_bits(params, keep)
    print(f"[obsnorm] gpu fold od {od}: {worst} ulp")
    # so100_policy_forward with a so100_policy_weights pointing into the folded block, on raw observations, against fp64 on normalised ones
    env = So100VecEnv(ENV_OF_OD[od], FN, seed=3)
    sim = env.sim
    assert sim.obs_dim == od
    raw = torch.from_numpy(OS.make_obs(1, FN, od, seed=5)[0].copy()).to(DEV)
    noise = torch.randn(FN, 6, device=DEV, generator=torch.Generator(device=DEV).manual_seed(od))
    mean, inv_std = OS.ref_scale(state)
    want = fp64_policy(od, state_dict(od), (raw.double().cpu() - torch.from_numpy(mean)) * torch.from_numpy(inv_std), noise)

    def run(weights, obs):
        sim.set_policy(views(weights, od))
        ae, ar = torch.zeros(FN, 6, device=DEV), torch.zeros(FN, 6, device=DEV)
        v, lp = torch.zeros(FN, device=DEV), torch.zeros(FN, device=DEV)
        sim.policy_forward(obs.contiguous(), ae, 0, noise=noise, act_raw=ar, value=v, logp=lp)
        return tuple(float((g.double().cpu() - w).abs().max()) for g, w in zip((ar, v, lp), want))

    e_fold = run(folded, raw)
    e_plain = run(params, torch.from_numpy(OS.ref_normalize(raw.cpu().numpy(), state)).to(DEV))
    print(f"[obsnorm] policy_forward od {od}: folded on raw (action, value, logp) = {e_fold[0]:.3e} {e_fold[1]:.3e} {e_fold[2]:.3e}; "
          f"plain on normalised = {e_plain[0]:.3e} {e_plain[1]:.3e} {e_plain[2]:.3e}")
    for got, measured in zip(e_fold, FOLD_MEASURED[od]):
        assert got <= 3 * measured, (e_fold, FOLD_MEASURED[od])
    for got, measured in zip(e_plain, PLAIN_MEASURED[od]):                     # the comparison DESIGN quotes: held the same way
        assert got <= 3 * measured, (e_plain, PLAIN_MEASURED[od])
    # the unfolded weights on raw observations are another policy
    sim.set_policy(views(params, od))
    ar = torch.zeros(FN, 6, device=DEV)
    sim.policy_forward(raw.contiguous(), torch.zeros(FN, 6, device=DEV), 0, noise=noise, act_raw=ar)
    assert float((ar.double().cpu() - want[0]).abs().max()) > 1e-3


# ---- 3. the learner normalises on load and changes nothing else -----------------------------------------------------------------------------------
LT, LN, LMB = 5, 67, 100
ROWS = LT * LN


@functools.lru_cache(maxsize=None)
def raw_chunk(od, seed=3, T=LT, N=LN):
    """learn_support.make_chunk with every observation moved to obs_norm_support's scales, on the device"""
    buf, tobs, last_obs = LS.make_chunk(T, N, od, seed, state_dict(od))
    buf = buf.clone()
    buf[..., :od] = OS.scale_observations(buf[..., :od], od)
    tobs = torch.where(tobs > 1e29, tobs, OS.scale_observations(tobs, od))     # 1e30 stays where the code is not 2: the kernels must not read it
    assert (buf[..., od + 7] == 2).any()
    return buf.to(DEV), tobs.to(DEV), OS.scale_observations(last_obs, od).to(DEV)


def prenormalised(od, norm, chunk):
    """the chunk with every observation normalised on the device in fp32, one subtraction and one multiplication"""
    buf, tobs, last_obs = chunk
    m, s = norm[:od], norm[od:]
    nb = buf.clone()
    nb[..., :od] = (buf[..., :od] - m) * s
    return nb, torch.where(tobs > 1e29, tobs, (tobs - m) * s), (last_obs - m) * s


class Buffers:
    def __init__(self, L, od, extended):
        P = L.num_params
        self.params = LS.flat_params(state_dict(od), od, DEV); self.m = torch.zeros(P, device=DEV); self.v = torch.zeros(P, device=DEV)
        self.adv = torch.full((LT, LN), 3.0, device=DEV); self.ret = torch.full((LT, LN), 3.0, device=DEV); self.adv_stats = torch.full((2,), 3.0, device=DEV)
        self.perm = torch.full((ROWS,), -1, dtype=torch.int64, device=DEV)
        self.out = torch.full((15,), 7.0, device=DEV)
        self.stats = torch.full((4,), 7.0, device=DEV); self.diag = torch.full((8,), 7.0, device=DEV); self.grads = torch.full((P,), 7.0, device=DEV)
        self.state = torch.zeros(2, dtype=torch.int32, device=DEV) if extended else None
        self.rn_state = device_state(RS.fresh_state(LN))
        self.rewards = torch.full((LT, LN), 9.0, device=DEV)
        self.ws = torch.zeros(L.reward_norm_workspace_bytes(LT, LN) // 8, dtype=torch.float64, device=DEV)

    def everything(self):
        return [self.params, self.m, self.v, self.adv, self.ret, self.adv_stats, self.perm, self.out, self.stats, self.diag, self.grads, self.rn_state, self.rewards] + \
            ([self.state] if self.state is not None else [])


def run_entry_points(L, od, chunk):
    """every entry point that reads observations, on one chunk: so100_learner_advantages, an epoch of so100_learner_minibatch_step and of
    so100_learner_minibatch_step_ex with ALL_TERMS (the last minibatch holds the remainder 35), so100_learner_update_r with the reward
    normalisation and ALL_TERMS; returns every buffer they wrote"""
    buf, tobs, last_obs = chunk
    perm = torch.randperm(ROWS, generator=torch.Generator().manual_seed(11)).to(DEV)
    out = []
    A = Buffers(L, od, False)
    L.advantages(buf, last_obs, A.params, A.adv, A.ret, A.adv_stats, terminal_obs=tobs)
    for k, i in enumerate(range(0, ROWS, LMB)):
        L.minibatch_step(buf, perm[i:i + LMB], A.adv, A.ret, A.adv_stats, A.params, A.m, A.v, k + 1, A.stats, grads=A.grads)
    out += A.everything()
    B = Buffers(L, od, True)
    L.advantages(buf, last_obs, B.params, B.adv, B.ret, B.adv_stats, terminal_obs=tobs)
    for k, i in enumerate(range(0, ROWS, LMB)):
        L.minibatch_step_ex(buf, perm[i:i + LMB], B.adv, B.ret, B.adv_stats, B.params, B.m, B.v, k + 1, B.diag, update_state=B.state, grads=B.grads, **LS.ALL_TERMS)
    out += B.everything()
    U = Buffers(L, od, True)
    L.update(buf, last_obs, U.params, U.m, U.v, U.adv, U.ret, U.adv_stats, U.perm, U.out, epochs=2, mb=LMB, adam_step0=4, shuffle_seed=5, shuffle_epoch0=3,
             terminal_obs=tobs, terms=LS.ALL_TERMS, update_state=U.state, reward_norm=dict(state=U.rn_state, rewards=U.rewards, workspace=U.ws))
    out += U.everything()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("od", OS.OBS_DIMS)
def test_learner_normalises_on_load_and_changes_nothing_else(od):
    assert ROWS % LMB != 0
    chunk = raw_chunk(od)
    state = OS.reference(64, 300, od)
    on = make_learner(od, LMB)
    _, norm = fold_on_device(on, od, state, LS.flat_params(state_dict(od), od, DEV))
    assert OS.ulp_distance(norm.cpu().numpy(), OS.ref_fold(OS.policy_tensors(od), state)[1]) <= 1
    keep = [t.clone() for t in chunk]
    on.set_obs_norm(norm)
    got = run_entry_points(on, od, chunk)
    assert all(same_bits(a, b) for a, b in zip(chunk, keep))                   # the raw chunk is read only
    never = make_learner(od, LMB)
    want = run_entry_points(never, od, prenormalised(od, norm, chunk))
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), i
    assert all(torch.isfinite(g.double()).all() for g in got)
    # the normaliser is read when the kernels run: off again, the raw chunk gives what a handle that never had one gives
    plain = run_entry_points(never, od, chunk)
    assert not same_bits(plain[0], got[0]) and not same_bits(plain[3], got[3])   # (parameters and advantages: the option changed them)
    on.set_obs_norm(None)
    off = run_entry_points(on, od, chunk)
    for i, (g, w) in enumerate(zip(off, plain)):
        assert same_bits(g, w), i


# ---- 4. rejected calls ------------------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_enqueue_nothing():
    from so100_mujoco_rl_amd import lib
    od, T, N = 15, 4, 70
    learner = make_learner(od, 64)
    L, stream = learner.L, learner._stream()
    buf = packed(OS.make_obs(T, N, od))
    st = device_state(OS.fresh_state(od) + 0.25)
    need = learner.obs_norm_workspace_bytes(T, N)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    P = learner.num_params
    params = LS.flat_params(state_dict(od), od, DEV); folded = torch.full((P,), 7.0, device=DEV); norm = torch.full((2 * od,), 7.0, device=DEV)
    p = lambda t: t.data_ptr()

    def io(**over):
        kw = dict(rollout_dev=p(buf), state_dev=p(st), workspace_dev=p(ws), workspace_bytes=need)
        kw.update(over)
        return lib.ObsNormIO(**kw)

    fn = b"so100_learner_obs_norm_update: "
    upd = lambda T_=T, N_=N, **over: (lambda: L.so100_learner_obs_norm_update(learner.h, C.byref(io(**over)), T_, N_, stream))
    fold = lambda s=p(st), eps=1e-8, a=p(params), b=p(folded), c=p(norm): (lambda: L.so100_learner_obs_norm_fold(learner.h, s, eps, a, b, c, stream))
    calls = [(upd(T_=0), fn + b"T must be >= 1, got 0"),
             (upd(N_=-2), fn + b"N must be >= 1, got -2"),
             (upd(T_=4097, N_=4096), fn + b"T*N must be <= 16777216, got 16781312"),
             (upd(state_dev=None), fn + b"rollout/state/workspace pointers are required"),
             (upd(workspace_dev=None), fn + b"rollout/state/workspace pointers are required"),
             (upd(workspace_bytes=need - 8), fn + f"the workspace holds {need - 8} bytes, T = {T} and N = {N} need {need}".encode()),
             (upd(workspace_dev=p(ws) + 4), fn + b"the workspace must be 8-byte aligned"),
             (lambda: L.so100_learner_obs_norm_update(learner.h, None, T, N, stream), fn + b"null argument"),
             (lambda: L.so100_learner_obs_norm_init(learner.h, None, stream), b"so100_learner_obs_norm_init: the state pointer is required"),
             (fold(s=None), b"so100_learner_obs_norm_fold: state/params/folded_params/norm pointers are required"),
             (fold(c=None), b"so100_learner_obs_norm_fold: state/params/folded_params/norm pointers are required"),
             (fold(eps=-1.0), b"so100_learner_obs_norm_fold: epsilon must be >= 0"),
             (fold(eps=float("nan")), b"so100_learner_obs_norm_fold: epsilon must be >= 0"),
             (fold(b=p(params)), b"so100_learner_obs_norm_fold: the folded block must not be the plain block")]
    keep, keep_params = st.clone(), params.clone()
    for call, msg in calls:
        assert call() == -1, msg
        assert L.so100_last_error() == msg
        torch.cuda.synchronize()
        assert same_bits(st, keep) and same_bits(params, keep_params) and folded.unique().tolist() == [7.0] and norm.unique().tolist() == [7.0], msg
    assert upd()() == 0 and fold()() == 0                                      # the handle still works
    torch.cuda.synchronize()
    assert not same_bits(st, keep) and torch.isfinite(folded).all() and torch.isfinite(norm).all()
    learner.close()


# ---- 5. the Python learners, end to end -------------------------------------------------------------------------------------------------------------
ET, EN, EMB, EEPOCHS, EOD = 8, 67, 100, 2, 15


def end_to_end_chunks():
    return [raw_chunk(EOD, seed=s, T=ET, N=EN) for s in (1, 2)]


def as_batch(chunk):
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    buf, tobs, last_obs = chunk
    c = RolloutChunk(ET, EN, EOD, DEV); c.buf.copy_(buf)
    b = c.unpack(); b["last_obs"] = last_obs.clone(); b["terminal_obs"] = torch.where(tobs > 1e29, torch.zeros_like(tobs), tobs); b["packed"] = c.buf
    return b


# The parameters do not fit under PARAM_REF_TOL (5.07e-7), so the bound is three times the measured maximum.  The first update runs under the
# fresh statistics, whose (float) inv_std is exactly 1 and whose mean is 0: the towers see the RAW observations, with offsets up to 30 and
# spreads up to 6, and the fp32 first layer carries their magnitude into its rounding error; the second update starts from those parameters.
# Measured on an MI355X, largest per-tensor relative error after update 1 / 2: shuffle torch 9.026e-7 / 9.832e-7, device 7.160e-7 / 6.712e-7.
# The same learner with the option off at this shape: 2.119e-7 / 3.224e-7 on N(0, 1) observations (under PARAM_REF_TOL), 9.026e-7 / 1.023e-6
# on these scaled ones -- the excess is the input scale's, not the normalisation's.
E2E_PARAM_MEASURED = 9.832e-7
E2E_PARAM_TOL = 3 * E2E_PARAM_MEASURED
assert E2E_PARAM_TOL > PARAM_REF_TOL
@pytest.mark.parametrize("shuffle", ["torch", "device"])
def test_fused_ppo_matches_the_fp64_reference_on_the_normalised_observations(shuffle):
    from so100_mujoco_rl_amd.ppo import FusedPPO
    seed, n = 21, ET * EN
    f = FusedPPO(EOD, DEV, epochs=EEPOCHS, minibatch=EMB, seed=seed, shuffle=shuffle, normalize_obs=True)
    f.net.load_state_dict({k: v.to(DEV) for k, v in state_dict(EOD).items()})
    ref = LS.RefLearner(EOD, state_dict(EOD))
    state = OS.fresh_state(EOD)
    figures = []
    g = torch.Generator().manual_seed(77)
    for k, chunk in enumerate(end_to_end_chunks()):
        if shuffle == "torch":
            perms = [torch.randperm(n, generator=g) for _ in range(EEPOCHS)]
            stats = f.update(as_batch(chunk), perms=[p.to(DEV) for p in perms])
        else:
            perms = [torch.from_numpy(US.ref_perm_cached(seed, k * EEPOCHS + e, n).copy()) for e in range(EEPOCHS)]
            stats = f.update(as_batch(chunk))
        # the reference learner on the chunk normalised under the statistics of the chunks before
        buf, tobs, last_obs = (t.cpu() for t in chunk)
        nb = buf.clone(); nb[..., :EOD] = torch.from_numpy(OS.ref_normalize(buf[..., :EOD].numpy(), state))
        ntobs = torch.from_numpy(OS.ref_normalize(torch.where(tobs > 1e29, torch.zeros_like(tobs), tobs).numpy(), state))
        nlast = torch.from_numpy(OS.ref_normalize(last_obs.numpy(), state))
        adv, ret, mean, std = LS.ref_advantages(nb, nlast, ref.net, terminal_obs=ntobs)
        for perm in perms:
            for i in range(0, n, EMB):
                ref.step(nb, perm[i:i + EMB], adv, ret, mean, std)
        state = OS.ref_update(buf[..., :EOD].numpy(), state)
        want = ref.net.state_dict(); mom = ref.moments()
        got_p, got_m, got_v = LS.split_flat(f.params, EOD), LS.split_flat(f.adam_m, EOD), LS.split_flat(f.adam_v, EOD)
        ep = max(LS.rel_err(got_p[key], want[key]) for key in want)
        em = max(LS.rel_err(got_m[key], mom[key][0]) for key in want)
        ev = max(LS.rel_err(got_v[key], mom[key][1]) for key in want)
        print(f"[obsnorm] fused {shuffle} update {k + 1}: params {ep:.3e} exp_avg {em:.3e} exp_avg_sq {ev:.3e}")
        figures.append((ep, em, ev))
        sd = f.obs_norm_state()
        OS.check_state(np.concatenate([sd["mean"].numpy(), sd["var"].numpy(), [sd["count"].item()]]), state)
        assert math.isfinite(stats["value_loss"]) and stats["n_updates"] == EEPOCHS * math.ceil(n / EMB)
    for ep, em, ev in figures:
        assert ep <= E2E_PARAM_TOL and em <= MOMENT_TOL and ev <= MOMENT_TOL, figures
    assert max(float((got_p[key] - state_dict(EOD)[key].double()).abs().max()) for key in want) > 1e-3
    # the folded policy: the header's fold of the current parameters over the current statistics, and a restored learner continues identically
    psd = f.policy_state_dict()
    from so100_mujoco_rl_amd import lib
    got = {name: psd[key].cpu().numpy() for name, key in lib.SB3_STATE_DICT_KEYS.items()}
    tensors = {name: f.net.state_dict()[key].cpu().numpy() for name, key in lib.SB3_STATE_DICT_KEYS.items()}
    OS.check_fold(got, f._norm.cpu().numpy(), tensors, state)
    f2 = FusedPPO(EOD, DEV, epochs=EEPOCHS, minibatch=EMB, seed=seed, shuffle=shuffle, normalize_obs=True)
    f2.net.load_state_dict(f.net.state_dict()); f2.adam_m.copy_(f.adam_m); f2.adam_v.copy_(f.adam_v); f2.adam_step = f.adam_step; f2.shuffle_epoch = f.shuffle_epoch
    f2.load_obs_norm_state(f.obs_norm_state())
    extra = raw_chunk(EOD, seed=4, T=ET, N=EN)
    kw = {"perms": [torch.randperm(n, generator=g).to(DEV) for _ in range(EEPOCHS)]} if shuffle == "torch" else {}
    f.update(as_batch(extra), **kw); f2.update(as_batch(extra), **kw)
    assert same_bits(f.params, f2.params) and all(torch.equal(f.obs_norm_state()[key], f2.obs_norm_state()[key]) for key in sd)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_reward", [False, True], ids=["obs", "obs+reward"])
def test_cli_train_saves_reloads_and_runs_without_the_side_file(tmp_path, monkeypatch, caplog, with_reward):
    monkeypatch.chdir(tmp_path)
    d = tmp_path / "models" / "Env01-v1_PPO"
    from so100_mujoco_rl_amd import main as drv
    from so100_mujoco_rl_amd.ppo import ActorCritic
    from click.testing import CliRunner
    caplog.set_level(logging.INFO, logger=drv.logger.name)
    args = ["train", "-e", "Env01-v1", "--envs", "64", "--iters", "2", "--learner", "fused", "--normalize-obs"] + (["--normalize-reward"] if with_reward else [])
    r = CliRunner().invoke(drv.cli, ["-a", "PPO"] + args, catch_exceptions=False)
    assert r.exit_code == 0
    assert any("Observation normalisation: on" in l for l in caplog.messages), caplog.messages
    assert (d / "best_model.pt").is_file() and (d / "best_model.obs_norm.pt").is_file() and (d / "last_model.obs_norm.pt").is_file()
    assert (d / "last_model.reward_norm.pt").is_file() == with_reward
    sd = torch.load(d / "last_model.obs_norm.pt", weights_only=True)
    assert sd["mean"].shape == (15,) and sd["var"].shape == (15,) and sd["count"].item() == pytest.approx(1e-4 + 64 * 64 * 2, rel=1e-12)
    assert (sd["var"] > 0).all() and sd["mean"].abs().max() > 0
    model = torch.load(d / "last_model.pt", weights_only=True)
    assert list(model) == list(ActorCritic(15).state_dict())                   # the model file stays a plain, unfolded state_dict
    caplog.clear()
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "-m", str(d / "best_model.pt"), "test", "-e", "Env01-v1", "--envs", "8", "--steps", "10"], catch_exceptions=False)
    assert r.exit_code == 0 and any("folded the statistics" in l for l in caplog.messages), caplog.messages
    caplog.clear()
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "-m", str(d / "last_model.pt")] + args, catch_exceptions=False)
    assert r.exit_code == 0
    assert any("reloaded the running statistics" in l for l in caplog.messages), caplog.messages
    sd2 = torch.load(d / "last_model.obs_norm.pt", weights_only=True)
    assert sd2["count"].item() == pytest.approx(1e-4 + 64 * 64 * 4, rel=1e-12)                           # the second run continued the first's count
    os.remove(d / "best_model.obs_norm.pt")
    caplog.clear()
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "-m", str(d / "best_model.pt"), "test", "-e", "Env01-v1", "--envs", "8", "--steps", "10"], catch_exceptions=False)
    assert r.exit_code == 0 and not any("folded the statistics" in l for l in caplog.messages)          # the raw policy runs, without error
    if with_reward:
        return
    # a run WITHOUT the option from that model and into the same directory: it says what it is doing, and it leaves no statistics of the
    # earlier run beside the raw models it saves
    caplog.clear()
    off = [a for a in args if a != "--normalize-obs"]
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "-m", str(d / "last_model.pt")] + off, catch_exceptions=False)
    assert r.exit_code == 0
    assert any("without --normalize-obs training continues on raw ones" in rec.getMessage() and rec.levelno == logging.WARNING for rec in caplog.records)
    assert not (d / "last_model.obs_norm.pt").exists() and not (d / "best_model.obs_norm.pt").exists()
