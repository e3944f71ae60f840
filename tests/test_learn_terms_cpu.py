"""SB3's remaining PPO terms without a device: the extended loss-head templates of csrc/so100_learn.hpp (instantiated on the host by
tests/_learncheck) and ppo.PPO with each new option against the fp64 autograd reference of learn_support.py; the new struct and the two
new calls of include/so100_learn.h are bound, check their arguments and have no CPU fallback.  CPU only.

Bounds.  Twin in double: 1e-12, the existing twin's bound for the same kind of arithmetic; float twin against the double one: 2e-5 (likewise).
ppo.PPO is fp32 PyTorch, the reference fp64: a clipped gradient tensor agrees within GRAD_TOL = 2e-5 of its largest entry (fp32's 6e-8 times the
~100 rounded operations on the longest path through two tanh layers and a sum over <= 780 samples, times 3), a parameter tensor within
PARAM_TOL = 2e-6 of its largest entry (<= 9 Adam steps, each rounding the parameter once, <= 3e-8 of the largest entry, plus lr 3e-3 times the
gradient's relative error), a scalar diagnostic within STAT_TOL = 2e-5 of max(|reference|, 0.01).  A wrong or missing term costs a percent or more."""
import copy
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import hostlibs
import learn_support as LS
from learn_support import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12
GRAD_TOL, PARAM_TOL, STAT_TOL = 2e-5, 2e-6, 2e-5


def _close(got, want, what, rel=REL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= rel * scale, (what, np.abs(got - want).max())


# ---- 1. the host twin -------------------------------------------------------------------------------------------------------------------------
def _sample(rs, case):
    mu, ls, a = rs.randn(6) * 0.5, rs.randn(6) * 0.3, rs.randn(6)
    adv_n, V, ret = rs.randn(), rs.randn(), rs.randn()
    old_V = V + (0.0 if case % 7 == 0 else 0.4 * rs.randn())
    return mu, ls, a, adv_n, V, old_V, ret


@pytest.mark.parametrize("clip_vf,ent_coef", [(0.0, 0.0), (0.3, 0.0), (0.0, 0.01), (0.3, 0.01), (0.25, 0.01)])
def test_extended_head_in_double_matches_autograd(clip_vf, ent_coef):
    """per sample: every output derivative, approx_kl, the entropy and the value-clipped flag against autograd on the formulas of SB3's
    PPO.train; samples inside and outside either clip range, with V == old_V (case % 7 == 0) and, at clip_vf 0.25, exactly on the value
    clip's closed boundary, V - old_V == +-0.25 in binary (case % 9 == 1, 2): there the gradient passes and the sample does not count as clipped"""
    tw = hostlibs.learncheck()
    rs = np.random.RandomState(11)
    clip, vf, inv_mb = 0.2, 0.5, 1.0 / 37
    seen = set(); seen_boundary = False
    for case in range(200):
        mu, ls, a, adv_n, V, old_V, ret = _sample(rs, case)
        on_boundary = clip_vf == 0.25 and case % 9 in (1, 2)
        if on_boundary:
            V, old_V = 0.5, (0.25 if case % 9 == 1 else 0.75)
            assert abs(V - old_V) == clip_vf
        tmu, tls, tV = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (mu, ls, V))
        z = (torch.tensor(a) - tmu) / tls.exp()
        logp = (-0.5 * z * z - tls - 0.5 * math.log(2 * math.pi)).sum()
        logp_old = logp.item() + (0.0 if case % 10 == 0 else 0.3 * rs.randn())
        ratio = (logp - logp_old).exp()
        policy = -torch.minimum(ratio * adv_n, ratio.clamp(1 - clip, 1 + clip) * adv_n)
        v_pred = old_V + (tV - old_V).clamp(-clip_vf, clip_vf) if clip_vf > 0 else tV
        value = (ret - v_pred) ** 2
        entropy = tls.sum() + 6 * LS.GAUSS_ENTROPY
        ((policy - ent_coef * entropy + vf * value) * inv_mb).backward()
        inp = np.concatenate([mu, ls, a, [logp_old, adv_n, V, old_V, ret, clip, clip_vf, ent_coef, vf, inv_mb]]); out = np.zeros(19)
        tw.lc_head_ex_d(ptr(inp), ptr(out))
        _close(out[0], policy.item(), "policy loss"); _close(out[1], value.item(), "value loss")
        assert out[2] == float(abs(ratio.item() - 1) > clip)
        _close(out[3:9], tmu.grad.numpy(), "dmu"); _close(out[9:15], tls.grad.numpy(), "dlog_std")
        _close(out[15], 0.0 if tV.grad is None else tV.grad.item(), "dV")
        _close(out[16], (ratio.item() - 1) - (logp.item() - logp_old), "approx_kl"); _close(out[17], entropy.item(), "entropy")
        outside = clip_vf > 0 and abs(V - old_V) > clip_vf
        assert out[18] == float(outside) and (not outside or out[15] == 0.0)
        if on_boundary:
            assert not outside and out[15] != 0.0
        seen.add(outside); seen_boundary = seen_boundary or on_boundary
    assert seen == ({False, True} if clip_vf > 0 else {False}) and seen_boundary == (clip_vf == 0.25)


def test_extended_head_with_every_term_off_is_the_old_head():
    """clip_vf 0 and ent_coef 0: the same loss terms and derivatives as ppo_loss_head's formulas give, whatever old_V is"""
    tw = hostlibs.learncheck()
    rs = np.random.RandomState(12)
    base = np.concatenate([rs.randn(6) * 0.5, rs.randn(6) * 0.3, rs.randn(6), [-8.0, 0.7, 0.2, 0.0, -0.4, 0.2, 0.0, 0.0, 0.5, 1.0 / 64]])
    outs = []
    for old_V in (0.2, 5.0, -3.0):
        inp = base.copy(); inp[21] = old_V; out = np.zeros(19)
        tw.lc_head_ex_d(ptr(inp), ptr(out)); outs.append(out)
    assert all(np.array_equal(o, outs[0]) for o in outs) and outs[0][18] == 0.0
    assert outs[0][15] == 2 * 0.5 * (0.2 - -0.4) / 64


def test_float_instantiation_of_the_extended_head_is_the_double_one_rounded():
    tw = hostlibs.learncheck()
    rs = np.random.RandomState(13)
    for old_V in (0.1, 0.9):                                     # inside / outside the value clip
        inp = np.concatenate([rs.randn(6) * 0.5, rs.randn(6) * 0.3, rs.randn(6), [-8.0, 0.7, 0.2, old_V, -0.4, 0.2, 0.3, 0.01, 0.5, 1.0 / 64]])
        out_d = np.zeros(19); out_f = np.zeros(19, np.float32)
        inp_f = inp.astype(np.float32)
        tw.lc_head_ex_d(ptr(inp_f.astype(np.float64)), ptr(out_d)); tw.lc_head_ex_f(ptr(inp_f), ptr(out_f))
        assert out_d[18] == out_f[18] == float(old_V == 0.9)
        assert np.abs(out_f - out_d).max() <= 2e-5 * max(1.0, np.abs(out_d).max())


# ---- 2. ppo.PPO with each option --------------------------------------------------------------------------------------------------------------
OD, T, N = 15, 6, 130


def _inputs(od=OD, t=T, n=N):
    sd = LS.make_state_dict(od, seed=od)
    buf, _, last_obs = LS.make_chunk(t, n, od, seed=3, state_dict=sd)
    b = {"obs": buf[..., :od], "actions": buf[..., od:od + 6], "rewards": buf[..., od + 6], "dones": (buf[..., od + 7] != 0).float(),
         "values": buf[..., od + 8], "log_probs": buf[..., od + 9], "last_obs": last_obs}
    # PPO's GAE ends an episode on every done and adds no bootstrap: the reference's code-1 behaviour on every episode end
    rbuf = buf.clone(); rbuf[..., od + 7] = b["dones"]
    return sd, rbuf, b


def _run_both(terms, epochs, mb, lr=3e-4, target_kl=None, od=OD, t=T, n=N, lr_schedule=None, progress=1.0):
    """PPO.update and the reference on the same permutations; returns (ppo, its stats, reference learner, its per-step diagnostics, last gradients)"""
    from so100_mujoco_rl_amd.ppo import PPO
    sd, rbuf, b = _inputs(od, t, n)
    ppo = PPO(od, "cpu", lr=lr, epochs=epochs, minibatch=mb, seed=1, target_kl=target_kl, lr_schedule=lr_schedule, **terms)
    ppo.net.load_state_dict(sd)
    torch.manual_seed(5)
    stats = ppo.update(b, progress) if lr_schedule is not None else ppo.update(b)
    ref = LS.RefLearner(od, sd, lr=lr if lr_schedule is None else lr_schedule(progress), target_kl=target_kl, **terms)
    adv, ret, mean, std = LS.ref_advantages(rbuf, b["last_obs"], ref.net)
    torch.manual_seed(5)
    steps, grads = [], None
    for _ in range(epochs):
        perm = torch.randperm(t * n)
        for i in range(0, t * n, mb):
            st, g = ref.step(rbuf, perm[i:i + mb], adv, ret, mean, std)
            if st is not None:
                steps.append(st)
            if g is not None:
                grads = g
    return ppo, stats, ref, steps, grads, (rbuf, ret)


def _compare(ppo, stats, ref, steps, grads, chunk, stopped=False):
    want = ref.net.state_dict()
    for k, p in ppo.net.named_parameters():
        assert LS.rel_err(p.data, want[k]) <= PARAM_TOL, k
        if not stopped:                                          # the module keeps the last applied step's clipped gradient
            assert LS.rel_err(p.grad, grads[k]) <= GRAD_TOL, k
    last = steps[-1]
    for k in ("value_loss", "approx_kl", "entropy_loss", "loss"):
        assert abs(stats[k] - last[k]) <= STAT_TOL * max(abs(last[k]), 1e-2), (k, stats[k], last[k])
    rbuf, ret = chunk
    ev = LS.ref_explained_variance(ret.numpy(), rbuf[..., OD + 8].double().numpy())
    assert abs(stats["explained_variance"] - ev) <= STAT_TOL * max(abs(ev), 1e-2)
    assert abs(stats["std"] - want["log_std"].exp().mean().item()) <= STAT_TOL
    assert stats["n_updates"] == ref.applied and stats["early_stop"] == ref.stopped


TERM_CASES = {"ent_coef": dict(ent_coef=0.01), "clip_range_vf": dict(clip_range_vf=0.3), "minibatch": dict(normalize_advantage="minibatch"),
              "all": LS.ALL_TERMS, "none": {}}


@pytest.mark.parametrize("case", list(TERM_CASES))
def test_ppo_with_each_option_matches_the_reference(case):
    out = _run_both(TERM_CASES[case], epochs=1, mb=260)
    _compare(*out)
    ppo, stats, ref, steps, grads, _ = out
    assert len(steps) == 3 and stats["n_updates"] == 3 and not stats["early_stop"]
    if "clip_range_vf" in TERM_CASES[case]:                       # the value clip is really engaged, and not everywhere
        assert 0.2 * 260 <= steps[-1]["v_clipped_count"] <= 0.8 * 260 and steps[-1]["v_borderline"] == 0
    # the option changes the step: against the plain loss the last gradient differs by far more than the tolerance
    if case != "none":
        plain = _run_both({}, epochs=1, mb=260)[4]
        assert max(LS.rel_err(grads[k], plain[k]) for k in grads) > 100 * GRAD_TOL


@pytest.mark.parametrize("mb", [1, 2])
def test_minibatch_normalisation_with_one_and_two_samples(mb):
    """SB3 normalises only when the minibatch has more than one sample; with two the normalised advantages are +-1/sqrt(2)"""
    out = _run_both(dict(normalize_advantage="minibatch"), epochs=1, mb=mb, t=2, n=3)
    ppo, stats, ref, steps, grads, _ = out
    assert len(steps) == 6 // mb
    want = ref.net.state_dict()
    for k, p in ppo.net.named_parameters():
        assert LS.rel_err(p.data, want[k]) <= PARAM_TOL and LS.rel_err(p.grad, grads[k]) <= GRAD_TOL, k
    assert all(torch.isfinite(p).all() for p in ppo.net.parameters())


def test_learning_rate_schedule_is_evaluated_once_per_update():
    sched = lambda progress: 3e-3 * progress
    out = _run_both({}, epochs=1, mb=260, lr_schedule=sched, progress=0.25)
    _compare(*out)
    assert all(g["lr"] == 3e-3 * 0.25 for g in out[0].opt.param_groups)


def test_target_kl_stops_the_update():
    """3 epochs x 3 minibatches at lr 3e-3.  The reference, run without a stop, yields approx_kl k_1..k_9; s is the first step (2 <= s <= 8)
    whose k_s is at least 1.2 x every earlier one, and 1.5 target_kl is put at the geometric mean of k_s and that maximum: the steps
    before s are applied, step s and every later one are not."""
    _, _, _, free, _, _ = _run_both(LS.ALL_TERMS, epochs=3, mb=260, lr=3e-3)
    k = [st["approx_kl"] for st in free]
    assert len(k) == 9
    picks = [s for s in range(2, 9) if k[s - 1] >= 1.2 * max(k[:s - 1])]
    assert picks, k
    s = picks[0]
    target = math.sqrt(k[s - 1] * max(k[:s - 1])) / 1.5
    out = _run_both(LS.ALL_TERMS, epochs=3, mb=260, lr=3e-3, target_kl=target)
    ppo, stats, ref, steps, grads, _ = out
    assert ref.stopped and ref.applied == s - 1 and len(steps) == s
    assert stats["n_updates"] == s - 1 and stats["early_stop"] is True
    assert abs(stats["approx_kl"] - k[s - 1]) <= STAT_TOL * max(k[s - 1], 1e-2)
    _compare(*out, stopped=True)
    # and the s - 1 applied steps really moved the parameters
    assert max(float((p.data.double() - LS.make_state_dict(OD, OD)[n_].double()).abs().max()) for n_, p in ppo.net.named_parameters()) > 1e-3


def test_defaults_give_the_bits_of_the_loss_as_it_was():
    """With no new option PPO.update computes what it always did: a copy of that loss, written here, gives the same parameters bit for bit"""
    from so100_mujoco_rl_amd.ppo import PPO
    sd, _, b = _inputs()
    ppo = PPO(OD, "cpu", epochs=2, minibatch=260, seed=1)
    ppo.net.load_state_dict(sd)
    net = copy.deepcopy(ppo.net)
    opt = torch.optim.Adam(net.parameters(), lr=3e-4, eps=1e-5)
    torch.manual_seed(5)
    stats = ppo.update(b)
    assert stats["n_updates"] == 6 and not stats["early_stop"]
    torch.manual_seed(5)
    with torch.no_grad():
        last_v = net.value(b["last_obs"]); g = torch.zeros_like(last_v); adv = torch.zeros(T, N)
        for t in reversed(range(T)):
            nv = last_v if t == T - 1 else b["values"][t + 1]
            nonterm = 1.0 - b["dones"][t]
            delta = b["rewards"][t] + 0.99 * nv * nonterm - b["values"][t]
            g = delta + 0.99 * 0.95 * nonterm * g
            adv[t] = g
        ret = (adv + b["values"]).reshape(-1)
        a = adv.reshape(-1)
        adv_n = (a - a.mean()) / (a.std() + 1e-8)
    obs, act, old_lp = b["obs"].reshape(-1, OD), b["actions"].reshape(-1, 6), b["log_probs"].reshape(-1)
    for _ in range(2):
        perm = torch.randperm(T * N)
        for i in range(0, T * N, 260):
            idx = perm[i:i + 260]
            opt.zero_grad(set_to_none=True)
            v, lp = net.evaluate(obs.index_select(0, idx), act.index_select(0, idx))
            an = adv_n.index_select(0, idx)
            ratio = (lp - old_lp.index_select(0, idx)).exp()
            pg = -torch.min(ratio * an, ratio.clamp(1 - 0.2, 1 + 0.2) * an).mean()
            vl = (ret.index_select(0, idx) - v).pow(2).mean()
            (pg + 0.5 * vl).backward()
            nn.utils.clip_grad_norm_(net.parameters(), 0.5); opt.step()
    for (k, p), q in zip(ppo.net.named_parameters(), net.parameters()):
        assert torch.equal(p.data, q.data), k
    assert stats["value_loss"] == vl.item()


def test_options_are_validated():
    from so100_mujoco_rl_amd.ppo import PPO, FusedPPO
    for cls in (PPO, FusedPPO):
        for bad in (dict(ent_coef=-0.1), dict(clip_range_vf=0.0), dict(normalize_advantage="chunk"), dict(target_kl=-1.0)):
            with pytest.raises(ValueError):
                cls(15, "cpu", **bad)


# ---- 3. header, ctypes, argument errors, no CPU fallback ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib.load()


def test_ppo_terms_struct_matches_the_header():
    from so100_mujoco_rl_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "so100_learn.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} so100_ppo_terms;", src).group(1)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert [d[-1] for d in decls] == [f[0] for f in lib.PpoTerms._fields_] == ["ent_coef", "clip_range_vf", "normalize_advantage", "target_kl", "lr"]
    ctype = {"float": C.c_float, "int32_t": C.c_int32, "double": C.c_double}
    assert [ctype[d[0]] for d in decls] == [f[1] for f in lib.PpoTerms._fields_]
    assert C.sizeof(lib.PpoTerms) == 24 and lib.PpoTerms.lr.offset == 16
    assert {"so100_learner_minibatch_step_ex", "so100_learner_explained_variance"} <= set(lib.LEARN_EXPORTS)
    assert lib.LEARNER_DIAG[:4] == lib.LEARNER_STATS and len(lib.LEARNER_DIAG) == 8
    for s in ("so100_learner_minibatch_step_ex", "so100_learner_explained_variance"):
        assert re.search(r"\b" + s + r"\s*\(", src)


def test_new_calls_reject_null_arguments_and_have_no_cpu_fallback(L):
    from so100_mujoco_rl_amd import lib
    io, terms = lib.MinibatchIO(), lib.PpoTerms(0.0, 0.0, 0, 0.0, -1.0)
    assert L.so100_learner_minibatch_step_ex(None, C.byref(io), C.byref(terms), None, None, None) == -1
    assert b"so100_learner_minibatch_step_ex" in L.so100_last_error() and b"null" in L.so100_last_error()
    assert L.so100_learner_explained_variance(None, None, None, 1, None, None) == -1
    assert b"so100_learner_explained_variance" in L.so100_last_error()
    assert L.so100_abi_version() == 3
    if not torch.cuda.is_available():
        from so100_mujoco_rl_amd.ppo import FusedPPO
        f = FusedPPO(15, "cpu", ent_coef=0.01, target_kl=0.05)
        assert f._extended
        _, _, b = _inputs()
        with pytest.raises(lib.So100Error, match="no CPU fallback"):
            f.update(b)
        assert not FusedPPO(15, "cpu")._extended                # the defaults keep the old entry point
