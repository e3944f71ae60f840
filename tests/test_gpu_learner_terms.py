"""The learner's extended step on the GPU (so100_learner_minibatch_step_ex, so100_learner_explained_variance, ppo.FusedPPO with SB3's
remaining options) against the fp64 autograd reference of learn_support.py: gradients and diagnostics per option, bitwise identity
with the old step when every term is off, whole updates with the target_kl stop, explained variance, one training iteration against the
PyTorch learner and the command line.

Tolerances.  Every bound is 3 x the largest error measured on an MI355X over the cases of its test, rounded down to three
digits; each test prints its figures as `[terms-tol] name value` before it asserts.  Errors are relative to the largest magnitude of the
reference tensor they belong to; scalar diagnostics relative to max(|reference|, 0.01).  A bound that has not been measured yet is the
ceiling of 1e-3, above which an error is a wrong term whatever was measured.  The reference is the fp64 one, never ppo.py or the kernels."""
import functools
import math

import pytest
import torch

import learn_support as LS
from learn_support import make_learner, minibatch_indices, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"

CEILING = 1e-3
#                           bound = 3 x measured maximum on an MI355X, rounded DOWN to three digits
GRAD_TOL = 9.22e-6        # each gradient tensor of the extended step                                      measured 3.074e-6 (od 8, mb 2, all terms)
STAT_TOL = 1.49e-5        # policy/value/entropy/total loss, approx_kl, gradient norm                      measured 4.982e-6 (approx_kl, od 8, mb 1)
#                           (the default-path diagnostics of FusedPPO are held to it too: their largest error is 1.713e-6, policy loss, od 8)
PARAM_TOL = 6.04e-6       # parameters after an update with a stop (lr 3e-3), against the fp64 reference   measured 2.016e-6 (od 15, stop at 6)
MOMENT_TOL = 3.77e-6      # Adam's moments after that update                                               measured 1.257e-6 (exp_avg, od 15, stop at 6)
EV_TOL = 1.04e-7          # explained variance, absolute (it is a ratio of order 1)                        measured 3.49e-8 (9 x 1031)
E2E_PARAM_TOL = 5.91e-6   # FusedPPO against the fp32 PyTorch learner, parameters after one update         measured 1.970e-6
E2E_STAT_TOL = 6.50e-6    # ... and each returned diagnostic                                               measured 2.168e-6 (explained_variance)
assert max(GRAD_TOL, STAT_TOL, PARAM_TOL, MOMENT_TOL, EV_TOL, E2E_PARAM_TOL, E2E_STAT_TOL) <= CEILING

CT, CN = 6, 130                                   # the chunk: 780 rows
TERM_CASES = {"ent_coef": dict(ent_coef=0.01), "clip_range_vf": dict(clip_range_vf=0.3), "minibatch": dict(normalize_advantage="minibatch"),
              "all": LS.ALL_TERMS}


def report(name, value):
    print(f"[terms-tol] {name} {value:.3e}")
    return value


@functools.lru_cache(maxsize=None)
def chunk(od, T=CT, N=CN):
    """(packed chunk, terminal obs, last obs) float32 on the CPU; shared, never modified"""
    return LS.make_chunk(T, N, od, seed=3, state_dict=state_dict(od))


@functools.lru_cache(maxsize=None)
def reference_advantages(od):
    buf, tobs, last_obs = chunk(od)
    return LS.ref_advantages(buf, last_obs, LS.RefNet(od, state_dict(od)), terminal_obs=tobs)


def step_inputs(od):
    """the chunk with the reference's advantages rounded to float32: what both sides are fed"""
    adv, ret, mean, std = reference_advantages(od)
    return chunk(od)[0], adv.float(), ret.float(), torch.stack([mean, std]).float()


def gpu_step(L, od, idx, terms, target_kl=None, use_state=True, start=None):
    """one extended step from the shared initial weights (or from `start` = (params, m, v, adam_step)); returns params, m, v, diag, grads, state"""
    buf, adv, ret, adv_stats = (t.to(DEV) for t in step_inputs(od))
    P = L.num_params
    if start is None:
        params = LS.flat_params(state_dict(od), od, DEV); m = torch.zeros(P, device=DEV); v = torch.zeros(P, device=DEV); step = 1
    else:
        params, m, v, step = start
    diag = torch.full((8,), float("nan"), device=DEV); grads = torch.full((P,), float("nan"), device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV) if use_state else None
    L.minibatch_step_ex(buf, idx.to(DEV), adv, ret, adv_stats, params, m, v, step, diag, target_kl=target_kl, update_state=state, grads=grads, **terms)
    return params, m, v, diag, grads, state


def check_step(od, mb, idx, terms, name):
    from so100_mujoco_rl_amd import lib
    buf, adv, ret, adv_stats = step_inputs(od)
    ref = LS.RefLearner(od, state_dict(od), **terms)
    st_r, grads_r = ref.step(buf, idx, adv.double(), ret.double(), adv_stats[0].double(), adv_stats[1].double())
    L = make_learner(od)
    _, _, _, diag, grads, state = gpu_step(L, od, idx, terms)
    assert state.tolist() == [0, 1]
    got = LS.split_flat(grads, od)
    errs = {k: LS.rel_err(got[k], g_r) for k, g_r in grads_r.items()}
    worst = max(errs, key=errs.get)
    report(f"grad od{od} mb{mb} {name} ({worst})", errs[worst])
    d = dict(zip(lib.LEARNER_DIAG, diag.tolist()))
    e_stat = {k: report(f"stat-{k} od{od} mb{mb} {name}", abs(d[k] - st_r[k]) / max(abs(st_r[k]), 1e-2))
              for k in ("policy_loss", "value_loss", "grad_norm", "approx_kl", "entropy_loss", "loss")}
    assert errs[worst] <= GRAD_TOL, errs
    assert all(e <= STAT_TOL for e in e_stat.values()), (e_stat, d, st_r)
    # the two clip fractions are counts over mb: exact, except for samples whose fp64 value lies within 1e-5 of the boundary
    for frac, count, border in (("clip_fraction", "clipped_count", "borderline"), ("value_clip_fraction", "v_clipped_count", "v_borderline")):
        c = d[frac] * len(idx)
        report(f"count-{frac} od{od} mb{mb} {name} (borderline {st_r[border]})", abs(c - st_r[count]))
        assert abs(c - round(c)) < 1e-3 and abs(round(c) - st_r[count]) <= st_r[border], (frac, d, st_r)
    return st_r


@pytest.mark.parametrize("name", list(TERM_CASES))
@pytest.mark.parametrize("mb", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("od", [15, 8])
def test_extended_gradient_and_diagnostics_match_autograd(od, mb, name):
    idx = minibatch_indices(mb, CT * CN, seed=mb)
    st_r = check_step(od, mb, idx, TERM_CASES[name], name)
    if mb == 257 and "clip_range_vf" in TERM_CASES[name]:          # the inputs really exercise the value clip, and none sits on its boundary
        assert 0.2 * mb <= st_r["v_clipped_count"] <= 0.8 * mb and st_r["v_borderline"] == 0, st_r
    if "clip_range_vf" not in TERM_CASES[name]:
        assert st_r["v_clipped_count"] == 0


@pytest.mark.parametrize("od", [15, 8])
def test_out_of_range_indices_are_left_out_of_the_statistics_and_every_sum(od):
    n = CT * CN
    good = minibatch_indices(40, n, seed=9)
    bad = torch.tensor([-1, n, -7, n + 5, 2 ** 40, -2 ** 40] * 5)[:25]
    idx = torch.cat([good, bad])[torch.randperm(65, generator=torch.Generator().manual_seed(4))]
    st_r = check_step(od, 65, idx, LS.ALL_TERMS, "all+bad-indices")
    assert st_r["valid"] == 40
    # a minibatch whose only valid row is one sample: its advantage is used as it is
    one = torch.cat([bad[:3], torch.tensor([17]), bad[3:6]])
    check_step(od, 7, one, LS.ALL_TERMS, "all+one-valid-row")


@pytest.mark.parametrize("od", [15, 8])
def test_every_term_off_gives_the_bits_of_the_old_step(od):
    mb = 257
    idx = minibatch_indices(mb, CT * CN, seed=mb)
    buf, adv, ret, adv_stats = (t.to(DEV) for t in step_inputs(od))
    L = make_learner(od)
    P = L.num_params
    params = LS.flat_params(state_dict(od), od, DEV); m = torch.zeros(P, device=DEV); v = torch.zeros(P, device=DEV)
    stats = torch.zeros(4, device=DEV); grads = torch.full((P,), float("nan"), device=DEV)
    for step in (1, 2):                                          # the second step starts from non-zero moments
        L.minibatch_step(buf, idx.to(DEV), adv, ret, adv_stats, params, m, v, step, stats, grads=grads)
    start = None
    for step in (1, 2):
        p2, m2, v2, diag, g2, state = gpu_step(L, od, idx, {}, use_state=False, start=start)
        start = (p2, m2, v2, 2)
    assert state is None
    assert torch.equal(p2, params) and torch.equal(m2, m) and torch.equal(v2, v) and torch.equal(g2, grads) and torch.equal(diag[:4], stats)
    assert float((p2 - LS.flat_params(state_dict(od), od, DEV)).abs().max()) > 1e-4
    a = gpu_step(L, od, idx, LS.ALL_TERMS, target_kl=10.0)
    b = gpu_step(L, od, idx, LS.ALL_TERMS, target_kl=10.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], p2)


def test_extended_step_checks_its_arguments():
    from so100_mujoco_rl_amd.lib import So100Error
    od = 15
    L = make_learner(od, 64)
    idx = minibatch_indices(8, CT * CN, seed=1)
    before = gpu_step(L, od, idx, {})[0]
    for terms, kw, word in ((dict(ent_coef=-0.01), {}, "ent_coef"), (dict(ent_coef=float("nan")), {}, "ent_coef"),
                            ({}, dict(target_kl=0.05, use_state=False), "target_kl"), (dict(clip_range_vf=float("nan")), {}, "clip_range_vf")):
        with pytest.raises(So100Error, match=word):
            gpu_step(L, od, idx, terms, **kw)
    with pytest.raises(So100Error, match="mb"):
        gpu_step(L, od, minibatch_indices(65, CT * CN, seed=1), {})
    with pytest.raises(So100Error, match="normalize_advantage"):
        gpu_step(L, od, idx, dict(normalize_advantage="chunk"))
    buf, _, ret, _ = (t.to(DEV) for t in step_inputs(od))
    with pytest.raises(So100Error):
        L.explained_variance(buf, ret, torch.zeros(2, device=DEV))
    assert torch.equal(gpu_step(L, od, idx, {})[0], before)      # the handle is as good as before


# ---- whole updates with a stop ------------------------------------------------------------------------------------------------------------------
UPD_EPOCHS, UPD_MB, UPD_LR = 3, 260, 3e-3


def update_perms():
    g = torch.Generator().manual_seed(77)
    return [torch.randperm(CT * CN, generator=g) for _ in range(UPD_EPOCHS)]


def update_minibatches():
    return [perm[i:i + UPD_MB] for perm in update_perms() for i in range(0, CT * CN, UPD_MB)]


def reference_update(od, target_kl):
    buf = chunk(od)[0]
    ref = LS.RefLearner(od, state_dict(od), lr=UPD_LR, target_kl=target_kl, **LS.ALL_TERMS)
    adv, ret, mean, std = reference_advantages(od)
    steps = [ref.step(buf, idx, adv, ret, mean, std)[0] for idx in update_minibatches()]
    return ref, [st for st in steps if st is not None]


@functools.lru_cache(maxsize=None)
def free_running_kl(od):
    return [st["approx_kl"] for st in reference_update(od, None)[1]]


def update_batch(od):
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    buf, tobs, last_obs = chunk(od)
    c = RolloutChunk(CT, CN, od, DEV); c.buf.copy_(buf)
    b = c.unpack(); b["last_obs"] = last_obs.to(DEV); b["terminal_obs"] = tobs.to(DEV); b["packed"] = c.buf
    return b


def fused_update(od, target_kl):
    from so100_mujoco_rl_amd.ppo import FusedPPO
    f = FusedPPO(od, DEV, lr=UPD_LR, epochs=UPD_EPOCHS, minibatch=UPD_MB, seed=1, target_kl=target_kl, **LS.ALL_TERMS)
    f.net.load_state_dict({k: v.to(DEV) for k, v in state_dict(od).items()})
    return f, f.update(update_batch(od), perms=[p.to(DEV) for p in update_perms()])


def fused_steps(od, count):
    """the first `count` steps of the update through the C ABI, with no stop"""
    L = make_learner(od, UPD_MB, lr=UPD_LR)
    b = update_batch(od)
    P = L.num_params
    params = LS.flat_params(state_dict(od), od, DEV); m = torch.zeros(P, device=DEV); v = torch.zeros(P, device=DEV)
    adv = torch.zeros(CT, CN, device=DEV); ret = torch.zeros(CT, CN, device=DEV); adv_stats = torch.zeros(2, device=DEV); diag = torch.zeros(8, device=DEV)
    L.advantages(b["packed"], b["last_obs"], params, adv, ret, adv_stats, terminal_obs=b["terminal_obs"])
    for step, idx in enumerate(update_minibatches()[:count], 1):
        L.minibatch_step_ex(b["packed"], idx.to(DEV), adv, ret, adv_stats, params, m, v, step, diag, **LS.ALL_TERMS)
    return params, m, v


def stop_step(od, later):
    """a step s whose approx_kl is at least 1.2 x every earlier one: the first such from 2 on, or the first from 4 on (a later epoch)"""
    k = free_running_kl(od)
    assert len(k) == 9
    picks = [s for s in range(4 if later else 2, 9) if k[s - 1] >= 1.2 * max(k[:s - 1])]
    assert picks, k
    return picks[0], k


@pytest.mark.parametrize("od,later", [(15, False), (8, False), (15, True)])
def test_update_with_a_stop(od, later):
    s, k = stop_step(od, later)
    print(f"[terms-tol] reference approx_kl od{od}", [f"{x:.5f}" for x in k], "stop at", s, "ratio", k[s - 1] / max(k[:s - 1]))
    target = math.sqrt(k[s - 1] * max(k[:s - 1])) / 1.5            # 1.5 target_kl: the geometric mean, >= 9.5 % away from either side
    ref, steps = reference_update(od, target)
    assert ref.stopped and ref.applied == s - 1 and len(steps) == s
    f, stats = fused_update(od, target)
    assert stats["n_updates"] == s - 1 and stats["early_stop"] is True and f.adam_step == s - 1
    assert f._state.tolist() == [1, s - 1]
    e_kl = report(f"stop-approx_kl od{od} s{s}", abs(stats["approx_kl"] - k[s - 1]) / max(k[s - 1], 1e-2))
    assert e_kl <= STAT_TOL
    want = ref.net.state_dict(); mom = ref.moments()
    got_p, got_m, got_v = LS.split_flat(f.params, od), LS.split_flat(f.adam_m, od), LS.split_flat(f.adam_v, od)
    ep = max(LS.rel_err(got_p[n], want[n]) for n in want)
    em = max(LS.rel_err(got_m[n], mom[n][0]) for n in want); ev = max(LS.rel_err(got_v[n], mom[n][1]) for n in want)
    report(f"stop-params od{od} s{s}", ep); report(f"stop-exp_avg od{od} s{s}", em); report(f"stop-exp_avg_sq od{od} s{s}", ev)
    assert ep <= PARAM_TOL and em <= MOMENT_TOL and ev <= MOMENT_TOL
    p, m, v = fused_steps(od, s - 1)                             # a run that was simply given s - 1 steps: the same bits
    assert torch.equal(f.params, p) and torch.equal(f.adam_m, m) and torch.equal(f.adam_v, v)
    assert float((f.params - LS.flat_params(state_dict(od), od, DEV)).abs().max()) > 1e-3
    # without target_kl all nine steps are applied
    if not later:
        g, st = fused_update(od, None)
        assert st["n_updates"] == 9 and st["early_stop"] is False and g.adam_step == 9 and not torch.equal(g.params, f.params)
        e = report(f"free-approx_kl od{od}", abs(st["approx_kl"] - k[8]) / max(k[8], 1e-2))
        assert e <= STAT_TOL


@pytest.mark.parametrize("od", [15, 8])
def test_default_fused_update_keeps_the_old_bits_and_reports_the_diagnostics(od):
    """FusedPPO with no new option: the parameters and moments are those of the old entry point called step by step (what the learner did before
    it had options), and the diagnostics it now returns beside them agree with the fp64 reference.  vf_coef 0.7, not the default, so that `loss`
    is held to its own coefficient.  The one exception to "both learners return the same keys": approx_kl is NaN here, because the old step does
    not form it and the default path runs nothing but the old step; ppo.PPO and the extended step return a value."""
    from so100_mujoco_rl_amd.ppo import FusedPPO
    vf, epochs = 0.7, 2
    perms = update_perms()[:epochs]
    batches = update_minibatches()[:epochs * 3]
    f = FusedPPO(od, DEV, epochs=epochs, minibatch=UPD_MB, vf_coef=vf, seed=1)
    assert not f._extended
    f.net.load_state_dict({k: v.to(DEV) for k, v in state_dict(od).items()})
    stats = f.update(update_batch(od), perms=[p.to(DEV) for p in perms])
    # the old entry point, step by step
    L = make_learner(od, UPD_MB, vf_coef=vf)
    b = update_batch(od)
    P = L.num_params
    params = LS.flat_params(state_dict(od), od, DEV); m = torch.zeros(P, device=DEV); v = torch.zeros(P, device=DEV)
    adv = torch.zeros(CT, CN, device=DEV); ret = torch.zeros(CT, CN, device=DEV); adv_stats = torch.zeros(2, device=DEV); st4 = torch.zeros(4, device=DEV)
    L.advantages(b["packed"], b["last_obs"], params, adv, ret, adv_stats, terminal_obs=b["terminal_obs"])
    for step, idx in enumerate(batches, 1):
        L.minibatch_step(b["packed"], idx.to(DEV), adv, ret, adv_stats, params, m, v, step, st4)
    assert torch.equal(f.params, params) and torch.equal(f.adam_m, m) and torch.equal(f.adam_v, v) and f.adam_step == 6
    assert [stats[k] for k in ("policy_loss", "value_loss", "clip_fraction", "grad_norm")] == st4.tolist()
    # the fp64 reference
    ref = LS.RefLearner(od, state_dict(od), vf_coef=vf)
    adv_r, ret_r, mean_r, std_r = reference_advantages(od)
    for idx in batches:
        last, _ = ref.step(chunk(od)[0], idx, adv_r, ret_r, mean_r, std_r)
    want = {"value_loss": last["value_loss"], "policy_loss": last["policy_loss"], "entropy_loss": last["entropy_loss"], "loss": last["loss"],
            "explained_variance": LS.ref_explained_variance(ret_r.numpy(), chunk(od)[0][..., od + 8].double().numpy()),
            "std": ref.net.log_std.detach().exp().mean().item()}
    assert abs(last["loss"] - (last["policy_loss"] + vf * last["value_loss"])) < 1e-12 and abs(want["entropy_loss"]) > 1.0
    for k, w in want.items():
        e = report(f"default-{k} od{od}", abs(stats[k] - w) / max(abs(w), 1e-2))
        assert e <= STAT_TOL, (k, stats[k], w)
    assert stats["n_updates"] == 6 and stats["early_stop"] is False and math.isnan(stats["approx_kl"])
    # no raw_reward_mean in this batch: both reward means are the mean of the chunk's reward column (780 values of order 1 summed in fp32:
    # within 780 x 6e-8 x max|r| / 780 < 1e-6 of the fp64 mean, whatever the order of the sum)
    assert stats["mean_reward"] == stats["mean_bootstrapped_reward"]
    assert abs(stats["mean_reward"] - chunk(od)[0][..., od + 6].double().mean().item()) < 1e-6


# ---- explained variance -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od,T,N", [(15, 6, 130), (8, 6, 130), (15, 1, 1), (15, 9, 1031)])
def test_explained_variance_matches_numpy(od, T, N):
    """(1, 1): var(ret) = 0, NaN.  (9, 1031): 9279 rows, ten workgroups with a ragged last one -- the ordered merge of the second stage; the
    same chunk with a constant ret of 0.1 (whose rounded mean need not equal it) has variance 0 all the same: NaN, not a ratio of roundings."""
    buf = chunk(od, T, N)[0]
    g = torch.Generator().manual_seed(T * N)
    ret = buf[..., od + 8] + 0.7 * torch.randn(T, N, generator=g) + 0.3
    L = make_learner(od, 64)
    out = torch.full((1,), 7.0, device=DEV)
    if T * N > 5000:
        L.explained_variance(buf.to(DEV), torch.full((T, N), 0.1, device=DEV), out)
        assert math.isnan(out.item())
        # the row counts are carried as floats: more than 2^24 rows are refused before anything is launched
        assert L.L.so100_learner_explained_variance(L.h, buf.to(DEV).data_ptr(), ret.to(DEV).data_ptr(), 2 ** 24 + 1, out.data_ptr(), L._stream()) == -1
        assert b"num_samples" in L.L.so100_last_error()
    L.explained_variance(buf.to(DEV), ret.to(DEV), out)
    want = LS.ref_explained_variance(ret.numpy(), buf[..., od + 8].numpy())
    if T * N == 1:
        assert math.isnan(want) and math.isnan(out.item())
        return
    assert 0.05 < want < 0.95
    assert report(f"explained-variance od{od} {T}x{N}", abs(out.item() - want)) <= EV_TOL
    out2 = torch.zeros(1, device=DEV)
    L.explained_variance(buf.to(DEV), ret.to(DEV), out2)
    assert torch.equal(out, out2)


# ---- against the PyTorch learner, and the command line -----------------------------------------------------------------------------------------
def test_one_training_iteration_with_all_options_against_the_torch_learner():
    """test_one_training_iteration_against_the_torch_learner with every option on: Env01 x 256 envs, T = 16, one update, the same seeds.
    target_kl 0.5 is far above any approx_kl of a first update: the stop machinery runs and never fires."""
    from so100_mujoco_rl_amd.collector import RolloutCollector
    from so100_mujoco_rl_amd.ppo import PPO, FusedPPO
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    opts = dict(target_kl=0.5, lr_schedule=lambda progress: 3e-4 * progress, **LS.ALL_TERMS)
    out = {}
    for name, cls, defer in (("torch", PPO, False), ("fused", FusedPPO, True)):
        learner = cls(15, DEV, seed=3, **opts)
        env = So100VecEnv("Env01-v1", 256, seed=11, max_episode_steps=8)
        col = RolloutCollector(env, learner.net.state_dict(), T=16, defer_bootstrap=defer)
        b = col.collect()
        torch.manual_seed(99)
        stats = learner.update(b, progress_remaining=0.5)
        out[name] = ({k: v.detach().clone() for k, v in learner.net.state_dict().items()}, stats)
    (p_t, s_t), (p_f, s_f) = out["torch"], out["fused"]
    worst = max(LS.rel_err(p_f[k], p_t[k]) for k in p_t)
    report("end-to-end params fused vs torch, all options", worst)
    assert worst <= E2E_PARAM_TOL
    assert s_f["n_updates"] == s_t["n_updates"] == 4 and s_f["early_stop"] is False and s_t["early_stop"] is False
    for k in ("value_loss", "approx_kl", "entropy_loss", "loss", "explained_variance", "std", "mean_reward"):
        e = report(f"end-to-end {k} fused vs torch", abs(s_f[k] - s_t[k]) / max(abs(s_t[k]), 1e-2))
        assert e <= E2E_STAT_TOL, (k, s_f[k], s_t[k])


@pytest.mark.parametrize("learner", ["fused", "torch"])
def test_cli_train_with_the_new_flags(tmp_path, monkeypatch, caplog, learner):
    import logging
    from click.testing import CliRunner
    from so100_mujoco_rl_amd import main as drv
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO, logger=drv.logger.name)
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "-e", "Env01-v1", "--envs", "256", "--iters", "2", "--learner", learner, "--ent-coef", "0.01",
                                     "--clip-range-vf", "0.3", "--target-kl", "0.05", "--normalize-advantage", "minibatch"], catch_exceptions=False)
    assert r.exit_code == 0
    assert (tmp_path / "models" / "Env01-v1_PPO" / "best_model.pt").is_file()
    lines = caplog.messages
    diag = [l for l in lines if "approx_kl" in l]
    assert diag and all(w in diag[-1] for w in ("entropy_loss", "explained_variance", "std", "n_updates")), lines
