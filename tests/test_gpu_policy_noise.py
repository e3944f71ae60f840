"""Every random number the kernels draw for themselves against an independent reference.

The policy noise: with mu_w = 0, mu_b = 0 and log_std = 0 the stored raw action is fma(exp(0), eps, 0) = eps, so the noise both kernels
drew can be read out of the rollout buffer and compared, EVERY value, with oracle.so100_oracle.policy_noise_ref (numpy uint64 Philox +
float64 Box-Muller; tests/test_rng_reference.py holds that sampler to Random123's known answers and to N(0, 1)).  Covered: the stepwise
kernel so100_policy_forward_mfma at the edges of its step counter; the persistent kernel so100_rollout_fused at observation widths 15 / 8
and 16 / 32 / 64 envs per workgroup, with a partly filled last workgroup, across two launches (the counter hand-over, the prologue draw and
wave 3's pre-draw for step t + 1) and across auto-resets; seeds with and without a high word; env_id_offset up to the wrap of its uint32;
sharding; the stored log-prob against the log-density of the reference noise; a resumed run (sim checkpoint + collector.state_dict()).

The env's own draws: every kind 1-6 stepped without injected uniforms against OracleEnv(kind, seed, env_id) drawing its own, at the seed
whose float32 host twin tests/test_rng_reference.py::test_uninjected_task_layer_fp32_vs_oracle holds to the same bounds."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import LOG2PI_HALF, policy_tensors, run_pair, state_err   # noqa: E402
from oracle import so100_oracle as O                      # noqa: E402  (the checker)
from scenes import FREE, UNINJECTED_CASES, UNINJECTED_N, UNINJECTED_SEED, UNINJECTED_STEPS, UNINJECTED_TIMELIMIT      # noqa: E402

BIG_SEED = 0xDEADBEEF12345                                 # seed_hi != 0
# bounds against the float64 reference sampler: about 3x the worst error measured on MI355X over every case below
NOISE_EPS = 2.3e-6                                         # measured 7.6e-7: |raw action - eps_ref| over every case below, both kernels (they agree bit for bit)
NOISE_LOGP = 1.1e-5                                        # measured 3.6e-6: |stored log-prob - (sum(-eps_ref^2 / 2) - 6 ln(2 pi) / 2)|, at |eps_ref| up to 4.5


def _noise_policy(od, device, seed=0):
    """random towers, mu_w = 0, mu_b = 0, log_std = 0: the raw action IS the noise"""
    from so100_mujoco_rl_amd.collector import RolloutCollector
    sd = RolloutCollector.random_policy_state(od, device, seed=seed)
    sd["action_net.weight"] = torch.zeros_like(sd["action_net.weight"]); sd["action_net.bias"] = torch.zeros_like(sd["action_net.bias"])
    assert float(sd["log_std"].abs().max()) == 0.0
    return sd


def _gid(offset, n):
    return (offset + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)        # env_id_offset + env in uint32 arithmetic


def _logp_ref(eps):
    return (-0.5*eps**2).sum(-1) - 6*LOG2PI_HALF


def _check(raw, logp, ref, what):
    """every value of raw [.., n, 6] and logp [.., n] (device float32) against the reference noise ref (float64)"""
    raw = raw.double().cpu().numpy(); logp = logp.double().cpu().numpy()
    assert raw.shape == ref.shape and np.isfinite(raw).all()
    ee = float(np.abs(raw - ref).max()); el = float(np.abs(logp - _logp_ref(ref)).max())
    print(f"[policy noise vs reference, {what}] {raw.size} draws: eps {ee:.2e} log-prob {el:.2e} (max |eps_ref| {np.abs(ref).max():.2f})")
    assert ee < NOISE_EPS, (what, ee)
    assert el < NOISE_LOGP, (what, el)
    return ee, el


@pytest.mark.parametrize("kind", [1, 5])
@pytest.mark.parametrize("seed,offset", [(4, 0), (BIG_SEED, 1000), (4, 2**31), (BIG_SEED, 2**32 - 100)])
def test_stepwise_kernel_noise_vs_reference(kind, seed, offset):
    """so100_policy_forward_mfma with noise=None at step counters 0, 1, 2^31 and 2^32 - 1: act_raw, logp, the rollout row and
    act_env == clamp(act_raw), all 200 x 6 values per counter"""
    from so100_mujoco_rl_amd.lib import So100Sim
    n = 200
    sim = So100Sim(kind, n, flags=FREE, seed=seed, env_id_offset=offset)
    od = sim.obs_dim
    sim.set_policy(policy_tensors(_noise_policy(od, sim.device, seed=kind)))
    g = torch.Generator(device="cuda"); g.manual_seed(kind)
    obs = torch.randn(n, od, device="cuda", generator=g).contiguous()
    # exp(0) == 1 on the device and the zero head gives mean == 0: an injected noise comes back as the raw action, bit for bit
    given = (torch.randn(n, 6, device="cuda", generator=g)*2).contiguous()
    act_env = torch.zeros(n, 6, device="cuda"); raw = torch.zeros_like(act_env); logp = torch.zeros(n, device="cuda")
    sim.policy_forward(obs, act_env, 0, noise=given, act_raw=raw, logp=logp)
    assert torch.equal(raw, given)
    for counter in (0, 1, 2**31, 2**32 - 1):
        raw.zero_(); logp.zero_(); act_env.zero_(); value = torch.zeros(n, device="cuda"); row = torch.zeros(n, od + 10, device="cuda")
        sim.policy_forward(obs, act_env, counter, act_raw=raw, value=value, logp=logp, rollout_row=row)
        ref = O.policy_noise_ref(seed, _gid(offset, n), counter)
        _check(raw, logp, ref, f"stepwise kernel, obs width {od}, seed {seed:#x}, offset {offset}, counter {counter}")
        assert torch.equal(row[:, od:od + 6], raw) and torch.equal(row[:, od + 9], logp) and torch.equal(row[:, od + 8], value)
        assert torch.equal(row[:, :od], obs) and torch.equal(act_env, raw.clamp(-1, 1))
    sim.close()


def _collect_two_chunks(kind, n, seed, offset, epw, T=10, T2=5, tl=7, flags=FREE):
    """(raw actions [T + T2, n, 6], log-probs, dones, obs) of two launches of the persistent kernel; the TimeLimit fires inside both"""
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    from so100_mujoco_rl_amd.collector import RolloutCollector
    env = So100VecEnv(kind, n, flags=flags, seed=seed, env_id_offset=offset, max_episode_steps=tl, envs_per_workgroup=epw)
    if epw:
        assert env.sim.envs_per_workgroup == epw
    col = RolloutCollector(env, _noise_policy(env.sim.obs_dim, env.device, seed=kind), T=T, persistent=True, bootstrap_truncated=False)
    b1 = {k: v.clone() for k, v in col.collect().items()}
    b2 = {k: v.clone() for k, v in col.collect(T2).items()}
    assert col.counter == T + T2
    out = {k: torch.cat([b1[k], b2[k]], 0) for k in ("actions", "log_probs", "dones", "obs", "values")}
    env.close()
    return out


@pytest.mark.parametrize("kind", [1, 5])
@pytest.mark.parametrize("epw", [16, 32, 64])
@pytest.mark.parametrize("seed,offset", [(4, 0), (BIG_SEED, 1000), (4, 2**31), (BIG_SEED, 2**32 - 100)])
def test_persistent_kernel_noise_vs_reference(kind, epw, seed, offset):
    """so100_rollout_fused, two launches of 10 and 5 steps over 200 envs (the last workgroup is partly filled): step s of launch 2 must
    carry the reference noise of counter 10 + s, and an env that was auto-reset inside a launch keeps drawing at the global counter"""
    n, T, T2, tl = 200, 10, 5, 7
    b = _collect_two_chunks(kind, n, seed, offset, epw, T, T2, tl)
    ref = O.policy_noise_ref(seed, _gid(offset, n)[None, :], np.arange(T + T2)[:, None])
    done = b["dones"].cpu().numpy() > 0
    assert done[:T].any() and done[T:].any() and done.sum() == 2*n             # every env: auto-reset in launch 1 (step 7) and in launch 2 (step 14)
    _check(b["actions"], b["log_probs"], ref, f"persistent kernel, kind {kind}, epw {epw}, seed {seed:#x}, offset {offset}")
    # the steps after an auto-reset, on their own
    after = np.zeros_like(done); after[1:] = done[:-1]
    assert after.sum() == 2*n and np.abs(b["actions"].double().cpu().numpy()[after] - ref[after]).max() < NOISE_EPS


@pytest.mark.parametrize("kind", [1, 5])
def test_persistent_and_stepwise_kernels_draw_the_same_noise(kind):
    """the two kernels call one function with one keying: with a zero mean and exp(0) = 1 their raw actions are the same bits"""
    from so100_mujoco_rl_amd.lib import So100Sim
    n, seed, offset = 200, BIG_SEED, 1000
    b = _collect_two_chunks(kind, n, seed, offset, 32)
    sim = So100Sim(kind, n, flags=FREE, seed=seed, env_id_offset=offset)
    sim.set_policy(policy_tensors(_noise_policy(sim.obs_dim, sim.device, seed=kind)))
    act_env = torch.zeros(n, 6, device="cuda"); raw = torch.zeros_like(act_env); logp = torch.zeros(n, device="cuda")
    for t in range(15):
        sim.policy_forward(b["obs"][t].contiguous(), act_env, t, act_raw=raw, logp=logp)
        assert torch.equal(raw, b["actions"][t]), t
        assert torch.allclose(logp, b["log_probs"][t], rtol=0, atol=1e-6)          # the bound test_persistent_rollout_equals_stepwise uses
    sim.close()


@pytest.mark.parametrize("kind", [1, 5])
def test_two_shards_draw_the_noise_of_one_handle(kind):
    """two handles of 100 envs at env_id_offset 0 and 100 == one handle of 200, bit for bit (noise and its log-prob)"""
    whole = _collect_two_chunks(kind, 200, BIG_SEED, 0, 32)
    lo = _collect_two_chunks(kind, 100, BIG_SEED, 0, 32); hi = _collect_two_chunks(kind, 100, BIG_SEED, 100, 32)
    for k in ("actions", "log_probs"):
        assert torch.equal(torch.cat([lo[k], hi[k]], 1), whole[k]), k


def test_resumed_collector_continues_the_noise_stream(tmp_path):
    """collect, checkpoint (sim.save_state + collector.state_dict()), collect again; a fresh env and collector loaded from the checkpoint
    must reproduce that second chunk bit for bit, and its noise is the reference at the continued counter (not at 0 again)"""
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    from so100_mujoco_rl_amd.collector import RolloutCollector
    n, T, seed = 200, 6, BIG_SEED
    mk = lambda: So100VecEnv(1, n, seed=seed, max_episode_steps=4)             # the default physics; a TimeLimit reset inside every chunk
    env = mk(); sd = _noise_policy(15, env.device, seed=7)
    col = RolloutCollector(env, sd, T=T, persistent=True)
    first = {k: v.clone() for k, v in col.collect().items()}
    path = str(tmp_path / "sim.npz"); env.sim.save_state(path); saved = dict(col.state_dict())
    assert saved == {"counter": T, "started": True}
    second = {k: v.clone() for k, v in col.collect().items()}
    env2 = mk(); col2 = RolloutCollector(env2, sd, T=T, persistent=True)
    env2.sim.load_state(path); col2.load_state_dict(saved)
    again = col2.collect()
    for k in ("obs", "actions", "rewards", "dones", "values", "log_probs", "last_obs", "truncated"):
        assert torch.equal(again[k], second[k]), k
    assert col2.counter == 2*T and col2.state_dict() == col.state_dict()
    gid = _gid(0, n)
    _check(again["actions"], again["log_probs"], O.policy_noise_ref(seed, gid[None, :], T + np.arange(T)[:, None]), "resumed collector, second chunk")
    assert not torch.equal(again["actions"], first["actions"])                 # the stream went on; it did not start over
    env.close(); env2.close()


@pytest.mark.parametrize("kind", [1, 2, 3, 4, 5, 6])
def test_uninjected_env_draws_vs_oracle(kind):
    """The env's own Philox draws (reset pose, cube placement, cube targets, Env05's detection noise) never injected: 64 envs, two
    auto-resets each, against OracleEnv(kind, seed, env_id) drawing from its own stream.  Bounds: those of the injected comparisons of the
    same kind and flags (test_env01_vs_oracle, test_env02_vs_oracle_with_reach_branch, test_env06_vs_oracle_with_gripper_term,
    _lookat_envs_vs_oracle) and none beyond them."""
    flags, scale = UNINJECTED_CASES[kind]
    n, steps, seed, tl = UNINJECTED_N, UNINJECTED_STEPS, UNINJECTED_SEED, UNINJECTED_TIMELIMIT
    reach = kind in (1, 2, 6)
    n_px = n_px_bad = resets = 0
    worst_o = worst_r = 0.0
    for t, sim, orc, og, oo, rew, done, trunc, _ in run_pair(kind, flags, n, steps, seed=seed, action_scale=scale, max_steps=tl, inject=False):
        if t < 0:
            np.testing.assert_allclose(og, oo, rtol=0, atol=1e-6)              # the reset observation
            continue
        np.testing.assert_array_equal(done[0].astype(bool), done[1]); np.testing.assert_array_equal(trunc[0].astype(bool), trunc[1])
        resets += int(done[1].sum())
        if reach:
            worst_o = max(worst_o, float(np.abs(og - oo).max())); worst_r = max(worst_r, float(np.abs(rew[0] - rew[1]).max()))
            np.testing.assert_allclose(og, oo, rtol=0, atol=2e-5, err_msg=f"kind {kind} step {t}")
            np.testing.assert_allclose(rew[0], rew[1], rtol=0, atol=2e-3 if kind == 6 else 1e-4)
        else:
            np.testing.assert_allclose(og[:, :6], oo[:, :6], rtol=0, atol=1e-6)
            d = np.abs(og[:, 6:] - oo[:, 6:]); n_px += d.size; n_px_bad += int((d > 1e-4).sum())
            worst_o = max(worst_o, float(d.max())); worst_r = max(worst_r, float(np.abs(rew[0] - rew[1]).max()))
            assert d.max() < 6e-3, (t, d.max())
            np.testing.assert_allclose(rew[0], rew[1], rtol=0, atol=1.2e-2 if kind == 4 else 2e-3)
    assert t == steps - 1
    assert resets >= 2*n
    eq, ev = state_err(sim, orc)
    print(f"[un-injected env draws vs oracle, kind {kind}] obs {worst_o:.2e} reward {worst_r:.2e} pixel entries off by > 1e-4: {n_px_bad} of {n_px}; "
          f"qpos {eq:.2e} qvel {ev:.2e}; resets {resets}")
    assert n_px_bad <= 0.01*n_px
    assert eq < (2e-5 if reach else 3e-5) and ev < 5e-4
