"""The headline kernel and the policy phase against float64 references.

bench.py measures so100_rollout_fused<1, 8, 4, 32>: Env01, cube pinned (SO100_F_CUBE_PINNED), 32 envs per workgroup, the policy's
two towers on one 32-row MFMA tile each.  Here it runs through RolloutCollector(persistent=True) and 32 sampled envs are replayed in
the fp64 oracle with the actions the buffer recorded, clamped as the env applies them; the <1, 8, 4, 64> variant (two 32-row tiles)
is pinned with envs_per_workgroup=64.  Bounds: those of test_gpu_parity.py::test_env01_vs_oracle (obs 2e-5, reward 1e-4, final qpos
2e-5, qvel 5e-4) on every sampled row -- without contacts there is no contact-event class.

The policy phase (persistent kernel at 16 / 32 / 64 envs per workgroup, and the stepwise kernel so100_policy_forward_mfma; observation
widths 15 and 8) is recomputed in float64 from the stored observations, with weights that drive some units into tanh saturation
(|pre-activation| 5-20) and log_std at -3 and +1.  Bounds are about 3x the errors measured on MI355X, which stand beside them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_support import LOG2PI_HALF, torch_policy          # noqa: E402
from oracle import so100_oracle as O                      # noqa: E402  (the checker)
from scenes import FREE                                   # noqa: E402


@pytest.mark.parametrize("n,epw", [(200, 0), (4096, 0), (200, 64)])
def test_headline_rollout_kernel_vs_oracle(n, epw):
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    from so100_mujoco_rl_amd.collector import RolloutCollector
    T, T2, tl = 10, 5, 12                                    # a second, shorter chunk; the TimeLimit hits inside it
    env = So100VecEnv(1, n, flags=FREE, seed=4, max_episode_steps=tl, envs_per_workgroup=epw)
    want = 32 if epw == 0 else epw
    print(f"[headline kernel, n={n}] envs_per_workgroup == {env.sim.envs_per_workgroup}")
    assert env.sim.envs_per_workgroup == want                # 32: so100_rollout_fused<1, 8, 4, 32>, what bench.py measures
    sd = RolloutCollector.random_policy_state(15, env.device, seed=2)
    col = RolloutCollector(env, sd, T=T, persistent=True, bootstrap_truncated=False)
    b = {k: v.clone() for k, v in col.collect().items()}
    b2 = {k: v.clone() for k, v in col.collect(T2).items()}
    for k in ("obs", "actions", "rewards", "dones"):
        b[k] = torch.cat([b[k], b2[k]], 0)
    q, v = env.sim.get_state()
    T = T + T2
    assert b["dones"].sum() > 0
    act = b["actions"].clamp(-1, 1).cpu().numpy(); obs = b["obs"].cpu().numpy(); rew = b["rewards"].cpu().numpy()
    last = b2["last_obs"].cpu().numpy(); qg = q.cpu().numpy().T; vg = v.cpu().numpy().T
    worst_o = worst_r = worst_q = worst_v = 0.0
    for i in np.linspace(0, n - 1, 32).astype(int):
        e = O.OracleEnv(1, flags=FREE, iters=0, seed=4, env_id=int(i)); e.e.max_episode_steps = tl
        worst_o = max(worst_o, np.abs(e.reset() - obs[0, i]).max())
        for t in range(T):
            o, r = e.step(act[t, i], autoreset=True)[:2]
            og = obs[t + 1, i] if t + 1 < T else last[i]
            worst_o = max(worst_o, np.abs(og - o).max()); worst_r = max(worst_r, abs(rew[t, i] - r))
        worst_q = max(worst_q, np.abs(qg[i] - O.arr(e.d.qpos)).max()); worst_v = max(worst_v, np.abs(vg[i] - O.arr(e.d.qvel)).max())
    print(f"[headline kernel vs oracle, n={n} epw={want}] 32 envs x {T} steps: obs {worst_o:.2e} reward {worst_r:.2e} qpos {worst_q:.2e} qvel {worst_v:.2e}")
    assert worst_o < 2e-5 and worst_r < 1e-4
    assert worst_q < 2e-5 and worst_v < 5e-4


def _saturating_policy(od, seed):
    """random towers whose first- and second-layer pre-activations reach |x| ~ 5-20 in some units (row scales 0.1 .. 2), log_std -3 / +1"""
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    rows = torch.linspace(0.1, 2.0, 64, dtype=torch.float64)[torch.randperm(64, generator=g)]
    t = {}
    for tw in ("pi", "vf"):
        t[f"{tw}_w0"] = rnd(64, od)*rows[:, None]; t[f"{tw}_b0"] = rnd(64)*0.5
        t[f"{tw}_w1"] = rnd(64, 64)*rows[:, None]*0.5; t[f"{tw}_b1"] = rnd(64)*0.5
    t["mu_w"] = rnd(6, 64)*0.3; t["mu_b"] = rnd(6)*0.1; t["log_std"] = torch.tensor([-3.0, 1.0, -3.0, 1.0, -3.0, 1.0], dtype=torch.float64)
    t["v_w"] = rnd(1, 64)*0.5; t["v_b"] = rnd(1)
    return {k: v.float().cuda().contiguous() for k, v in t.items()}


def _fp64(t, obs):
    """(mean, value) of both towers in float64 on the host from float32 weights and observations"""
    t64 = {k: v.double().cpu() for k, v in t.items()}
    mean, value, _ = torch_policy(t64, obs.double().cpu(), torch.zeros(obs.shape[0], 6, dtype=torch.float64))
    return mean, value


def _pre_activation_range(t, obs):
    t = {k: v.double().cpu() for k, v in t.items()}
    x1 = obs.double().cpu() @ t["pi_w0"].T + t["pi_b0"]
    x2 = torch.tanh(x1) @ t["pi_w1"].T + t["pi_b1"]
    return float(x1.abs().max()), float(x2.abs().max()), float((x1.abs() > 5).double().mean()), float((x2.abs() > 5).double().mean())


# bounds against float64: about 3x the worst error measured on MI355X over obs widths 15 / 8 and 16 / 32 / 64 envs per workgroup.
# The persistent kernel's log-prob is recomputed from the stored raw action: at log_std = -3 an fp32 mean error of ~2e-6 moves the
# recovered eps by ~4e-5, which is what dominates that bound.
PERSISTENT_VALUE, PERSISTENT_LOGP = 1.5e-5, 4e-4           # measured 4.9e-6, 1.4e-4
# ... and against the reference noise itself (oracle.policy_noise_ref: the eps the kernel must have drawn for that env and step), which
# needs no recovery: raw action against mean64 + exp(log_std) eps_ref, stored log-prob against the log-density of eps_ref
PERSISTENT_ACTION_REF, PERSISTENT_LOGP_REF = 1e-5, 5e-6    # measured 3.4e-6, 1.6e-6 (the recovered-eps log-prob above: 1.4e-4, bound 4e-4)
STEPWISE_ACTION, STEPWISE_VALUE, STEPWISE_LOGP = 8e-6, 8e-6, 2.5e-6     # measured 2.7e-6, 2.7e-6, 8.1e-7


@pytest.mark.parametrize("kind,epw", [(1, 16), (1, 32), (1, 64), (5, 16), (5, 32), (5, 64)])
def test_policy_phase_vs_fp64(kind, epw):
    """persistent kernel (obs width 15: Env01; 8: Env05) at 16 / 32 / 64 envs per workgroup, then the stepwise kernel on the same
    observations.  Persistent: value within the bound of the fp64 value; eps = (raw action - mean64) / exp(log_std) and the kernel's
    log-prob within the bound of the fp64 log-prob of that eps; the env stepped with clamp(raw, -1, 1) (oracle replay).  And with nothing
    taken from the kernel: raw action against mean64 + exp(log_std) eps_ref and the stored log-prob against the log-density of eps_ref, where
    eps_ref = oracle.policy_noise_ref(seed, env, step) is the noise the kernel is meant to have drawn."""
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    from so100_mujoco_rl_amd.collector import RolloutCollector
    from so100_mujoco_rl_amd.lib import POLICY_TENSORS, SB3_STATE_DICT_KEYS
    n, T = 200, 8
    env = So100VecEnv(kind, n, flags=FREE, seed=6, max_episode_steps=5, envs_per_workgroup=epw)
    assert env.sim.envs_per_workgroup == epw
    od = env.sim.obs_dim
    t = _saturating_policy(od, 10*kind + epw)
    sd = {SB3_STATE_DICT_KEYS[k]: t[k].clone() for k in POLICY_TENSORS}
    col = RolloutCollector(env, sd, T=T, persistent=True, bootstrap_truncated=False)
    b = col.collect()
    obs = b["obs"].reshape(-1, od); raw = b["actions"].reshape(-1, 6).double().cpu()
    mean, value = _fp64(t, obs)
    ls = t["log_std"].double().cpu()
    eps = (raw - mean)/ls.exp()
    logp = (-0.5*eps**2 - ls - LOG2PI_HALF).sum(1)
    ev = float((b["values"].reshape(-1).double().cpu() - value).abs().max()); el = float((b["log_probs"].reshape(-1).double().cpu() - logp).abs().max())
    # the same two quantities with eps known from outside: the reference sampler at (seed 6, env, step counter = row of the chunk)
    eps_ref = torch.from_numpy(O.policy_noise_ref(6, np.arange(n)[None, :], np.arange(T)[:, None])).reshape(-1, 6)
    pa = float((raw - (mean + ls.exp()*eps_ref)).abs().max())
    pl = float((b["log_probs"].reshape(-1).double().cpu() - (-0.5*eps_ref**2 - ls - LOG2PI_HALF).sum(1)).abs().max())
    print(f"[policy vs fp64 and reference noise, obs width {od}, epw {epw}] persistent: raw action {pa:.2e} log-prob {pl:.2e} (recovered-eps log-prob {el:.2e})")
    x1, x2, s1, s2 = _pre_activation_range(t, obs)
    clipped = float((raw.abs() > 1).double().mean())
    # the stepwise policy kernel on the same observations, with the noise given explicitly: action, value and log-prob against fp64
    sim = env.sim
    noise = torch.randn(n, 6, device=sim.device, generator=torch.Generator(device=sim.device).manual_seed(kind))
    o0 = b["obs"][T//2].contiguous(); ae = torch.zeros(n, 6, device=sim.device); ar = torch.zeros_like(ae)
    vs = torch.zeros(n, device=sim.device); lps = torch.zeros(n, device=sim.device)
    sim.policy_forward(o0, ae, 0, noise=noise, act_raw=ar, value=vs, logp=lps)
    m0, v0 = _fp64(t, o0)
    nz = noise.double().cpu()
    sa = float((ar.double().cpu() - (m0 + ls.exp()*nz)).abs().max()); sv = float((vs.double().cpu() - v0).abs().max())
    sl = float((lps.double().cpu() - (-0.5*nz**2 - ls - LOG2PI_HALF).sum(1)).abs().max())
    print(f"[policy vs fp64, obs width {od}, epw {epw}] pre-activations max |x1| {x1:.1f} |x2| {x2:.1f} (share > 5: {s1:.2f} / {s2:.2f}), "
          f"raw actions outside [-1, 1] {clipped:.2f}; persistent: value {ev:.2e} log-prob {el:.2e}; stepwise: action {sa:.2e} value {sv:.2e} log-prob {sl:.2e}")
    assert x1 > 5 and x2 > 5 and s1 > 0.05 and s2 > 0.05 and clipped > 0.05   # saturated units and clipped actions were exercised
    assert ev < PERSISTENT_VALUE and el < PERSISTENT_LOGP
    assert pa < PERSISTENT_ACTION_REF and pl < PERSISTENT_LOGP_REF
    assert sa < STEPWISE_ACTION and sv < STEPWISE_VALUE and sl < STEPWISE_LOGP
    assert torch.equal(ae, ar.clamp(-1, 1))
    # what the env received: clamp(raw, -1, 1), replayed in the oracle (8 envs; Env05's last two observations carry 5 x the pixel centre)
    act = b["actions"].clamp(-1, 1).cpu().numpy(); ob = b["obs"].cpu().numpy(); last = b["last_obs"].cpu().numpy()
    worst = 0.0
    for i in range(0, n, n//8):
        e = O.OracleEnv(kind, flags=FREE, iters=0, seed=6, env_id=i); e.e.max_episode_steps = 5
        e.reset()
        for s in range(T):
            o = e.step(act[s, i], autoreset=True)[0]
            og = ob[s + 1, i] if s + 1 < T else last[i]
            worst = max(worst, np.abs(og[:6] - o[:6]).max())
            if kind == 5:
                assert np.abs(og[6:] - o[6:]).max() < 6e-3
            else:
                worst = max(worst, np.abs(og[6:] - o[6:]).max())
    assert worst < 2e-5, worst
