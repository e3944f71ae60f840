"""Every reachable cell of env kind x flag set x launcher against the fp64 oracle, on one small run (tests/matrix_support.py).

KindOps<KIND>::step and ::rollout (csrc/so100_kernels.hpp) pick one of ~110 kernel instantiations by env kind (1..6), flag set (FREE 8, ARM
11, NOPADS 7, REFP 23, C5 55 -- for the reach kinds -- and the run-time-flags build -1, reached here through UNINSTANTIATED 21 and, for the
look-at kinds, through C5 as well) and launcher:

  rollout     RolloutCollector(persistent=True), 64 envs per workgroup      so100_rollout_fused<K, FL, 4>
  rollout32   the same at 32 envs per workgroup, FREE only                  so100_rollout_fused<K, 8, 4, 32>
  mw          persistent=False: so100_policy_forward + so100_step           so100_step_mw<K, FL>
  one_wave    the same, handle created under one_wave_step_kernel()         so100_step_fused<K, FL>

114 cells.  They differ in which state rows they load and store (uses_group<KIND, FL>), in the task-layer seams (stale poses, Env03's
retarget clock, the lost counter, Env06's gripper term), in the observation width, and the persistent kernel keeps the env state in
registers across an auto-reset.  Each cell replays the 16 envs of matrix_support.SAMPLE in the oracle with the actions its buffer
recorded, clamped as the env applies them, and compares every observation, reward, done code, terminal observation, reset observation,
ep_length, the elapsed_steps / rng_counter / lost_count rows that one launch hands to the next, and the final state.  The oracle's replay itself must show each kind's branch (matrix_support.assert_events): no env is left out.

Bounds: the project's own for the same quantities, fp32 kernel against the fp64 oracle; the run is contact-free, so there is no event class
and the pad flag sets get the bounds of NOPADS (test_gpu_parity.py::_lookat_envs_vs_oracle states that rule).

  reach kinds 1, 2, 6   observations 2e-5, rewards 1e-4 (Env06: 2e-3), final qpos 2e-5, qvel 5e-4
                        (test_gpu_parity.py::test_env01/02/06_vs_oracle, test_gpu_rollout_oracle.py::test_headline_rollout_kernel_vs_oracle)
  look-at kinds 3-5     joint entries 1e-6, pixel entries < 6e-3 with at most 1 % above 1e-4, rewards 2e-3 (Env04: 1.2e-2), final qpos 3e-5,
                        qvel 5e-4 (test_gpu_parity.py::_lookat_envs_vs_oracle)

Across launchers, for one (kind, flag set), the buffers of rollout, mw and one_wave agree row by row within the tolerances of
test_gpu_parity.py::test_persistent_rollout_equals_stepwise (1e-6; rewards 2e-5); the look-at kinds' pixel entries, and what is computed
from them in the same step (reward, and the value / log-prob of the next row), have the look-at bounds of
test_gpu_parity.py::test_multiwave_step_kernel_equals_throughput_kernel (6e-3, 2e-3).  The done codes must be equal.

Worst deviations measured on MI355X per (launcher, kind family) stand in MEASURED below."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import matrix_support as S                                # noqa: E402
from gpu_support import inject_state, one_wave_step_kernel  # noqa: E402

REACH_OBS, REACH_REW, REACH_QPOS, REACH_QVEL = 2e-5, {1: 1e-4, 2: 1e-4, 6: 2e-3}, 2e-5, 5e-4
LOOK_JOINT, LOOK_PX, LOOK_PX_TIGHT, LOOK_PX_SHARE, LOOK_REW, LOOK_QPOS, LOOK_QVEL = 1e-6, 6e-3, 1e-4, 0.01, {3: 2e-3, 4: 1.2e-2, 5: 2e-3}, 3e-5, 5e-4
ACROSS, ACROSS_REW, ACROSS_PX, ACROSS_LOOK_REW = 1e-6, 2e-5, 6e-3, 2e-3

# Worst deviation from the oracle over the cells of a (launcher, kind family), measured on MI355X.  Reach kinds: (obs, reward of Env01/02,
# reward of Env06, qpos, qvel); look-at kinds: (joint entries, pixel entries, share of pixel entries above 1e-4, reward of Env03/05, reward of
# Env04, qpos, qvel).  Not asserted: the bounds above are the project's, these say how far inside them the cells sit.
MEASURED = {
    ("rollout", "reach"): (4.8e-7, 7.2e-6, 7.2e-6, 3.3e-7, 2.3e-6),   ("rollout", "look-at"): (0.0, 4.8e-7, 0.0, 1.0e-6, 1.1e-6, 1.4e-7, 9.5e-7),
    ("rollout32", "reach"): (4.8e-7, 5.3e-6, 6.7e-6, 2.9e-7, 2.3e-6), ("rollout32", "look-at"): (0.0, 4.8e-7, 0.0, 1.0e-6, 1.1e-6, 1.4e-7, 9.5e-7),
    ("mw", "reach"): (4.8e-7, 7.2e-6, 7.6e-6, 3.3e-7, 2.6e-6),        ("mw", "look-at"): (0.0, 4.8e-7, 0.0, 1.0e-6, 1.1e-6, 1.4e-7, 9.5e-7),
    ("one_wave", "reach"): (4.8e-7, 7.2e-6, 7.6e-6, 3.3e-7, 2.6e-6),  ("one_wave", "look-at"): (0.0, 4.8e-7, 0.0, 1.0e-6, 1.1e-6, 1.4e-7, 9.5e-7),
}
# ... and from the rollout launcher's buffers, all 97 envs (obs incl. terminal and last, actions, rewards, values, log-probs, qpos, qvel):
# rollout32 is bit-identical for every kind; mw / one_wave, reach kinds: 5.2e-7, 6.0e-8, 1.0e-5, 3.6e-7, 0, 2.4e-7, 3.1e-6; look-at kinds:
# 0, 0, 9.5e-7, 0, 0, 2.4e-7, 1.1e-6 -- no pixel centre differed between two launchers in any cell


def _counter_rows(kind):
    """the integer state rows a launch hands over to the next one, by their names in the state matrix and in the oracle's Env struct: within
    15 steps Env04's lost counter shows in no observation, so it is compared itself"""
    return ("elapsed_steps", "rng_counter") + (("lost_count",) if kind in S.LOOKAT else ())


@functools.lru_cache(maxsize=None)
def _device_run(launcher, kind, flag_name):
    """The run of matrix_support on the device through one launcher; everything it produced, on the host.  Shared by the cell's own test
    and the across-launcher test; never written to."""
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    from so100_mujoco_rl_amd.collector import RolloutCollector
    flags = S.FLAG_SETS[flag_name]
    epw = {"rollout": 64, "rollout32": 32}.get(launcher, 0)
    with one_wave_step_kernel(launcher == "one_wave"):
        env = So100VecEnv(kind, S.N, flags=flags, seed=S.SEED, max_episode_steps=S.TIMELIMIT, solver_iters=S.SHIPPED[0],
                          contact_iters=S.SHIPPED[1], envs_per_workgroup=epw)
    sim = env.sim
    if epw:
        assert sim.envs_per_workgroup == epw
    od = sim.obs_dim
    col = RolloutCollector(env, S.policy_state(od, env.device), T=S.T1, persistent=launcher.startswith("rollout"), bootstrap_truncated=False)
    col.tobs = torch.zeros(S.T1, S.N, od, device=env.device)        # raw env rewards AND the terminal observations of the chunk
    env.reset_tensor(); col._started = True
    marked = torch.arange(S.N, device=env.device) % S.EVERY == 0
    if kind in S.LOOKAT:                                             # the base turned away from the cube (matrix_support.OracleEnvRun)
        q, v = sim.get_state()
        q = q.cpu().numpy().T.copy(); v = v.cpu().numpy().T.copy()
        q[::S.EVERY, 0] += np.float32(S.TURN)
        inject_state(sim, q, v)
        cmd0 = sim.get_field("cmd0"); cmd0[marked] += S.TURN; sim.set_field("cmd0", cmd0)
        if kind != 4:
            lost = sim.get_field("lost_count", dtype=torch.int32); lost[marked] = S.LOST0; sim.set_field("lost_count", lost)
    pads = bool(flags & S.PAD_FLAGS)
    chunks, tobs, lengths, cstat, counters = [], [], [], [], []
    for launch, steps in enumerate((S.T1, S.T2)):
        if launch == 1 and kind in S.BLOCK:                          # the stale cube onto the stale end effector
            for c in "xyz":
                cx = sim.get_field(f"cx_{c}"); cx[marked] = sim.get_field(f"ee_{c}")[marked]; sim.set_field(f"cx_{c}", cx)
        b = col.collect(steps)
        chunks.append({k: b[k].cpu().numpy().copy() for k in ("obs", "actions", "rewards", "dones", "truncated", "values", "log_probs", "last_obs")})
        tobs.append(col.tobs[:steps].cpu().numpy().copy()); lengths.append(sim.ep_length.cpu().numpy().copy())
        counters.append({k: sim.get_field(k, dtype=torch.int32).cpu().numpy().copy() for k in _counter_rows(kind)})
        if pads:
            cstat.append(sim.get_field("contact_stat", dtype=torch.int32).cpu().numpy().copy())
    q, v = sim.get_state()
    out = {k: np.concatenate([c[k] for c in chunks], 0) for k in chunks[0] if k != "last_obs"}
    out.update(last_obs=chunks[1]["last_obs"], tobs=np.concatenate(tobs, 0), lengths=lengths, cstat=cstat, counters=counters,
               qpos=q.cpu().numpy().T.copy(), qvel=v.cpu().numpy().T.copy())
    out["codes"] = np.where(out["dones"] == 0, 0, np.where(out["truncated"], 2, 1))
    env.close()
    return out


def _handover(g, launch, run):
    """what the device holds for env run.i after a launch beside its observation: ep_length and the counter rows, against the oracle's"""
    assert g["lengths"][launch][run.i] == run.last_length, (run.i, launch)
    for k, row in g["counters"][launch].items():
        assert row[run.i] == getattr(run.e.e, k), (run.i, launch, k, row[run.i], getattr(run.e.e, k))


def _ids(cell):
    return "-".join(str(x) for x in cell)


@pytest.mark.parametrize("launcher,kind,flag_name", S.CELLS, ids=[_ids(c) for c in S.CELLS])
def test_cell_vs_oracle(launcher, kind, flag_name):
    g = _device_run(launcher, kind, flag_name)
    flags = S.FLAG_SETS[flag_name]
    assert all(np.isfinite(g[k]).all() for k in ("obs", "actions", "rewards", "values", "log_probs", "last_obs", "qpos", "qvel"))
    assert g["dones"].sum() >= S.N
    for cs in g["cstat"]:
        assert (cs & 255).max() == 0                             # no pad contact on the device either
    act = np.clip(g["actions"], -1.0, 1.0)
    lookat = kind in S.LOOKAT
    w = dict(obs=0.0, px=0.0, rew=0.0, qpos=0.0, qvel=0.0); n_px = n_px_bad = 0

    def obs_err(got, want):
        nonlocal n_px, n_px_bad
        w["obs"] = max(w["obs"], np.abs(got[:6] - want[:6]).max())
        d = np.abs(got[6:] - want[6:])
        if lookat:
            w["px"] = max(w["px"], d.max()); n_px += d.size; n_px_bad += int((d > LOOK_PX_TIGHT).sum())
        else:
            w["obs"] = max(w["obs"], d.max())

    runs = []
    for i in S.SAMPLE:
        run = S.OracleEnvRun(kind, flags, i); runs.append(run)
        obs_err(g["obs"][0, i], run.obs0)
        for t in range(S.T):
            if t == S.T1:
                run.between_launches()
                _handover(g, 0, run)
            o, r, code, tobs = run.step(act[t, i])
            assert g["codes"][t, i] == code, (i, t, g["codes"][t, i], code)       # wherever dones is set it equals the oracle's, and nowhere else
            obs_err(g["obs"][t + 1, i] if t + 1 < S.T else g["last_obs"][i], o)
            if code:
                obs_err(g["tobs"][t, i], tobs)
            w["rew"] = max(w["rew"], abs(g["rewards"][t, i] - r))
        _handover(g, 1, run)
        qo, vo = run.state()
        w["qpos"] = max(w["qpos"], np.abs(g["qpos"][i] - qo).max()); w["qvel"] = max(w["qvel"], np.abs(g["qvel"][i] - vo).max())
    share = n_px_bad/max(n_px, 1)
    print(f"[matrix {launcher} kind {kind} {flag_name}] 16 envs x {S.T} steps vs oracle: obs {w['obs']:.2e} px {w['px']:.2e} px-share {share:.4f} "
          f"reward {w['rew']:.2e} qpos {w['qpos']:.2e} qvel {w['qvel']:.2e}")
    S.assert_events(kind, runs)
    if lookat:
        assert w["obs"] < LOOK_JOINT and w["px"] < LOOK_PX and share <= LOOK_PX_SHARE
        assert w["rew"] < LOOK_REW[kind] and w["qpos"] < LOOK_QPOS and w["qvel"] < LOOK_QVEL
    else:
        assert w["obs"] < REACH_OBS and w["rew"] < REACH_REW[kind]
        assert w["qpos"] < REACH_QPOS and w["qvel"] < REACH_QVEL


PAIRS = [(kind, name) for kind in S.KINDS for name in S.FLAG_SETS]


@pytest.mark.parametrize("kind,flag_name", PAIRS, ids=[_ids(p) for p in PAIRS])
def test_launchers_agree(kind, flag_name):
    """rollout, mw and one_wave (and rollout32 for FREE) are separate compilations of the same arithmetic on the same policy-noise stream:
    their buffers agree row by row, all 97 envs"""
    base = _device_run("rollout", kind, flag_name)
    lookat = kind in S.LOOKAT
    for other in [l for l, names in S.LAUNCHERS.items() if l != "rollout" and flag_name in names]:
        g = _device_run(other, kind, flag_name)
        assert np.array_equal(base["codes"], g["codes"]), other
        assert all(np.array_equal(a, b) for a, b in zip(base["lengths"], g["lengths"])), other
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(base["counters"], g["counters"]) for k in a), other
        d = {k: np.abs(base[k] - g[k]) for k in ("obs", "actions", "rewards", "values", "log_probs", "last_obs", "qpos", "qvel")}
        dt = np.abs(np.where(base["codes"][..., None] != 0, base["tobs"] - g["tobs"], 0.0))
        worst = {k: float(v.max()) for k, v in d.items()}; worst["tobs"] = float(dt.max())
        print(f"[matrix {other} vs rollout, kind {kind} {flag_name}] " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        if lookat:
            # a pixel centre is an integer: where two compilations round a projection to different pixels the entry moves by 5/1080, and
            # with it the reward of that step and the value of the next row
            assert max(d["obs"][..., :6].max(), d["last_obs"][..., :6].max(), dt[..., :6].max()) <= ACROSS, other
            assert max(d["obs"][..., 6:].max(), d["last_obs"][..., 6:].max(), dt[..., 6:].max()) < ACROSS_PX, other
            same = np.concatenate([d["obs"][1:, :, 6:].max(-1), d["last_obs"][None, :, 6:].max(-1)], 0) <= ACROSS      # [T, N]: pixel entries written by step t agree
            assert d["rewards"][same].max() <= ACROSS_REW and d["rewards"].max() < ACROSS_LOOK_REW, other
            same_row = (d["obs"][..., 6:].max(-1) <= ACROSS)
            for k in ("actions", "values", "log_probs"):
                assert d[k][same_row].max() <= ACROSS, (other, k)
            assert same.mean() > 0.99 and same_row.mean() > 0.99, other
        else:
            for k in ("obs", "actions", "values", "log_probs", "last_obs", "tobs"):
                assert worst[k] <= ACROSS, (other, k)
            assert worst["rewards"] <= ACROSS_REW, other
        assert worst["qpos"] <= ACROSS and worst["qvel"] <= 1e-5, other
