"""The pad-contact kernels at 16, 32 and 64 envs per workgroup against the fp64 oracle, on the contact-rich run of
tests/contact_matrix_support.py: the sibling of tests/test_gpu_kernel_matrix.py, whose run is contact-free by construction.

choose_envs_per_workgroup (csrc/so100_sim.hip) gives the contact flag sets 16 envs per workgroup up to 4096 envs, 32 up to 8192 and 64 above;
the contact wave then works with 4, 2 or 1 lanes per env, the contact records [MAXC][CF][64] share their LDS pool with the policy phase's
activation images, and the lane-slot map (csrc/so100_balance.hpp) is dealt per workgroup of that size.  Every other test that puts a pad on
something inside the persistent kernel runs it at 16.  Here, pinned:

  rollout16/32/64   RolloutCollector(persistent=True)                          so100_rollout_fused<K, 23 | 55 | -1, 4>
  mw16/32/64        persistent=False: so100_policy_forward + so100_step        so100_step_mw<K, 23 | 55 | -1>
  one_wave          the same, handle created under one_wave_step_kernel()      so100_step_fused<K, 23 | 55 | -1>

x kinds 1..6 x REFP (23), C5 (55; the look-at kinds reach <K, -1>) and C5 | PROXIES (the run-time-flags build with every pair live): 126
cells.  Each replays the 16 envs of contact_matrix_support.SAMPLE in the oracle (its primal Newton) with the actions its buffer recorded,
clamped as the env applies them.  Done codes, ep_length and the elapsed_steps / rng_counter / lost_count rows must be equal; every (env, step)
row is classified as tests/test_gpu_default_physics.py does (tight < 2e-5, event < 2e-2: a corner that makes or breaks contact a substep
apart in fp32 and fp64; rewards / 20, pixel entries / 5, terminal observations included): no fail, median tight, and at most
max(3 x TWIN_EVENTS[kind, flag set], 15/480 of the rows) rows outside the tight class -- TWIN_EVENTS is what the fp32 host twin leaves
outside it on the CPU (tests/test_contact_matrix_cpu.py), 15 of 480 the allowance of test_default_rollout_kernel_vs_stepwise_and_oracle.
"parity unpinned (physics)": the oracle restates MuJoCo's algorithm; MuJoCo is not available.

Across lane groupings, for one (kind, flag set), every launcher is compared with rollout16 over all 200 envs: equal done codes, every row
within 2e-2, and 99 % of the rows within 1e-5 (Env02 under C5: 98.5 %, test_gpu_default_physics.TIGHT_SHARE) -- the contact solve's
summation order depends on the lanes per env, so the groupings agree to round-off until a contact event lands a substep apart.

Bit-exact, no tolerance (include/so100_sim.h: a pinned envs_per_workgroup gives bit-identical results whatever N and whichever lane holds
the env): envs [0, n) of a 256-env handle against an n-env handle through the rollout kernel, and two 100-env shards against one 200-env
handle, at each of 16, 32, 64.  The same promise through so100_step is tests/test_gpu_contacts.py::test_tail_workgroups_with_pad_contacts,
SO100_BALANCE=1 against 0 is tests/test_gpu_default_physics.py::test_workgroup_balancing_leaves_every_result_bit_identical; both run at
16, 32 and 64.

Worst figures measured on MI355X per (launcher family, kind family) stand in MEASURED below."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import contact_matrix_support as S                        # noqa: E402
from gpu_support import inject_state, one_wave_step_kernel  # noqa: E402

ALLOWANCE = 15/480                                         # rows outside the tight class: test_gpu_default_physics.py's 15 of 480
# A cell that needs more than its cap, with the measurement and its reason.  (Env02 | Env06, REFP) at 16 and 32 envs per workgroup, rollout and
# mw alike: 9 rows, env 53 on steps 3..11 (until the TimeLimit reset), worst 5.7e-4 -- one pad corner that leaves the table a substep
# apart in fp32 and fp64.  It is the event the fp32 host twin has on the CPU for Env01 from the same start (TWIN_EVENTS[1, REFP] = 9: env
# 53, steps 3..11, worst 5.7e-4), where the device has none: the reach kinds share starts and physics, and which compilation's round-off
# lands on the other side of that substep is not a property of the kind.  At 64 envs per workgroup and in the one-wave kernel the same
# cells have 0.  Bound: Env01's, 3 x 9.
EVENT_CAP = {(2, "REFP"): 27, (6, "REFP"): 27}
TOUCHED_SHARE = 0.2
ACROSS_LOOSE, ACROSS_TIGHT = 2e-2, 1e-5
ACROSS_SHARE = {(2, "C5"): 0.985}                          # test_gpu_default_physics.TIGHT_SHARE; every other pair 0.99

# Worst over the cells of a (launcher family, kind family), measured on MI355X: (most rows of 240 outside the tight class, largest median
# row error, smallest share of the 200 envs with a pad / link contact in step 10, most contact records of an env in a substep of that step).
# Not asserted: the bounds above say what must hold, these say how far inside them the cells sit.  No row was in the fail class, no parked env
# touched anything.  Every row outside the tight class belongs to one of five envs (53, 119, 145, 185, 199: one event each, then its wake
# until the TimeLimit reset), e.g. env 53 on steps 3..11 in (Env01, REFP) at 32 and 64 envs per workgroup and in (Env02 | Env06, REFP) at 16 and 32.
MEASURED = {
    ("rollout", "reach"): (9, 2.4e-7, 0.225, 5),  ("rollout", "look-at"): (1, 0.0, 0.365, 12),
    ("mw", "reach"): (9, 2.4e-7, 0.225, 5),       ("mw", "look-at"): (2, 0.0, 0.365, 12),
    ("one_wave", "reach"): (0, 2.4e-7, 0.225, 5), ("one_wave", "look-at"): (7, 0.0, 0.365, 12),
}
# ... and against rollout16, all 200 envs x 16 rows: smallest share of rows within 1e-5 and worst row, over the 18 (kind, flag set) pairs:
# rollout32 0.9975 / 4.6e-3, rollout64 0.9934 / 4.6e-3, mw16 0.9941 / 4.6e-3, mw32 0.9941 / 1.4e-3, mw64 0.9934 / 4.6e-3, one_wave 0.9903 /
# 4.6e-3 (31 of 3200 rows: Env02 | Env06 under REFP; 4.6e-3 = 5/1080 is one pixel of a look-at kind's centre)


def _epw(launcher):
    return 0 if launcher == "one_wave" else int(launcher[-2:])


def _start(env, col, kind, qpos, qvel):
    """reset, then the injected state; the look-at kinds' commanded angles and Env02's stale cube position with it (contact_matrix_support)"""
    sim = env.sim
    env.reset_tensor()
    inject_state(sim, qpos, qvel)
    if kind in S.LOOKAT:
        for i in range(6):
            sim.set_field(f"cmd{i}", torch.from_numpy(np.ascontiguousarray(qpos[:, i])).cuda())
    if kind in S.STALE_CUBE:
        for i, c in enumerate("xyz"):
            sim.set_field(f"cx_{c}", torch.from_numpy(np.ascontiguousarray(qpos[:, 6 + i])).cuda())
    col._started = True


def _collector(kind, flags, n, epw, persistent, env_id_offset=0, one_wave=False):
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    from so100_mujoco_rl_amd.collector import RolloutCollector
    with one_wave_step_kernel(one_wave):
        env = So100VecEnv(kind, n, flags=flags, seed=S.SEED, max_episode_steps=S.TIMELIMIT, solver_iters=S.SHIPPED[0],
                          contact_iters=S.SHIPPED[1], envs_per_workgroup=epw, env_id_offset=env_id_offset)
    if epw:
        assert env.sim.envs_per_workgroup == epw
    col = RolloutCollector(env, S.policy_state(env.sim.obs_dim, env.device, flags), T=S.T1, persistent=persistent, bootstrap_truncated=False)
    col.tobs = torch.zeros(S.T1, n, env.sim.obs_dim, device=env.device)      # raw env rewards AND the terminal observations of the chunk
    return env, col


KEYS = ("obs", "actions", "rewards", "dones", "truncated", "values", "log_probs", "last_obs")


def _launches(env, col, kind, launches):
    """the launches of a started collector; everything they produced, on the host"""
    sim = env.sim
    chunks, tobs, lengths, cstat, counters = [], [], [], [], []
    names = ("elapsed_steps", "rng_counter") + (("lost_count",) if kind in S.LOOKAT else ())
    for steps in launches:
        b = col.collect(steps)
        chunks.append({k: b[k].cpu().numpy().copy() for k in KEYS})
        tobs.append(col.tobs[:steps].cpu().numpy().copy()); lengths.append(sim.ep_length.cpu().numpy().copy())
        counters.append({k: sim.get_field(k, dtype=torch.int32).cpu().numpy().copy() for k in names})
        cstat.append(sim.get_field("contact_stat", dtype=torch.int32).cpu().numpy().copy())
    q, v = sim.get_state()
    out = {k: np.concatenate([c[k] for c in chunks], 0) for k in KEYS if k != "last_obs"}
    out.update(last_obs=chunks[-1]["last_obs"], tobs=np.concatenate(tobs, 0), lengths=lengths, cstat=cstat, counters=counters,
               qpos=q.cpu().numpy().T.copy(), qvel=v.cpu().numpy().T.copy())
    out["codes"] = np.where(out["dones"] == 0, 0, np.where(out["truncated"], 2, 1))
    return out


@functools.lru_cache(maxsize=None)
def _device_run(launcher, kind, flag_name):
    """The run of contact_matrix_support on the device through one launcher.  Shared by the cell's own test and the grouping test; never
    written to."""
    flags = S.FLAG_SETS[flag_name]
    env, col = _collector(kind, flags, S.N, _epw(launcher), launcher.startswith("rollout"), one_wave=launcher == "one_wave")
    _start(env, col, kind, *S.starts(flags))
    out = _launches(env, col, kind, (S.T1, S.T2))
    env.close()
    return out


def _ids(cell):
    return "-".join(str(x) for x in cell)


@pytest.mark.parametrize("launcher,kind,flag_name", S.CELLS, ids=[_ids(c) for c in S.CELLS])
def test_cell_vs_oracle(launcher, kind, flag_name):
    g = _device_run(launcher, kind, flag_name)
    flags = S.FLAG_SETS[flag_name]
    assert all(np.isfinite(g[k]).all() for k in ("obs", "actions", "rewards", "values", "log_probs", "last_obs", "qpos", "qvel"))
    act = np.clip(g["actions"], -1.0, 1.0)
    errs, dq, events = [], 0.0, {}
    for i in S.SAMPLE:
        run = S.OracleContactRun(kind, flags, i)
        assert np.abs(g["obs"][0, i] - run.obs0).max() < 1e-6, i                  # the reset observation: the injection does not refresh it
        for t in range(S.T):
            if t == S.T1:
                _handover(g, 0, run)
            o, r, code, tobs = run.step(act[t, i])
            assert g["codes"][t, i] == code, (i, t, g["codes"][t, i], code)       # wherever dones is set it equals the oracle's, and nowhere else
            got = g["obs"][t + 1, i] if t + 1 < S.T else g["last_obs"][i]
            errs.append(S.row_error(kind, got, o, g["rewards"][t, i], r, g["tobs"][t, i] if code else None, tobs))
            if errs[-1] >= S.TIGHT:
                events.setdefault(i, []).append(t)
        _handover(g, 1, run)
        dq = max(dq, np.abs(g["qpos"][i, :6] - run.state()[0][:6]).max())
    classes = S.classify(errs)
    cs = g["cstat"][0]                                                            # after the first launch: before the TimeLimit sends every arm back to its start pose
    touched = float(((cs & 255) > 0).mean())
    cap = max(3*S.TWIN_EVENTS[kind, flag_name], ALLOWANCE*len(errs), EVENT_CAP.get((kind, flag_name), 0))
    print(f"[contact matrix {launcher} kind {kind} {flag_name}] {len(S.SAMPLE)} envs x {S.T} steps vs oracle: {classes} (cap {cap:.1f}), median {np.median(errs):.2e}, "
          f"worst {max(errs):.2e}; final arm |dq| {dq:.2e}; envs with a contact in step {S.T1} {touched:.3f}, parked {float(((cs[::S.PARK_EVERY] & 255) > 0).mean()):.3f}, most records {int((cs & 255).max())}; rows outside tight by env {events}")
    assert len(errs) == len(S.SAMPLE)*S.T
    assert classes["fail"] == 0 and dq < S.EVENT
    assert len(errs) - classes["tight"] <= cap
    assert np.median(errs) < S.TIGHT
    assert touched > TOUCHED_SHARE
    assert max(int((c >> 8).max()) for c in g["cstat"]) == 0                      # nothing over the contact budget, in either launch


def _handover(g, launch, run):
    """what the device holds for env run.i after a launch beside its observation: ep_length and the counter rows, against the oracle's"""
    assert g["lengths"][launch][run.i] == run.last_length, (run.i, launch)
    for k, row in g["counters"][launch].items():
        assert row[run.i] == getattr(run.e.e, k), (run.i, launch, k, row[run.i], getattr(run.e.e, k))


PAIRS = [(kind, name) for kind in S.KINDS for name in S.FLAG_SETS]


@pytest.mark.parametrize("kind,flag_name", PAIRS, ids=[_ids(p) for p in PAIRS])
def test_lane_groupings_agree(kind, flag_name):
    """rollout32, rollout64, mw16/32/64 and one_wave against rollout16, all 200 envs: the policy noise stream is shared, so rows can be
    compared one by one"""
    base = _device_run("rollout16", kind, flag_name)
    for other in S.LAUNCHERS[1:]:
        g = _device_run(other, kind, flag_name)
        assert np.array_equal(base["codes"], g["codes"]), other
        assert all(np.array_equal(a, b) for a, b in zip(base["lengths"], g["lengths"])), other
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(base["counters"], g["counters"]) for k in a), other
        d = np.concatenate([np.abs(base["obs"] - g["obs"]).max(-1).ravel(), np.abs(base["last_obs"] - g["last_obs"]).max(-1).ravel()])
        tight = float((d < ACROSS_TIGHT).mean())
        print(f"[contact matrix {other} vs rollout16, kind {kind} {flag_name}] rows within 1e-5: {tight:.4f} ({int((d >= ACROSS_TIGHT).sum())} of {d.size} outside), worst {d.max():.2e}; "
              f"rewards worst {np.abs(base['rewards'] - g['rewards']).max():.2e}; final |dqpos| {np.abs(base['qpos'] - g['qpos']).max():.2e}")
        assert d.max() < ACROSS_LOOSE, other
        assert tight >= ACROSS_SHARE.get((kind, flag_name), 0.99), (other, tight)


# ---- bit-exact promises of a pinned envs_per_workgroup -----------------------------------------------------------------------------
BIT_KEYS = ("obs", "actions", "rewards", "dones", "truncated", "values", "log_probs", "tobs")


def _rollout_chunks(flags, n, epw, rows, env_id_offset=0):
    """kind 1 through the persistent kernel (balancing on) from the matrix's starts `rows`, two launches of 6 steps: the TimeLimit reset is
    the last step of the second"""
    env, col = _collector(1, flags, n, epw, True, env_id_offset=env_id_offset)
    assert env.sim.envs_per_workgroup == epw
    qpos, qvel = S.starts(flags)
    _start(env, col, 1, qpos[rows], qvel[rows])
    out = _launches(env, col, 1, (6, 6))
    env.close()
    return out


def _assert_same_bits(whole, part, sl, what):
    for k in BIT_KEYS:
        assert np.array_equal(whole[k][:, sl], part[k]), (what, k)
    for k in ("last_obs", "qpos", "qvel"):
        assert np.array_equal(whole[k][sl], part[k]), (what, k)
    for a, b in zip(whole["cstat"] + whole["lengths"], part["cstat"] + part["lengths"]):
        assert np.array_equal(a[sl], b), (what, "contact_stat / ep_length")
    for a, b in zip(whole["counters"], part["counters"]):
        assert all(np.array_equal(a[k][sl], b[k]) for k in a), (what, "counters")


@functools.lru_cache(maxsize=None)
def _rollout_256(flags, epw):
    return _rollout_chunks(flags, 256, epw, np.arange(256) % S.N)


@pytest.mark.parametrize("n_of", ["1", "epw+1", "130"])
@pytest.mark.parametrize("flag_name", ["REFP", "C5"])
@pytest.mark.parametrize("epw", [16, 32, 64])
def test_rollout_kernel_is_batch_size_invariant(epw, flag_name, n_of):
    """envs [0, n) of a 256-env handle against an n-env handle, both pinned to `epw`, through so100_rollout with the workgroup balancing
    on (the two handles deal different slot maps): every buffer row, last_obs, qpos, qvel, contact_stat, ep_length and the counter rows
    are equal to the bit"""
    flags = S.FLAG_SETS[flag_name]
    n = {"1": 1, "epw+1": epw + 1, "130": 130}[n_of]
    big = _rollout_256(flags, epw)
    small = _rollout_chunks(flags, n, epw, np.arange(n))
    _assert_same_bits(big, small, slice(0, n), (epw, flag_name, n))
    if n > 1:                                                # (env 0 is parked: alone it touches nothing)
        assert max(int((c & 255).max()) for c in small["cstat"]) >= 2
    assert max(int((c & 255).max()) for c in big["cstat"]) >= 2 and np.isfinite(big["obs"]).all()


@pytest.mark.parametrize("flag_name", ["REFP", "C5"])
@pytest.mark.parametrize("epw", [16, 32, 64])
def test_rollout_kernel_is_shard_invariant(epw, flag_name):
    """two 100-env handles at env_id_offset 0 / 100 against one 200-env handle, pinned `epw`, rollout kernel: equal to the bit"""
    flags = S.FLAG_SETS[flag_name]
    whole = _rollout_chunks(flags, S.N, epw, np.arange(S.N))
    half = S.N//2
    for off in (0, half):
        part = _rollout_chunks(flags, half, epw, np.arange(off, off + half), env_id_offset=off)
        _assert_same_bits(whole, part, slice(off, off + half), (epw, flag_name, off))
    assert ((whole["cstat"][0] & 255) > 0).mean() > TOUCHED_SHARE and np.isfinite(whole["obs"]).all()
