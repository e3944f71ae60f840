"""The contact matrix's scenario (tests/test_gpu_contact_matrix.py, tests/test_contact_matrix_cpu.py): the sibling of tests/matrix_support.py
whose arms are ON the table.  Its cells, the injected starts, the policy, the oracle's side of the run and the fp32 host twin's.

The run: N = 200 envs (4 workgroups at 64 envs per workgroup, 7 at 32, 13 at 16, the last one holding 8 envs each time), solver settings
SHIPPED, seed 4, TimeLimit 12, two launches of 10 and 5 steps: the auto-reset falls inside the second launch, and the persistent kernel
deals the second launch's lane-slot map (csrc/so100_balance.hpp) from the contact loads the first one left.

Starts (starts(flags); fixed seeds, the generators of tests/scenes.py as tests/test_gpu_default_physics.py::_contact_rich_state uses them):
floor_batch arms with a finger pad within 2 mm of the table; under F_PADS_CUBE the envs from GRASP_FROM on are grasp_batch jaws closing on a
floating cube; under the proxy flags the envs of WRIST are wrist_first_batch arms (a link capsule reaches the table first) and those of
LINK_CUBE link_cube_batch arms (the cube 0.2-3 mm inside a link capsule).  Every 4th env (0, 4, ..) is parked: folded up 28 cm above the
table at rest, its cube lying on the floor -- contact and contact-free lanes then share every wave, and the slot map differs from the identity.
The look-at kinds servo to their commanded angles, so their cmd rows are set to the injected ones.  Env02 re-draws its cube whenever the
STALE cube position is within 3 cm of the stale end effector, which is so on the first step of every episode (all stale poses read zero after
a reset): its stale cube position (the cx rows, the oracle's xpos[8]) is therefore set to the injected cube's, as a forward pass after the
injection would leave it, and the grasped cube is still between the jaws when the first step ends.  The branch then fires on the second
step -- a cube between the jaws IS within 3 cm of the end effector -- so Env02 holds a pad/cube record for one step; that is Env02, not the
scenario.  After the TimeLimit reset the branch fires as it always does.

Policy: SB3's default initialisation (seed 2), action_net.bias[1] = SHOULDER_BIAS (shoulder down: the pads stay on / are pressed into the table),
bias[5] = -0.5 under F_PADS_CUBE (the jaw closes), log_std raised by 0.3.  The first action is computed from the reset observation (the
injection does not refresh it), on the device and here alike.

Nothing here needs a GPU; the device side of the run lives in the GPU module."""
import ctypes as C
import functools

import numpy as np

from hostlibs import hostcheck, ptr
from matrix_support import dispatched_flag_sets                # noqa: F401  (re-exported: the CPU module holds the cell list to it)
from oracle import so100_oracle as O
from scenes import C5, PROXIES, REFP, SHIPPED, floor_batch, grasp_batch, link_cube_batch, wrist_first_batch      # noqa: F401  (SHIPPED: re-exported)

KINDS = (1, 2, 3, 4, 5, 6)
REACH, LOOKAT = (1, 2, 6), (3, 4, 5)
STALE_CUBE = (2,)                                              # kinds whose stale cube position is set with the injected state (see above)
FLAG_SETS = {"REFP": REFP, "C5": C5, "C5_PROXIES": C5 | PROXIES}
ROLLOUTS, STEPWISE = ("rollout16", "rollout32", "rollout64"), ("mw16", "mw32", "mw64")
LAUNCHERS = ROLLOUTS + STEPWISE + ("one_wave",)
CELLS = [(launcher, kind, name) for launcher in LAUNCHERS for kind in KINDS for name in FLAG_SETS]

N, SEED, TIMELIMIT, T1, T2 = 200, 4, 12, 10, 5
T = T1 + T2
POLICY_SEED, LOG_STD, SHOULDER_BIAS, JAW_BIAS = 2, 0.3, 0.5, -0.5
PARK_EVERY = 4
PARKED_POSE = (0.0, -1.9, 1.6, 0.3, 1.5708, 0.1)             # scenes.grasp_state's arm: gripper horizontal, 28 cm above the table
RESTING_CUBE = (0.15, -0.25, 0.0099, 1.0, 0.0, 0.0, 0.0)
FLOOR_SEED, GRASP_SEED, WRIST_SEED, LINK_SEED = 31, 32, 33, 34      # of the four start families (chosen: tests/test_contact_matrix_cpu.py holds the conditions)
GRASP_FROM = 140                                               # F_PADS_CUBE: envs [GRASP_FROM, N) start as closing-jaw grasps
WRIST, LINK_CUBE = range(80, 110), range(110, 140)             # proxy flags: wrist-first arms, cubes against a link capsule
# The contact budget (16 pad / link records per env; the device's count adds the cube's <= 4 floor records) must hold with a manifold to
# spare in EVERY env and kind, in the oracle and in the fp32 host twin (tests/test_contact_matrix_cpu.py: at most BUDGET_MARGIN records in any
# substep, nothing dropped).  The look-at kinds move their cube by hand, now and then into an arm or a closed jaw; a start that ends so in any
# kind is replaced in its slot (the slot keys the env's draws): a floor_batch start by a spare of the generator (FLOOR_SWAP: slot -> index
# into its pool), a grasp by the slot's floor_batch start (FLOOR_NOT_GRASP: the cube's path through the jaws is the slot's, not the start's).
BUDGET_MARGIN = 12
FLOOR_POOL = N + 8
FLOOR_SWAP = {58: 200}
FLOOR_NOT_GRASP = (162, 166, 170, 178, 186, 194, 197, 198)     # slots from GRASP_FROM on that keep their floor_batch start

SAMPLE = tuple(int(i) for i in np.linspace(0, N - 1, 16).astype(int))     # env 0 and env 199; 39 and 53 sit at columns >= 32 of a full 64-env workgroup
TIGHT, EVENT = 2e-5, 2e-2
REWARD_SCALE, PIXEL_SCALE = 20.0, 5.0                          # a reward spans ~20 observation units; look-at observations carry 5 x (pixel centre)

# Rows (env, step) of the sample, 16 x 15 = 240 per cell, that the fp32 HOST TWIN (tests/_hostcheck: the device's own headers compiled for
# the CPU, one env at a time, no lanes, no LDS) leaves outside the tight class against the fp64 oracle on the oracle's own actions, with 0
# rows in the fail class: contact events that fp32 and fp64 see a substep apart.  tests/test_contact_matrix_cpu.py measures them and holds
# this table to the measurement; the GPU module caps a cell's count at 3 x its entry, or at the default-physics test's allowance where that
# is larger (its EVENT_CAP names the two pairs that need more, with the measurement).
TWIN_EVENTS = {(1, "REFP"): 9, (2, "REFP"): 0, (3, "REFP"): 0, (4, "REFP"): 0, (5, "REFP"): 0, (6, "REFP"): 0,
               (1, "C5"): 3, (2, "C5"): 0, (3, "C5"): 2, (4, "C5"): 1, (5, "C5"): 0, (6, "C5"): 0,
               (1, "C5_PROXIES"): 3, (2, "C5_PROXIES"): 0, (3, "C5_PROXIES"): 0, (4, "C5_PROXIES"): 1, (5, "C5_PROXIES"): 0, (6, "C5_PROXIES"): 0}


def parked(i):
    return i % PARK_EVERY == 0


@functools.lru_cache(maxsize=None)
def _floor_starts():
    """floor_batch's first N starts, the slots of FLOOR_SWAP filled from the spares behind them"""
    qpos, qvel, _ = floor_batch(FLOOR_POOL, FLOOR_SEED)
    for slot, k in FLOOR_SWAP.items():
        qpos[slot] = qpos[k]; qvel[slot] = qvel[k]
    return qpos[:N], qvel[:N]


@functools.lru_cache(maxsize=None)
def starts(flags):
    """(qpos [N, 13], qvel [N, 12]) float32 of the run under `flags`; shared by every kind and launcher, never written to"""
    qpos, qvel = (a.copy() for a in _floor_starts())
    if flags & O.F_PADS_CUBE:
        gq, gv, _ = grasp_batch(N - GRASP_FROM, GRASP_SEED)
        for slot in range(GRASP_FROM, N):
            if slot not in FLOOR_NOT_GRASP:
                qpos[slot] = gq[slot - GRASP_FROM]; qvel[slot] = gv[slot - GRASP_FROM]
    if flags & O.F_LINKS_FLOOR:
        wq, wv, _ = wrist_first_batch(len(WRIST), WRIST_SEED)
        qpos[WRIST.start:WRIST.stop] = wq; qvel[WRIST.start:WRIST.stop] = wv
    if flags & O.F_LINKS_CUBE:
        lq, lv, _ = link_cube_batch(len(LINK_CUBE), LINK_SEED)
        qpos[LINK_CUBE.start:LINK_CUBE.stop] = lq; qvel[LINK_CUBE.start:LINK_CUBE.stop] = lv
    qpos[::PARK_EVERY, :6] = PARKED_POSE; qpos[::PARK_EVERY, 6:] = RESTING_CUBE; qvel[::PARK_EVERY] = 0.0
    qpos = qpos.astype(np.float32); qvel = qvel.astype(np.float32)
    qpos.setflags(write=False); qvel.setflags(write=False)
    return qpos, qvel


def policy_state(obs_dim, device, flags):
    """SB3-keyed state dict of the run's policy"""
    from so100_mujoco_rl_amd.collector import RolloutCollector
    sd = RolloutCollector.random_policy_state(obs_dim, device, seed=POLICY_SEED)
    sd["action_net.bias"][1] = SHOULDER_BIAS
    if flags & O.F_PADS_CUBE:
        sd["action_net.bias"][5] = JAW_BIAS
    sd["log_std"] = sd["log_std"] + LOG_STD
    return sd


def policy_mean64(obs_dim, flags):
    """obs (float32 [obs_dim]) -> the policy's action mean in float64 on the host, from the float32 weights"""
    sd = {k: v.double().numpy() for k, v in policy_state(obs_dim, "cpu", flags).items()}
    w0, b0 = sd["mlp_extractor.policy_net.0.weight"], sd["mlp_extractor.policy_net.0.bias"]
    w1, b1 = sd["mlp_extractor.policy_net.2.weight"], sd["mlp_extractor.policy_net.2.bias"]
    wm, bm = sd["action_net.weight"], sd["action_net.bias"]
    return lambda obs: wm @ np.tanh(w1 @ np.tanh(w0 @ obs.astype(np.float64) + b0) + b1) + bm


class OracleContactRun:
    """Env i of the run in the fp64 oracle (its primal Newton, iters = -1).  step() takes the action the env receives (already clamped) and
    returns what the device writes for that step: observation (the reset one where the episode ended), reward, done code (0 running, 1
    terminated, 2 truncated only) and the terminal observation (None while running).  Kept per step for the scenario's proofs: the pad and
    link records (oracle contact kinds 1-4) and the pad/cube records (kind 2) at the end of the step, before a reset; the records dropped over
    the budget; the done code."""

    def __init__(self, kind, flags, i):
        self.kind, self.i = kind, i
        qpos, qvel = starts(flags)
        self.e = O.OracleEnv(kind, flags=flags, iters=-1, seed=SEED, env_id=i)
        self.e.e.max_episode_steps = TIMELIMIT
        self.obs0 = self.e.reset()
        O.arr(self.e.d.qpos)[:] = qpos[i].astype(np.float64); O.arr(self.e.d.qvel)[:] = qvel[i].astype(np.float64)
        if kind in LOOKAT:
            O.arr(self.e.e.cmd)[:] = qpos[i, :6].astype(np.float64)
        if kind in STALE_CUBE:
            O.arr(self.e.d.xpos)[8] = qpos[i, 6:9].astype(np.float64)
        self.records, self.pad_cube, self.codes = [], [], []
        self.dropped = 0
        self.last_length = 0           # length of the last finished episode (the device's ep_length row; 0 = none finished)

    def step(self, act):
        e = self.e
        obs, r, term, trunc, _ = e.step(np.asarray(act, np.float32), autoreset=False)
        d = e.d
        kinds = [d.con[k].kind for k in range(d.ncon)]
        self.records.append(sum(1 for k in kinds if k in (1, 2, 3, 4))); self.pad_cube.append(kinds.count(2))
        self.dropped += int(d.ncon_dropped)
        code = 1 if term else 2 if trunc else 0
        tobs = None
        if code:
            self.last_length = int(e.e.episode_length)
            tobs, obs = obs, e.reset()         # what so100o_env_step does itself with autoreset = 1
        self.codes.append(code)
        return obs, r, code, tobs

    def state(self):
        return O.arr(self.e.d.qpos).copy(), O.arr(self.e.d.qvel).copy()


def row_error(kind, got_obs, want_obs, got_rew, want_rew, got_tobs=None, want_tobs=None):
    """one (env, step) row against the oracle's, in observation units: joint entries as they are, the look-at kinds' pixel entries / 5,
    the reward / 20 -- tests/test_gpu_default_physics.py's measure -- and, where the episode ended, the terminal observation as well"""
    scale = PIXEL_SCALE if kind in LOOKAT else 1.0
    err = max(np.abs(got_obs[:6] - want_obs[:6]).max(), np.abs(got_obs[6:] - want_obs[6:]).max()/scale, abs(got_rew - want_rew)/REWARD_SCALE)
    if want_tobs is not None:
        err = max(err, np.abs(got_tobs[:6] - want_tobs[:6]).max(), np.abs(got_tobs[6:] - want_tobs[6:]).max()/scale)
    return float(err)


def classify(errs):
    """{"tight": n, "event": n, "fail": n} of a list of row errors"""
    errs = np.asarray(errs)
    return {"tight": int((errs < TIGHT).sum()), "event": int(((errs >= TIGHT) & (errs < EVENT)).sum()), "fail": int((errs >= EVENT).sum())}


def oracle_alone(kind, flags, envs=SAMPLE):
    """The run with the oracle alone: actions clip(mean64(obs) + exp(LOG_STD) policy_noise_ref(SEED, env, step)), the policy step counter
    running on through resets and over both launches.  Returns [(OracleContactRun, actions [T, 6] float32, rows)] per env, rows[t] = what
    step t returned."""
    mean = policy_mean64(O.lib().so100o_obs_dim(kind), flags)
    sigma = np.exp(LOG_STD)
    out = []
    for i in envs:
        run = OracleContactRun(kind, flags, i)
        noise = O.policy_noise_ref(SEED, i, np.arange(T))
        obs = run.obs0; acts = np.zeros((T, 6), np.float32); rows = []
        for t in range(T):
            acts[t] = np.clip(mean(obs) + sigma*noise[t], -1.0, 1.0)
            rows.append(run.step(acts[t]))
            obs = rows[-1][0]
        out.append((run, acts, rows))
    return out


def twin_rows(kind, flags, i, acts):
    """Env i of the run in the fp32 host twin (hc_env_step at the SHIPPED settings) on the actions `acts`: (reset observation, rows as
    oracle_alone returns them, most contact records in any substep, records dropped over the budget -- the two halves of the device's
    contact_stat row, over the whole run)"""
    H = hostcheck()
    od = O.lib().so100o_obs_dim(kind)
    qpos, qvel = starts(flags)
    h = H.hc_env_new(kind)
    try:
        obs0 = np.zeros(od, np.float32)
        H.hc_env_reset(h, kind, SEED, i, None, ptr(obs0))
        q = qpos[i].astype(np.float64); v = qvel[i].astype(np.float64)
        H.hc_env_set_state(h, ptr(q), ptr(v), ptr(q[:6].copy()) if kind in LOOKAT else None, ptr(q[6:9].copy()) if kind in STALE_CUBE else None)
        rows, most, dropped, st = [], 0, 0, np.zeros(2)
        for t in range(len(acts)):
            a = np.ascontiguousarray(acts[t], np.float32)
            obs = np.zeros(od, np.float32); tobs = np.zeros(od, np.float32); r = C.c_float(); done = C.c_int(); trunc = C.c_int()
            H.hc_env_step(h, kind, flags, SHIPPED[0], SHIPPED[1], TIMELIMIT, SEED, i, ptr(a), None, ptr(obs), ptr(tobs), C.byref(r), C.byref(done), C.byref(trunc))
            code = 0 if not done.value else 2 if trunc.value else 1
            rows.append((obs, r.value, code, tobs if code else None))
            H.hc_env_stats(h, ptr(st))
            most = max(most, int(st[0]) & 255); dropped += int(st[0]) >> 8
    finally:
        H.hc_env_free(h)
    return obs0, rows, most, dropped


def assert_coverage(kind, flags, runs):
    """The oracle-side proof that the run is about contacts; `runs`: the OracleContactRun of every sampled env after its 15 steps"""
    live = [r for r in runs if not parked(r.i)]
    rest = [r for r in runs if parked(r.i)]
    assert len(runs) == len(SAMPLE) and live and rest
    in_contact = [r.i for r in live if sum(1 for c in r.records[:T1] if c) >= 3]
    assert 4*len(in_contact) >= len(live), (kind, flags, in_contact)
    for r in rest:
        assert not any(r.records[:TIMELIMIT]), (kind, flags, r.i, r.records)       # parked: nothing touches before the reset
    if flags & O.F_PADS_CUBE:
        assert any(any(r.pad_cube[:T1]) for r in live), (kind, flags)
    for r in runs:
        assert r.dropped == 0, (kind, flags, r.i, r.dropped)
        assert r.codes == [0]*(TIMELIMIT - 1) + [2] + [0]*(T - TIMELIMIT), (kind, flags, r.i, r.codes)
    return len(in_contact), len(live)
