"""The kernel matrix's scenario (tests/test_gpu_kernel_matrix.py, tests/test_kernel_matrix_cpu.py): its cells, the run every cell shares,
the oracle's side of that run, and the source reader that keeps the cell list in step with KindOps<KIND>::step / ::rollout.

The run: N = 97 envs (one full workgroup and a partly filled one at 64 and at 32 envs per workgroup, and for the 64-thread one-wave grid),
seed 4 (scenes.UNINJECTED_SEED: the oracle's own Philox stream drives every reset and retarget, nothing is injected), TimeLimit 12, two
launches of 10 and 5 steps, solver settings SHIPPED.  The policy is SB3's default initialisation (seed 2) with log_std lowered to -1.5, so
the arms stay off the table and no finger pad touches anything: this run is about the seams between env kind, flag set and launcher, the
pad-contact physics has its own per-substep modules.  The branches that tell the kinds apart are set up through state fields, on the
device and in the oracle's Env struct alike, in every 4th env (0, 4, .. 96):

  kinds 3, 4, 5   before the first launch the base joint (q0 and its commanded angle cmd0) is turned TURN rad away from the cube; kinds
                  3 and 5 start LOST0 steps into the lost counter, so the episode ends TERMINATED (lost_count > 30) on step 5 of the first
                  launch; Env04 only re-uses its last centre (lost_count > 0) and never terminates within 15 steps
  kinds 2, 6      between the launches the stale cube position is put onto the stale end effector: the reach branch fires on step 11
                  (and, as all poses read zero after a reset, on the first step of every episode)
  all kinds       the TimeLimit truncates every other episode on step 12, inside the second launch

Nothing here needs a GPU; the device side of the run lives in the GPU module."""
import ctypes as C
import os
import re

import numpy as np

from oracle import so100_oracle as O
from scenes import ARM, C5, FREE, NOPADS, REFP, SHIPPED, UNINJECTED_SEED, UNINSTANTIATED      # noqa: F401  (SHIPPED: re-exported)

KINDS = (1, 2, 3, 4, 5, 6)
REACH, LOOKAT, BLOCK = (1, 2, 6), (3, 4, 5), (2, 6)
FLAG_SETS = {"FREE": FREE, "ARM": ARM, "NOPADS": NOPADS, "REFP": REFP, "C5": C5, "UNINSTANTIATED": UNINSTANTIATED}
PAD_FLAGS = O.F_PADS_FLOOR | O.F_PADS_CUBE
# launcher -> the flag sets it runs: so100_rollout_fused<K, 8, 4, 32> exists for the contact-disabled flags alone
LAUNCHERS = {"rollout": tuple(FLAG_SETS), "rollout32": ("FREE",), "mw": tuple(FLAG_SETS), "one_wave": tuple(FLAG_SETS)}
CELLS = [(launcher, kind, name) for launcher, names in LAUNCHERS.items() for kind in KINDS for name in names]

N, SEED, TIMELIMIT, T1, T2 = 97, UNINJECTED_SEED, 12, 10, 5
T = T1 + T2
LOG_STD, POLICY_SEED = -1.5, 2
EVERY, TURN, LOST0, LOST_LIMIT = 4, 2.0, 27, 30


def oracle_iters(flags):
    """The oracle's solver for a flag set: its primal Newton (-1) wherever a contact row can be active, its dual PGS run to a change below
    1e-15 (0) otherwise.  gpu_support.run_pair draws that line at the pad rows; here it is drawn at F_FLOOR as well, because of Env04: it
    sets its cube flat into the floor (z = 0.01, no rotation) after every reset and when the centre first comes within 0.1 of the frame's,
    and on that cube, pushed out on four equal corners, the oracle's two solvers do not agree with each other.  Measured over the steps of
    this run (NOPADS, Env04): the Newton solve keeps the cube's angular velocity below 1e-14 rad/s, as the symmetry demands; the dual PGS
    meets its stopping rule after 300-460 sweeps with 9.7e-2 rad/s about y on the first step, and the two states stay more than 1e-5 apart for
    nine steps.  While the cube rests (Env01/02/06, and Env04 before the event) the two agree to 4e-13, and the Newton solve is the same to the
    last bit with and without the pad rows -- so it is the reference wherever the floor is simulated."""
    return -1 if flags & (O.F_FLOOR | PAD_FLAGS) else 0


SAMPLE = tuple(int(i) for i in np.linspace(0, N - 1, 16).astype(int))       # env 0 and env 96 included


def marked(i):
    """the envs whose kind-specific branch is set up"""
    return i % EVERY == 0


def policy_state(obs_dim, device):
    """SB3-keyed state dict of the run's policy"""
    from so100_mujoco_rl_amd.collector import RolloutCollector
    sd = RolloutCollector.random_policy_state(obs_dim, device, seed=POLICY_SEED)
    sd["log_std"] = sd["log_std"] + LOG_STD
    return sd


def policy_mean64(obs_dim):
    """obs (float32 [obs_dim]) -> the policy's action mean in float64 on the host, from the float32 weights"""
    sd = {k: v.double().numpy() for k, v in policy_state(obs_dim, "cpu").items()}
    w0, b0 = sd["mlp_extractor.policy_net.0.weight"], sd["mlp_extractor.policy_net.0.bias"]
    w1, b1 = sd["mlp_extractor.policy_net.2.weight"], sd["mlp_extractor.policy_net.2.bias"]
    wm, bm = sd["action_net.weight"], sd["action_net.bias"]
    return lambda obs: wm @ np.tanh(w1 @ np.tanh(w0 @ obs.astype(np.float64) + b0) + b1) + bm


class OracleEnvRun:
    """Env i of the run in the fp64 oracle.  step() takes the action the env receives (already clamped) and returns what the device writes
    for that step: observation (the reset one where the episode ended), reward, done code (0 running, 1 terminated, 2 truncated only) and the
    terminal observation (None while running); the pad contacts and the lost counter it leaves are kept for the event assertions."""

    def __init__(self, kind, flags, i):
        self.kind, self.i = kind, i
        self.e = O.OracleEnv(kind, flags=flags, iters=oracle_iters(flags), seed=SEED, env_id=i)
        self.e.e.max_episode_steps = TIMELIMIT
        self.obs0 = self.e.reset()
        if kind in LOOKAT and marked(i):
            q0 = float(np.float32(O.arr(self.e.d.qpos)[0]) + np.float32(TURN))
            O.arr(self.e.d.qpos)[0] = q0; O.arr(self.e.e.cmd)[0] = q0
            if kind != 4:
                self.e.e.lost_count = LOST0
        self.pad_contacts = 0          # pad/floor and pad/cube records (kinds 1, 2 of the oracle's contact list) at the end of any step
        self.max_lost = 0
        self.last_length = 0           # length of the last finished episode (the device's ep_length row; 0 = none finished)
        self.codes, self.rewards, self.cube = [], [], []   # per step: done code, reward, cube position at the end of the step (before a reset)

    def between_launches(self):
        if self.kind in BLOCK and marked(self.i):
            d = self.e.d
            ee = np.zeros(3); O.lib().so100o_end_effector(d.xpos[6], d.xmat[6], ee.ctypes.data_as(C.c_void_p))
            O.arr(d.xpos)[8] = ee

    def step(self, act):
        e = self.e
        obs, r, term, trunc, _ = e.step(np.asarray(act, np.float32), autoreset=False)
        d = e.d
        self.pad_contacts += sum(1 for k in range(d.ncon) if d.con[k].kind in (1, 2))
        self.max_lost = max(self.max_lost, int(e.e.lost_count))
        code = 1 if term else 2 if trunc else 0
        self.cube.append(O.arr(d.qpos)[6:9].copy())
        tobs = None
        if code:
            self.last_length = int(e.e.episode_length)
            tobs, obs = obs, e.reset()         # what so100o_env_step does itself with autoreset = 1
        self.codes.append(code); self.rewards.append(r)
        return obs, r, code, tobs

    def state(self):
        return O.arr(self.e.d.qpos).copy(), O.arr(self.e.d.qvel).copy()


def oracle_alone(kind, flags, envs=range(N)):
    """The run with the oracle alone: actions clip(mean64(obs) + exp(LOG_STD) policy_noise_ref(SEED, env, step)), the policy step counter
    running on through resets and over both launches.  Returns the OracleEnvRun of every env."""
    mean = policy_mean64(O.lib().so100o_obs_dim(kind))
    sigma = np.exp(LOG_STD)
    runs = []
    for i in envs:
        run = OracleEnvRun(kind, flags, i)
        noise = O.policy_noise_ref(SEED, i, np.arange(T))
        obs = run.obs0
        for t in range(T):
            if t == T1:
                run.between_launches()
            obs = run.step(np.clip(mean(obs) + sigma*noise[t], -1.0, 1.0))[0]
        runs.append(run)
    return runs


def assert_events(kind, runs):
    """The oracle-side proof that the run reached each kind's branches; `runs`: OracleEnvRun of some or all envs after their 15 steps."""
    for r in runs:
        assert r.pad_contacts == 0, (kind, r.i, r.pad_contacts)          # contact-free: the condition the bounds rest on
    hit = [r for r in runs if marked(r.i)]
    rest = [r for r in runs if not marked(r.i)]
    assert hit and rest
    if kind in (3, 5):
        # turned away, LOST0 steps into the counter: terminated on step LOST_LIMIT + 2 - LOST0 of the first launch, not truncated
        for r in hit:
            assert r.codes[:T1].count(1) == 1 and r.codes.index(1) == LOST_LIMIT + 1 - LOST0 and 2 not in r.codes, (kind, r.i, r.codes)
            assert r.last_length == LOST_LIMIT + 2 - LOST0
    if kind == 4:
        for r in hit:
            assert r.max_lost > 0 and 1 not in r.codes, (kind, r.i, r.max_lost, r.codes)      # last centre re-used, never terminated
    if kind in BLOCK:
        # the reach branch on the step after the teleport.  Env06: the gripper sigmoid lifts every such reward above 5, as on the first step
        # of every episode.  Env02: the bonus is 20 |block_pos - last_block_pos| of two random draws, on a base reward near -4, so the reward
        # passes 1 in some envs only (as in test_gpu_parity.py::test_env02_vs_oracle_with_reach_branch, at least one must) -- but the branch
        # also re-draws the cube's position, which every marked env must show (the cube rests or is pinned otherwise) and no other env may
        if kind == 6:
            for r in hit:
                assert r.rewards[T1] > 5.0, (kind, r.i, r.rewards[T1])
            for r in runs:
                assert r.rewards[0] > 5.0 and r.rewards[TIMELIMIT] > 5.0, (kind, r.i)
        else:
            assert sum(r.rewards[T1] > 1.0 for r in hit) > 0
            for r in runs:
                jump = np.linalg.norm(r.cube[T1] - r.cube[T1 - 1])
                assert (jump > 0.01) == marked(r.i), (kind, r.i, jump)
    for r in rest if kind in (3, 5) else runs:
        assert r.codes == [0]*(TIMELIMIT - 1) + [2] + [0]*(T - TIMELIMIT), (kind, r.i, r.codes)  # the TimeLimit, inside the second launch


# ---- the dispatch table, read from the source ----------------------------------------------------------------------------------
_FLAG_BITS = {"SO100_F_FRICTIONLOSS": O.F_FRICTIONLOSS, "SO100_F_LIMITS": O.F_LIMITS, "SO100_F_FLOOR": O.F_FLOOR, "SO100_F_CUBE_PINNED": O.F_CUBE_PINNED,
              "SO100_F_PADS_FLOOR": O.F_PADS_FLOOR, "SO100_F_PADS_CUBE": O.F_PADS_CUBE, "SO100_F_LINKS_FLOOR": O.F_LINKS_FLOOR,
              "SO100_F_LINKS_CUBE": O.F_LINKS_CUBE, "SO100_F_NOPADS": NOPADS, "SO100_F_REFERENCE": O.F_REFERENCE, "SO100_F_CONTACT5": O.F_CONTACT5}


def dispatched_flag_sets(root):
    """{"step": set, "rollout": set} of the compile-time flag values (-1 = run-time flags) that KindOps<KIND>::step and ::rollout in
    csrc/so100_kernels.hpp instantiate kernels for: every argument of their SO100_STEP / SO100_STEP_ROWS / SO100_RL launch macros and every
    explicit <KIND, flags, ...> template argument list in the two bodies."""
    src = open(os.path.join(root, "so100_mujoco_rl_amd", "csrc", "so100_kernels.hpp")).read()
    out = {}
    for fn in ("step", "rollout"):
        m = re.search(r"KindOps<KIND>::%s\(.*?\n}\n" % fn, src, re.S)
        assert m, fn
        body = re.sub(r"#define(?:[^\n\\]|\\.)*", "", m.group(0), flags=re.S)    # the macro definitions name their parameter, not a flag set
        exprs = re.findall(r"SO100_(?:STEP|STEP_ROWS|RL)\(([^()]*)\)", body) + re.findall(r"<KIND,\s*([^,<>]+),", body)
        vals = set()
        for ex in exprs:
            val = 0
            for tok in ex.split("|"):
                tok = tok.strip()
                val |= _FLAG_BITS[tok] if tok in _FLAG_BITS else int(tok)      # an unknown name is a KeyError / ValueError: extend _FLAG_BITS
            vals.add(val)
        assert vals, fn
        out[fn] = vals
    return out
