"""Shared by tests/test_trajectory_cpu.py and tests/test_gpu_trajectory.py: the host twin of the trajectory query (tests/_trajcheck), the
cases of its checks, the fp64 oracle's answer for each and the bounds.

References.  Every reference is the ORACLE's: so100o_step(..., -1, 1) chained from the fp32-rounded start, the controls rounded as the device
sees them (float32 actions or targets; in actions mode the target is the oracle's own q at the start of the control step + 0.075f a).
Cases, references and masks are computed once per process and never modified."""
import ctypes as C
import functools

import numpy as np

import query_support as QS
import scenes
import substep_harness as H
from hostlibs import ptr, trajcheck
from oracle import so100_oracle as O

L, M = scenes.L, scenes.M
TARGETS, ACTIONS = 0, 1
MODES = {"targets": TARGETS, "actions": ACTIONS}
JS64 = float(scenes.JS)                                    # (double)0.075f: what the fp64 twin multiplies an action by


def twin(ctrl, qpos, qvel=None, mode="targets", nsub=16, flags=scenes.REFP, dtype=np.float32, solver_iters=2, contact_iters=20, warm=None):
    """the host twin on problem-major arrays: ctrl [T, n, 6], qpos [n, 13], qvel [n, 12] or None, warm [n, 31] or None (trajcheck.cpp).  Returns
    the dict So100Sim.trajectory returns, as numpy arrays, plus "qpos_final" and "qvel_final"."""
    lib = trajcheck()
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    u, q, v, w = cast(ctrl), cast(qpos), cast(qvel), cast(warm)
    T, n = u.shape[0], u.shape[1]
    assert u.shape == (T, n, 6) and q.shape == (n, 13)
    i32 = np.int32
    out = {"qpos": np.zeros((T, n, 13), dtype), "qvel": np.zeros((T, n, 12), dtype), "ee": np.zeros((T, n, 3), dtype),
           "qpos_final": np.zeros((n, 13), dtype), "qvel_final": np.zeros((n, 12), dtype), "ncon": np.zeros((T, n), i32), "dropped": np.zeros((T, n), i32),
           "sig": np.zeros((T, n), i32), "residual": np.zeros((T, n), dtype), "bad_step": np.zeros(n, i32)}
    fn = lib.tc_trajectory_d if dtype == np.float64 else lib.tc_trajectory_f
    fn(n, ptr(q), ptr(v), ptr(w), ptr(u), MODES[mode], T, nsub, int(flags), solver_iters, contact_iters,
       *[ptr(out[k]) for k in ("qpos", "qvel", "ee", "qpos_final", "qvel_final", "ncon", "dropped", "sig", "residual", "bad_step")])
    return out


# ---- A: the query as one substep of substep_harness.run_substep_parity --------------------------------------------------------------------------
PARITY_ITERS = (64, 64)        # every call starts cold; DESIGN.md section 12.3: the cold-started fp32 solve at 64 / 64 stays inside the per-substep bounds


class TwinSubstep:
    """device_substep of the harness: T = 1, nsub = 1, mode = actions, explicit states, on the fp32 twin"""
    def __init__(self, flags, iters=PARITY_ITERS):
        self.flags, self.iters = flags, iters

    def __call__(self, q32, v32, act):
        g = twin(act[None], q32, v32, "actions", 1, self.flags, np.float32, *self.iters)
        assert (g["dropped"] == 0).all() and (g["bad_step"] == -1).all()
        return g["qpos"][0].astype(np.float64), g["qvel"][0].astype(np.float64), g["ncon"][0], g["sig"][0], g["residual"][0]


# ---- B: contact-free trajectories ----------------------------------------------------------------------------------------------------------------
FREE_T, FREE_NSUB, FREE_M = 3, 16, 65
FREE_FLAGS = {"arm": scenes.ARM, "nopads": scenes.NOPADS}
ALL_CONTACTS = scenes.LCUBE | O.F_PADS_CUBE                # what "no arm contact" is asked of the oracle under


def oracle_ee(q):
    return QS.oracle_kinematics(np.ascontiguousarray(q, np.float64))["ee"]


@functools.lru_cache(maxsize=None)
def free_case(name, mode):
    """{"qpos" [M, 13], "qvel" [M, 12] float32 starts, "ctrl" [T, M, 6] float32, "ref": the oracle's qpos [T, M, 13], qvel [T, M, 12], ee [T, M, 3]}.
    Arms in the air around scenes.idle_batch's pose with random joint velocities, the cube at rest on the floor beside them; a pose is kept only
    where the oracle, asked with every contact flag on, finds no arm contact before any of the T x nsub substeps or after the last."""
    flags = FREE_FLAGS[name]
    rs = np.random.RandomState(11)
    base_q, base_v = scenes.idle_batch(1)
    qs, vs, us, refs = [], [], [], []
    while len(qs) < FREE_M:
        qpos = base_q[0].copy(); qvel = base_v[0].copy()
        qpos[:6] += rs.uniform(-0.3, 0.3, 6); qvel[:6] = rs.uniform(-0.5, 0.5, 6)
        q32, v32 = qpos.astype(np.float32), qvel.astype(np.float32)
        a = rs.uniform(-1, 1, (FREE_T, 6)).astype(np.float32)
        # targets mode: servo targets near the start, as float32
        u = a if mode == "actions" else (q32[None, :6] + np.float32(2.0)*scenes.JS*a).astype(np.float32)
        d = scenes.fresh(); O.arr(d.qpos)[:] = q32.astype(np.float64); O.arr(d.qvel)[:] = v32.astype(np.float64)
        rq, rv, clear = [], [], True
        for t in range(FREE_T):
            O.arr(d.ctrl)[:] = O.arr(d.qpos)[:6] + JS64*u[t].astype(np.float64) if mode == "actions" else u[t].astype(np.float64)
            for _ in range(FREE_NSUB):
                clear = clear and _no_arm_contact(d)
                L.so100o_step(C.byref(M), C.byref(d), flags, -1, 1)
            rq.append(O.arr(d.qpos).copy()); rv.append(O.arr(d.qvel).copy())
        if not (clear and _no_arm_contact(d)):
            continue
        qs.append(q32); vs.append(v32); us.append(u); refs.append((np.stack(rq), np.stack(rv)))
    ref_q = np.stack([r[0] for r in refs], axis=1); ref_v = np.stack([r[1] for r in refs], axis=1)
    return {"qpos": np.stack(qs), "qvel": np.stack(vs), "ctrl": np.stack(us, axis=1), "flags": flags,
            "ref": {"qpos": ref_q, "qvel": ref_v, "ee": oracle_ee(ref_q[..., :6].reshape(-1, 6)).reshape(FREE_T, FREE_M, 3)}}


def _no_arm_contact(d):
    dd = H.copy_data(d)
    L.so100o_forward(C.byref(M), C.byref(dd), ALL_CONTACTS, -1)
    return all(dd.con[i].kind == 0 for i in range(dd.ncon))


def deviation(got, ref, rows=None):
    """largest |got - ref| of "qpos" and "qvel" (over `rows`, a boolean problem mask, default all)"""
    rows = slice(None) if rows is None else rows
    return {k: float(np.abs(np.asarray(got[k], np.float64)[:, rows] - ref[k][:, rows]).max()) for k in ("qpos", "qvel")}


# ---- C: warm carry in contact ------------------------------------------------------------------------------------------------------------------------
WARM_T, WARM_NSUB, WARM_ITERS = 2, 4, (4, 30)


@functools.lru_cache(maxsize=None)
def warm_case():
    """scenes.floor_batch(48, 0) under REFP, T = 2, nsub = 4, mode = actions (the batch's action in both steps): the oracle's 8 free-running
    substeps from the fp32-rounded start.  "keep": the cases where the oracle alone shows the same (count, signature) in all 8 substeps and
    no knife-edge pose among them; "count", "sig": that set's."""
    qpos, qvel, act = scenes.floor_batch(48, 0)
    flags = scenes.REFP
    n = len(qpos)
    q32, v32 = qpos.astype(np.float32), qvel.astype(np.float32)
    ctrl = np.stack([act, act]).astype(np.float32)
    rs = np.random.RandomState(1)
    ref_q = np.zeros((WARM_T, n, 13)); ref_v = np.zeros((WARM_T, n, 12))
    keep = np.zeros(n, bool); count = np.zeros(n, np.int64); sig = np.zeros(n, np.int64); knife = np.zeros(n, bool); pads = np.zeros(n, bool)
    for i in range(n):
        d = scenes.fresh(); O.arr(d.qpos)[:] = q32[i].astype(np.float64); O.arr(d.qvel)[:] = v32[i].astype(np.float64)
        sets = []
        for t in range(WARM_T):
            O.arr(d.ctrl)[:] = O.arr(d.qpos)[:6] + JS64*ctrl[t, i].astype(np.float64)
            for _ in range(WARM_NSUB):
                d0 = H.copy_data(d)
                L.so100o_step(C.byref(M), C.byref(d), flags, -1, 1)
                s = H.oracle_contact_summary(d)
                sets.append(s[:2])
                knife[i] = knife[i] or (s[2] > 0 and H.knife_edge(d0, flags, s, rs))
            ref_q[t, i] = O.arr(d.qpos); ref_v[t, i] = O.arr(d.qvel)
        keep[i] = len(set(sets)) == 1 and not knife[i]
        count[i], sig[i] = sets[0]; pads[i] = sets[0][0] > 0
    return {"qpos": q32, "qvel": v32, "ctrl": ctrl, "flags": flags, "keep": keep, "in_contact": keep & pads, "knife": knife, "count": count, "sig": sig, "ref": {"qpos": ref_q, "qvel": ref_v}}


# ---- E: the inputs of the exact properties -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contact_inputs():
    """130 problems of scenes.floor_batch (pads on the floor, REFP) with T = 3 random actions each: qpos [130, 13], qvel [130, 12],
    actions [3, 130, 6], float32.  Shared: callers copy before they write."""
    qpos, qvel, act = scenes.floor_batch(130, 2)
    rs = np.random.RandomState(5)
    a = np.stack([act, rs.uniform(-1, 1, act.shape).astype(np.float32), rs.uniform(-1, 1, act.shape).astype(np.float32)])
    return qpos.astype(np.float32), qvel.astype(np.float32), a


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------------------------
# fp64 twin against the oracle: what tests/test_hostcheck.py holds the same templates to over its trajectories -- the arm's block PGS at 6
# sweeps and more 1e-13 / 1e-12 (test_block_pgs_reaches_the_oracle_optimum), the cube's Newton on the floor 1e-12 / 1e-10
# (test_cube_newton_reaches_the_oracle_optimum): (qpos, qvel)
FP64_ARM = (1e-13, 1e-12)
FP64_CUBE = (1e-12, 1e-10)
FP64_ITERS = (64, 64)
# The fp32 twin's largest deviation from the oracle, measured by tests/test_trajectory_cpu.py (which prints them as [traj-tol] lines and holds
# the twin to TWIN_FACTOR x these); the kernel is held to KERNEL_FACTOR x these (FMA contraction, the device reciprocal: DESIGN.md 11.3, 12.3).
# "arm" / "nopads": B, both modes, all three rows, at the shipped (2, 20); "warm": C's kept cases, both rows, at (4, 30).
FP32_MEASURED = {
    "arm":    {"qpos": 1.1e-7, "qvel": 1.4e-6},
    "nopads": {"qpos": 1.1e-7, "qvel": 1.4e-6},
    "warm":   {"qpos": 1.3e-7, "qvel": 8.0e-6},
}
TWIN_FACTOR = 1.05
KERNEL_FACTOR = 3.0
# ee: the bound tests/test_gpu_query.py holds kinematics()["ee"] to, widened by what the trajectory's own qpos bound moves the point by: each
# column of the point's Jacobian is no longer than the arm's reach, REACH, and there are six joints
REACH = 0.5


def ee_bound(qpos_bound):
    return QS.FP32_BOUNDS["ee"] + 6*REACH*qpos_bound
