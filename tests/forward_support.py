"""Shared by tests/test_forward_cpu.py and tests/test_gpu_forward.py: the states of the forward-dynamics query's checks (the recipe), the
fp64 oracle's answer for each (so100o_forward with its Newton run to convergence), the host twin (tests/_forwardcheck) and the comparison.

Recipe.  Every env follows the ORACLE's own trajectory (Newton solver, one substep at a time, qpos / qvel rounded to fp32 before every
substep, ctrl = fp32(q) + 0.075 act as in substep_harness); the state before substeps 0, 4, 8, ... is a case.  A case is a knife edge if
substep_harness.knife_edge / knife_edge_records says so under RandomState(1): both ask the oracle alone.  Reference, cases and knife-edge
classification are computed once per process and never modified."""
import ctypes as C
import functools

import numpy as np

import scenes
import substep_harness as H
from hostlibs import forwardcheck, ptr
from oracle import so100_oracle as O

L, M = scenes.L, scenes.M
MAXCON = 20
TIMESTEP = 0.002
# (name, batch, flags, substeps): DESIGN.md section 12
RECIPE = (("floor", lambda: scenes.floor_batch(48, 0), scenes.REFP, 24),
          ("grasp", lambda: scenes.grasp_batch(32, 0), scenes.C5, 24),
          ("floor_cube", lambda: scenes.floor_cube_batch(32, 0), scenes.C5, 24),
          ("link_cube", lambda: scenes.link_cube_batch(16, 0), scenes.LCUBE, 12),
          ("wrist_first", lambda: scenes.wrist_first_batch(16, 0), scenes.LINKS, 12))
EVERY = 4
QUANTITIES = ("con_pos", "con_frame", "con_dist", "con_force", "pad_force", "qacc", "qfrc_constraint")
FORCE_QUANTITIES = ("con_force", "pad_force")          # a problem's error is divided by 1 N + the sum of its oracle normal forces
NEWTON_TOL = {np.float64: 1e-10, np.float32: 1e-3}    # a residual is 0 (converged) or the last step's size: below primal_newton's `small` test


def decode(f):
    """mju_decodePyramid, mu = 1: four edge forces -> (normal, t1, t2)"""
    return np.array([f[0] + f[1] + f[2] + f[3], f[0] - f[1], f[2] - f[3]])


def oracle_forward(qpos, qvel, ctrl, flags):
    """the reference of one case: so100o_forward(..., -1) on the (widened fp32) state"""
    d = scenes.fresh()
    O.arr(d.qpos)[:] = qpos; O.arr(d.qvel)[:] = qvel; O.arr(d.ctrl)[:] = ctrl
    L.so100o_forward(C.byref(M), C.byref(d), flags, -1)
    n = d.ncon
    assert n <= MAXCON
    ref = {"ncon": n, "dropped": d.ncon_dropped, "qacc": O.arr(d.qacc).copy(), "qfrc_constraint": O.arr(d.qfrc_constraint).copy(),
           "feat": np.array([d.con[i].feat for i in range(n)], np.int64), "kind": np.array([d.con[i].kind for i in range(n)], np.int64),
           "pos": np.array([d.con[i].pos[:] for i in range(n)]).reshape(n, 3), "frame": np.array([d.con[i].frame[:] for i in range(n)]).reshape(n, 9),
           "dist": np.array([d.con[i].dist for i in range(n)]),
           "force": np.array([decode(O.arr(d.efc_force)[d.con[i].efc0:d.con[i].efc0 + 4]) for i in range(n)]).reshape(n, 3)}
    pf = np.zeros(8)
    for i in range(n):
        if d.con[i].kind in (1, 2):
            pf[d.con[i].geom] += ref["force"][i, 0]
    ref["pad_force"] = pf
    # the oracle's own consistency: qfrc_constraint = J' efc_force
    J = O.arr(d.efc_J)[:d.nefc]; f = O.arr(d.efc_force)[:d.nefc]
    ref["jtf_gap"] = float(np.abs(J.T @ f - ref["qfrc_constraint"]).max()) if d.nefc else 0.0
    return ref


class Family:
    """one batch family's cases: qpos [n, 13], qvel [n, 12], ctrl [n, 6] (float32), the oracle's answers and the knife-edge mask"""
    def __init__(self, name, batch, flags, nsub):
        self.name, self.flags = name, flags
        qpos, qvel, act = batch()
        ds = H.oracle_states(qpos, qvel)
        rs, rs_free = np.random.RandomState(1), np.random.RandomState(1)
        qs, vs, us, refs, knife = [], [], [], [], []
        for s in range(nsub):
            for i, d in enumerate(ds):
                H.round_state_to_fp32(d)
                q32 = O.arr(d.qpos).astype(np.float32); v32 = O.arr(d.qvel).astype(np.float32)
                u32 = (q32[:6] + act[i].astype(np.float32)*scenes.JS).astype(np.float32)
                if s % EVERY == 0:
                    O.arr(d.ctrl)[:] = u32.astype(np.float64)
                    d0 = H.copy_data(d)
                    ref = oracle_forward(q32.astype(np.float64), v32.astype(np.float64), u32.astype(np.float64), flags)
                    dd = H.copy_data(d0); L.so100o_forward(C.byref(M), C.byref(dd), flags, -1)
                    summary = H.oracle_contact_summary(dd)
                    ke = (summary[2] > 0 and H.knife_edge(d0, flags, summary, rs)) or \
                         (summary[2] == 0 and dd.ncon > 0 and H.knife_edge_records(d0, flags, dd.ncon, rs_free))
                    qs.append(q32); vs.append(v32); us.append(u32); refs.append(ref); knife.append(bool(ke))
                H.oracle_substep(d, act[i], flags)
        self.qpos, self.qvel, self.ctrl = np.stack(qs), np.stack(vs), np.stack(us)
        self.refs, self.knife = refs, np.array(knife)

    def __len__(self):
        return len(self.refs)


@functools.lru_cache(maxsize=None)
def family(name):
    for n, batch, flags, nsub in RECIPE:
        if n == name:
            return Family(n, batch, flags, nsub)
    raise KeyError(name)


def families():
    return [family(r[0]) for r in RECIPE]


def twin(qpos, qvel, ctrl, flags, dtype, solver_iters=64, contact_iters=64):
    """the host twin on problem-major arrays; qvel / ctrl may be None.  Returns the dict So100Sim.forward returns, as numpy arrays."""
    lib = forwardcheck()
    n = len(qpos)
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    q, v, u = cast(qpos), cast(qvel), cast(ctrl)
    out = {"qacc": np.zeros((n, 12), dtype), "qfrc_constraint": np.zeros((n, 12), dtype), "ncon": np.zeros(n, np.int32), "dropped": np.zeros(n, np.int32),
           "pad_force": np.zeros((n, 8), dtype), "residual": np.zeros(n, dtype)}
    con = {"kind": np.zeros((n, MAXCON), np.int32), "feat": np.zeros((n, MAXCON), np.int32), "pos": np.zeros((n, MAXCON, 3), dtype),
           "frame": np.zeros((n, MAXCON, 3, 3), dtype), "dist": np.zeros((n, MAXCON), dtype), "force": np.zeros((n, MAXCON, 3), dtype)}
    fn = lib.fc_forward_d if dtype == np.float64 else lib.fc_forward_f
    fn(n, ptr(q), ptr(v), ptr(u), int(flags), solver_iters, contact_iters, ptr(out["qacc"]), ptr(out["qfrc_constraint"]), ptr(out["ncon"]),
       ptr(out["dropped"]), ptr(con["kind"]), ptr(con["feat"]), ptr(con["pos"]), ptr(con["frame"]), ptr(con["dist"]), ptr(con["force"]),
       ptr(out["pad_force"]), ptr(out["residual"]))
    out["contacts"] = con
    return out


def check_case(got, i, ref):
    """the exact checks of one non-knife-edge case and its deviations from the oracle: {quantity: error}, the two force quantities divided
    by 1 N + the sum of the oracle's normal forces.  got: a forward() result (numpy), i: the problem's row."""
    con = got["contacts"]
    n = int(got["ncon"][i])
    assert n == ref["ncon"], ("ncon", i, n, ref["ncon"])
    feat = con["feat"][i]
    assert sorted(feat[:n].tolist()) == sorted(ref["feat"].tolist()), ("feat", i, feat[:n], ref["feat"])
    assert int(got["dropped"][i]) == ref["dropped"], ("dropped", i)
    assert (feat[n:] == -1).all() and not con["kind"][i, n:].any() and not con["pos"][i, n:].any() and not con["frame"][i, n:].any() \
        and not con["dist"][i, n:].any() and not con["force"][i, n:].any(), ("empty slots", i)
    order = [int(np.nonzero(feat[:n] == f)[0][0]) for f in ref["feat"]]          # the oracle's record k is our slot order[k]
    assert (con["kind"][i, order] == ref["kind"]).all(), ("kind", i)
    # pad_force = the sum of its records' normal forces (the device's own list)
    pf = np.zeros(8)
    for s in range(n):
        if con["kind"][i, s] in (1, 2):
            pf[(feat[s] & 63) >> 3] += float(con["force"][i, s, 0])
    scale = 1.0 + ref["force"][:, 0].sum()
    assert np.abs(pf - got["pad_force"][i]).max() <= 1e-5*scale, ("pad_force vs own records", i)
    err = {"qacc": np.abs(got["qacc"][i] - ref["qacc"]).max(), "qfrc_constraint": np.abs(got["qfrc_constraint"][i] - ref["qfrc_constraint"]).max(),
           "pad_force": np.abs(got["pad_force"][i] - ref["pad_force"]).max()/scale,
           "con_pos": 0.0, "con_frame": 0.0, "con_dist": 0.0, "con_force": 0.0}
    if n:
        err["con_pos"] = np.abs(con["pos"][i, order] - ref["pos"]).max()
        err["con_frame"] = np.abs(con["frame"][i, order].reshape(n, 9) - ref["frame"]).max()
        err["con_dist"] = np.abs(con["dist"][i, order] - ref["dist"]).max()
        err["con_force"] = np.abs(con["force"][i, order] - ref["force"]).max()/scale
    return {k: float(v) for k, v in err.items()}


CUBE_MASS = float(M.body_mass[8])
GRAVITY = -float(M.gravity[2])
MARGIN = 0.0           # detection margin: every listed contact touches or penetrates


def check_physical(got, i, force_bound, dtype):
    """checks that need no oracle: Newton's second law for the cube, force signs, distances, the residual"""
    con = got["contacts"]
    n = int(got["ncon"][i])
    total = np.zeros(3)
    for s in range(n):
        k = int(con["kind"][i, s])
        if k in (0, 2, 4):                                   # the force acts on geom2; cube/floor: the floor pushes the cube (geom1 = floor)
            total += con["frame"][i, s].astype(np.float64).T @ con["force"][i, s].astype(np.float64)
    lhs = CUBE_MASS*(got["qacc"][i, 6:9].astype(np.float64) + np.array([0.0, 0.0, GRAVITY]))
    scale = 1.0 + con["force"][i, :n, 0].astype(np.float64).sum()
    assert np.abs(lhs - total).max() <= force_bound*scale, ("newton", i, lhs, total)
    assert (con["force"][i, :n, 0] >= 0).all() and (con["dist"][i, :n] <= MARGIN).all(), ("signs", i)
    assert got["residual"][i] == 0 or got["residual"][i] < NEWTON_TOL[dtype]*(1 + np.abs(got["qacc"][i]).max()), ("residual", i, got["residual"][i])


def measure(got, fam, rows=None):
    """exact checks on every non-knife-edge case of a family (rows: the cases `got` holds, default all); returns the largest deviation per quantity"""
    rows = range(len(fam)) if rows is None else rows
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for j, c in enumerate(rows):
        if fam.knife[c]:
            continue
        for k, e in check_case(got, j, fam.refs[c]).items():
            worst[k] = max(worst[k], e)
    return worst


# The fp32 twin's largest deviation from the oracle per batch family and quantity, measured by tests/test_forward_cpu.py (which prints
# them as [forward-tol] lines and holds the twin to TWIN_FACTOR x these); the kernels are held to 3 x these (FMA contraction, the device reciprocal).
FP32_MEASURED = {
    "floor":       {"con_pos": 1.1e-7, "con_frame": 0.0,    "con_dist": 4.5e-8, "con_force": 4.5e-3, "pad_force": 4.5e-3, "qacc": 2.0e-3, "qfrc_constraint": 2.1e-4},
    "grasp":       {"con_pos": 6.2e-7, "con_frame": 3.4e-7, "con_dist": 2.5e-8, "con_force": 1.1e-4, "pad_force": 1.1e-4, "qacc": 1.1e-1, "qfrc_constraint": 8.8e-4},
    "floor_cube":  {"con_pos": 1.3e-7, "con_frame": 3.2e-7, "con_dist": 5.6e-8, "con_force": 2.8e-4, "pad_force": 2.8e-4, "qacc": 3.8e-2, "qfrc_constraint": 7.9e-5},
    "link_cube":   {"con_pos": 2.0e-8, "con_frame": 3.8e-7, "con_dist": 1.2e-8, "con_force": 1.9e-7, "pad_force": 0.0,    "qacc": 1.9e-3, "qfrc_constraint": 3.2e-6},
    "wrist_first": {"con_pos": 3.8e-8, "con_frame": 0.0,    "con_dist": 2.5e-8, "con_force": 3.7e-5, "pad_force": 0.0,    "qacc": 5.4e-4, "qfrc_constraint": 5.7e-5},
}
KERNEL_FACTOR = 3.0
FP32_BOUNDS = {f: {k: KERNEL_FACTOR*v for k, v in row.items()} for f, row in FP32_MEASURED.items()}
# Two fp64 solvers on one strictly convex problem: every quantity, and rows 0..8 of qacc, to 1e-9.  The cube's angular rows (qacc 9..11,
# rad/s^2) have a bound of their own: both solvers stop on the size of their last step and measure the cube's angular acceleration at the
# cube's corner (x CUBE_HALF = 0.01 m); the twin's stop tolerance there is 1e-11 (1 + 0.01 |x|max) m/s^2 = 2.5e-11 at the 145 rad/s^2 these
# states reach, i.e. 2.5e-9 rad/s^2 per solver, and the cube's inertia is 5e-7 kg m^2 with angular accelerations up to 4e3 rad/s^2: 1e-8.
# Measured: 7.2e-11 on rows 0..8, 2.1e-9 rad/s^2 on rows 9..11.
FP64_BOUND = 1e-9
FP64_BOUND_CUBE_ANGULAR = 1e-8
CUBE_HALF = 0.01
# the fp32 twin itself is held to its recorded figures (rounded up when recorded; 5 % for another compiler's or libm's last bits)
TWIN_FACTOR = 1.05
# the project's per-substep bounds on h * qacc for the same solver on the same kinds of state (substep_harness.check_tally / check_moving_cube)
HQACC_FREE, HQACC_PAD = 2e-6, 5e-5


def qacc_errors(got, fam):
    """(largest |qacc - oracle's| on rows 0..8, on the cube's angular rows 9..11) over the non-knife-edge cases"""
    ref = np.stack([r["qacc"] for r in fam.refs])
    e = np.abs(got["qacc"].astype(np.float64) - ref)[~fam.knife]
    return float(e[:, :9].max()), float(e[:, 9:].max())


def hqacc_errors(got, fam):
    """(largest |h qacc - oracle's| without pad or proxy contact, with it): arm and cube translation rows, and the cube's angular rows at its corner"""
    ref = np.stack([r["qacc"] for r in fam.refs])
    e = (TIMESTEP*np.abs(got["qacc"].astype(np.float64) - ref)*np.array([1.0]*9 + [CUBE_HALF]*3)).max(axis=1)
    pad = np.array([bool((r["kind"] != 0).any()) for r in fam.refs])
    keep = ~fam.knife
    return float(e[keep & ~pad].max()) if (keep & ~pad).any() else 0.0, float(e[keep & pad].max()) if (keep & pad).any() else 0.0
