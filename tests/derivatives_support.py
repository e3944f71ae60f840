"""Shared by tests/test_derivatives_cpu.py and tests/test_gpu_derivatives.py: the host twin of the derivatives query (tests/_derivcheck), the
cases of its checks, the fp64 oracle's answer for each and the bounds.

References.  Every reference is the ORACLE's centred secant at the same eps: so100o_step(..., -1, 1) chained nsub times per evaluation, in
fp64 from the fp32-rounded start, the controls float32 as the device sees them (in actions mode the target is the oracle's own perturbed q +
0.075f a), perturbed and differenced in fp64 by the rule of csrc/so100_derivative.hpp (one add; the cube's orientation through the quaternion
product, its rotation rows through mju_subQuat).  Neither the twin nor the kernel is ever its own reference.  Cases and references are
computed once per process and never modified."""
import ctypes as C
import functools

import numpy as np

import scenes
import trajectory_support as TS
from hostlibs import derivcheck, ptr
from oracle import so100_oracle as O

L, M = scenes.L, scenes.M
NX, NU, NCOL = 24, 6, 30
EPS = 2.0**-6                                              # SO100_DERIV_EPS
ITERS = (64, 64)                                           # the smooth families: every evaluation starts cold (trajectory_support.PARITY_ITERS)
NSUB = 16


def twin(ctrl, qpos, qvel=None, mode="targets", nsub=NSUB, flags=scenes.REFP, dtype=np.float32, solver_iters=2, contact_iters=20, eps=EPS, warm=None):
    """the host twin on problem-major arrays: ctrl [n, 6], qpos [n, 13], qvel [n, 12] or None, warm [n, 31] or None.  Returns the dict
    So100Sim.derivatives returns, as numpy arrays."""
    lib = derivcheck()
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    u, q, v, w = cast(ctrl), cast(qpos), cast(qvel), cast(warm)
    n = u.shape[0]
    assert u.shape == (n, 6) and q.shape == (n, 13)
    out = {"A": np.zeros((n, NX, NX), dtype), "B": np.zeros((n, NX, NU), dtype), "qpos_next": np.zeros((n, 13), dtype), "qvel_next": np.zeros((n, 12), dtype),
           "bad": np.zeros(n, np.int32)}
    fn = lib.dc_derivatives_d if dtype == np.float64 else lib.dc_derivatives_f
    fn(n, ptr(q), ptr(v), ptr(w), ptr(u), TS.MODES[mode], nsub, int(flags), solver_iters, contact_iters, float(eps),
       *[ptr(out[k]) for k in ("A", "B", "qpos_next", "qvel_next", "bad")])
    return out


# ---- the oracle's secant ------------------------------------------------------------------------------------------------------------------------
def quat_mul(a, b):
    return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                     a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]])


def perturbed(qpos, qvel, u, col, d):
    """column col of (x, u) moved by d (signed), in fp64: the rule of derivative_perturb"""
    qpos, qvel, u = qpos.copy(), qvel.copy(), u.copy()
    if col < 9:
        qpos[col] += d
    elif col < 12:
        r = np.zeros(4); r[0] = np.cos(0.5*abs(d)); r[1 + col - 9] = np.sign(d)*np.sin(0.5*abs(d))
        q = quat_mul(qpos[9:13], r)
        qpos[9:13] = q/np.linalg.norm(q)
    elif col < 24:
        qvel[col - 12] += d
    else:
        u[col - 24] += d
    return qpos, qvel, u


def tangent_difference(qp, vp, qm, vm, r):
    """(y+ - y-) r in the tangent space: the rule of derivative_column"""
    col = np.zeros(NX)
    col[:9] = (qp[:9] - qm[:9])*r
    col[12:] = (vp - vm)*r
    d = quat_mul(np.array([qm[9], -qm[10], -qm[11], -qm[12]]), qp[9:13])
    sn = np.linalg.norm(d[1:])
    angle = 2.0*np.arctan2(sn, d[0])
    if angle > np.pi:
        angle -= 2.0*np.pi
    col[9:12] = d[1:]*(angle/sn if sn >= 1e-15 else 0.0)*r
    return col


def oracle_next(qpos, qvel, u, mode, nsub, flags, check=None):
    """the oracle's control step from fp64 (qpos, qvel) under the controls u: (qpos', qvel').  check(d) is called before every substep."""
    d = scenes.fresh(); O.arr(d.qpos)[:] = qpos; O.arr(d.qvel)[:] = qvel
    O.arr(d.ctrl)[:] = qpos[:6] + TS.JS64*u if mode == "actions" else u
    for _ in range(nsub):
        if check is not None:
            check(d)
        L.so100o_step(C.byref(M), C.byref(d), int(flags), -1, 1)
    return O.arr(d.qpos).copy(), O.arr(d.qvel).copy()


def oracle_secant(q32, v32, u32, mode, nsub, flags, eps, check=None):
    """{"A" [n, 24, 24], "B" [n, 24, 6], "qpos_next", "qvel_next"} in fp64 from float32 starts and controls"""
    n = len(q32)
    A = np.zeros((n, NX, NX)); B = np.zeros((n, NX, NU)); qn = np.zeros((n, 13)); vn = np.zeros((n, 12))
    r = 0.5/eps
    for i in range(n):
        q, v, u = q32[i].astype(np.float64), v32[i].astype(np.float64), u32[i].astype(np.float64)
        qn[i], vn[i] = oracle_next(q, v, u, mode, nsub, flags, check)
        for col in range(NCOL):
            yp = oracle_next(*perturbed(q, v, u, col, eps), mode, nsub, flags)
            ym = oracle_next(*perturbed(q, v, u, col, -eps), mode, nsub, flags)
            c = tangent_difference(*yp, *ym, r)
            if col < NX:
                A[i, :, col] = c
            else:
                B[i, :, col - NX] = c
    return {"A": A, "B": B, "qpos_next": qn, "qvel_next": vn}


def _no_contact_at_all(d):
    """trajectory_support._no_arm_contact's forward pass with every contact flag on, asked for NO contact, the cube's with the floor included"""
    import substep_harness as H
    dd = H.copy_data(d)
    L.so100o_forward(C.byref(M), C.byref(dd), TS.ALL_CONTACTS, -1)
    assert dd.ncon == 0


# ---- A: the smooth families ---------------------------------------------------------------------------------------------------------------------
# one family per form of the kernel: <8>, <11>, <7> and the run-time-flags form
FAMILY_FLAGS = {"arm": scenes.FREE, "rows": scenes.ARM, "cube": scenes.NOPADS, "pads": scenes.REFP}
PINNED = ("arm", "rows")
AIRBORNE = ("cube", "pads")


@functools.lru_cache(maxsize=None)
def family(name, mode):
    """{"qpos" [65, 13], "qvel" [65, 12], "ctrl" [65, 6] float32, "flags"}.  arm: the starts and the first control row of
    trajectory_support.free_case("arm", mode), under F_CUBE_PINNED.  cube: the same arms under F_NOPADS with the cube 5 cm above the floor at a
    random orientation, linear velocity within 0.1 m/s and body angular velocity within 2 rad/s: in 16 substeps it falls under 6 mm and never
    touches (smooth_reference asserts it on the oracle).  rows: arm's starts with friction loss and joint limits on (the step is then only
    piecewise smooth; the reference is still the oracle's secant at the same eps).  pads: cube's starts under F_REFERENCE -- the finger pads
    are tested against the floor and meet nothing."""
    c = TS.free_case("arm", mode)
    qpos, qvel, ctrl = c["qpos"].copy(), c["qvel"].copy(), c["ctrl"][0].copy()
    if name in AIRBORNE:
        rs = np.random.RandomState(23)
        n = len(qpos)
        quat = rs.randn(n, 4); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
        qpos[:, 8] = 0.05; qpos[:, 9:13] = quat
        qvel[:, 6:9] = rs.uniform(-0.1, 0.1, (n, 3)); qvel[:, 9:12] = rs.uniform(-2.0, 2.0, (n, 3))
    return {"qpos": qpos.astype(np.float32), "qvel": qvel.astype(np.float32), "ctrl": ctrl.astype(np.float32), "flags": FAMILY_FLAGS[name]}


@functools.lru_cache(maxsize=None)
def smooth_reference(name, mode, eps=EPS, nsub=NSUB):
    """the oracle's secant for family(name, mode); on the cube family the unperturbed evaluation asserts ncon == 0 before every substep"""
    c = family(name, mode)
    return oracle_secant(c["qpos"], c["qvel"], c["ctrl"], mode, nsub, c["flags"], eps, _no_contact_at_all if name in AIRBORNE else None)


def deviation(got, ref):
    """largest |got - ref| over A and B, separately for the tangent rows 0..11 ("q") and 12..23 ("v"), and of the next state ("qpos", "qvel")"""
    dA = np.abs(np.asarray(got["A"], np.float64) - ref["A"]); dB = np.abs(np.asarray(got["B"], np.float64) - ref["B"])
    return {"q": float(max(dA[:, :12].max(), dB[:, :12].max())), "v": float(max(dA[:, 12:].max(), dB[:, 12:].max())),
            "qpos": float(np.abs(np.asarray(got["qpos_next"], np.float64) - ref["qpos_next"]).max()),
            "qvel": float(np.abs(np.asarray(got["qvel_next"], np.float64) - ref["qvel_next"]).max())}


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------------
# The fp32 twin's largest deviation from the oracle's secant at the same eps = SO100_DERIV_EPS, nsub 16, iterations (64, 64), both modes, measured
# by tests/test_derivatives_cpu.py (which prints them as [deriv-tol] lines and holds the twin to TWIN_FACTOR x these); the kernel is held to
# KERNEL_FACTOR x these: trajectory_support's rule.  "q": tangent rows 0..11, "v": rows 12..23 of (A | B); "qpos", "qvel": the unperturbed evaluation's
# next state (the tumbling cube's quaternion is what sets the cube families' "qpos").
FP32_MEASURED = {
    "arm":  {"q": 4.1e-6, "v": 4.6e-5, "qpos": 8.1e-8, "qvel": 1.2e-6},
    "rows": {"q": 4.2e-6, "v": 4.7e-5, "qpos": 7.6e-8, "qvel": 9.5e-7},
    "cube": {"q": 5.1e-5, "v": 4.7e-5, "qpos": 3.7e-7, "qvel": 9.5e-7},
    "pads": {"q": 5.1e-5, "v": 4.7e-5, "qpos": 3.7e-7, "qvel": 9.5e-7},
}
TWIN_FACTOR, KERNEL_FACTOR = TS.TWIN_FACTOR, TS.KERNEL_FACTOR


def fp64_bounds(eps):
    """(arm rows, cube rows) x (q, v): what trajectory_support takes from tests/test_hostcheck.py for a state, over 2 eps"""
    return {"arm": (TS.FP64_ARM[0]/(2*eps), TS.FP64_ARM[1]/(2*eps)), "cube": (TS.FP64_CUBE[0]/(2*eps), TS.FP64_CUBE[1]/(2*eps))}


ARM_ROWS = np.r_[0:6, 12:18]
CUBE_ROWS = np.r_[6:12, 18:24]


def cube_block_is_the_identity(got, bound):
    """F_CUBE_PINNED: the cube neither moves nor couples, so its block of A is I and the rest of its rows and columns 0, within the bound"""
    A = np.asarray(got["A"], np.float64)
    want = np.zeros((NX, NX)); want[CUBE_ROWS, CUBE_ROWS] = 1.0
    d = np.abs(A - want)
    cube = np.zeros((NX, NX), bool); cube[CUBE_ROWS] = True; cube[:, CUBE_ROWS] = True
    q = np.zeros((NX, NX), bool); q[:12] = True
    assert d[:, cube & q].max() <= bound["q"] and d[:, cube & ~q].max() <= bound["v"], d[:, cube].max()
    assert np.abs(np.asarray(got["B"], np.float64)[:, CUBE_ROWS]).max() == 0.0


# ---- B / C: the inputs of the exact properties -----------------------------------------------------------------------------------------------------
STRUCT_EPS = 2.0**-8
ROT = (9, 10, 11)                                          # the cube's rotation columns / rows: not one rounded add, not one rounded subtraction
PLAIN_COLS = [c for c in range(NCOL) if c not in ROT]
PLAIN_ROWS = [r for r in range(NX) if r not in ROT]


@functools.lru_cache(maxsize=None)
def contact_inputs(name):
    """(qpos [n, 13], qvel [n, 12], actions [n, 6], flags): "floor": 5 problems of scenes.floor_batch under REFP (pads on the floor), "grasp": 3 of
    scenes.grasp_batch under C5 (the jaw closing on the cube).  Shared: callers copy before they write."""
    if name == "floor":
        q, v, a = scenes.floor_batch(5, 2); flags = scenes.REFP
    else:
        q, v, a = scenes.grasp_batch(3, 1); flags = scenes.C5
    return q.astype(np.float32), v.astype(np.float32), a.astype(np.float32), flags


def perturbed_starts(q, v, u, eps):
    """the 2 x 27 perturbed copies of every problem for the columns that are one rounded add, in float32: (cols, qpos [2, 27, n, 13], qvel, ctrl)"""
    e = np.float32(eps)
    Q = np.broadcast_to(q, (2, len(PLAIN_COLS)) + q.shape).copy(); V = np.broadcast_to(v, (2, len(PLAIN_COLS)) + v.shape).copy()
    U = np.broadcast_to(u, (2, len(PLAIN_COLS)) + u.shape).copy()
    for j, c in enumerate(PLAIN_COLS):
        for s, d in enumerate((e, -e)):
            if c < 9:
                Q[s, j, :, c] = q[:, c] + d
            elif c < 24:
                V[s, j, :, c - 12] = v[:, c - 12] + d
            else:
                U[s, j, :, c - 24] = u[:, c - 24] + d
    return Q, V, U


def expected_plain(step, q, v, u, eps):
    """(A | B) [n, 21 plain rows, 27 plain columns] as (y+ - y-) / (2 eps) in float32 from `step(qpos [k, 13], qvel [k, 12], ctrl [k, 6]) -> (qpos' [k, 13],
    qvel' [k, 12])`, a T = 1 trajectory on the perturbed starts"""
    Q, V, U = perturbed_starts(q, v, u, eps)
    n = len(q)
    qn, vn = step(Q.reshape(-1, 13), V.reshape(-1, 12), U.reshape(-1, 6))
    y = np.concatenate([qn[:, :9], np.zeros((len(qn), 3), np.float32), vn], axis=1).reshape(2, len(PLAIN_COLS), n, NX)
    r = np.float32(0.5/eps)
    return np.transpose(((y[0] - y[1]).astype(np.float32)*r).astype(np.float32), (1, 2, 0))[:, PLAIN_ROWS]


def plain_block(res):
    """the same block of a derivatives result"""
    AB = np.concatenate([res["A"], res["B"]], axis=2)
    return AB[:, PLAIN_ROWS][:, :, PLAIN_COLS]
