"""What the model-query tests share (test_query_cpu.py, test_gpu_query.py): the host twin of csrc/so100_query.hpp
(tests/_querycheck/libquerycheck.so, loaded by hostlibs.querycheck()), the fp64 oracle's side of every comparison, the cases and the bounds.

Cases.  CASES poses with q uniform over the full joint ranges, v uniform in +-2 rad/s, qacc uniform in +-20 rad/s^2, seed 0; every
input is rounded to fp32 once and the oracle gets those values widened, so a difference is the code's, not the inputs'.  IK: ik_recipe().

Bounds.  FP64_BOUND: the fp64 twin and the oracle are two fp64 formulations of the same quantities; the project's figure for that on the
physics is 1e-15, the bound 1e-12.  FP32_BOUNDS: per quantity, 3 x the largest difference between the fp32 twin and the oracle over
the cases (the margin the contact tests use; it covers FMA contraction and the device's reciprocal), measured on the CPU and printed
as [query-tol] lines by test_query_cpu.py::test_fp32_twin_against_the_oracle, which also holds the twin to them; the GPU tests hold
the kernels to the same numbers."""
import ctypes as C
import functools

import numpy as np

import hostlibs
from hostlibs import ptr
from oracle import so100_oracle as O

CASES = 512
FP64_BOUND = 1e-12
# the measured maxima of the fp32 twin against the oracle over the CASES poses (metres; xmat / cam_mat / jacr entries; kg m^2; N m)
FP32_MEASURED = {"xpos": 6.6e-8, "xmat": 2.3e-7, "ee": 7.8e-8, "cam_pos": 8.5e-8, "cam_mat": 2.2e-7, "jacp": 1.2e-7, "jacr": 2.0e-7,
                 "M": 1.1e-8, "bias": 2.7e-7, "tau": 5.9e-7}
FP32_BOUNDS = {k: 3.0 * v for k, v in FP32_MEASURED.items()}
IK_DEFAULTS = dict(iters=64, damping=0.02, tol=1e-4, max_step=0.3)
IK_Q_MEASURED = 1.2e-6                 # largest |q fp32 twin - q fp64 twin| over the converged cases of ik_recipe() (rad)
IK_Q_BOUND = 3.0 * IK_Q_MEASURED     # what the kernel's q may differ from the fp32 twin's by
IK_TOL_BAND = 1e-6                   # cases whose fp64 residual at the deciding check lies this close to tol are left out of the flag comparison
EE_LINK, EE_LOCAL = 4, np.array([0.0, float(np.float32(-0.1)), 0.0])


def joint_range():
    out = np.zeros(12)
    hostlibs.querycheck().qc_joint_range(ptr(out))
    return out.reshape(6, 2)


# ---- the host twin ------------------------------------------------------------------------------------------------------------------------------
def _as(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _suffix(dtype):
    return "d" if np.dtype(dtype) == np.float64 else "f"


def twin_kinematics(q, dtype):
    q = _as(q, dtype); n = len(q)
    o = {"xpos": np.zeros((n, 6, 3), dtype), "xmat": np.zeros((n, 6, 9), dtype), "ee": np.zeros((n, 3), dtype),
         "cam_pos": np.zeros((n, 3), dtype), "cam_mat": np.zeros((n, 9), dtype)}
    getattr(hostlibs.querycheck(), "qc_kinematics_" + _suffix(dtype))(n, ptr(q), *[ptr(o[k]) for k in ("xpos", "xmat", "ee", "cam_pos", "cam_mat")])
    return o


def twin_jacobian(q, dtype, link=EE_LINK, offset=None):
    q = _as(q, dtype); n = len(q); off = _as(offset, dtype)
    o = {"jacp": np.zeros((n, 3, 6), dtype), "jacr": np.zeros((n, 3, 6), dtype)}
    getattr(hostlibs.querycheck(), "qc_jacobian_" + _suffix(dtype))(n, ptr(q), link, ptr(off), ptr(o["jacp"]), ptr(o["jacr"]))
    return o


def twin_dynamics(q, v, qacc, dtype):
    q, v, qacc = _as(q, dtype), _as(v, dtype), _as(qacc, dtype); n = len(q)
    o = {"M": np.zeros((n, 6, 6), dtype), "bias": np.zeros((n, 6), dtype), "tau": np.zeros((n, 6), dtype)}
    getattr(hostlibs.querycheck(), "qc_dynamics_" + _suffix(dtype))(n, ptr(q), ptr(v), ptr(qacc), ptr(o["M"]), ptr(o["bias"]), ptr(o["tau"]))
    if qacc is None:
        del o["tau"]
    return o


def twin_ik(q0, target, dtype, link=EE_LINK, offset=None, iters=64, damping=0.02, tol=1e-4, max_step=0.3):
    q0, target, off = _as(q0, dtype), _as(target, dtype), _as(offset, dtype); n = len(q0)
    o = {"q": np.zeros((n, 6), dtype), "residual": np.zeros(n, dtype), "iterations": np.zeros(n, np.int32), "converged": np.zeros(n, np.uint8)}
    getattr(hostlibs.querycheck(), "qc_ik_" + _suffix(dtype))(n, ptr(q0), ptr(target), link, ptr(off), iters, damping, tol, max_step,
                                               ptr(o["q"]), ptr(o["residual"]), ptr(o["iterations"]), ptr(o["converged"]))
    return o


# ---- the oracle's side ----------------------------------------------------------------------------------------------------------------------------
def _data_at(d, q, v=None):
    L, m = O.lib(), O.model()
    L.so100o_reset_data(C.byref(m), C.byref(d))
    O.arr(d.qpos)[:6] = q
    if v is not None:
        O.arr(d.qvel)[:6] = v


def oracle_kinematics(q):
    """q [n, 6] float64 -> xpos [n, 6, 3], xmat [n, 6, 9], ee, cam_pos, cam_mat of so100o_kinematics / so100o_end_effector, and the joints'
    xaxis / xanchor [n, 6, 3] (link k is body k + 2, joint k is dof k)"""
    L, m, d = O.lib(), O.model(), O.Data()
    q = np.asarray(q, np.float64); n = len(q)
    o = {"xpos": np.zeros((n, 6, 3)), "xmat": np.zeros((n, 6, 9)), "ee": np.zeros((n, 3)), "cam_pos": np.zeros((n, 3)), "cam_mat": np.zeros((n, 9)),
         "xaxis": np.zeros((n, 6, 3)), "xanchor": np.zeros((n, 6, 3))}
    for i in range(n):
        _data_at(d, q[i])
        L.so100o_kinematics(C.byref(m), C.byref(d))
        o["xpos"][i], o["xmat"][i] = O.arr(d.xpos)[2:8], O.arr(d.xmat)[2:8]
        o["cam_pos"][i], o["cam_mat"][i] = O.arr(d.cam_xpos), O.arr(d.cam_xmat)
        o["xaxis"][i], o["xanchor"][i] = O.arr(d.xaxis)[:6], O.arr(d.xanchor)[:6]
        xp, xm = np.array(o["xpos"][i, EE_LINK]), np.array(o["xmat"][i, EE_LINK])
        L.so100o_end_effector(ptr(xp), ptr(xm), ptr(o["ee"][i]))
    return o


def oracle_point(q, link=EE_LINK, offset=EE_LOCAL):
    """world position [n, 3] of the point at `offset` of link `link`'s frame, from the oracle's FK"""
    k = oracle_kinematics(q)
    return k["xpos"][:, link] + np.einsum("nij,j->ni", k["xmat"][:, link].reshape(-1, 3, 3), np.asarray(offset, np.float64))


def oracle_jacobian(q, link=EE_LINK, offset=EE_LOCAL):
    """mj_jac's formula over the oracle's xaxis / xanchor: column k = axis_k x (p - anchor_k) | axis_k for k <= link, zero behind it"""
    k = oracle_kinematics(q)
    p = k["xpos"][:, link] + np.einsum("nij,j->ni", k["xmat"][:, link].reshape(-1, 3, 3), np.asarray(offset, np.float64))
    jacp, jacr = np.zeros((len(p), 3, 6)), np.zeros((len(p), 3, 6))
    for j in range(link + 1):
        jacp[:, :, j] = np.cross(k["xaxis"][:, j], p - k["xanchor"][:, j])
        jacr[:, :, j] = k["xaxis"][:, j]
    return {"jacp": jacp, "jacr": jacr}


def oracle_dynamics(q, v, qacc=None):
    """d.M[0:6, 0:6], d.qfrc_bias[0:6] of so100o_forward and, with qacc, M qacc + bias in fp64"""
    L, m, d = O.lib(), O.model(), O.Data()
    q = np.asarray(q, np.float64); n = len(q)
    v = np.zeros((n, 6)) if v is None else np.asarray(v, np.float64)
    o = {"M": np.zeros((n, 6, 6)), "bias": np.zeros((n, 6))}
    for i in range(n):
        _data_at(d, q[i], v[i])
        L.so100o_forward(C.byref(m), C.byref(d), 0, 1)
        o["M"][i] = O.arr(d.M).reshape(O.NV, O.NV)[:6, :6]
        o["bias"][i] = O.arr(d.qfrc_bias)[:6]
    if qacc is not None:
        o["tau"] = np.einsum("nij,nj->ni", o["M"], np.asarray(qacc, np.float64)) + o["bias"]
    return o


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def cases():
    """(q, v, qacc) float32 [CASES, 6]"""
    rs = np.random.RandomState(0)
    r = joint_range()
    q = rs.uniform(r[:, 0], r[:, 1], (CASES, 6)).astype(np.float32)
    v = rs.uniform(-2.0, 2.0, (CASES, 6)).astype(np.float32)
    qacc = rs.uniform(-20.0, 20.0, (CASES, 6)).astype(np.float32)
    return q, v, qacc


@functools.lru_cache(None)
def closed_form_reference():
    """the oracle on cases(), computed once: every quantity of FP32_BOUNDS"""
    q, v, qacc = (a.astype(np.float64) for a in cases())
    ref = oracle_kinematics(q)
    ref.update(oracle_jacobian(q))
    ref.update(oracle_dynamics(q, v, qacc))
    return ref


@functools.lru_cache(None)
def ik_recipe(n=400):
    """(q0, target, qstar) float32: q* uniform in the middle 80 % of every joint range, the target the oracle's end-effector point at q*,
    q0 = q* plus a uniform +-0.3 rad on joints 0..4; RandomState(0)"""
    rs = np.random.RandomState(0)
    r = joint_range()
    w = r[:, 1] - r[:, 0]
    qstar = rs.uniform(r[:, 0] + 0.1 * w, r[:, 1] - 0.1 * w, (n, 6)).astype(np.float32)
    noise = np.zeros((n, 6))
    noise[:, :5] = rs.uniform(-0.3, 0.3, (n, 5))
    q0 = (qstar.astype(np.float64) + noise).astype(np.float32)
    target = oracle_kinematics(qstar.astype(np.float64))["ee"].astype(np.float32)
    return q0, target, qstar


def max_abs_diff(got, ref, keys=None):
    """{quantity: max |got - ref|} over the quantities both have"""
    return {k: float(np.abs(np.asarray(got[k], np.float64).reshape(np.shape(ref[k])) - ref[k]).max()) for k in (keys or got) if k in ref}


def flags_comparable(q0, target, r64, a, b, tol=IK_DEFAULTS["tol"]):
    """mask of the cases whose converged flags and iteration counts are compared between the IK results a and b: those whose fp64 residual
    at the deciding check -- the first check at which either of the two stopped -- is not within IK_TOL_BAND of tol.  r64 is the fp64
    twin's result: where it stopped at that same check its returned residual is the one; elsewhere the fp64 twin is run again up to that check."""
    k = np.minimum(a["iterations"], b["iterations"])
    res = np.array(r64["residual"], np.float64)
    for i in np.where(k != r64["iterations"])[0]:
        if k[i] > 0:
            res[i] = twin_ik(q0[i:i + 1], target[i:i + 1], np.float64, **{**IK_DEFAULTS, "iters": int(k[i])})["residual"][0]
        else:
            start = np.clip(q0[i:i + 1].astype(np.float64), *joint_range().T)
            res[i] = np.linalg.norm(target[i].astype(np.float64) - oracle_point(start)[0])
    return np.abs(res - tol) > IK_TOL_BAND
