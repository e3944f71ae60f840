"""Shared by tests/test_lqr_cpu.py and tests/test_gpu_lqr.py: the host twin of the LQR query (tests/_lqrcheck), the input families, the
references and the bounds.

References.  (1) reference(): the recursion of include/so100_query.h in numpy fp64, written from the formulas, on the float32 inputs as the
device sees them.  (2) dense_minimiser(): independent of any recursion -- dx = S du condensed, the 6T x 6T Hessian and gradient of the
quadratic model assembled, one np.linalg.solve; with reg = 0, alpha = 1, no bounds and dx0 = 0 the forward pass's du must equal it.
Neither the twin nor the kernel is ever its own reference.  Inputs and references are computed once per process and never modified."""
import functools

import numpy as np

import trajectory_support as TS
from hostlibs import lqrcheck, ptr

NU = 6
ARM = np.r_[0:6, 12:18]                                    # the arm block of the 24 tangent indices: nx = 12
IDX = {24: np.arange(24), 12: ARM}
FLOAT_OUT = ("k", "K", "Vx0", "Vxx0", "dV", "du", "dx")
OUT = FLOAT_OUT + ("bad",)


def problem(A, B, lx, lxx, lu=None, luu=None, lux=None, nx=24, reg=0.0, alpha=1.0, u=None, u_lo=-1.0, u_hi=1.0, dx0=None):
    """the arguments of So100Sim.lqr as one dict (arrays float32, as the device sees them)"""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    return {"A": f(A), "B": f(B), "lx": f(lx), "lxx": f(lxx), "lu": f(lu), "luu": f(luu), "lux": f(lux), "nx": nx, "reg": float(reg), "alpha": float(alpha),
            "u": f(u), "u_lo": float(u_lo), "u_hi": float(u_hi), "dx0": f(dx0)}


def shapes(p):
    T, M = p["A"].shape[:2]
    n = p["nx"]
    return T, M, n, {"k": (T, M, NU), "K": (T, M, NU, n), "Vx0": (M, n), "Vxx0": (M, n, n), "dV": (M, 2), "du": (T, M, NU), "dx": (T + 1, M, n), "bad": (M,)}


def twin(p, dtype=np.float32):
    """the host twin on a problem(): every output, as numpy arrays of `dtype`"""
    lib = lqrcheck()
    T, M, n, shp = shapes(p)
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    ins = [cast(p[k]) for k in ("A", "B", "lx", "lxx", "lu", "luu", "lux", "u", "dx0")]
    out = {k: np.zeros(shp[k], np.int32 if k == "bad" else dtype) for k in OUT}
    fn = lib.lq_lqr_d if dtype == np.float64 else lib.lq_lqr_f
    fn(M, n, T, *[ptr(a) for a in ins], p["reg"], p["alpha"], p["u_lo"], p["u_hi"], *[ptr(out[k]) for k in OUT])
    return out


# ---- reference 1: the recursion in numpy fp64 --------------------------------------------------------------------------------------------------------
def _f64(p):
    """(A [T, M, n, n], B [T, M, n, 6], lx, lxx, lu, luu, lux) in fp64 and in the n of the call, the nullable costs as zeros"""
    T, M, n, _ = shapes(p)
    ix = IDX[n]
    A = p["A"].astype(np.float64)[:, :, ix][:, :, :, ix]; B = p["B"].astype(np.float64)[:, :, ix]
    z = lambda a, shape: np.zeros(shape) if a is None else a.astype(np.float64)
    return A, B, p["lx"].astype(np.float64), p["lxx"].astype(np.float64), z(p["lu"], (T, M, NU)), z(p["luu"], (T, M, NU, NU)), z(p["lux"], (T, M, NU, n))


def reference(p):
    """the outputs in fp64, plus "eig": [T, M, 2] the smallest and largest eigenvalue of each step's Quu + reg I (NaN from the step a problem fails
    at, downwards).  A problem with a non-finite input anywhere: bad = T."""
    T, M, n, shp = shapes(p)
    A, B, lx, lxx, lu, luu, lux = _f64(p)
    mv = lambda X, v: np.einsum("mij,mj->mi", X, v)
    tr = lambda X: np.swapaxes(X, 1, 2)
    bad = np.full(M, -1, np.int32)
    for a in (A, B, lx[:T], lxx[:T], lu, luu, lux) + (() if p["u"] is None else (p["u"].astype(np.float64),)):
        bad[~np.isfinite(a).reshape(T, M, -1).all(axis=(0, 2))] = T
    bad[~np.isfinite(lx[T]).all(axis=1) | ~np.isfinite(lxx[T]).all(axis=(1, 2))] = T
    if p["dx0"] is not None:
        bad[~np.isfinite(p["dx0"]).all(axis=1)] = T
    clean = lambda a: np.where(np.isfinite(a), a, 0.0)
    A, B, lx, lxx, lu, luu, lux = (clean(a) for a in (A, B, lx, lxx, lu, luu, lux))
    Vx, Vxx = lx[T].copy(), 0.5*(lxx[T] + tr(lxx[T]))
    k = np.zeros((T, M, NU)); K = np.zeros((T, M, NU, n)); dV = np.zeros((M, 2)); eig = np.full((T, M, 2), np.nan)
    eye = np.eye(NU)
    for t in range(T - 1, -1, -1):
        At, Bt = A[t], B[t]
        Qx = lx[t] + mv(tr(At), Vx); Qu = lu[t] + mv(tr(Bt), Vx)
        Qxx = lxx[t] + tr(At) @ Vxx @ At; Qux = lux[t] + tr(Bt) @ Vxx @ At; Quu = luu[t] + tr(Bt) @ Vxx @ Bt
        Quu_r = Quu + p["reg"]*eye
        w = np.linalg.eigvalsh(0.5*(Quu_r + tr(Quu_r)))
        alive = bad < 0
        eig[t, alive, 0], eig[t, alive, 1] = w[alive, 0], w[alive, -1]
        failed = alive & ~(w[:, 0] > 0.0)
        bad[failed] = t
        Quu_r = np.where((bad < 0)[:, None, None], Quu_r, eye)             # a failed problem goes on as a harmless one; its outputs are NaN in the end
        kt = -np.linalg.solve(Quu_r, Qu[..., None])[..., 0]; Kt = -np.linalg.solve(Quu_r, Qux)
        k[t], K[t] = kt, Kt
        Quuk = mv(Quu, kt)
        dV[:, 0] += np.einsum("mi,mi->m", kt, Qu); dV[:, 1] += 0.5*np.einsum("mi,mi->m", kt, Quuk)
        Vx = Qx + mv(tr(Kt), Quuk) + mv(tr(Kt), Qu) + mv(tr(Qux), kt)
        Vxx = Qxx + tr(Kt) @ Quu @ Kt + tr(Kt) @ Qux + tr(Qux) @ Kt
        Vxx = 0.5*(Vxx + tr(Vxx))
    dx = np.zeros((T + 1, M, n)); du = np.zeros((T, M, NU))
    if p["dx0"] is not None:
        dx[0] = clean(p["dx0"].astype(np.float64))
    for t in range(T):
        d = p["alpha"]*k[t] + mv(K[t], dx[t])
        if p["u"] is not None:
            u = clean(p["u"][t].astype(np.float64))
            d = np.clip(u + d, p["u_lo"], p["u_hi"]) - u
        du[t] = d
        dx[t + 1] = mv(A[t], dx[t]) + mv(B[t], d)
    out = {"k": k, "K": K, "Vx0": Vx, "Vxx0": Vxx, "dV": dV, "du": du, "dx": dx, "bad": bad, "eig": eig}
    for name in FLOAT_OUT:
        a = out[name]
        (a if name in ("Vx0", "Vxx0", "dV") else np.swapaxes(a, 0, 1))[bad >= 0] = np.nan
    return out


# ---- reference 2: the dense minimiser ----------------------------------------------------------------------------------------------------------------
def dense_minimiser(p):
    """du [T, M, 6] minimising the quadratic model from dx0 = 0, without a recursion: dx = S du, H du = -g"""
    T, M, n, _ = shapes(p)
    A, B, lx, lxx, lu, luu, lux = _f64(p)
    du = np.zeros((T, M, NU))
    for m in range(M):
        S = np.zeros(((T + 1)*n, T*NU))                        # dx_t = S[t] du
        for t in range(T):
            S[(t + 1)*n:(t + 2)*n] = A[t, m] @ S[t*n:(t + 1)*n]
            S[(t + 1)*n:(t + 2)*n, t*NU:(t + 1)*NU] += B[t, m]
        Lxx = np.zeros(((T + 1)*n, (T + 1)*n)); Luu = np.zeros((T*NU, T*NU)); Lux = np.zeros((T*NU, (T + 1)*n))
        for t in range(T + 1):
            Lxx[t*n:(t + 1)*n, t*n:(t + 1)*n] = 0.5*(lxx[t, m] + lxx[t, m].T)
            if t < T:
                Luu[t*NU:(t + 1)*NU, t*NU:(t + 1)*NU] = 0.5*(luu[t, m] + luu[t, m].T)
                Lux[t*NU:(t + 1)*NU, t*n:(t + 1)*n] = lux[t, m]
        H = S.T @ Lxx @ S + Luu + Lux @ S + (Lux @ S).T
        g = S.T @ lx[:, m].reshape(-1) + lu[:, m].reshape(-1)
        du[:, m] = -np.linalg.solve(H, g).reshape(T, NU)
    return du


def model_value(p, du, dx):
    """the quadratic model at (du [T, M, 6], dx [T + 1, M, n]) in fp64: [M]"""
    T, M, n, _ = shapes(p)
    _, _, lx, lxx, lu, luu, lux = _f64(p)
    v = np.einsum("tmi,tmi->m", lx, dx) + 0.5*np.einsum("tmi,tmij,tmj->m", dx, lxx, dx)
    return v + np.einsum("tmi,tmi->m", lu, du) + 0.5*np.einsum("tmi,tmij,tmj->m", du, luu, du) + np.einsum("tmi,tmij,tmj->m", du, lux, dx[:T])


# ---- family S: synthetic ----------------------------------------------------------------------------------------------------------------------------------
S_T = (1, 2, 5, 16, 64)
S_M = 65


@functools.lru_cache(maxsize=None)
def family_s(n, T, M=S_M):
    """per problem and step: A = I + 0.3 N / sqrt(n), B = 0.3 N, [lxx lxu; lux luu] = C C' + 0.1 I with C = N / sqrt(n + 6), lx, lu = N -- seeded.
    A and B are drawn as full 24-row matrices; the arm form reads its block."""
    rng = np.random.default_rng(0)
    A = np.eye(24) + 0.3*rng.standard_normal((T, M, 24, 24))/np.sqrt(n)
    B = 0.3*rng.standard_normal((T, M, 24, NU))
    Cm = rng.standard_normal((T + 1, M, n + NU, n + NU))/np.sqrt(n + NU)
    P = Cm @ np.swapaxes(Cm, 2, 3) + 0.1*np.eye(n + NU)
    lx = rng.standard_normal((T + 1, M, n)); lu = rng.standard_normal((T, M, NU))
    return problem(A, B, lx, P[:, :, :n, :n], lu, P[:T, :, n:, n:], P[:T, :, n:, :n], nx=n)


def first(p, M):
    """the first M problems of a problem()"""
    q = dict(p)
    for name in ("A", "B", "lx", "lxx", "lu", "luu", "lux", "u"):
        if p[name] is not None:
            q[name] = np.ascontiguousarray(p[name][:, :M])
    if p["dx0"] is not None:
        q["dx0"] = np.ascontiguousarray(p["dx0"][:M])
    return q


@functools.lru_cache(maxsize=None)
def reference_s(n, T, M=S_M):
    return reference(family_s(n, T, M))


# ---- family P: physics ---------------------------------------------------------------------------------------------------------------------------------
P_T, P_M, P_NSUB = 8, 3, 16
P_CONTROL_COST, P_DAMPING = 1e-5, 1e-5                      # examples/ilqr_reach.py


def family_p(n, roll, derivatives, jacobian):
    """the example's problem on the first P_M starts of trajectory_support.free_case("arm", "actions") under F_CUBE_PINNED: a seeded plan of P_T
    actions is rolled out, every (state, action) pair linearised, and |ee - cube|^2 after each action gets its Gauss-Newton terms.
    roll(U [T, M, 6], qpos, qvel) -> {"qpos" [T, M, 13], "qvel" [T, M, 12], "ee" [T, M, 3]}; derivatives(U [TM, 6], qpos [TM, 13], qvel [TM, 12]) ->
    {"A", "B"}; jacobian(q [TM, 6]) -> jacp [TM, 3, 6]: the twins on the CPU, So100Sim's queries on the GPU.  Returns (problem, the plan)."""
    c = TS.free_case("arm", "actions")
    q0, v0 = c["qpos"][:P_M], c["qvel"][:P_M]
    T, M = P_T, P_M
    U = np.random.default_rng(1).uniform(-0.5, 0.5, (T, M, NU)).astype(np.float32)
    U[..., 5] = 0.0
    r = roll(U, q0, v0)
    qn, vn, ee = (np.asarray(r[name], np.float32) for name in ("qpos", "qvel", "ee"))
    Xq = np.concatenate([q0[None], qn[:-1]]); Xv = np.concatenate([v0[None], vn[:-1]])
    d = derivatives(U.reshape(T*M, NU), Xq.reshape(T*M, 13), Xv.reshape(T*M, 12))
    A = np.asarray(d["A"], np.float32).reshape(T, M, 24, 24); B = np.asarray(d["B"], np.float32).reshape(T, M, 24, NU).copy()
    B[..., 5] = 0.0                                              # the jaw does not move the end-effector point
    J = np.asarray(jacobian(qn[..., :6].reshape(T*M, 6)), np.float64).reshape(T, M, 3, 6)
    res = (ee - qn[..., 6:9]).astype(np.float64)
    lx = np.zeros((T + 1, M, n)); lxx = np.zeros((T + 1, M, n, n))
    lx[1:, :, :6] = 2.0*np.einsum("tmij,tmi->tmj", J, res)
    lxx[1:, :, :6, :6] = 2.0*np.einsum("tmij,tmik->tmjk", J, J)
    lu = 2.0*P_CONTROL_COST*U
    luu = np.broadcast_to(2.0*P_CONTROL_COST*np.eye(NU), (T, M, NU, NU))
    return problem(A, B, lx, lxx, lu, luu, None, nx=n, reg=P_DAMPING), U


@functools.lru_cache(maxsize=None)
def family_p_cpu(n):
    """family_p from the host twins of the three queries (fp32, as the device computes them)"""
    import derivatives_support as DS
    import query_support as QS
    import scenes
    roll = lambda U, q, v: TS.twin(U, q, v, "actions", P_NSUB, scenes.FREE, np.float32)
    der = lambda U, q, v: DS.twin(U, q, v, "actions", P_NSUB, scenes.FREE, np.float32)
    jac = lambda q: QS.twin_jacobian(q, np.float32)["jacp"]
    return family_p(n, roll, der, jac)[0]


# ---- the failure cases ---------------------------------------------------------------------------------------------------------------------------------
FAIL_T, FAIL_M, FAIL_AT, FAIL_PROBLEM = 5, 3, 2, 1
GOOD_RATIO, BAD_EIG = 1e-3, -1e-2


@functools.lru_cache(maxsize=None)
def indefinite_case(n):
    """family S at T = 5, M = 3 with luu = -I (and lux = 0, B a tenth) at step FAIL_AT of problem FAIL_PROBLEM: (the problem with reg = 0, the
    same with reg = 4).  Asserted on the fp64 reference alone: under reg = 0 that step's smallest eigenvalue is <= -1e-2 and every other Quu_r has an
    eigenvalue ratio >= 1e-3; under reg = 4 every one has, so fp32 and fp64 cannot disagree on which problem fails where."""
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in first(family_s(n, FAIL_T), FAIL_M).items()}
    p["luu"][FAIL_AT, FAIL_PROBLEM] = -np.eye(NU); p["lux"][FAIL_AT, FAIL_PROBLEM] = 0.0; p["B"][FAIL_AT, FAIL_PROBLEM] *= np.float32(0.1)
    q = dict(p); q["reg"] = 4.0
    e0, e4 = reference(p)["eig"], reference(q)["eig"]
    assert e0[FAIL_AT, FAIL_PROBLEM, 0] <= BAD_EIG
    good = np.ones(e0.shape[:2], bool); good[:FAIL_AT + 1, FAIL_PROBLEM] = False
    assert (e0[good, 0]/e0[good, 1] >= GOOD_RATIO).all() and (e4[..., 0]/e4[..., 1] >= GOOD_RATIO).all()
    return p, q


@functools.lru_cache(maxsize=None)
def nonfinite_cases(n):
    """family S at T = 5, M = 3: (a NaN in problem 1's A at step 3, an inf in problem 1's lx at step 0): bad = T there"""
    base = first(family_s(n, FAIL_T), FAIL_M)
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    a["A"][3, FAIL_PROBLEM, 1, 13] = np.nan                   # row 1, column 13: in the arm block too
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    b["lx"][0, FAIL_PROBLEM, 2] = np.inf
    return a, b


def assert_quu_is_well_conditioned(ref):
    e = ref["eig"]
    assert (e[..., 0]/e[..., 1] >= GOOD_RATIO).all(), float((e[..., 0]/e[..., 1]).min())


# ---- deviations and bounds -------------------------------------------------------------------------------------------------------------------------------
def deviation(got, ref):
    """{group: max |got - ref| / max(1, max |ref|)} over the float outputs present in `got`, always against the fp64 reference"""
    out = {}
    for name in FLOAT_OUT:
        if name in got and got[name] is not None:
            r = ref[name]
            out[name] = float(np.abs(np.asarray(got[name], np.float64) - r).max()/max(1.0, np.abs(r).max()))
    return out


FP64_BOUND = 1e-11
# The fp32 twin's largest deviation from the fp64 reference per output group, rounded up: family S over n in {12, 24} x T in S_T (65 problems
# each), family P over both n -- measured by tests/test_lqr_cpu.py, which prints them as [lqr-tol] lines and holds the twin to TWIN_FACTOR x
# these; the kernel is held to KERNEL_FACTOR x these (trajectory_support's rule: the kernel sums in another order).
FP32_MEASURED = {
    "S": {"k": 7.3e-7, "K": 6.9e-7, "Vx0": 6.4e-7, "Vxx0": 7.6e-7, "dV": 2.6e-7, "du": 1.1e-6, "dx": 9.4e-7},
    "P": {"k": 2.3e-6, "K": 9.3e-7, "Vx0": 9.6e-8, "Vxx0": 6.8e-8, "dV": 6.1e-8, "du": 2.4e-6, "dx": 2.6e-6},
}
TWIN_FACTOR, KERNEL_FACTOR = TS.TWIN_FACTOR, TS.KERNEL_FACTOR


def within(dev, family, factor):
    """asserts every group of a deviation() inside factor x the record"""
    for name, d in dev.items():
        assert d <= factor*FP32_MEASURED[family][name], (family, name, d, factor*FP32_MEASURED[family][name])
