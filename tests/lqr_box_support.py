"""For tests/test_lqr_box_cpu.py: the host twin of the control-limited LQR pass of tests/_lqrboxcheck/lqr_box.hpp (built by the Makefile
beside it), the input families, the reference and the bounds.

Reference.  reference(): the recursion of lqr_box.hpp's header comment in numpy fp64, written from the formulas, on the float32
inputs as a device would see them.  Each step's QP is NOT solved by the projected-Newton iteration lqr_boxqp6 fixes: all 3^6 assignments of
(free, at the lower bound, at the upper bound) to the six controls are solved and the one that satisfies the KKT conditions -- free components
inside their bounds, the gradient's sign right on the clamped ones -- is taken; H is positive definite, so that one is the minimiser.  It also
records each problem's margin: the smallest, over its steps, of the distance of a free component to a bound and |grad| of a clamped one.  An
active set that flips moves K discontinuously, so a problem whose margin is under MARGIN proves nothing and is left out (family SB only; never
more than a quarter of a shape, asserted on the reference alone).  The twin is never its own reference.  Inputs and
references are computed once per process and never modified."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np

import lqr_support as S
from hostlibs import ptr

NU = S.NU
FLOAT_OUT, OUT = S.FLOAT_OUT, S.OUT + ("clamped", "qp_used")
QP_ITERS = 16
RAN_OUT = 1 << 16
MARGIN = 1e-3
HERE = os.path.dirname(os.path.abspath(__file__))

_p, _i, _l, _f, _d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double
LQRBOXCHECK = {"lb_lqr_box_d": (None, [_l, _i, _i] + [_p]*9 + [_d]*4 + [_i] + [_p]*10),
               "lb_lqr_box_f": (None, [_l, _i, _i] + [_p]*9 + [_f]*4 + [_i] + [_p]*10)}


@functools.lru_cache(maxsize=None)
def lqrboxcheck():
    """tests/_lqrboxcheck/liblqrboxcheck.so, made and loaded once, every symbol with its signature"""
    d = os.path.join(HERE, "_lqrboxcheck")
    subprocess.check_call(["make", "-C", d, "-s", "liblqrboxcheck.so"])
    lib = C.CDLL(os.path.join(d, "liblqrboxcheck.so"))
    for name, (restype, argtypes) in LQRBOXCHECK.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def shapes(p):
    T, M, n, shp = S.shapes(p)
    return T, M, n, dict(shp, clamped=(T, M), qp_used=(T, M))


def twin(p, dtype=np.float32, qp_iters=QP_ITERS):
    """the host twin on a lqr_support.problem() with u: every output, as numpy arrays of `dtype` (bad, clamped, qp_used: int32)"""
    lib = lqrboxcheck()
    T, M, n, shp = shapes(p)
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    ins = [cast(p[k]) for k in ("A", "B", "lx", "lxx", "lu", "luu", "lux", "u", "dx0")]
    out = {k: np.zeros(shp[k], np.int32 if k in ("bad", "clamped", "qp_used") else dtype) for k in OUT}
    fn = lib.lb_lqr_box_d if dtype == np.float64 else lib.lb_lqr_box_f
    fn(M, n, T, *[ptr(a) for a in ins], p["reg"], p["alpha"], p["u_lo"], p["u_hi"], qp_iters, *[ptr(out[k]) for k in OUT])
    return out


# ---- the reference: the recursion in numpy fp64, each step's QP by enumeration ----------------------------------------------------------------------
STATES = np.array(list(itertools.product((0, 1, 2), repeat=NU)))           # [729, 6]: 0 free, 1 at the lower bound, 2 at the upper bound


def box_qp(H, g, lo, hi):
    """argmin x'Hx/2 + g'x over lo <= x <= hi for M problems at once (H [M, 6, 6] positive definite, the rest [M, 6]) by enumeration:
    (x [M, 6], state [M, 6] of STATES' codes, margin [M])"""
    M = H.shape[0]
    free = (STATES == 0)[None]                                              # [1, 729, 6]
    xc = np.where(STATES[None] == 1, lo[:, None], np.where(STATES[None] == 2, hi[:, None], 0.0))      # [M, 729, 6]: the clamped components, 0 elsewhere
    ff = free[..., :, None] & free[..., None, :]
    Hm = np.where(ff, H[:, None], 0.0) + np.where(free, 0.0, 1.0)[..., None]*np.eye(NU)
    rhs = np.where(free, -(g[:, None] + np.einsum("mij,msj->msi", H, xc)), xc)
    x = np.linalg.solve(Hm, rhs[..., None])[..., 0]
    grad = g[:, None] + np.einsum("mij,msj->msi", H, x)
    slack = np.where(free, np.minimum(x - lo[:, None], hi[:, None] - x), np.where(STATES[None] == 1, grad, -grad))      # >= 0 everywhere: a KKT point
    worst = slack.min(axis=2)                                               # [M, 729]
    best = worst.argmax(axis=1)                                             # the one KKT point (degenerate ties: the same x)
    m = np.arange(M)
    assert (worst[m, best] >= 0.0).all(), float(worst[m, best].min())
    return x[m, best], np.broadcast_to(STATES[best], (M, NU)), worst[m, best]


def reference(p):
    """the outputs in fp64 with "clamped" in LqrBoxArgs' bits, plus "margin" [M], "gscale" [M] (the largest |Qu_j| over the problem's steps: the scale
    of its gradients) and "eig" as lqr_support.reference gives it.  A problem fails
    where Quu + reg I is not positive definite (every failure case here starts its QP with nothing clamped, where the whole matrix is factored)."""
    T, M, n, shp = S.shapes(p)
    A, B, lx, lxx, lu, luu, lux = S._f64(p)
    mv = lambda X, v: np.einsum("mij,mj->mi", X, v)
    tr = lambda X: np.swapaxes(X, 1, 2)
    u = p["u"].astype(np.float64)
    bad = np.full(M, -1, np.int32)
    for a in (A, B, lx[:T], lxx[:T], lu, luu, lux, u):
        bad[~np.isfinite(a).reshape(T, M, -1).all(axis=(0, 2))] = T
    bad[~np.isfinite(lx[T]).all(axis=1) | ~np.isfinite(lxx[T]).all(axis=(1, 2))] = T
    if p["dx0"] is not None:
        bad[~np.isfinite(p["dx0"]).all(axis=1)] = T
    clean = lambda a: np.where(np.isfinite(a), a, 0.0)
    A, B, lx, lxx, lu, luu, lux, u = (clean(a) for a in (A, B, lx, lxx, lu, luu, lux, u))
    lo, hi = p["u_lo"] - u, p["u_hi"] - u                                   # each difference rounded once, here in fp64
    Vx, Vxx = lx[T].copy(), 0.5*(lxx[T] + tr(lxx[T]))
    k = np.zeros((T, M, NU)); K = np.zeros((T, M, NU, n)); dV = np.zeros((M, 2)); eig = np.full((T, M, 2), np.nan)
    clamped = np.zeros((T, M), np.int32); margin = np.full(M, np.inf); gscale = np.zeros(M)
    eye = np.eye(NU)
    for t in range(T - 1, -1, -1):
        At, Bt = A[t], B[t]
        Qx = lx[t] + mv(tr(At), Vx); Qu = lu[t] + mv(tr(Bt), Vx)
        Qxx = lxx[t] + tr(At) @ Vxx @ At; Qux = lux[t] + tr(Bt) @ Vxx @ At; Quu = luu[t] + tr(Bt) @ Vxx @ Bt
        Quu_r = Quu + p["reg"]*eye
        w = np.linalg.eigvalsh(0.5*(Quu_r + tr(Quu_r)))
        alive = bad < 0
        eig[t, alive, 0], eig[t, alive, 1] = w[alive, 0], w[alive, -1]
        bad[alive & ~(w[:, 0] > 0.0)] = t
        Quu_r = np.where((bad < 0)[:, None, None], Quu_r, eye)             # a failed problem goes on as a harmless one; its outputs are NaN in the end
        kt, state, mg = box_qp(Quu_r, Qu, lo[t], hi[t])
        free = state == 0
        margin = np.where(bad < 0, np.minimum(margin, mg), margin)
        gscale = np.where(bad < 0, np.maximum(gscale, np.abs(Qu).max(axis=1)), gscale)
        clamped[t] = ((state == 1) << np.arange(NU)).sum(axis=1) + ((state == 2) << (8 + np.arange(NU))).sum(axis=1)
        Hm = np.where(free[:, :, None] & free[:, None, :], Quu_r, 0.0) + np.where(free, 0.0, 1.0)[..., None]*eye
        Kt = -np.linalg.solve(Hm, np.where(free[..., None], Qux, 0.0))
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
        du[t] = np.clip(u[t] + p["alpha"]*k[t] + mv(K[t], dx[t]), p["u_lo"], p["u_hi"]) - u[t]
        dx[t + 1] = mv(A[t], dx[t]) + mv(B[t], du[t])
    out = {"k": k, "K": K, "Vx0": Vx, "Vxx0": Vxx, "dV": dV, "du": du, "dx": dx, "bad": bad, "eig": eig, "clamped": clamped, "margin": margin, "gscale": gscale}
    for name in FLOAT_OUT:
        a = out[name]
        (a if name in ("Vx0", "Vxx0", "dV") else np.swapaxes(a, 0, 1))[bad >= 0] = np.nan
    clamped[:, bad >= 0] = 0
    return out


def select(p, idx):
    """the problems `idx` of a problem() or of a reference(), in that order"""
    idx = np.asarray(idx)
    q = dict(p)
    for name, a in p.items():
        if isinstance(a, np.ndarray):
            q[name] = np.ascontiguousarray(a[idx] if name in ("Vx0", "Vxx0", "dV", "bad", "dx0", "margin", "gscale") else a[:, idx])
    return q


def count_clamped(clamped):
    """the number of clamped controls per step, from the bits of `clamped`"""
    c = np.asarray(clamped)
    return sum(((c >> j) & 1) + ((c >> (8 + j)) & 1) for j in range(NU))


# ---- family SB: lqr_support's family S with nominal controls near the bounds -----------------------------------------------------------------------------
SB_T = (1, 2, 5, 16)
SB_GENERATED, SB_M = 88, 65                                # 65 of 88 is the quarter that may be left out, to the problem


@functools.lru_cache(maxsize=None)
def family_sb(n, T):
    """(the first SB_M problems of family S at SB_GENERATED problems with u uniform in +-0.8 under bounds +-1 whose reference margin is at least MARGIN,
    their reference, the share of generated problems kept)"""
    p = dict(S.family_s(n, T, SB_GENERATED))
    p["u"] = np.random.default_rng(5).uniform(-0.8, 0.8, (T, SB_GENERATED, NU)).astype(np.float32)
    ref = reference(p)
    assert (ref["bad"] == -1).all()
    kept = np.flatnonzero(ref["margin"] >= MARGIN)
    return select(p, kept[:SB_M]), select(ref, kept[:SB_M]), len(kept)/SB_GENERATED


# ---- family AB: every control of every step clamps ----------------------------------------------------------------------------------------------------------
AB_T, AB_M, AB_LU = 5, 3, 1e5


@functools.lru_cache(maxsize=None)
def family_ab(n):
    """family S at T = 5, M = 3 with luu = 1e-3 I, no cross term and lu = +-1e5 with seeded signs: (the problem, its reference)"""
    p = dict(S.first(S.family_s(n, AB_T), AB_M))
    rng = np.random.default_rng(6)
    p["u"] = rng.uniform(-0.8, 0.8, (AB_T, AB_M, NU)).astype(np.float32)
    p["lu"] = (AB_LU*rng.choice([-1.0, 1.0], (AB_T, AB_M, NU))).astype(np.float32)
    p["luu"] = np.ascontiguousarray(np.broadcast_to(1e-3*np.eye(NU), (AB_T, AB_M, NU, NU)), np.float32)
    p["lux"] = None
    return p, reference(p)


def value_without_feedback(p):
    """Vxx0 of the recursion with K = 0: Vxx <- sym(lxx_t + A_t' Vxx A_t), in fp64"""
    T, M, n, _ = S.shapes(p)
    A, _, _, lxx, _, _, _ = S._f64(p)
    tr = lambda X: np.swapaxes(X, 1, 2)
    V = 0.5*(lxx[T] + tr(lxx[T]))
    for t in range(T - 1, -1, -1):
        V = lxx[t] + tr(A[t]) @ V @ A[t]
        V = 0.5*(V + tr(V))
    return V


# ---- family PB: lqr_support's family P under bounds +-1, the plan scaled towards them --------------------------------------------------------------------
PB_SCALE = 1.9                                             # family P draws its plan in +-0.5: +-0.95 here
# No problem of PB is left out, so each must stand clear of a flip by the same rule as SB.  Its cost is in metres squared, so its gradients are
# far below SB's order 1 (the reference's "gscale": about 0.05); scaling the plan does not move its margin (4e-4 at every scale from 1 to 2), which a
# clamped control's gradient sets.  The floor is therefore MARGIN relative to the problem's own gradient scale: margin >= MARGIN * min(1, gscale).


def pb_margin_floor(ref):
    return MARGIN*np.minimum(1.0, ref["gscale"])


def family_pb(n, roll, derivatives, jacobian):
    """lqr_support.family_p on PB_SCALE x its plan (the callables scale the plan they are handed, so the rollout, the linearisation and the
    cost are those of the scaled plan; lu, which family_p forms from the plan itself, is scaled after it) with u = that plan: the problem"""
    s = np.float32(PB_SCALE)
    p, U = S.family_p(n, lambda U, q, v: roll(s*U, q, v), lambda U, q, v: derivatives(s*U, q, v), jacobian)
    p = dict(p)
    p["u"] = np.ascontiguousarray(s*U, np.float32)
    p["lu"] = np.ascontiguousarray(s*p["lu"], np.float32)
    return p


@functools.lru_cache(maxsize=None)
def family_pb_cpu(n):
    """family_pb from the host twins of the three queries (fp32, as the device computes them)"""
    import derivatives_support as DS
    import query_support as QS
    import scenes
    import trajectory_support as TS
    roll = lambda U, q, v: TS.twin(U, q, v, "actions", S.P_NSUB, scenes.FREE, np.float32)
    der = lambda U, q, v: DS.twin(U, q, v, "actions", S.P_NSUB, scenes.FREE, np.float32)
    jac = lambda q: QS.twin_jacobian(q, np.float32)["jacp"]
    return family_pb(n, roll, der, jac)


# ---- deviations and bounds -------------------------------------------------------------------------------------------------------------------------------
deviation = S.deviation
FP64_BOUND, TWIN_FACTOR, KERNEL_FACTOR = S.FP64_BOUND, S.TWIN_FACTOR, S.KERNEL_FACTOR
# The fp32 twin's largest deviation from the fp64 reference per output group, rounded up: family SB over n in {12, 24} x T in SB_T (65 retained
# problems each), family AB and family PB over both n -- measured by tests/test_lqr_box_cpu.py, which prints them as [lqr-box-tol] lines and
# holds the twin to TWIN_FACTOR x these; a kernel is to be held to KERNEL_FACTOR x these (lqr_support's rule).
FP32_MEASURED_BOX = {
    "SB": {"k": 5.9e-7, "K": 7.3e-7, "Vx0": 6.7e-7, "Vxx0": 5.1e-7, "dV": 2.3e-7, "du": 1.2e-6, "dx": 6.8e-7},
    "AB": {"k": 3.4e-8, "K": 0.0, "Vx0": 3.1e-7, "Vxx0": 3.8e-7, "dV": 1.6e-7, "du": 3.4e-8, "dx": 2.1e-7},      # K is exactly 0 there
    "PB": {"k": 3.1e-8, "K": 6.1e-8, "Vx0": 1.6e-7, "Vxx0": 2.0e-7, "dV": 2.9e-8, "du": 3.1e-8, "dx": 1.1e-7},
}


def within(dev, family, factor):
    """asserts every group of a deviation() inside factor x the record"""
    for name, d in dev.items():
        assert d <= factor*FP32_MEASURED_BOX[family][name], (family, name, d, factor*FP32_MEASURED_BOX[family][name])
