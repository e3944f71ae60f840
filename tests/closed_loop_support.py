"""Shared by tests/test_closed_loop_cpu.py and tests/test_gpu_closed_loop.py: the host twin of the closed-loop trajectory query
(tests/_closedcheck, built and loaded by tests/hostlibs.py), the input families, the references and the bounds.

Reference.  The fp64 ORACLE chained as trajectory_support chains it (so100o_step from the fp32-rounded start), with the feedback law of
include/so100_query.h written in numpy fp64 from its formula, on the float32 inputs as the device sees them (gains, nominal controls,
references, alpha).  It is not a second instantiation of so100_closed_loop.hpp.  Families and references are computed once per process and
never modified."""
import ctypes as C
import functools

import numpy as np

import derivatives_support as DS
import lqr_support as LS
import scenes
import trajectory_support as TS
from hostlibs import closedcheck, ptr


NU = 6
IDX = LS.IDX                                               # nx -> the tangent indices of the form
FLOAT_OUT = ("u", "qpos", "qvel", "ee", "residual")
INT_OUT = ("ncon", "dropped", "sig")
FIELDS = FLOAT_OUT + INT_OUT
MAX_L = 16


def twin(u, qpos_ref, qvel_ref, K, k=None, *, alphas=(1.0,), nx=24, qpos, qvel=None, ref0=None, mode="targets", nsub=16, flags=scenes.REFP, clamp=None,
         dtype=np.float32, solver_iters=2, contact_iters=20, warm=None):
    """the host twin on problem-major arrays: u [T, n, 6], qpos_ref [T, n, 13], qvel_ref [T, n, 12] (None with T = 1), K [T, n, 6, nx], k [T, n, 6] or
    None, qpos [n, 13], qvel [n, 12] or None, ref0 = (qpos [n, 13], qvel [n, 12]) or None, clamp = (lo, hi) or None.  Returns the dict
    So100Sim.closed_loop returns, as numpy arrays [T, n, L, .] (bad_step [n, L]), plus "qpos_final" and "qvel_final" [n, L, .]."""
    lib = closedcheck()
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    uu, rq, rv, KK, kk, q, v, w = (cast(a) for a in (u, qpos_ref, qvel_ref, K, k, qpos, qvel, warm))
    r0q, r0v = (None, None) if ref0 is None else (cast(ref0[0]), cast(ref0[1]))
    T, n = uu.shape[0], uu.shape[1]
    L = len(alphas)
    assert uu.shape == (T, n, 6) and q.shape == (n, 13) and KK.shape == (T, n, 6, nx) and (T == 1 or (rq.shape == (T, n, 13) and rv.shape == (T, n, 12)))
    al = np.asarray(np.asarray(alphas, np.float32), dtype)     # the device's float alpha, in the twin's precision
    i32 = np.int32
    out = {"u": np.zeros((T, n, L, 6), dtype), "qpos": np.zeros((T, n, L, 13), dtype), "qvel": np.zeros((T, n, L, 12), dtype), "ee": np.zeros((T, n, L, 3), dtype),
           "qpos_final": np.zeros((n, L, 13), dtype), "qvel_final": np.zeros((n, L, 12), dtype), "ncon": np.zeros((T, n, L), i32),
           "dropped": np.zeros((T, n, L), i32), "sig": np.zeros((T, n, L), i32), "residual": np.zeros((T, n, L), dtype), "bad_step": np.zeros((n, L), i32)}
    lo, hi = (0.0, 0.0) if clamp is None else clamp
    fn = lib.cc_closed_loop_d if dtype == np.float64 else lib.cc_closed_loop_f
    fn(n, ptr(q), ptr(v), ptr(w), ptr(uu), TS.MODES[mode], T, nsub, int(flags), solver_iters, contact_iters, ptr(rq), ptr(rv), ptr(r0q), ptr(r0v), nx, ptr(kk), ptr(KK),
       L, ptr(al), int(clamp is not None), float(lo), float(hi),
       *[ptr(out[name]) for name in ("u", "qpos", "qvel", "ee", "qpos_final", "qvel_final", "ncon", "dropped", "sig", "residual", "bad_step")])
    return out


# ---- the reference: the oracle under the law in numpy fp64 ---------------------------------------------------------------------------------------------
def law(qpos, qvel, xq, xv, u, k, K, alpha, nx, clamp=None):
    """c [6] of one rollout at one step in fp64: u + (alpha k + K dx), clamped; xq None: dx = 0"""
    dx = np.zeros(24) if xq is None else DS.tangent_difference(qpos, qvel, xq, xv, 1.0)
    c = u + (alpha*k + K @ dx[IDX[nx]])
    return c if clamp is None else np.clip(c, clamp[0], clamp[1])


def reference(u, qpos_ref, qvel_ref, K, k, alphas, nx, qpos, qvel, ref0, mode, nsub, flags, clamp=None, check=None):
    """{"u" [T, n, L, 6], "qpos" [T, n, L, 13], "qvel" [T, n, L, 12], "ee" [T, n, L, 3]} in fp64 from float32 inputs; check(d) is called on the oracle's
    data before every substep"""
    f64 = lambda a: None if a is None else np.asarray(a, np.float32).astype(np.float64)
    u, qpos_ref, qvel_ref, K, k, qpos, qvel = (f64(a) for a in (u, qpos_ref, qvel_ref, K, k, qpos, qvel))
    r0 = None if ref0 is None else (f64(ref0[0]), f64(ref0[1]))
    al = np.asarray(alphas, np.float32).astype(np.float64)
    T, n, L = u.shape[0], u.shape[1], len(al)
    out = {"u": np.zeros((T, n, L, 6)), "qpos": np.zeros((T, n, L, 13)), "qvel": np.zeros((T, n, L, 12))}
    for m in range(n):
        for a in range(L):
            q, v = qpos[m].copy(), qvel[m].copy()
            for t in range(T):
                if t == 0:
                    xq, xv = (None, None) if r0 is None else (r0[0][m], r0[1][m])
                else:
                    xq, xv = qpos_ref[t - 1, m], qvel_ref[t - 1, m]
                c = law(q, v, xq, xv, u[t, m], np.zeros(6) if k is None else k[t, m], K[t, m], al[a], nx, clamp)
                q, v = DS.oracle_next(q, v, c, mode, nsub, flags, check)
                out["u"][t, m, a], out["qpos"][t, m, a], out["qvel"][t, m, a] = c, q, v
    out["ee"] = TS.oracle_ee(out["qpos"][..., :6].reshape(-1, 6)).reshape(T, n, L, 3)
    return out


def deviation(got, ref, rows=None):
    """largest |got - ref| of "u", "qpos", "qvel" and "ee" (over `rows`, a boolean problem mask, default all)"""
    rows = slice(None) if rows is None else rows
    return {name: float(np.abs(np.asarray(got[name], np.float64)[:, rows] - ref[name][:, rows]).max()) for name in ("u", "qpos", "qvel", "ee")}


# ---- family P: the iLQR problem of lqr_support.family_p --------------------------------------------------------------------------------------------------
P_ALPHAS = (0.0, 0.25, 1.0)
P_CLAMP = (-1.0, 1.0)
P_SHIFT = 0.02                                             # rad: the second set's nominal start, moved off the real one


def family_p(n, roll, derivatives, jacobian, lqr):
    """lqr_support.family_p's problem with its gains: 3 contact-free starts under F_CUBE_PINNED, T = 8, actions mode, the nominal rollout as the
    reference.  roll / derivatives / jacobian as there; lqr(problem) -> {"k", "K"}.  Returns the inputs of the query as float32 arrays."""
    c = TS.free_case("arm", "actions")
    q0, v0 = c["qpos"][:LS.P_M], c["qvel"][:LS.P_M]
    p, U = LS.family_p(n, roll, derivatives, jacobian)
    s = lqr(p)
    r = roll(U, q0, v0)
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    shifted = q0.copy(); shifted[:, :6] += np.float32(P_SHIFT)
    return {"u": f(U), "qpos_ref": f(r["qpos"]), "qvel_ref": f(r["qvel"]), "K": f(s["K"]), "k": f(s["k"]), "nx": n, "qpos": q0, "qvel": v0, "ref0": (shifted, v0.copy()),
            "mode": "actions", "nsub": LS.P_NSUB, "flags": scenes.FREE}


@functools.lru_cache(maxsize=None)
def family_p_cpu(n):
    """family_p from the host twins of the four queries (fp32, as the device computes them)"""
    import query_support as QS
    roll = lambda U, q, v: TS.twin(U, q, v, "actions", LS.P_NSUB, scenes.FREE, np.float32)
    der = lambda U, q, v: DS.twin(U, q, v, "actions", LS.P_NSUB, scenes.FREE, np.float32)
    jac = lambda q: QS.twin_jacobian(q, np.float32)["jacp"]
    return family_p(n, roll, der, jac, lambda p: LS.twin(p, np.float32))


def run_p(f, c, with_ref0, **kw):
    """f = twin or a wrapper of So100Sim.closed_loop with twin's signature, on a family_p()"""
    return f(c["u"], c["qpos_ref"], c["qvel_ref"], c["K"], c["k"], alphas=P_ALPHAS, nx=c["nx"], qpos=c["qpos"], qvel=c["qvel"], ref0=c["ref0"] if with_ref0 else None,
             mode=c["mode"], nsub=c["nsub"], flags=c["flags"], clamp=P_CLAMP, **kw)


@functools.lru_cache(maxsize=None)
def reference_p(n, with_ref0):
    c = family_p_cpu(n)
    return reference(c["u"], c["qpos_ref"], c["qvel_ref"], c["K"], c["k"], P_ALPHAS, n, c["qpos"], c["qvel"], c["ref0"] if with_ref0 else None, c["mode"], c["nsub"],
                     c["flags"], P_CLAMP)


# ---- family G: synthetic gains on trajectory_support.free_case ------------------------------------------------------------------------------------------
G_ALPHAS = (0.0, 0.5, 1.0)
G_SEED = 4
G_K_SCALE = {"actions": 0.2, "targets": 0.03}                # k in the size of a control of that mode (free_case's targets stay within 0.15 rad of the start)


def pd_gains(T, n, nx, seed, noise=0.05, k_scale=0.2):
    """K [T, n, 6, nx]: -2 on the joint's own position column, -0.1 on its velocity column, noise * N elsewhere; k [T, n, 6] = k_scale * N -- float32"""
    rng = np.random.default_rng(seed)
    K = noise*rng.standard_normal((T, n, NU, nx))
    for j in range(NU):
        K[..., j, j] = -2.0; K[..., j, nx//2 + j] = -0.1
    return K.astype(np.float32), (k_scale*rng.standard_normal((T, n, NU))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def family_g(name, mode):
    """free_case(name, mode)'s 65 starts and controls, T = 3, nx = 24, pd_gains.  The reference plan is the oracle's open-loop rollout MOVED by a
    seeded offset (arm 0.02 rad, cube 5 mm and a rotation of about 0.1 rad, velocities 0.05), and ref0 the start moved likewise, so that every
    tangent row -- the cube's and the quaternion difference among them -- carries a difference of a size fp32 rounding cannot hide.  Asserted on
    the oracle alone: no rollout of the reference touches anything with the arm (free_case's rule, every contact flag on)."""
    c = TS.free_case(name, mode)
    T, n = TS.FREE_T, TS.FREE_M
    rng = np.random.default_rng(G_SEED)

    def moved(qp, qv):
        qp, qv = np.array(qp, np.float64), np.array(qv, np.float64)
        qp[..., :6] += 0.02*rng.standard_normal(qp[..., :6].shape); qp[..., 6:9] += 0.005*rng.standard_normal(qp[..., 6:9].shape)
        rot = 0.05*rng.standard_normal(qp[..., 9:13].shape); rot[..., 0] = 1.0
        flat_q, flat_r = qp[..., 9:13].reshape(-1, 4), rot.reshape(-1, 4)
        for i in range(len(flat_q)):
            w = DS.quat_mul(flat_q[i], flat_r[i]); flat_q[i] = w/np.linalg.norm(w)
        qp[..., 9:13] = flat_q.reshape(qp[..., 9:13].shape)
        qv += 0.05*rng.standard_normal(qv.shape)
        return qp.astype(np.float32), qv.astype(np.float32)

    qref, vref = moved(c["ref"]["qpos"], c["ref"]["qvel"])
    ref0 = moved(c["qpos"], c["qvel"])
    K, k = pd_gains(T, n, 24, G_SEED + 1, k_scale=G_K_SCALE[mode])
    g = {"u": c["ctrl"], "qpos_ref": qref, "qvel_ref": vref, "K": K, "k": k, "nx": 24, "qpos": c["qpos"], "qvel": c["qvel"], "ref0": ref0, "mode": mode,
         "nsub": TS.FREE_NSUB, "flags": c["flags"]}
    clear = [True]

    def check(d):
        clear[0] = clear[0] and TS._no_arm_contact(d)
    g["ref"] = reference(g["u"], qref, vref, K, k, G_ALPHAS, 24, g["qpos"], g["qvel"], ref0, mode, g["nsub"], g["flags"], None, check)
    assert clear[0], "family G touches something with the arm: reseed it (G_SEED)"
    return g


def run_g(f, g, **kw):
    return f(g["u"], g["qpos_ref"], g["qvel_ref"], g["K"], g["k"], alphas=G_ALPHAS, nx=24, qpos=g["qpos"], qvel=g["qvel"], ref0=g["ref0"], mode=g["mode"], nsub=g["nsub"],
             flags=g["flags"], **kw)


# ---- the contact case: trajectory_support.warm_case under PD gains ----------------------------------------------------------------------------------------
W_ALPHAS = (0.0, 1.0)


W_SEED, W_SHIFT, W_K_SCALE = 0, 1e-3, 0.02


@functools.lru_cache(maxsize=None)
def warm_family():
    """warm_case()'s 48 problems (pads on the floor, REFP, T = 2, nsub = 4, actions), nx = 12, pd_gains without noise and k = W_K_SCALE * N.  The
    reference plan is the oracle's own rollout with its arm angles MOVED by W_SHIFT * N rad, and ref0 the start moved likewise, so both candidates
    feed K a difference rounding cannot hide and alpha = 1 adds k: a wrong gain term under contact shows.  "ref": the oracle under the numpy law.
    The controls move by some 1e-3 only, and it is asserted on the oracle alone that every substep of every candidate of a problem warm_case() keeps
    shows warm_case()'s (count, signature) and no knife-edge pose -- so that case's `keep` mask holds for every rollout here and nothing else is
    left out; a family that cannot meet this is reseeded (W_SEED), not masked."""
    import substep_harness as H
    from oracle import so100_oracle as O
    c = TS.warm_case()
    T, n, L = TS.WARM_T, len(c["qpos"]), len(W_ALPHAS)
    rng = np.random.default_rng(W_SEED)
    K, k = pd_gains(T, n, 12, W_SEED + 1, noise=0.0, k_scale=W_K_SCALE)
    qref = c["ref"]["qpos"].copy(); qref[..., :6] += W_SHIFT*rng.standard_normal(qref[..., :6].shape)
    q0ref = c["qpos"].astype(np.float64); q0ref[:, :6] += W_SHIFT*rng.standard_normal(q0ref[:, :6].shape)
    qref, vref, ref0 = qref.astype(np.float32), c["ref"]["qvel"].astype(np.float32), (q0ref.astype(np.float32), c["qvel"].copy())
    al = np.asarray(W_ALPHAS, np.float32).astype(np.float64)
    f64 = lambda a: a.astype(np.float64)
    ref = {"u": np.zeros((T, n, L, 6)), "qpos": np.zeros((T, n, L, 13)), "qvel": np.zeros((T, n, L, 12))}
    rs = np.random.RandomState(1)
    for i in range(n):
        for a in range(L):
            d = scenes.fresh(); O.arr(d.qpos)[:] = f64(c["qpos"][i]); O.arr(d.qvel)[:] = f64(c["qvel"][i])
            for t in range(T):
                xq, xv = (f64(ref0[0][i]), f64(ref0[1][i])) if t == 0 else (f64(qref[t - 1, i]), f64(vref[t - 1, i]))
                u = law(O.arr(d.qpos).copy(), O.arr(d.qvel).copy(), xq, xv, f64(c["ctrl"][t, i]), f64(k[t, i]), f64(K[t, i]), al[a], 12)
                O.arr(d.ctrl)[:] = O.arr(d.qpos)[:6] + TS.JS64*u
                for _ in range(TS.WARM_NSUB):
                    d0 = H.copy_data(d)
                    scenes.L.so100o_step(C.byref(scenes.M), C.byref(d), scenes.REFP, -1, 1)
                    if c["keep"][i]:
                        sm = H.oracle_contact_summary(d)
                        assert sm[:2] == (c["count"][i], c["sig"][i]) and not (sm[2] > 0 and H.knife_edge(d0, scenes.REFP, sm, rs)), \
                            f"problem {i}, candidate {a}: the law moved a kept problem's contact set: reseed (W_SEED) or shrink W_SHIFT / W_K_SCALE"
                ref["u"][t, i, a], ref["qpos"][t, i, a], ref["qvel"][t, i, a] = u, O.arr(d.qpos), O.arr(d.qvel)
    return {"u": c["ctrl"], "qpos_ref": qref, "qvel_ref": vref, "ref0": ref0, "K": K, "k": k, "nx": 12, "qpos": c["qpos"], "qvel": c["qvel"], "keep": c["keep"],
            "in_contact": c["in_contact"], "count": c["count"], "sig": c["sig"], "ref": ref}


def run_warm(f, w, **kw):
    return f(w["u"], w["qpos_ref"], w["qvel_ref"], w["K"], w["k"], alphas=W_ALPHAS, nx=12, qpos=w["qpos"], qvel=w["qvel"], ref0=w["ref0"], mode="actions",
             nsub=TS.WARM_NSUB, flags=scenes.REFP, solver_iters=TS.WARM_ITERS[0], contact_iters=TS.WARM_ITERS[1], **kw)


def warm_deviation(got, w):
    keep = w["keep"]
    return {name: float(np.abs(np.asarray(got[name], np.float64)[:, keep] - w["ref"][name][:, keep]).max()) for name in ("u", "qpos", "qvel")}


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------------------------
# fp64 twin against the reference: the same templates as the oracle's arithmetic up to the solvers' stopping (trajectory_support.FP64_ARM / FP64_CUBE
# are 1e-13 .. 1e-10 open loop), amplified by the gains over the horizon; orders of magnitude below fp32 rounding, so a wrong term cannot hide
FP64_BOUND = 1e-9
FP64_ITERS = (64, 64)
# The fp32 twin's largest deviation from the reference, measured by tests/test_closed_loop_cpu.py (which prints them as [cl-tol] lines and holds the
# twin to TWIN_FACTOR x these); the kernel is held to KERNEL_FACTOR x these.  "P": both nx, both reference sets, at the shipped (2, 20); "G": both
# flag sets and modes at (2, 20); "warm": the kept problems of warm_family() at (4, 30), measured as trajectory_support's "warm" record is.
FP32_MEASURED = {
    "P":    {"u": 3.5e-6, "qpos": 2.3e-7, "qvel": 1.8e-6, "ee": 6.5e-8},
    "G":    {"u": 4.1e-7, "qpos": 1.2e-7, "qvel": 2.8e-6, "ee": 8.3e-8},
    "warm": {"u": 8.9e-7, "qpos": 1.4e-7, "qvel": 9.2e-6},
}
TWIN_FACTOR, KERNEL_FACTOR = TS.TWIN_FACTOR, TS.KERNEL_FACTOR


def within(dev, family, factor):
    for name, d in dev.items():
        assert d <= factor*FP32_MEASURED[family][name], (family, name, d, factor*FP32_MEASURED[family][name])
