"""Shared by tests/test_cost_cpu.py and tests/test_gpu_cost.py: the host twin of the two cost queries (tests/_costcheck, built and loaded by
tests/hostlibs.py), the seeded cases, the numpy reference, the bounds and the exact properties both the twin and the kernels
are held to.

Cases need no physics: states are seeded arrays -- q uniform over the joint ranges, v in +-2 rad/s, the cube in a +-0.3 m box, u in +-1, targets in
a +-0.3 m box -- rounded to fp32 once and widened for the reference.

Reference.  numpy fp64 written from the formulas of include/so100_query.h over query_support.oracle_point / oracle_jacobian (the oracle's FK and
mj_jac's formula); it is not a second instantiation of so100_cost.hpp.  Computed once per process and never modified.

A `terms` callable is f(cost, qpos [T, M, 13], qvel [T, M, 12] or None, u [T, M, 6], target, nx) -> {"lx", "lxx", "lu", "luu"}; a `select` callable is
f(cost, qpos [T, M, L, 13], qvel, u [T, M, L, 6], target, bad_step=None, u_fallback=None) -> {"cost", "best", "best_cost", "u_best"}; numpy in and out.
`cost` is a dict of So100Sim.cost_terms' cost arguments (cost_def())."""
import functools

import numpy as np

import query_support as QS
from hostlibs import costcheck, ptr

TARGETS = {"fixed": 0, "traj": 1, "cube": 2}
IDX = {24: np.arange(24), 12: np.r_[0:6, 12:18]}           # nx -> the tangent indices of the form
MAX_L = 16


# ---- the cost definition -----------------------------------------------------------------------------------------------------------------------------
def cost_def(target_mode="cube", link=QS.EE_LINK, offset=None, w_point=1.0, w_q=0.0, q_nom=0.0, w_v=0.0, w_u=0.0, w_terminal=1.0):
    six = lambda w: tuple(float(np.float32(x)) for x in (np.full(6, w) if np.isscalar(w) else w))
    return {"target_mode": target_mode, "link": link, "offset": None if offset is None else tuple(float(np.float32(x)) for x in offset),
            "w_point": float(np.float32(w_point)), "w_q": six(w_q), "q_nom": six(q_nom), "w_v": six(w_v), "w_u": six(w_u), "w_terminal": float(np.float32(w_terminal))}


def point_offset(cost):
    """the offset the header's NULL stands for: the end-effector point on link 4, the frame origin elsewhere"""
    if cost["offset"] is not None:
        return np.asarray(cost["offset"], np.float64)
    return QS.EE_LOCAL if cost["link"] == QS.EE_LINK else np.zeros(3)


def packed(cost, dtype):
    """costcheck.cpp's 29 numbers"""
    return np.concatenate([point_offset(cost), [cost["w_point"]], cost["w_q"], cost["q_nom"], cost["w_v"], cost["w_u"], [cost["w_terminal"]]]).astype(dtype)


ZEROS_IN = (0.1, 0.2, 0.0, 0.05, 0.3, 0.0)                   # a weight vector with zeros in it
Q_NOM = (0.1, -0.8, 0.9, 0.3, -0.2, 0.15)
W_U = (0.01, 0.02, 0.01, 0.03, 0.01, 0.0)
OFFSET2 = (0.01, -0.02, 0.03)
COSTS = {
    "cube-ee":   cost_def("cube", w_point=1.5, w_q=ZEROS_IN, q_nom=Q_NOM, w_v=0.01, w_u=W_U, w_terminal=2.5),
    "fixed-ee":  cost_def("fixed", w_point=1.0, w_q=0.05, q_nom=Q_NOM, w_v=ZEROS_IN, w_u=W_U, w_terminal=0.5),
    "traj-ee":   cost_def("traj", w_point=2.0, w_q=ZEROS_IN, q_nom=0.0, w_v=0.02, w_u=0.01, w_terminal=4.0),
    "cube-l2":   cost_def("cube", 2, OFFSET2, w_point=1.0, w_q=0.05, q_nom=Q_NOM, w_v=ZEROS_IN, w_u=W_U, w_terminal=3.0),
    "fixed-l2":  cost_def("fixed", 2, OFFSET2, w_point=1.5, w_q=ZEROS_IN, q_nom=Q_NOM, w_v=0.01, w_u=W_U, w_terminal=2.5),
    "traj-l2":   cost_def("traj", 2, OFFSET2, w_point=0.7, w_q=0.1, q_nom=Q_NOM, w_v=0.01, w_u=0.02, w_terminal=0.0),
}
ALL_ZERO = {mode: cost_def(mode, w_point=0.0, q_nom=Q_NOM, w_terminal=2.0) for mode in TARGETS}


# ---- the twin --------------------------------------------------------------------------------------------------------------------------------------------
def _as(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def twin_terms(cost, qpos, qvel, u, target, nx, dtype=np.float32):
    q, v, uu, tg, w = _as(qpos, dtype), _as(qvel, dtype), _as(u, dtype), _as(target, dtype), packed(cost, dtype)
    T, M = uu.shape[0], uu.shape[1]
    assert q.shape == (T, M, 13) and (v is None or v.shape == (T, M, 12)) and uu.shape == (T, M, 6)
    assert tg is None or tg.shape == ((M, 3) if cost["target_mode"] == "fixed" else (T, M, 3))
    out = {"lx": np.zeros((T + 1, M, nx), dtype), "lxx": np.zeros((T + 1, M, nx, nx), dtype), "lu": np.zeros((T, M, 6), dtype), "luu": np.zeros((T, M, 6, 6), dtype)}
    fn = costcheck().ck_terms_d if np.dtype(dtype) == np.float64 else costcheck().ck_terms_f
    fn(M, T, nx, cost["link"], TARGETS[cost["target_mode"]], ptr(w), ptr(tg), ptr(q), ptr(v), ptr(uu), *[ptr(out[k]) for k in ("lx", "lxx", "lu", "luu")])
    return out


def twin_select(cost, qpos, qvel, u, target, bad_step=None, u_fallback=None, dtype=np.float32):
    q, v, uu, tg, fb, w = _as(qpos, dtype), _as(qvel, dtype), _as(u, dtype), _as(target, dtype), _as(u_fallback, dtype), packed(cost, dtype)
    bs = None if bad_step is None else np.ascontiguousarray(bad_step, np.int32)
    T, M, L = uu.shape[0], uu.shape[1], uu.shape[2]
    assert q.shape == (T, M, L, 13) and (v is None or v.shape == (T, M, L, 12)) and (bs is None or bs.shape == (M, L)) and (fb is None or fb.shape == (T, M, 6))
    out = {"cost": np.zeros((M, L), dtype), "best": np.zeros(M, np.int32), "best_cost": np.zeros(M, dtype), "u_best": np.zeros((T, M, 6), dtype)}
    fn = costcheck().ck_select_d if np.dtype(dtype) == np.float64 else costcheck().ck_select_f
    fn(M, T, L, cost["link"], TARGETS[cost["target_mode"]], ptr(w), ptr(tg), ptr(q), ptr(v), ptr(uu), ptr(bs), ptr(fb),
       *[ptr(out[k]) for k in ("cost", "best", "best_cost", "u_best")])
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------
TERMS_M, TERMS_T = (1, 3, 65, 130), (1, 3)
SELECT_L, SELECT_M, SELECT_T = (1, 3, 8, 16), (1, 3, 65), 3


def seeded_states(shape, seed):
    """float32 qpos [*shape, 13], qvel [*shape, 12], u [*shape, 6]"""
    rs = np.random.RandomState(seed)
    r = QS.joint_range()
    qpos = np.zeros(shape + (13,)); qvel = rs.uniform(-2.0, 2.0, shape + (12,))
    qpos[..., :6] = rs.uniform(r[:, 0], r[:, 1], shape + (6,))
    qpos[..., 6:9] = rs.uniform(-0.3, 0.3, shape + (3,))
    qpos[..., 9] = 1.0
    return qpos.astype(np.float32), qvel.astype(np.float32), rs.uniform(-1.0, 1.0, shape + (6,)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def terms_case():
    """the largest shape, T = 3 and M = 130; a smaller case is its [:T, :M] corner (a problem's bits do not depend on M or its place)"""
    qpos, qvel, u = seeded_states((3, 130), 11)
    rs = np.random.RandomState(12)
    return {"qpos": qpos, "qvel": qvel, "u": u, "fixed": rs.uniform(-0.3, 0.3, (130, 3)).astype(np.float32), "traj": rs.uniform(-0.3, 0.3, (3, 130, 3)).astype(np.float32)}


def corner(c, T, M, mode):
    """(qpos, qvel, u, target) of the [:T, :M] corner of a terms_case() for a target mode"""
    tg = None if mode == "cube" else (c["fixed"][:M] if mode == "fixed" else c["traj"][:T, :M])
    return c["qpos"][:T, :M], c["qvel"][:T, :M], c["u"][:T, :M], tg


@functools.lru_cache(maxsize=None)
def select_case(L, M):
    qpos, qvel, u = seeded_states((SELECT_T, M, L), 100*L + M)
    rs = np.random.RandomState(7 + 100*L + M)
    return {"qpos": qpos, "qvel": qvel, "u": u, "fixed": rs.uniform(-0.3, 0.3, (M, 3)).astype(np.float32),
            "traj": rs.uniform(-0.3, 0.3, (SELECT_T, M, 3)).astype(np.float32), "fallback": rs.uniform(-1.0, 1.0, (SELECT_T, M, 6)).astype(np.float32)}


def select_args(c, mode):
    return c["qpos"], c["qvel"], c["u"], (None if mode == "cube" else c[mode])


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
def f64(a):
    return None if a is None else np.asarray(a, np.float32).astype(np.float64)


def _targets(cost, qpos, target):
    """g [..., 3] for state rows qpos [T, M, (L,) 13]; fixed and traj targets are per problem"""
    mode = cost["target_mode"]
    if mode == "cube":
        return qpos[..., 6:9]
    g = target[None] if mode == "fixed" else target         # [1 or T, M, 3]
    if qpos.ndim == 4:
        g = g[:, :, None]
    return np.broadcast_to(g, qpos.shape[:-1] + (3,))


def ref_state_cost(cost, q, v, g, point=None):
    """s [...] in fp64 for q, v [..., 6], g [..., 3]"""
    p = QS.oracle_point(q.reshape(-1, 6), cost["link"], point_offset(cost)).reshape(q.shape[:-1] + (3,)) if point is None else point
    r = p - g
    return cost["w_point"]*(r**2).sum(-1) + (np.asarray(cost["w_q"])*(q - np.asarray(cost["q_nom"]))**2).sum(-1) + (np.asarray(cost["w_v"])*v**2).sum(-1)


def sigma(cost, T):
    s = np.ones(T); s[T - 1] = cost["w_terminal"]
    return s


def reference_terms(cost, qpos, qvel, u, target, nx):
    """{"lx" [T + 1, M, nx], "lxx", "lu", "luu"} in fp64 from float32 inputs"""
    qpos, qvel, u, target = f64(qpos), f64(qvel), f64(u), f64(target)
    T, M = u.shape[:2]
    q, v = qpos[..., :6], (np.zeros((T, M, 6)) if qvel is None else qvel[..., :6])
    off = point_offset(cost)
    p = QS.oracle_point(q.reshape(-1, 6), cost["link"], off).reshape(T, M, 3)
    J = QS.oracle_jacobian(q.reshape(-1, 6), cost["link"], off)["jacp"].reshape(T, M, 3, 6)
    r = p - _targets(cost, qpos, target)
    two_sigma = 2.0*sigma(cost, T)[:, None]
    wp, wq, wv, wu = cost["w_point"], np.asarray(cost["w_q"]), np.asarray(cost["w_v"]), np.asarray(cost["w_u"])
    lx, lxx = np.zeros((T + 1, M, 24)), np.zeros((T + 1, M, 24, 24))
    lx[1:, :, :6] = two_sigma[..., None]*(wp*np.einsum("tmak,tma->tmk", J, r) + wq*(q - np.asarray(cost["q_nom"])))
    lx[1:, :, 12:18] = two_sigma[..., None]*(wv*v)
    lxx[1:, :, :6, :6] = two_sigma[..., None, None]*(wp*np.einsum("tmai,tmaj->tmij", J, J) + np.diag(wq))
    lxx[1:, :, 12:18, 12:18] = two_sigma[..., None, None]*np.diag(wv)
    if cost["target_mode"] == "cube":
        lx[1:, :, 6:9] = -two_sigma[..., None]*wp*r
        lxx[1:, :, :6, 6:9] = -two_sigma[..., None, None]*wp*J.transpose(0, 1, 3, 2)
        lxx[1:, :, 6:9, :6] = -two_sigma[..., None, None]*wp*J
        lxx[1:, :, 6:9, 6:9] = two_sigma[..., None, None]*wp*np.eye(3)
    i = IDX[nx]
    return {"lx": lx[..., i], "lxx": lxx[..., i, :][..., i], "lu": 2.0*wu*u, "luu": np.broadcast_to(np.diag(2.0*wu), (T, M, 6, 6)).copy()}


def reference_lx_by_differences(cost, qpos, qvel, target, h=1e-6):
    """central differences of the reference's OWN s over the 24 tangent directions the cost can see (q, the cube's position, the arm's v): lx rows 1..T"""
    qpos, qvel, target = f64(qpos), f64(qvel), f64(target)
    T, M = qpos.shape[:2]
    s = lambda qp, qv: ref_state_cost(cost, qp[..., :6], qv[..., :6], _targets(cost, qp, target))
    lx = np.zeros((T, M, 24))
    for k in list(range(9)) + list(range(12, 18)):
        d = np.zeros(13 if k < 12 else 12); d[k if k < 12 else k - 12] = h
        lx[..., k] = (s(qpos + d, qvel) - s(qpos - d, qvel))/(2*h) if k < 12 else (s(qpos, qvel + d) - s(qpos, qvel - d))/(2*h)
    return sigma(cost, T)[:, None, None]*lx


def reference_select(cost, qpos, qvel, u, target, bad_step=None):
    """{"cost" [M, L] (+inf where bad_step >= 0), "best" [M], "best_cost" [M], "gap" [M]: the two smallest costs' distance (inf with one candidate)}"""
    qpos, qvel, u, target = f64(qpos), f64(qvel), f64(u), f64(target)
    T, M, L = u.shape[:3]
    v = np.zeros((T, M, L, 6)) if qvel is None else qvel[..., :6]
    s = ref_state_cost(cost, qpos[..., :6], v, _targets(cost, qpos, target))
    c = (np.asarray(cost["w_u"])*u**2).sum(-1)
    J = (c + sigma(cost, T)[:, None, None]*s).sum(0)
    if bad_step is not None:
        J = np.where(np.asarray(bad_step) >= 0, np.inf, J)
    order = np.sort(J, axis=1)
    with np.errstate(invalid="ignore"):
        gap = order[:, 1] - order[:, 0] if L > 1 else np.full(M, np.inf)
    best = np.where(np.isinf(order[:, 0]), -1, J.argmin(1))
    return {"cost": J, "best": best, "best_cost": order[:, 0], "gap": np.where(np.isnan(gap), np.inf, gap)}


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------------------
# two fp64 formulations of a query: the project's figure
FP64_BOUND = 1e-12
FD_BOUND = 1e-8                                              # lx against central differences at h = 1e-6, like jacp in DESIGN.md 11.3
# The fp32 twin's largest deviation from the reference per output over every case of tests/test_cost_cpu.py (which prints them as [cost-tol] lines and
# holds the twin to TWIN_FACTOR x these); the kernels are held to KERNEL_FACTOR x these: the project's margin for contraction and the device reciprocal.
FP32_MEASURED = {"lx": 8.0e-7, "lxx": 1.0e-6, "lu": 1.9e-9, "cost": 5.5e-6}
TWIN_FACTOR, KERNEL_FACTOR = 1.05, 3.0
KNIFE_EDGE = 4.0                                             # x the fp32 cost bound: closer candidates are left out of the `best` comparison
KNIFE_EDGE_SHARE = 0.01                                      # at most this share of the problems may be left out
KNIFE_EDGE_COUNT = 0                                         # how many of the seeded select problems the reference alone leaves out (test_cost_cpu.py)


def terms_deviation(got, ref):
    return {k: float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()) for k in ("lx", "lxx", "lu")} | \
           {"luu": float(np.abs(np.asarray(got["luu"], np.float64) - ref["luu"]).max())}


def comparable(ref, factor=KERNEL_FACTOR):
    """the problems whose `best` is compared: the reference's two smallest costs at least KNIFE_EDGE x the fp32 cost bound apart"""
    return ref["gap"] >= KNIFE_EDGE*factor*FP32_MEASURED["cost"]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- exact properties, of the twin and of the kernels alike ----------------------------------------------------------------------------------------------
def check_terms_exact(terms, cost, T, M, dtype=np.float32):
    """row 0 zero; lxx its own transpose; zero outside the documented blocks; n = 12 the picked n = 24; a second call the same bits.  Returns the n = 24 result."""
    qpos, qvel, u, tg = corner(terms_case(), T, M, cost["target_mode"])
    full, arm = terms(cost, qpos, qvel, u, tg, 24), terms(cost, qpos, qvel, u, tg, 12)
    again = terms(cost, qpos, qvel, u, tg, 24)
    for k in ("lx", "lxx", "lu", "luu"):
        assert bits(full[k]) == bits(again[k]), k
        assert np.isfinite(full[k]).all(), k
    assert not full["lx"][0].any() and not full["lxx"][0].any() and not arm["lx"][0].any() and not arm["lxx"][0].any()
    assert bits(full["lxx"]) == bits(np.swapaxes(full["lxx"], -1, -2))
    i = IDX[12]
    assert bits(arm["lx"]) == bits(full["lx"][..., i]) and bits(arm["lxx"]) == bits(full["lxx"][..., i, :][..., i])
    assert bits(arm["lu"]) == bits(full["lu"]) and bits(arm["luu"]) == bits(full["luu"])
    mask = np.zeros((24, 24), bool)
    mask[:6, :6] = True; mask[np.arange(12, 18), np.arange(12, 18)] = True
    if cost["target_mode"] == "cube":
        mask[:6, 6:9] = mask[6:9, :6] = True; mask[np.arange(6, 9), np.arange(6, 9)] = True
    assert not full["lxx"][..., ~mask].any()
    lxm = np.zeros(24, bool); lxm[:6] = lxm[12:18] = True; lxm[6:9] = cost["target_mode"] == "cube"
    assert not full["lx"][..., ~lxm].any()
    assert not full["luu"][..., ~np.eye(6, dtype=bool)].any()
    link = cost["link"]                                       # the joints behind the link do not move the point: only w_q is left of their rows
    for k in range(link + 1, 6):
        off = np.ones(24, bool); off[k] = False
        assert not full["lxx"][:, :, k, off].any(), k
    return full


def check_terms_zero_weights(terms, T=3, M=65):
    c = terms_case()
    for mode, cost in ALL_ZERO.items():
        for nx in (12, 24):
            got = terms(cost, *corner(c, T, M, mode), nx)
            for k in ("lx", "lxx", "lu", "luu"):
                assert not got[k].any(), (mode, nx, k)


def check_terms_place(terms, cost, nx=24):
    """a problem's bits depend neither on M nor on its place in the batch"""
    c = terms_case()
    mode = cost["target_mode"]
    full = terms(cost, *corner(c, 3, 130, mode), nx)
    for M, sl in ((1, slice(129, 130)), (3, slice(63, 66)), (65, slice(40, 105))):
        tg = None if mode == "cube" else (c["fixed"][sl] if mode == "fixed" else c["traj"][:, sl])
        part = terms(cost, c["qpos"][:, sl], c["qvel"][:, sl], c["u"][:, sl], tg, nx)
        for k in ("lx", "lxx", "lu", "luu"):
            assert bits(part[k]) == bits(full[k][:, sl]), (k, M)
    # a shorter horizon: the rows before the last are the same where w_terminal is the only difference at the new last row
    short = terms(cost, *corner(c, 1, 130, mode), nx)
    assert bits(short["lu"]) == bits(full["lu"][:1]) and bits(short["luu"]) == bits(full["luu"][:1])


def check_terms_non_finite(terms, cost, nx=24):
    """a NaN in one qpos entry: that (step, problem)'s lx and lxx are NaN, all of them, and nothing else changes; likewise lu and luu for a bad u"""
    c = terms_case()
    qpos, qvel, u, tg = corner(c, 3, 65, cost["target_mode"])
    clean = terms(cost, qpos, qvel, u, tg, nx)
    q2, u2 = qpos.copy(), u.copy()
    q2[1, 64, 2] = np.nan; u2[2, 7, 4] = np.inf
    got = terms(cost, q2, qvel, u2, tg, nx)
    assert np.isnan(got["lx"][2, 64]).all() and np.isnan(got["lxx"][2, 64]).all() and np.isnan(got["lu"][2, 7]).all() and np.isnan(got["luu"][2, 7]).all()
    for k, (t, m) in (("lx", (2, 64)), ("lxx", (2, 64)), ("lu", (2, 7)), ("luu", (2, 7))):
        a, b = got[k].copy(), clean[k].copy()
        a[t, m] = 0; b[t, m] = 0
        assert bits(a) == bits(b), k
    v2 = qvel.copy(); v2[0, 3, 5] = np.nan
    got = terms(cost, qpos, v2, u, tg, nx)
    assert np.isnan(got["lx"][1, 3]).all() and np.isnan(got["lxx"][1, 3]).all() and np.isfinite(np.delete(got["lx"], 3, axis=1)).all()


def check_select_exact(select, cost, L=8, M=65):
    """ties, best_cost <= every cost, independence of L and place, the fallback, a failed cheapest candidate, a NaN"""
    c = select_case(L, M)
    qpos, qvel, u, tg = (a.copy() if a is not None else None for a in select_args(c, cost["target_mode"]))
    qpos[:, :, 5], qvel[:, :, 5], u[:, :, 5] = qpos[:, :, 2], qvel[:, :, 2], u[:, :, 2]      # candidate 5 is candidate 2 again
    got = select(cost, qpos, qvel, u, tg, u_fallback=c["fallback"])
    again = select(cost, qpos, qvel, u, tg, u_fallback=c["fallback"])
    for k in got:
        assert bits(got[k]) == bits(again[k]), k
    assert bits(got["cost"][:, 5]) == bits(got["cost"][:, 2]) and np.isfinite(got["cost"]).all()
    assert (got["best"] != 5).all() and (got["best"] >= 0).all()
    assert (got["best_cost"][:, None] <= got["cost"]).all()
    env = np.arange(M)
    u, fallback = np.asarray(u, got["u_best"].dtype), np.asarray(c["fallback"], got["u_best"].dtype)      # (the fp64 twin widens: the same values)
    assert bits(got["best_cost"]) == bits(got["cost"][env, got["best"]])
    assert (got["best"] == np.argmin(got["cost"], axis=1)).all()                 # numpy's argmin takes the first of equals too
    assert bits(got["u_best"]) == bits(u[:, env, got["best"]])
    tied = got["best"] == 2
    assert tied.any(), "no problem's cheapest candidate is the doubled one: reseed"
    # a candidate's cost depends neither on L nor on its place, nor a problem's on M
    first = select(cost, qpos[:, :, :3], qvel[:, :, :3], u[:, :, :3], tg)
    assert bits(first["cost"]) == bits(got["cost"][:, :3])
    rev = select(cost, qpos[:, :, ::-1], qvel[:, :, ::-1], u[:, :, ::-1], tg)
    assert bits(rev["cost"][:, ::-1]) == bits(got["cost"])
    assert (rev["best"][tied] == L - 1 - 5).all()                                # the doubled pair reversed: the lower index is now the other one
    sl = slice(31, 34)
    sub_tg = None if tg is None else (tg[sl] if cost["target_mode"] == "fixed" else tg[:, sl])
    sub = select(cost, qpos[:, sl], qvel[:, sl], u[:, sl], sub_tg, u_fallback=c["fallback"][:, sl])
    for k in ("cost", "best", "best_cost"):
        assert bits(sub[k]) == bits(got[k][sl]), k
    assert bits(sub["u_best"]) == bits(got["u_best"][:, sl])
    # every candidate of problem 4 failed: the fallback (NaN without one); the neighbours untouched
    bad = np.full((M, L), -1, np.int32); bad[4] = 1
    for fb in (c["fallback"], None):
        f = select(cost, qpos, qvel, u, tg, bad_step=bad, u_fallback=fb)
        assert f["best"][4] == -1 and np.isposinf(f["best_cost"][4]) and np.isposinf(f["cost"][4]).all()
        assert bits(f["u_best"][:, 4]) == bits(fallback[:, 4]) if fb is not None else np.isnan(f["u_best"][:, 4]).all()
        keep = env != 4
        assert bits(f["cost"][keep]) == bits(got["cost"][keep]) and bits(f["best"][keep]) == bits(got["best"][keep]) and bits(f["u_best"][:, keep]) == bits(got["u_best"][:, keep])
    # only the cheapest failed: the second cheapest wins (of equal ones the lowest)
    bad = np.full((M, L), -1, np.int32); bad[env, got["best"]] = 0
    f = select(cost, qpos, qvel, u, tg, bad_step=bad, u_fallback=c["fallback"])
    masked = np.where(bad >= 0, np.inf, got["cost"]).astype(got["cost"].dtype)
    assert (f["best"] == np.argmin(masked, axis=1)).all() and bits(f["cost"]) == bits(masked) and bits(f["u_best"]) == bits(u[:, env, f["best"]])
    # a NaN in one qpos entry: that rollout's cost is +inf, nothing else moves
    q2 = qpos.copy(); q2[1, 9, 3, 1] = np.nan
    f = select(cost, q2, qvel, u, tg)
    assert np.isposinf(f["cost"][9, 3])
    a, b = f["cost"].copy(), got["cost"].copy(); a[9, 3] = b[9, 3] = 0
    assert bits(a) == bits(b)
