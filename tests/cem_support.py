"""Shared by tests/test_cem_cpu.py and tests/test_gpu_cem.py: the host twin of the two cross-entropy planner queries (tests/_cemcheck, built and
loaded by tests/hostlibs.py), the cases, the numpy reference, the bounds and the exact properties both the twin and the kernels
are held to.

Cases need no physics: the rollouts are mppi_support.blend_case's seeded states and controls, the old plans mppi_support.sample_case's, the old sigmas
seeded here; everything is rounded to fp32 once and widened for the reference.

Reference.  numpy fp64 written from the formulas of include/so100_query.h: the costs from cost_support.reference_select, the order from np.lexsort over
(k, J), the elites as a mask, plain sums over it, the noise from mppi_support.reference_eps.  It is not a second instantiation of so100_cem.hpp.  The
statistics are compared on the elite set the code under test chose (reference_refit_on), after that set has been held to its own costs exactly and to
the reference's costs within twice the cost bound (check_elites): a near-tie at the boundary can neither hide nor fake a deviation.

A `sample` callable is mppi_support's with sigma [T, N, 6]; a `refit` callable is f(cost, qpos [T, N, K, 13], qvel, u [T, N, K, 6], target, E, alpha=0.0,
plan=None, sigma=None [T, N, 6], sigma_min=, sigma_max=, sigma_init= [6], bad_step=None [N, K], u_fallback=None [T, N, 6], shift=0, tail="zero") ->
{"cost" [N, K], "best", "best_cost" [N], "elite" [N, E], "n_elite", "threshold" [N], "mean", "sigma_out" [T, N, 6], "u_first" [N, 6]}; numpy in and out."""
import functools

import numpy as np

import cost_support as CS
import mppi_support as MS
from hostlibs import cemcheck, ptr

OUTPUTS = ("cost", "best", "best_cost", "elite", "n_elite", "threshold", "mean", "sigma_out", "u_first")
PER_PROBLEM = ("cost", "best", "best_cost", "elite", "n_elite", "threshold", "u_first")        # outputs with the problem in axis 0; mean and sigma_out: axis 1
bits = CS.bits


# ---- the twin --------------------------------------------------------------------------------------------------------------------------------------------
def _as(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def twin_sample(plan, K, sigma, seed=0, draw=0, id_offset=0, u_lo=-1.0, u_hi=1.0, qpos=None, qvel=None, dtype=np.float32):
    p, sg, q, v = _as(plan, dtype), _as(sigma, dtype), _as(qpos, dtype), _as(qvel, dtype)
    T, N = p.shape[:2]
    assert p.shape == (T, N, 6) and sg.shape == (T, N, 6) and (q is None or q.shape == (N, 13)) and (v is None or v.shape == (N, 12))
    out = {"ctrl": np.zeros((T, N, K, 6), dtype), "qpos": None if q is None else np.zeros((N, K, 13), dtype), "qvel": None if v is None else np.zeros((N, K, 12), dtype)}
    fn = cemcheck().cm_sample_d if np.dtype(dtype) == np.float64 else cemcheck().cm_sample_f
    fn(N, K, T, ptr(p), ptr(sg), float(dtype(u_lo)), float(dtype(u_hi)), seed, draw, id_offset, ptr(q), ptr(v), ptr(out["ctrl"]), ptr(out["qpos"]), ptr(out["qvel"]))
    return {k: a for k, a in out.items() if a is not None}


def six(x, dtype=np.float32):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float32), (6,)), dtype)


def twin_refit(cost, qpos, qvel, u, target, E, alpha=0.0, plan=None, sigma=None, sigma_min=0.0, sigma_max=1.0, sigma_init=0.5, bad_step=None, u_fallback=None,
               shift=0, tail="zero", dtype=np.float32):
    q, v, uu, tg, fb, w = _as(qpos, dtype), _as(qvel, dtype), _as(u, dtype), _as(target, dtype), _as(u_fallback, dtype), CS.packed(cost, dtype)
    pl, sg = _as(plan, dtype), _as(sigma, dtype)
    bs = None if bad_step is None else np.ascontiguousarray(bad_step, np.int32)
    T, N, K = uu.shape[:3]
    assert q.shape == (T, N, K, 13) and (v is None or v.shape == (T, N, K, 12)) and (bs is None or bs.shape == (N, K)) and 1 <= E <= K
    assert all(a is None or a.shape == (T, N, 6) for a in (fb, pl, sg)) and (alpha == 0 or (pl is not None and sg is not None))
    out = {"cost": np.zeros((N, K), dtype), "best": np.zeros(N, np.int32), "best_cost": np.zeros(N, dtype), "elite": np.zeros((N, E), np.int32), "n_elite": np.zeros(N, np.int32),
           "threshold": np.zeros(N, dtype), "mean": np.zeros((T, N, 6), dtype), "sigma_out": np.zeros((T, N, 6), dtype), "u_first": np.zeros((N, 6), dtype)}
    lo, hi, init = six(sigma_min, dtype), six(sigma_max, dtype), six(sigma_init, dtype)
    fn = cemcheck().cm_refit_d if np.dtype(dtype) == np.float64 else cemcheck().cm_refit_f
    fn(N, T, K, cost["link"], CS.TARGETS[cost["target_mode"]], ptr(w), ptr(tg), ptr(q), ptr(v), ptr(uu), ptr(bs), ptr(fb), E, float(np.float32(alpha)), ptr(pl), ptr(sg),
       ptr(lo), ptr(hi), ptr(init), shift, MS.TAILS[tail], *[ptr(out[k]) for k in OUTPUTS])
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = MS.SHAPES                                           # K in {1, 3, 63, 64, 65, 256, 257, 1030} x N in {1, 3} x T in {1, 3}, (4096, 1, 1), N = 70 at K = 3
COST_NAMES = MS.COST_NAMES                                   # one cube target, one traj target
ALPHAS = (0.0, 0.25)
SIGMA_MIN = (0.01, 0.02, 0.0, 0.3, 0.05, 0.0)                # joint 3's interval is a point, joint 5's is [0, 0], joint 4's top lies below most deviations
SIGMA_MAX = (1.0, 0.5, 2.0, 0.3, 0.2, 0.0)
SIGMA_INIT = (0.5, 0.25, 0.0, 1.0, 0.5, 0.125)
LIMITS = dict(sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX, sigma_init=SIGMA_INIT)
SEED, DRAW, ID_OFFSET = MS.SEED, MS.DRAW, MS.ID_OFFSET


def elites_of(K):
    """E in {1, 2, ceil(K / 8), K - 1, K}, clipped to 1..K, each once"""
    return sorted({min(max(e, 1), K) for e in (1, 2, -(-K//8), K - 1, K)})


@functools.lru_cache(maxsize=None)
def old_case(N, T):
    """the old mean (mppi_support's plan, some entries beyond the bounds) and the old sigma"""
    rs = np.random.RandomState(900 + 10*N + T)
    return {"plan": MS.sample_case(N, T)["plan"], "sigma": rs.uniform(0.05, 0.6, (T, N, 6)).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def entry_sigma(N, T):
    """a sigma per entry in [0, 1): every entry its own"""
    return np.random.RandomState(950 + 10*N + T).uniform(0.0, 1.0, (T, N, 6)).astype(np.float32)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_cost(name, K, N, T):
    cost = CS.COSTS[name]
    return CS.reference_select(cost, *MS.blend_args(MS.blend_case(K, N, T), cost["target_mode"]))["cost"]


def reference_order(J):
    """[N, K]: the candidates in ascending (J, k)"""
    J = np.asarray(J)
    return np.lexsort((np.broadcast_to(np.arange(J.shape[1]), J.shape), J), axis=1)


def shifted_sigma(sigma_new, shift, sigma_init):
    if not shift:
        return sigma_new
    last = np.broadcast_to(np.asarray(sigma_init, sigma_new.dtype), sigma_new[-1:].shape)
    return np.concatenate([sigma_new[1:], last])


def reference_refit_on(elite, n_elite, u, alpha, plan, sigma, sigma_min, sigma_max, sigma_init, shift, tail):
    """fp64 {"mean", "sigma_out" [T, N, 6], "u_first" [N, 6]} of the elite lists `elite` [N, E] (their first n_elite [N] slots); a problem without an elite:
    rows left at 0 -- the exact checks compare those to the fallback"""
    u = CS.f64(u)
    T, N, K = u.shape[:3]
    mask = np.zeros((N, K), bool)
    for n in range(N):
        mask[n, elite[n, :n_elite[n]]] = True
    m = mask[None, :, :, None]
    cnt = np.maximum(mask.sum(1), 1).astype(np.float64)[None, :, None]
    mu = np.where(m, u, 0.0).sum(2)/cnt
    sd = np.sqrt(np.where(m, (np.where(m, u, 0.0) - mu[:, :, None])**2, 0.0).sum(2)/cnt)
    a = float(np.float32(alpha))
    mean_new = a*CS.f64(plan) + (1.0 - a)*mu if a > 0 else mu
    sigma_new = np.clip(a*CS.f64(sigma) + (1.0 - a)*sd if a > 0 else sd, CS.f64(sigma_min), CS.f64(sigma_max))
    return {"mean": MS.shifted(mean_new, shift, tail), "sigma_out": shifted_sigma(sigma_new, shift, CS.f64(sigma_init)), "u_first": mean_new[0]}


def reference_sample(plan, K, sigma, seed=0, draw=0, id_offset=0, u_lo=-1.0, u_hi=1.0):
    """ctrl [T, N, K, 6] in fp64 from the float32 plan and the per-entry sigma [T, N, 6]"""
    plan, sigma = CS.f64(plan), CS.f64(sigma)
    T, N = plan.shape[:2]
    eps = MS.reference_eps(seed, draw, id_offset + np.arange(N), K, T).transpose(2, 0, 1, 3)        # [T, N, K, 6]
    eps[:, :, 0] = 0.0
    return np.clip(plan[:, :, None] + sigma[:, :, None]*eps, float(np.float32(u_lo)), float(np.float32(u_hi)))


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------------------
FP64_BOUND = 1e-12                                           # two fp64 formulations of a query: the project's figure
# The fp32 twin's largest deviation from the reference per output over every case of tests/test_cem_cpu.py (which prints them as [cem-tol] lines and holds the
# twin to TWIN_FACTOR x these); the kernels are held to KERNEL_FACTOR x these: the margin for the device's sqrt and division, and for exp, log and sincos in
# the sampler.  cost: the same code on the same cases as mppi_support's, so its record is that one.
FP32_MEASURED = {"ctrl": 8.9e-7, "cost": MS.FP32_MEASURED["cost"], "mean": 8.9e-8, "sigma_out": 8.5e-8, "u_first": 8.2e-8}
TWIN_FACTOR, KERNEL_FACTOR = 1.05, 3.0
# what the kernels gave on an MI355X (tests/test_gpu_cem.py prints them)
MEASURED = {"ctrl": 4.9e-7, "cost": 4.1e-6, "mean": 8.9e-8, "sigma_out": 8.5e-8, "u_first": 8.2e-8,
            "two rounds chained on physics against torch fp64 (cost, mean, sigma_out, u_first)": (6.3e-8, 5.1e-8, 6.2e-8, 3.0e-8),
            "cem_reach, 8 envs x 64 samples (8 elites) x T = 8, 3 rounds, 40 steps, final mean |cube - ee| in m (zero action: 0.4092)": 0.2149}
CTRL_DERIVED = 1.0*MS.NOISE_EPS + 2.0**-23                   # max(sigma) x the transform's error + 1 ulp of a control of size <= 2; entry_sigma() stays below 1


def cost_bound(dtype=np.float32, factor=TWIN_FACTOR):
    return FP64_BOUND if np.dtype(dtype) == np.float64 else factor*FP32_MEASURED["cost"]


def check_elites(got, J_ref, E, bound):
    """no problem is left out.  Exact against the costs the code under test returned: the elite list is the head of np.lexsort over (k, J), n_elite and
    threshold to the bit.  Valid against the reference's costs: every elite within, every other candidate beyond, the reference's E-th cost -+ 2 x bound"""
    J = got["cost"]
    N, K = J.shape
    order = reference_order(J)
    n_elite = np.minimum(E, np.isfinite(J).sum(1))
    assert (got["n_elite"] == n_elite).all() and got["elite"].shape == (N, E)
    want = np.where(np.arange(E)[None] < n_elite[:, None], order[:, :E], -1)
    assert (got["elite"] == want).all()
    rows = np.arange(N)
    last = J[rows, order[rows, np.maximum(n_elite, 1) - 1]]
    assert bits(got["threshold"]) == bits(np.where(n_elite > 0, last, np.inf).astype(J.dtype))
    assert (got["best"] == np.where(n_elite > 0, order[:, 0], -1)).all() and bits(got["best_cost"]) == bits(J[rows, order[:, 0]])
    edge = np.sort(J_ref, axis=1)[:, E - 1]
    mask = np.zeros((N, K), bool)
    for n in range(N):
        mask[n, got["elite"][n, :n_elite[n]]] = True
    with np.errstate(invalid="ignore"):
        assert (J_ref[mask] <= np.broadcast_to(edge[:, None], (N, K))[mask] + 2*bound).all()
        assert (J_ref[~mask] >= np.broadcast_to(edge[:, None], (N, K))[~mask] - 2*bound).all()


def refit_deviation(got, ref):
    some = got["n_elite"] > 0
    d = {k: float(np.abs(np.asarray(got[k], np.float64) - ref[k])[:, some].max(initial=0.0)) for k in ("mean", "sigma_out")}
    d["u_first"] = float(np.abs(np.asarray(got["u_first"], np.float64) - ref["u_first"])[some].max(initial=0.0))
    return d


def refit_deviations(refit, names=COST_NAMES, dtype=np.float32, factor=TWIN_FACTOR):
    """largest deviation per output over every shape x E x alpha x cost, the (shift, tail) pairs in turn; the elite set checked in each"""
    worst = {k: 0.0 for k in ("cost", "mean", "sigma_out", "u_first")}
    bound = cost_bound(dtype, factor)
    i = 0
    for name in names:
        cost = CS.COSTS[name]
        for K, N, T in SHAPES:
            args = MS.blend_args(MS.blend_case(K, N, T), cost["target_mode"])
            J_ref, old = reference_cost(name, K, N, T), old_case(N, T)
            for E in elites_of(K):
                for alpha in ALPHAS:
                    shift, tail = MS.shift_of(i); i += 1
                    got = refit(cost, *args, E, alpha=alpha, plan=old["plan"], sigma=old["sigma"], shift=shift, tail=tail, **LIMITS)
                    worst["cost"] = max(worst["cost"], float(np.abs(got["cost"].astype(np.float64) - J_ref).max()))
                    check_elites(got, J_ref, E, bound)
                    ref = reference_refit_on(got["elite"], got["n_elite"], args[2], alpha, old["plan"], old["sigma"], SIGMA_MIN, SIGMA_MAX, SIGMA_INIT, shift, tail)
                    d = refit_deviation(got, ref)
                    worst = {k: max(v, d.get(k, 0.0)) for k, v in worst.items()}
    return worst


def sample_deviation(sample, plain_sample):
    """at every shape: a broadcast sigma[j] gives plain_sample's bits (so100_query_plan_sample), the fan-out rows are the source's, and under a sigma per entry
    ctrl stays within the reference; returns the largest deviation"""
    worst = 0.0
    for K, N, T in SHAPES:
        c = MS.sample_case(N, T)
        kw = dict(seed=SEED, draw=DRAW, id_offset=ID_OFFSET, qpos=c["qpos"], qvel=c["qvel"])
        wide = np.broadcast_to(np.asarray(MS.SIGMA, np.float32), (T, N, 6))
        got, plain = sample(c["plan"], K, wide, **kw), plain_sample(c["plan"], K, MS.SIGMA, **kw)
        for k in ("ctrl", "qpos", "qvel"):
            assert bits(got[k]) == bits(plain[k]), (k, K, N, T)
        sg = entry_sigma(N, T)
        got = sample(c["plan"], K, sg, **kw)
        for k, w in (("qpos", 13), ("qvel", 12)):
            assert bits(got[k]) == bits(np.broadcast_to(c[k].astype(got[k].dtype)[:, None], (N, K, w))), (k, K, N, T)
        worst = max(worst, float(np.abs(got["ctrl"].astype(np.float64) - reference_sample(c["plan"], K, sg, SEED, DRAW, ID_OFFSET)).max()))
    return worst


# ---- exact properties, of the twin and of the kernels alike ----------------------------------------------------------------------------------------------
def check_sample_exact(sample, K=65, N=3, T=3):
    """a sigma of 0 perturbs nothing; a sigma that is negative, NaN or infinite gives NaN in the perturbed candidates of that entry and moves nothing else"""
    c = MS.sample_case(N, T)
    kw = dict(seed=SEED, draw=DRAW, id_offset=ID_OFFSET)
    sg = entry_sigma(N, T).copy()
    sg[0, 0, 1] = 0.0; sg[T - 1, N - 1, 4] = 0.0
    base = sample(c["plan"], K, sg, **kw)["ctrl"]
    assert bits(sample(c["plan"], K, sg, **kw)["ctrl"]) == bits(base) and np.isfinite(base).all()
    clamped = np.clip(c["plan"], -1.0, 1.0).astype(base.dtype)
    assert bits(base[:, :, 0]) == bits(clamped)
    for t, n, j in ((0, 0, 1), (T - 1, N - 1, 4)):
        assert bits(base[t, n, :, j]) == bits(np.full(K, clamped[t, n, j]))
    if K > 1:
        inside = (np.abs(c["plan"]) < 1.0) & (sg > 1e-3)
        assert (base.transpose(0, 1, 3, 2)[inside][:, 1:] != clamped[inside][:, None]).mean() > 0.99
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        s2 = sg.copy(); s2[T - 1, 0, 3] = bad
        g = sample(c["plan"], K, s2, **kw)["ctrl"]
        assert np.isnan(g[T - 1, 0, 1:, 3]).all() and bits(g[T - 1, 0, 0, 3]) == bits(clamped[T - 1, 0, 3])
        a, b = g.copy(), base.copy(); a[T - 1, 0, 1:, 3] = b[T - 1, 0, 1:, 3] = 0
        assert bits(a) == bits(b), bad
    for n in range(N):                                       # a problem's candidates depend on its global id and its own sigma alone
        one = sample(c["plan"][:, n:n + 1], K, sg[:, n:n + 1], seed=SEED, draw=DRAW, id_offset=ID_OFFSET + n)
        assert bits(one["ctrl"][:, 0]) == bits(base[:, n]), n


def check_refit_exact(refit, blend, name, K, N=3, T=3):
    """the properties of include/so100_query.h that hold to the bit.  blend: so100_query_cost_blend behind mppi_support's `blend` signature"""
    cost = CS.COSTS[name]
    c = MS.blend_case(K, N, T)
    qpos, qvel, u, tg = (a.copy() if a is not None else None for a in MS.blend_args(c, cost["target_mode"]))
    old, fb = old_case(N, T), c["fallback"]
    E = max(1, K//4)
    kw = dict(alpha=0.25, plan=old["plan"], sigma=old["sigma"], u_fallback=fb, **LIMITS)
    got = refit(cost, qpos, qvel, u, tg, E, **kw)
    again = refit(cost, qpos, qvel, u, tg, E, **kw)
    for k in OUTPUTS:
        assert bits(got[k]) == bits(again[k]), k
    f = got["cost"].dtype.type
    lo, hi, init = six(SIGMA_MIN, f), six(SIGMA_MAX, f), six(SIGMA_INIT, f)
    assert np.isfinite(got["cost"]).all() and (got["n_elite"] == E).all() and (got["sigma_out"] >= lo).all() and (got["sigma_out"] <= hi).all()
    check_elites(got, got["cost"].astype(np.float64), E, 0.0)
    mixed = blend(cost, qpos, qvel, u, tg, 1.0)
    for k in ("cost", "best", "best_cost"):
        assert bits(got[k]) == bits(mixed[k]), k
    assert bits(got["u_first"]) == bits(got["mean"][0])
    # the shift and the tails: rows 1..T-1 moved up, the mean's tail as in the blend, sigma_out's last row sigma_init
    for shift, tail in MS.SHIFTS:
        s = refit(cost, qpos, qvel, u, tg, E, shift=shift, tail=tail, **kw)
        for k in PER_PROBLEM:
            assert bits(s[k]) == bits(got[k]), (k, shift, tail)
        assert bits(s["mean"]) == bits(MS.shifted(got["mean"], shift, tail)) and bits(s["sigma_out"]) == bits(shifted_sigma(got["sigma_out"], shift, init)), (shift, tail)
    # a problem's bits depend neither on N nor on its place
    sl = slice(N - 1, N)
    sub = refit(cost, qpos[:, sl], qvel[:, sl], u[:, sl], None if tg is None else tg[:, sl], E, shift=1, tail="hold",
                **dict(kw, plan=old["plan"][:, sl], sigma=old["sigma"][:, sl], u_fallback=fb[:, sl]))
    full = refit(cost, qpos, qvel, u, tg, E, shift=1, tail="hold", **kw)
    for k in OUTPUTS:
        assert bits(sub[k]) == bits(full[k][sl] if k in PER_PROBLEM else full[k][:, sl]), k
    # every candidate of problem 0 failed: the shifted fallback (NaN without one), sigma_init in every row; the neighbours untouched
    bad = np.full((N, K), -1, np.int32); bad[0] = 1
    for fallback in (fb, None):
        for shift, tail in MS.SHIFTS:
            x = refit(cost, qpos, qvel, u, tg, E, bad_step=bad, shift=shift, tail=tail, **dict(kw, u_fallback=fallback))
            assert x["best"][0] == -1 and np.isposinf(x["best_cost"][0]) and np.isposinf(x["cost"][0]).all() and x["n_elite"][0] == 0 and np.isposinf(x["threshold"][0])
            assert (x["elite"][0] == -1).all() and bits(x["sigma_out"][:, 0]) == bits(np.broadcast_to(init, (T, 6)))
            if fallback is None:
                lost = MS.shifted(np.full((T, 1, 6), np.nan, f), shift, tail)
                assert bits(np.isnan(x["mean"][:, :1])) == bits(np.isnan(lost)) and not np.nan_to_num(x["mean"][:, 0]).any() and np.isnan(x["u_first"][0]).all()
            else:
                assert bits(x["mean"][:, 0]) == bits(MS.shifted(fb.astype(f), shift, tail)[:, 0]) and bits(x["u_first"][0]) == bits(fb[0, 0].astype(f))
            for k in OUTPUTS:
                want = got[k] if k in PER_PROBLEM else (MS.shifted(got[k], shift, tail) if k == "mean" else shifted_sigma(got[k], shift, init))
                assert bits(x[k][1:] if k in PER_PROBLEM else x[k][:, 1:]) == bits(want[1:] if k in PER_PROBLEM else want[:, 1:]), (k, shift, tail)
    # one elite: its controls are the mean to the bit, sd = 0 and sigma_out = sigma_min (alpha = 0), clamp(alpha sigma) (alpha > 0)
    one = refit(cost, qpos, qvel, u, tg, 1, **LIMITS)
    rows = np.arange(N)
    assert (one["n_elite"] == 1).all() and (one["elite"][:, 0] == one["best"]).all() and bits(one["threshold"]) == bits(one["best_cost"])
    assert bits(one["mean"]) == bits(u[:, rows, one["best"]].astype(f)) and bits(one["sigma_out"]) == bits(np.broadcast_to(lo, (T, N, 6)))
    one = refit(cost, qpos, qvel, u, tg, 1, **kw)
    a = f(np.float32(0.25))
    assert bits(one["sigma_out"]) == bits(np.clip(a*old["sigma"].astype(f) + (f(1) - a)*f(0), lo, hi).astype(f))
    if K == 1:
        return got
    # two bit-equal columns straddling the boundary: the lower index is the elite
    E2 = max(1, K//2)
    first = refit(cost, qpos, qvel, u, tg, E2, **kw)
    order = reference_order(first["cost"])
    q2, v2, u2 = qpos.copy(), qvel.copy(), u.copy()
    pairs = []
    for n in range(N):
        inside, outside = int(order[n, E2 - 1]), int(order[n, E2])
        k_lo, k_hi = min(inside, outside), max(inside, outside)
        for a2 in (q2, v2, u2):
            a2[:, n, k_lo] = a2[:, n, inside]; a2[:, n, k_hi] = a2[:, n, inside]
        pairs.append((k_lo, k_hi))
    tie = refit(cost, q2, v2, u2, tg, E2, **kw)
    for n, (k_lo, k_hi) in enumerate(pairs):
        assert bits(tie["cost"][n, k_lo]) == bits(tie["cost"][n, k_hi]) and tie["elite"][n, E2 - 1] == k_lo and k_hi not in tie["elite"][n]
        assert bits(tie["threshold"][n]) == bits(tie["cost"][n, k_lo])
    check_elites(tie, tie["cost"].astype(np.float64), E2, 0.0)
    # a failed rollout and one with a NaN state and NaN controls are never elites, even with E = K; every output stays finite; the neighbours untouched
    k_bad, k_nan = int(got["best"][1]), (int(got["best"][1]) + 1) % K
    bad = np.full((N, K), -1, np.int32); bad[1, k_bad] = 0
    q2, u2 = qpos.copy(), u.copy()
    q2[T - 1, 1, k_nan, 1] = np.nan; u2[:, 1, k_nan] = np.nan
    lost = 1 if k_bad == k_nan else 2
    for E3 in (E, K):
        ref3 = refit(cost, qpos, qvel, u, tg, E3, **kw)
        x = refit(cost, q2, qvel, u2, tg, E3, bad_step=bad, **kw)
        assert np.isposinf(x["cost"][1, [k_bad, k_nan]]).all() and k_bad not in x["elite"][1] and k_nan not in x["elite"][1]
        assert x["n_elite"][1] == min(E3, K - lost) and (x["elite"][1, x["n_elite"][1]:] == -1).all()
        if K > lost:
            assert all(np.isfinite(x[k]).all() for k in ("mean", "sigma_out", "u_first", "threshold", "best_cost"))
        keep = rows != 1
        for k in OUTPUTS:
            assert bits(x[k][keep] if k in PER_PROBLEM else x[k][:, keep]) == bits(ref3[k][keep] if k in PER_PROBLEM else ref3[k][:, keep]), k
    return got
