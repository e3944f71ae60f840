"""Shared by tests/test_mppi_cpu.py and tests/test_gpu_mppi.py: the host twin of the two sampling-planner queries (tests/_mppicheck, built and
loaded by tests/hostlibs.py), the seeded cases, the numpy reference, the bounds and the exact properties both the twin and
the kernels are held to.

Cases need no physics: states and controls are cost_support.seeded_states' arrays, plans uniform in +-1.2 (so that some entries clamp), rounded to
fp32 once and widened for the reference.

Reference.  numpy fp64 written from the formulas of include/so100_query.h: the noise from the oracle's philox4x32_np and box_muller_ref with the
header's counter words, the costs from cost_support.reference_select (K in place of L), the weights, the effective sample size and the blend in fp64
from those.  It is not a second instantiation of so100_mppi.hpp.

A `sample` callable is f(plan [T, N, 6], K, sigma [6], seed=, draw=, id_offset=, u_lo=, u_hi=, qpos= [N, 13] or None, qvel= [N, 12] or None) ->
{"ctrl" [T, N, K, 6], "qpos" [N, K, 13], "qvel" [N, K, 12]}; a `blend` callable is f(cost, qpos [T, N, K, 13], qvel, u [T, N, K, 6], target, temperature,
bad_step=None [N, K], u_fallback=None [T, N, 6], shift=0, tail="zero") -> {"cost", "weight" [N, K], "best", "best_cost", "ess" [N], "u_plan" [T, N, 6],
"u_first" [N, 6]}; numpy in and out."""
import functools

import numpy as np

import cost_support as CS
from hostlibs import mppicheck, ptr
from oracle import so100_oracle as O

TAILS = {"zero": 0, "hold": 1}
MAX_K = 4096
STREAM_C3 = 0x4D500000
bits = CS.bits


# ---- the twin --------------------------------------------------------------------------------------------------------------------------------------------
def _as(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def twin_sample(plan, K, sigma, seed=0, draw=0, id_offset=0, u_lo=-1.0, u_hi=1.0, qpos=None, qvel=None, dtype=np.float32):
    p, sg, q, v = _as(plan, dtype), _as(sigma, dtype), _as(qpos, dtype), _as(qvel, dtype)
    T, N = p.shape[:2]
    assert p.shape == (T, N, 6) and sg.shape == (6,) and (q is None or q.shape == (N, 13)) and (v is None or v.shape == (N, 12))
    out = {"ctrl": np.zeros((T, N, K, 6), dtype), "qpos": None if q is None else np.zeros((N, K, 13), dtype), "qvel": None if v is None else np.zeros((N, K, 12), dtype)}
    fn = mppicheck().mp_sample_d if np.dtype(dtype) == np.float64 else mppicheck().mp_sample_f
    fn(N, K, T, ptr(p), ptr(sg), float(dtype(u_lo)), float(dtype(u_hi)), seed, draw, id_offset, ptr(q), ptr(v), ptr(out["ctrl"]), ptr(out["qpos"]), ptr(out["qvel"]))
    return {k: a for k, a in out.items() if a is not None}


def twin_blend(cost, qpos, qvel, u, target, temperature, bad_step=None, u_fallback=None, shift=0, tail="zero", dtype=np.float32):
    q, v, uu, tg, fb, w = _as(qpos, dtype), _as(qvel, dtype), _as(u, dtype), _as(target, dtype), _as(u_fallback, dtype), CS.packed(cost, dtype)
    bs = None if bad_step is None else np.ascontiguousarray(bad_step, np.int32)
    T, N, K = uu.shape[:3]
    assert q.shape == (T, N, K, 13) and (v is None or v.shape == (T, N, K, 12)) and (bs is None or bs.shape == (N, K)) and (fb is None or fb.shape == (T, N, 6))
    out = {"cost": np.zeros((N, K), dtype), "best": np.zeros(N, np.int32), "best_cost": np.zeros(N, dtype), "weight": np.zeros((N, K), dtype), "ess": np.zeros(N, dtype),
           "u_plan": np.zeros((T, N, 6), dtype), "u_first": np.zeros((N, 6), dtype)}
    fn = mppicheck().mp_blend_d if np.dtype(dtype) == np.float64 else mppicheck().mp_blend_f
    fn(N, T, K, cost["link"], CS.TARGETS[cost["target_mode"]], ptr(w), ptr(tg), ptr(q), ptr(v), ptr(uu), ptr(bs), ptr(fb), float(np.float32(temperature)), shift, TAILS[tail],
       *[ptr(out[k]) for k in ("cost", "best", "best_cost", "weight", "ess", "u_plan", "u_first")])
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------
# K: inside a wave, a full wave, one over; a full workgroup of 256, one over; more than four rounds per thread with a ragged tail.  (4096, 1, 1): the limit.
# (3, 70, 1): many small problems.
KS, NS, TS = (1, 3, 63, 64, 65, 256, 257, 1030), (1, 3), (1, 3)
SHAPES = tuple((K, N, T) for K in KS for N in NS for T in TS) + ((4096, 1, 1), (3, 70, 1), (3, 70, 3))
COST_NAMES = ("cube-ee", "traj-l2")                          # one cube target, one traj target
SIGMA = (0.5, 0.25, 0.0, 1.0, 0.125, 0.0)                    # two dimensions never perturbed
SEED, DRAW, ID_OFFSET = 0x5EED0123456789AB, 11, 1000
SHIFTS = ((0, "zero"), (1, "zero"), (1, "hold"), (0, "hold"))


def shift_of(i):
    return SHIFTS[i % 4]


@functools.lru_cache(maxsize=None)
def blend_case(K, N, T):
    qpos, qvel, u = CS.seeded_states((T, N, K), 7919*K + 31*N + T)
    rs = np.random.RandomState(5 + 7919*K + 31*N + T)
    return {"qpos": qpos, "qvel": qvel, "u": u, "traj": rs.uniform(-0.3, 0.3, (T, N, 3)).astype(np.float32),
            "fallback": rs.uniform(-1.0, 1.0, (T, N, 6)).astype(np.float32)}


def blend_args(c, mode):
    return c["qpos"], c["qvel"], c["u"], (None if mode == "cube" else c[mode])


@functools.lru_cache(maxsize=None)
def sample_case(N, T):
    rs = np.random.RandomState(300 + 10*N + T)
    plan = rs.uniform(-1.2, 1.2, (T, N, 6)).astype(np.float32)
    qpos, qvel, _ = CS.seeded_states((N,), 400 + N)
    return {"plan": plan, "qpos": qpos, "qvel": qvel}


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
def reference_eps(seed, draw, gid, K, T):
    """float64 [N, K, T, 6]: the header's noise for the global problem ids gid [N] (candidate 0 included: the caller zeroes it)"""
    g, k, t = np.asarray(gid, np.uint64)[:, None, None], np.arange(K, dtype=np.uint64)[None, :, None], np.arange(T, dtype=np.uint64)[None, None, :]
    eps = np.empty((len(gid), K, T, 8))
    for b in range(2):
        r = O.philox4x32_np(g, np.uint64(draw), k, np.uint64(STREAM_C3) | (t << np.uint64(1)) | np.uint64(b), seed & 0xFFFFFFFF, seed >> 32)
        for i in range(2):
            eps[..., 4*b + 2*i], eps[..., 4*b + 2*i + 1] = O.box_muller_ref(r[..., 2*i], r[..., 2*i + 1])
    return eps[..., :6]


def reference_sample(plan, K, sigma, seed=0, draw=0, id_offset=0, u_lo=-1.0, u_hi=1.0):
    """ctrl [T, N, K, 6] in fp64 from the float32 plan and sigma"""
    plan, sigma = CS.f64(plan), CS.f64(sigma)
    T, N = plan.shape[:2]
    eps = reference_eps(seed, draw, id_offset + np.arange(N), K, T).transpose(2, 0, 1, 3)        # [T, N, K, 6]
    eps[:, :, 0] = 0.0
    return np.clip(plan[:, :, None] + sigma*eps, float(np.float32(u_lo)), float(np.float32(u_hi)))


def shifted(blend, shift, tail):
    """u_plan [T, N, 6] of a blend [T, N, 6]"""
    if not shift:
        return blend
    last = blend[-1:] if tail == "hold" else np.zeros_like(blend[-1:])
    return np.concatenate([blend[1:], last])


def reference_blend(cost, qpos, qvel, u, target, temperature, bad_step=None, shift=0, tail="zero"):
    """fp64 {"cost", "weight" [N, K], "best_cost", "ess" [N], "u_plan" [T, N, 6], "u_first" [N, 6]} (a problem without a candidate: weights and ess 0, the
    blend's rows left at 0 -- the caller compares those to the fallback)"""
    J = CS.reference_select(cost, qpos, qvel, u, target, bad_step)["cost"]
    lam = float(np.float32(temperature))
    j_min = J.min(1, keepdims=True)
    some = np.isfinite(j_min[:, 0])
    with np.errstate(invalid="ignore"):
        e = np.where(np.isinf(J), 0.0, np.exp(-(J - j_min)/lam))
    w = np.where(some[:, None], e/np.where(some, e.sum(1), 1.0)[:, None], 0.0)
    with np.errstate(divide="ignore"):
        ess = np.where(some, 1.0/(w**2).sum(1), 0.0)
    blend = np.einsum("nk,tnkj->tnj", w, np.where(w[None, :, :, None] > 0, CS.f64(u), 0.0))
    return {"cost": J, "weight": w, "best_cost": j_min[:, 0], "ess": ess, "u_plan": shifted(blend, shift, tail), "u_first": blend[0]}


@functools.lru_cache(maxsize=None)
def case_reference(name, K, N, T):
    """(temperature, the reference at shift 0): lambda is the fp64 standard deviation of the case's finite reference costs, rounded to fp32 (1 where that is
    0 or K = 1), so that the blend is a blend and the weights' sensitivity dw / w = dJ / lambda stays small"""
    cost = CS.COSTS[name]
    args = blend_args(blend_case(K, N, T), cost["target_mode"])
    J = CS.reference_select(cost, *args)["cost"]
    sd = float(np.float32(J[np.isfinite(J)].std()))
    lam = 1.0 if K == 1 or sd == 0.0 else sd
    return lam, reference_blend(cost, *args, lam)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------------------
FP64_BOUND = 1e-12                                           # two fp64 formulations of a query: the project's figure
# The fp32 twin's largest deviation from the reference per output over every case of tests/test_mppi_cpu.py (which prints them as [mppi-tol] lines and holds
# the twin to TWIN_FACTOR x these); the kernels are held to KERNEL_FACTOR x these: the margin for the device's exp, log and sincos, which differ from
# glibc's in the last places.  ess is an absolute figure on a quantity of up to K.
FP32_MEASURED = {"ctrl": 8.7e-7, "cost": 3.5e-6, "weight": 2.2e-7, "ess": 2.0e-4, "u_plan": 3.5e-7, "u_first": 2.4e-7}
TWIN_FACTOR, KERNEL_FACTOR = 1.05, 3.0
# what the kernels gave on an MI355X (tests/test_gpu_mppi.py prints them)
MEASURED = {"ctrl": 6.1e-7, "cost": 4.1e-6, "weight": 2.2e-7, "ess": 1.5e-4, "u_plan": 3.3e-7, "u_first": 3.0e-7,
            "mppi_reach --plan query, 8 envs x 64 samples x T = 8, 40 steps, final mean |cube - ee| in m (zero action: 0.4092; --plan torch: 0.2662)": 0.2429}
NOISE_EPS = 2.3e-6                                           # tests/test_gpu_policy_noise.py: the same transform on the same device
CTRL_DERIVED = max(SIGMA)*NOISE_EPS + 2.0**-23               # sigma x the transform's error + 1 ulp of a control of size <= 2


def sum_bound(dtype=np.float32, factor=TWIN_FACTOR):
    """|sum_k w_k - 1| (summed in fp64): within the record, like a single weight -- factor x FP32_MEASURED["weight"]; FP64_BOUND for the fp64 twin"""
    return FP64_BOUND if np.dtype(dtype) == np.float64 else factor*FP32_MEASURED["weight"]


def blend_deviation(got, ref, fallback=None):
    """largest |got - ref| per output; rows of a problem without a candidate are compared to the (shifted) fallback by the exact checks, not here"""
    some = np.isfinite(ref["best_cost"])
    d = {k: float(np.abs(np.asarray(got[k], np.float64) - ref[k])[some].max(initial=0.0)) for k in ("cost", "weight", "ess", "u_first")}
    d["u_plan"] = float(np.abs(np.asarray(got["u_plan"], np.float64) - ref["u_plan"])[:, some].max(initial=0.0))
    return d


def check_best(got, ref, cost_bound):
    """no problem is left out: the picked candidate is within twice the cost bound of the reference's minimum, and best_cost is its own cost to the bit"""
    n = np.arange(len(got["best"]))
    assert (got["best"] >= 0).all()
    assert (ref["cost"][n, got["best"]] <= ref["best_cost"] + 2*cost_bound).all()
    assert bits(got["best_cost"]) == bits(got["cost"][n, got["best"]])


def all_deviations(sample, blend):
    """largest deviation per output over every case; `best` checked in each"""
    worst = {k: 0.0 for k in FP32_MEASURED}
    for K, N, T in SHAPES:                                   # the sampler at every shape, K = 4096 and N = 70 included, with its fan-out rows
        c = sample_case(N, T)
        got = sample(c["plan"], K, SIGMA, seed=SEED, draw=DRAW, id_offset=ID_OFFSET, qpos=c["qpos"], qvel=c["qvel"])
        ref = reference_sample(c["plan"], K, SIGMA, SEED, DRAW, ID_OFFSET)
        worst["ctrl"] = max(worst["ctrl"], float(np.abs(got["ctrl"].astype(np.float64) - ref).max()))
        for k, w in (("qpos", 13), ("qvel", 12)):
            assert bits(got[k]) == bits(np.broadcast_to(c[k].astype(got[k].dtype)[:, None], (N, K, w))), (k, K, N, T)
    i = 0
    for name in COST_NAMES:
        cost = CS.COSTS[name]
        for K, N, T in SHAPES:
            lam, ref0 = case_reference(name, K, N, T)
            shift, tail = shift_of(i); i += 1
            ref = dict(ref0, u_plan=shifted(ref0["u_plan"], shift, tail))
            got = blend(cost, *blend_args(blend_case(K, N, T), cost["target_mode"]), lam, shift=shift, tail=tail)
            d = blend_deviation(got, ref)
            worst = {k: max(worst[k], d.get(k, 0.0)) for k in worst}
            check_best(got, ref, d["cost"])
    return worst


# ---- exact properties, of the twin and of the kernels alike ----------------------------------------------------------------------------------------------
def check_sample_exact(sample, dtype=np.float32, K=65, N=3, T=3):
    c = sample_case(N, T)
    plan = c["plan"].copy()
    plan[0, 0, 1] = -0.0; plan[0, 0, 2] = -0.0                # a -0 stays a -0 in candidate 0 and under sigma = 0
    kw = dict(seed=SEED, draw=DRAW, id_offset=ID_OFFSET)
    qpos, qvel = c["qpos"].copy(), c["qvel"].copy()
    qpos[0, 3] = np.nan; qvel[N - 1, 4] = -0.0; qpos[N - 1, 0] = np.inf      # the fan-out copies whatever is there
    got = sample(plan, K, SIGMA, qpos=qpos, qvel=qvel, **kw)
    again = sample(plan, K, SIGMA, qpos=qpos, qvel=qvel, **kw)
    for k in got:
        assert bits(got[k]) == bits(again[k]), k
    ctrl = got["ctrl"]
    assert ctrl.shape == (T, N, K, 6) and np.isfinite(ctrl).all()
    clamped = np.clip(plan, -1.0, 1.0).astype(ctrl.dtype)
    assert bits(ctrl[:, :, 0]) == bits(clamped) and np.signbit(ctrl[0, 0, 0, 1])
    for j, s in enumerate(SIGMA):
        if s == 0.0:
            assert bits(ctrl[..., j]) == bits(np.broadcast_to(clamped[:, :, None, j], (T, N, K))), j
        elif K > 1:                                          # a plan entry inside the bounds: its perturbed candidates leave it (or sit on a bound)
            inside = np.abs(plan[..., j]) < 1.0
            assert not inside.any() or (ctrl[inside][:, 1:, j] != clamped[inside][:, None, j]).mean() > 0.99, j
    assert (ctrl >= -1.0).all() and (ctrl <= 1.0).all() and (ctrl == 1.0).any() and (ctrl == -1.0).any()
    assert bits(got["qpos"]) == bits(np.broadcast_to(qpos.astype(ctrl.dtype)[:, None], (N, K, 13)))
    assert bits(got["qvel"]) == bits(np.broadcast_to(qvel.astype(ctrl.dtype)[:, None], (N, K, 12)))
    # ctrl alone, the fan-out alone: the same bits
    assert bits(sample(plan, K, SIGMA, **kw)["ctrl"]) == bits(ctrl)
    # a problem's candidates depend on its global id alone, not on N or its place
    for n in range(N):
        one = sample(plan[:, n:n + 1], K, SIGMA, seed=SEED, draw=DRAW, id_offset=ID_OFFSET + n)
        assert bits(one["ctrl"][:, 0]) == bits(ctrl[:, n]), n
    # nothing clamps here: another draw, another seed and another id change EVERY perturbed entry
    wide = dict(u_lo=-10.0, u_hi=10.0)
    small = (0.2*plan).astype(np.float32)
    base = sample(small, K, SIGMA, **wide, **kw)["ctrl"]
    live = np.asarray(SIGMA) > 0
    for other in (dict(kw, draw=DRAW + 1), dict(kw, seed=SEED + 1), dict(kw, seed=SEED ^ (1 << 40)), dict(kw, id_offset=ID_OFFSET + 1)):
        moved = sample(small, K, SIGMA, **wide, **other)["ctrl"]
        assert (moved[:, :, 1:][..., live] != base[:, :, 1:][..., live]).all() and bits(moved[:, :, 0]) == bits(base[:, :, 0])
    # (n, k) is not (k, n)
    eps = sample(np.zeros((1, 3, 6), np.float32), 3, (1.0,)*6, **wide, **kw)["ctrl"][0]
    assert np.abs(eps[1, 2] - eps[2, 1]).max() > 1e-3 and not eps[:, 0].any()
    # a plan entry that is not finite is NaN in all K candidates, and only there
    for bad in (np.nan, np.inf, -np.inf):
        p2 = plan.copy(); p2[T - 1, N - 1, 3] = bad
        g2 = sample(p2, K, SIGMA, **kw)["ctrl"]
        assert np.isnan(g2[T - 1, N - 1, :, 3]).all()
        a, b = g2.copy(), ctrl.copy(); a[T - 1, N - 1, :, 3] = b[T - 1, N - 1, :, 3] = 0
        assert bits(a) == bits(b)
    return ctrl


def check_blend_exact(blend, select_cost, name, K, dtype=np.float32, N=3, T=3, factor=TWIN_FACTOR):
    """the properties of include/so100_query.h that hold to the bit.  select_cost(cost, qpos, qvel, u, target, bad_step) -> so100_query_cost_select's "cost" [N, K]"""
    cost = CS.COSTS[name]
    c = blend_case(K, N, T)
    lam, _ = case_reference(name, K, N, T)
    qpos, qvel, u, tg = (a.copy() if a is not None else None for a in blend_args(c, cost["target_mode"]))
    if K >= 6:
        qpos[:, :, 5], qvel[:, :, 5], u[:, :, 5] = qpos[:, :, 2], qvel[:, :, 2], u[:, :, 2]      # candidate 5 is candidate 2 again
    fb = c["fallback"]
    got = blend(cost, qpos, qvel, u, tg, lam, u_fallback=fb)
    again = blend(cost, qpos, qvel, u, tg, lam, u_fallback=fb)
    for k in got:
        assert bits(got[k]) == bits(again[k]), k
    f = got["cost"].dtype
    n = np.arange(N)
    w = got["weight"]
    assert np.isfinite(got["cost"]).all() and (w >= 0).all() and np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= sum_bound(f, factor)
    assert (got["best"] == np.argmin(got["cost"], axis=1)).all() and bits(got["best_cost"]) == bits(got["cost"][n, got["best"]])
    assert (w[n, got["best"]][:, None] >= w).all() and (got["ess"] >= 1.0 - 1e-6).all() and (got["ess"] <= K*(1.0 + 1e-6)).all()
    assert bits(got["cost"]) == bits(select_cost(cost, qpos, qvel, u, tg, None))
    if K >= 6:
        assert bits(w[:, 5]) == bits(w[:, 2]) and (got["best"] != 5).all()
    if K == 1:
        assert (w == 1.0).all() and (got["ess"] == 1.0).all() and bits(got["u_plan"]) == bits(u[:, :, 0].astype(f)) and bits(got["u_first"]) == bits(u[0, :, 0].astype(f))
    # the shift and the tails
    assert bits(got["u_first"]) == bits(got["u_plan"][0])
    for shift, tail in SHIFTS:
        s = blend(cost, qpos, qvel, u, tg, lam, u_fallback=fb, shift=shift, tail=tail)
        for k in ("cost", "weight", "best", "best_cost", "ess", "u_first"):
            assert bits(s[k]) == bits(got[k]), (k, shift, tail)
        assert bits(s["u_plan"]) == bits(shifted(got["u_plan"], shift, tail)), (shift, tail)
    # a problem's bits depend neither on N nor on its place
    sl = slice(N - 1, N)
    sub_tg = None if tg is None else tg[:, sl]
    sub = blend(cost, qpos[:, sl], qvel[:, sl], u[:, sl], sub_tg, lam, u_fallback=fb[:, sl], shift=1, tail="hold")
    full = blend(cost, qpos, qvel, u, tg, lam, u_fallback=fb, shift=1, tail="hold")
    for k in ("cost", "weight", "best", "best_cost", "ess", "u_first"):
        assert bits(sub[k]) == bits(full[k][sl]), k
    assert bits(sub["u_plan"]) == bits(full["u_plan"][:, sl])
    # every candidate of problem 0 failed: the shifted fallback (NaN without one); the neighbours untouched
    bad = np.full((N, K), -1, np.int32); bad[0] = 1
    for fallback in (fb, None):
        for shift, tail in SHIFTS:
            x = blend(cost, qpos, qvel, u, tg, lam, bad_step=bad, u_fallback=fallback, shift=shift, tail=tail)
            assert x["best"][0] == -1 and np.isposinf(x["best_cost"][0]) and np.isposinf(x["cost"][0]).all() and not x["weight"][0].any() and x["ess"][0] == 0
            if fallback is None:                             # a column of NaN, shifted like any other: a "zero" tail row is 0 here too
                lost = shifted(np.full((T, 1, 6), np.nan, f), shift, tail)
                assert bits(np.isnan(x["u_plan"][:, :1])) == bits(np.isnan(lost)) and not np.nan_to_num(x["u_plan"][:, 0]).any() and np.isnan(x["u_first"][0]).all()
            else:
                want = shifted(fb.astype(f), shift, tail)
                assert bits(x["u_plan"][:, 0]) == bits(want[:, 0]) and bits(x["u_first"][0]) == bits(fb[0, 0].astype(f))
            for k in ("cost", "weight", "best", "best_cost", "ess", "u_first"):
                assert bits(x[k][1:]) == bits(got[k][1:]), k
            assert bits(x["u_plan"][:, 1:]) == bits(shifted(got["u_plan"], shift, tail)[:, 1:])
    if K == 1:
        return got
    # one failed rollout and one with a NaN state and NaN controls: weight exactly 0, the blend finite, the neighbours untouched
    k_bad, k_nan = int(got["best"][1]), (int(got["best"][1]) + 1) % K
    bad = np.full((N, K), -1, np.int32); bad[1, k_bad] = 0
    q2, u2 = qpos.copy(), u.copy()
    q2[T - 1, 1, k_nan, 1] = np.nan; u2[:, 1, k_nan] = np.nan
    x = blend(cost, q2, qvel, u2, tg, lam, bad_step=bad, u_fallback=fb)
    assert x["weight"][1, k_bad] == 0 and x["weight"][1, k_nan] == 0 and np.isposinf(x["cost"][1, [k_bad, k_nan]]).all()
    assert np.isfinite(x["u_plan"]).all() and np.isfinite(x["u_first"]).all() and np.isfinite(x["ess"]).all() and x["best"][1] not in (k_bad, k_nan)
    if K > 2:
        assert np.abs(x["weight"][1].astype(np.float64).sum() - 1.0) <= sum_bound(f, factor)
    keep = n != 1
    for k in ("cost", "weight", "best", "best_cost", "ess", "u_first"):
        assert bits(x[k][keep]) == bits(got[k][keep]), k
    assert bits(x["u_plan"][:, keep]) == bits(got["u_plan"][:, keep])
    return got
