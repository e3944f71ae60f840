"""The two sampling-planner queries on the CPU: the surface of include/so100_query.h (so100_query_plan_sample, so100_query_cost_blend), the host twin of
so100_mppi.hpp (tests/_mppicheck) against the numpy reference of tests/mppi_support.py, the reference's own properties (the noise's moments, the
effective sample sizes), the exact properties.  The twin's table and its stand-alone program are held in tests/test_hostlibs.py.  The same cases run on the kernels in tests/test_gpu_mppi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cost_support as CS
import mppi_support as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "so100_query.h")
C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float,
           "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


def show(tag, dev, bound=None):
    print(f"[mppi-tol] {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in dev.items()) + ("" if bound is None else f" (bound {bound})"))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def struct_fields(name):
    from so100_mujoco_rl_amd import lib
    types = dict(C_TYPES, **{"const so100_cost_def*": C.POINTER(lib.CostDef)})
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header_text()).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, field, count = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)(?:\[(\d+)\])?\s*$", decl).groups()
            t = types[re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()]
            fields.append((field, t*int(count) if count else t))
    return fields


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------------------
def test_structs_match_the_header_field_for_field():
    from so100_mujoco_rl_amd import lib
    same = lambda a, b: len(a) == len(b) and all(x[0] == y[0] and (x[1] is y[1] or (getattr(x[1], "_length_", 0) == getattr(y[1], "_length_", 1) and
                                                                                   x[1]._type_ is y[1]._type_)) for x, y in zip(a, b))
    assert same(struct_fields("so100_plan_sample_io"), list(lib.PlanSampleIO._fields_))
    assert same(struct_fields("so100_cost_blend_io"), list(lib.CostBlendIO._fields_))
    text = header_text()
    for fn, io, cls in (("so100_query_plan_sample", "so100_plan_sample_io", lib.PlanSampleIO), ("so100_query_cost_blend", "so100_cost_blend_io", lib.CostBlendIO)):
        assert lib.QUERY_IO[fn] is cls and fn in lib.QUERY_EXPORTS
        assert re.search(r"int %s\(so100_sim\* sim, const %s\* io, int32_t N, void\* hip_stream\);" % (fn, io), text)
    macro = lambda name: int(re.search(r"#define %s\s+(\d+)\b" % name, text).group(1))
    assert macro("SO100_MPPI_MAX_K") == lib.MPPI_MAX_K == S.MAX_K == 4096
    assert {"zero": macro("SO100_BLEND_TAIL_ZERO"), "hold": macro("SO100_BLEND_TAIL_HOLD")} == lib.BLEND_TAILS == S.TAILS
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    for fn, io in (("so100_query_plan_sample", lib.PlanSampleIO), ("so100_query_cost_blend", lib.CostBlendIO)):
        assert getattr(L, fn)(None, C.byref(io()), 1, None) == -1
        assert L.so100_last_error() == (fn + ": null argument").encode()


# ---- the reference by itself -----------------------------------------------------------------------------------------------------------------------------
def test_the_stream_is_its_own():
    """the last counter word can be neither 0 (the simulator's draws) nor 0x504F4C (the policy noise) at any t the header admits"""
    t = np.arange(4096, dtype=np.uint64)
    for b in (0, 1):
        c3 = np.uint64(S.STREAM_C3) | (t << np.uint64(1)) | np.uint64(b)
        assert (c3 >> np.uint64(13) == np.uint64(S.STREAM_C3 >> 13)).all() and (c3 != 0).all() and (c3 != 0x504F4C).all()


@pytest.mark.parametrize("which", ["reference", "twin"])
def test_the_noise_is_standard_normal(which):
    """17 problems x 4095 perturbed candidates x 6 = 417 690 draws (2^16 and more per dimension): the bands tests/test_rng_reference.py holds policy_noise_ref to"""
    N, K = 17, 4096
    if which == "reference":
        x = S.reference_eps(S.SEED, S.DRAW, S.ID_OFFSET + np.arange(N), K, 1)[:, 1:, 0]
    else:
        x = S.twin_sample(np.zeros((1, N, 6), np.float32), K, (1.0,)*6, S.SEED, S.DRAW, S.ID_OFFSET, -100.0, 100.0)["ctrl"][0, :, 1:].astype(np.float64)
    assert x.shape == (N, K - 1, 6) and np.isfinite(x).all()
    n = x.size
    se = lambda var, m=n: 4.0*np.sqrt(var/m)
    flat = x.reshape(-1)
    mean, var, m3, m4 = flat.mean(), (flat**2).mean(), (flat**3).mean(), (flat**4).mean()
    lag_n = (x[1:]*x[:-1]).mean(); lag_k = (x[:, 1:]*x[:, :-1]).mean(); lag_j = (x[..., 1:]*x[..., :-1]).mean()
    off = np.abs(np.corrcoef(x.reshape(-1, 6).T) - np.eye(6)).max()
    print(f"[mppi noise, {which}] mean {mean:.2e} var-1 {var - 1:.2e} m3 {m3:.2e} m4-3 {m4 - 3:.2e} lag-1 n {lag_n:.2e} k {lag_k:.2e} j {lag_j:.2e} max corr {off:.2e}")
    assert abs(mean) < se(1.0) and abs(var - 1) < se(2.0) and abs(m3) < se(15.0) and abs(m4 - 3) < se(96.0)
    assert abs(lag_n) < se(1.0, (N - 1)*(K - 1)*6) and abs(lag_k) < se(1.0, N*(K - 2)*6) and abs(lag_j) < se(1.0, N*(K - 1)*5)
    assert off < se(1.0, N*(K - 1)) and np.abs(flat).max() <= np.sqrt(48*np.log(2.0)) + 1e-5


def test_the_blend_is_a_blend():
    """on the reference alone: under the per-case temperature every problem of K >= 64 candidates has an effective sample size of 4 or more"""
    least = {}
    for name in S.COST_NAMES:
        for K, N, T in S.SHAPES:
            if K >= 64:
                ess = S.case_reference(name, K, N, T)[1]["ess"]
                least[K] = min(least.get(K, np.inf), float(ess.min()))
    print("[mppi-tol] least effective sample size per K: " + " ".join(f"{K}: {v:.1f}" for K, v in sorted(least.items())))
    assert min(least.values()) >= 4.0


# ---- deviation bounds ------------------------------------------------------------------------------------------------------------------------------------
def test_fp64_twin_against_the_reference():
    d = S.all_deviations(lambda *a, **k: S.twin_sample(*a, dtype=np.float64, **k), lambda *a, **k: S.twin_blend(*a, dtype=np.float64, **k))
    show("fp64 twin", d, S.FP64_BOUND)
    assert max(d.values()) <= S.FP64_BOUND


def test_fp32_twin_against_the_reference():
    d = S.all_deviations(S.twin_sample, S.twin_blend)
    show("fp32 twin (the record of mppi_support.FP32_MEASURED)", d)
    print(f"[mppi-tol] ctrl: the derived bound max(sigma) x NOISE_EPS + 1 ulp = {S.CTRL_DERIVED:.3e}")
    for k, v in S.FP32_MEASURED.items():
        assert d[k] <= S.TWIN_FACTOR*v, (k, d[k], v)
    assert S.FP32_MEASURED["ctrl"] <= S.CTRL_DERIVED


# ---- exact properties ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K, N, T", [(1, 3, 3), (3, 3, 3), (65, 3, 3), (257, 3, 3), (4096, 1, 1), (3, 70, 1), (3, 70, 3)])
def test_sample_exact_properties(K, N, T, dtype):
    S.check_sample_exact(lambda *a, **k: S.twin_sample(*a, dtype=dtype, **k), dtype, K=K, N=N, T=T)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("name", S.COST_NAMES)
def test_blend_exact_properties(name, K, dtype):
    select_cost = lambda cost, qpos, qvel, u, tg, bad: CS.twin_select(cost, qpos, qvel, u, tg, bad, dtype=dtype)["cost"]
    S.check_blend_exact(lambda *a, **k: S.twin_blend(*a, dtype=dtype, **k), select_cost, name, K, dtype)


def test_without_velocities_is_zero_velocities():
    cost = CS.COSTS["cube-ee"]
    qpos, qvel, u, tg = S.blend_args(S.blend_case(65, 3, 3), "cube")
    a, b = S.twin_blend(cost, qpos, None, u, tg, 0.5), S.twin_blend(cost, qpos, np.zeros_like(qvel), u, tg, 0.5)
    for k in a:
        assert S.bits(a[k]) == S.bits(b[k])
