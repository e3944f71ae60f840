"""The two cross-entropy planner queries on the CPU: the surface of include/so100_query.h (so100_query_plan_sample_tv, so100_query_cost_refit), the host twin
of so100_cem.hpp (tests/_cemcheck) against the numpy reference of tests/cem_support.py, the exact properties in both precisions, and the integer keys' order.
The twin's table and its stand-alone program are held in tests/test_hostlibs.py.  The same cases run on the kernels in tests/test_gpu_cem.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cem_support as S
import mppi_support as MS
import test_mppi_cpu as TM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def show(tag, dev, bound=None):
    print(f"[cem-tol] {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in dev.items()) + ("" if bound is None else f" (bound {bound})"))


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------------------
def test_structs_match_the_header_field_for_field():
    from so100_mujoco_rl_amd import lib
    same = lambda a, b: len(a) == len(b) and all(x[0] == y[0] and (x[1] is y[1] or (getattr(x[1], "_length_", 0) == getattr(y[1], "_length_", 1) and
                                                                                   x[1]._type_ is y[1]._type_)) for x, y in zip(a, b))
    assert same(TM.struct_fields("so100_plan_sample_tv_io"), list(lib.PlanSampleTvIO._fields_))
    assert same(TM.struct_fields("so100_cost_refit_io"), list(lib.CostRefitIO._fields_))
    # the sampler's struct is so100_plan_sample_io's with sigma_dev in place of sigma[6]
    plain, tv = TM.struct_fields("so100_plan_sample_io"), TM.struct_fields("so100_plan_sample_tv_io")
    assert [f[0] for f in plain if f[0] != "sigma"] == [f[0] for f in tv if f[0] != "sigma_dev"] and tv[1] == ("sigma_dev", C.c_void_p)
    text = TM.header_text()
    for fn, io, cls in (("so100_query_plan_sample_tv", "so100_plan_sample_tv_io", lib.PlanSampleTvIO), ("so100_query_cost_refit", "so100_cost_refit_io", lib.CostRefitIO)):
        assert lib.QUERY_IO[fn] is cls and fn in lib.QUERY_EXPORTS
        assert re.search(r"int %s\(so100_sim\* sim, const %s\* io, int32_t N, void\* hip_stream\);" % (fn, io), text)
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    for fn, io in (("so100_query_plan_sample_tv", lib.PlanSampleTvIO), ("so100_query_cost_refit", lib.CostRefitIO)):
        assert getattr(L, fn)(None, C.byref(io()), 1, None) == -1
        assert L.so100_last_error() == (fn + ": null argument").encode()


# ---- the keys -------------------------------------------------------------------------------------------------------------------------------------------
def test_the_integer_keys_order_is_the_definitions():
    """the kernel sorts cem_key(J, k); over all pairs of 600 costs -- zeros of both signs, denormals, infinities, repeats, negative values -- that order is
    cem_before's, every key lies below the padding and returns its index"""
    rs = np.random.RandomState(4)
    J = np.concatenate([[0.0, -0.0, 1e-45, -1e-45, np.inf, np.inf, -np.inf, 3.4e38, -3.4e38], rs.uniform(-4, 4, 291), rs.choice(rs.uniform(0, 1, 20), 300)]).astype(np.float32)
    rs.shuffle(J)
    assert S.cemcheck().cm_key_disagreements(len(J), S.ptr(J)) == 0


# ---- deviation bounds ------------------------------------------------------------------------------------------------------------------------------------
def test_fp64_twin_against_the_reference():
    d = S.refit_deviations(lambda *a, **k: S.twin_refit(*a, dtype=np.float64, **k), dtype=np.float64)
    d["ctrl"] = S.sample_deviation(lambda *a, **k: S.twin_sample(*a, dtype=np.float64, **k), lambda *a, **k: MS.twin_sample(*a, dtype=np.float64, **k))
    show("fp64 twin", d, S.FP64_BOUND)
    assert max(d.values()) <= S.FP64_BOUND


def test_fp32_twin_against_the_reference():
    d = S.refit_deviations(S.twin_refit)
    d["ctrl"] = S.sample_deviation(S.twin_sample, MS.twin_sample)
    show("fp32 twin (the record of cem_support.FP32_MEASURED)", d)
    print(f"[cem-tol] ctrl: the derived bound max(sigma) x NOISE_EPS + 1 ulp = {S.CTRL_DERIVED:.3e}")
    for k, v in S.FP32_MEASURED.items():
        assert d[k] <= S.TWIN_FACTOR*v, (k, d[k], v)
    assert S.FP32_MEASURED["ctrl"] <= S.CTRL_DERIVED


# ---- exact properties ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K, N, T", [(1, 3, 3), (65, 3, 3), (257, 3, 1), (3, 70, 3)])
def test_sample_exact_properties(K, N, T, dtype):
    S.check_sample_exact(lambda *a, **k: S.twin_sample(*a, dtype=dtype, **k), K=K, N=N, T=T)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("name", S.COST_NAMES)
def test_refit_exact_properties(name, K, dtype):
    S.check_refit_exact(lambda *a, **k: S.twin_refit(*a, dtype=dtype, **k), lambda *a, **k: MS.twin_blend(*a, dtype=dtype, **k), name, K)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_many_small_problems(dtype):
    """N = 70 at K = 3 against N = 3 inside it"""
    import cost_support as CS
    cost, c, old = CS.COSTS["cube-ee"], MS.blend_case(3, 70, 3), S.old_case(70, 3)
    sl = slice(64, 67)
    kw = lambda s: dict(alpha=0.25, plan=old["plan"][:, s], sigma=old["sigma"][:, s], shift=1, tail="hold", dtype=dtype, **S.LIMITS)
    full = S.twin_refit(cost, c["qpos"], c["qvel"], c["u"], None, 2, **kw(slice(None)))
    sub = S.twin_refit(cost, c["qpos"][:, sl], c["qvel"][:, sl], c["u"][:, sl], None, 2, **kw(sl))
    for k in S.OUTPUTS:
        assert S.bits(sub[k]) == S.bits(full[k][sl] if k in S.PER_PROBLEM else full[k][:, sl]), k
