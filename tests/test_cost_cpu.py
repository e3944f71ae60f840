"""The two cost queries on the CPU: the surface of include/so100_query.h (so100_cost_def, so100_query_cost_terms, so100_query_cost_select), the host twin
of so100_cost.hpp (tests/_costcheck) against the numpy reference of tests/cost_support.py, the reference's own lx against central differences, the
exact properties.  The twin's table and its stand-alone program are held in tests/test_hostlibs.py.  The same cases run on the kernels in tests/test_gpu_cost.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cost_support as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "so100_query.h")
C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}


def show(tag, dev, bound=None):
    print(f"[cost-tol] {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in dev.items()) + ("" if bound is None else f" (bound {bound})"))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def struct_fields(name, pointers=None):
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
    assert same(struct_fields("so100_cost_def"), list(lib.CostDef._fields_))
    assert same(struct_fields("so100_cost_terms_io"), list(lib.CostTermsIO._fields_))
    assert same(struct_fields("so100_cost_select_io"), list(lib.CostSelectIO._fields_))
    text = header_text()
    for fn, io, cls in (("so100_query_cost_terms", "so100_cost_terms_io", lib.CostTermsIO), ("so100_query_cost_select", "so100_cost_select_io", lib.CostSelectIO)):
        assert lib.QUERY_IO[fn] is cls and fn in lib.QUERY_EXPORTS
        assert re.search(r"int %s\(so100_sim\* sim, const %s\* io, int32_t M, void\* hip_stream\);" % (fn, io), text)
    modes = {name: int(re.search(r"#define SO100_COST_TARGET_%s\s+(\d+)\b" % name.upper(), text).group(1)) for name in S.TARGETS}
    assert modes == lib.COST_TARGETS == S.TARGETS
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    for fn, io in (("so100_query_cost_terms", lib.CostTermsIO), ("so100_query_cost_select", lib.CostSelectIO)):
        assert getattr(L, fn)(None, C.byref(io()), 1, None) == -1
        assert L.so100_last_error() == (fn + ": null argument").encode()


# ---- the reference against itself -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.COSTS))
def test_the_references_lx_against_central_differences(name):
    """the Gauss-Newton model drops a SECOND derivative only: lx is the exact gradient of sigma s"""
    cost = S.COSTS[name]
    qpos, qvel, u, tg = S.corner(S.terms_case(), 3, 65, cost["target_mode"])
    ref = S.reference_terms(cost, qpos, qvel, u, tg, 24)
    fd = S.reference_lx_by_differences(cost, qpos, qvel, tg)
    d = float(np.abs(ref["lx"][1:] - fd).max())
    print(f"[cost-tol] reference lx vs central differences, {name}: {d:.3e} (bound {S.FD_BOUND})")
    assert d <= S.FD_BOUND and not ref["lx"][0].any()


# ---- deviation bounds ------------------------------------------------------------------------------------------------------------------------------------
def all_terms_deviations(terms):
    """largest deviation per output over COSTS x TERMS_M x TERMS_T x both nx"""
    worst = {"lx": 0.0, "lxx": 0.0, "lu": 0.0, "luu": 0.0}
    c = S.terms_case()
    for name, cost in S.COSTS.items():
        for nx in (12, 24):
            ref = S.reference_terms(cost, *S.corner(c, 3, 130, cost["target_mode"]), nx)
            for T in S.TERMS_T:
                small = ref if T == 3 else S.reference_terms(cost, *S.corner(c, T, 130, cost["target_mode"]), nx)       # the terminal weight moves
                for M in S.TERMS_M:
                    d = S.terms_deviation(terms(cost, *S.corner(c, T, M, cost["target_mode"]), nx), {k: v[:, :M] for k, v in small.items()})
                    worst = {k: max(worst[k], d[k]) for k in worst}
    return worst


def all_select_deviations(select):
    """(largest cost deviation, problems compared, problems left out as knife-edge, wrong `best`) over COSTS' modes x SELECT_L x SELECT_M"""
    worst, compared, left, wrong = 0.0, 0, 0, 0
    for name in ("cube-ee", "fixed-l2", "traj-ee"):
        cost = S.COSTS[name]
        for L in S.SELECT_L:
            for M in S.SELECT_M:
                c = S.select_case(L, M)
                args = S.select_args(c, cost["target_mode"])
                ref, got = S.reference_select(cost, *args), select(cost, *args, u_fallback=c["fallback"])
                worst = max(worst, float(np.abs(np.asarray(got["cost"], np.float64) - ref["cost"]).max()))
                ok = S.comparable(ref)
                compared += int(ok.sum()); left += int((~ok).sum())
                wrong += int((got["best"][ok] != ref["best"][ok]).sum())
                env = np.arange(M)
                assert S.bits(got["u_best"][:, ok]) == S.bits(np.asarray(c["u"], got["u_best"].dtype)[:, env[ok], got["best"][ok]])
    return worst, compared, left, wrong


def test_fp64_twin_against_the_reference():
    d = all_terms_deviations(lambda *a: S.twin_terms(*a, dtype=np.float64))
    cost, compared, left, wrong = all_select_deviations(lambda *a, **k: S.twin_select(*a, dtype=np.float64, **k))
    d["cost"] = cost
    show("fp64 twin", d, S.FP64_BOUND)
    assert max(d.values()) <= S.FP64_BOUND and wrong == 0


def test_fp32_twin_against_the_reference():
    d = all_terms_deviations(S.twin_terms)
    cost, compared, left, wrong = all_select_deviations(S.twin_select)
    d["cost"] = cost
    show("fp32 twin (the record of cost_support.FP32_MEASURED)", d)
    print(f"[cost-tol] best: {compared} problems compared, {left} left out as knife-edge, {wrong} wrong")
    assert d["luu"] == 0.0                                  # 2 w_u in fp32 is exact
    for k, v in S.FP32_MEASURED.items():
        assert d[k] <= S.TWIN_FACTOR*v, (k, d[k], v)
    assert wrong == 0 and left == S.KNIFE_EDGE_COUNT and left <= S.KNIFE_EDGE_SHARE*(compared + left)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(S.COSTS))
def test_terms_exact_properties(name, dtype):
    terms = lambda *a: S.twin_terms(*a, dtype=dtype)
    for T, M in ((3, 65), (1, 3)):
        S.check_terms_exact(terms, S.COSTS[name], T, M)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_terms_zero_weights_place_and_non_finite_inputs(dtype):
    terms = lambda *a: S.twin_terms(*a, dtype=dtype)
    S.check_terms_zero_weights(terms)
    for name in ("cube-ee", "fixed-l2", "traj-ee"):
        S.check_terms_place(terms, S.COSTS[name])
        S.check_terms_non_finite(terms, S.COSTS[name], 12 if name == "fixed-l2" else 24)


def test_terms_without_velocities_are_those_of_zero_velocities():
    c = S.terms_case()
    cost = S.COSTS["cube-ee"]
    qpos, qvel, u, tg = S.corner(c, 3, 3, "cube")
    a, b = S.twin_terms(cost, qpos, None, u, tg, 24), S.twin_terms(cost, qpos, np.zeros_like(qvel), u, tg, 24)
    for k in a:
        assert S.bits(a[k]) == S.bits(b[k])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["cube-ee", "fixed-l2", "traj-ee"])
def test_select_exact_properties(name, dtype):
    S.check_select_exact(lambda *a, **k: S.twin_select(*a, dtype=dtype, **k), S.COSTS[name])


def test_the_lqr_twin_takes_the_terms_and_flags_a_nan_row():
    """the arrays are what the LQR query reads: its twin runs on them (synthetic stable A, B) and reports bad = T where a state row was not finite"""
    import lqr_support as LS
    cost = S.COSTS["cube-ee"]
    qpos, qvel, u, tg = S.corner(S.terms_case(), 3, 3, "cube")
    q2 = qpos.copy(); q2[1, 2, 0] = np.nan
    t = S.twin_terms(cost, q2, qvel, u, tg, 12)
    A = np.zeros((3, 3, 24, 24), np.float32); A[..., np.arange(24), np.arange(24)] = 0.9
    B = np.zeros((3, 3, 24, 6), np.float32); B[..., np.arange(6), np.arange(6)] = 0.1
    got = LS.twin(LS.problem(A, B, t["lx"], t["lxx"], t["lu"], t["luu"], None, nx=12, reg=1e-6), np.float32)
    assert got["bad"].tolist() == [-1, -1, 3]
