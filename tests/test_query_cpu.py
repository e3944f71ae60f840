"""Model queries (include/so100_query.h) without a GPU: the ABI surface, and the host twin of csrc/so100_query.hpp -- the templates the
kernels instantiate -- against the fp64 oracle.  Cases, references and bounds: tests/query_support.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import query_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "so100_query.h")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.fixture(scope="module")
def L():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib.load()


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_declared_symbol_is_exported_and_bound(L):
    from so100_mujoco_rl_amd import lib
    declared = sorted(set(re.findall(r"\b(so100_[a-z_]+)\s*\(", header_text())))
    assert declared == sorted(lib.QUERY_EXPORTS)
    for s in declared:
        assert getattr(L, s).argtypes == [C.c_void_p, C.POINTER(lib.QUERY_IO[s]), C.c_int32, C.c_void_p], s
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "uint8_t*": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}


@pytest.mark.parametrize("struct, cls", [("so100_kinematics_io", "KinematicsIO"), ("so100_jacobian_io", "JacobianIO"),
                                         ("so100_dynamics_io", "DynamicsIO"), ("so100_ik_io", "IkIO")])
def test_structs_match_the_header_field_for_field(struct, cls):
    from so100_mujoco_rl_amd import lib
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header_text()).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, name = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", decl).groups()
            fields.append((name, C_TYPES[re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()]))
    assert fields == list(getattr(lib, cls)._fields_)


def test_defaults_match_the_header():
    from so100_mujoco_rl_amd import lib
    src = header_text()
    macro = lambda name: re.search(r"#define %s\s+\(?(-?[0-9.e-]+)f?\)?" % name, src).group(1)
    assert (int(macro("SO100_IK_ITERS")), float(macro("SO100_IK_DAMPING")), float(macro("SO100_IK_TOL")), float(macro("SO100_IK_MAX_STEP"))) == \
        (lib.IK_ITERS, lib.IK_DAMPING, lib.IK_TOL, lib.IK_MAX_STEP) == (64, 0.02, 1e-4, 0.3)
    assert int(macro("SO100_EE_LINK")) == lib.EE_LINK == S.EE_LINK and float(macro("SO100_EE_OFFSET_Y")) == -0.1


def test_null_arguments_are_refused_without_a_device(L):
    """the handle is checked first: the only argument error that can be reached without a GPU (the others: test_gpu_query.py)"""
    from so100_mujoco_rl_amd import lib
    for fn, io in lib.QUERY_IO.items():
        assert getattr(L, fn)(None, C.byref(io()), 1, None) == -1
        assert L.so100_last_error() == (fn + ": null argument").encode()


# ---- the fp64 twin against the oracle -----------------------------------------------------------------------------------------------------------------
def twin_closed_form(dtype):
    q, v, qacc = S.cases()
    got = S.twin_kinematics(q, dtype)
    got.update(S.twin_jacobian(q, dtype))
    got.update(S.twin_dynamics(q, v, qacc, dtype))
    return got


def test_fp64_twin_against_the_oracle():
    diff = S.max_abs_diff(twin_closed_form(np.float64), S.closed_form_reference())
    assert sorted(diff) == sorted(S.FP32_BOUNDS)
    for k, d in diff.items():
        print(f"[query-tol] fp64 twin {k}: {d:.3e}")
    assert max(diff.values()) <= S.FP64_BOUND, diff


@pytest.mark.parametrize("link, offset", [(0, None), (2, (0.01, -0.02, 0.03)), (4, (0.0, 0.0, 0.0)), (5, None), (5, (0.0, -0.05, 0.01))])
def test_fp64_jacobian_of_other_points(link, offset):
    """other links, explicit offsets and the default point of a link other than 4 (its origin); columns behind the link are zero"""
    q = S.cases()[0][:64].astype(np.float64)
    got = S.twin_jacobian(q, np.float64, link, offset)
    ref = S.oracle_jacobian(q, link, (0.0, 0.0, 0.0) if offset is None else offset)
    assert max(S.max_abs_diff(got, ref).values()) <= S.FP64_BOUND
    assert not got["jacp"][:, :, link + 1:].any() and not got["jacr"][:, :, link + 1:].any()


def test_dynamics_without_velocity_or_acceleration():
    q = S.cases()[0][:64].astype(np.float64)
    got = S.twin_dynamics(q, None, None, np.float64)
    assert "tau" not in got
    assert max(S.max_abs_diff(got, S.oracle_dynamics(q, None)).values()) <= S.FP64_BOUND


def test_jacobian_against_finite_differences():
    """central differences of the ORACLE's forward kinematics, h = 1e-6: truncation h^2 |p'''| / 6 ~ 1e-13, round-off 1e-16 / h ~ 1e-10"""
    q = S.cases()[0].astype(np.float64)
    h = 1e-6
    fd = np.zeros((len(q), 3, 6))
    for j in range(6):
        e = np.zeros(6); e[j] = h
        fd[:, :, j] = (S.oracle_point(q + e) - S.oracle_point(q - e)) / (2 * h)
    d = np.abs(S.twin_jacobian(q, np.float64)["jacp"] - fd).max()
    print(f"[query-tol] fp64 twin jacp against finite differences: {d:.3e}")
    assert d <= 1e-8


# ---- the fp32 twin ------------------------------------------------------------------------------------------------------------------------------------
def test_fp32_twin_against_the_oracle():
    diff = S.max_abs_diff(twin_closed_form(np.float32), S.closed_form_reference())
    for k, d in diff.items():
        print(f"[query-tol] fp32 twin {k}: {d:.3e} (recorded {S.FP32_MEASURED[k]:.1e}, bound {S.FP32_BOUNDS[k]:.2e})")
    for k, d in diff.items():
        assert d <= S.FP32_BOUNDS[k], (k, d)


# ---- IK -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ik_results():
    q0, target, _ = S.ik_recipe()
    return {dt: S.twin_ik(q0, target, dt, **S.IK_DEFAULTS) for dt in (np.float64, np.float32)}


@pytest.mark.parametrize("dtype, repro", [(np.float64, 1e-9), (np.float32, 1e-5)])
def test_ik_converges(ik_results, dtype, repro):
    q0, target, _ = S.ik_recipe()
    r = ik_results[dtype]
    n = len(q0)
    unconverged = int(n - r["converged"].sum())
    print(f"[query-tol] IK {np.dtype(dtype).name}: {n - unconverged} of {n} converged, {r['iterations'].mean():.2f} iterations on average, "
          f"worst residual {r['residual'].max():.3e}")
    assert unconverged <= 0.02 * n
    # every case, converged or not: the oracle's FK of the returned q reproduces the reported residual
    dist = np.linalg.norm(target.astype(np.float64) - S.oracle_point(r["q"].astype(np.float64)), axis=1)
    assert np.abs(dist - r["residual"]).max() <= repro
    assert ((r["residual"] <= dtype(S.IK_DEFAULTS["tol"])) == (r["converged"] == 1)).all()
    rng = S.joint_range()
    assert (r["q"] >= rng[:, 0].astype(dtype)).all() and (r["q"] <= rng[:, 1].astype(dtype)).all()
    assert (r["q"][:, 5] == q0[:, 5].astype(dtype)).all()
    assert (r["iterations"] >= 0).all() and (r["iterations"] <= S.IK_DEFAULTS["iters"]).all()


def test_ik_fp32_and_fp64_twins_agree(ik_results):
    q0, target, _ = S.ik_recipe()
    r64, r32 = ik_results[np.float64], ik_results[np.float32]
    keep = S.flags_comparable(q0, target, r64, r64, r32)
    assert (~keep).sum() <= 0.01 * len(q0)
    assert (r64["converged"][keep] == r32["converged"][keep]).all() and (r64["iterations"][keep] == r32["iterations"][keep]).all()
    both = (r64["converged"] == 1) & (r32["converged"] == 1)
    d = np.abs(r64["q"] - r32["q"])[both].max()
    print(f"[query-tol] IK q, fp32 twin against fp64 twin on converged cases: {d:.3e} (recorded {S.IK_Q_MEASURED:.1e}, bound {S.IK_Q_BOUND:.2e})")
    assert d <= S.IK_Q_BOUND


def test_ik_other_links_and_a_start_outside_the_ranges():
    """link 2 with an offset: joints 3..5 keep q0's value (unclamped), joints 0..2 are clamped into their ranges before the first step"""
    q, _, _ = S.cases()
    q = q[:64].astype(np.float64)
    off = (0.0, 0.05, 0.02)
    target = S.oracle_point(q, 2, off)
    q0 = q + np.array([0.2, -0.2, 0.2, 9.0, -9.0, 9.0])
    r = S.twin_ik(q0, target, np.float64, link=2, offset=off)
    assert (r["q"][:, 3:] == q0[:, 3:]).all()
    rng = S.joint_range()
    assert (r["q"][:, :3] >= rng[:3, 0]).all() and (r["q"][:, :3] <= rng[:3, 1]).all()
    dist = np.linalg.norm(target - S.oracle_point(r["q"], 2, off), axis=1)
    assert np.abs(dist - r["residual"]).max() <= 1e-9
    assert r["converged"].mean() >= 0.9


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ik_on_an_unreachable_target(dtype):
    rng = S.joint_range()
    q0 = np.clip(np.array([[0.0, -1.57, 1.57, 1.0, 0.0, 0.0]]), rng[:, 0], rng[:, 1])
    target = np.array([[0.0, -2.0, 0.3]])
    r = S.twin_ik(q0, target, dtype, **S.IK_DEFAULTS)
    assert r["converged"][0] == 0 and r["iterations"][0] == S.IK_DEFAULTS["iters"]
    assert all(np.isfinite(r[k]).all() for k in r)
    dist = np.linalg.norm(target[0] - S.oracle_point(r["q"].astype(np.float64))[0])
    assert abs(dist - r["residual"][0]) <= 1e-6
