"""The LQR query (include/so100_query.h: so100_query_lqr) without a GPU: the ABI surface, and the host twin of csrc/so100_lqr.hpp -- the
recursion the kernel deals over a wave -- against the numpy fp64 recursion and the dense minimiser.  Inputs, references and bounds:
tests/lqr_support.py; the same checks on the kernel: tests/test_gpu_lqr.py.

A  the twin against the reference on family S (synthetic) at T in {1, 2, 5, 16, 64} and on family P (physics), fp64 and fp32,
B  identities: du = the dense minimiser, the T = 1 known answer, dV1 + dV2 = the model at (du, dx), clamping, alpha = 0, nullable costs = zeros,
   the arm form = the full form with an identity cube block,
C  the failure cases,
F  the surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lqr_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "so100_query.h")
NS = (12, 24)


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- F: the surface ---------------------------------------------------------------------------------------------------------------------------------
C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
FIELDS = ["nx", "T", "A_dev", "B_dev", "lx_dev", "lxx_dev", "lu_dev", "luu_dev", "lux_dev", "u_dev", "dx0_dev", "reg", "alpha", "u_lo", "u_hi", "k_dev", "K_dev",
          "Vx0_dev", "Vxx0_dev", "dV_dev", "du_dev", "dx_dev", "bad_dev"]


def test_struct_matches_the_header_field_for_field():
    from so100_mujoco_rl_amd import lib
    body = re.search(r"typedef struct \{([^}]*)\} so100_lqr_io;", header_text()).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, name = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", decl).groups()
            fields.append((name, C_TYPES[re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()]))
    assert fields == list(lib.LqrIO._fields_) and [f[0] for f in fields] == FIELDS
    assert lib.QUERY_IO["so100_query_lqr"] is lib.LqrIO and "so100_query_lqr" in lib.QUERY_EXPORTS
    assert re.search(r"int so100_query_lqr\(so100_sim\* sim, const so100_lqr_io\* io, int32_t M, void\* hip_stream\);", header_text())
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_macros_match_the_header():
    from so100_mujoco_rl_amd import lib
    macro = lambda name: int(re.search(r"#define %s\s+(\d+)\b" % name, header_text()).group(1))
    assert (macro("SO100_LQR_NU"), macro("SO100_LQR_MAX_T")) == (lib.LQR_NU, lib.LQR_MAX_T) == (S.NU, 4096)
    assert (macro("SO100_DERIV_NX"), macro("SO100_DERIV_NU")) == (24, 6)            # the layout of A and B


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    assert L.so100_query_lqr(None, C.byref(lib.LqrIO()), 1, None) == -1
    assert L.so100_last_error() == b"so100_query_lqr: null argument"


# ---- A: the twin against the fp64 recursion -------------------------------------------------------------------------------------------------------------
def worst(devs):
    return {name: max(d[name] for d in devs) for name in S.FLOAT_OUT}


def test_family_s_twin_against_the_reference():
    """every n x T of family S, all outputs (the forward pass from dx0 = 0 under alpha = 1, no bounds): fp64 within 1e-11, fp32 within TWIN_FACTOR x
    the record; the reference's Quu is well conditioned throughout"""
    d64, d32 = [], []
    for n in NS:
        for T in S.S_T:
            p, ref = S.family_s(n, T), S.reference_s(n, T)
            assert (ref["bad"] == -1).all()
            S.assert_quu_is_well_conditioned(ref)
            g64, g32 = S.twin(p, np.float64), S.twin(p, np.float32)
            assert (g64["bad"] == -1).all() and (g32["bad"] == -1).all()
            d64.append(S.deviation(g64, ref)); d32.append(S.deviation(g32, ref))
    w64, w32 = worst(d64), worst(d32)
    print("[lqr-tol] S fp64 " + " ".join(f"{k}={v:.2e}" for k, v in w64.items()))
    print("[lqr-tol] S fp32 " + " ".join(f"{k}={v:.2e}" for k, v in w32.items()))
    assert max(w64.values()) <= S.FP64_BOUND, w64
    S.within(w32, "S", S.TWIN_FACTOR)


def test_family_p_twin_against_the_reference():
    d64, d32 = [], []
    for n in NS:
        p = S.family_p_cpu(n)
        ref = S.reference(p)
        assert (ref["bad"] == -1).all()
        e = ref["eig"]
        print(f"[lqr-tol] P n={n} smallest Quu_r eigenvalue ratio {float((e[..., 0]/e[..., 1]).min()):.2e}")
        g64, g32 = S.twin(p, np.float64), S.twin(p, np.float32)
        assert (g64["bad"] == -1).all() and (g32["bad"] == -1).all()
        d64.append(S.deviation(g64, ref)); d32.append(S.deviation(g32, ref))
    w64, w32 = worst(d64), worst(d32)
    print("[lqr-tol] P fp64 " + " ".join(f"{k}={v:.2e}" for k, v in w64.items()))
    print("[lqr-tol] P fp32 " + " ".join(f"{k}={v:.2e}" for k, v in w32.items()))
    assert max(w64.values()) <= S.FP64_BOUND, w64
    S.within(w32, "P", S.TWIN_FACTOR)


# ---- B: identities ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("T", S.S_T)
def test_du_is_the_dense_minimiser(n, T):
    """reg = 0, alpha = 1, no bounds, dx0 = 0: the forward pass's du against one np.linalg.solve of the condensed problem -- the fp64 recursion to 2e-11
    (what it gave when the family was chosen), the fp64 twin likewise, the fp32 twin within the du record"""
    p = S.first(S.family_s(n, T), 5)
    dense = S.dense_minimiser(p)
    scale = max(1.0, np.abs(dense).max())
    ref = S.reference(p)
    assert np.abs(ref["du"] - dense).max()/scale <= 2e-11
    assert np.abs(S.twin(p, np.float64)["du"] - dense).max()/scale <= 2e-11
    assert np.abs(S.twin(p, np.float32)["du"] - dense).max()/scale <= S.TWIN_FACTOR*S.FP32_MEASURED["S"]["du"]


@pytest.mark.parametrize("n", NS)
def test_known_answer_at_horizon_one(n):
    """T = 1: k = -(luu + B' lxx_1 B)^-1 (lu + B' lx_1)"""
    p = S.first(S.family_s(n, 1), 5)
    A, B, lx, lxx, lu, luu, lux = S._f64(p)
    want = np.stack([-np.linalg.solve(luu[0, m] + B[0, m].T @ lxx[1, m] @ B[0, m], lu[0, m] + B[0, m].T @ lx[1, m]) for m in range(5)])
    assert np.abs(S.twin(p, np.float64)["k"][0] - want).max() <= 1e-12*max(1.0, np.abs(want).max())


@pytest.mark.parametrize("n", NS)
def test_value_decrease_is_the_model_at_the_step(n):
    """dV1 + dV2 = the quadratic model evaluated at the returned du, dx (alpha = 1, reg = 0, dx0 = 0, no bounds)"""
    p = S.first(S.family_s(n, 16), 5)
    g = S.twin(p, np.float64)
    m = S.model_value(p, g["du"], g["dx"])
    assert np.abs(g["dV"].sum(axis=1) - m).max() <= 1e-11*max(1.0, np.abs(m).max())


@pytest.mark.parametrize("n", NS)
def test_clamping_keeps_the_controls_in_their_bounds(n):
    """with u: every u + du lies in [u_lo, u_hi]; a control whose unclamped value (at the returned dx) is interior is that value, every other one
    sits on its bound; the gains are those of the call without u"""
    p = dict(S.first(S.family_s(n, 5), 9))
    u = np.random.default_rng(3).uniform(-0.6, 0.6, (5, 9, 6)).astype(np.float32)
    free = S.twin(p, np.float64)
    p["u"], p["u_lo"], p["u_hi"] = u, -0.75, 0.5
    g = S.twin(p, np.float64)
    new = u + g["du"]
    assert new.min() >= -0.75 - 1e-12 and new.max() <= 0.5 + 1e-12
    want = p["alpha"]*g["k"] + np.einsum("tmij,tmj->tmi", g["K"], g["dx"][:5])          # the unclamped control change at the returned dx
    interior = (u + want > -0.75) & (u + want < 0.5)
    assert interior.any() and (~interior).any()
    assert np.abs(g["du"] - want)[interior].max() <= 1e-12
    assert np.array_equal(new[~interior], np.clip(u + want, -0.75, 0.5)[~interior])
    assert bits(g["k"]) == bits(free["k"]) and bits(g["K"]) == bits(free["K"])            # the backward pass does not see u


@pytest.mark.parametrize("n", NS)
def test_alpha_zero_from_the_origin_moves_nothing(n):
    p = dict(S.first(S.family_s(n, 5), 5)); p["alpha"] = 0.0
    for dtype in (np.float64, np.float32):
        g = S.twin(p, dtype)
        assert not g["du"].any() and not g["dx"].any() and g["k"].any()


@pytest.mark.parametrize("n", NS)
def test_null_costs_are_explicit_zeros(n):
    p = dict(S.first(S.family_s(n, 5), 5))
    T, M = 5, 5
    p["luu"] = p["luu"] + p["lux"] @ np.swapaxes(p["lux"], 2, 3)                            # keeps Quu positive definite without the cross term
    zero = dict(p, lu=np.zeros((T, M, 6), np.float32), lux=np.zeros((T, M, 6, n), np.float32))
    null = dict(p, lu=None, lux=None)
    for dtype in (np.float64, np.float32):
        a, b = S.twin(zero, dtype), S.twin(null, dtype)
        assert all(bits(a[k]) == bits(b[k]) for k in S.OUT) and (a["bad"] == -1).all()
    # luu: null against zeros needs a Quu that stands without it -- no cross term either, Quu = B'Vxx B
    zero = dict(p, luu=np.zeros((T, M, 6, 6), np.float32), lux=None); null = dict(p, luu=None, lux=None)
    a, b = S.twin(zero, np.float32), S.twin(null, np.float32)
    assert all(bits(a[k]) == bits(b[k]) for k in S.OUT) and (a["bad"] == -1).all()


def test_arm_form_is_the_full_form_with_an_identity_cube_block():
    """A, B whose cube rows and columns are the identity and zero (what F_CUBE_PINNED gives): the n = 12 call on them equals the n = 24 call on the
    embedded cost, restricted to the arm indices -- k, the arm columns of K, Vx0, Vxx0, dV, du"""
    p12 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S.first(S.family_s(12, 5), 5).items()}
    T, M = 5, 5
    cube = np.setdiff1d(np.arange(24), S.ARM)
    p12["A"][:, :, cube, :] = 0.0; p12["A"][:, :, :, cube] = 0.0; p12["A"][:, :, cube, cube] = 1.0; p12["B"][:, :, cube] = 0.0
    lx = np.zeros((T + 1, M, 24), np.float32); lx[:, :, S.ARM] = p12["lx"]
    lxx = np.zeros((T + 1, M, 24, 24), np.float32); lxx[np.ix_(range(T + 1), range(M), S.ARM, S.ARM)] = p12["lxx"]
    lux = np.zeros((T, M, 6, 24), np.float32); lux[:, :, :, S.ARM] = p12["lux"]
    p24 = dict(p12, lx=lx, lxx=lxx, lux=lux, nx=24)
    a, b = S.twin(p12, np.float64), S.twin(p24, np.float64)
    assert (a["bad"] == -1).all() and (b["bad"] == -1).all()
    close = lambda x, y: np.abs(x - y).max() <= 1e-11*max(1.0, np.abs(y).max())
    assert close(a["k"], b["k"]) and close(a["K"], b["K"][..., S.ARM]) and np.abs(b["K"][..., cube]).max() <= 1e-11
    assert close(a["Vx0"], b["Vx0"][:, S.ARM]) and close(a["Vxx0"], b["Vxx0"][:, S.ARM][:, :, S.ARM]) and close(a["dV"], b["dV"]) and close(a["du"], b["du"])
    assert close(a["dx"], b["dx"][..., S.ARM])


# ---- C: the failure cases -------------------------------------------------------------------------------------------------------------------------------
def neighbours_untouched(got, clean):
    """problems 0 and 2 of a 3-problem call carry the bits of the clean call"""
    for name in S.OUT:
        g, c = got[name], clean[name]
        if name in ("Vx0", "Vxx0", "dV", "bad"):
            assert bits(g[[0, 2]]) == bits(c[[0, 2]]), name
        else:
            assert bits(g[:, [0, 2]]) == bits(c[:, [0, 2]]), name


def failed_outputs_are_nan(got, m):
    for name in S.FLOAT_OUT:
        g = got[name]
        assert np.isnan(g[m] if name in ("Vx0", "Vxx0", "dV") else g[:, m]).all(), name


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_indefinite_quu_fails_at_its_step_and_regularisation_mends_it(n, dtype):
    p0, p4 = S.indefinite_case(n)
    clean = S.twin(S.first(S.family_s(n, S.FAIL_T), S.FAIL_M), dtype)
    g = S.twin(p0, dtype)
    assert g["bad"].tolist() == [-1, S.FAIL_AT, -1] == S.reference(p0)["bad"].tolist()
    failed_outputs_are_nan(g, S.FAIL_PROBLEM)
    neighbours_untouched(g, clean)
    g4, ref4 = S.twin(p4, dtype), S.reference(p4)
    assert (g4["bad"] == -1).all() and (ref4["bad"] == -1).all()
    dev = S.deviation(g4, ref4)
    if dtype == np.float64:
        assert max(dev.values()) <= S.FP64_BOUND, dev
    else:
        S.within(dev, "S", S.TWIN_FACTOR)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_non_finite_inputs_fail_with_the_horizon(n, dtype):
    clean = S.twin(S.first(S.family_s(n, S.FAIL_T), S.FAIL_M), dtype)
    for p in S.nonfinite_cases(n):
        g = S.twin(p, dtype)
        assert g["bad"].tolist() == [-1, S.FAIL_T, -1] == S.reference(p)["bad"].tolist()
        failed_outputs_are_nan(g, S.FAIL_PROBLEM)
        neighbours_untouched(g, clean)
