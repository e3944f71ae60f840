"""The control-limited LQR pass of tests/_lqrboxcheck/lqr_box.hpp (lqr_boxqp6 inside lqr_box_problem; box-DDP), on the host: its twin against
the numpy fp64 recursion whose QPs are solved by enumerating the active sets.  Inputs, reference and bounds: tests/lqr_box_support.py.  The
library has no such pass yet; the check functions here take any implementation's outputs.

A  the families on the reference alone: how much of SB is kept, what clamps where,
B  the twin against the reference on SB, AB and PB, fp64 and fp32, the clamped sets exactly,
C  identities: wide bounds = so100_query_lqr bit for bit, feasibility, zero rows, all clamped, iterations running out, u outside its bounds,
D  the failure cases,
F  the twin's exports and the stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lqr_box_support as X
import lqr_support as S

NS = (12, 24)
INTS = ("bad", "clamped", "qp_used")


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def worst(devs):
    return {name: max(d[name] for d in devs) for name in X.FLOAT_OUT}


# ---- A: the families, on the reference alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("T", X.SB_T)
def test_family_sb_keeps_enough_and_clamps_enough(n, T):
    """at most a quarter of the generated problems is left out for a margin under 1e-3, SB_M remain, and the retained steps include some with
    nothing clamped and some with at least two controls clamped"""
    p, ref, share = X.family_sb(n, T)
    count = X.count_clamped(ref["clamped"])
    print(f"[lqr-box-tol] SB n={n} T={T}: kept {share:.0%}; clamped per step min {count.min()} max {count.max()}, none in {np.mean(count == 0):.0%} of steps; "
          f"smallest margin kept {ref['margin'].min():.2e}")
    assert share >= 0.75 and p["A"].shape[1] == X.SB_M and (ref["margin"] >= X.MARGIN).all()
    assert (count == 0).any() and (count >= 2).any()
    S.assert_quu_is_well_conditioned(ref)


@pytest.mark.parametrize("n", NS)
def test_family_ab_clamps_every_control_at_both_kinds_of_bound(n):
    _, ref = X.family_ab(n)
    c = ref["clamped"]
    assert (X.count_clamped(c) == 6).all() and (c & 0x3F).any() and (c >> 8).any() and (ref["margin"] >= X.MARGIN).all() and (ref["bad"] == -1).all()


# ---- B: the twin against the reference ---------------------------------------------------------------------------------------------------------------------
def test_family_sb_twin_against_the_reference():
    """every n x T of family SB, all outputs: the clamped sets exactly, fp64 within 1e-11, fp32 within TWIN_FACTOR x the record; no step ran out of
    iterations"""
    d64, d32, used = [], [], []
    for n in NS:
        for T in X.SB_T:
            p, ref, _ = X.family_sb(n, T)
            for dtype, devs in ((np.float64, d64), (np.float32, d32)):
                g = X.twin(p, dtype)
                assert (g["bad"] == -1).all() and np.array_equal(g["clamped"], ref["clamped"]), (n, T, dtype)
                assert (g["qp_used"] >= 1).all() and (g["qp_used"] < X.RAN_OUT).all()
                devs.append(X.deviation(g, ref))
                used.append(g["qp_used"].mean())
    w64, w32 = worst(d64), worst(d32)
    print("[lqr-box-tol] SB fp64 " + " ".join(f"{k}={v:.2e}" for k, v in w64.items()))
    print("[lqr-box-tol] SB fp32 " + " ".join(f"{k}={v:.2e}" for k, v in w32.items()))
    print(f"[lqr-box-tol] SB mean qp_used {np.mean(used):.2f}")
    assert max(w64.values()) <= X.FP64_BOUND, w64
    X.within(w32, "SB", X.TWIN_FACTOR)


def test_family_ab_twin_against_the_reference():
    d64, d32 = [], []
    for n in NS:
        p, ref = X.family_ab(n)
        for dtype, devs in ((np.float64, d64), (np.float32, d32)):
            g = X.twin(p, dtype)
            assert (g["bad"] == -1).all() and np.array_equal(g["clamped"], ref["clamped"])
            devs.append(X.deviation(g, ref))
    w64, w32 = worst(d64), worst(d32)
    print("[lqr-box-tol] AB fp64 " + " ".join(f"{k}={v:.2e}" for k, v in w64.items()))
    print("[lqr-box-tol] AB fp32 " + " ".join(f"{k}={v:.2e}" for k, v in w32.items()))
    assert max(w64.values()) <= X.FP64_BOUND, w64
    X.within(w32, "AB", X.TWIN_FACTOR)


def test_family_pb_twin_against_the_reference():
    d64, d32 = [], []
    for n in NS:
        p = X.family_pb_cpu(n)
        ref = X.reference(p)
        count = X.count_clamped(ref["clamped"])
        print(f"[lqr-box-tol] PB n={n}: clamped per step min {count.min()} max {count.max()}; smallest margin {ref['margin'].min():.2e}, gradient scale "
              f"{ref['gscale'].min():.2e}..{ref['gscale'].max():.2e}, smallest margin / floor {(ref['margin']/X.pb_margin_floor(ref)).min():.1f}")
        assert (ref["bad"] == -1).all() and (count.max(axis=0) >= 1).all() and (ref["margin"] >= X.pb_margin_floor(ref)).all()
        for dtype, devs in ((np.float64, d64), (np.float32, d32)):
            g = X.twin(p, dtype)
            assert (g["bad"] == -1).all() and np.array_equal(g["clamped"], ref["clamped"])
            devs.append(X.deviation(g, ref))
    w64, w32 = worst(d64), worst(d32)
    print("[lqr-box-tol] PB fp64 " + " ".join(f"{k}={v:.2e}" for k, v in w64.items()))
    print("[lqr-box-tol] PB fp32 " + " ".join(f"{k}={v:.2e}" for k, v in w32.items()))
    assert max(w64.values()) <= X.FP64_BOUND, w64
    X.within(w32, "PB", X.TWIN_FACTOR)


# ---- C: identities ----------------------------------------------------------------------------------------------------------------------------------------
def check_wide_bounds(box, plain):
    """with bounds that never bind, the box pass is one full unclipped Newton step from 0: so100_query_lqr's bits in every output"""
    for name in S.OUT:
        assert bits(box[name]) == bits(plain[name]), name
    assert not box["clamped"].any() and (box["qp_used"] == 1).all()


def check_feasible(p, g):
    """lo <= k <= hi with lo and hi as the pass forms them, and u + du inside the bounds (to the rounding of that sum)"""
    dtype = g["k"].dtype.type
    u = p["u"].astype(dtype)
    lo, hi = dtype(p["u_lo"]) - u, dtype(p["u_hi"]) - u
    assert (g["k"] >= lo).all() and (g["k"] <= hi).all()
    new = u + g["du"]
    slack = 1e-12 if dtype == np.float64 else 1e-6
    assert new.min() >= p["u_lo"] - slack and new.max() <= p["u_hi"] + slack
    return lo, hi


def check_clamped_rows(g, lo, hi):
    """a clamped control sits exactly on the bound its bit names and its row of K is exactly 0; no control is on both lists"""
    c = g["clamped"]
    for j in range(6):
        low, up = ((c >> j) & 1).astype(bool), ((c >> (8 + j)) & 1).astype(bool)
        assert not (low & up).any()
        assert np.array_equal(g["k"][..., j][low], lo[..., j][low]) and np.array_equal(g["k"][..., j][up], hi[..., j][up])
        assert not g["K"][:, :, j][low | up].any()
    assert (c & ~0x3F3F).max() == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_wide_bounds_give_the_unconstrained_pass_bit_for_bit(n, dtype):
    for T in (1, 5, 16):
        p = dict(S.first(S.family_s(n, T), 5), u_lo=-1e6, u_hi=1e6)
        p["u"] = np.random.default_rng(7).uniform(-0.8, 0.8, (T, 5, 6)).astype(np.float32)
        check_wide_bounds(X.twin(p, dtype), S.twin(p, dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_wide_bounds_keep_the_sign_of_a_zero_gradient(zero, dtype):
    """a control that nothing moves (its column of B, its row of lux and its coupling in luu are zero: the example's jaw) with lu = +0 or -0 has
    Qu = +-0 exactly; the unconstrained pass gives k = -+0 there, and so does the box pass, to the sign bit"""
    T, M = 5, 3
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S.first(S.family_s(12, T), M).items()}
    p["B"][..., 5] = 0.0; p["lux"][:, :, 5] = 0.0; p["luu"][:, :, 5, :5] = 0.0; p["luu"][:, :, :5, 5] = 0.0
    p["lu"][..., 5] = zero
    p.update(u=np.zeros((T, M, 6), np.float32), u_lo=-1e6, u_hi=1e6)
    box, plain = X.twin(p, dtype), S.twin(p, dtype)
    assert not plain["k"][..., 5].any() and not plain["K"][:, :, 5].any()        # the case is what it says
    check_wide_bounds(box, plain)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_feasibility_and_clamped_rows(n, dtype):
    for T in X.SB_T:
        p, _, _ = X.family_sb(n, T)
        g = X.twin(p, dtype)
        check_clamped_rows(g, *check_feasible(p, g))


def check_all_clamped(p, g, tol):
    """family AB: K = 0, k is the bound itself, Vxx0 is the recursion without feedback"""
    u = p["u"].astype(g["k"].dtype)
    lo, hi = g["k"].dtype.type(p["u_lo"]) - u, g["k"].dtype.type(p["u_hi"]) - u
    assert not g["K"].any() and ((g["k"] == lo) | (g["k"] == hi)).all()
    want = X.value_without_feedback(p)
    assert np.abs(g["Vxx0"] - want).max()/max(1.0, np.abs(want).max()) <= tol


@pytest.mark.parametrize("n", NS)
def test_all_clamped(n):
    p, _ = X.family_ab(n)
    check_all_clamped(p, X.twin(p, np.float64), X.FP64_BOUND)
    check_all_clamped(p, X.twin(p, np.float32), X.TWIN_FACTOR*X.FP32_MEASURED_BOX["AB"]["Vxx0"])


def check_one_iteration(p, ref, g):
    """qp_iters = 1: one iteration everywhere.  At the last step, whose QP does not depend on what the other steps did, every problem where the
    reference clamps a control reports that the iterations ran out (from 0 the first set is empty and the unconstrained minimiser lies outside, so
    the full step is clipped), and every other one does not; the result is still feasible"""
    assert (g["bad"] == -1).all() and ((g["qp_used"] & 0xFFFF) == 1).all()
    where = X.count_clamped(ref["clamped"][-1]) > 0
    assert where.any() and (~where).any() and np.array_equal(g["qp_used"][-1], np.where(where, X.RAN_OUT | 1, 1))
    check_clamped_rows(g, *check_feasible(p, g))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_one_iteration_runs_out_where_the_reference_clamps(n, dtype):
    p, ref, _ = X.family_sb(n, 5)
    check_one_iteration(p, ref, X.twin(p, dtype, qp_iters=1))


OUTSIDE = ((1, 1, 2), (3, 1, 4))                          # (step, problem, control) of the controls that start outside


def outside_case(n):
    """family SB at T = 5, its first 3 problems, with two nominal controls 0.5 outside the bounds (1.5 and the bounds are exact in fp32), each on
    the side its step pushes towards in the reference of the unmodified problem -- so that the minimiser stays on the bound it is brought back
    to, which the test asserts on the reference of THIS problem: (the problem, the side of each: -1 or 1)"""
    base, ref, _ = X.family_sb(n, 5)
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in X.select(base, [0, 1, 2]).items()}
    sides = [1 if ref["k"][t, m, j] > 0 else -1 for t, m, j in OUTSIDE]
    for (t, m, j), side in zip(OUTSIDE, sides):
        p["u"][t, m, j] = 1.5*side
    return p, sides


def check_outside(p, sides, g):
    """finite throughout, and u + k of a control that starts outside lands on the bound it crossed, which `clamped` names"""
    assert (g["bad"] == -1).all() and all(np.isfinite(g[name]).all() for name in X.FLOAT_OUT)
    for (t, m, j), side in zip(OUTSIDE, sides):
        assert p["u"][t, m, j] + g["k"][t, m, j] == side
        assert (g["clamped"][t, m] >> (j + (8 if side > 0 else 0))) & 1
    check_clamped_rows(g, *check_feasible(p, g))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_a_nominal_control_outside_the_bounds_comes_back_to_its_bound(n, dtype):
    p, sides = outside_case(n)
    ref = X.reference(p)
    assert all((ref["clamped"][t, m] >> (j + (8 if side > 0 else 0))) & 1 for (t, m, j), side in zip(OUTSIDE, sides))      # the minimiser stays there
    check_outside(p, sides, X.twin(p, dtype))


# ---- D: the failure cases ---------------------------------------------------------------------------------------------------------------------------------
def with_u(p):
    T, M = p["A"].shape[:2]
    return dict(p, u=np.random.default_rng(8).uniform(-0.8, 0.8, (T, M, 6)).astype(np.float32))


def neighbours_untouched(got, clean):
    """problems 0 and 2 of a 3-problem call carry the bits of the clean call"""
    for name in X.OUT:
        g, c = got[name], clean[name]
        if name in ("Vx0", "Vxx0", "dV", "bad"):
            assert bits(g[[0, 2]]) == bits(c[[0, 2]]), name
        else:
            assert bits(g[:, [0, 2]]) == bits(c[:, [0, 2]]), name


def failed_outputs(got, m):
    """NaN in every float output of problem m, 0 in its clamped and qp_used"""
    for name in X.FLOAT_OUT:
        g = got[name]
        assert np.isnan(g[m] if name in ("Vx0", "Vxx0", "dV") else g[:, m]).all(), name
    assert not got["clamped"][:, m].any() and not got["qp_used"][:, m].any()


def failure_cases(n):
    """lqr_support's cases with nominal controls: (the clean problem, [(problem, the bad it must report)])"""
    p0, p4 = S.indefinite_case(n)
    return with_u(S.first(S.family_s(n, S.FAIL_T), S.FAIL_M)), with_u(p4), \
        [(with_u(p0), S.FAIL_AT)] + [(with_u(p), S.FAIL_T) for p in S.nonfinite_cases(n)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_failure_cases(n, dtype):
    """a negative luu: bad = t; a NaN or an inf: bad = T; the neighbours' bits untouched; regularisation mends the first"""
    base, mended, cases = failure_cases(n)
    clean = X.twin(base, dtype)
    assert (clean["bad"] == -1).all()
    for p, want in cases:
        g = X.twin(p, dtype)
        assert g["bad"].tolist() == [-1, want, -1] == X.reference(p)["bad"].tolist()
        failed_outputs(g, S.FAIL_PROBLEM)
        neighbours_untouched(g, clean)
    g4 = X.twin(mended, dtype)
    assert (g4["bad"] == -1).all() and (X.reference(mended)["bad"] == -1).all() and (g4["qp_used"] >= 1).all()


def test_a_bad_pivot_on_a_clamped_control_is_never_seen():
    """T = 1, B = 0, luu diagonal with -1 on control 2: so100_query_lqr fails the problem at t = 0.  With u_2 = 1.5 under bounds +-1 the box pass starts
    control 2 on its upper bound, lu_2 = -1 keeps it there (grad = -1 + 0.5 < 0), the masked factor never reads its pivot and the problem passes with
    that control clamped; with u_2 inside the bounds the first set is empty, the whole matrix is factored and the problem fails as before"""
    n, M = 12, 1
    z = lambda *shape: np.zeros(shape, np.float32)
    luu = np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]).astype(np.float32)[None, None]
    lu = z(1, M, 6); lu[..., 2] = -1.0
    A = np.ascontiguousarray(np.broadcast_to(np.eye(24, dtype=np.float32), (1, M, 24, 24)))
    lxx = np.ascontiguousarray(np.broadcast_to(np.eye(n, dtype=np.float32), (2, M, n, n)))
    u = z(1, M, 6); u[..., 2] = 1.5
    p = S.problem(A, z(1, M, 24, 6), z(2, M, n), lxx, lu, luu, None, nx=n, u=u)
    for dtype in (np.float64, np.float32):
        assert S.twin(p, dtype)["bad"].tolist() == [0]
        g = X.twin(p, dtype)
        assert g["bad"].tolist() == [-1] and g["clamped"].tolist() == [[1 << 10]] and g["k"][0, 0, 2] == -0.5 and not g["K"][0, 0, 2].any()
        inside = X.twin(dict(p, u=z(1, M, 6)), dtype)
        assert inside["bad"].tolist() == [0] and not inside["clamped"].any() and not inside["qp_used"].any()


# ---- F: the twin ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_twin_exports_what_the_support_module_declares():
    """the extern "C" definitions of tests/_lqrboxcheck/lqrboxcheck.cpp are exactly the table the loader gives signatures to"""
    import test_hostlibs as H
    src = H.expand_macros(re.sub(r"//[^\n]*", "", open(os.path.join(X.HERE, "_lqrboxcheck", "lqrboxcheck.cpp")).read()))
    found = {}
    for ret, name, params in re.findall(r"^\s*(void)\s+(lb_\w+)\s*\(([^)]*)\)\s*\{", src, flags=re.M):
        found[name] = (None, [C.c_void_p if "*" in prm else H.SCALARS[" ".join(prm.split()[:-1])] for prm in (x.strip() for x in params.split(","))])
    assert found == X.LQRBOXCHECK
    lib = X.lqrboxcheck()
    assert all(list(getattr(lib, name).argtypes) == args for name, (_, args) in found.items())


def test_stand_alone_program_builds_and_passes(tmp_path):
    """the program a host sanitizer run uses (make -C tests/_lqrboxcheck selftest SAN=...), here without a sanitizer"""
    run = subprocess.run(["make", "-C", os.path.join(X.HERE, "_lqrboxcheck"), "-s", "selftest", f"BUILD={tmp_path}"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    for precision in ("double", "float"):
        assert re.search(r"lqrboxcheck selftest \(%s\):.*: ok$" % precision, run.stdout, flags=re.M), run.stdout
