"""The LQR query with a regulariser per problem and its schedule (include/so100_query.h: so100_query_lqr_reg, so100_query_reg_schedule) without a
GPU: the ABI surface, and the host twin of csrc/so100_lqr.hpp's lqr_reg_problem -- the retry loop the kernel runs inside a wave -- against the
numpy retry loop round the fp64 recursion.  Inputs, references and bounds: tests/lqr_reg_support.py; the same checks on the kernel:
tests/test_gpu_lqr_reg.py.

A  the retry case and its variants, fp64 and fp32: integers and regs exact, floats against the reference,
B  the two identities, bit for bit,
C  raise and the schedule's table, exact,
F  the surface.  Only the null-argument check can be reached without a handle, and a handle needs a device: the order and the messages of the
   other checks are in tests/test_gpu_lqr_reg.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lqr_reg_support as R
import lqr_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "so100_query.h")
NS = (12, 24)


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def problem_of(out, m):
    """problem m's part of every output present"""
    return {k: (v[m] if k in ("Vx0", "Vxx0", "dV", "bad", "reg_used", "tries") else v[:, m]) for k, v in out.items() if k in R.OUT}


def check_against(got, ref, dtype):
    """integers and regs exact; floats of the problems that got through against the reference; those of the others NaN"""
    assert got["bad"].tolist() == ref["bad"].tolist() and got["tries"].tolist() == ref["tries"].tolist()
    assert bits(got["reg_used"].astype(np.float32)) == bits(ref["reg_used"])
    ok = np.flatnonzero(ref["bad"] < 0)
    for m in np.flatnonzero(ref["bad"] >= 0):
        S_failed(got, m)
    dev = R.deviation(R.select({k: got[k] for k in R.FLOAT_OUT}, ok), R.select({k: ref[k] for k in R.FLOAT_OUT}, ok))
    if dtype == np.float64:
        assert max(dev.values()) <= R.FP64_BOUND, dev
    else:
        R.within(dev, R.TWIN_FACTOR)
    return dev


def S_failed(got, m):
    for name in R.FLOAT_OUT:
        g = got[name]
        assert np.isnan(g[m] if name in ("Vx0", "Vxx0", "dV") else g[:, m]).all(), name


# ---- F: the surface ---------------------------------------------------------------------------------------------------------------------------------
C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p, "uint8_t*": C.c_void_p, "int32_t": C.c_int32,
           "float": C.c_float}


def header_fields(struct, nested):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header_text()).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, name = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", decl).groups()
            ctype = re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()
            fields.append((name, nested[ctype] if ctype in nested else C_TYPES[ctype]))
    return fields


def test_structs_match_the_header_field_for_field():
    from so100_mujoco_rl_amd import lib
    assert header_fields("so100_lqr_reg_io", {"so100_lqr_io": lib.LqrIO}) == list(lib.LqrRegIO._fields_)
    assert [f[0] for f in lib.LqrRegIO._fields_] == ["base", "reg_dev", "reg_min", "reg_max", "reg_up", "tries", "reg_used_dev", "tries_dev"]
    assert header_fields("so100_reg_schedule_io", {}) == list(lib.RegScheduleIO._fields_)
    assert [f[0] for f in lib.RegScheduleIO._fields_] == ["reg_used_dev", "best_dev", "keep", "reg_min", "reg_max", "reg_up", "reg_down", "reg_dev", "improved_dev"]
    for fn, cls, struct in (("so100_query_lqr_reg", lib.LqrRegIO, "so100_lqr_reg_io"), ("so100_query_reg_schedule", lib.RegScheduleIO, "so100_reg_schedule_io")):
        assert lib.QUERY_IO[fn] is cls and fn in lib.QUERY_EXPORTS
        assert re.search(r"int %s\(so100_sim\* sim, const %s\* io, int32_t M, void\* hip_stream\);" % (fn, struct), header_text())
    assert int(re.search(r"#define SO100_LQR_REG_MAX_TRIES\s+(\d+)\b", header_text()).group(1)) == lib.LQR_REG_MAX_TRIES == 16
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    for fn, cls in (("so100_query_lqr_reg", lib.LqrRegIO), ("so100_query_reg_schedule", lib.RegScheduleIO)):
        for call in (lambda: getattr(L, fn)(None, C.byref(cls()), 1, None), lambda: getattr(L, fn)(None, None, 1, None)):
            assert call() == -1
            assert L.so100_last_error() == (fn + ": null argument").encode()


# ---- A: the retry case ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_the_retry_case(n, dtype):
    """problem 1 fails at step 2 under 0, 0.125 and 0.5 and goes through under 2; its neighbours take one pass under 0"""
    p, ref = R.retry_case(n)
    got = R.twin(p, dtype, **R.KNOBS)
    assert got["tries"].tolist() == [1, 4, 1] and got["reg_used"].tolist() == [0.0, 2.0, 0.0] and got["bad"].tolist() == [-1, -1, -1]
    dev = check_against(got, ref, dtype)
    print(f"[lqr-reg-tol] retry n={n} {np.dtype(dtype).name} " + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_the_retry_gives_up_where_tries_or_reg_max_say_so(n, dtype):
    p, _ = R.retry_case(n)
    for knobs in (dict(R.KNOBS, tries=3), dict(R.KNOBS, tries=8, reg_max=0.5)):
        ref = R.reference(p, **knobs)
        R.assert_premises(ref, S.FAIL_T)
        got = R.twin(p, dtype, **knobs)
        assert got["bad"].tolist() == [-1, S.FAIL_AT, -1] and got["reg_used"][1] == 0.5 and got["tries"].tolist() == [1, 3, 1]
        check_against(got, ref, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_regs_per_problem(n, dtype):
    """[0, 2, 0] with one try: problem 1 passes at once; a NaN or a negative start: no pass, tries = 0, reg_used = NaN, its neighbours untouched"""
    p, _ = R.retry_case(n)
    one = dict(R.KNOBS, tries=1)
    start = np.array([0.0, 2.0, 0.0], np.float32)
    ref = R.reference(p, start, **one)
    got = R.twin(p, dtype, start, **one)
    assert got["bad"].tolist() == [-1, -1, -1] and got["tries"].tolist() == [1, 1, 1] and got["reg_used"].tolist() == [0.0, 2.0, 0.0]
    check_against(got, ref, dtype)
    for value in (np.nan, -1.0):
        start = np.array([value, 2.0, 0.0], np.float32)
        bad = R.twin(p, dtype, start, **R.KNOBS)
        assert bad["bad"].tolist() == [S.FAIL_T, -1, -1] and bad["tries"].tolist() == [0, 1, 1] and np.isnan(bad["reg_used"][0]) and bad["reg_used"][1:].tolist() == [2.0, 0.0]
        S_failed(bad, 0)
        check_against(bad, R.reference(p, start, **R.KNOBS), dtype)
        for m in (1, 2):
            a, b = problem_of(bad, m), problem_of(got, m)
            assert all(bits(a[k]) == bits(b[k]) for k in R.OUT), m


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_a_non_finite_input_is_found_by_the_first_pass_and_not_retried(n, dtype):
    for p in S.nonfinite_cases(n):
        got = R.twin(p, dtype, **R.KNOBS)
        assert got["bad"].tolist() == [-1, S.FAIL_T, -1] and got["tries"].tolist() == [1, 1, 1] and got["reg_used"].tolist() == [0.0, 0.0, 0.0]
        S_failed(got, S.FAIL_PROBLEM)


# ---- B: the identities ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("n", NS)
def test_one_try_without_regs_is_the_plain_query(n, T):
    for M in (1, 3):
        p = dict(S.first(S.family_s(n, T), M), reg=0.25)
        for dtype in (np.float64, np.float32):
            a, b = R.twin(p, dtype, reg_min=0.125, reg_max=32.0, reg_up=4.0, tries=1), S.twin(p, dtype)
            assert all(bits(a[k]) == bits(b[k]) for k in S.OUT), (M, dtype)
            assert (a["tries"] == 1).all() and (a["reg_used"] == 0.25).all()


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("n", NS)
def test_a_problem_that_succeeds_is_the_plain_query_alone_under_reg_used(n, T):
    """family S, and the retry case where T is its horizon: each problem's float outputs are lqr_problem's for that problem alone under reg_used"""
    cases = [(S.first(S.family_s(n, T), 3), np.array([0.0, 0.7, 3.0], np.float32))] + ([(R.retry_case(n)[0], None)] if T == S.FAIL_T else [])
    for p, start in cases:
        for dtype in (np.float64, np.float32):
            got = R.twin(p, dtype, start, **R.KNOBS)
            assert (got["bad"] == -1).all()
            for m in range(3):
                alone = S.twin(dict(R.select(p, [m]), reg=float(got["reg_used"][m])), dtype)
                a, b = problem_of(got, m), problem_of(alone, 0)
                assert all(bits(a[k]) == bits(b[k]) for k in S.FLOAT_OUT), (m, dtype)


# ---- C: raise and the schedule ----------------------------------------------------------------------------------------------------------------------------
def test_raise():
    k = (0.125, 32.0, 4.0)
    assert R.twin_raise(0.0, *k) == np.float32(0.125) == R.raise32(0.0, *k)           # raise(0) = reg_min
    for r in (0.01, 0.125, 0.3, 2.0, 7.9, 8.0, 8.1, 32.0, 100.0):
        assert R.twin_raise(r, *k) == R.raise32(np.float32(r), *k), r
    assert R.twin_raise(0.3, 0.125, 32.0, 1.1) == np.float32(0.3)*np.float32(1.1)     # the product rounded once in fp32


@pytest.mark.parametrize("alias", [False, True])
def test_the_schedule_table(alias):
    reg_used, best, want, improved = R.schedule_table()
    ref, ref_imp = R.schedule_reference(reg_used, best, R.SCHEDULE_KEEP, **R.SCHEDULE_KNOBS)
    assert bits(ref) == bits(want) and bits(ref_imp) == bits(improved)                 # the reference against the table written out by hand
    got, imp = R.twin_schedule(reg_used, best, R.SCHEDULE_KEEP, alias=alias, **R.SCHEDULE_KNOBS)
    assert bits(got) == bits(want) and bits(imp) == bits(improved)
    # keep = -1: no candidate is the old plan, so every best >= 0 improved
    got, imp = R.twin_schedule(reg_used, best, -1, **R.SCHEDULE_KNOBS)
    ref, ref_imp = R.schedule_reference(reg_used, best, -1, **R.SCHEDULE_KNOBS)
    assert bits(got) == bits(ref) and bits(imp) == bits(ref_imp) and imp.tolist() == [0]*6 + [1]*12
