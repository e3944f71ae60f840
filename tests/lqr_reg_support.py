"""Shared by tests/test_lqr_reg_cpu.py and tests/test_gpu_lqr_reg.py: the host twin of the LQR query with a regulariser per problem and of its
schedule (tests/_lqrregcheck, built by the Makefile beside it: lqr_reg_problem, lqr_reg_raise and lqr_reg_next of csrc/so100_lqr.hpp), the retry
case, the references and the bounds.

References.  reference(): the retry loop of include/so100_query.h (so100_lqr_reg_io) in numpy round lqr_support.reference -- each pass is the fp64
recursion on the problems still running, under their own reg -- with the regs carried as np.float32, so that reg_used compares exactly.
schedule_reference(): the rule of so100_reg_schedule_io in np.float32: its results compare exactly.  Neither the twin nor the kernel is ever its
own reference.  Inputs and references are computed once per process and never modified."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import lqr_support as S
from hostlibs import ptr
from lqr_box_support import select

NU = S.NU
FLOAT_OUT = S.FLOAT_OUT
OUT = S.OUT + ("reg_used", "tries")
HERE = os.path.dirname(os.path.abspath(__file__))
# the retry case's knobs: the ladder from 0 is 0, 0.125, 0.5, 2, 8, 32
KNOBS = dict(reg_min=0.125, reg_max=32.0, reg_up=4.0, tries=4)
REG_DOWN = 0.25

_p, _i, _l, _f, _d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double
LQRREGCHECK = {"lr_lqr_reg_d": (None, [_l, _i, _i] + [_p]*9 + [_d]*4 + [_p] + [_d]*3 + [_i] + [_p]*10),
               "lr_lqr_reg_f": (None, [_l, _i, _i] + [_p]*9 + [_f]*4 + [_p] + [_f]*3 + [_i] + [_p]*10),
               "lr_raise_f": (_f, [_f]*4),
               "lr_schedule_f": (None, [_l, _p, _p, _i] + [_f]*4 + [_p, _p])}


@functools.lru_cache(maxsize=None)
def lqrregcheck():
    """tests/_lqrregcheck/liblqrregcheck.so, made and loaded once, every symbol with its signature"""
    d = os.path.join(HERE, "_lqrregcheck")
    subprocess.check_call(["make", "-C", d, "-s", "liblqrregcheck.so"])
    lib = C.CDLL(os.path.join(d, "liblqrregcheck.so"))
    for name, (restype, argtypes) in LQRREGCHECK.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def shapes(p):
    T, M, n, shp = S.shapes(p)
    return T, M, n, dict(shp, reg_used=(M,), tries=(M,))


def twin(p, dtype=np.float32, reg=None, *, reg_min, reg_max, reg_up, tries):
    """the host twin on a lqr_support.problem(); reg: [M] starting regs or None (p["reg"] for all).  Every output, as numpy arrays of `dtype`
    (bad, tries: int32)"""
    lib = lqrregcheck()
    T, M, n, shp = shapes(p)
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    ins = [cast(p[k]) for k in ("A", "B", "lx", "lxx", "lu", "luu", "lux", "u", "dx0")]
    out = {k: np.zeros(shp[k], np.int32 if k in ("bad", "tries") else dtype) for k in OUT}
    fn = lib.lr_lqr_reg_d if dtype == np.float64 else lib.lr_lqr_reg_f
    fn(M, n, T, *[ptr(a) for a in ins], p["reg"], p["alpha"], p["u_lo"], p["u_hi"], ptr(cast(reg)), reg_min, reg_max, reg_up, tries, *[ptr(out[k]) for k in OUT])
    return out


def raise32(r, reg_min, reg_max, reg_up):
    """raise(r) of so100_lqr_reg_io in np.float32: the product rounded once"""
    f = np.float32
    return np.minimum(f(reg_max), np.maximum(f(reg_min), np.asarray(r, f)*f(reg_up)))


def twin_raise(r, reg_min, reg_max, reg_up):
    return np.float32(lqrregcheck().lr_raise_f(r, reg_min, reg_max, reg_up))


# ---- the reference: the retry loop in numpy, each pass the fp64 recursion of lqr_support --------------------------------------------------------------
def reference(p, reg=None, *, reg_min, reg_max, reg_up, tries):
    """the outputs in fp64 (reg_used: float32, bad and tries: int32) plus "passes": per pass a list of (the problems that ran it, their reg, the
    lqr_support.reference of those problems under it) -- the eigenvalues the premises are asserted on"""
    T, M, n, shp = shapes(p)
    r = np.full(M, p["reg"], np.float32) if reg is None else np.array(reg, np.float32)
    out = {k: np.full(shp[k], np.nan) for k in FLOAT_OUT}
    bad = np.full(M, T, np.int32); ran = np.zeros(M, np.int32); used = np.full(M, np.nan, np.float32)
    active = np.isfinite(r) & (r >= 0)
    passes = []
    for a in range(1, tries + 1):
        if not active.any():
            break
        this = []
        for value in np.unique(r[active]):
            idx = np.flatnonzero(active & (r == value))
            ref = S.reference(dict(select(p, idx), reg=float(value)))
            for k in FLOAT_OUT:
                if k in ("Vx0", "Vxx0", "dV"):
                    out[k][idx] = ref[k]
                else:
                    out[k][:, idx] = ref[k]
            bad[idx] = ref["bad"]
            this.append((idx, np.float32(value), ref))
        passes.append(this)
        ran[active], used[active] = a, r[active]
        active = active & (bad >= 0) & (bad < T) & (a < tries) & (r < np.float32(reg_max))
        r[active] = raise32(r[active], reg_min, reg_max, reg_up)
    return dict(out, bad=bad, tries=ran, reg_used=used, passes=passes)


def assert_premises(ref, T):
    """on the fp64 reference alone: wherever a pass fails at a step, that step's smallest eigenvalue of Quu + reg I is <= BAD_EIG, and every other
    Quu_r a pass factors has an eigenvalue ratio >= GOOD_RATIO -- so fp32 and fp64 cannot disagree on any decision"""
    for this in ref["passes"]:
        for idx, _, r in this:
            e = r["eig"]
            for j in range(len(idx)):
                t = int(r["bad"][j])
                assert t != T                                    # no premise covers a non-finite input: such cases are not passed here
                good = e[t + 1:, j] if t >= 0 else e[:, j]
                assert (good[:, 0]/good[:, 1] >= S.GOOD_RATIO).all(), (idx[j], t, good)
                if t >= 0:
                    assert e[t, j, 0] <= S.BAD_EIG, (idx[j], t, e[t, j])


@functools.lru_cache(maxsize=None)
def retry_case(n):
    """lqr_support.indefinite_case(n)[0] (T = 5, M = 3, luu = -I at step 2 of problem 1, reg = 0) and its reference under KNOBS, the premises
    asserted: problem 1 fails at step 2 under 0, 0.125 and 0.5 and goes through under 2"""
    p = S.indefinite_case(n)[0]
    ref = reference(p, **KNOBS)
    assert_premises(ref, S.FAIL_T)
    assert ref["tries"].tolist() == [1, 4, 1] and ref["reg_used"].tolist() == [0.0, 2.0, 0.0] and ref["bad"].tolist() == [-1, -1, -1]
    return p, ref


def embedded_case(n, place, M=65):
    """family S at T = 5 and M problems with the retry problem (problem 1 of retry_case) in `place`"""
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S.first(S.family_s(n, S.FAIL_T), M).items()}
    q = S.indefinite_case(n)[0]
    for name in ("A", "B", "lx", "lxx", "lu", "luu", "lux"):
        p[name][:, place] = q[name][:, S.FAIL_PROBLEM]
    return p


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------------------------
def schedule_reference(reg_used, best, keep, reg_min, reg_max, reg_up, reg_down):
    """(reg [M] float32, improved [M] uint8) by the rule of so100_reg_schedule_io, in np.float32"""
    f = np.float32
    r = np.array(reg_used, f)
    r[~(np.isfinite(r) & (r >= 0))] = 0
    improved = (np.asarray(best) >= 0) & (np.asarray(best) != keep)
    down = r*f(reg_down)
    down[down < f(reg_min)] = 0
    return np.where(improved, down, raise32(r, reg_min, reg_max, reg_up)).astype(f), improved.astype(np.uint8)


def twin_schedule(reg_used, best, keep, reg_min, reg_max, reg_up, reg_down, alias=False):
    ru = np.ascontiguousarray(reg_used, np.float32).copy(); bs = np.ascontiguousarray(best, np.int32)
    reg = ru if alias else np.full(len(ru), -7.0, np.float32)
    imp = np.full(len(ru), 9, np.uint8)
    lqrregcheck().lr_schedule_f(len(ru), ptr(ru), ptr(bs), keep, reg_min, reg_max, reg_up, reg_down, ptr(reg), ptr(imp))
    return reg, imp


SCHEDULE_KEEP = 0
SCHEDULE_KNOBS = dict(reg_min=0.125, reg_max=32.0, reg_up=4.0, reg_down=REG_DOWN)


def schedule_table():
    """best in {-1, keep, another} x r in {0, under reg_min / reg_down, between, reg_max, NaN, -1}: (reg_used [18], best [18], the next reg written
    out by hand [18], improved [18])"""
    nan = np.nan
    r = [0.0, 0.25, 2.0, 32.0, nan, -1.0]
    up = [0.125, 1.0, 8.0, 32.0, 0.125, 0.125]                # raise(r); NaN and -1 count as 0
    down = [0.0, 0.0, 0.5, 8.0, 0.0, 0.0]                     # r / 4, and 0 where that is under 0.125
    reg_used = np.array(r*3, np.float32)
    best = np.repeat(np.array([-1, SCHEDULE_KEEP, 3], np.int32), len(r))
    return reg_used, best, np.array(up + up + down, np.float32), np.repeat(np.array([0, 0, 1], np.uint8), len(r))


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------------------------
deviation = S.deviation
FP64_BOUND, TWIN_FACTOR, KERNEL_FACTOR = S.FP64_BOUND, S.TWIN_FACTOR, S.KERNEL_FACTOR
# The retry case's passes that go through are family S problems under reg in {0, 2}: the fp32 twin stays inside lqr_support's record for family S
# (tests/test_lqr_reg_cpu.py prints its deviations as [lqr-reg-tol] lines), so that record is the one used, under the same factors.
RECORD = "S"


def within(dev, factor):
    S.within(dev, RECORD, factor)
