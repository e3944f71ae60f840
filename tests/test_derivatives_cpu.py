"""The derivatives query (include/so100_query.h: so100_query_derivatives) without a GPU: the ABI surface, and the host twin of
csrc/so100_derivative.hpp -- the templates the kernel instantiates -- against the fp64 oracle's centred secant at the same eps.  Cases,
references and bounds: tests/derivatives_support.py; the same checks on the kernel: tests/test_gpu_derivatives.py.

A  the smooth families (the arm under F_CUBE_PINNED, without and with friction loss and limits; a tumbling cube in the air under F_NOPADS and
   under F_REFERENCE: one family per form of the kernel) against the oracle, fp64 and fp32, both modes,
B  structure, bit for bit on the fp32 twin in live contact: every entry that is one rounded add and one rounded subtraction equals the
   difference of two T = 1 trajectories on starts perturbed in numpy,
F  the surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import derivatives_support as S
import scenes
import trajectory_support as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "so100_query.h")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- F: the surface ---------------------------------------------------------------------------------------------------------------------------------
C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
FIELDS = ["qpos_dev", "qvel_dev", "ctrl_dev", "mode", "nsub", "flags", "solver_iters", "contact_iters", "eps", "A_dev", "B_dev", "qpos_next_dev",
          "qvel_next_dev", "bad_dev"]


def test_struct_matches_the_header_field_for_field():
    from so100_mujoco_rl_amd import lib
    body = re.search(r"typedef struct \{([^}]*)\} so100_derivatives_io;", header_text()).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, name = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", decl).groups()
            fields.append((name, C_TYPES[re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()]))
    assert fields == list(lib.DerivativesIO._fields_) and [f[0] for f in fields] == FIELDS
    assert lib.QUERY_IO["so100_query_derivatives"] is lib.DerivativesIO and "so100_query_derivatives" in lib.QUERY_EXPORTS
    assert re.search(r"int so100_query_derivatives\(so100_sim\* sim, const so100_derivatives_io\* io, int32_t M, void\* hip_stream\);", header_text())
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_macros_match_the_header():
    from so100_mujoco_rl_amd import lib
    macro = lambda name: re.search(r"#define %s\s+([0-9.e-]+)f?\b" % name, header_text()).group(1)
    assert (int(macro("SO100_DERIV_NX")), int(macro("SO100_DERIV_NU"))) == (lib.DERIV_NX, lib.DERIV_NU) == (S.NX, S.NU) == (24, 6)
    eps = float(macro("SO100_DERIV_EPS"))
    assert eps == lib.DERIV_EPS == S.EPS and np.log2(eps) == round(np.log2(eps))       # a power of two: 1 / (2 eps) is exact


def test_the_header_says_what_the_result_is():
    text = " ".join(open(HEADER).read().split())
    for phrase in ("CENTRED SECANT", "mjd_transitionFD", "depends on eps", "differ by up to 0.17 on entries of size 8", "Forward (one-sided) differences are not offered"):
        assert phrase in text, phrase


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    assert L.so100_query_derivatives(None, C.byref(lib.DerivativesIO()), 1, None) == -1
    assert L.so100_last_error() == b"so100_query_derivatives: null argument"


# ---- A: the smooth families against the oracle's secant ---------------------------------------------------------------------------------------------
def rows_deviation(got, ref, rows):
    d = np.abs(np.concatenate([got["A"], got["B"]], axis=2) - np.concatenate([ref["A"], ref["B"]], axis=2))[:, rows]
    half = len(rows)//2
    return float(d[:, :half].max()), float(d[:, half:].max())


@pytest.mark.parametrize("mode", ["actions", "targets"])
@pytest.mark.parametrize("name", sorted(S.FAMILY_FLAGS))
def test_fp64_twin_smooth(name, mode):
    c = S.family(name, mode); ref = S.smooth_reference(name, mode)
    got = S.twin(c["ctrl"], c["qpos"], c["qvel"], mode, S.NSUB, c["flags"], np.float64, *S.ITERS)
    assert not got["bad"].any()
    arm = rows_deviation(got, ref, S.ARM_ROWS); cube = rows_deviation(got, ref, S.CUBE_ROWS)
    b = S.fp64_bounds(S.EPS)
    print(f"[deriv-tol] fp64 twin {name} {mode}: arm rows q {arm[0]:.3e} v {arm[1]:.3e} (bounds {b['arm'][0]:.1e} / {b['arm'][1]:.1e}), "
          f"cube rows q {cube[0]:.3e} v {cube[1]:.3e} (bounds {b['cube'][0]:.1e} / {b['cube'][1]:.1e})")
    assert arm[0] <= b["arm"][0] and arm[1] <= b["arm"][1]
    assert cube[0] <= b["cube"][0] and cube[1] <= b["cube"][1]
    assert np.abs(got["qpos_next"] - ref["qpos_next"]).max() <= TS.FP64_CUBE[0] and np.abs(got["qvel_next"] - ref["qvel_next"]).max() <= TS.FP64_CUBE[1]
    if name in S.PINNED:
        S.cube_block_is_the_identity(got, {"q": b["cube"][0], "v": b["cube"][1]})


@pytest.mark.parametrize("name", sorted(S.FAMILY_FLAGS))
def test_fp32_twin_smooth(name):
    worst = {"q": 0.0, "v": 0.0, "qpos": 0.0, "qvel": 0.0}
    for mode in ("actions", "targets"):
        c = S.family(name, mode); ref = S.smooth_reference(name, mode)
        got = S.twin(c["ctrl"], c["qpos"], c["qvel"], mode, S.NSUB, c["flags"], np.float32, *S.ITERS)
        assert not got["bad"].any()
        dev = S.deviation(got, ref)
        print(f"[deriv-tol] fp32 twin {name} {mode} eps 2^{int(np.log2(S.EPS))}: q rows {dev['q']:.3e} v rows {dev['v']:.3e}, next qpos {dev['qpos']:.3e} qvel {dev['qvel']:.3e} (recorded {S.FP32_MEASURED[name]}); "
              f"largest |entry| q rows {np.abs(ref['A'][:, :12]).max():.2f} v rows {max(np.abs(ref['A'][:, 12:]).max(), np.abs(ref['B'][:, 12:]).max()):.2f}")
        worst = {k: max(worst[k], dev[k]) for k in worst}
        if name in S.PINNED:
            S.cube_block_is_the_identity(got, {k: S.TWIN_FACTOR*S.FP32_MEASURED[name][k] for k in worst})
    for k in worst:
        assert worst[k] <= S.TWIN_FACTOR*S.FP32_MEASURED[name][k], (k, worst[k])


def test_cube_at_rest_record():
    """a record, not a gate: the cube at rest on the floor (its contact rows are live: the step is only piecewise smooth), against the oracle at
    the same eps.  Friction loss and limits on the arm family were such a record too, until the twin confirmed them on all 30 columns: they are
    the gated family "rows" now."""
    c = S.family("arm", "targets")
    n = 8
    qpos = c["qpos"][:n].copy(); qpos[:, 6:9] = [0.2, -0.2, 0.0099]; qpos[:, 9:13] = [1, 0, 0, 0]
    qvel = c["qvel"][:n].copy(); qvel[:, 6:] = 0
    ref = S.oracle_secant(qpos, qvel, c["ctrl"][:n], "targets", S.NSUB, scenes.NOPADS, S.EPS)
    got = S.twin(c["ctrl"][:n], qpos, qvel, "targets", S.NSUB, scenes.NOPADS, np.float32, *S.ITERS)
    q, v = rows_deviation(got, ref, S.CUBE_ROWS)
    print(f"[deriv-tol] fp32 twin F_NOPADS, the cube at rest on the floor, cube rows (record): q rows {q:.3e} v rows {v:.3e}")
    assert not got["bad"].any()


# ---- B: structure, bit for bit on the fp32 twin, contacts live ---------------------------------------------------------------------------------------
def twin_step(mode, nsub, flags):
    def step(q, v, u):
        g = TS.twin(u[None], q, v, mode, nsub, flags)
        assert (g["bad_step"] == -1).all()
        return g["qpos_final"], g["qvel_final"]
    return step


@pytest.mark.parametrize("nsub", [1, 4, 16])
@pytest.mark.parametrize("mode", ["actions", "targets"])
@pytest.mark.parametrize("name", ["floor", "grasp"])
def test_plain_entries_are_differences_of_two_trajectories(name, mode, nsub):
    """pins the lane map, the column order, the control columns and the actions-mode coupling without a tolerance"""
    q, v, a, flags = S.contact_inputs(name)
    u = a if mode == "actions" else (q[:, :6] + (a*scenes.JS).astype(np.float32)).astype(np.float32)
    got = S.twin(u, q, v, mode, nsub, flags, eps=S.STRUCT_EPS)
    assert not got["bad"].any()
    want = S.expected_plain(twin_step(mode, nsub, flags), q, v, u, S.STRUCT_EPS)
    assert bits(S.plain_block(got)) == bits(want)
    assert np.abs(want).max() > 0.5                           # (the block is not trivially zero)
    nominal = TS.twin(u[None], q, v, mode, nsub, flags)
    assert nominal["ncon"].any()                              # contacts are live
    assert bits(got["qpos_next"]) == bits(nominal["qpos_final"]) and bits(got["qvel_next"]) == bits(nominal["qvel_final"])


def test_repeat_batch_and_place_independence():
    q, v, a, flags = S.contact_inputs("floor")
    full = S.twin(a, q, v, "actions", 4, flags, eps=S.STRUCT_EPS)
    again = S.twin(a, q, v, "actions", 4, flags, eps=S.STRUCT_EPS)
    for k in full:
        assert bits(full[k]) == bits(again[k]), k
    for m in (0, 2, 4):                                       # M = 1 against inside 5; a prefix of 3
        one = S.twin(a[m:m + 1], q[m:m + 1], v[m:m + 1], "actions", 4, flags, eps=S.STRUCT_EPS)
        for k in full:
            assert bits(full[k][m:m + 1]) == bits(one[k]), (k, m)
    part = S.twin(a[:3], q[:3], v[:3], "actions", 4, flags, eps=S.STRUCT_EPS)
    for k in full:
        assert bits(full[k][:3]) == bits(part[k]), k


def test_qvel_null_is_zero():
    q, v, a, flags = S.contact_inputs("grasp")
    for dt in (np.float32, np.float64):
        x = S.twin(a, q, None, "actions", 4, flags, dt, eps=S.STRUCT_EPS)
        y = S.twin(a, q, np.zeros_like(v), "actions", 4, flags, dt, eps=S.STRUCT_EPS)
        for k in x:
            assert bits(x[k]) == bits(y[k]), k


def test_non_finite_start_or_control():
    q, v, a, flags = S.contact_inputs("floor")
    q, v, a = q.copy(), v.copy(), a.copy()
    clean = S.twin(a, q, v, "actions", 4, flags, eps=S.STRUCT_EPS)
    a[1, 3] = np.nan; q[2, 8] = np.inf; v[3, 2] = np.nan; a[4, 0] = np.inf
    got = S.twin(a, q, v, "actions", 4, flags, eps=S.STRUCT_EPS)
    assert got["bad"].tolist() == [0, 1, 1, 1, 1]
    for k in ("A", "B", "qpos_next", "qvel_next"):
        assert np.isnan(got[k][1:]).all(), k
        assert bits(got[k][0]) == bits(clean[k][0]), k        # the other problem never sees it
