"""The forward-dynamics query (include/so100_query.h: so100_query_forward) without a GPU: the ABI surface, and the host twin of
csrc/so100_forward.hpp -- the templates the kernel instantiates -- against the fp64 oracle's so100o_forward on every state of the recipe.
Cases, references, checks and bounds: tests/forward_support.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import forward_support as S
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "so100_query.h")
FAMILIES = [r[0] for r in S.RECIPE]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------
C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "int32_t": C.c_int32, "uint32_t": C.c_uint32}


def test_struct_matches_the_header_field_for_field():
    from so100_mujoco_rl_amd import lib
    body = re.search(r"typedef struct \{([^}]*)\} so100_forward_io;", header_text()).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, name = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", decl).groups()
            fields.append((name, C_TYPES[re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()]))
    assert fields == list(lib.ForwardIO._fields_)
    assert lib.QUERY_IO["so100_query_forward"] is lib.ForwardIO and "so100_query_forward" in lib.QUERY_EXPORTS
    assert re.search(r"int so100_query_forward\(so100_sim\* sim, const so100_forward_io\* io, int32_t M, void\* hip_stream\);", header_text())


def test_defaults_match_the_header():
    from so100_mujoco_rl_amd import lib
    macro = lambda name: int(re.search(r"#define %s\s+(\d+)" % name, header_text()).group(1))
    assert (macro("SO100_FWD_SOLVER_ITERS"), macro("SO100_FWD_CONTACT_ITERS")) == (lib.FWD_SOLVER_ITERS, lib.FWD_CONTACT_ITERS) == (64, 64)
    assert macro("SO100_FWD_MAXCON") == lib.FWD_MAXCON == S.MAXCON == 20


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    assert L.so100_query_forward(None, C.byref(lib.ForwardIO()), 1, None) == -1
    assert L.so100_last_error() == b"so100_query_forward: null argument"


# ---- the recipe -------------------------------------------------------------------------------------------------------------------------------------
def test_recipe_is_what_the_bounds_were_measured_on():
    """a guard on the RECIPE, not on the feature (it asks the oracle and tests/scenes.py alone and would pass without so100_forward.hpp): the
    state counts, contact kinds, knife-edge share and the oracle's own consistency that FP32_MEASURED and DESIGN.md section 12.3 were recorded on"""
    fams = S.families()
    assert [len(f) for f in fams] == [288, 192, 192, 48, 48]
    in_contact = [sum(r["ncon"] > 0 for r in f.refs) for f in fams]
    print(f"[forward-tol] recipe: states {[len(f) for f in fams]}, in contact {in_contact}, knife edges {[int(f.knife.sum()) for f in fams]}, "
          f"largest normal force {max(r['force'][:, 0].max() for f in fams for r in f.refs if r['ncon']):.1f} N, "
          f"oracle |J' f - qfrc_constraint| {max(r['jtf_gap'] for f in fams for r in f.refs):.1e}")
    assert in_contact == [288, 86, 192, 46, 48]
    assert sum(int(f.knife.sum()) for f in fams) <= 0.02*sum(len(f) for f in fams)
    assert max(r["jtf_gap"] for f in fams for r in f.refs) <= 1e-12
    kinds = [sorted({int(k) for r in f.refs for k in r["kind"]}) for f in fams]
    assert kinds == [[0, 1], [2], [0, 1, 2], [4], [0, 3]], kinds
    assert max(r["ncon"] for f in fams for r in f.refs) <= S.MAXCON and all(r["dropped"] == 0 for f in fams for r in f.refs)


@pytest.fixture(scope="module")
def twins():
    return {(f.name, dt): S.twin(f.qpos, f.qvel, f.ctrl, f.flags, dt) for f in S.families() for dt in (np.float64, np.float32)}


@pytest.mark.parametrize("name", FAMILIES)
def test_fp64_twin_against_the_oracle(twins, name):
    fam, got = S.family(name), twins[name, np.float64]
    worst = S.measure(got, fam)
    worst["qacc"], angular = S.qacc_errors(got, fam)           # (rows 0..8; the cube's angular rows have a bound of their own: forward_support)
    for k in S.QUANTITIES:
        print(f"[forward-tol] fp64 twin {name} {k}: {worst[k]:.3e}")
    print(f"[forward-tol] fp64 twin {name} qacc rows 9..11 (rad/s^2): {angular:.3e}")
    assert max(worst.values()) <= S.FP64_BOUND, worst
    assert angular <= S.FP64_BOUND_CUBE_ANGULAR
    for i in range(len(fam)):
        if not fam.knife[i]:
            S.check_physical(got, i, S.FP64_BOUND, np.float64)


@pytest.mark.parametrize("name", FAMILIES)
def test_fp32_twin_against_the_oracle(twins, name):
    fam, got = S.family(name), twins[name, np.float32]
    worst = S.measure(got, fam)
    for k in S.QUANTITIES:
        print(f"[forward-tol] fp32 twin {name} {k}: {worst[k]:.3e} (recorded {S.FP32_MEASURED[name][k]:.1e}, kernel bound {S.FP32_BOUNDS[name][k]:.2e})")
    free, pad = S.hqacc_errors(got, fam)
    print(f"[forward-tol] fp32 twin {name} h qacc: {free:.3e} without arm contact (bound {S.HQACC_FREE:g}), {pad:.3e} with (bound {S.HQACC_PAD:g}); "
          f"worst residual {got['residual'].max():.3e}")
    for k in S.QUANTITIES:
        assert worst[k] <= S.TWIN_FACTOR*S.FP32_MEASURED[name][k], (k, worst[k])      # the recorded figures still hold; 3 x them is the KERNEL's bound
    assert free < S.HQACC_FREE and pad < S.HQACC_PAD            # the cold start costs the solve nothing the warm-started substep had
    for i in range(len(fam)):
        if not fam.knife[i]:
            S.check_physical(got, i, S.FP32_BOUNDS[name]["con_force"], np.float32)


def test_twin_at_the_shipped_iteration_counts_meets_the_same_contact_answer(twins):
    """solver_iters only sets the block PGS of contact-free arms; the contact Newton converges well inside 20 iterations on these states"""
    fam = S.family("floor_cube")
    got = S.twin(fam.qpos, fam.qvel, fam.ctrl, fam.flags, np.float32, *scenes.SHIPPED)
    assert (got["ncon"] == twins["floor_cube", np.float32]["ncon"]).all()
    assert np.abs(got["qacc"] - twins["floor_cube", np.float32]["qacc"]).max() == 0


def test_cube_pinned():
    fam = S.family("floor")
    flags = (fam.flags & ~scenes.O.F_FLOOR) | scenes.O.F_CUBE_PINNED
    for dt in (np.float64, np.float32):
        got = S.twin(fam.qpos, fam.qvel, fam.ctrl, flags, dt)
        assert not got["qacc"][:, 6:].any() and not got["qfrc_constraint"][:, 6:].any()
        con = got["contacts"]
        live = con["feat"] >= 0
        assert live.any() and (con["kind"][live] == 1).all() and (live.sum(axis=1) == got["ncon"]).all()
        # the arm does not feel the cube: its rows are those of the unpinned solve, whose cube rests on the floor away from the pads
        ref = S.twin(fam.qpos, fam.qvel, fam.ctrl, fam.flags, dt)
        assert (got["qacc"][:, :6] == ref["qacc"][:, :6]).all() and (got["pad_force"] == ref["pad_force"]).all()


def test_qvel_null_is_zero_and_ctrl_null_holds_the_pose():
    fam = S.family("grasp")
    for dt in (np.float64, np.float32):
        a = S.twin(fam.qpos, None, None, fam.flags, dt)
        b = S.twin(fam.qpos, np.zeros_like(fam.qvel), fam.qpos[:, :6], fam.flags, dt)
        for k in ("qacc", "qfrc_constraint", "ncon", "pad_force", "residual"):
            assert a[k].tobytes() == b[k].tobytes(), k
        for k in a["contacts"]:
            assert a["contacts"][k].tobytes() == b["contacts"][k].tobytes(), k


def test_non_finite_input():
    fam = S.family("grasp")
    q = fam.qpos[:4].copy(); q[1, 2] = np.nan; q[2, 8] = np.inf
    v = fam.qvel[:4].copy(); v[3, 10] = np.nan
    for dt in (np.float64, np.float32):
        got = S.twin(q, v, fam.ctrl[:4], fam.flags, dt)
        assert (got["ncon"][1:] == 0).all() and np.isnan(got["qacc"][1:]).all() and (got["contacts"]["feat"][1:] == -1).all()
        assert np.isfinite(got["qacc"][0]).all()
