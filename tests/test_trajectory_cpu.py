"""The trajectory query (include/so100_query.h: so100_query_trajectory) without a GPU: the ABI surface, and the host twin of
csrc/so100_trajectory.hpp -- the templates the kernel instantiates -- against the fp64 oracle.  Cases, references and bounds:
tests/trajectory_support.py; the same checks on the kernel: tests/test_gpu_trajectory.py.

A  per-substep parity with the oracle on every contact kind (the query with T = 1, nsub = 1 is a device_substep of substep_harness),
B  contact-free trajectories of 3 x 16 substeps against the oracle, both modes,
C  the warm starts carried through 2 x 4 substeps in pad contact, against the oracle's free-running substeps,
E  exact properties, bit for bit on the fp32 twin,
F  the surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scenes
import substep_harness as SH
import trajectory_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "so100_query.h")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- F: the surface ---------------------------------------------------------------------------------------------------------------------------------
C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "int32_t": C.c_int32, "uint32_t": C.c_uint32}


def test_struct_matches_the_header_field_for_field():
    from so100_mujoco_rl_amd import lib
    body = re.search(r"typedef struct \{([^}]*)\} so100_trajectory_io;", header_text()).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, name = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", decl).groups()
            fields.append((name, C_TYPES[re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()]))
    assert fields == list(lib.TrajectoryIO._fields_) and len(fields) == 19
    assert lib.QUERY_IO["so100_query_trajectory"] is lib.TrajectoryIO and "so100_query_trajectory" in lib.QUERY_EXPORTS
    assert re.search(r"int so100_query_trajectory\(so100_sim\* sim, const so100_trajectory_io\* io, int32_t M, void\* hip_stream\);", header_text())
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_macros_match_the_header():
    from so100_mujoco_rl_amd import lib
    macro = lambda name: int(re.search(r"#define %s\s+(\d+)" % name, header_text()).group(1))
    assert (macro("SO100_TRAJ_TARGETS"), macro("SO100_TRAJ_ACTIONS")) == (lib.TRAJ_MODES["targets"], lib.TRAJ_MODES["actions"]) == (S.TARGETS, S.ACTIONS) == (0, 1)
    assert (macro("SO100_TRAJ_MAX_T"), macro("SO100_TRAJ_MAX_NSUB"), macro("SO100_TRAJ_MAX_SUBSTEPS")) == \
        (lib.TRAJ_MAX_T, lib.TRAJ_MAX_NSUB, lib.TRAJ_MAX_SUBSTEPS) == (4096, 1024, 65536)


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    assert L.so100_query_trajectory(None, C.byref(lib.TrajectoryIO()), 1, None) == -1
    assert L.so100_last_error() == b"so100_query_trajectory: null argument"


# ---- A: per-substep parity with the oracle, every contact kind ------------------------------------------------------------------------------------------
def test_pad_floor_per_substep():
    n, nsub = 64, 32
    qpos, qvel, act = scenes.floor_batch(n, 0)
    T = SH.run_substep_parity(S.TwinSubstep(scenes.REFP), qpos, qvel, act, scenes.REFP, nsub, f"trajectory twin fp32 {S.PARITY_ITERS}, pad/floor")
    SH.check_tally(T, min_contact=n*nsub//3, iters=S.PARITY_ITERS)


def test_pad_cube_grasp_per_substep():
    n, nsub = 32, 48
    qpos, qvel, act = scenes.grasp_batch(n, 1)
    T = SH.run_substep_parity(S.TwinSubstep(scenes.C5), qpos, qvel, act, scenes.C5, nsub, f"trajectory twin fp32 {S.PARITY_ITERS}, grasp")
    SH.check_tally(T, min_contact=n*nsub//3, min_coupled=n*nsub//4, iters=S.PARITY_ITERS)


def test_floor_cube_per_substep():
    n, nsub = 64, 24
    qpos, qvel, act = scenes.floor_cube_batch(n, 0)
    T = SH.run_substep_parity(S.TwinSubstep(scenes.C5), qpos, qvel, act, scenes.C5, nsub, f"trajectory twin fp32 {S.PARITY_ITERS}, cube on the floor")
    SH.check_tally(T, min_contact=n*nsub//3, min_coupled=n*nsub//4, iters=S.PARITY_ITERS)
    SH.check_moving_cube(T)


def test_link_proxies_per_substep():
    n, nsub = 48, 32
    qpos, qvel, act = scenes.wrist_first_batch(n, 0)
    T = SH.run_substep_parity(S.TwinSubstep(scenes.LINKS), qpos, qvel, act, scenes.LINKS, nsub, f"trajectory twin fp32 {S.PARITY_ITERS}, link proxies, wrist first")
    SH.check_tally(T, min_contact=n*nsub//3, iters=S.PARITY_ITERS)


def test_link_cube_per_substep():
    n, nsub = 32, 12
    qpos, qvel, act = scenes.link_cube_batch(n, 0)
    T = SH.run_substep_parity(S.TwinSubstep(scenes.LCUBE), qpos, qvel, act, scenes.LCUBE, nsub, f"trajectory twin fp32 {S.PARITY_ITERS}, link proxies vs cube")
    SH.check_tally(T, min_contact=n*nsub//3, min_coupled=n*nsub//3, iters=S.PARITY_ITERS)


def test_pad_floor_per_substep_at_shipped_settings_record():
    """a record, not a gate: the cold-started query at the shipped (2, 20)"""
    n, nsub = 64, 8
    qpos, qvel, act = scenes.floor_batch(n, 0)
    T = SH.run_substep_parity(S.TwinSubstep(scenes.REFP, scenes.SHIPPED), qpos, qvel, act, scenes.REFP, nsub, f"trajectory twin fp32 {scenes.SHIPPED} cold (record), pad/floor")
    assert T.pairs == n*nsub


# ---- B: contact-free trajectories against the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["actions", "targets"])
@pytest.mark.parametrize("name", sorted(S.FREE_FLAGS))
def test_fp64_twin_contact_free(name, mode):
    c = S.free_case(name, mode)
    got = S.twin(c["ctrl"], c["qpos"], c["qvel"], mode, S.FREE_NSUB, c["flags"], np.float64, *S.FP64_ITERS)
    assert (got["bad_step"] == -1).all() and not got["ncon"].any()
    arm_q = np.abs(got["qpos"][..., :6] - c["ref"]["qpos"][..., :6]).max(); arm_v = np.abs(got["qvel"][..., :6] - c["ref"]["qvel"][..., :6]).max()
    cube_q = np.abs(got["qpos"][..., 6:] - c["ref"]["qpos"][..., 6:]).max(); cube_v = np.abs(got["qvel"][..., 6:] - c["ref"]["qvel"][..., 6:]).max()
    ee = np.abs(got["ee"] - c["ref"]["ee"]).max()
    print(f"[traj-tol] fp64 twin {name} {mode}: arm qpos {arm_q:.3e} qvel {arm_v:.3e}, cube qpos {cube_q:.3e} qvel {cube_v:.3e}, ee {ee:.3e}")
    assert arm_q <= S.FP64_ARM[0] and arm_v <= S.FP64_ARM[1]
    assert cube_q <= S.FP64_CUBE[0] and cube_v <= S.FP64_CUBE[1]
    assert ee <= S.QS.FP64_BOUND + 6*S.REACH*S.FP64_ARM[0]


@pytest.mark.parametrize("name", sorted(S.FREE_FLAGS))
def test_fp32_twin_contact_free(name):
    worst = {"qpos": 0.0, "qvel": 0.0}
    for mode in ("actions", "targets"):
        c = S.free_case(name, mode)
        got = S.twin(c["ctrl"], c["qpos"], c["qvel"], mode, S.FREE_NSUB, c["flags"], np.float32, *scenes.SHIPPED)
        assert (got["bad_step"] == -1).all() and not got["ncon"].any()
        dev = S.deviation(got, c["ref"])
        ee = np.abs(got["ee"].astype(np.float64) - c["ref"]["ee"]).max()
        print(f"[traj-tol] fp32 twin {name} {mode}: qpos {dev['qpos']:.3e} qvel {dev['qvel']:.3e} ee {ee:.3e} "
              f"(recorded {S.FP32_MEASURED[name]}, ee bound {S.ee_bound(S.TWIN_FACTOR*S.FP32_MEASURED[name]['qpos']):.2e})")
        assert ee <= S.ee_bound(S.TWIN_FACTOR*S.FP32_MEASURED[name]["qpos"])
        worst = {k: max(worst[k], dev[k]) for k in worst}
    for k in worst:
        assert worst[k] <= S.TWIN_FACTOR*S.FP32_MEASURED[name][k], (k, worst[k])


# ---- C: warm carry in contact against the oracle ------------------------------------------------------------------------------------------------------
def test_warm_carry_in_contact():
    """the oracle's set is constant over the 8 substeps and free of knife edges in the kept cases: there ncon and sig are the oracle's at both
    steps, exactly, and the state is held to the recorded deviation"""
    c = S.warm_case()
    print(f"[traj-tol] warm carry: {int(c['keep'].sum())} of {len(c['keep'])} cases kept, {int(c['in_contact'].sum())} of them in pad contact, "
          f"{int(c['knife'].sum())} lost to a knife edge")
    assert c["in_contact"].sum() >= 20                        # a condition on the cases, not a tolerance
    got = S.twin(c["ctrl"], c["qpos"], c["qvel"], "actions", S.WARM_NSUB, c["flags"], np.float32, *S.WARM_ITERS)
    keep = c["keep"]
    for t in range(S.WARM_T):
        assert (got["ncon"][t][keep] == c["count"][keep]).all() and (got["sig"][t][keep] == c["sig"][keep]).all(), t
    assert not got["dropped"][:, keep].any() and (got["bad_step"] == -1).all()
    dev = S.deviation(got, c["ref"], keep)
    print(f"[traj-tol] fp32 twin warm carry {S.WARM_ITERS}: qpos {dev['qpos']:.3e} qvel {dev['qvel']:.3e} (recorded {S.FP32_MEASURED['warm']})")
    for k in dev:
        assert dev[k] <= S.TWIN_FACTOR*S.FP32_MEASURED["warm"][k], (k, dev[k])
    # the fp64 twin meets the same sets
    g64 = S.twin(c["ctrl"], c["qpos"], c["qvel"], "actions", S.WARM_NSUB, c["flags"], np.float64, *S.FP64_ITERS)
    for t in range(S.WARM_T):
        assert (g64["ncon"][t][keep] == c["count"][keep]).all() and (g64["sig"][t][keep] == c["sig"][keep]).all(), t
    d64 = S.deviation(g64, c["ref"], keep)
    print(f"[traj-tol] fp64 twin warm carry {S.FP64_ITERS}: qpos {d64['qpos']:.3e} qvel {d64['qvel']:.3e}")


# ---- E: exact properties, on the fp32 twin ----------------------------------------------------------------------------------------------------------------
FIELDS = ("qpos", "qvel", "ee", "ncon", "dropped", "sig", "residual")


def contact_inputs():
    q, v, a = S.contact_inputs()
    return q.copy(), v.copy(), a.copy()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_prefix_batch_and_repeat_independence():
    q, v, a = contact_inputs()
    full = S.twin(a, q, v, "actions", 4, scenes.REFP)
    assert full["ncon"].any()
    again = S.twin(a, q, v, "actions", 4, scenes.REFP)
    for k in FIELDS + ("qpos_final", "qvel_final", "bad_step"):
        assert bits(full[k]) == bits(again[k]), k
    for Tp in (1, 2):                                         # row t < T' of a T-step call = row t of the T'-step call
        part = S.twin(a[:Tp], q, v, "actions", 4, scenes.REFP)
        for k in FIELDS:
            assert bits(full[k][:Tp]) == bits(part[k]), (k, Tp)
    for m in (0, 64, 129):                                    # a problem's rows depend neither on M nor on its position
        one = S.twin(a[:, m:m + 1], q[m:m + 1], v[m:m + 1], "actions", 4, scenes.REFP)
        for k in FIELDS:
            assert bits(full[k][:, m:m + 1]) == bits(one[k]), (k, m)
    assert bits(full["qpos_final"]) == bits(full["qpos"][-1]) and bits(full["qvel_final"]) == bits(full["qvel"][-1])


@pytest.mark.parametrize("nsub", [1, 4, 16])
def test_targets_mode_reproduces_an_actions_run(nsub):
    """targets = q_t + 0.075 a_t in float32 (a product rounded, a sum rounded) from the actions run's own rows"""
    q, v, a = contact_inputs()
    run = S.twin(a, q, v, "actions", nsub, scenes.REFP)
    starts = np.concatenate([q[None, :, :6], run["qpos"][:-1, :, :6]])
    targets = (starts + (a*scenes.JS).astype(np.float32)).astype(np.float32)
    rerun = S.twin(targets, q, v, "targets", nsub, scenes.REFP)
    for k in FIELDS:
        assert bits(run[k]) == bits(rerun[k]), k


def test_qvel_null_is_zero():
    q, v, a = contact_inputs()
    for dt in (np.float32, np.float64):
        x = S.twin(a, q, None, "actions", 4, scenes.C5, dt)
        y = S.twin(a, q, np.zeros_like(v), "actions", 4, scenes.C5, dt)
        for k in FIELDS:
            assert bits(x[k]) == bits(y[k]), k


def test_non_finite_control_or_state():
    q, v, a = contact_inputs()
    q, v, a = q[:6].copy(), v[:6].copy(), a[:, :6].copy()
    clean = S.twin(a, q, v, "actions", 4, scenes.REFP)
    a[1, 1, 3] = np.nan; a[2, 2, 0] = np.inf; a[0, 3, 5] = np.nan
    q[4, 8] = np.nan; v[5, 2] = np.inf
    got = S.twin(a, q, v, "actions", 4, scenes.REFP)
    assert got["bad_step"].tolist() == [-1, 1, 2, 0, 0, 0]
    for m, t0 in ((1, 1), (2, 2), (3, 0), (4, 0), (5, 0)):
        for k in FIELDS:
            assert bits(got[k][:t0, m]) == bits(clean[k][:t0, m]), (k, m)       # the rows before it
        for k in ("qpos", "qvel", "ee", "residual"):
            assert np.isnan(got[k][t0:, m]).all(), (k, m)
        for k in ("ncon", "dropped", "sig"):
            assert not got[k][t0:, m].any(), (k, m)
        assert np.isnan(got["qpos_final"][m]).all() and np.isnan(got["qvel_final"][m]).all()
    for k in FIELDS:
        assert bits(got[k][:, 0]) == bits(clean[k][:, 0]), k                   # the other problems never see it
