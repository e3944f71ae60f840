"""The closed-loop trajectory query on the CPU: the host twin of so100_closed_loop.hpp (tests/_closedcheck) against the fp64 oracle under the
feedback law in numpy (tests/closed_loop_support.py), the exact properties of the law and the rollout, and the failure cases.  The twin's table and its
stand-alone program are held in tests/test_hostlibs.py.  The same cases run on the kernel in tests/test_gpu_closed_loop.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import closed_loop_support as S
import scenes
import trajectory_support as TS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "so100_query.h")
C_TYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
IO_FIELDS = ["qpos_dev", "qvel_dev", "u_dev", "mode", "T", "nsub", "flags", "solver_iters", "contact_iters", "qpos_ref_dev", "qvel_ref_dev", "qpos_ref0_dev", "qvel_ref0_dev",
             "nx", "k_dev", "K_dev", "L", "alpha", "clamp", "u_lo", "u_hi", "u_traj_dev", "qpos_traj_dev", "qvel_traj_dev", "ee_traj_dev", "qpos_final_dev", "qvel_final_dev",
             "ncon_dev", "dropped_dev", "sig_dev", "residual_dev", "bad_step_dev"]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def show(tag, dev, bound=None):
    print(f"[cl-tol] {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in dev.items()) + ("" if bound is None else f" (bound {bound})"))


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------------------
def test_struct_matches_the_header_field_for_field():
    from so100_mujoco_rl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} so100_closed_loop_io;", text).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, name = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", decl).groups()
            fields.append((name, C_TYPES[re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()]))
    assert fields == list(lib.ClosedLoopIO._fields_) and [f[0] for f in fields] == IO_FIELDS
    assert lib.QUERY_IO["so100_query_closed_loop"] is lib.ClosedLoopIO and "so100_query_closed_loop" in lib.QUERY_EXPORTS
    assert re.search(r"int so100_query_closed_loop\(so100_sim\* sim, const so100_closed_loop_io\* io, int32_t M, void\* hip_stream\);", text)
    assert int(re.search(r"#define SO100_CL_MAX_L\s+(\d+)\b", text).group(1)) == lib.CL_MAX_L == S.MAX_L
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive


def test_null_arguments_are_refused_without_a_device():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    L = lib.load()
    assert L.so100_query_closed_loop(None, C.byref(lib.ClosedLoopIO()), 1, None) == -1
    assert L.so100_last_error() == b"so100_query_closed_loop: null argument"


# ---- deviation bounds ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ref0", [False, True])
@pytest.mark.parametrize("n", [12, 24])
def test_family_p_against_the_oracle(n, with_ref0):
    c, ref = S.family_p_cpu(n), S.reference_p(n, with_ref0)
    d64 = S.deviation(S.run_p(S.twin, c, with_ref0, dtype=np.float64, solver_iters=S.FP64_ITERS[0], contact_iters=S.FP64_ITERS[1]), ref)
    got = S.run_p(S.twin, c, with_ref0)
    assert (got["bad_step"] == -1).all()
    d32 = S.deviation(got, ref)
    show(f"P nx {n} ref0 {with_ref0} fp64", d64, S.FP64_BOUND); show(f"P nx {n} ref0 {with_ref0} fp32", d32)
    # the candidates do differ: the alpha = 1 and alpha = 0 controls by more than 0.1 somewhere
    assert np.abs(ref["u"][:, :, 2] - ref["u"][:, :, 0]).max() > 0.1
    assert max(d64.values()) <= S.FP64_BOUND
    S.within(d32, "P", S.TWIN_FACTOR)


@pytest.mark.parametrize("mode", ["actions", "targets"])
@pytest.mark.parametrize("name", sorted(TS.FREE_FLAGS))
def test_family_g_against_the_oracle(name, mode):
    g = S.family_g(name, mode)
    d64 = S.deviation(S.run_g(S.twin, g, dtype=np.float64, solver_iters=S.FP64_ITERS[0], contact_iters=S.FP64_ITERS[1]), g["ref"])
    got = S.run_g(S.twin, g)
    assert (got["bad_step"] == -1).all() and not got["ncon"].any()
    d32 = S.deviation(got, g["ref"])
    show(f"G {name} {mode} fp64", d64, S.FP64_BOUND); show(f"G {name} {mode} fp32", d32)
    assert max(d64.values()) <= S.FP64_BOUND
    S.within(d32, "G", S.TWIN_FACTOR)


def test_warm_contact_record():
    w = S.warm_family()
    assert w["in_contact"].sum() >= 20
    got = S.run_warm(S.twin, w)
    keep = w["keep"]
    for t in range(TS.WARM_T):
        assert (got["ncon"][t][keep] == w["count"][keep, None]).all() and (got["sig"][t][keep] == w["sig"][keep, None]).all(), t
    d = S.warm_deviation(got, w)
    d64 = S.warm_deviation(S.run_warm(S.twin, w, dtype=np.float64), w)
    show("warm fp64", d64, S.FP64_BOUND); show("warm fp32", d)
    # the law bites: the candidates' controls differ by more than 0.01, and alpha = 0's differ from the open-loop ones by more than 1e-3
    assert np.abs(w["ref"]["u"][:, keep, 1] - w["ref"]["u"][:, keep, 0]).max() > 0.01 and np.abs(w["ref"]["u"][:, keep, 0] - w["u"][:, keep]).max() > 1e-3
    assert max(d64.values()) <= S.FP64_BOUND
    S.within(d, "warm", S.TWIN_FACTOR)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------------------------
def inputs(nx, n=5, T=3, seed=0, mode="actions"):
    """contact_inputs' first n problems (pads on the floor, REFP) with T = 3 actions, seeded PD gains and the fp32 twin's open-loop rollout as plan"""
    q, v, a = TS.contact_inputs()
    q, v, a = q[:n].copy(), v[:n].copy(), (0.5*a[:T, :n]).copy()
    K, k = S.pd_gains(T, n, nx, seed)
    roll = TS.twin(a, q, v, mode, 4, scenes.REFP)
    return {"u": a, "qpos_ref": roll["qpos"], "qvel_ref": roll["qvel"], "K": K, "k": k, "nx": nx, "qpos": q, "qvel": v, "roll": roll}


def run(c, alphas, **kw):
    args = dict(alphas=alphas, nx=c["nx"], qpos=c["qpos"], qvel=c["qvel"], mode="actions", nsub=4, flags=scenes.REFP)
    args.update(kw)
    return S.twin(c["u"], c["qpos_ref"], c["qvel_ref"], args.pop("K", c["K"]), args.pop("k", c["k"]), **args)


@pytest.mark.parametrize("nx", [12, 24])
def test_alpha_zero_on_the_plans_own_rollout_is_the_open_loop_rollout(nx):
    c = inputs(nx)
    got = run(c, (0.0,))
    assert c["roll"]["ncon"].any()
    for name in ("qpos", "qvel", "ee", "ncon", "dropped", "sig", "residual"):
        assert bits(got[name][:, :, 0]) == bits(c["roll"][name]), name
    assert bits(got["u"][:, :, 0]) == bits(c["u"]) and bits(got["qpos_final"][:, 0]) == bits(c["roll"]["qpos_final"])


@pytest.mark.parametrize("nx", [12, 24])
def test_zero_gains_are_open_loop_for_any_alpha(nx):
    c = inputs(nx)
    moved = c["qpos_ref"] + np.float32(0.1)                     # any reference: it meets K = 0
    got = S.twin(c["u"], moved, c["qvel_ref"], np.zeros_like(c["K"]), np.zeros_like(c["k"]), alphas=(0.0, 0.7, -3.0), nx=nx, qpos=c["qpos"], qvel=c["qvel"],
                 ref0=(moved[0], c["qvel_ref"][0]), mode="actions", nsub=4, flags=scenes.REFP)
    for a in range(3):
        for name in ("qpos", "qvel", "ee", "sig", "residual"):
            assert bits(got[name][:, :, a]) == bits(c["roll"][name]), (name, a)
    none = S.twin(c["u"], moved, c["qvel_ref"], np.zeros_like(c["K"]), None, alphas=(2.0,), nx=nx, qpos=c["qpos"], qvel=c["qvel"], mode="actions", nsub=4, flags=scenes.REFP)
    assert bits(none["qpos"][:, :, 0]) == bits(c["roll"]["qpos"])                # k NULL is zero


def test_the_clamp():
    c = inputs(24)
    free = run(c, (0.0, 1.0, 4.0))
    lo, hi = -0.3, 0.25
    got = run(c, (0.0, 1.0, 4.0), clamp=(lo, hi))
    assert (got["u"] >= np.float32(lo)).all() and (got["u"] <= np.float32(hi)).all()
    # step 0 starts from the same state in both runs: the clamped entry is the unclamped one where that is interior, else the bound
    u0, f0 = got["u"][0], free["u"][0]
    interior = (f0 > lo) & (f0 < hi)
    assert interior.any() and (~interior).any()
    assert bits(u0[interior]) == bits(f0[interior])
    assert bits(u0[~interior]) == bits(np.clip(f0, np.float32(lo), np.float32(hi))[~interior])


def test_a_candidate_does_not_depend_on_L_its_index_or_M():
    c = inputs(12, n=5)
    al = (0.0, 0.3, 1.0, -0.5, 0.25, 0.125, 2.0, 0.75)
    full = run(c, al)
    assert (full["bad_step"] == -1).all()
    for a, alpha in enumerate(al):
        one = run(c, (alpha,))
        for name in S.FIELDS:
            assert bits(full[name][:, :, a]) == bits(one[name][:, :, 0]), (name, a)
    rev = run(c, al[::-1])
    for name in S.FIELDS:
        assert bits(rev[name][:, :, ::-1]) == bits(full[name]), name
    sixteen = run(c, al + al)
    for name in S.FIELDS:
        assert bits(sixteen[name][:, :, :8]) == bits(full[name]) and bits(sixteen[name][:, :, 8:]) == bits(full[name]), name
    for m in (0, 3):                                               # M = 1 against inside 5
        sub = S.twin(c["u"][:, m:m + 1], c["qpos_ref"][:, m:m + 1], c["qvel_ref"][:, m:m + 1], c["K"][:, m:m + 1], c["k"][:, m:m + 1], alphas=al, nx=12,
                     qpos=c["qpos"][m:m + 1], qvel=c["qvel"][m:m + 1], mode="actions", nsub=4, flags=scenes.REFP)
        for name in S.FIELDS:
            assert bits(sub[name]) == bits(full[name][:, m:m + 1]), (name, m)


@pytest.mark.parametrize("nx", [12, 24])
def test_one_step_reads_no_reference_row(nx):
    c = inputs(nx)
    al = (0.0, 1.0)
    full = run(c, al)
    one = S.twin(c["u"][:1], None, None, c["K"][:1], c["k"][:1], alphas=al, nx=nx, qpos=c["qpos"], qvel=c["qvel"], mode="actions", nsub=4, flags=scenes.REFP)
    for name in S.FIELDS:
        assert bits(one[name][0]) == bits(full[name][0]), name
    # and row T - 1 of a longer reference is never read
    poisoned = {**c, "qpos_ref": c["qpos_ref"].copy(), "qvel_ref": c["qvel_ref"].copy()}
    poisoned["qpos_ref"][-1] = np.nan; poisoned["qvel_ref"][-1] = np.inf
    again = run(poisoned, al)
    for name in S.FIELDS + ("bad_step",):
        assert bits(again[name]) == bits(full[name]), name
    if nx == 12:                                                   # the arm form never reads the reference's cube rows
        poisoned = {**c, "qpos_ref": c["qpos_ref"].copy(), "qvel_ref": c["qvel_ref"].copy()}
        poisoned["qpos_ref"][..., 6:] = np.nan; poisoned["qvel_ref"][..., 6:] = np.nan
        again = run(poisoned, al)
        for name in S.FIELDS + ("bad_step",):
            assert bits(again[name]) == bits(full[name]), name


def test_the_first_control_is_the_numpy_law():
    """step 0 from a moved nominal start: the control applied is the formula's, to fp32 rounding of a sum of 25 terms of size <= 2 x 0.3"""
    c = inputs(24)
    rng = np.random.default_rng(5)
    r0q = c["qpos"].copy(); r0q[:, :9] += (0.1*rng.standard_normal((len(r0q), 9))).astype(np.float32)
    r0v = c["qvel"] + (0.1*rng.standard_normal(c["qvel"].shape)).astype(np.float32)
    al = (0.0, 1.0)
    got = run(c, al, ref0=(r0q, r0v))
    want = np.array([[S.law(c["qpos"][m].astype(np.float64), c["qvel"][m].astype(np.float64), r0q[m].astype(np.float64), r0v[m].astype(np.float64),
                            c["u"][0, m].astype(np.float64), c["k"][0, m].astype(np.float64), c["K"][0, m].astype(np.float64), a, 24) for a in al] for m in range(len(r0q))])
    assert np.abs(got["u"][0] - want).max() <= 25*2.0**-23
    assert np.abs(want[:, 1] - want[:, 0]).max() > 0.1             # alpha = 1 against alpha = 0
    assert np.abs(got["qpos"][-1][:, 1] - got["qpos"][-1][:, 0]).max() > 1e-3


# ---- failure cases -----------------------------------------------------------------------------------------------------------------------------------------
def assert_failed_from(got, clean, m, t0, L):
    assert got["bad_step"][m].tolist() == [t0]*L
    for name in S.FIELDS:
        assert bits(got[name][:t0, m]) == bits(clean[name][:t0, m]), name
    for name in S.FLOAT_OUT:
        assert np.isnan(got[name][t0:, m]).all(), name
    for name in S.INT_OUT:
        assert not got[name][t0:, m].any(), name
    assert np.isnan(got["qpos_final"][m]).all() and np.isnan(got["qvel_final"][m]).all()
    others = [i for i in range(got["bad_step"].shape[0]) if i != m]
    assert (got["bad_step"][others] == -1).all()
    for name in S.FIELDS:
        assert bits(got[name][:, others]) == bits(clean[name][:, others]), name


@pytest.mark.parametrize("nx", [12, 24])
def test_non_finite_inputs_fail_their_problem_at_their_step(nx):
    c = inputs(nx, n=3)
    al = (0.0, 0.5, 1.0)
    clean = run(c, al)
    K = c["K"].copy(); K[2, 1, 4, 7] = np.nan
    assert_failed_from(run(c, al, K=K), clean, 1, 2, 3)
    q = {**c, "qpos_ref": c["qpos_ref"].copy()}; q["qpos_ref"][0, 1, 2] = np.inf
    assert_failed_from(run(q, al), clean, 1, 1, 3)
    u = {**c, "u": c["u"].copy()}; u["u"][0, 1, 3] = np.nan
    assert_failed_from(run(u, al), clean, 1, 0, 3)
    k = c["k"].copy(); k[1, 1, 0] = np.inf
    assert_failed_from(run(c, al, k=k), clean, 1, 1, 3)          # alpha = 0 too: 0 x inf is not finite
