"""The trajectory query on the GPU (include/so100_query.h: so100_query_trajectory), through the C ABI and So100Sim.trajectory: the checks of
tests/test_trajectory_cpu.py on the kernel, under the bounds fixed there (tests/trajectory_support.py: 3 x the fp32 twin's recorded deviation
from the oracle), plus what only a handle can show: the handle's own state predicted against step(), that a query only reads the state
matrix, nullable outputs, graph capture, every argument error, and examples/mppi_reach.py end to end.

Shapes: M in {1, 65, 130} (a lone lane, a tail, three workgroups), T in {1, 2, 3}, nsub in {1, 4, 16}."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import scenes                                             # noqa: E402
import substep_harness as SH                              # noqa: E402
import trajectory_support as S                            # noqa: E402
from gpu_support import inject_state, make_sim            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 65
FIELDS = ("qpos", "qvel", "ee", "ncon", "dropped", "sig", "residual")
# name -> (rows per step, dtype, per step?) of so100_trajectory_io's outputs, in the struct's order
OUTPUTS = {"qpos_traj_dev": (13, torch.float32, True), "qvel_traj_dev": (12, torch.float32, True), "ee_traj_dev": (3, torch.float32, True),
           "qpos_final_dev": (13, torch.float32, False), "qvel_final_dev": (12, torch.float32, False), "ncon_dev": (1, torch.int32, True),
           "dropped_dev": (1, torch.int32, True), "sig_dev": (1, torch.int32, True), "residual_dev": (1, torch.float32, True),
           "bad_step_dev": (1, torch.int32, False)}
SENTINEL = -777


@pytest.fixture(scope="module")
def sim():
    """N = 65, Env01, the reference physics, after three random steps"""
    from so100_mujoco_rl_amd import lib
    s = lib.So100Sim(lib.ENV01, N, flags=lib.F_REFERENCE, max_episode_steps=0, seed=3)
    s.reset()
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(3):
        s.step((torch.rand(N, 6, generator=g)*2 - 1).to(s.device))
    torch.cuda.synchronize()
    yield s
    s.close()


def state_words(sim):
    return torch.stack([sim.get_field(n, dtype=torch.int32) for n in sim.field_names()]).cpu().numpy()


def host(res):
    return {k: v.contiguous().cpu().numpy() for k, v in res.items()}


def dev(a, sim):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(sim.device)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def query(sim, a, q, v, mode, nsub, flags, iters=scenes.SHIPPED):
    return host(sim.trajectory(dev(a, sim), dev(q, sim), dev(v, sim), mode=mode, nsub=nsub, flags=flags, solver_iters=iters[0], contact_iters=iters[1]))


def raw(sim, a, q, v, mode, nsub, flags, want, iters=scenes.SHIPPED, stream=None):
    """the C ABI itself with the outputs of `want` alone, every output buffer pre-filled with SENTINEL: returns {name: tensor [rows..., M]}"""
    from so100_mujoco_rl_amd import lib
    T, M = a.shape[0], a.shape[1]
    us = dev(a, sim).permute(0, 2, 1).contiguous()
    qs = None if q is None else dev(q, sim).t().contiguous()
    vs = None if v is None else dev(v, sim).t().contiguous()
    out = {k: torch.full(((T,) if per_step else ()) + (rows, M), SENTINEL, dtype=dt, device=sim.device) for k, (rows, dt, per_step) in OUTPUTS.items()}
    io = lib.TrajectoryIO(qpos_dev=None if qs is None else qs.data_ptr(), qvel_dev=None if vs is None else vs.data_ptr(), ctrl_dev=us.data_ptr(),
                          mode=S.MODES[mode], T=T, nsub=nsub, flags=flags, solver_iters=iters[0], contact_iters=iters[1],
                          **{k: out[k].data_ptr() for k in want})
    assert sim.L.so100_query_trajectory(sim.h, C.byref(io), M, sim._stream() if stream is None else stream) == 0
    out["_keep"] = (us, qs, vs)
    return out


# ---- A: per-substep parity with the oracle, every contact kind --------------------------------------------------------------------------------------------
class HipTrajectory:
    """device_substep of the harness: T = 1, nsub = 1, mode = actions, explicit states.  The m problems sit at the even places among 2 m + 1
    (the rest: scenes.idle_batch), so M is no multiple of 64 and every wave holds both."""
    def __init__(self, sim, m, flags, iters=S.PARITY_ITERS):
        self.sim, self.m, self.flags, self.iters = sim, m, flags, iters
        self.QP, self.QV = (a.astype(np.float32) for a in scenes.idle_batch(2*m + 1)); self.A = np.zeros((1, 2*m + 1, 6), np.float32)

    def __call__(self, q32, v32, act):
        m = self.m
        self.QP[0:2*m:2] = q32; self.QV[0:2*m:2] = v32; self.A[0, 0:2*m:2] = act
        g = query(self.sim, self.A, self.QP, self.QV, "actions", 1, self.flags, self.iters)
        assert not g["dropped"].any() and (g["bad_step"] == -1).all()
        pick = slice(0, 2*m, 2)
        return (g["qpos"][0, pick].astype(np.float64), g["qvel"][0, pick].astype(np.float64), g["ncon"][0, pick], g["sig"][0, pick], g["residual"][0, pick])


def test_pad_floor_per_substep(sim):
    m, nsub = 96, 24
    qpos, qvel, act = scenes.floor_batch(m, 0)
    T = SH.run_substep_parity(HipTrajectory(sim, m, scenes.REFP), qpos, qvel, act, scenes.REFP, nsub, f"HIP trajectory {S.PARITY_ITERS} pad/floor")
    SH.check_tally(T, m*nsub//3, iters=S.PARITY_ITERS)


def test_pad_cube_grasp_per_substep(sim):
    m, nsub = 64, 40
    qpos, qvel, act = scenes.grasp_batch(m, 1)
    T = SH.run_substep_parity(HipTrajectory(sim, m, scenes.C5), qpos, qvel, act, scenes.C5, nsub, f"HIP trajectory {S.PARITY_ITERS} grasp")
    SH.check_tally(T, m*nsub//3, m*nsub//4, iters=S.PARITY_ITERS)


def test_floor_cube_per_substep(sim):
    m, nsub = 64, 24
    qpos, qvel, act = scenes.floor_cube_batch(m, 0)
    T = SH.run_substep_parity(HipTrajectory(sim, m, scenes.C5), qpos, qvel, act, scenes.C5, nsub, f"HIP trajectory {S.PARITY_ITERS} cube on the floor")
    SH.check_tally(T, m*nsub//3, m*nsub//4, iters=S.PARITY_ITERS)
    SH.check_moving_cube(T)


def test_link_proxies_per_substep(sim):
    m, nsub = 48, 24
    qpos, qvel, act = scenes.wrist_first_batch(m, 0)
    T = SH.run_substep_parity(HipTrajectory(sim, m, scenes.LINKS), qpos, qvel, act, scenes.LINKS, nsub, f"HIP trajectory {S.PARITY_ITERS} link proxies")
    SH.check_tally(T, m*nsub//3, iters=S.PARITY_ITERS)


def test_link_cube_per_substep(sim):
    m, nsub = 32, 12
    qpos, qvel, act = scenes.link_cube_batch(m, 0)
    T = SH.run_substep_parity(HipTrajectory(sim, m, scenes.LCUBE), qpos, qvel, act, scenes.LCUBE, nsub, f"HIP trajectory {S.PARITY_ITERS} link proxies vs cube")
    SH.check_tally(T, m*nsub//3, m*nsub//3, iters=S.PARITY_ITERS)


# ---- B: contact-free trajectories against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["actions", "targets"])
@pytest.mark.parametrize("name", sorted(S.FREE_FLAGS))
def test_contact_free_against_the_oracle(sim, name, mode):
    """flags 11 and 7: compile-time forms of the kernel (the run-time-flags form: A, C and E)"""
    c = S.free_case(name, mode)
    got = query(sim, c["ctrl"], c["qpos"], c["qvel"], mode, S.FREE_NSUB, c["flags"])
    assert (got["bad_step"] == -1).all() and not got["ncon"].any() and not got["sig"].any()
    dev_ = S.deviation(got, c["ref"])
    ee = float(np.abs(got["ee"].astype(np.float64) - c["ref"]["ee"]).max())
    bound = {k: S.KERNEL_FACTOR*S.FP32_MEASURED[name][k] for k in dev_}
    print(f"[traj-tol] gpu {name} {mode}: qpos {dev_['qpos']:.3e} (bound {bound['qpos']:.2e}) qvel {dev_['qvel']:.3e} (bound {bound['qvel']:.2e}) "
          f"ee {ee:.3e} (bound {S.ee_bound(bound['qpos']):.2e})")
    for k in dev_:
        assert dev_[k] <= bound[k], (k, dev_[k])
    assert ee <= S.ee_bound(bound["qpos"])


# ---- C: warm carry in contact against the oracle --------------------------------------------------------------------------------------------------------
def test_warm_carry_in_contact(sim):
    c = S.warm_case()
    assert c["in_contact"].sum() >= 20
    got = query(sim, c["ctrl"], c["qpos"], c["qvel"], "actions", S.WARM_NSUB, c["flags"], S.WARM_ITERS)
    keep = c["keep"]
    for t in range(S.WARM_T):
        assert (got["ncon"][t][keep] == c["count"][keep]).all() and (got["sig"][t][keep] == c["sig"][keep]).all(), t
    assert not got["dropped"][:, keep].any() and (got["bad_step"] == -1).all()
    dev_ = S.deviation(got, c["ref"], keep)
    bound = {k: S.KERNEL_FACTOR*S.FP32_MEASURED["warm"][k] for k in dev_}
    print(f"[traj-tol] gpu warm carry {S.WARM_ITERS}: qpos {dev_['qpos']:.3e} (bound {bound['qpos']:.2e}) qvel {dev_['qvel']:.3e} (bound {bound['qvel']:.2e})")
    for k in dev_:
        assert dev_[k] <= bound[k], (k, dev_[k])


# ---- D: the handle's state: prediction against step() -------------------------------------------------------------------------------------------------------
def predict_and_step(flags, states=None):
    """Env01, N = 65, the shipped (2, 20), frame_skip 16, no TimeLimit: a few random steps (the warm rows are live), then trajectory(actions[3])
    on the handle's state against three step() calls with the same actions.  Returns (largest |qpos| and |qvel| difference, words unchanged)."""
    s = make_sim(1, N, flags=flags, solver_iters=2, contact_iters=20, frame_skip=16, max_episode_steps=0, seed=4)
    try:
        s.reset()
        if states is not None:
            inject_state(s, *states)
        g = torch.Generator(device="cpu").manual_seed(1)
        for _ in range(4):
            s.step((torch.rand(N, 6, generator=g)*2 - 1).to(s.device))
        act = (torch.rand(3, N, 6, generator=g)*2 - 1).to(s.device)
        before = state_words(s)
        got = host(s.trajectory(act, mode="actions"))
        unchanged = (state_words(s) == before).all()
        dq = dv = 0.0
        for t in range(3):
            s.step(act[t].contiguous())
            qpos, qvel = s.get_state()
            dq = max(dq, float(np.abs(got["qpos"][t] - qpos.t().cpu().numpy()).max())); dv = max(dv, float(np.abs(got["qvel"][t] - qvel.t().cpu().numpy()).max()))
        assert (got["bad_step"] == -1).all()
        return dq, dv, unchanged
    finally:
        s.close()


@pytest.mark.parametrize("flags", [scenes.FREE, scenes.ARM, scenes.NOPADS])
def test_the_handles_state_is_predicted(flags):
    """bounds: those test_multiwave_step_kernel_equals_throughput_kernel holds the two step kernels to each other with"""
    dq, dv, unchanged = predict_and_step(flags)
    print(f"[traj-tol] gpu prediction vs step, flags {flags}: qpos {dq:.3e} (bound 2e-6) qvel {dv:.3e} (bound 2e-5)")
    assert unchanged                                          # the whole state matrix, bit for bit
    assert dq <= 2e-6 and dv <= 2e-5


def test_the_handles_state_in_pad_contact_record():
    """a record, not a gate: the 4-wave step kernel sums its contact rows over several lanes, and no bound for that difference is known"""
    qpos, qvel, _ = scenes.floor_batch(N, 0)
    dq, dv, unchanged = predict_and_step(scenes.REFP, (qpos, qvel))
    print(f"[traj-tol] gpu prediction vs step, F_REFERENCE on floor_batch states (record): qpos {dq:.3e} qvel {dv:.3e}")
    assert unchanged


# ---- E: exact properties --------------------------------------------------------------------------------------------------------------------------------------
def test_prefix_batch_and_repeat_independence(sim):
    q, v, a = S.contact_inputs()
    full = query(sim, a, q, v, "actions", 4, scenes.REFP)
    assert full["ncon"].any()
    again = query(sim, a, q, v, "actions", 4, scenes.REFP)
    for k in FIELDS + ("bad_step",):
        assert bits(full[k]) == bits(again[k]), k
    for Tp in (1, 2):                                         # row t < T' of a T-step call = row t of the T'-step call
        part = query(sim, a[:Tp], q, v, "actions", 4, scenes.REFP)
        for k in FIELDS:
            assert bits(full[k][:Tp]) == bits(part[k]), (k, Tp)
    for m in (0, 64, 129):                                    # M = 1 against inside 130
        one = query(sim, a[:, m:m + 1], q[m:m + 1], v[m:m + 1], "actions", 4, scenes.REFP)
        for k in FIELDS:
            assert bits(full[k][:, m:m + 1]) == bits(one[k]), (k, m)
    tail = query(sim, a[:, :65], q[:65], v[:65], "actions", 4, scenes.REFP)
    for k in FIELDS:
        assert bits(full[k][:, :65]) == bits(tail[k]), k


@pytest.mark.parametrize("nsub", [1, 4, 16])
def test_targets_mode_reproduces_an_actions_run(sim, nsub):
    """targets = q_t + 0.075 a_t in float32 (a product rounded, a sum rounded) from the actions run's own rows"""
    q, v, a = S.contact_inputs()
    run = query(sim, a, q, v, "actions", nsub, scenes.REFP)
    starts = np.concatenate([q[None, :, :6], run["qpos"][:-1, :, :6]])
    targets = (starts + (a*scenes.JS).astype(np.float32)).astype(np.float32)
    rerun = query(sim, targets, q, v, "targets", nsub, scenes.REFP)
    for k in FIELDS:
        assert bits(run[k]) == bits(rerun[k]), k


def test_every_nullable_output_alone_and_the_finals(sim):
    q, v, a = (x[:65] if x.ndim == 2 else x[:, :65] for x in S.contact_inputs())
    full = raw(sim, a, q, v, "actions", 4, scenes.C5, list(OUTPUTS))
    torch.cuda.synchronize()
    assert bits(full["qpos_final_dev"].cpu().numpy()) == bits(full["qpos_traj_dev"][-1].cpu().numpy())
    assert bits(full["qvel_final_dev"].cpu().numpy()) == bits(full["qvel_traj_dev"][-1].cpu().numpy())
    via = query(sim, a, q, v, "actions", 4, scenes.C5)
    assert bits(via["qpos"]) == bits(full["qpos_traj_dev"].permute(0, 2, 1).contiguous().cpu().numpy())
    for name in OUTPUTS:
        one = raw(sim, a, q, v, "actions", 4, scenes.C5, [name])
        torch.cuda.synchronize()
        for k in OUTPUTS:
            if k == name:
                assert bits(one[k].cpu().numpy()) == bits(full[k].cpu().numpy()), k
            else:
                assert (one[k] == SENTINEL).all(), (name, k)
    # qvel NULL equals an explicit zero
    x = raw(sim, a, q, None, "actions", 4, scenes.C5, list(OUTPUTS)); y = raw(sim, a, q, np.zeros_like(v), "actions", 4, scenes.C5, list(OUTPUTS))
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert bits(x[k].cpu().numpy()) == bits(y[k].cpu().numpy()), k


def test_the_state_matrix_is_only_read(sim):
    before = state_words(sim)
    g = torch.Generator(device="cpu").manual_seed(2)
    act = (torch.rand(2, N, 6, generator=g)*2 - 1).to(sim.device)
    a = host(sim.trajectory(act, mode="actions")); b = host(sim.trajectory(act, mode="actions"))
    assert (state_words(sim) == before).all()
    for k in FIELDS:
        assert bits(a[k]) == bits(b[k]), k
    assert np.isfinite(a["qpos"]).all() and (a["bad_step"] == -1).all()


def test_a_linear_graph_capture_replays_the_same_bits(sim):
    """nothing allocates, frees or synchronises: the call is captured into a hipGraph and replayed"""
    from so100_mujoco_rl_amd import lib
    q, v, a = (x[:65] if x.ndim == 2 else x[:, :65] for x in S.contact_inputs())
    direct = raw(sim, a, q, v, "actions", 4, scenes.REFP, list(OUTPUTS))
    torch.cuda.synchronize()
    us, qs, vs = direct["_keep"]
    T, M = a.shape[0], a.shape[1]
    out = {k: torch.full(((T,) if per_step else ()) + (rows, M), SENTINEL, dtype=dt, device=sim.device) for k, (rows, dt, per_step) in OUTPUTS.items()}
    io = lib.TrajectoryIO(qpos_dev=qs.data_ptr(), qvel_dev=vs.data_ptr(), ctrl_dev=us.data_ptr(), mode=S.ACTIONS, T=T, nsub=4, flags=scenes.REFP,
                          solver_iters=scenes.SHIPPED[0], contact_iters=scenes.SHIPPED[1], **{k: out[k].data_ptr() for k in OUTPUTS})
    side = torch.cuda.Stream(device=sim.device)
    side.wait_stream(torch.cuda.current_stream(sim.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert sim.L.so100_query_trajectory(sim.h, C.byref(io), M, side.cuda_stream) == 0
    torch.cuda.current_stream(sim.device).wait_stream(side)
    for t in out.values():
        t.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert bits(out[k].cpu().numpy()) == bits(direct[k].cpu().numpy()), k


def test_non_finite_control_or_state(sim):
    q, v, a = S.contact_inputs()
    q, v, a = q[:6].copy(), v[:6].copy(), a[:, :6].copy()
    clean = query(sim, a, q, v, "actions", 4, scenes.REFP)
    a[1, 1, 3] = np.nan; a[2, 2, 0] = np.inf; a[0, 3, 5] = np.nan
    q[4, 8] = np.nan; v[5, 2] = np.inf
    got = query(sim, a, q, v, "actions", 4, scenes.REFP)
    assert got["bad_step"].tolist() == [-1, 1, 2, 0, 0, 0]
    for m, t0 in ((1, 1), (2, 2), (3, 0), (4, 0), (5, 0)):
        for k in FIELDS:
            assert bits(got[k][:t0, m]) == bits(clean[k][:t0, m]), (k, m)       # the rows before it
        for k in ("qpos", "qvel", "ee", "residual"):
            assert np.isnan(got[k][t0:, m]).all(), (k, m)
        for k in ("ncon", "dropped", "sig"):
            assert not got[k][t0:, m].any(), (k, m)
    for k in FIELDS:
        assert bits(got[k][:, 0]) == bits(clean[k][:, 0]), k                   # the other problems never see it
    fin = raw(sim, a, q, v, "actions", 4, scenes.REFP, ["qpos_final_dev", "qvel_final_dev"])
    torch.cuda.synchronize()
    assert torch.isnan(fin["qpos_final_dev"][:, 1:]).all() and torch.isfinite(fin["qpos_final_dev"][:, 0]).all() and torch.isnan(fin["qvel_final_dev"][:, 1:]).all()


# ---- F: the surface -----------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(sim):
    """exact code and message of every check, in the header's order; a rejected call enqueues nothing and the handle goes on working"""
    from so100_mujoco_rl_amd import lib
    L, h, st = sim.L, sim.h, sim._stream()
    buf = torch.full((64, N), float(SENTINEL), dtype=torch.float32, device=sim.device)
    inp = torch.zeros(64, N, dtype=torch.float32, device=sim.device)
    p, o = inp.data_ptr(), buf.data_ptr()
    fn = b"so100_query_trajectory: "
    ok = dict(qpos_dev=p, qvel_dev=p, ctrl_dev=p, mode=1, T=2, nsub=4, flags=lib.F_REFERENCE, solver_iters=2, contact_iters=20, qpos_traj_dev=o, bad_step_dev=o)
    io = lambda **over: C.byref(lib.TrajectoryIO(**{**ok, **over}))
    flags_msg = fn + b"SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)"
    limits = lambda T, nsub: fn + b"T must be in 1..4096, nsub in 1..1024 and T * nsub <= 65536, got T = %d, nsub = %d" % (T, nsub)
    calls = [
        (lambda: L.so100_query_trajectory(h, None, N, st), fn + b"null argument"),
        (lambda: L.so100_query_trajectory(h, io(), 0, st), fn + b"M must be >= 1, got 0"),
        (lambda: L.so100_query_trajectory(h, io(qpos_dev=None, qvel_dev=None), N - 1, st), fn + b"M must be the handle's N (65) where its state is read, got 64"),
        (lambda: L.so100_query_trajectory(h, io(qpos_dev=None), N, st), fn + b"qvel_dev given without qpos_dev"),
        (lambda: L.so100_query_trajectory(h, io(ctrl_dev=None), N, st), fn + b"ctrl_dev is required"),
        (lambda: L.so100_query_trajectory(h, io(mode=2), N, st), fn + b"unknown mode 2"),
        (lambda: L.so100_query_trajectory(h, io(mode=-1), N, st), fn + b"unknown mode -1"),
        (lambda: L.so100_query_trajectory(h, io(T=0), N, st), limits(0, 4)),
        (lambda: L.so100_query_trajectory(h, io(T=4097, nsub=1), N, st), limits(4097, 1)),
        (lambda: L.so100_query_trajectory(h, io(nsub=0), N, st), limits(2, 0)),
        (lambda: L.so100_query_trajectory(h, io(T=1, nsub=1025), N, st), limits(1, 1025)),
        (lambda: L.so100_query_trajectory(h, io(T=4096, nsub=17), N, st), limits(4096, 17)),
        (lambda: L.so100_query_trajectory(h, io(flags=256), N, st), fn + b"unknown flag bits"),
        (lambda: L.so100_query_trajectory(h, io(flags=lib.F_CUBE_PINNED | lib.F_PADS_CUBE), N, st), flags_msg),
        (lambda: L.so100_query_trajectory(h, io(flags=lib.F_CUBE_PINNED | lib.F_LINKS_CUBE), N, st), flags_msg),
        (lambda: L.so100_query_trajectory(h, io(solver_iters=0), N, st), fn + b"solver_iters must be in 1..64, got 0"),
        (lambda: L.so100_query_trajectory(h, io(contact_iters=65), N, st), fn + b"contact_iters must be in 1..64, got 65"),
        (lambda: L.so100_query_trajectory(h, io(qpos_traj_dev=None, bad_step_dev=None), N, st), fn + b"no output requested"),
        # the order: the first of several
        (lambda: L.so100_query_trajectory(h, io(qpos_dev=None, ctrl_dev=None, mode=7, T=0, flags=256, solver_iters=0, qpos_traj_dev=None, bad_step_dev=None), 0, st),
         fn + b"M must be >= 1, got 0"),
        (lambda: L.so100_query_trajectory(h, io(qpos_dev=None, ctrl_dev=None, mode=7, T=0, flags=256, solver_iters=0, qpos_traj_dev=None, bad_step_dev=None), N, st),
         fn + b"qvel_dev given without qpos_dev"),
        (lambda: L.so100_query_trajectory(h, io(ctrl_dev=None, mode=7, T=0, flags=256, solver_iters=0, qpos_traj_dev=None, bad_step_dev=None), N, st), fn + b"ctrl_dev is required"),
        (lambda: L.so100_query_trajectory(h, io(mode=7, T=0, flags=256, solver_iters=0, qpos_traj_dev=None, bad_step_dev=None), N, st), fn + b"unknown mode 7"),
        (lambda: L.so100_query_trajectory(h, io(T=0, flags=256, solver_iters=0, qpos_traj_dev=None, bad_step_dev=None), N, st), limits(0, 4)),
        (lambda: L.so100_query_trajectory(h, io(flags=256 | lib.F_CUBE_PINNED | lib.F_PADS_CUBE, solver_iters=0, qpos_traj_dev=None, bad_step_dev=None), N, st), fn + b"unknown flag bits"),
        (lambda: L.so100_query_trajectory(h, io(flags=lib.F_CUBE_PINNED | lib.F_PADS_CUBE, solver_iters=0, qpos_traj_dev=None, bad_step_dev=None), N, st), flags_msg),
        (lambda: L.so100_query_trajectory(h, io(solver_iters=0, contact_iters=0, qpos_traj_dev=None, bad_step_dev=None), N, st), fn + b"solver_iters must be in 1..64, got 0"),
    ]
    current = torch.cuda.current_device()
    for call, msg in calls:
        assert call() == -1, msg
        assert L.so100_last_error() == msg
        assert torch.cuda.current_device() == current
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()                                # nothing was enqueued
    with pytest.raises(lib.So100Error):
        sim.trajectory(torch.zeros(1, N, 6, device=sim.device), mode="velocities")
    assert torch.isfinite(sim.trajectory(torch.zeros(1, N, 6, device=sim.device), mode="actions")["qpos"]).all()


def test_mppi_reach_end_to_end():
    """examples/mppi_reach.py on 8 envs x 64 samples x T = 8: the planner's final mean |cube - ee| is below the zero-action baseline's on the same starts"""
    from so100_mujoco_rl_amd import lib
    spec = importlib.util.spec_from_file_location("mppi_reach", os.path.join(ROOT, "examples", "mppi_reach.py"))
    mppi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mppi)
    result = {}
    for name, policy in (("mppi", mppi.Mppi(64, 8)), ("zero", mppi.zero_action)):
        s = lib.So100Sim(lib.ENV01, 8, flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
        result[name] = mppi.run(s, 40, policy)
        s.close()
    print(f"[traj-tol] MPPI reach, 8 envs x 64 samples x T = 8, 40 steps: mean |cube - ee| {result['mppi'][0]:.4f} m at reset -> {result['mppi'][1]:.4f} m "
          f"(reward/step {result['mppi'][2]:+.4f}); zero action -> {result['zero'][1]:.4f} m (reward/step {result['zero'][2]:+.4f})")
    assert result["mppi"][0] == result["zero"][0]                 # the same starts
    assert result["mppi"][1] < result["zero"][1]
