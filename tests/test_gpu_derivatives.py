"""The derivatives query on the GPU (include/so100_query.h: so100_query_derivatives), through the C ABI and So100Sim.derivatives: the checks of
tests/test_derivatives_cpu.py on the kernel, under the bounds fixed there (tests/derivatives_support.py: 3 x the fp32 twin's recorded deviation
from the oracle's secant), plus what only a handle can show: the handle's own state, that a query only reads the state matrix, nullable
outputs, graph capture, every argument error, and examples/ilqr_reach.py end to end.

Shapes: M in {1, 3, 5, 65} (a lone wave, a few waves, more waves than one launch row), nsub in {1, 4, 16}."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import derivatives_support as S                           # noqa: E402
import scenes                                             # noqa: E402
import trajectory_support as TS                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 65
KEYS = ("A", "B", "qpos_next", "qvel_next", "bad")
# name -> (shape for M problems, dtype) of so100_derivatives_io's outputs, in the struct's order
OUTPUTS = {"A_dev": (lambda M: (M, 24, 24), torch.float32), "B_dev": (lambda M: (M, 24, 6), torch.float32), "qpos_next_dev": (lambda M: (13, M), torch.float32),
           "qvel_next_dev": (lambda M: (12, M), torch.float32), "bad_dev": (lambda M: (M,), torch.int32)}
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


def query(sim, u, q, v, mode, nsub, flags, iters=scenes.SHIPPED, eps=S.EPS):
    return host(sim.derivatives(dev(u, sim), dev(q, sim), dev(v, sim), mode=mode, nsub=nsub, flags=flags, eps=eps, solver_iters=iters[0], contact_iters=iters[1]))


def raw(sim, u, q, v, mode, nsub, flags, want, iters=scenes.SHIPPED, eps=S.STRUCT_EPS, stream=None, out=None):
    """the C ABI itself with the outputs of `want` alone, every output buffer pre-filled with SENTINEL: returns {name: tensor}"""
    from so100_mujoco_rl_amd import lib
    M = u.shape[0]
    us = dev(u, sim).t().contiguous()
    qs = None if q is None else dev(q, sim).t().contiguous()
    vs = None if v is None else dev(v, sim).t().contiguous()
    if out is None:
        out = {k: torch.full(shape(M), SENTINEL, dtype=dt, device=sim.device) for k, (shape, dt) in OUTPUTS.items()}
    io = lib.DerivativesIO(qpos_dev=None if qs is None else qs.data_ptr(), qvel_dev=None if vs is None else vs.data_ptr(), ctrl_dev=us.data_ptr(),
                           mode=TS.MODES[mode], nsub=nsub, flags=flags, solver_iters=iters[0], contact_iters=iters[1], eps=eps,
                           **{k: out[k].data_ptr() for k in want})
    assert sim.L.so100_query_derivatives(sim.h, C.byref(io), M, sim._stream() if stream is None else stream) == 0
    out["_keep"] = (us, qs, vs)
    return out


# ---- A: the smooth families against the oracle's secant ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["actions", "targets"])
@pytest.mark.parametrize("name", sorted(S.FAMILY_FLAGS))
def test_smooth_against_the_oracle(sim, name, mode):
    """flags 8, 11, 7 and F_REFERENCE: one family per form of the kernel"""
    c = S.family(name, mode); ref = S.smooth_reference(name, mode)
    got = query(sim, c["ctrl"], c["qpos"], c["qvel"], mode, S.NSUB, c["flags"], S.ITERS)
    assert not got["bad"].any()
    dev_ = S.deviation(got, ref)
    bound = {k: S.KERNEL_FACTOR*S.FP32_MEASURED[name][k] for k in dev_}
    print(f"[deriv-tol] gpu {name} {mode}: q rows {dev_['q']:.3e} (bound {bound['q']:.2e}) v rows {dev_['v']:.3e} (bound {bound['v']:.2e}), "
          f"next qpos {dev_['qpos']:.3e} (bound {bound['qpos']:.2e}) qvel {dev_['qvel']:.3e} (bound {bound['qvel']:.2e})")
    for k in dev_:
        assert dev_[k] <= bound[k], (k, dev_[k])
    if name in S.PINNED:                                      # the pinned cube's block is the identity, its couplings zero
        S.cube_block_is_the_identity(got, bound)


# ---- C: structure against So100Sim.trajectory on perturbed starts -----------------------------------------------------------------------
def struct_case(name):
    if name in ("floor", "grasp"):
        return S.contact_inputs(name)[:3]
    c = S.family(name, "actions")
    return c["qpos"], c["qvel"], TS.free_case("arm", "actions")["ctrl"][1]


def trajectory_step(sim, mode, nsub, flags):
    def step(q, v, u):
        g = sim.trajectory(dev(u[None], sim), dev(q, sim), dev(v, sim), mode=mode, nsub=nsub, flags=flags)
        assert (g["bad_step"] == -1).all()
        return g["qpos"][0].contiguous().cpu().numpy(), g["qvel"][0].contiguous().cpu().numpy()
    return step


# (inputs, flags, nsub): the run-time-flags form in live contact, then the three compile-time forms <8>, <11>, <7>
STRUCT = [("floor", scenes.REFP, 4), ("grasp", scenes.C5, 16), ("floor", scenes.FREE, 1), ("arm", scenes.ARM, 4), ("cube", scenes.NOPADS, 16)]


@pytest.mark.parametrize("mode", ["actions", "targets"])
@pytest.mark.parametrize("name, flags, nsub", STRUCT)
def test_structure_against_the_trajectory_query_record(sim, name, flags, nsub, mode):
    """A record, not a gate.  Both kernels instantiate the same trajectory_step<float> in one translation unit, but their code is generated
    separately: on the GPU the <11> form's matrices were 1-2 entries of 36 855 one ulp of the state away from the differences of two T = 1
    trajectory() calls on starts perturbed on the host, and the <7> form's unperturbed lane was not trajectory()'s row bit for bit; the
    run-time-flags form and <8> were equal throughout.  So the kernel's matrices and next state are held to the oracle in all four forms
    instead (A above), and the lane map, the column order and the actions-mode coupling are pinned bit for bit on the host twin
    (tests/test_derivatives_cpu.py, B).  Printed per form: the share of unequal entries and the largest difference."""
    q, v, a = struct_case(name)
    u = a if mode == "actions" else (q[:, :6] + (a*scenes.JS).astype(np.float32)).astype(np.float32)
    got = query(sim, u, q, v, mode, nsub, flags, eps=S.STRUCT_EPS)
    assert not got["bad"].any()
    step = trajectory_step(sim, mode, nsub, flags)
    qn, vn = step(q, v, u)
    nominal = np.concatenate([got["qpos_next"] != qn, got["qvel_next"] != vn], axis=1)
    nominal_diff = max(float(np.abs(got["qpos_next"] - qn).max()), float(np.abs(got["qvel_next"] - vn).max()))
    want = np.ascontiguousarray(S.expected_plain(step, q, v, u, S.STRUCT_EPS))
    have = np.ascontiguousarray(S.plain_block(got))
    unequal = have.view(np.int32) != want.view(np.int32)
    print(f"[deriv-tol] gpu structure {name} flags {flags} nsub {nsub} {mode} (record): matrices {int(unequal.sum())} of {unequal.size} entries differ, largest "
          f"|difference| {float(np.abs(have - want).max()):.3e}; unperturbed lane {int(nominal.sum())} of {nominal.size} differ, largest {nominal_diff:.3e}")
    assert have.shape == want.shape == (len(q), len(S.PLAIN_ROWS), len(S.PLAIN_COLS))


# ---- D: handle and surface -----------------------------------------------------------------------------------------------------------------------------
def test_the_handles_state(sim):
    """both-NULL state: the whole state matrix is bit-equal before and after, and the unperturbed lane is trajectory()'s prediction (bit for bit
    in this form, the run-time-flags one, as in every run-time-flags case of C)"""
    before = state_words(sim)
    g = torch.Generator(device="cpu").manual_seed(2)
    act = (torch.rand(N, 6, generator=g)*2 - 1).to(sim.device)
    a = host(sim.derivatives(act, mode="actions")); b = host(sim.derivatives(act, mode="actions"))
    pred = sim.trajectory(act[None], mode="actions")
    torch.cuda.synchronize()
    assert (state_words(sim) == before).all()
    for k in KEYS:
        assert bits(a[k]) == bits(b[k]), k
    assert not a["bad"].any() and np.isfinite(a["A"]).all() and np.isfinite(a["B"]).all()
    assert bits(a["qpos_next"]) == bits(pred["qpos"][0].contiguous().cpu().numpy()) and bits(a["qvel_next"]) == bits(pred["qvel"][0].contiguous().cpu().numpy())


def test_every_nullable_output_alone(sim):
    q, v, a, flags = S.contact_inputs("floor")
    full = raw(sim, a, q, v, "actions", 4, flags, list(OUTPUTS))
    torch.cuda.synchronize()
    via = query(sim, a, q, v, "actions", 4, flags, eps=S.STRUCT_EPS)
    assert bits(via["A"]) == bits(full["A_dev"].cpu().numpy()) and bits(via["qpos_next"]) == bits(full["qpos_next_dev"].t().contiguous().cpu().numpy())
    for name in OUTPUTS:
        one = raw(sim, a, q, v, "actions", 4, flags, [name])
        torch.cuda.synchronize()
        for k in OUTPUTS:
            if k == name:
                assert bits(one[k].cpu().numpy()) == bits(full[k].cpu().numpy()), k
            else:
                assert (one[k] == SENTINEL).all(), (name, k)
    # qvel NULL equals an explicit zero
    x = raw(sim, a, q, None, "actions", 4, flags, list(OUTPUTS)); y = raw(sim, a, q, np.zeros_like(v), "actions", 4, flags, list(OUTPUTS))
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert bits(x[k].cpu().numpy()) == bits(y[k].cpu().numpy()), k


def test_batch_and_place_independence(sim):
    c = S.family("cube", "targets")
    q, v, u = c["qpos"], c["qvel"], c["ctrl"]
    full = query(sim, u, q, v, "targets", 4, scenes.REFP)
    for m, k in ((0, 1), (64, 1), (31, 3)):                   # a lone wave and a few waves against their places among 65
        part = query(sim, u[m:m + k], q[m:m + k], v[m:m + k], "targets", 4, scenes.REFP)
        for key in KEYS:
            assert bits(full[key][m:m + k]) == bits(part[key]), (key, m)


def test_a_linear_graph_capture_replays_the_same_bits(sim):
    """nothing allocates, frees or synchronises: the call is captured into a hipGraph and replayed"""
    from so100_mujoco_rl_amd import lib
    q, v, a, flags = S.contact_inputs("floor")
    direct = raw(sim, a, q, v, "actions", 4, flags, list(OUTPUTS))
    torch.cuda.synchronize()
    us, qs, vs = direct["_keep"]
    M = a.shape[0]
    out = {k: torch.full(shape(M), SENTINEL, dtype=dt, device=sim.device) for k, (shape, dt) in OUTPUTS.items()}
    io = lib.DerivativesIO(qpos_dev=qs.data_ptr(), qvel_dev=vs.data_ptr(), ctrl_dev=us.data_ptr(), mode=TS.ACTIONS, nsub=4, flags=flags,
                           solver_iters=scenes.SHIPPED[0], contact_iters=scenes.SHIPPED[1], eps=S.STRUCT_EPS, **{k: out[k].data_ptr() for k in OUTPUTS})
    side = torch.cuda.Stream(device=sim.device)
    side.wait_stream(torch.cuda.current_stream(sim.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert sim.L.so100_query_derivatives(sim.h, C.byref(io), M, side.cuda_stream) == 0
    torch.cuda.current_stream(sim.device).wait_stream(side)
    for t in out.values():
        t.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert bits(out[k].cpu().numpy()) == bits(direct[k].cpu().numpy()), k


def test_non_finite_start_or_control(sim):
    q, v, a, flags = S.contact_inputs("floor")
    q, v, a = q.copy(), v.copy(), a.copy()
    clean = query(sim, a, q, v, "actions", 4, flags, eps=S.STRUCT_EPS)
    a[1, 3] = np.nan; q[2, 8] = np.inf; v[3, 2] = np.nan; a[4, 0] = np.inf
    got = query(sim, a, q, v, "actions", 4, flags, eps=S.STRUCT_EPS)
    assert got["bad"].tolist() == [0, 1, 1, 1, 1]
    for k in ("A", "B", "qpos_next", "qvel_next"):
        assert np.isnan(got[k][1:]).all(), k
        assert bits(got[k][0]) == bits(clean[k][0]), k        # the other problem never sees it


def test_argument_errors(sim):
    """exact code and message of every check, in the header's order; a rejected call enqueues nothing and the handle goes on working"""
    from so100_mujoco_rl_amd import lib
    L, h, st = sim.L, sim.h, sim._stream()
    buf = torch.full((24*24, N), float(SENTINEL), dtype=torch.float32, device=sim.device)
    inp = torch.zeros(64, N, dtype=torch.float32, device=sim.device)
    p, o = inp.data_ptr(), buf.data_ptr()
    fn = b"so100_query_derivatives: "
    ok = dict(qpos_dev=p, qvel_dev=p, ctrl_dev=p, mode=1, nsub=4, flags=lib.F_REFERENCE, solver_iters=2, contact_iters=20, eps=2.0**-6, A_dev=o, bad_dev=o)
    io = lambda **over: C.byref(lib.DerivativesIO(**{**ok, **over}))
    flags_msg = fn + b"SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)"
    nsub_msg = lambda nsub: fn + b"nsub must be in 1..1024, got %d" % nsub
    none = dict(A_dev=None, bad_dev=None)
    call = L.so100_query_derivatives
    calls = [
        (lambda: call(h, None, N, st), fn + b"null argument"),
        (lambda: call(h, io(), 0, st), fn + b"M must be >= 1, got 0"),
        (lambda: call(h, io(qpos_dev=None, qvel_dev=None), N - 1, st), fn + b"M must be the handle's N (65) where its state is read, got 64"),
        (lambda: call(h, io(qpos_dev=None), N, st), fn + b"qvel_dev given without qpos_dev"),
        (lambda: call(h, io(ctrl_dev=None), N, st), fn + b"ctrl_dev is required"),
        (lambda: call(h, io(mode=2), N, st), fn + b"unknown mode 2"),
        (lambda: call(h, io(mode=-1), N, st), fn + b"unknown mode -1"),
        (lambda: call(h, io(nsub=0), N, st), nsub_msg(0)),
        (lambda: call(h, io(nsub=1025), N, st), nsub_msg(1025)),
        (lambda: call(h, io(flags=256), N, st), fn + b"unknown flag bits"),
        (lambda: call(h, io(flags=lib.F_CUBE_PINNED | lib.F_PADS_CUBE), N, st), flags_msg),
        (lambda: call(h, io(flags=lib.F_CUBE_PINNED | lib.F_LINKS_CUBE), N, st), flags_msg),
        (lambda: call(h, io(solver_iters=0), N, st), fn + b"solver_iters must be in 1..64, got 0"),
        (lambda: call(h, io(contact_iters=65), N, st), fn + b"contact_iters must be in 1..64, got 65"),
        (lambda: call(h, io(eps=0.0), N, st), fn + b"eps must be finite and > 0, got 0"),
        (lambda: call(h, io(eps=-0.5), N, st), fn + b"eps must be finite and > 0, got -0.5"),
        (lambda: call(h, io(eps=float("inf")), N, st), fn + b"eps must be finite and > 0, got inf"),
        (lambda: call(h, io(eps=float("nan")), N, st), fn + b"eps must be finite and > 0, got nan"),
        (lambda: call(h, io(**none), N, st), fn + b"no output requested"),
        # the order: the first of several
        (lambda: call(h, io(qpos_dev=None, ctrl_dev=None, mode=7, nsub=0, flags=256, solver_iters=0, eps=0.0, **none), 0, st), fn + b"M must be >= 1, got 0"),
        (lambda: call(h, io(qpos_dev=None, ctrl_dev=None, mode=7, nsub=0, flags=256, solver_iters=0, eps=0.0, **none), N, st), fn + b"qvel_dev given without qpos_dev"),
        (lambda: call(h, io(ctrl_dev=None, mode=7, nsub=0, flags=256, solver_iters=0, eps=0.0, **none), N, st), fn + b"ctrl_dev is required"),
        (lambda: call(h, io(mode=7, nsub=0, flags=256, solver_iters=0, eps=0.0, **none), N, st), fn + b"unknown mode 7"),
        (lambda: call(h, io(nsub=0, flags=256, solver_iters=0, eps=0.0, **none), N, st), nsub_msg(0)),
        (lambda: call(h, io(flags=256 | lib.F_CUBE_PINNED | lib.F_PADS_CUBE, solver_iters=0, eps=0.0, **none), N, st), fn + b"unknown flag bits"),
        (lambda: call(h, io(flags=lib.F_CUBE_PINNED | lib.F_PADS_CUBE, solver_iters=0, eps=0.0, **none), N, st), flags_msg),
        (lambda: call(h, io(solver_iters=0, contact_iters=0, eps=0.0, **none), N, st), fn + b"solver_iters must be in 1..64, got 0"),
        (lambda: call(h, io(contact_iters=0, eps=0.0, **none), N, st), fn + b"contact_iters must be in 1..64, got 0"),
        (lambda: call(h, io(eps=0.0, **none), N, st), fn + b"eps must be finite and > 0, got 0"),
    ]
    current = torch.cuda.current_device()
    for c, msg in calls:
        assert c() == -1, msg
        assert L.so100_last_error() == msg
        assert torch.cuda.current_device() == current
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()                                # nothing was enqueued
    with pytest.raises(lib.So100Error):
        sim.derivatives(torch.zeros(N, 6, device=sim.device), mode="velocities")
    assert torch.isfinite(sim.derivatives(torch.zeros(N, 6, device=sim.device), mode="actions")["A"]).all()


def test_header_struct_and_macros():
    """header <-> lib.DerivativesIO field for field, and the macros: the CPU suite's checks, here as well"""
    import test_derivatives_cpu as CPU
    CPU.test_struct_matches_the_header_field_for_field()
    CPU.test_macros_match_the_header()
    CPU.test_the_header_says_what_the_result_is()


# ---- E: the example ----------------------------------------------------------------------------------------------------------------------------------------
def test_ilqr_reach_end_to_end():
    """examples/ilqr_reach.py on 8 envs, horizon 8, 40 steps: the planner's final mean |cube - ee| is below the zero-action baseline's on the same
    starts (examples/mppi_reach.py with 64 samples reaches 0.2662 m there; not a gate)"""
    from so100_mujoco_rl_amd import lib
    spec = importlib.util.spec_from_file_location("ilqr_reach", os.path.join(ROOT, "examples", "ilqr_reach.py"))
    ilqr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ilqr)
    result = {}
    for name, policy in (("ilqr", ilqr.Ilqr(8)), ("zero", ilqr.zero_action)):
        s = lib.So100Sim(lib.ENV01, 8, flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
        result[name] = ilqr.run(s, 40, policy)
        s.close()
    print(f"[deriv-tol] iLQR reach, 8 envs x H = 8, 40 steps: mean |cube - ee| {result['ilqr'][0]:.4f} m at reset -> {result['ilqr'][1]:.4f} m "
          f"(reward/step {result['ilqr'][2]:+.4f}); zero action -> {result['zero'][1]:.4f} m (reward/step {result['zero'][2]:+.4f}); MPPI: 0.2662 m")
    assert result["ilqr"][0] == result["zero"][0]                 # the same starts
    assert result["ilqr"][1] < result["zero"][1]
