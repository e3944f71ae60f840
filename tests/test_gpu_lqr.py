"""The LQR query on the GPU (include/so100_query.h: so100_query_lqr), through the C ABI and So100Sim.lqr: the checks of tests/test_lqr_cpu.py on
the kernel, under the bounds fixed in tests/lqr_support.py (KERNEL_FACTOR x the fp32 twin's recorded deviation from the numpy fp64 recursion), plus
what only a handle can show: nullable outputs, independence of M and place, repeatability, graph capture, that the handle's state is never
touched, every argument error, and examples/ilqr_reach.py --backward query end to end.

Shapes: M in {1, 3, 65} (bad and dV rows cross a 64 boundary at 65), T in {1, 2, 5, 16} (no carried Vxx, the first carry, ...), nx in {12, 24}."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import lqr_support as S                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8
NS = (12, 24)
TS_ = (1, 2, 5, 16)
MS = (1, 3, 65)
SENTINEL = -777
INPUTS = ("A", "B", "lx", "lxx", "lu", "luu", "lux", "u", "dx0")


@pytest.fixture(scope="module")
def sim():
    """N = 8, Env01 under F_CUBE_PINNED (the example's handle), after three random steps"""
    from so100_mujoco_rl_amd import lib
    s = lib.So100Sim(lib.ENV01, N, flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=3)
    s.reset()
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(3):
        s.step((torch.rand(N, 6, generator=g)*2 - 1).to(s.device))
    torch.cuda.synchronize()
    yield s
    s.close()


def state_words(sim):
    return torch.stack([sim.get_field(n, dtype=torch.int32) for n in sim.field_names()]).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def dev(a, sim):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(sim.device)


def query(sim, p):
    """So100Sim.lqr on a lqr_support.problem(): numpy outputs"""
    r = sim.lqr(dev(p["A"], sim), dev(p["B"], sim), dev(p["lx"], sim), dev(p["lxx"], sim), dev(p["lu"], sim), dev(p["luu"], sim), dev(p["lux"], sim), nx=p["nx"],
                reg=p["reg"], alpha=p["alpha"], u=dev(p["u"], sim), u_lo=p["u_lo"], u_hi=p["u_hi"], dx0=dev(p["dx0"], sim))
    return {k: v.cpu().numpy() for k, v in r.items()}


def raw(sim, p, want, stream=None, keep=None):
    """the C ABI itself with the outputs of `want` alone, every output buffer pre-filled with SENTINEL: ({name: tensor}, the io, the inputs kept alive)"""
    from so100_mujoco_rl_amd import lib
    T, M, n, shp = S.shapes(p)
    ins = keep if keep is not None else {k: dev(p[k], sim) for k in INPUTS}
    out = {k: torch.full(shp[k], SENTINEL, dtype=torch.int32 if k == "bad" else torch.float32, device=sim.device) for k in S.OUT}
    io = lib.LqrIO(nx=n, T=T, reg=p["reg"], alpha=p["alpha"], u_lo=p["u_lo"], u_hi=p["u_hi"],
                   **{k + "_dev": (None if t is None else t.data_ptr()) for k, t in ins.items()}, **{k + "_dev": out[k].data_ptr() for k in want})
    if stream is not False:
        assert sim.L.so100_query_lqr(sim.h, C.byref(io), M, sim._stream() if stream is None else stream) == 0
    return out, io, ins


# ---- A: against the references ----------------------------------------------------------------------------------------------------------------------------
def test_family_s_against_the_reference(sim):
    """every nx x T x M of the shapes: the kernel within KERNEL_FACTOR x the fp32 twin's record of the fp64 recursion"""
    worst = {k: 0.0 for k in S.FLOAT_OUT}
    for n in NS:
        for T in TS_:
            ref = S.reference_s(n, T)
            for M in MS:
                got = query(sim, S.first(S.family_s(n, T), M))
                assert (got["bad"] == -1).all()
                sub = {k: (ref[k][:M] if k in ("Vx0", "Vxx0", "dV") else ref[k][:, :M]) for k in S.FLOAT_OUT}
                for k, d in S.deviation(got, sub).items():
                    worst[k] = max(worst[k], d)
    print("[lqr-tol] gpu S " + " ".join(f"{k}={v:.2e} (bound {S.KERNEL_FACTOR*S.FP32_MEASURED['S'][k]:.1e})" for k, v in worst.items()))
    S.within(worst, "S", S.KERNEL_FACTOR)


def physics_problem(sim, n):
    """lqr_support.family_p from So100Sim's own queries"""
    from so100_mujoco_rl_amd import lib
    F = lib.F_CUBE_PINNED
    host = lambda r: {k: v.contiguous().cpu().numpy() for k, v in r.items()}
    roll = lambda U, q, v: host(sim.trajectory(dev(U, sim), dev(q, sim), dev(v, sim), mode="actions", nsub=S.P_NSUB, flags=F))
    der = lambda U, q, v: host(sim.derivatives(dev(U, sim), dev(q, sim), dev(v, sim), mode="actions", nsub=S.P_NSUB, flags=F))
    jac = lambda q: sim.jacobian(dev(q, sim))["jacp"].contiguous().cpu().numpy()
    return S.family_p(n, roll, der, jac)


def test_family_p_against_the_reference(sim):
    worst = {k: 0.0 for k in S.FLOAT_OUT}
    for n in NS:
        p, _ = physics_problem(sim, n)
        ref = S.reference(p)
        got = query(sim, p)
        assert (got["bad"] == -1).all() and (ref["bad"] == -1).all()
        for k, d in S.deviation(got, ref).items():
            worst[k] = max(worst[k], d)
    print("[lqr-tol] gpu P " + " ".join(f"{k}={v:.2e} (bound {S.KERNEL_FACTOR*S.FP32_MEASURED['P'][k]:.1e})" for k, v in worst.items()))
    S.within(worst, "P", S.KERNEL_FACTOR)


@pytest.mark.parametrize("n", NS)
def test_du_is_the_dense_minimiser(sim, n):
    for T in TS_:
        p = S.first(S.family_s(n, T), 3)
        dense = S.dense_minimiser(p)
        d = np.abs(query(sim, p)["du"] - dense).max()/max(1.0, np.abs(dense).max())
        assert d <= S.KERNEL_FACTOR*S.FP32_MEASURED["S"]["du"], (T, d)


@pytest.mark.parametrize("n", NS)
def test_clamp_step_and_start(sim, n):
    """u with bounds, alpha and dx0 through the kernel against the reference; every u + du inside the bounds; alpha = 0 from the origin moves nothing"""
    p = dict(S.first(S.family_s(n, 5), 3))
    rng = np.random.default_rng(4)
    p.update(u=rng.uniform(-0.6, 0.6, (5, 3, 6)).astype(np.float32), u_lo=-0.75, u_hi=0.5, alpha=0.5, dx0=(0.1*rng.standard_normal((3, n))).astype(np.float32))
    got, ref = query(sim, p), S.reference(p)
    S.within(S.deviation(got, ref), "S", S.KERNEL_FACTOR)
    new = p["u"] + got["du"]
    assert new.min() >= -0.75 - 1e-6 and new.max() <= 0.5 + 1e-6
    still = query(sim, dict(S.first(S.family_s(n, 5), 3), alpha=0.0))
    assert not still["du"].any() and not still["dx"].any() and still["k"].any()


# ---- B: what only the device shows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_each_output_alone_leaves_the_others_untouched(sim, n):
    p = S.first(S.family_s(n, 5), 3)
    full, _, _ = raw(sim, p, list(S.OUT))
    torch.cuda.synchronize()
    for name in S.OUT:
        want = [name] + (["k", "K"] if name in ("du", "dx") else [])
        out, _, _ = raw(sim, p, want)
        torch.cuda.synchronize()
        for k in S.OUT:
            if k in want:
                assert bits(out[k].cpu().numpy()) == bits(full[k].cpu().numpy()), (name, k)
            else:
                assert (out[k] == SENTINEL).all(), (name, k)


@pytest.mark.parametrize("n", NS)
def test_bits_do_not_depend_on_m_or_place_and_repeat(sim, n):
    base = S.family_s(n, 5)
    full, again = query(sim, base), query(sim, base)
    for k in S.OUT:
        assert bits(full[k]) == bits(again[k]), k               # two calls give the same bits
    sel = lambda a, k, m, c: a[m:m + c] if k in ("Vx0", "Vxx0", "dV", "bad") else a[:, m:m + c]
    for m, c in ((0, 1), (64, 1), (31, 3)):
        q = {k: (v if not isinstance(v, np.ndarray) else np.ascontiguousarray(v[:, m:m + c])) for k, v in base.items()}
        part = query(sim, q)
        for k in S.OUT:
            assert bits(sel(full[k], k, m, c)) == bits(part[k]), (k, m)


def test_a_linear_graph_capture_replays_the_same_bits(sim):
    p = dict(S.first(S.family_s(24, 5), 3))
    p["u"] = np.zeros((5, 3, 6), np.float32)
    direct, _, ins = raw(sim, p, list(S.OUT))
    torch.cuda.synchronize()
    out, io, _ = raw(sim, p, list(S.OUT), stream=False, keep=ins)
    side = torch.cuda.Stream(device=sim.device)
    side.wait_stream(torch.cuda.current_stream(sim.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert sim.L.so100_query_lqr(sim.h, C.byref(io), 3, side.cuda_stream) == 0
    torch.cuda.current_stream(sim.device).wait_stream(side)
    for t in out.values():
        t.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for k in S.OUT:
        assert bits(out[k].cpu().numpy()) == bits(direct[k].cpu().numpy()), k


def test_the_handle_state_is_never_touched(sim):
    before = state_words(sim)
    for n in NS:
        query(sim, S.first(S.family_s(n, 2), 3))
    torch.cuda.synchronize()
    assert bits(state_words(sim)) == bits(before)


# ---- C: the failure cases -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_failure_cases(sim, n):
    import test_lqr_cpu as CPU
    clean = query(sim, S.first(S.family_s(n, S.FAIL_T), S.FAIL_M))
    p0, p4 = S.indefinite_case(n)
    g = query(sim, p0)
    assert g["bad"].tolist() == [-1, S.FAIL_AT, -1]
    CPU.failed_outputs_are_nan(g, S.FAIL_PROBLEM)
    CPU.neighbours_untouched(g, clean)
    g4 = query(sim, p4)
    assert (g4["bad"] == -1).all()
    S.within(S.deviation(g4, S.reference(p4)), "S", S.KERNEL_FACTOR)
    for p in S.nonfinite_cases(n):
        g = query(sim, p)
        assert g["bad"].tolist() == [-1, S.FAIL_T, -1]
        CPU.failed_outputs_are_nan(g, S.FAIL_PROBLEM)
        CPU.neighbours_untouched(g, clean)


def test_argument_errors(sim):
    """exact code and message of every check, in the header's order; a rejected call enqueues nothing and the handle goes on working"""
    from so100_mujoco_rl_amd import lib
    L, h, st = sim.L, sim.h, sim._stream()
    M = 3
    buf = torch.full((4*M*24*24,), float(SENTINEL), dtype=torch.float32, device=sim.device)
    inp = torch.zeros(4*M*24*24, dtype=torch.float32, device=sim.device)
    p, o = inp.data_ptr(), buf.data_ptr()
    fn = b"so100_query_lqr: "
    ok = dict(nx=24, T=2, A_dev=p, B_dev=p, lx_dev=p, lxx_dev=p, reg=0.0, alpha=1.0, u_lo=-1.0, u_hi=1.0, k_dev=o, K_dev=o, bad_dev=o)
    io = lambda **over: C.byref(lib.LqrIO(**{**ok, **over}))
    none = dict(k_dev=None, K_dev=None, bad_dev=None)
    req = fn + b"A_dev, B_dev, lx_dev and lxx_dev are required"
    call = L.so100_query_lqr
    calls = [
        (lambda: call(h, None, M, st), fn + b"null argument"),
        (lambda: call(None, io(), M, st), fn + b"null argument"),
        (lambda: call(h, io(), 0, st), fn + b"M must be >= 1, got 0"),
        (lambda: call(h, io(nx=6), M, st), fn + b"nx must be 12 or 24, got 6"),
        (lambda: call(h, io(T=0), M, st), fn + b"T must be in 1..4096, got 0"),
        (lambda: call(h, io(T=4097), M, st), fn + b"T must be in 1..4096, got 4097"),
        (lambda: call(h, io(A_dev=None), M, st), req),
        (lambda: call(h, io(B_dev=None), M, st), req),
        (lambda: call(h, io(lx_dev=None), M, st), req),
        (lambda: call(h, io(lxx_dev=None), M, st), req),
        (lambda: call(h, io(reg=-1.0), M, st), fn + b"reg must be finite and >= 0, got -1"),
        (lambda: call(h, io(reg=float("nan")), M, st), fn + b"reg must be finite and >= 0, got nan"),
        (lambda: call(h, io(reg=float("inf")), M, st), fn + b"reg must be finite and >= 0, got inf"),
        (lambda: call(h, io(alpha=float("inf")), M, st), fn + b"alpha must be finite, got inf"),
        (lambda: call(h, io(u_lo=0.5, u_hi=0.25), M, st), fn + b"u_lo must be <= u_hi, got 0.5 and 0.25"),
        (lambda: call(h, io(du_dev=o, K_dev=None), M, st), fn + b"du_dev and dx_dev need k_dev and K_dev"),
        (lambda: call(h, io(dx_dev=o, k_dev=None), M, st), fn + b"du_dev and dx_dev need k_dev and K_dev"),
        (lambda: call(h, io(**none), M, st), fn + b"no output requested"),
        # the order: the first of several
        (lambda: call(h, io(nx=6, T=0, A_dev=None, reg=-1.0, du_dev=o, **none), 0, st), fn + b"M must be >= 1, got 0"),
        (lambda: call(h, io(nx=6, T=0, A_dev=None, reg=-1.0, du_dev=o, **none), M, st), fn + b"nx must be 12 or 24, got 6"),
        (lambda: call(h, io(T=0, A_dev=None, reg=-1.0, du_dev=o, **none), M, st), fn + b"T must be in 1..4096, got 0"),
        (lambda: call(h, io(A_dev=None, reg=-1.0, du_dev=o, **none), M, st), req),
        (lambda: call(h, io(reg=-1.0, alpha=float("nan"), u_lo=1.0, u_hi=0.0, du_dev=o, **none), M, st), fn + b"reg must be finite and >= 0, got -1"),
        (lambda: call(h, io(alpha=float("nan"), u_lo=1.0, u_hi=0.0, du_dev=o, **none), M, st), fn + b"alpha must be finite, got nan"),
        (lambda: call(h, io(u_lo=1.0, u_hi=0.0, du_dev=o, **none), M, st), fn + b"u_lo must be <= u_hi, got 1 and 0"),
        (lambda: call(h, io(du_dev=o, **none), M, st), fn + b"du_dev and dx_dev need k_dev and K_dev"),
    ]
    current = torch.cuda.current_device()
    for c, msg in calls:
        assert c() == -1, msg
        assert L.so100_last_error() == msg
        assert torch.cuda.current_device() == current
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()                                # nothing was enqueued
    with pytest.raises(lib.So100Error):
        sim.lqr(torch.zeros(2, M, 24, 24), torch.zeros(2, M, 24, 6), torch.zeros(3, M, 24), torch.zeros(3, M, 24, 24), nx=7)
    assert (query(sim, S.first(S.family_s(12, 2), M))["bad"] == -1).all()


def test_header_struct_and_macros():
    import test_lqr_cpu as CPU
    CPU.test_struct_matches_the_header_field_for_field()
    CPU.test_macros_match_the_header()


# ---- E: the example ----------------------------------------------------------------------------------------------------------------------------------------
def test_ilqr_reach_with_the_query_backward_pass():
    """examples/ilqr_reach.py --backward query on 8 envs, horizon 8, 40 steps ends below the zero-action baseline on the same starts; the torch
    backward pass's result is printed beside it (a record, not a gate: two fp32 paths through a closed loop need not agree)"""
    from so100_mujoco_rl_amd import lib
    spec = importlib.util.spec_from_file_location("ilqr_reach", os.path.join(ROOT, "examples", "ilqr_reach.py"))
    ilqr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ilqr)
    result = {}
    for name, policy in (("query", ilqr.Ilqr(8, backward="query")), ("torch", ilqr.Ilqr(8)), ("zero", ilqr.zero_action)):
        s = lib.So100Sim(lib.ENV01, 8, flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
        result[name] = ilqr.run(s, 40, policy)
        s.close()
    print(f"[lqr-tol] iLQR reach, 8 envs x H = 8, 40 steps: mean |cube - ee| {result['query'][0]:.4f} m at reset -> {result['query'][1]:.4f} m with "
          f"--backward query, {result['torch'][1]:.4f} m with the torch backward pass; zero action -> {result['zero'][1]:.4f} m")
    assert result["query"][0] == result["zero"][0]                # the same starts
    assert result["query"][1] < result["zero"][1]
