"""The two sampling-planner queries on the GPU (include/so100_query.h: so100_query_plan_sample, so100_query_cost_blend), through the C ABI and
So100Sim.plan_sample / cost_blend: the cases of tests/test_mppi_cpu.py on the kernels, under the bounds fixed there (tests/mppi_support.py: 3 x the fp32
twin's recorded deviation from the numpy reference), the exact properties within the kernels, plus what only the device can show: each output alone,
graph replay of the three-call planning step, the handle's state, the copies trajectory() does not make, every argument error, the three queries
chained on the device and examples/mppi_reach.py --plan query end to end.

Shapes (mppi_support.SHAPES): K in {1, 3, 63, 64, 65, 256, 257, 1030} -- inside a wave, a full wave, one over, a full workgroup, one over, more than
four rounds per thread -- x N in {1, 3} x T in {1, 3}, K = 4096 once, N = 70 at K = 3.  No physics but where trajectory() is called: every other case
is seeded arrays, a launch or two each."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cost_support as CS                                 # noqa: E402
import mppi_support as S                                  # noqa: E402
import scenes                                             # noqa: E402
import trajectory_support as TS                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5
SENTINEL = -777.0
bits = S.bits


@pytest.fixture(scope="module")
def sim():
    """N = 5, Env01, the reference physics, after three random steps (the two queries never look at it)"""
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


def dev(a, sim, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(sim.device)


def kernel_sample(sim):
    """So100Sim.plan_sample behind mppi_support's `sample` signature"""
    def f(plan, K, sigma, seed=0, draw=0, id_offset=0, u_lo=-1.0, u_hi=1.0, qpos=None, qvel=None):
        res = sim.plan_sample(dev(plan, sim), K, sigma, seed=seed, draw=draw, id_offset=id_offset, u_lo=u_lo, u_hi=u_hi, qpos=dev(qpos, sim), qvel=dev(qvel, sim))
        n = plan.shape[1]
        out = {"ctrl": res["ctrl"].contiguous().cpu().numpy().reshape(plan.shape[0], n, K, 6)}
        for k, w in (("qpos", 13), ("qvel", 12)):
            if k in res:
                out[k] = res[k].contiguous().cpu().numpy().reshape(n, K, w)
        return out
    return f


def kernel_blend(sim):
    def f(cost, qpos, qvel, u, target, temperature, bad_step=None, u_fallback=None, shift=0, tail="zero"):
        T, n, K = u.shape[:3]
        cols = lambda a: None if a is None else dev(a, sim).reshape(T, n*K, a.shape[-1])
        res = sim.cost_blend(cols(qpos), cols(qvel), cols(u), K, temperature=float(np.float32(temperature)), bad_step=dev(bad_step, sim, np.int32),
                             u_fallback=dev(u_fallback, sim), shift=shift, tail=tail, target=dev(target, sim), **cost)
        return {k: v.contiguous().cpu().numpy() for k, v in res.items()}
    return f


def kernel_select_cost(sim):
    """so100_query_cost_select's cost on the same columns, in chunks of at most its 16 candidates"""
    def f(cost, qpos, qvel, u, target, bad_step):
        parts = []
        for k0 in range(0, u.shape[2], CS.MAX_L):
            sl = slice(k0, k0 + CS.MAX_L)
            res = sim.cost_select(dev(qpos[:, :, sl], sim), dev(qvel[:, :, sl], sim), dev(u[:, :, sl], sim), bad_step=None if bad_step is None else dev(bad_step[:, sl], sim, np.int32),
                                  target=dev(target, sim), **cost)
            parts.append(res["cost"].cpu().numpy())
        return np.concatenate(parts, axis=1)
    return f


def show(tag, d):
    print(f"[mppi-tol] gpu {tag}: " + " ".join(f"{k} {v:.3e}" + (f" (bound {S.KERNEL_FACTOR*S.FP32_MEASURED[k]:.2e})" if k in S.FP32_MEASURED else "") for k, v in d.items()))


def within(d):
    for k, v in S.FP32_MEASURED.items():
        if k in d:
            assert d[k] <= S.KERNEL_FACTOR*v, (k, d[k], S.KERNEL_FACTOR*v)


# ---- against the reference -------------------------------------------------------------------------------------------------------------------------------
def test_against_the_reference(sim):
    d = S.all_deviations(kernel_sample(sim), kernel_blend(sim))
    show("every case", d)
    print(f"[mppi-tol] gpu ctrl: the derived bound max(sigma) x NOISE_EPS + 1 ulp = {S.CTRL_DERIVED:.3e}")
    within(d)
    assert d["ctrl"] <= S.CTRL_DERIVED


# ---- exactness within the kernels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, N, T", [(1, 3, 3), (3, 3, 3), (65, 3, 3), (257, 3, 3), (4096, 1, 1), (3, 70, 1), (3, 70, 3)])
def test_sample_exact_properties(sim, K, N, T):
    S.check_sample_exact(kernel_sample(sim), K=K, N=N, T=T)


@pytest.mark.parametrize("K", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("name", S.COST_NAMES)
def test_blend_exact_properties(sim, name, K):
    S.check_blend_exact(kernel_blend(sim), kernel_select_cost(sim), name, K, factor=S.KERNEL_FACTOR)


def test_many_small_problems_and_the_largest_k(sim):
    """N = 70 at K = 3 against N = 3 inside it; K = 4096: the weights sum to 1 and the best one is the largest"""
    blend, cost = kernel_blend(sim), CS.COSTS["cube-ee"]
    c = S.blend_case(3, 70, 3)
    lam, _ = S.case_reference("cube-ee", 3, 70, 3)
    full = blend(cost, c["qpos"], c["qvel"], c["u"], None, lam)
    sl = slice(64, 67)
    sub = blend(cost, c["qpos"][:, sl], c["qvel"][:, sl], c["u"][:, sl], None, lam)
    for k in ("cost", "weight", "best", "best_cost", "ess", "u_first"):
        assert bits(sub[k]) == bits(full[k][sl]), k
    assert bits(sub["u_plan"]) == bits(full["u_plan"][:, sl])
    c = S.blend_case(4096, 1, 1)
    lam, _ = S.case_reference("traj-l2", 4096, 1, 1)
    got = blend(CS.COSTS["traj-l2"], c["qpos"], c["qvel"], c["u"], c["traj"], lam)
    w = got["weight"].astype(np.float64)
    assert abs(w.sum() - 1.0) <= S.sum_bound(factor=S.KERNEL_FACTOR) and w[0, got["best"][0]] == w.max() and got["best"][0] == np.argmin(got["cost"][0])


# ---- the C ABI itself: each output alone, the copies trajectory() does not make, graph replay ---------------------------------------------------------------
BLEND_OUT = {"cost_dev": (lambda T, n, K: n*K, torch.float32), "best_dev": (lambda T, n, K: n, torch.int32), "best_cost_dev": (lambda T, n, K: n, torch.float32),
             "weight_dev": (lambda T, n, K: n*K, torch.float32), "ess_dev": (lambda T, n, K: n, torch.float32), "u_plan_dev": (lambda T, n, K: T*6*n, torch.float32),
             "u_first_dev": (lambda T, n, K: 6*n, torch.float32)}
SAMPLE_OUT = {"ctrl_dev": lambda T, n, K: T*6*n*K, "qpos_rep_dev": lambda T, n, K: 13*n*K, "qvel_rep_dev": lambda T, n, K: 12*n*K}


def cost_struct(cost):
    from so100_mujoco_rl_amd import lib
    six = lambda w: (C.c_float*6)(*w)
    off = None if cost["offset"] is None else (C.c_float*3)(*cost["offset"])
    d = lib.CostDef(cost["link"], C.cast(off, C.c_void_p) if off is not None else None, CS.TARGETS[cost["target_mode"]], cost["w_point"], six(cost["w_q"]),
                    six(cost["q_nom"]), six(cost["w_v"]), six(cost["w_u"]), cost["w_terminal"])
    return d, off


def raw_blend(sim, name, K, n, T, want, shift=1, tail=1):
    """so100_query_cost_blend with the outputs of `want` alone into SENTINEL-filled buffers; one rollout failed, problem 0 failed throughout"""
    from so100_mujoco_rl_amd import lib
    cost = CS.COSTS[name]
    c = S.blend_case(K, n, T)
    qpos, qvel, u, tg = S.blend_args(c, cost["target_mode"])
    cols = lambda a: dev(a, sim).permute(0, 3, 1, 2).reshape(T, a.shape[-1], n*K).contiguous()
    soa = lambda a: None if a is None else dev(a, sim).transpose(-1, -2).contiguous()
    bad = np.full((n, K), -1, np.int32); bad[0] = 0; bad[n - 1, K//2] = 1
    keep = [cols(qpos), cols(qvel), cols(u), soa(tg), cost_struct(cost), dev(bad.reshape(-1), sim, np.int32), soa(c["fallback"])]
    out = {k: torch.full((size(T, n, K),), SENTINEL, dtype=dt, device=sim.device) for k, (size, dt) in BLEND_OUT.items()}
    io = lib.CostBlendIO(cost=C.pointer(keep[4][0]), target_dev=None if keep[3] is None else keep[3].data_ptr(), T=T, K=K, qpos_traj_dev=keep[0].data_ptr(),
                         qvel_traj_dev=keep[1].data_ptr(), u_traj_dev=keep[2].data_ptr(), bad_step_dev=keep[5].data_ptr(), u_fallback_dev=keep[6].data_ptr(),
                         temperature=S.case_reference(name, K, n, T)[0], shift=shift, tail=tail, **{k: out[k].data_ptr() for k in want})
    assert sim.L.so100_query_cost_blend(sim.h, C.byref(io), n, sim._stream()) == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def raw_sample(sim, K, n, T, want):
    from so100_mujoco_rl_amd import lib
    c = S.sample_case(n, T)
    soa = lambda a: dev(a, sim).transpose(-1, -2).contiguous()
    keep = [soa(c["plan"]), soa(c["qpos"]), soa(c["qvel"])]
    out = {k: torch.full((size(T, n, K),), SENTINEL, device=sim.device) for k, size in SAMPLE_OUT.items()}
    io = lib.PlanSampleIO(plan_dev=keep[0].data_ptr(), sigma=(C.c_float*6)(*S.SIGMA), u_lo=-1.0, u_hi=1.0, K=K, T=T, seed=S.SEED, draw=S.DRAW, id_offset=S.ID_OFFSET,
                          qpos_dev=keep[1].data_ptr(), qvel_dev=keep[2].data_ptr(), **{k: out[k].data_ptr() for k in want})
    assert sim.L.so100_query_plan_sample(sim.h, C.byref(io), n, sim._stream()) == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("K", [3, 257])
def test_each_output_alone(sim, K):
    before = state_words(sim)
    full = raw_blend(sim, "traj-l2", K, 3, 3, list(BLEND_OUT))
    assert int(full["best_dev"][0]) == -1 and not (full["u_plan_dev"] == SENTINEL).any()
    for k in BLEND_OUT:
        one = raw_blend(sim, "traj-l2", K, 3, 3, [k])
        for k2 in BLEND_OUT:
            assert bits(one[k2]) == bits(full[k2]) if k2 == k else bool((one[k2] == SENTINEL).all()), (k, k2)
    full = raw_sample(sim, K, 3, 3, list(SAMPLE_OUT))
    for k in SAMPLE_OUT:
        one = raw_sample(sim, K, 3, 3, [k])
        for k2 in SAMPLE_OUT:
            assert bits(one[k2]) == bits(full[k2]) if k2 == k else bool((one[k2] == SENTINEL).all()), (k, k2)
    assert (state_words(sim) == before).all()                     # the handle's state is never read or written


def planning_step(sim, plan, q0, v0, K, draw):
    """plan_sample -> trajectory -> cost_blend on the current stream, every output passed straight on"""
    cand = sim.plan_sample(plan, K, S.SIGMA, seed=S.SEED, draw=draw, qpos=q0, qvel=v0)
    roll = sim.trajectory(cand["ctrl"], cand["qpos"], cand["qvel"], mode="actions", nsub=TS.FREE_NSUB, flags=scenes.FREE)
    out = sim.cost_blend(roll["qpos"], roll["qvel"], cand["ctrl"], K, temperature=0.05, bad_step=roll["bad_step"], u_fallback=plan, shift=1, tail="zero",
                         target_mode="cube", w_u=1e-3)
    return cand, roll, out


def free_starts(sim, n=3):
    c = TS.free_case("arm", "actions")
    return dev(c["qpos"][:n], sim), dev(c["qvel"][:n], sim)


class Spy:
    """records the io struct each named query entry is called with, for the span of a `with`"""
    def __init__(self, sim, *names):
        self.L, self.names, self.seen, self.real = sim.L, names, {}, {}

    def __enter__(self):
        for name in self.names:
            self.real[name] = real = getattr(self.L, name)
            setattr(self.L, name, lambda h, ref, m, st, name=name, real=real: (self.seen.__setitem__(name, ref._obj), real(h, ref, m, st))[1])
        return self.seen

    def __exit__(self, *exc):
        for name, real in self.real.items():
            setattr(self.L, name, real)


def test_trajectory_copies_nothing(sim):
    """the pointers the ABI entries are called with: trajectory() reads plan_sample()'s three buffers, cost_blend() reads trajectory()'s rows and the
    sampler's ctrl, the next plan_sample() reads cost_blend()'s u_plan -- no copy anywhere in the chain"""
    q0, v0 = free_starts(sim)
    plan = torch.zeros(4, 3, 6, device=sim.device)
    with Spy(sim, "so100_query_plan_sample", "so100_query_trajectory", "so100_query_cost_blend") as seen:
        cand = sim.plan_sample(plan, 64, S.SIGMA, qpos=q0, qvel=v0)
        assert tuple(cand["ctrl"].shape) == (4, 3*64, 6) and tuple(cand["qpos"].shape) == (3*64, 13) and tuple(cand["qvel"].shape) == (3*64, 12)
        sample_io = seen["so100_query_plan_sample"]
        assert (sample_io.ctrl_dev, sample_io.qpos_rep_dev, sample_io.qvel_rep_dev) == (cand["ctrl"].data_ptr(), cand["qpos"].data_ptr(), cand["qvel"].data_ptr())
        roll = sim.trajectory(cand["ctrl"], cand["qpos"], cand["qvel"], mode="actions", nsub=TS.FREE_NSUB, flags=scenes.FREE)
        traj_io = seen["so100_query_trajectory"]
        assert (traj_io.ctrl_dev, traj_io.qpos_dev, traj_io.qvel_dev) == (sample_io.ctrl_dev, sample_io.qpos_rep_dev, sample_io.qvel_rep_dev)
        out = sim.cost_blend(roll["qpos"], roll["qvel"], cand["ctrl"], 64, temperature=0.05, target_mode="cube", shift=1)
        blend_io = seen["so100_query_cost_blend"]
        assert (blend_io.qpos_traj_dev, blend_io.qvel_traj_dev, blend_io.u_traj_dev) == (traj_io.qpos_traj_dev, traj_io.qvel_traj_dev, sample_io.ctrl_dev)
        sim.plan_sample(out["u_plan"], 64, S.SIGMA)
        assert seen["so100_query_plan_sample"].plan_dev == blend_io.u_plan_dev
    assert sim.L.so100_query_trajectory.argtypes is not None        # the entries are back


def test_a_graph_replay_of_the_planning_step_gives_the_same_bits(sim):
    """a linear chain on one stream: no parallel branches"""
    before = state_words(sim)
    q0, v0 = free_starts(sim)
    plan = (0.3*torch.rand(4, 3, 6, generator=torch.Generator().manual_seed(5)) - 0.15).to(sim.device)
    eager = planning_step(sim, plan, q0, v0, 64, 2)
    torch.cuda.synchronize()
    want = [eager[0]["ctrl"].clone(), eager[1]["qpos"].clone(), eager[2]["weight"].clone(), eager[2]["u_plan"].clone(), eager[2]["u_first"].clone(), eager[2]["ess"].clone()]
    side = torch.cuda.Stream(device=sim.device)
    side.wait_stream(torch.cuda.current_stream(sim.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap = planning_step(sim, plan, q0, v0, 64, 2)
    torch.cuda.current_stream(sim.device).wait_stream(side)
    held = [cap[0]["ctrl"], cap[1]["qpos"], cap[2]["weight"], cap[2]["u_plan"], cap[2]["u_first"], cap[2]["ess"]]
    for v in held:
        v.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(held, want):
        assert bits(a.contiguous().cpu().numpy()) == bits(b.contiguous().cpu().numpy())
    assert (state_words(sim) == before).all()


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(sim):
    """exact code and message of every check, in the header's order; a rejected call enqueues nothing and the handle goes on working"""
    from so100_mujoco_rl_amd import lib
    L, h, st = sim.L, sim.h, sim._stream()
    K, T = 4, 2
    buf = torch.full((7, T*6*N*K), SENTINEL, dtype=torch.float32, device=sim.device)
    inp = torch.zeros(13*T, N*K, dtype=torch.float32, device=sim.device)
    inp[9::13] = 1.0
    p, o = inp.data_ptr(), [buf[i].data_ptr() for i in range(7)]
    six = lambda *w: (C.c_float*6)(*(w if len(w) == 6 else w*6))
    nan, inf = float("nan"), float("inf")
    current = torch.cuda.current_device()
    big = (2**31 - 1)//4096 + 1

    def run(fn, calls):
        for f, msg in calls:
            assert f() == -1, msg
            assert L.so100_last_error() == fn + msg
            assert torch.cuda.current_device() == current
        torch.cuda.synchronize()
        assert (buf == SENTINEL).all()                            # nothing was enqueued

    # plan_sample
    ok = dict(plan_dev=p, sigma=six(0.5), u_lo=-1.0, u_hi=1.0, K=K, T=T, seed=1, draw=0, id_offset=0, qpos_dev=p, qvel_dev=p, ctrl_dev=o[0], qpos_rep_dev=o[1], qvel_rep_dev=o[2])
    call = lambda n=N, **over: (lambda: L.so100_query_plan_sample(h, C.byref(lib.PlanSampleIO(**{**ok, **over})), n, st))
    kmsg = lambda k, n=N: b"K must be in 1..4096 and N * K <= 2147483647, got K = %d, N = %d" % (k, n)
    smsg, umsg = b"sigma must be finite and >= 0", b"u_lo and u_hi must be finite and u_lo <= u_hi"
    rmsg = b"qpos_rep_dev needs qpos_dev and qvel_rep_dev needs qvel_dev"
    none = dict(ctrl_dev=None, qpos_rep_dev=None, qvel_rep_dev=None)
    run(b"so100_query_plan_sample: ", [
        (lambda: L.so100_query_plan_sample(h, None, N, st), b"null argument"), (call(0), b"M must be >= 1, got 0"),
        (call(T=0), b"T must be in 1..4096, got 0"), (call(T=4097), b"T must be in 1..4096, got 4097"),
        (call(K=0), kmsg(0)), (call(K=4097), kmsg(4097)), (call(big, K=4096), kmsg(4096, big)),
        (call(sigma=six(0.1, 0.1, -0.1, 0.1, 0.1, 0.1)), smsg), (call(sigma=six(0.1, 0.1, 0.1, 0.1, 0.1, nan)), smsg), (call(sigma=six(inf)), smsg),
        (call(u_lo=nan), umsg), (call(u_hi=inf), umsg), (call(u_lo=0.5, u_hi=0.25), umsg),
        (call(plan_dev=None), b"plan_dev is required"),
        (call(qpos_dev=None, qpos_rep_dev=None), b"qvel_dev needs qpos_dev"),
        (call(qpos_dev=None, qvel_dev=None, qvel_rep_dev=None), rmsg), (call(qvel_dev=None), rmsg),
        (call(**none), b"no output requested"),
        # the order: the first of several
        (call(0, T=0, K=0), b"M must be >= 1, got 0"), (call(T=0, K=0, sigma=six(-1.0)), b"T must be in 1..4096, got 0"), (call(K=0, sigma=six(-1.0)), kmsg(0)),
        (call(sigma=six(-1.0), u_lo=nan, plan_dev=None), smsg), (call(u_lo=nan, plan_dev=None), umsg), (call(plan_dev=None, qpos_dev=None, **none), b"plan_dev is required"),
        (call(qpos_dev=None, **none), b"qvel_dev needs qpos_dev"), (call(qpos_dev=None, qvel_dev=None, ctrl_dev=None), rmsg),
    ])
    # accepted: the limits' edges, no start states, an empty interval
    assert call(qpos_dev=None, qvel_dev=None, qpos_rep_dev=None, qvel_rep_dev=None, u_lo=0.25, u_hi=0.25, sigma=six(0.0))() == 0
    torch.cuda.synchronize()
    assert (buf[0][:T*6*N*K] == 0.25).all() and (buf[1:] == SENTINEL).all()
    buf.fill_(SENTINEL)

    # cost_blend
    good = dict(link=4, offset=None, target_mode=0, w_point=1.0, w_q=six(0.1), q_nom=six(0.0), w_v=six(0.0), w_u=six(0.01), w_terminal=1.0)
    keep = []

    def cdef(**over):
        keep.append(lib.CostDef(**{**good, **over}))
        return C.pointer(keep[-1])
    wmsg = b"w_point, w_q, w_v, w_u and w_terminal must be finite and >= 0 and q_nom finite"
    req = b"qpos_traj_dev, u_traj_dev and (unless the target is the cube) target_dev are required"
    tmsg = b"temperature must be finite and > 0"
    ok = dict(target_dev=p, T=T, K=K, qpos_traj_dev=p, qvel_traj_dev=p, u_traj_dev=p, bad_step_dev=None, u_fallback_dev=None, temperature=0.5, shift=1, tail=1,
              cost_dev=o[0], best_dev=o[1], best_cost_dev=o[2], weight_dev=o[3], ess_dev=o[4], u_plan_dev=o[5], u_first_dev=o[6])
    none = {k: None for k in BLEND_OUT}
    call = lambda n=N, **over: (lambda: L.so100_query_cost_blend(h, C.byref(lib.CostBlendIO(**{"cost": cdef(), **ok, **over})), n, st))
    bad_off = (C.c_float*3)(0.0, nan, 0.0)
    run(b"so100_query_cost_blend: ", [
        (lambda: L.so100_query_cost_blend(h, None, N, st), b"null argument"), (call(0), b"M must be >= 1, got 0"),
        (call(T=0), b"T must be in 1..4096, got 0"), (call(T=4097), b"T must be in 1..4096, got 4097"),
        (call(K=0), kmsg(0)), (call(K=4097), kmsg(4097)), (call(big, K=4096), kmsg(4096, big)),
        (call(cost=None), b"cost is required"), (call(cost=cdef(link=6)), b"link must be in 0..5, got 6"),
        (call(cost=cdef(offset=C.cast(bad_off, C.c_void_p))), b"offset must be finite"), (call(cost=cdef(target_mode=3)), b"unknown target_mode 3"),
        (call(cost=cdef(w_point=-1.0)), wmsg), (call(cost=cdef(w_u=six(inf))), wmsg), (call(cost=cdef(q_nom=six(0.0, nan, 0.0, 0.0, 0.0, 0.0))), wmsg),
        (call(temperature=0.0), tmsg), (call(temperature=-1.0), tmsg), (call(temperature=nan), tmsg), (call(temperature=inf), tmsg),
        (call(shift=2), b"shift must be 0 or 1, got 2"), (call(shift=-1), b"shift must be 0 or 1, got -1"), (call(tail=2), b"unknown tail 2"),
        (call(qpos_traj_dev=None), req), (call(u_traj_dev=None), req), (call(target_dev=None), req), (call(target_dev=None, cost=cdef(target_mode=1)), req),
        (call(**none), b"no output requested"),
        # the order: the first of several
        (call(0, T=0, K=0, cost=None), b"M must be >= 1, got 0"), (call(T=0, K=0, cost=None), b"T must be in 1..4096, got 0"), (call(K=0, cost=None), kmsg(0)),
        (call(cost=cdef(w_point=-1.0), temperature=0.0, shift=2), wmsg), (call(temperature=0.0, shift=2, tail=2), tmsg), (call(shift=2, tail=2, qpos_traj_dev=None), b"shift must be 0 or 1, got 2"),
        (call(tail=2, qpos_traj_dev=None), b"unknown tail 2"), (call(qpos_traj_dev=None, **none), req),
    ])
    # accepted: the cube target needs no target_dev, velocities are optional
    assert call(target_dev=None, qvel_traj_dev=None, cost=cdef(target_mode=2))() == 0
    torch.cuda.synchronize()
    assert not (buf[:, :N] == SENTINEL).any()
    z = lambda *s: torch.zeros(*s, device=sim.device)
    for bad_call in (lambda: sim.plan_sample(z(2, N, 6), 0, 0.5), lambda: sim.plan_sample(z(2, N, 6), 4097, 0.5), lambda: sim.plan_sample(z(2, N, 5), 4, 0.5),
                     lambda: sim.plan_sample(z(2, N, 6), 4, 0.5, qvel=z(N, 12)), lambda: sim.plan_sample(z(2, N, 6), 4, -0.5),
                     lambda: sim.cost_blend(z(2, N*4, 13), None, z(2, N*4, 6), 3, temperature=1.0), lambda: sim.cost_blend(z(2, N*4, 13), None, z(2, N*4, 6), 4, temperature=0.0),
                     lambda: sim.cost_blend(z(2, N*4, 13), None, z(2, N*4, 6), 4, temperature=1.0, tail="keep")):
        with pytest.raises(lib.So100Error):
            bad_call()


# ---- the three queries chained on the device --------------------------------------------------------------------------------------------------------------------
def test_the_planning_step_chained_on_the_device(sim):
    """3 contact-free starts, F_CUBE_PINNED, K = 64, T = 4, actions: plan_sample's ctrl through trajectory(); cost_blend's cost, weight and u_plan against the same
    quantities in torch fp64 from trajectory()'s own output with the header's cost formula"""
    q0, v0 = free_starts(sim)
    K, T, lam, w_u = 64, 4, 0.05, 1e-3
    plan = (0.3*torch.rand(T, 3, 6, generator=torch.Generator().manual_seed(7)) - 0.15).to(sim.device)
    cand, roll, out = planning_step(sim, plan, q0, v0, K, 0)
    assert (roll["bad_step"] == -1).all()
    u = cand["ctrl"].double()
    J = ((roll["ee"].double() - roll["qpos"][:, :, 6:9].double()).square().sum(-1) + w_u*u.square().sum(-1)).sum(0).reshape(3, K)
    w = torch.softmax(-(J - J.min(dim=1, keepdim=True).values)/float(np.float32(lam)), dim=1)
    blend = (w[None, :, :, None]*u.reshape(T, 3, K, 6)).sum(2)
    shifted = torch.cat([blend[1:], torch.zeros_like(blend[:1])])
    d = {"cost": float((out["cost"].double() - J).abs().max()), "weight": float((out["weight"].double() - w).abs().max()),
         "u_plan": float((out["u_plan"].double() - shifted).abs().max()), "u_first": float((out["u_first"].double() - blend[0]).abs().max()),
         "ess": float((out["ess"].double() - 1.0/w.square().sum(1)).abs().max())}
    show("chained vs torch fp64 on the device's rollouts", d)
    print(f"[mppi-tol] gpu chained: ess {out['ess'].cpu().numpy()}, best {out['best'].cpu().numpy()}")
    within(d)
    picked = J.gather(1, out["best"].long()[:, None])[:, 0]
    assert float((picked - J.min(dim=1).values).max()) <= 2*S.KERNEL_FACTOR*S.FP32_MEASURED["cost"]
    assert bits(out["best_cost"].cpu().numpy()) == bits(out["cost"].gather(1, out["best"].long()[:, None])[:, 0].cpu().numpy())


# ---- the example -------------------------------------------------------------------------------------------------------------------------------------------------
def test_mppi_reach_with_the_queries():
    """examples/mppi_reach.py --plan query on 8 envs x 64 samples x T = 8, 40 steps: the final mean |cube - ee| is below the zero-action baseline's on the same
    starts; printed next to the torch path's 0.2662 m (a record: the noise and the cost differ, the two are not expected to be equal).
    Measured on an MI355X: see mppi_support.MEASURED."""
    from so100_mujoco_rl_amd import lib
    spec = importlib.util.spec_from_file_location("mppi_reach", os.path.join(ROOT, "examples", "mppi_reach.py"))
    mppi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mppi)
    result = {}
    for name, policy in (("query", mppi.Mppi(64, 8, plan="query")), ("zero", mppi.zero_action)):
        s = lib.So100Sim(lib.ENV01, 8, flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
        result[name] = mppi.run(s, 40, policy)
        s.close()
    print(f"[mppi-tol] MPPI reach --plan query, 8 envs x 64 samples x T = 8, 40 steps: mean |cube - ee| {result['query'][0]:.4f} m at reset -> {result['query'][1]:.4f} m "
          f"(zero action: {result['zero'][1]:.4f} m; --plan torch: 0.2662 m)")
    assert result["query"][0] == result["zero"][0] and result["query"][1] < result["zero"][1]
