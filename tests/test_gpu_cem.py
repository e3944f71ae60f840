"""The two cross-entropy planner queries on the GPU (include/so100_query.h: so100_query_plan_sample_tv, so100_query_cost_refit), through the C ABI and
So100Sim.plan_sample_tv / cost_refit: the cases of tests/test_cem_cpu.py on the kernels, under the bounds fixed there (tests/cem_support.py: 3 x the fp32
twin's recorded deviation from the numpy reference), the exact properties within the kernels, plus what only the device can show: each output alone, graph
replay of the three-call round, the handle's state, the pointers handed on uncopied, every argument error, two rounds chained on physics and
examples/cem_reach.py end to end.

Shapes (cem_support.SHAPES): K in {1, 3, 63, 64, 65, 256, 257, 1030} -- below the sort's smallest table, a full one, one over (a table of 128 keys, half of
them padding), a full workgroup, one over, a table of 2048 with a ragged tail -- x N in {1, 3} x T in {1, 3}, K = 4096 once, N = 70 at K = 3; for each, E in
{1, 2, ceil(K / 8), K - 1, K}.  No physics but where trajectory() is called: every other case is seeded arrays, a launch or two each."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cem_support as S                                   # noqa: E402
import cost_support as CS                                 # noqa: E402
import mppi_support as MS                                 # noqa: E402
import scenes                                             # noqa: E402
import test_gpu_mppi as GM                                # noqa: E402
import trajectory_support as TS                           # noqa: E402
from test_gpu_mppi import sim                             # noqa: E402, F401  (the fixture: N = 5, Env01, the reference physics, after three random steps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = GM.N
SENTINEL = GM.SENTINEL
bits = S.bits
dev = GM.dev
_held = {}


def held(a, sim, shape):
    """the device copy of a cached case array in the queries' row layout [T, N K, w], uploaded once"""
    if a is None:
        return None
    key = (id(a), str(sim.device))
    if key not in _held or _held[key][0] is not a:
        _held[key] = (a, dev(a, sim).reshape(shape))
    return _held[key][1]


def kernel_sample(sim):
    """So100Sim.plan_sample_tv behind cem_support's `sample` signature"""
    def f(plan, K, sigma, seed=0, draw=0, id_offset=0, u_lo=-1.0, u_hi=1.0, qpos=None, qvel=None):
        res = sim.plan_sample_tv(dev(plan, sim), K, dev(sigma, sim), seed=seed, draw=draw, id_offset=id_offset, u_lo=u_lo, u_hi=u_hi, qpos=dev(qpos, sim), qvel=dev(qvel, sim))
        n = plan.shape[1]
        out = {"ctrl": res["ctrl"].contiguous().cpu().numpy().reshape(plan.shape[0], n, K, 6)}
        for k, w in (("qpos", 13), ("qvel", 12)):
            if k in res:
                out[k] = res[k].contiguous().cpu().numpy().reshape(n, K, w)
        return out
    return f


def kernel_refit(sim):
    def f(cost, qpos, qvel, u, target, E, alpha=0.0, plan=None, sigma=None, sigma_min=0.0, sigma_max=1.0, sigma_init=0.5, bad_step=None, u_fallback=None, shift=0,
          tail="zero"):
        T, n, K = u.shape[:3]
        cols = lambda a: held(a, sim, (T, n*K, a.shape[-1])) if a is not None else None
        res = sim.cost_refit(cols(qpos), cols(qvel), cols(u), K, E, alpha=alpha, plan=dev(plan, sim), sigma=dev(sigma, sim), sigma_min=sigma_min, sigma_max=sigma_max,
                             sigma_init=sigma_init, bad_step=dev(bad_step, sim, np.int32), u_fallback=dev(u_fallback, sim), shift=shift, tail=tail, target=dev(target, sim),
                             **cost)
        return {k: v.contiguous().cpu().numpy() for k, v in res.items()}
    return f


def show(tag, d):
    print(f"[cem-tol] gpu {tag}: " + " ".join(f"{k} {v:.3e}" + (f" (bound {S.KERNEL_FACTOR*S.FP32_MEASURED[k]:.2e})" if k in S.FP32_MEASURED else "") for k, v in d.items()))


def within(d):
    for k, v in S.FP32_MEASURED.items():
        if k in d:
            assert d[k] <= S.KERNEL_FACTOR*v, (k, d[k], S.KERNEL_FACTOR*v)


# ---- against the reference -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.COST_NAMES)
def test_refit_against_the_reference(sim, name):
    d = S.refit_deviations(kernel_refit(sim), names=(name,), factor=S.KERNEL_FACTOR)
    _held.clear()
    show(f"refit, every shape x E x alpha, {name}", d)
    within(d)


def test_sample_against_the_reference(sim):
    """a broadcast sigma is so100_query_plan_sample to the bit at every shape; a sigma per entry stays within the derived bound"""
    d = {"ctrl": S.sample_deviation(kernel_sample(sim), GM.kernel_sample(sim))}
    show("sample, every shape", d)
    print(f"[cem-tol] gpu ctrl: the derived bound max(sigma) x NOISE_EPS + 1 ulp = {S.CTRL_DERIVED:.3e}")
    within(d)
    assert d["ctrl"] <= S.CTRL_DERIVED


# ---- exactness within the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, N, T", [(1, 3, 3), (65, 3, 3), (257, 3, 1), (3, 70, 3)])
def test_sample_exact_properties(sim, K, N, T):
    S.check_sample_exact(kernel_sample(sim), K=K, N=N, T=T)


@pytest.mark.parametrize("K", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("name", S.COST_NAMES)
def test_refit_exact_properties(sim, name, K):
    S.check_refit_exact(kernel_refit(sim), GM.kernel_blend(sim), name, K)
    _held.clear()


def test_many_small_problems_and_the_largest_k(sim):
    """N = 70 at K = 3 against N = 3 inside it; K = 4096 with E = K, one rollout failed: 4095 elites, the failed one last and left out"""
    refit, cost = kernel_refit(sim), CS.COSTS["cube-ee"]
    c, old = MS.blend_case(3, 70, 3), S.old_case(70, 3)
    sl = slice(64, 67)
    kw = lambda s: dict(alpha=0.25, plan=old["plan"][:, s], sigma=old["sigma"][:, s], shift=1, tail="hold", **S.LIMITS)
    full = refit(cost, c["qpos"], c["qvel"], c["u"], None, 2, **kw(slice(None)))
    sub = refit(cost, np.ascontiguousarray(c["qpos"][:, sl]), np.ascontiguousarray(c["qvel"][:, sl]), np.ascontiguousarray(c["u"][:, sl]), None, 2, **kw(sl))
    for k in S.OUTPUTS:
        assert bits(sub[k]) == bits(full[k][sl] if k in S.PER_PROBLEM else full[k][:, sl]), k
    c = MS.blend_case(4096, 1, 1)
    bad = np.full((1, 4096), -1, np.int32); bad[0, 1234] = 0
    got = refit(CS.COSTS["traj-l2"], c["qpos"], c["qvel"], c["u"], c["traj"], 4096, bad_step=bad, **S.LIMITS)
    S.check_elites(got, got["cost"].astype(np.float64), 4096, 0.0)
    assert got["n_elite"][0] == 4095 and got["elite"][0, -1] == -1 and 1234 not in got["elite"][0] and sorted(got["elite"][0, :-1]) == [k for k in range(4096) if k != 1234]
    _held.clear()


# ---- the C ABI itself: each output alone, graph replay, the pointers ---------------------------------------------------------------------------------------
REFIT_OUT = {"cost_dev": (lambda T, n, K, E: n*K, torch.float32), "best_dev": (lambda T, n, K, E: n, torch.int32), "best_cost_dev": (lambda T, n, K, E: n, torch.float32),
             "elite_dev": (lambda T, n, K, E: n*E, torch.int32), "n_elite_dev": (lambda T, n, K, E: n, torch.int32), "threshold_dev": (lambda T, n, K, E: n, torch.float32),
             "mean_dev": (lambda T, n, K, E: T*6*n, torch.float32), "sigma_out_dev": (lambda T, n, K, E: T*6*n, torch.float32),
             "u_first_dev": (lambda T, n, K, E: 6*n, torch.float32)}
SAMPLE_OUT = GM.SAMPLE_OUT


def raw_refit(sim, name, K, E, n, T, want, shift=1, tail=1):
    """so100_query_cost_refit with the outputs of `want` alone into SENTINEL-filled buffers; one rollout failed, problem 0 failed throughout"""
    from so100_mujoco_rl_amd import lib
    cost = CS.COSTS[name]
    c, old = MS.blend_case(K, n, T), S.old_case(n, T)
    qpos, qvel, u, tg = MS.blend_args(c, cost["target_mode"])
    cols = lambda a: dev(a, sim).permute(0, 3, 1, 2).reshape(T, a.shape[-1], n*K).contiguous()
    soa = lambda a: None if a is None else dev(a, sim).transpose(-1, -2).contiguous()
    bad = np.full((n, K), -1, np.int32); bad[0] = 0; bad[n - 1, K//2] = 1
    keep = [cols(qpos), cols(qvel), cols(u), soa(tg), GM.cost_struct(cost), dev(bad.reshape(-1), sim, np.int32), soa(c["fallback"]), soa(old["plan"]), soa(old["sigma"])]
    out = {k: torch.full((size(T, n, K, E),), SENTINEL, dtype=dt, device=sim.device) for k, (size, dt) in REFIT_OUT.items()}
    six = lambda w: (C.c_float*6)(*w)
    io = lib.CostRefitIO(cost=C.pointer(keep[4][0]), target_dev=None if keep[3] is None else keep[3].data_ptr(), T=T, K=K, qpos_traj_dev=keep[0].data_ptr(),
                         qvel_traj_dev=keep[1].data_ptr(), u_traj_dev=keep[2].data_ptr(), bad_step_dev=keep[5].data_ptr(), u_fallback_dev=keep[6].data_ptr(),
                         E=E, alpha=0.25, plan_dev=keep[7].data_ptr(), sigma_dev=keep[8].data_ptr(), sigma_min=six(S.SIGMA_MIN), sigma_max=six(S.SIGMA_MAX),
                         sigma_init=six(S.SIGMA_INIT), shift=shift, tail=tail, **{k: out[k].data_ptr() for k in want})
    assert sim.L.so100_query_cost_refit(sim.h, C.byref(io), n, sim._stream()) == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def raw_sample(sim, K, n, T, want):
    from so100_mujoco_rl_amd import lib
    c = MS.sample_case(n, T)
    soa = lambda a: dev(a, sim).transpose(-1, -2).contiguous()
    keep = [soa(c["plan"]), soa(c["qpos"]), soa(c["qvel"]), soa(S.entry_sigma(n, T))]
    out = {k: torch.full((size(T, n, K),), SENTINEL, device=sim.device) for k, size in SAMPLE_OUT.items()}
    io = lib.PlanSampleTvIO(plan_dev=keep[0].data_ptr(), sigma_dev=keep[3].data_ptr(), u_lo=-1.0, u_hi=1.0, K=K, T=T, seed=S.SEED, draw=S.DRAW, id_offset=S.ID_OFFSET,
                            qpos_dev=keep[1].data_ptr(), qvel_dev=keep[2].data_ptr(), **{k: out[k].data_ptr() for k in want})
    assert sim.L.so100_query_plan_sample_tv(sim.h, C.byref(io), n, sim._stream()) == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("K, E", [(3, 2), (257, 33)])
def test_each_output_alone(sim, K, E):
    before = GM.state_words(sim)
    full = raw_refit(sim, "traj-l2", K, E, 3, 3, list(REFIT_OUT))
    assert int(full["best_dev"][0]) == -1 and int(full["n_elite_dev"][0]) == 0 and not any((v == SENTINEL).any() for v in full.values())
    for k in REFIT_OUT:
        one = raw_refit(sim, "traj-l2", K, E, 3, 3, [k])
        for k2 in REFIT_OUT:
            assert bits(one[k2]) == bits(full[k2]) if k2 == k else bool((one[k2] == SENTINEL).all()), (k, k2)
    full = raw_sample(sim, K, 3, 3, list(SAMPLE_OUT))
    for k in SAMPLE_OUT:
        one = raw_sample(sim, K, 3, 3, [k])
        for k2 in SAMPLE_OUT:
            assert bits(one[k2]) == bits(full[k2]) if k2 == k else bool((one[k2] == SENTINEL).all()), (k, k2)
    assert (GM.state_words(sim) == before).all()                  # the handle's state is never read or written


def cem_round(sim, mean, sigma, q0, v0, K, E, draw, shift):
    """plan_sample_tv -> trajectory -> cost_refit on the current stream, every output passed straight on"""
    cand = sim.plan_sample_tv(mean, K, sigma, seed=S.SEED, draw=draw, qpos=q0, qvel=v0)
    roll = sim.trajectory(cand["ctrl"], cand["qpos"], cand["qvel"], mode="actions", nsub=TS.FREE_NSUB, flags=scenes.FREE)
    out = sim.cost_refit(roll["qpos"], roll["qvel"], cand["ctrl"], K, E, alpha=0.25, plan=mean, sigma=sigma, sigma_min=0.02, sigma_max=1.0, sigma_init=0.5,
                         bad_step=roll["bad_step"], u_fallback=mean, shift=shift, tail="zero", target_mode="cube", w_u=1e-3)
    return cand, roll, out


def start_plan(sim, T, seed):
    mean = (0.3*torch.rand(T, 3, 6, generator=torch.Generator().manual_seed(seed)) - 0.15).to(sim.device)
    return mean, torch.full((T, 3, 6), 0.5, device=sim.device)


def test_the_pointers_are_handed_on_uncopied(sim):
    """the pointers the ABI entries are called with: trajectory() reads plan_sample_tv()'s three buffers, cost_refit() reads trajectory()'s rows and the sampler's
    ctrl, the next plan_sample_tv() reads cost_refit()'s mean and sigma_out -- no copy anywhere in the chain"""
    q0, v0 = GM.free_starts(sim)
    mean, sigma = start_plan(sim, 4, 3)
    with GM.Spy(sim, "so100_query_plan_sample_tv", "so100_query_trajectory", "so100_query_cost_refit") as seen:
        cand, roll, out = cem_round(sim, mean, sigma, q0, v0, 64, 8, 0, 1)
        sample_io, traj_io, refit_io = seen["so100_query_plan_sample_tv"], seen["so100_query_trajectory"], seen["so100_query_cost_refit"]
        assert tuple(cand["ctrl"].shape) == (4, 3*64, 6) and tuple(out["mean"].shape) == (4, 3, 6) and tuple(out["sigma_out"].shape) == (4, 3, 6) and tuple(out["elite"].shape) == (3, 8)
        assert (sample_io.ctrl_dev, sample_io.qpos_rep_dev, sample_io.qvel_rep_dev) == (cand["ctrl"].data_ptr(), cand["qpos"].data_ptr(), cand["qvel"].data_ptr())
        assert (traj_io.ctrl_dev, traj_io.qpos_dev, traj_io.qvel_dev) == (sample_io.ctrl_dev, sample_io.qpos_rep_dev, sample_io.qvel_rep_dev)
        assert (refit_io.qpos_traj_dev, refit_io.qvel_traj_dev, refit_io.u_traj_dev) == (traj_io.qpos_traj_dev, traj_io.qvel_traj_dev, sample_io.ctrl_dev)
        assert (refit_io.mean_dev, refit_io.sigma_out_dev) == (out["mean"].data_ptr(), out["sigma_out"].data_ptr())
        sim.plan_sample_tv(out["mean"], 64, out["sigma_out"])
        assert (seen["so100_query_plan_sample_tv"].plan_dev, seen["so100_query_plan_sample_tv"].sigma_dev) == (refit_io.mean_dev, refit_io.sigma_out_dev)
    assert sim.L.so100_query_trajectory.argtypes is not None        # the entries are back


def test_a_graph_replay_of_the_round_gives_the_same_bits(sim):
    """a linear chain on one stream: no parallel branches"""
    before = GM.state_words(sim)
    q0, v0 = GM.free_starts(sim)
    mean, sigma = start_plan(sim, 4, 5)
    eager = cem_round(sim, mean, sigma, q0, v0, 64, 8, 2, 1)
    torch.cuda.synchronize()
    names = ("cost", "elite", "n_elite", "threshold", "mean", "sigma_out", "u_first")
    want = [eager[0]["ctrl"].clone(), eager[1]["qpos"].clone()] + [eager[2][k].clone() for k in names]
    side = torch.cuda.Stream(device=sim.device)
    side.wait_stream(torch.cuda.current_stream(sim.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap = cem_round(sim, mean, sigma, q0, v0, 64, 8, 2, 1)
    torch.cuda.current_stream(sim.device).wait_stream(side)
    held_out = [cap[0]["ctrl"], cap[1]["qpos"]] + [cap[2][k] for k in names]
    for v in held_out:
        v.fill_(-7 if v.dtype == torch.int32 else SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(held_out, want):
        assert bits(a.contiguous().cpu().numpy()) == bits(b.contiguous().cpu().numpy())
    assert (GM.state_words(sim) == before).all()


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(sim):
    """exact code and message of every check, in the header's order; a rejected call enqueues nothing and the handle goes on working"""
    from so100_mujoco_rl_amd import lib
    L, h, st = sim.L, sim.h, sim._stream()
    K, T = 4, 2
    buf = torch.full((9, T*6*N*K), SENTINEL, dtype=torch.float32, device=sim.device)
    inp = torch.zeros(13*T, N*K, dtype=torch.float32, device=sim.device)
    inp[9::13] = 1.0
    p, o = inp.data_ptr(), [buf[i].data_ptr() for i in range(9)]
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

    # plan_sample_tv: so100_query_plan_sample's list with the null sigma_dev where the sigma check stands
    ok = dict(plan_dev=p, sigma_dev=p, u_lo=-1.0, u_hi=1.0, K=K, T=T, seed=1, draw=0, id_offset=0, qpos_dev=p, qvel_dev=p, ctrl_dev=o[0], qpos_rep_dev=o[1], qvel_rep_dev=o[2])
    call = lambda n=N, **over: (lambda: L.so100_query_plan_sample_tv(h, C.byref(lib.PlanSampleTvIO(**{**ok, **over})), n, st))
    kmsg = lambda k, n=N: b"K must be in 1..4096 and N * K <= 2147483647, got K = %d, N = %d" % (k, n)
    smsg, umsg = b"sigma_dev is required", b"u_lo and u_hi must be finite and u_lo <= u_hi"
    rmsg = b"qpos_rep_dev needs qpos_dev and qvel_rep_dev needs qvel_dev"
    none = dict(ctrl_dev=None, qpos_rep_dev=None, qvel_rep_dev=None)
    run(b"so100_query_plan_sample_tv: ", [
        (lambda: L.so100_query_plan_sample_tv(h, None, N, st), b"null argument"), (call(0), b"M must be >= 1, got 0"),
        (call(T=0), b"T must be in 1..4096, got 0"), (call(T=4097), b"T must be in 1..4096, got 4097"),
        (call(K=0), kmsg(0)), (call(K=4097), kmsg(4097)), (call(big, K=4096), kmsg(4096, big)),
        (call(sigma_dev=None), smsg),
        (call(u_lo=nan), umsg), (call(u_hi=inf), umsg), (call(u_lo=0.5, u_hi=0.25), umsg),
        (call(plan_dev=None), b"plan_dev is required"),
        (call(qpos_dev=None, qpos_rep_dev=None), b"qvel_dev needs qpos_dev"),
        (call(qpos_dev=None, qvel_dev=None, qvel_rep_dev=None), rmsg), (call(qvel_dev=None), rmsg),
        (call(**none), b"no output requested"),
        # the order: the first of several
        (call(0, T=0, K=0), b"M must be >= 1, got 0"), (call(T=0, K=0, sigma_dev=None), b"T must be in 1..4096, got 0"), (call(K=0, sigma_dev=None), kmsg(0)),
        (call(sigma_dev=None, u_lo=nan, plan_dev=None), smsg), (call(u_lo=nan, plan_dev=None), umsg), (call(plan_dev=None, qpos_dev=None, **none), b"plan_dev is required"),
        (call(qpos_dev=None, **none), b"qvel_dev needs qpos_dev"), (call(qpos_dev=None, qvel_dev=None, ctrl_dev=None), rmsg),
    ])
    # accepted: no start states, an empty interval, a sigma of zeros
    assert call(qpos_dev=None, qvel_dev=None, qpos_rep_dev=None, qvel_rep_dev=None, u_lo=0.25, u_hi=0.25)() == 0
    torch.cuda.synchronize()
    assert (buf[0][:T*6*N*K] == 0.25).all() and (buf[1:] == SENTINEL).all()
    buf.fill_(SENTINEL)

    # cost_refit
    good = dict(link=4, offset=None, target_mode=0, w_point=1.0, w_q=six(0.1), q_nom=six(0.0), w_v=six(0.0), w_u=six(0.01), w_terminal=1.0)
    keep = []

    def cdef(**over):
        keep.append(lib.CostDef(**{**good, **over}))
        return C.pointer(keep[-1])
    wmsg = b"w_point, w_q, w_v, w_u and w_terminal must be finite and >= 0 and q_nom finite"
    req = b"qpos_traj_dev, u_traj_dev, (unless the target is the cube) target_dev and (with alpha > 0) plan_dev and sigma_dev are required"
    emsg = lambda e: b"E must be in 1..K, got E = %d, K = %d" % (e, K)
    amsg = b"alpha must be finite and in [0, 1)"
    gmsg = b"sigma_min, sigma_max and sigma_init must be finite, 0 <= sigma_min <= sigma_max and sigma_init >= 0"
    ok = dict(target_dev=p, T=T, K=K, qpos_traj_dev=p, qvel_traj_dev=p, u_traj_dev=p, bad_step_dev=None, u_fallback_dev=None, E=2, alpha=0.25, plan_dev=p, sigma_dev=p,
              sigma_min=six(0.0), sigma_max=six(1.0), sigma_init=six(0.5), shift=1, tail=1,
              cost_dev=o[0], best_dev=o[1], best_cost_dev=o[2], elite_dev=o[3], n_elite_dev=o[4], threshold_dev=o[5], mean_dev=o[6], sigma_out_dev=o[7], u_first_dev=o[8])
    none = {k: None for k in REFIT_OUT}
    call = lambda n=N, **over: (lambda: L.so100_query_cost_refit(h, C.byref(lib.CostRefitIO(**{"cost": cdef(), **ok, **over})), n, st))
    bad_off = (C.c_float*3)(0.0, nan, 0.0)
    run(b"so100_query_cost_refit: ", [
        (lambda: L.so100_query_cost_refit(h, None, N, st), b"null argument"), (call(0), b"M must be >= 1, got 0"),
        (call(T=0), b"T must be in 1..4096, got 0"), (call(T=4097), b"T must be in 1..4096, got 4097"),
        (call(K=0), kmsg(0)), (call(K=4097), kmsg(4097)), (call(big, K=4096), kmsg(4096, big)),
        (call(cost=None), b"cost is required"), (call(cost=cdef(link=6)), b"link must be in 0..5, got 6"),
        (call(cost=cdef(offset=C.cast(bad_off, C.c_void_p))), b"offset must be finite"), (call(cost=cdef(target_mode=3)), b"unknown target_mode 3"),
        (call(cost=cdef(w_point=-1.0)), wmsg), (call(cost=cdef(w_u=six(inf))), wmsg), (call(cost=cdef(q_nom=six(0.0, nan, 0.0, 0.0, 0.0, 0.0))), wmsg),
        (call(E=0), emsg(0)), (call(E=K + 1), emsg(K + 1)), (call(E=-3), emsg(-3)),
        (call(alpha=1.0), amsg), (call(alpha=-0.25), amsg), (call(alpha=nan), amsg), (call(alpha=inf), amsg),
        (call(sigma_min=six(-0.1)), gmsg), (call(sigma_min=six(0.0, 0.0, 2.0, 0.0, 0.0, 0.0)), gmsg), (call(sigma_max=six(1.0, 1.0, 1.0, 1.0, 1.0, inf)), gmsg),
        (call(sigma_min=six(nan)), gmsg), (call(sigma_init=six(0.5, -0.5, 0.5, 0.5, 0.5, 0.5)), gmsg), (call(sigma_init=six(nan)), gmsg),
        (call(shift=2), b"shift must be 0 or 1, got 2"), (call(shift=-1), b"shift must be 0 or 1, got -1"), (call(tail=2), b"unknown tail 2"),
        (call(qpos_traj_dev=None), req), (call(u_traj_dev=None), req), (call(target_dev=None), req), (call(target_dev=None, cost=cdef(target_mode=1)), req),
        (call(plan_dev=None), req), (call(sigma_dev=None), req),
        (call(**none), b"no output requested"),
        # the order: the first of several
        (call(0, T=0, K=0, cost=None), b"M must be >= 1, got 0"), (call(T=0, K=0, cost=None), b"T must be in 1..4096, got 0"), (call(K=0, cost=None, E=0), kmsg(0)),
        (call(cost=cdef(w_point=-1.0), E=0, alpha=1.0), wmsg), (call(E=0, alpha=1.0, sigma_min=six(-1.0)), emsg(0)), (call(alpha=1.0, sigma_min=six(-1.0), shift=2), amsg),
        (call(sigma_min=six(-1.0), shift=2, tail=2), gmsg), (call(shift=2, tail=2, qpos_traj_dev=None), b"shift must be 0 or 1, got 2"),
        (call(tail=2, qpos_traj_dev=None), b"unknown tail 2"), (call(plan_dev=None, **none), req),
    ])
    # accepted: the cube target needs no target_dev, velocities are optional, alpha = 0 needs neither plan nor sigma, sigma_min = sigma_max, E = K
    assert call(target_dev=None, qvel_traj_dev=None, cost=cdef(target_mode=2), alpha=0.0, plan_dev=None, sigma_dev=None, sigma_min=six(0.5), sigma_max=six(0.5), E=K)() == 0
    torch.cuda.synchronize()
    assert not (buf[:, :N] == SENTINEL).any()
    z = lambda *s: torch.zeros(*s, device=sim.device)
    lim = dict(sigma_min=0.0, sigma_max=1.0, sigma_init=0.5)
    for bad_call in (lambda: sim.plan_sample_tv(z(2, N, 6), 0, z(2, N, 6)), lambda: sim.plan_sample_tv(z(2, N, 6), 4, z(2, N, 5)), lambda: sim.plan_sample_tv(z(2, N, 6), 4, z(6)),
                     lambda: sim.plan_sample_tv(z(2, N, 6), 4, z(2, N, 6), qvel=z(N, 12)),
                     lambda: sim.cost_refit(z(2, N*4, 13), None, z(2, N*4, 6), 4, 5, **lim), lambda: sim.cost_refit(z(2, N*4, 13), None, z(2, N*4, 6), 4, 0, **lim),
                     lambda: sim.cost_refit(z(2, N*4, 13), None, z(2, N*4, 6), 4, 2, alpha=0.5, **lim), lambda: sim.cost_refit(z(2, N*4, 13), None, z(2, N*4, 6), 4, 2, tail="keep", **lim),
                     lambda: sim.cost_refit(z(2, N*4, 13), None, z(2, N*4, 6), 4, 2, sigma_min=2.0, sigma_max=1.0, sigma_init=0.5)):
        with pytest.raises(lib.So100Error):
            bad_call()


# ---- two rounds chained on the device ----------------------------------------------------------------------------------------------------------------------------
def test_two_rounds_chained_on_the_device(sim):
    """3 contact-free starts, F_CUBE_PINNED, K = 64, E = 8, T = 4, actions, two rounds (the second shifted): every bad_step is -1; the elites are held to torch
    fp64 costs from trajectory()'s own output with the header's cost formula, mean and sigma_out to torch fp64 statistics of the kernel's elites"""
    q0, v0 = GM.free_starts(sim)
    K, E, T, w_u, alpha = 64, 8, 4, 1e-3, 0.25
    mean, sigma = start_plan(sim, T, 7)
    worst = {"cost": 0.0, "mean": 0.0, "sigma_out": 0.0, "u_first": 0.0}
    for rnd in range(2):
        cand, roll, out = cem_round(sim, mean, sigma, q0, v0, K, E, rnd, rnd)
        assert (roll["bad_step"] == -1).all() and (out["n_elite"] == E).all()
        u = cand["ctrl"].double()
        J = ((roll["ee"].double() - roll["qpos"][:, :, 6:9].double()).square().sum(-1) + w_u*u.square().sum(-1)).sum(0).reshape(3, K)
        worst["cost"] = max(worst["cost"], float((out["cost"].double() - J).abs().max()))
        got = {k: v.contiguous().cpu().numpy() for k, v in out.items()}
        S.check_elites(got, J.cpu().numpy(), E, S.cost_bound(factor=S.KERNEL_FACTOR))
        ue = u.reshape(T, 3, K, 6).gather(2, out["elite"].long()[None, :, :, None].expand(T, 3, E, 6))
        mu, sd = ue.mean(2), ue.var(2, unbiased=False).sqrt()
        mean_new = alpha*mean.double() + (1 - alpha)*mu
        sigma_new = (alpha*sigma.double() + (1 - alpha)*sd).clamp(float(np.float32(0.02)), 1.0)
        if rnd:
            mean_ref = torch.cat([mean_new[1:], torch.zeros_like(mean_new[:1])])
            sigma_ref = torch.cat([sigma_new[1:], torch.full_like(sigma_new[:1], 0.5)])
        else:
            mean_ref, sigma_ref = mean_new, sigma_new
        for k, ref in (("mean", mean_ref), ("sigma_out", sigma_ref), ("u_first", mean_new[0])):
            worst[k] = max(worst[k], float((out[k].double() - ref).abs().max()))
        mean, sigma = out["mean"], out["sigma_out"]
    show("two rounds vs torch fp64 on the device's rollouts", worst)
    within(worst)


# ---- the example -------------------------------------------------------------------------------------------------------------------------------------------------
def test_cem_reach():
    """examples/cem_reach.py on 8 envs x 64 samples x T = 8, 40 steps (the MPPI example test's setting): the final mean |cube - ee| is below the zero-action
    baseline's on the same starts.  Measured on an MI355X: see cem_support.MEASURED."""
    from so100_mujoco_rl_amd import lib
    spec = importlib.util.spec_from_file_location("cem_reach", os.path.join(ROOT, "examples", "cem_reach.py"))
    cem = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cem)
    result = {}
    for name, policy in (("cem", cem.Cem(64, 8, 8)), ("zero", cem.zero_action)):
        s = lib.So100Sim(lib.ENV01, 8, flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
        result[name] = cem.run(s, 40, policy)
        s.close()
    print(f"[cem-tol] CEM reach, 8 envs x 64 samples (8 elites) x T = 8, 3 rounds, 40 steps: mean |cube - ee| {result['cem'][0]:.4f} m at reset -> {result['cem'][1]:.4f} m "
          f"(zero action: {result['zero'][1]:.4f} m)")
    assert result["cem"][0] == result["zero"][0] and result["cem"][1] < result["zero"][1]
