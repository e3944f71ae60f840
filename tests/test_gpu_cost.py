"""The two cost queries on the GPU (include/so100_query.h: so100_query_cost_terms, so100_query_cost_select), through the C ABI and So100Sim.cost_terms /
cost_select: the cases of tests/test_cost_cpu.py on the kernels, under the bounds fixed there (tests/cost_support.py: 3 x the fp32 twin's recorded
deviation from the numpy reference), the exact properties within the kernels, plus what only the device can show: each output alone, pointers
that are not 16-byte aligned, graph replay, the handle's state, every argument error, the six queries chained on the device and
examples/ilqr_reach.py --cost query end to end.

Shapes: terms M in {1, 3, 65, 130} (one problem; a partial block of 64; a full block and one problem of the next workgroup; two full blocks and two problems of a third),
T in {1, 3}, both nx, the three target modes, link 4 with its default point and link 2 with an offset; select L in {1, 3, 8, 16} (L = 3: 21 groups and an
idle lane per wave) x M in {1, 3, 65}, T = 3.  No physics: every case is seeded arrays, a launch or two each."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cost_support as S                                  # noqa: E402
import lqr_support as LS                                  # noqa: E402
import scenes                                             # noqa: E402
import trajectory_support as TS                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 65
SENTINEL = -777.0
bits = S.bits


@pytest.fixture(scope="module")
def sim():
    """N = 65, Env01, the reference physics, after three random steps (the cost queries never look at it)"""
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


def dev(a, sim, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(sim.device)


def kernel_terms(sim):
    """So100Sim.cost_terms behind cost_support's `terms` signature"""
    def f(cost, qpos, qvel, u, target, nx):
        return host(sim.cost_terms(dev(qpos, sim), dev(qvel, sim), dev(u, sim), nx=nx, target=dev(target, sim), **cost))
    return f


def kernel_select(sim):
    def f(cost, qpos, qvel, u, target, bad_step=None, u_fallback=None):
        return host(sim.cost_select(dev(qpos, sim), dev(qvel, sim), dev(u, sim), bad_step=dev(bad_step, sim, np.int32), u_fallback=dev(u_fallback, sim),
                                    target=dev(target, sim), **cost))
    return f


def show(tag, d):
    print(f"[cost-tol] gpu {tag}: " + " ".join(f"{k} {v:.3e}" + (f" (bound {S.KERNEL_FACTOR*S.FP32_MEASURED[k]:.2e})" if k in S.FP32_MEASURED else "") for k, v in d.items()))


def within(d):
    for k, v in S.FP32_MEASURED.items():
        if k in d:
            assert d[k] <= S.KERNEL_FACTOR*v, (k, d[k], S.KERNEL_FACTOR*v)


# ---- against the reference -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.COSTS))
def test_terms_against_the_reference(sim, name):
    cost, c, terms = S.COSTS[name], S.terms_case(), kernel_terms(sim)
    worst = {"lx": 0.0, "lxx": 0.0, "lu": 0.0, "luu": 0.0}
    for nx in (12, 24):
        for T in S.TERMS_T:
            ref = S.reference_terms(cost, *S.corner(c, T, 130, cost["target_mode"]), nx)
            for M in S.TERMS_M:
                d = S.terms_deviation(terms(cost, *S.corner(c, T, M, cost["target_mode"]), nx), {k: v[:, :M] for k, v in ref.items()})
                worst = {k: max(worst[k], d[k]) for k in worst}
    show(f"terms {name}", worst)
    assert worst["luu"] == 0.0
    within(worst)


@pytest.mark.parametrize("name", ["cube-ee", "fixed-l2", "traj-ee"])
def test_select_against_the_reference(sim, name):
    cost, select = S.COSTS[name], kernel_select(sim)
    worst, compared, left = 0.0, 0, 0
    for L in S.SELECT_L:
        for M in S.SELECT_M:
            c = S.select_case(L, M)
            args = S.select_args(c, cost["target_mode"])
            ref, got = S.reference_select(cost, *args), select(cost, *args, u_fallback=c["fallback"])
            worst = max(worst, float(np.abs(got["cost"].astype(np.float64) - ref["cost"]).max()))
            ok = S.comparable(ref)
            compared += int(ok.sum()); left += int((~ok).sum())
            assert (got["best"][ok] == ref["best"][ok]).all(), (L, M)
            env = np.arange(M)
            assert bits(got["u_best"]) == bits(c["u"][:, env, got["best"]]), (L, M)       # the winner's column, whichever it is
            assert bits(got["best_cost"]) == bits(got["cost"][env, got["best"]])
    show(f"select {name}", {"cost": worst})
    print(f"[cost-tol] gpu best {name}: {compared} problems compared, {left} left out as knife-edge")
    within({"cost": worst})
    assert left <= S.KNIFE_EDGE_SHARE*(compared + left)


# ---- exactness within the kernels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.COSTS))
def test_terms_exact_properties(sim, name):
    for T, M in ((3, 130), (3, 65), (1, 3), (1, 1)):
        S.check_terms_exact(kernel_terms(sim), S.COSTS[name], T, M)


def test_terms_zero_weights_place_and_non_finite_inputs(sim):
    terms = kernel_terms(sim)
    S.check_terms_zero_weights(terms)
    for name in ("cube-ee", "fixed-l2", "traj-ee"):
        S.check_terms_place(terms, S.COSTS[name], 12 if name == "traj-ee" else 24)
        S.check_terms_non_finite(terms, S.COSTS[name], 12 if name == "fixed-l2" else 24)


@pytest.mark.parametrize("L", [3, 8, 16])
@pytest.mark.parametrize("name", ["cube-ee", "fixed-l2", "traj-ee"])
def test_select_exact_properties(sim, name, L):
    if L == 8:
        S.check_select_exact(kernel_select(sim), S.COSTS[name])
        return
    # the other group sizes: candidate L - 1 doubles candidate 0, M = 65 against M = 3 inside it
    select, cost = kernel_select(sim), S.COSTS[name]
    c = S.select_case(L, 65)
    qpos, qvel, u, tg = (a.copy() if a is not None else None for a in S.select_args(c, cost["target_mode"]))
    qpos[:, :, L - 1], qvel[:, :, L - 1], u[:, :, L - 1] = qpos[:, :, 0], qvel[:, :, 0], u[:, :, 0]
    got = select(cost, qpos, qvel, u, tg)
    assert bits(got["cost"][:, L - 1]) == bits(got["cost"][:, 0]) and (got["best"] != L - 1).all() and (got["best"] == 0).any()
    assert (got["best_cost"][:, None] <= got["cost"]).all() and (got["best"] == np.argmin(got["cost"], axis=1)).all()
    sl = slice(20, 23)
    sub = select(cost, qpos[:, sl], qvel[:, sl], u[:, sl], None if tg is None else (tg[sl] if cost["target_mode"] == "fixed" else tg[:, sl]))
    for k in ("cost", "best", "best_cost"):
        assert bits(sub[k]) == bits(got[k][sl]), k
    assert bits(sub["u_best"]) == bits(got["u_best"][:, sl])
    one = select(cost, qpos[:, :, :1], qvel[:, :, :1], u[:, :, :1], tg)                      # L = 1: the candidate itself
    assert bits(one["cost"][:, 0]) == bits(got["cost"][:, 0]) and not one["best"].any() and bits(one["u_best"]) == bits(u[:, :, 0])


# ---- the C ABI itself: each output alone, unaligned pointers, graph replay -----------------------------------------------------------------------------------
TERMS_OUT = {"lx_dev": lambda T, M, n: (T + 1)*M*n, "lxx_dev": lambda T, M, n: (T + 1)*M*n*n, "lu_dev": lambda T, M, n: T*M*6, "luu_dev": lambda T, M, n: T*M*36}
SELECT_OUT = {"cost_dev": (lambda T, M, L: M*L, torch.float32), "best_dev": (lambda T, M, L: M, torch.int32), "best_cost_dev": (lambda T, M, L: M, torch.float32),
              "u_best_dev": (lambda T, M, L: T*6*M, torch.float32)}


def cost_struct(cost):
    from so100_mujoco_rl_amd import lib
    six = lambda w: (C.c_float*6)(*w)
    off = None if cost["offset"] is None else (C.c_float*3)(*cost["offset"])
    d = lib.CostDef(cost["link"], C.cast(off, C.c_void_p) if off is not None else None, S.TARGETS[cost["target_mode"]], cost["w_point"], six(cost["w_q"]),
                    six(cost["q_nom"]), six(cost["w_v"]), six(cost["w_u"]), cost["w_terminal"])
    return d, off


def raw_terms(sim, cost, nx, T, M, want, stream=None, out=None, keep=None, shift=0):
    """so100_query_cost_terms with the outputs of `want` alone into SENTINEL-filled buffers (each `shift` floats into its allocation)"""
    from so100_mujoco_rl_amd import lib
    c = S.terms_case()
    qpos, qvel, u, tg = S.corner(c, T, M, cost["target_mode"])
    soa = lambda a: None if a is None else dev(a, sim).transpose(-1, -2).contiguous()
    keep = [soa(qpos), soa(qvel), soa(u), soa(tg), cost_struct(cost)] if keep is None else keep
    out = {k: torch.full((size(T, M, nx) + shift,), SENTINEL, device=sim.device) for k, size in TERMS_OUT.items()} if out is None else out
    io = lib.CostTermsIO(cost=C.pointer(keep[4][0]), target_dev=None if keep[3] is None else keep[3].data_ptr(), nx=nx, T=T, qpos_traj_dev=keep[0].data_ptr(),
                         qvel_traj_dev=keep[1].data_ptr(), u_dev=keep[2].data_ptr(), **{k: out[k].data_ptr() + 4*shift for k in want})
    assert sim.L.so100_query_cost_terms(sim.h, C.byref(io), M, sim._stream() if stream is None else stream) == 0
    return out, keep


def raw_select(sim, cost, L, M, want, stream=None, out=None, keep=None):
    from so100_mujoco_rl_amd import lib
    c = S.select_case(L, M)
    qpos, qvel, u, tg = S.select_args(c, cost["target_mode"])
    T = S.SELECT_T
    cols = lambda a: dev(a, sim).permute(0, 3, 1, 2).reshape(T, a.shape[-1], M*L).contiguous()
    soa = lambda a: None if a is None else dev(a, sim).transpose(-1, -2).contiguous()
    bad = np.full((M, L), -1, np.int32); bad[M//2] = 0
    keep = [cols(qpos), cols(qvel), cols(u), soa(tg), cost_struct(cost), dev(bad.reshape(-1), sim, np.int32), soa(c["fallback"])] if keep is None else keep
    out = {k: torch.full((size(T, M, L),), SENTINEL, dtype=dt, device=sim.device) for k, (size, dt) in SELECT_OUT.items()} if out is None else out
    io = lib.CostSelectIO(cost=C.pointer(keep[4][0]), target_dev=None if keep[3] is None else keep[3].data_ptr(), T=T, L=L, qpos_traj_dev=keep[0].data_ptr(),
                          qvel_traj_dev=keep[1].data_ptr(), u_traj_dev=keep[2].data_ptr(), bad_step_dev=keep[5].data_ptr(), u_fallback_dev=keep[6].data_ptr(),
                          **{k: out[k].data_ptr() for k in want})
    assert sim.L.so100_query_cost_select(sim.h, C.byref(io), M, sim._stream() if stream is None else stream) == 0
    return out, keep


def test_each_output_alone_and_unaligned_pointers(sim):
    before = state_words(sim)
    for name, nx in (("cube-ee", 24), ("fixed-l2", 12)):
        cost = S.COSTS[name]
        full, keep = raw_terms(sim, cost, nx, 3, 65, list(TERMS_OUT))
        torch.cuda.synchronize()
        via = kernel_terms(sim)(cost, *S.corner(S.terms_case(), 3, 65, cost["target_mode"]), nx)
        for k in TERMS_OUT:
            assert bits(full[k].cpu().numpy()) == bits(via[k[:-4]]), k
        for k in TERMS_OUT:
            one, _ = raw_terms(sim, cost, nx, 3, 65, [k], keep=keep)
            torch.cuda.synchronize()
            for k2 in TERMS_OUT:
                assert bits(one[k2].cpu().numpy()) == bits(full[k2].cpu().numpy()) if k2 == k else bool((one[k2] == SENTINEL).all()), (k, k2)
        # outputs one float into their allocations: 4-byte stores (another instantiation of the kernel: the reference's bound, and the same properties)
        odd, _ = raw_terms(sim, cost, nx, 3, 65, list(TERMS_OUT), keep=keep, shift=1)
        torch.cuda.synchronize()
        assert all(float(odd[k][0]) == SENTINEL for k in TERMS_OUT)
        ref = S.reference_terms(cost, *S.corner(S.terms_case(), 3, 65, cost["target_mode"]), nx)
        got = {k[:-4]: odd[k][1:].cpu().numpy().reshape(ref[k[:-4]].shape) for k in TERMS_OUT}
        d = S.terms_deviation(got, ref)
        show(f"terms {name} nx {nx}, 4-byte stores", d)
        within(d)
        assert bits(got["lxx"]) == bits(np.swapaxes(got["lxx"], -1, -2)) and not got["lx"][0].any() and not got["lxx"][0].any()
    cost = S.COSTS["traj-ee"]
    full, keep = raw_select(sim, cost, 3, 65, list(SELECT_OUT))
    torch.cuda.synchronize()
    assert int(full["best_dev"][32]) == -1 and bits(full["u_best_dev"].cpu().numpy().reshape(3, 6, 65)[:, :, 32]) == bits(keep[6].cpu().numpy()[:, :, 32])
    for k in SELECT_OUT:
        one, _ = raw_select(sim, cost, 3, 65, [k], keep=keep)
        torch.cuda.synchronize()
        for k2 in SELECT_OUT:
            assert bits(one[k2].cpu().numpy()) == bits(full[k2].cpu().numpy()) if k2 == k else bool((one[k2] == SENTINEL).all()), (k, k2)
    assert (state_words(sim) == before).all()                     # the handle's state is never read or written


def test_a_graph_replay_gives_the_same_bits(sim):
    cost = S.COSTS["cube-ee"]
    direct_t, keep_t = raw_terms(sim, cost, 24, 3, 130, list(TERMS_OUT))
    direct_s, keep_s = raw_select(sim, cost, 8, 65, list(SELECT_OUT))
    torch.cuda.synchronize()
    out_t = {k: torch.full_like(v, SENTINEL) for k, v in direct_t.items()}
    out_s = {k: torch.full_like(v, int(SENTINEL)) for k, v in direct_s.items()}
    side = torch.cuda.Stream(device=sim.device)
    side.wait_stream(torch.cuda.current_stream(sim.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            raw_terms(sim, cost, 24, 3, 130, list(TERMS_OUT), stream=side.cuda_stream, out=out_t, keep=keep_t)
            raw_select(sim, cost, 8, 65, list(SELECT_OUT), stream=side.cuda_stream, out=out_s, keep=keep_s)
    torch.cuda.current_stream(sim.device).wait_stream(side)
    for v in list(out_t.values()) + list(out_s.values()):
        v.fill_(int(SENTINEL))
    graph.replay()
    torch.cuda.synchronize()
    for k in TERMS_OUT:
        assert bits(out_t[k].cpu().numpy()) == bits(direct_t[k].cpu().numpy()), k
    for k in SELECT_OUT:
        assert bits(out_s[k].cpu().numpy()) == bits(direct_s[k].cpu().numpy()), k


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(sim):
    """exact code and message of every check, in the header's order; a rejected call enqueues nothing and the handle goes on working"""
    from so100_mujoco_rl_amd import lib
    L, h, st = sim.L, sim.h, sim._stream()
    buf = torch.full((4, 2*N*24*24*2), SENTINEL, dtype=torch.float32, device=sim.device)
    inp = torch.zeros(13*2*2, N, dtype=torch.float32, device=sim.device)
    inp[9::13] = 1.0
    p, o = inp.data_ptr(), buf.data_ptr()
    six = lambda *w: (C.c_float*6)(*(w if len(w) == 6 else w*6))
    nan, inf = float("nan"), float("inf")
    bad_off = (C.c_float*3)(0.0, nan, 0.0)
    good = dict(link=4, offset=None, target_mode=0, w_point=1.0, w_q=six(0.1), q_nom=six(0.0), w_v=six(0.0), w_u=six(0.01), w_terminal=1.0)
    keep = []

    def cdef(**over):
        keep.append(lib.CostDef(**{**good, **over}))
        return C.pointer(keep[-1])
    wmsg = b"w_point, w_q, w_v, w_u and w_terminal must be finite and >= 0 and q_nom finite"
    current = torch.cuda.current_device()
    for fn, io_cls, entry, ok, extra, req in (
            (b"so100_query_cost_terms: ", lib.CostTermsIO, L.so100_query_cost_terms,
             dict(target_dev=p, nx=24, T=2, qpos_traj_dev=p, qvel_traj_dev=p, u_dev=p, lx_dev=o, lu_dev=o + 4*buf.shape[1]),
             [(dict(nx=18), b"nx must be 12 or 24, got 18"), (dict(T=0), b"T must be in 1..4096, got 0"), (dict(T=4097), b"T must be in 1..4096, got 4097")],
             ("u_dev", b"qpos_traj_dev, u_dev and (unless the target is the cube) target_dev are required")),
            (b"so100_query_cost_select: ", lib.CostSelectIO, L.so100_query_cost_select,
             dict(target_dev=p, T=2, L=2, qpos_traj_dev=p, qvel_traj_dev=p, u_traj_dev=p, cost_dev=o, best_dev=o + 4*buf.shape[1]),
             [(dict(T=0), b"T must be in 1..4096, got 0"), (dict(T=4097), b"T must be in 1..4096, got 4097"),
              (dict(L=0), b"L must be in 1..16 and M * L <= 2147483647, got L = 0, M = %d" % N), (dict(L=17), b"L must be in 1..16 and M * L <= 2147483647, got L = 17, M = %d" % N)],
             ("u_traj_dev", b"qpos_traj_dev, u_traj_dev and (unless the target is the cube) target_dev are required"))):
        outs = [k for k in ok if k.endswith("_dev") and k in ("lx_dev", "lxx_dev", "lu_dev", "luu_dev", "cost_dev", "best_dev", "best_cost_dev", "u_best_dev")]
        none = {k: None for k in outs}
        io = lambda **over: C.byref(io_cls(**{"cost": cdef(), **ok, **over}))
        call = lambda M=N, **over: (lambda: entry(h, io(**over), M, st))
        calls = [(lambda: entry(h, None, N, st), b"null argument"), (call(0), b"M must be >= 1, got 0")]
        calls += [(call(**over), msg) for over, msg in extra]
        calls += [
            (call(cost=None), b"cost is required"),
            (call(cost=cdef(link=6)), b"link must be in 0..5, got 6"),
            (call(cost=cdef(link=-1)), b"link must be in 0..5, got -1"),
            (call(cost=cdef(offset=C.cast(bad_off, C.c_void_p))), b"offset must be finite"),
            (call(cost=cdef(target_mode=3)), b"unknown target_mode 3"),
            (call(cost=cdef(w_point=-1.0)), wmsg), (call(cost=cdef(w_point=inf)), wmsg), (call(cost=cdef(w_terminal=nan)), wmsg),
            (call(cost=cdef(w_q=six(0.0, 0.0, -0.5, 0.0, 0.0, 0.0))), wmsg), (call(cost=cdef(w_v=six(0.0, 0.0, 0.0, 0.0, 0.0, nan))), wmsg),
            (call(cost=cdef(w_u=six(inf))), wmsg), (call(cost=cdef(q_nom=six(0.0, nan, 0.0, 0.0, 0.0, 0.0))), wmsg),
            (call(qpos_traj_dev=None), req[1]), (call(**{req[0]: None}), req[1]), (call(target_dev=None), req[1]),
            (call(target_dev=None, cost=cdef(target_mode=1)), req[1]),
            (call(**none), b"no output requested"),
            # the order: the first of several
            (call(cost=cdef(link=9, target_mode=7, w_point=-1.0), qpos_traj_dev=None, **none), b"link must be in 0..5, got 9"),
            (call(cost=cdef(target_mode=7, w_point=-1.0), qpos_traj_dev=None, **none), b"unknown target_mode 7"),
            (call(cost=cdef(w_point=-1.0), qpos_traj_dev=None, **none), wmsg),
            (call(qpos_traj_dev=None, **none), req[1]),
            (call(0, **dict(extra[0][0]), cost=None), b"M must be >= 1, got 0"),
            (call(**dict(extra[0][0]), cost=None), extra[0][1]),
        ]
        for f, msg in calls:
            assert f() == -1, msg
            assert L.so100_last_error() == fn + msg
            assert torch.cuda.current_device() == current
        torch.cuda.synchronize()
        assert (buf == SENTINEL).all()                            # nothing was enqueued
        # accepted: the cube target needs no target_dev, velocities are optional
        assert call(target_dev=None, qvel_traj_dev=None, cost=cdef(target_mode=2))() == 0
        torch.cuda.synchronize()
        assert not (buf[0] == SENTINEL).all() and not (buf[1] == SENTINEL).all() and (buf[2:] == SENTINEL).all()
        buf.fill_(SENTINEL)
    z = lambda *s: torch.zeros(*s, device=sim.device)
    with pytest.raises(lib.So100Error):
        sim.cost_terms(z(2, N, 13), None, z(2, N, 6), nx=18)
    with pytest.raises(lib.So100Error):
        sim.cost_terms(z(2, N, 13), None, z(2, N, 6), target_mode="fixed")
    with pytest.raises(lib.So100Error):
        sim.cost_terms(z(2, N, 13), None, z(2, N, 6), target=z(N, 3), target_mode="traj")
    with pytest.raises(lib.So100Error):
        sim.cost_select(z(2, N, 17, 13), None, z(2, N, 17, 6))
    with pytest.raises(lib.So100Error):
        sim.cost_terms(z(2, N, 13), None, z(2, N, 6), w_point=-1.0)
    assert torch.isfinite(sim.cost_terms(z(2, N, 13), None, z(2, N, 6), target=z(N, 3))["lxx"]).all()


# ---- the six queries chained on the device -----------------------------------------------------------------------------------------------------------------------
def test_the_planner_iteration_chained_on_the_device(sim):
    """section 15's physics family (3 contact-free starts, F_CUBE_PINNED, T = 8, actions): trajectory -> derivatives -> cost_terms -> lqr -> closed_loop ->
    cost_select with every device output passed straight in; cost_terms' arrays against the example's arithmetic (lqr_support.family_p writes it in
    numpy from the device's own Jacobians and ee), the selection against the torch argmin on the same rollouts"""
    t = lambda a: dev(a, sim)
    roll = lambda U, q, v: host(sim.trajectory(t(U), t(q), t(v), mode="actions", nsub=LS.P_NSUB, flags=scenes.FREE))
    der = lambda U, q, v: host(sim.derivatives(t(U), t(q), t(v), mode="actions", nsub=LS.P_NSUB, flags=scenes.FREE))
    jac = lambda q: sim.jacobian(t(q))["jacp"].contiguous().cpu().numpy()
    p, U = LS.family_p(12, roll, der, jac)
    c = TS.free_case("arm", "actions")
    q0, v0 = t(c["qpos"][:LS.P_M]), t(c["qvel"][:LS.P_M])
    T, M = LS.P_T, LS.P_M
    Ut = t(U)
    cost = dict(target_mode="cube", w_point=1.0, w_u=LS.P_CONTROL_COST)
    nominal = sim.trajectory(Ut, q0, v0, mode="actions", nsub=LS.P_NSUB, flags=scenes.FREE)
    Xq, Xv = torch.cat([q0[None], nominal["qpos"][:-1]]), torch.cat([v0[None], nominal["qvel"][:-1]])
    d = sim.derivatives(Ut.reshape(T*M, 6), Xq.reshape(T*M, 13), Xv.reshape(T*M, 12), mode="actions", nsub=LS.P_NSUB, flags=scenes.FREE)
    terms = sim.cost_terms(nominal["qpos"], nominal["qvel"], Ut, nx=12, **cost)
    dv = {k: float(np.abs(terms[k].cpu().numpy().astype(np.float64) - np.asarray(p[k], np.float64)).max()) for k in ("lx", "lxx", "lu", "luu")}
    show("chained terms vs the example's arithmetic", dv)
    within(dv)
    B = d["B"].reshape(T, M, 24, 6).clone(); B[..., 5] = 0.0
    s = sim.lqr(d["A"].reshape(T, M, 24, 24), B, terms["lx"], terms["lxx"], lu=terms["lu"], luu=terms["luu"], nx=12, reg=LS.P_DAMPING)
    assert (s["bad"] == -1).all()
    alphas = (0.0,) + tuple(2.0**-i for i in range(7))
    cl = sim.closed_loop(Ut, nominal["qpos"], nominal["qvel"], s["K"], s["k"], alphas=alphas, nx=12, qpos=q0, qvel=v0, mode="actions", nsub=LS.P_NSUB,
                         flags=scenes.FREE, clamp=(-1.0, 1.0))
    assert (cl["bad_step"] == -1).all()
    pick = host(sim.cost_select(cl["qpos"], cl["qvel"], cl["u"], bad_step=cl["bad_step"], u_fallback=Ut, **cost))
    cube = q0[:, 6:9]
    torch_cost = ((cl["ee"] - cube[None, :, None]).square().sum(-1) + LS.P_CONTROL_COST*cl["u"].square().sum(-1)).sum(0)
    ref = S.reference_select(S.cost_def(**cost), cl["qpos"].cpu().numpy(), cl["qvel"].cpu().numpy(), cl["u"].cpu().numpy(), None)
    dc = float(np.abs(pick["cost"].astype(np.float64) - ref["cost"]).max())
    show("chained select vs the reference", {"cost": dc, "vs torch": float((torch_cost.cpu() - torch.from_numpy(pick["cost"])).abs().max())})
    within({"cost": dc})
    ok = S.comparable(ref)
    print(f"[cost-tol] gpu chained best: {int(ok.sum())} of {M} problems compared (gaps {ref['gap']}), best {pick['best']}")
    assert (pick["best"][ok] == torch_cost.argmin(dim=1).cpu().numpy()[ok]).all() and (pick["best"][ok] == ref["best"][ok]).all()
    assert (pick["best_cost"] <= pick["cost"][:, 0]).all()
    env = np.arange(M)
    assert bits(pick["u_best"]) == bits(cl["u"].cpu().numpy()[:, env, pick["best"]])


# ---- the example -------------------------------------------------------------------------------------------------------------------------------------------------
def test_ilqr_reach_with_the_cost_queries():
    """examples/ilqr_reach.py --forward closed --cost query on 8 envs, horizon 8, 10 steps: at every iteration and env the chosen plan's cost is at most the
    old plan's; the final distances with --cost query and --cost torch are printed (a record)"""
    from so100_mujoco_rl_amd import lib
    spec = importlib.util.spec_from_file_location("ilqr_reach", os.path.join(ROOT, "examples", "ilqr_reach.py"))
    ilqr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ilqr)
    result = {}
    for cost in ("query", "torch"):
        policy = ilqr.Ilqr(8, 2, backward="query", forward="closed", cost=cost)
        s = lib.So100Sim(lib.ENV01, 8, flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
        result[cost] = ilqr.run(s, 10, policy)
        s.close()
        assert len(policy.costs) == 20
        for chosen, old in policy.costs:
            assert chosen.shape == (8,) and bool((chosen <= old).all())
        assert any(bool((chosen < old).any()) for chosen, old in policy.costs)
    print(f"[cost-tol] iLQR reach, 8 envs, horizon 8, 10 steps, --forward closed: mean |cube - ee| {result['query'][0]:.4f} m at reset -> --cost query "
          f"{result['query'][1]:.4f} m, --cost torch {result['torch'][1]:.4f} m")
    assert result["query"][0] == result["torch"][0]
