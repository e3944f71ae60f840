"""The LQR query with a regulariser per problem and its schedule on the GPU (include/so100_query.h: so100_query_lqr_reg,
so100_query_reg_schedule), through the C ABI, So100Sim.lqr_reg and So100Sim.reg_schedule: the checks of tests/test_lqr_reg_cpu.py on the kernel,
under the bounds of tests/lqr_reg_support.py (KERNEL_FACTOR x the fp32 twin's record of the fp64 recursion; integers and regs exact), plus what
only a handle can show: the two identities against the plain kernel bit for bit, independence of M and place, nullable outputs, that the
handle's state is never touched, every argument error in the header's order, and examples/ilqr_reach.py --reg adaptive end to end.

Shapes: T in {1, 5}, M in {1, 3, 65} (the per-problem rows cross a 64 boundary at 65), nx in {12, 24}; the retry problem at places 0, 1 and 64."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import lqr_reg_support as R                               # noqa: E402
import lqr_support as S                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8
NS = (12, 24)
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


def args(sim, p):
    return ([dev(p[k], sim) for k in ("A", "B", "lx", "lxx", "lu", "luu", "lux")],
            dict(nx=p["nx"], alpha=p["alpha"], u=dev(p["u"], sim), u_lo=p["u_lo"], u_hi=p["u_hi"], dx0=dev(p["dx0"], sim)))


def query(sim, p, reg=None, **knobs):
    """So100Sim.lqr_reg on a lqr_support.problem(); reg: [M] starting regs or None (p["reg"] for all): numpy outputs"""
    pos, kw = args(sim, p)
    r = sim.lqr_reg(*pos, reg=p["reg"] if reg is None else dev(np.asarray(reg, np.float32), sim), **kw, **knobs)
    return {k: v.cpu().numpy() for k, v in r.items()}


def plain(sim, p):
    """So100Sim.lqr on the same: numpy outputs"""
    pos, kw = args(sim, p)
    return {k: v.cpu().numpy() for k, v in sim.lqr(*pos, reg=p["reg"], **kw).items()}


def problem_of(out, m):
    return {k: (v[m] if k in ("Vx0", "Vxx0", "dV", "bad", "reg_used", "tries") else v[:, m]) for k, v in out.items()}


def failed(got, m):
    for name in R.FLOAT_OUT:
        g = got[name]
        assert np.isnan(g[m] if name in ("Vx0", "Vxx0", "dV") else g[:, m]).all(), name


def check_against(got, ref):
    """integers and regs exact; floats of the problems that got through within KERNEL_FACTOR x the record; those of the others NaN"""
    assert got["bad"].tolist() == ref["bad"].tolist() and got["tries"].tolist() == ref["tries"].tolist()
    assert bits(got["reg_used"]) == bits(ref["reg_used"])
    ok = np.flatnonzero(ref["bad"] < 0)
    for m in np.flatnonzero(ref["bad"] >= 0):
        failed(got, m)
    d = R.deviation(R.select({k: got[k] for k in R.FLOAT_OUT}, ok), R.select({k: ref[k] for k in R.FLOAT_OUT}, ok))
    print("[lqr-reg-tol] gpu " + " ".join(f"{k}={v:.2e} (bound {R.KERNEL_FACTOR*S.FP32_MEASURED[R.RECORD][k]:.1e})" for k, v in d.items()))
    R.within(d, R.KERNEL_FACTOR)


# ---- A: the retry case and its variants ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_the_retry_case(sim, n):
    p, ref = R.retry_case(n)
    got = query(sim, p, **R.KNOBS)
    assert got["tries"].tolist() == [1, 4, 1] and got["reg_used"].tolist() == [0.0, 2.0, 0.0] and got["bad"].tolist() == [-1, -1, -1]
    check_against(got, ref)


@pytest.mark.parametrize("n", NS)
def test_the_retry_gives_up_where_tries_or_reg_max_say_so(sim, n):
    p, _ = R.retry_case(n)
    for knobs in (dict(R.KNOBS, tries=3), dict(R.KNOBS, tries=8, reg_max=0.5)):
        got = query(sim, p, **knobs)
        assert got["bad"].tolist() == [-1, S.FAIL_AT, -1] and got["reg_used"][1] == 0.5 and got["tries"].tolist() == [1, 3, 1]
        ref = R.reference(p, **knobs)
        R.assert_premises(ref, S.FAIL_T)
        check_against(got, ref)


@pytest.mark.parametrize("n", NS)
def test_regs_per_problem_and_non_finite_inputs(sim, n):
    p, _ = R.retry_case(n)
    one = dict(R.KNOBS, tries=1)
    start = np.array([0.0, 2.0, 0.0], np.float32)
    got = query(sim, p, start, **one)
    assert got["bad"].tolist() == [-1, -1, -1] and got["tries"].tolist() == [1, 1, 1] and got["reg_used"].tolist() == [0.0, 2.0, 0.0]
    check_against(got, R.reference(p, start, **one))
    for value in (np.nan, -1.0):
        start = np.array([value, 2.0, 0.0], np.float32)
        bad = query(sim, p, start, **R.KNOBS)
        assert bad["bad"].tolist() == [S.FAIL_T, -1, -1] and bad["tries"].tolist() == [0, 1, 1] and np.isnan(bad["reg_used"][0]) and bad["reg_used"][1:].tolist() == [2.0, 0.0]
        failed(bad, 0)
        for m in (1, 2):
            a, b = problem_of(bad, m), problem_of(got, m)
            assert all(bits(a[k]) == bits(b[k]) for k in R.OUT), m
    for q in S.nonfinite_cases(n):
        g = query(sim, q, **R.KNOBS)
        assert g["bad"].tolist() == [-1, S.FAIL_T, -1] and g["tries"].tolist() == [1, 1, 1] and g["reg_used"].tolist() == [0.0, 0.0, 0.0]
        failed(g, S.FAIL_PROBLEM)


# ---- B: the identities ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("n", NS)
def test_one_try_without_regs_is_the_plain_query(sim, n, T):
    for M in (1, 3, 65):
        p = dict(S.first(S.family_s(n, T), M), reg=0.25)
        a, b = query(sim, p, reg_min=0.125, reg_max=32.0, reg_up=4.0, tries=1), plain(sim, p)
        assert all(bits(a[k]) == bits(b[k]) for k in S.OUT), M
        assert (a["tries"] == 1).all() and (a["reg_used"] == 0.25).all()


@pytest.mark.parametrize("n", NS)
def test_a_problem_that_succeeds_is_the_plain_query_alone_under_reg_used(sim, n):
    p, _ = R.retry_case(n)
    got = query(sim, p, **R.KNOBS)
    assert got["reg_used"].tolist() == [0.0, 2.0, 0.0]
    for m in range(3):
        alone = plain(sim, dict(R.select(p, [m]), reg=float(got["reg_used"][m])))
        a, b = problem_of(got, m), problem_of(alone, 0)
        assert b["bad"] == -1 and all(bits(a[k]) == bits(b[k]) for k in S.FLOAT_OUT), m


@pytest.mark.parametrize("n", NS)
def test_bits_do_not_depend_on_m_or_place_and_repeat(sim, n):
    p3, _ = R.retry_case(n)
    want = problem_of(query(sim, p3, **R.KNOBS), S.FAIL_PROBLEM)
    clean = plain(sim, dict(S.first(S.family_s(n, S.FAIL_T), 65), reg=0.0))
    for place in (0, 1, 64):
        p = R.embedded_case(n, place)
        got, again = query(sim, p, **R.KNOBS), query(sim, p, **R.KNOBS)
        assert all(bits(got[k]) == bits(again[k]) for k in R.OUT)
        assert got["tries"].tolist() == [4 if m == place else 1 for m in range(65)] and got["reg_used"][place] == 2.0 and (got["bad"] == -1).all()
        a = problem_of(got, place)
        assert all(bits(a[k]) == bits(want[k]) for k in R.OUT), place
        other = 2 if place != 2 else 3
        a, b = problem_of(got, other), problem_of(clean, other)
        assert all(bits(a[k]) == bits(b[k]) for k in S.OUT), place


# ---- C: what only the device shows ------------------------------------------------------------------------------------------------------------------------
def raw(sim, p, want, **knobs):
    """the C ABI itself with the outputs of `want` alone, every output buffer pre-filled with SENTINEL: {name: tensor}"""
    from so100_mujoco_rl_amd import lib
    T, M, n, shp = R.shapes(p)
    ins = {k: dev(p[k], sim) for k in INPUTS}
    out = {k: torch.full(shp[k], SENTINEL, dtype=torch.int32 if k in ("bad", "tries") else torch.float32, device=sim.device) for k in R.OUT}
    base = lib.LqrIO(nx=n, T=T, reg=p["reg"], alpha=p["alpha"], u_lo=p["u_lo"], u_hi=p["u_hi"],
                     **{k + "_dev": (None if t is None else t.data_ptr()) for k, t in ins.items()}, **{k + "_dev": out[k].data_ptr() for k in want if k in S.OUT})
    io = lib.LqrRegIO(base=base, reg_dev=None, **knobs, **{k + "_dev": out[k].data_ptr() for k in want if k not in S.OUT})
    assert sim.L.so100_query_lqr_reg(sim.h, C.byref(io), M, sim._stream()) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n", NS)
def test_each_output_alone_leaves_the_others_untouched_and_the_state_alone(sim, n):
    before = state_words(sim)
    p, _ = R.retry_case(n)
    for knobs in (R.KNOBS, dict(R.KNOBS, tries=3)):                # all through; problem 1 failed (the NaN fill)
        full = raw(sim, p, list(R.OUT), **knobs)
        for name in R.OUT:
            want = [name] + (["k", "K"] if name in ("du", "dx") else [])
            out = raw(sim, p, want, **knobs)
            for k in R.OUT:
                if k in want:
                    assert bits(out[k].cpu().numpy()) == bits(full[k].cpu().numpy()), (name, k)
                else:
                    assert (out[k] == SENTINEL).all(), (name, k)
    assert bits(state_words(sim)) == bits(before)


@pytest.mark.parametrize("M", [18, 65])
def test_the_schedule_table(sim, M):
    """the exact table, with reg_dev = reg_used_dev and without; M = 65: the table repeated past a wave"""
    reg_used, best, want, improved = R.schedule_table()
    reps = -(-M//len(want))
    reg_used, best, want, improved = (np.tile(a, reps)[:M] for a in (reg_used, best, want, improved))
    r = sim.reg_schedule(dev(reg_used, sim), dev(best, sim), keep=R.SCHEDULE_KEEP, **R.SCHEDULE_KNOBS)
    assert bits(r["reg"].cpu().numpy()) == bits(want) and bits(r["improved"].cpu().numpy()) == bits(improved)
    same = dev(reg_used, sim)
    r = sim.reg_schedule(same, dev(best, sim), keep=R.SCHEDULE_KEEP, out=same, **R.SCHEDULE_KNOBS)
    assert r["reg"] is same and bits(same.cpu().numpy()) == bits(want) and bits(r["improved"].cpu().numpy()) == bits(improved)
    r = sim.reg_schedule(dev(reg_used, sim), dev(best, sim), keep=-1, **R.SCHEDULE_KNOBS)
    ref, ref_imp = R.schedule_reference(reg_used, best, -1, **R.SCHEDULE_KNOBS)
    assert bits(r["reg"].cpu().numpy()) == bits(ref) and bits(r["improved"].cpu().numpy()) == bits(ref_imp)


def test_argument_errors(sim):
    """exact code and message of every check of both entries, in the header's order; a rejected call enqueues nothing and the handle goes on working"""
    from so100_mujoco_rl_amd import lib
    L, h, st = sim.L, sim.h, sim._stream()
    M = 3
    buf = torch.full((4*M*24*24,), float(SENTINEL), dtype=torch.float32, device=sim.device)
    inp = torch.zeros(4*M*24*24, dtype=torch.float32, device=sim.device)
    p, o = inp.data_ptr(), buf.data_ptr()
    nan, inf = float("nan"), float("inf")
    fn = b"so100_query_lqr_reg: "
    okb = dict(nx=24, T=2, A_dev=p, B_dev=p, lx_dev=p, lxx_dev=p, reg=0.0, alpha=1.0, u_lo=-1.0, u_hi=1.0, k_dev=o, K_dev=o, bad_dev=o)
    okr = dict(reg_dev=None, reg_min=0.125, reg_max=32.0, reg_up=4.0, tries=4, reg_used_dev=o, tries_dev=o)
    none = dict(k_dev=None, K_dev=None, bad_dev=None)
    io = lambda base={}, **over: C.byref(lib.LqrRegIO(base=lib.LqrIO(**{**okb, **base}), **{**okr, **over}))
    req = fn + b"A_dev, B_dev, lx_dev and lxx_dev are required"
    call = L.so100_query_lqr_reg
    worst = dict(reg_min=0.0, reg_max=-1.0, reg_up=1.0, tries=0, reg_used_dev=None, tries_dev=None)
    calls = [
        (lambda: call(h, None, M, st), fn + b"null argument"),
        (lambda: call(None, io(), M, st), fn + b"null argument"),
        # those of so100_query_lqr on base, under this entry's name
        (lambda: call(h, io(), 0, st), fn + b"M must be >= 1, got 0"),
        (lambda: call(h, io(dict(nx=6)), M, st), fn + b"nx must be 12 or 24, got 6"),
        (lambda: call(h, io(dict(T=4097)), M, st), fn + b"T must be in 1..4096, got 4097"),
        (lambda: call(h, io(dict(lxx_dev=None)), M, st), req),
        (lambda: call(h, io(dict(reg=-1.0)), M, st), fn + b"reg must be finite and >= 0, got -1"),
        (lambda: call(h, io(dict(reg=nan), reg_dev=p), M, st), fn + b"reg must be finite and >= 0, got nan"),        # checked with reg_dev too
        (lambda: call(h, io(dict(alpha=inf)), M, st), fn + b"alpha must be finite, got inf"),
        (lambda: call(h, io(dict(u_lo=0.5, u_hi=0.25)), M, st), fn + b"u_lo must be <= u_hi, got 0.5 and 0.25"),
        (lambda: call(h, io(dict(du_dev=o, K_dev=None)), M, st), fn + b"du_dev and dx_dev need k_dev and K_dev"),
        # its own
        (lambda: call(h, io(reg_min=0.0), M, st), fn + b"reg_min must be finite and > 0, got 0"),
        (lambda: call(h, io(reg_min=nan), M, st), fn + b"reg_min must be finite and > 0, got nan"),
        (lambda: call(h, io(reg_min=inf), M, st), fn + b"reg_min must be finite and > 0, got inf"),
        (lambda: call(h, io(reg_max=0.0625), M, st), fn + b"reg_max must be finite and >= reg_min, got 0.0625"),
        (lambda: call(h, io(reg_max=inf), M, st), fn + b"reg_max must be finite and >= reg_min, got inf"),
        (lambda: call(h, io(reg_up=1.0), M, st), fn + b"reg_up must be finite and > 1, got 1"),
        (lambda: call(h, io(reg_up=inf), M, st), fn + b"reg_up must be finite and > 1, got inf"),
        (lambda: call(h, io(tries=0), M, st), fn + b"tries must be in 1..16, got 0"),
        (lambda: call(h, io(tries=17), M, st), fn + b"tries must be in 1..16, got 17"),
        (lambda: call(h, io(none, reg_used_dev=None, tries_dev=None), M, st), fn + b"no output requested"),
        # the order: the first of several
        (lambda: call(h, io(dict(du_dev=o, **none), **worst), M, st), fn + b"du_dev and dx_dev need k_dev and K_dev"),
        (lambda: call(h, io(none, **worst), M, st), fn + b"reg_min must be finite and > 0, got 0"),
        (lambda: call(h, io(none, **dict(worst, reg_min=0.125)), M, st), fn + b"reg_max must be finite and >= reg_min, got -1"),
        (lambda: call(h, io(none, **dict(worst, reg_min=0.125, reg_max=32.0)), M, st), fn + b"reg_up must be finite and > 1, got 1"),
        (lambda: call(h, io(none, **dict(worst, reg_min=0.125, reg_max=32.0, reg_up=4.0)), M, st), fn + b"tries must be in 1..16, got 0"),
        (lambda: call(h, io(none, **dict(worst, reg_min=0.125, reg_max=32.0, reg_up=4.0, tries=1)), M, st), fn + b"no output requested"),
    ]
    fs = b"so100_query_reg_schedule: "
    oks = dict(reg_used_dev=p, best_dev=p, keep=0, reg_min=0.125, reg_max=32.0, reg_up=4.0, reg_down=0.25, reg_dev=o, improved_dev=None)
    sio = lambda **over: C.byref(lib.RegScheduleIO(**{**oks, **over}))
    sreq = fs + b"reg_used_dev, best_dev and reg_dev are required"
    sched = L.so100_query_reg_schedule
    calls += [
        (lambda: sched(h, None, M, st), fs + b"null argument"),
        (lambda: sched(None, sio(), M, st), fs + b"null argument"),
        (lambda: sched(h, sio(), 0, st), fs + b"M must be >= 1, got 0"),
        (lambda: sched(h, sio(reg_used_dev=None), M, st), sreq),
        (lambda: sched(h, sio(best_dev=None), M, st), sreq),
        (lambda: sched(h, sio(reg_dev=None), M, st), sreq),
        (lambda: sched(h, sio(keep=-2), M, st), fs + b"keep must be a candidate index or -1, got -2"),
        (lambda: sched(h, sio(reg_min=-1.0), M, st), fs + b"reg_min must be finite and > 0, got -1"),
        (lambda: sched(h, sio(reg_max=0.0), M, st), fs + b"reg_max must be finite and >= reg_min, got 0"),
        (lambda: sched(h, sio(reg_up=nan), M, st), fs + b"reg_up must be finite and > 1, got nan"),
        (lambda: sched(h, sio(reg_down=0.0), M, st), fs + b"reg_down must be in (0, 1], got 0"),
        (lambda: sched(h, sio(reg_down=1.5), M, st), fs + b"reg_down must be in (0, 1], got 1.5"),
        (lambda: sched(h, sio(reg_down=nan), M, st), fs + b"reg_down must be in (0, 1], got nan"),
        (lambda: sched(h, sio(reg_dev=None, keep=-2, reg_min=0.0, reg_down=2.0), 0, st), fs + b"M must be >= 1, got 0"),
        (lambda: sched(h, sio(reg_dev=None, keep=-2, reg_min=0.0, reg_down=2.0), M, st), sreq),
        (lambda: sched(h, sio(keep=-2, reg_min=0.0, reg_down=2.0), M, st), fs + b"keep must be a candidate index or -1, got -2"),
        (lambda: sched(h, sio(reg_min=0.0, reg_down=2.0), M, st), fs + b"reg_min must be finite and > 0, got 0"),
    ]
    current = torch.cuda.current_device()
    for c, msg in calls:
        assert c() == -1, msg
        assert L.so100_last_error() == msg
        assert torch.cuda.current_device() == current
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()                                # nothing was enqueued
    A, B, lx, lxx = torch.zeros(2, M, 24, 24), torch.zeros(2, M, 24, 6), torch.zeros(3, M, 24), torch.zeros(3, M, 24, 24)
    with pytest.raises(lib.So100Error):
        sim.lqr_reg(A, B, lx, lxx, reg=torch.zeros(M + 1))        # one reg per problem
    with pytest.raises(lib.So100Error):
        sim.lqr_reg(A, B, lx, lxx, tries=17)
    with pytest.raises(lib.So100Error):
        sim.reg_schedule(torch.zeros(M), torch.zeros(M + 1, dtype=torch.int32))
    assert sim.reg_schedule(torch.zeros(M), torch.zeros(M, dtype=torch.int32))["reg"].shape == (M,)       # reg_down = 1 is allowed too
    assert sim.reg_schedule(torch.zeros(M), torch.zeros(M, dtype=torch.int32), reg_down=1.0)["improved"].tolist() == [0]*M


def test_header_structs():
    import test_lqr_reg_cpu as CPU
    CPU.test_structs_match_the_header_field_for_field()


# ---- E: the example ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ilqr():
    spec = importlib.util.spec_from_file_location("ilqr_reach", os.path.join(ROOT, "examples", "ilqr_reach.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_example(ilqr, policy, steps=20):
    from so100_mujoco_rl_amd import lib
    s = lib.So100Sim(lib.ENV01, 8, flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
    result = ilqr.run(s, steps, policy)
    s.close()
    return result


def test_ilqr_reach_with_a_reg_per_env(ilqr):
    """examples/ilqr_reach.py --reg adaptive on 8 envs, horizon 8, 20 steps ends below the zero-action baseline on the same starts, and the line
    search never takes a plan that costs more than the one it had"""
    policy = ilqr.Ilqr(8, reg="adaptive")
    got, zero = run_example(ilqr, policy), run_example(ilqr, ilqr.zero_action)
    print(f"[lqr-reg-tol] iLQR reach --reg adaptive, 8 envs x H = 8, 20 steps: mean |cube - ee| {got[0]:.4f} m at reset -> {got[1]:.4f} m; zero action -> "
          f"{zero[1]:.4f} m; regs at the end {policy.regs.cpu().tolist()}")
    assert got[0] == zero[0]                                      # the same starts
    assert got[1] < zero[1]
    assert len(policy.costs) == 40                                # two improvements per step, none skipped
    for chosen, old in policy.costs:
        assert not (chosen > old).any()


def test_ilqr_reach_over_a_zero_pivot(ilqr):
    """--control-cost 0 --damping 0: the jaw's zero column of B makes a pivot of Quu exactly zero.  The fixed reg fails every env and the plan stays
    at exactly zero; the adaptive one lifts itself off zero and the plan moves"""
    fixed = ilqr.Ilqr(8, control_cost=0.0, damping=0.0, forward="closed", cost="query")
    run_example(ilqr, fixed)
    assert fixed.plan is not None and not fixed.plan.any() and not fixed.costs
    adaptive = ilqr.Ilqr(8, control_cost=0.0, damping=0.0, reg="adaptive")
    got = run_example(ilqr, adaptive)
    print(f"[lqr-reg-tol] iLQR reach --reg adaptive --control-cost 0 --damping 0: {got[0]:.4f} m -> {got[1]:.4f} m; regs at the end {adaptive.regs.cpu().tolist()}")
    assert adaptive.plan.any() and (adaptive.regs >= 0).all()
