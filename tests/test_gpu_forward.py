"""The forward-dynamics query on the GPU (so100_query_forward, So100Sim.forward): the kernel against the fp64 oracle on cases drawn from the
recipe of tests/forward_support.py, held to 3 x the fp32 host twin's measured deviation per batch family; checks that need no oracle (Newton's
second law for the cube, signs, the residual); the handle's own state; read-only; determinism; every argument error; one graph capture; and
examples/grasp_probe.py end to end.

Shapes: M = 1 (one quad), 65 (a quad past a 16-problem workgroup and a 64-lane wave), 321 (a tail in a later workgroup), mixed over the batch
families that share a flag set, so that contact lanes and contact-free lanes share a wave."""
import ctypes as C
import importlib.util
import os
import signal

import numpy as np
import pytest
import torch

import forward_support as S
import scenes
from gpu_support import inject_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 65
FLAG_SETS = {"REFP": ("floor",), "C5": ("grasp", "floor_cube"), "LCUBE": ("link_cube",), "LINKS": ("wrist_first",)}


@pytest.fixture(autouse=True)
def own_time_limit():
    """a test that hangs ends the process (SIGALRM's default action) instead of holding the GPU"""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(120)
    yield
    signal.alarm(0)


@pytest.fixture(scope="module")
def sim():
    """N = 65, Env01, F_CONTACT5, the jaw closing on the cube (grasp_batch through set_state), three steps"""
    from so100_mujoco_rl_amd import lib
    s = lib.So100Sim(lib.ENV01, N, flags=lib.F_CONTACT5, seed=3)
    s.reset()
    qpos, qvel, act = scenes.grasp_batch(N, 0)
    inject_state(s, qpos, qvel)
    a = torch.from_numpy(act).to(s.device)
    for _ in range(3):
        s.step(a)
    torch.cuda.synchronize()
    yield s
    s.close()


def host(res):
    out = {k: v.contiguous().cpu().numpy() for k, v in res.items() if k != "contacts"}
    out["contacts"] = {k: v.contiguous().cpu().numpy() for k, v in res["contacts"].items()}
    return out


def dev(a, sim):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(sim.device)


def state_words(sim):
    return torch.stack([sim.get_field(n, dtype=torch.int32) for n in sim.field_names()]).cpu().numpy()


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a if k != "contacts") and \
        all(a["contacts"][k].tobytes() == b["contacts"][k].tobytes() for k in a["contacts"])


def draw(names, M):
    """M (family, case) pairs, interleaved over the families and spread over each one's cases (repeated where a family has fewer)"""
    fams = [S.family(n) for n in names]
    picks = []
    for j in range(M):
        f = fams[j % len(fams)]
        picks.append((f, (7*(j//len(fams)) + 3) % len(f)))
    return picks


@pytest.mark.parametrize("M", [1, 65, 321])
@pytest.mark.parametrize("flagset", sorted(FLAG_SETS))
def test_kernel_against_the_oracle(sim, flagset, M):
    picks = draw(FLAG_SETS[flagset], M)
    flags = picks[0][0].flags
    qpos, qvel, ctrl = (np.stack([getattr(f, a)[c] for f, c in picks]) for a in ("qpos", "qvel", "ctrl"))
    got = host(sim.forward(dev(qpos, sim), dev(qvel, sim), dev(ctrl, sim), flags=flags))
    assert got["qacc"].shape == (M, 12) and got["contacts"]["frame"].shape == (M, S.MAXCON, 3, 3) and got["contacts"]["feat"].dtype == np.int32
    worst = {f.name: dict.fromkeys(S.QUANTITIES, 0.0) for f, _ in picks}
    for j, (f, c) in enumerate(picks):
        if f.knife[c]:
            continue
        for k, e in S.check_case(got, j, f.refs[c]).items():
            worst[f.name][k] = max(worst[f.name][k], e)
    for name, row in worst.items():
        for k, e in row.items():
            print(f"[forward-tol] gpu {flagset} M={M} {name} {k}: {e:.3e} (bound {S.FP32_BOUNDS[name][k]:.2e})")
    for name, row in worst.items():
        for k, e in row.items():
            assert e <= S.FP32_BOUNDS[name][k], (name, k, e)
    for j, (f, c) in enumerate(picks):
        if not f.knife[c]:
            S.check_physical(got, j, S.FP32_BOUNDS[f.name]["con_force"], np.float32)


def test_the_handles_own_state_read_only_and_deterministic(sim):
    from so100_mujoco_rl_amd import lib
    before = state_words(sim)
    qpos, qvel = (t.cpu().numpy().T for t in sim.get_state())
    a, b = host(sim.forward()), host(sim.forward())
    assert same_bits(a, b)
    # no arguments = the handle's state, its flags, ctrl = q: the same bits as the same state handed in
    c = host(sim.forward(dev(qpos, sim), dev(qvel, sim), dev(qpos[:, :6], sim), flags=lib.F_CONTACT5))
    assert same_bits(a, c)
    assert a["ncon"].shape == (N,) and a["pad_force"].shape == (N, 8) and (a["ncon"] > 0).any()
    worst = dict.fromkeys(S.QUANTITIES, 0.0)
    for i in range(N):
        ref = S.oracle_forward(qpos[i].astype(np.float64), qvel[i].astype(np.float64), qpos[i, :6].astype(np.float64), scenes.C5)
        for k, e in S.check_case(a, i, ref).items():
            worst[k] = max(worst[k], e)
        S.check_physical(a, i, S.FP32_BOUNDS["grasp"]["con_force"], np.float32)
    for k, e in worst.items():
        print(f"[forward-tol] gpu handle state {k}: {e:.3e} (bound {S.FP32_BOUNDS['grasp'][k]:.2e})")
        assert e <= S.FP32_BOUNDS["grasp"][k], (k, e)
    torch.cuda.synchronize()
    assert (state_words(sim) == before).all()


def test_nullable_outputs_and_null_velocity(sim):
    from so100_mujoco_rl_amd import lib
    fam = S.family("grasp")
    M = 65
    qs = dev(fam.qpos[:M].T, sim)
    full = host(sim.forward(dev(fam.qpos[:M], sim), flags=fam.flags))
    zero = host(sim.forward(dev(fam.qpos[:M], sim), dev(np.zeros((M, 12), np.float32), sim), dev(fam.qpos[:M, :6], sim), flags=fam.flags))
    assert same_bits(full, zero)
    sentinel = -777.0
    arena = torch.full((12 + 8 + 12, M), sentinel, dtype=torch.float32, device=sim.device)       # qacc | pad_force | a guard
    io = lib.ForwardIO(qpos_dev=qs.data_ptr(), flags=fam.flags, solver_iters=64, contact_iters=64, pad_force_dev=arena[12:20].data_ptr())
    assert sim.L.so100_query_forward(sim.h, C.byref(io), M, sim._stream()) == 0
    a = arena.cpu().numpy()
    assert (a[12:20].T == full["pad_force"]).all() and (a[:12] == sentinel).all() and (a[20:] == sentinel).all()


def test_non_finite_input(sim):
    fam = S.family("grasp")
    q = fam.qpos[:8].copy(); q[1, 2] = np.nan; q[6, 8] = np.inf
    got = host(sim.forward(dev(q, sim), dev(fam.qvel[:8], sim), dev(fam.ctrl[:8], sim), flags=fam.flags))
    for i in (1, 6):
        assert got["ncon"][i] == 0 and np.isnan(got["qacc"][i]).all() and (got["contacts"]["feat"][i] == -1).all()
    ok = [0, 2, 3, 4, 5, 7]
    assert np.isfinite(got["qacc"][ok]).all() and same_bits(host(sim.forward(dev(q[ok], sim), dev(fam.qvel[ok], sim), dev(fam.ctrl[ok], sim), flags=fam.flags)),
                                                             {**{k: v[ok] for k, v in got.items() if k != "contacts"}, "contacts": {k: v[ok] for k, v in got["contacts"].items()}})


def test_argument_errors(sim):
    """exact code and message of every check, in the header's order; a rejected call leaves poisoned output buffers untouched"""
    from so100_mujoco_rl_amd import lib
    L, h, st = sim.L, sim.h, sim._stream()
    poison = 0x7fc0dead
    buf = torch.full((64, N), poison, dtype=torch.int32, device=sim.device)
    p = buf.data_ptr()
    fwd = lambda **over: lib.ForwardIO(**{**dict(qpos_dev=p, qvel_dev=p, flags=lib.F_CONTACT5, solver_iters=64, contact_iters=64, qacc_dev=p, ncon_dev=p), **over})
    call = lambda io, M=N: L.so100_query_forward(h, C.byref(io), M, st)
    calls = [
        (lambda: L.so100_query_forward(h, None, N, st), b"so100_query_forward: null argument"),
        (lambda: L.so100_query_forward(None, C.byref(fwd()), N, st), b"so100_query_forward: null argument"),
        (lambda: call(fwd(), 0), b"so100_query_forward: M must be >= 1, got 0"),
        (lambda: call(fwd(qpos_dev=None, qvel_dev=None), N - 1), b"so100_query_forward: M must be the handle's N (65) where its state is read, got 64"),
        (lambda: call(fwd(qpos_dev=None)), b"so100_query_forward: qvel_dev given without qpos_dev"),
        (lambda: call(fwd(flags=256)), b"so100_query_forward: unknown flag bits"),
        (lambda: call(fwd(flags=lib.F_CONTACT5 | lib.F_CUBE_PINNED)),
         b"so100_query_forward: SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)"),
        (lambda: call(fwd(flags=lib.F_LINKS_CUBE | lib.F_CUBE_PINNED)),
         b"so100_query_forward: SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)"),
        (lambda: call(fwd(solver_iters=0)), b"so100_query_forward: solver_iters must be in 1..64, got 0"),
        (lambda: call(fwd(solver_iters=65)), b"so100_query_forward: solver_iters must be in 1..64, got 65"),
        (lambda: call(fwd(contact_iters=0)), b"so100_query_forward: contact_iters must be in 1..64, got 0"),
        (lambda: call(fwd(contact_iters=65)), b"so100_query_forward: contact_iters must be in 1..64, got 65"),
        (lambda: call(fwd(qacc_dev=None, ncon_dev=None)), b"so100_query_forward: no output requested"),
        # the order: the earlier check answers when two apply
        (lambda: call(fwd(qpos_dev=None, flags=256, solver_iters=0)), b"so100_query_forward: qvel_dev given without qpos_dev"),
        (lambda: call(fwd(flags=256, solver_iters=0, qacc_dev=None, ncon_dev=None)), b"so100_query_forward: unknown flag bits"),
        (lambda: call(fwd(solver_iters=0, qacc_dev=None, ncon_dev=None)), b"so100_query_forward: solver_iters must be in 1..64, got 0"),
    ]
    current = torch.cuda.current_device()
    for fn, msg in calls:
        assert fn() == -1, msg
        assert L.so100_last_error() == msg
        assert torch.cuda.current_device() == current
    torch.cuda.synchronize()
    assert (buf == poison).all()                                 # nothing was enqueued
    assert torch.isfinite(sim.forward()["qacc"]).all()


def test_graph_capture(sim):
    """nothing allocates, frees or synchronises: one call captured on one stream, replayed, equals the direct call bit for bit"""
    from so100_mujoco_rl_amd import lib
    fam = S.family("floor_cube")
    M = 65
    qs, vs, us = (dev(getattr(fam, a)[:M].T, sim) for a in ("qpos", "qvel", "ctrl"))
    out = {k: torch.zeros(n, M, dtype=torch.float32, device=sim.device) for k, n in (("qacc", 12), ("force", 60), ("pad", 8))}
    ncon = torch.zeros(M, dtype=torch.int32, device=sim.device)
    io = lib.ForwardIO(qpos_dev=qs.data_ptr(), qvel_dev=vs.data_ptr(), ctrl_dev=us.data_ptr(), flags=fam.flags, solver_iters=64, contact_iters=64,
                       qacc_dev=out["qacc"].data_ptr(), ncon_dev=ncon.data_ptr(), con_force_dev=out["force"].data_ptr(), pad_force_dev=out["pad"].data_ptr())
    side = torch.cuda.Stream(device=sim.device)
    side.wait_stream(torch.cuda.current_stream(sim.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert sim.L.so100_query_forward(sim.h, C.byref(io), M, side.cuda_stream) == 0
    torch.cuda.current_stream(sim.device).wait_stream(side)
    for t in out.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    direct = host(sim.forward(dev(fam.qpos[:M], sim), dev(fam.qvel[:M], sim), dev(fam.ctrl[:M], sim), flags=fam.flags))
    assert out["qacc"].t().contiguous().cpu().numpy().tobytes() == direct["qacc"].tobytes()
    assert out["pad"].t().contiguous().cpu().numpy().tobytes() == direct["pad_force"].tobytes()
    assert out["force"].view(S.MAXCON, 3, M).permute(2, 0, 1).contiguous().cpu().numpy().tobytes() == direct["contacts"]["force"].tobytes()
    assert (ncon.cpu().numpy() == direct["ncon"]).all() and direct["ncon"].any()


def test_grasp_probe_end_to_end():
    """examples/grasp_probe.py on 64 envs: no jaw reports force at reset, both jaws report force at some step"""
    spec = importlib.util.spec_from_file_location("grasp_probe", os.path.join(ROOT, "examples", "grasp_probe.py"))
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    log = probe.run(64, 12)
    assert not log[0]["held"].any() and log[0]["fixed"].max() == 0 and log[0]["moving"].max() == 0
    assert any(row["held"].any() for row in log[1:])
    print(f"[forward-tol] grasp probe: held per step {[int(row['held'].sum()) for row in log]}")
