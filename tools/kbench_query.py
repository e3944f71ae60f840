#!/usr/bin/env python3
"""Time the model queries (include/so100_query.h) with HIP events, through the C ABI on preallocated buffers (needs a GPU).

    python tools/kbench_query.py [--out profiles/query_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --forward [--out profiles/forward_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --trajectory [--out profiles/trajectory_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --derivatives [--out profiles/derivatives_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --lqr [--form mfma] [--out profiles/lqr_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --lqr-reg [--out profiles/lqr_reg_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --closed-loop [--form global] [--out profiles/closed_loop_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --cost [--out profiles/cost_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --mppi [--out profiles/mppi_kbench.json] [--commit LABEL] [--rounds 5]
    python tools/kbench_query.py --cem [--out profiles/cem_kbench.json] [--commit LABEL] [--rounds 5]

Cases, at M = 4096 and M = 1 048 576 problems: kinematics with every output and with the end-effector point alone, the Jacobian (jacp and
jacr), the dynamics (M, bias and tau) and the IK.  Poses are uniform over the joint ranges; the IK problems are the 400 of the tests' recipe
(tests/query_support.py: a reachable target, a start up to 0.3 rad away, the default parameters) repeated to fill M.  The cases are timed
in alternation, `--rounds` times each; a figure is the median of the rounds, one round the mean over its calls.  There is nothing to
compare against: the file is a record, not a gate.

--forward times the forward-dynamics query (so100_query_forward, every output, 64 / 64 iterations) instead, at M = 4096 and M = 262 144, on
three populations: poses drawn uniformly over the joint ranges and kept where no arm geom touches anything (the cube rests on the floor), the
pad/floor states of the tests' recipe (tests/forward_support.py: family "floor") and its coupled states (family "floor_cube" and the states of
"grasp" that are in contact), each repeated to fill M.  Beside each figure stands one so100_step of a handle of M envs with frame_skip = 1 and
the same flags and iteration counts, its state set to the same states before every call.  The two are timed alike (timed_pairs: an event pair
round each single call, the set_state copies outside the span, the calls enqueued without waiting); the forward query's back-to-back time,
one event pair round all calls of a round, is recorded as well:
the existing code doing the same solve from the warm-start rows of its state, plus the integration and the task layer.

--trajectory times the trajectory query (so100_query_trajectory) at M = 4096 and M = 262 144, T = 16 control steps of 16 substeps, per flag set
beside the 16 so100_step calls it predicts (trajectory_main).

--derivatives times the derivatives query (so100_query_derivatives) at M = 4096 and M = 65 536, nsub = 16, per form of the kernel, beside what a
user did before it existed: the same 61 M evaluations through so100_query_trajectory (T = 1, the final rows alone) with the perturbed copies
built and the results differenced in torch (derivatives_main).

--lqr times the LQR query (so100_query_lqr, every output, with nominal controls and bounds) at M in {8, 4096}, T in {8, 64}, both nx, beside what
a user did before it existed: the backward and forward loops of examples/ilqr_reach.py in torch, on identical inputs (lqr_main).  --form labels
the cases with the form of the kernel the loaded library holds (SO100_LIB=<a side build with -DSO100_LQR_VALU=1> --form valu); the cases of
other forms already in the output file are kept.

--closed-loop times the closed-loop trajectory query (so100_query_closed_loop; u, qpos, qvel, ee and bad_step asked for) at (M, L, T) in {(8, 8, 8),
(4096, 8, 8), (4096, 8, 64), (65536, 1, 16)}, nsub = 16, both nx, beside what a user did before it existed: T calls of so100_query_trajectory (T = 1)
on M L problems with the feedback law in torch between them (closed_loop_main).  --form labels the cases with how the loaded library's kernel
reads its gains (global: the product; lds: SO100_LIB=<a side build with -DSO100_CL_LDS=1> --form lds).

--cost times the two cost queries (so100_query_cost_terms with every output; so100_query_cost_select with every output at L = 8) at (M, T) in {(8, 8),
(4096, 8), (4096, 64)}, both nx for the terms, beside what examples/ilqr_reach.py did before they existed: So100Sim.jacobian plus the einsums, zero
fills and cats for the terms; the torch sum, mask, argmin and gather for the selection (cost_main).

--mppi times the two sampling-planner queries (so100_query_plan_sample and so100_query_cost_blend, every output) at (N, K, T) in {(8, 64, 8), (8, 256, 8),
(512, 256, 16)} beside the torch arithmetic of examples/mppi_reach.py for the same job, and at the first two sizes the whole planning step: the three
queries against the example's torch path around the same trajectory call (mppi_main).

--cem times so100_query_plan_sample_tv against so100_query_plan_sample on equal inputs and so100_query_cost_refit (every output, E = K / 8) against the torch
arithmetic for the same job at (N, K, T) in {(8, 64, 8), (8, 256, 8), (512, 256, 16), (1, 4096, 1)}, and at the first two sizes a whole CEM round both ways
(cem_main)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402
import torch          # noqa: E402

from so100_mujoco_rl_amd import lib   # noqa: E402
import query_support as S             # noqa: E402

SIZES = [(4096, 200), (1 << 20, 10)]          # (M, calls per timed round)


FORWARD_SIZES = [(4096, 200), (262144, 20)]     # (M, calls per timed round)


def forward_populations(sim):
    """{name: (flags, qpos [n, 13], qvel [n, 12], ctrl [n, 6])}, float32"""
    import forward_support as F
    import scenes
    rs = np.random.RandomState(0)
    rng = S.joint_range()
    n = 1 << 16
    qpos = np.zeros((n, 13), np.float32); qpos[:, :6] = rs.uniform(rng[:, 0], rng[:, 1], (n, 6)); qpos[:, 6:9] = [0.15, -0.25, 0.0099]; qpos[:, 9] = 1.0
    qvel = np.zeros((n, 12), np.float32); qvel[:, :6] = rs.randn(n, 6)*0.3
    ctrl = (qpos[:, :6] + rs.uniform(-1, 1, (n, 6))*0.075).astype(np.float32)
    t = lambda x: torch.from_numpy(x).to(sim.device)
    con = sim.forward(t(qpos), t(qvel), t(ctrl), flags=lib.F_REFERENCE)["contacts"]
    free = ~((con["kind"] > 0).any(dim=1)).cpu().numpy()
    floor, cube, grasp = F.family("floor"), F.family("floor_cube"), F.family("grasp")
    touching = np.array([r["ncon"] > 0 for r in grasp.refs])
    both = lambda a: np.concatenate([getattr(cube, a), getattr(grasp, a)[touching]])
    return {"free": (lib.F_REFERENCE, qpos[free], qvel[free], ctrl[free]),
            "pad_floor": (scenes.REFP, floor.qpos, floor.qvel, floor.ctrl),
            "coupled": (scenes.C5, both("qpos"), both("qvel"), both("ctrl"))}


def forward_main(a):
    probe = lib.So100Sim(lib.ENV01, 64, device="cuda:0", flags=lib.F_REFERENCE, seed=0)
    pops = forward_populations(probe)
    dev, L = probe.device, probe.L
    doc = {"what": "HIP-event time per call of so100_query_forward (every output, 64 / 64 iterations) and of one so100_step with frame_skip = 1 on the "
                   "same states, flags and iteration counts, both as an event pair round each single call; forward also back to back; medians of alternated rounds", "commit": a.commit, "card": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "cases": []}
    for M, reps in FORWARD_SIZES:
        for name, (flags, qpos, qvel, ctrl) in pops.items():
            idx = np.arange(M) % len(qpos)
            soa = lambda x: torch.from_numpy(np.ascontiguousarray(x[idx].T, np.float32)).to(dev)
            qs, vs, us_ = soa(qpos), soa(qvel), soa(ctrl)
            act = ((us_[:6] - qs[:6])/0.075).t().contiguous()          # Env01: ctrl = q + 0.075 action
            out = torch.empty(12 + 12 + 8 + 1 + 20*(3 + 9 + 1 + 3), M, dtype=torch.float32, device=dev)
            ints = torch.empty(2 + 40, M, dtype=torch.int32, device=dev)
            p, pi = (lambda r: out[r].data_ptr()), (lambda r: ints[r].data_ptr())
            io = lib.ForwardIO(qs.data_ptr(), vs.data_ptr(), us_.data_ptr(), flags, 64, 64, p(0), p(12), pi(0), pi(1), pi(2), pi(22), p(33), p(93), p(273), p(293), p(24), p(32))
            sim = lib.So100Sim(lib.ENV01, M, device="cuda:0", flags=flags, solver_iters=64, contact_iters=64, frame_skip=1, max_episode_steps=0, seed=0)
            sim.reset()
            st = sim._stream()

            def timed_forward(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    rc = L.so100_query_forward(sim.h, C.byref(io), M, st)
                    assert rc == 0, L.so100_last_error()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)*1e3/n

            def timed_pairs(call, n):
                """forward and step timed alike: n times {set_state copies, event, ONE call, event}, enqueued without waiting, one synchronise at
                the end; the sum of the n event spans.  (A step moves the state, so its calls cannot run back to back on the same states.)"""
                pairs = []
                for _ in range(n):
                    sim.set_state(qs, vs)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); call(); e1.record()
                    pairs.append((e0, e1))
                torch.cuda.synchronize()
                return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

            def one_forward():
                rc = L.so100_query_forward(sim.h, C.byref(io), M, st)
                assert rc == 0, L.so100_last_error()

            one_step = lambda: sim.step(act)
            timed_forward(a.warmup); timed_pairs(one_forward, a.warmup); timed_pairs(one_step, a.warmup)
            fw, fp, sp = [], [], []
            for _ in range(a.rounds):
                fw.append(timed_forward(reps)); fp.append(timed_pairs(one_forward, reps)); sp.append(timed_pairs(one_step, reps))
            ncon = ints[0].float()
            med, medp, meds = statistics.median(fw), statistics.median(fp), statistics.median(sp)
            case = {"case": name, "M": M, "flags": int(flags), "states": int(len(qpos)), "forward_back_to_back_us_per_call": round(med, 2),
                    "forward_us_per_call": round(medp, 2), "step_us_per_call": round(meds, 2), "forward_over_step": round(medp/meds, 3),
                    "forward_back_to_back_rounds_us": [round(x, 2) for x in fw], "forward_rounds_us": [round(x, 2) for x in fp],
                    "step_rounds_us": [round(x, 2) for x in sp],
                    "calls_per_round": reps, "problems_per_s": round(M/(med*1e-6), 1), "mean_ncon": round(ncon.mean().item(), 3),
                    "share_in_contact": round((ncon > 0).float().mean().item(), 4), "worst_residual": float(out[32].max().item())}
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
            sim.close()
            del out, ints
    probe.close()
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


TRAJECTORY_SIZES = [(4096, 20), (262144, 3)]     # (M, timed units per round)
TRAJECTORY_T, TRAJECTORY_NSUB = 16, 16
# (name, the handle's flags, the query's flags): the contact-disabled sets with a compile-time form of the kernel, each beside a query that simulates
# the same thing through the run-time-flags form (SO100_F_FLOOR acts on the cube alone, which SO100_F_CUBE_PINNED holds still; a handle refuses the
# pair, a query's flags are its own), then the sets with a dynamic cube
_FREE, _ROWS = lib.F_CUBE_PINNED, lib.F_FRICTIONLOSS | lib.F_LIMITS | lib.F_CUBE_PINNED
TRAJECTORY_FLAGS = [("free", _FREE, _FREE), ("free_runtime_form", _FREE, _FREE | lib.F_FLOOR),
                    ("contact_disabled", _ROWS, _ROWS), ("contact_disabled_runtime_form", _ROWS, _ROWS | lib.F_FLOOR),
                    ("nopads", lib.F_NOPADS, lib.F_NOPADS), ("reference", lib.F_REFERENCE, lib.F_REFERENCE)]
# (F_NOPADS has a compile-time form too; no other flag set simulates the same thing, so its run-time-form figure is the one measured before the form was added: DESIGN.md 13.4)


def trajectory_main(a):
    """One so100_query_trajectory call (the handle's state, mode = actions, every output) against the T so100_step calls it predicts, on a handle
    of M Env01 envs after a reset and a few random steps, with the same flags and iteration counts.  Both are timed with forward_main's
    per-call protocol: the state put back outside the span, an event pair round each single call, enqueued without waiting; a step figure
    is the sum of its T spans."""
    T, nsub = TRAJECTORY_T, TRAJECTORY_NSUB
    doc = {"what": f"HIP-event time of one so100_query_trajectory call (T = {T}, nsub = {nsub}, the handle's state, actions, every output) and of the "
                   f"{T} so100_step calls (frame_skip = {nsub}) it predicts, the shipped (2, 20) iterations; an event pair round each single call, "
                   "medians of alternated rounds", "commit": a.commit, "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    for M, reps in TRAJECTORY_SIZES:
        for name, flags, qflags in TRAJECTORY_FLAGS:
            sim = lib.So100Sim(lib.ENV01, M, device="cuda:0", flags=flags, frame_skip=nsub, max_episode_steps=0, seed=0)
            dev, L, st = sim.device, sim.L, sim._stream()
            sim.reset()
            g = torch.Generator(device=dev).manual_seed(0)
            for _ in range(3):
                sim.step(torch.rand(M, 6, generator=g, device=dev)*2 - 1)
            qs, vs = sim.get_state()
            act = torch.rand(T, M, 6, generator=g, device=dev)*2 - 1
            us_ = act.permute(0, 2, 1).contiguous()
            out = torch.empty(T*(13 + 12 + 3 + 1) + 25, M, dtype=torch.float32, device=dev)
            ints = torch.empty(3*T + 1, M, dtype=torch.int32, device=dev)
            p, pi = (lambda r: out[r].data_ptr()), (lambda r: ints[r].data_ptr())
            io = lib.TrajectoryIO(None, None, us_.data_ptr(), lib.TRAJ_MODES["actions"], T, nsub, qflags, sim.cfg.solver_iters, sim.cfg.contact_iters,
                                  p(0), p(13*T), p(25*T), p(29*T), p(29*T + 13), pi(0), pi(T), pi(2*T), p(28*T), pi(3*T))

            def pair(call):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record()
                return e0, e1

            def one_query():
                rc = L.so100_query_trajectory(sim.h, C.byref(io), M, st)
                assert rc == 0, L.so100_last_error()

            def timed_query(n):
                pairs = []
                for _ in range(n):
                    sim.set_state(qs, vs)
                    pairs.append(pair(one_query))
                torch.cuda.synchronize()
                return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

            def timed_steps(n):
                pairs = []
                for _ in range(n):
                    sim.set_state(qs, vs)
                    pairs += [pair(lambda t=t: sim.step(act[t])) for t in range(T)]
                torch.cuda.synchronize()
                return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

            timed_query(1); timed_steps(1)
            tq, ts = [], []
            for _ in range(a.rounds):
                tq.append(timed_query(reps)); ts.append(timed_steps(reps))
            sim.set_state(qs, vs); one_query(); torch.cuda.synchronize()
            ncon = ints[0:T].float()
            mq, ms = statistics.median(tq), statistics.median(ts)
            case = {"case": name, "M": M, "flags": int(flags), "query_flags": int(qflags), "T": T, "nsub": nsub, "trajectory_us_per_call": round(mq, 1), "steps_us_per_T_calls": round(ms, 1),
                    "trajectory_over_steps": round(mq/ms, 3), "trajectory_rounds_us": [round(x, 1) for x in tq], "steps_rounds_us": [round(x, 1) for x in ts],
                    "units_per_round": reps, "problem_substeps_per_s": round(M*T*nsub/(mq*1e-6), 1),
                    "share_of_steps_in_contact": round((ncon > 0).float().mean().item(), 4), "bad_problems": int((ints[3*T] >= 0).sum().item())}
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
            sim.close()
            del out, ints
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


DERIVATIVES_SIZES = [(4096, 20), (65536, 4)]     # (M, timed units per round)
DERIVATIVES_NSUB = 16
# (name, flags): the three compile-time forms <8>, <11>, <7> and F_REFERENCE through <-1>
DERIVATIVES_FLAGS = [("free", _FREE), ("contact_disabled", _ROWS), ("nopads", lib.F_NOPADS), ("reference_runtime_form", lib.F_REFERENCE)]


def _quat_mul(a, b):
    return torch.stack([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                        a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]])


def emulated_derivatives(sim, qs, vs, us_, nsub, flags, eps, io_out):
    """What a user did before the query existed, on SoA arrays [k][M]: 61 copies of every problem (copy r M + i: role r of problem i), 60 of them
    perturbed, through so100_query_trajectory with T = 1 and the final rows alone, then the tangent difference in torch.  Returns (A [24][24][M]
    row-major in the leading indices, B [24][6][M])."""
    M = qs.shape[1]
    Q, V, U = qs.repeat(1, 61), vs.repeat(1, 61), us_.repeat(1, 61)
    sn, cs = float(np.sin(0.5*eps)), float(np.cos(0.5*eps))
    for c in range(30):
        for s, d in ((0, eps), (1, -eps)):
            sl = slice((2*c + s)*M, (2*c + s + 1)*M)
            if c < 9:
                Q[c, sl] += d
            elif c < 12:
                r = torch.zeros(4, 1, device=qs.device); r[0] = cs; r[1 + c - 9] = sn if s == 0 else -sn
                q = _quat_mul(Q[9:13, sl], r)
                Q[9:13, sl] = q/q.norm(dim=0, keepdim=True)
            elif c < 24:
                V[c - 12, sl] += d
            else:
                U[c - 24, sl] += d
    qf, vf = io_out(61*M)
    io = lib.TrajectoryIO(Q.data_ptr(), V.data_ptr(), U.data_ptr(), lib.TRAJ_MODES["actions"], 1, nsub, flags, sim.cfg.solver_iters, sim.cfg.contact_iters,
                          None, None, None, qf.data_ptr(), vf.data_ptr(), None, None, None, None, None)
    rc = sim.L.so100_query_trajectory(sim.h, C.byref(io), 61*M, sim._stream())
    assert rc == 0, sim.L.so100_last_error()
    qp, qm = qf[:, :60*M].reshape(13, 30, 2, M)[:, :, 0], qf[:, :60*M].reshape(13, 30, 2, M)[:, :, 1]
    vp, vm = vf[:, :60*M].reshape(12, 30, 2, M)[:, :, 0], vf[:, :60*M].reshape(12, 30, 2, M)[:, :, 1]
    r = 0.5/eps
    dq = _quat_mul(torch.stack([qm[9], -qm[10], -qm[11], -qm[12]]), qp[9:13])
    s_ = dq[1:].norm(dim=0)
    ang = 2.0*torch.atan2(s_, dq[0]); ang = torch.where(ang > np.pi, ang - 2.0*np.pi, ang)
    rot = dq[1:]*torch.where(s_ < 1e-15, torch.zeros_like(s_), ang/s_)
    AB = torch.cat([(qp[:9] - qm[:9])*r, rot*r, (vp - vm)*r])          # [24][30][M]
    return AB[:, :24], AB[:, 24:]


def derivatives_main(a):
    """One so100_query_derivatives call (explicit states, mode = actions, every output, the default eps) against the emulation through
    so100_query_trajectory, on the states of a handle of M Env01 envs after a reset and a few random steps.  An event pair round each unit,
    enqueued without waiting; the emulation's trajectory call is timed on its own as well."""
    nsub, eps = DERIVATIVES_NSUB, lib.DERIV_EPS
    doc = {"what": f"HIP-event time of one so100_query_derivatives call (nsub = {nsub}, explicit states, actions, every output, eps = {eps}) and of the "
                   "emulation a user needed before it: 61 M problems built in torch, one so100_query_trajectory call (T = 1, final rows alone), the tangent "
                   "difference in torch; the shipped (2, 20) iterations; an event pair round each unit, medians of alternated rounds",
           "commit": a.commit, "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    for M, reps in DERIVATIVES_SIZES:
        for name, flags in DERIVATIVES_FLAGS:
            sim = lib.So100Sim(lib.ENV01, M, device="cuda:0", flags=flags, frame_skip=nsub, max_episode_steps=0, seed=0)
            dev, L, st = sim.device, sim.L, sim._stream()
            sim.reset()
            g = torch.Generator(device=dev).manual_seed(0)
            for _ in range(3):
                sim.step(torch.rand(M, 6, generator=g, device=dev)*2 - 1)
            qs, vs = (t.contiguous() for t in sim.get_state())
            us_ = (torch.rand(M, 6, generator=g, device=dev)*2 - 1).t().contiguous()
            A = torch.empty(M, 24, 24, dtype=torch.float32, device=dev); B = torch.empty(M, 24, 6, dtype=torch.float32, device=dev)
            nxt = torch.empty(25, M, dtype=torch.float32, device=dev); bad = torch.empty(M, dtype=torch.int32, device=dev)
            io = lib.DerivativesIO(qs.data_ptr(), vs.data_ptr(), us_.data_ptr(), lib.TRAJ_MODES["actions"], nsub, flags, sim.cfg.solver_iters, sim.cfg.contact_iters,
                                   eps, A.data_ptr(), B.data_ptr(), nxt[0].data_ptr(), nxt[13].data_ptr(), bad.data_ptr())
            fin = torch.empty(25, 61*M, dtype=torch.float32, device=dev)
            io_out = lambda n: (fin[:13], fin[13:])
            spans = {}

            def pair(call):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record()
                return e0, e1

            def one_query():
                rc = L.so100_query_derivatives(sim.h, C.byref(io), M, st)
                assert rc == 0, L.so100_last_error()

            def one_emulation():
                spans["AB"] = emulated_derivatives(sim, qs, vs, us_, nsub, flags, eps, io_out)

            def timed(call, n):
                pairs = [pair(call) for _ in range(n)]
                torch.cuda.synchronize()
                return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

            timed(one_query, 1); timed(one_emulation, 1)
            tq, te = [], []
            for _ in range(a.rounds):
                tq.append(timed(one_query, reps)); te.append(timed(one_emulation, max(1, reps//4)))
            Ae, Be = spans["AB"]
            diff = max((A - Ae.permute(2, 0, 1)).abs().max().item(), (B - Be.permute(2, 0, 1)).abs().max().item())
            mq, me = statistics.median(tq), statistics.median(te)
            case = {"case": name, "M": M, "flags": int(flags), "nsub": nsub, "derivatives_us_per_call": round(mq, 1), "emulation_us": round(me, 1),
                    "derivatives_over_emulation": round(mq/me, 3), "derivatives_rounds_us": [round(x, 1) for x in tq], "emulation_rounds_us": [round(x, 1) for x in te],
                    "units_per_round": reps, "evaluations_per_s": round(61*M/(mq*1e-6), 1), "problem_substeps_per_s": round(61*M*nsub/(mq*1e-6), 1),
                    "largest_difference_to_emulation": diff, "bad_problems": int(bad.sum().item())}
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
            sim.close()
            del fin, A, B, spans
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


LQR_SIZES = [(8, 8, 50, 5), (8, 64, 20, 3), (4096, 8, 20, 3), (4096, 64, 5, 2)]       # (M, T, query calls, torch loops per timed round)
LQR_ARM = list(range(0, 6)) + list(range(12, 18))


def torch_lqr(A, B, lx, lxx, lu, luu, reg, U):
    """the loops of examples/ilqr_reach.py (backward pass, then the clamped linear forward pass) on A [T, M, n, n], B [T, M, n, 6], lx [T + 1, M, n],
    lxx [T + 1, M, n, n], lu [T, M, 6], luu [6, 6], the plan U [T, M, 6]: (k, K, du)"""
    T, M, n = A.shape[0], A.shape[1], A.shape[2]
    dev = A.device
    eye = torch.eye(6, device=dev)
    Vx, Vxx = lx[T], lxx[T]
    k = torch.zeros(T, M, 6, device=dev); K = torch.zeros(T, M, 6, n, device=dev)
    for t in range(T - 1, -1, -1):
        At, Bt = A[t], B[t]
        Qx = lx[t] + torch.einsum("nij,ni->nj", At, Vx)
        Qu = lu[t] + torch.einsum("nij,ni->nj", Bt, Vx)
        VA = Vxx @ At
        Qxx = lxx[t] + At.transpose(1, 2) @ VA
        Qux = Bt.transpose(1, 2) @ VA
        Quu = Bt.transpose(1, 2) @ Vxx @ Bt + luu
        Quu_r = Quu + reg*eye
        k[t] = -torch.linalg.solve(Quu_r, Qu[..., None])[..., 0]
        K[t] = -torch.linalg.solve(Quu_r, Qux)
        Vx = Qx + torch.einsum("nij,ni->nj", K[t], Qu + torch.einsum("nij,nj->ni", Quu, k[t])) + torch.einsum("nij,ni->nj", Qux, k[t])
        Vxx = Qxx + K[t].transpose(1, 2) @ Quu @ K[t] + K[t].transpose(1, 2) @ Qux + Qux.transpose(1, 2) @ K[t]
        Vxx = 0.5*(Vxx + Vxx.transpose(1, 2))
    dx = torch.zeros(M, n, device=dev)
    du = torch.zeros(T, M, 6, device=dev)
    for t in range(T):
        du[t] = (U[t] + k[t] + torch.einsum("nij,nj->ni", K[t], dx)).clamp(-1.0, 1.0) - U[t]
        dx = torch.einsum("nij,nj->ni", A[t], dx) + torch.einsum("nij,nj->ni", B[t], du[t])
    return k, K, du


def lqr_main(a):
    """One so100_query_lqr call (every output, nominal controls with bounds) against torch_lqr on the same inputs: seeded synthetic problems of the
    tests' family S (A = I + 0.3 N / sqrt(n), B = 0.3 N, lxx = C C' + 0.1 I, lx, lu = N, luu = 0.2 I, no cross term, reg = 1e-5).  An event pair round
    each unit, enqueued without waiting."""
    sim = lib.So100Sim(lib.ENV01, 8, device="cuda:0", flags=lib.F_CUBE_PINNED, seed=0)
    dev, L, st = sim.device, sim.L, sim._stream()
    doc = {"what": "HIP-event time of one so100_query_lqr call (every output, u with bounds) and of the torch loops of examples/ilqr_reach.py (backward pass "
                   "and clamped forward pass; the arm block sliced beforehand, outside the span) on identical inputs; an event pair round each unit, medians of "
                   "alternated rounds; `form`: the kernel's products on the matrix instruction (mfma) or as plain FMA loops (valu, a side build)",
           "commit": a.commit, "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    if os.path.exists(a.out):
        doc["cases"] = [c for c in json.load(open(a.out)).get("cases", []) if c.get("form") != a.form]
    reg = 1e-5
    for nx in (12, 24):
        for M, T, reps, loops in LQR_SIZES:
            g = torch.Generator(device=dev).manual_seed(0)
            rn = lambda *shape: torch.randn(*shape, generator=g, device=dev)
            A = torch.eye(24, device=dev) + 0.3*rn(T, M, 24, 24)/nx**0.5
            B = 0.3*rn(T, M, 24, 6)
            Cm = rn(T + 1, M, nx, nx)/nx**0.5
            lxx = (Cm @ Cm.transpose(2, 3) + 0.1*torch.eye(nx, device=dev)).contiguous()
            del Cm
            lx, lu = rn(T + 1, M, nx), rn(T, M, 6)
            luu1 = 0.2*torch.eye(6, device=dev)
            luu = luu1.expand(T, M, 6, 6).contiguous()
            U = torch.zeros(T, M, 6, device=dev)
            out = {"k": (T, M, 6), "K": (T, M, 6, nx), "Vx0": (M, nx), "Vxx0": (M, nx, nx), "dV": (M, 2), "du": (T, M, 6), "dx": (T + 1, M, nx)}
            out = {k: torch.empty(*shape, dtype=torch.float32, device=dev) for k, shape in out.items()}
            bad = torch.empty(M, dtype=torch.int32, device=dev)
            io = lib.LqrIO(nx, T, A.data_ptr(), B.data_ptr(), lx.data_ptr(), lxx.data_ptr(), lu.data_ptr(), luu.data_ptr(), None, U.data_ptr(), None, reg, 1.0, -1.0, 1.0,
                           *[out[k].data_ptr() for k in ("k", "K", "Vx0", "Vxx0", "dV", "du", "dx")], bad.data_ptr())
            idx = LQR_ARM if nx == 12 else list(range(24))
            As = A[:, :, idx][:, :, :, idx].contiguous() if nx == 12 else A
            Bs = B[:, :, idx].contiguous() if nx == 12 else B
            spans = {}

            def pair(call):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record()
                return e0, e1

            def one_query():
                rc = L.so100_query_lqr(sim.h, C.byref(io), M, st)
                assert rc == 0, L.so100_last_error()

            def one_torch():
                spans["r"] = torch_lqr(As, Bs, lx, lxx, lu, luu1, reg, U)

            def timed(call, n):
                pairs = [pair(call) for _ in range(n)]
                torch.cuda.synchronize()
                return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

            timed(one_query, 2); timed(one_torch, 1)
            tq, tt = [], []
            for _ in range(a.rounds):
                tq.append(timed(one_query, reps)); tt.append(timed(one_torch, loops))
            kt, Kt, dut = spans["r"]
            diff = {"k": (out["k"] - kt).abs().max().item(), "K": (out["K"] - Kt).abs().max().item(), "du": (out["du"] - dut).abs().max().item()}
            mq, mt = statistics.median(tq), statistics.median(tt)
            words = T*M*(576 + 144 + nx*nx + nx + 6 + 36 + 6) + M*(nx*nx + nx) + T*M*(6 + 6*nx)*2 + T*M*(6 + nx)
            case = {"form": a.form, "nx": nx, "M": M, "T": T, "lqr_us_per_call": round(mq, 1), "torch_loops_us": round(mt, 1), "lqr_over_torch": round(mq/mt, 4),
                    "lqr_rounds_us": [round(x, 1) for x in tq], "torch_rounds_us": [round(x, 1) for x in tt], "units_per_round": [reps, loops],
                    "problem_steps_per_s": round(M*T/(mq*1e-6), 1), "GB_per_s": round(words*4/(mq*1e-6)/1e9, 1),
                    "largest_difference_to_torch": {k: float(f"{v:.3e}") for k, v in diff.items()}, "bad_problems": int((bad >= 0).sum().item())}
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
            del A, B, lxx, lx, lu, luu, out, As, Bs, spans
    sim.close()
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def lqr_reg_main(a):
    """so100_query_lqr_reg and so100_query_reg_schedule at lqr_main's shapes and inputs, in three parts.  (a) lqr_reg with tries = 1 and no reg_dev
    against lqr: the same work through the REG kernel.  (b) every fourth problem made to need four passes (lqr_support's indefinite case: luu = -I,
    B a tenth at the middle step; reg 0 -> 0.125 -> 0.5 -> 2), one lqr_reg call with tries = 4 against what a caller does today: a call, a readback of
    bad on the host, and three more whole-batch calls under the raised regs.  (c) reg_schedule against the same arithmetic in torch.  An event pair
    round each unit; (b)'s baseline has a host synchronisation inside its span, which is part of what it costs."""
    sim = lib.So100Sim(lib.ENV01, 8, device="cuda:0", flags=lib.F_CUBE_PINNED, seed=0)
    dev, L, st = sim.device, sim.L, sim._stream()
    knobs = dict(reg_min=0.125, reg_max=32.0, reg_up=4.0)
    doc = {"what": "HIP-event times of so100_query_lqr_reg and so100_query_reg_schedule; an event pair round each unit, medians of alternated rounds.  "
                   "(a) lqr_reg with tries = 1 against lqr on identical inputs; (b) a quarter of the problems needing four passes: one lqr_reg call against "
                   "a lqr call, a readback of bad and three more whole-batch lqr calls; (c) reg_schedule against the same arithmetic in torch",
           "commit": a.commit, "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "knobs": dict(knobs, tries=4), "same_work": [], "retry": [], "schedule": []}

    def pair(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        return e0, e1

    def timed(call, n):
        pairs = [pair(call) for _ in range(n)]
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

    def rounds(one, other, reps):
        timed(one, 2); timed(other, 2)
        t1, t2 = [], []
        for _ in range(a.rounds):
            t1.append(timed(one, reps)); t2.append(timed(other, reps))
        return t1, t2

    us = lambda xs: [round(x, 1) for x in xs]
    for nx in (12, 24):
        for M, T, reps, _ in LQR_SIZES:
            g = torch.Generator(device=dev).manual_seed(0)
            rn = lambda *shape: torch.randn(*shape, generator=g, device=dev)
            A = torch.eye(24, device=dev) + 0.3*rn(T, M, 24, 24)/nx**0.5
            B = 0.3*rn(T, M, 24, 6)
            Cm = rn(T + 1, M, nx, nx)/nx**0.5
            lxx = (Cm @ Cm.transpose(2, 3) + 0.1*torch.eye(nx, device=dev)).contiguous()
            del Cm
            lx, lu = rn(T + 1, M, nx), rn(T, M, 6)
            luu = (0.2*torch.eye(6, device=dev)).expand(T, M, 6, 6).contiguous()
            U = torch.zeros(T, M, 6, device=dev)
            shapes = {"k": (T, M, 6), "K": (T, M, 6, nx), "Vx0": (M, nx), "Vxx0": (M, nx, nx), "dV": (M, 2), "du": (T, M, 6), "dx": (T + 1, M, nx)}
            new = lambda: {k: torch.empty(*shape, dtype=torch.float32, device=dev) for k, shape in shapes.items()}
            o1, o2 = new(), new()
            bad1, bad2 = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
            used, ran = torch.empty(M, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
            base = lambda o, bad, reg: lib.LqrIO(nx, T, A.data_ptr(), B.data_ptr(), lx.data_ptr(), lxx.data_ptr(), lu.data_ptr(), luu.data_ptr(), None, U.data_ptr(), None,
                                                 reg, 1.0, -1.0, 1.0, *[o[k].data_ptr() for k in ("k", "K", "Vx0", "Vxx0", "dV", "du", "dx")], bad.data_ptr())
            state = {"tries": 1, "reg": 1e-5}

            def one_reg():
                io = lib.LqrRegIO(base(o1, bad1, state["reg"]), None, knobs["reg_min"], knobs["reg_max"], knobs["reg_up"], state["tries"], used.data_ptr(), ran.data_ptr())
                rc = L.so100_query_lqr_reg(sim.h, C.byref(io), M, st)
                assert rc == 0, L.so100_last_error()

            def one_plain(reg=1e-5):
                io = base(o2, bad2, reg)
                rc = L.so100_query_lqr(sim.h, C.byref(io), M, st)
                assert rc == 0, L.so100_last_error()

            # (a) the same work
            tr, tp = rounds(one_reg, one_plain, reps)
            torch.cuda.synchronize()
            equal = all(torch.equal(o1[k], o2[k]) for k in o1) and torch.equal(bad1, bad2)
            mr, mp = statistics.median(tr), statistics.median(tp)
            case = {"nx": nx, "M": M, "T": T, "lqr_reg_us_per_call": round(mr, 1), "lqr_us_per_call": round(mp, 1), "lqr_reg_over_lqr": round(mr/mp, 4),
                    "lqr_reg_rounds_us": us(tr), "lqr_rounds_us": us(tp), "calls_per_round": reps, "outputs_bit_equal": bool(equal)}
            doc["same_work"].append(case)
            print(json.dumps(dict(case, part="a")), flush=True)

            # (b) every fourth problem needs four passes
            at = T//2
            hard = torch.arange(1, M, 4, device=dev)
            luu[at, hard] = -torch.eye(6, device=dev)
            B[at, hard] *= 0.1
            state.update(tries=4, reg=0.0)

            def today():
                one_plain(0.0)
                if bool((bad2 >= 0).any()):                      # the look at the result every caller has to take
                    for reg in (0.125, 0.5, 2.0):
                        one_plain(reg)

            tr, tp = rounds(one_reg, today, reps)
            torch.cuda.synchronize()
            hist = torch.bincount(ran, minlength=5).tolist()
            mr, mp = statistics.median(tr), statistics.median(tp)
            case = {"nx": nx, "M": M, "T": T, "lqr_reg_us_per_call": round(mr, 1), "four_calls_and_a_readback_us": round(mp, 1), "lqr_reg_over_today": round(mr/mp, 4),
                    "lqr_reg_rounds_us": us(tr), "today_rounds_us": us(tp), "units_per_round": reps, "problems_by_passes_run": hist,
                    "bad_problems": [int((bad1 >= 0).sum().item()), int((bad2 >= 0).sum().item())]}
            doc["retry"].append(case)
            print(json.dumps(dict(case, part="b")), flush=True)
            del A, B, lxx, lx, lu, luu, o1, o2
    # (c) the schedule
    for M in sorted({m for m, _, _, _ in LQR_SIZES}):
        g = torch.Generator(device=dev).manual_seed(1)
        reg_used = torch.rand(M, generator=g, device=dev)*40.0 - 4.0
        best = torch.randint(-1, 8, (M,), generator=g, device=dev, dtype=torch.int32)
        reg, imp = torch.empty(M, device=dev), torch.empty(M, dtype=torch.uint8, device=dev)
        io = lib.RegScheduleIO(reg_used.data_ptr(), best.data_ptr(), 0, knobs["reg_min"], knobs["reg_max"], knobs["reg_up"], 0.25, reg.data_ptr(), imp.data_ptr())
        spans = {}

        def one_query():
            rc = L.so100_query_reg_schedule(sim.h, C.byref(io), M, st)
            assert rc == 0, L.so100_last_error()

        def one_torch():
            r = torch.where(torch.isfinite(reg_used) & (reg_used >= 0), reg_used, torch.zeros_like(reg_used))
            improved = (best >= 0) & (best != 0)
            down = r*0.25
            down = torch.where(down < knobs["reg_min"], torch.zeros_like(down), down)
            spans["r"] = torch.where(improved, down, (r*knobs["reg_up"]).clamp(knobs["reg_min"], knobs["reg_max"])), improved

        tq, tt = rounds(one_query, one_torch, 50)
        torch.cuda.synchronize()
        mq, mt = statistics.median(tq), statistics.median(tt)
        case = {"M": M, "reg_schedule_us_per_call": round(mq, 1), "torch_us": round(mt, 1), "reg_schedule_over_torch": round(mq/mt, 4), "reg_schedule_rounds_us": us(tq),
                "torch_rounds_us": us(tt), "units_per_round": 50, "equal_to_torch": bool(torch.equal(reg, spans["r"][0]) and torch.equal(imp.bool(), spans["r"][1]))}
        doc["schedule"].append(case)
        print(json.dumps(dict(case, part="c")), flush=True)
    sim.close()
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


CLOSED_LOOP_SIZES = [(8, 8, 8, 20, 5), (4096, 8, 8, 5, 2), (4096, 8, 64, 2, 1), (65536, 1, 16, 2, 1)]      # (M, L, T, query calls, baseline runs) per round


def torch_tangent_difference(qp, qv, xq, xv):
    """x (-) xref on SoA rows [k][n]: derivative_column with r = 1, in torch"""
    d = torch.empty(24, qp.shape[1], device=qp.device)
    d[:9] = qp[:9] - xq[:9]; d[12:] = qv - xv
    a0, a1, a2, a3 = xq[9], -xq[10], -xq[11], -xq[12]
    b0, b1, b2, b3 = qp[9], qp[10], qp[11], qp[12]
    w = a0*b0 - a1*b1 - a2*b2 - a3*b3
    vec = torch.stack([a0*b1 + a1*b0 + a2*b3 - a3*b2, a0*b2 - a1*b3 + a2*b0 + a3*b1, a0*b3 + a1*b2 - a2*b1 + a3*b0])
    sn = vec.norm(dim=0)
    angle = 2.0*torch.atan2(sn, w)
    angle = torch.where(angle > torch.pi, angle - 2.0*torch.pi, angle)
    d[9:12] = vec*torch.where(sn < 1e-15, torch.zeros_like(sn), angle/sn.clamp_min(1e-30))
    return d


def closed_loop_main(a):
    """One so100_query_closed_loop call against T so100_query_trajectory calls (T = 1, M L problems, final rows and ee) with the law in torch between
    them, on identical inputs: arms around the idle pose under SO100_F_CUBE_PINNED, a seeded plan of actions with its own rollout as the reference, PD-like
    gains (-2 / -0.1 on a joint's own position / velocity column, 0.05 N elsewhere, k = 0.2 N), alpha = 0, 1, 1/2, .., clamp to [-1, 1].  The gains
    repeated per candidate are built outside the baseline's span.  An event pair round each unit, enqueued without waiting."""
    sim = lib.So100Sim(lib.ENV01, 8, device="cuda:0", flags=lib.F_CUBE_PINNED, seed=0)
    dev, L_, st = sim.device, sim.L, sim._stream()
    doc = {"what": "HIP-event time of one so100_query_closed_loop call (u, qpos, qvel, ee, bad_step) and of its emulation: T so100_query_trajectory calls "
                   "(T = 1) on M L problems with the feedback law in torch between them, on identical inputs, nsub = 16, SO100_F_CUBE_PINNED; an event pair round "
                   "each unit, medians of alternated rounds; `form`: the kernel reads its gains from global memory per lane (global) or through a cooperative "
                   "coalesced load into LDS (lds, a side build)",
           "commit": a.commit, "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    if os.path.exists(a.out):
        doc["cases"] = [c for c in json.load(open(a.out)).get("cases", []) if c.get("form") != a.form]
    nsub, flags, iters = 16, lib.F_CUBE_PINNED, (2, 20)
    idle = np.array([0, -1.5, 1.5, 0.5, 0, 0.2, 0.2, -0.2, 0.0099, 1, 0, 0, 0], np.float32)      # tests/scenes.idle_batch: the arm folded above the table
    for nx in (12, 24):
        idx = torch.tensor(list(range(6)) + list(range(12, 18)) if nx == 12 else list(range(24)), device=dev)
        for M, Lc, T, reps, loops in CLOSED_LOOP_SIZES:
            ML = M*Lc
            g = torch.Generator(device=dev).manual_seed(0)
            rn = lambda *shape: torch.randn(*shape, generator=g, device=dev)
            qpos = torch.from_numpy(idle).to(dev)[:, None].repeat(1, M).contiguous()
            qpos[:6] += 0.3*(2*torch.rand(6, M, generator=g, device=dev) - 1)
            qvel = torch.zeros(12, M, device=dev); qvel[:6] = 0.5*(2*torch.rand(6, M, generator=g, device=dev) - 1)
            U = (torch.rand(T, 6, M, generator=g, device=dev) - 0.5).contiguous()
            K = 0.05*rn(T, M, 6, nx)
            for j in range(6):
                K[..., j, j] = -2.0; K[..., j, nx//2 + j] = -0.1
            k = 0.2*rn(T, M, 6)
            alphas = [0.0] + [2.0**-i for i in range(Lc - 1)] if Lc > 1 else [1.0]
            al = (C.c_float*Lc)(*alphas)
            rq, rv = torch.empty(T, 13, M, device=dev), torch.empty(T, 12, M, device=dev)
            tio = lib.TrajectoryIO(qpos_dev=qpos.data_ptr(), qvel_dev=qvel.data_ptr(), ctrl_dev=U.data_ptr(), mode=1, T=T, nsub=nsub, flags=flags, solver_iters=iters[0],
                                   contact_iters=iters[1], qpos_traj_dev=rq.data_ptr(), qvel_traj_dev=rv.data_ptr())
            assert L_.so100_query_trajectory(sim.h, C.byref(tio), M, st) == 0, L_.so100_last_error()
            out = {"u": torch.empty(T, 6, ML, device=dev), "qpos": torch.empty(T, 13, ML, device=dev), "qvel": torch.empty(T, 12, ML, device=dev),
                   "ee": torch.empty(T, 3, ML, device=dev)}
            bad = torch.empty(ML, dtype=torch.int32, device=dev)
            io = lib.ClosedLoopIO(qpos_dev=qpos.data_ptr(), qvel_dev=qvel.data_ptr(), u_dev=U.data_ptr(), mode=1, T=T, nsub=nsub, flags=flags, solver_iters=iters[0],
                                  contact_iters=iters[1], qpos_ref_dev=rq.data_ptr(), qvel_ref_dev=rv.data_ptr(), nx=nx, k_dev=k.data_ptr(), K_dev=K.data_ptr(), L=Lc,
                                  alpha=C.cast(al, C.c_void_p), clamp=1, u_lo=-1.0, u_hi=1.0, u_traj_dev=out["u"].data_ptr(), qpos_traj_dev=out["qpos"].data_ptr(),
                                  qvel_traj_dev=out["qvel"].data_ptr(), ee_traj_dev=out["ee"].data_ptr(), bad_step_dev=bad.data_ptr())
            # the baseline's buffers: everything per rollout, the gains repeated per candidate outside the span
            rep = lambda t, dim: t.repeat_interleave(Lc, dim=dim).contiguous()
            Ur, kr, Kr = rep(U, 2), rep(k, 1).permute(0, 2, 1).contiguous(), rep(K, 1)                # [T, 6, ML], [T, 6, ML], [T, ML, 6, nx]
            rqr, rvr = rep(rq, 2), rep(rv, 2)
            alr = torch.tensor(alphas, device=dev).repeat(M)[None]                                      # [1, ML]
            q0r, v0r = rep(qpos, 1), rep(qvel, 1)
            base = {"u": torch.empty(T, 6, ML, device=dev), "qpos": torch.empty(T, 13, ML, device=dev), "qvel": torch.empty(T, 12, ML, device=dev),
                    "ee": torch.empty(T, 3, ML, device=dev)}
            ios = []
            for t in range(T):
                src_q, src_v = (q0r, v0r) if t == 0 else (base["qpos"][t - 1], base["qvel"][t - 1])
                ios.append(lib.TrajectoryIO(qpos_dev=src_q.data_ptr(), qvel_dev=src_v.data_ptr(), ctrl_dev=base["u"][t].data_ptr(), mode=1, T=1, nsub=nsub, flags=flags,
                                            solver_iters=iters[0], contact_iters=iters[1], qpos_final_dev=base["qpos"][t].data_ptr(),
                                            qvel_final_dev=base["qvel"][t].data_ptr(), ee_traj_dev=base["ee"][t].data_ptr()))

            def one_query():
                rc = L_.so100_query_closed_loop(sim.h, C.byref(io), M, st)
                assert rc == 0, L_.so100_last_error()

            def one_baseline():
                for t in range(T):
                    if t == 0:
                        c = Ur[0] + alr*kr[0]
                    else:
                        dx = torch_tangent_difference(base["qpos"][t - 1], base["qvel"][t - 1], rqr[t - 1], rvr[t - 1])
                        c = Ur[t] + (alr*kr[t] + torch.einsum("mji,im->jm", Kr[t], dx[idx]))
                    torch.clamp(c, -1.0, 1.0, out=base["u"][t])
                    rc = L_.so100_query_trajectory(sim.h, C.byref(ios[t]), ML, st)
                    assert rc == 0, L_.so100_last_error()

            def pair(call):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record()
                return e0, e1

            def timed(call, n):
                pairs = [pair(call) for _ in range(n)]
                torch.cuda.synchronize()
                return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

            timed(one_query, 2); timed(one_baseline, 1)
            tq, tb = [], []
            for _ in range(a.rounds):
                tq.append(timed(one_query, reps)); tb.append(timed(one_baseline, loops))
            diff = {name: (out[name] - base[name]).abs().max().item() for name in ("u", "qpos", "qvel", "ee")}
            mq, mb = statistics.median(tq), statistics.median(tb)
            case = {"form": a.form, "nx": nx, "M": M, "L": Lc, "T": T, "nsub": nsub, "closed_loop_us_per_call": round(mq, 1), "trajectory_calls_and_torch_us": round(mb, 1),
                    "closed_loop_over_baseline": round(mq/mb, 4), "baseline_us_per_step": round(mb/T, 1), "closed_loop_rounds_us": [round(x, 1) for x in tq],
                    "baseline_rounds_us": [round(x, 1) for x in tb], "units_per_round": [reps, loops], "rollout_substeps_per_s": round(ML*T*nsub/(mq*1e-6), 1),
                    "largest_difference_to_baseline": {name: float(f"{v:.3e}") for name, v in diff.items()}, "bad_rollouts": int((bad >= 0).sum().item())}
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
            del out, base, Ur, kr, Kr, rqr, rvr, ios, K, k, rq, rv
    sim.close()
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


COST_SIZES = [(8, 8, 50, 20), (4096, 8, 20, 10), (4096, 64, 5, 3)]      # (M, T, query calls, baseline runs) per round
COST_L = 8


def cost_main(a):
    """One so100_query_cost_terms / so100_query_cost_select call against the torch arithmetic of examples/ilqr_reach.py on identical inputs: seeded states
    (q uniform over the joint ranges, v in +-2, the cube in a +-0.3 m box, u in +-1), the example's cost (cube target, w_point = 1, w_u = 1e-5).  An event
    pair round each unit, enqueued without waiting; medians of alternated rounds."""
    sim = lib.So100Sim(lib.ENV01, 8, device="cuda:0", flags=lib.F_CUBE_PINNED, seed=0)
    dev, L, st = sim.device, sim.L, sim._stream()
    cc = 1e-5
    six = lambda w: (C.c_float*6)(*([w]*6))
    cdef = lib.CostDef(lib.EE_LINK, None, lib.COST_TARGETS["cube"], 1.0, six(0.0), six(0.0), six(0.0), six(cc), 1.0)
    doc = {"what": "HIP-event time of one so100_query_cost_terms call (lx, lxx, lu, luu) and one so100_query_cost_select call (cost, best, best_cost, u_best; "
                   "L = 8) and of the torch arithmetic of examples/ilqr_reach.py they replace, on identical inputs: So100Sim.jacobian, two einsums, the zero "
                   "fills, the two cats and lu / luu for the terms (the ee rows it reads are the trajectory query's, not timed); the sum over ee and u rows, "
                   "mask, argmin and gather for the selection (the query recomputes the point from qpos).  An event pair round each unit, medians of "
                   "alternated rounds.  A record, not a gate: nothing comparable existed",
           "commit": a.commit, "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    rng = torch.as_tensor(S.joint_range(), dtype=torch.float32, device=dev)

    def pair(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        return e0, e1

    def timed(call, n):
        pairs = [pair(call) for _ in range(n)]
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

    def states(T, cols):
        g = torch.Generator(device=dev).manual_seed(0)
        r = lambda *shape: torch.rand(*shape, generator=g, device=dev)
        qpos = torch.zeros(T, cols, 13, device=dev)
        qpos[..., :6] = rng[:, 0] + (rng[:, 1] - rng[:, 0])*r(T, cols, 6)
        qpos[..., 6:9] = 0.6*r(T, cols, 3) - 0.3
        qpos[..., 9] = 1.0
        return qpos, 4.0*r(T, cols, 12) - 2.0, 2.0*r(T, cols, 6) - 1.0

    for M, T, reps, loops in COST_SIZES:
        qpos, qvel, u = states(T, M)
        ee = sim.kinematics(qpos[..., :6].reshape(T*M, 6))["ee"].reshape(T, M, 3).contiguous()
        qs, vs, us = (x.permute(0, 2, 1).contiguous() for x in (qpos, qvel, u))
        for nx in (12, 24):
            out = {"lx": torch.empty(T + 1, M, nx, device=dev), "lxx": torch.empty(T + 1, M, nx, nx, device=dev), "lu": torch.empty(T, M, 6, device=dev),
                   "luu": torch.empty(T, M, 6, 6, device=dev)}
            io = lib.CostTermsIO(C.pointer(cdef), None, nx, T, qs.data_ptr(), vs.data_ptr(), us.data_ptr(), *[out[k].data_ptr() for k in ("lx", "lxx", "lu", "luu")])
            keep = {}

            def one_query():
                rc = L.so100_query_cost_terms(sim.h, C.byref(io), M, st)
                assert rc == 0, L.so100_last_error()

            def one_torch():
                J = sim.jacobian(qpos[..., :6].reshape(T*M, 6))["jacp"].reshape(T, M, 3, 6)
                r = ee - qpos[..., 6:9]
                lx = torch.zeros(T, M, nx, device=dev); lxx = torch.zeros(T, M, nx, nx, device=dev)
                lx[..., :6] = 2.0*torch.einsum("hnij,hni->hnj", J, r)
                lxx[..., :6, :6] = 2.0*torch.einsum("hnij,hnik->hnjk", J, J)
                if nx == 24:
                    lx[..., 6:9] = -2.0*r
                    lxx[..., :6, 6:9] = -2.0*J.transpose(2, 3); lxx[..., 6:9, :6] = -2.0*J
                    lxx[..., 6:9, 6:9] = 2.0*torch.eye(3, device=dev)
                zero = torch.zeros(1, M, nx, device=dev)
                keep["r"] = (torch.cat([zero, lx]), torch.cat([zero[..., None].expand(1, M, nx, nx), lxx]), 2.0*cc*u,
                             (2.0*cc*torch.eye(6, device=dev)).expand(T, M, 6, 6).contiguous())

            timed(one_query, 2); timed(one_torch, 1)
            tq, tt = [], []
            for _ in range(a.rounds):
                tq.append(timed(one_query, reps)); tt.append(timed(one_torch, loops))
            diff = {k: (out[k] - ref).abs().max().item() for k, ref in zip(("lx", "lxx", "lu", "luu"), keep["r"])}
            mq, mt = statistics.median(tq), statistics.median(tt)
            words = T*M*(13 + 12 + 6) + (T + 1)*M*(nx + nx*nx) + T*M*42
            case = {"query": "cost_terms", "nx": nx, "M": M, "T": T, "query_us_per_call": round(mq, 1), "torch_us": round(mt, 1), "query_over_torch": round(mq/mt, 4),
                    "query_rounds_us": [round(x, 1) for x in tq], "torch_rounds_us": [round(x, 1) for x in tt], "units_per_round": [reps, loops],
                    "GB_per_s": round(words*4/(mq*1e-6)/1e9, 1), "largest_difference_to_torch": {k: float(f"{v:.3e}") for k, v in diff.items()}}
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
            del out, keep
        # the selection: M problems x COST_L candidates
        Lc = COST_L
        qpos, qvel, u = states(T, M*Lc)
        ee = sim.kinematics(qpos[..., :6].reshape(T*M*Lc, 6))["ee"].reshape(T, M, Lc, 3).contiguous()
        qs, vs, us = (x.permute(0, 2, 1).contiguous() for x in (qpos, qvel, u))
        u4, cube = u.reshape(T, M, Lc, 6), qpos.reshape(T, M, Lc, 13)[0, :, 0, 6:9].contiguous()
        qs[:, 6:9] = cube.t().repeat_interleave(Lc, dim=1)[None]          # pinned: every row holds the start's cube, so both sides measure the same thing
        bad = torch.full((M, Lc), -1, dtype=torch.int32, device=dev); bad[::7, 3] = 2
        fb = torch.zeros(T, 6, M, device=dev)
        cost, best, bc, ub = torch.empty(M*Lc, device=dev), torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, device=dev), torch.empty(T, 6, M, device=dev)
        io = lib.CostSelectIO(C.pointer(cdef), None, T, Lc, qs.data_ptr(), vs.data_ptr(), us.data_ptr(), bad.data_ptr(), fb.data_ptr(), cost.data_ptr(), best.data_ptr(),
                              bc.data_ptr(), ub.data_ptr())
        keep = {}

        def one_query():
            rc = L.so100_query_cost_select(sim.h, C.byref(io), M, st)
            assert rc == 0, L.so100_last_error()

        def one_torch():
            c = ((ee - cube[None, :, None]).square().sum(-1) + cc*u4.square().sum(-1)).sum(0)
            c = torch.where(bad >= 0, torch.full_like(c, float("inf")), c)
            b = c.argmin(dim=1)
            env = torch.arange(M, device=dev)
            keep["r"] = (c, b, c[env, b], u4[:, env, b].permute(1, 0, 2).contiguous())

        timed(one_query, 2); timed(one_torch, 1)
        tq, tt = [], []
        for _ in range(a.rounds):
            tq.append(timed(one_query, reps)); tt.append(timed(one_torch, loops))
        c, b, _, plan = keep["r"]
        mq, mt = statistics.median(tq), statistics.median(tt)
        words = T*M*Lc*(9 + 6 + 6) + M*Lc*2 + M*2 + 2*T*M*6
        case = {"query": "cost_select", "L": Lc, "M": M, "T": T, "query_us_per_call": round(mq, 1), "torch_us": round(mt, 1), "query_over_torch": round(mq/mt, 4),
                "query_rounds_us": [round(x, 1) for x in tq], "torch_rounds_us": [round(x, 1) for x in tt], "units_per_round": [reps, loops],
                "GB_per_s": round(words*4/(mq*1e-6)/1e9, 1),
                "largest_difference_to_torch": {"cost": float(f"{(cost.reshape(M, Lc) - c).nan_to_num(posinf=0.0).abs().max().item():.3e}")},
                "same_best_share": round((best == b).float().mean().item(), 4),
                "same_plan_where_same_best": bool((ub.permute(2, 0, 1)[best == b] == plan[best == b]).all().item())}
        doc["cases"].append(case)
        print(json.dumps(case), flush=True)
    sim.close()
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


MPPI_SIZES = [(8, 64, 8, 50, 20, True), (8, 256, 8, 50, 20, True), (512, 256, 16, 5, 3, False)]      # (N, K, T, query calls, torch runs per round, time the whole step too)
MPPI_SIGMA, MPPI_TEMPERATURE = 0.5, 0.01


def mppi_main(a):
    """One so100_query_plan_sample / so100_query_cost_blend call against the torch arithmetic of examples/mppi_reach.py for the same job on identical
    inputs, and the whole planning step (plan_sample -> trajectory -> cost_blend against the example's torch path around the same trajectory call).  An
    event pair round each unit, enqueued without waiting; medians of alternated rounds."""
    doc = {"what": "HIP-event time of one so100_query_plan_sample call (ctrl, qpos_rep, qvel_rep) against randn, the zeroing of candidate 0, add, scale, clamp, "
                   "the two repeat_interleaves and the permute().contiguous() of examples/mppi_reach.py; of one so100_query_cost_blend call (all seven outputs, "
                   "shift 1) against the example's cost sum from the trajectory query's ee rows, mask, min, softmax, weighted sum and shift (the query recomputes "
                   "the point from qpos and its cost is quadratic: the same job, not the same numbers); and of the whole planning step, the three queries against "
                   "the example's torch path around the same so100_query_trajectory call.  An event pair round each unit, medians of alternated rounds.  A "
                   "record, not a gate: nothing comparable existed",
           "commit": a.commit, "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}

    def pair(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        return e0, e1

    def timed(call, n):
        pairs = [pair(call) for _ in range(n)]
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

    def rounds(one_query, one_torch, reps, loops):
        timed(one_query, 2); timed(one_torch, 1)
        tq, tt = [], []
        for _ in range(a.rounds):
            tq.append(timed(one_query, reps)); tt.append(timed(one_torch, loops))
        mq, mt = statistics.median(tq), statistics.median(tt)
        return {"query_us_per_call": round(mq, 1), "torch_us": round(mt, 1), "query_over_torch": round(mq/mt, 4), "query_rounds_us": [round(x, 1) for x in tq],
                "torch_rounds_us": [round(x, 1) for x in tt], "units_per_round": [reps, loops]}, mq

    for N, K, T, reps, loops, whole in MPPI_SIZES:
        sim = lib.So100Sim(lib.ENV01, N, device="cuda:0", flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
        sim.reset()
        dev, L, st = sim.device, sim.L, sim._stream()
        NK = N*K
        plan = (0.4*torch.rand(T, N, 6, device=dev) - 0.2)
        plan_soa = plan.permute(0, 2, 1).contiguous()
        qpos, qvel = sim.get_state()                                 # [13, N], [12, N]
        ctrl, qr, vr = torch.empty(T, 6, NK, device=dev), torch.empty(13, NK, device=dev), torch.empty(12, NK, device=dev)
        sio = lib.PlanSampleIO(plan_soa.data_ptr(), (C.c_float*6)(*([MPPI_SIGMA]*5 + [0.0])), -1.0, 1.0, K, T, 0, 0, 0, qpos.data_ptr(), qvel.data_ptr(),
                               ctrl.data_ptr(), qr.data_ptr(), vr.data_ptr())
        gen = torch.Generator(device=dev).manual_seed(0)
        plan_nt = plan.permute(1, 0, 2).contiguous()                 # the example's [N, T, 6]
        keep = {}

        def sample_query():
            rc = L.so100_query_plan_sample(sim.h, C.byref(sio), N, st)
            assert rc == 0, L.so100_last_error()

        def sample_torch():
            eps = torch.randn(N, K, T, 6, device=dev, generator=gen)
            eps[:, 0] = 0.0
            cand = (plan_nt[:, None] + MPPI_SIGMA*eps).clamp(-1.0, 1.0)
            cand[..., 5] = 0.0
            keep["s"] = (cand, qpos.t().repeat_interleave(K, dim=0), qvel.t().repeat_interleave(K, dim=0), cand.reshape(NK, T, 6).permute(1, 0, 2).contiguous())

        case, mq = rounds(sample_query, sample_torch, reps, loops)
        case = {"query": "plan_sample", "N": N, "K": K, "T": T, **case, "GB_per_s": round((T*6 + 25)*NK*4/(mq*1e-6)/1e9, 1)}
        doc["cases"].append(case); print(json.dumps(case), flush=True)

        # the blend: on the rollouts of the sampled candidates
        cand, sq, sv, cc = keep["s"]
        roll = sim.trajectory(ctrl.permute(0, 2, 1), qr.t(), vr.t(), mode="actions")
        qs, us = roll["qpos"].permute(0, 2, 1).contiguous(), ctrl
        ee, cube, bad = roll["ee"].contiguous(), roll["qpos"][:, :, 6:9].contiguous(), roll["bad_step"]
        cand_q = ctrl.permute(2, 0, 1).reshape(N, K, T, 6).contiguous()           # the example's cand, holding the query's candidates
        six = lambda w: (C.c_float*6)(*([w]*6))
        cdef = lib.CostDef(lib.EE_LINK, None, lib.COST_TARGETS["cube"], 1.0, six(0.0), six(0.0), six(0.0), six(0.0), 1.0)
        out = [torch.empty(NK, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, device=dev), torch.empty(NK, device=dev), torch.empty(N, device=dev),
               torch.empty(T, 6, N, device=dev), torch.empty(6, N, device=dev)]
        bio = lib.CostBlendIO(C.pointer(cdef), None, T, K, qs.data_ptr(), None, us.data_ptr(), bad.data_ptr(), plan_soa.data_ptr(), MPPI_TEMPERATURE, 1, 0,
                              *[t.data_ptr() for t in out])

        def blend_query():
            rc = L.so100_query_cost_blend(sim.h, C.byref(bio), N, st)
            assert rc == 0, L.so100_last_error()

        def blend_torch():
            cost = (cube - ee).norm(dim=2).sum(dim=0).reshape(N, K)
            cost = torch.where(bad.reshape(N, K) >= 0, torch.full_like(cost, float("inf")), cost)
            w = torch.softmax(-(cost - cost.min(dim=1, keepdim=True).values)/0.02, dim=1)
            p = (w[:, :, None, None]*cand_q).sum(dim=1)
            keep["b"] = (p[:, 0].contiguous(), torch.cat([p[:, 1:], torch.zeros(N, 1, 6, device=dev)], dim=1))

        case, mq = rounds(blend_query, blend_torch, reps, loops)
        case = {"query": "cost_blend", "N": N, "K": K, "T": T, **case, "GB_per_s": round((T*(9 + 6 + 6) + 3)*NK*4/(mq*1e-6)/1e9, 1),
                "least_ess": round(out[4].min().item(), 2), "form": a.form}
        doc["cases"].append(case); print(json.dumps(case), flush=True)

        if whole:
            sys.path.insert(0, os.path.join(ROOT, "examples"))
            import mppi_reach
            planners = {m: mppi_reach.Mppi(K, T, plan=m) for m in ("query", "torch")}
            case, _ = rounds(lambda: planners["query"](sim, None), lambda: planners["torch"](sim, None), loops, loops)
            roll_us = timed(lambda: sim.trajectory(ctrl.permute(0, 2, 1), qr.t(), vr.t(), mode="actions"), loops)
            case = {"query": "planning_step", "N": N, "K": K, "T": T, **case, "trajectory_alone_us": round(roll_us, 1)}
            doc["cases"].append(case); print(json.dumps(case), flush=True)
        sim.close()
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


CEM_SIZES = [(8, 64, 8, 50, 20, True), (8, 256, 8, 50, 20, True), (512, 256, 16, 5, 3, False), (1, 4096, 1, 50, 20, False)]      # as MPPI_SIZES; E = K / 8
CEM_ALPHA, CEM_SIGMA_MIN = 0.1, 0.05


def cem_main(a):
    """One so100_query_plan_sample_tv call against one so100_query_plan_sample call on equal inputs (what reading sigma from memory costs), one
    so100_query_cost_refit call against the torch arithmetic for the same job, and a whole CEM round both ways around the same trajectory call.  An event
    pair round each unit, enqueued without waiting; medians of alternated rounds."""
    doc = {"what": "HIP-event time of one so100_query_plan_sample_tv call (ctrl, qpos_rep, qvel_rep; sigma_dev holding sigma[j] in every entry) against one "
                   "so100_query_plan_sample call with that sigma[6] on the same plan and states (tv_over_plain); of one so100_query_cost_refit call (all nine "
                   "outputs, E = K / 8, alpha 0.1, shift 1) against torch for the same job: the cost sum from the trajectory query's ee rows, mask, topk, gather, "
                   "mean, var, sqrt, smoothing, clamp and shift (the query recomputes the point from qpos and its cost is quadratic: the same job, not the same "
                   "numbers); and of a whole CEM round, plan_sample_tv -> trajectory -> cost_refit against randn sampling, the same trajectory call and the "
                   "torch refit.  An event pair round each unit, medians of alternated rounds.  A record, not a gate: nothing comparable existed",
           "commit": a.commit, "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}

    def pair(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        return e0, e1

    def timed(call, n):
        pairs = [pair(call) for _ in range(n)]
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in pairs)*1e3/n

    def rounds(one_query, one_other, reps, loops, names=("query_us_per_call", "torch_us", "query_over_torch")):
        timed(one_query, 2); timed(one_other, 1)
        tq, tt = [], []
        for _ in range(a.rounds):
            tq.append(timed(one_query, reps)); tt.append(timed(one_other, loops))
        mq, mt = statistics.median(tq), statistics.median(tt)
        return {names[0]: round(mq, 1), names[1]: round(mt, 1), names[2]: round(mq/mt, 4), "first_rounds_us": [round(x, 1) for x in tq],
                "second_rounds_us": [round(x, 1) for x in tt], "units_per_round": [reps, loops]}, mq

    for N, K, T, reps, loops, whole in CEM_SIZES:
        sim = lib.So100Sim(lib.ENV01, N, device="cuda:0", flags=lib.F_CUBE_PINNED, max_episode_steps=0, seed=0)
        sim.reset()
        dev, L, st = sim.device, sim.L, sim._stream()
        NK, E = N*K, K//8
        six = lambda w: (C.c_float*6)(*w)
        sig6 = [MPPI_SIGMA]*5 + [0.0]
        plan = (0.4*torch.rand(T, N, 6, device=dev) - 0.2)
        plan_soa = plan.permute(0, 2, 1).contiguous()
        sigma = torch.tensor(sig6, device=dev).expand(T, N, 6).contiguous()
        sigma_soa = sigma.permute(0, 2, 1).contiguous()
        qpos, qvel = sim.get_state()                                 # [13, N], [12, N]
        ctrl, qr, vr = torch.empty(T, 6, NK, device=dev), torch.empty(13, NK, device=dev), torch.empty(12, NK, device=dev)
        sio = lib.PlanSampleIO(plan_soa.data_ptr(), six(sig6), -1.0, 1.0, K, T, 0, 0, 0, qpos.data_ptr(), qvel.data_ptr(), ctrl.data_ptr(), qr.data_ptr(), vr.data_ptr())
        tio = lib.PlanSampleTvIO(plan_soa.data_ptr(), sigma_soa.data_ptr(), -1.0, 1.0, K, T, 0, 0, 0, qpos.data_ptr(), qvel.data_ptr(), ctrl.data_ptr(), qr.data_ptr(),
                                 vr.data_ptr())

        def sample_tv():
            rc = L.so100_query_plan_sample_tv(sim.h, C.byref(tio), N, st)
            assert rc == 0, L.so100_last_error()

        def sample_plain():
            rc = L.so100_query_plan_sample(sim.h, C.byref(sio), N, st)
            assert rc == 0, L.so100_last_error()

        case, mq = rounds(sample_tv, sample_plain, reps, reps, ("tv_us_per_call", "plain_us_per_call", "tv_over_plain"))
        case = {"query": "plan_sample_tv", "N": N, "K": K, "T": T, **case, "GB_per_s": round((T*6 + 25)*NK*4/(mq*1e-6)/1e9, 1)}
        doc["cases"].append(case); print(json.dumps(case), flush=True)

        # the refit: on the rollouts of the sampled candidates
        roll = sim.trajectory(ctrl.permute(0, 2, 1), qr.t(), vr.t(), mode="actions")
        qs, us = roll["qpos"].permute(0, 2, 1).contiguous(), ctrl
        ee, cube, bad = roll["ee"].contiguous(), roll["qpos"][:, :, 6:9].contiguous(), roll["bad_step"]
        cand_q = ctrl.permute(2, 0, 1).reshape(N, K, T, 6).contiguous()           # [N, K, T, 6], holding the query's candidates
        plan_nt, sigma_nt = plan.permute(1, 0, 2).contiguous(), sigma.permute(1, 0, 2).contiguous()
        lo_t, hi_t, init_t = (torch.tensor(v, device=dev) for v in ([CEM_SIGMA_MIN]*5 + [0.0], sig6, sig6))
        cdef = lib.CostDef(lib.EE_LINK, None, lib.COST_TARGETS["cube"], 1.0, six([0.0]*6), six([0.0]*6), six([0.0]*6), six([0.0]*6), 1.0)
        out = [torch.empty(NK, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, device=dev), torch.empty(N*E, dtype=torch.int32, device=dev),
               torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, device=dev), torch.empty(T, 6, N, device=dev), torch.empty(T, 6, N, device=dev),
               torch.empty(6, N, device=dev)]
        rio = lib.CostRefitIO(C.pointer(cdef), None, T, K, qs.data_ptr(), None, us.data_ptr(), bad.data_ptr(), plan_soa.data_ptr(), E, CEM_ALPHA, plan_soa.data_ptr(),
                              sigma_soa.data_ptr(), six([CEM_SIGMA_MIN]*5 + [0.0]), six(sig6), six(sig6), 1, 0, *[t.data_ptr() for t in out])
        keep = {}

        def refit_query():
            rc = L.so100_query_cost_refit(sim.h, C.byref(rio), N, st)
            assert rc == 0, L.so100_last_error()

        def torch_refit(ee, cube, bad, cand, old_mean, old_sigma):
            cost = (cube - ee).norm(dim=2).sum(dim=0).reshape(N, K)
            cost = torch.where(bad.reshape(N, K) >= 0, torch.full_like(cost, float("inf")), cost)
            top = torch.topk(cost, E, dim=1, largest=False)
            el = cand.gather(1, top.indices[:, :, None, None].expand(N, E, T, 6))
            mu, sd = el.mean(dim=1), el.var(dim=1, unbiased=False).sqrt()
            mean = CEM_ALPHA*old_mean + (1.0 - CEM_ALPHA)*mu
            sg = torch.minimum(torch.maximum(CEM_ALPHA*old_sigma + (1.0 - CEM_ALPHA)*sd, lo_t), hi_t)
            return (mean[:, 0].contiguous(), torch.cat([mean[:, 1:], torch.zeros(N, 1, 6, device=dev)], dim=1),
                    torch.cat([sg[:, 1:], init_t.expand(N, 1, 6)], dim=1), top.values[:, -1])

        def refit_torch():
            keep["r"] = torch_refit(ee, cube, bad, cand_q, plan_nt, sigma_nt)

        case, mq = rounds(refit_query, refit_torch, reps, loops)
        case = {"query": "cost_refit", "N": N, "K": K, "E": E, "T": T, **case, "GB_per_s": round((T*(9 + 6 + 2*6*E/K) + 2)*NK*4/(mq*1e-6)/1e9, 1),
                "least_n_elite": int(out[4].min().item())}
        doc["cases"].append(case); print(json.dumps(case), flush=True)

        if whole:
            gen = torch.Generator(device=dev).manual_seed(0)
            state = {"q": (plan, sigma, 0), "t": (plan_nt, sigma_nt)}

            def round_query():
                mean, sg, draw = state["q"]
                cand = sim.plan_sample_tv(mean, K, sg, draw=draw, qpos=qpos.t(), qvel=qvel.t())
                r = sim.trajectory(cand["ctrl"], cand["qpos"], cand["qvel"], mode="actions")
                o = sim.cost_refit(r["qpos"], None, cand["ctrl"], K, E, alpha=CEM_ALPHA, plan=mean, sigma=sg, sigma_min=[CEM_SIGMA_MIN]*5 + [0.0], sigma_max=sig6,
                                   sigma_init=sig6, bad_step=r["bad_step"], u_fallback=mean, shift=1, target_mode="cube")
                state["q"] = (o["mean"], o["sigma_out"], draw + 1)

            def round_torch():
                mean, sg = state["t"]
                eps = torch.randn(N, K, T, 6, device=dev, generator=gen)
                eps[:, 0] = 0.0
                cand = (mean[:, None] + sg[:, None]*eps).clamp(-1.0, 1.0)
                r = sim.trajectory(cand.reshape(NK, T, 6).permute(1, 0, 2).contiguous(), qpos.t().repeat_interleave(K, dim=0), qvel.t().repeat_interleave(K, dim=0),
                                   mode="actions")
                _, m2, s2, _ = torch_refit(r["ee"], r["qpos"][:, :, 6:9], r["bad_step"], cand, mean, sg)
                state["t"] = (m2, s2)

            case, _ = rounds(round_query, round_torch, loops, loops)
            roll_us = timed(lambda: sim.trajectory(ctrl.permute(0, 2, 1), qr.t(), vr.t(), mode="actions"), loops)
            case = {"query": "cem_round", "N": N, "K": K, "E": E, "T": T, **case, "trajectory_alone_us": round(roll_us, 1)}
            doc["cases"].append(case); print(json.dumps(case), flush=True)
        sim.close()
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None); ap.add_argument("--commit", default="unknown")
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forward", action="store_true", help="time the forward-dynamics query against so100_step (profiles/forward_kbench.json)")
    ap.add_argument("--trajectory", action="store_true", help="time the trajectory query against the so100_step calls it predicts (profiles/trajectory_kbench.json)")
    ap.add_argument("--derivatives", action="store_true", help="time the derivatives query against its emulation through the trajectory query (profiles/derivatives_kbench.json)")
    ap.add_argument("--lqr", action="store_true", help="time the LQR query against the torch loops of examples/ilqr_reach.py (profiles/lqr_kbench.json)")
    ap.add_argument("--lqr-reg", action="store_true", help="time so100_query_lqr_reg against so100_query_lqr, alone and with the caller's retry round it, and so100_query_reg_schedule against torch (profiles/lqr_reg_kbench.json)")
    ap.add_argument("--closed-loop", action="store_true", help="time the closed-loop trajectory query against T trajectory calls with the law in torch (profiles/closed_loop_kbench.json)")
    ap.add_argument("--cost", action="store_true", help="time the two cost queries against the torch arithmetic of examples/ilqr_reach.py (profiles/cost_kbench.json)")
    ap.add_argument("--mppi", action="store_true", help="time the two sampling-planner queries and the whole planning step against the torch arithmetic of examples/mppi_reach.py (profiles/mppi_kbench.json)")
    ap.add_argument("--cem", action="store_true", help="time the two cross-entropy planner queries and a whole CEM round against so100_query_plan_sample and the torch arithmetic for the same job (profiles/cem_kbench.json)")
    ap.add_argument("--form", default=None, help="--lqr: the label of the loaded library's kernel form (mfma, or valu for a -DSO100_LQR_VALU=1 side build); "
                                                 "--closed-loop: global, or lds for a -DSO100_CL_LDS=1 side build; --mppi: the blend's workgroup form")
    a = ap.parse_args()
    if a.form is None:
        a.form = "four waves per problem at every K (ships)" if a.mppi else "global" if a.closed_loop else "mfma"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "lqr_reg_kbench.json" if a.lqr_reg else "cem_kbench.json" if a.cem else "mppi_kbench.json" if a.mppi else "cost_kbench.json" if a.cost else "closed_loop_kbench.json" if a.closed_loop else "lqr_kbench.json" if a.lqr else "derivatives_kbench.json" if a.derivatives else "trajectory_kbench.json" if a.trajectory else "forward_kbench.json" if a.forward else "query_kbench.json")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.lqr_reg:
        return lqr_reg_main(a)
    if a.cem:
        return cem_main(a)
    if a.mppi:
        return mppi_main(a)
    if a.cost:
        return cost_main(a)
    if a.closed_loop:
        return closed_loop_main(a)
    if a.lqr:
        return lqr_main(a)
    if a.derivatives:
        return derivatives_main(a)
    if a.trajectory:
        return trajectory_main(a)
    if a.forward:
        return forward_main(a)
    sim = lib.So100Sim(lib.ENV01, 64, device="cuda:0", flags=lib.F_REFERENCE, seed=0)
    dev, L, h = sim.device, sim.L, sim.h
    rs = np.random.RandomState(0)
    rng = S.joint_range()
    q0r, tgr, _ = S.ik_recipe()
    doc = {"what": "HIP-event time per call of the model queries through the C ABI; medians of alternated rounds", "commit": a.commit,
           "card": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": []}
    for M, reps in SIZES:
        f = dict(dtype=torch.float32, device=dev)
        soa = lambda x: torch.from_numpy(np.ascontiguousarray(x.T, np.float32)).to(dev)
        q = soa(rs.uniform(rng[:, 0], rng[:, 1], (M, 6))); v = soa(rs.uniform(-2, 2, (M, 6))); acc = soa(rs.uniform(-20, 20, (M, 6)))
        idx = np.arange(M) % len(q0r)
        q0, tg = soa(q0r[idx]), soa(tgr[idx])
        out = torch.empty(93, M, **f)            # the largest output set: xpos 18 | xmat 54 | ee 3 | cam_pos 3 | cam_mat 9
        its, conv = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.uint8, device=dev)
        p = lambda row: out[row].data_ptr()
        calls = {
            "kinematics_all": ("so100_query_kinematics", lib.KinematicsIO(q.data_ptr(), p(0), p(18), p(72), p(75), p(78)), 6 + 87),
            "kinematics_ee": ("so100_query_kinematics", lib.KinematicsIO(q.data_ptr(), None, None, p(72), None, None), 6 + 3),
            "jacobian": ("so100_query_jacobian", lib.JacobianIO(q.data_ptr(), 4, None, p(0), p(18)), 6 + 36),
            "dynamics": ("so100_query_dynamics", lib.DynamicsIO(q.data_ptr(), v.data_ptr(), acc.data_ptr(), p(0), p(36), p(42)), 18 + 48),
            "ik": ("so100_query_ik", lib.IkIO(tg.data_ptr(), q0.data_ptr(), 4, None, 64, 0.02, 1e-4, 0.3, p(0), p(6), its.data_ptr(), conv.data_ptr()), 9 + 7 + 1.25),
        }
        st = sim._stream()

        def timed(fn, io, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                rc = getattr(L, fn)(h, C.byref(io), M, st)
                assert rc == 0, L.so100_last_error()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n

        for fn, io, _ in calls.values():
            timed(fn, io, a.warmup)
        us = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, (fn, io, _) in calls.items():
                us[k].append(timed(fn, io, reps))
        for k, (fn, io, words) in calls.items():
            med = statistics.median(us[k])
            case = {"case": k, "M": M, "us_per_call": round(med, 2), "rounds_us": [round(x, 2) for x in us[k]], "calls_per_round": reps,
                    "problems_per_s": round(M / (med * 1e-6), 1), "bytes_moved": int(words * 4 * M), "GB_per_s": round(words * 4 * M / (med * 1e-6) / 1e9, 1)}
            if k == "ik":
                case["mean_iterations"] = round(its.float().mean().item(), 3); case["converged_share"] = round(conv.float().mean().item(), 4)
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
    sim.close()
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
