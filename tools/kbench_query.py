#!/usr/bin/env python3
"""Time the model queries (include/so100_query.h) with HIP events, through the C ABI on preallocated buffers (needs a GPU).

    python tools/kbench_query.py [--out profiles/query_kbench.json] [--commit LABEL] [--rounds 5]

Cases, at M = 4096 and M = 1 048 576 problems: kinematics with every output and with the end-effector point alone, the Jacobian (jacp and
jacr), the dynamics (M, bias and tau) and the IK.  Poses are uniform over the joint ranges; the IK problems are the 400 of the tests' recipe
(tests/query_support.py: a reachable target, a start up to 0.3 rad away, the default parameters) repeated to fill M.  The cases are timed
in alternation, `--rounds` times each; a figure is the median of the rounds, one round the mean over its calls.  There is nothing to
compare against: the file is a record, not a gate."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_kbench.json")); ap.add_argument("--commit", default="unknown")
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
