#!/usr/bin/env python3
"""One full PPO update, PyTorch learner against the library's kernels, and `main.py train` end to end with either (needs a GPU).

    python tools/kbench_learner.py [--out profiles/learner_update_kbench.json] [--commit LABEL] [--iters 100]

Update: T = 64, N = 4096, 4 epochs of 32 768-sample minibatches (the PPO defaults), obs_dim 15 and 8; ppo.PPO.update and ppo.FusedPPO.update in
one process on ONE synthetic chunk (no terminal observations: both take the rewards as they are).  First both learners make one update from
the same initial weights with the same permutations and the largest parameter difference is reported (relative to each tensor's largest
entry): the timed path is a compared path.  Then the two are timed in alternation, `--rounds` times each, HIP events around `reps` updates
after a warm-up (every update ends in the .item() of its statistics, so the events bracket finished work); every round's figure is kept.
Train: `main.py -a PPO train -e Env01-v1 --iters N --learner torch|fused`, alternating, twice each.  timesteps/s covers the window from the
driver's first progress line (iteration 10: code objects loaded, buffers allocated) to its `done:` line, on the host clock -- rollouts,
updates, the evaluations that fall into the run and the final saves; the driver's own summary line (whole run, 0.1 s resolution) is kept too.
Every GPU step runs in a child process under its own time limit; the first one that fails ends the run.  One JSON document is written.

    python tools/kbench_learner.py --part update --obs-dim 15 [--rounds 1]      # one step by hand (e.g. under rocprofv3)
    python tools/kbench_learner.py --part update --obs-dim 15 --shuffle device   # FusedPPO(shuffle="device") against FusedPPO's default path
    python tools/kbench_learner.py --terms [--out profiles/learner_terms_kbench.json] [--commit LABEL]

--terms: the extended step (so100_learner_minibatch_step_ex, SB3's remaining loss terms) against the old one, per minibatch of 32 768 on the
same chunk through the C ABI: the old step, the extended step with every term off, with entropy bonus and value clipping, with per-minibatch
normalisation as well (one more launch: the difference is the cost of the statistics launch), and a skipped step (the update stopped by
target_kl: every kernel returns at once).  Timed in alternation, `--rounds` times each, HIP events around 200 steps.

    python tools/kbench_learner.py --normalize-reward [--out profiles/learner_rewnorm_kbench.json] [--commit LABEL]

--normalize-reward: FusedPPO.update with and without normalize_reward, in both of its paths (the steps enqueued from Python; the one-call update),
the four in alternation on the chunk of --part update, and the normalisation pass alone (so100_learner_normalize_rewards, three launches) per
call.  The added time per update is held against one minibatch step of the same run (the update without the option / 32).

    python tools/kbench_learner.py --normalize-obs [--parent-tree DIR] [--out profiles/learner_obsnorm_kbench.json] [--commit LABEL]

--normalize-obs: the same for normalize_obs -- FusedPPO.update with and without it in both paths, in alternation, and the moments + fold passes
alone (so100_learner_obs_norm_update + so100_learner_obs_norm_fold, three launches) per call.  --parent-tree: a built checkout of the parent
commit; the update without the option is then timed in child processes of their own in the order parent, this, parent, this (the child
imports the package of the tree it is given), and the document says whether this commit's figures lie inside the parent's own spread.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SO100_KBENCH_TREE", ROOT))      # --part off_only in another tree (--parent-tree): that tree's package and library

T, N, EPOCHS, MB = 64, 4096, 4, 32768


def part_update(obs_dim, rounds, reps, warmup, shuffle="torch"):
    if shuffle == "device":
        return part_update_shuffle(obs_dim, rounds, reps["fused"], warmup)
    import torch
    from so100_mujoco_rl_amd.ppo import PPO, FusedPPO
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(obs_dim)
    o = obs_dim
    learners = {"torch": PPO(o, dev, seed=0), "fused": FusedPPO(o, dev, seed=0)}          # the same initial weights
    c = RolloutChunk(T, N, o, dev)
    c.buf.copy_(torch.randn(c.buf.shape, device=dev, generator=g))
    with torch.no_grad():                                        # a chunk the policy could have produced: its own values and log-probs, rare episode ends
        v, lp = learners["torch"].net.evaluate(c.buf[..., :o].reshape(-1, o), c.buf[..., o:o + 6].reshape(-1, 6))
        c.buf[..., o + 8] = v.reshape(T, N); c.buf[..., o + 9] = lp.reshape(T, N)
        c.buf[..., o + 7] = (torch.rand(T, N, device=dev, generator=g) < 1e-3).float() * 2.0
    b = c.unpack(); b["last_obs"] = torch.randn(N, o, device=dev, generator=g); b["packed"] = c.buf
    res = {"obs_dim": o, "T": T, "N": N, "epochs": EPOCHS, "minibatch": MB, "samples": T * N, "card": torch.cuda.get_device_name(0)}
    # ---- the timed path is a compared path: one update each from the same weights, the same permutations
    stats = {}
    for name, learner in learners.items():
        torch.manual_seed(1234)
        stats[name] = learner.update(b)
    sd_t, sd_f = learners["torch"].net.state_dict(), learners["fused"].net.state_dict()
    res["first_update_max_param_difference"] = max(float((sd_f[k] - sd_t[k]).abs().max() / sd_t[k].abs().max()) for k in sd_t)
    res["first_update_value_loss"] = {k: stats[k]["value_loss"] for k in stats}
    for learner in learners.values():
        for _ in range(warmup):
            learner.update(b)
    ms = {"torch": [], "fused": []}
    for _ in range(rounds):                                      # alternating: what drifts on a shared host hits both
        for name, learner in learners.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(reps[name]):
                learner.update(b)
            e1.record(); torch.cuda.synchronize()
            ms[name].append(round(e0.elapsed_time(e1) / reps[name], 4))
    for name in ms:
        med = sorted(ms[name])[len(ms[name]) // 2]
        res[name] = {"ms_per_update_rounds": ms[name], "ms_per_update": med, "updates_per_round": reps[name], "samples_per_s": round(T * N * EPOCHS / med * 1e3)}
    res["torch_over_fused"] = round(res["torch"]["ms_per_update"] / res["fused"]["ms_per_update"], 2)
    print("KBENCH " + json.dumps(res), flush=True)


def part_update_shuffle(obs_dim, rounds, reps, warmup):
    """--part update --shuffle device: FusedPPO.update with the one-call update and the device shuffle against the default path (torch.randperm,
    the steps enqueued from Python), on the chunk of part_update, in alternation"""
    import torch
    from so100_mujoco_rl_amd.ppo import FusedPPO
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(obs_dim)
    o = obs_dim
    learners = {"torch": FusedPPO(o, dev, seed=0), "device": FusedPPO(o, dev, seed=0, shuffle="device")}
    c = RolloutChunk(T, N, o, dev)
    c.buf.copy_(torch.randn(c.buf.shape, device=dev, generator=g))
    with torch.no_grad():
        v, lp = learners["torch"].net.evaluate(c.buf[..., :o].reshape(-1, o), c.buf[..., o:o + 6].reshape(-1, 6))
        c.buf[..., o + 8] = v.reshape(T, N); c.buf[..., o + 9] = lp.reshape(T, N)
        c.buf[..., o + 7] = (torch.rand(T, N, device=dev, generator=g) < 1e-3).float() * 2.0
    b = c.unpack(); b["last_obs"] = torch.randn(N, o, device=dev, generator=g); b["packed"] = c.buf
    res = {"obs_dim": o, "T": T, "N": N, "epochs": EPOCHS, "minibatch": MB, "samples": T * N, "card": torch.cuda.get_device_name(0)}
    for learner in learners.values():
        for _ in range(warmup):
            learner.update(b)
    ms = {k: [] for k in learners}
    for _ in range(rounds):
        for name, learner in learners.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(reps):
                learner.update(b)
            e1.record(); torch.cuda.synchronize()
            ms[name].append(round(e0.elapsed_time(e1) / reps, 4))
    for name in ms:
        res["shuffle_" + name] = {"ms_per_update_rounds": ms[name], "ms_per_update": sorted(ms[name])[len(ms[name]) // 2], "updates_per_round": reps}
    res["device_over_torch"] = round(res["shuffle_device"]["ms_per_update"] / res["shuffle_torch"]["ms_per_update"], 4)
    print("KBENCH " + json.dumps(res), flush=True)


def part_rewnorm(obs_dim, rounds, reps, warmup):
    """--part rewnorm: FusedPPO.update off / on in both paths, in alternation, and so100_learner_normalize_rewards alone"""
    import torch
    from so100_mujoco_rl_amd.ppo import FusedPPO
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(obs_dim)
    o = obs_dim
    learners = {f"{path}_{'on' if on else 'off'}": FusedPPO(o, dev, seed=0, shuffle=shuffle, normalize_reward=on)
                for path, shuffle in (("three_call", "torch"), ("one_call", "device")) for on in (False, True)}
    c = RolloutChunk(T, N, o, dev)
    c.buf.copy_(torch.randn(c.buf.shape, device=dev, generator=g))
    with torch.no_grad():
        v, lp = learners["three_call_off"].net.evaluate(c.buf[..., :o].reshape(-1, o), c.buf[..., o:o + 6].reshape(-1, 6))
        c.buf[..., o + 6] = 1.5 + 0.5 * c.buf[..., o + 6]         # the tasks pay 1-2 per step
        c.buf[..., o + 8] = v.reshape(T, N); c.buf[..., o + 9] = lp.reshape(T, N)
        c.buf[..., o + 7] = (torch.rand(T, N, device=dev, generator=g) < 1e-3).float() * 2.0
    b = c.unpack(); b["last_obs"] = torch.randn(N, o, device=dev, generator=g); b["packed"] = c.buf
    res = {"obs_dim": o, "T": T, "N": N, "epochs": EPOCHS, "minibatch": MB, "samples": T * N, "card": torch.cuda.get_device_name(0)}

    def window(fn, count):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(count):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / count

    L = learners["three_call_on"]._handle()
    rn = learners["three_call_on"]._reward_norm(L, T, N)
    alone = lambda: L.normalize_rewards(c.buf, rn["state"], rn["rewards"], rn["workspace"])
    for learner in learners.values():
        for _ in range(warmup):
            learner.update(b)
    window(alone, 20)
    ms = {k: [] for k in learners}; us_alone = []
    for _ in range(rounds):
        for name, learner in learners.items():
            ms[name].append(round(window(lambda: learner.update(b), reps), 4))
        us_alone.append(round(window(alone, 200) * 1e3, 2))
    med = lambda x: sorted(x)[len(x) // 2]
    for name in ms:
        res[name] = {"ms_per_update_rounds": ms[name], "ms_per_update": med(ms[name]), "updates_per_round": reps}
    res["normalize_rewards_alone"] = {"us_per_call_rounds": us_alone, "us_per_call": med(us_alone), "calls_per_window": 200, "launches": 3}
    for path in ("three_call", "one_call"):
        off, on = res[path + "_off"]["ms_per_update"], res[path + "_on"]["ms_per_update"]
        res[path + "_added_us_per_update"] = round((on - off) * 1e3, 1)
        res[path + "_one_minibatch_step_us"] = round(off * 1e3 / (EPOCHS * (T * N // MB)), 1)
    res["return_std"] = float(rn["state"][1].sqrt().item())
    print("KBENCH " + json.dumps(res), flush=True)


def _kbench_chunk(torch, net, o, dev, g):
    """the chunk of part_update: noise the policy could have produced, rare episode ends"""
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    c = RolloutChunk(T, N, o, dev)
    c.buf.copy_(torch.randn(c.buf.shape, device=dev, generator=g))
    with torch.no_grad():
        v, lp = net.evaluate(c.buf[..., :o].reshape(-1, o), c.buf[..., o:o + 6].reshape(-1, 6))
        c.buf[..., o + 8] = v.reshape(T, N); c.buf[..., o + 9] = lp.reshape(T, N)
        c.buf[..., o + 7] = (torch.rand(T, N, device=dev, generator=g) < 1e-3).float() * 2.0
    b = c.unpack(); b["last_obs"] = torch.randn(N, o, device=dev, generator=g); b["packed"] = c.buf
    return c, b


def _window(torch, fn, count):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(count):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count


def part_obsnorm(obs_dim, rounds, reps, warmup):
    """--part obsnorm: FusedPPO.update off / on in both paths, in alternation, and the moments + fold passes alone"""
    import torch
    from so100_mujoco_rl_amd.ppo import FusedPPO
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(obs_dim)
    o = obs_dim
    learners = {f"{path}_{'on' if on else 'off'}": FusedPPO(o, dev, seed=0, shuffle=shuffle, normalize_obs=on)
                for path, shuffle in (("three_call", "torch"), ("one_call", "device")) for on in (False, True)}
    c, b = _kbench_chunk(torch, learners["three_call_off"].net, o, dev, g)
    res = {"obs_dim": o, "T": T, "N": N, "epochs": EPOCHS, "minibatch": MB, "samples": T * N, "card": torch.cuda.get_device_name(0)}
    f = learners["three_call_on"]
    L = f._handle()
    alone = lambda: f._absorb_observations(L, c.buf)
    for learner in learners.values():
        for _ in range(warmup):
            learner.update(b)
    _window(torch, alone, 20)
    ms = {k: [] for k in learners}; us_alone = []
    for _ in range(rounds):
        for name, learner in learners.items():
            ms[name].append(round(_window(torch, lambda: learner.update(b), reps), 4))
        us_alone.append(round(_window(torch, alone, 200) * 1e3, 2))
    med = lambda x: sorted(x)[len(x) // 2]
    for name in ms:
        res[name] = {"ms_per_update_rounds": ms[name], "ms_per_update": med(ms[name]), "updates_per_round": reps}
    res["moments_and_fold_alone"] = {"us_per_call_rounds": us_alone, "us_per_call": med(us_alone), "calls_per_window": 200, "launches": 3}
    for path in ("three_call", "one_call"):
        off, on = res[path + "_off"]["ms_per_update"], res[path + "_on"]["ms_per_update"]
        res[path + "_added_us_per_update"] = round((on - off) * 1e3, 1)
        res[path + "_one_minibatch_step_us"] = round(off * 1e3 / (EPOCHS * (T * N // MB)), 1)
    print("KBENCH " + json.dumps(res), flush=True)


def part_off_only(obs_dim, rounds, reps, warmup):
    """--part off_only: FusedPPO.update without any option in both paths, in the tree SO100_KBENCH_TREE names (the parent commit's or this one's)"""
    import torch
    from so100_mujoco_rl_amd.ppo import FusedPPO
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(obs_dim)
    o = obs_dim
    learners = {"three_call_off": FusedPPO(o, dev, seed=0), "one_call_off": FusedPPO(o, dev, seed=0, shuffle="device")}
    c, b = _kbench_chunk(torch, learners["three_call_off"].net, o, dev, g)
    for learner in learners.values():
        for _ in range(warmup):
            learner.update(b)
    res = {"obs_dim": o, "has_normalize_obs": "normalize_obs" in FusedPPO.__init__.__code__.co_varnames}       # tells the two trees apart
    for name, learner in learners.items():
        ms = [round(_window(torch, lambda: learner.update(b), reps), 4) for _ in range(rounds)]
        res[name] = {"ms_per_update_rounds": ms, "ms_per_update": sorted(ms)[len(ms) // 2], "updates_per_round": reps}
    print("KBENCH " + json.dumps(res), flush=True)


def part_terms(obs_dim, rounds, reps=200, warmup=20):
    import torch
    from so100_mujoco_rl_amd.lib import So100Learner
    from so100_mujoco_rl_amd.ppo import FusedPPO
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(obs_dim)
    o = obs_dim
    f = FusedPPO(o, dev, seed=0)
    buf = torch.randn(T, N, o + 10, device=dev, generator=g)
    with torch.no_grad():
        v, lp = f.net.evaluate(buf[..., :o].reshape(-1, o), buf[..., o:o + 6].reshape(-1, 6))
        buf[..., o + 8] = v.reshape(T, N) + 0.5 * torch.randn(T, N, device=dev, generator=g); buf[..., o + 9] = lp.reshape(T, N)
        buf[..., o + 7] = (torch.rand(T, N, device=dev, generator=g) < 1e-3).float() * 2.0
    L = So100Learner(o, dev, max_minibatch=MB)
    P = L.num_params
    adv = torch.zeros(T, N, device=dev); ret = torch.zeros(T, N, device=dev); adv_stats = torch.zeros(2, device=dev)
    L.advantages(buf, torch.randn(N, o, device=dev, generator=g), f.params, adv, ret, adv_stats)
    perm = torch.randperm(T * N, device=dev, generator=g)
    idx = [perm[i:i + MB] for i in range(0, T * N, MB)]
    stats = torch.zeros(4, device=dev); diag = torch.zeros(8, device=dev)
    live = torch.zeros(2, dtype=torch.int32, device=dev); stopped = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    on = dict(ent_coef=0.01, clip_range_vf=0.3)
    variants = {"old_step": None, "extended_every_term_off": {}, "extended_entropy_value_clip": dict(on, update_state=live, target_kl=1e9),
                "extended_all_terms": dict(on, normalize_advantage="minibatch", update_state=live, target_kl=1e9),
                "extended_skipped": dict(on, normalize_advantage="minibatch", update_state=stopped, target_kl=1e9)}

    def run(kw, count):
        p = f.params.clone(); m = torch.zeros(P, device=dev); v = torch.zeros(P, device=dev)          # every window starts from the same weights
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for i in range(count):
            if kw is None:
                L.minibatch_step(buf, idx[i % len(idx)], adv, ret, adv_stats, p, m, v, i + 1, stats)
            else:
                L.minibatch_step_ex(buf, idx[i % len(idx)], adv, ret, adv_stats, p, m, v, i + 1, diag, **kw)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / count

    for kw in variants.values():
        run(kw, warmup)
    us = {k: [] for k in variants}
    for _ in range(rounds):
        for k, kw in variants.items():
            us[k].append(round(run(kw, reps) * 1e3, 2))
    med = {k: sorted(x)[len(x) // 2] for k, x in us.items()}
    assert stopped.tolist() == [1, 0]
    res = {"obs_dim": o, "minibatch": MB, "steps_per_window": reps, "card": torch.cuda.get_device_name(0), "us_per_minibatch_rounds": us, "us_per_minibatch": med,
           "extended_all_terms_over_old_step": round(med["extended_all_terms"] / med["old_step"], 4),
           "extended_every_term_off_over_old_step": round(med["extended_every_term_off"] / med["old_step"], 4),
           "statistics_launch_us": round(med["extended_all_terms"] - med["extended_entropy_value_clip"], 2), "skipped_step_us": med["extended_skipped"]}
    print("KBENCH " + json.dumps(res), flush=True)


def part_train(learner, iters):
    import logging
    import time
    from click.testing import CliRunner
    from so100_mujoco_rl_amd import main as drv
    lines = []
    h = logging.Handler(); h.emit = lambda rec: lines.append((time.perf_counter(), rec.getMessage()))
    drv.logger.addHandler(h)
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "-e", "Env01-v1", "--envs", str(N), "--iters", str(iters), "--learner", learner], catch_exceptions=False)
        os.chdir(ROOT)
    assert r.exit_code == 0, r.output
    t10 = [t for t, l in lines if l.startswith("iter    10 ")][0]
    t_done, summary = [(t, l) for t, l in lines if l.startswith("done:")][-1]
    steps = (iters - 10) * T * N
    print("KBENCH " + json.dumps({"learner": learner, "envs": N, "iters": iters, "window": "first progress line (iteration 10) to the driver's done line",
                                  "window_timesteps": steps, "window_s": round(t_done - t10, 4), "timesteps_per_s": round(steps / (t_done - t10)),
                                  "driver_summary": summary}), flush=True)


def child(args, limit, tree=None):
    """one GPU step in a process of its own, under its own time limit; returns its KBENCH document.  tree: the checkout whose package it imports"""
    env = dict(os.environ, SO100_KBENCH_TREE=os.path.abspath(tree)) if tree else None
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit, cwd=ROOT, env=env)
    if out.returncode != 0:
        raise SystemExit(f"step {args} failed ({out.returncode}); nothing further is started\n{out.stdout[-2000:]}{out.stderr[-2000:]}")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("KBENCH ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("all", "update", "train", "terms", "rewnorm", "obsnorm", "off_only"), default="all")
    ap.add_argument("--normalize-obs", action="store_true", help="time FusedPPO.update with and without normalize_obs; writes profiles/learner_obsnorm_kbench.json")
    ap.add_argument("--parent-tree", default=None, help="--normalize-obs: a built checkout of the parent commit, for the option-off comparison")
    ap.add_argument("--normalize-reward", action="store_true", help="time FusedPPO.update with and without normalize_reward; writes profiles/learner_rewnorm_kbench.json")
    ap.add_argument("--terms", action="store_true", help="time the extended step with all terms on against the old one; writes profiles/learner_terms_kbench.json")
    ap.add_argument("--obs-dim", type=int, default=15); ap.add_argument("--learner", default="fused")
    ap.add_argument("--shuffle", choices=("torch", "device"), default="torch", help="--part update: device times FusedPPO(shuffle='device') against FusedPPO's default path")
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learner_update_kbench.json")); ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    if a.part == "update":
        return part_update(a.obs_dim, a.rounds, {"torch": 10, "fused": 100}, a.warmup, a.shuffle)      # >= 0.5 s per timed window
    if a.part == "train":
        return part_train(a.learner, a.iters)
    if a.part == "terms":
        return part_terms(a.obs_dim, a.rounds)
    if a.part == "rewnorm":
        return part_rewnorm(a.obs_dim, a.rounds, 100, a.warmup)
    if a.part == "obsnorm":
        return part_obsnorm(a.obs_dim, a.rounds, 100, a.warmup)
    if a.part == "off_only":
        return part_off_only(a.obs_dim, a.rounds, 100, a.warmup)
    if a.normalize_obs:
        doc = {"what": "FusedPPO.update (4 epochs x 8 minibatches of 32768 over 64 x 4096 samples) with and without normalize_obs, both paths, and the moments + fold alone",
               "commit": a.commit, "steps": [child(["--part", "obsnorm", "--obs-dim", str(od), "--rounds", str(a.rounds)], 300) for od in (15, 8)]}
        doc["card"] = doc["steps"][0]["card"]
        if a.parent_tree:
            order = [("parent", a.parent_tree), ("this", ROOT), ("parent", a.parent_tree), ("this", ROOT)]
            runs = [dict(child(["--part", "off_only", "--obs-dim", "15", "--rounds", str(a.rounds)], 300, tree=tree), tree=name) for name, tree in order]
            cmp = {"order": [name for name, _ in order], "runs": runs}
            for path in ("three_call_off", "one_call_off"):
                parent = [x for r in runs if r["tree"] == "parent" for x in r[path]["ms_per_update_rounds"]]
                this = [r[path]["ms_per_update"] for r in runs if r["tree"] == "this"]
                cmp[path] = {"parent_min_ms": min(parent), "parent_max_ms": max(parent), "this_medians_ms": this,
                             "this_inside_parent_spread": all(min(parent) <= x <= max(parent) for x in this),
                             "this_at_most_parent_max": all(x <= max(parent) for x in this)}
            doc["option_off_against_parent"] = cmp
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "learner_obsnorm_kbench.json")
        with open(out, "w") as f:
            json.dump(doc, f, indent=1); f.write("\n")
        print(json.dumps(doc, indent=1))
        return
    if a.normalize_reward:
        doc = {"what": "FusedPPO.update (4 epochs x 8 minibatches of 32768 over 64 x 4096 samples) with and without normalize_reward, both paths, and the pass alone",
               "commit": a.commit, "steps": [child(["--part", "rewnorm", "--obs-dim", str(od), "--rounds", str(a.rounds)], 300) for od in (15, 8)]}
        doc["card"] = doc["steps"][0]["card"]
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "learner_rewnorm_kbench.json")
        with open(out, "w") as f:
            json.dump(doc, f, indent=1); f.write("\n")
        print(json.dumps(doc, indent=1))
        return
    if a.terms:
        doc = {"what": "one minibatch step of 32768 samples (64 x 4096 chunk): so100_learner_minibatch_step against so100_learner_minibatch_step_ex",
               "commit": a.commit, "steps": [child(["--part", "terms", "--obs-dim", str(od), "--rounds", str(a.rounds)], 300) for od in (15, 8)]}
        doc["card"] = doc["steps"][0]["card"]
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "learner_terms_kbench.json")
        with open(out, "w") as f:
            json.dump(doc, f, indent=1); f.write("\n")
        print(json.dumps(doc, indent=1))
        return
    doc = {"what": "one PPO update (4 epochs x 8 minibatches of 32768 over 64 x 4096 samples) and main.py train end to end, PyTorch learner vs the HIP learner",
           "commit": a.commit, "update": [], "train": []}
    for od in (15, 8):
        doc["update"].append(child(["--part", "update", "--obs-dim", str(od), "--rounds", str(a.rounds)], 300))
    for learner in ("torch", "fused", "torch", "fused"):
        doc["train"].append(child(["--part", "train", "--learner", learner, "--iters", str(a.iters)], 300))
    doc["card"] = doc["update"][0]["card"]
    tr = {k: [t["timesteps_per_s"] for t in doc["train"] if t["learner"] == k] for k in ("torch", "fused")}
    doc["train_timesteps_per_s"] = tr
    doc["train_fused_over_torch"] = round((sum(tr["fused"]) / len(tr["fused"])) / (sum(tr["torch"]) / len(tr["torch"])), 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
