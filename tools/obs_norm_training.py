#!/usr/bin/env python3
"""`main.py -a PPO train --iters 100 --learner fused` with and without --normalize-obs, seeds 0-2, on Env01-v1 and Env05-v1 (needs a GPU):
what the update sees with raw and with normalised observations.  Reported, not judged: the option stays off by default.

    python tools/obs_norm_training.py [--out profiles/obs_norm_training.json] [--commit LABEL] [--iters 100] [--envs 4096]

Each run is the driver itself in a child process under its own time limit (the first that fails ends the tool); the learner's update() is
wrapped to keep the statistics it returns.  Per run: value_loss, explained_variance and the pre-clip grad_norm of the last minibatch at
iterations 1, 10, 50 and the last, their means over the last ten iterations, the share of iterations whose last minibatch was clipped
(grad_norm > max_grad_norm 0.5), the driver's best evaluation reward and, with the option, the running mean and std per dimension at the end.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("value_loss", "explained_variance", "grad_norm")
ENVIRONMENTS = ("Env01-v1", "Env05-v1")


def run(environment, seed, normalize, iters, envs):
    import logging
    from click.testing import CliRunner
    from so100_mujoco_rl_amd import main as drv
    hist, lines, made = [], [], []
    make = drv.make_ppo_learner

    def recording(*a, **kw):
        learner = make(*a, **kw)
        update = learner.update

        def wrapped(b, **k):
            s = update(b, **k)
            hist.append(s)
            return s
        learner.update = wrapped
        made.append(learner)
        return learner
    drv.make_ppo_learner = recording
    h = logging.Handler(); h.emit = lambda rec: lines.append(rec.getMessage())
    drv.logger.addHandler(h)
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        args = ["-a", "PPO", "train", "-e", environment, "--envs", str(envs), "--iters", str(iters), "--seed", str(seed), "--learner", "fused"]
        r = CliRunner().invoke(drv.cli, args + (["--normalize-obs"] if normalize else []), catch_exceptions=False)
        os.chdir(ROOT)
    assert r.exit_code == 0 and len(hist) == iters, r.output
    best = float(re.search(r"best evaluation reward (\S+)", [l for l in lines if l.startswith("done:")][-1]).group(1))
    at = sorted({1, 10, 50, iters} & set(range(1, iters + 1)))
    tail = hist[-10:]
    doc = {"environment": environment, "seed": seed, "normalize_obs": normalize, "iters": iters, "envs": envs, "best_evaluation_reward": best,
           "mean_reward_per_step_last": hist[-1]["mean_reward"],
           "at_iteration": {str(i): {k: hist[i - 1][k] for k in KEYS} for i in at},
           "mean_of_last_10": {k: sum(s[k] for s in tail) / len(tail) for k in KEYS},
           "share_of_iterations_clipped": sum(s["grad_norm"] > 0.5 for s in hist) / len(hist)}
    if normalize:
        sd = made[-1].obs_norm_state()
        doc["obs_mean_last"] = [round(x, 5) for x in sd["mean"].tolist()]
        doc["obs_std_last"] = [round(x ** 0.5, 5) for x in sd["var"].tolist()]
    print("TRAINING " + json.dumps(doc), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_norm_training.json")); ap.add_argument("--commit", default="unknown")
    ap.add_argument("--iters", type=int, default=100); ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--environment", default=None); ap.add_argument("--seed", type=int, default=None); ap.add_argument("--normalize-obs", action="store_true")
    a = ap.parse_args()
    if a.seed is not None:
        return run(a.environment or ENVIRONMENTS[0], a.seed, a.normalize_obs, a.iters, a.envs)
    runs = []
    for environment in ([a.environment] if a.environment else ENVIRONMENTS):
        for seed in (0, 1, 2):
            for normalize in (False, True):
                cmd = [sys.executable, os.path.abspath(__file__), "--environment", environment, "--seed", str(seed), "--iters", str(a.iters), "--envs", str(a.envs)] + \
                    (["--normalize-obs"] if normalize else [])
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
                if out.returncode != 0:
                    raise SystemExit(f"run {cmd[2:]} failed ({out.returncode}); nothing further is started\n{out.stdout[-2000:]}{out.stderr[-2000:]}")
                runs.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("TRAINING ")][-1][9:]))
                print(f"{environment} seed {seed} normalize_obs {normalize}: best evaluation reward {runs[-1]['best_evaluation_reward']}", flush=True)
    import torch
    doc = {"what": "main.py -a PPO train --learner fused, with and without --normalize-obs: the last minibatch's statistics per update",
           "commit": a.commit, "card": torch.cuda.get_device_name(0), "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
