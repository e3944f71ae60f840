#!/usr/bin/env python3
"""A cross-entropy planner (CEM) for Env01 on the queries alone (needs a GPU).  Every control step each env runs `--iters` rounds of three calls on
one stream with nothing in between: So100Sim.plan_sample_tv draws K candidates around the current mean with the current per-entry sigma,
trajectory rolls all N x K of them out from the envs' state, cost_refit takes the E cheapest by the cost family of include/so100_query.h (the cube
target: |cube - ee|^2 per step) and refits mean and sigma to them.  The last round shifts both for the receding horizon, and the first action of
its mean is executed through step().  `draw` goes up every round, so every round has noise of its own.  Printed next to the zero-action and the
uniformly random baselines of examples/mppi_reach.py, whose distance, run and baselines this imports.

    python examples/cem_reach.py [--envs 8] [--samples 256] [--elites 32] [--horizon 8] [--iters 3] [--steps 100] [--contact]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mppi_reach import random_action, run, zero_action                             # noqa: E402
from so100_mujoco_rl_amd.lib import ENV01, F_CUBE_PINNED, F_REFERENCE, So100Sim   # noqa: E402


class Cem:
    """policy(sim, obs) -> action [N, 6].  mean and sigma [horizon, N, 6] are the queries' own layout; sigma starts at sigma_init (the jaw's is 0: it
    does not move the end-effector point) and stays within [sigma_min, sigma_init]; alpha: the share of the old mean and sigma kept per round."""

    def __init__(self, samples=256, elites=None, horizon=8, iters=3, sigma_init=0.5, sigma_min=0.05, alpha=0.1, seed=0):
        self.K, self.E, self.T, self.iters = samples, (max(1, samples//8) if elites is None else elites), horizon, iters
        self.init, self.lo, self.alpha, self.seed = (sigma_init,)*5 + (0.0,), (sigma_min,)*5 + (0.0,), alpha, seed
        self.mean, self.sigma, self.draw = None, None, 0

    def __call__(self, sim, obs):
        if self.mean is None:
            self.mean = torch.zeros(self.T, sim.n, 6, device=sim.device)
            self.sigma = torch.tensor(self.init, device=sim.device).expand(self.T, sim.n, 6)
        qpos, qvel = sim.get_state()                                 # [13, N], [12, N]
        for it in range(self.iters):
            cand = sim.plan_sample_tv(self.mean, self.K, self.sigma, seed=self.seed, draw=self.draw, qpos=qpos.t(), qvel=qvel.t())
            self.draw += 1
            roll = sim.trajectory(cand["ctrl"], cand["qpos"], cand["qvel"], mode="actions")
            out = sim.cost_refit(roll["qpos"], None, cand["ctrl"], self.K, self.E, alpha=self.alpha, plan=self.mean, sigma=self.sigma, sigma_min=self.lo,
                                 sigma_max=self.init, sigma_init=self.init, bad_step=roll["bad_step"], u_fallback=self.mean,
                                 shift=int(it == self.iters - 1), tail="zero", target_mode="cube")
            self.mean, self.sigma = out["mean"], out["sigma_out"]
        return out["u_first"].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8); ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--elites", type=int, default=None, help="default: samples / 8")
    ap.add_argument("--horizon", type=int, default=8); ap.add_argument("--iters", type=int, default=3); ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--contact", action="store_true", help="the reference scene's contacts (default: contact disabled, cube pinned)")
    args = ap.parse_args()
    torch.manual_seed(0)
    for name, policy in [("CEM", Cem(args.samples, args.elites, args.horizon, args.iters)), ("zero action", zero_action), ("random", random_action)]:
        sim = So100Sim(ENV01, args.envs, flags=F_REFERENCE if args.contact else F_CUBE_PINNED, max_episode_steps=0, seed=0)
        d0, d1, r = run(sim, args.steps, policy)
        print(f"{name:12s} mean |cube - ee|: {d0:.4f} m at reset -> {d1:.4f} m after {args.steps} steps; reward/step {r:+.4f}")
        sim.close()


if __name__ == "__main__":
    main()
