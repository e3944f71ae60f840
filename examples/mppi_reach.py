#!/usr/bin/env python3
"""A sampling planner (MPPI) for Env01 built on the trajectory query (needs a GPU): every step each env samples K action sequences of
`horizon` control steps around its current plan, So100Sim.trajectory rolls all N x K of them out from the envs' current state in one
launch, the cost of a sequence is |cube - ee| summed over the horizon (from the query's own ee and qpos rows), and the first action of
the cost-weighted mean is executed through step().  Printed next to the zero-action and the uniformly random baselines, like
examples/ik_reach.py.

--plan torch (the default) does everything around the rollout in torch.  --plan query is three calls on one stream with nothing in between:
So100Sim.plan_sample draws the candidates straight into the trajectory query's layout (Philox noise, reproducible from (seed, draw) in any language),
trajectory rolls them out, cost_blend sums the cost family of include/so100_query.h (the cube target: |cube - ee|^2 per step), takes the soft-min weights
and returns the blended plan, already shifted.  That cost is quadratic in the distance where the torch path sums norms, so the two paths have
temperatures of their own and are not expected to end at the same figure; --plan query prints both paths' lines.

    python examples/mppi_reach.py [--envs 8] [--samples 256] [--horizon 8] [--steps 100] [--contact] [--plan {torch,query}]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so100_mujoco_rl_amd.lib import ENV01, F_CUBE_PINNED, F_REFERENCE, So100Sim   # noqa: E402


class Mppi:
    """policy(sim, obs) -> action [N, 6].  plan [N, horizon, 6] is the mean sequence, shifted by one step after every call; sigma: the
    sampling noise (actions live in [-1, 1]); temperature: the softmax's, in metres summed over the horizon (plan "torch"; None: 0.02) or in
    metres squared summed over the horizon (plan "query"; None: QUERY_TEMPERATURE)."""
    QUERY_TEMPERATURE = 0.01                                         # d(sum |r|^2) = 2 |r| d(sum |r|): the torch path's 0.02 at |r| = 0.25 m

    def __init__(self, samples=256, horizon=8, sigma=0.5, temperature=None, seed=0, plan="torch"):
        if plan not in ("torch", "query"):
            raise ValueError(f"plan must be 'torch' or 'query', got {plan!r}")
        if temperature is None:
            temperature = 0.02 if plan == "torch" else self.QUERY_TEMPERATURE
        self.K, self.T, self.sigma, self.temperature = samples, horizon, sigma, temperature
        self.gen, self.seed, self.plan, self.mode, self.draw = None, seed, None, plan, 0

    def query_step(self, sim):
        """plan_sample -> trajectory -> cost_blend; self.plan is [horizon, N, 6] here, the queries' own layout"""
        if self.plan is None:
            self.plan = torch.zeros(self.T, sim.n, 6, device=sim.device)
        qpos, qvel = sim.get_state()                                 # [13, N], [12, N]
        cand = sim.plan_sample(self.plan, self.K, (self.sigma,)*5 + (0.0,), seed=self.seed, draw=self.draw, qpos=qpos.t(), qvel=qvel.t())
        self.draw += 1                                               # the jaw's sigma is 0: it does not move the end-effector point
        roll = sim.trajectory(cand["ctrl"], cand["qpos"], cand["qvel"], mode="actions")
        out = sim.cost_blend(roll["qpos"], None, cand["ctrl"], self.K, temperature=self.temperature, bad_step=roll["bad_step"], u_fallback=self.plan,
                             shift=1, tail="zero", target_mode="cube")
        self.plan = out["u_plan"]
        return out["u_first"].contiguous()

    def __call__(self, sim, obs):
        if self.mode == "query":
            return self.query_step(sim)
        N, K, T = sim.n, self.K, self.T
        if self.plan is None:
            self.plan = torch.zeros(N, T, 6, device=sim.device)
            self.gen = torch.Generator(device=sim.device).manual_seed(self.seed)
        eps = torch.randn(N, K, T, 6, device=sim.device, generator=self.gen)
        eps[:, 0] = 0.0                                              # the plan itself is one of the candidates
        cand = (self.plan[:, None] + self.sigma*eps).clamp(-1.0, 1.0)
        cand[..., 5] = 0.0                                           # the jaw does not move the end-effector point
        qpos, qvel = sim.get_state()                                 # [13, N], [12, N]
        start_q = qpos.t().repeat_interleave(K, dim=0); start_v = qvel.t().repeat_interleave(K, dim=0)      # problem n K + k
        ctrl = cand.reshape(N*K, T, 6).permute(1, 0, 2).contiguous()
        roll = sim.trajectory(ctrl, start_q, start_v, mode="actions")
        cost = (roll["qpos"][:, :, 6:9] - roll["ee"]).norm(dim=2).sum(dim=0).reshape(N, K)
        cost = torch.where(roll["bad_step"].reshape(N, K) >= 0, torch.full_like(cost, float("inf")), cost)
        w = torch.softmax(-(cost - cost.min(dim=1, keepdim=True).values)/self.temperature, dim=1)
        self.plan = (w[:, :, None, None]*cand).sum(dim=1)
        act = self.plan[:, 0].contiguous()
        self.plan = torch.cat([self.plan[:, 1:], torch.zeros(N, 1, 6, device=sim.device)], dim=1)
        return act


def distance(sim):
    """mean |cube - ee| from the handle's state: the cube's position (rows 6..8 of qpos) against the end-effector point of the queries"""
    cube = sim.get_state()[0][6:9].t()
    return (cube - sim.kinematics()["ee"]).norm(dim=1).mean().item()


def run(sim, steps, policy):
    """(mean |cube - ee| at reset, the same after `steps` steps, mean reward per step) of `policy(sim, obs) -> action`, both distances
    read from the state"""
    obs = sim.reset()
    d0 = distance(sim)
    total = 0.0
    for _ in range(steps):
        obs, rew, _, _ = sim.step(policy(sim, obs))
        total += rew.mean().item()
    return d0, distance(sim), total/steps


def zero_action(sim, obs):
    return torch.zeros(sim.n, 6, device=sim.device)


def random_action(sim, obs):
    return torch.rand(sim.n, 6, device=sim.device)*2.0 - 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8); ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=8); ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--contact", action="store_true", help="the reference scene's contacts (default: contact disabled, cube pinned)")
    ap.add_argument("--plan", choices=("torch", "query"), default="torch", help="torch: sample and re-weight in torch; query: plan_sample -> trajectory -> cost_blend")
    args = ap.parse_args()
    torch.manual_seed(0)
    # --plan query prints both MPPI lines: the torch path's (the default's, unchanged) and the query path's with its own temperature
    planners = [("MPPI", Mppi(args.samples, args.horizon))]
    if args.plan == "query":
        query = Mppi(args.samples, args.horizon, plan="query")
        planners.append(("MPPI (query)", query))
        print(f"temperature: torch path {planners[0][1].temperature} m, query path {query.temperature} m^2, each summed over the horizon")
    for name, policy in planners + [("zero action", zero_action), ("random", random_action)]:
        sim = So100Sim(ENV01, args.envs, flags=F_REFERENCE if args.contact else F_CUBE_PINNED, max_episode_steps=0, seed=0)
        d0, d1, r = run(sim, args.steps, policy)
        print(f"{name:12s} mean |cube - ee|: {d0:.4f} m at reset -> {d1:.4f} m after {args.steps} steps; reward/step {r:+.4f}")
        sim.close()


if __name__ == "__main__":
    main()
