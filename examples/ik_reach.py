#!/usr/bin/env python3
"""A scripted reach expert for Env01 built on the model queries (needs a GPU): every step the cube position from the observation is
handed to the batched IK (So100Sim.ik), and the action steps the joints towards its answer.  A baseline to judge a learned policy's
reward per step and distance against, next to a uniformly random policy.

    python examples/ik_reach.py [--envs 1024] [--steps 200] [--contact]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so100_mujoco_rl_amd.constants import JOINT_STEP_SCALE                       # noqa: E402
from so100_mujoco_rl_amd.lib import ENV01, F_CUBE_PINNED, F_REFERENCE, So100Sim   # noqa: E402


def expert_action(sim, obs):
    """Env01 observation [N, 15] (joints 0:6, cube - ee 6:9, cube 9:12, ee 12:15) -> action [N, 6]: the IK's joints for the end-effector
    point on the cube, approached by at most one joint step per env step; the jaw (joint 5) is held.  A reset observation carries zeros
    in place of every pose (as the reference's does): such an env waits one step."""
    q = obs[:, 0:6]
    q_ik = sim.ik(obs[:, 9:12])["q"]
    act = ((q_ik - q) / JOINT_STEP_SCALE).clamp(-1.0, 1.0)
    act[:, 5] = 0.0
    act[(obs[:, 6:15] == 0).all(dim=1)] = 0.0
    return act.contiguous()


def distance(sim):
    """mean |cube - ee| from the handle's state: the cube's position (rows 6..8 of qpos) against the end-effector point of the queries"""
    cube = sim.get_state()[0][6:9].t()
    return (cube - sim.kinematics()["ee"]).norm(dim=1).mean().item()


def run(sim, steps, policy):
    """(mean |cube - ee| at reset, the same after `steps` steps, mean reward per step) of `policy(sim, obs) -> action`; the distance at
    reset is read from the state (the reset observation has no poses), the one at the end from the observation (obs[6:9] = cube - ee)"""
    obs = sim.reset()
    d0 = distance(sim)
    total = 0.0
    for _ in range(steps):
        obs, rew, _, _ = sim.step(policy(sim, obs))
        total += rew.mean().item()
    return d0, obs[:, 6:9].norm(dim=1).mean().item(), total / steps


def random_action(sim, obs):
    return torch.rand(sim.n, 6, device=sim.device) * 2.0 - 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024); ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--contact", action="store_true", help="the reference scene's contacts (default: contact disabled, cube pinned)")
    args = ap.parse_args()
    torch.manual_seed(0)
    for name, policy in (("IK expert", expert_action), ("random", random_action)):
        sim = So100Sim(ENV01, args.envs, flags=F_REFERENCE if args.contact else F_CUBE_PINNED, seed=0)
        d0, d1, r = run(sim, args.steps, policy)
        print(f"{name:10s} mean |cube - ee|: {d0:.4f} m at reset -> {d1:.4f} m after {args.steps} steps; reward/step {r:+.4f}")
        sim.close()


if __name__ == "__main__":
    main()
