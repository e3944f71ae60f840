#!/usr/bin/env python3
"""A "held" detector built on the forward-dynamics query (needs a GPU): Env01 under F_CONTACT5, the gripper horizontal with the cube
floating between the finger pads, the jaw closing on it.  Every step So100Sim.forward() -- mj_forward on the handle's own state, which it
only reads -- gives the normal force on each of the eight pads; a cube is held when both jaws carry force.

    python examples/grasp_probe.py [--envs 64] [--steps 12]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so100_mujoco_rl_amd.lib import ENV01, F_CONTACT5, So100Sim   # noqa: E402

FIXED_JAW_PADS, MOVING_JAW_PADS = slice(0, 4), slice(4, 8)     # pads 0..3 sit on Fixed_Jaw (link 4), 4..7 on Moving_Jaw (link 5)
GRASP_Q = (0.0, -1.9, 1.6, 0.3, 1.5708, 0.1)                  # gripper horizontal 28 cm above the table, closing direction along world x
CUBE_IN_JAW = (-0.0026, -0.088, 0.0)                          # the cube's centre in Fixed_Jaw's frame: between the pads, 0.5 mm off the fixed ones
CUBE_QUAT = (0.0, 0.0, 1.0, 0.0)                              # cube axes = jaw axes


def grasp_state(sim, seed=0):
    """qpos [13, N], qvel [12, N]: the pose above with the jaw 0.07 .. 0.08 rad open (its pads 0.35 .. 0.85 mm from the cube) and the cube
    shifted by up to 0.2 / 2 / 2 mm, so that nothing touches yet; the cube's place follows from Fixed_Jaw's pose, which the kinematics query gives"""
    n = sim.n
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.tensor(GRASP_Q).repeat(n, 1)
    q[:, 5] = 0.07 + 0.01*torch.rand(n, generator=g)
    kin = sim.kinematics(q.to(sim.device))
    centre = kin["xpos"][:, 4] + (kin["xmat"][:, 4] @ torch.tensor(CUBE_IN_JAW, device=sim.device))
    centre = centre + ((torch.rand(n, 3, generator=g)*2 - 1)*torch.tensor([0.0002, 0.002, 0.002])).to(sim.device)
    qpos = torch.cat([q.to(sim.device), centre, torch.tensor(CUBE_QUAT, device=sim.device).repeat(n, 1)], dim=1)
    return qpos.t().contiguous(), torch.zeros(12, n, device=sim.device)


def probe(sim):
    """(force on the fixed jaw's pads [N], on the moving jaw's [N], held [N]) at the handle's current state"""
    pad = sim.forward()["pad_force"]
    fixed, moving = pad[:, FIXED_JAW_PADS].sum(dim=1), pad[:, MOVING_JAW_PADS].sum(dim=1)
    return fixed, moving, (fixed > 0) & (moving > 0)


def run(envs, steps, verbose=False):
    """the probe at reset and after each of `steps` env steps with the jaw closing as fast as the action allows; one dict of numpy arrays per row"""
    sim = So100Sim(ENV01, envs, flags=F_CONTACT5, seed=0)
    sim.reset()
    sim.set_state(*grasp_state(sim))
    act = torch.zeros(envs, 6, device=sim.device); act[:, 5] = -1.0
    log = []
    for t in range(steps + 1):
        if t:
            sim.step(act)
        fixed, moving, held = (x.cpu().numpy() for x in probe(sim))
        log.append({"fixed": fixed, "moving": moving, "held": held})
        if verbose:
            print(f"step {t:3d}  fixed jaw {fixed.mean():7.3f} N (max {fixed.max():7.3f})  moving jaw {moving.mean():7.3f} N (max {moving.max():7.3f})  "
                  f"held {int(held.sum()):4d} of {envs}")
    sim.close()
    return log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64); ap.add_argument("--steps", type=int, default=12)
    args = ap.parse_args()
    log = run(args.envs, args.steps, verbose=True)
    print(f"held at some step: {int(np.any([row['held'] for row in log], axis=0).sum())} of {args.envs} envs")


if __name__ == "__main__":
    main()
