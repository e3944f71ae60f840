#!/usr/bin/env python3
"""Minimal PPO on top of the on-device rollout collector (needs a GPU).  Functional evidence that the batched simulator
is a learnable stand-in for the reference's `main.py -a PPO train -e Env01-v1` loop (main.py:177-238) -- stable-baselines3
is not installed in this image, so the learner here is ~80 lines of plain PyTorch with SB3's PPO defaults
(MlpPolicy 2x64 tanh towers, gamma 0.99, gae_lambda 0.95, clip 0.2, lr 3e-4, 10 epochs are reduced to 4 for speed).

    python examples/train_ppo.py [--env Env01-v1] [--envs 4096] [--iters 150] [--learner torch|fused] [--shuffle torch|device] [--normalize-reward] [--normalize-obs]

--learner fused runs the update in the library's own kernels (include/so100_learn.h) instead of PyTorch autograd; with --shuffle device
the minibatch permutations are the library's too and the whole update is one so100_learner_update call (examples/train_ppo.cpp is that
loop without Python).  --normalize-reward trains on rewards divided by the running std of the envs' discounted returns (SB3's
VecNormalize(norm_reward=True)), with either learner; the TimeLimit bootstrap is then left to the learner, which adds it after the normalisation.
--normalize-obs is the observation half (norm_obs=True), folded into the policy's first layer: the collector runs learner.policy_state_dict()
on raw observations, the learner normalises a chunk on load under the statistics it was collected with and then merges it into them.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so100_mujoco_rl_amd.vec_env import So100VecEnv               # noqa: E402
from so100_mujoco_rl_amd.collector import RolloutCollector        # noqa: E402
from so100_mujoco_rl_amd.lib import F_REFERENCE                    # noqa: E402


from so100_mujoco_rl_amd.ppo import PPO, FusedPPO                       # noqa: E402  (the learner lives in the package)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Env01-v1"); ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=150); ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--learner", choices=("torch", "fused"), default="torch")
    ap.add_argument("--shuffle", choices=("torch", "device"), default="torch")
    ap.add_argument("--normalize-reward", action="store_true")
    ap.add_argument("--normalize-obs", action="store_true")
    args = ap.parse_args()
    if args.shuffle == "device" and args.learner != "fused":
        ap.error("--shuffle device needs --learner fused")
    env = So100VecEnv(args.env, args.envs, flags=F_REFERENCE, seed=0, stagger_episodes=True)
    dev = env.device
    fused = args.learner == "fused"
    rn = dict(normalize_reward=args.normalize_reward, normalize_obs=args.normalize_obs)
    learner = FusedPPO(env.sim.obs_dim, dev, seed=0, shuffle=args.shuffle, **rn) if fused else PPO(env.sim.obs_dim, dev, seed=0, **rn)
    # fused: the advantage kernel applies the TimeLimit bootstrap; --normalize-reward: either learner applies it, after the normalisation
    # policy_state_dict(): net.state_dict(), or with --normalize-obs its fold over the current statistics
    col = RolloutCollector(env, learner.policy_state_dict(), T=args.T, defer_bootstrap=fused or args.normalize_reward)
    t0 = time.time(); steps = 0
    for it in range(args.iters):
        b = col.collect()
        stats = learner.update(b)
        col.load_policy(learner.policy_state_dict())
        steps += args.T * args.envs
        if it % 10 == 0 or it == args.iters - 1:
            torch.cuda.synchronize()
            print(f"iter {it:4d}  env-steps {steps/1e6:7.1f} M  mean reward/step {stats['mean_reward']:+.4f}  "
                  f"value loss {stats['value_loss']:.4f}  log_std {learner.net.log_std.mean().item():+.3f}  wall {time.time() - t0:6.1f} s"
                  + (f"  return_std {stats['return_var'] ** 0.5:.4f}" if args.normalize_reward else ""), flush=True)


if __name__ == "__main__":
    main()
