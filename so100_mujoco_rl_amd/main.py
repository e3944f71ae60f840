"""Experiment driver with the reference's CLI surface (ref: /root/reference/src/so100_mujoco_rl/main.py:241-284):

    python -m so100_mujoco_rl_amd.main -a PPO [-m MODEL] train  -e Env01-v1 [--envs 4096] [--iters N] [--learner torch|fused] [--shuffle torch|device]
                                                               [--ent-coef C] [--clip-range-vf C] [--target-kl K]
                                                               [--normalize-advantage batch|minibatch] [--lr-schedule constant|linear]
                                                               [--normalize-reward] [--normalize-obs]
    python -m so100_mujoco_rl_amd.main -a PPO [-m MODEL] test   -e Env01-v1 [--show-io] [--show-i]
    python -m so100_mujoco_rl_amd.main -a PPO [-m MODEL] record -e Env01-v1 [--steps 3000] [--video/--no-video]
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m so100_mujoco_rl_amd.main -a PPO train -e Env01-v1     # 8 x 4096 envs

Same directory layout (models/ logs/ movies/), default model path models/{env}_{algo}/best_model.*, reward thresholds
(6000 / 8000, ref: __init__.py:9,16) and checkpoint naming ({env}_{algo}_cp_*, ref: main.py:227-232).  Differences, all
forced by the environment being a batched GPU simulator: N envs instead of 1; the learner is stable-baselines3 when it
is importable and the built-in PPO (ppo.py) or DDPG (ddpg.py; ref: main.py:38-55), both with SB3-compatible state_dicts, otherwise; `record` writes a state trajectory
(.npz) beside its video, which is a Motion-JPEG AVI (video.py) of the GPU ray caster's frames (DESIGN.md "Rendering") instead of
VecVideoRecorder's MP4.
"""
import logging
import os
import time

import click
import numpy as np
import torch

from . import constants as K
import torch.distributed as dist

from .callbacks import EvalCallback, StopTrainingOnNoModelImprovement, StopTrainingOnRewardThreshold
from .collector import RolloutCollector
from .ddpg import DDPG, DDPGPolicy
from .lib import F_REFERENCE
from .ppo import PPO, ActorCritic, FusedPPO, fold_obs_norm
from .rollout import broadcast_policy
from .vec_env import So100VecEnv, kind_from_id

logging.basicConfig(level=logging.INFO, format="%(message)s")
logger = logging.getLogger("so100")

MODEL_DIR, LOG_DIR, RECORDING_DIR = "models", "logs", "movies"          # ref: main.py:28-30


def _have_sb3():
    try:
        import stable_baselines3  # noqa: F401
        return True
    except Exception:
        return False


def _default_model_path(environment, algorithm):
    return os.path.join(MODEL_DIR, f"{environment}_{algorithm}", "best_model.zip" if _have_sb3() else "best_model.pt")


NATIVE_ALGORITHMS = ("PPO", "DDPG")


def _load_native(path, obs_dim, device, algorithm="PPO"):
    """the policy of a model file, taking RAW observations: with <model>.obs_norm.pt beside it (train --normalize-obs) the weights are folded over
    the saved statistics; without it the file's own weights run"""
    net = (DDPGPolicy(obs_dim) if algorithm == "DDPG" else ActorCritic(obs_dim)).to(device)
    sd = torch.load(path, map_location=device, weights_only=True)
    side = _obs_norm_path(path)
    if algorithm == "PPO" and os.path.isfile(side):
        sd = fold_obs_norm(sd, torch.load(side, map_location="cpu", weights_only=True))
        logger.info(f"Observation normalisation: folded the statistics of {side} into the policy")
    net.load_state_dict(sd)
    return net


@click.group()
@click.option("-a", "--algorithm", required=True, type=str, default="PPO", help="algorithm (PPO and DDPG natively; any Stable-Baselines3 name when SB3 is installed)")
@click.option("-m", "--model", default=None, type=click.Path(exists=False), help="Path to model file")
@click.pass_context
def cli(ctx, algorithm, model):
    if not _have_sb3() and algorithm not in NATIVE_ALGORITHMS:
        raise RuntimeError(f"algorithm {algorithm} needs stable-baselines3, which is not installed; the built-in learners are {' and '.join(NATIVE_ALGORITHMS)}")
    ctx.ensure_object(dict)
    ctx.obj["ALGORITHM_NAME"] = algorithm
    ctx.obj["MODEL_PATH"] = model
    for d in (MODEL_DIR, LOG_DIR, RECORDING_DIR):
        os.makedirs(d, exist_ok=True)


@cli.command(name="train", help="Train a model with a given environment")
@click.option("-e", "--environment", required=True, type=str, help="id of the environment (eg; Env01-v1)")
@click.option("--envs", default=4096, type=int, help="envs stepped in parallel on the GPU")
@click.option("--iters", default=0, type=int, help="PPO updates (0 = until the reward threshold / no improvement)")
@click.option("--seed", default=0, type=int)
@click.option("--learner", "learner_kind", default="torch", type=click.Choice(["torch", "fused"]),
              help="built-in PPO update: PyTorch autograd (torch) or the library's HIP kernels (fused; include/so100_learn.h)")
@click.option("--ent-coef", default=None, type=float, help="entropy bonus coefficient (SB3 ent_coef; default 0)")
@click.option("--clip-range-vf", default=None, type=float, help="value clipping range (SB3 clip_range_vf; default none)")
@click.option("--target-kl", default=None, type=float, help="stop an update once approx_kl exceeds 1.5 x this (SB3 target_kl; default none)")
@click.option("--normalize-advantage", default=None, type=click.Choice(["batch", "minibatch"]),
              help="advantage normalisation over the whole rollout chunk (batch, the default) or per minibatch as SB3 does")
@click.option("--lr-schedule", default=None, type=click.Choice(["constant", "linear"]), help="learning rate 3e-4 (constant, the default) or 3e-4 x remaining progress (linear; needs --iters)")
@click.option("--shuffle", default="torch", type=click.Choice(["torch", "device"]),
              help="minibatch permutations of --learner fused: torch.randperm (torch) or the library's, a function of seed and epoch; the whole update is then one call (device)")
@click.option("--normalize-reward", is_flag=True, default=False,
              help="train on rewards divided by the running std of the envs' discounted returns (SB3 VecNormalize(norm_reward=True)); the state is saved beside each model")
@click.option("--normalize-obs", is_flag=True, default=False,
              help="train on observations normalised by their running mean and std (SB3 VecNormalize(norm_obs=True), folded into the policy's first layer); "
                   "the statistics are saved beside each model")
@click.pass_context
def train(ctx, environment, envs, iters, seed, learner_kind, ent_coef, clip_range_vf, target_kl, normalize_advantage, lr_schedule, shuffle, normalize_reward,
          normalize_obs):
    algorithm = ctx.obj["ALGORITHM_NAME"]
    if shuffle == "device" and learner_kind != "fused":
        raise RuntimeError("--shuffle device is the fused learner's on-device shuffle: it needs --learner fused")
    if lr_schedule == "linear" and iters <= 0:
        raise RuntimeError("--lr-schedule linear needs --iters > 0: the schedule runs over a known number of updates")
    # SB3's remaining PPO options: given on the command line, they reach whichever learner runs and a second log line shows their diagnostics.
    # `--normalize-advantage batch` and `--lr-schedule constant` name what runs anyway: they select nothing and print nothing more.
    terms = {k: v for k, v in (("ent_coef", ent_coef), ("clip_range_vf", clip_range_vf), ("target_kl", target_kl)) if v is not None}
    if normalize_advantage == "minibatch":
        terms["normalize_advantage"] = "minibatch"
    if lr_schedule == "linear":
        terms["lr_schedule"] = lambda progress: PPO_LR * progress
    if normalize_reward:
        terms["normalize_reward"] = True
    if normalize_obs:
        terms["normalize_obs"] = True
    if terms and algorithm != "PPO":
        raise RuntimeError("--ent-coef, --clip-range-vf, --target-kl, --normalize-advantage, --lr-schedule, --normalize-reward and --normalize-obs are PPO's options")
    kind = kind_from_id(environment)
    # Multi-GPU (one process per GPU under torchrun): rank r steps global envs [r*envs, (r+1)*envs); once per rollout chunk the
    # packed rollout goes to rank 0 over RCCL (the path's ONE collective), rank 0 learns, the policy is broadcast back.
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0")); local = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1 or os.environ.get("SO100_FORCE_DIST") == "1"      # SO100_FORCE_DIST: the same code path on a one-GPU box
    if normalize_reward and distributed:
        # a gathered chunk is bootstrapped by each rank before the gather, which would put gamma * V under the normalisation
        raise RuntimeError("--normalize-reward runs on one GPU: with WORLD_SIZE > 1 the TimeLimit bootstrap is applied before the gather, ahead of the "
                           "normalisation (the multi-GPU order cannot be tested on one card, so it is not offered)")
    if normalize_obs and distributed:
        raise RuntimeError("--normalize-obs runs on one GPU: with WORLD_SIZE > 1 every rank's collector would need the folded policy of statistics only "
                           "rank 0 holds (the multi-GPU order cannot be tested on one card, so it is not offered)")
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29544")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        if _have_sb3():
            raise RuntimeError("multi-GPU training uses the built-in PPO learner; run SB3 single-GPU")
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    lead = rank == 0
    env = So100VecEnv(environment, envs, device=torch.device("cuda", local) if distributed else None, flags=F_REFERENCE, seed=seed,
                      env_id_offset=rank * envs, stagger_episodes=True)
    save_dir = os.path.join(MODEL_DIR, f"{environment}_{algorithm}")
    os.makedirs(save_dir, exist_ok=True)
    if lead:
        logger.info("Starting training process"); logger.info(f"Algorithm: {algorithm}"); logger.info(f"Environment: {environment} x {envs}" + (f" x {world} GPUs" if distributed else ""))
    if learner_kind == "fused" and (_have_sb3() or algorithm != "PPO"):
        raise RuntimeError("--learner fused selects the built-in PPO learner's kernels; it does not apply to " + ("stable-baselines3" if _have_sb3() else algorithm))
    if _have_sb3():                                          # unchanged SB3 learner over the batched VecEnv (ref: main.py:199-238)
        import stable_baselines3
        from stable_baselines3.common.callbacks import CheckpointCallback
        cls = getattr(stable_baselines3, algorithm)
        model_file = ctx.obj["MODEL_PATH"]
        sb3_terms = {k: v for k, v in terms.items() if k in ("ent_coef", "clip_range_vf", "target_kl")}
        if normalize_reward or normalize_obs:
            from stable_baselines3.common.vec_env import VecNormalize
            env = VecNormalize(env, norm_obs=normalize_obs, norm_reward=normalize_reward)
        if "normalize_advantage" in terms:
            sb3_terms["normalize_advantage"] = True          # "minibatch" is SB3's own normalisation (and its default); it has no per-chunk one
        if "lr_schedule" in terms:
            sb3_terms["learning_rate"] = terms["lr_schedule"]
        model = cls.load(model_file, env=env, tensorboard_log=LOG_DIR) if model_file else cls("MlpPolicy", env, verbose=1, device="cuda", tensorboard_log=LOG_DIR, **sb3_terms)
        cb = CheckpointCallback(save_freq=max(1, 40000 // envs), save_path=save_dir, name_prefix=f"{environment}_{algorithm}_cp_", verbose=2)
        model.learn(total_timesteps=int(1e10) if iters == 0 else iters * 64 * envs, tb_log_name=f"{environment}_{algorithm}", callback=cb)
        model.save(os.path.join(save_dir, "best_model"))
        return
    if algorithm == "DDPG":
        if distributed:
            raise RuntimeError("multi-GPU training uses the built-in PPO learner; DDPG runs on one GPU")
        return _train_ddpg(env, environment, ctx.obj["MODEL_PATH"], save_dir, iters, seed, kind)
    if shuffle == "device":
        terms["shuffle"] = "device"
    learner = make_ppo_learner(learner_kind, env.sim.obs_dim, env.device, seed, **terms)
    if ctx.obj["MODEL_PATH"]:
        if not os.path.isfile(ctx.obj["MODEL_PATH"]):
            raise RuntimeError(f"Model file {ctx.obj['MODEL_PATH']} does not exist")
        learner.net.load_state_dict(torch.load(ctx.obj["MODEL_PATH"], map_location=env.device, weights_only=True))
        logger.info(f"Model: starting with {ctx.obj['MODEL_PATH']}")
        if normalize_reward:
            side = _reward_norm_path(ctx.obj["MODEL_PATH"])
            if os.path.isfile(side):
                learner.load_reward_norm_state(torch.load(side, map_location="cpu", weights_only=True))
                logger.info(f"Reward normalisation: reloaded the running state from {side}")
            else:
                logger.info(f"Reward normalisation: no saved state at {side}, starting from a fresh one")
        if normalize_obs:
            side = _obs_norm_path(ctx.obj["MODEL_PATH"])
            if os.path.isfile(side):
                learner.load_obs_norm_state(torch.load(side, map_location="cpu", weights_only=True))
                logger.info(f"Observation normalisation: reloaded the running statistics from {side}")
            else:
                logger.info(f"Observation normalisation: no saved statistics at {side}, starting from fresh ones")
        elif os.path.isfile(_obs_norm_path(ctx.obj["MODEL_PATH"])):
            logger.warning(f"Observation normalisation: {_obs_norm_path(ctx.obj['MODEL_PATH'])} says this model was trained on normalised observations; "
                           "without --normalize-obs training continues on raw ones")
    else:
        logger.info("Model: starting with new model")
    if normalize_reward:
        logger.info(f"Reward normalisation: on (running std of the discounted returns, clip {learner.clip_reward:g}); evaluation and reward/step stay in the env's scale")
    if normalize_obs:
        logger.info("Observation normalisation: on (running mean and std per dimension, updated once per chunk, folded into the first layer; no clipping)")
    if distributed:
        broadcast_policy(list(learner.net.state_dict().values()), src=0)          # every rank starts from rank 0's weights
    # fused on one GPU: the advantage kernel applies the TimeLimit bootstrap (the chunk keeps the env's rewards); a gathered chunk is bootstrapped
    # by each rank before the gather, as with the torch learner
    # --normalize-reward, either learner: the bootstrap must follow the normalisation, so it is deferred to the learner as well
    # --normalize-obs: the collectors run the FOLDED policy on raw observations (policy_state_dict(); net.state_dict() without the option)
    col = RolloutCollector(env, learner.policy_state_dict(), T=64, defer_bootstrap=(learner_kind == "fused" or normalize_reward) and not distributed)
    threshold = K.REWARD_THRESHOLD[kind]                     # StopTrainingOnRewardThreshold (ref: main.py:211; the registered threshold of the env id)
    steps, t0, it = 0, time.time(), 0
    ep_sum = ep_cnt = 0.0
    stop = torch.zeros(1, device=env.device)
    eval_cb = None
    if lead:
        # ref: main.py:211-225 -- EvalCallback(best_model_save_path, callback_on_new_best = StopTrainingOnRewardThreshold, callback_after_eval =
        # StopTrainingOnNoModelImprovement(max_no_improvement_evals=5, min_evals=10000)), restated for the built-in learner (callbacks.py).  The reference
        # evaluates every 20 000 timesteps of ONE env; here an update is 64 x envs timesteps, so an evaluation every EVAL_EVERY updates.
        eval_env = So100VecEnv(environment, N_EVAL_EPISODES, device=env.device, flags=F_REFERENCE, seed=seed + 1000)
        eval_col = RolloutCollector(eval_env, learner.policy_state_dict(), T=64, bootstrap_truncated=False)
        eval_cb = EvalCallback(lambda: _evaluate(eval_env, eval_col, learner), lambda: _save_model(learner, os.path.join(save_dir, "best_model.pt")),
                               EVAL_EVERY, on_new_best=StopTrainingOnRewardThreshold(threshold), after_eval=StopTrainingOnNoModelImprovement(5, 10000), log=logger.info)
    while True:
        b = col.collect(gather_dst=0 if distributed else None)
        it += 1
        if lead:
            done = (b["dones"] > 0).any(0)[:envs]            # episode statistics from this rank's own envs
            if done.any():                                   # ep_return holds the return of the latest episode that ended in the chunk
                ep_sum += env.sim.ep_return[done].sum().item(); ep_cnt += int(done.sum().item())
            stats = learner.update(b, progress_remaining=1.0 - it / iters) if iters else learner.update(b)      # SB3's progress_remaining at the time of train()
            steps += b["rewards"].numel()
            if it % 10 == 0:
                mean_ep = ep_sum / ep_cnt if ep_cnt else float("nan")
                logger.info(f"iter {it:5d}  timesteps {steps/1e6:8.1f} M  reward/step {stats['mean_reward']:+.4f}  ep_rew_mean {mean_ep:9.2f}  "
                            f"value_loss {stats['value_loss']:.4f}  fps {steps/(time.time()-t0)/1e6:.1f} M")
                dropped = int(env.sim.contacts_dropped().max().item())
                if dropped > 0:                              # over the contact budget: this step deviates from the reference model (MuJoCo keeps every contact)
                    logger.warning(f"contact budget exceeded: up to {dropped} contacts dropped in an env of the last step")
                ep_sum = ep_cnt = 0.0
            if terms and (it % 10 == 0 or (iters and it >= iters)):
                logger.info(f"iter {it:5d}  approx_kl {stats['approx_kl']:.5f}  entropy_loss {stats['entropy_loss']:.4f}  loss {stats['loss']:.4f}  "
                            f"explained_variance {stats['explained_variance']:.4f}  std {stats['std']:.4f}  n_updates {stats['n_updates']}"
                            + (f"  return_std {stats['return_var'] ** 0.5:.4f}" if normalize_reward else "") + ("  (early stop)" if stats["early_stop"] else ""))
            if not eval_cb.step():
                logger.info(f"Stopping training: best evaluation reward {eval_cb.best_mean_reward:.1f} (threshold {threshold})"); stop.fill_(1.0)
            if it % 40 == 0:                                 # CheckpointCallback (ref: main.py:227-232)
                _save_model(learner, os.path.join(save_dir, f"{environment}_{algorithm}_cp__{steps}_steps.pt"))
            if iters and it >= iters:
                stop.fill_(1.0)
        if distributed:
            broadcast_policy(list(learner.net.state_dict().values()) + [stop], src=0)
        col.load_policy(learner.policy_state_dict())
        if stop.item() > 0:
            break
    if lead and eval_cb.n_evals == 0:                        # a short run (--iters): one evaluation at the end, so that best_model exists
        eval_cb.eval_every = 1; eval_cb.step()
    if lead:
        _save_model(learner, os.path.join(save_dir, "last_model.pt"))
        logger.info(f"done: {steps/1e6:.1f} M timesteps in {time.time()-t0:.1f} s; best evaluation reward {eval_cb.best_mean_reward:.1f} ({eval_cb.n_evals} evaluations); models in {save_dir}")
    if distributed:
        dist.barrier(); dist.destroy_process_group()


def _reward_norm_path(model_path):
    """<model>.reward_norm.pt beside <model>.pt: the running state of --normalize-reward (the model file stays a plain state_dict)"""
    return os.path.splitext(model_path)[0] + ".reward_norm.pt"


def _obs_norm_path(model_path):
    """<model>.obs_norm.pt beside <model>.pt: the running statistics of --normalize-obs (the model file stays the raw, unfolded state_dict)"""
    return os.path.splitext(model_path)[0] + ".obs_norm.pt"


def _save_model(learner, path):
    torch.save(learner.net.state_dict(), path)
    if getattr(learner, "normalize_reward", False):
        torch.save(learner.reward_norm_state(), _reward_norm_path(path))
    side = _obs_norm_path(path)
    if getattr(learner, "normalize_obs", False):
        torch.save(learner.obs_norm_state(), side)
    elif os.path.isfile(side):
        # a side file left by an earlier run with --normalize-obs belongs to the model this one replaces: `test` / `record` would fold its
        # statistics into a policy trained on raw observations
        os.remove(side)
        logger.info(f"Observation normalisation: removed {side}, the statistics of the model this one replaces")


PPO_LR = 3e-4                                                # the learners' default learning rate: where --lr-schedule linear starts


def make_ppo_learner(kind, obs_dim, device, seed, **terms):
    """the built-in PPO learner `train --learner` names: "torch" (ppo.PPO, the default) or "fused" (ppo.FusedPPO, HIP kernels); terms: SB3's
    remaining options (ent_coef, clip_range_vf, target_kl, normalize_advantage, lr_schedule), normalize_reward and normalize_obs, the same for
    both, and the fused learner's shuffle"""
    if kind == "torch":
        return PPO(obs_dim, device, lr=PPO_LR, seed=seed, **terms)
    if kind != "fused":
        raise RuntimeError(f"unknown learner {kind!r}: torch or fused")
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"--learner fused runs on a HIP device, not on {device}: there is no CPU fallback (use --learner torch)")
    if obs_dim not in (15, 8):
        raise RuntimeError(f"--learner fused is built for the so100 observations (obs_dim 15 or 8), not obs_dim {obs_dim}")
    return FusedPPO(obs_dim, device, lr=PPO_LR, seed=seed, **terms)


def _train_ddpg(env, environment, model_path, save_dir, iters, seed, kind):
    """The reference's DDPG branch (ref: main.py:38-55) on the built-in learner (ddpg.py): off-policy, one vector step at a time through
    the tensor API; an "iter" is 64 vector steps (the PPO driver's chunk), evaluation / stop / checkpoint callbacks as in train()."""
    learner = DDPG(env.sim.obs_dim, env.device, seed=seed, buffer_size=max(1_000_000, 16 * env.num_envs), gradient_steps=DDPG_GRADIENT_STEPS)
    if model_path:
        if not os.path.isfile(model_path):
            raise RuntimeError(f"Model file {model_path} does not exist")
        learner.net.load_state_dict(torch.load(model_path, map_location=env.device, weights_only=True))
        logger.info(f"Model: starting with {model_path}")
    else:
        logger.info("Model: starting with new model")
    threshold = K.REWARD_THRESHOLD[kind]
    eval_env = So100VecEnv(environment, N_EVAL_EPISODES, device=env.device, flags=F_REFERENCE, seed=seed + 1000)
    eval_cb = EvalCallback(lambda: _evaluate_actor(eval_env, learner.net.mean_action), lambda: torch.save(learner.net.state_dict(), os.path.join(save_dir, "best_model.pt")),
                           EVAL_EVERY, on_new_best=StopTrainingOnRewardThreshold(threshold), after_eval=StopTrainingOnNoModelImprovement(5, 10000), log=logger.info)
    obs, steps, it, t0 = None, 0, 0, time.time()
    while True:
        obs, stats = learner.learn_steps(env, 64, obs)
        it += 1; steps += 64 * env.num_envs
        if it % 10 == 0:
            logger.info(f"iter {it:5d}  timesteps {steps/1e6:8.1f} M  reward/step {stats['mean_reward']:+.4f}  critic_loss {stats.get('critic_loss', float('nan')):.4f}  "
                        f"updates {learner.n_updates}  fps {steps/(time.time()-t0)/1e6:.2f} M")
        if not eval_cb.step():
            logger.info(f"Stopping training: best evaluation reward {eval_cb.best_mean_reward:.1f} (threshold {threshold})"); break
        if it % 40 == 0:
            torch.save(learner.net.state_dict(), os.path.join(save_dir, f"{environment}_DDPG_cp__{steps}_steps.pt"))
        if iters and it >= iters:
            break
    if eval_cb.n_evals == 0:
        eval_cb.eval_every = 1; eval_cb.step()
    torch.save(learner.net.state_dict(), os.path.join(save_dir, "last_model.pt"))
    logger.info(f"done: {steps/1e6:.1f} M timesteps in {time.time()-t0:.1f} s; best evaluation reward {eval_cb.best_mean_reward:.1f} ({eval_cb.n_evals} evaluations); models in {save_dir}")


@torch.no_grad()
def _evaluate_actor(eval_env, act_fn):
    """evaluate_policy(deterministic=True) through the stepwise tensor API (any policy: obs -> action): every env's first episode."""
    obs = eval_env.reset_tensor()
    n = eval_env.num_envs
    ret = torch.zeros(n, device=eval_env.device); alive = torch.ones(n, dtype=torch.bool, device=eval_env.device)
    for _ in range(eval_env.sim.cfg.max_episode_steps + 1):
        obs, r, d, _tr = eval_env.step_tensor(act_fn(obs).clamp(-1, 1).contiguous())
        ret += torch.where(alive, r, torch.zeros_like(ret)); alive &= ~d.bool()
        if not bool(alive.any()):
            break
    return float(ret.mean().item())


DDPG_GRADIENT_STEPS = 4   # updates of 256 per VECTOR step (SB3: 1 per step of ONE env; a vector step adds `envs` transitions, see ddpg.py)
N_EVAL_EPISODES = 5       # SB3 EvalCallback's default n_eval_episodes (ref: main.py:217-224 passes none)
EVAL_EVERY = 50           # updates between evaluations (an update is 64 x envs timesteps; the reference's eval_freq is 20 000 timesteps of one env)


@torch.no_grad()
def _evaluate(eval_env, eval_col, learner):
    """SB3 evaluate_policy(deterministic=True) over N_EVAL_EPISODES episodes: one env per episode, the policy's MEAN action (log_std -> -30
    in the copy the kernels read), every env's FIRST episode after a reset; returns the mean episode reward."""
    sd = {k: v.clone() for k, v in learner.policy_state_dict().items()}
    sd["log_std"] = torch.full_like(sd["log_std"], -30.0)
    eval_col.load_policy(sd)
    eval_env.reset_tensor(); eval_col._started = True
    n = eval_env.num_envs
    ret = torch.zeros(n, device=eval_env.device); alive = torch.ones(n, dtype=torch.bool, device=eval_env.device)
    for _ in range(eval_env.sim.cfg.max_episode_steps // eval_col.T + 2):
        b = eval_col.collect()
        for t in range(b["rewards"].shape[0]):
            ret += torch.where(alive, b["rewards"][t], torch.zeros_like(ret))
            alive &= ~(b["dones"][t] > 0)
        if not bool(alive.any()):
            break
    return float(ret.mean().item())


def _rollout_policy(environment, algorithm, model_file, n, steps, show_io, show_i, record_path=None, video_path=None):
    env = So100VecEnv(environment, n, flags=F_REFERENCE, seed=1, render_mode="rgb_array" if video_path else None, render_envs=1)
    if model_file is None:
        model_file = _default_model_path(environment, algorithm)
    if not os.path.isfile(model_file):
        raise RuntimeError(f"Could not open model file: {model_file}")
    logger.info(f"Algorithm: {algorithm}"); logger.info(f"Environment: {environment}"); logger.info(f"Model: {model_file}")
    if model_file.endswith(".zip"):
        import stable_baselines3
        policy = getattr(stable_baselines3, algorithm).load(model_file, device="cuda").policy
        act_fn = lambda o: policy._predict(o, deterministic=True)
    else:
        net = _load_native(model_file, env.sim.obs_dim, env.device, algorithm)
        act_fn = net.mean_action
    obs = env.reset_tensor()
    total = 0.0; traj = []
    writer = None
    if video_path is not None:                         # ref: main.py:151-171 (VecVideoRecorder: one frame of env 0 per step)
        from .video import MjpegAviWriter
        os.makedirs(os.path.dirname(video_path) or ".", exist_ok=True)
        writer = MjpegAviWriter(video_path, *K.SCENE_CAMERA_SIZE, K.RENDER_FPS)
    with torch.no_grad():
        for t in range(steps):
            if writer is not None:
                writer.write(env.get_images()[0])
            a = act_fn(obs).clamp(-1, 1).contiguous()
            if (show_io or show_i) and t % 30 == 0:           # ref: main.py:110-113
                logger.info(str(obs[0].tolist() + (a[0].tolist() if show_io else [])) + ("," if show_i else ""))
            if record_path is not None:
                q, v = env.sim.get_state()
                traj.append(np.concatenate([q[:, 0].cpu().numpy(), v[:, 0].cpu().numpy(), obs[0].cpu().numpy(), a[0].cpu().numpy()]))
            obs, r, d, tr = env.step_tensor(a)
            total += r.mean().item()
    logger.info(f"mean reward/step over {steps} steps x {n} envs: {total/steps:+.4f}")
    if record_path is not None:
        np.savez(record_path, trajectory=np.stack(traj), layout="qpos[13] qvel[12] obs action[6] per step, env 0")
        logger.info(f"wrote {record_path} (state trajectory)")
    if writer is not None:
        writer.close()
        logger.info(f"wrote {video_path} ({writer.frames} frames, {K.SCENE_CAMERA_SIZE[0]} x {K.SCENE_CAMERA_SIZE[1]} Motion-JPEG at {K.RENDER_FPS} fps)")
    return total / steps


@cli.command(name="test", help="Test the current model")
@click.option("-e", "--environment", required=True, type=str)
@click.option("--show-io", is_flag=True, default=False, help="log model inputs and outputs")
@click.option("--show-i", is_flag=True, default=False, help="log model inputs in Python array syntax")
@click.option("--envs", default=256, type=int)
@click.option("--steps", default=1000, type=int)
@click.pass_context
def test(ctx, environment, show_io, show_i, envs, steps):
    logger.info("Starting test simulation")
    _rollout_policy(environment, ctx.obj["ALGORITHM_NAME"], ctx.obj["MODEL_PATH"], envs, steps, show_io, show_i)


@cli.command(name="record", help="Record a model with a given environment")
@click.option("-e", "--environment", required=True, type=str)
@click.option("--steps", default=3000, type=int, help="steps to record (ref: main.py:151 video_length)")
@click.option("--video/--no-video", default=True, help="also write movies/rec-<env>-step-0-to-step-<steps>.avi (Motion-JPEG)")
@click.pass_context
def record(ctx, environment, steps, video):
    path = os.path.join(RECORDING_DIR, f"{environment}_{ctx.obj['ALGORITHM_NAME']}.npz")
    # VecVideoRecorder's file name (name_prefix "rec-<env>", ref: main.py:154-160)
    video_path = os.path.join(RECORDING_DIR, f"rec-{environment}-step-0-to-step-{steps}.avi") if video else None
    _rollout_policy(environment, ctx.obj["ALGORITHM_NAME"], ctx.obj["MODEL_PATH"], 1, steps, False, False, record_path=path, video_path=video_path)


if __name__ == "__main__":
    cli(obj={})
