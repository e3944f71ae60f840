"""Plain-PyTorch PPO on top of the on-device rollout collector -- the learner used by `main.py train` when
stable-baselines3 is not importable (it is not in this image).  Network and loss follow SB3's PPO
(ref: main.py:56-64 -> stable_baselines3.PPO("MlpPolicy")): 2x64 tanh towers, gamma 0.99, gae_lambda 0.95, clip 0.2,
lr 3e-4, vf_coef 0.5, max_grad_norm 0.5.  NOT SB3's defaults: 4 epochs instead of 10, minibatches of 32 768 instead of
64, rollouts of 64 steps x N envs instead of 2048 x 1 (the batch is 262 144 samples per update at 4096 envs).
TimeLimit truncations are bootstrapped by the collector exactly as SB3 does (rewards += gamma V(terminal_obs)), so
`dones` below ends the GAE recursion with the right target for both terminations and truncations.  (Round 1's
hipGraph-replayed update is gone: see PPO.__init__.)
The network's state_dict keys equal SB3's ActorCriticPolicy keys, so checkpoints and RolloutCollector.load_policy()
interoperate with an SB3 policy.
FusedPPO is the same learner on the library's own kernels (include/so100_learn.h): same constructor, same update(b), same state_dict.
Both take SB3's remaining options -- ent_coef, clip_range_vf, per-minibatch advantage normalisation, target_kl, a learning-rate schedule --
all off by default (then the loss is the one above, to the bit), and return SB3's per-update diagnostics.
normalize_reward=True is the reward half of SB3's VecNormalize(norm_reward=True): the rewards an update trains on are divided by the running
standard deviation of the envs' discounted returns (include/so100_learn.h "Reward normalisation" is the specification); the state carries
over from update to update and is saved and restored with reward_norm_state() / load_reward_norm_state().
normalize_obs=True is the observation half (norm_obs=True), folded into the policy (include/so100_learn.h "Observation normalisation"): the
learner normalises the raw observations of a chunk on load with the statistics the chunk was collected under, then merges the chunk into the
statistics; policy_state_dict() is the state_dict folded over the current statistics, which a collector, an evaluation or an export runs on
raw observations.  One iteration: update(chunk k), then collector.load_policy(learner.policy_state_dict()).  The state is saved and restored
with obs_norm_state() / load_obs_norm_state(); net.state_dict() stays the unfolded network."""
import math
import os

import torch
import torch.nn as nn


class ActorCritic(nn.Module):
    def __init__(self, obs_dim, act_dim=6):
        super().__init__()
        mk = lambda: nn.Sequential(nn.Linear(obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh())
        self.mlp_extractor = nn.ModuleDict({"policy_net": mk(), "value_net": mk()})
        self.action_net = nn.Linear(64, act_dim); self.value_net = nn.Linear(64, 1)
        self.log_std = nn.Parameter(torch.zeros(act_dim))
        for m, g in ((self.mlp_extractor, 2 ** 0.5), (self.action_net, 0.01), (self.value_net, 1.0)):
            for l in m.modules():
                if isinstance(l, nn.Linear):
                    nn.init.orthogonal_(l.weight, g); nn.init.zeros_(l.bias)

    def value(self, obs):
        return self.value_net(self.mlp_extractor["value_net"](obs)).squeeze(-1)

    def mean_action(self, obs):
        return self.action_net(self.mlp_extractor["policy_net"](obs))

    def evaluate(self, obs, act):
        mean = self.mean_action(obs)
        std = self.log_std.exp()
        logp = (-0.5 * ((act - mean) / std) ** 2 - self.log_std - 0.9189385332046727).sum(-1)
        return self.value(obs), logp


ENTROPY_CONST = 0.5 + 0.5 * math.log(2.0 * math.pi)      # entropy of a unit Gaussian, per action dimension


def _set_terms(learner, ent_coef, clip_range_vf, normalize_advantage, target_kl, lr_schedule):
    """checks SB3's optional terms and stores them on a PPO / FusedPPO"""
    if not ent_coef >= 0:
        raise ValueError(f"ent_coef must be >= 0, got {ent_coef}")
    if clip_range_vf is not None and not clip_range_vf > 0:
        raise ValueError(f"clip_range_vf must be > 0 (None: no value clipping), got {clip_range_vf}")
    if normalize_advantage not in ("batch", "minibatch"):
        raise ValueError(f"normalize_advantage must be 'batch' or 'minibatch', got {normalize_advantage!r}")
    if target_kl is not None and not target_kl > 0:
        raise ValueError(f"target_kl must be > 0 (None: no early stop), got {target_kl}")
    learner.ent_coef, learner.clip_range_vf, learner.normalize_advantage, learner.target_kl, learner.lr_schedule = ent_coef, clip_range_vf, normalize_advantage, target_kl, lr_schedule


REWARD_NORM_EPSILON = 1e-8                                # VecNormalize's epsilon


def _set_reward_norm(learner, normalize_reward, clip_reward):
    """checks the reward-normalisation options and stores them on a PPO / FusedPPO"""
    if not clip_reward > 0:
        raise ValueError(f"clip_reward must be > 0, got {clip_reward}")
    learner.normalize_reward, learner.clip_reward = bool(normalize_reward), float(clip_reward)
    learner._rn = None                                    # the running state, made at the first update (it is sized by the envs)


def _fresh_reward_norm(n, device):
    """[3 + n] float64: mean 0, var 1, count 1e-4 (a fresh RunningMeanStd), then n zero running returns"""
    st = torch.zeros(3 + n, dtype=torch.float64, device=device)
    st[1] = 1.0; st[2] = 1e-4
    return st


def _reward_norm_state_dict(st):
    st = _fresh_reward_norm(0, "cpu") if st is None else st.detach().cpu()
    return {"mean": st[0].clone(), "var": st[1].clone(), "count": st[2].clone(), "returns": st[3:].clone()}


def _reward_norm_from_state_dict(sd, device):
    """the [3 + N] state of a saved dict; None when it was saved before the first update (no env count yet)"""
    ret = torch.as_tensor(sd["returns"], dtype=torch.float64).reshape(-1)
    head = torch.stack([torch.as_tensor(sd[k], dtype=torch.float64).reshape(()) for k in ("mean", "var", "count")])
    fresh = ret.numel() == 0 and head.tolist() == _fresh_reward_norm(0, "cpu").tolist()
    return None if fresh else torch.cat([head, ret]).to(device)


OBS_NORM_EPSILON = 1e-8                                   # VecNormalize's epsilon
FIRST_LAYERS = ("mlp_extractor.policy_net.0", "mlp_extractor.value_net.0")       # the two towers' first layers: what the fold rewrites


def _fresh_obs_norm(obs_dim, device):
    """[2 obs_dim + 1] float64: mean 0, var 1, count 1e-4 (a fresh RunningMeanStd per observation dimension)"""
    st = torch.zeros(2 * obs_dim + 1, dtype=torch.float64, device=device)
    st[obs_dim:2 * obs_dim] = 1.0; st[2 * obs_dim] = 1e-4
    return st


def _obs_norm_state_dict(st):
    o = (st.numel() - 1) // 2
    st = st.detach().cpu()
    return {"mean": st[:o].clone(), "var": st[o:2 * o].clone(), "count": st[2 * o].clone()}


def _obs_norm_from_state_dict(sd, obs_dim, device):
    mean, var = (torch.as_tensor(sd[k], dtype=torch.float64).reshape(-1) for k in ("mean", "var"))
    if mean.numel() != obs_dim or var.numel() != obs_dim:
        raise ValueError(f"the observation-normalisation state holds {mean.numel()} dimensions, the policy has {obs_dim}")
    return torch.cat([mean, var, torch.as_tensor(sd["count"], dtype=torch.float64).reshape(1)]).to(device)


def obs_norm_scale(obs_norm, epsilon=OBS_NORM_EPSILON):
    """(mean, inv_std) in float64 on the CPU from a saved state ({"mean", "var", "count"}): inv_std = 1/sqrt(var + epsilon)"""
    mean = torch.as_tensor(obs_norm["mean"], dtype=torch.float64).detach().cpu().reshape(-1)
    var = torch.as_tensor(obs_norm["var"], dtype=torch.float64).detach().cpu().reshape(-1)
    return mean, 1.0 / torch.sqrt(var + epsilon)


def fold_obs_norm(state_dict, obs_norm, epsilon=OBS_NORM_EPSILON):
    """The state_dict whose network, fed RAW observations, computes what `state_dict`'s computes on the normalised ones (include/so100_learn.h
    "Observation normalisation"): in both towers' first layers W0' = W0 inv_std, b0' = b0 - W0' mean, formed in float64 and rounded once; the
    other tensors are copied.  obs_norm: a saved state ({"mean", "var", "count"}).  The result lives where state_dict does."""
    mean, inv = obs_norm_scale(obs_norm, epsilon)
    out = {k: v.detach().clone() for k, v in state_dict.items()}
    for layer in FIRST_LAYERS:
        w, b = state_dict[layer + ".weight"].detach(), state_dict[layer + ".bias"].detach()
        wf = w.double().cpu() * inv
        out[layer + ".weight"] = wf.to(w.dtype).to(w.device)
        out[layer + ".bias"] = (b.double().cpu() - (wf * mean).sum(1)).to(b.dtype).to(b.device)
    return out


def _done_code(b):
    """the chunk's done code as a tensor: 0 running, 1 terminated, 2 TimeLimit-truncated only"""
    return b["dones"] * (1.0 + b["truncated"].to(b["dones"].dtype)) if "truncated" in b else b["dones"]


class PPO:
    """ent_coef, clip_range_vf, target_kl as in stable_baselines3.PPO; normalize_advantage "batch" normalises over the whole chunk (this
    driver's default), "minibatch" per minibatch as SB3 does; lr_schedule(progress_remaining) as in SB3, evaluated once per update."""

    def __init__(self, obs_dim, device, lr=3e-4, gamma=0.99, gae_lambda=0.95, clip=0.2, epochs=4, minibatch=32768,
                 vf_coef=0.5, max_grad_norm=0.5, seed=0, use_graph=False, ent_coef=0.0, clip_range_vf=None, normalize_advantage="batch",
                 target_kl=None, lr_schedule=None, normalize_reward=False, clip_reward=10.0, normalize_obs=False):
        _set_terms(self, ent_coef, clip_range_vf, normalize_advantage, target_kl, lr_schedule)
        _set_reward_norm(self, normalize_reward, clip_reward)
        self.normalize_obs, self.obs_dim = bool(normalize_obs), obs_dim
        self._on = _fresh_obs_norm(obs_dim, device)           # mean, var, count: float64 on this learner's device
        torch.manual_seed(seed)
        self.net = ActorCritic(obs_dim).to(device)
        on_gpu = torch.device(device).type == "cuda"
        self.opt = torch.optim.Adam(self.net.parameters(), lr=lr, eps=1e-5)
        self.gamma, self.lam, self.clip, self.epochs, self.mb = gamma, gae_lambda, clip, epochs, minibatch
        self.vf_coef, self.max_grad_norm, self.device = vf_coef, max_grad_norm, device
        # use_graph is accepted and ignored.  Round 1 replayed the update from two captured hipGraphs (+14 % end to end when the
        # rollout ran at 54 M env-steps/s).  With the collector's truncation bootstrap in the loop it produced policy collapses
        # after ~60 updates: replays launched on the legacy default stream were not ordered against the next rollout's raw kernel
        # launch, which read half-updated parameters; fencing fixed the collapses, but from its third update on the replayed
        # learner still differed from the eager one on identical inputs (5e-3 in the weights, cause not found), so it was removed
        # rather than shipped as an option nobody can vouch for.  The eager update is ~60 ms per 262 144 samples.
        del use_graph

    # ---- the two pieces of an update, written over the buffers self._s -------------------------------------------------
    def _gae(self):
        S = self._s; net = self.net
        with torch.no_grad():
            last_v = net.value(S["last_obs"])
            T = S["rewards"].shape[0]
            g = torch.zeros_like(last_v)
            for t in reversed(range(T)):                       # GAE; dones[t] ends the episode after step t
                nv = last_v if t == T - 1 else S["values"][t + 1]
                nonterm = 1.0 - S["dones"][t]
                delta = S["rewards"][t] + self.gamma * nv * nonterm - S["values"][t]
                g = delta + self.gamma * self.lam * nonterm * g
                S["adv"][t] = g
            S["ret"].copy_((S["adv"] + S["values"]).reshape(-1))
            a = S["adv"].reshape(-1)
            S["adv_n"].copy_((a - a.mean()) / (a.std() + 1e-8))
            old_v = S["values"].reshape(-1)
            var_ret = S["ret"].var(unbiased=False)
            S["ev"].copy_(torch.where(var_ret == 0, torch.full_like(var_ret, float("nan")), 1 - (S["ret"] - old_v).var(unbiased=False) / var_ret))

    def _step(self):
        """one minibatch step on the rows S["idx"]; returns False (and leaves parameters and optimiser alone) when target_kl stops the update.
        S["diag"]: policy loss, value loss, approx_kl, entropy_loss, total loss of this minibatch."""
        S = self._s; net = self.net; idx = S["idx"]
        obs = S["obs"].reshape(-1, S["obs"].shape[-1]); act = S["actions"].reshape(-1, S["actions"].shape[-1])
        v, lp = net.evaluate(obs.index_select(0, idx), act.index_select(0, idx))
        if self.normalize_advantage == "batch":
            adv = S["adv_n"].index_select(0, idx)
        else:
            adv = S["adv"].reshape(-1).index_select(0, idx)
            if adv.numel() > 1:
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        log_ratio = lp - S["log_probs"].reshape(-1).index_select(0, idx)
        ratio = log_ratio.exp()
        pg = -torch.min(ratio * adv, ratio.clamp(1 - self.clip, 1 + self.clip) * adv).mean()
        if self.clip_range_vf is not None:
            old_v = S["values"].reshape(-1).index_select(0, idx)
            v = old_v + (v - old_v).clamp(-self.clip_range_vf, self.clip_range_vf)
        vl = (S["ret"].index_select(0, idx) - v).pow(2).mean()
        ent_loss = -(net.log_std.sum() + net.log_std.numel() * ENTROPY_CONST)         # -mean(entropy): the entropy is the same for every sample
        loss = pg + self.vf_coef * vl if self.ent_coef == 0 else pg + self.ent_coef * ent_loss + self.vf_coef * vl
        with torch.no_grad():
            kl = ((ratio - 1) - log_ratio).mean()
            S["diag"].copy_(torch.stack([pg, vl, kl, ent_loss, pg + self.ent_coef * ent_loss + self.vf_coef * vl]))
        S["vl"].copy_(vl.detach())
        if self.target_kl is not None and kl.item() > 1.5 * self.target_kl:
            return False
        loss.backward()
        nn.utils.clip_grad_norm_(net.parameters(), self.max_grad_norm); self.opt.step()
        return True

    # ---- reward normalisation: include/so100_learn.h's arithmetic in torch fp64 on this learner's device ----------------------------------
    def reward_norm_state(self):
        """{"mean", "var", "count": 0-d float64, "returns": float64 [N]} on the CPU (returns is empty before the first update)"""
        return _reward_norm_state_dict(self._rn)

    def load_reward_norm_state(self, sd):
        self._rn = _reward_norm_from_state_dict(sd, self.device)

    # ---- observation normalisation: include/so100_learn.h's arithmetic in torch (fp64 moments and fold, fp32 load) --------------------------------
    def obs_norm_state(self):
        """{"mean", "var": float64 [obs_dim], "count": 0-d float64} on the CPU"""
        return _obs_norm_state_dict(self._on)

    def load_obs_norm_state(self, sd):
        self._on = _obs_norm_from_state_dict(sd, self.obs_dim, self.device)

    def policy_state_dict(self):
        """what a collector, an evaluation or an export loads: with normalize_obs the state_dict folded over the current statistics (it takes
        raw observations), otherwise net.state_dict() itself"""
        return fold_obs_norm(self.net.state_dict(), self.obs_norm_state()) if self.normalize_obs else self.net.state_dict()

    def _obs_scale(self):
        """(mean, inv_std) as float32 on the device: the learner's load is (x - mean) * inv_std in fp32"""
        o = self.obs_dim
        return self._on[:o].float(), (1.0 / torch.sqrt(self._on[o:2 * o] + OBS_NORM_EPSILON)).float()

    @torch.no_grad()
    def _absorb_observations(self, obs):
        """the moment update of one chunk: obs [T, N, obs_dim], the batch is its T*N rows"""
        o = self.obs_dim
        x = obs.reshape(-1, o).to(self.device, torch.float64)
        bc = float(x.shape[0])
        bm, bv = x.mean(0), x.var(0, unbiased=False)
        mean, var, count = self._on[:o], self._on[o:2 * o], self._on[2 * o]
        d, tot = bm - mean, count + bc
        self._on = torch.cat([mean + d * bc / tot, (var * count + bv * bc + d * d * count * bc / tot) / tot, tot.reshape(1)])

    @torch.no_grad()
    def _normalized_rewards(self, rewards, ended):
        """rewards [T, N] float32 and ended [T, N] bool (the done code != 0) -> the normalised rewards, float32; advances self._rn"""
        T, N = rewards.shape
        if self._rn is None:
            self._rn = _fresh_reward_norm(N, self.device)
        if self._rn.numel() != 3 + N:
            raise ValueError(f"the reward-normalisation state holds {self._rn.numel() - 3} envs, the rollout has {N}")
        gamma = torch.tensor(self.gamma, dtype=torch.float32).double().item()        # the learner's gamma is a float in the library: widened from it
        r = rewards.double()
        R = self._rn[3:].clone()
        Rs = torch.empty(T, N, dtype=torch.float64, device=rewards.device)
        for t in range(T):
            R = R * gamma + r[t]
            Rs[t] = R
            R = torch.where(ended[t], torch.zeros_like(R), R)
        bms, bvs = Rs.mean(1).tolist(), Rs.var(1, unbiased=False).tolist()
        mean, var, count = self._rn[:3].tolist()
        denom = []
        for bm, bv in zip(bms, bvs):                         # RunningMeanStd.update_from_moments, one vector step at a time
            d, tot = bm - mean, count + N
            mean, var, count = mean + d * N / tot, (var * count + bv * N + d * d * count * N / tot) / tot, tot
            denom.append(math.sqrt(var + REWARD_NORM_EPSILON))
        self._rn[:3] = torch.tensor([mean, var, count], dtype=torch.float64)
        self._rn[3:] = R
        den = torch.tensor(denom, dtype=torch.float64, device=rewards.device).unsqueeze(1)
        return (r / den).clamp(-self.clip_reward, self.clip_reward).float()

    def _alloc(self, b):
        dev = self.device
        self._s = {k: torch.empty(b[k].shape, dtype=torch.float32, device=dev) for k in ("obs", "actions", "rewards", "dones", "values", "log_probs", "last_obs")}
        T, N = b["rewards"].shape
        self._s.update(adv=torch.zeros(T, N, device=dev), ret=torch.zeros(T * N, device=dev), adv_n=torch.zeros(T * N, device=dev),
                       idx=torch.zeros(min(self.mb, T * N), dtype=torch.long, device=dev), vl=torch.zeros((), device=dev),
                       ev=torch.zeros((), device=dev), diag=torch.zeros(5, device=dev))
        self._shape = tuple(b["obs"].shape)

    def update(self, b, progress_remaining=1.0):
        """b: RolloutCollector.collect() output ([T, N, ...] device tensors + last_obs).  progress_remaining: 1 at the start of training, 0 at
        its end; the argument of lr_schedule.  Returns value_loss, approx_kl, entropy_loss and loss of the last minibatch evaluated (the one
        that stopped the update, if target_kl did), explained_variance of the chunk, std after the update, n_updates (steps applied); with
        normalize_reward also return_var and return_count, the running variance of the discounted returns and its sample count.
        With b["terminal_obs"] (RolloutCollector(defer_bootstrap=True)) the TimeLimit bootstrap is applied here, after the normalisation;
        mean_reward stays the env's raw mean."""
        if self.lr_schedule is not None:
            for g in self.opt.param_groups:
                g["lr"] = float(self.lr_schedule(progress_remaining))
        if getattr(self, "_s", None) is None or self._shape != tuple(b["obs"].shape):
            self._alloc(b)
        S = self._s
        for k in ("obs", "actions", "rewards", "dones", "values", "log_probs", "last_obs"):
            S[k].copy_(b[k])
        tobs = b.get("terminal_obs")
        if self.normalize_obs:                                # under the statistics the chunk was collected with; the chunk itself keeps the raw observations
            m, inv = self._obs_scale()
            S["obs"].copy_((S["obs"] - m) * inv); S["last_obs"].copy_((S["last_obs"] - m) * inv)
            if tobs is not None:
                tobs = (tobs.to(self.device, torch.float32) - m) * inv
        if self.normalize_reward:
            S["rewards"].copy_(self._normalized_rewards(S["rewards"], S["dones"] != 0))
        if tobs is not None:                                  # a deferred TimeLimit bootstrap (RolloutCollector(defer_bootstrap=True)): after the normalisation
            from .rollout import bootstrap_truncated
            with torch.no_grad():
                bootstrap_truncated(S["rewards"], _done_code(b), tobs, self.net.value, self.gamma)
        n = S["ret"].numel(); mb = S["idx"].numel()
        self._gae()
        applied, stopped = 0, False
        for _ in range(self.epochs):
            perm = torch.randperm(n, device=self.device)
            for i in range(0, n, mb):
                S["idx"] = perm[i:i + mb]
                self.opt.zero_grad(set_to_none=True)
                if not self._step():
                    stopped = True
                    break
                applied += 1
            if stopped:
                break
        S["idx"] = torch.zeros(mb, dtype=torch.long, device=self.device)
        if self.normalize_obs:                                # after the update: the next chunk is collected, and trained on, under the new statistics
            self._absorb_observations(b["obs"])
        # mean_reward = the ENV's mean reward per step (the collector takes it before its TimeLimit bootstrap adds gamma * V to the
        # truncated steps); S["rewards"] holds the bootstrapped rewards the advantages are computed from
        raw = b.get("raw_reward_mean")
        if raw is None and (self.normalize_reward or "terminal_obs" in b):       # S["rewards"] no longer holds the env's rewards: the chunk does
            raw = b["rewards"].mean()
        d = S["diag"].tolist()
        rn = {"return_var": self._rn[1].item(), "return_count": self._rn[2].item()} if self.normalize_reward else {}
        return {**rn, "value_loss": S["vl"].item(), "mean_reward": (raw if raw is not None else S["rewards"].mean()).item(),
                "mean_bootstrapped_reward": S["rewards"].mean().item(), "approx_kl": d[2], "entropy_loss": d[3], "loss": d[4],
                "explained_variance": S["ev"].item(), "std": self.net.log_std.detach().exp().mean().item(), "n_updates": applied, "early_stop": stopped}


class FusedPPO:
    """PPO with the advantages and the whole minibatch step (forward, backward, gradient-norm clip, Adam) in the library's HIP kernels
    (include/so100_learn.h; DESIGN.md "On-device learner"): 3 launches per update + 3 per minibatch instead of ~100 per minibatch.
    Constructor arguments and update(b) are PPO's.  `.net` is an ActorCritic whose 13 parameters are VIEWS of one flat float32 block
    (`.params`, the layout of so100_learner_param_offset), so state_dict(), checkpoints, RolloutCollector.load_policy and export.py see an
    ordinary policy while the kernels update the block in place.  All launches go to torch's current stream, as So100Sim's do."""

    def __init__(self, obs_dim, device, lr=3e-4, gamma=0.99, gae_lambda=0.95, clip=0.2, epochs=4, minibatch=32768,
                 vf_coef=0.5, max_grad_norm=0.5, seed=0, use_graph=False, ent_coef=0.0, clip_range_vf=None, normalize_advantage="batch",
                 target_kl=None, lr_schedule=None, shuffle="torch", normalize_reward=False, clip_reward=10.0, normalize_obs=False):
        from . import lib
        del use_graph
        _set_terms(self, ent_coef, clip_range_vf, normalize_advantage, target_kl, lr_schedule)
        _set_reward_norm(self, normalize_reward, clip_reward)
        self.normalize_obs = bool(normalize_obs)
        if shuffle not in ("torch", "device"):
            raise ValueError(f"shuffle must be 'torch' or 'device', got {shuffle!r}")
        # "device": the whole update is one so100_learner_update call and the minibatches are a function of (seed, shuffle_epoch) alone --
        # torch's generator has no part in them.  shuffle_epoch counts the epochs shuffled so far; a resumed run sets it.
        self.shuffle, self.shuffle_seed, self.shuffle_epoch = shuffle, seed, 0
        # any option on: the extended step (so100_learner_minibatch_step_ex); none: the step as it always was
        self._extended = ent_coef != 0 or clip_range_vf is not None or normalize_advantage != "batch" or target_kl is not None or lr_schedule is not None
        self.vf_coef = vf_coef
        torch.manual_seed(seed)
        self.net = ActorCritic(obs_dim)                          # the draws of PPO's initialisation for the same seed
        layout, P = lib.learner_layout(obs_dim)
        self.device = torch.device(device)
        self.params = torch.zeros(P, dtype=torch.float32, device=self.device)
        named = dict(self.net.named_parameters())
        for k, (off, shape) in layout.items():
            p = named[lib.SB3_STATE_DICT_KEYS[k]]
            view = self.params[off:off + p.numel()].view(shape)
            view.copy_(p.data)
            p.data = view                                        # from here on the module's parameter IS this slice of the block
        self.net.requires_grad_(False)                           # nothing here goes through autograd
        self.adam_m = torch.zeros_like(self.params); self.adam_v = torch.zeros_like(self.params)
        self.adam_step = 0
        self.obs_dim, self.epochs, self.mb = obs_dim, epochs, minibatch
        self._hyper = dict(gamma=gamma, gae_lambda=gae_lambda, clip_range=clip, vf_coef=vf_coef, max_grad_norm=max_grad_norm, lr=lr, adam_eps=1e-5)
        self._learner = None
        self._shape = None
        self._rn_shape = None
        self._side = None
        if self.normalize_obs:
            # the running moments (float64 [2 obs_dim + 1]), the folded copy of the block the collector and the exports read, and the
            # (mean, inv_std) pair the learner's kernels read: the fold writes the last two, after every update and whenever the state is loaded
            self._on = _fresh_obs_norm(obs_dim, self.device)
            self._folded = torch.zeros_like(self.params); self._norm = torch.zeros(2 * obs_dim, dtype=torch.float32, device=self.device)
            self._on_shape = None

    def _handle(self):
        if self._learner is None:
            from . import lib
            if self.device.type != "cuda":
                raise lib.So100Error(f"FusedPPO runs on a HIP device, not on {self.device}: there is no CPU fallback (use PPO)")
            self._learner = lib.So100Learner(self.obs_dim, self.device, max_minibatch=self.mb, **self._hyper)
            if self.normalize_obs:
                self._learner.obs_norm_fold(self._on, self.params, self._folded, self._norm)
                self._learner.set_obs_norm(self._norm)
        return self._learner

    def obs_norm_state(self):
        """PPO.obs_norm_state: the device state as a dict of CPU tensors"""
        return _obs_norm_state_dict(self._on if self.normalize_obs else _fresh_obs_norm(self.obs_dim, "cpu"))

    def load_obs_norm_state(self, sd):
        if not self.normalize_obs:
            raise ValueError("this learner was built without normalize_obs")
        self._on.copy_(_obs_norm_from_state_dict(sd, self.obs_dim, self.device))
        if self._learner is not None:
            self._learner.obs_norm_fold(self._on, self.params, self._folded, self._norm)

    def policy_state_dict(self):
        """PPO.policy_state_dict.  With normalize_obs: views of the folded block, folded here from the current parameters and statistics (one
        launch on the current stream); a collector copies them in load_policy.  update() has folded already, so after an update this launch
        repeats that one; it is kept because the parameters are plain tensors that anything may have written since (net.load_state_dict, a
        checkpoint copied into .params), which nothing here can observe: a few microseconds buy a folded block that is never stale."""
        if not self.normalize_obs:
            return self.net.state_dict()
        from . import lib
        self._handle().obs_norm_fold(self._on, self.params, self._folded, self._norm)
        layout, _ = lib.learner_layout(self.obs_dim)
        by_key = {lib.SB3_STATE_DICT_KEYS[k]: self._folded[off:off + math.prod(shape)].view(shape) for k, (off, shape) in layout.items()}
        return {k: by_key[k] for k in self.net.state_dict()}

    def _absorb_observations(self, L, buf):
        """after an update: the chunk's observations join the running moments and the fold is renewed, so that the next chunk is collected (once
        policy_state_dict() has been loaded) and trained on under the new statistics.  Three launches, no host round trip."""
        T, N = buf.shape[0], buf.shape[1]
        if self._on_shape != (T, N):
            self._on_ws = torch.zeros(L.obs_norm_workspace_bytes(T, N) // 8, dtype=torch.float64, device=self.device)
            self._on_shape = (T, N)
        L.obs_norm_update(buf, self._on, self._on_ws)
        L.obs_norm_fold(self._on, self.params, self._folded, self._norm)

    def reward_norm_state(self):
        """PPO.reward_norm_state: the device state [mean, var, count, returns] as a dict of CPU tensors"""
        return _reward_norm_state_dict(self._rn)

    def load_reward_norm_state(self, sd):
        self._rn = _reward_norm_from_state_dict(sd, self.device)

    def _reward_norm(self, L, T, N):
        """the arguments of the normalisation kernels for a [T, N] chunk: the running state (made at the first update), the dense rewards they
        write and their workspace"""
        if self._rn is None:
            self._rn = torch.empty(3 + N, dtype=torch.float64, device=self.device)
            L.reward_norm_init(self._rn)
        if self._rn.numel() != 3 + N:
            raise ValueError(f"the reward-normalisation state holds {self._rn.numel() - 3} envs, the rollout has {N}")
        if self._rn_shape != (T, N):
            self._rn_rewards = torch.zeros(T, N, device=self.device)
            self._rn_ws = torch.zeros(L.reward_norm_workspace_bytes(T, N) // 8, dtype=torch.float64, device=self.device)
            self._rn_shape = (T, N)
        return dict(state=self._rn, rewards=self._rn_rewards, workspace=self._rn_ws, clip_reward=self.clip_reward, epsilon=REWARD_NORM_EPSILON)

    def _packed(self, b):
        """the [T, N, obs_dim+10] chunk: b["packed"] as RolloutCollector.collect() hands it over (read in place, no copy); a dict without it
        (separate tensors, e.g. from another collector) is packed here, once per update"""
        obs = b["obs"]; T, N, o = obs.shape
        if o != self.obs_dim:
            raise ValueError(f"this learner was built for obs_dim {self.obs_dim}, the rollout has {o}")
        buf = b.get("packed")
        if buf is not None:
            if tuple(buf.shape) != (T, N, o + 10) or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device != obs.device:
                raise ValueError(f"packed chunk: want contiguous float32 {(T, N, o + 10)}, got {buf.dtype} {tuple(buf.shape)}")
            return buf
        code = b["dones"] * (1.0 + b["truncated"].to(b["dones"].dtype)) if "truncated" in b else b["dones"]
        return torch.cat([obs, b["actions"], b["rewards"].unsqueeze(-1), code.unsqueeze(-1), b["values"].unsqueeze(-1), b["log_probs"].unsqueeze(-1)],
                         dim=-1).to(self.device, torch.float32).contiguous()

    def update(self, b, perms=None, *, progress_remaining=1.0):
        """b: RolloutCollector.collect() output.  With b["terminal_obs"] (RolloutCollector(defer_bootstrap=True)) the TimeLimit bootstrap is
        applied by the advantage kernel; otherwise the rewards are taken as they are (the collector's eager bootstrap has been added).
        perms: one int64 permutation of range(T*N) per epoch (tests); default torch.randperm, drawn as PPO.update draws them.
        With normalize_reward the chunk's rewards are normalised by the library's kernels first (the chunk itself stays as it is) and the
        advantages read the normalised rewards; the bootstrap is added to those.
        Returns PPO.update's keys plus policy_loss, clip_fraction and grad_norm of the last minibatch.  mean_bootstrapped_reward is the
        mean of the chunk's reward column: with a deferred bootstrap that column keeps the env's own rewards (the bootstrapped ones are
        never materialised), so it then equals the raw mean.
        Also PPO.update's diagnostics.  With an option on they come from the extended step: the last minibatch's, or the stopping one's if
        target_kl stopped the update; the applied steps are counted on the device and read here, once, with the statistics -- nothing
        synchronises in the middle of an update.  At the defaults the old step runs and approx_kl, which only the extended step forms, is NaN.
        progress_remaining (keyword only, after perms: PPO.update(b, progress_remaining) has no perms) is the argument of lr_schedule.
        The explained-variance launches go to a side stream, beside the minibatch steps, and are joined before the one read of the results.
        With shuffle="device" (constructor) the same update is one so100_learner_update call: the permutations are the library's, a function of
        (seed, shuffle_epoch), everything runs on the current stream, and the returned keys mean what they mean above."""
        if self.shuffle == "device" and perms is not None:
            raise ValueError("perms= injects torch-side permutations: with shuffle='device' the library draws them from (seed, shuffle_epoch)")
        L = self._handle()
        buf = self._packed(b)
        T, N = buf.shape[0], buf.shape[1]
        if self._shape != (T, N):
            dev = self.device
            self._adv = torch.zeros(T, N, device=dev); self._ret = torch.zeros(T, N, device=dev)
            self._adv_stats = torch.zeros(2, device=dev)
            # everything an update leaves for the host, in one buffer read in one transfer: [0:8] the step's statistics (the old step writes four,
            # the extended one eight), [8] explained variance, [9:15] log_std before the last step (old step only), [15:21] log_std after the update,
            # [21] mean of the reward column, [22] the env's own mean reward, [23:25] the update state (extended step only)
            self._out = torch.zeros(25, device=dev)
            self._stats, self._diag, self._ev = self._out[0:4], self._out[0:8], self._out[8:9]
            self._state = torch.zeros(2, dtype=torch.int32, device=dev)
            self._perm = torch.zeros(T * N, dtype=torch.int64, device=dev) if self.shuffle == "device" else None
            self._shape = (T, N)
        tobs = b.get("terminal_obs")
        rn = self._reward_norm(L, T, N) if self.normalize_reward else None
        if self.shuffle == "device":
            return self._update_on_device(L, b, buf, tobs, progress_remaining, rn)
        if rn is not None:
            L.normalize_rewards(buf, rn["state"], rn["rewards"], rn["workspace"], clip_reward=rn["clip_reward"], epsilon=rn["epsilon"])
        L.advantages(buf, b["last_obs"].contiguous(), self.params, self._adv, self._ret, self._adv_stats, terminal_obs=tobs,
                     rewards=None if rn is None else rn["rewards"])
        cur = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(cur)                                      # behind the advantages ...
        with torch.cuda.stream(self._side):
            L.explained_variance(buf, self._ret, self._ev)               # ... and beside the minibatch steps, which read the same buffers
        n = T * N; mb = min(self.mb, n)
        first_step = self.adam_step
        last = first_step + self.epochs * ((n + mb - 1) // mb)
        if self._extended:
            lr = None if self.lr_schedule is None else float(self.lr_schedule(progress_remaining))
            self._state.zero_()
        step = first_step
        for e in range(self.epochs):
            perm = torch.randperm(n, device=self.device) if perms is None else perms[e]
            for i in range(0, n, mb):
                step += 1               # the number this step carries if it is applied: after a stop none is, so the applied ones are contiguous
                if self._extended:
                    L.minibatch_step_ex(buf, perm[i:i + mb], self._adv, self._ret, self._adv_stats, self.params, self.adam_m, self.adam_v, step, self._diag,
                                        ent_coef=self.ent_coef, clip_range_vf=self.clip_range_vf, normalize_advantage=self.normalize_advantage,
                                        target_kl=self.target_kl, lr=lr, update_state=self._state)
                else:
                    if step == last:
                        self._out[9:15].copy_(self.net.log_std.detach())    # the entropy of the policy the last minibatch was evaluated with
                    L.minibatch_step(buf, perm[i:i + mb], self._adv, self._ret, self._adv_stats, self.params, self.adam_m, self.adam_v, step, self._stats)
        if self._extended:
            self._out[23:25].copy_(self._state)
        if self.normalize_obs:
            self._absorb_observations(L, buf)
        st = self._read_out(b, buf, cur)                                 # the update's only synchronisation
        return self._results(st, first_step, last)

    def _update_on_device(self, L, b, buf, tobs, progress_remaining, rn):
        """shuffle="device": everything update() enqueues above, the permutations included, by one so100_learner_update call on the current stream"""
        n = buf.shape[0] * buf.shape[1]; mb = min(self.mb, n)
        first_step = self.adam_step
        last = first_step + self.epochs * ((n + mb - 1) // mb)
        terms = None
        if self._extended:
            terms = dict(ent_coef=self.ent_coef, clip_range_vf=self.clip_range_vf, normalize_advantage=self.normalize_advantage, target_kl=self.target_kl,
                         lr=None if self.lr_schedule is None else float(self.lr_schedule(progress_remaining)))
        L.update(buf, b["last_obs"].contiguous(), self.params, self.adam_m, self.adam_v, self._adv, self._ret, self._adv_stats, self._perm, self._out[0:15],
                 epochs=self.epochs, mb=mb, adam_step0=first_step, shuffle_seed=self.shuffle_seed, shuffle_epoch0=self.shuffle_epoch, terminal_obs=tobs,
                 terms=terms, update_state=self._state if self._extended else None, reward_norm=rn)
        self.shuffle_epoch += self.epochs
        if self._extended:
            self._out[23:25].copy_(self._state)
        if self.normalize_obs:
            self._absorb_observations(L, buf)
        return self._results(self._read_out(b, buf, None), first_step, last)

    def _results(self, st, first_step, last):
        """update()'s dict from the values of self._out on the host; advances adam_step by the steps applied"""
        if self._extended:
            stopped, applied = int(st[23]), int(st[24])
            assert applied == last - first_step or stopped
            extra = {"approx_kl": st[4], "entropy_loss": st[5], "loss": st[6], "value_clip_fraction": st[7], "n_updates": applied, "early_stop": bool(stopped)}
        else:
            applied = last - first_step
            ent_loss = -(math.fsum(st[9:15]) + 6 * ENTROPY_CONST)
            extra = {"approx_kl": float("nan"), "entropy_loss": ent_loss, "loss": st[0] + self.vf_coef * st[1], "n_updates": applied, "early_stop": False}
        self.adam_step = first_step + applied
        if self.normalize_reward:                                 # the running moments in full precision: a second small read, after the one that synchronised
            _, var, count = self._rn[:3].tolist()
            extra = {**extra, "return_var": var, "return_count": count}
        # mean_bootstrapped_reward: the mean of the chunk's reward column -- with a deferred bootstrap that column holds the env's own rewards
        return {"value_loss": st[1], "mean_reward": st[22], "mean_bootstrapped_reward": st[21],
                "policy_loss": st[0], "clip_fraction": st[2], "grad_norm": st[3], "explained_variance": st[8], "std": math.fsum(math.exp(x) for x in st[15:21]) / 6, **extra}

    def _read_out(self, b, buf, cur):
        """log_std after the update and the two reward means join the statistics in self._out (one small launch), the side stream is joined,
        (cur: the stream it ran beside; None when nothing went there) and the whole buffer comes to the host in one transfer"""
        rew = buf[..., self.obs_dim + 6].mean().view(1)
        raw = b.get("raw_reward_mean")
        torch.cat([self.net.log_std.detach(), rew, rew if raw is None else raw.detach().to(torch.float32).view(1)], out=self._out[15:23])
        if cur is not None:
            cur.wait_stream(self._side)
        return self._out.tolist()
