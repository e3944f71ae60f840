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
FusedPPO is the same learner on the library's own kernels (include/so100_learn.h): same constructor, same update(b), same state_dict."""
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


class PPO:
    def __init__(self, obs_dim, device, lr=3e-4, gamma=0.99, gae_lambda=0.95, clip=0.2, epochs=4, minibatch=32768,
                 vf_coef=0.5, max_grad_norm=0.5, seed=0, use_graph=False):
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

    def _step(self):
        S = self._s; net = self.net; idx = S["idx"]
        obs = S["obs"].reshape(-1, S["obs"].shape[-1]); act = S["actions"].reshape(-1, S["actions"].shape[-1])
        v, lp = net.evaluate(obs.index_select(0, idx), act.index_select(0, idx))
        adv = S["adv_n"].index_select(0, idx)
        ratio = (lp - S["log_probs"].reshape(-1).index_select(0, idx)).exp()
        pg = -torch.min(ratio * adv, ratio.clamp(1 - self.clip, 1 + self.clip) * adv).mean()
        vl = (S["ret"].index_select(0, idx) - v).pow(2).mean()
        loss = pg + self.vf_coef * vl
        loss.backward()
        nn.utils.clip_grad_norm_(net.parameters(), self.max_grad_norm); self.opt.step()
        S["vl"].copy_(vl.detach())

    def _alloc(self, b):
        dev = self.device
        self._s = {k: torch.empty(b[k].shape, dtype=torch.float32, device=dev) for k in ("obs", "actions", "rewards", "dones", "values", "log_probs", "last_obs")}
        T, N = b["rewards"].shape
        self._s.update(adv=torch.zeros(T, N, device=dev), ret=torch.zeros(T * N, device=dev), adv_n=torch.zeros(T * N, device=dev),
                       idx=torch.zeros(min(self.mb, T * N), dtype=torch.long, device=dev), vl=torch.zeros((), device=dev))
        self._shape = tuple(b["obs"].shape)

    def update(self, b):
        """b: RolloutCollector.collect() output ([T, N, ...] device tensors + last_obs)."""
        if getattr(self, "_s", None) is None or self._shape != tuple(b["obs"].shape):
            self._alloc(b)
        S = self._s
        for k in ("obs", "actions", "rewards", "dones", "values", "log_probs", "last_obs"):
            S[k].copy_(b[k])
        n = S["ret"].numel(); mb = S["idx"].numel()
        self._gae()
        for _ in range(self.epochs):
            perm = torch.randperm(n, device=self.device)
            for i in range(0, n, mb):
                S["idx"] = perm[i:i + mb]
                self.opt.zero_grad(set_to_none=True); self._step()
        S["idx"] = torch.zeros(mb, dtype=torch.long, device=self.device)
        # mean_reward = the ENV's mean reward per step (the collector takes it before its TimeLimit bootstrap adds gamma * V to the
        # truncated steps); S["rewards"] holds the bootstrapped rewards the advantages are computed from
        raw = b.get("raw_reward_mean")
        return {"value_loss": S["vl"].item(), "mean_reward": (raw if raw is not None else S["rewards"].mean()).item(),
                "mean_bootstrapped_reward": S["rewards"].mean().item()}


class FusedPPO:
    """PPO with the advantages and the whole minibatch step (forward, backward, gradient-norm clip, Adam) in the library's HIP kernels
    (include/so100_learn.h; DESIGN.md "On-device learner"): 3 launches per update + 3 per minibatch instead of ~100 per minibatch.
    Constructor arguments and update(b) are PPO's.  `.net` is an ActorCritic whose 13 parameters are VIEWS of one flat float32 block
    (`.params`, the layout of so100_learner_param_offset), so state_dict(), checkpoints, RolloutCollector.load_policy and export.py see an
    ordinary policy while the kernels update the block in place.  All launches go to torch's current stream, as So100Sim's do."""

    def __init__(self, obs_dim, device, lr=3e-4, gamma=0.99, gae_lambda=0.95, clip=0.2, epochs=4, minibatch=32768,
                 vf_coef=0.5, max_grad_norm=0.5, seed=0, use_graph=False):
        from . import lib
        del use_graph
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

    def _handle(self):
        if self._learner is None:
            from . import lib
            if self.device.type != "cuda":
                raise lib.So100Error(f"FusedPPO runs on a HIP device, not on {self.device}: there is no CPU fallback (use PPO)")
            self._learner = lib.So100Learner(self.obs_dim, self.device, max_minibatch=self.mb, **self._hyper)
        return self._learner

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

    def update(self, b, perms=None):
        """b: RolloutCollector.collect() output.  With b["terminal_obs"] (RolloutCollector(defer_bootstrap=True)) the TimeLimit bootstrap is
        applied by the advantage kernel; otherwise the rewards are taken as they are (the collector's eager bootstrap has been added).
        perms: one int64 permutation of range(T*N) per epoch (tests); default torch.randperm, drawn as PPO.update draws them.
        Returns PPO.update's keys plus policy_loss, clip_fraction and grad_norm of the last minibatch.  mean_bootstrapped_reward is the
        mean of the chunk's reward column: with a deferred bootstrap that column keeps the env's own rewards (the bootstrapped ones are
        never materialised), so it then equals the raw mean."""
        L = self._handle()
        buf = self._packed(b)
        T, N = buf.shape[0], buf.shape[1]
        if self._shape != (T, N):
            dev = self.device
            self._adv = torch.zeros(T, N, device=dev); self._ret = torch.zeros(T, N, device=dev)
            self._adv_stats = torch.zeros(2, device=dev); self._stats = torch.zeros(4, device=dev)
            self._shape = (T, N)
        tobs = b.get("terminal_obs")
        L.advantages(buf, b["last_obs"].contiguous(), self.params, self._adv, self._ret, self._adv_stats, terminal_obs=tobs)
        n = T * N; mb = min(self.mb, n)
        for e in range(self.epochs):
            perm = torch.randperm(n, device=self.device) if perms is None else perms[e]
            for i in range(0, n, mb):
                self.adam_step += 1
                L.minibatch_step(buf, perm[i:i + mb], self._adv, self._ret, self._adv_stats, self.params, self.adam_m, self.adam_v, self.adam_step, self._stats)
        o = self.obs_dim
        rew = buf[..., o + 6].mean()
        raw = b.get("raw_reward_mean")
        st = self._stats.tolist()
        # mean_bootstrapped_reward: the mean of the chunk's reward column -- with a deferred bootstrap that column holds the env's own rewards
        return {"value_loss": st[1], "mean_reward": (raw if raw is not None else rew).item(), "mean_bootstrapped_reward": rew.item(),
                "policy_loss": st[0], "clip_fraction": st[2], "grad_norm": st[3]}
