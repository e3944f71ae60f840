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
all off by default (then the loss is the one above, to the bit), and return SB3's per-update diagnostics."""
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


class PPO:
    """ent_coef, clip_range_vf, target_kl as in stable_baselines3.PPO; normalize_advantage "batch" normalises over the whole chunk (this
    driver's default), "minibatch" per minibatch as SB3 does; lr_schedule(progress_remaining) as in SB3, evaluated once per update."""

    def __init__(self, obs_dim, device, lr=3e-4, gamma=0.99, gae_lambda=0.95, clip=0.2, epochs=4, minibatch=32768,
                 vf_coef=0.5, max_grad_norm=0.5, seed=0, use_graph=False, ent_coef=0.0, clip_range_vf=None, normalize_advantage="batch",
                 target_kl=None, lr_schedule=None):
        _set_terms(self, ent_coef, clip_range_vf, normalize_advantage, target_kl, lr_schedule)
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
        that stopped the update, if target_kl did), explained_variance of the chunk, std after the update, n_updates (steps applied)."""
        if self.lr_schedule is not None:
            for g in self.opt.param_groups:
                g["lr"] = float(self.lr_schedule(progress_remaining))
        if getattr(self, "_s", None) is None or self._shape != tuple(b["obs"].shape):
            self._alloc(b)
        S = self._s
        for k in ("obs", "actions", "rewards", "dones", "values", "log_probs", "last_obs"):
            S[k].copy_(b[k])
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
        # mean_reward = the ENV's mean reward per step (the collector takes it before its TimeLimit bootstrap adds gamma * V to the
        # truncated steps); S["rewards"] holds the bootstrapped rewards the advantages are computed from
        raw = b.get("raw_reward_mean")
        d = S["diag"].tolist()
        return {"value_loss": S["vl"].item(), "mean_reward": (raw if raw is not None else S["rewards"].mean()).item(),
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
                 target_kl=None, lr_schedule=None, shuffle="torch"):
        from . import lib
        del use_graph
        _set_terms(self, ent_coef, clip_range_vf, normalize_advantage, target_kl, lr_schedule)
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
        self._side = None

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

    def update(self, b, perms=None, *, progress_remaining=1.0):
        """b: RolloutCollector.collect() output.  With b["terminal_obs"] (RolloutCollector(defer_bootstrap=True)) the TimeLimit bootstrap is
        applied by the advantage kernel; otherwise the rewards are taken as they are (the collector's eager bootstrap has been added).
        perms: one int64 permutation of range(T*N) per epoch (tests); default torch.randperm, drawn as PPO.update draws them.
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
        if self.shuffle == "device":
            return self._update_on_device(L, b, buf, tobs, progress_remaining)
        L.advantages(buf, b["last_obs"].contiguous(), self.params, self._adv, self._ret, self._adv_stats, terminal_obs=tobs)
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
        st = self._read_out(b, buf, cur)                                 # the update's only synchronisation
        return self._results(st, first_step, last)

    def _update_on_device(self, L, b, buf, tobs, progress_remaining):
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
                 terms=terms, update_state=self._state if self._extended else None)
        self.shuffle_epoch += self.epochs
        if self._extended:
            self._out[23:25].copy_(self._state)
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
