"""What the learner tests share (test_learn_cpu.py, test_learn_terms_cpu.py, test_gpu_learner.py, test_gpu_learner_terms.py): the fp64 autograd
reference of include/so100_learn.h -- SB3's MlpPolicy network and PPO.train loss written from their formulas, clip_grad_norm_, torch.optim.Adam,
the target_kl stop and the GAE recursion with the TimeLimit bootstrap applied -- and the inputs the tests are run on.  The reference is never
the code under test: it shares no line with csrc/so100_learn.* or ppo.py.  (The host twin of so100_learn.hpp is hostlibs.learncheck().)"""
import functools
import math

import numpy as np
import torch
import torch.nn as nn

from hostlibs import ptr  # noqa: F401  (re-exported for the tests)

HYPER = dict(gamma=0.99, gae_lambda=0.95, clip=0.2, vf_coef=0.5, max_grad_norm=0.5, lr=3e-4, beta1=0.9, beta2=0.999, adam_eps=1e-5)      # ppo.py's
GAUSS_ENTROPY = 0.5 + 0.5 * math.log(2 * math.pi)               # per action dimension, at log_std 0
ALL_TERMS = dict(ent_coef=0.01, clip_range_vf=0.3, normalize_advantage="minibatch")


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------------------
class RefNet(nn.Module):
    """SB3's MlpPolicy network, 2 x 64 tanh towers, state-independent log_std; float64; state_dict keys are SB3's"""

    def __init__(self, obs_dim, state_dict):
        super().__init__()
        tower = lambda: nn.Sequential(nn.Linear(obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh())
        self.mlp_extractor = nn.ModuleDict({"policy_net": tower(), "value_net": tower()})
        self.action_net = nn.Linear(64, 6); self.value_net = nn.Linear(64, 1)
        self.log_std = nn.Parameter(torch.zeros(6))
        self.double()
        self.load_state_dict({k: v.detach().cpu().double() for k, v in state_dict.items()})

    def value(self, obs):
        return self.value_net(self.mlp_extractor["value_net"](obs)).squeeze(-1)

    def mean_action(self, obs):
        return self.action_net(self.mlp_extractor["policy_net"](obs))

    def log_prob(self, obs, act):
        z = (act - self.mean_action(obs)) / self.log_std.exp()
        return (-0.5 * z * z - self.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)


def ref_advantages(buf, last_obs, net, terminal_obs=None, gamma=HYPER["gamma"], lam=HYPER["gae_lambda"]):
    """GAE over the packed chunk [T, N, od+10] (any float dtype), rewards += gamma V(terminal_obs) on the code-2 steps first (the TimeLimit
    bootstrap); returns adv [T, N], ret [T, N], mean, unbiased std as float64 tensors"""
    buf = buf.detach().cpu().double(); T, N, k = buf.shape; o = k - 10
    rew, code, val = buf[..., o + 6].clone(), buf[..., o + 7], buf[..., o + 8]
    with torch.no_grad():
        last_v = net.value(last_obs.detach().cpu().double())
        if terminal_obs is not None:
            for t, n in (code == 2).nonzero().tolist():
                rew[t, n] += gamma * net.value(terminal_obs[t, n].detach().cpu().double().unsqueeze(0))[0]
    adv = torch.zeros(T, N, dtype=torch.float64)
    run = torch.zeros(N, dtype=torch.float64)
    for t in reversed(range(T)):
        nxt = last_v if t == T - 1 else val[t + 1]
        live = (code[t] == 0).double()
        run = rew[t] + gamma * nxt * live - val[t] + gamma * lam * live * run
        adv[t] = run
    flat = adv.reshape(-1)
    return adv, adv + val, flat.mean(), (flat.std() if flat.numel() > 1 else torch.tensor(float("nan"), dtype=torch.float64))


def ref_loss(net, buf, idx, adv, ret, mean, std, clip=HYPER["clip"], vf_coef=HYPER["vf_coef"], ent_coef=0.0, clip_range_vf=None,
             normalize_advantage="batch"):
    """SB3's PPO.train loss on rows idx of the packed chunk, float64.  Indices outside the chunk are left out of every sum and of the
    minibatch statistics; every mean divides by len(idx) (include/so100_learn.h).  Returns the loss and the diagnostics with the exact
    counts and the number of samples within 1e-5 of a clip boundary."""
    buf = buf.detach().cpu().double(); k = buf.shape[-1]; o = k - 10
    table = buf.reshape(-1, k); n = table.shape[0]; mb = len(idx)
    idx = torch.as_tensor(idx)
    keep = idx[(idx >= 0) & (idx < n)]
    rows = table[keep]
    a = adv.reshape(-1).double()[keep]
    if normalize_advantage == "batch":
        a = (a - mean) / (std + 1e-8)
    elif len(keep) > 1:
        a = (a - a.mean()) / (a.std() + 1e-8)
    log_ratio = net.log_prob(rows[:, :o], rows[:, o:o + 6]) - rows[:, o + 9]
    ratio = log_ratio.exp()
    policy_loss = -torch.minimum(ratio * a, ratio.clamp(1 - clip, 1 + clip) * a).sum() / mb
    v, old_v, target = net.value(rows[:, :o]), rows[:, o + 8], ret.reshape(-1).double()[keep]
    v_pred = v if clip_range_vf is None else old_v + (v - old_v).clamp(-clip_range_vf, clip_range_vf)
    value_loss = (target - v_pred).pow(2).sum() / mb
    entropy = net.log_std.sum() + 6 * GAUSS_ENTROPY
    entropy_loss = -entropy * len(keep) / mb
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    r, dv = ratio.detach(), (v - old_v).detach()
    outside = (r - 1).abs() > clip
    active = ((a > 0) & (r > 1 + clip)) | ((a < 0) & (r < 1 - clip))                  # the clip removes this sample's policy gradient
    # clipped_count: samples with |ratio - 1| > clip; borderline: those whose ratio lies within 1e-5 of 1 +- clip, the only ones an fp32
    # ratio (relative error ~1e-6 after the exp of a sum of ~20 terms) can put on the other side
    st = {"policy_loss": policy_loss.item(), "value_loss": value_loss.item(), "entropy_loss": entropy_loss.item(), "loss": loss.item(),
          "approx_kl": (((r - 1) - log_ratio.detach()).sum() / mb).item(),
          "clip_fraction": int(outside.sum()) / mb, "clipped_count": int(outside.sum()), "borderline": int((((r - 1).abs() - clip).abs() < 1e-5).sum()),
          "active_share": int(active.sum()) / mb, "high": int((active & (r > 1)).sum()), "low": int((active & (r < 1)).sum()),
          "v_clipped_count": 0, "v_borderline": 0, "valid": len(keep)}
    if clip_range_vf is not None:
        st["v_clipped_count"] = int((dv.abs() > clip_range_vf).sum()); st["v_borderline"] = int(((dv.abs() - clip_range_vf).abs() < 1e-5).sum())
    return loss, st


class RefLearner:
    """the update of SB3's PPO.train in float64 on given permutations: loss, clip_grad_norm_, Adam, the target_kl stop"""

    def __init__(self, obs_dim, state_dict, max_grad_norm=HYPER["max_grad_norm"], lr=HYPER["lr"], target_kl=None, **terms):
        self.net = RefNet(obs_dim, state_dict)
        self.opt = torch.optim.Adam(self.net.parameters(), lr=lr, eps=HYPER["adam_eps"])
        self.max_grad_norm, self.target_kl, self.terms = max_grad_norm, target_kl, terms
        self.stopped, self.applied = False, 0

    def step(self, buf, idx, adv, ret, mean, std):
        """one minibatch step; returns (diagnostics incl. the pre-clip grad_norm, {state_dict key: clipped gradient}); after a stop (and on
        the stopping step) nothing is applied and the gradients are None"""
        if self.stopped:
            return None, None
        self.opt.zero_grad(set_to_none=True)
        loss, st = ref_loss(self.net, buf, idx, adv, ret, mean, std, **self.terms)
        if self.target_kl is not None and st["approx_kl"] > 1.5 * self.target_kl:
            self.stopped = True
            return st, None
        loss.backward()
        st["grad_norm"] = float(nn.utils.clip_grad_norm_(self.net.parameters(), self.max_grad_norm))
        grads = {k: p.grad.detach().clone() for k, p in self.net.named_parameters()}
        self.opt.step()
        self.applied += 1
        return st, grads

    def moments(self):
        """{state_dict key: (exp_avg, exp_avg_sq)}"""
        return {k: (self.opt.state[p]["exp_avg"], self.opt.state[p]["exp_avg_sq"]) for k, p in self.net.named_parameters()}


def ref_explained_variance(ret, old_v):
    ret, old_v = np.asarray(ret, np.float64).reshape(-1), np.asarray(old_v, np.float64).reshape(-1)
    return float("nan") if ret.var() == 0 else 1.0 - (ret - old_v).var() / ret.var()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def make_state_dict(obs_dim, seed):
    """a random SB3 initialisation perturbed by N(0, 0.1) (the action head would otherwise sit at gain 0.01 and every gradient path
    through mu would be dwarfed), log_std with six distinct non-zero entries; float32 on the CPU"""
    from so100_mujoco_rl_amd.collector import RolloutCollector
    g = torch.Generator().manual_seed(1000 + seed)
    sd = RolloutCollector.random_policy_state(obs_dim, "cpu", seed=seed)
    sd = {k: (v + 0.1 * torch.randn(v.shape, generator=g)).float() for k, v in sd.items()}
    sd["log_std"] = torch.tensor([-0.5, -0.3, -0.1, 0.1, 0.2, 0.4]) + sd["log_std"] * 0.1
    return sd


def make_chunk(T, N, obs_dim, seed, state_dict, logp_noise=0.3):
    """a packed chunk [T, N, od+10] float32 with terminal observations [T, N, od] and last observations [N, od]: observations N(0, 1),
    actions the policy's samples, rewards N(0, 1), values V + N(0, 0.5), logp_old the reference log-prob + logp_noise N(0, 1); done codes
    0 / 1 / 2 drawn so that each occurs (when T*N allows), with a code 2 at t = T-1, a code 1 directly followed by a code 2 in one env and
    one env without an episode end; terminal observations hold 1e30 wherever the code is not 2"""
    g = torch.Generator().manual_seed(7000 + 131 * seed + T * 1009 + N)
    net = RefNet(obs_dim, state_dict)
    o = obs_dim
    obs = torch.randn(T, N, o, generator=g, dtype=torch.float64)
    with torch.no_grad():
        mean = net.mean_action(obs.reshape(-1, o)).reshape(T, N, 6)
        act = mean + net.log_std.exp() * torch.randn(T, N, 6, generator=g, dtype=torch.float64)
        v, lp = net.value(obs.reshape(-1, o)), net.log_prob(obs.reshape(-1, o), act.reshape(-1, 6))
    code = torch.multinomial(torch.tensor([0.7, 0.15, 0.15]), T * N, replacement=True, generator=g).reshape(T, N).double()
    if N >= 3:
        code[:, 0] = 0.0                                         # env 0: no episode end
        code[T - 1, 1] = 2.0                                     # env 1: truncated on the chunk's last step
        if T >= 2:
            code[0, 2] = 1.0; code[1, 2] = 2.0                   # env 2: terminated, then truncated one step later
        if T >= 3:
            code[2, 2] = 0.0
    buf = torch.zeros(T, N, o + 10, dtype=torch.float64)
    buf[..., :o] = obs; buf[..., o:o + 6] = act
    buf[..., o + 6] = torch.randn(T, N, generator=g, dtype=torch.float64)
    buf[..., o + 7] = code
    buf[..., o + 8] = v.reshape(T, N) + 0.5 * torch.randn(T, N, generator=g, dtype=torch.float64)
    buf[..., o + 9] = lp.reshape(T, N) + logp_noise * torch.randn(T, N, generator=g, dtype=torch.float64)
    tobs = torch.randn(T, N, o, generator=g, dtype=torch.float64)
    tobs[code != 2] = 1e30
    last_obs = torch.randn(N, o, generator=g, dtype=torch.float64)
    return buf.float(), tobs.float(), last_obs.float()


def flat_params(state_dict, obs_dim, device):
    """the state dict as the flat block of so100_learner_param_offset, float32 on `device`"""
    from so100_mujoco_rl_amd import lib
    layout, P = lib.learner_layout(obs_dim)
    flat = torch.zeros(P, dtype=torch.float32)
    for k, (off, shape) in layout.items():
        t = state_dict[lib.SB3_STATE_DICT_KEYS[k]].detach().cpu().float()
        assert tuple(t.shape) == tuple(shape)
        flat[off:off + t.numel()] = t.reshape(-1)
    return flat.to(device)


def split_flat(flat, obs_dim):
    """{state_dict key: float64 CPU tensor in its PyTorch shape} of a flat block"""
    from so100_mujoco_rl_amd import lib
    layout, _ = lib.learner_layout(obs_dim)
    f = flat.detach().cpu().double()
    return {lib.SB3_STATE_DICT_KEYS[k]: f[off:off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in layout.items()}


def rel_err(got, want):
    """max |got - want| / max |want| (float64 on the CPU)"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


# ---- what the two GPU modules do alike --------------------------------------------------------------------------------------------------------
def make_learner(od, max_minibatch=1024, **kw):
    from so100_mujoco_rl_amd.lib import So100Learner
    return So100Learner(od, "cuda", max_minibatch=max_minibatch, **kw)


@functools.lru_cache(maxsize=None)
def state_dict(od):
    return make_state_dict(od, seed=od)


def minibatch_indices(mb, n, seed):
    """mb distinct indices in random order, index 0 and index n - 1 among them (mb = 1: the last index)"""
    g = torch.Generator().manual_seed(seed)
    if mb == 1:
        return torch.tensor([n - 1])
    inner = (torch.randperm(n - 2, generator=g) + 1)[:mb - 2]
    idx = torch.cat([torch.tensor([0, n - 1]), inner])
    return idx[torch.randperm(mb, generator=g)]
