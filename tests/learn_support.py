"""What the learner tests share (test_learn_cpu.py, test_gpu_learner.py): the host twin of so100_learn.hpp (tests/_learncheck, loaded through
hostlibs._load with every signature declared), the fp64 PyTorch reference of include/so100_learn.h -- ActorCritic, the PPO._step loss, autograd,
clip_grad_norm_, torch.optim.Adam and the hand GAE recursion of test_ppo_cpu.py with the TimeLimit bootstrap applied -- and the inputs the GPU
tests are run on.  The reference is never the code under test: it shares no line with csrc/so100_learn.*."""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

import hostlibs
from hostlibs import ptr  # noqa: F401  (re-exported for the tests)

_p, _i, _l, _f, _d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double

# name: (restype, argtypes) of every extern "C" symbol of tests/_learncheck/learncheck.cpp
LEARNCHECK = {
    "lc_num_params": (_i, [_i]),
    "lc_tensor_offset": (_i, [_i, _i]),
    "lc_tensor_size": (_i, [_i, _i]),
    "lc_gae_d": (None, [_i, _p, _p, _p, _l, _p, _d, _d, _d, _p, _p, _l]),
    "lc_gae_f": (None, [_i, _p, _p, _p, _l, _p, _f, _f, _f, _p, _p, _l]),
    "lc_head_d": (None, [_p, _p]),
    "lc_head_f": (None, [_p, _p]),
    "lc_adam_d": (None, [_i, _p, _p, _p, _p, _d, _p]),
    "lc_adam_f": (None, [_i, _p, _p, _p, _p, _f, _p]),
}


def learncheck():
    d = os.path.join(hostlibs.HERE, "_learncheck")
    return hostlibs._load(os.path.join(d, "liblearncheck.so"), d, [], LEARNCHECK)


HYPER = dict(gamma=0.99, gae_lambda=0.95, clip=0.2, vf_coef=0.5, max_grad_norm=0.5, lr=3e-4, beta1=0.9, beta2=0.999, adam_eps=1e-5)      # ppo.py's


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------------------
def ref_net(obs_dim, state_dict):
    """ActorCritic in float64 holding a copy of state_dict"""
    from so100_mujoco_rl_amd.ppo import ActorCritic
    net = ActorCritic(obs_dim).double()
    net.load_state_dict({k: v.detach().cpu().double() for k, v in state_dict.items()})
    return net


def ref_advantages(buf, last_obs, net, terminal_obs=None, gamma=HYPER["gamma"], lam=HYPER["gae_lambda"]):
    """buf: packed chunk [T, N, od+10] (any float dtype); returns adv [T, N], ret [T, N], mean, unbiased std as float64 tensors: the hand
    recursion of test_ppo_cpu.py, rewards += gamma V(terminal_obs) on the code-2 steps first (rollout.bootstrap_truncated)"""
    buf = buf.detach().cpu().double(); T, N, k = buf.shape; o = k - 10
    rew, code, val = buf[..., o + 6].clone(), buf[..., o + 7], buf[..., o + 8]
    with torch.no_grad():
        last_v = net.value(last_obs.detach().cpu().double())
        if terminal_obs is not None:
            for t, n in (code == 2).nonzero().tolist():
                rew[t, n] += gamma * net.value(terminal_obs[t, n].detach().cpu().double().unsqueeze(0))[0]
    adv = torch.zeros(T, N, dtype=torch.float64)
    for n in range(N):
        g = 0.0
        for t in reversed(range(T)):
            nv = last_v[n] if t == T - 1 else val[t + 1, n]
            nonterm = 1.0 if code[t, n] == 0 else 0.0
            delta = rew[t, n] + gamma * nv * nonterm - val[t, n]
            g = delta + gamma * lam * nonterm * g
            adv[t, n] = g
    a = adv.reshape(-1)
    return adv, adv + val, a.mean(), a.std()


def ref_loss(net, buf, idx, adv, ret, mean, std, clip=HYPER["clip"], vf_coef=HYPER["vf_coef"]):
    """the PPO._step loss on rows idx of the packed chunk, float64; returns loss and the parts the stats are made of"""
    buf = buf.detach().cpu().double(); k = buf.shape[-1]; o = k - 10
    rows = buf.reshape(-1, k)[idx]
    v, lp = net.evaluate(rows[:, :o], rows[:, o:o + 6])
    adv_n = ((adv.reshape(-1) - mean) / (std + 1e-8))[idx]
    ratio = (lp - rows[:, o + 9]).exp()
    pg = -torch.min(ratio * adv_n, ratio.clamp(1 - clip, 1 + clip) * adv_n).mean()
    vl = (ret.reshape(-1)[idx] - v).pow(2).mean()
    r = ratio.detach()
    active = ((adv_n > 0) & (r > 1 + clip)) | ((adv_n < 0) & (r < 1 - clip))          # the clip removes this sample's policy gradient
    # clipped_count: samples with |ratio - 1| > clip; borderline: those whose ratio lies within 1e-5 of 1 +- clip, the only ones an fp32
    # ratio (relative error ~1e-6 after the exp of a sum of ~20 terms) can put on the other side
    border = int((((r - 1).abs() - clip).abs() < 1e-5).sum())
    return pg + vf_coef * vl, {"policy_loss": pg.item(), "value_loss": vl.item(), "clip_fraction": ((r - 1).abs() > clip).double().mean().item(),
                               "clipped_count": int(((r - 1).abs() > clip).sum()), "borderline": border,
                               "active_share": active.double().mean().item(), "high": int((active & (r > 1)).sum()), "low": int((active & (r < 1)).sum())}


class RefLearner:
    """net + torch.optim.Adam + clip_grad_norm_, float64: the update PPO.update makes, on given permutations"""

    def __init__(self, obs_dim, state_dict, max_grad_norm=HYPER["max_grad_norm"], lr=HYPER["lr"]):
        self.net = ref_net(obs_dim, state_dict)
        self.opt = torch.optim.Adam(self.net.parameters(), lr=lr, eps=HYPER["adam_eps"])
        self.max_grad_norm = max_grad_norm

    def step(self, buf, idx, adv, ret, mean, std):
        """one minibatch step; returns (stats incl. the pre-clip grad_norm, {state_dict key: clipped gradient})"""
        self.opt.zero_grad(set_to_none=True)
        loss, st = ref_loss(self.net, buf, idx, adv, ret, mean, std)
        loss.backward()
        st["grad_norm"] = float(nn.utils.clip_grad_norm_(self.net.parameters(), self.max_grad_norm))
        grads = {k: p.grad.detach().clone() for k, p in self.net.named_parameters()}
        self.opt.step()
        return st, grads

    def moments(self):
        """{state_dict key: (exp_avg, exp_avg_sq)}"""
        return {k: (self.opt.state[p]["exp_avg"], self.opt.state[p]["exp_avg_sq"]) for k, p in self.net.named_parameters()}


# ---- inputs of the GPU tests ----------------------------------------------------------------------------------------------------------------
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
    net = ref_net(obs_dim, state_dict)
    o = obs_dim
    obs = torch.randn(T, N, o, generator=g, dtype=torch.float64)
    with torch.no_grad():
        mean = net.mean_action(obs.reshape(-1, o)).reshape(T, N, 6)
        act = mean + net.log_std.exp() * torch.randn(T, N, 6, generator=g, dtype=torch.float64)
        v, lp = net.evaluate(obs.reshape(-1, o), act.reshape(-1, 6))
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
