"""The on-device learner without a device: include/so100_learn.h is exported and bound, argument checks and the missing-device error are loud,
the flat parameter block is laid out as documented, the arithmetic templates of csrc/so100_learn.hpp (instantiated on the host in double by
tests/_learncheck) agree with the fp64 reference of learn_support.py, and FusedPPO's network is an ordinary ActorCritic over views of one block.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hostlibs
import learn_support as LS
from learn_support import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib.load()


def test_every_declared_learner_symbol_is_exported(L):
    from so100_mujoco_rl_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "so100_learn.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(so100_[a-z_]+)\s*\(", src)))
    assert len(syms) >= 6 and syms == sorted(lib.LEARN_EXPORTS), (syms, lib.LEARN_EXPORTS)
    for s in syms:
        assert hasattr(L, s), s
    assert not set(lib.LEARN_EXPORTS) & set(lib.EXPORTS)         # additive: the list of so100_sim.h is untouched
    assert L.so100_abi_version() == 3


def test_ctypes_structs_match_the_header():
    """field names and order of the three structs, as the header declares them"""
    from so100_mujoco_rl_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "so100_learn.h")).read(), flags=re.S)
    for cname, struct in (("so100_learner_config", lib.LearnerConfig), ("so100_advantages_io", lib.AdvantagesIO), ("so100_minibatch_io", lib.MinibatchIO)):
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", src).group(1)
        names = []
        for decl in body.split(";"):
            names += [w.strip(" *") for w in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip(), count=1).split(",") if w.strip()]
        assert names == [f[0] for f in struct._fields_], cname


def _cfg(lib, **over):
    kw = dict(obs_dim=15, device=0, max_minibatch=64, gamma=0.99, gae_lambda=0.95, clip_range=0.2, vf_coef=0.5, max_grad_norm=0.5, lr=3e-4,
              beta1=0.9, beta2=0.999, adam_eps=1e-5)
    kw.update(over)
    return lib.LearnerConfig(*[kw[f[0]] for f in lib.LearnerConfig._fields_])


def test_create_validates_arguments_and_has_no_cpu_fallback(L):
    from so100_mujoco_rl_amd import lib
    h = C.c_void_p()
    for over, word in ((dict(obs_dim=9), b"obs_dim"), (dict(obs_dim=0), b"obs_dim"), (dict(max_minibatch=0), b"max_minibatch"), (dict(max_minibatch=-5), b"max_minibatch"),
                       (dict(clip_range=0.0), b"clip_range"), (dict(beta2=1.0), b"beta"), (dict(adam_eps=0.0), b"adam_eps")):
        assert L.so100_learner_create(C.byref(_cfg(lib, **over)), C.byref(h)) == -1, over
        assert word in L.so100_last_error(), (over, L.so100_last_error())
        assert not h.value
    assert L.so100_learner_create(None, C.byref(h)) == -1
    if not torch.cuda.is_available():
        assert L.so100_learner_create(C.byref(_cfg(lib)), C.byref(h)) == -2
        assert b"no CPU fallback" in L.so100_last_error()
        with pytest.raises(lib.So100Error):
            lib.So100Learner(15)


def test_parameter_block_layout(L):
    from so100_mujoco_rl_amd import lib
    from so100_mujoco_rl_amd.ppo import ActorCritic
    assert L.so100_learner_num_params(15) == 10829 and L.so100_learner_num_params(8) == 9933
    assert L.so100_learner_num_params(7) < 0 and L.so100_learner_param_offset(15, b"nope") < 0 and L.so100_learner_param_offset(3, b"pi_w0") < 0
    tw = hostlibs.learncheck()
    for od in (15, 8):
        shapes = {k: tuple(v.shape) for k, v in ActorCritic(od).state_dict().items()}
        layout, P = lib.learner_layout(od)
        assert list(layout) == lib.POLICY_TENSORS and P == sum(int(np.prod(s)) for s in shapes.values()) == tw.lc_num_params(od)
        off = 0
        for i, k in enumerate(lib.POLICY_TENSORS):               # contiguous, in POLICY_TENSORS order, PyTorch shapes
            assert layout[k] == (off, shapes[lib.SB3_STATE_DICT_KEYS[k]]), k
            assert L.so100_learner_param_size(od, k.encode()) == int(np.prod(layout[k][1])) == tw.lc_tensor_size(i, od)
            assert tw.lc_tensor_offset(i, od) == off
            off += int(np.prod(layout[k][1]))
        assert off == P


REL = 1e-12      # fp64 arithmetic on both sides (the hostcheck convention)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= REL * scale, (what, np.abs(got - want).max())


@pytest.mark.parametrize("od", [15, 8])
def test_gae_scan_in_double_matches_the_reference(od):
    tw = hostlibs.learncheck()
    T, N = 7, 9
    sd = LS.make_state_dict(od, 3)
    buf, tobs, last_obs = LS.make_chunk(T, N, od, 3, sd)
    net = LS.RefNet(od, sd)
    b = buf.double().numpy(); k = od + 10
    with torch.no_grad():
        last_v = net.value(last_obs.double()).numpy()
        boot = np.zeros((T, N))
        for t, n in (buf[..., od + 7] == 2).nonzero().tolist():
            boot[t, n] = float(net.value(tobs[t, n].double().unsqueeze(0))[0])
    assert set(np.unique(b[..., od + 7])) == {0.0, 1.0, 2.0}
    for use_boot in (True, False):
        adv_r, ret_r, _, _ = LS.ref_advantages(buf, last_obs, net, terminal_obs=tobs if use_boot else None)
        adv = np.zeros((T, N)); ret = np.zeros((T, N))
        for n in range(N):
            col = lambda c: C.c_void_p(b.ctypes.data + 8 * (n * k + od + c))
            tw.lc_gae_d(T, col(6), col(7), col(8), N * k, C.c_void_p(boot.ctypes.data + 8 * n) if use_boot else None, float(last_v[n]),
                        LS.HYPER["gamma"], LS.HYPER["gae_lambda"], C.c_void_p(adv.ctypes.data + 8 * n), C.c_void_p(ret.ctypes.data + 8 * n), N)
        _close(adv, adv_r.numpy(), "adv"); _close(ret, ret_r.numpy(), "ret")
    # the bootstrap value may sit in the return buffer itself (what the kernel does): entry t is read before ret[t] is written
    ret2 = boot.copy(); adv2 = np.zeros((T, N))
    for n in range(N):
        col = lambda c: C.c_void_p(b.ctypes.data + 8 * (n * k + od + c))
        tw.lc_gae_d(T, col(6), col(7), col(8), N * k, C.c_void_p(ret2.ctypes.data + 8 * n), float(last_v[n]), LS.HYPER["gamma"], LS.HYPER["gae_lambda"],
                    C.c_void_p(adv2.ctypes.data + 8 * n), C.c_void_p(ret2.ctypes.data + 8 * n), N)
    assert np.array_equal(adv2, adv_with_boot(tw, b, boot, last_v, T, N, od)) and not np.array_equal(ret2, boot)


def adv_with_boot(tw, b, boot, last_v, T, N, od):
    k = od + 10
    adv = np.zeros((T, N)); ret = np.zeros((T, N))
    for n in range(N):
        col = lambda c: C.c_void_p(b.ctypes.data + 8 * (n * k + od + c))
        tw.lc_gae_d(T, col(6), col(7), col(8), N * k, C.c_void_p(boot.ctypes.data + 8 * n), float(last_v[n]), LS.HYPER["gamma"], LS.HYPER["gae_lambda"],
                    C.c_void_p(adv.ctypes.data + 8 * n), C.c_void_p(ret.ctypes.data + 8 * n), N)
    return adv


def test_loss_head_in_double_matches_autograd():
    """per sample: the loss terms and d(minibatch loss)/d(mu, log_std, V) against autograd on the PPO._step expression; samples inside the clip
    range, clipped on either side with either sign of the advantage, and exactly on the tie ratio*A == clamp(ratio)*A"""
    tw = hostlibs.learncheck()
    rs = np.random.RandomState(5)
    clip, vf, inv_mb = 0.2, 0.5, 1.0 / 37
    seen = set()
    for case in range(200):
        mu, ls, a = rs.randn(6) * 0.5, rs.randn(6) * 0.3, rs.randn(6)
        adv_n, V, ret = rs.randn(), rs.randn(), rs.randn()
        tmu, tls, tV = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (mu, ls, V))
        lp = (-0.5 * ((torch.tensor(a) - tmu) / tls.exp()) ** 2 - tls - 0.9189385332046727).sum()
        logp_old = lp.item() + (0.0 if case % 10 == 0 else 0.3 * rs.randn())       # case % 10 == 0: ratio == 1 exactly, the tie
        ratio = (lp - logp_old).exp()
        pg = -torch.min(ratio * adv_n, ratio.clamp(1 - clip, 1 + clip) * adv_n)
        vl = (ret - tV) ** 2
        ((pg + vf * vl) * inv_mb).backward()
        seen.add((ratio.item() > 1 + clip, ratio.item() < 1 - clip, adv_n > 0))
        inp = np.concatenate([mu, ls, a, [logp_old, adv_n, V, ret, clip, vf, inv_mb]]); out = np.zeros(16)
        tw.lc_head_d(ptr(inp), ptr(out))
        _close(out[0], pg.item(), "pg"); _close(out[1], vl.item(), "vl")
        assert out[2] == float(abs(ratio.item() - 1) > clip)
        _close(out[3:9], tmu.grad.numpy(), "dmu"); _close(out[9:15], tls.grad.numpy(), "dlog_std"); _close(out[15], tV.grad.item(), "dV")
    assert len(seen) == 6                                         # inside / above / below the range x both signs of the advantage


def test_clip_and_adam_in_double_match_torch():
    tw = hostlibs.learncheck()
    rs = np.random.RandomState(6)
    n = 50
    for max_norm in (0.05, 100.0):                                # clipping engaged / not engaged
        p0 = rs.randn(n)
        p = torch.nn.Parameter(torch.tensor(p0))
        opt = torch.optim.Adam([p], lr=3e-4, eps=1e-5)
        pt, m, v = p0.copy(), np.zeros(n), np.zeros(n)
        for step in range(1, 6):
            g = rs.randn(n) * 0.1
            p.grad = torch.tensor(g.copy())
            norm = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
            assert (norm > max_norm) == (max_norm < 1.0)
            clipped = p.grad.numpy().copy()
            opt.step()
            hyper = np.array([max_norm, 3e-4 / (1 - 0.9 ** step), 1 - 0.9, 0.999, 1 - 0.999, 1e-5, (1 - 0.999 ** step) ** 0.5])
            gt = g.copy()
            tw.lc_adam_d(n, ptr(gt), ptr(pt), ptr(m), ptr(v), float(np.sqrt((g * g).sum())), ptr(hyper))
            _close(gt, clipped, "clipped gradient"); _close(pt, p.detach().numpy(), "param")
            _close(m, opt.state[p]["exp_avg"].numpy(), "m"); _close(v, opt.state[p]["exp_avg_sq"].numpy(), "v")


def test_float_instantiation_is_the_double_one_rounded():
    """the float twin (what the kernels instantiate) follows the double one to fp32 rounding"""
    tw = hostlibs.learncheck()
    rs = np.random.RandomState(8)
    inp = np.concatenate([rs.randn(6) * 0.5, rs.randn(6) * 0.3, rs.randn(6), [-8.0, 0.7, 0.2, -0.4, 0.2, 0.5, 1.0 / 64]])
    out_d = np.zeros(16); out_f = np.zeros(16, np.float32)
    inp_f = inp.astype(np.float32)
    tw.lc_head_d(ptr(inp_f.astype(np.float64)), ptr(out_d)); tw.lc_head_f(ptr(inp_f), ptr(out_f))
    assert np.abs(out_f - out_d).max() <= 2e-5 * max(1.0, np.abs(out_d).max())


@pytest.mark.parametrize("od", [15, 8])
def test_fused_ppo_network_is_an_actor_critic_over_one_flat_block(od):
    from so100_mujoco_rl_amd import lib
    from so100_mujoco_rl_amd.ppo import PPO, ActorCritic, FusedPPO
    f = FusedPPO(od, "cpu", seed=4)
    sd = f.net.state_dict()
    assert list(sd) == list(ActorCritic(od).state_dict())
    layout, P = lib.learner_layout(od)
    assert f.params.shape == (P,) and f.adam_m.shape == (P,) and f.adam_v.shape == (P,)
    base = f.params.data_ptr()
    for k, (off, shape) in layout.items():
        t = sd[lib.SB3_STATE_DICT_KEYS[k]]
        assert t.data_ptr() == base + 4 * off and tuple(t.shape) == tuple(shape) and t.is_contiguous(), k
    ref = PPO(od, "cpu", seed=4).net.state_dict()                 # the same initialisation for the same seed
    assert all(torch.equal(sd[k], ref[k]) for k in ref)
    f.params.add_(1.0)                                            # the block IS the network
    assert all(torch.equal(f.net.state_dict()[k], ref[k] + 1.0) for k in ref)
    f.net.load_state_dict(ref)                                    # and a loaded checkpoint lands in the block
    assert torch.equal(f.params[layout["v_b"][0]], ref["value_net.bias"][0]) and f.net.state_dict()["log_std"].data_ptr() == base + 4 * layout["log_std"][0]
    obs = torch.randn(5, od)
    assert torch.equal(f.net.mean_action(obs), PPO(od, "cpu", seed=4).net.mean_action(obs))
    if not torch.cuda.is_available():
        with pytest.raises(lib.So100Error, match="no CPU fallback"):
            f.update({"obs": torch.zeros(2, 3, od), "actions": torch.zeros(2, 3, 6), "rewards": torch.zeros(2, 3), "dones": torch.zeros(2, 3),
                      "values": torch.zeros(2, 3), "log_probs": torch.zeros(2, 3), "last_obs": torch.zeros(3, od)})


def test_collector_defer_bootstrap_is_opt_in():
    import inspect
    from so100_mujoco_rl_amd.collector import RolloutCollector
    sig = inspect.signature(RolloutCollector.__init__)
    assert sig.parameters["defer_bootstrap"].default is False
