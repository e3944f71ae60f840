"""Reward normalisation on the GPU (so100_learner_normalize_rewards, so100_learner_advantages_r, so100_learner_update_r, both Python learners,
`train --normalize-reward`): the kernels against the numpy reference of reward_norm_support.py, the new entry points against the old ones on
the same floats (to the bit), the one call against its launches made by hand (to the bit), FusedPPO against the fp64 reference learner of
learn_support.py fed the reference's normalised rewards, the argument errors and the command line.

Tolerances.  The kernels: reward_norm_support.py (1 fp32 ulp, 1e-10 on the moments, derived there).  The learner: PARAM_REF_TOL / MOMENT_TOL of
test_gpu_learner.py, the bounds the project holds for the same comparison without the normalisation.  Shapes: one env; one block of 64 and
three envs; several blocks with T = 64; and two blocks plus six envs, the smallest N at which a third, partial block is merged."""
import ctypes as C
import functools
import logging
import math

import numpy as np
import pytest
import torch

import hostlibs
import learn_support as LS
import reward_norm_support as RS
import update_support as US
from learn_support import make_learner, state_dict
from test_gpu_learner import MOMENT_TOL, PARAM_REF_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
OD = 15
BLOCK = 64                                            # csrc/so100_learn.hpp RN_BLOCK (asserted against the twin below)
GPU_SHAPES = RS.SHAPES + [(16, 2 * BLOCK + 6)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def packed(rewards, codes, od=OD, seed=0):
    """a [T, N, od+10] chunk on the device whose reward and done-code columns are the given ones; the other columns hold noise"""
    T, N = rewards.shape
    g = torch.Generator().manual_seed(50 + seed)
    buf = torch.randn(T, N, od + 10, generator=g)
    buf[..., od + 6] = torch.from_numpy(np.array(rewards)); buf[..., od + 7] = torch.from_numpy(np.array(codes))
    return buf.to(DEV)


def device_state(st):
    return torch.from_numpy(np.array(st, np.float64)).to(DEV)


def run_normalize(L, buf, state):
    T, N = buf.shape[0], buf.shape[1]
    out = torch.full((T, N), 77.0, device=DEV)
    ws = torch.zeros(L.reward_norm_workspace_bytes(T, N) // 8, dtype=torch.float64, device=DEV)
    L.normalize_rewards(buf, state, out, ws)
    return out


# ---- 1. the kernels against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", GPU_SHAPES)
def test_normalize_rewards_matches_the_reference(T, N):
    assert hostlibs.learncheck().rn_block() == BLOCK
    L = make_learner(OD, 64)
    rewards, codes = RS.make_inputs(T, N)
    want, want_st = RS.reference(T, N)
    buf = packed(rewards, codes); before = buf.clone()
    st = torch.full((3 + N,), 5.0, dtype=torch.float64, device=DEV)
    L.reward_norm_init(st)
    assert st.tolist() == RS.fresh_state(N).tolist()
    out = run_normalize(L, buf, st)
    ulps, rel = RS.check_against_reference(out.cpu().numpy(), st.cpu().numpy(), want, want_st, codes)
    print(f"[rewnorm] gpu ({T}, {N}): {ulps} ulp, mean {rel[0]:.2e}, var {rel[1]:.2e}")
    assert same_bits(buf, before)                                              # the chunk is read only
    # determinism: the same call from a restored copy of the state
    st2 = device_state(RS.fresh_state(N))
    out2 = run_normalize(L, buf, st2)
    assert same_bits(out, out2) and same_bits(st, st2)
    # a second chunk continues from the first's state and equals the run of 2T
    rb, cb = RS.make_inputs(T, N, seed=2)
    out_b = run_normalize(L, packed(rb, cb, seed=1), st)
    both_r, both_c = np.concatenate([rewards, rb]), np.concatenate([codes, cb])
    st_w = device_state(RS.fresh_state(N))
    whole = run_normalize(L, packed(both_r, both_c), st_w)
    assert same_bits(torch.cat([out, out_b]), whole) and same_bits(st, st_w)
    want2, want_st2 = RS.ref_normalize(both_r, both_c, RS.fresh_state(N))
    RS.check_against_reference(whole.cpu().numpy(), st_w.cpu().numpy(), want2, want_st2, both_c)


def test_one_env_clips_on_the_device():
    L = make_learner(OD, 64)
    st = device_state(RS.fresh_state(1))
    out = run_normalize(L, packed(np.array([[5.0], [-7.0]], np.float32), np.zeros((2, 1), np.float32)), st)
    want, _ = RS.ref_normalize(np.array([[5.0], [-7.0]], np.float32), np.zeros((2, 1)), RS.fresh_state(1))
    assert out[0, 0].item() == 10.0 and RS.ulp_distance(out.cpu().numpy(), want) <= 1


# ---- 2. the advantages' second reward source ------------------------------------------------------------------------------------------------------
AT, AN = 8, 67


@functools.lru_cache(maxsize=None)
def adv_chunk(od):
    buf, tobs, last_obs = LS.make_chunk(AT, AN, od, 3, state_dict(od))
    assert (buf[..., od + 7] == 2).any()
    return buf.to(DEV), tobs.to(DEV), last_obs.to(DEV)


@pytest.mark.parametrize("od", [15, 8])
def test_advantages_r_equals_the_old_call_on_the_same_floats(od):
    L = make_learner(od, 64)
    buf, tobs, last_obs = adv_chunk(od)
    params = LS.flat_params(state_dict(od), od, DEV)
    dense = (torch.randn(AT, AN, generator=torch.Generator().manual_seed(8)) * 2 + 1).to(DEV)
    moved = buf.clone(); moved[..., od + 6] = dense
    res = []
    for chunk, rewards in ((moved, None), (buf, dense)):
        adv, ret, stats = torch.full((AT, AN), 3.0, device=DEV), torch.full((AT, AN), 3.0, device=DEV), torch.full((2,), 3.0, device=DEV)
        L.advantages(chunk, last_obs, params, adv, ret, stats, terminal_obs=tobs, rewards=rewards)
        res.append((adv, ret, stats))
    assert all(same_bits(a, b) for a, b in zip(*res))
    # a null reward_dev is the old call
    from so100_mujoco_rl_amd import lib
    adv, ret, stats = torch.full((AT, AN), 3.0, device=DEV), torch.full((AT, AN), 3.0, device=DEV), torch.full((2,), 3.0, device=DEV)
    io = lib.AdvantagesIO(moved.data_ptr(), tobs.data_ptr(), last_obs.data_ptr(), params.data_ptr(), adv.data_ptr(), ret.data_ptr(), stats.data_ptr())
    assert L.L.so100_learner_advantages_r(L.h, C.byref(io), None, AT, AN, L._stream()) == 0
    assert all(same_bits(a, b) for a, b in zip(res[0], (adv, ret, stats)))
    assert not torch.equal(res[0][0], torch.full((AT, AN), 3.0, device=DEV))


# ---- 3. the one call ------------------------------------------------------------------------------------------------------------------------------
UMB, UEPOCHS = 100, 2
ROWS = AT * AN


class Buffers:
    def __init__(self, L, od, extended):
        P = L.num_params
        self.params = LS.flat_params(state_dict(od), od, DEV); self.m = torch.zeros(P, device=DEV); self.v = torch.zeros(P, device=DEV)
        self.adv = torch.full((AT, AN), 3.0, device=DEV); self.ret = torch.full((AT, AN), 3.0, device=DEV); self.adv_stats = torch.full((2,), 3.0, device=DEV)
        self.perm = torch.full((ROWS,), -1, dtype=torch.int64, device=DEV)
        self.out = torch.full((15,), 7.0, device=DEV)
        self.state = torch.full((2,), 7, dtype=torch.int32, device=DEV) if extended else None
        self.rn_state = device_state(RS.fresh_state(AN))
        self.rewards = torch.full((AT, AN), 9.0, device=DEV)
        self.ws = torch.zeros(L.reward_norm_workspace_bytes(AT, AN) // 8, dtype=torch.float64, device=DEV)

    def everything(self):
        return [self.params, self.m, self.v, self.adv, self.ret, self.adv_stats, self.perm, self.out, self.rn_state, self.rewards] + ([self.state] if self.state is not None else [])


@pytest.mark.parametrize("od,terms", [(15, None), (15, LS.ALL_TERMS), (8, LS.ALL_TERMS)], ids=["od15-plain", "od15-all", "od8-all"])
def test_update_r_equals_its_launches_by_hand_to_the_bit(od, terms):
    from so100_mujoco_rl_amd import lib
    L = make_learner(od, UMB)
    buf, tobs, last_obs = adv_chunk(od)
    before = buf.clone()
    seed, e0, step0 = 5, 3, 4
    H = Buffers(L, od, terms is not None)
    off = lib.learner_layout(od)[0]["log_std"][0]
    L.normalize_rewards(buf, H.rn_state, H.rewards, H.ws)
    L.advantages(buf, last_obs, H.params, H.adv, H.ret, H.adv_stats, terminal_obs=tobs, rewards=H.rewards)
    L.explained_variance(buf, H.ret, H.out[8:9])
    if H.state is not None:
        H.state.zero_()
    step, last = step0, step0 + UEPOCHS * math.ceil(ROWS / UMB)
    for e in range(UEPOCHS):
        L.shuffle(seed, e0 + e, ROWS, H.perm)
        for i in range(0, ROWS, UMB):
            step += 1
            if step == last:
                H.out[9:15].copy_(H.params[off:off + 6])
            if terms is None:
                L.minibatch_step(buf, H.perm[i:i + UMB], H.adv, H.ret, H.adv_stats, H.params, H.m, H.v, step, H.out[0:4])
            else:
                L.minibatch_step_ex(buf, H.perm[i:i + UMB], H.adv, H.ret, H.adv_stats, H.params, H.m, H.v, step, H.out[0:8], update_state=H.state, **terms)
    U = Buffers(L, od, terms is not None)
    L.update(buf, last_obs, U.params, U.m, U.v, U.adv, U.ret, U.adv_stats, U.perm, U.out, epochs=UEPOCHS, mb=UMB, adam_step0=step0, shuffle_seed=seed,
             shuffle_epoch0=e0, terminal_obs=tobs, terms=terms, update_state=U.state, reward_norm=dict(state=U.rn_state, rewards=U.rewards, workspace=U.ws))
    for i, (h, u) in enumerate(zip(H.everything(), U.everything())):
        assert same_bits(h, u), i
    assert same_bits(buf, before)
    want, want_st = RS.ref_normalize(buf[..., od + 6].cpu().numpy(), buf[..., od + 7].cpu().numpy(), RS.fresh_state(AN))
    RS.check_against_reference(U.rewards.cpu().numpy(), U.rn_state.cpu().numpy(), want, want_st, buf[..., od + 7].cpu().numpy())
    assert float((U.params - LS.flat_params(state_dict(od), od, DEV)).abs().max()) > 2e-4
    # the normalised rewards were what the advantages read: with the chunk's own rewards they differ
    P = Buffers(L, od, terms is not None)
    L.advantages(buf, last_obs, P.params, P.adv, P.ret, P.adv_stats, terminal_obs=tobs)
    assert not torch.equal(P.adv, U.adv)


def test_update_r_without_a_norm_io_is_the_old_update():
    from so100_mujoco_rl_amd import lib
    od = 15
    L = make_learner(od, UMB)
    buf, tobs, last_obs = adv_chunk(od)
    A, B = Buffers(L, od, False), Buffers(L, od, False)
    L.update(buf, last_obs, A.params, A.m, A.v, A.adv, A.ret, A.adv_stats, A.perm, A.out, epochs=UEPOCHS, mb=UMB, adam_step0=0, shuffle_seed=9, terminal_obs=tobs)
    p = lambda t: t.data_ptr()
    io = lib.UpdateIO(rollout_dev=p(buf), terminal_obs_chunk_dev=p(tobs), last_obs_dev=p(last_obs), T=AT, N=AN, params_dev=p(B.params), adam_m_dev=p(B.m),
                      adam_v_dev=p(B.v), adv_dev=p(B.adv), ret_dev=p(B.ret), adv_stats_dev=p(B.adv_stats), perm_dev=p(B.perm), epochs=UEPOCHS, mb=UMB, adam_step0=0,
                      shuffle_epoch0=0, shuffle_seed=9, out_dev=p(B.out))
    assert L.L.so100_learner_update_r(L.h, C.byref(io), None, L._stream()) == 0
    for a, b in zip(A.everything(), B.everything()):
        assert same_bits(a, b)
    assert B.rewards.unique().tolist() == [9.0]                                # nothing touched the normalisation's buffers


# ---- 4. the Python learners -------------------------------------------------------------------------------------------------------------------------
FT, FN, FMB, FEPOCHS = 4, 300, 400, 2              # test_gpu_learner.py's update shape: 1200 rows, 2 epochs x 3 minibatches


@functools.lru_cache(maxsize=None)
def learner_chunk():
    return LS.make_chunk(FT, FN, OD, 0, state_dict(OD))


def learner_batch():
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    buf, tobs, last_obs = learner_chunk()
    c = RolloutChunk(FT, FN, OD, DEV); c.buf.copy_(buf)
    b = c.unpack(); b["last_obs"] = last_obs.to(DEV); b["terminal_obs"] = torch.where(tobs > 1e29, torch.zeros_like(tobs), tobs).to(DEV); b["packed"] = c.buf
    return b


@functools.lru_cache(maxsize=None)
def normalised_chunk():
    """the chunk with the reference's normalised rewards in its reward column, and the reference's state after it"""
    buf, tobs, last_obs = learner_chunk()
    want, want_st = RS.ref_normalize(buf[..., OD + 6].numpy(), buf[..., OD + 7].numpy(), RS.fresh_state(FN))
    nb = buf.clone(); nb[..., OD + 6] = torch.from_numpy(want)
    return nb, want_st


def reference_learner(perms):
    nb, _ = normalised_chunk()
    _, tobs, last_obs = learner_chunk()
    ref = LS.RefLearner(OD, state_dict(OD))
    adv, ret, mean, std = LS.ref_advantages(nb, last_obs, LS.RefNet(OD, state_dict(OD)), terminal_obs=tobs)
    for perm in perms:
        for i in range(0, FT * FN, FMB):
            ref.step(nb, perm[i:i + FMB], adv, ret, mean, std)
    return ref


@pytest.mark.parametrize("shuffle", ["torch", "device"])
def test_fused_ppo_matches_the_fp64_reference_on_the_normalised_rewards(shuffle):
    from so100_mujoco_rl_amd.ppo import PPO, FusedPPO
    seed = 21
    f = FusedPPO(OD, DEV, epochs=FEPOCHS, minibatch=FMB, seed=seed, shuffle=shuffle, normalize_reward=True)
    f.net.load_state_dict({k: v.to(DEV) for k, v in state_dict(OD).items()})
    if shuffle == "torch":
        g = torch.Generator().manual_seed(77)
        perms = [torch.randperm(FT * FN, generator=g) for _ in range(FEPOCHS)]
        stats = f.update(learner_batch(), perms=[p.to(DEV) for p in perms])
    else:
        perms = [torch.from_numpy(US.ref_perm_cached(seed, e, FT * FN).copy()) for e in range(FEPOCHS)]
        stats = f.update(learner_batch())
    ref = reference_learner(perms)
    want = ref.net.state_dict(); mom = ref.moments()
    got_p, got_m, got_v = LS.split_flat(f.params, OD), LS.split_flat(f.adam_m, OD), LS.split_flat(f.adam_v, OD)
    ep = max(LS.rel_err(got_p[k], want[k]) for k in want)
    em = max(LS.rel_err(got_m[k], mom[k][0]) for k in want)
    ev = max(LS.rel_err(got_v[k], mom[k][1]) for k in want)
    print(f"[rewnorm] fused {shuffle}: params {ep:.3e} exp_avg {em:.3e} exp_avg_sq {ev:.3e}")
    assert ep <= PARAM_REF_TOL and em <= MOMENT_TOL and ev <= MOMENT_TOL
    assert max(float((got_p[k] - state_dict(OD)[k].double()).abs().max()) for k in want) > 1e-3
    _, want_st = normalised_chunk()
    sd = f.reward_norm_state()
    assert stats["return_count"] == sd["count"].item() == want_st[2] and stats["return_var"] == sd["var"].item()
    assert abs(stats["return_var"] - want_st[1]) <= RS.MOMENT_TOL * want_st[1]
    buf = learner_chunk()[0]
    assert stats["mean_reward"] == pytest.approx(buf[..., OD + 6].mean().item(), rel=1e-6)      # the env's raw mean
    # the PyTorch learner on the same device agrees on the running variance, and a restored fused learner continues from the saved state
    t = PPO(OD, DEV, epochs=1, minibatch=FT * FN, seed=seed, normalize_reward=True)
    s_t = t.update(learner_batch())
    assert abs(s_t["return_var"] - stats["return_var"]) <= RS.MOMENT_TOL * stats["return_var"] and s_t["return_count"] == stats["return_count"]
    f2 = FusedPPO(OD, DEV, epochs=FEPOCHS, minibatch=FMB, seed=seed, shuffle=shuffle, normalize_reward=True)
    f2.load_reward_norm_state(sd)
    assert all(torch.equal(f2.reward_norm_state()[k], sd[k]) for k in sd)
    f.update(learner_batch(), **({"perms": [p.to(DEV) for p in perms]} if shuffle == "torch" else {}))
    f2.update(learner_batch(), **({"perms": [p.to(DEV) for p in perms]} if shuffle == "torch" else {}))
    assert all(torch.equal(f2.reward_norm_state()[k], f.reward_norm_state()[k]) for k in sd) and same_bits(f._rn_rewards, f2._rn_rewards)


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_enqueue_nothing():
    from so100_mujoco_rl_amd import lib
    T, N = 4, 70
    learner = make_learner(OD, 64)
    L, stream = learner.L, learner._stream()
    rewards, codes = RS.make_inputs(T, N)
    buf = packed(rewards, codes)
    st = device_state(RS.fresh_state(N) + 0.25); out = torch.full((T, N), 77.0, device=DEV)
    need = learner.reward_norm_workspace_bytes(T, N)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    p = lambda t: t.data_ptr()

    def io(**over):
        kw = dict(rollout_dev=p(buf), state_dev=p(st), reward_dev=p(out), workspace_dev=p(ws), workspace_bytes=need, clip_reward=10.0, epsilon=1e-8)
        kw.update(over)
        return lib.RewardNormIO(**kw)

    fn = b"so100_learner_normalize_rewards: "
    norm = lambda T_=T, N_=N, **over: (lambda: L.so100_learner_normalize_rewards(learner.h, C.byref(io(**over)), T_, N_, stream))
    calls = [(norm(T_=0), fn + b"T must be >= 1, got 0"),
             (norm(N_=-2), fn + b"N must be >= 1, got -2"),
             (norm(state_dev=None), fn + b"rollout/state/reward/workspace pointers are required"),
             (norm(workspace_dev=None), fn + b"rollout/state/reward/workspace pointers are required"),
             (norm(clip_reward=0.0), fn + b"clip_reward must be > 0"),
             (norm(clip_reward=float("nan")), fn + b"clip_reward must be > 0"),
             (norm(epsilon=-1.0), fn + b"epsilon must be >= 0"),
             (norm(workspace_bytes=need - 8), fn + f"the workspace holds {need - 8} bytes, T = {T} and N = {N} need {need}".encode()),
             (lambda: L.so100_learner_normalize_rewards(learner.h, None, T, N, stream), fn + b"null argument"),
             (lambda: L.so100_learner_reward_norm_init(learner.h, None, N, stream), b"so100_learner_reward_norm_init: the state pointer is required"),
             (lambda: L.so100_learner_reward_norm_init(learner.h, p(st), 0, stream), b"so100_learner_reward_norm_init: N must be >= 1, got 0")]
    # the one call checks the normalisation's arguments with its own, before it enqueues anything
    P = learner.num_params
    f = dict(dtype=torch.float32, device=DEV)
    params = torch.zeros(P, **f); m, v = torch.zeros_like(params), torch.zeros_like(params)
    adv, ret, adv_stats, uout = torch.full((T, N), 5.0, **f), torch.zeros(T, N, **f), torch.zeros(2, **f), torch.zeros(15, **f)
    perm = torch.zeros(T * N, dtype=torch.int64, device=DEV); last_obs = torch.zeros(N, OD, **f)
    uio = lib.UpdateIO(rollout_dev=p(buf), last_obs_dev=p(last_obs), T=T, N=N, params_dev=p(params), adam_m_dev=p(m), adam_v_dev=p(v), adv_dev=p(adv), ret_dev=p(ret),
                       adv_stats_dev=p(adv_stats), perm_dev=p(perm), epochs=1, mb=64, adam_step0=0, shuffle_seed=1, out_dev=p(uout))
    upd = lambda **over: (lambda: L.so100_learner_update_r(learner.h, C.byref(uio), C.byref(io(**over)), stream))
    calls += [(upd(clip_reward=-1.0), b"so100_learner_update_r: clip_reward must be > 0"),
              (upd(state_dev=None), b"so100_learner_update_r: rollout/state/reward/workspace pointers are required"),
              (upd(workspace_bytes=8), f"so100_learner_update_r: the workspace holds 8 bytes, T = {T} and N = {N} need {need}".encode()),
              (upd(rollout_dev=p(ret)), b"so100_learner_update_r: the reward normalisation reads another chunk than the update")]
    keep = st.clone()
    for call, msg in calls:
        assert call() == -1, msg
        assert L.so100_last_error() == msg
        torch.cuda.synchronize()
        assert same_bits(st, keep) and out.unique().tolist() == [77.0] and adv.unique().tolist() == [5.0], msg
    assert L.so100_learner_update_r(learner.h, C.byref(uio), C.byref(io()), stream) == 0      # the handle still works
    torch.cuda.synchronize()
    assert not same_bits(st, keep) and torch.isfinite(adv).all() and torch.isfinite(out).all()
    learner.close()


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------------------
def test_cli_train_saves_and_reloads_the_state(tmp_path, monkeypatch, caplog):
    monkeypatch.chdir(tmp_path)
    d = tmp_path / "models" / "Env01-v1_PPO"
    from so100_mujoco_rl_amd import main as drv
    from click.testing import CliRunner
    caplog.set_level(logging.INFO, logger=drv.logger.name)
    args = ["train", "-e", "Env01-v1", "--envs", "64", "--iters", "2", "--learner", "fused", "--shuffle", "device", "--normalize-reward"]
    r = CliRunner().invoke(drv.cli, ["-a", "PPO"] + args, catch_exceptions=False)
    assert r.exit_code == 0
    lines = list(caplog.messages)
    assert any("Reward normalisation: on" in l for l in lines) and any("return_std" in l for l in lines), lines
    assert (d / "last_model.pt").is_file() and (d / "last_model.reward_norm.pt").is_file() and (d / "best_model.reward_norm.pt").is_file()
    sd = torch.load(d / "last_model.reward_norm.pt", weights_only=True)
    assert sd["returns"].shape == (64,) and sd["count"].item() == pytest.approx(1e-4 + 64 * 64 * 2, rel=1e-12) and sd["var"].item() > 0
    model = torch.load(d / "last_model.pt", weights_only=True)
    from so100_mujoco_rl_amd.ppo import ActorCritic
    assert list(model) == list(ActorCritic(15).state_dict())                   # the model file stays a plain state_dict
    caplog.clear()
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "-m", str(d / "last_model.pt")] + args, catch_exceptions=False)
    assert r.exit_code == 0
    assert any("reloaded the running state" in l for l in caplog.messages), caplog.messages
    sd2 = torch.load(d / "last_model.reward_norm.pt", weights_only=True)
    assert sd2["count"].item() == pytest.approx(1e-4 + 64 * 64 * 4, rel=1e-12)                           # the second run continued the first's count


def test_cli_train_with_the_torch_learner(tmp_path, monkeypatch, caplog):
    monkeypatch.chdir(tmp_path)
    from so100_mujoco_rl_amd import main as drv
    from click.testing import CliRunner
    caplog.set_level(logging.INFO, logger=drv.logger.name)
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "-e", "Env01-v1", "--envs", "64", "--iters", "2", "--learner", "torch", "--normalize-reward"],
                           catch_exceptions=False)
    assert r.exit_code == 0
    assert any("return_std" in l for l in caplog.messages)
    assert (tmp_path / "models" / "Env01-v1_PPO" / "last_model.reward_norm.pt").is_file()
