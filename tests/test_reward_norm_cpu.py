"""Reward normalisation (SB3 VecNormalize's reward half; include/so100_learn.h "Reward normalisation") without a device: the numpy reference
of reward_norm_support.py against the header's known answer, the host twin of csrc/so100_learn.hpp's templates against that reference, the
PyTorch learner's own implementation, the option checks, the additive C ABI and the command line.  CPU only.  Tolerances: the support file."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import hostlibs
import learn_support as LS
import reward_norm_support as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_known_answer():
    """gamma 0.99, N = 2: pins the order of update, normalise and reset (the variance of step t includes step t; the return is reset after it)"""
    st = RS.fresh_state(2)
    for t in range(2):
        out, st = RS.ref_normalize(RS.KNOWN_REWARDS[t:t + 1], RS.KNOWN_CODES[t:t + 1], st, gamma=0.99)
        assert np.array_equal(out[0], RS.KNOWN_OUT[t].astype(np.float32))
        assert np.allclose(st[3:], RS.KNOWN_RETURNS[t], rtol=1e-15, atol=0.0)
        assert np.allclose(st[:3], RS.KNOWN_MOMENTS[t], rtol=1e-15, atol=0.0)
    whole, st2 = RS.ref_normalize(RS.KNOWN_REWARDS, RS.KNOWN_CODES, RS.fresh_state(2), gamma=0.99)
    assert np.array_equal(whole, RS.KNOWN_OUT.astype(np.float32)) and np.array_equal(st2, st)


@pytest.mark.parametrize("normalize", [RS.ref_normalize, RS.twin_normalize], ids=["reference", "twin"])
def test_one_env_clips_at_plus_ten(normalize):
    """N = 1: the batch variance is 0, the first step's running variance collapses towards 1e-4/1.0001, and 5/sqrt(that) = 500 clips"""
    out, st = normalize(np.array([[5.0], [-7.0], [0.001]], np.float32), np.zeros((3, 1), np.float32), RS.fresh_state(1))
    assert out[0, 0] == np.float32(10.0) and -10.0 < out[1, 0] < 0.0 < out[2, 0] < 10.0      # from the second step on the mean has moved: var is of order R^2
    assert st[2] == 1e-4 + 1 + 1 + 1
    out, _ = normalize(np.array([[-5.0]], np.float32), np.zeros((1, 1), np.float32), RS.fresh_state(1))
    assert out[0, 0] == np.float32(-10.0)


# ---- 2. the twin ----------------------------------------------------------------------------------------------------------------------------------
def test_twin_reproduces_the_known_answer():
    out, st = RS.twin_normalize(RS.KNOWN_REWARDS, RS.KNOWN_CODES, RS.fresh_state(2), gamma=0.99)
    assert RS.ulp_distance(out, RS.KNOWN_OUT.astype(np.float32)) <= 1
    assert np.allclose(st[:3], RS.KNOWN_MOMENTS[1], rtol=RS.MOMENT_TOL, atol=0.0) and np.allclose(st[3:], RS.KNOWN_RETURNS[1], rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("T,N", RS.SHAPES)
def test_twin_equals_the_reference(T, N):
    rewards, codes = RS.make_inputs(T, N)
    assert 0.1 < (codes != 0).mean() < 0.3 or T * N < 50
    want_out, want_st = RS.reference(T, N)
    out, st = RS.twin_normalize(rewards, codes, RS.fresh_state(N))
    ulps, rel = RS.check_against_reference(out, st, want_out, want_st, codes)
    print(f"[rewnorm] twin ({T}, {N}): {ulps} ulp, mean {rel[0]:.2e}, var {rel[1]:.2e}")


@pytest.mark.parametrize("T,N", RS.SHAPES)
def test_two_chunks_chained_equal_one_of_double_length(T, N):
    """the state carries over; the twin's order of sums does not depend on T, so the chained run has the same bits"""
    ra, ca = RS.make_inputs(T, N, seed=1)
    rb, cb = RS.make_inputs(T, N, seed=2)
    rewards, codes = np.concatenate([ra, rb]), np.concatenate([ca, cb])
    for normalize in (RS.ref_normalize, RS.twin_normalize):
        whole, st = normalize(rewards, codes, RS.fresh_state(N))
        first, st1 = normalize(ra, ca, RS.fresh_state(N))
        second, st2 = normalize(rb, cb, st1)
        assert np.array_equal(np.concatenate([first, second]).view(np.int32), whole.view(np.int32))
        assert np.array_equal(st2.view(np.int64), st.view(np.int64))
    want, want_st = RS.ref_normalize(rewards, codes, RS.fresh_state(N))
    RS.check_against_reference(whole, st, want, want_st, codes)


# ---- 3. the PyTorch learner -----------------------------------------------------------------------------------------------------------------------
OD, PT, PN = 15, 6, 130


def ppo_batch(seed, with_tobs=True, N=PN):
    """a [6, 130] chunk as the collector hands it over, rewards 5 + 3 x make_chunk's N(0, 1); its terminal observations hold 1e30 off the
    code-2 steps, which a dense value pass would turn into NaN-free but huge numbers: zero them, as the collector's buffer holds finite rows"""
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    buf, tobs, last_obs = LS.make_chunk(PT, N, OD, seed, LS.state_dict(OD))
    buf = buf.clone(); buf[..., OD + 6] = 5.0 + 3.0 * buf[..., OD + 6]
    c = RolloutChunk(PT, N, OD, "cpu"); c.buf.copy_(buf)
    b = c.unpack(); b["last_obs"] = last_obs; b["packed"] = c.buf
    if with_tobs:
        b["terminal_obs"] = torch.where(tobs > 1e29, torch.zeros_like(tobs), tobs)
    return b


def make_ppo(**kw):
    from so100_mujoco_rl_amd.ppo import PPO
    p = PPO(OD, "cpu", epochs=2, minibatch=300, seed=5, **kw)
    p.net.load_state_dict(LS.state_dict(OD))
    return p


def test_ppo_forms_the_reference_rewards_and_trains_on_them_to_the_bit():
    from so100_mujoco_rl_amd.rollout import bootstrap_truncated
    b = ppo_batch(1)
    rewards, codes = b["rewards"].numpy().copy(), b["packed"][..., OD + 7].numpy().copy()
    want, want_st = RS.ref_normalize(rewards, codes, RS.fresh_state(PN))
    assert (codes == 2).any() and (codes == 1).any()
    learner = make_ppo(normalize_reward=True)
    torch.manual_seed(31)
    stats = learner.update(b)
    assert np.array_equal(b["rewards"].numpy(), rewards)                       # the chunk keeps the env's rewards
    # the plain learner: the same chunk with the reference's rewards in the reward column and the bootstrap added to them with the same net
    plain = make_ppo()
    b2 = ppo_batch(1, with_tobs=False)
    b2["packed"][..., OD + 6] = torch.from_numpy(want)
    with torch.no_grad():
        bootstrap_truncated(b2["rewards"], b2["packed"][..., OD + 7], b["terminal_obs"], plain.net.value, 0.99)
    torch.manual_seed(31)
    plain_stats = plain.update(b2)
    assert torch.equal(learner._s["rewards"], plain._s["rewards"])             # (the learner's working copy: normalised, then bootstrapped)
    for k, v in plain.net.state_dict().items():
        assert torch.equal(learner.net.state_dict()[k], v), k
    assert max(float((v - LS.state_dict(OD)[k]).abs().max()) for k, v in plain.net.state_dict().items()) > 1e-3
    assert stats["value_loss"] == plain_stats["value_loss"] and stats["mean_reward"] == b["rewards"].mean().item() != plain_stats["mean_reward"]
    sd = learner.reward_norm_state()
    assert stats["return_var"] == sd["var"].item() and stats["return_count"] == sd["count"].item() == want_st[2]
    assert abs(sd["mean"].item() - want_st[0]) <= RS.MOMENT_TOL * abs(want_st[0]) and abs(sd["var"].item() - want_st[1]) <= RS.MOMENT_TOL * want_st[1]
    assert "return_var" not in plain_stats


def test_ppo_state_round_trips_and_a_restored_learner_continues_identically():
    b1, b2 = ppo_batch(1, with_tobs=False), ppo_batch(2, with_tobs=False)
    a = make_ppo(normalize_reward=True)
    fresh = a.reward_norm_state()
    assert fresh["returns"].numel() == 0 and [fresh[k].item() for k in ("mean", "var", "count")] == [0.0, 1.0, 1e-4]
    a.update(b1)
    sd = a.reward_norm_state()
    assert set(sd) == {"mean", "var", "count", "returns"} and sd["returns"].shape == (PN,) and all(v.dtype == torch.float64 for v in sd.values())
    c = make_ppo(normalize_reward=True)
    c.load_reward_norm_state({k: v.clone() for k, v in sd.items()})
    assert all(torch.equal(c.reward_norm_state()[k], sd[k]) for k in sd)
    a.update(b2); c.update(b2)
    assert torch.equal(a._s["rewards"], c._s["rewards"])
    assert all(torch.equal(a.reward_norm_state()[k], c.reward_norm_state()[k]) for k in sd)
    # ... and both continue as the reference does over the two chunks
    r = np.concatenate([b1["rewards"].numpy(), b2["rewards"].numpy()]); codes = np.concatenate([b1["packed"][..., OD + 7].numpy(), b2["packed"][..., OD + 7].numpy()])
    want, want_st = RS.ref_normalize(r, codes, RS.fresh_state(PN))
    assert RS.ulp_distance(a._s["rewards"].numpy(), want[PT:]) <= 1
    assert a.reward_norm_state()["count"].item() == want_st[2]
    c.load_reward_norm_state(fresh)                                            # a state saved before the first update restores a fresh one
    assert c.reward_norm_state()["returns"].numel() == 0
    with pytest.raises(ValueError, match="envs"):
        a.update(ppo_batch(1, with_tobs=False, N=7))                           # another env count than the state's


# ---- 4. options -----------------------------------------------------------------------------------------------------------------------------------
def test_option_validation_and_no_cpu_fallback():
    from so100_mujoco_rl_amd import lib
    from so100_mujoco_rl_amd.ppo import PPO, FusedPPO
    for cls in (PPO, FusedPPO):
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="clip_reward"):
                cls(OD, "cpu", normalize_reward=True, clip_reward=bad)
        off = cls(OD, "cpu")
        assert off.normalize_reward is False and off.clip_reward == 10.0
    f = FusedPPO(OD, "cpu", normalize_reward=True, clip_reward=5.0)
    assert f.normalize_reward is True and f.clip_reward == 5.0
    with pytest.raises(lib.So100Error, match="no CPU fallback"):
        f.update(ppo_batch(1))
    sd = f.reward_norm_state()
    assert sd["returns"].numel() == 0 and [sd[k].item() for k in ("mean", "var", "count")] == [0.0, 1.0, 1e-4]


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from so100_mujoco_rl_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    return lib.load()


def test_reward_norm_struct_matches_the_header():
    from so100_mujoco_rl_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "so100_learn.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} so100_reward_norm_io;", src).group(1)
    names = []
    for decl in body.split(";"):
        names += [w.strip(" *") for w in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip(), count=1).split(",") if w.strip()]
    assert names == [f[0] for f in lib.RewardNormIO._fields_]
    assert C.sizeof(lib.RewardNormIO) == 4 * 8 + 8 + 2 * 8                     # four pointers, one int64, two doubles
    new = ["so100_learner_reward_norm_workspace", "so100_learner_reward_norm_init", "so100_learner_normalize_rewards", "so100_learner_advantages_r",
           "so100_learner_update_r"]
    assert all(n in lib.LEARN_EXPORTS for n in new)
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive
    assert (lib.REWARD_NORM_EPSILON, lib.REWARD_NORM_CLIP, lib.REWARD_NORM_INIT) == (1e-8, 10.0, (0.0, 1.0, 1e-4))


def test_null_arguments_are_refused_without_a_device(L):
    from so100_mujoco_rl_amd import lib
    assert L.so100_abi_version() == 3
    calls = [(lambda: L.so100_learner_normalize_rewards(None, C.byref(lib.RewardNormIO()), 1, 1, None), b"so100_learner_normalize_rewards: null argument"),
             (lambda: L.so100_learner_reward_norm_init(None, None, 1, None), b"so100_learner_reward_norm_init: null argument"),
             (lambda: L.so100_learner_advantages_r(None, C.byref(lib.AdvantagesIO()), None, 1, 1, None), b"so100_learner_advantages_r: null argument"),
             (lambda: L.so100_learner_update_r(None, C.byref(lib.UpdateIO()), C.byref(lib.RewardNormIO()), None), b"so100_learner_update_r: null argument"),
             (lambda: L.so100_learner_update_r(None, None, None, None), b"so100_learner_update_r: null argument"),
             (lambda: L.so100_learner_reward_norm_workspace(0, 5), b"so100_learner_reward_norm_workspace: T and N must be >= 1, got 0 and 5"),
             (lambda: L.so100_learner_reward_norm_workspace(5, -1), b"so100_learner_reward_norm_workspace: T and N must be >= 1, got 5 and -1")]
    for call, msg in calls:
        assert call() == -1, msg
        assert L.so100_last_error() == msg
    block = hostlibs.learncheck().rn_block()
    assert block == 64
    for T, N in ((1, 1), (64, 4096), (5, 67)):                                 # [T][blocks] (mean, M2) pairs and T denominators, fp64
        assert L.so100_learner_reward_norm_workspace(T, N) == 8 * (T * -(-N // block) * 2 + T)
        assert lib.So100Learner.reward_norm_workspace_bytes(T, N) == L.so100_learner_reward_norm_workspace(T, N)


# ---- 6. the command line --------------------------------------------------------------------------------------------------------------------------
def test_cli_lists_the_flag_and_keeps_it_to_ppo(tmp_path, monkeypatch):
    from so100_mujoco_rl_amd import main as drv
    monkeypatch.chdir(tmp_path)
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "--help"])
    assert r.exit_code == 0 and "--normalize-reward" in r.output
    r = CliRunner().invoke(drv.cli, ["-a", "DDPG", "train", "-e", "Env01-v1", "--normalize-reward"])
    assert r.exit_code != 0 and isinstance(r.exception, RuntimeError) and "PPO" in str(r.exception) and "--normalize-reward" in str(r.exception)
    monkeypatch.setenv("WORLD_SIZE", "2")
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "-e", "Env01-v1", "--normalize-reward"])
    assert r.exit_code != 0 and isinstance(r.exception, RuntimeError) and "one GPU" in str(r.exception)
