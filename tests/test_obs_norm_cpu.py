"""Observation normalisation without a GPU (include/so100_learn.h "Observation normalisation"): the numpy reference against the header's known
answer, the host twin of csrc/so100_learn.hpp against the reference (moments, chunk splitting, fold, load), the PyTorch learner against a
plain learner fed pre-normalised chunks (to the bit), the state's round trip, the command line and the export.

Tolerances: obs_norm_support.py (derived there).  The export's bound is three times the error measured against an fp64 evaluation (see the test)."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import hostlibs
import learn_support as LS
import obs_norm_support as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the reference's known answer ----------------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_known_answer():
    st = OS.ref_update(OS.KNOWN_OBS, OS.fresh_state(2))
    assert np.allclose(st, OS.KNOWN_STATE, rtol=1e-14, atol=0.0) and st[4] == 2.0001
    mean, inv_std = OS.ref_scale(st)
    assert np.allclose(inv_std, OS.KNOWN_INV_STD, rtol=1e-14, atol=0.0)
    wf, bf = OS.ref_fold_layer(OS.KNOWN_W0, OS.KNOWN_B0, st)
    assert np.allclose(wf, OS.KNOWN_W0_FOLDED, rtol=1e-14, atol=0.0) and np.allclose(bf, OS.KNOWN_B0_FOLDED, rtol=1e-14, atol=0.0)
    # the same, to the eight digits the feature's description quotes
    assert np.allclose(st[:4], [1.9999, 11.99940003, 1.00019998, 4.00704929], rtol=0, atol=5e-9)
    assert np.allclose(inv_std, [0.99990002, 0.49956], rtol=0, atol=5e-9)
    assert np.allclose(wf, [[0.49995001, -0.12489]], rtol=0, atol=5e-9) and np.allclose(bf, [0.62375504], rtol=0, atol=5e-9)
    # the header prints the same digits
    hdr = open(os.path.join(ROOT, "include", "so100_learn.h")).read()
    for v in (1.9999000049997500, 4.0070492875536214, 0.49956000038410525, 0.62375504340489438):
        assert f"{v:.17g}"[:14] in hdr, v
    # and the twin computes them
    assert np.allclose(OS.twin_update(OS.KNOWN_OBS, OS.fresh_state(2)), OS.KNOWN_STATE, rtol=1e-14, atol=0.0)


# ---- 2. the twin's moments against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", OS.OBS_DIMS)
@pytest.mark.parametrize("T,N", OS.SHAPES)
def test_twin_moments_match_the_reference(T, N, od):
    assert hostlibs.learncheck().on_block() == 256 and hostlibs.learncheck().on_group() == 64
    obs = OS.make_obs(T, N, od)
    got = OS.twin_update(obs, OS.fresh_state(od))
    rel = OS.check_state(got, OS.reference(T, N, od))
    print(f"[obsnorm] twin ({T}, {N}) od {od}: mean {rel[0]:.2e} var {rel[1]:.2e}")
    assert np.array_equal(OS.twin_update(obs, OS.fresh_state(od)), got)        # the same bits again


def test_twin_moments_over_several_groups():
    """more than 64 blocks (the second level of the merge) and a remainder in the last block: 20 000 rows = 78 full blocks and one of 32"""
    T, N, od = 50, 400, 8
    obs = OS.make_obs(T, N, od)
    OS.check_state(OS.twin_update(obs, OS.fresh_state(od)), OS.ref_update(obs, OS.fresh_state(od)))


# ---- 3. two chunks in a row are one chunk of 2T ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", OS.OBS_DIMS)
@pytest.mark.parametrize("T,N", OS.SHAPES)
def test_two_chunks_in_a_row_equal_one_of_twice_the_length(T, N, od):
    a, b = OS.make_obs(T, N, od), OS.make_obs(T, N, od, seed=2)
    both = np.concatenate([a, b])
    want = OS.ref_update(both, OS.fresh_state(od))
    two = OS.twin_update(b, OS.twin_update(a, OS.fresh_state(od)))
    OS.check_state(two, want, exact_count=False)
    OS.check_state(OS.twin_update(both, OS.fresh_state(od)), want)
    OS.check_state(two, OS.ref_update(b, OS.ref_update(a, OS.fresh_state(od))))                 # the same two steps on the reference: the count to the bit


# ---- 4. the fold and the load -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", OS.OBS_DIMS)
def test_twin_fold_matches_the_reference(od):
    tensors = OS.policy_tensors(od)
    state = OS.reference(64, 300, od)
    got, norm = OS.twin_fold(tensors, state)
    worst = OS.check_fold(got, norm, tensors, state)
    print(f"[obsnorm] twin fold od {od}: {worst} ulp")
    assert not np.array_equal(got["pi_w0"], tensors["pi_w0"]) and not np.array_equal(got["vf_b0"], tensors["vf_b0"])
    # a fresh state folds to almost the identity: inv_std = 1/sqrt(1 + 1e-8), mean 0
    got0, norm0 = OS.twin_fold(tensors, OS.fresh_state(od))
    OS.check_fold(got0, norm0, tensors, OS.fresh_state(od))
    assert np.array_equal(got0["pi_b0"], tensors["pi_b0"]) and np.array_equal(norm0[:od], np.zeros(od, np.float32))


@pytest.mark.parametrize("od", OS.OBS_DIMS)
def test_twin_load_is_one_subtraction_and_one_multiplication(od):
    obs = OS.make_obs(5, 67, od)
    state = OS.reference(5, 67, od)
    _, norm = OS.ref_fold(OS.policy_tensors(od), state)
    want = OS.ref_normalize(obs, state)
    assert np.array_equal(OS.twin_normalize(obs, norm).view(np.int32), want.view(np.int32))
    assert abs(want.reshape(-1, od).mean(0)).max() < 0.5 and abs(want.reshape(-1, od).std(0) - 1).max() < 0.2


# ---- 5. the PyTorch learner ---------------------------------------------------------------------------------------------------------------------
PT, PN, POD = 5, 67, 15


def raw_chunk(seed, T=PT, N=PN, od=POD):
    """learn_support.make_chunk with its observations (the chunk's, the terminal and the last ones) moved to obs_norm_support's scales"""
    buf, tobs, last_obs = LS.make_chunk(T, N, od, seed, LS.state_dict(od))
    buf = buf.clone()
    buf[..., :od] = OS.scale_observations(buf[..., :od], od)
    tobs = torch.where(tobs > 1e29, torch.zeros_like(tobs), OS.scale_observations(tobs, od))
    return buf, tobs, OS.scale_observations(last_obs, od)


def batch(buf, tobs, last_obs, od=POD, device="cpu"):
    """what RolloutCollector.collect(defer_bootstrap=True) hands a learner"""
    from so100_mujoco_rl_amd.rollout import RolloutChunk
    T, N = buf.shape[0], buf.shape[1]
    c = RolloutChunk(T, N, od, device); c.buf.copy_(buf)
    b = c.unpack(); b["last_obs"] = last_obs.to(device).clone(); b["terminal_obs"] = tobs.to(device).clone(); b["packed"] = c.buf
    return b


def normalised(buf, tobs, last_obs, state, od=POD):
    """the chunk with every observation normalised in fp32 under the reference's statistics"""
    nb = buf.clone()
    nb[..., :od] = torch.from_numpy(OS.ref_normalize(buf[..., :od].numpy(), state))
    return nb, torch.from_numpy(OS.ref_normalize(tobs.numpy(), state)), torch.from_numpy(OS.ref_normalize(last_obs.numpy(), state))


def make_ppo(**kw):
    from so100_mujoco_rl_amd.ppo import PPO
    p = PPO(POD, "cpu", epochs=2, minibatch=100, seed=5, **kw)
    p.net.load_state_dict(LS.state_dict(POD))
    return p


def test_ppo_trains_on_the_reference_normalised_observations_to_the_bit():
    chunks = [raw_chunk(1), raw_chunk(2)]
    assert (chunks[0][0][..., POD + 7] == 2).any()
    learner, plain = make_ppo(normalize_obs=True), make_ppo()
    state = OS.fresh_state(POD)
    for k, (buf, tobs, last_obs) in enumerate(chunks):
        b = batch(buf, tobs, last_obs)
        torch.manual_seed(31 + k)
        stats = learner.update(b)
        assert torch.equal(b["packed"], buf)                                   # the chunk keeps the raw observations
        torch.manual_seed(31 + k)
        plain_stats = plain.update(batch(*normalised(buf, tobs, last_obs, state)))
        assert torch.equal(learner._s["obs"], plain._s["obs"]) and torch.equal(learner._s["rewards"], plain._s["rewards"])
        for key, v in plain.net.state_dict().items():
            assert torch.equal(learner.net.state_dict()[key], v), (k, key)
        assert stats["value_loss"] == plain_stats["value_loss"] and stats["explained_variance"] == plain_stats["explained_variance"]
        state = OS.ref_update(buf[..., :POD].numpy(), state)                   # the statistics the next chunk is read under
        sd = learner.obs_norm_state()
        OS.check_state(np.concatenate([sd["mean"].numpy(), sd["var"].numpy(), [sd["count"].item()]]), state)
    assert max(float((v - LS.state_dict(POD)[k]).abs().max()) for k, v in plain.net.state_dict().items()) > 1e-3
    # the folded policy on raw observations is the trained policy on normalised ones
    buf, _, _ = chunks[1]
    folded = LS.RefNet(POD, learner.policy_state_dict())
    net = LS.RefNet(POD, learner.net.state_dict())
    raw = buf[..., :POD].reshape(-1, POD)
    mean, inv_std = OS.ref_scale(state)
    with torch.no_grad():
        want = net.mean_action((raw.double() - torch.from_numpy(mean)) * torch.from_numpy(inv_std))
        got = folded.mean_action(raw.double())
    assert float((got - want).abs().max()) < 1e-5                              # fp32 rounding of the folded weights, evaluated in fp64


# ---- 6. state, options, command line ----------------------------------------------------------------------------------------------------------
def test_state_round_trips_and_the_option_is_off_by_default():
    from so100_mujoco_rl_amd import lib
    from so100_mujoco_rl_amd.ppo import PPO, FusedPPO
    a = make_ppo(normalize_obs=True)
    fresh = a.obs_norm_state()
    assert set(fresh) == {"mean", "var", "count"} and all(v.dtype == torch.float64 for v in fresh.values())
    assert fresh["mean"].tolist() == [0.0] * POD and fresh["var"].tolist() == [1.0] * POD and fresh["count"].item() == 1e-4
    b1, b2 = batch(*raw_chunk(1)), batch(*raw_chunk(2))
    a.update(b1)
    sd = a.obs_norm_state()
    c = make_ppo(normalize_obs=True)
    c.net.load_state_dict(a.net.state_dict()); c.opt.load_state_dict(copy.deepcopy(a.opt.state_dict()))      # (a shallow copy would share Adam's moments)
    c.load_obs_norm_state({k: v.clone() for k, v in sd.items()})
    assert all(torch.equal(c.obs_norm_state()[k], sd[k]) for k in sd)
    torch.manual_seed(3); a.update(b2)
    torch.manual_seed(3); c.update(b2)
    assert all(torch.equal(a.obs_norm_state()[k], c.obs_norm_state()[k]) for k in sd)
    assert all(torch.equal(v, c.net.state_dict()[k]) for k, v in a.net.state_dict().items())
    with pytest.raises(ValueError, match="dimensions"):
        c.load_obs_norm_state({"mean": torch.zeros(8), "var": torch.ones(8), "count": torch.tensor(1.0)})
    # off: policy_state_dict() is net.state_dict() itself, for both learners
    for cls in (PPO, FusedPPO):
        off = cls(POD, "cpu")
        assert off.normalize_obs is False
        psd, nsd = off.policy_state_dict(), off.net.state_dict()
        assert list(psd) == list(nsd) and all(psd[k].data_ptr() == nsd[k].data_ptr() for k in nsd)
    on = make_ppo(normalize_obs=True)
    on.load_obs_norm_state(sd)
    psd = on.policy_state_dict()
    assert list(psd) == list(on.net.state_dict())
    changed = {k for k in psd if not torch.equal(psd[k], on.net.state_dict()[k])}
    assert changed == {f"mlp_extractor.{t}.0.{w}" for t in ("policy_net", "value_net") for w in ("weight", "bias")}
    f = FusedPPO(POD, "cpu", normalize_obs=True)
    assert f.normalize_obs is True and f.obs_norm_state()["count"].item() == 1e-4
    with pytest.raises(lib.So100Error, match="no CPU fallback"):
        f.update(b1)


def test_struct_and_exports_match_the_header():
    from so100_mujoco_rl_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "so100_learn.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} so100_obs_norm_io;", src).group(1)
    names = []
    for decl in body.split(";"):
        names += [w.strip(" *") for w in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip(), count=1).split(",") if w.strip()]
    assert names == [f[0] for f in lib.ObsNormIO._fields_] and C.sizeof(lib.ObsNormIO) == 4 * 8
    new = ["so100_learner_obs_norm_init", "so100_learner_obs_norm_workspace", "so100_learner_obs_norm_update", "so100_learner_obs_norm_fold",
           "so100_learner_set_obs_norm"]
    assert all(n in lib.LEARN_EXPORTS and re.search(r"\b%s\(" % n, src) for n in new)
    assert re.search(r"#define SO100_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "so100_sim.h")).read())      # additive
    L = lib.load()
    calls = [(lambda: L.so100_learner_obs_norm_init(None, None, None), b"so100_learner_obs_norm_init: null argument"),
             (lambda: L.so100_learner_obs_norm_update(None, C.byref(lib.ObsNormIO()), 1, 1, None), b"so100_learner_obs_norm_update: null argument"),
             (lambda: L.so100_learner_obs_norm_fold(None, None, 1e-8, None, None, None, None), b"so100_learner_obs_norm_fold: null argument"),
             (lambda: L.so100_learner_set_obs_norm(None, None), b"so100_learner_set_obs_norm: null argument"),
             (lambda: L.so100_learner_obs_norm_workspace(0, 5), b"so100_learner_obs_norm_workspace: T and N must be >= 1, got 0 and 5"),
             (lambda: L.so100_learner_obs_norm_workspace(4097, 4096), b"so100_learner_obs_norm_workspace: T*N must be <= 16777216, got 16781312")]
    for call, msg in calls:
        assert call() == -1, msg
        assert L.so100_last_error() == msg
    block, group = hostlibs.learncheck().on_block(), hostlibs.learncheck().on_group()
    for T, N in ((1, 1), (64, 4096), (5, 67), (4096, 4096)):                   # [blocks][15] (mean, M2) pairs, then [groups][15] (n, mean, M2) triples, fp64
        blocks = -(-T * N // block)
        assert L.so100_learner_obs_norm_workspace(T, N) == 8 * 15 * (2 * blocks + 3 * -(-blocks // group))
        assert lib.So100Learner.obs_norm_workspace_bytes(T, N) == L.so100_learner_obs_norm_workspace(T, N)


def test_cli_lists_the_flag_and_keeps_it_to_ppo_on_one_gpu(tmp_path, monkeypatch):
    from so100_mujoco_rl_amd import main as drv
    monkeypatch.chdir(tmp_path)
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "--help"])
    assert r.exit_code == 0 and "--normalize-obs" in r.output
    r = CliRunner().invoke(drv.cli, ["-a", "DDPG", "train", "-e", "Env01-v1", "--normalize-obs"])
    assert r.exit_code != 0 and isinstance(r.exception, RuntimeError) and "PPO" in str(r.exception) and "--normalize-obs" in str(r.exception)
    monkeypatch.setenv("WORLD_SIZE", "2")
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "train", "-e", "Env01-v1", "--normalize-obs"])
    assert r.exit_code != 0 and isinstance(r.exception, RuntimeError) and "one GPU" in str(r.exception) and "--normalize-obs" in str(r.exception)


def test_model_loader_folds_the_side_file_and_runs_the_raw_policy_without_it(tmp_path):
    from so100_mujoco_rl_amd import main as drv
    from so100_mujoco_rl_amd.ppo import fold_obs_norm
    od = 8
    sd = LS.state_dict(od)
    st = OS.reference(5, 67, od)
    side = {"mean": torch.from_numpy(st[:od].copy()), "var": torch.from_numpy(st[od:2 * od].copy()), "count": torch.tensor(st[2 * od])}
    path = str(tmp_path / "best_model.pt")
    torch.save(sd, path); torch.save(side, drv._obs_norm_path(path))
    assert drv._obs_norm_path(path) == str(tmp_path / "best_model.obs_norm.pt")
    net = drv._load_native(path, od, "cpu")
    want = fold_obs_norm(sd, side)
    assert all(torch.equal(v, want[k]) for k, v in net.state_dict().items())
    from so100_mujoco_rl_amd import lib
    got = {k: want[key].numpy() for k, key in lib.SB3_STATE_DICT_KEYS.items()}
    OS.check_fold(got, np.concatenate([st[:od], OS.ref_scale(st)[1]]).astype(np.float32), OS.policy_tensors(od), st)     # ppo.fold_obs_norm is the header's fold
    os.remove(drv._obs_norm_path(path))
    net = drv._load_native(path, od, "cpu")
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())


def test_saving_with_the_option_off_removes_a_side_file_left_by_an_earlier_run(tmp_path, caplog):
    """every run saves into the same directory: a run with the option followed by one without must not leave the first run's statistics beside
    the second run's raw model, or `test` / `record` would fold them into it"""
    import logging
    from so100_mujoco_rl_amd import main as drv
    caplog.set_level(logging.INFO, logger=drv.logger.name)
    path = str(tmp_path / "best_model.pt")
    on = make_ppo(normalize_obs=True)
    on.update(batch(*raw_chunk(1)))
    drv._save_model(on, path)
    assert os.path.isfile(drv._obs_norm_path(path))
    folded = drv._load_native(path, POD, "cpu").state_dict()
    assert not torch.equal(folded["mlp_extractor.policy_net.0.weight"], on.net.state_dict()["mlp_extractor.policy_net.0.weight"])
    off = make_ppo()
    drv._save_model(off, path)                                                 # the same path, the option off
    assert not os.path.exists(drv._obs_norm_path(path)) and any("removed" in m for m in caplog.messages)
    net = drv._load_native(path, POD, "cpu")
    assert all(torch.equal(v, off.net.state_dict()[k]) for k, v in net.state_dict().items())      # the raw policy, as it was trained
    drv._save_model(off, path)                                                 # nothing to remove: nothing happens
    drv._save_model(on, path)
    assert os.path.isfile(drv._obs_norm_path(path))


# ---- 7. the export ------------------------------------------------------------------------------------------------------------------------------
# The exported module runs the FOLDED first layer on raw observations in fp32, DeterministicPolicy the plain one on observations normalised in
# fp32.  Both are held to an fp64 evaluation of the normalised network.  Measured maximum of |action - fp64 action| over the 335 rows of the
# (5, 67) chunk (this file, CPU): folded 6.33e-7 (obs_dim 15), 4.47e-7 (obs_dim 8); normalised beforehand 4.31e-7 / 6.26e-7.  The fold's
# first layer adds W0' x and b0', each up to |mean|/std (here 5) times larger than their sum; at these ratios that costs no more than the fp32
# normalisation itself does.  Bound: three times the largest of the four.
EXPORT_TOL = 3 * 6.33e-7


@pytest.mark.parametrize("od", OS.OBS_DIMS)
def test_exported_policy_takes_raw_observations(od, tmp_path):
    from so100_mujoco_rl_amd.export import DeterministicPolicy, export_policy
    sd = LS.state_dict(od)
    st = OS.reference(5, 67, od)
    side = {"mean": torch.from_numpy(st[:od].copy()), "var": torch.from_numpy(st[od:2 * od].copy()), "count": torch.tensor(st[2 * od])}
    raw = torch.from_numpy(OS.make_obs(5, 67, od).reshape(-1, od).copy())
    scripted = export_policy(sd, str(tmp_path / "policy.pt"), obs_norm=side)
    plain = export_policy(sd, str(tmp_path / "plain.pt"))
    assert isinstance(plain.original_name, str) and DeterministicPolicy(od) is not None
    mean, inv_std = OS.ref_scale(st)
    with torch.no_grad():
        want = LS.RefNet(od, sd).mean_action((raw.double() - torch.from_numpy(mean)) * torch.from_numpy(inv_std)).clamp(-1, 1)
        got = torch.jit.load(str(tmp_path / "policy.pt"))(raw)
        pre = plain(torch.from_numpy(OS.ref_normalize(raw.numpy(), st)))
    e_fold, e_pre = float((got.double() - want).abs().max()), float((pre.double() - want).abs().max())
    print(f"[obsnorm] export od {od}: folded on raw {e_fold:.2e}, plain on normalised {e_pre:.2e}")
    assert e_fold <= EXPORT_TOL and e_pre <= EXPORT_TOL
    assert float((got - pre).abs().max()) <= 2 * EXPORT_TOL
    with torch.no_grad():
        assert float((plain(raw) - pre).abs().max()) > 1e-3                    # the unfolded export on raw observations is another policy
