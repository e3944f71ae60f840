"""What the observation-normalisation tests share (test_obs_norm_cpu.py, test_gpu_obs_norm.py): the numpy fp64 reference of the section
"Observation normalisation" of include/so100_learn.h -- SB3's VecNormalize(norm_obs=True) over its RunningMeanStd and the fold into the first
layers, written from the header's text; it shares no line with csrc/ or ppo.py -- the calls into the host twin of csrc/so100_learn.hpp's
templates (tests/_learncheck/obsnormcheck.cpp in hostlibs.learncheck()), and the inputs and comparisons both modules use.

Tolerances (derived, not measured).  The reference sums with numpy's pairwise order, the code under test with blocks of 256, a fixed tree and
Chan's merge in two levels: fp64 sums in another order differ by about T N 2^-53 relative, so mean and var match to MOMENT_TOL = 1e-10
relative (the reward half's bound; 3e-11 at 262 144 rows); count is exact (both add the integer T N to the same double).  The fold's outputs
are fp64 values rounded once to fp32; two fp64 evaluations a few fp64 ulps apart round to the same float or to neighbours: 1 fp32 ulp.  For
b0' the two evaluations differ by about 1e-15 of the TERMS of the sum (|b0| + sum |W0' mean|); the inputs keep |mean|/std <= 5 and every
spread non-zero, so b0' stays within a few orders of its terms (it would have to cancel to 1e-8 of them to cost an ulp).  A dimension that
never varies makes inv_std 1e4 and the terms huge: that is the documentation's matter, not a tolerance's."""
import functools

import numpy as np

import hostlibs
from hostlibs import ptr
from reward_norm_support import ulp_distance              # noqa: F401  (the tests reach it through either module)

EPSILON = 1e-8
MOMENT_TOL = 1e-10
SHAPES = [(3, 1), (5, 67), (16, 134), (64, 300)]
OBS_DIMS = [15, 8]
FIRST = ("pi_w0", "pi_b0", "vf_w0", "vf_b0")          # the tensors the fold rewrites, in the twin's argument order

KNOWN_OBS = np.array([[[1.0, 10.0]], [[3.0, 14.0]]], np.float32)              # [T = 2][N = 1][obs_dim = 2]
KNOWN_STATE = np.array([1.99990000499975, 11.9994000299985, 1.00019998000149990, 4.00704928755362142, 2.0001])
KNOWN_INV_STD = np.array([0.999900019995251125, 0.499560000384105248])
KNOWN_W0, KNOWN_B0 = np.array([[0.5, -0.25]], np.float32), np.array([0.125], np.float32)
KNOWN_W0_FOLDED, KNOWN_B0_FOLDED = np.array([[0.499950009997625562, -0.124890000096026312]]), np.array([0.623755043404894375])


def fresh_state(od):
    """[2 od + 1] float64: mean 0, var 1, count 1e-4"""
    return np.concatenate([np.zeros(od), np.ones(od), [1e-4]])


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
def ref_update(obs, state):
    """obs [T, N, od] float32 (the chunk's observation columns); state [2 od + 1] float64 (not modified).  Returns the state after the chunk."""
    obs = np.asarray(obs, np.float32)
    od = obs.shape[-1]
    batch = obs.reshape(-1, od).astype(np.float64)
    mean, var, count = np.array(state[:od]), np.array(state[od:2 * od]), float(state[2 * od])
    batch_mean, batch_var, batch_count = batch.mean(axis=0), batch.var(axis=0), batch.shape[0]
    delta = batch_mean - mean
    total = count + batch_count
    new_mean = mean + delta * batch_count / total
    new_var = (var * count + batch_var * batch_count + delta * delta * count * batch_count / total) / total
    return np.concatenate([new_mean, new_var, [total]])


def ref_scale(state, epsilon=EPSILON):
    """(mean, inv_std) in float64"""
    od = (len(state) - 1) // 2
    return np.array(state[:od]), 1.0 / np.sqrt(np.array(state[od:2 * od]) + epsilon)


def ref_fold_layer(w0, b0, state, epsilon=EPSILON):
    """one first layer: (W0' float64, b0' float64) of W0 [H, od], b0 [H] (any float dtype)"""
    mean, inv_std = ref_scale(state, epsilon)
    wf = np.asarray(w0, np.float64) * inv_std[None, :]
    return wf, np.asarray(b0, np.float64) - wf @ mean


def ref_fold(tensors, state, epsilon=EPSILON):
    """tensors: {name: float32 array} of the 13 policy tensors.  Returns ({name: float32}, norm float32 [2 od]): the four first-layer tensors folded
    in float64 and rounded once, the other nine as they are"""
    out = {k: np.array(v, np.float32) for k, v in tensors.items()}
    for w, b in (("pi_w0", "pi_b0"), ("vf_w0", "vf_b0")):
        wf, bf = ref_fold_layer(tensors[w], tensors[b], state, epsilon)
        out[w], out[b] = wf.astype(np.float32), bf.astype(np.float32)
    mean, inv_std = ref_scale(state, epsilon)
    return out, np.concatenate([mean, inv_std]).astype(np.float32)


def ref_normalize(obs, state, epsilon=EPSILON):
    """the learner's load in fp32: (obs - (float) mean) * (float) inv_std, one subtraction and one multiplication"""
    mean, inv_std = ref_scale(state, epsilon)
    return (np.asarray(obs, np.float32) - mean.astype(np.float32)) * inv_std.astype(np.float32)


# ---- the host twin ------------------------------------------------------------------------------------------------------------------------------
def twin_update(obs, state):
    """ref_update's interface on the twin; the observations travel in the first od entries of rows of od + 10 floats, as in the packed chunk"""
    obs = np.asarray(obs, np.float32); od = obs.shape[-1]
    chunk = np.full((obs.shape[0] * obs.shape[1], od + 10), 1e30, np.float32)
    chunk[:, :od] = obs.reshape(-1, od)
    st = np.array(state, np.float64)
    hostlibs.learncheck().on_update(chunk.shape[0], od, od + 10, ptr(chunk), ptr(st))
    return st


def layout(od):
    """{name: (offset, shape)} and the length of the flat parameter block (metadata of the library: needs no GPU)"""
    from so100_mujoco_rl_amd import lib
    return lib.learner_layout(od)


def flatten(tensors, od):
    lay, P = layout(od)
    flat = np.zeros(P, np.float32)
    for k, (off, shape) in lay.items():
        flat[off:off + int(np.prod(shape))] = np.asarray(tensors[k], np.float32).reshape(-1)
    return flat


def unflatten(flat, od):
    lay, _ = layout(od)
    return {k: np.array(flat[off:off + int(np.prod(shape))], np.float32).reshape(shape) for k, (off, shape) in lay.items()}


def twin_fold(tensors, state, epsilon=EPSILON):
    """ref_fold's interface on the twin, through the flat block"""
    od = (len(state) - 1) // 2
    lay, P = layout(od)
    flat = flatten(tensors, od)
    folded, norm = np.full(P, 7.0, np.float32), np.full(2 * od, 7.0, np.float32)
    first = np.array([lay[k][0] for k in FIRST], np.int32)
    st = np.array(state, np.float64)
    hostlibs.learncheck().on_fold(od, P, ptr(first), ptr(st), epsilon, ptr(flat), ptr(folded), ptr(norm))
    return unflatten(folded, od), norm


def twin_normalize(obs, norm):
    obs = np.ascontiguousarray(obs, np.float32); od = obs.shape[-1]
    out = np.empty_like(obs)
    nm = np.ascontiguousarray(norm, np.float32)
    hostlibs.learncheck().on_normalize(obs.size // od, od, ptr(obs), ptr(nm), ptr(out))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def scales(od):
    """per observation dimension a spread and an offset, all distinct: spreads from 0.02 (cube coordinates) to 6 (joint velocities, pixel slots),
    offset/spread ratios from -5 to 5 (the fold's b0' then cancels up to that ratio), every spread non-zero"""
    i = np.arange(od)
    std = 0.02 * (300.0 ** (i / max(od - 1, 1)))
    ratio = 5.0 * np.cos(2.0 + 2.399963 * i)                                   # the golden angle: spread over [-5, 5] with no two alike
    return ratio * std, std


@functools.lru_cache(maxsize=None)
def make_obs(T, N, od, seed=0):
    """[T, N, od] float32, dimension i drawn from N(offset_i, std_i); read-only, shared between tests"""
    g = np.random.default_rng(4000 + 977 * seed + 31 * T + N + 7 * od)
    off, std = scales(od)
    obs = (off + std * g.standard_normal((T, N, od))).astype(np.float32)
    assert (obs.reshape(-1, od).max(0) > obs.reshape(-1, od).min(0)).all()     # every dimension varies (three rows suffice)
    obs.setflags(write=False)
    return obs


@functools.lru_cache(maxsize=None)
def reference(T, N, od, seed=0):
    """ref_update of make_obs(T, N, od, seed) from a fresh state, computed once"""
    st = ref_update(make_obs(T, N, od, seed), fresh_state(od))
    st.setflags(write=False)
    return st


def scale_observations(x, od):
    """N(0, 1) observations of a test chunk (learn_support.make_chunk) moved to the scales above; works on numpy arrays and torch tensors"""
    off, std = scales(od)
    if isinstance(x, np.ndarray):
        return (x * std.astype(np.float32) + off.astype(np.float32)).astype(np.float32)
    import torch
    return x * torch.from_numpy(std.astype(np.float32)).to(x.device) + torch.from_numpy(off.astype(np.float32)).to(x.device)


# ---- comparisons --------------------------------------------------------------------------------------------------------------------------------
def check_state(state, want, exact_count=True):
    """mean and var within MOMENT_TOL relative, count exact; returns the two largest relative errors.  exact_count=False, for two chunks against
    one of 2T: 1e-4 + TN + TN and 1e-4 + 2TN round differently, so the count is held to MOMENT_TOL there"""
    od = (len(want) - 1) // 2
    state, want = np.asarray(state, np.float64), np.asarray(want, np.float64)
    rel_mean = float(np.max(np.abs(state[:od] - want[:od]) / np.abs(want[:od])))
    rel_var = float(np.max(np.abs(state[od:2 * od] - want[od:2 * od]) / want[od:2 * od]))
    assert rel_mean <= MOMENT_TOL and rel_var <= MOMENT_TOL, (rel_mean, rel_var)
    assert state[2 * od] == want[2 * od] if exact_count else abs(state[2 * od] - want[2 * od]) <= MOMENT_TOL * want[2 * od]
    return rel_mean, rel_var


def check_fold(got, got_norm, tensors, state, epsilon=EPSILON):
    """the fold's outputs against the reference: the four folded tensors and the norm pair within 1 fp32 ulp, the nine others copied exactly;
    returns the largest ulp distance seen"""
    want, want_norm = ref_fold(tensors, state, epsilon)
    worst = 0
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32, k
        if k in FIRST:
            u = ulp_distance(got[k], want[k])
            assert u <= 1, (k, u)
            worst = max(worst, u)
        else:
            assert np.array_equal(got[k].view(np.int32), np.asarray(tensors[k], np.float32).view(np.int32)), k
    u = ulp_distance(got_norm, want_norm)
    assert u <= 1, ("norm", u)
    return max(worst, u)


def policy_tensors(od, seed=None):
    """{name: float32 numpy array} of learn_support.state_dict(od), keyed by the library's tensor names"""
    import learn_support as LS
    from so100_mujoco_rl_amd import lib
    sd = LS.state_dict(od) if seed is None else LS.make_state_dict(od, seed)
    return {k: sd[lib.SB3_STATE_DICT_KEYS[k]].detach().cpu().numpy().astype(np.float32) for k in lib.POLICY_TENSORS}
