"""What the reward-normalisation tests share (test_reward_norm_cpu.py, test_gpu_reward_norm.py): the numpy fp64 reference of the section
"Reward normalisation" of include/so100_learn.h -- SB3's VecNormalize(norm_reward=True) over its RunningMeanStd, written from the header's
text; it shares no line with csrc/ or ppo.py -- the calls into the host twin of csrc/so100_learn.hpp's templates
(tests/_learncheck/rewnormcheck.cpp in hostlibs.learncheck()), and the inputs and comparisons both modules use.

Tolerances (derived, not measured).  The reference sums with numpy's pairwise order, the code under test with blocks of 64, a fixed tree
and Chan's merge: in fp64 the two differ by about N 2^-53 relative, far below half an fp32 ulp, so an output differs from the reference's
only where the fp64 value sits on an fp32 rounding boundary: every output is within 1 fp32 ulp.  mean and var match to 1e-10 relative
(the linear worst case T N 2^-53 is 3e-11 at 262 144 entries).  count and the final return of an env whose episode ended on the chunk's last
step (0) are exact."""
import functools

import numpy as np

import hostlibs
from hostlibs import ptr

EPSILON, CLIP = 1e-8, 10.0
GAMMA = float(np.float32(0.99))                       # the learner's gamma is a float: widened from it
MOMENT_TOL = 1e-10
SHAPES = [(3, 1), (5, 67), (64, 300)]

KNOWN_REWARDS = np.array([[1.0, 3.0], [2.0, -1.0]], np.float32)
KNOWN_CODES = np.array([[0.0, 1.0], [0.0, 0.0]], np.float32)
KNOWN_OUT = np.array([[0.99990004301, 2.99970006943], [1.20768642426, -0.60384321213]])
KNOWN_RETURNS = [np.array([1.0, 0.0]), np.array([2.99, -1.0])]
KNOWN_MOMENTS = [(1.9999000049997497, 1.0001999800015, 2.0001), (1.497462563435914, 2.7425312479735195, 4.0001)]


def fresh_state(n):
    """[3 + n] float64: mean 0, var 1, count 1e-4, n zero returns"""
    st = np.zeros(3 + n)
    st[1], st[2] = 1.0, 1e-4
    return st


def ref_normalize(rewards, codes, state, gamma=GAMMA, epsilon=EPSILON, clip=CLIP):
    """rewards, codes [T, N] float32; state [3 + N] float64 (not modified).  Returns (out [T, N] float32, the state after the chunk)."""
    rewards = np.asarray(rewards, np.float32); codes = np.asarray(codes)
    T, N = rewards.shape
    mean, var, count = (float(x) for x in state[:3])
    ret = np.array(state[3:], np.float64)
    out = np.empty((T, N), np.float32)
    for t in range(T):
        r = rewards[t].astype(np.float64)
        ret = ret * gamma + r
        batch_mean, batch_var, batch_count = ret.mean(), ret.var(), N
        delta = batch_mean - mean
        total = count + batch_count
        new_mean = mean + delta * batch_count / total
        m2 = var * count + batch_var * batch_count + delta * delta * count * batch_count / total
        mean, var, count = new_mean, m2 / total, total
        out[t] = np.clip(r / np.sqrt(var + epsilon), -clip, clip).astype(np.float32)
        ret[codes[t] != 0] = 0.0
    return out, np.concatenate([[mean, var, count], ret])


def twin_normalize(rewards, codes, state, gamma=GAMMA, epsilon=EPSILON, clip=CLIP):
    """ref_normalize's interface on the twin; the two columns travel in rows of 5 floats, as columns 3 and 4 (a stride, as in the packed chunk)"""
    rewards = np.asarray(rewards, np.float32); T, N = rewards.shape
    chunk = np.full((T, N, 5), 1e30, np.float32)
    chunk[..., 3] = rewards; chunk[..., 4] = codes
    st = np.array(state, np.float64)
    out = np.empty((T, N), np.float32)
    hostlibs.learncheck().rn_normalize(T, N, 5, 3, 4, ptr(chunk), gamma, epsilon, clip, ptr(st), ptr(out))
    return out, st


@functools.lru_cache(maxsize=None)
def make_inputs(T, N, seed=0):
    """rewards 5 + 3 N(0, 1) as float32, done codes 0 / 1 / 2 with about 20 % ends; read-only arrays, shared between tests"""
    g = np.random.default_rng(9000 + 1013 * seed + 31 * T + N)
    rewards = (5.0 + 3.0 * g.standard_normal((T, N))).astype(np.float32)
    codes = g.choice([0.0, 1.0, 2.0], size=(T, N), p=[0.8, 0.1, 0.1]).astype(np.float32)
    rewards.setflags(write=False); codes.setflags(write=False)
    return rewards, codes


@functools.lru_cache(maxsize=None)
def reference(T, N, seed=0):
    """ref_normalize of make_inputs(T, N, seed) from a fresh state, computed once"""
    rewards, codes = make_inputs(T, N, seed)
    out, st = ref_normalize(rewards, codes, fresh_state(N))
    out.setflags(write=False); st.setflags(write=False)
    return out, st


def ulp_distance(a, b):
    """the largest distance in fp32 units in the last place between two float32 arrays of finite values"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


def check_against_reference(out, state, want_out, want_state, codes):
    """the module docstring's tolerances; returns the figures"""
    ulps = ulp_distance(out, want_out)
    rel = [abs(state[i] - want_state[i]) / max(abs(want_state[i]), 1e-300) for i in (0, 1)]
    assert ulps <= 1, ulps
    assert rel[0] <= MOMENT_TOL and rel[1] <= MOMENT_TOL, rel
    assert state[2] == want_state[2]
    ended = np.asarray(codes)[-1] != 0
    assert np.array_equal(state[3:][ended], np.zeros(int(ended.sum())))
    assert np.allclose(state[3:], want_state[3:], rtol=MOMENT_TOL, atol=0.0)
    return ulps, rel
