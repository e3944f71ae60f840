"""The random numbers the kernels draw for themselves, against references that share nothing with them.  CPU only.

Three Philox4x32-10 implementations exist here: the device's philox4x32 (csrc/so100_task.hpp, compiled for the host in
tests/_hostcheck), the oracle's so100o_philox4x32 (C) and philox4x32_np (numpy uint64, written from the paper), on which the
reference sampler oracle.so100_oracle.policy_noise_ref stands.  All three must reproduce Random123's published known answers.
On top of that: the env's uniforms (draw8) bit for bit against so100o_uniform4, the counter layouts of the two streams (they cannot
overlap), the reference sampler as a standard normal sample, the edges of the Box-Muller transform, the device's fp32 transform
(policy_noise, host twin) over every value of u1 and a dense sweep of u2, and the fp32 task layer stepped WITHOUT injected uniforms
against the oracle for every env kind -- the CPU half of tests/test_gpu_policy_noise.py::test_uninjected_env_draws_vs_oracle."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import ndtr

from hostlibs import hostcheck, ptr
from oracle import so100_oracle as O
from scenes import UNINJECTED_CASES, UNINJECTED_N, UNINJECTED_SEED, UNINJECTED_STEPS, UNINJECTED_TIMELIMIT

u32 = lambda x: np.ascontiguousarray(x, np.uint32)


@pytest.fixture(scope="module")
def H():
    return hostcheck()


# ---- known answers ------------------------------------------------------------------------------------------------------------
# Random123 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), kat_vectors, philox4x32-10:
# counter / key -> output
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _philox_oracle(c, k):
    out = np.zeros(4, np.uint32)
    O.lib().so100o_philox4x32(*[C.c_uint32(x) for x in c], *[C.c_uint32(x) for x in k], ptr(out))
    return tuple(int(x) for x in out)


def _philox_numpy(c, k):
    return tuple(int(x) for x in O.philox4x32_np(*c, *k))


def _philox_device(H, c, k):
    out = np.zeros(4, np.uint32)
    H.hc_philox4x32(ptr(u32(c)), ptr(u32(k)), ptr(out))
    return tuple(int(x) for x in out)


@pytest.mark.parametrize("impl", ["oracle", "numpy", "device"])
def test_philox_known_answers(H, impl):
    """A multiplier or Weyl constant wrong in any one of them -- or in all of them alike -- fails here."""
    fn = {"oracle": _philox_oracle, "numpy": _philox_numpy, "device": lambda c, k: _philox_device(H, c, k)}[impl]
    for c, k, want in KAT:
        got = fn(c, k)
        assert got == want, (impl, [f"{x:08x}" for x in got], [f"{x:08x}" for x in want])


def test_philox_implementations_agree_on_random_and_edge_inputs(H):
    rs = np.random.RandomState(1)
    cases = rs.randint(0, 2**32, (200, 6), dtype=np.uint64)
    cases[:8, :4] = [[0, 0, 0, 0], [2**32 - 1] * 4, [2**31] * 4, [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [2**32 - 1, 0, 2**32 - 1, 0]]
    for row in cases:
        c = tuple(int(x) for x in row[:4]); k = tuple(int(x) for x in row[4:])
        assert _philox_numpy(c, k) == _philox_oracle(c, k) == _philox_device(H, c, k)
    # and the vectorised form of the numpy one is the scalar form
    vec = O.philox4x32_np(cases[:, 0], cases[:, 1], cases[:, 2], cases[:, 3], int(cases[0, 4]), int(cases[0, 5]))
    for i, row in enumerate(cases):
        assert tuple(int(x) for x in vec[i]) == _philox_numpy(tuple(int(x) for x in row[:4]), (int(cases[0, 4]), int(cases[0, 5])))


# ---- the two streams ----------------------------------------------------------------------------------------------------------
SEEDS = (0, 4, 0xDEADBEEF12345, 2**64 - 1)                     # two above 2^32: seed_hi is the second key word
EDGE_U32 = (0, 1, 1000, 2**31 - 1, 2**31, 2**32 - 1)


def test_draw8_is_the_oracles_uniform_stream(H):
    """The env's uniforms, device source on the host, bit for bit: against so100o_uniform4 (the oracle's stream) and against the counter
    layout written out -- counter (env_gid, counter, 2 phase + b, 0), key (seed_lo, seed_hi), u = (r >> 8) 2^-24 in float32."""
    L = O.lib()
    for seed in SEEDS:
        for env in EDGE_U32:
            for counter in EDGE_U32:
                for phase in (0, 1):
                    u = np.zeros(8, np.float32); H.hc_draw8(seed, env, counter, phase, ptr(u))
                    uo = np.zeros(8, np.float32)
                    L.so100o_uniform4(seed, env, counter, 2*phase, ptr(uo[:4])); L.so100o_uniform4(seed, env, counter, 2*phase + 1, ptr(uo[4:]))
                    assert np.array_equal(u, uo), (hex(seed), env, counter, phase)
                    r = np.concatenate([O.philox4x32_np(env, counter, 2*phase + b, 0, seed & 0xFFFFFFFF, seed >> 32) for b in (0, 1)])
                    want = ((r >> np.uint64(8)).astype(np.float64) * 2.0**-24).astype(np.float32)      # 24 bits: exact in float32
                    assert np.array_equal(u, want) and u.min() >= 0.0 and u.max() < 1.0


def test_policy_noise_keying_and_streams_do_not_overlap(H):
    """policy_noise (device source on the host) draws from counter (env_gid, step, 16 + b, 0x504F4C) under the same key: it follows the
    reference sampler, which is keyed so, at edge values of every counter word and of the seed -- and follows no other layout (words swapped,
    the env's c3 = 0, the env's c2).  With both layouts pinned, the streams are disjoint as sets of counters, for every env, step, counter and
    phase: Philox is a bijection of the counter for a fixed key, draw8 only forms c3 = 0 with c2 in {0, 1, 2, 3}, the policy only
    c3 = 0x504F4C with c2 in {16, 17}."""
    for seed in SEEDS:
        for env in EDGE_U32:
            for step in EDGE_U32:
                e = np.zeros(8, np.float32); H.hc_policy_noise(seed, env, step, ptr(e))
                ref = O.policy_noise_ref(seed, env, step)
                assert np.abs(e[:6] - ref).max() < HOST_TWIN_EPS, (hex(seed), env, step)
                if env != step:
                    assert np.abs(e[:6] - O.policy_noise_ref(seed, step, env)).max() > 1e-3          # (env, step) is not (step, env)
    # the layouts as sets: word 3 tells the streams apart whatever the other words are; word 2 does so as well
    draw8_c2 = {2*phase + b for phase in (0, 1) for b in (0, 1)}; draw8_c3 = {0}
    policy_c2 = {O.POLICY_STREAM_C2 + b for b in (0, 1)}; policy_c3 = {O.POLICY_STREAM_C3}
    assert not (draw8_c3 & policy_c3) and not (draw8_c2 & policy_c2)
    assert O.POLICY_STREAM_C3 == 0x504F4C and O.POLICY_STREAM_C2 == 16
    # a policy draw keyed like an env draw (c3 = 0) is a different sample: the reference would notice
    r_pol = O.philox4x32_np(7, 3, 16, O.POLICY_STREAM_C3, 4, 0); r_env = O.philox4x32_np(7, 3, 16, 0, 4, 0)
    assert not np.array_equal(r_pol, r_env)


# ---- the reference sampler is a standard normal sample ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [4, 6, 0xDEADBEEF12345])
def test_reference_sampler_is_standard_normal(seed):
    """64 steps x 4096 envs x 6 = 1 572 864 draws.  Every moment within 4 standard errors of its N(0, 1) value (independent draws), the
    Kolmogorov-Smirnov distance to Phi below the 1 % critical value 1.628 / sqrt(N)."""
    T, N = 64, 4096
    x = O.policy_noise_ref(seed, np.arange(N)[None, :], np.arange(T)[:, None])
    assert x.shape == (T, N, 6) and x.dtype == np.float64 and np.isfinite(x).all()
    n = x.size
    se = lambda var, m=n: 4.0*np.sqrt(var/m)
    flat = x.reshape(-1)
    mean, var = flat.mean(), (flat**2).mean()
    m3, m4 = (flat**3).mean(), (flat**4).mean()
    lag_env = (x[:, 1:]*x[:, :-1]).mean(); lag_step = (x[1:]*x[:-1]).mean(); lag_act = (x[..., 1:]*x[..., :-1]).mean()
    corr = np.corrcoef(x.reshape(-1, 6).T); off = np.abs(corr - np.eye(6)).max()
    s = np.sort(flat); cdf = ndtr(s); i = np.arange(n)
    ks = max(((i + 1)/n - cdf).max(), (cdf - i/n).max())
    print(f"[policy_noise_ref seed {seed:#x}] mean {mean:.2e} var-1 {var - 1:.2e} m3 {m3:.2e} m4-3 {m4 - 3:.2e} lag-1 env {lag_env:.2e} step {lag_step:.2e} "
          f"action {lag_act:.2e} max corr {off:.2e} KS {ks:.2e} max |eps| {np.abs(flat).max():.2f}")
    assert abs(mean) < se(1.0)                                # Var x = 1
    assert abs(var - 1) < se(2.0)                             # Var x^2 = 2
    assert abs(m3) < se(15.0)                                 # Var x^3 = 15
    assert abs(m4 - 3) < se(96.0)                             # Var x^4 = 105 - 9
    assert abs(lag_env) < se(1.0, T*(N - 1)*6) and abs(lag_step) < se(1.0, (T - 1)*N*6) and abs(lag_act) < se(1.0, T*N*5)
    assert off < se(1.0, T*N)                                 # each of the 15 entries: s.e. 1 / sqrt(T N)
    assert ks < 1.628/np.sqrt(n)
    assert np.abs(flat).max() <= np.sqrt(48*np.log(2.0))


# ---- the transform: edges, and the device's fp32 arithmetic --------------------------------------------------------------------
RAD_MAX = float(np.sqrt(48*np.log(2.0)))                       # sqrt(-2 ln 2^-24) = 5.768
# host twin of policy_noise (float32, g++ -ffp-contract=off, glibc logf) against box_muller_ref (float64), absolute:
HOST_TWIN_EPS = 6e-6                                           # measured 2.0e-6 (every u1 x hashed u2: 1.5e-6; every u2 at u1 = 2^-24 and 2^-23: 1.9e-6, 2.0e-6)
HOST_TWIN_RAD = 1.1e-6                                         # measured 3.5e-7: the radius alone (u2 = 1/2: angle 0, cos 1, sin 0), every u1


def _pairs(H, r_even, r_odd):
    r_even = u32(r_even); r_odd = u32(r_odd)
    e0 = np.empty(r_even.size, np.float32); e1 = np.empty(r_even.size, np.float32)
    H.hc_policy_noise_pairs(ptr(r_even), ptr(r_odd), r_even.size, ptr(e0), ptr(e1))
    return e0, e1


def test_box_muller_edges(H):
    """u1 = 2^-24 (largest radius) and 1 (radius exactly 0), u2 = 0 and 1 - 2^-24 (both ends of the angle): finite, |eps| <= sqrt(48 ln 2),
    in the reference and in the device's float32 code alike"""
    re = u32([0x00000000, 0x000000FF, 0xFFFFFF00, 0xFFFFFFFF]); ro = u32([0x00000000, 0x000000FF, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF])
    RE, RO = [a.reshape(-1) for a in np.meshgrid(re, ro, indexing="ij")]
    r0, r1 = O.box_muller_ref(RE, RO); e0, e1 = _pairs(H, RE, RO)
    for a in (r0, r1, e0, e1):
        assert np.isfinite(a).all() and np.abs(a).max() <= RAD_MAX*(1 + 1e-6)
    top = RE >= 0xFFFFFF00                                      # u1 = 1: rad = sqrt(-2 ln 1) = 0 exactly
    for a in (r0, r1, e0, e1):
        assert np.all(a[top] == 0.0)
    low = RE <= 0xFF                                            # u1 = 2^-24
    assert np.allclose(np.hypot(r0[low], r1[low]), RAD_MAX, rtol=1e-15) and np.abs(np.hypot(e0[low].astype(np.float64), e1[low].astype(np.float64)) - RAD_MAX).max() < HOST_TWIN_EPS
    # u2 = 0: angle -pi; u2 = 1/2: angle 0
    assert abs(r0[0] + RAD_MAX) < 1e-14 and abs(r1[0]) < 1e-14
    k = np.nonzero((RE == 0) & (RO == 0x80000000))[0][0]
    assert abs(r0[k] - RAD_MAX) < 1e-14 and r1[k] == 0.0 and e1[k] == 0.0
    assert np.abs(e0 - r0).max() < HOST_TWIN_EPS and np.abs(e1 - r1).max() < HOST_TWIN_EPS


def test_policy_noise_fp32_transform_vs_fp64(H):
    """The device's policy_noise arithmetic, compiled for the host, against the float64 reference: all 2^24 values of u1 (the radius), with
    u2 = 1/2 and with a u2 that hops over the whole circle, and all 2^24 values of u2 at the two largest radii and at a middling one."""
    k = np.arange(1 << 24, dtype=np.uint64)
    every = (k << np.uint64(8)).astype(np.uint32)              # the 24 bits that are used, low byte 0
    worst = {}

    def err(name, r_even, r_odd):
        e0, e1 = _pairs(H, r_even, r_odd); r0, r1 = O.box_muller_ref(r_even, r_odd)
        assert np.isfinite(e0).all() and np.isfinite(e1).all()
        worst[name] = max(float(np.abs(e0 - r0).max()), float(np.abs(e1 - r1).max()))
    err("radius", every, np.full(every.size, 0x80000000, np.uint32))
    err("u1 x hashed u2", every, ((k * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    for r_even in (0x00000000, 0x00000100, 0x80000000):
        err(f"u2 at r_even {r_even:08x}", np.full(every.size, r_even, np.uint32), every)
    print("[policy_noise host twin vs fp64] " + ", ".join(f"{n}: {v:.2e}" for n, v in worst.items()))
    assert worst.pop("radius") < HOST_TWIN_RAD
    assert max(worst.values()) < HOST_TWIN_EPS


def test_policy_noise_is_its_pair_transform_of_the_philox_words(H):
    """policy_noise == the pair transform of the reference Philox's words for (env, step): ties the sweep above to the sampler the kernels call"""
    rs = np.random.RandomState(3)
    for seed in SEEDS:
        for env, step in rs.randint(0, 2**32, (50, 2), dtype=np.uint64):
            e = np.zeros(8, np.float32); H.hc_policy_noise(seed, int(env), int(step), ptr(e))
            r = np.concatenate([O.philox4x32_np(env, step, 16 + b, 0x504F4C, seed & 0xFFFFFFFF, seed >> 32) for b in (0, 1)])
            e0, e1 = _pairs(H, r[0::2], r[1::2])
            assert np.array_equal(e[0::2], e0) and np.array_equal(e[1::2], e1)


# ---- the env's own draws, every kind, no injection -------------------------------------------------------------------------------
def uninjected_actions(kind, seed, n, steps):
    """the actions gpu_support.run_pair draws for (kind's action scale, seed): same generator, same consumption"""
    rs = np.random.RandomState(seed); rs.random_sample((n, 16))
    for _ in range(steps):
        a = np.clip(rs.uniform(-1, 1, (n, 6)) * UNINJECTED_CASES[kind][1], -1, 1).astype(np.float32); rs.random_sample((n, 16))
        yield a


@pytest.mark.parametrize("kind", [1, 2, 3, 4, 5, 6])
def test_uninjected_task_layer_fp32_vs_oracle(H, kind):
    """so100_task.hpp on the host in float32, drawing its own uniforms (draw8 keyed by seed and env id), against OracleEnv(kind, seed, env_id)
    drawing its own: reset pose and cube placement (Env01/02/06), cube targets (Env03/05), detection noise (Env05).  Bounds: those of the
    injected comparisons of the same kind (tests/test_gpu_parity.py)."""
    flags, _ = UNINJECTED_CASES[kind]
    seed, n, steps, tl = UNINJECTED_SEED, UNINJECTED_N, UNINJECTED_STEPS, UNINJECTED_TIMELIMIT
    reach = kind in (1, 2, 6); od = 15 if reach else 8
    orc = [O.OracleEnv(kind, flags=flags, iters=0, seed=seed, env_id=i) for i in range(n)]
    hs = [H.hc_env_new(kind) for _ in range(n)]
    for e in orc:
        e.e.max_episode_steps = tl
    for i in range(n):
        oh = np.zeros(od, np.float32); H.hc_env_reset(hs[i], kind, seed, i, None, ptr(oh))
        np.testing.assert_allclose(oh, orc[i].reset(), rtol=0, atol=1e-6)
    n_px = n_px_bad = resets = 0
    for t, a in enumerate(uninjected_actions(kind, seed, n, steps)):
        for i in range(n):
            oo, ro, to, tro, tobo = orc[i].step(a[i], autoreset=True)
            oh = np.zeros(od, np.float32); th = np.zeros(od, np.float32); rh = C.c_float(); dh = C.c_int(); trh = C.c_int()
            H.hc_env_step(hs[i], kind, flags, 4, 6, tl, seed, i, ptr(a[i]), None, ptr(oh), ptr(th), C.byref(rh), C.byref(dh), C.byref(trh))
            assert bool(dh.value) == (to or tro) and bool(trh.value) == (tro and not to), (kind, t, i)
            resets += int(to or tro)
            if reach:
                np.testing.assert_allclose(oh, oo, rtol=0, atol=2e-5, err_msg=f"kind {kind} step {t} env {i}")
                assert abs(rh.value - ro) < (2e-3 if kind == 6 else 1e-4)
            else:
                np.testing.assert_allclose(oh[:6], oo[:6], rtol=0, atol=1e-6)
                d = np.abs(oh[6:] - oo[6:]); n_px += d.size; n_px_bad += int((d > 1e-4).sum())
                assert d.max() < 6e-3, (kind, t, i, d.max())
                assert abs(rh.value - ro) < (1.2e-2 if kind == 4 else 2e-3)
    assert resets >= 2*n                                       # two auto-resets per env: three episodes' worth of reset draws
    assert n_px_bad <= 0.01*n_px, (n_px_bad, n_px)
    wq = wv = 0.0
    for i in range(n):
        q = np.zeros(13); v = np.zeros(12); H.hc_env_qpos(hs[i], ptr(q), ptr(v)); H.hc_env_free(hs[i])
        wq = max(wq, np.abs(q - O.arr(orc[i].d.qpos)).max()); wv = max(wv, np.abs(v - O.arr(orc[i].d.qvel)).max())
    print(f"[un-injected host twin vs oracle, kind {kind}] pixel entries off by > 1e-4: {n_px_bad} of {n_px}; qpos {wq:.2e} qvel {wv:.2e}")
    assert wq < (2e-5 if reach else 3e-5) and wv < 5e-4
