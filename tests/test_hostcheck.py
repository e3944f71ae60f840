"""The DEVICE physics / task headers (csrc/so100_physics.hpp, so100_cube.hpp, so100_task.hpp) instantiated on the host
(tests/_hostcheck, fp64 and fp32) against the oracle.  This is how the kernel's formulation -- link-frame RNEA + CRBA,
per-joint block PGS, Newton for the cube/floor block, the fp32 task layer -- is checked without a GPU.  CPU only.

The two sides share NO code: the oracle is MuJoCo-structured (world-frame spatial algebra, dense rows, scalar PGS to
convergence); the device headers use a different formulation throughout.  Agreement to 1e-14 in fp64 is the evidence
that both are right; the fp32 numbers below are the device's expected round-off."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as R

import substep_harness as SH
from hostlibs import hostcheck, ptr
from oracle import so100_oracle as O
from scenes import ARM, C5, L, M, floor_cube_batch, fresh


@pytest.fixture(scope="module")
def H():
    return hostcheck()


RNG = np.array(M.jnt_range)


def test_sincos_fp32(H):
    xs = np.linspace(-7.5, 7.5, 200001).astype(np.float32)
    s = C.c_float(); c = C.c_float(); worst = 0
    for x in xs[::97]:
        H.hc_sincos_f(C.c_float(float(x)), C.byref(s), C.byref(c))
        worst = max(worst, abs(s.value - np.sin(np.float64(x))), abs(c.value - np.cos(np.float64(x))))
    assert worst < 1.5e-7


def test_dynamics_and_poses_match_oracle(H):
    rs = np.random.RandomState(0)
    w = dict(M=0, b=0, Mf=0, bf=0, pose=0, posef=0)
    for _ in range(100):
        q = rs.uniform(RNG[:, 0], RNG[:, 1]); v = rs.uniform(-4, 4, 6)
        d = fresh(q, v); L.so100o_forward(C.byref(M), C.byref(d), 0, 0)
        Mo = O.arr(d.M).reshape(12, 12)[:6, :6]; bo = O.arr(d.qfrc_bias)[:6]
        Mh = np.zeros(36); bh = np.zeros(6)
        H.hc_dyn_d(ptr(q), ptr(v), ptr(Mh), ptr(bh))
        w["M"] = max(w["M"], np.abs(Mh.reshape(6, 6) - Mo).max()); w["b"] = max(w["b"], np.abs(bh - bo).max())
        H.hc_dyn_f(ptr(q), ptr(v), ptr(Mh), ptr(bh))
        w["Mf"] = max(w["Mf"], np.abs(Mh.reshape(6, 6) - Mo).max()); w["bf"] = max(w["bf"], np.abs(bh - bo).max())
        out = np.zeros(27)
        ref = np.r_[O.arr(d.xpos)[5], O.arr(d.xpos)[6], O.arr(d.xmat)[6], O.arr(d.cam_xpos), O.arr(d.cam_xmat)]
        H.hc_poses_d(ptr(q), ptr(out)); w["pose"] = max(w["pose"], np.abs(out - ref).max())
        H.hc_poses_f(ptr(q), ptr(out)); w["posef"] = max(w["posef"], np.abs(out - ref).max())
    assert w["M"] < 1e-15 and w["b"] < 1e-13 and w["pose"] < 1e-14          # fp64: same mechanics, different algorithm
    assert w["Mf"] < 1e-7 and w["bf"] < 2e-6 and w["posef"] < 2e-6          # fp32 round-off


def _arm_traj(H, fn, iters_o, iters_h, flags, nenv, nstep, seed):
    rs = np.random.RandomState(seed); wq = wv = 0
    for _ in range(nenv):
        q = rs.uniform(RNG[:, 0] - 0.02, RNG[:, 1] + 0.02); v = rs.uniform(-2, 2, 6)
        d = fresh(q, v); qh = q.copy(); vh = v.copy(); ff = np.zeros(6); fl = np.zeros(6)
        for _ in range(nstep):
            ctrl = O.arr(d.qpos)[:6] + rs.uniform(-1, 1, 6) * 0.075
            O.arr(d.ctrl)[:] = ctrl
            L.so100o_step(C.byref(M), C.byref(d), flags, iters_o, 16)
            fn(ptr(qh), ptr(vh), ptr(ctrl.copy()), ptr(ff), ptr(fl), flags, iters_h, 16)
            wq = max(wq, np.abs(qh - O.arr(d.qpos)[:6]).max()); wv = max(wv, np.abs(vh - O.arr(d.qvel)[:6]).max())
    return wq, wv


def test_block_pgs_reaches_the_oracle_optimum(H):
    """Per-joint block PGS (device) vs scalar PGS to convergence (oracle): same optimum, 3 sweeps reach fp32 level."""
    e2 = _arm_traj(H, H.hc_sub_d, 0, 2, ARM, 3, 60, 1)
    e3 = _arm_traj(H, H.hc_sub_d, 0, 3, ARM, 3, 60, 1)
    e6 = _arm_traj(H, H.hc_sub_d, 0, 6, ARM, 3, 60, 1)
    assert e6[0] < 1e-13 and e6[1] < 1e-12
    assert e3[0] < 1e-8 and e3[1] < 1e-6
    assert e2[0] < 1e-6


def test_arm_fp32_drift_is_within_the_stated_tolerance(H):
    """fp32 device arithmetic vs fp64 oracle over 100 env steps = 1600 substeps: the north star's 1e-5 relative."""
    wq, wv = _arm_traj(H, H.hc_sub_f, 0, 3, ARM, 6, 100, 2)
    assert wq < 1e-5 and wv < 1e-4
    wq, wv = _arm_traj(H, H.hc_sub_f, 0, 0, O.F_CUBE_PINNED, 6, 100, 3)
    assert wq < 1e-5 and wv < 1e-4


def _cube_traj(H, fn, iters_h, tilt, seed, nsub=400):
    rs = np.random.RandomState(seed); w = wv = 0
    for _ in range(4):
        d = fresh()
        pos = np.array([rs.uniform(-.3, .3), rs.uniform(-.3, .3), rs.uniform(0.0, 0.02)]); quat = np.array([1., 0, 0, 0])
        if tilt:
            x = R.from_rotvec(rs.uniform(-0.3, 0.3, 3)).as_quat(); quat = np.array([x[3], x[0], x[1], x[2]])
        vel = np.r_[rs.uniform(-.1, .1, 3), rs.uniform(-1, 1, 3) * tilt]
        O.arr(d.qpos)[6:9] = pos; O.arr(d.qpos)[9:13] = quat; O.arr(d.qvel)[6:] = vel
        ph = pos.copy(); qh = quat.copy(); vh = vel.copy(); wh = np.zeros(16); ap = np.zeros(3)
        for _ in range(nsub // 8):
            L.so100o_step(C.byref(M), C.byref(d), O.F_FLOOR, 0, 8)
            fn(ptr(ph), ptr(qh), ptr(vh), ptr(wh), ptr(ap), O.F_FLOOR, iters_h, 8)
            w = max(w, np.abs(ph - O.arr(d.qpos)[6:9]).max(), np.abs(qh - O.arr(d.qpos)[9:13]).max())
            wv = max(wv, np.abs(vh - O.arr(d.qvel)[6:]).max())
    return w, wv


def test_cube_newton_reaches_the_oracle_optimum(H):
    """Primal Newton + exact line search (device) vs dual PGS to convergence (oracle) on the 16 pyramid rows."""
    w, wv = _cube_traj(H, H.hc_cube_d, 6, 0, 5)
    assert w < 1e-12 and wv < 1e-10                              # flat cube incl. impacts from random heights / velocities: <= 6 iterations
    w, wv = _cube_traj(H, H.hc_cube_d, 8, 1, 6)
    assert w < 1e-11 and wv < 1e-9                               # tumbling cube
    w, wv = _cube_traj(H, H.hc_cube_f, 6, 0, 7)
    assert w < 5e-5 and wv < 2e-3                                # fp32 (bouncing transient included)


def test_cube_newton_per_substep_on_a_sliding_tumbling_cube(H):
    """The cube/floor Newton ALONE (hc_cube_f / hc_cube_d: cube_substep of so100_cube.hpp, cold start), one substep at a time from the
    fp32-rounded states of the oracle's own trajectory of scenes.floor_cube_batch: every pad-free pair in which the cube moves on the floor
    (>= 1 cube/floor record, max |qvel[6:12]| > 1e-3), i.e. a cube that a finger pad has knocked and that slides and tumbles on 1-4 corners.
    test_cube_newton_reaches_the_oracle_optimum sees such a cube only over whole trajectories, with bounds 1000 times looser.
    fp64: 1e-12 on all six velocities.  fp32: the bound of every contact-free pair of tests/test_substep_parity.py, 2e-6 m/s on h * qacc of
    the translation, and the same at the cube's corner for the angular part, |d(h alpha)| * CUBE_HALF < 2e-6.  A pose whose corner count is
    decided inside fp32 round-off (SH.knife_edge_records, the oracle alone) is left to the 2 % cap.
    Measured (64 envs x 24 substeps, seed 0: 719 pairs, 3 knife-edge, 246 on 1-3 corners), contact_iters 30 and 20 alike: fp64 2.0e-13;
    fp32 3.9e-8 m/s and 3.4e-6 rad/s.  With the early stop that compared the cost at x + dx with the quadratic model instead of the active
    sets (seed 1, 650 pairs): fp64 2.0e-6, fp32 9.0e-4 m/s and 0.23 rad/s, 62 pairs above 2e-6 m/s or 2e-4 rad/s."""
    n, nsub = 64, 24
    qpos, qvel, act = floor_cube_batch(n, 0)
    ds = SH.oracle_states(qpos, qvel)
    rs = np.random.RandomState(0)
    pairs = knife = corners13 = 0
    w = {(T, it): np.zeros(2) for T in "fd" for it in (30, 20)}
    for _ in range(nsub):
        for i, d in enumerate(ds):
            SH.round_state_to_fp32(d)
            q0 = O.arr(d.qpos).copy(); v0 = O.arr(d.qvel).copy()
            O.arr(d.ctrl)[:] = (q0[:6].astype(np.float32) + act[i]*SH.JS).astype(np.float64)
            d0 = SH.copy_data(d)
            L.so100o_step(C.byref(M), C.byref(d), C5, -1, 1)
            nfloor = SH.floor_records(d)
            if SH.oracle_contact_summary(d)[2] > 0 or nfloor == 0 or np.abs(v0[6:12]).max() <= SH.MOVING_CUBE_VEL:
                continue
            pairs += 1
            if SH.knife_edge_records(d0, C5, d.ncon, rs):
                knife += 1
                continue
            corners13 += nfloor < 4
            for (T, it), worst in w.items():
                p = q0[6:9].copy(); q = q0[9:13].copy(); v = v0[6:12].copy(); warm = np.zeros(6); ap = np.zeros(3)
                (H.hc_cube_f if T == "f" else H.hc_cube_d)(ptr(p), ptr(q), ptr(v), ptr(warm), ptr(ap), O.F_FLOOR, it, 1)
                e = np.abs(v - O.arr(d.qvel)[6:12])
                worst[:] = np.maximum(worst, [e[:3].max(), e[3:].max()])
    print(f"cube alone, per substep: pad-free pairs with a moving cube {pairs} (knife-edge {knife}, on 1-3 corners {corners13})  " +
          "  ".join(f"{'fp32' if T == 'f' else 'fp64'} iters {it}: |d(h a)| {e[0]:.2e} |d(h alpha)| {e[1]:.2e}" for (T, it), e in w.items()))
    assert pairs >= n*nsub//4 and corners13 >= n*nsub//24 and knife <= 0.02*pairs
    for (T, it), e in w.items():
        if T == "d":
            assert e.max() < 1e-12
        else:
            assert e[0] < 2e-6 and e[1]*SH.CUBE_HALF < 2e-6


@pytest.mark.parametrize("kind,flags", [(1, O.F_FRICTIONLOSS | O.F_LIMITS | O.F_FLOOR), (2, ARM), (5, O.F_FRICTIONLOSS | O.F_LIMITS | O.F_FLOOR),
                                        (3, ARM), (4, O.F_FRICTIONLOSS | O.F_LIMITS | O.F_FLOOR), (6, O.F_FRICTIONLOSS | O.F_LIMITS | O.F_FLOOR)])
def test_task_layer_fp32_vs_oracle(H, kind, flags):
    """so100_task.hpp (what the kernel runs per lane) on the host in fp32 vs the oracle's C task layer."""
    rs = np.random.RandomState(40 + kind)
    reach = kind in (1, 2, 6)
    od = 15 if reach else 8
    for env in range(3):
        e = O.OracleEnv(kind, flags=flags, iters=0); e.e.max_episode_steps = 25
        h = H.hc_env_new(kind)
        inj = rs.random_sample(16).astype(np.float32)
        oo = e.reset(inject=inj); oh = np.zeros(od, np.float32); H.hc_env_reset(h, kind, 0, 0, ptr(inj), ptr(oh))
        np.testing.assert_allclose(oh, oo, rtol=0, atol=1e-6)
        for t in range(60):
            a = np.clip(rs.uniform(-1, 1, 6) * 0.7, -1, 1).astype(np.float32); inj = rs.random_sample(16).astype(np.float32)
            oo, ro, to, tro, tobo = e.step(a, inject=inj, autoreset=True)
            oh = np.zeros(od, np.float32); th = np.zeros(od, np.float32); rh = C.c_float(); dh = C.c_int(); trh = C.c_int()
            H.hc_env_step(h, kind, flags, 4, 6, 25, 0, 0, ptr(a), ptr(inj), ptr(oh), ptr(th), C.byref(rh), C.byref(dh), C.byref(trh))
            tol = 2e-5 if reach else 6e-3
            np.testing.assert_allclose(oh[:6], oo[:6], rtol=0, atol=1e-5 if reach else 2e-6)
            np.testing.assert_allclose(oh, oo, rtol=0, atol=tol, err_msg=f"kind {kind} step {t}")
            assert abs(rh.value - ro) < (1e-4 if kind <= 2 else 2e-3 if kind == 6 else 1.2e-2)
            assert bool(dh.value) == (to or tro) and bool(trh.value) == (tro and not to)
            if to or tro:
                np.testing.assert_allclose(th, tobo, rtol=0, atol=tol)
        H.hc_env_free(h)
