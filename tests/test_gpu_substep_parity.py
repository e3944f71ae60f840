"""Per-substep contact parity of the HIP kernels (through the C ABI, handle created with frame_skip = 1) against the fp64
oracle: EVERY env in EVERY substep -- same contact count, same contact features (contact_sig state row vs the oracle's
so100o_contact.feat), h * qacc within the stated fp32 bound, solver residual (tests/substep_harness.py; the host-instantiation
twin of this test is tests/test_substep_parity.py).  All four step kernels are covered through the batch size: 4-wave latency
kernel with 16 / 32 / 64 envs per workgroup (4 / 2 / 1 cooperating contact lanes per env) and the one-wave throughput kernel; plus
a flag set WITHOUT a compile-time instantiation (run-time-flags kernels so100_step_mw / so100_step_fused<K, -1>).  The cube pushed along
the floor by a finger pad (mixed contact sets, then a cube sliding and tumbling on 1-4 corners) runs on the 4-wave, one-wave and <K, -1> kernels.

Every case runs at the shipped solver settings (2, 20) and at (4, 30), with the same bounds (the residual check of the 2-sweep leg is
split: tests/substep_harness.py check_residual).  Stated fp32 bound on h * qacc from identical fp32-rounded states (h = 2 ms):
2e-6 rad/s without pad contact, 5e-5 rad/s (m/s for the cube) and 1e-2 relative with it (stiff pad rows: condition ~1e5).
"parity unpinned (physics)": MuJoCo is not available."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import substep_harness as SH                              # noqa: E402
from gpu_support import inject_state, make_sim            # noqa: E402
from oracle import so100_oracle as O                      # noqa: E402  (the checker)
from scenes import (C5, LCUBE, LINKS, PROXIES, REFP, SHIPPED, UNINSTANTIATED, floor_batch, floor_cube_batch, grasp_batch,   # noqa: E402
                    idle_batch, link_cube_batch, wrist_first_batch)


class HipDevice:
    def __init__(self, n, m, flags, iters=(4, 30)):
        self.sim = make_sim(1, n, flags=flags, solver_iters=iters[0], contact_iters=iters[1], frame_skip=1, max_episode_steps=0, seed=3)
        self.n, self.m, self.flags, self.iters = n, m, flags, iters
        self.twin = None
        self.sim.reset()
        self.QP, self.QV = idle_batch(n); self.A = np.zeros((n, 6), np.float32)

    def __call__(self, q32, v32, act):
        m, sim = self.m, self.sim
        self.QP[:m] = q32; self.QV[:m] = v32; self.A[:m] = act
        inject_state(sim, self.QP, self.QV)
        if self.iters[0] < 4:                             # every state row (warm starts included) as the step sees it, for resolve()
            self.before = {f: sim.get_field(f, dtype=torch.int32) for f in sim.field_names()}
        sim.step(torch.from_numpy(self.A).cuda())
        gq, gv = sim.get_state()
        cs = sim.get_field("contact_stat", dtype=torch.int32).cpu().numpy()[:m]
        assert (cs >> 8).max() == 0                       # nothing over the contact budget
        return (gq.cpu().numpy().T[:m].astype(np.float64), gv.cpu().numpy().T[:m].astype(np.float64), cs & 255,
                sim.get_field("contact_sig", dtype=torch.int32).cpu().numpy()[:m], sim.get_field("solver_residual").cpu().numpy()[:m])

    def resolve(self, envs, iters):
        """the last substep again on a twin handle (same batch size, so the same kernel) with `iters` block-PGS sweeps, from the same state rows"""
        if self.twin is None:
            self.twin = make_sim(1, self.n, flags=self.flags, solver_iters=iters, contact_iters=self.iters[1], frame_skip=1, max_episode_steps=0, seed=3)
        for f, w in self.before.items():
            self.twin.set_field(f, w)
        self.twin.step(torch.from_numpy(self.A).cuda())
        return self.twin.get_state()[1].cpu().numpy().T[envs].astype(np.float64)


@pytest.mark.parametrize("n,flags", [(96, REFP), (8192, REFP), (16384, REFP), (16384 + 96, REFP), (96, UNINSTANTIATED), (16384 + 96, UNINSTANTIATED)])
def test_pad_floor_per_substep(n, flags):
    _pad_floor_per_substep(n, flags, (4, 30))


@pytest.mark.parametrize("n,flags", [(96, REFP), (8192, REFP), (16384, REFP), (16384 + 96, REFP), (96, UNINSTANTIATED), (16384 + 96, UNINSTANTIATED)])
def test_pad_floor_per_substep_at_shipped_settings(n, flags):
    """test_pad_floor_per_substep at the shipped solver settings (solver_iters, contact_iters) = SHIPPED = (2, 20), with the same bounds"""
    _pad_floor_per_substep(n, flags, SHIPPED)


def _pad_floor_per_substep(n, flags, iters):
    m, nsub = 96, 24
    qpos, qvel, act = floor_batch(m, 0)
    T = SH.run_substep_parity(HipDevice(n, m, flags, iters), qpos, qvel, act, flags, nsub, f"HIP {iters} n={n} flags={flags} pad/floor")
    SH.check_tally(T, m*nsub//3, iters=iters)


@pytest.mark.parametrize("n", [48, 8192, 16384 + 48])
def test_link_proxies_per_substep(n):
    _link_proxies_per_substep(n, (4, 30))


@pytest.mark.parametrize("n", [48, 8192, 16384 + 48])
def test_link_proxies_per_substep_at_shipped_settings(n):
    """test_link_proxies_per_substep at the shipped solver settings (solver_iters, contact_iters) = SHIPPED = (2, 20), with the same bounds"""
    _link_proxies_per_substep(n, SHIPPED)


def _link_proxies_per_substep(n, iters):
    """SO100_F_LINKS_FLOOR (capsule proxies of the arm's collision meshes: contacts on ANY link, the general form of the solver), through
    the run-time-flags kernels: poses that reach the table wrist / forearm first"""
    m, nsub = 48, 24
    qpos, qvel, act = wrist_first_batch(m, 0)
    T = SH.run_substep_parity(HipDevice(n, m, LINKS, iters), qpos, qvel, act, LINKS, nsub, f"HIP {iters} n={n} link proxies")
    SH.check_tally(T, m*nsub//3, iters=iters)


@pytest.mark.parametrize("n", [64, 8192, 16384, 16384 + 64])
def test_pad_cube_grasp_per_substep(n):
    _pad_cube_grasp_per_substep(n, (4, 30))


@pytest.mark.parametrize("n", [64, 8192, 16384, 16384 + 64])
def test_pad_cube_grasp_per_substep_at_shipped_settings(n):
    """test_pad_cube_grasp_per_substep at the shipped solver settings (solver_iters, contact_iters) = SHIPPED = (2, 20), with the same bounds"""
    _pad_cube_grasp_per_substep(n, SHIPPED)


def _pad_cube_grasp_per_substep(n, iters):
    m, nsub = 64, 40
    qpos, qvel, act = grasp_batch(m, 1)
    T = SH.run_substep_parity(HipDevice(n, m, C5, iters), qpos, qvel, act, C5, nsub, f"HIP {iters} n={n} grasp")
    SH.check_tally(T, m*nsub//3, m*nsub//4, iters=iters)


@pytest.mark.parametrize("n", [32, 8192, 16384 + 32])
def test_link_cube_per_substep(n):
    _link_cube_per_substep(n, (4, 30))


@pytest.mark.parametrize("n", [32, 8192, 16384 + 32])
def test_link_cube_per_substep_at_shipped_settings(n):
    """test_link_cube_per_substep at the shipped solver settings (solver_iters, contact_iters) = SHIPPED = (2, 20), with the same bounds"""
    _link_cube_per_substep(n, SHIPPED)


def _link_cube_per_substep(n, iters):
    """SO100_F_LINKS_CUBE (Rotation_Pitch / Upper_Arm capsules vs the cube: the pairs the reference scene leaves live) through the
    run-time-flags kernels -- 4 / 2 / 1 contact lanes per env and the one-wave kernel: the cube placed against either capsule, arm and cube
    solved together (12 unknowns, records on links 0 / 1); then the closing-jaw grasp with every proxy pair switched on as well"""
    m, nsub = 32, 12
    qpos, qvel, act = link_cube_batch(m, 0)
    T = SH.run_substep_parity(HipDevice(n, m, LCUBE, iters), qpos, qvel, act, LCUBE, nsub, f"HIP {iters} n={n} link proxies vs cube")
    SH.check_tally(T, m*nsub//3, m*nsub//3, iters=iters)
    if n == 32:
        flags = LCUBE | O.F_PADS_CUBE
        qpos, qvel, act = grasp_batch(m, 2)
        T = SH.run_substep_parity(HipDevice(n, m, flags, iters), qpos, qvel, act, flags, 32, f"HIP {iters} n={n} all proxies + grasp")
        SH.check_tally(T, m*32//4, m*32//5, iters=iters)


FLOOR_CUBE_CASES = [(64, C5), (16384 + 64, C5), (64, C5 | PROXIES)]      # 4-wave kernel, 16 envs per workgroup / one-wave kernel / <K, -1> kernels


@pytest.mark.parametrize("n,flags", FLOOR_CUBE_CASES)
def test_floor_cube_per_substep(n, flags):
    _floor_cube_per_substep(n, flags, (4, 30))


@pytest.mark.parametrize("n,flags", FLOOR_CUBE_CASES)
def test_floor_cube_per_substep_at_shipped_settings(n, flags):
    """test_floor_cube_per_substep at the shipped solver settings (solver_iters, contact_iters) = SHIPPED = (2, 20), with the same bounds"""
    _floor_cube_per_substep(n, flags, SHIPPED)


def _floor_cube_per_substep(n, flags, iters):
    """The cube lying on the floor at a random yaw, knocked by a finger pad (scenes.floor_cube_batch: what F_CONTACT5 training and bench.py's
    env01_contact meet): cube/floor, pad/cube and pad/floor records in one coupled 12-unknown solve, then the cube/floor Newton alone on a
    cube that slides and tumbles on 1-4 corners.  The same conditions and bounds as the host twin's
    tests/test_substep_parity.py::test_floor_cube_per_substep_host_fp32, against the oracle: both classes populated, knife-edge poses (pad-free
    ones included) <= 2 %, h * qacc within 2e-6 without pad contact and 5e-5 / 1e-2 relative with, the cube's angular h * alpha within the
    same at the cube's corner (SH.check_moving_cube)."""
    m, nsub = 64, 24
    qpos, qvel, act = floor_cube_batch(m, 0)
    T = SH.run_substep_parity(HipDevice(n, m, flags, iters), qpos, qvel, act, flags, nsub, f"HIP {iters} n={n} flags={flags} cube on the floor")
    SH.check_tally(T, m*nsub//3, m*nsub//4, iters=iters)
    SH.check_moving_cube(T)
