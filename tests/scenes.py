"""Injected states and named constants shared by the test modules (and tools/kbench_split.py): oracle states, the pose generators of
the contact tests, the batches built from them, the flag sets and the shipped solver settings.  Every generator keeps its seeds and
its RNG call order: the batches are part of what the parity tests assert on."""
import ctypes as C

import numpy as np

from hostlibs import ptr
from oracle import so100_oracle as O

L = O.lib()
M = O.model()

# ---- flag sets ----------------------------------------------------------------------------------------------------------------
FREE = O.F_CUBE_PINNED
ARM = O.F_FRICTIONLOSS | O.F_LIMITS | O.F_CUBE_PINNED
NOPADS = O.F_FRICTIONLOSS | O.F_LIMITS | O.F_FLOOR         # friction loss + limits + cube/floor, no finger-pad contacts (round 1's "reference")
REFP = O.F_REFERENCE                                       # + the 8 finger pads vs the floor: what So100Sim / So100VecEnv / main.py run by default
C5 = O.F_CONTACT5                                          # + pad/cube: BASELINE.json configs[4]
LINKS = O.F_REFERENCE | O.F_LINKS_FLOOR                    # link proxies: stand-in capsules for the arm's collision meshes, contacts on ANY link
LCUBE = O.F_REFERENCE | O.F_LINKS_FLOOR | O.F_LINKS_CUBE   # ... and Rotation_Pitch / Upper_Arm vs the cube
PROXIES = O.F_LINKS_FLOOR | O.F_LINKS_CUBE                 # every capsule proxy pair: the run-time-flags kernels so100_rollout_fused / so100_step_mw<K, -1>
UNINSTANTIATED = O.F_FRICTIONLOSS | O.F_FLOOR | O.F_PADS_FLOOR      # 21: no limits -> KindOps::step falls through to <K, -1>

SHIPPED = (2, 20)                                          # (solver_iters, contact_iters): lib.So100Sim, vec_env.So100VecEnv, bench.py
JS = np.float32(0.075)                                     # Env01's action scale (env01_v1.py:18-24)
JNT_LO = np.array([-2.2, -3.14158, 0, -2.0, -3.14158, -0.2]); JNT_HI = np.array([2.2, 0.2, 3.14158, 1.8, 3.14158, 2.0])

# The env's own draws, every kind, no injection: tests/test_rng_reference.py::test_uninjected_task_layer_fp32_vs_oracle (host twin) and
# tests/test_gpu_policy_noise.py::test_uninjected_env_draws_vs_oracle share (flags, action scale) per kind, seed, envs, steps, TimeLimit.
# Un-injected, a float32 and a float64 env can take different branches (a lost cube, a pixel on an integer boundary) and no allowance covers
# that, so the seed is chosen here: with it the float32 host twin already meets every bound the GPU test asserts.  The TimeLimit gives every
# env two auto-resets; the run ends 10 steps after the second, when Env04's cube has settled again (it is dropped onto the floor by every reset).
UNINJECTED_CASES = {1: (NOPADS, 1.0), 2: (ARM, 1.0), 3: (NOPADS, 0.6), 4: (NOPADS, 0.6), 5: (NOPADS, 0.6), 6: (ARM, 1.0)}
UNINJECTED_SEED, UNINJECTED_N, UNINJECTED_STEPS, UNINJECTED_TIMELIMIT = 4, 64, 40, 15


# ---- oracle states and geometry -----------------------------------------------------------------------------------------------
def fresh(q=None, v=None, cube=None, cquat=None):
    """oracle data at its reset values, then qpos[:len(q)] = q, qvel[:len(v)] = v, the cube's position and (normalised) quaternion"""
    d = O.Data()
    L.so100o_reset_data(C.byref(M), C.byref(d))
    if q is not None:
        O.arr(d.qpos)[:len(q)] = q
    if v is not None:
        O.arr(d.qvel)[:len(v)] = v
    if cube is not None:
        O.arr(d.qpos)[6:9] = cube
    if cquat is not None:
        O.arr(d.qpos)[9:13] = np.asarray(cquat) / np.linalg.norm(cquat)
    return d


def pad_frames(d):
    """world centre and rotation of the 8 pad boxes"""
    xp = O.arr(d.xpos); xm = O.arr(d.xmat)
    out = []
    for g in range(8):
        b = M.pad_body[g]; R = xm[b].reshape(3, 3)
        out.append((xp[b] + R @ np.array(M.pad_pos[g][:]), R.copy(), np.array(M.pad_size[g][:])))
    return out


def proxy_bottoms(d):
    """world z of the lowest point of the two end spheres of every link proxy (after so100o_kinematics)"""
    xp = O.arr(d.xpos); xm = O.arr(d.xmat); out = []
    for k in range(O.NPROX):
        b = M.prox_body[k]; R = xm[b].reshape(3, 3)
        for e in range(2):
            out.append((xp[b] + R @ np.array(M.prox_p[k][e][:]))[2] - M.prox_radius[k])
    return np.array(out)


def rot(rs):
    q = rs.randn(4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y)], [2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x)],
                     [2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]]), q


def box_box(cA, RA, hA, cB, RB, hB):
    pos = np.zeros((8, 3)); n = np.zeros(3); dist = np.zeros(8)
    cA, RA, hA, cB, RB, hB = [np.ascontiguousarray(a, np.float64) for a in (cA, RA, hA, cB, RB, hB)]
    k = L.so100o_box_box(ptr(cA), ptr(RA), ptr(hA), ptr(cB), ptr(RB), ptr(hB), ptr(pos), ptr(n), ptr(dist))
    return k, pos[:k].copy(), n.copy(), dist[:k].copy()


def capsule_box(a, b, r, c, R, h):
    a, b, c, R, h = [np.ascontiguousarray(x, np.float64) for x in (a, b, c, R, h)]
    pos = np.zeros(3); n = np.zeros(3); dist = C.c_double(0)
    k = L.so100o_capsule_box(ptr(a), ptr(b), float(r), ptr(c), ptr(R), ptr(h), ptr(pos), ptr(n), C.byref(dist))
    return k, pos, n, dist.value


# ---- pose generators ----------------------------------------------------------------------------------------------------------
def floor_poses(n, seed, band=0.003):
    """random arm poses whose lowest pad corner is within `band` below .. above the floor"""
    rs = np.random.RandomState(seed); out = []
    while len(out) < n:
        q = JNT_LO + (JNT_HI - JNT_LO) * rs.rand(6)
        d = fresh(q); L.so100o_kinematics(C.byref(M), C.byref(d))
        z = min(c[2] - (np.abs(R[2]) * h).sum() for c, R, h in pad_frames(d))
        if -band < z < 0.0005 and O.arr(d.xpos)[5][2] > 0.03:
            out.append(q)
    return out


def grasp_state():
    """gripper horizontal 28 cm above the floor, closing direction along world x, gravity along the pads' short side; the cube
    floats between the jaws: 0.5 mm from the fixed jaw's pads, ~1.5 mm from the moving jaw's (jaw angle 0.1 rad)"""
    q = np.array([0.0, -1.9, 1.6, 0.3, 1.5708, 0.1])
    d = fresh(q); L.so100o_kinematics(C.byref(M), C.byref(d))
    xp = O.arr(d.xpos)[6].copy(); R = O.arr(d.xmat)[6].reshape(3, 3).copy()
    centre = xp + R @ np.array([-0.0026, -0.088, 0.0])
    # cube axes = jaw axes (a 180-degree turn about y here: w ~ 0, so the quaternion is taken from the largest diagonal term)
    cq = np.array([0.0, 0.0, 1.0, 0.0])
    Rq = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1.0]])
    assert np.allclose(R, Rq, atol=1e-4)
    return q, centre, cq


def wrist_first_poses(n, seed):
    """arm poses whose lowest point is a LINK proxy (not a finger pad), within 3 mm above the floor"""
    rs = np.random.RandomState(seed); out = []
    while len(out) < n:
        q = JNT_LO + (JNT_HI - JNT_LO)*rs.rand(6)
        d = fresh(q); L.so100o_kinematics(C.byref(M), C.byref(d))
        pb = proxy_bottoms(d)
        zpad = min(c[2] - (np.abs(R[2])*h).sum() for c, R, h in pad_frames(d))
        if 0.0 < pb[:6].min() < 0.003 and zpad > pb[:6].min() + 0.02:
            out.append(q)
    return out


def link_cube_states(n, seed, pen=(0.0002, 0.003)):
    """arm poses with the cube placed against the Rotation_Pitch (even i) or Upper_Arm (odd i) capsule, penetrating by pen[0]..pen[1] metres"""
    rs = np.random.RandomState(seed); out = []
    hs = np.full(3, 0.01)
    while len(out) < n:
        k = len(out) % 2
        q = JNT_LO + (JNT_HI - JNT_LO)*rs.rand(6)
        d = fresh(q); L.so100o_kinematics(C.byref(M), C.byref(d))
        xp = O.arr(d.xpos); b = M.cprox_body[k]
        a_, b_ = xp[b].copy(), xp[b + 1].copy()
        s = a_ + (0.15 + 0.85*rs.rand())*(b_ - a_)
        u = rs.randn(3); u /= np.linalg.norm(u)
        Rc, qc = rot(rs)
        want = -(pen[0] + (pen[1] - pen[0])*rs.rand())
        lo_, hi_ = 0.0, 0.08                                 # bisection on the cube's offset along u for the wanted penetration
        for _ in range(40):
            mid = 0.5*(lo_ + hi_)
            kk, _, _, dist = capsule_box(a_, b_, M.cprox_radius[k], s + u*mid, Rc, hs)
            if kk and dist < want: lo_ = mid
            else: hi_ = mid
        c = s + u*lo_
        kk, _, _, dist = capsule_box(a_, b_, M.cprox_radius[k], c, Rc, hs)
        if not kk or abs(dist - want) > 2e-4 or c[2] < 0.012 + 0.0174:      # (cube clear of the floor: the pair under test alone)
            continue
        # no other proxy / pad may touch anything in this pose
        dd = fresh(q); O.arr(dd.qpos)[6:9] = c; O.arr(dd.qpos)[9:13] = qc
        L.so100o_forward(C.byref(M), C.byref(dd), LCUBE | O.F_PADS_CUBE, -1)
        if dd.ncon != 1 or dd.con[0].kind != 4:
            continue
        out.append((q, c, qc))
    return out


def floor_cube_states(n, seed, pen=(5e-5, 2e-3)):
    """arm poses with a finger pad 0.5 .. 30 mm above the floor and the cube LYING on the floor (z = 0.0099) at a random yaw, walked towards
    one of the 8 pads along a random horizontal direction until the oracle reports a pad/cube record (kind 2) that is pen[0] .. pen[1]
    metres deep: the pad knocks the cube, which then slides and tumbles on one to four corners (what F_CONTACT5 training meets)"""
    rs = np.random.RandomState(seed); out = []
    while len(out) < n:
        q = JNT_LO + (JNT_HI - JNT_LO)*rs.rand(6)
        d = fresh(q); L.so100o_kinematics(C.byref(M), C.byref(d))
        frames = pad_frames(d)
        z = min(c[2] - (np.abs(R[2])*h).sum() for c, R, h in frames)
        if not 0.0005 < z < 0.03:
            continue
        centre = frames[rs.randint(8)][0]
        yaw = rs.uniform(-np.pi, np.pi); phi = rs.uniform(-np.pi, np.pi)
        qc = np.array([np.cos(yaw/2), 0.0, 0.0, np.sin(yaw/2)]); u = np.array([np.cos(phi), np.sin(phi), 0.0])
        for s in np.arange(60, -1, -1)*0.0005:             # 30 mm .. 0 in 0.5 mm steps: the first offset at which the pad touches
            c = np.array([centre[0], centre[1], 0.0099]) + u*s
            dd = fresh(q, cube=c, cquat=qc)
            L.so100o_forward(C.byref(M), C.byref(dd), C5, -1)
            deep = [dd.con[i].dist for i in range(dd.ncon) if dd.con[i].kind == 2]
            if deep:
                if -pen[1] < min(deep) < -pen[0]:
                    out.append((q, c, qc))
                break
    return out


# ---- batches: (qpos [n, 13], qvel [n, 12], act [n, 6]) ------------------------------------------------------------------------
def floor_batch(n, seed, band=0.002):
    """arm poses with the lowest pad corner within `band` of the floor, moderate joint velocities, cube resting on the floor"""
    rs = np.random.RandomState(seed)
    poses = floor_poses(n, seed + 100, band=band)
    qpos = np.zeros((n, 13)); qvel = np.zeros((n, 12))
    for i, q in enumerate(poses):
        qpos[i, :6] = q; qpos[i, 6:9] = [0.15 + 0.02*rs.randn(), -0.25, 0.0099]; qpos[i, 9] = 1.0
        qvel[i, :6] = rs.randn(6)*0.3
    act = rs.uniform(-1, 1, (n, 6)).astype(np.float32)
    return qpos, qvel, act


def grasp_batch(n, seed):
    """the jaw closing on a cube that floats between the pads (BASELINE.json configs[4]): generic small cube rotations"""
    rs = np.random.RandomState(seed)
    q, centre, cq = grasp_state()
    qpos = np.zeros((n, 13)); qvel = np.zeros((n, 12))
    qpos[:, :6] = q; qpos[:, 5] = 0.065 + rs.uniform(0.0, 0.01, n)          # moving pads 0.1 .. 0.6 mm from the cube: contact within the first step
    qpos[:, 6:9] = centre + rs.uniform(-1, 1, (n, 3))*np.array([0.0004, 0.002, 0.002])
    # cube axes = jaw axes, turned by a small random rotation (generic orientations: no two SAT axes tie)
    for i in range(n):
        w = rs.randn(3)*0.03; ang = np.linalg.norm(w); ax = w/ang
        dq = np.array([np.cos(ang/2), *(np.sin(ang/2)*ax)])
        a, b = cq, dq
        qpos[i, 9:13] = [a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                         a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]]
    act = np.zeros((n, 6), np.float32); act[:, 5] = -1.0                    # close the jaw as fast as the action allows
    return qpos, qvel, act


def wrist_first_batch(n, seed):
    """poses whose lowest point is a link proxy (wrist / forearm first), pushed 1e-2 rad into the table; random joint velocities"""
    rs = np.random.RandomState(seed)
    qpos = np.zeros((n, 13)); qvel = np.zeros((n, 12))
    for i, q in enumerate(wrist_first_poses(n, seed + 7)):
        qpos[i, :6] = q; qpos[i, 1] += 0.01; qpos[i, 6:9] = [0.15, -0.25, 0.0099]; qpos[i, 9] = 1.0; qvel[i, :6] = rs.randn(6)*0.3
    act = rs.uniform(-1, 1, (n, 6)).astype(np.float32); act[:, 1] = 0.5
    return qpos, qvel, act


def link_cube_batch(n, seed):
    """the cube placed against the Rotation_Pitch / Upper_Arm capsule (alternating), 0.2-3 mm deep, random joint and cube velocities"""
    rs = np.random.RandomState(seed)
    qpos = np.zeros((n, 13)); qvel = np.zeros((n, 12))
    for i, (q, c, qc) in enumerate(link_cube_states(n, seed + 3)):
        qpos[i, :6] = q; qpos[i, 6:9] = c; qpos[i, 9:13] = qc
        qvel[i, :6] = rs.randn(6)*0.3; qvel[i, 6:9] = rs.randn(3)*0.02
    act = rs.uniform(-1, 1, (n, 6)).astype(np.float32)
    return qpos, qvel, act


def floor_cube_batch(n, seed):
    """the cube on the floor at a random yaw with a finger pad 0.05-2 mm inside it (floor_cube_states): random joint velocities and actions,
    the cube at rest -- cube/floor, pad/cube and sometimes pad/floor records in one coupled solve, then a cube sliding on 1-4 corners"""
    rs = np.random.RandomState(seed)
    qpos = np.zeros((n, 13)); qvel = np.zeros((n, 12))
    for i, (q, c, qc) in enumerate(floor_cube_states(n, seed + 11)):
        qpos[i, :6] = q; qpos[i, 6:9] = c; qpos[i, 9:13] = qc
        qvel[i, :6] = rs.randn(6)*0.3
    act = rs.uniform(-1, 1, (n, 6)).astype(np.float32)
    return qpos, qvel, act


def idle_batch(n):
    """(qpos, qvel) of the filler envs of a batch larger than the injected one: arm folded above the table, cube at rest beside it, no velocities"""
    qpos = np.zeros((n, 13)); qpos[:, 9] = 1.0; qpos[:, 6:9] = [0.2, -0.2, 0.0099]; qpos[:, :6] = [0, -1.5, 1.5, 0.5, 0, 0.2]
    return qpos, np.zeros((n, 12))
