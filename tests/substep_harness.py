"""Per-substep contact parity harness (shared by the CPU host-instantiation test and the GPU test).

Every env follows the ORACLE's trajectory: before each substep the oracle's state is rounded to fp32 and handed to the device
code (host instantiation, or the HIP kernels created with frame_skip = 1), both sides take ONE physics substep from that same
state, and EVERY env is compared in EVERY substep -- no survivor filter decides what is looked at:
  * the same number of contact records and the same set of contact features (pad corner / manifold slot ids: the oracle's
    so100o_contact.feat against the device's contact_sig state row),
  * the acceleration the substep applied, h * qacc = v_after - v_before, within the stated fp32 bound,
  * the solver residual, split: on contact substeps the Newton's; on contact-free substeps the block PGS's.  At 2 sweeps (the shipped
    setting) that row reports the change made by the LAST sweep, which can be large when the first sweep moves far from the warm start:
    such "stale" envs are counted, held to the free h * qacc bound against the oracle, and re-solved from the same state with 64 sweeps
    on the device (`device_substep.resolve`), which their velocities must match within the same bound.
A pose whose contact set is decided inside fp32 round-off (a corner within ~1e-7 m of the plane, two separating axes tied) is
classified as `knife_edge` -- by re-running the ORACLE on the state nudged by a few fp32 ulps, for EVERY pose, never by looking at
the device's answer -- and counted; on all other poses count and set must match exactly, and the caller bounds the knife-edge share.
A pair with a "moving cube on the floor" (>= 1 cube/floor record, max |qvel[6:12]| > MOVING_CUBE_VEL before the substep; the oracle's state
alone decides) is tallied a second time in fields of its own, with the cube's angular h * alpha, which h * qacc leaves out; a pad-free pose
of that class is a knife edge if the oracle's total record count changes under the same nudges (check_moving_cube holds the conditions).
"parity unpinned (physics)": the oracle restates MuJoCo's algorithm (oracle/so100_oracle.c), MuJoCo itself is not available."""
import ctypes as C

import numpy as np

from oracle import so100_oracle as O
from scenes import JS, L, M, fresh


def feature_mix(fid):
    """csrc/so100_contact.hpp: contact_id_mix"""
    h = ((fid + 1)*0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h*0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> 13
    return h


def oracle_contact_summary(d):
    """(records the device keeps, signature of the pad-contact set, pad contacts, coupled) of the oracle's last forward pass"""
    pads = [d.con[i] for i in range(d.ncon) if d.con[i].kind != 0]
    coupled = any(c.kind in (2, 4) for c in pads)                # pad/cube or link proxy/cube: arm and cube solved together
    n = len(pads) + (sum(1 for i in range(d.ncon) if d.con[i].kind == 0) if coupled else 0)
    sig = sum(feature_mix(c.feat) for c in pads) & 0xFFFFFFFF
    return n, (sig - (1 << 32) if sig >= (1 << 31) else sig), len(pads), coupled


def round_state_to_fp32(d):
    q = O.arr(d.qpos); v = O.arr(d.qvel)
    q[:] = q.astype(np.float32).astype(np.float64); v[:] = v.astype(np.float32).astype(np.float64)


def oracle_substep(d, act, flags):
    """ctrl of Env01 (env01_v1.py:18-24: measured angle + 0.075 a), one mj_step with the oracle's Newton"""
    O.arr(d.ctrl)[:] = (O.arr(d.qpos)[:6].astype(np.float32) + act.astype(np.float32)*JS).astype(np.float64)
    L.so100o_step(C.byref(M), C.byref(d), flags, -1, 1)


def knife_edge(d0, flags, ref, rs, probes=8, ulps=8):
    """is the contact SET of this pose decided inside fp32 round-off?  The oracle's own forward pass is repeated on the state
    nudged by up to `ulps` fp32 ulps per coordinate (what fp32 kinematics loses along the 6-link chain: ~1e-7 m at the pads) in
    `probes` random directions; a pose is a knife edge if any of them changes the oracle's (count, feature set).
    d0: the pre-step oracle state (ctrl already set).  Independent of the device's answer."""
    q0 = O.arr(d0.qpos).astype(np.float32)
    for _ in range(probes):
        d = copy_data(d0)
        k = rs.randint(-ulps, ulps + 1, size=q0.shape)
        q = q0.copy()
        for _ in range(ulps):
            step = np.sign(k).astype(np.float32); k = k - np.sign(k)
            q = np.where(step > 0, np.nextafter(q, np.float32(np.inf)), np.where(step < 0, np.nextafter(q, np.float32(-np.inf)), q))
        O.arr(d.qpos)[:] = q.astype(np.float64)
        L.so100o_forward(C.byref(M), C.byref(d), flags, -1)
        if oracle_contact_summary(d)[:2] != ref[:2]:
            return True
    return False


MOVING_CUBE_VEL = 1e-3     # "moving cube on the floor": >= 1 cube/floor record (kind 0) and max |qvel[6:12]| above this before the substep


def floor_records(d):
    """cube/floor records (kind 0) of the oracle's last forward pass: the corners the cube stands on"""
    return sum(1 for i in range(d.ncon) if d.con[i].kind == 0)


def knife_edge_records(d0, flags, ncon, rs, probes=8, ulps=8):
    """knife_edge for a pose WITHOUT pad contact whose cube moves on the floor: the device keeps no record of the cube/floor corners of such
    a pose, so the probe asks whether the oracle's TOTAL record count changes under the same fp32 ulp nudges (a corner within round-off of the
    plane switches its four rows, and with them the damping force B J v, on or off).  Independent of the device's answer."""
    q0 = O.arr(d0.qpos).astype(np.float32)
    for _ in range(probes):
        d = copy_data(d0)
        k = rs.randint(-ulps, ulps + 1, size=q0.shape)
        q = q0.copy()
        for _ in range(ulps):
            step = np.sign(k).astype(np.float32); k = k - np.sign(k)
            q = np.where(step > 0, np.nextafter(q, np.float32(np.inf)), np.where(step < 0, np.nextafter(q, np.float32(-np.inf)), q))
        O.arr(d.qpos)[:] = q.astype(np.float64)
        L.so100o_forward(C.byref(M), C.byref(d), flags, -1)
        if d.ncon != ncon:
            return True
    return False


def copy_data(d):
    c = O.Data(); C.memmove(C.byref(c), C.byref(d), C.sizeof(O.Data))
    return c


STALE_RES = 1e-2           # a contact-free residual above this is re-solved with RESOLVE_ITERS sweeps
RESOLVE_ITERS = 64         # the largest solver_iters the handle accepts


class Tally:
    """what happened to every (env, substep) pair; printed so the test log carries the class counts"""
    def __init__(self):
        self.pairs = self.contact = self.coupled = self.knife = self.set_mismatch = self.count_mismatch = 0
        self.worst_dv = self.worst_dv_contact = self.worst_res = 0.0
        self.worst_rel = 0.0
        self.worst_res_contact = self.worst_res_free = 0.0
        self.stale = self.resolved = 0                       # contact-free env-substeps with residual > STALE_RES / of them re-solved
        self.worst_dv_stale = self.worst_dv_resolved = 0.0   # their |d(h qacc)| against the oracle / against RESOLVE_ITERS sweeps
        # the cube's angular h * alpha (qvel[9:12]), which worst_dv / worst_dv_contact leave out: without / with pad contact
        self.worst_dw = self.worst_dw_contact = 0.0
        # "moving cube on the floor" (MOVING_CUBE, from the oracle's state alone): pairs, the pad-free ones of them, the pairs with the
        # cube on 1-3 corners, and the class's own worst errors (translation + arm: dv, angular: dw; pad-free / in pad contact)
        self.moving = self.moving_free = self.corners13 = self.knife_free = 0
        self.worst_dv_moving = self.worst_dw_moving = self.worst_dv_moving_contact = self.worst_dw_moving_contact = 0.0
        self.worst_rel_moving = 0.0
        self.worst_dv_still = self.worst_dw_still = 0.0      # pad-free pairs outside that class

    def line(self, name):
        return (f"[{name}] env-substeps {self.pairs}  in pad contact {self.contact}  coupled {self.coupled}  knife-edge poses {self.knife}  "
                f"count mismatches {self.count_mismatch}  set mismatches {self.set_mismatch}  worst |d(h qacc)| free {self.worst_dv:.2e} contact {self.worst_dv_contact:.2e}  "
                f"worst relative {self.worst_rel:.2e}  worst residual {self.worst_res:.2e} (contact {self.worst_res_contact:.2e} free {self.worst_res_free:.2e})  "
                f"stale free residuals > {STALE_RES:g}: {self.stale} (re-solved {self.resolved}; worst |d(h qacc)| vs oracle {self.worst_dv_stale:.2e}, "
                f"vs {RESOLVE_ITERS} sweeps {self.worst_dv_resolved:.2e})  "
                f"cube angular worst |d(h alpha)| free {self.worst_dw:.2e} contact {self.worst_dw_contact:.2e}  "
                f"moving cube on the floor {self.moving} (pad-free {self.moving_free}, on 1-3 corners {self.corners13}, pad-free knife-edge "
                f"{self.knife_free}): worst |d(h qacc)| pad-free {self.worst_dv_moving:.2e} contact {self.worst_dv_moving_contact:.2e} "
                f"relative {self.worst_rel_moving:.2e}  worst |d(h alpha)| pad-free {self.worst_dw_moving:.2e} contact {self.worst_dw_moving_contact:.2e}  "
                f"pad-free pairs outside the class: worst |d(h qacc)| {self.worst_dv_still:.2e} |d(h alpha)| {self.worst_dw_still:.2e}")


def oracle_states(qpos, qvel):
    ds = []
    for i in range(len(qpos)):
        d = fresh(); O.arr(d.qpos)[:] = qpos[i]; O.arr(d.qvel)[:] = qvel[i]
        ds.append(d)
    return ds


def _halpha(v, v0):
    """the cube's angular velocity change (body frame, qvel[9:12])"""
    return v[9:12] - v0[9:12]


def _hqacc(v, v0):
    """the arm's and the cube translation's velocity change: what the substep applied"""
    return np.concatenate([v[:6] - v0[:6], v[6:9] - v0[6:9]])


def run_substep_parity(device_substep, qpos, qvel, act, flags, nsub, name, seed=0):
    """device_substep(q32 [n,13], v32 [n,12], act [n,6]) -> (qpos [n,13], qvel [n,12], count [n], sig [n], residual [n]) after ONE
    substep from exactly that state.  If it has resolve(envs, iters) -> qvel [len(envs), 12], that takes the substep it just took again,
    from the same state and warm starts, with `iters` block-PGS sweeps: contact-free envs whose residual exceeds STALE_RES are re-solved
    with RESOLVE_ITERS.  Returns the Tally; raises on the first non-knife-edge contact-set mismatch."""
    n = len(qpos)
    ds = oracle_states(qpos, qvel)
    rs = np.random.RandomState(seed)
    rs_free = np.random.RandomState(seed + 1)                # the pad-free probe's own stream: the draws of `rs` stay what they were
    T = Tally()
    h = M.timestep
    for s in range(nsub):
        for d in ds:
            round_state_to_fp32(d)
        q32 = np.stack([O.arr(d.qpos).copy() for d in ds]); v32 = np.stack([O.arr(d.qvel).copy() for d in ds])
        gq, gv, gcount, gsig, gres = device_substep(q32, v32, act)
        assert np.isfinite(gq).all() and np.isfinite(gv).all(), (name, s)
        stale = []
        for i, d in enumerate(ds):
            O.arr(d.ctrl)[:] = (q32[i, :6].astype(np.float32) + act[i].astype(np.float32)*JS).astype(np.float64)
            d0 = copy_data(d)
            L.so100o_step(C.byref(M), C.byref(d), flags, -1, 1)
            ref = oracle_contact_summary(d)
            T.pairs += 1; T.contact += ref[2] > 0; T.coupled += bool(ref[3])
            near = ref[2] > 0 or gcount[i] > 0
            ke = near and knife_edge(d0, flags, ref, rs)
            nfloor = floor_records(d)
            moving = nfloor > 0 and np.abs(v32[i, 6:12]).max() > MOVING_CUBE_VEL
            T.moving += bool(moving); T.moving_free += bool(moving and ref[2] == 0); T.corners13 += 1 <= nfloor <= 3
            if moving and not near and knife_edge_records(d0, flags, d.ncon, rs_free):
                ke = True; T.knife_free += 1
            T.knife += bool(ke)
            if not ke:
                if gcount[i] != ref[0]:
                    T.count_mismatch += 1
                elif gsig[i] != ref[1]:
                    T.set_mismatch += 1
                assert gcount[i] == ref[0] and gsig[i] == ref[1], (name, "substep", s, "env", i, "device", int(gcount[i]), int(gsig[i]), "oracle", ref)
                # h * qacc of the arm (and of the cube's translation): what the substep did to the velocities
                dvo = _hqacc(O.arr(d.qvel), v32[i])
                dvg = _hqacc(gv[i], v32[i])
                err = np.abs(dvg - dvo).max(); scale = np.abs(dvo).max()
                erw = np.abs(_halpha(gv[i], v32[i]) - _halpha(O.arr(d.qvel), v32[i])).max()
                if ref[2] > 0:
                    T.worst_dv_contact = max(T.worst_dv_contact, err); T.worst_rel = max(T.worst_rel, err/(1e-3 + scale))
                    T.worst_res_contact = max(T.worst_res_contact, float(gres[i]))
                    T.worst_dw_contact = max(T.worst_dw_contact, erw)
                    if moving:
                        T.worst_dv_moving_contact = max(T.worst_dv_moving_contact, err); T.worst_dw_moving_contact = max(T.worst_dw_moving_contact, erw)
                        T.worst_rel_moving = max(T.worst_rel_moving, err/(1e-3 + scale))
                else:
                    T.worst_dw = max(T.worst_dw, erw)
                    if moving:
                        T.worst_dv_moving = max(T.worst_dv_moving, err); T.worst_dw_moving = max(T.worst_dw_moving, erw)
                    else:
                        T.worst_dv_still = max(T.worst_dv_still, err); T.worst_dw_still = max(T.worst_dw_still, erw)
                    T.worst_dv = max(T.worst_dv, err)
                    T.worst_res_free = max(T.worst_res_free, float(gres[i]))
                    if gres[i] > STALE_RES:
                        T.stale += 1; T.worst_dv_stale = max(T.worst_dv_stale, err); stale.append(i)
                T.worst_res = max(T.worst_res, float(gres[i]))
        if stale and hasattr(device_substep, "resolve"):
            v64 = device_substep.resolve(stale, RESOLVE_ITERS)
            for k, i in enumerate(stale):
                T.resolved += 1
                T.worst_dv_resolved = max(T.worst_dv_resolved, float(np.abs(_hqacc(gv[i], v32[i]) - _hqacc(v64[k], v32[i])).max()))
    print(T.line(name))
    return T


def check_tally(T, min_contact, min_coupled=0, iters=(4, 30)):
    """the pass conditions of a run_substep_parity Tally, the same for the host twin and for the HIP kernels"""
    assert T.contact >= min_contact and T.coupled >= min_coupled                   # the batch did exercise the contact path
    assert T.knife <= 0.02*T.pairs                                                 # poses decided inside fp32 round-off are rare
    assert T.count_mismatch == 0 and T.set_mismatch == 0
    assert T.worst_dv < 2e-6
    assert T.worst_dv_contact < 5e-5 and T.worst_rel < 1e-2
    check_residual(T, iters)


CUBE_HALF = 0.01           # half edge of block_a: an angular velocity error w moves a corner's contact point by w * CUBE_HALF m/s


def check_moving_cube(T):
    """the conditions and bounds of a batch whose cube slides and tumbles on the floor (scenes.floor_cube_batch), on top of check_tally
    (whose bounds on h * qacc -- 2e-6 without pad contact, 5e-5 and 1e-2 relative with -- already cover every pair, the moving cube's
    included).  The class must not be empty: pad-free pairs with a moving cube, and pairs with the cube on 1-3 corners.  The cube's angular
    h * alpha is held to the same two bounds measured where the cube/floor Newton measures its own convergence, at the cube's corner:
    |d(h alpha)| * CUBE_HALF < 2e-6 m/s without pad contact, < 5e-5 m/s with it."""
    assert T.moving_free >= T.pairs//4 and T.corners13 >= T.pairs//24
    assert T.worst_dv_moving < 2e-6 and T.worst_dv_still < 2e-6
    assert T.worst_dv_moving_contact < 5e-5 and T.worst_rel_moving < 1e-2
    assert T.worst_dw*CUBE_HALF < 2e-6 and T.worst_dw_contact*CUBE_HALF < 5e-5


def check_residual(T, iters):
    """(4, 30): every residual < 1e-2.  2 sweeps: the Newton's residual < 1e-2 on contact substeps; a contact-free residual above 1e-2 is
    the last sweep's change (stale), so those envs must match the oracle AND a 64-sweep solve from the same state within the free bound"""
    assert T.worst_res_contact < 1e-2
    if iters[0] >= 4:
        assert T.worst_res < 1e-2
    else:
        assert T.resolved == T.stale
        assert T.worst_dv_stale < 2e-6 and T.worst_dv_resolved < 2e-6
