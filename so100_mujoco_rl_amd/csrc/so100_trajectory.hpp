// so100_trajectory.hpp -- the trajectory query: where a state ends up under an open-loop control sequence (include/so100_query.h,
// so100_query_trajectory).  No task layer: no reward, TimeLimit, reset, RNG or curriculum motion of the cube.
//
// Templated on the scalar like so100_forward.hpp: float in the kernel (so100_query_trajectory.hip), double and float in the host twin
// (tests/_trajcheck).  No second copy of the model or of a solver: a control step makes the calls physics_substeps (so100_task.hpp) makes,
// in its order, with frame_skip = nsub -- substep_with_pads where a contact flag is set, else arm_substep and cube_substep -- and carries
// what that function carries: the warm starts (ff, fl, aw, cube.warm) and the Kahan rows from substep to substep and from step to step, the
// contact store and the active-set memory (zones) for one control step.
//
// One lane per problem, nothing shared between lanes, every loop with a fixed bound (steps, nsub, the solvers' iteration counts).
#pragma once
#include "so100_query.hpp"
#include "so100_contact.hpp"

namespace so100 {

constexpr int TRAJ_TARGETS = 0, TRAJ_ACTIONS = 1;                                  // SO100_TRAJ_TARGETS / SO100_TRAJ_ACTIONS
constexpr int TRAJ_MAX_T = 4096, TRAJ_MAX_NSUB = 1024, TRAJ_MAX_SUBSTEPS = 65536;  // SO100_TRAJ_MAX_*
constexpr float TRAJ_ACTION_SCALE = 0.075f;                                        // JOINT_STEP_SCALE (so100_task.hpp; ref: utils.py:9)

// x as a value of its own: the kernels are built with -ffp-contract=fast, which fuses a product into the sum that follows and honours no pragma;
// a canonicalised product is not a product any more (and costs no instruction: a product is canonical already).  The host twins are built
// without contraction.
SO100_HD float trajectory_rounded(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_canonicalizef(x);
#else
    return x;
#endif
}
SO100_HD double trajectory_rounded(double x) { return x; }

// the physics rows of an EnvState
template <typename T> struct TrajState {
    T q[6], v[6], qc[6], ff[6], fl[6], aw[6];
    Cube<T> cube;
    T lift;                    // force on the cube along +z: m g where the handle's anti-gravity bit is set, else 0
};
// what physics_substeps leaves in res / cstat / csig for one control step
template <typename T> struct TrajStep { T res; int cstat, csig; };

// a cold start from qpos [13] / qvel [12] (so100_get_state's layout), as a freshly reset env: no warm start, no force on the cube
template <typename T> SO100_HD void trajectory_cold(const T qpos[13], const T qvel[12], TrajState<T>& s) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
        s.q[i] = qpos[i]; s.v[i] = qvel[i]; s.qc[i] = T(0); s.ff[i] = T(0); s.fl[i] = T(0); s.aw[i] = T(0);
        s.cube.vel[i] = qvel[6 + i]; s.cube.warm[i] = T(0);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) s.cube.pos[i] = qpos[6 + i];
#pragma unroll
    for (int i = 0; i < 4; i++) s.cube.quat[i] = qpos[9 + i];
    s.lift = T(0);
}
template <typename T> SO100_HD void trajectory_qpos_qvel(const TrajState<T>& s, T qpos[13], T qvel[12]) {
#pragma unroll
    for (int i = 0; i < 6; i++) { qpos[i] = s.q[i]; qvel[i] = s.v[i]; qvel[6 + i] = s.cube.vel[i]; }
#pragma unroll
    for (int i = 0; i < 3; i++) qpos[6 + i] = s.cube.pos[i];
#pragma unroll
    for (int i = 0; i < 4; i++) qpos[9 + i] = s.cube.quat[i];
}

// x * 0 is NaN for NaN and for inf (and is not folded away under IEEE rules): the state guard of env_step_finish
template <typename T> SO100_HD bool trajectory_finite(const TrajState<T>& s) {
    T z = T(0);
#pragma unroll
    for (int i = 0; i < 6; i++) z += s.q[i]*T(0) + s.v[i]*T(0) + s.cube.vel[i]*T(0);
#pragma unroll
    for (int i = 0; i < 3; i++) z += s.cube.pos[i]*T(0);
#pragma unroll
    for (int i = 0; i < 4; i++) z += s.cube.quat[i]*T(0);
    return z == T(0);
}

// the reference's end-effector point at q: link_frames and link_point, as query_kinematics forms it
template <typename T> SO100_HD void trajectory_ee(const T q[6], T ee[3]) {
    Arm<T> A;
    arm_trig(q, A);
    LinkFrames<T> F;
    link_frames(A.s, A.c, F);
    const T o[3] = { T(EE_OFFSET[0]), T(EE_OFFSET[1]), T(EE_OFFSET[2]) };
    link_point(F, EE_LINK, o, ee);
}

// One control step: nsub substeps under the controls c (targets, or actions on the angles the step starts from).  Returns false where c is
// not finite (s is then untouched) or the state it arrives at is not.
template <typename T>
SO100_HD bool trajectory_step(TrajState<T>& s, const T c[6], int mode, unsigned flags, int solver_iters, int contact_iters, int nsub, TrajStep<T>& o) {
    T z = T(0);
#pragma unroll
    for (int i = 0; i < 6; i++) z += c[i]*T(0);
    o.res = T(0); o.cstat = 0; o.csig = 0;
    if (!(z == T(0))) return false;
    // a product rounded, then a sum rounded -- env_step_pre's e.q[i] + a[i]*JOINT_STEP_SCALE in plain IEEE arithmetic: the caller can form the same
    // targets from the rows of an earlier call
    T ctrl[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const T d = trajectory_rounded(c[i]*T(TRAJ_ACTION_SCALE));
        ctrl[i] = mode == TRAJ_ACTIONS ? s.q[i] + d : c[i];
    }
    // ---- physics_substeps (so100_task.hpp), frame_skip = nsub
    Arm<T> A;
    T dq[6] = { T(0), T(0), T(0), T(0), T(0), T(0) };
    const T applied[3] = { T(0), T(0), s.lift };
    const bool pads = (flags & F_ANY_CONTACT) != 0u;
    ContactsPriv<T> cs; int zones = -1;                      // the contact solve's active-set memory lives for this control step
#pragma unroll 1
    for (int k = 0; k < nsub; k++) {
        if (pads) {
            int st[4];
            substep_with_pads<T>(s.q, s.v, s.qc, ctrl, s.ff, s.fl, s.aw, s.cube, applied, flags, solver_iters, contact_iters, A, k == 0, dq, &o.res, cs, zones, st);
            const int n = o.cstat & 255, dr = o.cstat >> 8;
            o.cstat = (st[0] > n ? st[0] : n) | ((dr + st[2] > 0xFFFF ? 0xFFFF : dr + st[2]) << 8);
            o.csig = st[3];
        } else {
            arm_substep<T, false>(s.q, s.v, s.qc, ctrl, s.ff, s.fl, flags, solver_iters, A, k == 0, dq, &o.res);
            cube_substep<T>(s.cube, applied, flags, contact_iters);
        }
    }
    return trajectory_finite(s);
}

// The whole query for one problem.  ctrl(t, c[6]) reads step t's controls; emit(t, ok, s, step) is called once per step, in order: ok = the
// problem got through step t, s = the state after it.  From the first step that fails (a non-finite start counts as step 0's) the problem is
// not advanced any further.  Returns that step, or -1.
template <typename T, class Ctrl, class Emit>
SO100_HD int trajectory_rollout(TrajState<T>& s, int steps, int mode, unsigned flags, int solver_iters, int contact_iters, int nsub, Ctrl ctrl, Emit emit) {
    int bad = trajectory_finite(s) ? -1 : 0;
#pragma unroll 1
    for (int t = 0; t < steps; t++) {
        TrajStep<T> o; o.res = T(0); o.cstat = 0; o.csig = 0;
        if (bad < 0) {
            T c[6];
            ctrl(t, c);
            if (!trajectory_step(s, c, mode, flags, solver_iters, contact_iters, nsub, o)) bad = t;
        }
        emit(t, bad < 0, s, o);
    }
    return bad;
}

}  // namespace so100
