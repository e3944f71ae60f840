// so100_query.hpp -- model queries (include/so100_query.h): per-problem arithmetic of the four query kernels, one GPU lane per problem.
//
// Nothing here restates the model: the poses come from fk_link / task_poses, the mass matrix and the bias force from arm_trig /
// arm_mass / arm_bias (so100_physics.hpp) -- the same templates the step kernels instantiate.  What is new is what a query adds on
// top: the six link poses kept (not only the ones the task reads), the point Jacobian in mj_jac's convention, the packed mass matrix
// unfolded, M qacc + bias, and the damped-least-squares iteration of so100_query_ik.
//
// Templated on the scalar T: float on the device; float / double host instantiations exist ONLY for the CPU-side tests in
// tests/_querycheck (never linked into libso100sim.so).  The link and the offset of a point are uniform over a call; the link is a
// run-time value, so every loop over links is fully unrolled and picks with `k == link` / `k <= link` (an index into a register array
// would send it to scratch memory).
#pragma once
#include "so100_physics.hpp"

namespace so100 {

constexpr int EE_LINK = 4;                               // the reference's end-effector point: on Fixed_Jaw ...
constexpr double EE_OFFSET[3] = { 0.0, (double)-0.1f, 0.0 };      // ... 10 cm along its -y axis; the reference's local point is a float32 array
                                                                  // (so100_task.hpp reads the same point with -0.1f)

// world pose of the six link frames: pos[k] = xpos, R[k] = xmat (row-major) of link k
template <typename T> struct LinkFrames { T pos[6][3], R[6][9]; };
template <int K, typename T> SO100_HD void link_frames_step(const T s[6], const T c[6], T pos[3], T R[9], LinkFrames<T>& F) {
    fk_link<K, false>(s, c, pos, R);
#pragma unroll
    for (int i = 0; i < 3; i++) F.pos[K][i] = pos[i];
#pragma unroll
    for (int i = 0; i < 9; i++) F.R[K][i] = R[i];
}
template <typename T> SO100_HD void link_frames(const T s[6], const T c[6], LinkFrames<T>& F) {
    T pos[3] = { T(0), T(0), T(0) };
    T R[9] = { T(1), T(0), T(0), T(0), T(1), T(0), T(0), T(0), T(1) };
    link_frames_step<0>(s, c, pos, R, F); link_frames_step<1>(s, c, pos, R, F); link_frames_step<2>(s, c, pos, R, F);
    link_frames_step<3>(s, c, pos, R, F); link_frames_step<4>(s, c, pos, R, F); link_frames_step<5>(s, c, pos, R, F);
}

// p = pos_L + R_L o: the point fixed to link L at offset o of that link's frame
template <typename T> SO100_HD void link_point(const LinkFrames<T>& F, int L, const T o[3], T p[3]) {
    p[0] = p[1] = p[2] = T(0);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        if (k == L) {
#pragma unroll
            for (int i = 0; i < 3; i++) p[i] = F.pos[k][i] + F.R[k][3*i]*o[0] + F.R[k][3*i+1]*o[1] + F.R[k][3*i+2]*o[2];
        }
    }
}

// mj_jac of that point: column k of jacr is joint k's axis in the world, of jacp axis_k x (p - anchor_k) (the anchor is the link
// origin: joint pos = 0, so100_model_def.h); the joints behind link L do not move the point: zero columns.  jacp / jacr: [3][6]
template <typename T> SO100_HD void point_jacobian(const LinkFrames<T>& F, int L, const T p[3], T jacp[18], T jacr[18]) {
    constexpr int AX[6] = { so100g::LINK_AXIS[0], so100g::LINK_AXIS[1], so100g::LINK_AXIS[2], so100g::LINK_AXIS[3], so100g::LINK_AXIS[4], so100g::LINK_AXIS[5] };
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const bool on = k <= L;
        const T z[3] = { F.R[k][AX[k]], F.R[k][3 + AX[k]], F.R[k][6 + AX[k]] };
        const T d[3] = { p[0] - F.pos[k][0], p[1] - F.pos[k][1], p[2] - F.pos[k][2] };
        T jp[3];
        cross(z, d, jp);
#pragma unroll
        for (int i = 0; i < 3; i++) { jacp[6*i + k] = on ? jp[i] : T(0); jacr[6*i + k] = on ? z[i] : T(0); }
    }
}

// ---- kinematics ---------------------------------------------------------------------------------------------------------------
template <typename T> struct QueryPoses { LinkFrames<T> F; T ee[3], cam_pos[3], cam_mat[9]; };
template <typename T> SO100_HD void query_kinematics(const T q[6], QueryPoses<T>& Q) {
    Arm<T> A;
    arm_trig(q, A);
    link_frames(A.s, A.c, Q.F);
    const T o[3] = { T(EE_OFFSET[0]), T(EE_OFFSET[1]), T(EE_OFFSET[2]) };
    link_point(Q.F, EE_LINK, o, Q.ee);
    TaskPoses<T> P;
    task_poses(A.s, A.c, true, P);                        // the camera as the task and the renderer place it
#pragma unroll
    for (int i = 0; i < 3; i++) Q.cam_pos[i] = P.cam_pos[i];
#pragma unroll
    for (int i = 0; i < 9; i++) Q.cam_mat[i] = P.cam_mat[i];
}

template <typename T> SO100_HD void query_jacobian(const T q[6], int L, const T o[3], T jacp[18], T jacr[18]) {
    Arm<T> A;
    arm_trig(q, A);
    LinkFrames<T> F;
    link_frames(A.s, A.c, F);
    T p[3];
    link_point(F, L, o, p);
    point_jacobian(F, L, p, jacp, jacr);
}

// ---- dynamics -----------------------------------------------------------------------------------------------------------------
// Mfull [36]: the packed lower triangle of arm_mass unfolded (armature on the diagonal, as MuJoCo's qM has it); bias [6];
// tau = M qacc + bias where qacc is given (nullptr: tau is left alone)
template <typename T> SO100_HD void query_dynamics(const T q[6], const T v[6], const T* qacc, T Mfull[36], T bias[6], T tau[6]) {
    Arm<T> A;
    arm_trig(q, A);
    arm_bias(v, A);
    arm_mass(A);
#pragma unroll
    for (int i = 0; i < 6; i++) {
        bias[i] = A.bias[i];
#pragma unroll
        for (int j = 0; j < 6; j++) Mfull[6*i + j] = sym6(A.M, i, j);
    }
    if (qacc) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            T t = A.bias[i];
#pragma unroll
            for (int j = 0; j < 6; j++) t += sym6(A.M, i, j)*qacc[j];
            tau[i] = t;
        }
    }
}

// ---- inverse kinematics ---------------------------------------------------------------------------------------------------------
// y = A^-1 e for a symmetric positive definite 3 x 3 (xx, yy, zz, xy, xz, yz): LDL^T like ldl6
template <typename T> SO100_HD void spd3_solve(const T A[6], const T e[3], T y[3]) {
    const T i0 = trcp(A[0]);
    const T l10 = A[3]*i0, l20 = A[4]*i0;
    const T d1 = A[1] - l10*A[3];
    const T i1 = trcp(d1);
    const T l21 = (A[5] - l20*A[3])*i1;
    const T d2 = A[2] - l20*A[4] - l21*l21*d1;
    const T i2 = trcp(d2);
    const T z1 = e[1] - l10*e[0];
    const T z2 = e[2] - l20*e[0] - l21*z1;
    y[2] = z2*i2;
    y[1] = z1*i1 - l21*y[2];
    y[0] = e[0]*i0 - l10*y[1] - l20*y[2];
}

template <typename T> struct IkParams { int link, iters; T o[3], damping2, tol, max_step; };
template <typename T> struct IkResult { T q[6], residual; int iterations; bool converged; };

// the iteration of include/so100_query.h; columns k > link of the Jacobian are zero, so those joints get dq = 0 and add nothing to J J'
template <typename T> SO100_HD void query_ik(const T q0[6], const T target[3], const IkParams<T>& P, IkResult<T>& out) {
    T q[6];
#pragma unroll
    for (int k = 0; k < 6; k++) q[k] = k <= P.link ? tclamp(q0[k], T(so100g::JNT_RANGE[k][0]), T(so100g::JNT_RANGE[k][1])) : q0[k];
    T r;
    int it = 0;
    for (;; it++) {
        Arm<T> A;
        arm_trig(q, A);
        LinkFrames<T> F;
        link_frames(A.s, A.c, F);
        T p[3];
        link_point(F, P.link, P.o, p);
        const T e[3] = { target[0] - p[0], target[1] - p[1], target[2] - p[2] };
        r = tsqrt(dot(e, e));
        if (r <= P.tol || it >= P.iters) break;
        T jp[18], jr[18];
        point_jacobian(F, P.link, p, jp, jr);
        T S[6];                                            // J J' + damping^2 I
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a; b < 3; b++) {
                T t = a == b ? P.damping2 : T(0);
#pragma unroll
                for (int k = 0; k < 6; k++) t += jp[6*a + k]*jp[6*b + k];
                S[sym_idx(a, b)] = t;
            }
        T y[3], dq[6], big = T(0);
        spd3_solve(S, e, y);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            dq[k] = jp[k]*y[0] + jp[6 + k]*y[1] + jp[12 + k]*y[2];
            big = tmax(big, tabs(dq[k]));
        }
        const T sc = big > P.max_step ? P.max_step*trcp(big) : T(1);
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (k <= P.link) q[k] = tclamp(q[k] + sc*dq[k], T(so100g::JNT_RANGE[k][0]), T(so100g::JNT_RANGE[k][1]));
    }
#pragma unroll
    for (int k = 0; k < 6; k++) out.q[k] = q[k];
    out.residual = r; out.iterations = it; out.converged = r <= P.tol;
}

}  // namespace so100
