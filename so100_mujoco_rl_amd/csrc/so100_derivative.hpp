// so100_derivative.hpp -- the derivatives query: the linearisation A = dx'/dx, B = dx'/du of one control step by centred finite differences,
// what MuJoCo's users get from mjd_transitionFD (include/so100_query.h, so100_query_derivatives).
//
// Templated on the scalar like so100_trajectory.hpp: float in the kernel (so100_query_derivative.hip), double and float in the host twin
// (tests/_derivcheck).  No second copy of the model or of a solver: the only way to the physics is trajectory_cold / trajectory_step.
//
// Tangent state x = (dq [12], v [12]) in MuJoCo's dof order: arm 6, cube linear 3 (world frame), cube angular 3 (BODY frame), the same order
// for the position tangent and for qvel; u = the 6 controls of the step.  61 evaluations per problem, numbered by ROLE: for column c in 0..29
// role 2c is +eps and role 2c + 1 is -eps (columns 0..11 position, 12..23 velocity, 24..29 control); roles 60 and up are the unperturbed
// problem.  In the kernel a role is a lane of the problem's wave, in the twin a turn of a loop.
#pragma once
#include <math.h>
#include "so100_trajectory.hpp"

namespace so100 {

constexpr int DERIV_NX = 24, DERIV_NU = 6;                   // SO100_DERIV_NX / SO100_DERIV_NU
constexpr int DERIV_COLS = DERIV_NX + DERIV_NU;              // 30 columns, 60 perturbed roles
constexpr int DERIV_NOMINAL = 2*DERIV_COLS;                  // the first unperturbed role
constexpr float DERIV_EPS = 0.015625f;                       // SO100_DERIV_EPS = 2^-6

SO100_HD float  tatan2(float y, float x)   { return atan2f(y, x); }
SO100_HD double tatan2(double y, double x) { return atan2(y, x); }

// r = a (x) b
template <typename T> SO100_HD void quat_product(const T a[4], const T b[4], T r[4]) {
    r[0] = a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3];
    r[1] = a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2];
    r[2] = a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1];
    r[3] = a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0];
}

// The start and the controls of role `role`.  Every component but the cube's orientation: one rounded add, x +- eps (the components that are
// not perturbed keep their bits: they are selected, not added to).  The cube's orientation, columns 9..11: quat <- normalize(quat (x)
// (cos(eps/2), +-sin(eps/2) e_i)), mj_integratePos on a free joint, in the body frame.  No index of an array depends on the role.
template <typename T> SO100_HD void derivative_perturb(int role, T eps, TrajState<T>& s, T c[6]) {
    const int col = role >> 1;
    const T d = (role & 1) ? -eps : eps;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        s.q[k] = col == k ? s.q[k] + d : s.q[k];
        s.v[k] = col == 12 + k ? s.v[k] + d : s.v[k];
        s.cube.vel[k] = col == 18 + k ? s.cube.vel[k] + d : s.cube.vel[k];
        c[k] = col == 24 + k ? c[k] + d : c[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) s.cube.pos[k] = col == 6 + k ? s.cube.pos[k] + d : s.cube.pos[k];
    if (col >= 9 && col < 12) {
        T sn, cs;
        tsincos<T>(T(0.5)*eps, sn, cs);
        const T sd = (role & 1) ? -sn : sn;
        const T r[4] = { cs, col == 9 ? sd : T(0), col == 10 ? sd : T(0), col == 11 ? sd : T(0) };
        T q[4];
        quat_product(s.cube.quat, r, q);
        quat_normalize(q);
#pragma unroll
        for (int k = 0; k < 4; k++) s.cube.quat[k] = q[k];
    }
}

// One role's evaluation: the control step from the (perturbed) start s under the (perturbed) controls.  Returns false where the start, the
// controls or the state it arrives at are not finite.
template <typename T>
SO100_HD bool derivative_evaluate(int role, T eps, TrajState<T>& s, const T ctrl[6], int mode, unsigned flags, int solver_iters, int contact_iters, int nsub,
                                  T qpos[13], T qvel[12]) {
    T c[6];
#pragma unroll
    for (int k = 0; k < 6; k++) c[k] = ctrl[k];
    derivative_perturb(role, eps, s, c);
    bool ok = trajectory_finite(s);
    if (ok) {
        TrajStep<T> o;
        ok = trajectory_step(s, c, mode, flags, solver_iters, contact_iters, nsub, o);
    }
    trajectory_qpos_qvel(s, qpos, qvel);
    return ok;
}

// One column of (A | B) from the two next states of its +- pair, r = 1/(2 eps).  Every row but the cube's rotation rows: (y+ - y-) r, one
// rounded subtraction and one rounded product.  Rows 9..11: the rotation vector of (quat-)^-1 (x) quat+ (mju_subQuat, body frame) times r.
template <typename T>
SO100_HD void derivative_column(const T qp[13], const T vp[12], const T qm[13], const T vm[12], T r, T col[DERIV_NX]) {
#pragma unroll
    for (int k = 0; k < 9; k++) col[k] = (qp[k] - qm[k])*r;
#pragma unroll
    for (int k = 0; k < 12; k++) col[12 + k] = (vp[k] - vm[k])*r;
    const T inv[4] = { qm[9], -qm[10], -qm[11], -qm[12] };
    T d[4];
    quat_product(inv, qp + 9, d);
    // mju_quat2Vel: axis = d[1..3] / |d[1..3]|, angle = 2 atan2(|d[1..3]|, d[0]), taken into (-pi, pi]
    const T sn = tsqrt(d[1]*d[1] + d[2]*d[2] + d[3]*d[3]);
    T angle = T(2)*tatan2(sn, d[0]);
    if (angle > T(3.14159265358979323846)) angle -= T(2*3.14159265358979323846);
    const T scale = sn < T(1e-15) ? T(0) : angle*trcp(sn);
#pragma unroll
    for (int k = 0; k < 3; k++) col[9 + k] = (d[1 + k]*scale)*r;
}

}  // namespace so100
