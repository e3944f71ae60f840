// so100_closed_loop.hpp -- the closed-loop trajectory query: rollouts on the real dynamics under a time-varying feedback law around a nominal
// plan, u_t = u_nom_t + alpha k_t + K_t (x_t (-) x_nom_t), for L step sizes alpha per problem -- the nonlinear forward pass and the line-search
// candidates of iLQR, and LQR tracking from disturbed starts (include/so100_query.h, so100_query_closed_loop).
//
// Templated on the scalar like so100_trajectory.hpp: float in the kernel (so100_query_closed_loop.hip), double and float in the host twin
// (tests/_closedcheck).  No second copy of the physics or of the tangent: the only way to the physics is trajectory_cold / trajectory_step /
// trajectory_rollout, and x (-) x_nom is derivative_column(x, x_nom, r = 1) of so100_derivative.hpp.  The feedback enters through
// trajectory_rollout's Ctrl callback, which here reads the state the rollout holds.
//
// Src is where a rollout's inputs come from (global memory, LDS or host arrays):
//     void  stage(int t)                                    called by ALL rollouts of a wave together, before step t's reads (a cooperative load)
//     void  nominal(int t, T u[6], T k[6])                  the nominal controls and the feed-forward term of step t (k absent: zeros)
//     bool  starts_on_reference()                           no x_nom_0 was given: x_nom_0 is the start itself, dx_0 = 0 exactly
//     void  reference(int t, bool cube, T xq[13], T xv[12]) x_nom at the START of step t (row t - 1 of the plan's rollout; t = 0: x_nom_0);
//                                                           cube = false: only the arm rows (0..5 of each) are written
//     T     gain(int t, int j, int i)                       K_t[j][i], i in the nx of the call
#pragma once
#include "so100_derivative.hpp"

namespace so100 {

constexpr int CL_MAX_L = 16;                                 // SO100_CL_MAX_L
constexpr int CL_NU = 6;

// the tangent index of entry i of the nx-form's state: nx = 12 is the arm block, 0..5 and 12..17 (so100_lqr.hpp: lqr_idx)
template <int NX> SO100_HD constexpr int closed_loop_idx(int i) { return NX == 24 ? i : (i < 6 ? i : i + 6); }

template <typename T> struct ClosedLoopLaw { T alpha; bool clamp; T u_lo, u_hi; };

// The controls of step t from the state s the step starts from:  c_j = u_j + (alpha k_j + sum_i K_ji dx_i), i ascending, then the clamp.
// A gain, nominal control or reference value that is not finite makes c[0] NaN: trajectory_step then fails the rollout at this step.
template <typename T, int NX, class Src>
SO100_HD void closed_loop_control(int t, const TrajState<T>& s, const ClosedLoopLaw<T>& law, Src& src, T c[6]) {
    T u[6], k[6], dx[DERIV_NX];
    T z = T(0);                                              // x * 0 is NaN for NaN and for inf: the guard of trajectory_finite
    src.nominal(t, u, k);
    if (t == 0 && src.starts_on_reference()) {
#pragma unroll
        for (int i = 0; i < DERIV_NX; i++) dx[i] = T(0);
    } else {
        T qp[13], qv[12], xq[13], xv[12];
        trajectory_qpos_qvel(s, qp, qv);
        // nx = 12 never reads the reference's cube rows: the state's own stand in for them (their difference is not used)
#pragma unroll
        for (int i = 0; i < 13; i++) xq[i] = qp[i];
#pragma unroll
        for (int i = 0; i < 12; i++) xv[i] = qv[i];
        src.reference(t, NX == 24, xq, xv);
#pragma unroll
        for (int i = 0; i < 13; i++) z += xq[i]*T(0);
#pragma unroll
        for (int i = 0; i < 12; i++) z += xv[i]*T(0);
        derivative_column(qp, qv, xq, xv, T(1), dx);
    }
#pragma unroll
    for (int j = 0; j < CL_NU; j++) {
        T acc = trajectory_rounded(law.alpha*k[j]);
#pragma unroll
        for (int i = 0; i < NX; i++) {
            const T g = src.gain(t, j, i);
            z += g*T(0);
            acc += g*dx[closed_loop_idx<NX>(i)];
        }
        T v = u[j] + acc;
        if (law.clamp) { v = v < law.u_lo ? law.u_lo : v; v = v > law.u_hi ? law.u_hi : v; }
        c[j] = v;
        z += u[j]*T(0) + k[j]*T(0);
    }
    if (!(z == T(0))) c[0] = z;                              // z is NaN here
}

// One rollout.  emit(t, ok, s, step, c) is trajectory_rollout's emit with c = the controls applied at step t (meaningless where !ok).
// Returns the first step that failed (a non-finite start: 0), or -1.  Every rollout of a wave runs the same `steps` turns of the loop and
// calls src.stage() in each, whether it still advances or not.
template <typename T, class Src, class Emit>
SO100_HD int closed_loop_rollout(TrajState<T>& s, int nx, int steps, int mode, unsigned flags, int solver_iters, int contact_iters, int nsub,
                                 const ClosedLoopLaw<T>& law, Src& src, Emit emit) {
    T applied[6] = { T(0), T(0), T(0), T(0), T(0), T(0) };
    src.stage(0);
    return trajectory_rollout<T>(s, steps, mode, flags, solver_iters, contact_iters, nsub,
        [&](int t, T c[6]) {
            if (nx == 24) closed_loop_control<T, 24>(t, s, law, src, c);
            else          closed_loop_control<T, 12>(t, s, law, src, c);
#pragma unroll
            for (int j = 0; j < CL_NU; j++) applied[j] = c[j];
        },
        [&](int t, bool ok, const TrajState<T>& st, const TrajStep<T>& o) {
            emit(t, ok, st, o, applied);
            if (t + 1 < steps) src.stage(t + 1);
        });
}

}  // namespace so100
