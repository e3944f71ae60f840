// derivcheck.cpp -- the derivatives query of so100_derivative.hpp on the host, in double (held to the fp64 oracle) and in float (the arithmetic
// the kernel ships, without FMA contraction), behind a C interface for ctypes (built by tests/Makefile, loaded by tests/hostlibs.py, called by
// tests/derivatives_support.py).  The same templates as the kernel, with a loop over the 61 roles where the kernel has lanes.  Arrays are
// problem-major (qpos [n][13], ctrl [n][6], A [n][24][24], B [n][24][6]); warm: null for a cold start, or [n][31] as in trajcheck.cpp.
// Test scaffolding only.
#include <stdint.h>
#include <limits>
#include "../../so100_mujoco_rl_amd/csrc/so100_derivative.hpp"

using namespace so100;

namespace {

// qvel null: zero.  Every output is required.
template <typename T> void derivatives(long n, const T* qpos, const T* qvel, const T* warm, const T* ctrl, int mode, int nsub, unsigned flags, int solver_iters,
                                       int contact_iters, T eps, T* A, T* B, T* qpos_next, T* qvel_next, int32_t* bad) {
    const T nan = std::numeric_limits<T>::quiet_NaN();
    const T r = T(0.5)/eps;
    for (long i = 0; i < n; i++) {
        T v[12];
        for (int k = 0; k < 12; k++) v[k] = qvel ? qvel[12*i + k] : T(0);
        TrajState<T> s0;
        trajectory_cold(qpos + 13*i, v, s0);
        if (warm) {
            const T* w = warm + 31*i;
            for (int k = 0; k < 6; k++) { s0.ff[k] = w[k]; s0.fl[k] = w[6 + k]; s0.cube.warm[k] = w[12 + k]; s0.qc[k] = w[18 + k]; s0.aw[k] = w[24 + k]; }
            s0.lift = w[30];
        }
        T qp[DERIV_NOMINAL + 1][13], qv[DERIV_NOMINAL + 1][12];
        bool any_bad = false;
        for (int role = 0; role <= DERIV_NOMINAL; role++) {      // the kernel: one lane each
            TrajState<T> s = s0;
            any_bad = !derivative_evaluate<T>(role, eps, s, ctrl + 6*i, mode, flags, solver_iters, contact_iters, nsub, qp[role], qv[role]) || any_bad;
        }
        for (int c = 0; c < DERIV_COLS; c++) {
            T col[DERIV_NX];
            derivative_column(qp[2*c], qv[2*c], qp[2*c + 1], qv[2*c + 1], r, col);
            for (int k = 0; k < DERIV_NX; k++) {
                if (c < DERIV_NX) A[(DERIV_NX*i + k)*DERIV_NX + c] = any_bad ? nan : col[k];
                else B[(DERIV_NX*i + k)*DERIV_NU + (c - DERIV_NX)] = any_bad ? nan : col[k];
            }
        }
        for (int k = 0; k < 13; k++) qpos_next[13*i + k] = any_bad ? nan : qp[DERIV_NOMINAL][k];
        for (int k = 0; k < 12; k++) qvel_next[12*i + k] = any_bad ? nan : qv[DERIV_NOMINAL][k];
        bad[i] = any_bad ? 1 : 0;
    }
}

}  // namespace

extern "C" {

#define DC_INSTANCE(S, T) \
    void dc_derivatives_##S(long n, const T* qpos, const T* qvel, const T* warm, const T* ctrl, int mode, int nsub, unsigned flags, int solver_iters, \
                            int contact_iters, T eps, T* A, T* B, T* qpos_next, T* qvel_next, int32_t* bad) { \
        derivatives<T>(n, qpos, qvel, warm, ctrl, mode, nsub, flags, solver_iters, contact_iters, eps, A, B, qpos_next, qvel_next, bad); }
DC_INSTANCE(d, double)
DC_INSTANCE(f, float)
#undef DC_INSTANCE

}  // extern "C"

#ifdef DERIVCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions over a few problems -- contact-free with a tumbling cube in the air, pads on the
// floor --, with velocities and with qvel null, in both modes; then a NaN control beside a clean neighbour
#include <stdio.h>
#include <vector>
namespace {
uint32_t g_state = 2026u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0; }

struct Case { double q[6], cube[3]; unsigned flags; };
const unsigned NOPADS = 1u | 2u | 4u, REFP = 1u | 2u | 4u | 16u;
const Case BASE[] = {
    { { 0.0, -1.5, 1.5, 0.5, 0.0, 0.2 }, { 0.2, -0.2, 0.05 }, NOPADS },      // the arm folded in the air, the cube falling
    { { 0.0, -3.0, 2.6, 1.2, 0.0, 0.3 }, { 0.15, -0.25, 0.0099 }, REFP },    // pads near the floor, the cube resting
};

template <typename T> int run(const char* name) {
    const long per = 4, nb = (long)(sizeof BASE/sizeof BASE[0]);
    const int nsub = 2;
    const T eps = T(1.0/256);
    int bad = 0; long n = 0;
    for (long b = 0; b < nb; b++) {
        std::vector<T> qpos(13*per), qvel(12*per), ctrl(6*per), A(576*per), B(144*per), A2(576*per), B2(144*per), qn(13*per), vn(12*per);
        std::vector<int32_t> flag(per);
        for (long i = 0; i < per; i++) {
            for (int k = 0; k < 6; k++) { qpos[13*i + k] = T(BASE[b].q[k] + 0.04*(uniform() - 0.5)); qvel[12*i + k] = T(0.6*(uniform() - 0.5)); }
            for (int k = 0; k < 3; k++) qpos[13*i + 6 + k] = T(BASE[b].cube[k]);
            T qq[4] = { T(1), T(0.3*uniform()), T(0.3*uniform()), T(0.3*uniform()) };
            if (b == 1) qq[1] = qq[2] = qq[3] = T(0);
            quat_normalize(qq);
            for (int k = 0; k < 4; k++) qpos[13*i + 9 + k] = qq[k];
            for (int k = 6; k < 12; k++) qvel[12*i + k] = b == 0 ? T(0.2*(uniform() - 0.5)) : T(0);
        }
        for (int pass = 0; pass < 3; pass++) {              // actions; actions with qvel null; targets
            const int mode = pass == 2 ? TRAJ_TARGETS : TRAJ_ACTIONS;
            for (long i = 0; i < per; i++)
                for (int k = 0; k < 6; k++) ctrl[6*i + k] = mode == TRAJ_ACTIONS ? T(2.0*(uniform() - 0.5)) : qpos[13*i + k] + T(0.15*(uniform() - 0.5));
            derivatives<T>(per, qpos.data(), pass == 1 ? nullptr : qvel.data(), nullptr, ctrl.data(), mode, nsub, BASE[b].flags, 4, 30, eps, A.data(), B.data(),
                           qn.data(), vn.data(), flag.data());
            derivatives<T>(per, qpos.data(), pass == 1 ? nullptr : qvel.data(), nullptr, ctrl.data(), mode, nsub, BASE[b].flags, 4, 30, eps, A2.data(), B2.data(),
                           qn.data(), vn.data(), flag.data());
            for (long i = 0; i < per; i++) {
                bad += flag[i] != 0;
                for (int k = 0; k < 576; k++) bad += !(A[576*i + k] == A2[576*i + k]);          // finite, and the same on a second call
                for (int k = 0; k < 144; k++) bad += !(B[144*i + k] == B2[144*i + k]);
                for (int k = 0; k < 13; k++) bad += !(qn[13*i + k] == qn[13*i + k]);
                if (pass == 0) n++;
            }
        }
        // a NaN control in problem 1: bad = 1 and NaN there, the neighbours as before
        ctrl[6*1 + 2] = std::numeric_limits<T>::quiet_NaN();
        derivatives<T>(per, qpos.data(), qvel.data(), nullptr, ctrl.data(), TRAJ_TARGETS, nsub, BASE[b].flags, 4, 30, eps, A2.data(), B2.data(), qn.data(), vn.data(),
                       flag.data());
        derivatives<T>(per, qpos.data(), nullptr, nullptr, ctrl.data(), TRAJ_TARGETS, nsub, BASE[b].flags, 4, 30, eps, A.data(), B.data(), qn.data(), vn.data(), flag.data());
        bad += flag[0] != 0 || flag[1] != 1 || flag[2] != 0;
        for (int k = 0; k < 576; k++) bad += (A[576 + k] == A[576 + k]) + !(A[k] == A[k]) + !(A[2*576 + k] == A[2*576 + k]);
        for (int k = 0; k < 13; k++) bad += qn[13 + k] == qn[13 + k];
    }
    printf("derivcheck selftest (%s): %ld problems x 61 evaluations x %d substeps: %s\n", name, n, nsub, bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
