// trajcheck.cpp -- the trajectory query of so100_trajectory.hpp on the host, in double (held to the fp64 oracle) and in float (the arithmetic
// the kernel ships, without FMA contraction), behind a C interface for ctypes (built by tests/Makefile, loaded by tests/hostlibs.py, called by
// tests/trajectory_support.py).  Arrays are problem-major here (qpos [n][13], ctrl [T][n][6], trajectories [T][n][k]); the SoA layout is the
// kernel's matter.  warm: null for a cold start, or [n][31] = ff 6, fl 6, cube.warm 6, qc 6, aw 6, lift 1 (the rows the kernel reads from a handle).
// Test scaffolding only.
#include <stdint.h>
#include <limits>
#include "../../so100_mujoco_rl_amd/csrc/so100_trajectory.hpp"

using namespace so100;

namespace {

// qvel null: zero.  Every output is required.
template <typename T> void trajectory(long n, const T* qpos, const T* qvel, const T* warm, const T* ctrl, int mode, int steps, int nsub, unsigned flags,
                                      int solver_iters, int contact_iters, T* qpos_traj, T* qvel_traj, T* ee_traj, T* qpos_final, T* qvel_final,
                                      int32_t* ncon, int32_t* dropped, int32_t* sig, T* residual, int32_t* bad_step) {
    const T nan = std::numeric_limits<T>::quiet_NaN();
    for (long i = 0; i < n; i++) {
        T v[12];
        for (int k = 0; k < 12; k++) v[k] = qvel ? qvel[12*i + k] : T(0);
        TrajState<T> s;
        trajectory_cold(qpos + 13*i, v, s);
        if (warm) {
            const T* w = warm + 31*i;
            for (int k = 0; k < 6; k++) { s.ff[k] = w[k]; s.fl[k] = w[6 + k]; s.cube.warm[k] = w[12 + k]; s.qc[k] = w[18 + k]; s.aw[k] = w[24 + k]; }
            s.lift = w[30];
        }
        const int bad = trajectory_rollout<T>(s, steps, mode, flags, solver_iters, contact_iters, nsub,
            [&](int t, T c[6]) { for (int k = 0; k < 6; k++) c[k] = ctrl[((long)t*n + i)*6 + k]; },
            [&](int t, bool ok, const TrajState<T>& st, const TrajStep<T>& o) {
                const long r = (long)t*n + i;
                T qp[13], qv[12], ee[3] = { nan, nan, nan };
                trajectory_qpos_qvel(st, qp, qv);
                if (ok) trajectory_ee(st.q, ee);
                for (int k = 0; k < 13; k++) qpos_traj[13*r + k] = ok ? qp[k] : nan;
                for (int k = 0; k < 12; k++) qvel_traj[12*r + k] = ok ? qv[k] : nan;
                for (int k = 0; k < 3; k++) ee_traj[3*r + k] = ee[k];
                ncon[r] = ok ? (o.cstat & 255) : 0; dropped[r] = ok ? (o.cstat >> 8) : 0; sig[r] = ok ? o.csig : 0; residual[r] = ok ? o.res : nan;
            });
        T qp[13], qv[12];
        trajectory_qpos_qvel(s, qp, qv);
        for (int k = 0; k < 13; k++) qpos_final[13*i + k] = bad < 0 ? qp[k] : nan;
        for (int k = 0; k < 12; k++) qvel_final[12*i + k] = bad < 0 ? qv[k] : nan;
        bad_step[i] = bad;
    }
}

}  // namespace

extern "C" {

#define TC_INSTANCE(S, T) \
    void tc_trajectory_##S(long n, const T* qpos, const T* qvel, const T* warm, const T* ctrl, int mode, int steps, int nsub, unsigned flags, \
                           int solver_iters, int contact_iters, T* qpos_traj, T* qvel_traj, T* ee_traj, T* qpos_final, T* qvel_final, \
                           int32_t* ncon, int32_t* dropped, int32_t* sig, T* residual, int32_t* bad_step) { \
        trajectory<T>(n, qpos, qvel, warm, ctrl, mode, steps, nsub, flags, solver_iters, contact_iters, qpos_traj, qvel_traj, ee_traj, qpos_final, qvel_final, \
                      ncon, dropped, sig, residual, bad_step); }
TC_INSTANCE(d, double)
TC_INSTANCE(f, float)
#undef TC_INSTANCE

}  // extern "C"

#ifdef TRAJCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions over a few dozen problems -- contact-free, pads on the floor, the jaw closed on the
// cube --, each with its velocities and with qvel null, in both modes; then a NaN control in the middle of a sequence
#include <math.h>
#include <stdio.h>
#include <vector>
namespace {
uint32_t g_state = 2025u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0; }

struct Case { double q[6], cube[3]; unsigned flags; bool grasp, contact; };
const unsigned ROWS = 1u | 2u | 8u, REFP = 1u | 2u | 4u | 16u, C5 = REFP | 32u;
// (1) the arm folded up in the air, the cube pinned; (2) pads near the floor; (3) tests/scenes.grasp_state: the cube between the jaws
const Case BASE[] = {
    { { 0.0, -1.9, 1.6, 0.3, 1.5708, 0.1 }, { 0.15, -0.25, 0.0099 }, ROWS, false, false },
    { { 0.0, -3.0, 2.6, 1.2, 0.0, 0.3 }, { 0.15, -0.25, 0.0099 }, REFP, false, true },
    { { 0.0, -1.9, 1.6, 0.3, 1.5708, 0.1 }, { 0.0, 0.0, 0.0 }, C5, true, true },
};

template <typename T> int run(const char* name) {
    const long per = 12, nb = (long)(sizeof BASE/sizeof BASE[0]);
    const int steps = 3, nsub = 4;
    int bad = 0; long in_contact = 0, n = 0;
    for (long b = 0; b < nb; b++) {
        std::vector<T> qpos(13*per), qvel(12*per), ctrl(6*per*steps), qt(13*per*steps), vt(12*per*steps), et(3*per*steps), qf(13*per), vf(12*per), res(per*steps);
        std::vector<int32_t> ncon(per*steps), drop(per*steps), sig(per*steps), bs(per);
        for (long i = 0; i < per; i++) {
            for (int k = 0; k < 6; k++) { qpos[13*i + k] = T(BASE[b].q[k] + 0.04*(uniform() - 0.5)); qvel[12*i + k] = T(0.6*(uniform() - 0.5)); }
            if (BASE[b].grasp) {                            // the cube between the jaws: 88 mm along the fixed jaw's -y, found from the pose itself
                Arm<T> A; WorldFK<T> W; arm_trig(&qpos[13*i], A); world_fk(A.s, A.c, W);
                const T o[3] = { T(-0.0026), T(-0.088), T(0) };
                for (int k = 0; k < 3; k++) qpos[13*i + 6 + k] = W.o[4][k] + W.R4[3*k]*o[0] + W.R4[3*k + 1]*o[1] + W.R4[3*k + 2]*o[2] + T(0.002*(uniform() - 0.5));
                qpos[13*i + 9] = T(0); qpos[13*i + 10] = T(0.02); qpos[13*i + 11] = T(1); qpos[13*i + 12] = T(0.01);
                qpos[13*i + 5] = T(0.06 + 0.02*uniform());
            } else {
                for (int k = 0; k < 3; k++) qpos[13*i + 6 + k] = T(BASE[b].cube[k] + (k < 2 ? 0.02*(uniform() - 0.5) : 0.0));
                qpos[13*i + 9] = T(1); qpos[13*i + 10] = qpos[13*i + 11] = qpos[13*i + 12] = T(0);
            }
            for (int k = 6; k < 12; k++) qvel[12*i + k] = T(0.02*(uniform() - 0.5));
        }
        for (int pass = 0; pass < 3; pass++) {              // actions; actions with qvel null; targets
            const int mode = pass == 2 ? TRAJ_TARGETS : TRAJ_ACTIONS;
            for (int t = 0; t < steps; t++)
                for (long i = 0; i < per; i++)
                    for (int k = 0; k < 6; k++) ctrl[((long)t*per + i)*6 + k] = mode == TRAJ_ACTIONS ? T(2.0*(uniform() - 0.5)) : qpos[13*i + k] + T(0.15*(uniform() - 0.5));
            trajectory<T>(per, qpos.data(), pass == 1 ? nullptr : qvel.data(), nullptr, ctrl.data(), mode, steps, nsub, BASE[b].flags, 4, 30, qt.data(), vt.data(),
                          et.data(), qf.data(), vf.data(), ncon.data(), drop.data(), sig.data(), res.data(), bs.data());
            for (long i = 0; i < per; i++) {
                bad += bs[i] != -1;
                for (int k = 0; k < 13; k++) bad += !(qf[13*i + k] == qt[13*((long)(steps - 1)*per + i) + k]);
                for (int k = 0; k < 12; k++) bad += !(vf[12*i + k] == vt[12*((long)(steps - 1)*per + i) + k]);
                bool touched = false;
                for (int t = 0; t < steps; t++) {
                    const long r = (long)t*per + i;
                    bad += ncon[r] < 0 || ncon[r] > MAXC || drop[r] < 0 || !(res[r] == res[r]) || (ncon[r] == 0 && sig[r] != 0);
                    for (int k = 0; k < 3; k++) bad += !(et[3*r + k] == et[3*r + k]);
                    touched = touched || ncon[r] > 0;
                }
                if (pass == 0) { in_contact += touched; n++; bad += !BASE[b].contact && touched; }
            }
        }
    }
    // a NaN control at step 1 of 3: bad_step = 1, row 0 as without it, rows 1 and 2 NaN / 0, the neighbour untouched
    {
        const long per2 = 2;
        std::vector<T> qpos(13*per2, T(0)), ctrl(6*per2*steps, T(0.1)), qt(13*per2*steps), vt(12*per2*steps), et(3*per2*steps), qf(13*per2), vf(12*per2), res(per2*steps);
        std::vector<T> qt0(13*per2*steps), vt0(12*per2*steps);
        std::vector<int32_t> ncon(per2*steps), drop(per2*steps), sig(per2*steps), bs(per2);
        for (long i = 0; i < per2; i++) { for (int k = 0; k < 6; k++) qpos[13*i + k] = T(BASE[1].q[k]); qpos[13*i + 6] = T(0.15); qpos[13*i + 7] = T(-0.25); qpos[13*i + 8] = T(0.0099); qpos[13*i + 9] = T(1); }
        trajectory<T>(per2, qpos.data(), nullptr, nullptr, ctrl.data(), TRAJ_ACTIONS, steps, nsub, REFP, 4, 30, qt0.data(), vt0.data(), et.data(), qf.data(), vf.data(),
                      ncon.data(), drop.data(), sig.data(), res.data(), bs.data());
        ctrl[(1*per2 + 0)*6 + 2] = T(NAN);
        trajectory<T>(per2, qpos.data(), nullptr, nullptr, ctrl.data(), TRAJ_ACTIONS, steps, nsub, REFP, 4, 30, qt.data(), vt.data(), et.data(), qf.data(), vf.data(),
                      ncon.data(), drop.data(), sig.data(), res.data(), bs.data());
        bad += bs[0] != 1 || bs[1] != -1;
        for (int k = 0; k < 13; k++) {
            bad += !(qt[13*0 + k] == qt0[13*0 + k]);                                   // problem 0, row 0
            bad += qt[13*(1*per2) + k] == qt[13*(1*per2) + k] || qt[13*(2*per2) + k] == qt[13*(2*per2) + k] || qf[k] == qf[k];
            for (int t = 0; t < steps; t++) bad += !(qt[13*(t*per2 + 1) + k] == qt0[13*(t*per2 + 1) + k]);      // problem 1, every row
        }
        bad += ncon[1*per2] != 0 || sig[2*per2] != 0 || res[1*per2] == res[1*per2];
    }
    bad += in_contact < n/4;
    printf("trajcheck selftest (%s): %ld problems x %d steps x %d substeps, %ld in contact: %s\n", name, n, steps, nsub, in_contact, bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
