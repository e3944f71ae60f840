// closedcheck.cpp -- the closed-loop trajectory query of so100_closed_loop.hpp on the host, in double (held to the fp64 oracle) and in float (the
// arithmetic the kernel ships, without FMA contraction), behind a C interface for ctypes (built by tests/Makefile, loaded by tests/hostlibs.py and
// called by tests/closed_loop_support.py).  Arrays are problem-major here (qpos [n][13], u [T][n][6], references [T][n][k], k [T][n][6],
// K [T][n][6][nx]); outputs are rollout-major ([T][n L][k], rollout (m, a) at m L + a); the SoA layout is the kernel's matter.  warm: null for a
// cold start, or [n][31] as in trajcheck.cpp.  Test scaffolding only.
#include <stdint.h>
#include <limits>
#include "../../so100_mujoco_rl_amd/csrc/so100_closed_loop.hpp"

using namespace so100;

namespace {

template <typename T> struct HostSrc {
    long n, m; int nx;
    const T *u, *qpos_ref, *qvel_ref, *qpos_ref0, *qvel_ref0, *k, *K;
    void stage(int) {}
    void nominal(int t, T uu[6], T kk[6]) {
        for (int j = 0; j < 6; j++) { uu[j] = u[((long)t*n + m)*6 + j]; kk[j] = k ? k[((long)t*n + m)*6 + j] : T(0); }
    }
    bool starts_on_reference() { return qpos_ref0 == nullptr; }
    void reference(int t, bool cube, T xq[13], T xv[12]) {
        const T* q = t == 0 ? qpos_ref0 + 13*m : qpos_ref + ((long)(t - 1)*n + m)*13;
        const T* v = t == 0 ? qvel_ref0 + 12*m : qvel_ref + ((long)(t - 1)*n + m)*12;
        for (int i = 0; i < 13; i++) if (cube || i < 6) xq[i] = q[i];
        for (int i = 0; i < 12; i++) if (cube || i < 6) xv[i] = v[i];
    }
    T gain(int t, int j, int i) { return K[(((long)t*n + m)*6 + j)*nx + i]; }
};

// qvel, warm, the references (steps = 1), ref0 and k may be null.  Every output is required.
template <typename T> void closed_loop(long n, const T* qpos, const T* qvel, const T* warm, const T* u, int mode, int steps, int nsub, unsigned flags,
                                       int solver_iters, int contact_iters, const T* qpos_ref, const T* qvel_ref, const T* qpos_ref0, const T* qvel_ref0,
                                       int nx, const T* k, const T* K, int L, const T* alpha, int clamp, T u_lo, T u_hi,
                                       T* u_traj, T* qpos_traj, T* qvel_traj, T* ee_traj, T* qpos_final, T* qvel_final,
                                       int32_t* ncon, int32_t* dropped, int32_t* sig, T* residual, int32_t* bad_step) {
    const T nan = std::numeric_limits<T>::quiet_NaN();
    const long nl = n*L;
    for (long i = 0; i < nl; i++) {
        const long m = i/L; const int a = (int)(i - m*L);
        T v[12];
        for (int c = 0; c < 12; c++) v[c] = qvel ? qvel[12*m + c] : T(0);
        TrajState<T> s;
        trajectory_cold(qpos + 13*m, v, s);
        if (warm) {
            const T* w = warm + 31*m;
            for (int c = 0; c < 6; c++) { s.ff[c] = w[c]; s.fl[c] = w[6 + c]; s.cube.warm[c] = w[12 + c]; s.qc[c] = w[18 + c]; s.aw[c] = w[24 + c]; }
            s.lift = w[30];
        }
        HostSrc<T> src{ n, m, nx, u, qpos_ref, qvel_ref, qpos_ref0, qvel_ref0, k, K };
        const ClosedLoopLaw<T> law{ alpha[a], clamp != 0, u_lo, u_hi };
        const int bad = closed_loop_rollout<T>(s, nx, steps, mode, flags, solver_iters, contact_iters, nsub, law, src,
            [&](int t, bool ok, const TrajState<T>& st, const TrajStep<T>& o, const T c[6]) {
                const long r = (long)t*nl + i;
                T qp[13], qv[12], ee[3] = { nan, nan, nan };
                trajectory_qpos_qvel(st, qp, qv);
                if (ok) trajectory_ee(st.q, ee);
                for (int c2 = 0; c2 < 6; c2++) u_traj[6*r + c2] = ok ? c[c2] : nan;
                for (int c2 = 0; c2 < 13; c2++) qpos_traj[13*r + c2] = ok ? qp[c2] : nan;
                for (int c2 = 0; c2 < 12; c2++) qvel_traj[12*r + c2] = ok ? qv[c2] : nan;
                for (int c2 = 0; c2 < 3; c2++) ee_traj[3*r + c2] = ee[c2];
                ncon[r] = ok ? (o.cstat & 255) : 0; dropped[r] = ok ? (o.cstat >> 8) : 0; sig[r] = ok ? o.csig : 0; residual[r] = ok ? o.res : nan;
            });
        T qp[13], qv[12];
        trajectory_qpos_qvel(s, qp, qv);
        for (int c = 0; c < 13; c++) qpos_final[13*i + c] = bad < 0 ? qp[c] : nan;
        for (int c = 0; c < 12; c++) qvel_final[12*i + c] = bad < 0 ? qv[c] : nan;
        bad_step[i] = bad;
    }
}

}  // namespace

extern "C" {

#define CC_INSTANCE(S, T) \
    void cc_closed_loop_##S(long n, const T* qpos, const T* qvel, const T* warm, const T* u, int mode, int steps, int nsub, unsigned flags, \
                            int solver_iters, int contact_iters, const T* qpos_ref, const T* qvel_ref, const T* qpos_ref0, const T* qvel_ref0, \
                            int nx, const T* k, const T* K, int L, const T* alpha, int clamp, T u_lo, T u_hi, \
                            T* u_traj, T* qpos_traj, T* qvel_traj, T* ee_traj, T* qpos_final, T* qvel_final, \
                            int32_t* ncon, int32_t* dropped, int32_t* sig, T* residual, int32_t* bad_step) { \
        closed_loop<T>(n, qpos, qvel, warm, u, mode, steps, nsub, flags, solver_iters, contact_iters, qpos_ref, qvel_ref, qpos_ref0, qvel_ref0, nx, k, K, L, alpha, \
                       clamp, u_lo, u_hi, u_traj, qpos_traj, qvel_traj, ee_traj, qpos_final, qvel_final, ncon, dropped, sig, residual, bad_step); }
CC_INSTANCE(d, double)
CC_INSTANCE(f, float)
#undef CC_INSTANCE

}  // extern "C"

#ifdef CLOSEDCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions, both nx, both modes, a handful of arms in the air with a tumbling cube under PD-like
// gains and three step sizes: alpha = 0 on the plan's own rollout reproduces it, the clamp holds, and a NaN gain fails one problem's candidates only
#include <math.h>
#include <stdio.h>
#include <vector>
namespace {
uint32_t g_state = 2027u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0; }

template <typename T> int run(const char* name) {
    const long n = 3; const int steps = 3, nsub = 4, L = 3;
    const unsigned NOPADS = 1u | 2u | 4u;
    const T alpha[3] = { T(0), T(0.5), T(1) };
    int bad = 0; long rollouts = 0;
    for (int nx = 12; nx <= 24; nx += 12)
        for (int mode = 0; mode < 2; mode++) {
            std::vector<T> qpos(13*n), qvel(12*n), u(6*n*steps), k(6*n*steps), K(6*nx*n*steps, T(0));
            const double base[6] = { 0.0, -1.5, 1.5, 0.5, 0.0, 0.2 };
            for (long i = 0; i < n; i++) {
                for (int c = 0; c < 6; c++) { qpos[13*i + c] = T(base[c] + 0.04*(uniform() - 0.5)); qvel[12*i + c] = T(0.6*(uniform() - 0.5)); }
                qpos[13*i + 6] = T(0.2); qpos[13*i + 7] = T(-0.2); qpos[13*i + 8] = T(0.05);
                T qq[4] = { T(1), T(0.3*uniform()), T(0.3*uniform()), T(0.3*uniform()) };
                quat_normalize(qq);
                for (int c = 0; c < 4; c++) qpos[13*i + 9 + c] = qq[c];
                for (int c = 6; c < 12; c++) qvel[12*i + c] = T(0.2*(uniform() - 0.5));
            }
            for (int t = 0; t < steps; t++)
                for (long i = 0; i < n; i++)
                    for (int j = 0; j < 6; j++) {
                        const long p = (long)t*n + i;
                        u[6*p + j] = mode == TRAJ_ACTIONS ? T(uniform() - 0.5) : qpos[13*i + j] + T(0.15*(uniform() - 0.5));
                        k[6*p + j] = T(0.4*(uniform() - 0.5));
                        for (int c = 0; c < nx; c++) K[(6*p + j)*nx + c] = T(0.05*(uniform() - 0.5));
                        K[(6*p + j)*nx + j] = T(-2); K[(6*p + j)*nx + nx/2 + j] = T(-0.1);
                    }
            const long nl = n*L;
            std::vector<T> ut(6*nl*steps), qt(13*nl*steps), vt(12*nl*steps), et(3*nl*steps), qf(13*nl), vf(12*nl), res(nl*steps);
            std::vector<int32_t> ncon(nl*steps), drop(nl*steps), sig(nl*steps), bs(nl);
            // the plan's own rollout: K = 0, k = 0, one candidate (the reference is read all the same: the start, repeated)
            std::vector<T> rq(13*n*steps), rv(12*n*steps);
            for (int t = 0; t < steps; t++)
                for (long i = 0; i < n; i++) {
                    for (int c = 0; c < 13; c++) rq[((long)t*n + i)*13 + c] = qpos[13*i + c];
                    for (int c = 0; c < 12; c++) rv[((long)t*n + i)*12 + c] = qvel[12*i + c];
                }
            std::vector<T> zero(6*nx*n*steps, T(0)), u0(6*n*steps), q0(13*n*steps), v0(12*n*steps), e0(3*n*steps), qf0(13*n), vf0(12*n), res0(n*steps);
            std::vector<int32_t> i0(n*steps), i1(n*steps), i2(n*steps), bs0(n);
            closed_loop<T>(n, qpos.data(), qvel.data(), nullptr, u.data(), mode, steps, nsub, NOPADS, 4, 30, rq.data(), rv.data(), nullptr, nullptr, nx, nullptr,
                           zero.data(), 1, alpha + 2, 0, T(0), T(0), u0.data(), q0.data(), v0.data(), e0.data(), qf0.data(), vf0.data(), i0.data(), i1.data(), i2.data(),
                           res0.data(), bs0.data());
            for (long i = 0; i < n; i++) bad += bs0[i] != -1;
            for (size_t c = 0; c < u0.size(); c++) bad += !(u0[c] == u[c]);
            // three candidates around it, clamped; then with a NaN gain at step 1 of problem 1
            for (int pass = 0; pass < 2; pass++) {
                if (pass == 1) K[(6*(1*n + 1) + 2)*nx + 3] = std::numeric_limits<T>::quiet_NaN();
                const T lo = mode == TRAJ_ACTIONS ? T(-0.45) : T(-3), hi = mode == TRAJ_ACTIONS ? T(0.45) : T(3);
                closed_loop<T>(n, qpos.data(), qvel.data(), nullptr, u.data(), mode, steps, nsub, NOPADS, 4, 30, q0.data(), v0.data(), nullptr, nullptr, nx, k.data(),
                               K.data(), L, alpha, 1, lo, hi, ut.data(), qt.data(), vt.data(), et.data(), qf.data(), vf.data(), ncon.data(), drop.data(), sig.data(),
                               res.data(), bs.data());
                for (long i = 0; i < nl; i++) {
                    const long m = i/L;
                    const bool fails = pass == 1 && m == 1;
                    bad += bs[i] != (fails ? 1 : -1);
                    for (int t = 0; t < steps; t++) {
                        const long r = (long)t*nl + i;
                        const bool gone = fails && t >= 1;
                        for (int c = 0; c < 6; c++) bad += gone ? ut[6*r + c] == ut[6*r + c] : !(ut[6*r + c] >= lo && ut[6*r + c] <= hi);
                        for (int c = 0; c < 13; c++) {
                            bad += gone ? qt[13*r + c] == qt[13*r + c] : !(qt[13*r + c] == qt[13*r + c]);
                        }
                    }
                    if (pass == 0) rollouts++;
                }
            }
        }
    printf("closedcheck selftest (%s): %ld rollouts x 3 steps x 4 substeps: %s\n", name, rollouts, bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
