// querycheck.cpp -- the model queries of so100_query.hpp on the host, in double (held to the fp64 oracle) and in float (the arithmetic
// the kernels ship, without FMA contraction), behind a C interface for ctypes (tests/hostlibs.py; called by tests/query_support.py).  Arrays are problem-major here
// ([n][k]: one problem's components together); the SoA layout is the kernels' matter.  Test scaffolding only.
#include <stdint.h>
#include "../../so100_mujoco_rl_amd/csrc/so100_query.hpp"

using namespace so100;

namespace {

template <typename T> void kinematics(long n, const T* q, T* xpos, T* xmat, T* ee, T* cam_pos, T* cam_mat) {
    for (long i = 0; i < n; i++) {
        QueryPoses<T> Q;
        query_kinematics<T>(q + 6*i, Q);
        for (int k = 0; k < 18; k++) xpos[18*i + k] = Q.F.pos[k/3][k%3];
        for (int k = 0; k < 54; k++) xmat[54*i + k] = Q.F.R[k/9][k%9];
        for (int k = 0; k < 3; k++) { ee[3*i + k] = Q.ee[k]; cam_pos[3*i + k] = Q.cam_pos[k]; }
        for (int k = 0; k < 9; k++) cam_mat[9*i + k] = Q.cam_mat[k];
    }
}

// o: three values, or null for the link's default point (the end-effector point on link 4, the origin elsewhere: include/so100_query.h)
template <typename T> void point_offset(int link, const T* o, T out[3]) {
    for (int k = 0; k < 3; k++) out[k] = o ? o[k] : (link == EE_LINK ? T((float)EE_OFFSET[k]) : T(0));
}

template <typename T> void jacobian(long n, const T* q, int link, const T* o, T* jacp, T* jacr) {
    T off[3];
    point_offset(link, o, off);
    for (long i = 0; i < n; i++) query_jacobian<T>(q + 6*i, link, off, jacp + 18*i, jacr + 18*i);
}

template <typename T> void dynamics(long n, const T* q, const T* v, const T* qacc, T* M, T* bias, T* tau) {
    const T zero[6] = { T(0), T(0), T(0), T(0), T(0), T(0) };
    for (long i = 0; i < n; i++) query_dynamics<T>(q + 6*i, v ? v + 6*i : zero, qacc ? qacc + 6*i : nullptr, M + 36*i, bias + 6*i, tau + 6*i);
}

template <typename T> void ik(long n, const T* q0, const T* target, int link, const T* o, int iters, T damping, T tol, T max_step,
                              T* q, T* residual, int32_t* iterations, uint8_t* converged) {
    IkParams<T> P;
    P.link = link; P.iters = iters; P.damping2 = damping*damping; P.tol = tol; P.max_step = max_step;
    point_offset(link, o, P.o);
    for (long i = 0; i < n; i++) {
        IkResult<T> R;
        query_ik<T>(q0 + 6*i, target + 3*i, P, R);
        for (int k = 0; k < 6; k++) q[6*i + k] = R.q[k];
        residual[i] = R.residual; iterations[i] = R.iterations; converged[i] = R.converged ? 1 : 0;
    }
}

}  // namespace

extern "C" {

#define QC_INSTANCE(S, T) \
    void qc_kinematics_##S(long n, const T* q, T* xpos, T* xmat, T* ee, T* cam_pos, T* cam_mat) { kinematics<T>(n, q, xpos, xmat, ee, cam_pos, cam_mat); } \
    void qc_jacobian_##S(long n, const T* q, int link, const T* o, T* jacp, T* jacr) { jacobian<T>(n, q, link, o, jacp, jacr); } \
    void qc_dynamics_##S(long n, const T* q, const T* v, const T* qacc, T* M, T* bias, T* tau) { dynamics<T>(n, q, v, qacc, M, bias, tau); } \
    void qc_ik_##S(long n, const T* q0, const T* target, int link, const T* o, int iters, T damping, T tol, T max_step, \
                   T* q, T* residual, int32_t* iterations, uint8_t* converged) { \
        ik<T>(n, q0, target, link, o, iters, damping, tol, max_step, q, residual, iterations, converged); }
QC_INSTANCE(d, double)
QC_INSTANCE(f, float)
#undef QC_INSTANCE

void qc_joint_range(double* out12) { for (int k = 0; k < 6; k++) { out12[2*k] = so100g::JNT_RANGE[k][0]; out12[2*k + 1] = so100g::JNT_RANGE[k][1]; } }

}  // extern "C"

#ifdef QUERYCHECK_MAIN
// a stand-alone run for a host sanitizer: the four queries in both precisions on 400 problems drawn like the IK tests' (a pose in the
// middle 80 % of the joint ranges, its end-effector point as the target, a start up to 0.3 rad away), and the unreachable target
#include <math.h>
#include <stdio.h>
#include <vector>
namespace {
uint32_t g_state = 12345u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0; }

template <typename T> int run(const char* name) {
    const long n = 400;
    int bad = 0;
    std::vector<T> qs(6*n), q0(6*n), v(6*n), a(6*n), xpos(18*n), xmat(54*n), ee(3*n), cp(3*n), cm(9*n), jp(18*n), jr(18*n), M(36*n), bias(6*n), tau(6*n);
    std::vector<T> q(6*n), res(n);
    std::vector<int32_t> its(n);
    std::vector<uint8_t> conv(n);
    for (long i = 0; i < n; i++)
        for (int k = 0; k < 6; k++) {
            const double lo = so100g::JNT_RANGE[k][0], hi = so100g::JNT_RANGE[k][1];
            qs[6*i + k] = T(lo + (0.1 + 0.8*uniform())*(hi - lo));
            q0[6*i + k] = qs[6*i + k] + T(k < 5 ? 0.6*uniform() - 0.3 : 0.0);
            v[6*i + k] = T(4.0*uniform() - 2.0); a[6*i + k] = T(40.0*uniform() - 20.0);
        }
    kinematics<T>(n, qs.data(), xpos.data(), xmat.data(), ee.data(), cp.data(), cm.data());
    for (int link = 0; link < 6; link++) jacobian<T>(n, qs.data(), link, nullptr, jp.data(), jr.data());
    dynamics<T>(n, qs.data(), v.data(), a.data(), M.data(), bias.data(), tau.data());
    dynamics<T>(n, qs.data(), nullptr, nullptr, M.data(), bias.data(), tau.data());
    for (long i = 0; i < 36*n; i++) bad += !(M[i] == M[i]);
    for (long i = 0; i < n; i++) for (int r = 0; r < 6; r++) for (int c = 0; c < r; c++) bad += M[36*i + 6*r + c] != M[36*i + 6*c + r];
    ik<T>(n, q0.data(), ee.data(), 4, nullptr, 64, T(0.02), T(1e-4), T(0.3), q.data(), res.data(), its.data(), conv.data());
    long nconv = 0;
    for (long i = 0; i < n; i++) {
        nconv += conv[i];
        bad += its[i] < 0 || its[i] > 64 || !(res[i] == res[i]) || q[6*i + 5] != q0[6*i + 5] || (conv[i] != 0) != (res[i] <= T(1e-4));
    }
    bad += nconv < (long)(0.98*n);
    // q aliasing q0, and the unreachable target
    std::vector<T> qa(q0);
    ik<T>(n, qa.data(), ee.data(), 4, nullptr, 64, T(0.02), T(1e-4), T(0.3), qa.data(), res.data(), its.data(), conv.data());
    for (long i = 0; i < 6*n; i++) bad += qa[i] != q[i];
    const T far[3] = { T(0), T(-2.0), T(0.3) }, start[6] = { T(0), T(-1.57), T(1.57), T(1.0), T(0), T(0) };
    T qf[6], rf; int32_t itf; uint8_t cf;
    ik<T>(1, start, far, 4, nullptr, 64, T(0.02), T(1e-4), T(0.3), qf, &rf, &itf, &cf);
    bad += cf != 0 || itf != 64 || !(rf > T(1)) || !(rf < T(3));
    printf("querycheck selftest (%s): %ld of %ld converged, unreachable residual %.6f after %d: %s\n", name, nconv, n, (double)rf, (int)itf, bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
