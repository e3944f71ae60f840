// lqrcheck.cpp -- the LQR query's recursion (lqr_problem of so100_lqr.hpp) on the host, in double (held to the numpy fp64 reference) and in
// float (the arithmetic the kernel ships, without FMA contraction), behind a C interface for ctypes (built by tests/Makefile, loaded by tests/hostlibs.py,
// called by tests/lqr_support.py).  Arrays as in include/so100_query.h: A [T][M][24][24], B [T][M][24][6], the rest problem-major in the
// n of the call; nullable where the header says so.  Test scaffolding only.
#include <stdint.h>
#include "../../so100_mujoco_rl_amd/csrc/so100_lqr.hpp"

using namespace so100;

namespace {

template <typename T> void lqr(long M, int nx, int horizon, const T* A, const T* B, const T* lx, const T* lxx, const T* lu, const T* luu, const T* lux, const T* u,
                               const T* dx0, T reg, T alpha, T u_lo, T u_hi, T* k, T* K, T* Vx0, T* Vxx0, T* dV, T* du, T* dx, int32_t* bad) {
    const LqrArgs<T> a{ A, B, lx, lxx, lu, luu, lux, u, dx0, horizon, reg, alpha, u_lo, u_hi, k, K, Vx0, Vxx0, dV, du, dx, bad };
    for (long m = 0; m < M; m++) {
        if (nx == 24) lqr_problem<T, 24>(a, (size_t)M, (size_t)m);
        else          lqr_problem<T, 12>(a, (size_t)M, (size_t)m);
    }
}

}  // namespace

extern "C" {

#define LQ_INSTANCE(S, T) \
    void lq_lqr_##S(long M, int nx, int horizon, const T* A, const T* B, const T* lx, const T* lxx, const T* lu, const T* luu, const T* lux, const T* u, \
                    const T* dx0, T reg, T alpha, T u_lo, T u_hi, T* k, T* K, T* Vx0, T* Vxx0, T* dV, T* du, T* dx, int32_t* bad) { \
        lqr<T>(M, nx, horizon, A, B, lx, lxx, lu, luu, lux, u, dx0, reg, alpha, u_lo, u_hi, k, K, Vx0, Vxx0, dV, du, dx, bad); }
LQ_INSTANCE(d, double)
LQ_INSTANCE(f, float)
#undef LQ_INSTANCE

}  // extern "C"

#ifdef LQRCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions and both forms over a few seeded problems at several horizons -- every output,
// twice (the same bits), the value-decrease identity dV1 + dV2 = model(du, dx), a clamped pass inside its bounds; then an indefinite luu and a
// NaN beside clean neighbours
#include <stdio.h>
#include <limits>
#include <vector>
namespace {
uint32_t g_state = 2027u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0 - 0.5; }

template <typename T> struct Problem {
    long M; int n, H;
    std::vector<T> A, B, lx, lxx, lu, luu, lux, u, k, K, Vx0, Vxx0, dV, du, dx;
    std::vector<int32_t> bad;
    Problem(long M_, int n_, int H_) : M(M_), n(n_), H(H_), A(H*M*576), B(H*M*144), lx((H + 1)*M*n), lxx((H + 1)*M*n*n), lu(H*M*6), luu(H*M*36), lux(H*M*6*n),
        u(H*M*6), k(H*M*6), K(H*M*6*n), Vx0(M*n), Vxx0(M*n*n), dV(M*2), du(H*M*6), dx((H + 1)*M*n), bad(M) {
        const int np = n + 6;
        for (long p = 0; p < (H + 1)*M; p++) {
            if (p < H*M) {
                for (int i = 0; i < 24; i++) {
                    for (int j = 0; j < 24; j++) A[p*576 + i*24 + j] = T((i == j) + 0.06*uniform());
                    for (int j = 0; j < 6; j++) B[p*144 + i*6 + j] = T(0.6*uniform());
                }
                for (int j = 0; j < 6; j++) { lu[p*6 + j] = T(2*uniform()); u[p*6 + j] = T(1.8*uniform()); }
            }
            std::vector<double> C(np*np);
            for (auto& c : C) c = uniform();
            for (int i = 0; i < np; i++)
                for (int j = 0; j < np; j++) {
                    double s = i == j ? 0.1 : 0.0;
                    for (int l = 0; l < np; l++) s += C[i*np + l]*C[j*np + l]*(4.0/np);
                    if (i < n && j < n) lxx[p*n*n + i*n + j] = T(s);
                    else if (p < H*M && i >= n && j < n) lux[(p*6 + i - n)*n + j] = T(s);
                    else if (p < H*M && i >= n && j >= n) luu[p*36 + (i - n)*6 + (j - n)] = T(s);
                }
            for (int i = 0; i < n; i++) lx[p*n + i] = T(2*uniform());
        }
    }
    void run(bool clamp, T reg, std::vector<T>& kk, std::vector<T>& dd) {
        lqr<T>(M, n, H, A.data(), B.data(), lx.data(), lxx.data(), lu.data(), luu.data(), lux.data(), clamp ? u.data() : nullptr, nullptr, reg, T(1), T(-1), T(1),
               kk.data(), K.data(), Vx0.data(), Vxx0.data(), dV.data(), dd.data(), dx.data(), bad.data());
    }
};

template <typename T> int run(const char* name) {
    int failures = 0; long count = 0;
    const T tol = sizeof(T) == 8 ? T(1e-9) : T(2e-3);
    for (int n : { 12, 24 })
        for (int H : { 1, 2, 7 }) {
            const long M = 3;
            Problem<T> P(M, n, H);
            std::vector<T> k2(P.k.size()), du2(P.du.size());
            P.run(false, T(0), P.k, P.du); P.run(false, T(0), k2, du2);
            for (size_t i = 0; i < k2.size(); i++) failures += !(P.k[i] == k2[i]) || !(P.du[i] == du2[i]);      // finite, and the same on a second call
            for (long m = 0; m < M; m++) {                  // dV1 + dV2 against the model at (du, dx)
                failures += P.bad[m] != -1;
                double model = 0.0;
                for (int t = 0; t <= H; t++) {
                    const long p = t*M + m;
                    for (int i = 0; i < n; i++) {
                        model += P.lx[p*n + i]*P.dx[p*n + i];
                        for (int j = 0; j < n; j++) model += 0.5*P.dx[p*n + i]*P.lxx[p*n*n + i*n + j]*P.dx[p*n + j];
                    }
                    if (t == H) break;
                    for (int i = 0; i < 6; i++) {
                        model += P.lu[p*6 + i]*P.du[p*6 + i];
                        for (int j = 0; j < 6; j++) model += 0.5*P.du[p*6 + i]*P.luu[p*36 + i*6 + j]*P.du[p*6 + j];
                        for (int j = 0; j < n; j++) model += P.du[p*6 + i]*P.lux[(p*6 + i)*n + j]*P.dx[p*n + j];
                    }
                }
                const double dv = (double)P.dV[2*m] + (double)P.dV[2*m + 1];
                failures += !(fabs(dv - model) <= tol*(1.0 + fabs(model)));
                count++;
            }
            P.run(true, T(0), P.k, P.du);                    // clamped: u + du inside [-1, 1]
            for (size_t i = 0; i < P.du.size(); i++) { const T v = P.u[i] + P.du[i]; failures += !(v >= T(-1) - T(1e-6) && v <= T(1) + T(1e-6)); }
            // problem 1: luu = -I at the last step fails there under reg = 0 and passes under reg = 4; then a NaN in its A: bad = H
            const int ts = H - 1;
            for (int i = 0; i < 36; i++) P.luu[(ts*M + 1)*36 + i] = (i % 7 == 0) ? T(-1) : T(0);
            for (int i = 0; i < 6*n; i++) P.lux[(ts*M + 1)*6*n + i] = T(0);
            for (int i = 0; i < 144; i++) P.B[(ts*M + 1)*144 + i] *= T(0.1);
            P.run(false, T(0), P.k, P.du);
            failures += P.bad[0] != -1 || P.bad[1] != ts || P.bad[2] != -1;
            failures += (P.k[(ts*M + 1)*6] == P.k[(ts*M + 1)*6]) + !(P.k[(ts*M + 0)*6] == P.k[(ts*M + 0)*6]) + (P.Vx0[n] == P.Vx0[n]) + !(P.Vx0[0] == P.Vx0[0]);
            P.run(false, T(4), P.k, P.du);
            failures += P.bad[1] != -1 || !(P.k[(ts*M + 1)*6] == P.k[(ts*M + 1)*6]);
            P.A[(0*M + 1)*576 + 24 + 13] = std::numeric_limits<T>::quiet_NaN();      // row 1, column 13: in the arm block too
            P.run(false, T(4), P.k, P.du);
            failures += P.bad[0] != -1 || P.bad[1] != H || P.bad[2] != -1 || (P.dx[1*n] == P.dx[1*n]) || !(P.dx[2*n] == P.dx[2*n]);
        }
    printf("lqrcheck selftest (%s): %ld problems: %s\n", name, count, failures ? "FAILED" : "ok");
    return failures;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
