// lqrboxcheck.cpp -- the control-limited LQR pass (lqr_box_problem of lqr_box.hpp: lqr_boxqp6 per step) on the host, in
// double (held to the numpy fp64 reference, which enumerates the active sets) and in float, behind a C interface for ctypes (built by the
// Makefile beside it, loaded and called by tests/lqr_box_support.py).  Arrays as in
// include/so100_query.h (so100_lqr_io) plus clamped [T][M] and used [T][M] of LqrBoxArgs.  Test scaffolding only.
#include <stdint.h>
#include "lqr_box.hpp"

using namespace so100;

namespace {

template <typename T> void lqr_box(long M, int nx, int horizon, const T* A, const T* B, const T* lx, const T* lxx, const T* lu, const T* luu, const T* lux, const T* u,
                                   const T* dx0, T reg, T alpha, T u_lo, T u_hi, int qp_iters, T* k, T* K, T* Vx0, T* Vxx0, T* dV, T* du, T* dx, int32_t* bad,
                                   int32_t* clamped, int32_t* used) {
    const LqrArgs<T> a{ A, B, lx, lxx, lu, luu, lux, u, dx0, horizon, reg, alpha, u_lo, u_hi, k, K, Vx0, Vxx0, dV, du, dx, bad };
    const LqrBoxArgs box{ qp_iters, clamped, used };
    for (long m = 0; m < M; m++) {
        if (nx == 24) lqr_box_problem<T, 24>(a, (size_t)M, (size_t)m, &box);
        else          lqr_box_problem<T, 12>(a, (size_t)M, (size_t)m, &box);
    }
}

}  // namespace

extern "C" {

#define LB_INSTANCE(S, T) \
    void lb_lqr_box_##S(long M, int nx, int horizon, const T* A, const T* B, const T* lx, const T* lxx, const T* lu, const T* luu, const T* lux, const T* u, \
                        const T* dx0, T reg, T alpha, T u_lo, T u_hi, int qp_iters, T* k, T* K, T* Vx0, T* Vxx0, T* dV, T* du, T* dx, int32_t* bad, \
                        int32_t* clamped, int32_t* used) { \
        lqr_box<T>(M, nx, horizon, A, B, lx, lxx, lu, luu, lux, u, dx0, reg, alpha, u_lo, u_hi, qp_iters, k, K, Vx0, Vxx0, dV, du, dx, bad, clamped, used); }
LB_INSTANCE(d, double)
LB_INSTANCE(f, float)
#undef LB_INSTANCE

}  // extern "C"

#ifdef LQRBOXCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions and both forms over a few seeded problems at several horizons -- k inside its room and
// u + du inside the bounds, zero rows of K where clamped says so, some steps with and some without a clamped control, every step's k a KKT point
// of its QP as far as the problem's own data tell (the clamped set against the sign of the gradient at the terminal step, where Quu and Qu are
// known without a recursion), wide bounds = the unconstrained pass bit for bit with qp_used = 1, one iteration sets bit 16, a nominal control
// outside the bounds, an indefinite luu and a NaN beside clean neighbours
#include <stdio.h>
#include <string.h>
#include <limits>
#include <vector>
namespace {
constexpr int ITERS = 16;
uint32_t g_state = 2029u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0 - 0.5; }

template <typename T> struct Problem {
    long M; int n, H;
    std::vector<T> A, B, lx, lxx, lu, luu, lux, u, k, K, Vx0, Vxx0, dV, du, dx;
    std::vector<int32_t> bad, clamped, used;
    Problem(long M_, int n_, int H_) : M(M_), n(n_), H(H_), A(H*M*576), B(H*M*144), lx((H + 1)*M*n), lxx((H + 1)*M*n*n), lu(H*M*6), luu(H*M*36), lux(H*M*6*n),
        u(H*M*6), k(H*M*6), K(H*M*6*n), Vx0(M*n), Vxx0(M*n*n), dV(M*2), du(H*M*6), dx((H + 1)*M*n), bad(M), clamped(H*M), used(H*M) {
        const int np = n + 6;
        for (long p = 0; p < (H + 1)*M; p++) {
            if (p < H*M) {
                for (int i = 0; i < 24; i++) {
                    for (int j = 0; j < 24; j++) A[p*576 + i*24 + j] = T((i == j) + 0.06*uniform());
                    for (int j = 0; j < 6; j++) B[p*144 + i*6 + j] = T(0.6*uniform());
                }
                for (int j = 0; j < 6; j++) { lu[p*6 + j] = T(2*uniform()); u[p*6 + j] = T(1.6*uniform()); }
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
    void run(int iters, T reg, T lo, T hi, std::vector<T>& kk, std::vector<T>& KK) {
        lqr_box<T>(M, n, H, A.data(), B.data(), lx.data(), lxx.data(), lu.data(), luu.data(), lux.data(), u.data(), nullptr, reg, T(1), lo, hi, iters,
                   kk.data(), KK.data(), Vx0.data(), Vxx0.data(), dV.data(), du.data(), dx.data(), bad.data(), clamped.data(), used.data());
    }
};

template <typename T> int run(const char* name) {
    int failures = 0; long count = 0, with = 0, without = 0;
    const T slack = sizeof(T) == 8 ? T(1e-12) : T(1e-6);
    for (int n : { 12, 24 })
        for (int H : { 1, 2, 7 }) {
            const long M = 3;
            Problem<T> P(M, n, H);
            std::vector<T> k2(P.k.size()), K2(P.K.size());
            P.run(ITERS, T(0), T(-1), T(1), P.k, P.K);
            for (long p = 0; p < H*M; p++) {
                failures += P.bad[p % M] != -1 || (P.used[p] >> 16) != 0 || P.used[p] < 1;
                (P.clamped[p] ? with : without)++;
                for (int j = 0; j < 6; j++) {
                    const T lo = T(-1) - P.u[p*6 + j], hi = T(1) - P.u[p*6 + j], x = P.k[p*6 + j], v = P.u[p*6 + j] + P.du[p*6 + j];
                    const bool low = (P.clamped[p] >> j) & 1, up = (P.clamped[p] >> (8 + j)) & 1;
                    failures += !(x >= lo && x <= hi) || !(v >= T(-1) - slack && v <= T(1) + slack) || (low && up) || (low && x != lo) || (up && x != hi);
                    for (int c = 0; c < n; c++) failures += (low || up) && !(P.K[(p*6 + j)*n + c] == T(0));
                }
                count++;
            }
            // the terminal step's QP is known without a recursion: H = luu + B'lxx_T B, g = lu + B'lx_T; the gradient at k has the multipliers' signs
            for (long m = 0; m < M; m++) {
                const long p = (H - 1)*M + m, q = H*M + m;
                std::vector<double> Bn(n*6), S(n*n);
                for (int i = 0; i < n; i++) {
                    for (int j = 0; j < 6; j++) Bn[i*6 + j] = P.B[p*144 + (n == 24 ? i : (i < 6 ? i : i + 6))*6 + j];
                    for (int j = 0; j < n; j++) S[i*n + j] = 0.5*((double)P.lxx[q*n*n + i*n + j] + (double)P.lxx[q*n*n + j*n + i]);
                }
                for (int i = 0; i < 6; i++) {
                    double g = P.lu[p*6 + i];
                    for (int a = 0; a < n; a++) g += Bn[a*6 + i]*P.lx[q*n + a];
                    for (int j = 0; j < 6; j++) {
                        double h = P.luu[p*36 + i*6 + j];
                        for (int a = 0; a < n; a++) for (int b = 0; b < n; b++) h += Bn[a*6 + i]*S[a*n + b]*Bn[b*6 + j];
                        g += h*P.k[p*6 + j];
                    }
                    const bool low = (P.clamped[p] >> i) & 1, up = (P.clamped[p] >> (8 + i)) & 1;
                    const double tol = sizeof(T) == 8 ? 1e-9 : 2e-3;
                    failures += low ? !(g > -tol) : up ? !(g < tol) : !(fabs(g) <= tol);
                }
            }
            // wide bounds: the unconstrained pass (qp_iters = 0 here) bit for bit, one iteration each, nothing clamped
            P.run(ITERS, T(0), T(-1e6), T(1e6), P.k, P.K);
            for (long p = 0; p < H*M; p++) failures += P.clamped[p] != 0 || P.used[p] != 1;
            std::vector<T> dV1 = P.dV, Vxx1 = P.Vxx0;
            {                                                // so100_lqr.hpp's own pass on the same problem
                const LqrArgs<T> plain{ P.A.data(), P.B.data(), P.lx.data(), P.lxx.data(), P.lu.data(), P.luu.data(), P.lux.data(), P.u.data(), nullptr, H, T(0), T(1),
                                        T(-1e6), T(1e6), k2.data(), K2.data(), P.Vx0.data(), P.Vxx0.data(), P.dV.data(), P.du.data(), P.dx.data(), P.bad.data() };
                for (long m = 0; m < M; m++) { if (n == 24) lqr_problem<T, 24>(plain, (size_t)M, (size_t)m); else lqr_problem<T, 12>(plain, (size_t)M, (size_t)m); }
            }
            failures += memcmp(P.k.data(), k2.data(), k2.size()*sizeof(T)) != 0 || memcmp(P.K.data(), K2.data(), K2.size()*sizeof(T)) != 0;
            failures += memcmp(dV1.data(), P.dV.data(), dV1.size()*sizeof(T)) != 0 || memcmp(Vxx1.data(), P.Vxx0.data(), Vxx1.size()*sizeof(T)) != 0;
            // one iteration: bit 16 wherever a control ends clamped or the step was cut, and still inside the room
            P.run(1, T(0), T(-1), T(1), P.k, P.K);
            long ran_out = 0;
            for (long p = 0; p < H*M; p++) {
                failures += (P.used[p] & 0xFFFF) != 1 || (P.clamped[p] != 0 && !(P.used[p] >> 16));
                ran_out += P.used[p] >> 16;
                for (int j = 0; j < 6; j++) { const T x = P.k[p*6 + j]; failures += !(x >= T(-1) - P.u[p*6 + j] && x <= T(1) - P.u[p*6 + j]); }
            }
            failures += ran_out == 0;
            // a nominal control outside the bounds: finite, and brought back onto the bound or inside
            const T keep = P.u[0];
            P.u[0] = T(3);
            P.run(ITERS, T(0), T(-1), T(1), P.k, P.K);
            failures += P.bad[0] != -1 || !(P.k[0] <= T(-2)) || !(P.k[0] >= T(-4)) || !(P.Vx0[0] == P.Vx0[0]);
            P.u[0] = keep;
            // problem 1: luu = -I at the last step fails there under reg = 0 and passes under reg = 4; then a NaN in its A: bad = H
            const int ts = H - 1;
            for (int i = 0; i < 36; i++) P.luu[(ts*M + 1)*36 + i] = (i % 7 == 0) ? T(-1) : T(0);
            for (int i = 0; i < 6*n; i++) P.lux[(ts*M + 1)*6*n + i] = T(0);
            for (int i = 0; i < 144; i++) P.B[(ts*M + 1)*144 + i] *= T(0.1);
            P.run(ITERS, T(0), T(-1), T(1), P.k, P.K);
            failures += P.bad[0] != -1 || P.bad[1] != ts || P.bad[2] != -1;
            failures += (P.k[(ts*M + 1)*6] == P.k[(ts*M + 1)*6]) + !(P.k[(ts*M + 0)*6] == P.k[(ts*M + 0)*6]) + (P.Vx0[n] == P.Vx0[n]) + !(P.Vx0[0] == P.Vx0[0]);
            for (int t = 0; t < H; t++) failures += P.clamped[t*M + 1] != 0 || P.used[t*M + 1] != 0 || P.used[t*M] == 0;
            P.run(ITERS, T(4), T(-1), T(1), P.k, P.K);
            failures += P.bad[1] != -1 || !(P.k[(ts*M + 1)*6] == P.k[(ts*M + 1)*6]);
            P.A[(0*M + 1)*576 + 24 + 13] = std::numeric_limits<T>::quiet_NaN();      // row 1, column 13: in the arm block too
            P.run(ITERS, T(4), T(-1), T(1), P.k, P.K);
            failures += P.bad[0] != -1 || P.bad[1] != H || P.bad[2] != -1 || (P.dx[1*n] == P.dx[1*n]) || !(P.dx[2*n] == P.dx[2*n]);
        }
    failures += with == 0 || without == 0;
    printf("lqrboxcheck selftest (%s): %ld steps, %ld with a clamped control: %s\n", name, count, with, failures ? "FAILED" : "ok");
    return failures;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
