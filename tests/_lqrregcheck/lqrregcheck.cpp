// lqrregcheck.cpp -- the LQR query with a regulariser per problem and its schedule (lqr_reg_problem, lqr_reg_raise, lqr_reg_next of
// csrc/so100_lqr.hpp) on the host, in double (held to the numpy fp64 reference) and in float (the kernel's arithmetic), behind a C interface for
// ctypes (built by the Makefile beside it, loaded and called by tests/lqr_reg_support.py).  Arrays as in include/so100_query.h
// (so100_lqr_reg_io, so100_reg_schedule_io).  Test scaffolding only.
#include <stdint.h>
#include "so100_lqr.hpp"

using namespace so100;

namespace {

template <typename T> void lqr_reg(long M, int nx, int horizon, const T* A, const T* B, const T* lx, const T* lxx, const T* lu, const T* luu, const T* lux, const T* u,
                                   const T* dx0, T reg, T alpha, T u_lo, T u_hi, const T* reg_in, T reg_min, T reg_max, T reg_up, int tries, T* k, T* K, T* Vx0,
                                   T* Vxx0, T* dV, T* du, T* dx, int32_t* bad, T* reg_used, int32_t* tries_out) {
    const LqrArgs<T> a{ A, B, lx, lxx, lu, luu, lux, u, dx0, horizon, reg, alpha, u_lo, u_hi, k, K, Vx0, Vxx0, dV, du, dx, bad };
    const LqrRegArgs<T> g{ reg_in, reg_min, reg_max, reg_up, tries, reg_used, tries_out };
    for (long m = 0; m < M; m++) {
        if (nx == 24) lqr_reg_problem<T, 24>(a, g, (size_t)M, (size_t)m);
        else          lqr_reg_problem<T, 12>(a, g, (size_t)M, (size_t)m);
    }
}

template <typename T> void plain(long M, int nx, const LqrArgs<T>& a) {
    for (long m = 0; m < M; m++) {
        if (nx == 24) lqr_problem<T, 24>(a, (size_t)M, (size_t)m);
        else          lqr_problem<T, 12>(a, (size_t)M, (size_t)m);
    }
}

}  // namespace

extern "C" {

#define LR_INSTANCE(S, T) \
    void lr_lqr_reg_##S(long M, int nx, int horizon, const T* A, const T* B, const T* lx, const T* lxx, const T* lu, const T* luu, const T* lux, const T* u, \
                        const T* dx0, T reg, T alpha, T u_lo, T u_hi, const T* reg_in, T reg_min, T reg_max, T reg_up, int tries, T* k, T* K, T* Vx0, T* Vxx0, \
                        T* dV, T* du, T* dx, int32_t* bad, T* reg_used, int32_t* tries_out) { \
        lqr_reg<T>(M, nx, horizon, A, B, lx, lxx, lu, luu, lux, u, dx0, reg, alpha, u_lo, u_hi, reg_in, reg_min, reg_max, reg_up, tries, k, K, Vx0, Vxx0, dV, du, \
                   dx, bad, reg_used, tries_out); }
LR_INSTANCE(d, double)
LR_INSTANCE(f, float)
#undef LR_INSTANCE

float lr_raise_f(float r, float reg_min, float reg_max, float reg_up) { return lqr_reg_raise(r, reg_min, reg_max, reg_up); }

// the schedule in the kernel's arithmetic; reg may be reg_used
void lr_schedule_f(long M, const float* reg_used, const int32_t* best, int keep, float reg_min, float reg_max, float reg_up, float reg_down, float* reg,
                   uint8_t* improved) {
    for (long m = 0; m < M; m++) {
        const bool imp = best[m] >= 0 && best[m] != keep;
        reg[m] = lqr_reg_next(reg_used[m], imp, reg_min, reg_max, reg_up, reg_down);
        if (improved) improved[m] = imp ? 1 : 0;
    }
}

}  // extern "C"

#ifdef LQRREGCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions and both forms over seeded problems at several horizons, problem 1 with luu = -I at one
// step -- tries = 1 without reg_in is the plain pass bit for bit; the retry ends on the first reg of the ladder that the plain pass accepts and
// gives that pass's bits, its neighbours untouched; too few tries or a low reg_max end in bad = that step and NaN; a start that is no reg runs
// no pass; a NaN input is not retried; raise and the schedule on their corner values
#include <stdio.h>
#include <string.h>
#include <limits>
#include <vector>
namespace {
uint32_t g_state = 2031u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0 - 0.5; }

template <typename T> struct Problem {
    long M; int n, H;
    std::vector<T> A, B, lx, lxx, lu, luu, lux;
    struct Out {
        std::vector<T> k, K, Vx0, Vxx0, dV, du, dx, reg_used; std::vector<int32_t> bad, tries;
        Out(long M, int n, int H) : k(H*M*6), K(H*M*6*n), Vx0(M*n), Vxx0(M*n*n), dV(M*2), du(H*M*6), dx((H + 1)*M*n), reg_used(M), bad(M), tries(M) {}
    };
    Problem(long M_, int n_, int H_) : M(M_), n(n_), H(H_), A(H*M*576), B(H*M*144), lx((H + 1)*M*n), lxx((H + 1)*M*n*n), lu(H*M*6), luu(H*M*36), lux(H*M*6*n) {
        const int np = n + 6;
        for (long p = 0; p < (H + 1)*M; p++) {
            if (p < H*M) {
                for (int i = 0; i < 24; i++) {
                    for (int j = 0; j < 24; j++) A[p*576 + i*24 + j] = T((i == j) + 0.06*uniform());
                    for (int j = 0; j < 6; j++) B[p*144 + i*6 + j] = T(0.6*uniform());
                }
                for (int j = 0; j < 6; j++) lu[p*6 + j] = T(2*uniform());
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
    LqrArgs<T> args(Out& o, T reg) {
        return LqrArgs<T>{ A.data(), B.data(), lx.data(), lxx.data(), lu.data(), luu.data(), lux.data(), nullptr, nullptr, H, reg, T(1), T(-1), T(1),
                           o.k.data(), o.K.data(), o.Vx0.data(), o.Vxx0.data(), o.dV.data(), o.du.data(), o.dx.data(), o.bad.data() };
    }
    void run(Out& o, T reg, const T* reg_in, T reg_min, T reg_max, T reg_up, int tries) {
        lqr_reg<T>(M, n, H, A.data(), B.data(), lx.data(), lxx.data(), lu.data(), luu.data(), lux.data(), nullptr, nullptr, reg, T(1), T(-1), T(1), reg_in, reg_min,
                   reg_max, reg_up, tries, o.k.data(), o.K.data(), o.Vx0.data(), o.Vxx0.data(), o.dV.data(), o.du.data(), o.dx.data(), o.bad.data(), o.reg_used.data(),
                   o.tries.data());
    }
};

template <typename T> bool same(const std::vector<T>& a, const std::vector<T>& b) { return memcmp(a.data(), b.data(), a.size()*sizeof(T)) == 0; }
// problem m's part of a [rows][M][w] array
template <typename T> bool same_problem(const std::vector<T>& a, const std::vector<T>& b, long rows, long M, long m, long w) {
    for (long t = 0; t < rows; t++) if (memcmp(&a[(t*M + m)*w], &b[(t*M + m)*w], w*sizeof(T)) != 0) return false;
    return true;
}

template <typename T> int run(const char* name) {
    int failures = 0; long count = 0;
    const T nan = std::numeric_limits<T>::quiet_NaN();
    for (int n : { 12, 24 })
        for (int H : { 1, 2, 7 }) {
            const long M = 3;
            Problem<T> P(M, n, H);
            typename Problem<T>::Out o(M, n, H), q(M, n, H);
            // tries = 1 without reg_in: the plain pass bit for bit
            P.run(o, T(0.25), nullptr, T(0.125), T(32), T(4), 1);
            plain<T>(M, n, P.args(q, T(0.25)));
            failures += !same(o.k, q.k) || !same(o.K, q.K) || !same(o.Vx0, q.Vx0) || !same(o.Vxx0, q.Vxx0) || !same(o.dV, q.dV) || !same(o.du, q.du) || !same(o.dx, q.dx);
            for (long m = 0; m < M; m++) failures += o.bad[m] != -1 || o.tries[m] != 1 || o.reg_used[m] != T(0.25);
            // problem 1: luu = -I at the last step fails under reg = 0; the ladder is 0, 0.125, 0.5, 2, 8, 32
            const int ts = H - 1;
            for (int i = 0; i < 36; i++) P.luu[(ts*M + 1)*36 + i] = (i % 7 == 0) ? T(-1) : T(0);
            for (int i = 0; i < 6*n; i++) P.lux[(ts*M + 1)*6*n + i] = T(0);
            for (int i = 0; i < 144; i++) P.B[(ts*M + 1)*144 + i] *= T(0.1);
            P.run(o, T(0), nullptr, T(0.125), T(32), T(4), 16);
            failures += o.bad[0] != -1 || o.bad[1] != -1 || o.bad[2] != -1 || o.tries[0] != 1 || o.tries[2] != 1 || o.reg_used[0] != T(0) || o.reg_used[2] != T(0);
            failures += o.tries[1] < 2 || o.tries[1] > 6 || !(o.reg_used[1] > T(0));
            const int passes = o.tries[1];
            const T used = o.reg_used[1];
            {                                                // the ladder's value at that pass, and the plain pass alone: fails one rung lower, and gives the retry's bits at this one
                T r = T(0);
                for (int a = 1; a < passes; a++) r = lqr_reg_raise(r, T(0.125), T(32), T(4));
                failures += r != used;
                plain<T>(M, n, P.args(q, used));
                failures += q.bad[1] != -1 || !same_problem(o.k, q.k, H, M, 1, 6) || !same_problem(o.K, q.K, H, M, 1, 6*n) || !same_problem(o.Vx0, q.Vx0, 1, M, 1, n);
                failures += !same_problem(o.Vxx0, q.Vxx0, 1, M, 1, n*n) || !same_problem(o.dV, q.dV, 1, M, 1, 2) || !same_problem(o.du, q.du, H, M, 1, 6);
                failures += !same_problem(o.dx, q.dx, H + 1, M, 1, n);
                plain<T>(M, n, P.args(q, T(0)));
                failures += q.bad[1] != ts || !same_problem(o.k, q.k, H, M, 0, 6) || !same_problem(o.k, q.k, H, M, 2, 6) || !same_problem(o.dx, q.dx, H + 1, M, 2, n);
            }
            // one try too few, and a reg_max one rung too low: bad = that step, the last reg tried, NaN
            if (passes >= 2) {
                P.run(o, T(0), nullptr, T(0.125), T(32), T(4), passes - 1);
                failures += o.bad[1] != ts || o.tries[1] != passes - 1 || !(o.reg_used[1] < used) || (o.k[(ts*M + 1)*6] == o.k[(ts*M + 1)*6]) || (o.dV[2] == o.dV[2]);
                failures += o.bad[0] != -1 || !(o.k[ts*M*6] == o.k[ts*M*6]);
                const T below = o.reg_used[1];
                if (below > T(0)) {
                    P.run(o, T(0), nullptr, T(0.125), below, T(4), 16);
                    failures += o.bad[1] != ts || o.tries[1] != passes - 1 || o.reg_used[1] != below || (o.Vx0[n] == o.Vx0[n]);
                }
            }
            // per-problem starts: the one that works at once, NaN and -1 (no pass), and a NaN in problem 0's A (one pass, never retried)
            std::vector<T> start = { nan, used, T(-1) };
            P.run(o, T(0), start.data(), T(0.125), T(32), T(4), 16);
            failures += o.bad[0] != H || o.tries[0] != 0 || (o.reg_used[0] == o.reg_used[0]) || (o.k[0] == o.k[0]) || (o.dx[0] == o.dx[0]);
            failures += o.bad[2] != H || o.tries[2] != 0 || (o.reg_used[2] == o.reg_used[2]) || (o.Vxx0[2*n*n] == o.Vxx0[2*n*n]);
            failures += o.bad[1] != -1 || o.tries[1] != 1 || o.reg_used[1] != used;
            P.A[(0*M + 0)*576 + 24 + 13] = nan;              // row 1, column 13: in the arm block too
            P.run(o, T(0), nullptr, T(0.125), T(32), T(4), 16);
            failures += o.bad[0] != H || o.tries[0] != 1 || o.reg_used[0] != T(0) || (o.k[0] == o.k[0]) || o.bad[1] != -1 || o.bad[2] != -1;
            count++;
        }
    // raise and the schedule
    failures += lqr_reg_raise(T(0), T(0.125), T(32), T(4)) != T(0.125) || lqr_reg_raise(T(0.125), T(0.125), T(32), T(4)) != T(0.5);
    failures += lqr_reg_raise(T(16), T(0.125), T(32), T(4)) != T(32) || lqr_reg_raise(T(32), T(0.125), T(32), T(4)) != T(32);
    failures += lqr_reg_next(T(2), true, T(0.125), T(32), T(4), T(0.25)) != T(0.5) || lqr_reg_next(T(0.25), true, T(0.125), T(32), T(4), T(0.25)) != T(0);
    failures += lqr_reg_next(T(2), false, T(0.125), T(32), T(4), T(0.25)) != T(8) || lqr_reg_next(nan, false, T(0.125), T(32), T(4), T(0.25)) != T(0.125);
    failures += lqr_reg_next(T(-1), true, T(0.125), T(32), T(4), T(0.25)) != T(0) || lqr_reg_next(nan, true, T(0.125), T(32), T(4), T(0.25)) != T(0);
    printf("lqrregcheck selftest (%s): %ld shapes: %s\n", name, count, failures ? "FAILED" : "ok");
    return failures;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
