// costcheck.cpp -- the two cost queries of so100_cost.hpp on the host, in double (held to the numpy reference) and in float (the arithmetic the
// kernels ship, without FMA contraction), behind a C interface for ctypes (built by tests/Makefile, loaded by tests/hostlibs.py and called by
// tests/cost_support.py).  Arrays are problem-major here: qpos [T][n][13], qvel [T][n][12] (null: zero), u [T][n][6], target [n][3] or [T][n][3];
// the select call's rollouts are [T][n L][.], rollout (m, a) at m L + a, its targets and fallback per problem.  The outputs are in the queries' own
// layouts (lx [T+1][n][nx], lxx [T+1][n][nx][nx], lu [T][n][6], luu [T][n][6][6]; cost [n L], best [n], best_cost [n], u_best [T][n][6]).  def: link,
// target_mode; w: offset 3, w_point, w_q 6, q_nom 6, w_v 6, w_u 6, w_terminal (29 numbers).  Test scaffolding only.
#include "../planner_twin.hpp"

using namespace so100;
using planner_twin::make_def; using planner_twin::target_of; using planner_twin::rollout_cost;

namespace {

template <typename T> void terms(long n, int steps, int nx, int link, int target_mode, const T* w, const T* target, const T* qpos, const T* qvel, const T* u,
                                 T* lx, T* lxx, T* lu, T* luu) {
    const T nan = std::numeric_limits<T>::quiet_NaN();
    const CostDef<T> c = make_def(link, target_mode, w);
    for (long m = 0; m < n; m++) {
        for (int i = 0; i < nx; i++) lx[m*nx + i] = T(0);
        for (int e = 0; e < nx*nx; e++) lxx[m*nx*nx + e] = T(0);
    }
    for (int t = 0; t < steps; t++)
        for (long m = 0; m < n; m++) {
            const long p = (long)t*n + m, r1 = (long)(t + 1)*n + m;
            const T* q = qpos + 13*p;
            T v[6], g[3];
            for (int j = 0; j < 6; j++) v[j] = qvel ? qvel[12*p + j] : T(0);
            target_of(c, target, q, n, m, t, g);
            CostRow<T> R;
            cost_row<T>(c, q, v, g, R);
            const T two_sigma = T(2)*cost_sigma(c, t, steps);
            const CostRowRef<T> row{ R };
            for (int i = 0; i < nx; i++) {
                lx[r1*nx + i] = R.ok ? cost_lx<T>(c, row, two_sigma, cost_idx(nx, i)) : nan;
                for (int j = 0; j < nx; j++) lxx[(r1*nx + i)*nx + j] = R.ok ? cost_lxx<T>(c, row, two_sigma, cost_idx(nx, i), cost_idx(nx, j)) : nan;
            }
            bool fin = true;
            for (int j = 0; j < 6; j++) fin = fin && cost_finite(u[6*p + j]);
            for (int i = 0; i < 6; i++) {
                lu[6*p + i] = fin ? cost_lu<T>(c, u + 6*p, i) : nan;
                for (int j = 0; j < 6; j++) luu[(6*p + i)*6 + j] = fin ? cost_luu<T>(c, i, j) : nan;
            }
        }
}

// bad_step and u_fallback may be null
template <typename T> void select(long n, int steps, int L, int link, int target_mode, const T* w, const T* target, const T* qpos, const T* qvel, const T* u,
                                  const int32_t* bad_step, const T* u_fallback, T* cost, int32_t* best, T* best_cost, T* u_best) {
    const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
    const CostDef<T> c = make_def(link, target_mode, w);
    const long nl = n*L;
    for (long m = 0; m < n; m++) {
        for (int a = 0; a < L; a++) {
            const long col = m*L + a;
            cost[col] = rollout_cost<T>(c, steps, n, nl, m, col, target, qpos, qvel, u, bad_step);
        }
        T bc;
        const int b = cost_argmin<T>(L, inf, [&](int a) { return cost[m*L + a]; }, bc);
        best[m] = b; best_cost[m] = bc;
        for (int t = 0; t < steps; t++)
            for (int j = 0; j < 6; j++)
                u_best[((long)t*n + m)*6 + j] = b >= 0 ? u[((long)t*nl + m*L + b)*6 + j] : (u_fallback ? u_fallback[((long)t*n + m)*6 + j] : nan);
    }
}

}  // namespace

extern "C" {

#define CK_INSTANCE(S, T) \
    void ck_terms_##S(long n, int steps, int nx, int link, int target_mode, const T* w, const T* target, const T* qpos, const T* qvel, const T* u, \
                      T* lx, T* lxx, T* lu, T* luu) { \
        terms<T>(n, steps, nx, link, target_mode, w, target, qpos, qvel, u, lx, lxx, lu, luu); } \
    void ck_select_##S(long n, int steps, int L, int link, int target_mode, const T* w, const T* target, const T* qpos, const T* qvel, const T* u, \
                       const int32_t* bad_step, const T* u_fallback, T* cost, int32_t* best, T* best_cost, T* u_best) { \
        select<T>(n, steps, L, link, target_mode, w, target, qpos, qvel, u, bad_step, u_fallback, cost, best, best_cost, u_best); }
CK_INSTANCE(d, double)
CK_INSTANCE(f, float)
#undef CK_INSTANCE

}  // extern "C"

#ifdef COSTCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions, both nx, the three target modes, a handful of seeded rows; row 0 is zero, lxx is
// symmetric to the bit, n = 12 is the n = 24 block picked, a NaN fails its own row only, and the selection takes the lowest of two equal columns
#include <stdio.h>
#include <string.h>
#include <vector>
namespace {
uint32_t g_state = 2029u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0; }

template <typename T> int run(const char* name) {
    const long n = 5; const int steps = 3, L = 4;
    int bad = 0; long rows = 0;
    T w[29];
    w[0] = T(0.01); w[1] = T(-0.05); w[2] = T(0.02); w[3] = T(1.5);
    for (int j = 0; j < 6; j++) { w[4 + j] = T(j == 2 ? 0 : 0.1*(j + 1)); w[10 + j] = T(0.2*(uniform() - 0.5)); w[16 + j] = T(0.01*(j + 1)); w[22 + j] = T(j == 5 ? 0 : 1e-3); }
    w[28] = T(3);
    for (int mode = 0; mode < 3; mode++) {
        const long nl = n*L;
        std::vector<T> qpos(13*nl*steps), qvel(12*nl*steps), u(6*nl*steps), target(3*n*steps), fb(6*n*steps);
        for (auto& x : qpos) x = T(1.2*(uniform() - 0.5));
        for (auto& x : qvel) x = T(4*(uniform() - 0.5));
        for (auto& x : u) x = T(2*(uniform() - 0.5));
        for (auto& x : target) x = T(0.6*(uniform() - 0.5));
        for (auto& x : fb) x = T(uniform());
        // terms on the first n columns of each step (any [T][n][.] block will do): copy them out
        std::vector<T> q1(13*n*steps), v1(12*n*steps), u1(6*n*steps);
        for (int t = 0; t < steps; t++)
            for (long m = 0; m < n; m++) {
                memcpy(&q1[((long)t*n + m)*13], &qpos[((long)t*nl + m)*13], 13*sizeof(T));
                memcpy(&v1[((long)t*n + m)*12], &qvel[((long)t*nl + m)*12], 12*sizeof(T));
                memcpy(&u1[((long)t*n + m)*6], &u[((long)t*nl + m)*6], 6*sizeof(T));
            }
        q1[(1*n + 2)*13 + 3] = std::numeric_limits<T>::quiet_NaN();          // step 1, problem 2
        std::vector<T> lx24(24*n*(steps + 1)), lxx24(576*n*(steps + 1)), lx12(12*n*(steps + 1)), lxx12(144*n*(steps + 1)), lu(6*n*steps), luu(36*n*steps);
        terms<T>(n, steps, 24, 2, mode, w, target.data(), q1.data(), v1.data(), u1.data(), lx24.data(), lxx24.data(), lu.data(), luu.data());
        terms<T>(n, steps, 12, 2, mode, w, target.data(), q1.data(), nullptr, u1.data(), lx12.data(), lxx12.data(), lu.data(), luu.data());
        terms<T>(n, steps, 12, 2, mode, w, target.data(), q1.data(), v1.data(), u1.data(), lx12.data(), lxx12.data(), lu.data(), luu.data());
        for (long r = 0; r < n*(steps + 1); r++) {
            const bool zero = r < n, gone = r == 2*n + 2;
            for (int i = 0; i < 24; i++) {
                bad += zero ? lx24[24*r + i] != T(0) : (gone ? lx24[24*r + i] == lx24[24*r + i] : !(lx24[24*r + i] == lx24[24*r + i]));
                for (int j = 0; j < 24; j++) {
                    const T x = lxx24[(24*r + i)*24 + j], y = lxx24[(24*r + j)*24 + i];
                    bad += zero ? x != T(0) : (gone ? x == x : memcmp(&x, &y, sizeof(T)) != 0);
                }
            }
            for (int i = 0; i < 12 && !gone; i++) {
                bad += memcmp(&lx12[12*r + i], &lx24[24*r + cost_idx(12, i)], sizeof(T)) != 0;
                for (int j = 0; j < 12; j++) bad += memcmp(&lxx12[(12*r + i)*12 + j], &lxx24[(24*r + cost_idx(12, i))*24 + cost_idx(12, j)], sizeof(T)) != 0;
            }
            rows++;
        }
        // select: candidate 2 of every problem is a copy of candidate 1; problem 3 fails throughout
        for (int t = 0; t < steps; t++)
            for (long m = 0; m < n; m++) {
                memcpy(&qpos[((long)t*nl + m*L + 2)*13], &qpos[((long)t*nl + m*L + 1)*13], 13*sizeof(T));
                memcpy(&qvel[((long)t*nl + m*L + 2)*12], &qvel[((long)t*nl + m*L + 1)*12], 12*sizeof(T));
                memcpy(&u[((long)t*nl + m*L + 2)*6], &u[((long)t*nl + m*L + 1)*6], 6*sizeof(T));
            }
        std::vector<int32_t> bs(nl, -1), best(n);
        for (int a = 0; a < L; a++) bs[3*L + a] = 1;
        std::vector<T> cost(nl), bc(n), ub(6*n*steps);
        select<T>(n, steps, L, 4, mode, w, target.data(), qpos.data(), qvel.data(), u.data(), bs.data(), fb.data(), cost.data(), best.data(), bc.data(), ub.data());
        for (long m = 0; m < n; m++) {
            bad += memcmp(&cost[m*L + 1], &cost[m*L + 2], sizeof(T)) != 0;
            bad += m == 3 ? (best[m] != -1 || bc[m] != std::numeric_limits<T>::infinity()) : (best[m] < 0 || best[m] == 2);
            for (int a = 0; a < L && m != 3; a++) bad += !(bc[m] <= cost[m*L + a]);
            for (int t = 0; t < steps; t++)
                for (int j = 0; j < 6; j++) {
                    const T want = m == 3 ? fb[((long)t*n + m)*6 + j] : u[((long)t*nl + m*L + best[m])*6 + j];
                    bad += memcmp(&ub[((long)t*n + m)*6 + j], &want, sizeof(T)) != 0;
                }
        }
    }
    printf("costcheck selftest (%s): %ld rows of terms, 3 selections: %s\n", name, rows, bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
