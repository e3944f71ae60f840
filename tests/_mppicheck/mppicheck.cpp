// mppicheck.cpp -- the two sampling-planner queries of so100_mppi.hpp on the host, in double (held to the numpy reference) and in float (the
// arithmetic the kernels ship, without FMA contraction), behind a C interface for ctypes (built by tests/Makefile, loaded by tests/hostlibs.py and called by
// tests/mppi_support.py).  Arrays are problem-major here: plan [T][n][6], qpos [n][13], qvel [n][12] -> ctrl [T][n K][6], qpos_rep [n K][13],
// qvel_rep [n K][12]; the blend's rollouts as costcheck.cpp's select takes them ([T][n K][.], rollout (m, k) at m K + k, targets and fallback per
// problem) -> cost [n K], best [n], best_cost [n], weight [n K], ess [n], u_plan [T][n][6], u_first [n][6].  def and w: costcheck.cpp's.  Test scaffolding only.
#include "../planner_twin.hpp"

using namespace so100;
using planner_twin::make_def; using planner_twin::rollout_cost;

namespace {

// ctrl, qpos_rep and qvel_rep may each be null; qpos_rep needs qpos, qvel_rep needs qvel
template <typename T> void sample(long n, int K, int steps, const T* plan, const T* sigma, T lo, T hi, unsigned long long seed, unsigned draw, unsigned id_offset,
                                  const T* qpos, const T* qvel, T* ctrl, T* qpos_rep, T* qvel_rep) {
    planner_twin::sample<T>(n, K, steps, seed, draw, id_offset, qpos, qvel, ctrl, qpos_rep, qvel_rep,
                            [&](long e, int j, T eps, bool perturbed) { return mppi_candidate<T>(plan[e], sigma[j], eps, perturbed, lo, hi); });
}

// bad_step and u_fallback may be null
template <typename T> void blend(long n, int steps, int K, int link, int target_mode, const T* w, const T* target, const T* qpos, const T* qvel, const T* u,
                                 const int32_t* bad_step, const T* u_fallback, T lambda, int shift, int tail,
                                 T* cost, int32_t* best, T* best_cost, T* weight, T* ess, T* u_plan, T* u_first) {
    const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
    const CostDef<T> c = make_def(link, target_mode, w);
    const long nk = n*K;
    for (long m = 0; m < n; m++) {
        T* J = cost + m*K; T* wt = weight + m*K;
        for (int k = 0; k < K; k++) {
            J[k] = rollout_cost<T>(c, steps, n, nk, m, m*K + k, target, qpos, qvel, u, bad_step);
        }
        T j_min; int arg;
        mppi_lane_min<T>(K, 0, 1, inf, [&](int k) { return J[k]; }, j_min, arg);         // one scan: the order of (J, k) is total
        const int b = arg == MPPI_NONE ? -1 : arg;
        best[m] = b; best_cost[m] = j_min;
        for (int k = 0; k < K; k++) wt[k] = mppi_unnormalised<T>(J[k], j_min, lambda, inf);
        const T sum_e = mppi_sum<T>(K, [&](int k) { return wt[k]; });
        for (int k = 0; k < K; k++) wt[k] = b >= 0 ? wt[k]/sum_e : T(0);
        const T s2 = mppi_sum<T>(K, [&](int k) { return trajectory_rounded(wt[k]*wt[k]); });
        ess[m] = b >= 0 ? T(1)/s2 : T(0);
        for (int t = 0; t < steps; t++)
            for (int j = 0; j < 6; j++) {
                T x;
                if (b >= 0) x = mppi_sum<T>(K, [&](int k) { return mppi_term<T>(wt[k], u[((long)t*nk + m*K + k)*6 + j]); });
                else x = u_fallback ? u_fallback[((long)t*n + m)*6 + j] : nan;
                mppi_place<T>(t, steps, shift, tail, x, [&](int row, T y) { u_plan[((long)row*n + m)*6 + j] = y; }, [&](T y) { u_first[m*6 + j] = y; });
            }
    }
}

}  // namespace

extern "C" {

#define MP_INSTANCE(S, T) \
    void mp_sample_##S(long n, int K, int steps, const T* plan, const T* sigma, T lo, T hi, unsigned long long seed, unsigned draw, unsigned id_offset, \
                       const T* qpos, const T* qvel, T* ctrl, T* qpos_rep, T* qvel_rep) { \
        sample<T>(n, K, steps, plan, sigma, lo, hi, seed, draw, id_offset, qpos, qvel, ctrl, qpos_rep, qvel_rep); } \
    void mp_blend_##S(long n, int steps, int K, int link, int target_mode, const T* w, const T* target, const T* qpos, const T* qvel, const T* u, \
                      const int32_t* bad_step, const T* u_fallback, T lambda, int shift, int tail, \
                      T* cost, int32_t* best, T* best_cost, T* weight, T* ess, T* u_plan, T* u_first) { \
        blend<T>(n, steps, K, link, target_mode, w, target, qpos, qvel, u, bad_step, u_fallback, lambda, shift, tail, cost, best, best_cost, weight, ess, u_plan, u_first); }
MP_INSTANCE(d, double)
MP_INSTANCE(f, float)
#undef MP_INSTANCE

}  // extern "C"

#ifdef MPPICHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions, K on both sides of a wave and of a workgroup, both shifts and tails; candidate 0 is the
// clamped plan, a sigma of 0 perturbs nothing, the bounds hold, the weights sum to 1, K = 1 returns its candidate, a failed problem takes the fallback
#include <stdio.h>
#include <vector>
namespace {
uint32_t g_state = 2031u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0; }

template <typename T> int run(const char* name) {
    int bad = 0; long cases = 0;
    T w[29];
    w[0] = T(0.01); w[1] = T(-0.05); w[2] = T(0.02); w[3] = T(1.5);
    for (int j = 0; j < 6; j++) { w[4 + j] = T(j == 2 ? 0 : 0.1*(j + 1)); w[10 + j] = T(0.2*(uniform() - 0.5)); w[16 + j] = T(0.01*(j + 1)); w[22 + j] = T(j == 5 ? 0 : 1e-3); }
    w[28] = T(3);
    const T sigma[6] = { T(0.5), T(0.25), T(0), T(1), T(0.5), T(0) };
    const int Ks[] = { 1, 3, 64, 65, 257 };
    for (int K : Ks)
        for (int shift = 0; shift < 2; shift++)
            for (int tail = 0; tail < 2; tail++) {
                const long n = 3, nk = n*K; const int steps = 3, mode = (K + shift) % 3;
                std::vector<T> plan(6*n*steps), q0(13*n), v0(12*n), ctrl(6*nk*steps), qr(13*nk), vr(12*nk);
                for (auto& x : plan) x = T(2.4*(uniform() - 0.5));
                for (auto& x : q0) x = T(uniform());
                for (auto& x : v0) x = T(uniform());
                sample<T>(n, K, steps, plan.data(), sigma, T(-1), T(1), 0x123456789abcdefULL, 7u, 40u, q0.data(), v0.data(), ctrl.data(), qr.data(), vr.data());
                for (int t = 0; t < steps; t++)
                    for (long m = 0; m < n; m++)
                        for (int j = 0; j < 6; j++) {
                            const T p = plan[((long)t*n + m)*6 + j], c0 = p < T(-1) ? T(-1) : (p > T(1) ? T(1) : p);
                            bad += memcmp(&ctrl[((long)t*nk + m*K)*6 + j], &c0, sizeof(T)) != 0;
                            for (int k = 0; k < K; k++) {
                                const T x = ctrl[((long)t*nk + m*K + k)*6 + j];
                                bad += !(x >= T(-1) && x <= T(1));
                                if (sigma[j] == T(0)) bad += memcmp(&x, &c0, sizeof(T)) != 0;
                            }
                        }
                for (long col = 0; col < nk; col++) bad += memcmp(&qr[13*col], &q0[13*(col/K)], 13*sizeof(T)) != 0 || memcmp(&vr[12*col], &v0[12*(col/K)], 12*sizeof(T)) != 0;
                std::vector<T> qpos(13*nk*steps), qvel(12*nk*steps), target(3*n*steps), fb(6*n*steps);
                for (auto& x : qpos) x = T(1.2*(uniform() - 0.5));
                for (auto& x : qvel) x = T(4*(uniform() - 0.5));
                for (auto& x : target) x = T(0.6*(uniform() - 0.5));
                for (auto& x : fb) x = T(uniform());
                std::vector<int32_t> bs(nk, -1), best(n);
                for (int k = 0; k < K; k++) bs[1*K + k] = 0;                                  // problem 1 fails throughout
                std::vector<T> cost(nk), bc(n), wt(nk), ess(n), up(6*n*steps), uf(6*n);
                blend<T>(n, steps, K, 4, mode, w, target.data(), qpos.data(), qvel.data(), ctrl.data(), bs.data(), fb.data(), T(0.5), shift, tail,
                         cost.data(), best.data(), bc.data(), wt.data(), ess.data(), up.data(), uf.data());
                for (long m = 0; m < n; m++) {
                    T s = T(0);
                    for (int k = 0; k < K; k++) { s += wt[m*K + k]; bad += !(wt[m*K + k] >= T(0)); }
                    if (m == 1) {
                        bad += best[m] != -1 || s != T(0) || ess[m] != T(0);
                        for (int j = 0; j < 6; j++) bad += memcmp(&uf[m*6 + j], &fb[m*6 + j], sizeof(T)) != 0;
                        const int src = shift ? (steps - 1) : 0;                             // row 0 of u_plan is the fallback's row `shift`
                        for (int j = 0; j < 6; j++) bad += memcmp(&up[m*6 + j], &fb[((long)(shift ? 1 : 0)*n + m)*6 + j], sizeof(T)) != 0;
                        for (int j = 0; j < 6 && shift; j++) {
                            const T want = tail == BLEND_TAIL_HOLD ? fb[((long)src*n + m)*6 + j] : T(0);
                            bad += memcmp(&up[((long)(steps - 1)*n + m)*6 + j], &want, sizeof(T)) != 0;
                        }
                        continue;
                    }
                    bad += best[m] < 0 || !(s > T(1) - T(1e-5) && s < T(1) + T(1e-5)) || !(ess[m] >= T(1) - T(1e-5) && ess[m] <= T(K)*(T(1) + T(1e-5)));
                    for (int k = 0; k < K; k++) bad += !(wt[m*K + best[m]] >= wt[m*K + k]);
                    if (K == 1 && !shift)
                        for (int t = 0; t < steps; t++)
                            for (int j = 0; j < 6; j++) bad += wt[m] != T(1) || memcmp(&up[((long)t*n + m)*6 + j], &ctrl[((long)t*nk + m)*6 + j], sizeof(T)) != 0;
                }
                cases++;
            }
    printf("mppicheck selftest (%s): %ld cases: %s\n", name, cases, bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
