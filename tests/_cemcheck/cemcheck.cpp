// cemcheck.cpp -- the two cross-entropy planner queries of so100_cem.hpp on the host, in double (held to the numpy reference) and in float (the
// arithmetic the kernels ship, without FMA contraction), behind a C interface for ctypes (built by tests/Makefile, loaded by tests/hostlibs.py and called by
// tests/cem_support.py).  Arrays are problem-major as in mppicheck.cpp: plan and sigma [T][n][6], qpos [n][13], qvel [n][12] -> ctrl [T][n K][6],
// qpos_rep [n K][13], qvel_rep [n K][12]; the refit's rollouts [T][n K][.], rollout (m, k) at m K + k, targets, fallback, plan and sigma per problem ->
// cost [n K], best [n], best_cost [n], elite [n][E], n_elite [n], threshold [n], mean [T][n][6], sigma_out [T][n][6], u_first [n][6].  def and w:
// costcheck.cpp's.  The elites are found by std::sort under cem_before -- not the kernel's sort of cem_key: cm_key_disagreements holds the two orders
// to each other.  Test scaffolding only.
#include <algorithm>
#include <vector>
#include "../planner_twin.hpp"
#include "../../so100_mujoco_rl_amd/csrc/so100_cem.hpp"

using namespace so100;
using planner_twin::make_def; using planner_twin::rollout_cost;

namespace {

// ctrl, qpos_rep and qvel_rep may each be null; qpos_rep needs qpos, qvel_rep needs qvel
template <typename T> void sample(long n, int K, int steps, const T* plan, const T* sigma, T lo, T hi, unsigned long long seed, unsigned draw, unsigned id_offset,
                                  const T* qpos, const T* qvel, T* ctrl, T* qpos_rep, T* qvel_rep) {
    planner_twin::sample<T>(n, K, steps, seed, draw, id_offset, qpos, qvel, ctrl, qpos_rep, qvel_rep,
                            [&](long e, int, T eps, bool perturbed) { return cem_candidate<T>(plan[e], sigma[e], eps, perturbed, lo, hi); });
}

// bad_step, u_fallback, plan and sigma may be null (the last two only with alpha = 0)
template <typename T> void refit(long n, int steps, int K, int link, int target_mode, const T* w, const T* target, const T* qpos, const T* qvel, const T* u,
                                 const int32_t* bad_step, const T* u_fallback, int E, T alpha, const T* plan, const T* sigma, const T* smin, const T* smax, const T* sinit,
                                 int shift, int tail, T* cost, int32_t* best, T* best_cost, int32_t* elite, int32_t* n_elite, T* threshold, T* mean, T* sigma_out, T* u_first) {
    const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
    const CostDef<T> c = make_def(link, target_mode, w);
    const long nk = n*K;
    std::vector<int> order(K);
    std::vector<char> is_elite(K);
    for (long m = 0; m < n; m++) {
        T* J = cost + m*K;
        for (int k = 0; k < K; k++) {
            J[k] = rollout_cost<T>(c, steps, n, nk, m, m*K + k, target, qpos, qvel, u, bad_step);
            order[k] = k;
        }
        std::sort(order.begin(), order.end(), [&](int a, int b) { return cem_before<T>(J[a], a, J[b], b); });
        int ne = 0;
        while (ne < E && J[order[ne]] < inf) ne++;
        for (int r = 0; r < K; r++) is_elite[order[r]] = r < ne;
        for (int r = 0; r < E; r++) elite[m*E + r] = r < ne ? order[r] : -1;
        best[m] = ne > 0 ? order[0] : -1; best_cost[m] = J[order[0]];
        n_elite[m] = ne; threshold[m] = ne > 0 ? J[order[ne - 1]] : inf;
        for (int t = 0; t < steps; t++)
            for (int j = 0; j < 6; j++) {
                const long e = ((long)t*n + m)*6 + j;
                const auto uk = [&](int k) { return u[((long)t*nk + m*K + k)*6 + j]; };
                T x, s;
                if (ne > 0) {
                    const T mu = cem_mean(mppi_sum<T>(K, [&](int k) { return cem_sum_term<T>(is_elite[k], uk(k)); }), ne);
                    const T sd = cem_sd(mppi_sum<T>(K, [&](int k) { return cem_dev_term<T>(is_elite[k], uk(k), mu); }), ne);
                    const bool old = alpha > T(0);
                    x = cem_mix<T>(alpha, old ? plan[e] : T(0), mu);
                    s = cem_sigma<T>(alpha, old ? sigma[e] : T(0), sd, smin[j], smax[j]);
                } else {
                    x = u_fallback ? u_fallback[e] : nan;
                    s = sinit[j];
                }
                mppi_place<T>(t, steps, shift, tail, x, [&](int row, T y) { mean[((long)row*n + m)*6 + j] = y; }, [&](T y) { u_first[m*6 + j] = y; });
                cem_place_sigma<T>(t, steps, shift, s, sinit[j], [&](int row, T y) { sigma_out[((long)row*n + m)*6 + j] = y; });
            }
    }
}

// over all pairs of (J[a], a), (J[b], b): how often the integer keys' order is not cem_before's
long key_disagreements(long count, const float* J) {
    long bad = 0;
    for (long a = 0; a < count; a++)
        for (long b = 0; b < count; b++)
            bad += (cem_key(J[a], (int)a) < cem_key(J[b], (int)b)) != cem_before<float>(J[a], (int)a, J[b], (int)b);
    for (long a = 0; a < count; a++) bad += !(cem_key(J[a], (int)a) < cem_key_pad(0)) || cem_key_index(cem_key(J[a], (int)a)) != (int)a;
    return bad;
}

}  // namespace

extern "C" {

#define CM_INSTANCE(S, T) \
    void cm_sample_##S(long n, int K, int steps, const T* plan, const T* sigma, T lo, T hi, unsigned long long seed, unsigned draw, unsigned id_offset, \
                       const T* qpos, const T* qvel, T* ctrl, T* qpos_rep, T* qvel_rep) { \
        sample<T>(n, K, steps, plan, sigma, lo, hi, seed, draw, id_offset, qpos, qvel, ctrl, qpos_rep, qvel_rep); } \
    void cm_refit_##S(long n, int steps, int K, int link, int target_mode, const T* w, const T* target, const T* qpos, const T* qvel, const T* u, \
                      const int32_t* bad_step, const T* u_fallback, int E, T alpha, const T* plan, const T* sigma, const T* smin, const T* smax, const T* sinit, \
                      int shift, int tail, T* cost, int32_t* best, T* best_cost, int32_t* elite, int32_t* n_elite, T* threshold, T* mean, T* sigma_out, T* u_first) { \
        refit<T>(n, steps, K, link, target_mode, w, target, qpos, qvel, u, bad_step, u_fallback, E, alpha, plan, sigma, smin, smax, sinit, shift, tail, \
                 cost, best, best_cost, elite, n_elite, threshold, mean, sigma_out, u_first); }
CM_INSTANCE(d, double)
CM_INSTANCE(f, float)
#undef CM_INSTANCE
long cm_key_disagreements(long count, const float* J) { return key_disagreements(count, J); }

}  // extern "C"

#ifdef CEMCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions, K on both sides of a wave and of a workgroup, both shifts and tails, alpha 0 and 0.25; the
// sampler under a sigma of 0 and one that cannot be used, the elite list against a plain count of who stands before whom, the bounds on sigma_out,
// E = K = 1, a problem that failed throughout, and the integer keys' order
#include <stdio.h>
namespace {
uint32_t g_state = 977u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0; }

template <typename T> int run(const char* name) {
    int bad = 0; long cases = 0;
    const T inf = std::numeric_limits<T>::infinity();
    T w[29];
    w[0] = T(0.01); w[1] = T(-0.05); w[2] = T(0.02); w[3] = T(1.5);
    for (int j = 0; j < 6; j++) { w[4 + j] = T(j == 2 ? 0 : 0.1*(j + 1)); w[10 + j] = T(0.2*(uniform() - 0.5)); w[16 + j] = T(0.01*(j + 1)); w[22 + j] = T(j == 5 ? 0 : 1e-3); }
    w[28] = T(3);
    const T smin[6] = { T(0.01), T(0.02), T(0), T(0.3), T(0.01), T(0) }, smax[6] = { T(1), T(0.5), T(2), T(0.3), T(0.02), T(0) };
    const T sinit[6] = { T(0.5), T(0.25), T(0), T(1), T(0.5), T(0.125) };
    const int Ks[] = { 1, 3, 64, 65, 257 };
    for (int K : Ks)
        for (int shift = 0; shift < 2; shift++)
            for (int tail = 0; tail < 2; tail++) {
                const long n = 3, nk = n*K; const int steps = 3, mode = (K + shift) % 3, E = K == 1 ? 1 : (tail ? (K + 7)/8 : K - 1);
                const T alpha = shift ? T(0.25) : T(0);
                std::vector<T> plan(6*n*steps), sg(6*n*steps), q0(13*n), v0(12*n), ctrl(6*nk*steps), qr(13*nk), vr(12*nk);
                for (auto& x : plan) x = T(2.4*(uniform() - 0.5));
                for (auto& x : sg) x = T(uniform());
                sg[0] = T(0); sg[6*n*steps - 1] = T(-1);                                      // entry (0, 0, 0) is never perturbed; the last one cannot be used
                for (auto& x : q0) x = T(uniform());
                for (auto& x : v0) x = T(uniform());
                sample<T>(n, K, steps, plan.data(), sg.data(), T(-1), T(1), 0x123456789abcdefULL, 7u, 40u, q0.data(), v0.data(), ctrl.data(), qr.data(), vr.data());
                for (int t = 0; t < steps; t++)
                    for (long m = 0; m < n; m++)
                        for (int j = 0; j < 6; j++) {
                            const long e = ((long)t*n + m)*6 + j;
                            const T p = plan[e], c0 = p < T(-1) ? T(-1) : (p > T(1) ? T(1) : p);
                            bad += memcmp(&ctrl[((long)t*nk + m*K)*6 + j], &c0, sizeof(T)) != 0;
                            for (int k = 1; k < K; k++) {
                                const T x = ctrl[((long)t*nk + m*K + k)*6 + j];
                                if (e == 6*n*steps - 1) bad += x == x;
                                else bad += !(x >= T(-1) && x <= T(1));
                                if (e == 0) bad += memcmp(&x, &c0, sizeof(T)) != 0;
                            }
                        }
                for (long col = 0; col < nk; col++) bad += memcmp(&qr[13*col], &q0[13*(col/K)], 13*sizeof(T)) != 0 || memcmp(&vr[12*col], &v0[12*(col/K)], 12*sizeof(T)) != 0;
                std::vector<T> qpos(13*nk*steps), qvel(12*nk*steps), target(3*n*steps), fb(6*n*steps), uu(6*nk*steps);
                for (auto& x : qpos) x = T(1.2*(uniform() - 0.5));
                for (auto& x : qvel) x = T(4*(uniform() - 0.5));
                for (auto& x : target) x = T(0.6*(uniform() - 0.5));
                for (auto& x : fb) x = T(uniform());
                for (auto& x : uu) x = T(2*(uniform() - 0.5));
                std::vector<int32_t> bs(nk, -1), best(n), el(n*E), ne(n);
                for (int k = 0; k < K; k++) bs[1*K + k] = 0;                                  // problem 1 fails throughout
                if (K > 2) bs[2*K + 1] = 2;                                                   // and one rollout of problem 2
                std::vector<T> cost(nk), bc(n), th(n), mean(6*n*steps), so(6*n*steps), uf(6*n);
                refit<T>(n, steps, K, 4, mode, w, target.data(), qpos.data(), qvel.data(), uu.data(), bs.data(), fb.data(), E, alpha, plan.data(), sg.data(), smin, smax, sinit,
                         shift, tail, cost.data(), best.data(), bc.data(), el.data(), ne.data(), th.data(), mean.data(), so.data(), uf.data());
                for (long m = 0; m < n; m++) {
                    if (m == 1) {
                        bad += best[m] != -1 || ne[m] != 0 || th[m] != inf || bc[m] != inf;
                        for (int r = 0; r < E; r++) bad += el[m*E + r] != -1;
                        for (int j = 0; j < 6; j++) {
                            bad += memcmp(&uf[m*6 + j], &fb[m*6 + j], sizeof(T)) != 0;
                            bad += memcmp(&mean[m*6 + j], &fb[((long)(shift ? 1 : 0)*n + m)*6 + j], sizeof(T)) != 0;
                            for (int t = 0; t < steps; t++) bad += memcmp(&so[((long)t*n + m)*6 + j], &sinit[j], sizeof(T)) != 0;
                        }
                        continue;
                    }
                    int finite = 0;
                    for (int k = 0; k < K; k++) finite += cost[m*K + k] < inf;
                    bad += ne[m] != (E < finite ? E : finite) || best[m] != el[m*E] || bc[m] != cost[m*K + best[m]] || th[m] != cost[m*K + el[m*E + ne[m] - 1]];
                    for (int r = 0; r < E; r++) {
                        const int k = el[m*E + r];
                        if (r >= ne[m]) { bad += k != -1; continue; }
                        int before = 0;
                        for (int k2 = 0; k2 < K; k2++) before += cem_before<T>(cost[m*K + k2], k2, cost[m*K + k], k);
                        bad += before != r;
                    }
                    for (int t = 0; t < steps; t++)
                        for (int j = 0; j < 6; j++) {
                            const T s = so[((long)t*n + m)*6 + j];
                            bad += (shift && t == steps - 1) ? memcmp(&s, &sinit[j], sizeof(T)) != 0 : !(s >= smin[j] && s <= smax[j]);
                            if (K == 1 && !shift) bad += memcmp(&mean[((long)t*n + m)*6 + j], &uu[((long)t*nk + m)*6 + j], sizeof(T)) != 0 || s != smin[j];
                        }
                }
                cases++;
            }
    printf("cemcheck selftest (%s): %ld cases: %s\n", name, cases, bad ? "FAILED" : "ok");
    return bad;
}

int keys() {
    std::vector<float> J;
    const float inf = std::numeric_limits<float>::infinity();
    for (float x : { 0.0f, -0.0f, 1e-45f, -1e-45f, 1.0f, 1.0f, -1.0f, 3.4e38f, -3.4e38f, inf, inf, -inf, 0.5f, 0.5f }) J.push_back(x);
    for (int i = 0; i < 50; i++) J.push_back((float)(8.0*(uniform() - 0.5)));
    const long bad = key_disagreements((long)J.size(), J.data());
    printf("cemcheck selftest (keys): %ld costs: %s\n", (long)J.size(), bad ? "FAILED" : "ok");
    return bad != 0;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float") + keys();
    return bad != 0;
}
#endif
