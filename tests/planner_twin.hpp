// planner_twin.hpp -- what the host twins of the planner queries share (tests/_costcheck/costcheck.cpp, tests/_mppicheck/mppicheck.cpp,
// tests/_cemcheck/cemcheck.cpp): the cost definition from the 29 numbers the C interface takes, a rollout's cost on problem-major arrays, and the
// samplers' loop over candidates.  The arithmetic is so100_cost.hpp's and so100_mppi.hpp's; this is only how the twins hand it their arrays.
// Test scaffolding only.
#pragma once
#include <stdint.h>
#include <string.h>
#include <limits>
#include "../so100_mujoco_rl_amd/csrc/so100_mppi.hpp"

namespace planner_twin {

using namespace so100;

// w: offset 3, w_point, w_q 6, q_nom 6, w_v 6, w_u 6, w_terminal (29 numbers)
template <typename T> CostDef<T> make_def(int link, int target_mode, const T* w) {
    CostDef<T> c;
    c.link = link; c.target_mode = target_mode;
    for (int i = 0; i < 3; i++) c.o[i] = w[i];
    c.w_point = w[3];
    for (int j = 0; j < 6; j++) { c.w_q[j] = w[4 + j]; c.q_nom[j] = w[10 + j]; c.w_v[j] = w[16 + j]; c.w_u[j] = w[22 + j]; }
    c.w_terminal = w[28];
    return c;
}

// the target of problem m at step t: the cube of the state row qpos_row, or target [n][3] / [T][n][3]
template <typename T> void target_of(const CostDef<T>& c, const T* target, const T* qpos_row, long n, long m, int t, T g[3]) {
    for (int i = 0; i < 3; i++)
        g[i] = c.target_mode == COST_TARGET_CUBE ? qpos_row[6 + i] : target[((c.target_mode == COST_TARGET_TRAJ ? (long)t*n : 0) + m)*3 + i];
}

// what rollout `col` (of `columns`; qpos [T][columns][13], qvel [T][columns][12] or null, u [T][columns][6]) of problem m (of n) costs: +inf where
// it failed (bad_step may be null) or its sum is not finite
template <typename T> T rollout_cost(const CostDef<T>& c, int steps, long n, long columns, long m, long col, const T* target, const T* qpos, const T* qvel,
                                     const T* u, const int32_t* bad_step) {
    const T total = cost_total<T>(c, steps, [&](int t, T q[6], T v[6], T uu[6], T g[3]) {
        const long p = (long)t*columns + col;
        for (int j = 0; j < 6; j++) { q[j] = qpos[13*p + j]; v[j] = qvel ? qvel[12*p + j] : T(0); uu[j] = u[6*p + j]; }
        target_of(c, target, qpos + 13*p, n, m, t, g);
    });
    return ((bad_step && bad_step[col] >= 0) || !cost_finite(total)) ? std::numeric_limits<T>::infinity() : total;
}

// the K candidates of each of n plans [T][n][6] -> ctrl [T][n K][6], and the start states' fan-out; ctrl, qpos_rep and qvel_rep may each be null,
// qpos_rep needs qpos, qvel_rep needs qvel.  candidate(e, j, eps, perturbed): the value from plan entry e = (t n + m) 6 + j
template <typename T, typename Candidate>
void sample(long n, int K, int steps, unsigned long long seed, unsigned draw, unsigned id_offset, const T* qpos, const T* qvel, T* ctrl, T* qpos_rep, T* qvel_rep,
            Candidate&& candidate) {
    const long nk = n*K;
    for (long m = 0; m < n; m++)
        for (int k = 0; k < K; k++) {
            const long col = m*K + k;
            for (int t = 0; t < steps && ctrl; t++) {
                T eps[8];
                mppi_noise<T>((uint32_t)(id_offset + (uint32_t)m), draw, (uint32_t)k, t, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), eps);
                for (int j = 0; j < 6; j++) ctrl[((long)t*nk + col)*6 + j] = candidate(((long)t*n + m)*6 + j, j, eps[j], k > 0);
            }
            if (qpos_rep) memcpy(qpos_rep + 13*col, qpos + 13*m, 13*sizeof(T));
            if (qvel_rep) memcpy(qvel_rep + 12*col, qvel + 12*m, 12*sizeof(T));
        }
}

}  // namespace planner_twin
