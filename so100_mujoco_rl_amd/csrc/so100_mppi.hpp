// so100_mppi.hpp -- the two sampling-planner queries of include/so100_query.h (so100_query_plan_sample, so100_query_cost_blend):
// what they compute per candidate and per problem, written once.  The rollout between them is the trajectory query's, the cost of a rollout is
// so100_cost.hpp's cost_total; nothing here restates either.
//
// Sample.  Candidate (n, k) of a plan entry p = plan[t][j][n]:  clamp(p + sigma_j eps(n, k, t, j), u_lo, u_hi), the product and the sum each
// rounded once (trajectory_rounded: the kernels are built with contraction).  Candidate 0 and a dimension with sigma_j = 0 are clamp(p) itself --
// no sum is formed, so a -0 stays a -0 -- and a p that is not finite is NaN in every candidate.  eps: policy_noise's scheme on a stream of its
// own, counter (id_offset + n, draw, k, MPPI_STREAM_C3 | t << 1 | b).
//
// Blend.  Per problem, over its K costs J_k (+inf: not a candidate):
//     best, J_min   the smallest, ties to the lowest index (an exact minimum: mppi_min_take is a total order on (J, k))
//     e_k = exp(-(J_k - J_min) / lambda), 0 where J_k = +inf;  w_k = e_k / sum e;  ess = 1 / sum w_k^2;  row (t, j) of the blend = sum_k w_k u[t][j][k]
// Every sum over k is taken in ONE order that depends on K alone -- the order of a 64-lane wave: lane l adds the terms k = l, l + 64, ... in
// ascending order (mppi_lane_sum), then the 64 partial sums meet in the exchange tree over lane distances 32, 16, .., 1 (mppi_tree_sum on the
// host; the kernel makes the same tree of lane exchanges).  IEEE addition commutes, so after the tree every lane holds the same bits.  A term
// with w_k = 0 is not formed: a failed rollout's controls may be anything.  Products are rounded before they are added, as above.
//
// Templated on the scalar T: float on the device; float / double host instantiations exist ONLY for the CPU-side tests in tests/_mppicheck.
#pragma once
#include "so100_cost.hpp"
#include "so100_task.hpp"           // philox4x32, policy_noise_pair
#include "so100_trajectory.hpp"     // trajectory_rounded

namespace so100 {

constexpr int MPPI_MAX_K = 4096, MPPI_WAVE = 64;               // SO100_MPPI_MAX_K; the width of the summation order
constexpr int BLEND_TAIL_ZERO = 0, BLEND_TAIL_HOLD = 1;        // SO100_BLEND_TAIL_*
constexpr uint32_t MPPI_STREAM_C3 = 0x4D500000u;               // neither 0 (draw8) nor 0x504F4C (policy_noise): t <= 4095 keeps the low field under 2^13

// Box-Muller of two words: policy_noise_pair in float; the same formula in double for the fp64 twin
SO100_HD void mppi_noise_pair(uint32_t r_even, uint32_t r_odd, float& e0, float& e1) { policy_noise_pair(r_even, r_odd, e0, e1); }
SO100_HD void mppi_noise_pair(uint32_t r_even, uint32_t r_odd, double& e0, double& e1) {
    const double u1 = ((double)(r_even >> 8) + 1.0) * (1.0/16777216.0);
    const double u2 = (double)(r_odd >> 8) * (1.0/16777216.0);
    const double rad = __builtin_sqrt(-2.0*__builtin_log(u1)), ang = 6.283185307179586*u2 - 3.141592653589793;
    e0 = rad*__builtin_cos(ang); e1 = rad*__builtin_sin(ang);
}

// the eight standard normals of (problem gid, draw, candidate k, step t); the first six are the controls' j = 0..5
template <typename T> SO100_HD void mppi_noise(uint32_t gid, uint32_t draw, uint32_t k, int t, uint32_t seed_lo, uint32_t seed_hi, T eps[8]) {
#pragma unroll
    for (int b = 0; b < 2; b++) {
        uint32_t r[4];
        philox4x32(gid, draw, k, MPPI_STREAM_C3 | ((uint32_t)t << 1) | (uint32_t)b, seed_lo, seed_hi, r);
#pragma unroll
        for (int i = 0; i < 2; i++) mppi_noise_pair(r[2*i], r[2*i + 1], eps[4*b + 2*i], eps[4*b + 2*i + 1]);
    }
}

// one entry of a candidate; perturbed: k > 0 (the caller's sigma decides the rest).  The comparisons keep a NaN where fmin / fmax would drop it.
template <typename T> SO100_HD T mppi_candidate(T p, T sigma, T eps, bool perturbed, T lo, T hi) {
    if (!cost_finite(p)) return p*T(0);                        // NaN for a NaN and for an infinity
    const T x = (perturbed && sigma != T(0)) ? p + trajectory_rounded(sigma*eps) : p;
    return x < lo ? lo : (x > hi ? hi : x);
}

// ---- the one summation order ----
// lane's partial sum of term(k), k = lane, lane + 64, ... < K, ascending.  It starts from -0, the one value x + (-0) = x holds for to the bit (a
// sum of the single term -0 is -0: K = 1 returns its candidate's controls as they are); a lane at or behind K keeps it
template <typename T, typename Term> SO100_HD T mppi_lane_sum(int K, int lane, Term&& term) {
    T s = T(-0.0);
    for (int k = lane; k < K; k += MPPI_WAVE) s += term(k);
    return s;
}
// the host's form of the exchange tree over 64 partial sums (the kernel: x += lane_exchange(x, d) for d = 32 .. 1)
template <typename T> inline T mppi_tree_sum(T p[MPPI_WAVE]) {
    for (int d = MPPI_WAVE/2; d >= 1; d >>= 1) {
        T n[MPPI_WAVE];
        for (int l = 0; l < MPPI_WAVE; l++) n[l] = p[l] + p[l ^ d];
        for (int l = 0; l < MPPI_WAVE; l++) p[l] = n[l];
    }
    return p[0];
}
template <typename T, typename Term> inline T mppi_sum(int K, Term&& term) {
    T p[MPPI_WAVE];
    for (int l = 0; l < MPPI_WAVE; l++) p[l] = mppi_lane_sum<T>(K, l, term);
    return mppi_tree_sum(p);
}

// ---- the minimum: (J, k) in lexicographic order; MPPI_NONE: no candidate below +inf yet ----
constexpr int MPPI_NONE = 0x7FFFFFFF;
template <typename T> SO100_HD void mppi_min_take(T& c, int& i, T c2, int i2) {
    if (c2 < c || (c2 == c && i2 < i)) { c = c2; i = i2; }
}
// a lane's share of the scan: k = lane, lane + stride, ...; a cost of +inf never enters (c starts there)
template <typename T, typename Get> SO100_HD void mppi_lane_min(int K, int lane, int stride, T inf, Get&& get, T& c, int& i) {
    c = inf; i = MPPI_NONE;
    for (int k = lane; k < K; k += stride) { const T x = get(k); if (x < c) { c = x; i = k; } }
}

// e_k: the weight before it is normalised
SO100_HD float mppi_exp(float x) { return __builtin_expf(x); }
SO100_HD double mppi_exp(double x) { return __builtin_exp(x); }
template <typename T> SO100_HD T mppi_unnormalised(T J, T J_min, T lambda, T inf) { return J == inf ? T(0) : mppi_exp(-(J - J_min)/lambda); }
// a term of a blended row; w = 0 forms no product
template <typename T> SO100_HD T mppi_term(T w, T u) { return w != T(0) ? trajectory_rounded(w*u) : T(-0.0); }

// where blended row t (value x) goes: put(row, value) into u_plan, first(value) into u_first
template <typename T, typename Put, typename First> SO100_HD void mppi_place(int t, int steps, int shift, int tail, T x, Put&& put, First&& first) {
    if (t == 0) first(x);
    if (!shift) { put(t, x); return; }
    if (t >= 1) put(t - 1, x);
    if (t == steps - 1) put(t, tail == BLEND_TAIL_HOLD ? x : T(0));
}

}  // namespace so100
