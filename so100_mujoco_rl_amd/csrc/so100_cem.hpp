// so100_cem.hpp -- the two cross-entropy planner queries of include/so100_query.h (so100_query_plan_sample_tv, so100_query_cost_refit; DESIGN.md
// section 19): what they compute per candidate and per problem, written once.  The noise, the candidate, the summation order, the minimum's total
// order and the placement of a shifted plan are so100_mppi.hpp's, the cost of a rollout is so100_cost.hpp's cost_total; nothing here restates them.
//
// Sample.  so100_mppi.hpp's candidate with a sigma per (step, joint, problem) read from memory: a sigma that is negative or not finite cannot be
// refused on the host, so that entry is NaN in every perturbed candidate (cem_candidate); with a sigma that is finite and >= 0 the entry IS
// mppi_candidate's, to the bit.
//
// Refit.  Per problem, over its K costs J_k (+inf: not a candidate):
//     order        k before k' iff J_k < J_k' or (J_k = J_k' and k < k'): mppi_min_take's total order (cem_before); rank(k): how many stand before k
//     elites       rank(k) < E and J_k < +inf;  n = min(E, the number of finite costs);  threshold: the cost of the elite of rank n - 1
//     row (t, j)   mu = (sum_elites u_k) / n;  var = (sum_elites (u_k - mu)^2) / n;  sd = sqrt(var)          (two passes, each product rounded once)
//                  mean_new = alpha plan + (1 - alpha) mu;  sigma_new = clamp(alpha sigma + (1 - alpha) sd, sigma_min_j, sigma_max_j)
//                  (cem_mix: each product rounded once; with alpha = 0 the old value's term is not formed and the new one is taken as it is)
// The order is total, so the elite set does not depend on how it is found: the kernel sorts 64-bit keys (cem_key: the order-preserving integer
// image of J above k), the host twin sorts pairs with cem_before; tests/_cemcheck holds the two orders to each other.  Both sums run in so100_mppi.hpp's
// ONE order over k = 0..K-1 (mppi_lane_sum, then the exchange tree); a non-elite's term is not formed (the -0 that adds nothing stands for it), so
// its controls may be anything and the bits depend on K and the elite set alone.
//
// Templated on the scalar T: float on the device; float / double host instantiations exist ONLY for the CPU-side tests in tests/_cemcheck.
#pragma once
#include "so100_mppi.hpp"

namespace so100 {

// ---- the sampler's candidate under a sigma from memory ----
template <typename T> SO100_HD T cem_candidate(T p, T sigma, T eps, bool perturbed, T lo, T hi) {
    if (perturbed && !(cost_finite(sigma) && sigma >= T(0))) return T(__builtin_nanf(""));
    return mppi_candidate<T>(p, sigma, eps, perturbed, lo, hi);
}

// ---- the order ----
template <typename T> SO100_HD bool cem_before(T J, int k, T J2, int k2) { return J < J2 || (J == J2 && k < k2); }
// the same order on integers: cem_key(J, k) < cem_key(J2, k2) iff cem_before(J, k, J2, k2), for costs that are not NaN (-0 and +0 are one cost).
// A key above CEM_KEY_PAD's high word belongs to no cost: the padding of a sort to a power of two
constexpr uint32_t CEM_KEY_PAD = 0xFFFFFFFFu;
SO100_HD uint64_t cem_key(float J, int k) {
    const float c = J == 0.0f ? 0.0f : J;
    uint32_t b;
    __builtin_memcpy(&b, &c, sizeof b);
    const uint32_t image = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)image << 32) | (uint32_t)k;
}
SO100_HD uint64_t cem_key_pad(int i) { return ((uint64_t)CEM_KEY_PAD << 32) | (uint32_t)i; }
SO100_HD int cem_key_index(uint64_t key) { return (int)(uint32_t)key; }

// ---- a row's statistics over the elites; n >= 1 is their number ----
SO100_HD float cem_sqrt(float x) { return __builtin_sqrtf(x); }
SO100_HD double cem_sqrt(double x) { return __builtin_sqrt(x); }
template <typename T> SO100_HD T cem_sum_term(bool elite, T u) { return elite ? u : T(-0.0); }
template <typename T> SO100_HD T cem_mean(T sum_u, int n) { return sum_u/T(n); }
template <typename T> SO100_HD T cem_dev_term(bool elite, T u, T mu) {
    if (!elite) return T(-0.0);
    const T d = u - mu;
    return trajectory_rounded(d*d);
}
template <typename T> SO100_HD T cem_sd(T sum_d2, int n) { return cem_sqrt(sum_d2/T(n)); }

// ---- the smoothing: alpha old + (1 - alpha) x; old is read by the caller only where alpha > 0 ----
template <typename T> SO100_HD T cem_mix(T alpha, T old, T x) {
    return alpha > T(0) ? trajectory_rounded(alpha*old) + trajectory_rounded((T(1) - alpha)*x) : x;
}
template <typename T> SO100_HD T cem_sigma(T alpha, T old, T sd, T lo, T hi) {
    const T x = cem_mix(alpha, old, sd);
    return x < lo ? lo : (x > hi ? hi : x);
}

// where sigma_new of row t (value x) goes: mppi_place's move, the last row of a shifted sigma_out is sigma_init under either tail
template <typename T, typename Put> SO100_HD void cem_place_sigma(int t, int steps, int shift, T x, T init, Put&& put) {
    if (!shift) { put(t, x); return; }
    if (t >= 1) put(t - 1, x);
    if (t == steps - 1) put(t, init);
}

}  // namespace so100
