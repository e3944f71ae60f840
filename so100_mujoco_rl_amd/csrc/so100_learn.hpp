// so100_learn.hpp -- the per-sample / per-parameter arithmetic of the on-device PPO learner (include/so100_learn.h), as templates on the
// scalar type: the HIP kernels of so100_learn.hip instantiate them in float, tests/_learncheck instantiates them on the host in double and
// float and holds them to an fp64 PyTorch reference.  Nothing here touches memory layouts beyond a stride or a device builtin, and nothing
// but the shuffle at the end reads a header of the simulator: the file compiles with a plain host compiler.
//   gae_scan_env        rollout.bootstrap_truncated + PPO._gae for one env (SB3 RolloutBuffer.compute_returns_and_advantage)
//   ppo_loss_head       the PPO._step loss of one sample with its derivatives towards the network outputs
//   ppo_loss_head_ex    the same with SB3's entropy bonus, value clipping and approx_kl
//   clip_adam_update    clip_grad_norm_'s scaling + one torch.optim.Adam step of one parameter
//   return_step .. reward_scale   SB3's VecNormalize(norm_reward=True): the running return, block moments, Chan merge, running moments, scale
//   obs_block_tree_sum .. obs_normalized   SB3's VecNormalize(norm_obs=True): block moments, the two-level Chan merge, the fold, the normalised load
//   shuffle_index       one entry of an epoch's permutation (the one piece that reads the simulator: see there)
#pragma once
#include <stdint.h>
#include "so100_policy_tensors.h"

#ifndef SO100_LHD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SO100_LHD __host__ __device__ __forceinline__
#else
#define SO100_LHD inline
#endif
#endif

namespace so100 {
namespace learn {

constexpr int ACT_DIM = 6, HID = 64;
// the flat parameter block: the tensors of so100_policy_tensors.h in its order, each in nn.Linear layout weight[rows][cols].  The two
// shape functions stay written as conditions (the advantages kernel evaluates tensor_offset at run time: another body is other device
// code); the asserts below hold them to the table for both observation widths.
constexpr int tensor_rows(int t, int /*od*/) { return (t == T_mu_w || t == T_mu_b || t == T_log_std) ? ACT_DIM : (t == T_v_w || t == T_v_b) ? 1 : HID; }
constexpr int tensor_cols(int t, int od) { return (t == T_pi_w0 || t == T_vf_w0) ? od : (t == T_pi_w1 || t == T_vf_w1 || t == T_mu_w || t == T_v_w) ? HID : 1; }
constexpr int tensor_size(int t, int od) { return tensor_rows(t, od)*tensor_cols(t, od); }
constexpr int tensor_offset(int t, int od) { return t == 0 ? 0 : tensor_offset(t - 1, od) + tensor_size(t - 1, od); }
constexpr int num_params(int od) { return tensor_offset(NUM_TENSORS - 1, od) + tensor_size(NUM_TENSORS - 1, od); }
constexpr bool shapes_match_table(int od) {
#define X(name, rows, cols) if (tensor_rows(T_##name, od) != (rows) || tensor_cols(T_##name, od) != (cols)) return false;
    SO100_POLICY_TENSORS(X)
#undef X
    return true;
}
static_assert(NUM_TENSORS == 13 && shapes_match_table(15) && shapes_match_table(8), "so100_policy_tensors.h");
static_assert(num_params(15) == 10829 && num_params(8) == 9933, "SB3 MlpPolicy, 2 x 64 towers");

SO100_LHD float  lexp(float x)   { return __builtin_expf(x); }
SO100_LHD double lexp(double x)  { return __builtin_exp(x); }
SO100_LHD float  lsqrt(float x)  { return __builtin_sqrtf(x); }
SO100_LHD double lsqrt(double x) { return __builtin_sqrt(x); }

// ---- advantages ---------------------------------------------------------------------------------------------------------------------------
// One env, backwards over its T steps.  reward / code / value: the env's columns of the packed chunk, `in_stride` scalars between steps.
// boot: gamma-less V(terminal_observation) of the steps whose done code is 2, `out_stride` between steps, or null (no bootstrap); it may
// alias `ret` (entry t is read before ret[t] is written).  next_v_last = V(last_obs).  Returns nothing; adv / ret get T entries each.
// The reward has a stride of its own: with reward normalisation it comes from a dense [T][N] array, not from the chunk.
template <class S>
SO100_LHD void gae_scan_env(int T, const S* reward, long reward_stride, const S* code, const S* value, long in_stride, const S* boot, S next_v_last,
                            S gamma, S lam, S* adv, S* ret, long out_stride) {
    S g = S(0), next_v = next_v_last;
    for (int t = T - 1; t >= 0; t--) {
        const S c = code[t*in_stride], v = value[t*in_stride];
        S r = reward[t*reward_stride];
        if (boot != nullptr && c == S(2)) r += gamma*boot[t*out_stride];          // TimeLimit truncation only: not a terminal state
        const S nonterm = c == S(0) ? S(1) : S(0);
        const S delta = r + gamma*next_v*nonterm - v;
        g = delta + gamma*lam*nonterm*g;
        adv[t*out_stride] = g;
        ret[t*out_stride] = g + v;
        next_v = v;
    }
}

// the three columns of one packed chunk: one stride
template <class S>
SO100_LHD void gae_scan_env(int T, const S* reward, const S* code, const S* value, long in_stride, const S* boot, S next_v_last,
                            S gamma, S lam, S* adv, S* ret, long out_stride) {
    gae_scan_env<S>(T, reward, in_stride, code, value, in_stride, boot, next_v_last, gamma, lam, adv, ret, out_stride);
}

// ---- loss head ----------------------------------------------------------------------------------------------------------------------------
template <class S>
struct LossHead {
    S pg_loss, v_loss;             // this sample's -min(ratio A, clamp(ratio) A) and (ret - V)^2: the means over the minibatch are the stats
    S clipped;                     // 1 where |ratio - 1| > clip_range (SB3's clip_fraction), else 0
    S dmu[ACT_DIM], dlog_std[ACT_DIM], dV;     // d(minibatch loss)/d(this sample's outputs): already scaled by inv_mb (and vf_coef)
};

// The two towers meet only in the sum of the loss, so the head has a policy half and a value half; the kernels run one tower at a time and
// call the halves, ppo_loss_head is both.  adv_n = (adv - mean)/(std + 1e-8), formed by the caller.  torch's derivative conventions:
// min() splits a tie evenly, clamp() passes the gradient on its closed interval.
// policy_loss_core is policy_loss_head's arithmetic with the two intermediates the extended head needs handed out as well: the ratio and
// logp - logp_old.  policy_loss_head is the core with those dropped: the same expressions, the same results.
template <class S>
SO100_LHD void policy_loss_core(const S* mu, const S* log_std, const S* a, S logp_old, S adv_n, S clip, S inv_mb, LossHead<S>& o, S& ratio_out, S& log_ratio_out) {
    S z[ACT_DIM], inv_sigma[ACT_DIM], logp = S(0);
    for (int i = 0; i < ACT_DIM; i++) {
        inv_sigma[i] = lexp(-log_std[i]);
        z[i] = (a[i] - mu[i])*inv_sigma[i];
        logp += S(-0.5)*z[i]*z[i] - log_std[i] - S(0.9189385332046727);
    }
    const S ratio = lexp(logp - logp_old);
    const S lo = S(1) - clip, hi = S(1) + clip;
    const bool inside = ratio >= lo && ratio <= hi;
    const S s1 = ratio*adv_n, s2 = (ratio < lo ? lo : ratio > hi ? hi : ratio)*adv_n;
    o.pg_loss = -(s1 < s2 ? s1 : s2);
    o.clipped = (ratio - S(1) > clip || S(1) - ratio > clip) ? S(1) : S(0);
    const S w1 = s1 < s2 ? S(1) : s1 == s2 ? S(0.5) : S(0);
    const S dratio = -(w1*adv_n + (inside ? (S(1) - w1)*adv_n : S(0)));
    const S dlogp = dratio*ratio*inv_mb;
    for (int i = 0; i < ACT_DIM; i++) {
        o.dmu[i] = dlogp*z[i]*inv_sigma[i];
        o.dlog_std[i] = dlogp*(z[i]*z[i] - S(1));
    }
    ratio_out = ratio; log_ratio_out = logp - logp_old;
}

template <class S>
SO100_LHD void policy_loss_head(const S* mu, const S* log_std, const S* a, S logp_old, S adv_n, S clip, S inv_mb, LossHead<S>& o) {
    S ratio, log_ratio;
    policy_loss_core(mu, log_std, a, logp_old, adv_n, clip, inv_mb, o, ratio, log_ratio);
}

template <class S>
SO100_LHD void value_loss_head(S V, S ret, S vf_coef, S inv_mb, LossHead<S>& o) {
    const S e = V - ret;
    o.v_loss = e*e;
    o.dV = S(2)*vf_coef*e*inv_mb;
}

template <class S>
SO100_LHD LossHead<S> ppo_loss_head(const S* mu, const S* log_std, const S* a, S logp_old, S adv_n, S V, S ret, S clip, S vf_coef, S inv_mb) {
    LossHead<S> o;
    policy_loss_head(mu, log_std, a, logp_old, adv_n, clip, inv_mb, o);
    value_loss_head(V, ret, vf_coef, inv_mb, o);
    return o;
}

// ---- extended loss head (so100_learner_minibatch_step_ex): SB3's remaining terms --------------------------------------------------------
// loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss with
//   entropy_loss = -mean(entropy), entropy = sum_i log_std_i + 6 (0.5 + 0.5 ln 2 pi): state-independent, its only gradient is -ent_coef on each log_std_i
//   value_loss = mean((ret - V_pred)^2), V_pred = old_V + clamp(V - old_V, -clip_vf, +clip_vf) when clip_vf > 0, else V
//   approx_kl = mean((ratio - 1) - (logp - logp_old))                  (a diagnostic: no gradient)
template <class S>
struct LossHeadEx : LossHead<S> {
    S approx_kl;                   // this sample's (ratio - 1) - (logp - logp_old)
    S entropy;                     // the Gaussian's entropy (the same for every sample)
    S v_clipped;                   // 1 where |V - old_V| > clip_vf (the clamp is active: no gradient reaches V), else 0; 0 with value clipping off
};

// entropy and the -ent_coef inv_mb it adds to every d/dlog_std ride on the policy half.  With ent_coef = 0 the derivatives are
// policy_loss_head's to the bit (x - 0 = x).
template <class S>
SO100_LHD void policy_loss_head_ex(const S* mu, const S* log_std, const S* a, S logp_old, S adv_n, S clip, S ent_coef, S inv_mb, LossHeadEx<S>& o) {
    S ratio, log_ratio;
    policy_loss_core<S>(mu, log_std, a, logp_old, adv_n, clip, inv_mb, o, ratio, log_ratio);
    o.approx_kl = (ratio - S(1)) - log_ratio;
    S h = S(0);
    for (int i = 0; i < ACT_DIM; i++) h += log_std[i];
    o.entropy = h + S(ACT_DIM)*S(1.4189385332046727);
    const S de = ent_coef*inv_mb;
    for (int i = 0; i < ACT_DIM; i++) o.dlog_std[i] -= de;
}

// torch's clamp passes the gradient on the closed interval [-clip_vf, +clip_vf] and none outside it.  clip_vf <= 0: value_loss_head.
template <class S>
SO100_LHD void value_loss_head_ex(S V, S old_V, S ret, S clip_vf, S vf_coef, S inv_mb, LossHeadEx<S>& o) {
    if (!(clip_vf > S(0))) {
        value_loss_head<S>(V, ret, vf_coef, inv_mb, o);
        o.v_clipped = S(0);
        return;
    }
    const S d = V - old_V;
    const bool outside = d > clip_vf || -d > clip_vf;
    const S v_pred = old_V + (d < -clip_vf ? -clip_vf : d > clip_vf ? clip_vf : d);
    const S e = v_pred - ret;
    o.v_loss = e*e;
    o.dV = outside ? S(0) : S(2)*vf_coef*e*inv_mb;
    o.v_clipped = outside ? S(1) : S(0);
}

template <class S>
SO100_LHD LossHeadEx<S> ppo_loss_head_ex(const S* mu, const S* log_std, const S* a, S logp_old, S adv_n, S V, S old_V, S ret, S clip, S clip_vf,
                                         S ent_coef, S vf_coef, S inv_mb) {
    LossHeadEx<S> o;
    policy_loss_head_ex(mu, log_std, a, logp_old, adv_n, clip, ent_coef, inv_mb, o);
    value_loss_head_ex(V, old_V, ret, clip_vf, vf_coef, inv_mb, o);
    return o;
}

// ---- optimiser ----------------------------------------------------------------------------------------------------------------------------
// clip_grad_norm_: every gradient is multiplied by min(1, max_norm/(norm + 1e-6)), norm = the L2 norm over all parameters
template <class S>
SO100_LHD S clip_coefficient(S grad_norm, S max_grad_norm) {
    const S c = max_grad_norm/(grad_norm + S(1e-6));
    return c < S(1) ? c : S(1);
}

// torch.optim.Adam (no weight decay, no amsgrad) with its scalars as torch forms them, in double on the host, before they meet the
// tensor's type: omb1 = 1 - beta1, omb2 = 1 - beta2 (0.999f is 1.3e-5 away from a (1 - beta2) of 0.001), step_size = lr/(1 - beta1^step),
// bc2_sqrt = sqrt(1 - beta2^step), step 1-based.  g is the reduced, not yet clipped gradient; returns the clipped one (what Adam consumed).
template <class S>
SO100_LHD S clip_adam_update(S g, S clip_coef, S& p, S& m, S& v, S step_size, S omb1, S beta2, S omb2, S eps, S bc2_sqrt) {
    g *= clip_coef;
    m = m + (g - m)*omb1;
    v = v*beta2 + omb2*g*g;
    const S denom = lsqrt(v)/bc2_sqrt + eps;
    p = p - step_size*(m/denom);
    return g;
}

// ---- reward normalisation -----------------------------------------------------------------------------------------------------------------
// SB3's VecNormalize(norm_reward=True) / RunningMeanStd as include/so100_learn.h ("Reward normalisation") specifies it.  S is double in both
// instantiations that ship (the kernels and tests/_rewnormcheck); only reward_scale's result is rounded, to OUT.
constexpr int RN_BLOCK = 64;       // envs per block of the moments: one wave, one workgroup of the scan

// the running discounted return of one env after this step's reward
template <class S>
SO100_LHD S return_step(S R, S gamma, S r) { return R*gamma + r; }

// The block moments' fixed tree over RN_BLOCK slots: slot i += slot i + w for w = 32, 16 .. 1; slot 0 ends as the sum.  The kernel runs
// the same additions across a wave's lanes (lane i takes lane i + w's value); slots past the block's count hold 0.
template <class S>
SO100_LHD S block_tree_sum(S* slot) {
    for (int w = RN_BLOCK/2; w > 0; w >>= 1)
        for (int i = 0; i < w; i++) slot[i] += slot[i + w];
    return slot[0];
}
template <class S>
SO100_LHD S block_mean(S sum, int count) { return sum/S(count); }
template <class S>
SO100_LHD S squared_deviation(S R, S mean) { const S d = R - mean; return d*d; }

// Chan et al.: (na, mean, m2) absorbs (nb, mean_b, m2_b); both counts positive
template <class S>
SO100_LHD void chan_merge(S& na, S& mean, S& m2, S nb, S mean_b, S m2_b) {
    const S tot = na + nb, d = mean_b - mean;
    mean = mean + d*nb/tot;
    m2 = m2 + m2_b + d*d*na*nb/tot;
    na = tot;
}

// RunningMeanStd.update_from_moments: (mean, var, count) absorbs one step's batch moments
template <class S>
SO100_LHD void running_moment_update(S& mean, S& var, S& count, S bm, S bv, S bc) {
    const S d = bm - mean, tot = count + bc;
    const S m_a = var*count, m_b = bv*bc;
    mean = mean + d*bc/tot;
    var = (m_a + m_b + d*d*count*bc/tot)/tot;
    count = tot;
}

template <class S>
SO100_LHD S reward_denominator(S var, S epsilon) { return lsqrt(var + epsilon); }

template <class OUT, class S>
SO100_LHD OUT reward_scale(S r, S denom, S clip) {
    const S x = r/denom;
    return (OUT)(x < -clip ? -clip : x > clip ? clip : x);
}

// ---- observation normalisation ------------------------------------------------------------------------------------------------------------
// SB3's VecNormalize(norm_obs=True) folded into the policy, as include/so100_learn.h ("Observation normalisation") specifies it.  The moments
// and the fold are fp64 (S = double in the kernels and in tests/_obsnormcheck), the load is the learner's fp32.  chan_merge and
// running_moment_update above are shared with the reward half.
constexpr int ON_BLOCK = 256;      // rows per block of the moments: one workgroup
constexpr int ON_GROUP = 64;       // blocks per group of the merge

constexpr long on_blocks(long rows) { return (rows + ON_BLOCK - 1)/ON_BLOCK; }
constexpr long on_groups(long rows) { return (on_blocks(rows) + ON_GROUP - 1)/ON_GROUP; }
constexpr long on_block_count(long rows, long b) { return rows - b*ON_BLOCK < ON_BLOCK ? rows - b*ON_BLOCK : ON_BLOCK; }

// The block moments' fixed tree over ON_BLOCK slots: slot j += slot j + w for w = 128, 64 .. 1; slot 0 ends as the sum.  The kernel runs the
// same additions with thread j owning slot j; slots past the block's count hold 0.
template <class S>
SO100_LHD S obs_block_tree_sum(S* slot) {
    for (int w = ON_BLOCK/2; w > 0; w >>= 1)
        for (int j = 0; j < w; j++) slot[j] += slot[j + w];
    return slot[0];
}

// One group of one dimension: its first block's (n, mean, M2) absorbs the group's other blocks in block order.  part: the blocks' (mean, M2)
// pairs of this dimension, `stride` scalars from block to block; blocks [b0, b1) of a chunk of `rows` rows.
template <class S>
SO100_LHD void obs_group_merge(const S* part, long stride, long rows, long b0, long b1, S& n, S& mean, S& m2) {
    n = S(on_block_count(rows, b0)); mean = part[b0*stride]; m2 = part[b0*stride + 1];
    for (long b = b0 + 1; b < b1; b++) chan_merge<S>(n, mean, m2, S(on_block_count(rows, b)), part[b*stride], part[b*stride + 1]);
}

// One dimension's batch moments from its groups' (n, mean, M2) triples (`stride` scalars from group to group, merged in group order), then the
// running update with the batch as one sample of `rows` rows.  count is advanced too: the caller stores it once for all dimensions.
template <class S>
SO100_LHD void obs_moment_update(const S* grp, long stride, long groups, long rows, S& mean, S& var, S& count) {
    S n = grp[0], bm = grp[1], m2 = grp[2];
    for (long g = 1; g < groups; g++) chan_merge<S>(n, bm, m2, grp[g*stride], grp[g*stride + 1], grp[g*stride + 2]);
    running_moment_update<S>(mean, var, count, bm, m2/S(rows), S(rows));
}

template <class S>
SO100_LHD S obs_inv_std(S var, S epsilon) { return S(1)/lsqrt(var + epsilon); }

// the fold of one first-layer row j: w [od] and b of the plain block -> w_out [od], b_out; the fp64 products are rounded once, at the store
template <class S>
SO100_LHD void obs_fold_row(int od, const float* w, float b, const S* mean, const S* inv_std, float* w_out, float& b_out) {
    S s = S(0);
    for (int i = 0; i < od; i++) {
        const S wf = S(w[i])*inv_std[i];
        s += wf*mean[i];
        w_out[i] = (float)wf;
    }
    b_out = (float)(S(b) - s);
}

// the learner's load of one observation entry: one subtraction, then one multiplication, each rounded (the specification's form: a bitwise test
// rests on it, so the product is kept from contracting with anything)
SO100_LHD float obs_normalized(float x, float mean, float inv_std) {
    const float d = x - mean;
    return d*inv_std;
}

}  // namespace learn
}  // namespace so100

// ---- shuffle ------------------------------------------------------------------------------------------------------------------------------
// The permutation of include/so100_learn.h ("The permutation"): a 6-round balanced Feistel network over 2h bits whose round function is the
// simulator's Philox4x32-10, cycle-walked back into [0, n).  philox4x32 lives in so100_task.hpp, so this section exists where that header came
// first (so100_learn.hip through so100_policy.hpp, tests/_shufflecheck); tests/_learncheck compiles the arithmetic above without it.
#ifdef SO100_HD
namespace so100 {
namespace learn {

constexpr uint32_t SHUFFLE_STREAM = 0x53484633u;       // counter word c3: the simulator's streams use 0 and 0x504F4C
constexpr int SHUFFLE_ROUNDS = 6;
constexpr int64_t SHUFFLE_MAX_N = (int64_t)1 << 30;    // the walk's x stays below 4^15

// the row at position i (0 <= i < n, 1 <= n <= 2^30) of epoch `epoch` under `seed`.  The Feistel map permutes [0, 4^h) and i < n <= 4^h,
// so the walk returns into [0, n) (at the latest at i itself); the domain is smaller than 4n, so it takes fewer than 4 maps on average.
SO100_HD uint32_t shuffle_index(uint32_t i, uint32_t n, uint64_t seed, uint32_t epoch) {
    if (n <= 1u) return 0u;
    int bits = 0;
    for (uint32_t m = n - 1u; m != 0u; m >>= 1) bits++;
    const int h = (bits + 1)/2;
    const uint32_t mask = (1u << h) - 1u, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t x = i;
    do {
        uint32_t L = x >> h, R = x & mask;
        for (int r = 0; r < SHUFFLE_ROUNDS; r++) {
            uint32_t o[4];
            philox4x32(R, (uint32_t)r, epoch, SHUFFLE_STREAM, k0, k1, o);
            const uint32_t t = L ^ (o[0] & mask);
            L = R; R = t;
        }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}

}  // namespace learn
}  // namespace so100
#endif
