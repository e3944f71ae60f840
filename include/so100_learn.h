/* so100_learn.h -- C ABI of the on-device PPO learner of libso100sim.so: advantages (GAE with the TimeLimit bootstrap), one
 * clipped-surrogate gradient step with gradient-norm clipping and Adam, and a whole update (epochs of shuffled minibatch steps) in one call, for the fixed SB3 "MlpPolicy" network the rollout kernels
 * run (two 2 x 64 tanh towers, state-independent log_std; so100_policy_weights in so100_sim.h).  It replaces, for that network,
 * stable_baselines3 RolloutBuffer.compute_returns_and_advantage and the body of PPO.train's minibatch loop (here: ppo.py PPO._gae /
 * PPO._step).  Additive to so100_sim.h: SO100_ABI_VERSION and every declaration there are unchanged; error codes and
 * so100_last_error() are shared.
 *
 * Conventions (those of so100_sim.h)
 *   - extern "C", plain pointers and sizes; `*_dev` pointers are DEVICE pointers owned by the caller: the parameters, the Adam
 *     moments and every rollout buffer.  The handle owns scratch only (per-workgroup partial gradients, bounded by max_minibatch).
 *   - 0 on success, a negative SO100_E_* code otherwise, message in so100_last_error().
 *   - all work is enqueued on the caller's `hip_stream`; after so100_learner_create nothing allocates, frees or synchronises.
 *   - there is NO CPU fallback.
 *   - deterministic: gradients are reduced in a fixed order (per-workgroup partials, then an ordered sum); no floating-point
 *     atomics.  The same inputs give bit-identical parameters.
 *
 * The flat parameter block: so100_learner_num_params(obs_dim) floats holding the 13 tensors of so100_policy_weights in that struct's
 * order (pi_w0, pi_b0, pi_w1, pi_b1, mu_w, mu_b, log_std, vf_w0, vf_b0, vf_w1, vf_b1, v_w, v_b), each in PyTorch nn.Linear layout
 * weight[out][in] row-major; so100_learner_param_offset() places them.  A so100_policy_weights may point straight into the block.
 * adam_m / adam_v / grads have the same layout.
 */
#ifndef SO100_LEARN_H
#define SO100_LEARN_H
#include <stdint.h>
#include "so100_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct so100_learner so100_learner;

typedef struct {
    int32_t obs_dim;              /* 15 or 8 (so100_obs_dim)                                                    */
    int32_t device;               /* HIP device ordinal                                                         */
    int32_t max_minibatch;        /* largest mb of so100_learner_minibatch_step (>= 1); bounds the scratch       */
    float   gamma;                /* 0.99                                                                        */
    float   gae_lambda;           /* 0.95                                                                        */
    float   clip_range;           /* 0.2                                                                         */
    float   vf_coef;              /* 0.5                                                                         */
    float   max_grad_norm;        /* 0.5                                                                         */
    double  lr;                   /* 3e-4.  Adam's scalars are doubles: torch forms 1 - beta, lr/(1 - beta1^t) in double      */
    double  beta1, beta2;         /* 0.9, 0.999   (as a float, 1 - 0.999f is 1.3e-5 away from 0.001)                          */
    double  adam_eps;             /* 1e-5 (added to sqrt(v_hat), as torch.optim.Adam does)                                    */
} so100_learner_config;

/* Advantages and returns of one rollout chunk: rollout.bootstrap_truncated followed by PPO._gae.
 *   r' = r + gamma V(terminal_obs) where the done code is 2 and terminal_obs_chunk_dev is non-null, else r
 *   nonterm = (code == 0);  next_v = V(last_obs) at t = T-1, else value[t+1]
 *   delta = r' + gamma next_v nonterm - value[t];  g = delta + gamma lambda nonterm g;  adv = g;  ret = adv + value
 * The chunk is read only (reward, done-code and value columns) and left unmodified.  The value tower runs on the N last observations
 * and on the code-2 entries alone.  N is any positive number (it need not be a sim handle's N). */
typedef struct {
    const float* rollout_dev;            /* [T][N][obs_dim+10], as so100_rollout wrote it                                  */
    const float* terminal_obs_chunk_dev; /* [T][N][obs_dim], read where the done code is 2; nullable (then no bootstrap)   */
    const float* last_obs_dev;           /* [N][obs_dim] observation after the chunk's last step                           */
    const float* params_dev;             /* the parameter block whose value tower produced the chunk's values              */
    float*       adv_dev;                /* [T][N] out                                                                     */
    float*       ret_dev;                /* [T][N] out                                                                     */
    float*       adv_stats_dev;          /* [2] out: mean and unbiased standard deviation of adv over all T*N entries      */
} so100_advantages_io;

/* One PPO gradient step on the samples idx_dev names (PPO._step + clip_grad_norm_ + Adam.step):
 *   A = (adv - mean)/(std + 1e-8);  logp = sum(-((a - mu)/sigma)^2/2 - log sigma - log(2 pi)/2);  ratio = exp(logp - logp_old)
 *   L = -mean(min(ratio A, clamp(ratio, 1-c, 1+c) A)) + vf_coef mean((ret - V)^2)          (no entropy term, no value clipping:
 *                                                                                             so100_learner_minibatch_step_ex has them)
 *   g *= min(1, max_grad_norm/(|g|_2 + 1e-6)) over all 13 tensors;  bias-corrected Adam.
 * Observation, raw action and old log-prob are read in place from the packed chunk through idx. */
typedef struct {
    const float*   rollout_dev;    /* [num_samples][obs_dim+10] the packed chunk, rows t*N + n                                  */
    int64_t        num_samples;    /* T*N: an index outside [0, num_samples) contributes nothing                                */
    const int64_t* idx_dev;        /* [mb] int64 flat row indices (what torch.randperm yields), any order; NULL = 0..mb-1       */
    int32_t        mb;             /* 1 <= mb <= max_minibatch                                                                  */
    int32_t        adam_step;      /* 1-based number of this Adam step                                                          */
    const float*   adv_dev;        /* [num_samples]  from so100_learner_advantages                                              */
    const float*   ret_dev;        /* [num_samples]                                                                             */
    const float*   adv_stats_dev;  /* [2]                                                                                       */
    float*         params_dev;     /* [P] updated in place                                                                      */
    float*         adam_m_dev;     /* [P] updated in place                                                                      */
    float*         adam_v_dev;     /* [P] updated in place                                                                      */
    float*         stats_dev;      /* [4] out: policy loss, value loss, clip fraction (|ratio - 1| > c), pre-clip gradient norm */
    float*         grads_dev;      /* [P] out, nullable: the reduced gradient times the clip coefficient (what Adam consumed)    */
} so100_minibatch_io;

/* The terms of SB3's PPO loss that so100_learner_minibatch_step leaves out, for so100_learner_minibatch_step_ex.  Per minibatch:
 *   A            normalize_advantage 0: (adv - mean_chunk)/(std_chunk + 1e-8) from adv_stats_dev, as above
 *                normalize_advantage 1: (adv - mean)/(std + 1e-8), mean and unbiased std over this minibatch's valid rows (a launch of its
 *                own into scratch the handle owns); with at most one valid row adv is used as it is
 *   V_pred       V, or old_V + clamp(V - old_V, -clip_range_vf, +clip_range_vf) with old_V the row's value column; the gradient passes on
 *                the closed interval and not outside it (torch.clamp); value_loss = mean((ret - V_pred)^2)
 *   entropy_loss -mean(entropy), entropy = sum_i log_std_i + 6 (0.5 + 0.5 ln 2 pi); its only gradient is -ent_coef on each log_std_i
 *   L            policy_loss + ent_coef entropy_loss + vf_coef value_loss
 *   approx_kl    mean((ratio - 1) - (logp - logp_old)), with the parameters before this step
 * Means are sums over the valid rows divided by mb, as in so100_learner_minibatch_step.
 * KL stop.  With target_kl > 0 the caller owns an update-state pair int32 {stopped, steps_applied} on the device and zeroes it at the start
 * of an update.  Every kernel of the step reads `stopped` first and does nothing when it is set.  If approx_kl > 1.5 target_kl the step is
 * not applied (parameters, moments and grads_dev untouched), `stopped` is set and diag holds the stopping minibatch's values; otherwise
 * the step is applied and steps_applied is incremented.  No step after the stop is applied, so the applied steps carry the contiguous
 * adam_step numbers 1..steps_applied the host passed, and nothing synchronises in the middle of an update. */
typedef struct {
    float   ent_coef;             /* >= 0; 0: no entropy bonus                                                   */
    float   clip_range_vf;        /* <= 0: no value clipping                                                     */
    int32_t normalize_advantage;  /* 0 batch (adv_stats_dev), 1 minibatch                                        */
    float   target_kl;            /* <= 0: no stop                                                               */
    double  lr;                   /* this step's learning rate (a schedule, evaluated by the caller); < 0: the handle's */
} so100_ppo_terms;

/* The permutation of one epoch: a pure function of (seed, epoch, n), the same on every device and in every version of this library.
 * A 6-round balanced Feistel network over 2h bits whose round function is Philox4x32-10 (the simulator's generator: multipliers 0xD2511F53 /
 * 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds), cycle-walked back into [0, n):
 *   perm(i), 0 <= i < n:
 *     n == 1: 0
 *     bits = bit length of n-1 (>= 1);  h = (bits + 1) / 2;  mask = 2^h - 1                  (the domain is 4^h, n <= 4^h < 4n)
 *     x = i
 *     do { L = x >> h;  R = x & mask
 *          for r = 0 .. 5:  f = philox4x32(counter (R, r, epoch, 0x53484633), key (seed & 0xffffffff, seed >> 32))[0] & mask
 *                           (L, R) = (R, L ^ f)
 *          x = (L << h) | R
 *     } while (x >= n)
 *     perm(i) = x
 * perm(i) is the row at position i of the epoch; minibatch k of size mb is the positions [k mb, min(n, (k+1) mb)).  The Feistel map is a
 * bijection of [0, 4^h) and i < n, so the walk ends and perm is a bijection of [0, n).  The counter word 0x53484633 keeps the stream apart
 * from the simulator's (0 and 0x504F4C) under equal seeds. */

/* so100_learner_update: one whole PPO update (SB3's PPO.train on one rollout chunk) enqueued by one call, in this order:
 *   1. so100_learner_advantages on the chunk                         -> adv_dev, ret_dev, adv_stats_dev
 *   2. so100_learner_explained_variance                              -> out_dev[8]
 *   3. update_state_dev (when given) is zeroed
 *   4. for e in 0 .. epochs-1: perm_dev = the permutation of (shuffle_seed, shuffle_epoch0 + e, T*N), then ceil(T*N/mb) minibatch steps, step k on
 *      idx = perm_dev + k mb with min(mb, T*N - k mb) rows; the steps carry adam_step = adam_step0 + 1, adam_step0 + 2, ...
 * terms null: so100_learner_minibatch_step, its four statistics in out_dev[0:4]; given: so100_learner_minibatch_step_ex, its eight diagnostics in
 * out_dev[0:8], the KL stop as documented there (the steps after a stop do nothing; steps_applied in update_state_dev says how many were applied,
 * and the caller's next adam_step0 is this one plus that).  Before the last enqueued step the six log_std it is about to read are copied to
 * out_dev[9:15].  Every buffer is the caller's; adv / ret / adv_stats / perm are outputs too (perm_dev ends holding the last epoch's
 * permutation).  Nothing allocates, frees or synchronises, no stream is created; a rejected call enqueues nothing. */
#define SO100_UPDATE_OUT 15
typedef struct {
    const float*           rollout_dev;            /* [T][N][obs_dim+10], as so100_rollout wrote it                                  */
    const float*           terminal_obs_chunk_dev; /* [T][N][obs_dim]; nullable (then no TimeLimit bootstrap)                        */
    const float*           last_obs_dev;           /* [N][obs_dim]                                                                   */
    int32_t                T, N;                   /* >= 1; T*N <= 2^24 (so100_learner_explained_variance)                           */
    float*                 params_dev;             /* [P] updated in place                                                           */
    float*                 adam_m_dev;             /* [P] updated in place                                                           */
    float*                 adam_v_dev;             /* [P] updated in place                                                           */
    float*                 adv_dev;                /* [T][N] out                                                                     */
    float*                 ret_dev;                /* [T][N] out                                                                     */
    float*                 adv_stats_dev;          /* [2] out                                                                        */
    int64_t*               perm_dev;               /* [T*N] out: the last epoch's permutation                                        */
    int32_t                epochs;                 /* >= 1                                                                           */
    int32_t                mb;                     /* 1 <= mb <= max_minibatch; the last minibatch of an epoch holds the remainder   */
    int32_t                adam_step0;             /* >= 0: Adam steps applied before this update                                    */
    uint32_t               shuffle_epoch0;         /* epoch e of this update shuffles with shuffle_epoch0 + e (mod 2^32)             */
    uint64_t               shuffle_seed;
    const so100_ppo_terms* terms;                  /* nullable: the plain step                                                       */
    int32_t*               update_state_dev;       /* [2] {stopped, steps_applied}; required with terms->target_kl > 0, else nullable */
    float*                 out_dev;                /* [SO100_UPDATE_OUT]: [0:8] statistics / diagnostics, [8] explained variance, [9:15] log_std */
} so100_update_io;

/* Reward normalisation: the reward half of SB3's VecNormalize(norm_reward=True) with its RunningMeanStd, on the device and before the
 * advantages (the TimeLimit bootstrap gamma V(terminal_obs) is added to the NORMALISED reward by the advantage pass, so V lives in the
 * normalised scale).  Off unless asked for: every entry point above is untouched by it.
 * State (state_dev, fp64, the caller's, carried from chunk to chunk): mean, var, count -- the running moments of the envs' discounted
 * returns, initially 0, 1, 1e-4 -- then one running discounted return R[n] per env, initially 0 (so100_learner_reward_norm_init).
 * For t = 0 .. T-1, with r[t][n] the chunk's reward column and c[t][n] its done code, everything in fp64:
 *   R[n]   = R[n] gamma + r[t][n]                                    (gamma: the handle's, widened from float)
 *   bm     = mean_n R[n];  bv = population variance_n R[n];  bc = N
 *   d      = bm - mean;  tot = count + bc
 *   mean'  = mean + d bc/tot
 *   var'   = (var count + bv bc + d d count bc/tot)/tot
 *   count' = tot
 *   out[t][n] = (float) clamp(r[t][n]/sqrt(var' + epsilon), -clip_reward, +clip_reward)       (SB3: epsilon 1e-8, clip_reward 10)
 *   R[n]   = 0 where c[t][n] != 0                                    (after the update; terminated or truncated)
 * The variance used at step t includes step t.  Two chunks processed one after the other equal one chunk of 2T.  The chunk is read only.
 * Order of the sums (the same bits every run, no floating-point atomics): the envs are cut into blocks of 64 in index order; a block's
 * mean is its sum by a fixed binary tree (slot i += slot i + w, w = 32, 16 .. 1) over its count, its M2 the same tree over the squared
 * deviations from that mean; the blocks' (n, mean, M2) are merged in block order by Chan et al.'s update; the steps follow in t order.
 * Three launches: the R recurrence and the block moments for every t (one workgroup per block), the merge with the T running-moment
 * updates, the elementwise scale.  workspace_dev holds the block moments and the T denominators between them; it is the caller's, at least
 * so100_learner_reward_norm_workspace(T, N) bytes, 8-byte aligned. */
typedef struct {
    const float* rollout_dev;      /* [T][N][obs_dim+10]: the reward and done-code columns are read                              */
    double*      state_dev;        /* [3 + N] in/out: mean, var, count, then R[N]                                                */
    float*       reward_dev;       /* [T][N] out: the normalised rewards                                                         */
    void*        workspace_dev;    /* scratch of this call                                                                       */
    int64_t      workspace_bytes;  /* >= so100_learner_reward_norm_workspace(T, N)                                               */
    double       clip_reward;      /* > 0; SB3: 10                                                                               */
    double       epsilon;          /* >= 0; SB3: 1e-8                                                                            */
} so100_reward_norm_io;

/* Observation normalisation: the observation half of SB3's VecNormalize(norm_obs=True) with its RunningMeanStd, folded into the policy.
 * Off unless asked for: with no normaliser set every entry point above computes what it always did, to the bit.
 * State (state_dev, fp64 [2 obs_dim + 1], the caller's, carried from chunk to chunk): mean[obs_dim], var[obs_dim], count -- initially 0, 1,
 * 1e-4 (so100_learner_obs_norm_init).
 * Moment update of one chunk (so100_learner_obs_norm_update).  The batch is the T*N observation columns of the chunk's rows (row r = t N + n,
 * observation i of row r at rollout_dev[r (obs_dim + 10) + i]): what the policy was fed, reset observations included.  Per dimension i, in fp64:
 *   bm = mean over the batch;  bv = population variance over the batch;  bc = T*N
 *   d = bm - mean;  tot = count + bc
 *   mean'  = mean + d bc/tot
 *   var'   = (var count + bv bc + d d count bc/tot)/tot
 *   count' = tot
 * Order of the sums -- a function of (T, N) alone, never of the grid; no floating-point atomics; the same inputs give the same bits:
 *   1. the rows are cut into blocks of 256 in row order (the last block holds the remainder).  A block's mean is its sum by a fixed binary
 *      tree over 256 slots (slot j holds the block's row j widened to fp64, 0 past the block's count; slot j += slot j + w for w = 128, 64 .. 1)
 *      divided by its count; its M2 is the same tree over the squared deviations (x - mean)(x - mean) from that mean.
 *   2. the blocks are cut into groups of 64 in block order.  A group's (n, mean, M2) starts as its first block's and absorbs its other blocks in
 *      block order by Chan et al.'s update:  tot = na + nb;  d = mean_b - mean;  mean += d nb/tot;  M2 += M2_b + d d na nb/tot;  na = tot.
 *   3. the groups are merged in group order by the same update, starting from the first group's; bm = mean, bv = M2/(T*N).
 * Two chunks in a row are not bit-equal to one chunk of 2T (the statistics of a chunk are merged as ONE batch), but equal it within rounding.
 * Two launches: the block moments (one workgroup per block), the merge with the update.  workspace_dev holds the blocks' and the groups'
 * moments between them; the caller's, at least so100_learner_obs_norm_workspace(T, N) bytes, 8-byte aligned.
 * Fold (so100_learner_obs_norm_fold).  For a frozen (mean, inv_std) the first layer of each tower on the normalised input equals a first layer
 * with folded weights on the raw input.  In fp64, rounded once to float at the store:
 *   inv_std[i] = 1/sqrt(var[i] + epsilon)                                             (SB3: epsilon 1e-8)
 *   W0'[j][i]  = W0[j][i] inv_std[i]
 *   b0'[j]     = b0[j] - sum_i W0'[j][i] mean[i]        (the unrounded W0'; the sum starts at 0 and runs in index order)
 * for (W0, b0) = (pi_w0, pi_b0) and (vf_w0, vf_b0).  folded_params_dev [P] gets the folded four tensors and copies of the other nine: a
 * so100_policy_weights may point into it, as into the plain block.  norm_dev, float [2 obs_dim], gets (float) mean[i], then (float) inv_std[i].
 * The rollout kernels, so100_policy_forward and an exported policy then run on RAW observations with the folded block and compute the policy of
 * the normalised ones; the rollout rows keep the raw observations, which the moment update needs.
 * Learner (so100_learner_set_obs_norm).  With a normaliser set, every observation the learner reads -- the chunk's rows, the terminal
 * observations, the last observations, in so100_learner_advantages(_r), both minibatch steps and both updates -- enters the towers as
 *   x[i] = (obs[i] - norm[i]) * norm[obs_dim + i]
 * in fp32: one subtraction, then one multiplication, each rounded (not a fused multiply-add).  params_dev is the PLAIN block there.
 * Deviations from SB3: the statistics are frozen while a chunk is collected and updated once per chunk (SB3 updates them every step);
 * clip_obs is not applied (a clamp cannot be folded, and the sampling policy and the trained policy must be the same function); the observation
 * after the final chunk is never counted.  A dimension that never varies gets inv_std 1/sqrt(epsilon) = 1e4: its folded weights grow by that factor.
 * Known answer: obs_dim 2, a fresh state, one chunk of two rows with the observations (1, 10) and (3, 14):
 *   mean' = (1.9999000049997500, 11.999400029998500)   var' = (1.0001999800014999, 4.0070492875536214)   count' = 2.0001
 *   inv_std = (0.99990001999525112, 0.49956000038410525)                             (epsilon 1e-8)
 *   W0 = [[0.5, -0.25]], b0 = [0.125]  ->  W0' = [[0.49995000999762556, -0.12489000009602631]], b0' = [0.62375504340489438] */
typedef struct {
    const float* rollout_dev;      /* [T][N][obs_dim+10]: the observation columns are read                                       */
    double*      state_dev;        /* [2 obs_dim + 1] in/out: mean, var, count                                                   */
    void*        workspace_dev;    /* scratch of this call                                                                       */
    int64_t      workspace_bytes;  /* >= so100_learner_obs_norm_workspace(T, N)                                                  */
} so100_obs_norm_io;

int  so100_learner_num_params(int32_t obs_dim);                          /* 10829 (obs_dim 15), 9933 (8); < 0 otherwise */
int  so100_learner_param_offset(int32_t obs_dim, const char* name);      /* name: a member of so100_policy_weights; < 0 if unknown */
int  so100_learner_param_size(int32_t obs_dim, const char* name);        /* elements of that tensor                      */
int  so100_learner_create(const so100_learner_config* cfg, so100_learner** out);
void so100_learner_destroy(so100_learner* learner);
int  so100_learner_advantages(so100_learner* learner, const so100_advantages_io* io, int32_t T, int32_t N, void* hip_stream);
int  so100_learner_minibatch_step(so100_learner* learner, const so100_minibatch_io* io, void* hip_stream);
/* so100_learner_minibatch_step with the terms above (one more launch when normalize_advantage is 1).  io->stats_dev is not used.
 * diag_dev [8] out: policy loss, value loss, clip fraction, pre-clip gradient norm (these four as stats_dev), approx_kl, entropy_loss,
 * total loss, value-clip fraction (|V - old_V| > clip_range_vf).  update_state_dev [2]: see above; nullable when target_kl is off (when
 * given it is honoured and counted all the same).  With every term off (ent_coef 0, clip_range_vf <= 0, normalize_advantage 0,
 * target_kl <= 0, lr < 0) parameters, moments, grads and the first four diagnostics equal so100_learner_minibatch_step's to the bit. */
int  so100_learner_minibatch_step_ex(so100_learner* learner, const so100_minibatch_io* io, const so100_ppo_terms* terms, float* diag_dev,
                                     int32_t* update_state_dev, void* hip_stream);
/* out_dev [1] = 1 - var(ret - old_V)/var(ret) over the chunk's num_samples rows (population variances; old_V is the value column of
 * rollout_dev, row stride obs_dim+10); NaN when var(ret) == 0, i.e. when every ret equals the first.  num_samples <= 2^24.
 * SB3's explained_variance. */
int  so100_learner_explained_variance(so100_learner* learner, const float* rollout_dev, const float* ret_dev, int64_t num_samples, float* out_dev,
                                      void* hip_stream);

/* perm_dev [n] int64 = the permutation of (seed, epoch, n) specified above, 1 <= n <= 2^30.  One launch. */
int  so100_learner_shuffle(so100_learner* learner, uint64_t seed, uint32_t epoch, int64_t n, int64_t* perm_dev, void* hip_stream);
int  so100_learner_update(so100_learner* learner, const so100_update_io* io, void* hip_stream);

/* bytes of so100_reward_norm_io.workspace_dev for a chunk of T steps x N envs; < 0 when T or N is not positive.  Needs no handle. */
int64_t so100_learner_reward_norm_workspace(int32_t T, int32_t N);
/* state_dev [3 + N] = 0, 1, 1e-4 and N zero returns.  One launch. */
int  so100_learner_reward_norm_init(so100_learner* learner, double* state_dev, int32_t N, void* hip_stream);
/* the normalisation specified above on one chunk: reward_dev [T][N] out, state_dev advanced by T steps.  Three launches. */
int  so100_learner_normalize_rewards(so100_learner* learner, const so100_reward_norm_io* io, int32_t T, int32_t N, void* hip_stream);
/* so100_learner_advantages reading the step's reward from reward_dev [T][N] (step stride N) instead of the chunk's reward column; the
 * TimeLimit bootstrap is added to it as there.  reward_dev null: exactly so100_learner_advantages. */
int  so100_learner_advantages_r(so100_learner* learner, const so100_advantages_io* io, const float* reward_dev, int32_t T, int32_t N, void* hip_stream);
/* so100_learner_update with so100_learner_normalize_rewards(norm_io, io->T, io->N) enqueued first and the advantages reading
 * norm_io->reward_dev: still one call, nothing synchronises, and a rejected call enqueues nothing.  norm_io null: so100_learner_update. */
int  so100_learner_update_r(so100_learner* learner, const so100_update_io* io, const so100_reward_norm_io* norm_io, void* hip_stream);

/* Observation normalisation (specified above).  obs_dim is the handle's throughout. */
/* state_dev [2 obs_dim + 1] = obs_dim zeros, obs_dim ones, 1e-4.  One launch. */
int  so100_learner_obs_norm_init(so100_learner* learner, double* state_dev, void* hip_stream);
/* bytes of so100_obs_norm_io.workspace_dev for a chunk of T steps x N envs (sized for obs_dim 15); < 0 when T or N is not positive or
 * T*N > 2^24.  Needs no handle. */
int64_t so100_learner_obs_norm_workspace(int32_t T, int32_t N);
/* the moment update of one chunk: state_dev absorbs the T*N observation rows.  The chunk is read only.  Two launches.  T*N <= 2^24. */
int  so100_learner_obs_norm_update(so100_learner* learner, const so100_obs_norm_io* io, int32_t T, int32_t N, void* hip_stream);
/* the fold: folded_params_dev [P] and norm_dev [2 obs_dim] from state_dev (read only), params_dev [P] (read only) and epsilon >= 0.
 * folded_params_dev must not alias params_dev.  One launch. */
int  so100_learner_obs_norm_fold(so100_learner* learner, const double* state_dev, double epsilon, const float* params_dev, float* folded_params_dev,
                                 float* norm_dev, void* hip_stream);
/* norm_dev: float [2 obs_dim] (mean, inv_std), the caller's; only the pointer is kept, its contents are read when the kernels run (a fold
 * enqueued on the same stream between two updates is seen by the second).  NULL: off, the state after so100_learner_create.  Enqueues nothing. */
int  so100_learner_set_obs_norm(so100_learner* learner, const float* norm_dev);

#ifdef __cplusplus
}
#endif
#endif /* SO100_LEARN_H */
