// so100_policy.hpp -- fused rollout-side actor-critic forward (SB3 "MlpPolicy" for a Box action space).
//
// This is a CALLER-side helper of the hot path (the rollout collector), not part of the
// simulator: it replaces the ~28 small PyTorch kernels SB3's `policy.forward(obs)` + `clip` + rollout-buffer writes
// launch per vectorised step (main.py:56-64 -> stable_baselines3 OnPolicyAlgorithm.collect_rollouts) with ONE launch.
//   pi tower: obs -> Linear(od,64) tanh -> Linear(64,64) tanh -> Linear(64,6) = mean;  log_std state independent
//   vf tower: obs -> Linear(od,64) tanh -> Linear(64,64) tanh -> Linear(64,1) = value
//   action = mean + exp(log_std) * eps, eps ~ N(0,1) (Philox4x32-10 + Box-Muller, or injected), log_prob, clip to [-1,1]
// Two kernels in so100_rollout.hpp run it: so100_policy_forward_mfma (its own launch) and the policy phase of
// so100_rollout_fused.  The two 64-wide hidden layers run on the matrix cores (exact-fp32 v_mfma_f32_32x32x2_f32), heads /
// sampling on the VALU (the 32-row contact-disabled rollout kernels run the heads on the matrix cores as well: v_mfma_f32_4x4x1_16b_f32,
// the same fmaf chain).  This header holds what the two share: the weight / IO structs, the LDS and rollout-row layouts and the
// tanh (the Philox + Box-Muller noise, policy_noise, is in so100_task.hpp).  The network itself is written out in each kernel, the same operations in the same
// order, and test_persistent_rollout_equals_stepwise holds the two together to 1e-6.  (It was also built as shared functions
// here; each of them, even the once-per-launch weight loading, changed the register allocation or scratch size of some
// instantiation of the rollout kernel, which is tuned to the last 16 B: DESIGN.md 8e.)
#pragma once
#include <hip/hip_runtime.h>
#include "so100_task.hpp"

namespace so100 {

// ---- layouts shared by the kernels ----------------------------------------------------------------------------
constexpr int POLICY_LD = 65;                          // LDS row stride of the [env][unit] activation images: conflict-free A read, D write and head read
constexpr int policy_odp(int od) { return (od + 3) & ~3; }     // K of layer 1: obs_dim padded with zero weights to whole k steps
// hd[]: the head weights in LDS, mu_w[6][64] | v_w[64] | mu_b[6] | log_std[6] | v_b
constexpr int HD_MU_W = 0, HD_V_W = 6*64, HD_MU_B = 7*64, HD_LOG_STD = HD_MU_B + 6, HD_V_B = HD_LOG_STD + 6, HD_WORDS = 7*64 + 16;
// hm[]: mu_w once more for the matrix-core mean head (so100_rollout.hpp: head_mfma), rows HM_LD floats apart.  One ds_read_b128 of that head
// touches the four rows (lane & 3) + 4*(lane >> 5) within a 16-lane group: 64 floats apart they share four banks, 68 apart they take sixteen.
constexpr int HM_LD = 68, HM_STD = 6*HM_LD, HM_WORDS = HM_STD + 8;
// hm[HM_STD + a] = exp(log_std[a]): the policy does not change inside a launch, so the rollout kernels that keep hm take the exponential once per
// launch, where hm is filled, with the builtin the sampling used per step (same bits).  It stands here and not in hd: hm exists in those kernels
// only, so every other kernel keeps the LDS image it had.  (HM_STD is a multiple of four words: the six values are read as b128 + b64.)
// rollout-buffer row of one env and step: obs[OD] | raw action[6] | reward | done code | value | log-prob (columns past the observation)
constexpr int ROW_ACT = 0, ROW_REWARD = 6, ROW_DONE = 7, ROW_VALUE = 8, ROW_LOGP = 9, ROW_EXTRA = 10;
__device__ __forceinline__ float done_code(bool done, bool trunc_only) { return done ? (trunc_only ? 2.0f : 1.0f) : 0.0f; }     // 2 = TimeLimit truncation only

struct PolicyWeights {                 // device pointers, PyTorch nn.Linear layout weight[out][in], row-major
    const float *pi_w0, *pi_b0, *pi_w1, *pi_b1, *mu_w, *mu_b, *log_std;
    const float *vf_w0, *vf_b0, *vf_w1, *vf_b1, *v_w, *v_b;
};
struct PolicyIO {
    const float* obs;                  // [N][OD]
    const float* noise;                // [N][6] standard normals, nullable (then Philox)
    float* act_env;                    // [N][6] clipped to [-1,1]  -> so100_step
    float* act_raw;                    // [N][6] unclipped (what SB3 stores), nullable
    float* value;                      // [N], nullable
    float* logp;                       // [N], nullable
    float* rollout_row;                // [N][OD+10]: obs | raw action | reward | done | value | logp ; nullable
};

__device__ __forceinline__ float fast_tanh(float x) {
    // tanh(x) = 1 - 2/(exp(2x)+1); exp via v_exp_f32 (2^x), rcp with one Newton step: abs error < 2e-7.
    // exp(2x) overflows to +inf for x > ~44 and rcp(inf) = 0 would make the Newton step of trcp 0*inf = NaN, so the
    // exponential is capped (1e30: 1 - 2/(1e30+1) rounds to exactly 1.0f): a saturated unit returns +-1, never NaN.
    const float e = __builtin_fminf(__builtin_amdgcn_exp2f(x * 2.885390081777927f), 1.0e30f);          // exp(2x)
    return 1.0f - 2.0f*trcp(e + 1.0f);
}

// The policy noise (Philox + Box-Muller) both kernels draw is policy_noise() in so100_task.hpp, beside the env's own draw8: host-compilable, so
// tests/_hostcheck holds its fp32 transform to the fp64 reference sampler.

}  // namespace so100
