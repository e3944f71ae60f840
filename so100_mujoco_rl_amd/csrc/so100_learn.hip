// so100_learn.hip -- the on-device PPO learner behind include/so100_learn.h: advantages (three launches), one minibatch gradient
// step (three launches: gradient, reduction, Adam) and, on top of those, a whole update with its shuffle (so100_learner_update), for the
// fixed 2 x 64 tanh towers of so100_policy.hpp.  The step has two loss heads, chosen at
// compile time (EX): the plain one of so100_learner_minibatch_step and the extended one of so100_learner_minibatch_step_ex with SB3's remaining
// loss terms and the KL stop (under per-minibatch normalisation one more launch, for the minibatch's advantage statistics).  Everything around the
// head -- checks, arguments, launches, kernels -- is written once.  The per-sample and per-parameter arithmetic is in
// so100_learn.hpp (host-compilable templates, held to an fp64 reference by tests/_learncheck); this file holds the data movement.
//
// Gradient kernel (so100_learn_grad): a bounded persistent grid of 256-thread workgroups; each owns tiles of 64 samples gathered
// through idx.  One tower at a time (the towers meet only in the sum of the loss).  In the sample-major phases lane = sample and wave
// q owns hidden units 16q..16q+15: the weights are wave-uniform, read straight from the parameter block through the scalar cache,
// the activations of a sample stay in its lane's registers or go through LDS images [sample][unit] with a row stride of 68 words
// (16-byte rows: every image access is a ds_read/write_b128; lanes 0..15 of a b128 group then cover all 64 banks).  The weight
// gradients dW = dZ^T . X need the reduction over samples, so that phase is unit-major: every thread owns a 4 x 4 block of dW1, four
// entries of dW0 and of the head, accumulates them in REGISTERS over all samples of all its tiles (two b128 LDS reads per 16 FMAs)
// and writes them once, as this workgroup's partial.  Plain FMA throughout: fp32-input MFMA runs at the VALU's rate on gfx950, and the
// unit-major products have the samples on the reduced axis, which the MFMA operand layout would want transposed once more.
// Reduction (so100_learn_reduce): one thread per parameter sums the partials in workgroup order and leaves each block's sum of
// squares; so100_learn_adam sums those in block order (every thread the same sum), decides the clip (EX: and the KL stop) and applies Adam.
// No floating-point atomics anywhere; every sum has a fixed order => bit-identical results for identical inputs.
// Reward normalisation (so100_learner_normalize_rewards, SB3's VecNormalize reward half): three launches in fp64 ahead of the advantages, which
// then read the normalised rewards from a dense array instead of the chunk's column; see "reward normalisation" below.
// Observation normalisation (SB3's VecNormalize observation half, folded into the policy): two fp64 launches merge a chunk's observation rows into
// the running moments, one folds them into a second parameter block for the collector; with a normaliser set (so100_learner_set_obs_norm) the
// gradient step launches so100_learn_grad_norm and the advantages the NORM value kernel, which read every observation as (x - mean)*inv_std; see
// "observation normalisation".
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <new>
#include <type_traits>
#include "../../include/so100_learn.h"
#include "so100_policy.hpp"
#include "so100_learn.hpp"
#include "so100_host.hpp"

namespace so100 {

namespace learn {

constexpr int LT = 64;                 // samples per tile
constexpr int LLD = 68;                // row stride (words) of the [sample][unit] LDS images
constexpr int XLD = 17, DOLD = 13, HPLD = 7;      // odd strides of the small images (scalar accesses, lane = sample)
constexpr int GRID_MAX = 256;          // workgroups of the gradient kernel = partials to reduce (one per CU of an MI355X)
constexpr int NSTAT = 3;               // sums riding behind a partial's P gradients: policy loss, value loss, clipped count
constexpr int NSTAT_EX = 6;            // the extended step's partials: the three above in their places, then approx_kl, value-clipped count, entropy
constexpr int ADV_THREADS = 1024;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float a, float b, float c, float d) { *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d); }

struct GradArgs {
    const float* chunk; long num_samples; const int64_t* idx; int mb;
    const float* adv; const float* ret; const float* adv_stats; const float* params; float* partial;
    float clip, vf_coef;
};

// the extended head's arguments behind the plain ones, so that tower_pass reads those under the same names
struct GradArgsEx : GradArgs {
    float ent_coef, clip_vf;           // clip_vf <= 0: no value clipping
    const int32_t* state;              // the caller's {stopped, steps_applied}, nullable
};
template <bool EX> using GradArgsOf = std::conditional_t<EX, GradArgsEx, GradArgs>;


template <bool EX> struct HeadOf { using type = LossHead<float>; };
template <> struct HeadOf<true> { using type = LossHeadEx<float>; };

struct GradSmem {
    alignas(16) float H1[LT*LLD], H2[LT*LLD], D2[LT*LLD], D1[LT*LLD];
    float X[LT*XLD], DO[LT*DOLD], HP[4*LT*HPLD];
};

// one tower's forward and backward pass over this workgroup's tiles; writes the tower's slice of the workgroup's partial
// EX selects the extended loss head (entropy bonus, value clipping, approx_kl) and its NSTAT_EX sums
// NORM: the observations enter as (x - mean)*inv_std (so100_learner_set_obs_norm).  The normaliser's 2 OD floats are wave-uniform and are read
// through a __restrict__ PARAMETER, the kernel's own (so100_learn_grad_norm): that keeps them on the scalar path in the second tower too,
// behind the first tower's stores to the partial.  (Read through a member of the argument struct they became per-lane vector loads there;
// read once into registers at the kernel's entry they stayed scalar but lived in spilled SGPRs, which cost more than the vector loads did.)
// Without NORM the body is the one it always was.
template <int OD, int TW, bool EX, bool NORM, class Args>
__device__ __forceinline__ void tower_pass(const Args& A, GradSmem& S, [[maybe_unused]] const float* __restrict__ nrm) {
    constexpr int ROW = OD + ROW_EXTRA, NH = TW ? 1 : ACT_DIM, P = num_params(OD), NS = EX ? NSTAT_EX : NSTAT;
    constexpr int oW0 = tensor_offset(TW ? T_vf_w0 : T_pi_w0, OD), oB0 = tensor_offset(TW ? T_vf_b0 : T_pi_b0, OD);
    constexpr int oW1 = tensor_offset(TW ? T_vf_w1 : T_pi_w1, OD), oB1 = tensor_offset(TW ? T_vf_b1 : T_pi_b1, OD);
    constexpr int oWH = tensor_offset(TW ? T_v_w : T_mu_w, OD), oBH = tensor_offset(TW ? T_v_b : T_mu_b, OD), oLS = tensor_offset(T_log_std, OD);
    const float* __restrict__ prm = A.params;
    const float* __restrict__ W0 = prm + oW0; const float* __restrict__ B0 = prm + oB0;
    const float* __restrict__ W1 = prm + oW1; const float* __restrict__ B1 = prm + oB1;
    const float* __restrict__ WH = prm + oWH; const float* __restrict__ BH = prm + oBH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);                // wave-uniform: weight addresses stay scalar
    const int u0 = 16*q;                                                    // first hidden unit of this wave in the sample-major phases
    const int jb = tid & 15, kb = tid >> 4;                                 // unit-major phase: rows 4jb.. x columns 4kb.. of dW1
    const int xi = kb < OD ? kb : OD - 1, hi = kb < NH ? kb : NH - 1, ci = tid < 2*ACT_DIM ? tid : 2*ACT_DIM;
    const float inv_mb = 1.0f/(float)A.mb;
    const float a_mean = A.adv_stats[0], a_scale = 1.0f/(A.adv_stats[1] + 1e-8f);
    float gW1[16], gW0[4], gB1[4], gB0[4], gWh[4], gcol = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; i++) gW1[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) gW0[i] = gB1[i] = gB0[i] = gWh[i] = 0.0f;
    float s_loss = 0.0f, s_clip = 0.0f;                                     // wave 0, lane = sample: sums over this lane's samples
    [[maybe_unused]] float s_kl = 0.0f, s_ent = 0.0f;                       // EX, policy tower: approx_kl and entropy
    const int ntiles = (A.mb + LT - 1)/LT;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int sm = tile*LT + lane;
        bool valid = sm < A.mb;
        long row = valid ? (A.idx ? (long)A.idx[sm] : (long)sm) : 0;
        if (row < 0 || row >= A.num_samples) { valid = false; row = 0; }  // an index outside the chunk contributes nothing
        const float* __restrict__ r = A.chunk + row*ROW;
        float x[OD];
#pragma unroll
        for (int i = 0; i < OD; i++) {
            // NORM: each entry compiles to a block of its own under `valid` (one vector load, two scalar loads, a wait).  Forming the value for
            // every lane and selecting it removes the blocks and was measured slower at obs_dim 15, so the form stays.
            if constexpr (NORM) x[i] = valid ? obs_normalized(r[i], nrm[i], nrm[OD + i]) : 0.0f;
            else x[i] = valid ? r[i] : 0.0f;
        }
        // ---- layer 1, units u0..u0+15 of this lane's sample
        float h1[16];
#pragma unroll
        for (int jj = 0; jj < 16; jj++) {
            float acc = B0[u0 + jj];
#pragma unroll
            for (int i = 0; i < OD; i++) acc = fmaf(W0[(u0 + jj)*OD + i], x[i], acc);
            h1[jj] = fast_tanh(acc);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) st4(&S.H1[lane*LLD + u0 + 4*c], h1[4*c], h1[4*c + 1], h1[4*c + 2], h1[4*c + 3]);
        if (q == 0) {
#pragma unroll
            for (int i = 0; i < OD; i++) S.X[lane*XLD + i] = x[i];
        }
        __syncthreads();
        // ---- layer 2
        float h2[16];
#pragma unroll
        for (int jj = 0; jj < 16; jj++) h2[jj] = B1[u0 + jj];
#pragma unroll 2
        for (int k = 0; k < HID; k += 4) {
            const float4 hv = ld4(&S.H1[lane*LLD + k]);
#pragma unroll
            for (int jj = 0; jj < 16; jj++) {
                const float* w = W1 + (u0 + jj)*HID + k;
                h2[jj] = fmaf(w[3], hv.w, fmaf(w[2], hv.z, fmaf(w[1], hv.y, fmaf(w[0], hv.x, h2[jj]))));
            }
        }
#pragma unroll
        for (int jj = 0; jj < 16; jj++) h2[jj] = fast_tanh(h2[jj]);
#pragma unroll
        for (int c = 0; c < 4; c++) st4(&S.H2[lane*LLD + u0 + 4*c], h2[4*c], h2[4*c + 1], h2[4*c + 2], h2[4*c + 3]);
        // ---- head: this wave's 16 units' share of each output
#pragma unroll
        for (int i = 0; i < NH; i++) {
            float p = 0.0f;
#pragma unroll
            for (int jj = 0; jj < 16; jj++) p = fmaf(WH[i*HID + u0 + jj], h2[jj], p);
            S.HP[(q*LT + lane)*HPLD + i] = p;
        }
        __syncthreads();
        // ---- loss head of this lane's sample (every wave computes it: each needs the output derivatives for its units)
        float out[NH], dout[NH];
#pragma unroll
        for (int i = 0; i < NH; i++)
            out[i] = (((BH[i] + S.HP[(0*LT + lane)*HPLD + i]) + S.HP[(1*LT + lane)*HPLD + i]) + S.HP[(2*LT + lane)*HPLD + i]) + S.HP[(3*LT + lane)*HPLD + i];
        typename HeadOf<EX>::type L;
        if constexpr (TW == 0) {
            float a[ACT_DIM], ls[ACT_DIM];
#pragma unroll
            for (int i = 0; i < ACT_DIM; i++) { a[i] = valid ? r[OD + ROW_ACT + i] : 0.0f; ls[i] = prm[oLS + i]; }
            const float logp_old = valid ? r[OD + ROW_LOGP] : 0.0f;
            const float adv_n = valid ? (A.adv[row] - a_mean)*a_scale : 0.0f;
            if constexpr (EX) {
                policy_loss_head_ex<float>(out, ls, a, logp_old, adv_n, A.clip, A.ent_coef, inv_mb, L);
                s_kl += valid ? L.approx_kl : 0.0f; s_ent += valid ? L.entropy : 0.0f;
            } else {
                policy_loss_head<float>(out, ls, a, logp_old, adv_n, A.clip, inv_mb, L);
            }
#pragma unroll
            for (int i = 0; i < ACT_DIM; i++) { dout[i] = valid ? L.dmu[i] : 0.0f; L.dlog_std[i] = valid ? L.dlog_std[i] : 0.0f; }
            s_loss += valid ? L.pg_loss : 0.0f; s_clip += valid ? L.clipped : 0.0f;
            if (q == 0) {
#pragma unroll
                for (int i = 0; i < ACT_DIM; i++) { S.DO[lane*DOLD + i] = dout[i]; S.DO[lane*DOLD + ACT_DIM + i] = L.dlog_std[i]; }
                S.DO[lane*DOLD + 2*ACT_DIM] = 0.0f;
            }
        } else {
            if constexpr (EX) {
                value_loss_head_ex<float>(out[0], valid ? r[OD + ROW_VALUE] : 0.0f, valid ? A.ret[row] : 0.0f, A.clip_vf, A.vf_coef, inv_mb, L);
                s_clip += valid ? L.v_clipped : 0.0f;
            } else {
                value_loss_head<float>(out[0], valid ? A.ret[row] : 0.0f, A.vf_coef, inv_mb, L);
            }
            dout[0] = valid ? L.dV : 0.0f;
            s_loss += valid ? L.v_loss : 0.0f;
            if (q == 0) {
                S.DO[lane*DOLD] = dout[0];
#pragma unroll
                for (int i = 1; i <= 2*ACT_DIM; i++) S.DO[lane*DOLD + i] = 0.0f;
            }
        }
        // ---- dZ2 of this wave's units
        float d2[16];
#pragma unroll
        for (int jj = 0; jj < 16; jj++) {
            float d = 0.0f;
#pragma unroll
            for (int i = 0; i < NH; i++) d = fmaf(WH[i*HID + u0 + jj], dout[i], d);
            d2[jj] = d*(1.0f - h2[jj]*h2[jj]);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) st4(&S.D2[lane*LLD + u0 + 4*c], d2[4*c], d2[4*c + 1], d2[4*c + 2], d2[4*c + 3]);
        __syncthreads();
        // ---- dZ1 of this wave's units: dH1 = dZ2 . W1
        float d1[16];
#pragma unroll
        for (int kk = 0; kk < 16; kk++) d1[kk] = 0.0f;
#pragma unroll 2
        for (int j = 0; j < HID; j += 4) {
            const float4 dv = ld4(&S.D2[lane*LLD + j]);
#pragma unroll
            for (int kk = 0; kk < 16; kk++) {
                const float* w = W1 + j*HID + u0 + kk;
                d1[kk] = fmaf(w[3*HID], dv.w, fmaf(w[2*HID], dv.z, fmaf(w[HID], dv.y, fmaf(w[0], dv.x, d1[kk]))));
            }
        }
#pragma unroll
        for (int kk = 0; kk < 16; kk++) d1[kk] *= 1.0f - h1[kk]*h1[kk];
#pragma unroll
        for (int c = 0; c < 4; c++) st4(&S.D1[lane*LLD + u0 + 4*c], d1[4*c], d1[4*c + 1], d1[4*c + 2], d1[4*c + 3]);
        __syncthreads();
        // ---- weight gradients, unit-major: sums over the tile's samples in sample order.  Every thread forms every kind of sum (clamped
        // indices); the write-out below keeps the ones it owns.
#pragma unroll 2
        for (int s = 0; s < LT; s++) {
            const float4 dj = ld4(&S.D2[s*LLD + 4*jb]), hk = ld4(&S.H1[s*LLD + 4*kb]);
            const float4 dk = ld4(&S.D1[s*LLD + 4*jb]), hj = ld4(&S.H2[s*LLD + 4*jb]);
            const float xs = S.X[s*XLD + xi], ds = S.DO[s*DOLD + hi];
            const float dja[4] = { dj.x, dj.y, dj.z, dj.w }, hka[4] = { hk.x, hk.y, hk.z, hk.w };
            const float dka[4] = { dk.x, dk.y, dk.z, dk.w }, hja[4] = { hj.x, hj.y, hj.z, hj.w };
#pragma unroll
            for (int a = 0; a < 4; a++) {
#pragma unroll
                for (int b = 0; b < 4; b++) gW1[4*a + b] = fmaf(dja[a], hka[b], gW1[4*a + b]);
                gB1[a] += dja[a];
                gW0[a] = fmaf(dka[a], xs, gW0[a]);
                gB0[a] += dka[a];
                gWh[a] = fmaf(ds, hja[a], gWh[a]);
            }
            gcol += S.DO[s*DOLD + ci];
        }
        __syncthreads();                                                    // the images are rewritten by the next tile
    }
    // ---- this workgroup's partial: [P gradients | NS sums]
    float* __restrict__ pp = A.partial + (size_t)blockIdx.x*(P + NS);
#pragma unroll
    for (int a = 0; a < 4; a++) {
#pragma unroll
        for (int b = 0; b < 4; b++) pp[oW1 + (4*jb + a)*HID + 4*kb + b] = gW1[4*a + b];
        if (kb < OD) pp[oW0 + (4*jb + a)*OD + kb] = gW0[a];
        if (kb == 0) { pp[oB1 + 4*jb + a] = gB1[a]; pp[oB0 + 4*jb + a] = gB0[a]; }
        if (kb < NH) pp[oWH + kb*HID + 4*jb + a] = gWh[a];
    }
    if (tid < NH) pp[oBH + tid] = gcol;
    if (TW == 0 && tid >= ACT_DIM && tid < 2*ACT_DIM) pp[oLS + tid - ACT_DIM] = gcol;
    // the loss sums of wave 0's lanes, added in lane order by one thread
    if (q == 0) { S.HP[lane] = s_loss; S.HP[LT + lane] = s_clip; }
    if constexpr (EX && TW == 0) {
        if (q == 0) { S.HP[2*LT + lane] = s_kl; S.HP[3*LT + lane] = s_ent; }
    }
    __syncthreads();
    if (tid == 0) {
        float a = 0.0f, c = 0.0f;
        for (int l = 0; l < LT; l++) { a += S.HP[l]; c += S.HP[LT + l]; }
        if (TW == 0) { pp[P + 0] = a; pp[P + 2] = c; } else pp[P + 1] = a;
        if constexpr (EX) {
            if (TW == 0) {
                float k = 0.0f, e = 0.0f;
                for (int l = 0; l < LT; l++) { k += S.HP[2*LT + l]; e += S.HP[3*LT + l]; }
                pp[P + 3] = k; pp[P + 5] = e;
            } else {
                pp[P + 4] = c;
            }
        }
    }
    __syncthreads();
}

// Like every kernel of an extended step, the EX one reads the update's `stopped` word first (set by so100_learn_adam_ex of an earlier step of
// this update, never by a kernel of this step before this one ran).
template <int OD, bool EX>
__global__ __launch_bounds__(256) void so100_learn_grad(GradArgsOf<EX> A) {
    if constexpr (EX) { if (A.state != nullptr && A.state[0] != 0) return; }
    __shared__ GradSmem S;
    tower_pass<OD, 0, EX, false>(A, S, nullptr);
    tower_pass<OD, 1, EX, false>(A, S, nullptr);
}

// the same with the observation normaliser (mean[OD], inv_std[OD]): a kernel of its own, so that so100_learn_grad keeps the argument block
// it always had and the normaliser is a __restrict__ parameter
template <int OD, bool EX>
__global__ __launch_bounds__(256) void so100_learn_grad_norm(GradArgsOf<EX> A, const float* __restrict__ norm) {
    if constexpr (EX) { if (A.state != nullptr && A.state[0] != 0) return; }
    __shared__ GradSmem S;
    tower_pass<OD, 0, EX, true>(A, S, norm);
    tower_pass<OD, 1, EX, true>(A, S, norm);
}

// one thread per entry of a partial: the sum over the G workgroups in workgroup order; each block leaves the sum of squares of its gradients
// (state: the extended step's, read by it alone)
template <int NS>
__global__ __launch_bounds__(256) void so100_learn_reduce(const float* __restrict__ partial, int G, int P, float* __restrict__ gsum, float* __restrict__ sq_block,
                                                          const int32_t* __restrict__ state) {
    if constexpr (NS == NSTAT_EX) { if (state != nullptr && state[0] != 0) return; }
    __shared__ float sq[256];
    const int p = blockIdx.x*256 + threadIdx.x, PS = P + NS;
    float s = 0.0f;
    if (p < PS) {
        int g = 0;
        for (; g + 8 <= G; g += 8) {                                       // eight loads in flight, added in workgroup order
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; i++) t[i] = partial[(size_t)(g + i)*PS + p];
#pragma unroll
            for (int i = 0; i < 8; i++) s += t[i];
        }
        for (; g < G; g++) s += partial[(size_t)g*PS + p];
        gsum[p] = s;
    }
    sq[threadIdx.x] = p < P ? s*s : 0.0f;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sq[threadIdx.x] += sq[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sq_block[blockIdx.x] = sq[0];
}

constexpr int reduce_blocks(int P, int NS) { return (P + NS + 255)/256; }

struct AdamArgs { float max_grad_norm, step_size, omb1, beta2, omb2, eps, bc2_sqrt, inv_mb; };     // formed in double on the host (clip_adam_update)
struct TermsArgs { float ent_coef, vf_coef, kl_limit; };               // kl_limit = 1.5 target_kl, <= 0: no stop

// Sums the blocks' sums of squares (every thread the same sum), decides the clip, applies Adam and leaves the step's statistics in out: the four
// of so100_learner_minibatch_step, or (EX) the eight of so100_learner_minibatch_step_ex.
// EX adds the KL stop.  approx_kl comes from the reduced sums, so every thread of every block forms the same value and takes the same
// decision.  Stopped: parameters and moments stay as they are, thread 0 sets state[0] and leaves the stopping minibatch's diagnostics.  A block
// that starts after thread 0 has set the word returns at once -- what it would have decided anyway.  Applied: state[1] counts the step.
template <bool EX>
__device__ __forceinline__ void adam_step(const float* __restrict__ gsum, const float* __restrict__ sq_block, int nblk, int P,
                                          float* __restrict__ params, float* __restrict__ m, float* __restrict__ v,
                                          float* __restrict__ grads_out, float* __restrict__ out, int32_t* state, const AdamArgs& a, const TermsArgs& t) {
    if constexpr (EX) { if (state != nullptr && state[0] != 0) return; }
    float ss = 0.0f;
    for (int b = 0; b < nblk; b++) ss += sq_block[b];                      // the same ordered sum in every thread
    const float norm = lsqrt(ss), coef = clip_coefficient<float>(norm, a.max_grad_norm);
    [[maybe_unused]] float kl = 0.0f;
    bool stop = false;
    if constexpr (EX) { kl = gsum[P + 3]*a.inv_mb; stop = t.kl_limit > 0.0f && kl > t.kl_limit; }
    const int p = blockIdx.x*256 + threadIdx.x;
    if (!stop && p < P) {
        float pv = params[p], mv = m[p], vv = v[p];
        const float g = clip_adam_update<float>(gsum[p], coef, pv, mv, vv, a.step_size, a.omb1, a.beta2, a.omb2, a.eps, a.bc2_sqrt);
        params[p] = pv; m[p] = mv; v[p] = vv;
        if (grads_out) grads_out[p] = g;
    }
    if (p == 0) {
        const float pg = gsum[P + 0]*a.inv_mb, vl = gsum[P + 1]*a.inv_mb;
        [[maybe_unused]] float ent_loss = 0.0f;
        if constexpr (EX) ent_loss = -(gsum[P + 5]*a.inv_mb);
        out[0] = pg; out[1] = vl; out[2] = gsum[P + 2]*a.inv_mb; out[3] = norm;
        if constexpr (EX) {
            out[4] = kl; out[5] = ent_loss; out[6] = pg + t.ent_coef*ent_loss + t.vf_coef*vl; out[7] = gsum[P + 4]*a.inv_mb;
            if (state != nullptr) {
                if (stop) state[0] = 1; else state[1] += 1;
            }
        }
    }
}

// the two argument lists differ in the middle (state lies before a), so each head keeps its own kernel around the one body
__global__ __launch_bounds__(256) void so100_learn_adam(const float* __restrict__ gsum, const float* __restrict__ sq_block, int nblk, int P,
                                                        float* __restrict__ params, float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ grads_out, float* __restrict__ stats_out, AdamArgs a) {
    adam_step<false>(gsum, sq_block, nblk, P, params, m, v, grads_out, stats_out, nullptr, a, TermsArgs{});
}

__global__ __launch_bounds__(256) void so100_learn_adam_ex(const float* __restrict__ gsum, const float* __restrict__ sq_block, int nblk, int P,
                                                           float* __restrict__ params, float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ grads_out, float* __restrict__ diag, int32_t* state, AdamArgs a, TermsArgs t) {
    adam_step<true>(gsum, sq_block, nblk, P, params, m, v, grads_out, diag, state, a, t);
}

// ---- advantages -------------------------------------------------------------------------------------------------------------------------
// V(obs) of one row in one lane: the weights are wave-uniform (scalar cache), the activations stay in registers
// NORM: nm is the observation normaliser (mean[OD], inv_std[OD]), wave-uniform like the weights
template <int OD, bool NORM>
__device__ __forceinline__ float value_tower(const float* __restrict__ prm, const float* __restrict__ obs, const float* __restrict__ nm) {
    const float* __restrict__ W0 = prm + tensor_offset(T_vf_w0, OD); const float* __restrict__ B0 = prm + tensor_offset(T_vf_b0, OD);
    const float* __restrict__ W1 = prm + tensor_offset(T_vf_w1, OD); const float* __restrict__ B1 = prm + tensor_offset(T_vf_b1, OD);
    const float* __restrict__ VW = prm + tensor_offset(T_v_w, OD);
    float x[OD], h1[HID];
#pragma unroll
    for (int i = 0; i < OD; i++) {
        if constexpr (NORM) x[i] = obs_normalized(obs[i], nm[i], nm[OD + i]);
        else x[i] = obs[i];
    }
#pragma unroll
    for (int j = 0; j < HID; j++) {
        float acc = B0[j];
#pragma unroll
        for (int i = 0; i < OD; i++) acc = fmaf(W0[j*OD + i], x[i], acc);
        h1[j] = fast_tanh(acc);
    }
    float v = prm[tensor_offset(T_v_b, OD)];
#pragma unroll 2
    for (int j = 0; j < HID; j++) {
        float acc = B1[j];
#pragma unroll
        for (int k = 0; k < HID; k++) acc = fmaf(W1[j*HID + k], h1[k], acc);
        v = fmaf(VW[j], fast_tanh(acc), v);
    }
    return v;
}

// The value tower where the scan needs it and nowhere else: rows [0, TN) are the chunk's entries, of which those with done code 2 get
// V(terminal_obs) parked in ret (the scan reads it before it writes ret); rows [TN, TN + N) are the last observations, V parked in adv[T-1].
template <int OD, bool NORM>
__global__ __launch_bounds__(256) void so100_learn_values(const float* __restrict__ chunk, const float* __restrict__ tobs, const float* __restrict__ last_obs,
                                                          const float* __restrict__ prm, long TN, int N, float* __restrict__ adv, float* __restrict__ ret,
                                                          const float* __restrict__ nm) {
    constexpr int ROW = OD + ROW_EXTRA;
    const long r = (long)blockIdx.x*256 + threadIdx.x;
    if (r < TN) {
        if (tobs != nullptr && chunk[r*ROW + OD + ROW_DONE] == 2.0f) ret[r] = value_tower<OD, NORM>(prm, tobs + r*OD, nm);
    } else if (r < TN + N) {
        adv[TN - N + (r - TN)] = value_tower<OD, NORM>(prm, last_obs + (r - TN)*OD, nm);
    }
}

// rewards: null, the chunk's reward column; else [T][N] dense (so100_learner_advantages_r), the step's reward in place of that column
template <int OD>
__global__ __launch_bounds__(64) void so100_learn_gae(const float* chunk, const float* rewards, int T, int N, bool bootstrap, float gamma, float lam, float* adv, float* ret) {
    constexpr int ROW = OD + ROW_EXTRA;
    const int n = blockIdx.x*64 + threadIdx.x;
    if (n >= N) return;
    const float* c = chunk + (size_t)n*ROW + OD;
    const float next_v_last = adv[(size_t)(T - 1)*N + n];
    const float* rew = rewards ? rewards + n : c + ROW_REWARD;
    const long rew_stride = rewards ? (long)N : (long)N*ROW;
    gae_scan_env<float>(T, rew, rew_stride, c + ROW_DONE, c + ROW_VALUE, (long)N*ROW, bootstrap ? ret + n : nullptr, next_v_last, gamma, lam, adv + n, ret + n, (long)N);
}

__device__ __forceinline__ float block_sum_1024(float v, float* sh) {      // fixed tree: the same order every run
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = ADV_THREADS/2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// mean and unbiased standard deviation of adv (torch: a.mean(), a.std()), two passes, one workgroup
__global__ __launch_bounds__(ADV_THREADS) void so100_learn_adv_stats(const float* __restrict__ adv, long n, float* __restrict__ stats) {
    __shared__ float sh[ADV_THREADS];
    float s = 0.0f;
    for (long i = threadIdx.x; i < n; i += ADV_THREADS) s += adv[i];
    const float mean = block_sum_1024(s, sh)/(float)n;
    float q = 0.0f;
    for (long i = threadIdx.x; i < n; i += ADV_THREADS) { const float d = adv[i] - mean; q = fmaf(d, d, q); }
    const float ss = block_sum_1024(q, sh);
    if (threadIdx.x == 0) { stats[0] = mean; stats[1] = lsqrt(ss/(float)(n - 1)); }       // n = 1: 0/0 = NaN, as torch
}

// mean and unbiased standard deviation of adv over the valid rows idx names (idx null: rows 0..mb-1), two passes, one workgroup: the
// statistics of SB3's per-minibatch normalisation.  With at most one valid row SB3 leaves the advantages as they are: the pair (0, 1)
// does that to the bit, (A - 0)*(1/(1 + 1e-8f)) = A in fp32.
__global__ __launch_bounds__(ADV_THREADS) void so100_learn_mb_adv_stats(const float* __restrict__ adv, long num_samples, const int64_t* __restrict__ idx, int mb,
                                                                        float* __restrict__ stats, const int32_t* __restrict__ state) {
    __shared__ float sh[ADV_THREADS];
    __shared__ int cnt;
    if (state != nullptr && state[0] != 0) return;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    float s = 0.0f; int c = 0;
    for (int i = threadIdx.x; i < mb; i += ADV_THREADS) {
        const long row = idx ? (long)idx[i] : (long)i;
        if (row >= 0 && row < num_samples) { s += adv[row]; c++; }
    }
    atomicAdd(&cnt, c);                                                     // an integer count: exact in any order
    const float sum = block_sum_1024(s, sh);                               // (its barriers publish cnt)
    const int n = cnt;
    const float mean = sum/(float)n;
    float q = 0.0f;
    for (int i = threadIdx.x; i < mb; i += ADV_THREADS) {
        const long row = idx ? (long)idx[i] : (long)i;
        if (row >= 0 && row < num_samples) { const float d = adv[row] - mean; q = fmaf(d, d, q); }
    }
    const float ss = block_sum_1024(q, sh);
    if (threadIdx.x == 0) {
        if (n > 1) { stats[0] = mean; stats[1] = lsqrt(ss/(float)(n - 1)); }
        else { stats[0] = 0.0f; stats[1] = 1.0f; }
    }
}

// explained_variance = 1 - var(ret - old_V)/var(ret) over the chunk (population variances), NaN when var(ret) == 0.  old_V is the chunk's
// value column (row stride `row` floats, first entry at chunk + value_col).  Stage 1: workgroup g owns the contiguous rows
// [g per, (g+1) per) and leaves their count, the two means and the two sums of squared deviations from those means (two passes, fixed trees).
// Stage 2: one thread merges the workgroups' moments in workgroup order (Chan et al.'s pairwise update).  The same bits every run.
// A thread keeps its first row in registers across the two passes: with at most 1024 rows per slice (any chunk up to 262 144 rows) the packed
// chunk is read once.  A constant ret has variance 0 by definition, whatever rounding leaves in the sum of squares: each slice also records
// whether any of its rows differs from ret[0], and the merge returns NaN when none does.
constexpr int EV_GRID_MAX = 256, EV_PART = 6;
__global__ __launch_bounds__(ADV_THREADS) void so100_learn_ev_moments(const float* __restrict__ chunk, int row, int value_col, const float* __restrict__ ret,
                                                                      long n, long per, float* __restrict__ part) {
    __shared__ float sh[ADV_THREADS];
    const long lo = (long)blockIdx.x*per, hi = lo + per < n ? lo + per : n;
    const float cnt = (float)(hi - lo), first = ret[0];
    const long i0 = lo + threadIdx.x;
    const bool own = i0 < hi;
    const float r0 = own ? ret[i0] : 0.0f, d0 = own ? r0 - chunk[i0*row + value_col] : 0.0f;
    float sr = r0, sd = d0;
    int differs = own && r0 != first;
    for (long i = i0 + ADV_THREADS; i < hi; i += ADV_THREADS) { const float r = ret[i]; sr += r; sd += r - chunk[i*row + value_col]; differs |= r != first; }
    const float mr = block_sum_1024(sr, sh)/cnt, md = block_sum_1024(sd, sh)/cnt;
    float qr = 0.0f, qd = 0.0f;
    if (own) { const float a = r0 - mr, b = d0 - md; qr = a*a; qd = b*b; }
    for (long i = i0 + ADV_THREADS; i < hi; i += ADV_THREADS) {
        const float r = ret[i], a = r - mr, b = (r - chunk[i*row + value_col]) - md;
        qr = fmaf(a, a, qr); qd = fmaf(b, b, qd);
    }
    const float m2r = block_sum_1024(qr, sh), m2d = block_sum_1024(qd, sh);
    const int any = __syncthreads_or(differs);
    if (threadIdx.x == 0) {
        float* o = part + (size_t)blockIdx.x*EV_PART;
        o[0] = cnt; o[1] = mr; o[2] = m2r; o[3] = md; o[4] = m2d; o[5] = any ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(256) void so100_learn_ev_merge(const float* __restrict__ gpart, int G, float* __restrict__ out) {
    __shared__ float part[EV_GRID_MAX*EV_PART];                            // fetched by all threads at once; the merge itself is one thread's, in order
    for (int i = threadIdx.x; i < G*EV_PART; i += 256) part[i] = gpart[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    float n = part[0], mr = part[1], m2r = part[2], md = part[3], m2d = part[4], differs = part[5];
    for (int g = 1; g < G; g++) {
        const float* p = part + g*EV_PART;
        const float ng = p[0], tot = n + ng, w = ng/tot, dr = p[1] - mr, dd = p[3] - md;
        mr = fmaf(dr, w, mr); m2r += p[2] + dr*dr*n*w;
        md = fmaf(dd, w, md); m2d += p[4] + dd*dd*n*w;
        n = tot; differs += p[5];
    }
    out[0] = (differs == 0.0f || m2r == 0.0f) ? __builtin_nanf("") : 1.0f - m2d/m2r;
}

// ---- reward normalisation (so100_learner_normalize_rewards) -------------------------------------------------------------------------------
// The dependency between steps runs through three scalars only (mean, var, count); each env's discounted return is a recurrence of its own.
// So the pass is three launches.  Scan: one wave per block of RN_BLOCK envs, lane = env, walks t with its R in a register and leaves the
// block's (mean, M2) of R for every t (two wave tree sums per step over DPP/permute lanes: no LDS, no barrier), all blocks side by side over
// the CUs; rewards and codes are fetched RN_AHEAD steps ahead of the sums that wait on nothing else.  Merge: one workgroup; thread t merges
// the blocks' moments of step t in block order (the steps are independent there), then one thread runs the T running-moment updates in t
// order from LDS and leaves the T denominators sqrt(var' + epsilon).  Scale: one thread per entry.  fp64 throughout, rounded at the store.
constexpr int RN_AHEAD = 8, RN_MERGE_THREADS = 256;

// workspace: [T][G][2] doubles (mean, M2 of block g at step t), then [T] denominators
__host__ __device__ constexpr long rn_blocks(long N) { return (N + RN_BLOCK - 1)/RN_BLOCK; }
constexpr long rn_workspace_doubles(long T, long N) { return T*rn_blocks(N)*2 + T; }

// lane 0 ends with block_tree_sum's sum: lane i += lane i + w for w = 32 .. 1 (a lane past 63 - w adds its own value: never read by lane 0's tree)
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
    for (int w = RN_BLOCK/2; w > 0; w >>= 1) v += __shfl_down(v, w, RN_BLOCK);
    return __shfl(v, 0, RN_BLOCK);
}

__global__ __launch_bounds__(RN_BLOCK) void so100_learn_rn_scan(const float* __restrict__ chunk, int row, int rew_col, int code_col, int T, int N, double gamma,
                                                               double* __restrict__ state, double* __restrict__ part) {
    const int g = blockIdx.x, G = gridDim.x, lane = threadIdx.x, n = g*RN_BLOCK + lane;
    const bool own = n < N;
    const int count = N - g*RN_BLOCK < RN_BLOCK ? N - g*RN_BLOCK : RN_BLOCK;
    double* __restrict__ Rn = state + 3 + (own ? n : 0);
    double R = own ? *Rn : 0.0;
    for (int t0 = 0; t0 < T; t0 += RN_AHEAD) {
        float r[RN_AHEAD], c[RN_AHEAD];
#pragma unroll
        for (int k = 0; k < RN_AHEAD; k++) {
            const bool in = own && t0 + k < T;
            const float* p = chunk + ((size_t)(in ? t0 + k : 0)*N + (in ? n : 0))*row;
            r[k] = in ? p[rew_col] : 0.0f; c[k] = in ? p[code_col] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < RN_AHEAD; k++) {
            const int t = t0 + k;
            if (t < T) {                                                     // uniform over the wave
                R = own ? return_step<double>(R, gamma, (double)r[k]) : 0.0;
                const double mean = block_mean<double>(wave_tree_sum(R), count);
                const double m2 = wave_tree_sum(own ? squared_deviation<double>(R, mean) : 0.0);
                if (lane == 0) { double* o = part + ((size_t)t*G + g)*2; o[0] = mean; o[1] = m2; }
                if (c[k] != 0.0f) R = 0.0;
            }
        }
    }
    if (own) *Rn = R;
}

__global__ __launch_bounds__(RN_MERGE_THREADS) void so100_learn_rn_merge(const double* __restrict__ part, int T, int N, int G, double epsilon,
                                                                         double* __restrict__ state, double* __restrict__ denom) {
    __shared__ double bm[RN_MERGE_THREADS], bv[RN_MERGE_THREADS];
    const int tid = threadIdx.x;
    double mean = 0.0, var = 0.0, cnt = 0.0;
    if (tid == 0) { mean = state[0]; var = state[1]; cnt = state[2]; }
    for (int base = 0; base < T; base += RN_MERGE_THREADS) {
        const int t = base + tid;
        if (t < T) {
            const double* p = part + (size_t)t*G*2;
            double na = (double)(N < RN_BLOCK ? N : RN_BLOCK), m = p[0], m2 = p[1];
            for (int g = 1; g < G; g++) {
                const int left = N - g*RN_BLOCK;
                chan_merge<double>(na, m, m2, (double)(left < RN_BLOCK ? left : RN_BLOCK), p[2*g], p[2*g + 1]);
            }
            bm[tid] = m; bv[tid] = m2/(double)N;
        }
        __syncthreads();
        if (tid == 0) {
            const int steps = T - base < RN_MERGE_THREADS ? T - base : RN_MERGE_THREADS;
            for (int i = 0; i < steps; i++) {
                running_moment_update<double>(mean, var, cnt, bm[i], bv[i], (double)N);
                bm[i] = reward_denominator<double>(var, epsilon);
            }
        }
        __syncthreads();
        if (t < T) denom[t] = bm[tid];
        __syncthreads();
    }
    if (tid == 0) { state[0] = mean; state[1] = var; state[2] = cnt; }
}

constexpr int RN_SCALE_GRID_MAX = 2048;
__global__ __launch_bounds__(256) void so100_learn_rn_scale(const float* __restrict__ chunk, int row, int rew_col, long TN, int N, const double* __restrict__ denom,
                                                            double clip, float* __restrict__ out) {
    for (long i = (long)blockIdx.x*256 + threadIdx.x; i < TN; i += (long)gridDim.x*256)
        out[i] = reward_scale<float, double>((double)chunk[i*row + rew_col], denom[i/N], clip);
}

__global__ __launch_bounds__(256) void so100_learn_rn_init(double* __restrict__ state, long len) {
    for (long i = (long)blockIdx.x*256 + threadIdx.x; i < len; i += (long)gridDim.x*256) state[i] = i == 1 ? 1.0 : i == 2 ? 1e-4 : 0.0;
}

// ---- observation normalisation (so100_learner_obs_norm_update / _fold) ----------------------------------------------------------------------
// Moments: one workgroup per block of ON_BLOCK rows, thread j = row j of the block.  A thread widens its row's observations to fp64 and parks
// them in LDS [dimension][slot]; the trees of all dimensions run side by side (one barrier per level, not per dimension), first over the values,
// then over the squared deviations.  Merge: one workgroup; a thread per (dimension, group) folds its group's blocks in block order, then a thread
// per dimension folds the groups in group order and applies the running update; thread 0 stores the count all dimensions share.  At 262 144
// rows that is 1024 blocks, 16 groups: chains of 64 and of 16 merges.  Fold: one thread per first-layer row or copied parameter.
constexpr int ON_MAX_OD = 15, ON_MERGE_THREADS = 256;
constexpr long ON_MAX_ROWS = 1L << 24;

// workspace: [B][od][2] doubles (mean, M2 of block b, dimension i), then [G][od][3] (n, mean, M2 of group g); sized for ON_MAX_OD
constexpr long on_workspace_doubles(long rows) { return on_blocks(rows)*ON_MAX_OD*2 + on_groups(rows)*ON_MAX_OD*3; }

__device__ __forceinline__ void on_tree(double* sh, int od, int tid) {
    for (int w = ON_BLOCK/2; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w)
            for (int i = 0; i < od; i++) sh[i*ON_BLOCK + tid] += sh[i*ON_BLOCK + tid + w];
    }
    __syncthreads();
}

template <int OD>
__global__ __launch_bounds__(ON_BLOCK) void so100_learn_on_moments(const float* __restrict__ chunk, long rows, double* __restrict__ part) {
    constexpr int od = OD, row = OD + ROW_EXTRA;
    __shared__ double sh[ON_MAX_OD*ON_BLOCK];
    __shared__ double bmean[ON_MAX_OD];
    const int tid = threadIdx.x;
    const long b = blockIdx.x, r = b*ON_BLOCK + tid;
    const bool own = r < rows;
    const long count = on_block_count(rows, b);
    double x[OD];
#pragma unroll
    for (int i = 0; i < od; i++) { x[i] = own ? (double)chunk[(size_t)r*row + i] : 0.0; sh[i*ON_BLOCK + tid] = x[i]; }
    on_tree(sh, od, tid);
    if (tid < od) bmean[tid] = block_mean<double>(sh[tid*ON_BLOCK], (int)count);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < od; i++) sh[i*ON_BLOCK + tid] = own ? squared_deviation<double>(x[i], bmean[i]) : 0.0;
    on_tree(sh, od, tid);
    if (tid < od) { double* o = part + ((size_t)b*od + tid)*2; o[0] = bmean[tid]; o[1] = sh[tid*ON_BLOCK]; }
}

__global__ __launch_bounds__(ON_MERGE_THREADS) void so100_learn_on_merge(const double* __restrict__ part, double* __restrict__ grp, int od, long rows,
                                                                         double* __restrict__ state) {
    const long B = on_blocks(rows), G = on_groups(rows);
    const int tid = threadIdx.x;
    for (long k = tid; k < G*od; k += ON_MERGE_THREADS) {
        const long g = k/od; const int i = (int)(k - g*od);
        const long b0 = g*ON_GROUP, b1 = b0 + ON_GROUP < B ? b0 + ON_GROUP : B;
        double n, m, m2;
        obs_group_merge<double>(part + 2*i, 2L*od, rows, b0, b1, n, m, m2);
        double* o = grp + (size_t)k*3; o[0] = n; o[1] = m; o[2] = m2;
    }
    __threadfence_block();
    __syncthreads();
    double count = state[2*od];
    __syncthreads();                                                        // every thread holds the old count before thread 0 stores the new one
    if (tid < od) {
        double mean = state[tid], var = state[od + tid];
        obs_moment_update<double>(grp + 3*tid, 3L*od, G, rows, mean, var, count);
        state[tid] = mean; state[od + tid] = var;
        if (tid == 0) state[2*od] = count;
    }
}

struct FoldArgs { int od, P, oW0[2], oB0[2]; };                             // the two towers' first layers in the block

__global__ __launch_bounds__(256) void so100_learn_on_fold(const double* __restrict__ state, double epsilon, const float* __restrict__ params,
                                                           float* __restrict__ folded, float* __restrict__ norm, FoldArgs a) {
    __shared__ double mean[ON_MAX_OD], inv[ON_MAX_OD];
    const int tid = threadIdx.x, od = a.od;
    if (tid < od) { mean[tid] = state[tid]; inv[tid] = obs_inv_std<double>(state[od + tid], epsilon); }
    __syncthreads();
    if (blockIdx.x == 0 && tid < od) { norm[tid] = (float)mean[tid]; norm[od + tid] = (float)inv[tid]; }
    const int p = blockIdx.x*256 + tid;
    if (p >= a.P) return;
    for (int tw = 0; tw < 2; tw++) {
        if (p >= a.oW0[tw] && p < a.oW0[tw] + HID*od) return;               // written by its row's thread below
        if (p >= a.oB0[tw] && p < a.oB0[tw] + HID) {
            const int j = p - a.oB0[tw];
            float w[ON_MAX_OD], b;
            obs_fold_row<double>(od, params + a.oW0[tw] + j*od, params[p], mean, inv, w, b);
            for (int i = 0; i < od; i++) folded[a.oW0[tw] + j*od + i] = w[i];
            folded[p] = b;
            return;
        }
    }
    folded[p] = params[p];
}

__global__ __launch_bounds__(64) void so100_learn_on_init(double* __restrict__ state, int od) {
    const int i = threadIdx.x;
    if (i <= 2*od) state[i] = i < od ? 0.0 : i < 2*od ? 1.0 : 1e-4;
}

// ---- the whole update (so100_learner_update) ---------------------------------------------------------------------------------------------
// One thread per position of the epoch, grid-stride; the only traffic is the store.  The walk of shuffle_index diverges (fewer than 4 maps
// per position on average, 26 at the worst seen), which costs a wave its longest lane's maps and nothing else: no LDS, no atomics.
constexpr int SHUFFLE_GRID_MAX = 1024;
__global__ __launch_bounds__(256) void so100_learn_shuffle(uint32_t n, uint32_t seed_lo, uint32_t seed_hi, uint32_t epoch, int64_t* __restrict__ perm) {
    const uint64_t seed = ((uint64_t)seed_hi << 32) | seed_lo;
    for (uint64_t i = (uint64_t)blockIdx.x*256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x*256) perm[i] = (int64_t)shuffle_index((uint32_t)i, n, seed, epoch);
}

// the two small stream-ordered writes of an update: the zeroed {stopped, steps_applied} pair, and log_std as the last step is about to read it
__global__ __launch_bounds__(64) void so100_learn_zero_state(int32_t* __restrict__ state) {
    if (threadIdx.x < 2) state[threadIdx.x] = 0;
}

__global__ __launch_bounds__(64) void so100_learn_copy_log_std(const float* __restrict__ log_std, float* __restrict__ out) {
    if (threadIdx.x < ACT_DIM) out[threadIdx.x] = log_std[threadIdx.x];
}

const char* const kTensorNames[NUM_TENSORS] = {
#define X(name, rows, cols) #name,
    SO100_POLICY_TENSORS(X)
#undef X
};

int tensor_index(const char* name) {
    if (!name) return -1;
    for (int t = 0; t < NUM_TENSORS; t++) if (strcmp(kTensorNames[t], name) == 0) return t;
    return -1;
}

}  // namespace learn
}  // namespace so100

using namespace so100;
using namespace so100::learn;

struct so100_learner {
    so100_learner_config cfg;
    int P = 0, grid_max = 0;
    float* partial = nullptr;      // [grid_max][P + NSTAT_EX] per-workgroup partial gradients (the plain head strides them by P + NSTAT)
    float* gsum = nullptr;         // [P + NSTAT_EX] their ordered sum
    float* sq_block = nullptr;     // [reduce_blocks(P, NSTAT_EX)] sum of squares per block of the reduction
    float* mb_stats = nullptr;     // [2] mean and std of the minibatch's advantages (normalize_advantage = 1)
    float* ev_part = nullptr;      // [EV_GRID_MAX][EV_PART] per-workgroup moments of so100_learner_explained_variance
    const float* obs_norm = nullptr;       // the caller's [2 obs_dim] normaliser (so100_learner_set_obs_norm); null: off
};

static AdamArgs adam_args(const so100_learner_config& c, double lr, int adam_step, int mb) {
    AdamArgs a;
    a.max_grad_norm = c.max_grad_norm;
    a.step_size = (float)(lr/(1.0 - pow(c.beta1, (double)adam_step))); a.bc2_sqrt = (float)sqrt(1.0 - pow(c.beta2, (double)adam_step));
    a.omb1 = (float)(1.0 - c.beta1); a.beta2 = (float)c.beta2; a.omb2 = (float)(1.0 - c.beta2); a.eps = (float)c.adam_eps;
    a.inv_mb = 1.0f/(float)mb;
    return a;
}

// the extended step's own argument checks (so100_learner_update runs them before it enqueues anything)
static int check_terms(const so100_ppo_terms* terms, const int32_t* state_dev, const char* fn) {
    if (!(terms->ent_coef >= 0.0f)) return fail(SO100_E_INVALID, "%s: ent_coef must be >= 0", fn);
    if (terms->clip_range_vf != terms->clip_range_vf) return fail(SO100_E_INVALID, "%s: clip_range_vf is NaN (<= 0 means off)", fn);
    if (terms->target_kl != terms->target_kl) return fail(SO100_E_INVALID, "%s: target_kl is NaN (<= 0 means off)", fn);
    if (terms->normalize_advantage != 0 && terms->normalize_advantage != 1)
        return fail(SO100_E_INVALID, "%s: normalize_advantage must be 0 (batch) or 1 (minibatch), got %d", fn, terms->normalize_advantage);
    if (terms->lr != terms->lr) return fail(SO100_E_INVALID, "%s: lr is NaN (negative means the handle's)", fn);
    if (terms->target_kl > 0.0f && !state_dev) return fail(SO100_E_INVALID, "%s: target_kl needs the update-state pointer", fn);
    return 0;
}

// The step behind both entry points.  terms null: the plain head, out_dev takes its four statistics; given: the extended head, out_dev takes
// the eight diagnostics and state_dev (nullable) is the update's {stopped, steps_applied}.  fn: the entry point's name, for the messages.
static int minibatch_step(so100_learner* L, const so100_minibatch_io* io, const so100_ppo_terms* terms, float* out_dev, int32_t* state_dev, void* stream, const char* fn) {
    if (!L || !io) return fail(SO100_E_INVALID, "%s: null argument", fn);
    if (io->mb < 1 || io->mb > L->cfg.max_minibatch) return fail(SO100_E_INVALID, "%s: mb must be in 1..max_minibatch, got %d", fn, io->mb);
    if (io->num_samples < 1) return fail(SO100_E_INVALID, "%s: num_samples must be >= 1, got %ld", fn, (long)io->num_samples);
    if (io->adam_step < 1) return fail(SO100_E_INVALID, "%s: adam_step is 1-based, got %d", fn, io->adam_step);
    if (!io->rollout_dev || !io->adv_dev || !io->ret_dev || !io->adv_stats_dev || !io->params_dev || !io->adam_m_dev || !io->adam_v_dev || !out_dev)
        return fail(SO100_E_INVALID, "%s: rollout/adv/ret/adv_stats/params/adam_m/adam_v/%s pointers are required", fn, terms ? "diag" : "stats");
    if (terms) {
        const int rc = check_terms(terms, state_dev, fn);
        if (rc != 0) return rc;
    }
    SO100_ON_DEVICE(L->cfg.device, fn);
    const hipStream_t st = (hipStream_t)stream;
    const int tiles = (io->mb + LT - 1)/LT, G = tiles < L->grid_max ? tiles : L->grid_max;
    const dim3 pblocks((unsigned)((L->P + 255)/256)), threads(256);
    GradArgsEx A;
    A.chunk = io->rollout_dev; A.num_samples = (long)io->num_samples; A.idx = io->idx_dev; A.mb = io->mb;
    A.adv = io->adv_dev; A.ret = io->ret_dev; A.adv_stats = io->adv_stats_dev; A.params = io->params_dev; A.partial = L->partial;
    A.clip = L->cfg.clip_range; A.vf_coef = L->cfg.vf_coef;
    const bool norm = L->obs_norm != nullptr;
    if (terms) {
        A.ent_coef = terms->ent_coef; A.clip_vf = terms->clip_range_vf > 0.0f ? terms->clip_range_vf : 0.0f; A.state = state_dev;
        if (terms->normalize_advantage == 1) {
            hipLaunchKernelGGL(so100_learn_mb_adv_stats, dim3(1), dim3(ADV_THREADS), 0, st, io->adv_dev, (long)io->num_samples, io->idx_dev, io->mb, L->mb_stats, A.state);
            A.adv_stats = L->mb_stats;
        }
        const int nblk = reduce_blocks(L->P, NSTAT_EX);
        const AdamArgs a = adam_args(L->cfg, terms->lr < 0.0 ? L->cfg.lr : terms->lr, io->adam_step, io->mb);
        const TermsArgs t = { terms->ent_coef, L->cfg.vf_coef, terms->target_kl > 0.0f ? (float)(1.5*(double)terms->target_kl) : 0.0f };
        if (norm) { SO100_WITH_OBS_DIM(L->cfg.obs_dim, hipLaunchKernelGGL((so100_learn_grad_norm<OD, true>), dim3((unsigned)G), threads, 0, st, A, L->obs_norm);); }
        else { SO100_WITH_OBS_DIM(L->cfg.obs_dim, hipLaunchKernelGGL((so100_learn_grad<OD, true>), dim3((unsigned)G), threads, 0, st, A);); }
        hipLaunchKernelGGL(so100_learn_reduce<NSTAT_EX>, dim3((unsigned)nblk), threads, 0, st, (const float*)L->partial, G, L->P, L->gsum, L->sq_block, A.state);
        hipLaunchKernelGGL(so100_learn_adam_ex, pblocks, threads, 0, st, (const float*)L->gsum, (const float*)L->sq_block, nblk, L->P,
                           io->params_dev, io->adam_m_dev, io->adam_v_dev, io->grads_dev, out_dev, state_dev, a, t);
    } else {
        const int nblk = reduce_blocks(L->P, NSTAT);
        const AdamArgs a = adam_args(L->cfg, L->cfg.lr, io->adam_step, io->mb);
        if (norm) { SO100_WITH_OBS_DIM(L->cfg.obs_dim, hipLaunchKernelGGL((so100_learn_grad_norm<OD, false>), dim3((unsigned)G), threads, 0, st, static_cast<const GradArgs&>(A), L->obs_norm);); }
        else { SO100_WITH_OBS_DIM(L->cfg.obs_dim, hipLaunchKernelGGL((so100_learn_grad<OD, false>), dim3((unsigned)G), threads, 0, st, static_cast<const GradArgs&>(A));); }
        hipLaunchKernelGGL(so100_learn_reduce<NSTAT>, dim3((unsigned)nblk), threads, 0, st, (const float*)L->partial, G, L->P, L->gsum, L->sq_block, (const int32_t*)nullptr);
        hipLaunchKernelGGL(so100_learn_adam, pblocks, threads, 0, st, (const float*)L->gsum, (const float*)L->sq_block, nblk, L->P,
                           io->params_dev, io->adam_m_dev, io->adam_v_dev, io->grads_dev, out_dev, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SO100_E_LAUNCH, "%s: %s (HIP error %ld)", fn, hipGetErrorString(e), (long)e);
    return 0;
}

// so100_reward_norm_io's checks and launches, apart: so100_learner_update_r runs every check of the update before it enqueues the first launch
static int check_reward_norm(const so100_reward_norm_io* io, int T, int N, const char* fn) {
    if (T < 1) return fail(SO100_E_INVALID, "%s: T must be >= 1, got %d", fn, T);
    if (N < 1) return fail(SO100_E_INVALID, "%s: N must be >= 1, got %d", fn, N);
    if (!io->rollout_dev || !io->state_dev || !io->reward_dev || !io->workspace_dev)
        return fail(SO100_E_INVALID, "%s: rollout/state/reward/workspace pointers are required", fn);
    if (!(io->clip_reward > 0.0)) return fail(SO100_E_INVALID, "%s: clip_reward must be > 0", fn);
    if (!(io->epsilon >= 0.0)) return fail(SO100_E_INVALID, "%s: epsilon must be >= 0", fn);
    const long need = rn_workspace_doubles(T, N)*(long)sizeof(double);
    if (io->workspace_bytes < need) return fail(SO100_E_INVALID, "%s: the workspace holds %ld bytes, T = %d and N = %d need %ld", fn, (long)io->workspace_bytes, T, N, need);
    if (((uintptr_t)io->workspace_dev & 7u) != 0) return fail(SO100_E_INVALID, "%s: the workspace must be 8-byte aligned", fn);
    return 0;
}

static void enqueue_reward_norm(const so100_learner* L, const so100_reward_norm_io* io, int T, int N, hipStream_t st) {
    const int od = L->cfg.obs_dim, row = od + ROW_EXTRA, G = (int)rn_blocks(N);
    const long TN = (long)T*(long)N, want = (TN + 255)/256;
    double* part = (double*)io->workspace_dev;
    double* denom = part + (size_t)T*G*2;
    hipLaunchKernelGGL(so100_learn_rn_scan, dim3((unsigned)G), dim3(RN_BLOCK), 0, st, io->rollout_dev, row, od + ROW_REWARD, od + ROW_DONE, T, N, (double)L->cfg.gamma,
                       io->state_dev, part);
    hipLaunchKernelGGL(so100_learn_rn_merge, dim3(1), dim3(RN_MERGE_THREADS), 0, st, (const double*)part, T, N, G, io->epsilon, io->state_dev, denom);
    hipLaunchKernelGGL(so100_learn_rn_scale, dim3((unsigned)(want < RN_SCALE_GRID_MAX ? want : RN_SCALE_GRID_MAX)), dim3(256), 0, st, io->rollout_dev, row, od + ROW_REWARD,
                       TN, N, (const double*)denom, io->clip_reward, io->reward_dev);
}

// so100_learner_advantages and so100_learner_advantages_r: reward_dev null reads the chunk's reward column
static int advantages(so100_learner* L, const so100_advantages_io* io, const float* reward_dev, int32_t T, int32_t N, void* stream, const char* fn) {
    if (!L || !io) return fail(SO100_E_INVALID, "%s: null argument", fn);
    if (T < 1) return fail(SO100_E_INVALID, "%s: T must be >= 1, got %d", fn, T);
    if (N < 1) return fail(SO100_E_INVALID, "%s: N must be >= 1, got %d", fn, N);
    if (!io->rollout_dev || !io->last_obs_dev || !io->params_dev || !io->adv_dev || !io->ret_dev || !io->adv_stats_dev)
        return fail(SO100_E_INVALID, "%s: rollout/last_obs/params/adv/ret/adv_stats pointers are required", fn);
    SO100_ON_DEVICE(L->cfg.device, fn);
    const long TN = (long)T*(long)N;
    const long vblocks = (TN + N + 255)/256;
    if (vblocks > 0x7fffffffL) return fail(SO100_E_INVALID, "%s: T*N is too large", fn);
    const hipStream_t st = (hipStream_t)stream;
    const bool boot = io->terminal_obs_chunk_dev != nullptr;
    const float* nm = L->obs_norm;
    if (nm) { SO100_WITH_OBS_DIM(L->cfg.obs_dim, hipLaunchKernelGGL((so100_learn_values<OD, true>), dim3((unsigned)vblocks), dim3(256), 0, st, io->rollout_dev, io->terminal_obs_chunk_dev, io->last_obs_dev, io->params_dev, TN, N, io->adv_dev, io->ret_dev, nm);); }
    else { SO100_WITH_OBS_DIM(L->cfg.obs_dim, hipLaunchKernelGGL((so100_learn_values<OD, false>), dim3((unsigned)vblocks), dim3(256), 0, st, io->rollout_dev, io->terminal_obs_chunk_dev, io->last_obs_dev, io->params_dev, TN, N, io->adv_dev, io->ret_dev, nm);); }
    SO100_WITH_OBS_DIM(L->cfg.obs_dim,
        hipLaunchKernelGGL((so100_learn_gae<OD>), dim3((unsigned)((N + 63)/64)), dim3(64), 0, st, io->rollout_dev, reward_dev, T, N, boot, L->cfg.gamma, L->cfg.gae_lambda, io->adv_dev, io->ret_dev););
    hipLaunchKernelGGL(so100_learn_adv_stats, dim3(1), dim3(ADV_THREADS), 0, st, (const float*)io->adv_dev, TN, io->adv_stats_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SO100_E_LAUNCH, "%s: %s (HIP error %ld)", fn, hipGetErrorString(e), (long)e);
    return 0;
}

extern "C" {

int so100_learner_num_params(int32_t obs_dim) { return obs_dim == 15 ? num_params(15) : obs_dim == 8 ? num_params(8) : SO100_E_INVALID; }

int so100_learner_param_offset(int32_t obs_dim, const char* name) {
    const int t = tensor_index(name);
    if (t < 0 || (obs_dim != 15 && obs_dim != 8)) return SO100_E_INVALID;
    return tensor_offset(t, obs_dim);
}

int so100_learner_param_size(int32_t obs_dim, const char* name) {
    const int t = tensor_index(name);
    if (t < 0 || (obs_dim != 15 && obs_dim != 8)) return SO100_E_INVALID;
    return tensor_size(t, obs_dim);
}

int so100_learner_create(const so100_learner_config* cfg, so100_learner** out) {
    if (!cfg || !out) return fail(SO100_E_INVALID, "so100_learner_create: null argument");
    *out = nullptr;
    if (cfg->obs_dim != 15 && cfg->obs_dim != 8) return fail(SO100_E_INVALID, "so100_learner_create: obs_dim must be 15 or 8, got %d", cfg->obs_dim);
    if (cfg->max_minibatch < 1) return fail(SO100_E_INVALID, "so100_learner_create: max_minibatch must be >= 1, got %d", cfg->max_minibatch);
    if (!(cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) return fail(SO100_E_INVALID, "so100_learner_create: gamma must be in [0, 1]");
    if (!(cfg->gae_lambda >= 0.0f && cfg->gae_lambda <= 1.0f)) return fail(SO100_E_INVALID, "so100_learner_create: gae_lambda must be in [0, 1]");
    if (!(cfg->clip_range > 0.0f)) return fail(SO100_E_INVALID, "so100_learner_create: clip_range must be > 0");
    if (!(cfg->vf_coef >= 0.0f)) return fail(SO100_E_INVALID, "so100_learner_create: vf_coef must be >= 0");
    if (!(cfg->max_grad_norm > 0.0f)) return fail(SO100_E_INVALID, "so100_learner_create: max_grad_norm must be > 0");
    if (!(cfg->lr >= 0.0)) return fail(SO100_E_INVALID, "so100_learner_create: lr must be >= 0");
    if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0))
        return fail(SO100_E_INVALID, "so100_learner_create: beta1 and beta2 must be in [0, 1)");
    if (!(cfg->adam_eps > 0.0)) return fail(SO100_E_INVALID, "so100_learner_create: adam_eps must be > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(SO100_E_NODEVICE, "so100_learner_create: no HIP device available (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(SO100_E_INVALID, "so100_learner_create: device ordinal out of range");
    SO100_ON_DEVICE(cfg->device, "so100_learner_create");
    so100_learner* L = new (std::nothrow) so100_learner();
    if (!L) return fail(SO100_E_NOMEM, "so100_learner_create: out of host memory");
    L->cfg = *cfg;
    L->P = num_params(cfg->obs_dim == 15 ? 15 : 8);
    const long tiles = ((long)cfg->max_minibatch + LT - 1)/LT;
    L->grid_max = (int)(tiles < GRID_MAX ? tiles : GRID_MAX);
    const size_t ps = (size_t)(L->P + NSTAT_EX);
    if (hipMalloc(&L->partial, (size_t)L->grid_max*ps*sizeof(float)) != hipSuccess || hipMalloc(&L->gsum, ps*sizeof(float)) != hipSuccess ||
        hipMalloc(&L->sq_block, (size_t)reduce_blocks(L->P, NSTAT_EX)*sizeof(float)) != hipSuccess || hipMalloc(&L->mb_stats, 2*sizeof(float)) != hipSuccess ||
        hipMalloc(&L->ev_part, (size_t)EV_GRID_MAX*EV_PART*sizeof(float)) != hipSuccess) {
        so100_learner_destroy(L);
        return fail(SO100_E_NOMEM, "so100_learner_create: hipMalloc of the partial-gradient scratch failed");
    }
    *out = L;
    return 0;
}

void so100_learner_destroy(so100_learner* L) {
    if (!L) return;
    DeviceGuard g(L->cfg.device);
    if (L->partial) (void)hipFree(L->partial);
    if (L->gsum) (void)hipFree(L->gsum);
    if (L->sq_block) (void)hipFree(L->sq_block);
    if (L->mb_stats) (void)hipFree(L->mb_stats);
    if (L->ev_part) (void)hipFree(L->ev_part);
    delete L;
}

int so100_learner_advantages(so100_learner* L, const so100_advantages_io* io, int32_t T, int32_t N, void* stream) {
    return advantages(L, io, nullptr, T, N, stream, "so100_learner_advantages");
}

int so100_learner_advantages_r(so100_learner* L, const so100_advantages_io* io, const float* reward_dev, int32_t T, int32_t N, void* stream) {
    return advantages(L, io, reward_dev, T, N, stream, "so100_learner_advantages_r");
}

int so100_learner_minibatch_step(so100_learner* L, const so100_minibatch_io* io, void* stream) {
    return minibatch_step(L, io, nullptr, io ? io->stats_dev : nullptr, nullptr, stream, "so100_learner_minibatch_step");
}

int so100_learner_minibatch_step_ex(so100_learner* L, const so100_minibatch_io* io, const so100_ppo_terms* terms, float* diag_dev, int32_t* update_state_dev, void* stream) {
    if (!terms) return fail(SO100_E_INVALID, "so100_learner_minibatch_step_ex: null argument");
    return minibatch_step(L, io, terms, diag_dev, update_state_dev, stream, "so100_learner_minibatch_step_ex");
}

int so100_learner_explained_variance(so100_learner* L, const float* rollout_dev, const float* ret_dev, int64_t num_samples, float* out_dev, void* stream) {
    if (!L) return fail(SO100_E_INVALID, "so100_learner_explained_variance: null argument");
    if (num_samples < 1) return fail(SO100_E_INVALID, "so100_learner_explained_variance: num_samples must be >= 1, got %ld", (long)num_samples);
    if (num_samples > (1L << 24))                                           // the row counts are carried as floats: exact up to 2^24
        return fail(SO100_E_INVALID, "so100_learner_explained_variance: num_samples must be <= 16777216, got %ld", (long)num_samples);
    if (!rollout_dev || !ret_dev || !out_dev) return fail(SO100_E_INVALID, "so100_learner_explained_variance: rollout/ret/out pointers are required");
    SO100_ON_DEVICE(L->cfg.device, "so100_learner_explained_variance");
    const int od = L->cfg.obs_dim;
    const long n = (long)num_samples, want = (n + ADV_THREADS - 1)/ADV_THREADS, G0 = want < EV_GRID_MAX ? want : EV_GRID_MAX;
    const long per = (n + G0 - 1)/G0;
    const int G = (int)((n + per - 1)/per);                                  // every workgroup owns at least one row
    hipLaunchKernelGGL(so100_learn_ev_moments, dim3((unsigned)G), dim3(ADV_THREADS), 0, (hipStream_t)stream, rollout_dev, od + ROW_EXTRA, od + ROW_VALUE, ret_dev,
                       n, per, L->ev_part);
    hipLaunchKernelGGL(so100_learn_ev_merge, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)L->ev_part, G, out_dev);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH, "so100_learner_explained_variance: ");
    return 0;
}

int so100_learner_shuffle(so100_learner* L, uint64_t seed, uint32_t epoch, int64_t n, int64_t* perm_dev, void* stream) {
    if (!L) return fail(SO100_E_INVALID, "so100_learner_shuffle: null argument");
    if (n < 1 || n > SHUFFLE_MAX_N) return fail(SO100_E_INVALID, "so100_learner_shuffle: n must be in 1..1073741824, got %ld", (long)n);
    if (!perm_dev) return fail(SO100_E_INVALID, "so100_learner_shuffle: the perm pointer is required");
    SO100_ON_DEVICE(L->cfg.device, "so100_learner_shuffle");
    const long want = ((long)n + 255)/256;
    hipLaunchKernelGGL(so100_learn_shuffle, dim3((unsigned)(want < SHUFFLE_GRID_MAX ? want : SHUFFLE_GRID_MAX)), dim3(256), 0, (hipStream_t)stream,
                       (uint32_t)n, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, perm_dev);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH, "so100_learner_shuffle: ");
    return 0;
}

}  // extern "C"

// so100_learner_update (nio null) and so100_learner_update_r
static int update(so100_learner* L, const so100_update_io* io, const so100_reward_norm_io* nio, void* stream, const char* fn) {
    if (!L || !io) return fail(SO100_E_INVALID, "%s: null argument", fn);
    if (io->T < 1) return fail(SO100_E_INVALID, "%s: T must be >= 1, got %d", fn, io->T);
    if (io->N < 1) return fail(SO100_E_INVALID, "%s: N must be >= 1, got %d", fn, io->N);
    if (io->epochs < 1) return fail(SO100_E_INVALID, "%s: epochs must be >= 1, got %d", fn, io->epochs);
    if (io->mb < 1 || io->mb > L->cfg.max_minibatch) return fail(SO100_E_INVALID, "%s: mb must be in 1..max_minibatch, got %d", fn, io->mb);
    if (io->adam_step0 < 0) return fail(SO100_E_INVALID, "%s: adam_step0 must be >= 0, got %d", fn, io->adam_step0);
    const long n = (long)io->T*(long)io->N;
    if (n > (1L << 24)) return fail(SO100_E_INVALID, "%s: T*N must be <= 16777216, got %ld", fn, n);          // the explained variance's limit
    const long per_epoch = (n + io->mb - 1)/io->mb, steps = per_epoch*(long)io->epochs;
    if ((long)io->adam_step0 + steps > 0x7fffffffL) return fail(SO100_E_INVALID, "%s: adam_step0 + epochs*ceil(T*N/mb) must fit 31 bits", fn);
    if (!io->rollout_dev || !io->last_obs_dev || !io->params_dev || !io->adam_m_dev || !io->adam_v_dev || !io->adv_dev || !io->ret_dev || !io->adv_stats_dev ||
        !io->perm_dev || !io->out_dev)
        return fail(SO100_E_INVALID, "%s: rollout/last_obs/params/adam_m/adam_v/adv/ret/adv_stats/perm/out pointers are required", fn);
    if (io->terms) {
        const int rc = check_terms(io->terms, io->update_state_dev, fn);
        if (rc != 0) return rc;
    }
    if (nio) {
        const int rc = check_reward_norm(nio, io->T, io->N, fn);
        if (rc != 0) return rc;
        if (nio->rollout_dev != io->rollout_dev) return fail(SO100_E_INVALID, "%s: the reward normalisation reads another chunk than the update", fn);
    }
    SO100_ON_DEVICE(L->cfg.device, fn);
    const hipStream_t st = (hipStream_t)stream;
    int rc;
    if (nio) enqueue_reward_norm(L, nio, io->T, io->N, st);
    so100_advantages_io aio = { io->rollout_dev, io->terminal_obs_chunk_dev, io->last_obs_dev, io->params_dev, io->adv_dev, io->ret_dev, io->adv_stats_dev };
    if ((rc = advantages(L, &aio, nio ? nio->reward_dev : nullptr, io->T, io->N, stream, fn)) != 0) return rc;
    if ((rc = so100_learner_explained_variance(L, io->rollout_dev, io->ret_dev, n, io->out_dev + 8, stream)) != 0) return rc;
    if (io->update_state_dev) hipLaunchKernelGGL(so100_learn_zero_state, dim3(1), dim3(64), 0, st, io->update_state_dev);
    so100_minibatch_io mio;
    mio.rollout_dev = io->rollout_dev; mio.num_samples = n; mio.adv_dev = io->adv_dev; mio.ret_dev = io->ret_dev; mio.adv_stats_dev = io->adv_stats_dev;
    mio.params_dev = io->params_dev; mio.adam_m_dev = io->adam_m_dev; mio.adam_v_dev = io->adam_v_dev; mio.stats_dev = io->out_dev; mio.grads_dev = nullptr;
    const float* log_std = io->params_dev + tensor_offset(T_log_std, L->cfg.obs_dim);
    int step = io->adam_step0;
    const int last = io->adam_step0 + (int)steps;
    for (int e = 0; e < io->epochs; e++) {
        if ((rc = so100_learner_shuffle(L, io->shuffle_seed, io->shuffle_epoch0 + (uint32_t)e, n, io->perm_dev, stream)) != 0) return rc;
        for (long k = 0; k < per_epoch; k++) {
            const long left = n - k*io->mb;
            mio.idx_dev = io->perm_dev + k*io->mb; mio.mb = (int32_t)(left < io->mb ? left : io->mb); mio.adam_step = ++step;
            if (step == last) hipLaunchKernelGGL(so100_learn_copy_log_std, dim3(1), dim3(64), 0, st, log_std, io->out_dev + 9);
            if ((rc = minibatch_step(L, &mio, io->terms, io->out_dev, io->update_state_dev, stream, fn)) != 0) return rc;
        }
    }
    return 0;
}

extern "C" {

int so100_learner_update(so100_learner* L, const so100_update_io* io, void* stream) { return update(L, io, nullptr, stream, "so100_learner_update"); }

int so100_learner_update_r(so100_learner* L, const so100_update_io* io, const so100_reward_norm_io* norm_io, void* stream) {
    return update(L, io, norm_io, stream, "so100_learner_update_r");
}

int64_t so100_learner_reward_norm_workspace(int32_t T, int32_t N) {
    if (T < 1 || N < 1) return (int64_t)fail(SO100_E_INVALID, "so100_learner_reward_norm_workspace: T and N must be >= 1, got %d and %d", T, N);
    return (int64_t)(rn_workspace_doubles(T, N)*(long)sizeof(double));
}

int so100_learner_reward_norm_init(so100_learner* L, double* state_dev, int32_t N, void* stream) {
    const char* const fn = "so100_learner_reward_norm_init";
    if (!L) return fail(SO100_E_INVALID, "%s: null argument", fn);
    if (N < 1) return fail(SO100_E_INVALID, "%s: N must be >= 1, got %d", fn, N);
    if (!state_dev) return fail(SO100_E_INVALID, "%s: the state pointer is required", fn);
    SO100_ON_DEVICE(L->cfg.device, fn);
    const long len = 3 + (long)N, want = (len + 255)/256;
    hipLaunchKernelGGL(so100_learn_rn_init, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, (hipStream_t)stream, state_dev, len);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH, "so100_learner_reward_norm_init: ");
    return 0;
}

int so100_learner_normalize_rewards(so100_learner* L, const so100_reward_norm_io* io, int32_t T, int32_t N, void* stream) {
    const char* const fn = "so100_learner_normalize_rewards";
    if (!L || !io) return fail(SO100_E_INVALID, "%s: null argument", fn);
    const int rc = check_reward_norm(io, T, N, fn);
    if (rc != 0) return rc;
    SO100_ON_DEVICE(L->cfg.device, fn);
    enqueue_reward_norm(L, io, T, N, (hipStream_t)stream);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH, "so100_learner_normalize_rewards: ");
    return 0;
}

int so100_learner_obs_norm_init(so100_learner* L, double* state_dev, void* stream) {
    const char* const fn = "so100_learner_obs_norm_init";
    if (!L) return fail(SO100_E_INVALID, "%s: null argument", fn);
    if (!state_dev) return fail(SO100_E_INVALID, "%s: the state pointer is required", fn);
    SO100_ON_DEVICE(L->cfg.device, fn);
    hipLaunchKernelGGL(so100_learn_on_init, dim3(1), dim3(64), 0, (hipStream_t)stream, state_dev, L->cfg.obs_dim);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH, "so100_learner_obs_norm_init: ");
    return 0;
}

int64_t so100_learner_obs_norm_workspace(int32_t T, int32_t N) {
    if (T < 1 || N < 1) return (int64_t)fail(SO100_E_INVALID, "so100_learner_obs_norm_workspace: T and N must be >= 1, got %d and %d", T, N);
    if ((long)T*(long)N > ON_MAX_ROWS) return (int64_t)fail(SO100_E_INVALID, "so100_learner_obs_norm_workspace: T*N must be <= 16777216, got %ld", (long)T*(long)N);
    return (int64_t)(on_workspace_doubles((long)T*(long)N)*(long)sizeof(double));
}

int so100_learner_obs_norm_update(so100_learner* L, const so100_obs_norm_io* io, int32_t T, int32_t N, void* stream) {
    const char* const fn = "so100_learner_obs_norm_update";
    if (!L || !io) return fail(SO100_E_INVALID, "%s: null argument", fn);
    if (T < 1) return fail(SO100_E_INVALID, "%s: T must be >= 1, got %d", fn, T);
    if (N < 1) return fail(SO100_E_INVALID, "%s: N must be >= 1, got %d", fn, N);
    const long rows = (long)T*(long)N;
    if (rows > ON_MAX_ROWS) return fail(SO100_E_INVALID, "%s: T*N must be <= 16777216, got %ld", fn, rows);
    if (!io->rollout_dev || !io->state_dev || !io->workspace_dev) return fail(SO100_E_INVALID, "%s: rollout/state/workspace pointers are required", fn);
    const long need = on_workspace_doubles(rows)*(long)sizeof(double);
    if (io->workspace_bytes < need) return fail(SO100_E_INVALID, "%s: the workspace holds %ld bytes, T = %d and N = %d need %ld", fn, (long)io->workspace_bytes, T, N, need);
    if (((uintptr_t)io->workspace_dev & 7u) != 0) return fail(SO100_E_INVALID, "%s: the workspace must be 8-byte aligned", fn);
    SO100_ON_DEVICE(L->cfg.device, fn);
    const hipStream_t st = (hipStream_t)stream;
    const int od = L->cfg.obs_dim;
    const long B = on_blocks(rows);
    double* part = (double*)io->workspace_dev;
    double* grp = part + (size_t)B*od*2;
    SO100_WITH_OBS_DIM(od, hipLaunchKernelGGL((so100_learn_on_moments<OD>), dim3((unsigned)B), dim3(ON_BLOCK), 0, st, io->rollout_dev, rows, part););
    hipLaunchKernelGGL(so100_learn_on_merge, dim3(1), dim3(ON_MERGE_THREADS), 0, st, (const double*)part, grp, od, rows, io->state_dev);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH, "so100_learner_obs_norm_update: ");
    return 0;
}

int so100_learner_obs_norm_fold(so100_learner* L, const double* state_dev, double epsilon, const float* params_dev, float* folded_params_dev, float* norm_dev,
                                void* stream) {
    const char* const fn = "so100_learner_obs_norm_fold";
    if (!L) return fail(SO100_E_INVALID, "%s: null argument", fn);
    if (!state_dev || !params_dev || !folded_params_dev || !norm_dev) return fail(SO100_E_INVALID, "%s: state/params/folded_params/norm pointers are required", fn);
    if (!(epsilon >= 0.0)) return fail(SO100_E_INVALID, "%s: epsilon must be >= 0", fn);
    if (folded_params_dev == params_dev) return fail(SO100_E_INVALID, "%s: the folded block must not be the plain block", fn);
    SO100_ON_DEVICE(L->cfg.device, fn);
    const int od = L->cfg.obs_dim;
    FoldArgs a;
    a.od = od; a.P = L->P;
    a.oW0[0] = tensor_offset(T_pi_w0, od); a.oB0[0] = tensor_offset(T_pi_b0, od); a.oW0[1] = tensor_offset(T_vf_w0, od); a.oB0[1] = tensor_offset(T_vf_b0, od);
    hipLaunchKernelGGL(so100_learn_on_fold, dim3((unsigned)((L->P + 255)/256)), dim3(256), 0, (hipStream_t)stream, state_dev, epsilon, params_dev, folded_params_dev, norm_dev, a);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH, "so100_learner_obs_norm_fold: ");
    return 0;
}

int so100_learner_set_obs_norm(so100_learner* L, const float* norm_dev) {
    if (!L) return fail(SO100_E_INVALID, "so100_learner_set_obs_norm: null argument");
    L->obs_norm = norm_dev;
    return 0;
}

}  // extern "C"
