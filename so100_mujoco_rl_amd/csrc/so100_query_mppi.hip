// so100_query_mppi.hip -- the two sampling-planner queries (gfx950) and their C ABI (include/so100_query.h: so100_query_plan_sample,
// so100_query_cost_blend); every number's arithmetic is in so100_mppi.hpp.  Like so100_query_cost.hip, not a translation unit of its own:
// so100_sim.hip includes it behind that file and it uses its cost_def(), cost_rollouts() and cost_rollout(), and the checks of the files before.
//
// Sample.  One lane per candidate column c = n K + k, walking t: two Philox blocks and four Box-Muller pairs per (column, step), six stores.  The
// lanes of a wave are consecutive k of a problem (or of two, at a problem's end), so each store of a wave is one contiguous segment of an SoA row
// and each plan entry is read by all of them at one address.  The start states' fan-out is 25 more stores per lane in the same launch.  No LDS.
//
// Blend.  One workgroup per problem; its K costs and then its K weights live in K floats of LDS (dynamic: 16 KB at K = 4096, 256 B at K = 64).
//   1. thread i sums the cost of rollouts i, i + B, ... (B: the workgroup's threads): cost_select's loop, loads coalesced over k
//   2. every wave scans the K costs for (J_min, best) -- lane l takes k = l, l + 64, ..., then six lane exchanges under the total order of
//      mppi_min_take -- so every thread holds them without another barrier
//   3. e_k over the threads; sum e in the ONE summation order of so100_mppi.hpp, by every wave alike; w_k = e_k / sum e over the threads
//   4. wave 0: sum w^2 and ess; the 6 T rows of the blend dealt over the waves, row r to wave r mod (B / 64): lanes stride over k (coalesced
//      loads of u_traj, the weights from LDS), then the exchange tree; lane 0 stores the row where the shift puts it
// No sum depends on B, so the bits do not either.  B = 256 at every K: at K <= 64 three of the four waves have no rollout to sum, but the 6 T rows
// of step 4 are a chain of load, tree and store per row, and four waves walk four such chains at once -- launched with B = 64 the same kernel took
// 41 us where this takes 22 (N = 8, K = 64, T = 8).  No atomics, no order that depends on timing.
#include "so100_mppi.hpp"

namespace so100 {

constexpr int MPPI_SAMPLE_WG = 256, MPPI_BLEND_WG = 256;

struct PlanSampleArgs {
    const float* plan; float sigma[6], lo, hi;
    int K, T;
    uint32_t seed_lo, seed_hi, draw, id_offset;
    const uint32_t *qpos, *qvel;                             // the fan-out copies words
    float* ctrl; uint32_t *qpos_rep, *qvel_rep;
};
struct CostBlendArgs {
    CostRollouts in;
    float lambda; int shift, tail;
    float* cost; int32_t* best; float *best_cost, *weight, *ess, *u_plan, *u_first;
};

// one candidate column: its T x 6 entries and its fan-out rows.  A: PlanSampleArgs, or the per-entry-sigma form of so100_query_cem.hip with the same
// fields; entry(row, j, n, p, eps, perturbed): the candidate's value from the plan entry p
template <typename A, typename Entry> __device__ __forceinline__ void plan_sample_column(const A& a, int N, Entry&& entry) {
    const size_t Nz = (size_t)N, NK = Nz*(size_t)a.K, col = (size_t)blockIdx.x*MPPI_SAMPLE_WG + threadIdx.x;
    if (col >= NK) return;
    const uint32_t n = (uint32_t)col/(uint32_t)a.K, k = (uint32_t)col - n*(uint32_t)a.K;      // N K <= INT32_MAX
    if (a.ctrl) {
        for (int t = 0; t < a.T; t++) {
            float eps[8];
            mppi_noise<float>(a.id_offset + n, a.draw, k, t, a.seed_lo, a.seed_hi, eps);
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const size_t row = (size_t)t*6 + j;
                a.ctrl[row*NK + col] = entry(row, j, n, a.plan[row*Nz + n], eps[j], k > 0);
            }
        }
    }
    if (a.qpos_rep) {
#pragma unroll
        for (int r = 0; r < 13; r++) a.qpos_rep[(size_t)r*NK + col] = a.qpos[(size_t)r*Nz + n];
    }
    if (a.qvel_rep) {
#pragma unroll
        for (int r = 0; r < 12; r++) a.qvel_rep[(size_t)r*NK + col] = a.qvel[(size_t)r*Nz + n];
    }
}

__global__ void __launch_bounds__(MPPI_SAMPLE_WG) so100_query_plan_sample_k(PlanSampleArgs a, int N) {
    plan_sample_column(a, N, [&](size_t, int j, uint32_t, float p, float eps, bool perturbed) { return mppi_candidate<float>(p, a.sigma[j], eps, perturbed, a.lo, a.hi); });
}

// the exchange tree of so100_mppi.hpp's summation order over the wave's 64 partial sums: every lane takes part and ends with the same bits
__device__ __forceinline__ float mppi_wave_sum(float x) {
#pragma unroll
    for (int d = MPPI_WAVE/2; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

__global__ void __launch_bounds__(MPPI_BLEND_WG) so100_query_cost_blend_k(CostBlendArgs a, int N) {
    extern __shared__ float w[];                             // K floats: the costs, then e, then the weights
    const int tid = (int)threadIdx.x, threads = (int)blockDim.x, lane = tid & (MPPI_WAVE - 1), wave = tid/MPPI_WAVE, waves = threads/MPPI_WAVE, K = a.in.K;
    const size_t Nz = (size_t)N, NK = Nz*(size_t)K, n = (size_t)blockIdx.x, base = n*(size_t)K;
    const float inf = __int_as_float(0x7F800000), nan = __int_as_float(0x7FC00000);
    for (int k = tid; k < K; k += threads) {
        const size_t col = base + (size_t)k;
        const float cost = cost_rollout(a.in, Nz, NK, n, col);
        if (a.cost) a.cost[col] = cost;
        w[k] = cost;
    }
    const bool weights = a.weight || a.ess || a.u_plan || a.u_first;
    if (!weights && !a.best && !a.best_cost) return;         // every exit before a barrier depends on the arguments alone: the whole workgroup takes it
    __syncthreads();
    float j_min; int arg;
    mppi_lane_min<float>(K, lane, MPPI_WAVE, inf, [&](int k) { return w[k]; }, j_min, arg);
#pragma unroll
    for (int d = MPPI_WAVE/2; d >= 1; d >>= 1) {
        const float c2 = __shfl_xor(j_min, d); const int i2 = __shfl_xor(arg, d);
        mppi_min_take<float>(j_min, arg, c2, i2);
    }
    const int best = arg == MPPI_NONE ? -1 : arg;
    if (tid == 0) {
        if (a.best) a.best[n] = best;
        if (a.best_cost) a.best_cost[n] = j_min;
    }
    if (!weights) return;
    __syncthreads();                                         // every wave has read the costs
    for (int k = tid; k < K; k += threads) w[k] = mppi_unnormalised<float>(w[k], j_min, a.lambda, inf);
    __syncthreads();
    const float sum_e = mppi_wave_sum(mppi_lane_sum<float>(K, lane, [&](int k) { return w[k]; }));
    __syncthreads();                                         // every wave has read e
    for (int k = tid; k < K; k += threads) {
        const float wk = best >= 0 ? w[k]/sum_e : 0.0f;
        w[k] = wk;
        if (a.weight) a.weight[base + (size_t)k] = wk;
    }
    __syncthreads();
    if (a.ess && wave == 0) {
        const float s2 = mppi_wave_sum(mppi_lane_sum<float>(K, lane, [&](int k) { return trajectory_rounded(w[k]*w[k]); }));
        if (lane == 0) a.ess[n] = best >= 0 ? 1.0f/s2 : 0.0f;
    }
    if (!a.u_plan && !a.u_first) return;
    for (int r = wave; r < a.in.T*COST_NU; r += waves) {      // row r = (t, j); r and best are the same in every lane of the wave
        const int t = r/COST_NU, j = r - t*COST_NU;
        float x;
        if (best >= 0) {
            const float* u = a.in.u + (size_t)r*NK + base;
            x = mppi_wave_sum(mppi_lane_sum<float>(K, lane, [&](int k) { return mppi_term<float>(w[k], u[k]); }));
        } else {
            x = a.in.u_fallback ? a.in.u_fallback[(size_t)r*Nz + n] : nan;
        }
        if (lane == 0)
            mppi_place<float>(t, a.in.T, a.shift, a.tail, x,
                              [&](int row, float y) { if (a.u_plan) a.u_plan[((size_t)row*COST_NU + j)*Nz + n] = y; },
                              [&](float y) { if (a.u_first) a.u_first[(size_t)j*Nz + n] = y; });
    }
}

}  // namespace so100

namespace so100 {
namespace {

// where a refreshed plan goes: the blend's and the refit's
int plan_placement(const char* fn, int32_t shift, int32_t tail) {
    if (shift != 0 && shift != 1) return fail(SO100_E_INVALID, "%s: shift must be 0 or 1, got %ld", fn, (long)shift);
    if (tail != SO100_BLEND_TAIL_ZERO && tail != SO100_BLEND_TAIL_HOLD) return fail(SO100_E_INVALID, "%s: unknown tail %ld", fn, (long)tail);
    return 0;
}

// a sampler's entry: Args is its kernel's argument struct; sigma(a) checks the io struct's sigma and puts it into a, where the two samplers differ
template <typename Args, typename IO, typename Sigma>
int plan_sample_entry(const char* fn, void (*kernel)(Args, int), so100_sim* sim, const IO* io, int32_t N, void* stream, Sigma&& sigma) {
    if (!sim || !io) return fail(SO100_E_INVALID, "%s: null argument", fn);
    if (const int rc = query_batch(fn, sim, false, N)) return rc;                 // no state is read: any N >= 1
    if (const int rc = query_steps(fn, io->T, SO100_TRAJ_MAX_T)) return rc;
    if (const int rc = query_candidates(fn, "K", "N", io->K, SO100_MPPI_MAX_K, N)) return rc;
    Args a{};
    if (const int rc = sigma(a)) return rc;
    const auto finite = [](float x) { return x*0.0f == 0.0f; };
    if (!finite(io->u_lo) || !finite(io->u_hi) || io->u_lo > io->u_hi) return fail(SO100_E_INVALID, "%s: u_lo and u_hi must be finite and u_lo <= u_hi", fn);
    if (!io->plan_dev) return fail(SO100_E_INVALID, "%s: plan_dev is required", fn);
    if (io->qvel_dev && !io->qpos_dev) return fail(SO100_E_INVALID, "%s: qvel_dev needs qpos_dev", fn);
    if ((io->qpos_rep_dev && !io->qpos_dev) || (io->qvel_rep_dev && !io->qvel_dev))
        return fail(SO100_E_INVALID, "%s: qpos_rep_dev needs qpos_dev and qvel_rep_dev needs qvel_dev", fn);
    if (!io->ctrl_dev && !io->qpos_rep_dev && !io->qvel_rep_dev) return fail(SO100_E_INVALID, "%s: no output requested", fn);
    a.plan = io->plan_dev; a.lo = io->u_lo; a.hi = io->u_hi; a.K = io->K; a.T = io->T;
    a.seed_lo = (uint32_t)(io->seed & 0xffffffffu); a.seed_hi = (uint32_t)(io->seed >> 32); a.draw = io->draw; a.id_offset = io->id_offset;
    a.qpos = reinterpret_cast<const uint32_t*>(io->qpos_dev); a.qvel = reinterpret_cast<const uint32_t*>(io->qvel_dev);
    a.ctrl = io->ctrl_dev; a.qpos_rep = reinterpret_cast<uint32_t*>(io->qpos_rep_dev); a.qvel_rep = reinterpret_cast<uint32_t*>(io->qvel_rep_dev);
    SO100_ON_DEVICE(sim->cfg.device, fn);
    const size_t cols = (size_t)N*(size_t)io->K;
    const dim3 grid((unsigned)((cols + MPPI_SAMPLE_WG - 1)/MPPI_SAMPLE_WG)), block(MPPI_SAMPLE_WG);
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, a, N);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // namespace
}  // namespace so100

static_assert(SO100_MPPI_MAX_K == so100::MPPI_MAX_K && SO100_BLEND_TAIL_ZERO == so100::BLEND_TAIL_ZERO && SO100_BLEND_TAIL_HOLD == so100::BLEND_TAIL_HOLD &&
              SO100_TRAJ_MAX_T <= 4096 && so100::MPPI_BLEND_WG % so100::MPPI_WAVE == 0,
              "the header names the limits and the tails; t << 1 | b stays under 2^13 in the counter's last word");

extern "C" {

int so100_query_plan_sample(so100_sim* sim, const so100_plan_sample_io* io, int32_t N, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_plan_sample";
    return plan_sample_entry(fn, so100_query_plan_sample_k, sim, io, N, stream, [&](PlanSampleArgs& a) {
        for (int j = 0; j < 6; j++) {
            if (!(io->sigma[j]*0.0f == 0.0f) || io->sigma[j] < 0.0f) return fail(SO100_E_INVALID, "%s: sigma must be finite and >= 0", fn);
            a.sigma[j] = io->sigma[j];
        }
        return 0;
    });
}

int so100_query_cost_blend(so100_sim* sim, const so100_cost_blend_io* io, int32_t N, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_cost_blend";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_cost_blend: null argument");
    if (const int rc = query_batch(fn, sim, false, N)) return rc;
    if (const int rc = query_steps(fn, io->T, SO100_TRAJ_MAX_T)) return rc;
    if (const int rc = query_candidates(fn, "K", "N", io->K, SO100_MPPI_MAX_K, N)) return rc;
    CostBlendArgs a{};
    if (const int rc = cost_def(fn, io->cost, a.in.c)) return rc;
    if (!(io->temperature*0.0f == 0.0f) || !(io->temperature > 0.0f)) return fail(SO100_E_INVALID, "%s: temperature must be finite and > 0", fn);
    if (const int rc = plan_placement(fn, io->shift, io->tail)) return rc;
    if (const int rc = cost_rollouts(fn, *io, io->K, COST_ROLLOUTS_REQUIRED, false, a.in)) return rc;
    if (!io->cost_dev && !io->best_dev && !io->best_cost_dev && !io->weight_dev && !io->ess_dev && !io->u_plan_dev && !io->u_first_dev)
        return fail(SO100_E_INVALID, "%s: no output requested", fn);
    a.lambda = io->temperature; a.shift = io->shift; a.tail = io->tail;
    a.cost = io->cost_dev; a.best = io->best_dev; a.best_cost = io->best_cost_dev; a.weight = io->weight_dev; a.ess = io->ess_dev;
    a.u_plan = io->u_plan_dev; a.u_first = io->u_first_dev;
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_cost_blend");
    const dim3 grid((unsigned)N), block(MPPI_BLEND_WG);
    hipLaunchKernelGGL(so100_query_cost_blend_k, grid, block, (size_t)io->K*sizeof(float), (hipStream_t)stream, a, N);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
