// so100_query_cem.hip -- the two cross-entropy planner queries (gfx950) and their C ABI (include/so100_query.h: so100_query_plan_sample_tv,
// so100_query_cost_refit); every number's arithmetic is in so100_cem.hpp.  Like so100_query_mppi.hip, not a translation unit of its own:
// so100_sim.hip includes it behind that file and it uses its plan_sample_column(), plan_sample_entry(), plan_placement() and mppi_wave_sum(), and
// cost_rollout(), cost_def(), cost_rollouts() and the checks of the files before.
//
// Sample.  so100_query_mppi.hip's column body with the entry's sigma loaded from sigma[t][j][n]: all lanes of a problem read one address, as they
// do for the plan.  No LDS.
//
// Refit.  One workgroup of four waves per problem.  LDS (dynamic): P 64-bit keys, P = K rounded up to a power of two and at least 64, then K floats
// -- 48 KB at K = 4096, 768 B at K = 64.
//   1. thread i sums the cost of rollouts i, i + 256, ... with the blend's code (cost_rollout) into the K floats; key (J_k, k) into the table,
//      a padding key above every cost behind them
//   2. a bitonic sort of the keys, ascending.  The steps at distances 32 .. 1 work on 64 consecutive keys: a wave holds them one per lane and
//      exchanges them across lanes, no LDS traffic and no barrier between such steps (all 21 steps up to runs of 64; the last six of every
//      longer run).  A chain of such steps is one exchange after another, so a wave walks four of its chunks at once where it has four: with one
//      at a time the sort of 4096 keys took 69 us, the chains' latency.  The steps at distances >= 64 go through LDS, thread p on keys (i, i + d) with consecutive p on consecutive i: 8-byte
//      accesses at unit stride, no bank conflict.  (log2 P)(log2 P + 1)/2 steps: 78 at K = 4096, 57 of them in registers, 29 barriers up to the sorted table
//   3. the keys are unique, so the table is the one order of so100_cem.hpp: n_elite by a count over the first E (every wave alike), best,
//      threshold and the elite list straight from it; then every key's place r < n_elite is written to its candidate's float as the elite flag
//   4. the 6 T rows dealt over the waves as in the blend, row r to wave r mod 4: two passes over the elites' controls in the ONE summation order
//      (lanes stride over k, then the exchange tree), the smoothing, and lane 0 stores mean, sigma_out and u_first where the shift puts them
// Every exit before a barrier depends on the arguments alone.  No atomics, no order that depends on timing, no private arrays.
#include "so100_cem.hpp"

namespace so100 {

constexpr int CEM_REFIT_WG = 256;

struct PlanSampleTvArgs {
    const float *plan, *sigma; float lo, hi;
    int K, T;
    uint32_t seed_lo, seed_hi, draw, id_offset;
    const uint32_t *qpos, *qvel;
    float* ctrl; uint32_t *qpos_rep, *qvel_rep;
};
struct CostRefitArgs {
    CostRollouts in;
    int E, P;
    float alpha; const float *plan, *sigma;
    float sigma_min[6], sigma_max[6], sigma_init[6];
    int shift, tail;
    float* cost; int32_t* best; float* best_cost; int32_t *elite, *n_elite; float *threshold, *mean, *sigma_out, *u_first;
};

__global__ void __launch_bounds__(MPPI_SAMPLE_WG) so100_query_plan_sample_tv_k(PlanSampleTvArgs a, int N) {
    const size_t Nz = (size_t)N;
    plan_sample_column(a, N, [&](size_t row, int, uint32_t n, float p, float eps, bool perturbed) {
        return cem_candidate<float>(p, a.sigma[row*Nz + n], eps, perturbed, a.lo, a.hi);
    });
}

__device__ __forceinline__ uint64_t cem_lane_exchange(uint64_t x, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
// the steps at distances D_MAX .. 1 of the run length `size` on the U elements i0 + u stride a lane holds, one chunk of 64 per u: the lower of a
// pair keeps the smaller key where the run ascends ((i & size) == 0), the larger where it descends.  The U chains are independent: their
// exchanges overlap
template <int D_MAX, int U> __device__ __forceinline__ void cem_wave_steps(uint64_t (&x)[U], int i0, int stride, int size) {
#pragma unroll
    for (int d = D_MAX; d >= 1; d >>= 1) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = i0 + u*stride;
            const uint64_t y = cem_lane_exchange(x[u], d);
            const bool smaller = ((i & size) == 0) == ((i & d) == 0);
            x[u] = (smaller == (x[u] < y)) ? x[u] : y;
        }
    }
}
// a wave's chunks i = first, first + stride, ... < P through steps(x, i0), four chunks in flight where it has that many; x lives in registers (every
// index is a constant once unrolled)
template <int U, typename Steps> __device__ __forceinline__ void cem_chunk_group(uint64_t* key, int i0, int stride, Steps&& steps) {
    uint64_t x[U];
#pragma unroll
    for (int u = 0; u < U; u++) x[u] = key[i0 + u*stride];
    steps(x, i0);
#pragma unroll
    for (int u = 0; u < U; u++) key[i0 + u*stride] = x[u];
}
template <typename Steps> __device__ __forceinline__ void cem_register_phase(uint64_t* key, int P, int first, int stride, Steps&& steps) {
    int i = first;
    for (; i + 3*stride < P; i += 4*stride) cem_chunk_group<4>(key, i, stride, steps);
    for (; i < P; i += stride) cem_chunk_group<1>(key, i, stride, steps);
}

__global__ void __launch_bounds__(CEM_REFIT_WG) so100_query_cost_refit_k(CostRefitArgs a, int N) {
    extern __shared__ unsigned long long cem_lds[];              // P keys, then K floats: the costs, then the elite flags
    uint64_t* key = reinterpret_cast<uint64_t*>(cem_lds);
    float* w = reinterpret_cast<float*>(cem_lds + a.P);
    const int tid = (int)threadIdx.x, threads = (int)blockDim.x, lane = tid & (MPPI_WAVE - 1), wave = tid/MPPI_WAVE, waves = threads/MPPI_WAVE, K = a.in.K, P = a.P;
    const size_t Nz = (size_t)N, NK = Nz*(size_t)K, n = (size_t)blockIdx.x, base = n*(size_t)K;
    const float inf = __int_as_float(0x7F800000), nan = __int_as_float(0x7FC00000);
    for (int k = tid; k < K; k += threads) {
        const size_t col = base + (size_t)k;
        const float cost = cost_rollout(a.in, Nz, NK, n, col);
        if (a.cost) a.cost[col] = cost;
        w[k] = cost;
        key[k] = cem_key(cost, k);
    }
    const bool refit = a.mean || a.sigma_out || a.u_first;
    if (!refit && !a.best && !a.best_cost && !a.elite && !a.n_elite && !a.threshold) return;      // the arguments alone: the whole workgroup takes it
    for (int i = K + tid; i < P; i += threads) key[i] = cem_key_pad(i);
    __syncthreads();
    // ---- the sort ----
    cem_register_phase(key, P, tid, threads, [&](auto& x, int i0) {     // runs of 2 .. 64 inside each 64 keys
        cem_wave_steps<1>(x, i0, threads, 2); cem_wave_steps<2>(x, i0, threads, 4); cem_wave_steps<4>(x, i0, threads, 8);
        cem_wave_steps<8>(x, i0, threads, 16); cem_wave_steps<16>(x, i0, threads, 32); cem_wave_steps<32>(x, i0, threads, 64);
    });
    __syncthreads();
    for (int size = 2*MPPI_WAVE; size <= P; size <<= 1) {
        for (int d = size/2; d >= MPPI_WAVE; d >>= 1) {
            for (int p = tid; p < P/2; p += threads) {
                const int i = ((p & ~(d - 1)) << 1) | (p & (d - 1));
                const uint64_t x = key[i], y = key[i + d];
                if ((x > y) == ((i & size) == 0)) { key[i] = y; key[i + d] = x; }
            }
            __syncthreads();
        }
        cem_register_phase(key, P, tid, threads, [&](auto& x, int i0) { cem_wave_steps<32>(x, i0, threads, size); });
        __syncthreads();
    }
    // ---- the elites: the first n_elite keys ----
    const uint32_t image_inf = (uint32_t)(cem_key(inf, 0) >> 32);
    int n_elite = 0;
    for (int r = lane; r < a.E; r += MPPI_WAVE) n_elite += (uint32_t)(key[r] >> 32) < image_inf;
#pragma unroll
    for (int d = MPPI_WAVE/2; d >= 1; d >>= 1) n_elite += __shfl_xor(n_elite, d);
    if (tid == 0) {
        const int first = cem_key_index(key[0]);
        if (a.best) a.best[n] = n_elite > 0 ? first : -1;
        if (a.best_cost) a.best_cost[n] = w[first];
        if (a.n_elite) a.n_elite[n] = n_elite;
        if (a.threshold) a.threshold[n] = n_elite > 0 ? w[cem_key_index(key[n_elite - 1])] : inf;
    }
    if (a.elite)
        for (int r = tid; r < a.E; r += threads) a.elite[n*(size_t)a.E + (size_t)r] = r < n_elite ? cem_key_index(key[r]) : -1;
    if (!refit) return;
    __syncthreads();                                         // thread 0 has read the costs
    for (int r = tid; r < K; r += threads) w[cem_key_index(key[r])] = r < n_elite ? 1.0f : 0.0f;
    __syncthreads();
    // ---- the rows ----
    for (int r = wave; r < a.in.T*COST_NU; r += waves) {      // row r = (t, j); r and n_elite are the same in every lane of the wave
        const int t = r/COST_NU, j = r - t*COST_NU;
        float m, s;
        if (n_elite > 0) {
            const float* u = a.in.u + (size_t)r*NK + base;
            const float mu = cem_mean(mppi_wave_sum(mppi_lane_sum<float>(K, lane, [&](int k) { return cem_sum_term<float>(w[k] != 0.0f, u[k]); })), n_elite);
            const float sd = cem_sd(mppi_wave_sum(mppi_lane_sum<float>(K, lane, [&](int k) { return cem_dev_term<float>(w[k] != 0.0f, u[k], mu); })), n_elite);
            const bool old = a.alpha > 0.0f;
            m = cem_mix<float>(a.alpha, old ? a.plan[(size_t)r*Nz + n] : 0.0f, mu);
            s = cem_sigma<float>(a.alpha, old ? a.sigma[(size_t)r*Nz + n] : 0.0f, sd, a.sigma_min[j], a.sigma_max[j]);
        } else {
            m = a.in.u_fallback ? a.in.u_fallback[(size_t)r*Nz + n] : nan;
            s = a.sigma_init[j];
        }
        if (lane == 0) {
            mppi_place<float>(t, a.in.T, a.shift, a.tail, m,
                              [&](int row, float y) { if (a.mean) a.mean[((size_t)row*COST_NU + j)*Nz + n] = y; },
                              [&](float y) { if (a.u_first) a.u_first[(size_t)j*Nz + n] = y; });
            cem_place_sigma<float>(t, a.in.T, a.shift, s, a.sigma_init[j], [&](int row, float y) { if (a.sigma_out) a.sigma_out[((size_t)row*COST_NU + j)*Nz + n] = y; });
        }
    }
}

}  // namespace so100

static_assert(so100::CEM_REFIT_WG % so100::MPPI_WAVE == 0 && so100::CEM_REFIT_WG/so100::MPPI_WAVE == 4, "four waves per problem");

extern "C" {

int so100_query_plan_sample_tv(so100_sim* sim, const so100_plan_sample_tv_io* io, int32_t N, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_plan_sample_tv";
    return plan_sample_entry(fn, so100_query_plan_sample_tv_k, sim, io, N, stream, [&](PlanSampleTvArgs& a) {
        if (!io->sigma_dev) return fail(SO100_E_INVALID, "%s: sigma_dev is required", fn);
        a.sigma = io->sigma_dev;
        return 0;
    });
}

int so100_query_cost_refit(so100_sim* sim, const so100_cost_refit_io* io, int32_t N, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_cost_refit";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_cost_refit: null argument");
    if (const int rc = query_batch(fn, sim, false, N)) return rc;
    if (const int rc = query_steps(fn, io->T, SO100_TRAJ_MAX_T)) return rc;
    if (const int rc = query_candidates(fn, "K", "N", io->K, SO100_MPPI_MAX_K, N)) return rc;
    CostRefitArgs a{};
    if (const int rc = cost_def(fn, io->cost, a.in.c)) return rc;
    if (io->E < 1 || io->E > io->K) return fail(SO100_E_INVALID, "%s: E must be in 1..K, got E = %ld, K = %ld", fn, (long)io->E, (long)io->K);
    const auto finite = [](float x) { return x*0.0f == 0.0f; };
    if (!finite(io->alpha) || !(io->alpha >= 0.0f && io->alpha < 1.0f)) return fail(SO100_E_INVALID, "%s: alpha must be finite and in [0, 1)", fn);
    for (int j = 0; j < 6; j++)
        if (!finite(io->sigma_min[j]) || !finite(io->sigma_max[j]) || !finite(io->sigma_init[j]) || io->sigma_min[j] < 0.0f || io->sigma_min[j] > io->sigma_max[j] ||
            io->sigma_init[j] < 0.0f)
            return fail(SO100_E_INVALID, "%s: sigma_min, sigma_max and sigma_init must be finite, 0 <= sigma_min <= sigma_max and sigma_init >= 0", fn);
    if (const int rc = plan_placement(fn, io->shift, io->tail)) return rc;
    if (const int rc = cost_rollouts(fn, *io, io->K, "qpos_traj_dev, u_traj_dev, (unless the target is the cube) target_dev and (with alpha > 0) plan_dev and sigma_dev",
                                     io->alpha > 0.0f && (!io->plan_dev || !io->sigma_dev), a.in)) return rc;
    if (!io->cost_dev && !io->best_dev && !io->best_cost_dev && !io->elite_dev && !io->n_elite_dev && !io->threshold_dev && !io->mean_dev && !io->sigma_out_dev &&
        !io->u_first_dev)
        return fail(SO100_E_INVALID, "%s: no output requested", fn);
    a.E = io->E; a.alpha = io->alpha; a.plan = io->plan_dev; a.sigma = io->sigma_dev;
    for (int j = 0; j < 6; j++) { a.sigma_min[j] = io->sigma_min[j]; a.sigma_max[j] = io->sigma_max[j]; a.sigma_init[j] = io->sigma_init[j]; }
    a.shift = io->shift; a.tail = io->tail;
    a.P = MPPI_WAVE;
    while (a.P < io->K) a.P <<= 1;
    a.cost = io->cost_dev; a.best = io->best_dev; a.best_cost = io->best_cost_dev; a.elite = io->elite_dev; a.n_elite = io->n_elite_dev;
    a.threshold = io->threshold_dev; a.mean = io->mean_dev; a.sigma_out = io->sigma_out_dev; a.u_first = io->u_first_dev;
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_cost_refit");
    const dim3 grid((unsigned)N), block(CEM_REFIT_WG);
    hipLaunchKernelGGL(so100_query_cost_refit_k, grid, block, (size_t)a.P*sizeof(uint64_t) + (size_t)io->K*sizeof(float), (hipStream_t)stream, a, N);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
