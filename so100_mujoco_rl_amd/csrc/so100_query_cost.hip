// so100_query_cost.hip -- the two cost queries (gfx950) and their C ABI (include/so100_query.h: so100_query_cost_terms, so100_query_cost_select);
// the cost family and every entry's arithmetic are in so100_cost.hpp.  Like so100_query_lqr.hip, not a translation unit of its own: so100_sim.hip
// includes it.
//
// Terms.  The outputs are PROBLEM-major (n + n^2 = 600 floats per step and problem at n = 24): a lane storing its own problem's block would scatter
// every store.  So one workgroup of four waves is 64 consecutive problems of ONE step t (blockIdx.x: the 64, blockIdx.y: t), in two phases:
//   1. lane l of wave 0 runs problem m0 + l's chain (FK, point, Jacobian, residual: the Jacobian query's) from coalesced SoA loads and leaves the 33 numbers
//      the block is made of (J 18, r 3, the two weighted differences 6 + 6), 2 w_u u and two finite bits in LDS, component-major (no bank conflict)
//   2. the 64 problems' lx rows are ONE contiguous span of lx, and so are their lxx, lu and luu blocks: thread l of the 256 takes words l, l + 256, ...
//      of a span (16-byte stores of words 4 l .. 4 l + 3 where the caller's arrays are 16-byte aligned), works out which (problem, i, j) a word is and makes
//      that entry from the problem's LDS record -- or writes the zero that most of the block is.  Within a 16-byte store the problem and the row are
//      the same (n is a multiple of 4), and the lanes of a wave read at most a few problems' records at a time: LDS broadcasts.
// The workgroup of step 0 also writes the zero row 0.  lu's span starts at a multiple of 6 words: 4-byte stores.  Four waves, not one: the chain is a
// small part of the work, the 38 400 words of a block at n = 24 are the rest, and one wave storing them alone left the small batches a planner runs
// (M <= 4096) waiting on that wave's 150 stores in a row (DESIGN.md 17.4 has both figures).
//
// Select.  One lane per rollout; a problem's L candidates are L neighbouring lanes that never straddle a wave: 64 / L problems per wave, the lanes
// behind them idle.  Rollout (m, a) is column m L + a, so a wave's loads are one contiguous segment of each SoA row.  Each lane sums its rollout's
// cost over t in registers; the argmin is L lane reads inside the group (every lane of a group walks the candidates in ascending order and comes to
// the same answer: no LDS, no atomics, the same bits whatever M); the group's lanes then share the gather of the winner's T x 6 controls.
#include "so100_cost.hpp"

namespace so100 {

constexpr int COST_WAVE = 64, COST_REC = 33;                 // J 18, r 3, gq 6, gv 6
constexpr int COST_TERMS_WG = 256;                           // the terms kernel's workgroup: wave 0 runs the 64 chains, all four waves store

struct CostTermsArgs {
    CostDef<float> c;
    const float *target, *qpos, *qvel, *u;
    int T;
    float *lx, *lxx, *lu, *luu;
};
// the rollouts a planner query prices (select, and the blend and refit of the files behind this one): [T][k][columns] rows of `columns` rollouts, the
// candidates of a problem side by side; target and u_fallback are per problem.  qvel, bad_step and u_fallback may be null
struct CostRollouts {
    CostDef<float> c;
    const float *target, *qpos, *qvel, *u;
    const int32_t* bad_step; const float* u_fallback;
    int T, K;                                                // steps; candidates of a problem (select's L)
};
struct CostSelectArgs {
    CostRollouts in;
    float* cost; int32_t* best; float* best_cost; float* u_best;
};

// a problem's record in LDS, behind so100_cost.hpp's accessor
struct CostLdsRow {
    const float (*rec)[COST_WAVE]; int p;
    __device__ float J(int a, int k) const { return rec[6*a + k][p]; }
    __device__ float r(int a) const { return rec[18 + a][p]; }
    __device__ float gq(int k) const { return rec[21 + k][p]; }
    __device__ float gv(int k) const { return rec[27 + k][p]; }
};

// thread `lane` of the workgroup stores words lane, lane + 256, ... of base[0 .. words) (V = 4: words 4 lane .. 4 lane + 3, ... in one store; words is
// then a multiple of 4 and base 16-byte aligned); entry(w) makes word w
template <int V, typename F> __device__ __forceinline__ void cost_store_span(float* base, int words, int lane, F&& entry) {
    if constexpr (V == 4) {
        for (int w = 4*lane; w < words; w += 4*COST_TERMS_WG) {
            float4 x;
            x.x = entry(w); x.y = entry(w + 1); x.z = entry(w + 2); x.w = entry(w + 3);
            *reinterpret_cast<float4*>(base + w) = x;
        }
    } else {
        for (int w = lane; w < words; w += COST_TERMS_WG) base[w] = entry(w);
    }
}

template <int N, int V>
__global__ void __launch_bounds__(COST_TERMS_WG) so100_query_cost_terms_k(CostTermsArgs a, int M) {
    __shared__ float rec[COST_REC][COST_WAVE], lus[COST_NU][COST_WAVE];
    __shared__ int oks[COST_WAVE];                           // bit 0: the state row's inputs are finite, bit 1: u_t's
    const int lane = (int)threadIdx.x, t = (int)blockIdx.y;
    const size_t Mz = (size_t)M, m0 = (size_t)blockIdx.x*COST_WAVE, m = m0 + (size_t)lane;
    const int cnt = Mz - m0 < (size_t)COST_WAVE ? (int)(Mz - m0) : COST_WAVE;
    const bool states = a.lx || a.lxx, controls = a.lu || a.luu;
    const float nan = __int_as_float(0x7FC00000);
    int ok = 0;
    if (lane < cnt) {
        if (states) {
            float q[6], v[6], g[3];
            const float* qp = a.qpos + (size_t)t*13*Mz;
#pragma unroll
            for (int j = 0; j < 6; j++) { q[j] = qp[(size_t)j*Mz + m]; v[j] = a.qvel ? a.qvel[((size_t)t*12 + j)*Mz + m] : 0.0f; }
#pragma unroll
            for (int i = 0; i < 3; i++) {
                if (a.c.target_mode == COST_TARGET_CUBE) g[i] = qp[(size_t)(6 + i)*Mz + m];
                else g[i] = a.target[((a.c.target_mode == COST_TARGET_TRAJ ? (size_t)t*3 : (size_t)0) + i)*Mz + m];
            }
            CostRow<float> R;
            cost_row<float>(a.c, q, v, g, R);
#pragma unroll
            for (int k = 0; k < 18; k++) rec[k][lane] = R.J[k];
#pragma unroll
            for (int k = 0; k < 3; k++) rec[18 + k][lane] = R.r[k];
#pragma unroll
            for (int k = 0; k < 6; k++) { rec[21 + k][lane] = R.gq[k]; rec[27 + k][lane] = R.gv[k]; }
            ok |= R.ok ? 1 : 0;
        }
        if (controls) {
            float u[6];
            bool fin = true;
#pragma unroll
            for (int j = 0; j < 6; j++) { u[j] = a.u[((size_t)t*6 + j)*Mz + m]; fin = fin && cost_finite(u[j]); }
#pragma unroll
            for (int j = 0; j < 6; j++) lus[j][lane] = cost_lu<float>(a.c, u, j);
            ok |= fin ? 2 : 0;
        }
    }
    if (lane < COST_WAVE) oks[lane] = ok;
    __syncthreads();
    const float two_sigma = 2.0f*cost_sigma<float>(a.c, t, a.T);
    const size_t row = ((size_t)(t + 1)*Mz + m0), step = (size_t)t*Mz + m0;
    if (a.lx) {
        if (t == 0) cost_store_span<V>(a.lx + m0*N, cnt*N, lane, [](int) { return 0.0f; });
        cost_store_span<V>(a.lx + row*N, cnt*N, lane, [&](int w) {
            const int p = w/N, i = w - p*N;
            const float x = cost_lx<float>(a.c, CostLdsRow{ rec, p }, two_sigma, cost_idx(N, i));
            return (oks[p] & 1) ? x : nan;
        });
    }
    if (a.lxx) {
        if (t == 0) cost_store_span<V>(a.lxx + m0*(size_t)(N*N), cnt*N*N, lane, [](int) { return 0.0f; });
        cost_store_span<V>(a.lxx + row*(size_t)(N*N), cnt*N*N, lane, [&](int w) {
            const int p = w/(N*N), e = w - p*(N*N), i = e/N, j = e - i*N;
            const float x = cost_lxx<float>(a.c, CostLdsRow{ rec, p }, two_sigma, cost_idx(N, i), cost_idx(N, j));
            return (oks[p] & 1) ? x : nan;
        });
    }
    if (a.lu) cost_store_span<1>(a.lu + step*COST_NU, cnt*COST_NU, lane, [&](int w) { const int p = w/COST_NU, j = w - p*COST_NU; return (oks[p] & 2) ? lus[j][p] : nan; });
    if (a.luu) cost_store_span<V>(a.luu + step*(COST_NU*COST_NU), cnt*COST_NU*COST_NU, lane, [&](int w) {
        const int p = w/(COST_NU*COST_NU), e = w - p*(COST_NU*COST_NU), i = e/COST_NU, j = e - i*COST_NU;
        return (oks[p] & 2) ? cost_luu<float>(a.c, i, j) : nan;
    });
}

// what rollout `col` of problem n costs: the sum of its T steps and the terminal term, +inf where it failed or the sum is not finite
__device__ __forceinline__ float cost_rollout(const CostRollouts& a, size_t problems, size_t columns, size_t n, size_t col) {
    const float total = cost_total<float>(a.c, a.T, [&](int t, float q[6], float v[6], float u[6], float g[3]) {
        const float* qp = a.qpos + (size_t)t*13*columns;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            q[j] = qp[(size_t)j*columns + col];
            v[j] = a.qvel ? a.qvel[((size_t)t*12 + j)*columns + col] : 0.0f;
            u[j] = a.u[((size_t)t*6 + j)*columns + col];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (a.c.target_mode == COST_TARGET_CUBE) g[i] = qp[(size_t)(6 + i)*columns + col];
            else g[i] = a.target[((a.c.target_mode == COST_TARGET_TRAJ ? (size_t)t*3 : (size_t)0) + i)*problems + n];
        }
    });
    const bool failed = a.bad_step && a.bad_step[col] >= 0;
    return (failed || !cost_finite(total)) ? __int_as_float(0x7F800000) : total;
}

__global__ void __launch_bounds__(COST_WAVE) so100_query_cost_select_k(CostSelectArgs a, int M) {
    const int lane = (int)threadIdx.x, L = a.in.K, G = COST_WAVE/L;
    const int grp = lane/L, cand = lane - grp*L;
    const size_t Mz = (size_t)M, ML = Mz*(size_t)L, m = (size_t)blockIdx.x*(size_t)G + (size_t)grp;
    const bool live = grp < G && m < Mz;
    const size_t col = m*(size_t)L + (size_t)cand;
    const float inf = __int_as_float(0x7F800000), nan = __int_as_float(0x7FC00000);
    float cost = inf;
    if (live) {
        cost = cost_rollout(a.in, Mz, ML, m, col);
        if (a.cost) a.cost[col] = cost;
    }
    if (!a.best && !a.best_cost && !a.u_best) return;        // uniform: the whole wave leaves or stays
    // every lane of the wave takes part in the lane reads; a lane without a rollout reads itself
    float best_cost;
    const int best = cost_argmin<float>(L, inf, [&](int k) { return __shfl(cost, live ? grp*L + k : lane); }, best_cost);
    if (!live) return;
    if (cand == 0) {
        if (a.best) a.best[m] = best;
        if (a.best_cost) a.best_cost[m] = best_cost;
    }
    if (a.u_best) {
        const int words = a.in.T*COST_NU;                     // the (t, j) rows of the winner's column, dealt over the group's lanes
        for (int w = cand; w < words; w += L) {
            float x = nan;
            if (best >= 0) x = a.in.u[(size_t)w*ML + m*(size_t)L + (size_t)best];
            else if (a.in.u_fallback) x = a.in.u_fallback[(size_t)w*Mz + m];
            a.u_best[(size_t)w*Mz + m] = x;
        }
    }
}

namespace {

// the checks of a so100_cost_def, in the header's order, and its copy for the launch
int cost_def(const char* fn, const so100_cost_def* d, CostDef<float>& c) {
    if (!d) return fail(SO100_E_INVALID, "%s: cost is required", fn);
    QueryPoint pt;
    if (const int rc = query_point(fn, d->link, d->offset, pt)) return rc;
    const auto finite = [](float x) { return x*0.0f == 0.0f; };
    if (!finite(pt.o[0]) || !finite(pt.o[1]) || !finite(pt.o[2])) return fail(SO100_E_INVALID, "%s: offset must be finite", fn);
    if (d->target_mode != SO100_COST_TARGET_FIXED && d->target_mode != SO100_COST_TARGET_TRAJ && d->target_mode != SO100_COST_TARGET_CUBE)
        return fail(SO100_E_INVALID, "%s: unknown target_mode %ld", fn, (long)d->target_mode);
    bool ok = finite(d->w_point) && d->w_point >= 0.0f && finite(d->w_terminal) && d->w_terminal >= 0.0f;
    for (int j = 0; j < 6; j++)
        ok = ok && finite(d->w_q[j]) && d->w_q[j] >= 0.0f && finite(d->w_v[j]) && d->w_v[j] >= 0.0f && finite(d->w_u[j]) && d->w_u[j] >= 0.0f && finite(d->q_nom[j]);
    if (!ok) return fail(SO100_E_INVALID, "%s: w_point, w_q, w_v, w_u and w_terminal must be finite and >= 0 and q_nom finite", fn);
    c.link = pt.link; c.target_mode = d->target_mode; c.w_point = d->w_point; c.w_terminal = d->w_terminal;
    for (int i = 0; i < 3; i++) c.o[i] = pt.o[i];
    for (int j = 0; j < 6; j++) { c.w_q[j] = d->w_q[j]; c.q_nom[j] = d->q_nom[j]; c.w_v[j] = d->w_v[j]; c.w_u[j] = d->w_u[j]; }
    return 0;
}

// the rollouts of a select, blend or refit io struct (K candidates a problem), behind cost_def(fn, io.cost, in.c): the pointers every one of them needs (`also_missing`: one the
// entry needs beside them is null; `required`: the message's list of both) and the block's copy for the launch
template <typename IO> int cost_rollouts(const char* fn, const IO& io, int32_t K, const char* required, bool also_missing, CostRollouts& in) {
    if (!io.qpos_traj_dev || !io.u_traj_dev || (in.c.target_mode != COST_TARGET_CUBE && !io.target_dev) || also_missing)
        return fail(SO100_E_INVALID, "%s: %s are required", fn, required);
    in.target = io.target_dev; in.qpos = io.qpos_traj_dev; in.qvel = io.qvel_traj_dev; in.u = io.u_traj_dev; in.bad_step = io.bad_step_dev;
    in.u_fallback = io.u_fallback_dev; in.T = io.T; in.K = K;
    return 0;
}
constexpr const char* COST_ROLLOUTS_REQUIRED = "qpos_traj_dev, u_traj_dev and (unless the target is the cube) target_dev";

bool cost_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace so100

static_assert(SO100_COST_TARGET_FIXED == so100::COST_TARGET_FIXED && SO100_COST_TARGET_TRAJ == so100::COST_TARGET_TRAJ &&
              SO100_COST_TARGET_CUBE == so100::COST_TARGET_CUBE && SO100_LQR_NU == so100::COST_NU && SO100_CL_MAX_L <= so100::COST_WAVE,
              "the header names the target modes; a candidate group fits a wave");

extern "C" {

int so100_query_cost_terms(so100_sim* sim, const so100_cost_terms_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_cost_terms";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_cost_terms: null argument");
    if (const int rc = query_batch(fn, sim, false, M)) return rc;                 // no state is read: any M >= 1
    if (io->nx != 12 && io->nx != 24) return fail(SO100_E_INVALID, "%s: nx must be 12 or 24, got %ld", fn, (long)io->nx);
    if (const int rc = query_steps(fn, io->T, SO100_LQR_MAX_T)) return rc;
    CostTermsArgs a{};
    if (const int rc = cost_def(fn, io->cost, a.c)) return rc;
    if (!io->qpos_traj_dev || !io->u_dev || (a.c.target_mode != COST_TARGET_CUBE && !io->target_dev))
        return fail(SO100_E_INVALID, "%s: qpos_traj_dev, u_dev and (unless the target is the cube) target_dev are required", fn);
    if (!io->lx_dev && !io->lxx_dev && !io->lu_dev && !io->luu_dev) return fail(SO100_E_INVALID, "%s: no output requested", fn);
    a.target = io->target_dev; a.qpos = io->qpos_traj_dev; a.qvel = io->qvel_traj_dev; a.u = io->u_dev; a.T = io->T;
    a.lx = io->lx_dev; a.lxx = io->lxx_dev; a.lu = io->lu_dev; a.luu = io->luu_dev;
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_cost_terms");
    const dim3 grid((unsigned)(((size_t)M + COST_WAVE - 1)/COST_WAVE), (unsigned)io->T), block(COST_TERMS_WG);
    const bool wide = cost_aligned16(io->lx_dev) && cost_aligned16(io->lxx_dev) && cost_aligned16(io->luu_dev);
    if (io->nx == 24) {
        if (wide) hipLaunchKernelGGL((so100_query_cost_terms_k<24, 4>), grid, block, 0, (hipStream_t)stream, a, M);
        else      hipLaunchKernelGGL((so100_query_cost_terms_k<24, 1>), grid, block, 0, (hipStream_t)stream, a, M);
    } else {
        if (wide) hipLaunchKernelGGL((so100_query_cost_terms_k<12, 4>), grid, block, 0, (hipStream_t)stream, a, M);
        else      hipLaunchKernelGGL((so100_query_cost_terms_k<12, 1>), grid, block, 0, (hipStream_t)stream, a, M);
    }
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

int so100_query_cost_select(so100_sim* sim, const so100_cost_select_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_cost_select";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_cost_select: null argument");
    if (const int rc = query_batch(fn, sim, false, M)) return rc;
    if (const int rc = query_steps(fn, io->T, SO100_LQR_MAX_T)) return rc;
    if (const int rc = query_candidates(fn, "L", "M", io->L, SO100_CL_MAX_L, M)) return rc;
    CostSelectArgs a{};
    if (const int rc = cost_def(fn, io->cost, a.in.c)) return rc;
    if (const int rc = cost_rollouts(fn, *io, io->L, COST_ROLLOUTS_REQUIRED, false, a.in)) return rc;
    if (!io->cost_dev && !io->best_dev && !io->best_cost_dev && !io->u_best_dev) return fail(SO100_E_INVALID, "%s: no output requested", fn);
    a.cost = io->cost_dev; a.best = io->best_dev; a.best_cost = io->best_cost_dev; a.u_best = io->u_best_dev;
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_cost_select");
    const size_t per_wave = (size_t)(COST_WAVE/io->L);
    const dim3 grid((unsigned)(((size_t)M + per_wave - 1)/per_wave)), block(COST_WAVE);
    hipLaunchKernelGGL(so100_query_cost_select_k, grid, block, 0, (hipStream_t)stream, a, M);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
