// so100_query_lqr.hip -- the LQR query (gfx950) and its C ABI (include/so100_query.h: so100_query_lqr, and with a regulariser per problem
// so100_query_lqr_reg and so100_query_reg_schedule); the recursion and the pieces shared with
// the host twin are in so100_lqr.hpp.  Like so100_query_derivative.hip, not a translation unit of its own: so100_sim.hip includes it.
//
// Shape: one workgroup is one wave is one problem (blockIdx.x).  Lane l = (c, h): c = l & 31 is a COLUMN of a 32 x 32 tile, h = l >> 5 picks
// which rows the lane's registers hold: register r is row  row(r, h) = (r & 3) + 8 (r >> 2) + 4 h  -- the C/D map of v_mfma_f32_32x32x2_f32.
// Vxx lives in that map (registers V[0..NR), NR = 12 rows-pairs for n = 24, 8 for n = 12; rows and columns >= n are zero) from the terminal
// cost to step 0 and never leaves the wave.  Per step, with G = [A_t | B_t | 0] (n x 32):
//   g[r]  = G[row(r, h)][c]                                  one global load per register, 24 consecutive words of a row of A per half-wave
//   W     = Vxx G:   NR issues  mfma(V[r], g[r], W)          A operand: lane (i, h) gives Vxx[i][row(r, h)] = Vxx[row(r, h)][i] = V[r] (Vxx is
//                                                            exactly symmetric: it is symmetrised every step); B operand: G[row(r, h)][c]
//   W[.][30] = Vx                                            column 30 of G is zero, so column 30 of W is free: it carries Vx through the
//                                                            second product, whose column 30 is then G'Vx
//   H     = G' W:    NR issues  mfma(g[r], W[r], H)          A operand: lane (i, h) gives G'[i][row(r, h)] = g[r] again; B operand: the
//                                                            accumulator tile of the first product as it stands, no lane movement
//   H += [lxx lux' . lx; lux luu . lu]                       rows 0..n-1: Qxx (and Qx in column 30); rows n..n+5: Qux | Quu | . | Qu
// Both products sum over the ROW index of the tile they take, in the permuted order the map gives; k runs over n/2 (n = 12: 8, four of them
// on zero rows) issues of two.  The rank-6 tail is VALU work: rows n..n+5 of H go through LDS, every lane factors Quu + reg I (the same
// 6 x 6 in all 64), solves for k and for ITS column of K, and updates its rows of its column of Vxx from K and Qux rows read back from LDS.
// The symmetrisation is one transposed read of the tile through LDS.  The linear forward pass afterwards is serial in t: lanes 0..5 form du,
// lanes 0..n-1 the next dx.  MFMA = false replaces the two mfma chains by plain FMA loops on LDS copies of Vxx and G (the form the matrix
// instruction was timed against); everything else is the same code.
#include "so100_lqr.hpp"

namespace so100 {

typedef float lqr_tile __attribute__((ext_vector_type(16)));

#ifdef SO100_LQR_VALU
constexpr bool LQR_MFMA = false;                             // a side build (tools/side_build.py): the plain-FMA products
#else
constexpr bool LQR_MFMA = true;
#endif

// REG (so100_query_lqr_reg): the regulariser is the problem's own, and a pass whose factor fails is run again from the terminal cost
// under a raised one.  reg, the pass count and the decision are the same in every lane (the factor's failure goes through a ballot), so the wave
// never diverges on it.  Beside the plain form's accesses: one read of reg[m] and lane 0's stores to reg_used[m] and tries_out[m] of LqrRegArgs; no LDS.
// Beyond three locals (reg, which the factor reads, pass and valid) every statement of it is behind if constexpr (REG): the plain instantiations
// take no second struct and compile to the instructions they had.
__device__ __forceinline__ const LqrRegArgs<float>& lqr_reg_args(const LqrRegArgs<float>& g) { return g; }

template <int N, bool MFMA, bool REG, typename... G>
__global__ void __launch_bounds__(64) so100_query_lqr_k(LqrArgs<float> a, int M, G... extra) {
    static_assert(sizeof...(G) == (REG ? 1 : 0), "the REG forms alone take the second argument struct");
    constexpr int NU = LQR_NU, NP = N + NU, NR = N == 24 ? 12 : 8, QCOL = 30;
    static_assert(NP <= QCOL && 2*NR >= N, "the tile holds G, and column 30 is free");
    __shared__ float S[32][36], Gs[32][32], Qs[6][32], Ks[6][32], vx[32], qx[32], dxs[32], dus[8];
    const size_t m = blockIdx.x, Mz = (size_t)M;
    const int lane = (int)threadIdx.x, c = lane & 31, h = lane >> 5;
    const int TT = a.horizon;
    const float nan = __int_as_float(0x7FC00000);
#define LQR_ROW(r) (((r) & 3) + 8*((r) >> 2) + 4*h)
    float V[NR];
    // V <- (V + V')/2 through LDS; rows and columns >= N come out zero.  MFMA = false: S keeps the result for the first product.
    auto symmetrise = [&]() {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NR; r++) S[LQR_ROW(r)][c] = V[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NR; r++) { const int i = LQR_ROW(r); V[r] = (i < N && c < N) ? 0.5f*(V[r] + S[c][i]) : 0.0f; }
        if constexpr (!MFMA) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < NR; r++) S[LQR_ROW(r)][c] = V[r];
        }
    };
    float reg = a.reg;
    int pass = 0;
    bool valid = true;
    if constexpr (REG) {
        const LqrRegArgs<float>& rg = lqr_reg_args(extra...);
        if (rg.reg) reg = rg.reg[m];                         // the same word in every lane
        valid = lqr_reg_valid(reg);
    }
again:                                                       // REG: a backward pass starts here, from the terminal cost; else reached once
    bool fin = true;
    {
        const float* lxx = a.lxx + ((size_t)TT*Mz + m)*(size_t)(N*N);
#pragma unroll
        for (int r = 0; r < NR; r++) { const int i = LQR_ROW(r); V[r] = (i < N && c < N) ? lxx[i*N + c] : 0.0f; fin = fin && lqr_finite(V[r]); }
        if (lane < 32) {
            const float v = lane < N ? a.lx[((size_t)TT*Mz + m)*N + lane] : 0.0f;
            fin = fin && lqr_finite(v);
            vx[lane] = v;
            if (a.dx0 && lane < N) fin = fin && lqr_finite(a.dx0[m*N + lane]);
        }
        symmetrise();
    }
    int bad = __builtin_amdgcn_ballot_w64(!fin) != 0ull ? TT : -1;
    if constexpr (REG) { if (valid) pass++; else bad = TT; } // a start that is no reg is a non-finite input, and no pass runs
    float dV1 = 0.0f, dV2 = 0.0f;
    for (int t = TT - 1; t >= 0 && bad < 0; t--) {
        const size_t p = (size_t)t*Mz + m;
        const float* At = a.A + p*576; const float* Bt = a.B + p*144;
        float g[NR];
        fin = true;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int k = LQR_ROW(r);
            float v = 0.0f;
            if (k < N && c < N) v = At[lqr_idx<N>(k)*24 + lqr_idx<N>(c)];
            else if (k < N && c < NP) v = Bt[lqr_idx<N>(k)*NU + (c - N)];
            g[r] = v; fin = fin && lqr_finite(v);
        }
        // the step's cost in the tile's map: [lxx lux']  and (lx; lu) in column 30
        //                                    [lux luu ]
        lqr_tile cost;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = LQR_ROW(r);
            float v = 0.0f;
            if ((r & 3) + 8*(r >> 2) < NP) {                 // a register whose rows are beyond the tile's 30 (18) in both halves holds nothing
                if (i < N) {
                    if (c < N) v = a.lxx[p*(size_t)(N*N) + i*N + c];
                    else if (c == QCOL) v = a.lx[p*N + i];
                } else if (i < NP) {
                    if (c < N) { if (a.lux) v = a.lux[(p*NU + (i - N))*N + c]; }
                    else if (c < NP) { if (a.luu) v = a.luu[p*(NU*NU) + (i - N)*NU + (c - N)]; }
                    else if (c == QCOL) { if (a.lu) v = a.lu[p*NU + (i - N)]; }
                }
            }
            cost[r] = v; fin = fin && lqr_finite(v);
        }
        if (a.u && lane < NU) fin = fin && lqr_finite(a.u[p*NU + lane]);
        if (__builtin_amdgcn_ballot_w64(!fin) != 0ull) { bad = TT; break; }
        lqr_tile W, H;
#pragma unroll
        for (int r = 0; r < 16; r++) { W[r] = 0.0f; H[r] = 0.0f; }
        if constexpr (MFMA) {
#pragma unroll
            for (int r = 0; r < NR; r++) W = __builtin_amdgcn_mfma_f32_32x32x2f32(V[r], g[r], W, 0, 0, 0);
            if (c == QCOL) {
#pragma unroll
                for (int r = 0; r < NR; r++) W[r] = vx[LQR_ROW(r)];
            }
#pragma unroll
            for (int r = 0; r < NR; r++) H = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], W[r], H, 0, 0, 0);
        } else {
            // the same two products, each lane its own rows of its own column: the other half's rows of G and W come by a lane exchange,
            // Vxx and G' are read from LDS
            float go[NR], wo[NR];
#pragma unroll
            for (int r = 0; r < NR; r++) { go[r] = __shfl_xor(g[r], 32); Gs[LQR_ROW(r)][c] = g[r]; }
            __syncthreads();                                 // S (written by symmetrise) and Gs
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int i = LQR_ROW(r);
                float s = 0.0f;
#pragma unroll
                for (int r2 = 0; r2 < NR; r2++) {
                    const int k0 = (r2 & 3) + 8*(r2 >> 2);
                    s = fmaf(S[i][k0 + 4*h], g[r2], s);
                    s = fmaf(S[i][k0 + 4 - 4*h], go[r2], s);
                }
                W[r] = c == QCOL ? vx[i] : s;
            }
#pragma unroll
            for (int r = 0; r < NR; r++) wo[r] = __shfl_xor(W[r], 32);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if ((r & 3) + 8*(r >> 2) >= NP) continue;
                const int i = LQR_ROW(r);
                float s = 0.0f;
#pragma unroll
                for (int r2 = 0; r2 < NR; r2++) {
                    const int k0 = (r2 & 3) + 8*(r2 >> 2);
                    s = fmaf(Gs[k0 + 4*h][i], W[r2], s);
                    s = fmaf(Gs[k0 + 4 - 4*h][i], wo[r2], s);
                }
                H[r] = s;
            }
        }
        H += cost;
        // rows n..n+5 (Qux | Quu | . | Qu) and Qx (column 30 of rows 0..n-1) to LDS
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = LQR_ROW(r);
            if ((r & 3) + 8*(r >> 2) + 4 >= N && i >= N && i < NP) Qs[i - N][c] = H[r];
        }
        if (c == QCOL) {
#pragma unroll
            for (int r = 0; r < NR; r++) { const int i = LQR_ROW(r); if (i < N) qx[i] = H[r]; }
        }
        __syncthreads();
        float Quu[6][6], Qu[6], Qc[6], L[6][6], inv[6], kk[6], Kc[6], Qk[6], QK[6];
#pragma unroll
        for (int i = 0; i < NU; i++) {
            Qu[i] = Qs[i][QCOL]; Qc[i] = Qs[i][c];
#pragma unroll
            for (int j = 0; j < NU; j++) Quu[i][j] = Qs[i][N + j];
        }
        const bool ok = lqr_chol6(Quu, reg, L, inv);
        if (__builtin_amdgcn_ballot_w64(!ok) != 0ull) { bad = t; break; }
        lqr_solve6(L, inv, Qu, kk);
        lqr_solve6(L, inv, Qc, Kc);
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < NU; i++) {
            float sk = 0.0f, sK = 0.0f;
#pragma unroll
            for (int j = 0; j < NU; j++) { sk += Quu[i][j]*kk[j]; sK += Quu[i][j]*Kc[j]; }
            Qk[i] = sk; QK[i] = sK;
            s1 += kk[i]*Qu[i]; s2 += kk[i]*sk;
        }
        dV1 += s1; dV2 += 0.5f*s2;
        if (lane < N) {
#pragma unroll
            for (int i = 0; i < NU; i++) { Ks[i][c] = Kc[i]; if (a.K) a.K[(p*NU + i)*N + c] = Kc[i]; }
        }
        if (a.k) {
#pragma unroll
            for (int i = 0; i < NU; i++) if (lane == i) a.k[p*NU + i] = kk[i];
        }
        __syncthreads();
        float vnew = qx[c];
#pragma unroll
        for (int i = 0; i < NU; i++) vnew += Kc[i]*(Qk[i] + Qu[i]) + Qc[i]*kk[i];
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int i = LQR_ROW(r);
            float s = H[r];
#pragma unroll
            for (int l = 0; l < NU; l++) s += Ks[l][i]*(QK[l] + Qc[l]) + Qs[l][i]*Kc[l];
            V[r] = s;
        }
        __syncthreads();                                     // every read of vx, qx, Qs and Ks of this step is done
        if (lane < N) vx[lane] = vnew;
        symmetrise();
    }
    if constexpr (REG) {
        const LqrRegArgs<float>& rg = lqr_reg_args(extra...);
        // the failed step's reads of vx, S and Gs lie before its barrier, and the next pass writes Qs, qx and Ks behind symmetrise's: no barrier here
        if (lqr_reg_again(bad, TT, pass, rg.tries, reg, rg.reg_max)) { reg = lqr_reg_raise(reg, rg.reg_min, rg.reg_max, rg.reg_up); goto again; }
        if (lane == 0 && rg.reg_used) rg.reg_used[m] = valid ? reg : nan;
        if (lane == 0 && rg.tries_out) rg.tries_out[m] = pass;
    }
    if (lane == 0 && a.bad) a.bad[m] = bad;
    if (bad >= 0) {                                          // every float output of a failed problem is NaN
        __syncthreads();                                     // behind the k and K rows other lanes wrote before the failure
        for (int t = 0; t < TT; t++) {
            const size_t p = (size_t)t*Mz + m;
            if (a.k && lane < NU) a.k[p*NU + lane] = nan;
            if (a.du && lane < NU) a.du[p*NU + lane] = nan;
            if (a.K) for (int j = lane; j < NU*N; j += 64) a.K[p*(size_t)(NU*N) + j] = nan;
        }
        if (a.dx && lane < N) for (int t = 0; t <= TT; t++) a.dx[((size_t)t*Mz + m)*N + lane] = nan;
        if (a.Vx0 && lane < N) a.Vx0[m*N + lane] = nan;
        if (a.Vxx0) for (int j = lane; j < N*N; j += 64) a.Vxx0[m*(size_t)(N*N) + j] = nan;
        if (a.dV && lane < 2) a.dV[2*m + lane] = nan;
        return;
    }
    if (a.Vx0 && lane < N) a.Vx0[m*N + lane] = vx[lane];    // symmetrise's barriers stand between vx's last write and this read
    if (a.Vxx0 && c < N) {
#pragma unroll
        for (int r = 0; r < NR; r++) { const int i = LQR_ROW(r); if (i < N) a.Vxx0[m*(size_t)(N*N) + i*N + c] = V[r]; }
    }
    if (a.dV && lane == 0) { a.dV[2*m] = dV1; a.dV[2*m + 1] = dV2; }
    if (!a.du && !a.dx) return;
    // the linear forward pass: k and K are read back from the output arrays (written above by other lanes of this wave)
    if (lane < 32) dxs[lane] = (lane < N && a.dx0) ? a.dx0[m*N + lane] : 0.0f;
    __syncthreads();
    for (int t = 0; t < TT; t++) {
        const size_t p = (size_t)t*Mz + m;
        const float* At = a.A + p*576; const float* Bt = a.B + p*144;
        if (a.dx && lane < N) a.dx[p*N + lane] = dxs[lane];
        if (lane < NU) {
            const float* Kr = a.K + (p*NU + lane)*N;
            float d = a.alpha*a.k[p*NU + lane];
#pragma unroll
            for (int j = 0; j < N; j++) d += Kr[j]*dxs[j];
            if (a.u) { const float u = a.u[p*NU + lane]; float v = u + d; v = v < a.u_lo ? a.u_lo : v; v = v > a.u_hi ? a.u_hi : v; d = v - u; }
            dus[lane] = d;
            if (a.du) a.du[p*NU + lane] = d;
        }
        __syncthreads();
        float s = 0.0f;
        if (lane < N) {
            const float* Ar = At + lqr_idx<N>(lane)*24; const float* Br = Bt + lqr_idx<N>(lane)*NU;
#pragma unroll
            for (int j = 0; j < N; j++) s += Ar[lqr_idx<N>(j)]*dxs[j];
#pragma unroll
            for (int j = 0; j < NU; j++) s += Br[j]*dus[j];
        }
        __syncthreads();
        if (lane < N) dxs[lane] = s;
        __syncthreads();
    }
    if (a.dx && lane < N) a.dx[((size_t)TT*Mz + m)*N + lane] = dxs[lane];
#undef LQR_ROW
}

// so100_query_reg_schedule: one lane per problem.  reg and reg_used may be the same array: a lane reads its word before it writes it.
struct RegScheduleArgs { const float* reg_used; const int32_t* best; int keep; float reg_min, reg_max, reg_up, reg_down; float* reg; uint8_t* improved; };

__global__ void __launch_bounds__(QUERY_THREADS) so100_query_reg_schedule_k(RegScheduleArgs s, int M) {
    const size_t i = (size_t)blockIdx.x*QUERY_THREADS + threadIdx.x;
    if (i >= (size_t)M) return;
    const int best = s.best[i];
    const bool improved = best >= 0 && best != s.keep;
    s.reg[i] = lqr_reg_next(s.reg_used[i], improved, s.reg_min, s.reg_max, s.reg_up, s.reg_down);
    if (s.improved) s.improved[i] = improved ? 1 : 0;
}

namespace {

// the checks so100_query_lqr and so100_query_lqr_reg share, up to the one on the outputs (each entry counts its own)
int lqr_check(const char* fn, const so100_sim* sim, const so100_lqr_io* io, int32_t M) {
    if (const int rc = query_batch(fn, sim, false, M)) return rc;                 // no state is read: any M >= 1
    if (io->nx != 12 && io->nx != 24) return fail(SO100_E_INVALID, "%s: nx must be 12 or 24, got %ld", fn, (long)io->nx);
    if (io->T < 1 || io->T > SO100_LQR_MAX_T) return fail(SO100_E_INVALID, "%s: T must be in 1..%d, got %ld", fn, SO100_LQR_MAX_T, (long)io->T);
    if (!io->A_dev || !io->B_dev || !io->lx_dev || !io->lxx_dev) return fail(SO100_E_INVALID, "%s: A_dev, B_dev, lx_dev and lxx_dev are required", fn);
    if (!(io->reg >= 0.0f) || !(io->reg*0.0f == 0.0f)) return fail(SO100_E_INVALID, "%s: reg must be finite and >= 0, got %g", fn, (double)io->reg);
    if (!(io->alpha*0.0f == 0.0f)) return fail(SO100_E_INVALID, "%s: alpha must be finite, got %g", fn, (double)io->alpha);
    if (!(io->u_lo <= io->u_hi)) return fail(SO100_E_INVALID, "%s: u_lo must be <= u_hi, got %g and %g", fn, (double)io->u_lo, (double)io->u_hi);
    if ((io->du_dev || io->dx_dev) && (!io->k_dev || !io->K_dev)) return fail(SO100_E_INVALID, "%s: du_dev and dx_dev need k_dev and K_dev", fn);
    return 0;
}
bool lqr_any_output(const so100_lqr_io* io) {
    return io->k_dev || io->K_dev || io->Vx0_dev || io->Vxx0_dev || io->dV_dev || io->du_dev || io->dx_dev || io->bad_dev;
}
LqrArgs<float> lqr_args(const so100_lqr_io* io) {
    LqrArgs<float> a{};
    a.A = io->A_dev; a.B = io->B_dev; a.lx = io->lx_dev; a.lxx = io->lxx_dev; a.lu = io->lu_dev; a.luu = io->luu_dev; a.lux = io->lux_dev;
    a.u = io->u_dev; a.dx0 = io->dx0_dev; a.horizon = io->T; a.reg = io->reg; a.alpha = io->alpha; a.u_lo = io->u_lo; a.u_hi = io->u_hi;
    a.k = io->k_dev; a.K = io->K_dev; a.Vx0 = io->Vx0_dev; a.Vxx0 = io->Vxx0_dev; a.dV = io->dV_dev; a.du = io->du_dev; a.dx = io->dx_dev; a.bad = io->bad_dev;
    return a;
}

}  // namespace
}  // namespace so100

static_assert(SO100_LQR_NU == so100::LQR_NU && SO100_LQR_MAX_T == so100::LQR_MAX_T && SO100_DERIV_NX == 24 && SO100_DERIV_NU == 6,
              "the header names the sizes; A and B are in the derivatives query's layout");
static_assert(SO100_LQR_REG_MAX_TRIES == so100::LQR_REG_MAX_TRIES, "the header names the limit");

extern "C" {

int so100_query_lqr(so100_sim* sim, const so100_lqr_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_lqr";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_lqr: null argument");
    if (const int rc = lqr_check(fn, sim, io, M)) return rc;
    if (!lqr_any_output(io)) return fail(SO100_E_INVALID, "%s: no output requested", fn);
    const LqrArgs<float> a = lqr_args(io);
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_lqr");
    const dim3 grid((unsigned)M), block(64);                 // one wave per problem
    if (io->nx == 24) hipLaunchKernelGGL((so100_query_lqr_k<24, LQR_MFMA, false>), grid, block, 0, (hipStream_t)stream, a, M);
    else              hipLaunchKernelGGL((so100_query_lqr_k<12, LQR_MFMA, false>), grid, block, 0, (hipStream_t)stream, a, M);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

int so100_query_lqr_reg(so100_sim* sim, const so100_lqr_reg_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_lqr_reg";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_lqr_reg: null argument");
    if (const int rc = lqr_check(fn, sim, &io->base, M)) return rc;
    if (const int rc = query_reg_range(fn, io->reg_min, io->reg_max, io->reg_up)) return rc;
    if (io->tries < 1 || io->tries > SO100_LQR_REG_MAX_TRIES) return fail(SO100_E_INVALID, "%s: tries must be in 1..%d, got %ld", fn, SO100_LQR_REG_MAX_TRIES, (long)io->tries);
    if (!lqr_any_output(&io->base) && !io->reg_used_dev && !io->tries_dev) return fail(SO100_E_INVALID, "%s: no output requested", fn);
    const LqrArgs<float> a = lqr_args(&io->base);
    const LqrRegArgs<float> rg{ io->reg_dev, io->reg_min, io->reg_max, io->reg_up, io->tries, io->reg_used_dev, io->tries_dev };
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_lqr_reg");
    const dim3 grid((unsigned)M), block(64);                 // one wave per problem
    if (io->base.nx == 24) hipLaunchKernelGGL((so100_query_lqr_k<24, LQR_MFMA, true, LqrRegArgs<float>>), grid, block, 0, (hipStream_t)stream, a, M, rg);
    else                   hipLaunchKernelGGL((so100_query_lqr_k<12, LQR_MFMA, true, LqrRegArgs<float>>), grid, block, 0, (hipStream_t)stream, a, M, rg);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

int so100_query_reg_schedule(so100_sim* sim, const so100_reg_schedule_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_reg_schedule";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_reg_schedule: null argument");
    if (const int rc = query_batch(fn, sim, false, M)) return rc;                 // no state is read: any M >= 1
    if (!io->reg_used_dev || !io->best_dev || !io->reg_dev) return fail(SO100_E_INVALID, "%s: reg_used_dev, best_dev and reg_dev are required", fn);
    if (io->keep < -1) return fail(SO100_E_INVALID, "%s: keep must be a candidate index or -1, got %ld", fn, (long)io->keep);
    if (const int rc = query_reg_range(fn, io->reg_min, io->reg_max, io->reg_up)) return rc;
    if (!(io->reg_down > 0.0f) || !(io->reg_down <= 1.0f)) return fail(SO100_E_INVALID, "%s: reg_down must be in (0, 1], got %g", fn, (double)io->reg_down);
    const RegScheduleArgs s{ io->reg_used_dev, io->best_dev, io->keep, io->reg_min, io->reg_max, io->reg_up, io->reg_down, io->reg_dev, io->improved_dev };
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_reg_schedule");
    hipLaunchKernelGGL(so100_query_reg_schedule_k, dim3(query_grid(M)), dim3(QUERY_THREADS), 0, (hipStream_t)stream, s, M);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
