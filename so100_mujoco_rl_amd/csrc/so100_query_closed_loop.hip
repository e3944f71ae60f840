// so100_query_closed_loop.hip -- the closed-loop trajectory query (gfx950) and its C ABI (include/so100_query.h: so100_query_closed_loop); the
// law and the rollout are in so100_closed_loop.hpp.  Like so100_query_trajectory.hip, not a translation unit of its own: so100_sim.hip includes it.
//
// Shape: the trajectory kernel's.  One lane per ROLLOUT, one wave per workgroup; lane i = m L + a is candidate a of problem m, so the L
// candidates of a problem are neighbours and read the same k_t, K_t, u_t and reference rows.  The rollout's physics rows stay in registers for
// all T x nsub substeps.  Lanes at or past M L redo the last rollout and store nothing: every lane of a wave runs the same T turns of the
// rollout's loop, which is what lets the wave load together (below).
// Memory.  The start, u and the references are [k][M]: lane i reads word m of a row.  Outputs are [k][M L]: lane i writes word i, one coalesced
// segment per wave and row.  The gains k [T][M][6] and K [T][M][6][nx] are problem-major (what so100_query_lqr writes), and reach the lanes in one
// of two ways:
//   global (shipped)        each lane loads K_t[j][i] of its problem as the law consumes it; the address is the same within a candidate group
//   LDS (SO100_CL_LDS)      for a fixed t the K_t blocks of the wave's problems are ONE contiguous span of K: the wave copies it into LDS with
//                           coalesced loads (lane l takes words l, l + 64, ...), then each lane reads its own problem's block back.  Staged for
//                           step t + 1 at the end of step t, where the whole wave is together again; dynamic LDS, sized by the launch for the
//                           most problems a wave of this L can hold.
// FL: as in so100_query_trajectory_k.
#include "so100_closed_loop.hpp"

namespace so100 {

#ifdef SO100_CL_LDS
constexpr bool CL_LDS = true;                                // a side build (tools/side_build.py): the gains through LDS
#else
constexpr bool CL_LDS = false;
#endif

struct ClosedLoopArgs {
    QueryStart start;
    const float *u, *qpos_ref, *qvel_ref, *qpos_ref0, *qvel_ref0, *k, *K;
    int nx, L; float alpha[CL_MAX_L];
    int clamp; float u_lo, u_hi;
    int mode, T, nsub; unsigned flags; int solver_iters, contact_iters;
    float* u_traj; QueryRollOut out;                         // u_traj [T][6][M L]: the controls the law made, NaN from a failed step on
};

// the most problems one wave of 64 consecutive rollouts can touch: 64 / L whole groups and, where L does not divide 64, a cut one at each end
SO100_HD constexpr int closed_loop_wave_problems(int L) { return (WG + L - 2)/L + 1; }

extern __shared__ float so100_closed_loop_lds[];

// where a lane's inputs come from (so100_closed_loop.hpp: Src)
template <bool LDS> struct ClosedLoopSrc {
    const ClosedLoopArgs& a;
    size_t M, m;                                             // problems, this lane's
    size_t m_first; int count;                               // LDS: the wave's first problem, and the words of one step's span
    __device__ void stage(int t) {
        if constexpr (LDS) {
            const float* span = a.K + ((size_t)t*M + m_first)*(size_t)(CL_NU*a.nx);
            __syncthreads();                                 // every read of the previous step's gains is done
            for (int w = (int)threadIdx.x; w < count; w += WG) so100_closed_loop_lds[w] = span[w];
            __syncthreads();
        }
    }
    __device__ void nominal(int t, float u[6], float k[6]) {
        const size_t p = (size_t)t*M + m;
#pragma unroll
        for (int j = 0; j < 6; j++) { u[j] = a.u[((size_t)t*6 + j)*M + m]; k[j] = a.k ? a.k[p*CL_NU + j] : 0.0f; }
    }
    __device__ bool starts_on_reference() { return a.qpos_ref0 == nullptr; }
    __device__ void reference(int t, bool cube, float xq[13], float xv[12]) {
        const float* q = t == 0 ? a.qpos_ref0 : a.qpos_ref + (size_t)(t - 1)*13*M;
        const float* v = t == 0 ? a.qvel_ref0 : a.qvel_ref + (size_t)(t - 1)*12*M;
#pragma unroll
        for (int i = 0; i < 13; i++) if (cube || i < 6) xq[i] = q[i*M + m];
#pragma unroll
        for (int i = 0; i < 12; i++) if (cube || i < 6) xv[i] = v[i*M + m];
    }
    __device__ float gain(int t, int j, int i) {
        if constexpr (LDS) return so100_closed_loop_lds[((int)(m - m_first)*CL_NU + j)*a.nx + i];
        else return a.K[(((size_t)t*M + m)*CL_NU + j)*(size_t)a.nx + i];
    }
};

template <int FL>
__global__ void __launch_bounds__(WG) so100_query_closed_loop_k(ClosedLoopArgs a, int M, int ML) {
    const size_t first = (size_t)blockIdx.x*WG, last = (size_t)ML - 1;
    const size_t lane = first + threadIdx.x;
    const bool live = lane < (size_t)ML;
    const size_t i = live ? lane : last;                     // a lane past the end redoes the last rollout and stores nothing
    const size_t L = (size_t)a.L, m = i/L;
    const int cand = (int)(i - m*L);
    const unsigned flags = FL >= 0 ? (unsigned)FL : a.flags;
    const size_t ml = (size_t)ML, ld = (size_t)a.start.ld;
    float qpos[13], qvel[12];
#pragma unroll
    for (int k = 0; k < 13; k++) qpos[k] = a.start.qpos[k*ld + m];
#pragma unroll
    for (int k = 0; k < 12; k++) qvel[k] = a.start.qvel ? a.start.qvel[k*ld + m] : 0.0f;
    TrajState<float> s;
    trajectory_cold(qpos, qvel, s);
    if (a.start.state) {                                     // the handle's simulation goes on: its warm starts, Kahan rows and anti-gravity bit
        const float* S = a.start.state;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            s.ff[k] = S[(SF_ff0 + k)*ld + m]; s.fl[k] = S[(SF_fl0 + k)*ld + m]; s.cube.warm[k] = S[(SF_cw0 + k)*ld + m]; s.qc[k] = S[(SF_qc0 + k)*ld + m];
            if ((flags & F_ANY_CONTACT) != 0u) s.aw[k] = S[(SF_aw0 + k)*ld + m];
        }
        if (__float_as_int(S[SF_bits*ld + m]) & B_ANTIGRAV) s.lift = (float)(so100g::CUBE_MASS*so100g::GRAVITY);
    }
    ClosedLoopLaw<float> law;
    law.alpha = 0.0f;                                        // selected, not indexed: the array is a launch argument
#pragma unroll
    for (int q = 0; q < CL_MAX_L; q++) law.alpha = cand == q ? a.alpha[q] : law.alpha;
    law.clamp = a.clamp != 0; law.u_lo = a.u_lo; law.u_hi = a.u_hi;
    const size_t m_first = first/L, m_last = (first + WG - 1 < last ? first + WG - 1 : last)/L;
    ClosedLoopSrc<CL_LDS> src{ a, (size_t)M, m, m_first, (int)(m_last - m_first + 1)*CL_NU*a.nx };
    const float nan = __int_as_float(0x7FC00000);
    const int bad = closed_loop_rollout<float>(s, a.nx, a.T, a.mode, flags, a.solver_iters, a.contact_iters, a.nsub, law, src,
        [&](int t, bool ok, const TrajState<float>& st, const TrajStep<float>& o, const float c[6]) {
            if (!live) return;
            const size_t row = (size_t)t;
            if (a.u_traj) {
#pragma unroll
                for (int k = 0; k < 6; k++) a.u_traj[(row*6 + k)*ml + i] = ok ? c[k] : nan;
            }
            if (a.out.qpos_traj || a.out.qvel_traj) {
                float qp[13], qv[12];
                trajectory_qpos_qvel(st, qp, qv);
                if (a.out.qpos_traj) {
#pragma unroll
                    for (int k = 0; k < 13; k++) a.out.qpos_traj[(row*13 + k)*ml + i] = ok ? qp[k] : nan;
                }
                if (a.out.qvel_traj) {
#pragma unroll
                    for (int k = 0; k < 12; k++) a.out.qvel_traj[(row*12 + k)*ml + i] = ok ? qv[k] : nan;
                }
            }
            if (a.out.ee_traj) {
                float ee[3] = { nan, nan, nan };
                if (ok) trajectory_ee(st.q, ee);
#pragma unroll
                for (int k = 0; k < 3; k++) a.out.ee_traj[(row*3 + k)*ml + i] = ee[k];
            }
            if (a.out.ncon) a.out.ncon[row*ml + i] = ok ? (o.cstat & 255) : 0;
            if (a.out.dropped) a.out.dropped[row*ml + i] = ok ? (o.cstat >> 8) : 0;
            if (a.out.sig) a.out.sig[row*ml + i] = ok ? o.csig : 0;
            if (a.out.residual) a.out.residual[row*ml + i] = ok ? o.res : nan;
        });
    if (!live) return;
    if (a.out.qpos_final || a.out.qvel_final) {
        float qp[13], qv[12];
        trajectory_qpos_qvel(s, qp, qv);
        if (a.out.qpos_final) {
#pragma unroll
            for (int k = 0; k < 13; k++) a.out.qpos_final[k*ml + i] = bad < 0 ? qp[k] : nan;
        }
        if (a.out.qvel_final) {
#pragma unroll
            for (int k = 0; k < 12; k++) a.out.qvel_final[k*ml + i] = bad < 0 ? qv[k] : nan;
        }
    }
    if (a.out.bad_step) a.out.bad_step[i] = bad;
}

}  // namespace so100

static_assert(SO100_CL_MAX_L == so100::CL_MAX_L, "the header names the limit");

extern "C" {

int so100_query_closed_loop(so100_sim* sim, const so100_closed_loop_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_closed_loop";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_closed_loop: null argument");
    QueryStart st;
    if (const int rc = query_start(fn, sim, io->qpos_dev, io->qvel_dev, M, st)) return rc;
    if (const int rc = query_control(fn, io->u_dev, io->mode)) return rc;
    if (const int rc = query_horizon(fn, io->T, io->nsub)) return rc;
    if (const int rc = query_solver(fn, io->flags, io->solver_iters, io->contact_iters)) return rc;
    if (io->nx != 12 && io->nx != 24) return fail(SO100_E_INVALID, "%s: nx must be 12 or 24, got %ld", fn, (long)io->nx);
    if (const int rc = query_candidates(fn, "L", "M", io->L, SO100_CL_MAX_L, M)) return rc;
    if (!io->alpha || !io->K_dev || (io->T > 1 && (!io->qpos_ref_dev || !io->qvel_ref_dev)))
        return fail(SO100_E_INVALID, "%s: alpha, K_dev and (for T > 1) qpos_ref_dev and qvel_ref_dev are required", fn);
    if (!io->qpos_ref0_dev != !io->qvel_ref0_dev) return fail(SO100_E_INVALID, "%s: qpos_ref0_dev and qvel_ref0_dev are given together or not at all", fn);
    for (int q = 0; q < io->L; q++)
        if (!(io->alpha[q]*0.0f == 0.0f)) return fail(SO100_E_INVALID, "%s: alpha[%d] must be finite, got %g", fn, q, (double)io->alpha[q]);
    if (io->clamp && (!(io->u_lo <= io->u_hi) || !((io->u_lo + io->u_hi)*0.0f == 0.0f)))
        return fail(SO100_E_INVALID, "%s: u_lo and u_hi must be finite with u_lo <= u_hi, got %g and %g", fn, (double)io->u_lo, (double)io->u_hi);
    ClosedLoopArgs a{};
    if (const int rc = query_roll_out(fn, *io, io->u_traj_dev, a.out)) return rc;
    a.start = st; a.u_traj = io->u_traj_dev;
    a.u = io->u_dev; a.qpos_ref = io->qpos_ref_dev; a.qvel_ref = io->qvel_ref_dev; a.qpos_ref0 = io->qpos_ref0_dev; a.qvel_ref0 = io->qvel_ref0_dev;
    a.k = io->k_dev; a.K = io->K_dev; a.nx = io->nx; a.L = io->L;
    for (int q = 0; q < CL_MAX_L; q++) a.alpha[q] = q < io->L ? io->alpha[q] : 0.0f;
    a.clamp = io->clamp; a.u_lo = io->u_lo; a.u_hi = io->u_hi;
    a.mode = io->mode; a.T = io->T; a.nsub = io->nsub; a.flags = io->flags; a.solver_iters = io->solver_iters; a.contact_iters = io->contact_iters;
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_closed_loop");
    const int ML = M*io->L;
    const dim3 grid((unsigned)(((size_t)ML + WG - 1)/WG)), block(WG);
    const size_t lds = CL_LDS ? (size_t)closed_loop_wave_problems(io->L)*CL_NU*(size_t)io->nx*sizeof(float) : 0;
    SO100_WITH_QUERY_FLAGS(io->flags, hipLaunchKernelGGL((so100_query_closed_loop_k<FL>), grid, block, lds, (hipStream_t)stream, a, M, ML););
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
