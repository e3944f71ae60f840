// so100_query_derivative.hip -- the derivatives query (gfx950) and its C ABI (include/so100_query.h: so100_query_derivatives); the arithmetic
// is in so100_derivative.hpp.  Like so100_query_trajectory.hip, not a translation unit of its own: so100_sim.hip includes it behind that file.
//
// Shape: one workgroup is one wave is one problem (blockIdx.x).  Lane 2c evaluates column c at +eps, lane 2c + 1 at -eps (c in 0..29), lanes
// 60..63 the unperturbed problem: 61 evaluations of trajectory_step side by side, a hair apart, so the lanes of a wave take the same branches
// and the same iteration counts.  The +- pair of a column sits in neighbouring lanes: the difference is one quad-permute DPP exchange per
// component (quad_xor1), no LDS, no barrier.  Every loop has a fixed bound (nsub, the iteration counts).
// Memory.  The start and the controls are wave-uniform, indexed by blockIdx.x alone (scalar loads).  A [M][24][24] and B [M][24][6] are
// problem-major, row-major -- the one exception to the SoA rule, because a wave owns a problem: for a fixed row the even lanes of columns
// 0..23 store 24 consecutive words of A, those of columns 24..29 6 consecutive words of B.  qpos_next [13][M], qvel_next [12][M] and bad [M]
// keep the SoA layout and are written by lane 60.
// FL: so100_query_trajectory_k's forms and dispatch rule.
#include "so100_derivative.hpp"

namespace so100 {

struct DerivativeArgs {
    QueryStart start;
    const float* ctrl;
    int mode, nsub; unsigned flags; int solver_iters, contact_iters;
    float eps, r;                                            // r = 1/(2 eps), formed once on the host
    float *A, *B, *qpos_next, *qvel_next; int32_t* bad;
};

template <int FL>
__global__ void __launch_bounds__(64) so100_query_derivative_k(DerivativeArgs a, int M) {
    const size_t i = blockIdx.x;                             // the problem: wave-uniform
    const int lane = (int)threadIdx.x;                       // the role
    const unsigned flags = FL >= 0 ? (unsigned)FL : a.flags;
    const size_t m = (size_t)M, ld = (size_t)a.start.ld;
    float qpos[13], qvel[12], c[6];
#pragma unroll
    for (int k = 0; k < 13; k++) qpos[k] = a.start.qpos[k*ld + i];
#pragma unroll
    for (int k = 0; k < 12; k++) qvel[k] = a.start.qvel ? a.start.qvel[k*ld + i] : 0.0f;
#pragma unroll
    for (int k = 0; k < 6; k++) c[k] = a.ctrl[k*m + i];
    TrajState<float> s;
    trajectory_cold(qpos, qvel, s);
    if (a.start.state) {                                     // every lane reads the same warm starts, Kahan rows and anti-gravity bit
        const float* S = a.start.state;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            s.ff[k] = S[(SF_ff0 + k)*ld + i]; s.fl[k] = S[(SF_fl0 + k)*ld + i]; s.cube.warm[k] = S[(SF_cw0 + k)*ld + i]; s.qc[k] = S[(SF_qc0 + k)*ld + i];
            if ((flags & F_ANY_CONTACT) != 0u) s.aw[k] = S[(SF_aw0 + k)*ld + i];
        }
        if (__float_as_int(S[SF_bits*ld + i]) & B_ANTIGRAV) s.lift = (float)(so100g::CUBE_MASS*so100g::GRAVITY);
    }
    float qp[13], qv[12];
    const bool ok = derivative_evaluate<float>(lane, a.eps, s, c, a.mode, flags, a.solver_iters, a.contact_iters, a.nsub, qp, qv);
    // all 64 lanes are here again: the problem is bad where any of its evaluations is
    const bool bad = __builtin_amdgcn_ballot_w64(!ok) != 0ull;
    const float nan = __int_as_float(0x7FC00000);
    if (a.A || a.B) {
        float qo[13], vo[12];                                // the neighbour's next state: lanes 2c <-> 2c + 1
#pragma unroll
        for (int k = 0; k < 13; k++) qo[k] = quad_xor1(qp[k]);
#pragma unroll
        for (int k = 0; k < 12; k++) vo[k] = quad_xor1(qv[k]);
        float col[DERIV_NX];
        derivative_column(qp, qv, qo, vo, a.r, col);           // in an even lane: own = +eps, neighbour = -eps
        const int cidx = lane >> 1;
        if ((lane & 1) == 0 && cidx < DERIV_NX && a.A) {
            float* A = a.A + i*(size_t)(DERIV_NX*DERIV_NX) + cidx;
#pragma unroll
            for (int r = 0; r < DERIV_NX; r++) A[r*DERIV_NX] = bad ? nan : col[r];
        }
        if ((lane & 1) == 0 && cidx >= DERIV_NX && cidx < DERIV_COLS && a.B) {
            float* B = a.B + i*(size_t)(DERIV_NX*DERIV_NU) + (cidx - DERIV_NX);
#pragma unroll
            for (int r = 0; r < DERIV_NX; r++) B[r*DERIV_NU] = bad ? nan : col[r];
        }
    }
    if (lane == DERIV_NOMINAL) {
        if (a.qpos_next) {
#pragma unroll
            for (int k = 0; k < 13; k++) a.qpos_next[k*m + i] = bad ? nan : qp[k];
        }
        if (a.qvel_next) {
#pragma unroll
            for (int k = 0; k < 12; k++) a.qvel_next[k*m + i] = bad ? nan : qv[k];
        }
        if (a.bad) a.bad[i] = bad ? 1 : 0;
    }
}

}  // namespace so100

static_assert(SO100_DERIV_NX == so100::DERIV_NX && SO100_DERIV_NU == so100::DERIV_NU && SO100_DERIV_EPS == so100::DERIV_EPS, "the header names the sizes and the default step");
static_assert(so100::DERIV_NOMINAL + 1 <= 64, "61 roles in one wave");

extern "C" {

int so100_query_derivatives(so100_sim* sim, const so100_derivatives_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_derivatives";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_derivatives: null argument");
    QueryStart st;
    if (const int rc = query_start(fn, sim, io->qpos_dev, io->qvel_dev, M, st)) return rc;
    if (const int rc = query_control(fn, io->ctrl_dev, io->mode)) return rc;
    if (io->nsub < 1 || io->nsub > SO100_TRAJ_MAX_NSUB)
        return fail(SO100_E_INVALID, "%s: nsub must be in 1..%d, got %ld", fn, SO100_TRAJ_MAX_NSUB, (long)io->nsub);
    if (const int rc = query_solver(fn, io->flags, io->solver_iters, io->contact_iters)) return rc;
    if (!(io->eps > 0.0f) || !(io->eps*0.0f == 0.0f)) return fail(SO100_E_INVALID, "%s: eps must be finite and > 0, got %g", fn, (double)io->eps);
    if (!io->A_dev && !io->B_dev && !io->qpos_next_dev && !io->qvel_next_dev && !io->bad_dev) return fail(SO100_E_INVALID, "%s: no output requested", fn);
    DerivativeArgs a{};
    a.start = st;
    a.ctrl = io->ctrl_dev; a.mode = io->mode; a.nsub = io->nsub; a.flags = io->flags; a.solver_iters = io->solver_iters; a.contact_iters = io->contact_iters;
    a.eps = io->eps; a.r = 0.5f/io->eps;
    a.A = io->A_dev; a.B = io->B_dev; a.qpos_next = io->qpos_next_dev; a.qvel_next = io->qvel_next_dev; a.bad = io->bad_dev;
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_derivatives");
    const dim3 grid((unsigned)M), block(64);                 // one wave per problem
    SO100_WITH_QUERY_FLAGS(io->flags, hipLaunchKernelGGL((so100_query_derivative_k<FL>), grid, block, 0, (hipStream_t)stream, a, M););
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
