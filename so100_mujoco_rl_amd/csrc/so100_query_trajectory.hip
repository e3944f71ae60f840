// so100_query_trajectory.hip -- the trajectory query (gfx950) and its C ABI (include/so100_query.h: so100_query_trajectory); the arithmetic is
// in so100_trajectory.hpp.  Like so100_query_forward.hip, not a translation unit of its own: so100_sim.hip includes it behind that file.
//
// Shape: so100_step_fused's.  One lane per problem, one wave per workgroup; the problem's physics rows stay in registers for all T x nsub
// substeps, so HBM sees the start once, one control row per step and the rows the caller asked for.  A lane at or past M returns at once;
// there is no LDS and no barrier, so no lane waits on another, and every loop has a fixed bound (T, nsub, the iteration counts).
// Memory.  Every array is [k][M] (ctrl and the trajectories: [T][k][M]): lane i of a wave touches word i of a row, one coalesced segment
// per wave and row.
// FL >= 0: the flags are a compile-time constant (so100_step_fused's FL), for the sets without arm contact (8, 11 and F_NOPADS = 7); FL < 0: decided at
// run time.
#include "so100_trajectory.hpp"

namespace so100 {

struct TrajectoryArgs {
    QueryStart start;
    const float* ctrl;
    int mode, T, nsub; unsigned flags; int solver_iters, contact_iters;
    QueryRollOut out;
};

template <int FL>
__global__ void __launch_bounds__(WG) so100_query_trajectory_k(TrajectoryArgs a, int M) {
    const size_t i = (size_t)blockIdx.x*WG + threadIdx.x;
    if (i >= (size_t)M) return;
    const unsigned flags = FL >= 0 ? (unsigned)FL : a.flags;
    const size_t m = (size_t)M, ld = (size_t)a.start.ld;
    float qpos[13], qvel[12];
#pragma unroll
    for (int k = 0; k < 13; k++) qpos[k] = a.start.qpos[k*ld + i];
#pragma unroll
    for (int k = 0; k < 12; k++) qvel[k] = a.start.qvel ? a.start.qvel[k*ld + i] : 0.0f;
    TrajState<float> s;
    trajectory_cold(qpos, qvel, s);
    if (a.start.state) {
        const float* S = a.start.state;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            s.ff[k] = S[(SF_ff0 + k)*ld + i]; s.fl[k] = S[(SF_fl0 + k)*ld + i]; s.cube.warm[k] = S[(SF_cw0 + k)*ld + i]; s.qc[k] = S[(SF_qc0 + k)*ld + i];
            if ((flags & F_ANY_CONTACT) != 0u) s.aw[k] = S[(SF_aw0 + k)*ld + i];
        }
        if (__float_as_int(S[SF_bits*ld + i]) & B_ANTIGRAV) s.lift = (float)(so100g::CUBE_MASS*so100g::GRAVITY);
    }
    const float nan = __int_as_float(0x7FC00000);
    const int bad = trajectory_rollout<float>(s, a.T, a.mode, flags, a.solver_iters, a.contact_iters, a.nsub,
        [&](int t, float c[6]) {
#pragma unroll
            for (int k = 0; k < 6; k++) c[k] = a.ctrl[((size_t)t*6 + k)*m + i];
        },
        [&](int t, bool ok, const TrajState<float>& st, const TrajStep<float>& o) {
            const size_t row = (size_t)t;
            if (a.out.qpos_traj || a.out.qvel_traj) {
                float qp[13], qv[12];
                trajectory_qpos_qvel(st, qp, qv);
                if (a.out.qpos_traj) {
#pragma unroll
                    for (int k = 0; k < 13; k++) a.out.qpos_traj[(row*13 + k)*m + i] = ok ? qp[k] : nan;
                }
                if (a.out.qvel_traj) {
#pragma unroll
                    for (int k = 0; k < 12; k++) a.out.qvel_traj[(row*12 + k)*m + i] = ok ? qv[k] : nan;
                }
            }
            if (a.out.ee_traj) {
                float ee[3] = { nan, nan, nan };
                if (ok) trajectory_ee(st.q, ee);
#pragma unroll
                for (int k = 0; k < 3; k++) a.out.ee_traj[(row*3 + k)*m + i] = ee[k];
            }
            if (a.out.ncon) a.out.ncon[row*m + i] = ok ? (o.cstat & 255) : 0;
            if (a.out.dropped) a.out.dropped[row*m + i] = ok ? (o.cstat >> 8) : 0;
            if (a.out.sig) a.out.sig[row*m + i] = ok ? o.csig : 0;
            if (a.out.residual) a.out.residual[row*m + i] = ok ? o.res : nan;
        });
    if (a.out.qpos_final || a.out.qvel_final) {
        float qp[13], qv[12];
        trajectory_qpos_qvel(s, qp, qv);
        if (a.out.qpos_final) {
#pragma unroll
            for (int k = 0; k < 13; k++) a.out.qpos_final[k*m + i] = bad < 0 ? qp[k] : nan;
        }
        if (a.out.qvel_final) {
#pragma unroll
            for (int k = 0; k < 12; k++) a.out.qvel_final[k*m + i] = bad < 0 ? qv[k] : nan;
        }
    }
    if (a.out.bad_step) a.out.bad_step[i] = bad;
}

}  // namespace so100

static_assert(SO100_TRAJ_TARGETS == so100::TRAJ_TARGETS && SO100_TRAJ_ACTIONS == so100::TRAJ_ACTIONS, "the header names the modes");
static_assert(SO100_TRAJ_MAX_T == so100::TRAJ_MAX_T && SO100_TRAJ_MAX_NSUB == so100::TRAJ_MAX_NSUB && SO100_TRAJ_MAX_SUBSTEPS == so100::TRAJ_MAX_SUBSTEPS,
              "the header names the limits");
static_assert(so100::TRAJ_ACTION_SCALE == so100::JOINT_STEP_SCALE, "actions mode is the reach envs' control law");

extern "C" {

int so100_query_trajectory(so100_sim* sim, const so100_trajectory_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_trajectory";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_trajectory: null argument");
    QueryStart st;
    if (const int rc = query_start(fn, sim, io->qpos_dev, io->qvel_dev, M, st)) return rc;
    if (const int rc = query_control(fn, io->ctrl_dev, io->mode)) return rc;
    if (const int rc = query_horizon(fn, io->T, io->nsub)) return rc;
    if (const int rc = query_solver(fn, io->flags, io->solver_iters, io->contact_iters)) return rc;
    TrajectoryArgs a{};
    if (const int rc = query_roll_out(fn, *io, nullptr, a.out)) return rc;
    a.start = st;
    a.ctrl = io->ctrl_dev; a.mode = io->mode; a.T = io->T; a.nsub = io->nsub; a.flags = io->flags; a.solver_iters = io->solver_iters; a.contact_iters = io->contact_iters;
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_trajectory");
    const dim3 grid((unsigned)(((size_t)M + WG - 1)/WG)), block(WG);
    SO100_WITH_QUERY_FLAGS(io->flags, hipLaunchKernelGGL((so100_query_trajectory_k<FL>), grid, block, 0, (hipStream_t)stream, a, M););
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
