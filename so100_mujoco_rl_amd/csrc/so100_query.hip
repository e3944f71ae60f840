// so100_query.hip -- the four query kernels (gfx950) and their C ABI (include/so100_query.h); the arithmetic is in so100_query.hpp.
// One lane per problem, any M >= 1.  Every load and store is a row of a component-major array: lane i of a wave touches word i of the
// row, so a wave's access is one contiguous 256-byte segment.  The kernels only READ the handle's state matrix.
// Workgroups of one wave: the kernels have no LDS and no barrier, so a larger workgroup would share nothing; with 64 lanes a batch of
// a few thousand problems is spread over that many more CUs (the latency of one lane's chain is what a small batch pays), and
// __launch_bounds__(64) leaves the register allocator the whole budget of a lane (no scratch memory).
// Not a translation unit of its own: so100_sim.hip includes this file at its end (the handle, the host layer and the state rows are
// in scope there), so the kernels below are part of so100_sim.o.
#include <cmath>
#include "so100_query.hpp"
#include "../../include/so100_query.h"

namespace so100 {

constexpr int QUERY_THREADS = 64;

struct QueryPoint { int link; float o[3]; };
struct QueryKinOut { float *xpos, *xmat, *ee, *cam_pos, *cam_mat; };
struct QueryDynIO { const float *v, *qacc; float *M, *bias, *tau; };
struct QueryIkIO { const float* target; int iters; float damping2, tol, max_step; float *q, *residual; int32_t* iterations; uint8_t* converged; };

// rows: k consecutive rows of `ld` words; lane i reads / writes word i of each
template <int K> __device__ __forceinline__ void load_rows(const float* p, size_t ld, size_t i, float x[K]) {
#pragma unroll
    for (int j = 0; j < K; j++) x[j] = p[(size_t)j*ld + i];
}
template <int K> __device__ __forceinline__ void store_rows(float* p, size_t ld, size_t i, const float x[K]) {
#pragma unroll
    for (int j = 0; j < K; j++) p[(size_t)j*ld + i] = x[j];
}

// q: [6][ld] (ld = M for the caller's array, N for rows q0..q5 of the state matrix); every output [k][M]
__global__ __launch_bounds__(QUERY_THREADS) void so100_query_kinematics_k(const float* __restrict__ q, int ld, int M, QueryKinOut o) {
    const size_t i = (size_t)blockIdx.x*QUERY_THREADS + threadIdx.x;
    if (i >= (size_t)M) return;
    float qi[6];
    load_rows<6>(q, (size_t)ld, i, qi);
    QueryPoses<float> Q;
    query_kinematics<float>(qi, Q);
    if (o.xpos) store_rows<18>(o.xpos, (size_t)M, i, &Q.F.pos[0][0]);
    if (o.xmat) store_rows<54>(o.xmat, (size_t)M, i, &Q.F.R[0][0]);
    if (o.ee) store_rows<3>(o.ee, (size_t)M, i, Q.ee);
    if (o.cam_pos) store_rows<3>(o.cam_pos, (size_t)M, i, Q.cam_pos);
    if (o.cam_mat) store_rows<9>(o.cam_mat, (size_t)M, i, Q.cam_mat);
}

__global__ __launch_bounds__(QUERY_THREADS) void so100_query_jacobian_k(const float* __restrict__ q, int ld, int M, QueryPoint pt,
                                                                        float* __restrict__ jacp, float* __restrict__ jacr) {
    const size_t i = (size_t)blockIdx.x*QUERY_THREADS + threadIdx.x;
    if (i >= (size_t)M) return;
    float qi[6], jp[18], jr[18];
    load_rows<6>(q, (size_t)ld, i, qi);
    query_jacobian<float>(qi, pt.link, pt.o, jp, jr);
    if (jacp) store_rows<18>(jacp, (size_t)M, i, jp);
    if (jacr) store_rows<18>(jacr, (size_t)M, i, jr);
}

// v: [6][ldv] or null (zero); qacc: [6][M] or null
__global__ __launch_bounds__(QUERY_THREADS) void so100_query_dynamics_k(const float* __restrict__ q, int ld, int ldv, int M, QueryDynIO io) {
    const size_t i = (size_t)blockIdx.x*QUERY_THREADS + threadIdx.x;
    if (i >= (size_t)M) return;
    float qi[6], vi[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, ai[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, Mf[36], bias[6], tau[6];
    load_rows<6>(q, (size_t)ld, i, qi);
    if (io.v) load_rows<6>(io.v, (size_t)ldv, i, vi);
    if (io.qacc) load_rows<6>(io.qacc, (size_t)M, i, ai);
    query_dynamics<float>(qi, vi, ai, Mf, bias, tau);
    if (io.M) store_rows<36>(io.M, (size_t)M, i, Mf);
    if (io.bias) store_rows<6>(io.bias, (size_t)M, i, bias);
    if (io.tau && io.qacc) store_rows<6>(io.tau, (size_t)M, i, tau);
}

// q0 and io.q may be the same array: a lane reads its column before it writes it, and no lane touches another's
__global__ __launch_bounds__(QUERY_THREADS) void so100_query_ik_k(const float* q0, int ld, int M, QueryPoint pt, QueryIkIO io) {
    const size_t i = (size_t)blockIdx.x*QUERY_THREADS + threadIdx.x;
    if (i >= (size_t)M) return;
    float qi[6], tg[3];
    load_rows<6>(q0, (size_t)ld, i, qi);
    load_rows<3>(io.target, (size_t)M, i, tg);
    IkParams<float> P;
    P.link = pt.link; P.iters = io.iters; P.o[0] = pt.o[0]; P.o[1] = pt.o[1]; P.o[2] = pt.o[2];
    P.damping2 = io.damping2; P.tol = io.tol; P.max_step = io.max_step;
    IkResult<float> R;
    query_ik<float>(qi, tg, P, R);
    if (io.q) store_rows<6>(io.q, (size_t)M, i, R.q);
    if (io.residual) io.residual[i] = R.residual;
    if (io.iterations) io.iterations[i] = R.iterations;
    if (io.converged) io.converged[i] = R.converged ? 1 : 0;
}

// forward, trajectory, derivatives and closed loop start from a whole state: the caller's rows (qvel may be null: zero), or the handle's
// so100_get_state rows, their row length ld = N and the state matrix itself (what a simulation that goes on reads beside qpos and qvel; else null).
// The rollout kernels' argument structs begin with one (filled by query_start below).
struct QueryStart { const float *qpos, *qvel; int ld; const float* state; };

// the trajectory-shaped outputs of a rollout kernel, each [T][k][stride] (the finals [k][stride], bad_step [stride]) or null (filled and checked by
// query_roll_out below); a rollout writes word `col` of every row
struct QueryRollOut {
    float *qpos_traj, *qvel_traj, *ee_traj, *qpos_final, *qvel_final;
    int32_t *ncon, *dropped, *sig; float* residual; int32_t* bad_step;
};

namespace {

// The checks the entries share (this file's and those of the files so100_sim.hip includes behind it).  Each returns fail()'s code or 0; an entry
// calls them in the order of its own checks, with what only it checks in between, so the first error of a call is the one its header names.

// the batch size of every query; reads_state: the caller gave no start of its own, so the problems are the handle's N envs
int query_batch(const char* fn, const so100_sim* s, bool reads_state, int32_t M) {
    const int n = s->prm.n;
    if (M < 1) return fail(SO100_E_INVALID, "%s: M must be >= 1, got %ld", fn, (long)M);
    if (reads_state && M != n) return fail(SO100_E_INVALID, "%s: M must be the handle's N (%ld) where its state is read, got %ld", fn, (long)n, (long)M);
    return 0;
}
// the four original queries start from joint rows (the caller's, or the state matrix's) and their row length
struct QuerySource { const float* q; int ld; };
int query_source(const char* fn, const so100_sim* s, const float* q_dev, int32_t M, QuerySource& src) {
    if (const int rc = query_batch(fn, s, !q_dev, M)) return rc;
    src.q = q_dev ? q_dev : s->state + (size_t)SF_q0*(size_t)s->prm.n;
    src.ld = q_dev ? M : s->prm.n;
    return 0;
}
int query_start(const char* fn, const so100_sim* s, const float* qpos_dev, const float* qvel_dev, int32_t M, QueryStart& st) {
    if (const int rc = query_batch(fn, s, !qpos_dev && !qvel_dev, M)) return rc;
    if (!qpos_dev && qvel_dev) return fail(SO100_E_INVALID, "%s: qvel_dev given without qpos_dev", fn);
    const size_t n = (size_t)s->prm.n;
    if (qpos_dev) st = { qpos_dev, qvel_dev, M, nullptr };
    else st = { s->state + (size_t)SF_QPOS0*n, s->state + (size_t)SF_QVEL0*n, s->prm.n, s->state };
    return 0;
}
// the horizon of the trajectory and closed-loop entries
int query_horizon(const char* fn, int32_t T, int32_t nsub) {
    if (T < 1 || T > SO100_TRAJ_MAX_T || nsub < 1 || nsub > SO100_TRAJ_MAX_NSUB || (long)T*(long)nsub > SO100_TRAJ_MAX_SUBSTEPS)
        return fail(SO100_E_INVALID, "%s: T must be in 1..%d, nsub in 1..%d and T * nsub <= %d, got T = %ld, nsub = %ld", fn, SO100_TRAJ_MAX_T, SO100_TRAJ_MAX_NSUB,
                    SO100_TRAJ_MAX_SUBSTEPS, (long)T, (long)nsub);
    return 0;
}
// the steps of an entry without substeps of its own (limit: SO100_LQR_MAX_T or SO100_TRAJ_MAX_T)
int query_steps(const char* fn, int32_t T, int limit) {
    if (T < 1 || T > limit) return fail(SO100_E_INVALID, "%s: T must be in 1..%d, got %ld", fn, limit, (long)T);
    return 0;
}
// the regulariser's range and its factor up (so100_query_lqr_reg, so100_query_reg_schedule)
int query_reg_range(const char* fn, float reg_min, float reg_max, float reg_up) {
    if (!(reg_min > 0.0f) || !std::isfinite(reg_min)) return fail(SO100_E_INVALID, "%s: reg_min must be finite and > 0, got %g", fn, (double)reg_min);
    if (!(reg_max >= reg_min) || !std::isfinite(reg_max)) return fail(SO100_E_INVALID, "%s: reg_max must be finite and >= reg_min, got %g", fn, (double)reg_max);
    if (!(reg_up > 1.0f) || !std::isfinite(reg_up)) return fail(SO100_E_INVALID, "%s: reg_up must be finite and > 1, got %g", fn, (double)reg_up);
    return 0;
}
// the candidates of each problem: `count` of them (named c: "L" or "K") for each of `batch` problems (named b: "M" or "N"); every rollout has an int32 index
int query_candidates(const char* fn, const char* c, const char* b, int32_t count, int limit, int32_t batch) {
    if (count < 1 || count > limit || (long long)batch*(long long)count > (long long)INT32_MAX)
        return fail(SO100_E_INVALID, "%s: %s must be in 1..%d and %s * %s <= %ld, got %s = %ld, %s = %ld", fn, c, limit, b, c, (long)INT32_MAX, c, (long)count, b, (long)batch);
    return 0;
}
// the trajectory-shaped outputs of an io struct (so100_trajectory_io, so100_closed_loop_io); also: an output the entry has beside them, or null
template <typename IO> int query_roll_out(const char* fn, const IO& io, const void* also, QueryRollOut& o) {
    o = { io.qpos_traj_dev, io.qvel_traj_dev, io.ee_traj_dev, io.qpos_final_dev, io.qvel_final_dev, io.ncon_dev, io.dropped_dev, io.sig_dev, io.residual_dev, io.bad_step_dev };
    if (!also && !o.qpos_traj && !o.qvel_traj && !o.ee_traj && !o.qpos_final && !o.qvel_final && !o.ncon && !o.dropped && !o.sig && !o.residual && !o.bad_step)
        return fail(SO100_E_INVALID, "%s: no output requested", fn);
    return 0;
}
int query_control(const char* fn, const float* ctrl_dev, int32_t mode) {
    if (!ctrl_dev) return fail(SO100_E_INVALID, "%s: ctrl_dev is required", fn);
    if (mode != SO100_TRAJ_TARGETS && mode != SO100_TRAJ_ACTIONS) return fail(SO100_E_INVALID, "%s: unknown mode %ld", fn, (long)mode);
    return 0;
}
constexpr uint32_t QUERY_FLAGS = SO100_F_FRICTIONLOSS | SO100_F_LIMITS | SO100_F_FLOOR | SO100_F_CUBE_PINNED | SO100_F_PADS_FLOOR | SO100_F_PADS_CUBE |
                                 SO100_F_LINKS_FLOOR | SO100_F_LINKS_CUBE;
int query_solver(const char* fn, uint32_t flags, int32_t solver_iters, int32_t contact_iters) {
    if (flags & ~QUERY_FLAGS) return fail(SO100_E_INVALID, "%s: unknown flag bits", fn);
    if ((flags & (SO100_F_PADS_CUBE | SO100_F_LINKS_CUBE)) && (flags & SO100_F_CUBE_PINNED))
        return fail(SO100_E_INVALID, "%s: SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)", fn);
    if (solver_iters < 1 || solver_iters > 64) return fail(SO100_E_INVALID, "%s: solver_iters must be in 1..64, got %ld", fn, (long)solver_iters);
    if (contact_iters < 1 || contact_iters > 64) return fail(SO100_E_INVALID, "%s: contact_iters must be in 1..64, got %ld", fn, (long)contact_iters);
    return 0;
}
// The flag sets without arm contact that the trajectory and derivatives kernels are also compiled for (their FL): SO100_WITH_QUERY_FLAGS(flags, body)
// runs `body` with constexpr int FL = that set where `flags` is one of them, else -1 (flags decided at run time), as SO100_WITH_OBS_DIM does with OD.
constexpr uint32_t QUERY_FL_FREE = SO100_F_CUBE_PINNED, QUERY_FL_ROWS = SO100_F_FRICTIONLOSS | SO100_F_LIMITS | SO100_F_CUBE_PINNED,
                   QUERY_FL_NOPADS = SO100_F_FRICTIONLOSS | SO100_F_LIMITS | SO100_F_FLOOR;
#define SO100_WITH_QUERY_FLAGS(flags, ...) do { \
    if ((flags) == QUERY_FL_FREE) { constexpr int FL = (int)QUERY_FL_FREE; __VA_ARGS__ } \
    else if ((flags) == QUERY_FL_ROWS) { constexpr int FL = (int)QUERY_FL_ROWS; __VA_ARGS__ } \
    else if ((flags) == QUERY_FL_NOPADS) { constexpr int FL = (int)QUERY_FL_NOPADS; __VA_ARGS__ } \
    else { constexpr int FL = -1; __VA_ARGS__ } } while (0)
int query_point(const char* fn, int32_t link, const float* offset, QueryPoint& pt) {
    if (link < 0 || link > 5) return fail(SO100_E_INVALID, "%s: link must be in 0..5, got %ld", fn, (long)link);
    pt.link = link;
    for (int i = 0; i < 3; i++) pt.o[i] = offset ? offset[i] : (link == EE_LINK ? (float)EE_OFFSET[i] : 0.0f);
    return 0;
}
unsigned query_grid(int M) { return (unsigned)((M + QUERY_THREADS - 1)/QUERY_THREADS); }

}  // namespace
}  // namespace so100

static_assert(SF_q5 == SF_q0 + 5 && SF_v5 == SF_v0 + 5, "the arm's qpos / qvel rows are contiguous");
static_assert(SO100_EE_LINK == EE_LINK, "the header names the same end-effector point");
static_assert(SF_ff0 + 5 == SF_ff5 && SF_fl0 + 5 == SF_fl5 && SF_cw0 + 5 == SF_cw5 && SF_qc0 + 5 == SF_qc5 && SF_aw0 + 5 == SF_aw5, "six consecutive rows each");

extern "C" {

int so100_query_kinematics(so100_sim* sim, const so100_kinematics_io* io, int32_t M, void* stream) {
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_kinematics: null argument");
    QuerySource src;
    if (const int rc = query_source("so100_query_kinematics", sim, io->q_dev, M, src)) return rc;
    if (!io->xpos_dev && !io->xmat_dev && !io->ee_dev && !io->cam_pos_dev && !io->cam_mat_dev)
        return fail(SO100_E_INVALID, "so100_query_kinematics: no output requested");
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_kinematics");
    const QueryKinOut o{ io->xpos_dev, io->xmat_dev, io->ee_dev, io->cam_pos_dev, io->cam_mat_dev };
    hipLaunchKernelGGL(so100_query_kinematics_k, dim3(query_grid(M)), dim3(QUERY_THREADS), 0, (hipStream_t)stream, src.q, src.ld, M, o);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

int so100_query_jacobian(so100_sim* sim, const so100_jacobian_io* io, int32_t M, void* stream) {
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_jacobian: null argument");
    QuerySource src;
    QueryPoint pt;
    if (const int rc = query_source("so100_query_jacobian", sim, io->q_dev, M, src)) return rc;
    if (const int rc = query_point("so100_query_jacobian", io->link, io->offset, pt)) return rc;
    if (!io->jacp_dev && !io->jacr_dev) return fail(SO100_E_INVALID, "so100_query_jacobian: no output requested");
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_jacobian");
    hipLaunchKernelGGL(so100_query_jacobian_k, dim3(query_grid(M)), dim3(QUERY_THREADS), 0, (hipStream_t)stream, src.q, src.ld, M, pt, io->jacp_dev, io->jacr_dev);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

int so100_query_dynamics(so100_sim* sim, const so100_dynamics_io* io, int32_t M, void* stream) {
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_dynamics: null argument");
    QuerySource src;
    if (const int rc = query_source("so100_query_dynamics", sim, io->q_dev, M, src)) return rc;
    if (!io->M_dev && !io->bias_dev && !(io->tau_dev && io->qacc_dev)) return fail(SO100_E_INVALID, "so100_query_dynamics: no output requested");
    QueryDynIO d{ io->v_dev, io->qacc_dev, io->M_dev, io->bias_dev, io->tau_dev };
    int ldv = M;
    if (!io->q_dev && !io->v_dev) { d.v = sim->state + (size_t)SF_v0*(size_t)sim->prm.n; ldv = sim->prm.n; }       // the handle's state: its qvel too
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_dynamics");
    hipLaunchKernelGGL(so100_query_dynamics_k, dim3(query_grid(M)), dim3(QUERY_THREADS), 0, (hipStream_t)stream, src.q, src.ld, ldv, M, d);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

int so100_query_ik(so100_sim* sim, const so100_ik_io* io, int32_t M, void* stream) {
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_ik: null argument");
    QuerySource src;
    QueryPoint pt;
    if (const int rc = query_source("so100_query_ik", sim, io->q0_dev, M, src)) return rc;
    if (const int rc = query_point("so100_query_ik", io->link, io->offset, pt)) return rc;
    if (io->iters < 1 || io->iters > 1024) return fail(SO100_E_INVALID, "so100_query_ik: iters must be in 1..1024, got %ld", (long)io->iters);
    if (!(io->damping > 0.0f) || !std::isfinite(io->damping)) return fail(SO100_E_INVALID, "so100_query_ik: damping must be > 0");
    if (!(io->tol > 0.0f) || !std::isfinite(io->tol)) return fail(SO100_E_INVALID, "so100_query_ik: tol must be > 0");
    if (!(io->max_step > 0.0f) || !std::isfinite(io->max_step)) return fail(SO100_E_INVALID, "so100_query_ik: max_step must be > 0");
    if (!io->target_dev) return fail(SO100_E_INVALID, "so100_query_ik: target_dev is required");
    if (!io->q_dev && !io->residual_dev && !io->iterations_dev && !io->converged_dev) return fail(SO100_E_INVALID, "so100_query_ik: no output requested");
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_ik");
    const QueryIkIO k{ io->target_dev, io->iters, io->damping*io->damping, io->tol, io->max_step, io->q_dev, io->residual_dev, io->iterations_dev, io->converged_dev };
    hipLaunchKernelGGL(so100_query_ik_k, dim3(query_grid(M)), dim3(QUERY_THREADS), 0, (hipStream_t)stream, src.q, src.ld, M, pt, k);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
