// so100_query_forward.hip -- the forward-dynamics query (gfx950) and its C ABI (include/so100_query.h: so100_query_forward); the arithmetic is
// in so100_forward.hpp.  Like so100_query.hip, not a translation unit of its own: so100_sim.hip includes it behind that file.
//
// Shape.  A query batch is a few hundred to a few thousand problems, and a problem with contacts runs a data-dependent Newton over its contact
// records.  One lane per problem is the wrong shape for that: a wave full of contact lanes runs at its slowest lane's pace
// through every row pass, and a private record array is 1 KB of scratch per lane.  So a QUAD of adjacent lanes holds one problem, as on the contact
// wave of the multi-wave step kernels: replicated arithmetic, the records in LDS [record][field][problem], record s owned by lane s mod 4, partial
// sums met by quad-permute DPP.  A workgroup is one wave = 16 problems: 4096 problems are 256 workgroups, one per CU; the LDS image is 16.6 KB
// (15 360 B of records + 1280 B of distances; `codes`, the list a NEXT substep would read, is written and never read here, and the compiler drops it).
// Memory.  Every array is [k][M].  The four lanes of a quad read the same word of a row (one request: 16 consecutive words per wave and row); on
// the way out row k of qacc / qfrc_constraint / pad_force is written by lane k mod 4 of the quad and slot s of the contact list by the lane that
// owns record s, so each store instruction of a wave writes 4 rows x 16 consecutive words and no value is written twice.
// Lanes past M (the last workgroup) redo problem M - 1 and store nothing: every lane reaches the barrier, every quad is whole for the DPP sums.
#include "so100_forward.hpp"

namespace so100 {

constexpr int FWD_THREADS = 64, FWD_PARTS = 4, FWD_PROBLEMS = FWD_THREADS/FWD_PARTS;

struct ForwardArgs {
    const float *qpos, *qvel, *ctrl; int ld;                 // ld: row length of qpos / qvel (M, or N for the handle's rows)
    unsigned flags; int solver_iters, contact_iters;
    float *qacc, *qfrc; int32_t *ncon, *dropped, *kind, *feat; float *pos, *frame, *dist, *force, *pad_force, *residual;
};

__global__ __launch_bounds__(FWD_THREADS) void so100_query_forward_k(ForwardArgs a, int M) {
    __shared__ float records[MAXC*CF*FWD_PROBLEMS];
    __shared__ float dists[MAXC*FWD_PROBLEMS];
    __shared__ unsigned char codes[MAXC*FWD_PROBLEMS];
    const int col = threadIdx.x/FWD_PARTS, part = threadIdx.x%FWD_PARTS;
    size_t i = (size_t)blockIdx.x*FWD_PROBLEMS + col;
    const bool live = i < (size_t)M;
    if (!live) i = (size_t)M - 1;
    float qpos[13], qvel[12], ctrl[6];
#pragma unroll
    for (int k = 0; k < 13; k++) qpos[k] = a.qpos[(size_t)k*a.ld + i];
#pragma unroll
    for (int k = 0; k < 12; k++) qvel[k] = a.qvel ? a.qvel[(size_t)k*a.ld + i] : 0.0f;
#pragma unroll
    for (int k = 0; k < 6; k++) ctrl[k] = a.ctrl ? a.ctrl[(size_t)k*M + i] : qpos[k];
    ForwardStore<float, FWD_PROBLEMS, true, FWD_PARTS> cs(records, codes, dists, col, part);
    ForwardResult<float> R;
    const size_t m = (size_t)M;
    forward_dynamics<float>(qpos, qvel, ctrl, a.flags, a.solver_iters, a.contact_iters, cs, R,
                            [&](int s, int kind, int feat, const float* p, const float* fr, float dist, const float* f) {
        if (!live) return;
        if (a.kind) a.kind[s*m + i] = kind;
        if (a.feat) a.feat[s*m + i] = feat;
        if (a.dist) a.dist[s*m + i] = dist;
        if (a.pos) {
#pragma unroll
            for (int k = 0; k < 3; k++) a.pos[(3*s + k)*m + i] = p[k];
        }
        if (a.force) {
#pragma unroll
            for (int k = 0; k < 3; k++) a.force[(3*s + k)*m + i] = f[k];
        }
        if (a.frame) {
#pragma unroll
            for (int k = 0; k < 9; k++) a.frame[(9*s + k)*m + i] = fr[k];
        }
    });
    if (!live) return;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        if (k%FWD_PARTS != part) continue;
        if (a.qacc) a.qacc[k*m + i] = R.qacc[k];
        if (a.qfrc) a.qfrc[k*m + i] = R.qfrc_constraint[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) if (k%FWD_PARTS == part && a.pad_force) a.pad_force[k*m + i] = R.pad_force[k];
    if (part == 0 && a.ncon) a.ncon[i] = R.ncon;
    if (part == 1 && a.dropped) a.dropped[i] = R.dropped;
    if (part == 2 && a.residual) a.residual[i] = R.residual;
}

}  // namespace so100

static_assert(SO100_FWD_MAXCON == so100::FWD_MAXCON, "the header names the contact list's length");
static_assert(SF_QPOS0 + 13 <= SF_COUNT && SF_QVEL0 + 12 <= SF_COUNT, "so100_get_state's rows");

extern "C" {

int so100_query_forward(so100_sim* sim, const so100_forward_io* io, int32_t M, void* stream) {
    using namespace so100;
    const char* const fn = "so100_query_forward";
    if (!sim || !io) return fail(SO100_E_INVALID, "so100_query_forward: null argument");
    QueryStart st;
    if (const int rc = query_start(fn, sim, io->qpos_dev, io->qvel_dev, M, st)) return rc;
    if (const int rc = query_solver(fn, io->flags, io->solver_iters, io->contact_iters)) return rc;
    if (!io->qacc_dev && !io->qfrc_constraint_dev && !io->ncon_dev && !io->dropped_dev && !io->con_kind_dev && !io->con_feat_dev && !io->con_pos_dev &&
        !io->con_frame_dev && !io->con_dist_dev && !io->con_force_dev && !io->pad_force_dev && !io->residual_dev)
        return fail(SO100_E_INVALID, "%s: no output requested", fn);
    ForwardArgs a{};
    a.qpos = st.qpos; a.qvel = st.qvel; a.ld = st.ld;
    a.ctrl = io->ctrl_dev; a.flags = io->flags; a.solver_iters = io->solver_iters; a.contact_iters = io->contact_iters;
    a.qacc = io->qacc_dev; a.qfrc = io->qfrc_constraint_dev; a.ncon = io->ncon_dev; a.dropped = io->dropped_dev; a.kind = io->con_kind_dev; a.feat = io->con_feat_dev;
    a.pos = io->con_pos_dev; a.frame = io->con_frame_dev; a.dist = io->con_dist_dev; a.force = io->con_force_dev; a.pad_force = io->pad_force_dev;
    a.residual = io->residual_dev;
    SO100_ON_DEVICE(sim->cfg.device, "so100_query_forward");
    hipLaunchKernelGGL(so100_query_forward_k, dim3((unsigned)((M + FWD_PROBLEMS - 1)/FWD_PROBLEMS)), dim3(FWD_THREADS), 0, (hipStream_t)stream, a, M);
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

}  // extern "C"
