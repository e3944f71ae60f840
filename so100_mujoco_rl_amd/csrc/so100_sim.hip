// so100_sim.hip -- the C ABI of libso100sim.so (include/so100_sim.h).  The kernels live in so100_kernels.hpp; their per-kind
// instantiations are compiled in so100_kind.hip (one object per env kind), this file only dispatches to them.
#include "so100_kernels.hpp"
#include "so100_balance.hpp"
#include "so100_render.hpp"
#include "so100_policy_tensors.h"
#include "so100_host.hpp"

namespace so100 {
extern template struct KindOps<1>; extern template struct KindOps<2>; extern template struct KindOps<3>;
extern template struct KindOps<4>; extern template struct KindOps<5>; extern template struct KindOps<6>;
}

namespace {

using namespace so100;

const char* const kFieldNames[] = {
#define X(name, member, kind, group) #name,
    SO100_STATE_FIELDS(X)
#undef X
};

#include "so100_start_positions.inc"

}  // namespace

struct so100_sim {
    so100_config cfg;
    SimParams prm;
    float* state = nullptr;        // [SF_COUNT][N]
    float* start_tab = nullptr;    // [36][6]
    int32_t* slot_env = nullptr;   // [workgroups x epw] lane-slot map of the persistent rollout kernel (pad-contact variants; so100_balance.hpp)
    float* render_scene = nullptr; // [envs][RS_STRIDE] scene records of so100_render (so100_render.hpp); allocated on first use, grown on demand
    int render_scene_envs = 0;
};

namespace {
#define DISPATCH_KIND(kind, fn) \
    ((kind) == 1 ? KindOps<1>::fn : (kind) == 2 ? KindOps<2>::fn : (kind) == 3 ? KindOps<3>::fn : (kind) == 4 ? KindOps<4>::fn : (kind) == 5 ? KindOps<5>::fn : KindOps<6>::fn)

// so100_policy_weights (the ABI) and PolicyWeights (the kernels) are the table of so100_policy_tensors.h, in its order
#define X(name, rows, cols) static_assert(offsetof(so100_policy_weights, name) == T_##name*sizeof(const float*) && \
                                          offsetof(PolicyWeights, name) == T_##name*sizeof(const float*), #name " is out of the table's order");
SO100_POLICY_TENSORS(X)
#undef X
static_assert(sizeof(so100_policy_weights) == NUM_TENSORS*sizeof(const float*) && sizeof(PolicyWeights) == sizeof(so100_policy_weights), "layout");

bool any_null(const so100_policy_weights& w) {
#define X(name, rows, cols) if (!w.name) return true;
    SO100_POLICY_TENSORS(X)
#undef X
    return false;
}

// Envs per workgroup of the multi-wave kernels.  Their step time is set by the slowest lane of a wave (a cube in a contact transient, a
// pad hitting the floor: data-dependent Newton iterations), so a batch that leaves CUs idle is spread thinner: 16 or 32 envs per 4-wave
// workgroup while that still fits one workgroup per CU.  Variants without a data-dependent solve (cube pinned) gain nothing and keep 64.
int choose_envs_per_workgroup(const so100_config& cfg, int cus) {
    if (cfg.envs_per_workgroup != 0) return (int)cfg.envs_per_workgroup;          // the caller pins it (validated by so100_create)
    int epw = 64;
    if (cfg.flags & (SO100_F_FLOOR | SO100_F_PADS_FLOOR | SO100_F_PADS_CUBE | SO100_F_LINKS_FLOOR | SO100_F_LINKS_CUBE))
        while (epw > 16 && (cfg.num_envs + epw/2 - 1)/(epw/2) <= cus) epw /= 2;
    // contact disabled (no data-dependent solve): 32 envs per workgroup while that fits the CUs -- the persistent kernel's policy phase then
    // runs one 32-row MFMA tile per tower instead of two (so100_rollout_fused<K, 8, 4, 32>: half the matrix-core time per step)
    if (cfg.flags == SO100_F_CUBE_PINNED && (cfg.num_envs + 31)/32 <= cus) epw = 32;
    return epw;
}

// what so100_create does on the device, under its guard; whatever a failure leaves allocated so100_destroy frees
int create_on_device(so100_sim* s) {
    const so100_config* cfg = &s->cfg;
    s->prm.n = cfg->num_envs; s->prm.flags = cfg->flags; s->prm.solver_iters = cfg->solver_iters;
    s->prm.contact_iters = cfg->contact_iters; s->prm.frame_skip = cfg->frame_skip;
    s->prm.max_episode_steps = cfg->max_episode_steps;
    s->prm.seed_lo = (uint32_t)cfg->seed; s->prm.seed_hi = (uint32_t)(cfg->seed >> 32);
    s->prm.env_id_offset = cfg->env_id_offset;
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    s->prm.epw = choose_envs_per_workgroup(*cfg, cus);
    s->prm.mw_max = MW_MAX_ENVS;
    if (const char* ov = getenv("SO100_MW_MAX_ENVS")) { const long v = atol(ov); if (v >= 0) s->prm.mw_max = (int32_t)(v > (1L << 30) ? (1L << 30) : v); }
    const size_t bytes = (size_t)SF_COUNT*(size_t)cfg->num_envs*sizeof(float);
    if (hipMalloc(&s->state, bytes) != hipSuccess) return fail(SO100_E_NOMEM, "so100_create: hipMalloc of %ld bytes failed", (long)bytes);
    float tab[36*6];
    for (int i = 0; i < 36; i++) for (int j = 0; j < 6; j++) tab[6*i + j] = (float)SO100_VALID_START_POSITIONS[i][j];
    if (hipMalloc(&s->start_tab, sizeof tab) != hipSuccess || hipMemcpy(s->start_tab, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SO100_E_NOMEM, "so100_create: start table upload failed");
    // workgroup load balancing of the persistent rollout kernel (pad-contact variants, batches it serves; SO100_BALANCE=0 turns it off)
    const char* bal = getenv("SO100_BALANCE");
    const bool pads = (cfg->flags & (SO100_F_PADS_FLOOR | SO100_F_PADS_CUBE | SO100_F_LINKS_FLOOR | SO100_F_LINKS_CUBE)) != 0;
    if (pads && cfg->num_envs <= BALANCE_MAX_ENVS && !(bal && atoi(bal) == 0)) {
        const size_t slots = (size_t)((cfg->num_envs + s->prm.epw - 1)/s->prm.epw)*(size_t)s->prm.epw;
        if (hipMalloc(&s->slot_env, slots*sizeof(int32_t)) != hipSuccess) return fail(SO100_E_NOMEM, "so100_create: hipMalloc of the slot map failed");
    }
    HIP_TRY(DISPATCH_KIND(cfg->env_kind, init)(s->prm.n, s->state), SO100_E_LAUNCH, "so100_create: ");
    return 0;
}

// `rows` rows of the [field][N] state matrix from row `row`: copied to `user` (or, to_state, from it); a null `user` zeroes them
struct RowCopy { int row, rows; const void* user; };
int move_rows(so100_sim* s, const char* fn, bool to_state, std::initializer_list<RowCopy> copies, void* stream) {
    SO100_ON_DEVICE(s->cfg.device, fn);
    const size_t n = (size_t)s->prm.n;
    for (const RowCopy& c : copies) {
        float* mine = s->state + (size_t)c.row*n;
        const size_t bytes = (size_t)c.rows*n*sizeof(float);
        if (!c.user) HIP_TRY(hipMemsetAsync(mine, 0, bytes, (hipStream_t)stream), SO100_E_LAUNCH);
        else if (to_state) HIP_TRY(hipMemcpyAsync(mine, c.user, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), SO100_E_LAUNCH);
        else HIP_TRY(hipMemcpyAsync(const_cast<void*>(c.user), mine, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), SO100_E_LAUNCH);
    }
    return 0;
}
}  // namespace

extern "C" {

int so100_abi_version(void) { return SO100_ABI_VERSION; }
int so100_obs_dim(int32_t kind) { return (kind == 1 || kind == 2 || kind == 6) ? 15 : (kind >= 3 && kind <= 5) ? 8 : -1; }
int so100_num_state_fields(void) { return SF_COUNT; }
int so100_state_field_index(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < SF_COUNT; i++) if (strcmp(kFieldNames[i], name) == 0) return i;
    return -1;
}
const char* so100_state_field_name(int32_t field) { return (field >= 0 && field < SF_COUNT) ? kFieldNames[field] : nullptr; }
const char* so100_last_error(void) { return g_last_error; }
#ifdef SO100_ROLLOUT_PROF
int so100_prof_read(int kind, long long* out64) { return DISPATCH_KIND(kind, prof_read)(out64); }
int so100_prof_read_wg(int kind, long long* wg4096, int* env32768) { return DISPATCH_KIND(kind, prof_read_wg)(wg4096, env32768); }
int so100_prof_read_hist(int kind, unsigned long long* hist48, int reset) { return DISPATCH_KIND(kind, prof_read_hist)(hist48, reset); }
#endif

int so100_create(const so100_config* cfg, so100_sim** out) {
    if (!cfg || !out) return fail(SO100_E_INVALID, "so100_create: null argument");
    *out = nullptr;
    if (cfg->env_kind < 1 || cfg->env_kind > 6) return fail(SO100_E_INVALID, "so100_create: env_kind must be 1..6");
    if (cfg->num_envs < 1) return fail(SO100_E_INVALID, "so100_create: num_envs must be >= 1");
    if (cfg->solver_iters < 1 || cfg->solver_iters > 64) return fail(SO100_E_INVALID, "so100_create: solver_iters must be in 1..64");
    if (cfg->contact_iters < 1 || cfg->contact_iters > 64) return fail(SO100_E_INVALID, "so100_create: contact_iters must be in 1..64");
    if (cfg->frame_skip < 1 || cfg->frame_skip > 1024) return fail(SO100_E_INVALID, "so100_create: frame_skip must be in 1..1024");
    if (cfg->max_episode_steps < 0) return fail(SO100_E_INVALID, "so100_create: max_episode_steps must be >= 0");
    if (cfg->flags & ~(SO100_F_FRICTIONLOSS | SO100_F_LIMITS | SO100_F_FLOOR | SO100_F_CUBE_PINNED | SO100_F_PADS_FLOOR | SO100_F_PADS_CUBE | SO100_F_LINKS_FLOOR | SO100_F_LINKS_CUBE))
        return fail(SO100_E_INVALID, "so100_create: unknown flag bits");
    if ((cfg->flags & (SO100_F_PADS_CUBE | SO100_F_LINKS_CUBE)) && (cfg->flags & SO100_F_CUBE_PINNED))
        return fail(SO100_E_INVALID, "so100_create: SO100_F_PADS_CUBE / SO100_F_LINKS_CUBE need a dynamic cube (not SO100_F_CUBE_PINNED)");
    if (cfg->envs_per_workgroup != 0 && cfg->envs_per_workgroup != 16 && cfg->envs_per_workgroup != 32 && cfg->envs_per_workgroup != 64)
        return fail(SO100_E_INVALID, "so100_create: envs_per_workgroup must be 0 (automatic), 16, 32 or 64");
    if ((cfg->flags & SO100_F_FLOOR) && (cfg->flags & SO100_F_CUBE_PINNED))
        return fail(SO100_E_INVALID, "so100_create: SO100_F_FLOOR and SO100_F_CUBE_PINNED are mutually exclusive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(SO100_E_NODEVICE, "so100_create: no HIP device available (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(SO100_E_INVALID, "so100_create: device ordinal out of range");
    SO100_ON_DEVICE(cfg->device, "so100_create");
    so100_sim* s = new (std::nothrow) so100_sim();
    if (!s) return fail(SO100_E_NOMEM, "so100_create: out of host memory");
    s->cfg = *cfg;
    const int rc = create_on_device(s);
    if (rc != 0) { so100_destroy(s); return rc; }
    *out = s;
    return 0;
}

int so100_envs_per_workgroup(const so100_sim* s) { return s ? s->prm.epw : SO100_E_INVALID; }

void so100_destroy(so100_sim* s) {
    if (!s) return;
    DeviceGuard g(s->cfg.device);
    if (s->state) (void)hipFree(s->state);
    if (s->start_tab) (void)hipFree(s->start_tab);
    if (s->slot_env) (void)hipFree(s->slot_env);
    if (s->render_scene) (void)hipFree(s->render_scene);
    delete s;
}

int so100_reset(so100_sim* s, const uint8_t* mask_dev, const float* inject_dev, float* obs_dev, void* stream) {
    if (!s) return fail(SO100_E_INVALID, "so100_reset: null handle");
    SO100_ON_DEVICE(s->cfg.device, "so100_reset");
    HIP_TRY(DISPATCH_KIND(s->cfg.env_kind, reset)(s->prm, s->state, s->start_tab, mask_dev, inject_dev, obs_dev, (hipStream_t)stream), SO100_E_LAUNCH);
    return 0;
}

int so100_step(so100_sim* s, const so100_step_io* io, void* stream) {
    if (!s || !io) return fail(SO100_E_INVALID, "so100_step: null argument");
    if (!io->act_dev || !io->obs_dev || !io->rew_dev || !io->done_dev || !io->trunc_dev)
        return fail(SO100_E_INVALID, "so100_step: act/obs/rew/done/trunc pointers are required");
    SO100_ON_DEVICE(s->cfg.device, "so100_step");
    StepPtrs p;
    p.state = s->state; p.start_tab = s->start_tab;
    p.act = io->act_dev; p.obs = io->obs_dev; p.rew = io->rew_dev; p.done = io->done_dev; p.trunc = io->trunc_dev;
    p.tobs = io->terminal_obs_dev; p.ep_ret = io->ep_return_dev; p.ep_len = io->ep_length_dev; p.inject = io->inject_dev; p.rollout_row = io->rollout_row_dev;
    HIP_TRY(DISPATCH_KIND(s->cfg.env_kind, step)(s->prm, p, (hipStream_t)stream), SO100_E_LAUNCH);
    return 0;
}

int so100_policy_forward(so100_sim* s, const so100_policy_weights* w, const so100_policy_io* io, uint32_t step_counter, void* stream) {
    if (!s || !w || !io) return fail(SO100_E_INVALID, "so100_policy_forward: null argument");
    if (!io->obs_dev || !io->act_env_dev) return fail(SO100_E_INVALID, "so100_policy_forward: obs and act_env pointers are required");
    if (any_null(*w)) return fail(SO100_E_INVALID, "so100_policy_forward: null weight pointer");
    SO100_ON_DEVICE(s->cfg.device, "so100_policy_forward");
    PolicyWeights pw; memcpy(&pw, w, sizeof pw);
    PolicyIO pio; pio.obs = io->obs_dev; pio.noise = io->noise_dev; pio.act_env = io->act_env_dev; pio.act_raw = io->act_raw_dev;
    pio.value = io->value_dev; pio.logp = io->logp_dev; pio.rollout_row = io->rollout_row_dev;
    // the matrix-core kernel, grid-stride over tiles of 64 envs, two workgroups per CU resident
    const int ntiles = (s->prm.n + 63)/64;
    const dim3 grid((unsigned)(ntiles < 512 ? ntiles : 512));
    SO100_WITH_OBS_DIM(so100_obs_dim(s->cfg.env_kind),
        hipLaunchKernelGGL((so100_policy_forward_mfma<OD>), grid, dim3(256), 0, (hipStream_t)stream, s->prm.n, pw, pio, s->prm.seed_lo, s->prm.seed_hi, s->prm.env_id_offset, step_counter););
    HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    return 0;
}

int so100_rollout(so100_sim* s, const so100_policy_weights* w, const so100_rollout_io* io, int32_t T, uint32_t step_counter0, void* stream) {
    if (!s || !w || !io) return fail(SO100_E_INVALID, "so100_rollout: null argument");
    if (T < 1) return fail(SO100_E_INVALID, "so100_rollout: T must be >= 1");
    if (!io->rollout_dev || !io->obs_dev || !io->rew_dev || !io->done_dev || !io->trunc_dev)
        return fail(SO100_E_INVALID, "so100_rollout: rollout/obs/rew/done/trunc pointers are required");
    if (any_null(*w)) return fail(SO100_E_INVALID, "so100_rollout: null weight pointer");
    SO100_ON_DEVICE(s->cfg.device, "so100_rollout");
    PolicyWeights pw; memcpy(&pw, w, sizeof pw);
    RolloutArgs ra; ra.buf = io->rollout_dev; ra.T = T; ra.step_counter0 = step_counter0; ra.obs_in = io->obs_dev; ra.tobs_chunk = io->terminal_obs_chunk_dev;
    ra.slot_env = s->slot_env;
    if (s->slot_env) {                                       // deal the envs out over the workgroups by their contact load
        const int nwg = (s->prm.n + s->prm.epw - 1)/s->prm.epw;
        hipLaunchKernelGGL(so100_build_slot_map, dim3(1), dim3(BALANCE_THREADS), 0, (hipStream_t)stream, s->prm.n, s->prm.epw, nwg,
                           reinterpret_cast<const int32_t*>(s->state + (size_t)SF_contact_load*(size_t)s->prm.n), s->slot_env);
        HIP_TRY(hipGetLastError(), SO100_E_LAUNCH);
    }
    RolloutPtrs rp{ io->obs_dev, io->rew_dev, io->done_dev, io->trunc_dev, io->terminal_obs_dev, io->ep_return_dev, io->ep_length_dev };
    HIP_TRY(DISPATCH_KIND(s->cfg.env_kind, rollout)(s->prm, s->state, s->start_tab, rp, pw, ra, (hipStream_t)stream), SO100_E_LAUNCH);
    return 0;
}

int so100_render(so100_sim* s, const so100_render_io* io, void* stream) {
    if (!s || !io) return fail(SO100_E_INVALID, "so100_render: null argument");
    if (io->camera != SO100_CAM_END && io->camera != SO100_CAM_SCENE)
        return fail(SO100_E_INVALID, "so100_render: camera must be SO100_CAM_END (0) or SO100_CAM_SCENE (1), got %ld", (long)io->camera);
    if (io->width < 1 || io->width > 4096) return fail(SO100_E_INVALID, "so100_render: width must be in 1..4096, got %ld", (long)io->width);
    if (io->height < 1 || io->height > 4096) return fail(SO100_E_INVALID, "so100_render: height must be in 1..4096, got %ld", (long)io->height);
    if (io->env_begin < 0 || io->env_begin >= s->prm.n) return fail(SO100_E_INVALID, "so100_render: env_begin must be in [0, N), got %ld", (long)io->env_begin);
    if (io->env_count < 1 || io->env_count > s->prm.n - io->env_begin)
        return fail(SO100_E_INVALID, "so100_render: env_count must be >= 1 with env_begin + env_count <= N, got %ld", (long)io->env_count);
    if (io->geom_mask & ~(SO100_GEOM_FLOOR | SO100_GEOM_CUBE | SO100_GEOM_LINKS | SO100_GEOM_PADS))
        return fail(SO100_E_INVALID, "so100_render: geom_mask has unknown bits (%ld)", (long)io->geom_mask);
    if (!io->rgb_dev && !io->depth_dev && !io->seg_dev) return fail(SO100_E_INVALID, "so100_render: rgb_dev, depth_dev and seg_dev are all NULL");
    if (io->free_cam && io->camera != SO100_CAM_SCENE) return fail(SO100_E_INVALID, "so100_render: free_cam is for the scene camera only");
    RenderLaunch L;
    L.camera = io->camera; L.W = io->width; L.H = io->height; L.begin = io->env_begin; L.count = io->env_count; L.n = s->prm.n;
    L.mask = io->geom_mask != 0 ? io->geom_mask : (io->camera == SO100_CAM_END ? RG_DEFAULT_END : RG_DEFAULT_SCENE);
    for (int i = 0; i < 3; i++) L.cam_p[i] = 0.0f;
    for (int i = 0; i < 9; i++) L.cam_R[i] = 0.0f;
    double fovy = RENDER_END_FOVY;
    if (io->camera == SO100_CAM_SCENE) {
        double lookat[3] = { RENDER_SCENE_LOOKAT[0], RENDER_SCENE_LOOKAT[1], RENDER_SCENE_LOOKAT[2] };
        double dist = RENDER_SCENE_DISTANCE, az = RENDER_SCENE_AZIMUTH, el = RENDER_SCENE_ELEVATION;
        fovy = RENDER_SCENE_FOVY;
        if (const float* fc = io->free_cam) {
            for (int i = 0; i < 7; i++) if (!std::isfinite(fc[i])) return fail(SO100_E_INVALID, "so100_render: free_cam[%ld] is not finite", (long)i);
            if (!(fc[3] > 0.0f)) return fail(SO100_E_INVALID, "so100_render: free_cam distance must be > 0");
            if (!(fc[6] > 0.0f && fc[6] < 180.0f)) return fail(SO100_E_INVALID, "so100_render: free_cam fovy_deg must be in (0, 180)");
            lookat[0] = fc[0]; lookat[1] = fc[1]; lookat[2] = fc[2]; dist = fc[3]; az = fc[4]; el = fc[5]; fovy = fc[6];
        }
        double p[3], R[9];
        free_camera_pose<double>(lookat, dist, az, el, p, R);
        for (int i = 0; i < 3; i++) L.cam_p[i] = (float)p[i];
        for (int i = 0; i < 9; i++) L.cam_R[i] = (float)R[i];
    }
    L.inv_f = (float)render_inv_focal(fovy, io->height);
    SO100_ON_DEVICE(s->cfg.device, "so100_render");
    if (io->env_count > s->render_scene_envs) {
        if (s->render_scene) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream), SO100_E_LAUNCH); (void)hipFree(s->render_scene); s->render_scene = nullptr; }
        s->render_scene_envs = 0;
        const size_t bytes = (size_t)io->env_count*RS_STRIDE*sizeof(float);
        if (hipMalloc(&s->render_scene, bytes) != hipSuccess) { s->render_scene = nullptr; return fail(SO100_E_NOMEM, "so100_render: hipMalloc of %ld bytes failed", (long)bytes); }
        s->render_scene_envs = io->env_count;
    }
    HIP_TRY(render_launch(s->state, L, s->render_scene, io->rgb_dev, io->depth_dev, io->seg_dev, (hipStream_t)stream), SO100_E_LAUNCH);
    return 0;
}

int so100_get_state(so100_sim* s, float* qpos_dev, float* qvel_dev, void* stream) {
    if (!s || !qpos_dev || !qvel_dev) return fail(SO100_E_INVALID, "so100_get_state: null argument");
    return move_rows(s, "so100_get_state", false, { { SF_QPOS0, 13, qpos_dev }, { SF_QVEL0, 12, qvel_dev } }, stream);
}
int so100_set_state(so100_sim* s, const float* qpos_dev, const float* qvel_dev, void* stream) {
    if (!s || !qpos_dev || !qvel_dev) return fail(SO100_E_INVALID, "so100_set_state: null argument");
    return move_rows(s, "so100_set_state", true, { { SF_QPOS0, 13, qpos_dev }, { SF_QVEL0, 12, qvel_dev }, { SF_qc0, 6, nullptr } }, stream);   // new q: drop the compensation
}
int so100_get_field(so100_sim* s, int32_t field, void* out_dev, void* stream) {
    if (!s || !out_dev || field < 0 || field >= SF_COUNT) return fail(SO100_E_INVALID, "so100_get_field: bad argument");
    return move_rows(s, "so100_get_field", false, { { field, 1, out_dev } }, stream);
}
int so100_set_field(so100_sim* s, int32_t field, const void* in_dev, void* stream) {
    if (!s || !in_dev || field < 0 || field >= SF_COUNT) return fail(SO100_E_INVALID, "so100_set_field: bad argument");
    return move_rows(s, "so100_set_field", true, { { field, 1, in_dev } }, stream);
}

}  // extern "C"

// the model queries (include/so100_query.h): kernels and ABI functions of their own file, compiled into this object -- they read the
// handle defined above, and the list of the product's objects stays what the side-build recipe names
#include "so100_query.hip"
#include "so100_query_forward.hip"
#include "so100_query_trajectory.hip"
#include "so100_query_derivative.hip"
#include "so100_query_lqr.hip"
#include "so100_query_closed_loop.hip"
#include "so100_query_cost.hip"
#include "so100_query_mppi.hip"
#include "so100_query_cem.hip"
