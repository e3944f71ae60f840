// train_ppo.cpp -- PPO training on the C ABI alone (include/so100_sim.h, include/so100_learn.h): no Python, no PyTorch.  Per iteration one
// so100_rollout (64 steps of every env, policy included) and one so100_learner_update (advantages, the on-device shuffle, every minibatch
// step); the policy the simulator runs is a so100_policy_weights pointing into the learner's flat parameter block, so nothing is copied
// between the two.
// Build:  hipcc -O2 -o train_ppo examples/train_ppo.cpp -Iinclude -Lso100_mujoco_rl_amd -lso100sim -Wl,-rpath,$PWD/so100_mujoco_rl_amd
// Run:    ./train_ppo [num_envs] [iters] [seed] [normalize_reward]
//         one line per iteration (mean reward per step, the update's out_dev), then "param_checksum": the fp64 sum of the parameters.
//         normalize_reward 1: the update normalises the rewards first (SB3 VecNormalize's reward half, so100_learner_update_r) and each
//         line ends with return_std, the running standard deviation of the envs' discounted returns
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "so100_sim.h"
#include "so100_learn.h"

#define CHECK(x) do { if ((x) != hipSuccess) { std::fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define CALL(x) do { if ((x) != 0) { std::fprintf(stderr, "%s: %s\n", #x, so100_last_error()); return 1; } } while (0)

// The initial parameters: tensor t, element i is u(t, i) * scale[t] with u in [-1, 1] from an integer hash -- exact in float, so any
// other program can form the same block (tests/test_gpu_learner_update.py does).  Biases and log_std start at 0.
static const char* const kTensors[13] = { "pi_w0", "pi_b0", "pi_w1", "pi_b1", "mu_w", "mu_b", "log_std", "vf_w0", "vf_b0", "vf_w1", "vf_b1", "v_w", "v_b" };
static const float kScale[13] = { 0.25f, 0.0f, 0.125f, 0.0f, 0.01f, 0.0f, 0.0f, 0.25f, 0.0f, 0.125f, 0.0f, 0.125f, 0.0f };

int main(int argc, char** argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 4096, iters = argc > 2 ? std::atoi(argv[2]) : 100;
    const unsigned long long seed = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 0;
    const bool normalize_reward = argc > 4 && std::atoi(argv[4]) != 0;
    const int T = 64, epochs = 4;
    const long rows = (long)T*n;
    const int mb = (int)(rows/4 < 32768 ? rows/4 : 32768);
    const int per_epoch = (int)((rows + mb - 1)/mb);

    so100_config cfg = {};
    cfg.env_kind = SO100_ENV01; cfg.num_envs = n; cfg.device = 0; cfg.flags = SO100_F_REFERENCE;
    cfg.solver_iters = 2; cfg.contact_iters = 20; cfg.frame_skip = 16; cfg.max_episode_steps = 4000; cfg.seed = seed;
    so100_sim* sim = nullptr;
    CALL(so100_create(&cfg, &sim));
    const int od = so100_obs_dim(cfg.env_kind), row = od + 10, P = so100_learner_num_params(od);
    so100_learner_config lc = {};
    lc.obs_dim = od; lc.device = 0; lc.max_minibatch = mb; lc.gamma = 0.99f; lc.gae_lambda = 0.95f; lc.clip_range = 0.2f; lc.vf_coef = 0.5f;
    lc.max_grad_norm = 0.5f; lc.lr = 3e-4; lc.beta1 = 0.9; lc.beta2 = 0.999; lc.adam_eps = 1e-5;
    so100_learner* learner = nullptr;
    CALL(so100_learner_create(&lc, &learner));

    std::vector<float> h_par(P, 0.0f);
    const float* slot[13];
    float *par, *mom;
    CHECK(hipMalloc(&par, sizeof(float)*P)); CHECK(hipMalloc(&mom, sizeof(float)*2*P));
    for (int t = 0; t < 13; t++) {
        const int off = so100_learner_param_offset(od, kTensors[t]), size = so100_learner_param_size(od, kTensors[t]);
        for (int i = 0; i < size; i++)
            h_par[off + i] = ((float)(((unsigned long long)i*2654435761ull + (unsigned long long)t*40503ull) % 2001ull)/1000.0f - 1.0f)*kScale[t];
        slot[t] = par + off;
    }
    so100_policy_weights w;
    std::memcpy(&w, slot, sizeof w);                                    // the struct is its 13 pointers in the order of kTensors
    static_assert(sizeof(so100_policy_weights) == 13*sizeof(const float*), "so100_policy_weights");
    CHECK(hipMemcpy(par, h_par.data(), sizeof(float)*P, hipMemcpyHostToDevice));
    CHECK(hipMemset(mom, 0, sizeof(float)*2*P));

    float *chunk, *tobs, *obs, *rew, *adv, *ret, *adv_stats, *out; uint8_t *done, *trunc; int64_t* perm;
    CHECK(hipMalloc(&chunk, sizeof(float)*rows*row)); CHECK(hipMalloc(&tobs, sizeof(float)*rows*od)); CHECK(hipMalloc(&obs, sizeof(float)*n*od));
    CHECK(hipMalloc(&rew, sizeof(float)*n)); CHECK(hipMalloc(&done, n)); CHECK(hipMalloc(&trunc, n));
    CHECK(hipMalloc(&adv, sizeof(float)*rows)); CHECK(hipMalloc(&ret, sizeof(float)*rows)); CHECK(hipMalloc(&adv_stats, sizeof(float)*2));
    CHECK(hipMalloc(&out, sizeof(float)*SO100_UPDATE_OUT)); CHECK(hipMalloc(&perm, sizeof(int64_t)*rows));
    CHECK(hipMemset(tobs, 0, sizeof(float)*rows*od));                   // the rollout writes it where an episode ended, the learner reads it there alone
    hipStream_t st; CHECK(hipStreamCreate(&st));
    CALL(so100_reset(sim, nullptr, nullptr, obs, st));

    so100_rollout_io rio = {};
    rio.rollout_dev = chunk; rio.obs_dev = obs; rio.rew_dev = rew; rio.done_dev = done; rio.trunc_dev = trunc; rio.terminal_obs_chunk_dev = tobs;
    so100_update_io uio = {};
    uio.rollout_dev = chunk; uio.terminal_obs_chunk_dev = tobs; uio.last_obs_dev = obs; uio.T = T; uio.N = n;
    uio.params_dev = par; uio.adam_m_dev = mom; uio.adam_v_dev = mom + P; uio.adv_dev = adv; uio.ret_dev = ret; uio.adv_stats_dev = adv_stats; uio.perm_dev = perm;
    uio.epochs = epochs; uio.mb = mb; uio.shuffle_seed = seed; uio.terms = nullptr; uio.update_state_dev = nullptr; uio.out_dev = out;

    // reward normalisation: the running state, the dense normalised rewards and the workspace are this program's, like every other buffer
    so100_reward_norm_io nio = {};
    if (normalize_reward) {
        const int64_t ws_bytes = so100_learner_reward_norm_workspace(T, n);
        double* rn_state; float* rn_rewards; void* rn_ws;
        CHECK(hipMalloc(&rn_state, sizeof(double)*(3 + (size_t)n))); CHECK(hipMalloc(&rn_rewards, sizeof(float)*rows)); CHECK(hipMalloc(&rn_ws, (size_t)ws_bytes));
        CALL(so100_learner_reward_norm_init(learner, rn_state, n, (void*)st));
        nio.rollout_dev = chunk; nio.state_dev = rn_state; nio.reward_dev = rn_rewards; nio.workspace_dev = rn_ws; nio.workspace_bytes = ws_bytes;
        nio.clip_reward = 10.0; nio.epsilon = 1e-8;
    }

    std::vector<float> h_chunk((size_t)rows*row);
    float h_out[SO100_UPDATE_OUT];
    for (int it = 0; it < iters; it++) {
        CALL(so100_rollout(sim, &w, &rio, T, (uint32_t)(it*T), (void*)st));
        uio.adam_step0 = it*epochs*per_epoch; uio.shuffle_epoch0 = (uint32_t)(it*epochs);
        CALL(so100_learner_update_r(learner, &uio, normalize_reward ? &nio : nullptr, (void*)st));      // a null norm_io: so100_learner_update
        CHECK(hipMemcpyAsync(h_chunk.data(), chunk, sizeof(float)*h_chunk.size(), hipMemcpyDeviceToHost, st));     // for the reward column alone: an example's shortcut
        CHECK(hipMemcpyAsync(h_out, out, sizeof h_out, hipMemcpyDeviceToHost, st));
        CHECK(hipStreamSynchronize(st));
        double r = 0;
        for (long i = 0; i < rows; i++) r += h_chunk[(size_t)i*row + od + 6];
        std::printf("iter %4d  mean_reward %+.6f  policy_loss %+.6f value_loss %.6f clip_fraction %.4f grad_norm %.6f  explained_variance %+.4f  log_std",
                    it, r/rows, h_out[0], h_out[1], h_out[2], h_out[3], h_out[8]);
        for (int i = 9; i < 15; i++) std::printf(" %+.4f", h_out[i]);
        if (normalize_reward) {
            double moments[3];
            CHECK(hipMemcpy(moments, nio.state_dev, sizeof moments, hipMemcpyDeviceToHost));
            std::printf("  return_std %.4f", std::sqrt(moments[1]));
        }
        std::printf("\n");
    }
    CHECK(hipMemcpy(h_par.data(), par, sizeof(float)*P, hipMemcpyDeviceToHost));
    double cs = 0;
    for (float v : h_par) cs += v;
    std::printf("param_checksum %.15e\n", cs);
    so100_learner_destroy(learner);
    so100_destroy(sim);
    return 0;
}
