// abi_demo.cpp -- a plain C++ consumer of the C ABI (include/so100_sim.h, include/so100_learn.h, include/so100_query.h): no Python, no PyTorch.
// Build:  hipcc -O2 -o abi_demo examples/abi_demo.cpp -Iinclude -Lso100_mujoco_rl_amd -lso100sim -Wl,-rpath,$PWD/so100_mujoco_rl_amd
// Run:    ./abi_demo [num_envs] [steps]     (prints a checksum of the final observations, one line from the model queries, then the learner's)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include "so100_sim.h"
#include "so100_learn.h"
#include "so100_query.h"

#define CHECK(x) do { if ((x) != hipSuccess) { std::fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)

int main(int argc, char** argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 4096, steps = argc > 2 ? std::atoi(argv[2]) : 100;
    so100_config cfg = {};
    cfg.env_kind = SO100_ENV01; cfg.num_envs = n; cfg.device = 0; cfg.flags = SO100_F_REFERENCE;
    cfg.solver_iters = 3; cfg.contact_iters = 4; cfg.frame_skip = 16; cfg.max_episode_steps = 4000; cfg.seed = 42;
    so100_sim* sim = nullptr;
    if (so100_create(&cfg, &sim) != 0) { std::fprintf(stderr, "so100_create: %s\n", so100_last_error()); return 1; }
    const int od = so100_obs_dim(cfg.env_kind);
    float *act, *obs, *rew; uint8_t *done, *trunc;
    CHECK(hipMalloc(&act, sizeof(float)*6*n)); CHECK(hipMalloc(&obs, sizeof(float)*od*n)); CHECK(hipMalloc(&rew, sizeof(float)*n));
    CHECK(hipMalloc(&done, n)); CHECK(hipMalloc(&trunc, n));
    std::vector<float> h_act(6*(size_t)n);
    for (size_t i = 0; i < h_act.size(); i++) h_act[i] = (float)((i*2654435761u) % 2001) / 1000.0f - 1.0f;   // fixed pseudo-random actions
    CHECK(hipMemcpy(act, h_act.data(), sizeof(float)*h_act.size(), hipMemcpyHostToDevice));
    hipStream_t st; CHECK(hipStreamCreate(&st));
    if (so100_reset(sim, nullptr, nullptr, obs, st) != 0) { std::fprintf(stderr, "so100_reset: %s\n", so100_last_error()); return 1; }
    so100_step_io io = {};
    io.act_dev = act; io.obs_dev = obs; io.rew_dev = rew; io.done_dev = done; io.trunc_dev = trunc;
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    CHECK(hipEventRecord(e0, st));
    for (int t = 0; t < steps; t++)
        if (so100_step(sim, &io, st) != 0) { std::fprintf(stderr, "so100_step: %s\n", so100_last_error()); return 1; }
    CHECK(hipEventRecord(e1, st)); CHECK(hipStreamSynchronize(st));
    float ms = 0; CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<float> h_obs((size_t)od*n), h_rew(n);
    CHECK(hipMemcpy(h_obs.data(), obs, sizeof(float)*h_obs.size(), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_rew.data(), rew, sizeof(float)*n, hipMemcpyDeviceToHost));
    double cs = 0, rs = 0; for (float v : h_obs) cs += v; for (float v : h_rew) rs += v;
    std::printf("envs %d steps %d  %.1f us/step  %.2f M env-steps/s  obs_checksum %.6f  reward_sum %.6f\n", n, steps, ms*1e3/steps, n*(double)steps/ms/1e3, cs, rs);
    // ---- model queries (so100_query.h) on the handle's own state: where every end effector is, and the joints that would put it on its env's cube
    {
        float *qpos, *qvel, *ee, *q_ik, *resid; uint8_t* conv;
        CHECK(hipMalloc(&qpos, sizeof(float)*13*n)); CHECK(hipMalloc(&qvel, sizeof(float)*12*n)); CHECK(hipMalloc(&ee, sizeof(float)*3*n));
        CHECK(hipMalloc(&q_ik, sizeof(float)*6*n)); CHECK(hipMalloc(&resid, sizeof(float)*n)); CHECK(hipMalloc(&conv, n));
        if (so100_get_state(sim, qpos, qvel, st) != 0) { std::fprintf(stderr, "so100_get_state: %s\n", so100_last_error()); return 1; }
        so100_kinematics_io kio = {};
        kio.ee_dev = ee;                                               // q_dev NULL: the handle's joints, M = N
        if (so100_query_kinematics(sim, &kio, n, st) != 0) { std::fprintf(stderr, "so100_query_kinematics: %s\n", so100_last_error()); return 1; }
        so100_ik_io iio = {};
        iio.target_dev = qpos + 6*(size_t)n;                           // rows 6..8 of qpos [13][N]: the cube's position, already [3][N]
        iio.link = SO100_EE_LINK; iio.iters = SO100_IK_ITERS; iio.damping = SO100_IK_DAMPING; iio.tol = SO100_IK_TOL; iio.max_step = SO100_IK_MAX_STEP;
        iio.q_dev = q_ik; iio.residual_dev = resid; iio.converged_dev = conv;
        if (so100_query_ik(sim, &iio, n, st) != 0) { std::fprintf(stderr, "so100_query_ik: %s\n", so100_last_error()); return 1; }
        CHECK(hipStreamSynchronize(st));
        std::vector<float> h_ee(3*(size_t)n), h_res(n); std::vector<uint8_t> h_conv(n);
        CHECK(hipMemcpy(h_ee.data(), ee, sizeof(float)*h_ee.size(), hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h_res.data(), resid, sizeof(float)*n, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(h_conv.data(), conv, n, hipMemcpyDeviceToHost));
        double ez = 0, rmax = 0; long nconv = 0;
        for (int i = 0; i < n; i++) { ez += h_ee[2*(size_t)n + i]; rmax = std::fmax(rmax, h_res[i]); nconv += h_conv[i]; }
        std::printf("queries: mean end-effector height %.4f m  IK onto the cube: %ld of %d converged, worst residual %.2e m\n", ez/n, nconv, n, rmax);
        // forward dynamics on the handle's own state (qpos_dev / qvel_dev NULL), the servos holding the pose: how many envs touch something, and how hard
        int32_t* ncon; float* padf;
        CHECK(hipMalloc(&ncon, sizeof(int32_t)*n)); CHECK(hipMalloc(&padf, sizeof(float)*8*n));
        so100_forward_io fio = {};
        fio.flags = cfg.flags; fio.solver_iters = SO100_FWD_SOLVER_ITERS; fio.contact_iters = SO100_FWD_CONTACT_ITERS;
        fio.ncon_dev = ncon; fio.pad_force_dev = padf;
        if (so100_query_forward(sim, &fio, n, st) != 0) { std::fprintf(stderr, "so100_query_forward: %s\n", so100_last_error()); return 1; }
        CHECK(hipStreamSynchronize(st));
        std::vector<int32_t> h_ncon(n); std::vector<float> h_padf(8*(size_t)n);
        CHECK(hipMemcpy(h_ncon.data(), ncon, sizeof(int32_t)*n, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h_padf.data(), padf, sizeof(float)*h_padf.size(), hipMemcpyDeviceToHost));
        long contacts = 0, touching = 0; double fmax = 0;
        for (int i = 0; i < n; i++) {
            contacts += h_ncon[i];
            double f = 0; for (int g = 0; g < 8; g++) f += h_padf[g*(size_t)n + i];
            touching += f > 0; fmax = std::fmax(fmax, f);
        }
        std::printf("forward: %ld contacts in all; %ld of %d envs press a finger pad on something, the hardest with %.3f N\n", contacts, touching, n, fmax);
    }
    // ---- the learner from plain C++ (so100_learn.h): advantages of a small synthetic chunk, then one PPO minibatch step on all of it
    {
        const int T = 4, k = od + 10, P = so100_learner_num_params(od);
        auto rnd = [](size_t i) { return (float)((i*2654435761u) % 2001) / 1000.0f - 1.0f; };
        std::vector<float> h_chunk((size_t)T*n*k), h_par(P), h_last((size_t)n*od);
        for (size_t i = 0; i < h_chunk.size(); i++) h_chunk[i] = rnd(i);
        for (size_t r = 0; r < (size_t)T*n; r++) { h_chunk[r*k + od + 7] = (float)(r % 7 == 3); h_chunk[r*k + od + 9] = -6.0f; }   // done code 0 / 1, old log-prob
        for (int i = 0; i < P; i++) h_par[i] = 0.2f*rnd(7919u*(size_t)i + 1);
        for (size_t i = 0; i < h_last.size(); i++) h_last[i] = rnd(i + 12345);
        so100_learner_config lc = {};
        lc.obs_dim = od; lc.device = 0; lc.max_minibatch = T*n; lc.gamma = 0.99f; lc.gae_lambda = 0.95f; lc.clip_range = 0.2f; lc.vf_coef = 0.5f;
        lc.max_grad_norm = 0.5f; lc.lr = 3e-4; lc.beta1 = 0.9; lc.beta2 = 0.999; lc.adam_eps = 1e-5;
        so100_learner* learner = nullptr;
        if (so100_learner_create(&lc, &learner) != 0) { std::fprintf(stderr, "so100_learner_create: %s\n", so100_last_error()); return 1; }
        float *chunk, *par, *mom, *last, *adv, *ret, *lstat;              // lstat: adv_stats[2] | stats[4]
        CHECK(hipMalloc(&chunk, sizeof(float)*h_chunk.size())); CHECK(hipMalloc(&par, sizeof(float)*P)); CHECK(hipMalloc(&mom, sizeof(float)*2*P));
        CHECK(hipMalloc(&last, sizeof(float)*h_last.size())); CHECK(hipMalloc(&adv, sizeof(float)*T*n)); CHECK(hipMalloc(&ret, sizeof(float)*T*n));
        CHECK(hipMalloc(&lstat, sizeof(float)*6));
        CHECK(hipMemcpy(chunk, h_chunk.data(), sizeof(float)*h_chunk.size(), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(par, h_par.data(), sizeof(float)*P, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(last, h_last.data(), sizeof(float)*h_last.size(), hipMemcpyHostToDevice));
        CHECK(hipMemset(mom, 0, sizeof(float)*2*P));
        so100_advantages_io aio = {};
        aio.rollout_dev = chunk; aio.last_obs_dev = last; aio.params_dev = par; aio.adv_dev = adv; aio.ret_dev = ret; aio.adv_stats_dev = lstat;
        if (so100_learner_advantages(learner, &aio, T, n, (void*)st) != 0) { std::fprintf(stderr, "so100_learner_advantages: %s\n", so100_last_error()); return 1; }
        so100_minibatch_io mio = {};
        mio.rollout_dev = chunk; mio.num_samples = (int64_t)T*n; mio.idx_dev = nullptr; mio.mb = T*n; mio.adam_step = 1;
        mio.adv_dev = adv; mio.ret_dev = ret; mio.adv_stats_dev = lstat; mio.params_dev = par; mio.adam_m_dev = mom; mio.adam_v_dev = mom + P; mio.stats_dev = lstat + 2;
        if (so100_learner_minibatch_step(learner, &mio, (void*)st) != 0) { std::fprintf(stderr, "so100_learner_minibatch_step: %s\n", so100_last_error()); return 1; }
        CHECK(hipStreamSynchronize(st));
        float h_st[6]; std::vector<float> h_new(P);
        CHECK(hipMemcpy(h_st, lstat, sizeof h_st, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h_new.data(), par, sizeof(float)*P, hipMemcpyDeviceToHost));
        double moved = 0; for (int i = 0; i < P; i++) moved += std::fabs((double)h_new[i] - h_par[i]);
        std::printf("learner: %d params  adv_mean %.6f adv_std %.6f  policy_loss %.6f value_loss %.6f clip_fraction %.4f grad_norm %.6f  mean_param_step %.3e\n",
                    P, h_st[0], h_st[1], h_st[2], h_st[3], h_st[4], h_st[5], moved/P);
        // ---- reward normalisation (SB3 VecNormalize's reward half): the chunk's rewards normalised into a dense array, the advantages read from it
        {
            const int64_t ws_bytes = so100_learner_reward_norm_workspace(T, n);
            double* rn_state; float* rn_rew; void* rn_ws;
            CHECK(hipMalloc(&rn_state, sizeof(double)*(3 + (size_t)n))); CHECK(hipMalloc(&rn_rew, sizeof(float)*T*n)); CHECK(hipMalloc(&rn_ws, (size_t)ws_bytes));
            so100_reward_norm_io nio = {};
            nio.rollout_dev = chunk; nio.state_dev = rn_state; nio.reward_dev = rn_rew; nio.workspace_dev = rn_ws; nio.workspace_bytes = ws_bytes;
            nio.clip_reward = 10.0; nio.epsilon = 1e-8;
            if (so100_learner_reward_norm_init(learner, rn_state, n, (void*)st) != 0 || so100_learner_normalize_rewards(learner, &nio, T, n, (void*)st) != 0 ||
                so100_learner_advantages_r(learner, &aio, rn_rew, T, n, (void*)st) != 0) { std::fprintf(stderr, "reward normalisation: %s\n", so100_last_error()); return 1; }
            double h_mom[3]; float h_adv[2];
            CHECK(hipStreamSynchronize(st));
            CHECK(hipMemcpy(h_mom, rn_state, sizeof h_mom, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h_adv, lstat, sizeof h_adv, hipMemcpyDeviceToHost));
            std::printf("reward normalisation: return_mean %.6f return_std %.6f count %.4f  adv_std %.6f (of the normalised rewards)\n", h_mom[0], std::sqrt(h_mom[1]), h_mom[2], h_adv[1]);
        }
        so100_learner_destroy(learner);
    }
    so100_destroy(sim);
    return 0;
}
