// learncheck.cpp -- so100_learn.hpp (the arithmetic the learner's HIP kernels call) instantiated on the host in double and float, behind a
// C interface for ctypes (tests/hostlibs.py; one library, liblearncheck.so, with the three sources beside it).  Test scaffolding only.
#include "../../so100_mujoco_rl_amd/csrc/so100_learn.hpp"

using namespace so100::learn;

// io layouts: head_in = mu[6] log_std[6] a[6] logp_old adv_n V ret clip vf_coef inv_mb (25); head_out = pg_loss v_loss clipped dmu[6] dlog_std[6] dV (16)
template <class S> static void head(const S* in, S* out) {
    const LossHead<S> h = ppo_loss_head<S>(in, in + 6, in + 12, in[18], in[19], in[20], in[21], in[22], in[23], in[24]);
    out[0] = h.pg_loss; out[1] = h.v_loss; out[2] = h.clipped;
    for (int i = 0; i < 6; i++) { out[3 + i] = h.dmu[i]; out[9 + i] = h.dlog_std[i]; }
    out[15] = h.dV;
}

// the extended head (entropy bonus, value clipping, approx_kl): in = mu[6] log_std[6] a[6] logp_old adv_n V old_V ret clip clip_vf ent_coef vf_coef inv_mb (28);
// out = head_out, then approx_kl entropy v_clipped (19)
template <class S> static void head_ex(const S* in, S* out) {
    const LossHeadEx<S> h = ppo_loss_head_ex<S>(in, in + 6, in + 12, in[18], in[19], in[20], in[21], in[22], in[23], in[24], in[25], in[26], in[27]);
    out[0] = h.pg_loss; out[1] = h.v_loss; out[2] = h.clipped;
    for (int i = 0; i < 6; i++) { out[3 + i] = h.dmu[i]; out[9 + i] = h.dlog_std[i]; }
    out[15] = h.dV; out[16] = h.approx_kl; out[17] = h.entropy; out[18] = h.v_clipped;
}

// hyper = max_grad_norm step_size (1 - beta1) beta2 (1 - beta2) eps sqrt(bc2) (7); g is replaced by the clipped gradient
template <class S> static void adam(int n, S* g, S* p, S* m, S* v, S grad_norm, const S* hyper) {
    const S coef = clip_coefficient<S>(grad_norm, hyper[0]);
    for (int i = 0; i < n; i++) g[i] = clip_adam_update<S>(g[i], coef, p[i], m[i], v[i], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5], hyper[6]);
}

extern "C" {

int lc_num_params(int obs_dim) { return obs_dim == 15 ? num_params(15) : obs_dim == 8 ? num_params(8) : -1; }
int lc_tensor_offset(int tensor, int obs_dim) { return tensor_offset(tensor, obs_dim); }
int lc_tensor_size(int tensor, int obs_dim) { return tensor_size(tensor, obs_dim); }

void lc_gae_d(int T, const double* reward, const double* code, const double* value, long in_stride, const double* boot, double next_v_last,
              double gamma, double lam, double* adv, double* ret, long out_stride) {
    gae_scan_env<double>(T, reward, code, value, in_stride, boot, next_v_last, gamma, lam, adv, ret, out_stride);
}
void lc_gae_f(int T, const float* reward, const float* code, const float* value, long in_stride, const float* boot, float next_v_last,
              float gamma, float lam, float* adv, float* ret, long out_stride) {
    gae_scan_env<float>(T, reward, code, value, in_stride, boot, next_v_last, gamma, lam, adv, ret, out_stride);
}
void lc_head_d(const double* in25, double* out16) { head<double>(in25, out16); }
void lc_head_f(const float* in25, float* out16) { head<float>(in25, out16); }
void lc_head_ex_d(const double* in28, double* out19) { head_ex<double>(in28, out19); }
void lc_head_ex_f(const float* in28, float* out19) { head_ex<float>(in28, out19); }
void lc_adam_d(int n, double* g, double* p, double* m, double* v, double grad_norm, const double* hyper7) { adam<double>(n, g, p, m, v, grad_norm, hyper7); }
void lc_adam_f(int n, float* g, float* p, float* m, float* v, float grad_norm, const float* hyper7) { adam<float>(n, g, p, m, v, grad_norm, hyper7); }

}
