// learnterms.cpp -- the extended loss head of so100_learn.hpp (entropy bonus, value clipping, approx_kl) instantiated on the host in double
// and float, behind a C interface for ctypes (tests/learn_terms_support.py).  Test scaffolding only.
#include "../../so100_mujoco_rl_amd/csrc/so100_learn.hpp"

using namespace so100::learn;

// io layouts: in = mu[6] log_std[6] a[6] logp_old adv_n V old_V ret clip clip_vf ent_coef vf_coef inv_mb (28);
// out = pg_loss v_loss clipped dmu[6] dlog_std[6] dV approx_kl entropy v_clipped (19)
template <class S> static void head_ex(const S* in, S* out) {
    const LossHeadEx<S> h = ppo_loss_head_ex<S>(in, in + 6, in + 12, in[18], in[19], in[20], in[21], in[22], in[23], in[24], in[25], in[26], in[27]);
    out[0] = h.pg_loss; out[1] = h.v_loss; out[2] = h.clipped;
    for (int i = 0; i < 6; i++) { out[3 + i] = h.dmu[i]; out[9 + i] = h.dlog_std[i]; }
    out[15] = h.dV; out[16] = h.approx_kl; out[17] = h.entropy; out[18] = h.v_clipped;
}

extern "C" {

void lt_head_ex_d(const double* in28, double* out19) { head_ex<double>(in28, out19); }
void lt_head_ex_f(const float* in28, float* out19) { head_ex<float>(in28, out19); }

}
