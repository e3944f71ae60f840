// forwardcheck.cpp -- the forward-dynamics query of so100_forward.hpp on the host, in double (held to the fp64 oracle) and in float (the
// arithmetic the kernel ships, without FMA contraction), with a group of one lane per problem, behind a C interface for ctypes
// (built by tests/Makefile, loaded by tests/hostlibs.py, called by tests/forward_support.py).  Arrays are problem-major here ([n][k]); the SoA layout is the kernel's matter.
// Test scaffolding only.
#include <stdint.h>
#include "../../so100_mujoco_rl_amd/csrc/so100_forward.hpp"

using namespace so100;

namespace {

// qvel null: zero; ctrl null: the joint angles (hold the pose).  Every output is required.
template <typename T> void forward(long n, const T* qpos, const T* qvel, const T* ctrl, unsigned flags, int solver_iters, int contact_iters,
                                   T* qacc, T* qfrc, int32_t* ncon, int32_t* dropped, int32_t* kind, int32_t* feat, T* pos, T* frame, T* dist,
                                   T* force, T* pad_force, T* residual) {
    for (long i = 0; i < n; i++) {
        T v[12], u[6];
        for (int k = 0; k < 12; k++) v[k] = qvel ? qvel[12*i + k] : T(0);
        for (int k = 0; k < 6; k++) u[k] = ctrl ? ctrl[6*i + k] : qpos[13*i + k];
        T records[MAXC*CF], dists[MAXC]; unsigned char codes[MAXC];
        ForwardStore<T, 1, false, 1> cs(records, codes, dists, 0, 0);
        ForwardResult<T> R;
        forward_dynamics<T>(qpos + 13*i, v, u, flags, solver_iters, contact_iters, cs, R,
                            [&](int s, int kd, int ft, const T* p, const T* fr, T d, const T* f) {
            const long o = FWD_MAXCON*i + s;
            kind[o] = kd; feat[o] = ft; dist[o] = d;
            for (int k = 0; k < 3; k++) { pos[3*o + k] = p[k]; force[3*o + k] = f[k]; }
            for (int k = 0; k < 9; k++) frame[9*o + k] = fr[k];
        });
        for (int k = 0; k < 12; k++) { qacc[12*i + k] = R.qacc[k]; qfrc[12*i + k] = R.qfrc_constraint[k]; }
        for (int k = 0; k < 8; k++) pad_force[8*i + k] = R.pad_force[k];
        ncon[i] = R.ncon; dropped[i] = R.dropped; residual[i] = R.residual;
    }
}

}  // namespace

extern "C" {

#define FC_INSTANCE(S, T) \
    void fc_forward_##S(long n, const T* qpos, const T* qvel, const T* ctrl, unsigned flags, int solver_iters, int contact_iters, \
                        T* qacc, T* qfrc, int32_t* ncon, int32_t* dropped, int32_t* kind, int32_t* feat, T* pos, T* frame, T* dist, \
                        T* force, T* pad_force, T* residual) { \
        forward<T>(n, qpos, qvel, ctrl, flags, solver_iters, contact_iters, qacc, qfrc, ncon, dropped, kind, feat, pos, frame, dist, force, pad_force, residual); }
FC_INSTANCE(d, double)
FC_INSTANCE(f, float)
#undef FC_INSTANCE

}  // extern "C"

#ifdef FORWARDCHECK_MAIN
// a stand-alone run for a host sanitizer: both precisions over states of the kinds the tests' recipe visits -- pads pressed into the floor, the
// jaw closed on a cube between the pads, a pad against a cube lying on the floor, a link proxy on the floor and against the cube --, each with
// its velocities, with qvel null and with the cube pinned
#include <math.h>
#include <stdio.h>
#include <vector>
namespace {
uint32_t g_state = 2024u;
double uniform() { g_state = g_state*1664525u + 1013904223u; return (double)(g_state >> 8)/16777216.0; }

struct Case { double q[6], cube[3], quat[4]; unsigned flags; };
const unsigned REFP = 1u | 2u | 4u | 16u, C5 = REFP | 32u, LINKS = REFP | 64u, LCUBE = LINKS | 128u;
// base poses: (1) pads near the floor; (2) tests/scenes.grasp_state: gripper horizontal, cube between the jaws; (3) arm low, the cube lying on
// the floor under the jaws; (4) the wrist on the table; (5) the cube against the upper arm.  The random offsets below move them in and out of contact.
const Case BASE[] = {
    { { 0.0, -1.9, 1.6, 0.3, 1.5708, 0.1 }, { 0.15, -0.25, 0.0099 }, { 1, 0, 0, 0 }, C5 },
    { { 0.0, -3.0, 2.6, 1.2, 0.0, 0.3 }, { 0.15, -0.25, 0.0099 }, { 1, 0, 0, 0 }, REFP },
    { { 0.0, -3.0, 2.6, 1.2, 0.0, 0.3 }, { 0.0, -0.30, 0.0099 }, { 1, 0, 0, 0 }, C5 },
    { { 0.3, -3.1, 3.0, 0.2, 0.0, 0.0 }, { 0.15, -0.25, 0.0099 }, { 1, 0, 0, 0 }, LINKS },
    { { 0.0, -1.5, 1.5, 0.5, 0.0, 0.2 }, { 0.0, -0.10, 0.12 }, { 0.9, 0.1, 0.3, 0.2 }, LCUBE },
};

template <typename T> int run(const char* name) {
    const long per = 64, nb = (long)(sizeof BASE/sizeof BASE[0]), n = per*nb;
    int bad = 0; long contacts = 0, in_contact = 0;
    for (long b = 0; b < nb; b++) {
        std::vector<T> qpos(13*per), qvel(12*per), ctrl(6*per), qacc(12*per), qfrc(12*per), pos(60*per), frame(180*per), dist(20*per), force(60*per), pf(8*per), res(per);
        std::vector<int32_t> ncon(per), drop(per), kind(20*per), feat(20*per);
        for (long i = 0; i < per; i++) {
            for (int k = 0; k < 6; k++) { qpos[13*i + k] = T(BASE[b].q[k] + 0.04*(uniform() - 0.5)); ctrl[6*i + k] = qpos[13*i + k] + T(0.15*(uniform() - 0.5)); qvel[12*i + k] = T(0.6*(uniform() - 0.5)); }
            if (b == 0) {                                   // the cube between the jaws: 88 mm along the fixed jaw's -y, found from the pose itself
                Arm<T> A; WorldFK<T> W; arm_trig(&qpos[13*i], A); world_fk(A.s, A.c, W);
                const T o[3] = { T(-0.0026), T(-0.088), T(0) };
                for (int k = 0; k < 3; k++) qpos[13*i + 6 + k] = W.o[4][k] + W.R4[3*k]*o[0] + W.R4[3*k + 1]*o[1] + W.R4[3*k + 2]*o[2] + T(0.002*(uniform() - 0.5));
                qpos[13*i + 9] = T(0); qpos[13*i + 10] = T(0.02); qpos[13*i + 11] = T(1); qpos[13*i + 12] = T(0.01);
                qpos[13*i + 5] = T(0.06 + 0.02*uniform());
            } else {
                for (int k = 0; k < 3; k++) qpos[13*i + 6 + k] = T(BASE[b].cube[k] + (k < 2 ? 0.02*(uniform() - 0.5) : 0.0));
                for (int k = 0; k < 4; k++) qpos[13*i + 9 + k] = T(BASE[b].quat[k]);
            }
            for (int k = 6; k < 12; k++) qvel[12*i + k] = T(0.02*(uniform() - 0.5));
        }
        for (int pass = 0; pass < 3; pass++) {
            const unsigned flags = pass == 2 ? ((BASE[b].flags & ~(4u | 32u | 128u)) | 8u) : BASE[b].flags;
            forward<T>(per, qpos.data(), pass == 1 ? nullptr : qvel.data(), pass == 1 ? nullptr : ctrl.data(), flags, 64, 64, qacc.data(), qfrc.data(), ncon.data(),
                       drop.data(), kind.data(), feat.data(), pos.data(), frame.data(), dist.data(), force.data(), pf.data(), res.data());
            for (long i = 0; i < per; i++) {
                bad += ncon[i] < 0 || ncon[i] > FWD_MAXCON || drop[i] < 0 || !(res[i] == res[i]);
                for (int k = 0; k < 12; k++) bad += !(qacc[12*i + k] == qacc[12*i + k]) || !(qfrc[12*i + k] == qfrc[12*i + k]);
                if (pass == 2) for (int k = 6; k < 12; k++) bad += qacc[12*i + k] != T(0);
                for (int s = 0; s < FWD_MAXCON; s++) {
                    const long o = 20*i + s;
                    if (s < ncon[i]) bad += feat[o] < 0 || kind[o] < 0 || kind[o] > 4 || !(force[3*o] >= T(0)) || !(dist[o] <= T(0)) || (pass == 2 && kind[o] == 0);
                    else bad += feat[o] != -1 || kind[o] != 0 || force[3*o] != T(0) || dist[o] != T(0);
                }
                if (pass == 0) { contacts += ncon[i]; in_contact += ncon[i] > 0; }
            }
        }
    }
    // a NaN input: no contacts, NaN accelerations
    {
        std::vector<T> qpos(13, T(0)), qacc(12), qfrc(12), pos(60), frame(180), dist(20), force(60), pf(8), res(1);
        std::vector<int32_t> ncon(1), drop(1), kind(20), feat(20);
        qpos[9] = T(1); qpos[2] = T(NAN);
        forward<T>(1, qpos.data(), nullptr, nullptr, C5, 64, 64, qacc.data(), qfrc.data(), ncon.data(), drop.data(), kind.data(), feat.data(), pos.data(),
                   frame.data(), dist.data(), force.data(), pf.data(), res.data());
        bad += ncon[0] != 0;
        for (int k = 0; k < 12; k++) bad += qacc[k] == qacc[k];
    }
    bad += in_contact < n/4;
    printf("forwardcheck selftest (%s): %ld problems, %ld in contact, %ld contacts: %s\n", name, n, in_contact, contacts, bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace
int main() {
    const int bad = run<double>("double") + run<float>("float");
    return bad != 0;
}
#endif
