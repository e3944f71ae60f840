// rewnormcheck.cpp -- the reward normalisation of so100_learn.hpp on the host, in the instantiation the kernels ship (double state, float
// out) and in the kernels' order: blocks of RN_BLOCK envs, the fixed tree inside a block, Chan's merge over the blocks in index order, the
// steps in t order.  Behind a C interface for ctypes (part of liblearncheck.so: tests/hostlibs.py; called by tests/reward_norm_support.py).  Test scaffolding only.
#include <stddef.h>
#include <vector>
#include "../../so100_mujoco_rl_amd/csrc/so100_learn.hpp"

using namespace so100::learn;

extern "C" {

int rn_block() { return RN_BLOCK; }

// chunk [T][N][row] floats (reward at rew_col, done code at code_col of a row); state [3 + N] in/out; out [T][N]
void rn_normalize(int T, int N, int row, int rew_col, int code_col, const float* chunk, double gamma, double epsilon, double clip, double* state, float* out) {
    const int G = (N + RN_BLOCK - 1)/RN_BLOCK;
    std::vector<double> part((size_t)T*G*2), denom(T);
    // scan: block by block, every step of a block before the next block (as a workgroup does)
    for (int g = 0; g < G; g++) {
        const int count = N - g*RN_BLOCK < RN_BLOCK ? N - g*RN_BLOCK : RN_BLOCK;
        double R[RN_BLOCK], slot[RN_BLOCK];
        for (int l = 0; l < RN_BLOCK; l++) R[l] = l < count ? state[3 + g*RN_BLOCK + l] : 0.0;
        for (int t = 0; t < T; t++) {
            const float* rowp = chunk + ((size_t)t*N + (size_t)g*RN_BLOCK)*row;
            for (int l = 0; l < RN_BLOCK; l++) {
                R[l] = l < count ? return_step<double>(R[l], gamma, (double)rowp[(size_t)l*row + rew_col]) : 0.0;
                slot[l] = R[l];
            }
            const double mean = block_mean<double>(block_tree_sum<double>(slot), count);
            for (int l = 0; l < RN_BLOCK; l++) slot[l] = l < count ? squared_deviation<double>(R[l], mean) : 0.0;
            const double m2 = block_tree_sum<double>(slot);
            part[((size_t)t*G + g)*2] = mean; part[((size_t)t*G + g)*2 + 1] = m2;
            for (int l = 0; l < count; l++) if (rowp[(size_t)l*row + code_col] != 0.0f) R[l] = 0.0;
        }
        for (int l = 0; l < count; l++) state[3 + g*RN_BLOCK + l] = R[l];
    }
    // merge: the blocks of a step in index order, then the steps in t order
    double mean = state[0], var = state[1], cnt = state[2];
    for (int t = 0; t < T; t++) {
        const double* p = &part[(size_t)t*G*2];
        double na = (double)(N < RN_BLOCK ? N : RN_BLOCK), m = p[0], m2 = p[1];
        for (int g = 1; g < G; g++) {
            const int left = N - g*RN_BLOCK;
            chan_merge<double>(na, m, m2, (double)(left < RN_BLOCK ? left : RN_BLOCK), p[2*g], p[2*g + 1]);
        }
        running_moment_update<double>(mean, var, cnt, m, m2/(double)N, (double)N);
        denom[t] = reward_denominator<double>(var, epsilon);
    }
    state[0] = mean; state[1] = var; state[2] = cnt;
    // scale
    for (long i = 0; i < (long)T*N; i++) out[i] = reward_scale<float, double>((double)chunk[(size_t)i*row + rew_col], denom[i/N], clip);
}

}  // extern "C"

#ifdef REWNORMCHECK_MAIN
// a stand-alone run for a host sanitizer: the header's known answer, then odd shapes (one env, a block and three envs, several blocks)
#include <stdio.h>
#include <math.h>
int main() {
    const float kc[2*2*2] = { 1.f, 0.f, 3.f, 1.f, 2.f, 0.f, -1.f, 0.f };
    double st[5] = { 0.0, 1.0, 1e-4, 0.0, 0.0 };
    float out[4];
    rn_normalize(2, 2, 2, 0, 1, kc, 0.99, 1e-8, 10.0, st, out);
    const double want[4] = { 0.99990004301, 2.99970006943, 1.20768642426, -0.60384321213 };
    int bad = 0;
    for (int i = 0; i < 4; i++) bad += fabs(out[i] - want[i]) > 2e-7;
    bad += fabs(st[0] - 1.497462563435914) > 1e-12 || fabs(st[1] - 2.7425312479735195) > 1e-12 || fabs(st[2] - 4.0001) > 1e-12 || fabs(st[3] - 2.99) > 1e-12 || st[4] != -1.0;
    const int shapes[3][2] = { { 3, 1 }, { 5, 67 }, { 9, 200 } };
    for (auto& s : shapes) {
        const int T = s[0], N = s[1], row = 5;
        std::vector<float> c((size_t)T*N*row), o((size_t)T*N);
        std::vector<double> state(3 + N, 0.0);
        state[1] = 1.0; state[2] = 1e-4;
        for (size_t i = 0; i < c.size(); i++) c[i] = (float)((i*2654435761u) % 1000u)/100.0f - 3.0f;
        for (long i = 0; i < (long)T*N; i++) c[(size_t)i*row + 4] = (float)((i*7) % 5 == 0);
        rn_normalize(T, N, row, 3, 4, c.data(), 0.99, 1e-8, 10.0, state.data(), o.data());
        for (float v : o) bad += !(v >= -10.0f && v <= 10.0f);
        bad += fabs(state[2] - (1e-4 + (double)T*N)) > 1e-9;
    }
    printf("rewnormcheck selftest: %s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
#endif
