// obsnormcheck.cpp -- the observation normalisation of so100_learn.hpp on the host, in the instantiation the kernels ship (double moments and
// fold, float load and outputs) and in the kernels' order: blocks of ON_BLOCK rows with the fixed tree inside a block, groups of ON_GROUP blocks
// merged in block order, the groups merged in group order, then the running update.  Behind a C interface for ctypes
// (part of liblearncheck.so: tests/hostlibs.py; called by tests/obs_norm_support.py).  Test scaffolding only.
#include <stddef.h>
#include <vector>
#include "../../so100_mujoco_rl_amd/csrc/so100_learn.hpp"

using namespace so100::learn;

extern "C" {

int on_block() { return ON_BLOCK; }
int on_group() { return ON_GROUP; }

// chunk [rows][row] floats, the observation of a row in its first od entries; state [2 od + 1] in/out (mean, var, count)
void on_update(long rows, int od, int row, const float* chunk, double* state) {
    const long B = on_blocks(rows), G = on_groups(rows);
    std::vector<double> part((size_t)B*od*2), grp((size_t)G*od*3);
    // block moments: what one workgroup does
    for (long b = 0; b < B; b++) {
        const long count = on_block_count(rows, b);
        for (int i = 0; i < od; i++) {
            double x[ON_BLOCK], slot[ON_BLOCK];
            for (int j = 0; j < ON_BLOCK; j++) { x[j] = j < count ? (double)chunk[(size_t)(b*ON_BLOCK + j)*row + i] : 0.0; slot[j] = x[j]; }
            const double mean = block_mean<double>(obs_block_tree_sum<double>(slot), (int)count);
            for (int j = 0; j < ON_BLOCK; j++) slot[j] = j < count ? squared_deviation<double>(x[j], mean) : 0.0;
            part[((size_t)b*od + i)*2] = mean; part[((size_t)b*od + i)*2 + 1] = obs_block_tree_sum<double>(slot);
        }
    }
    // the groups, then per dimension the groups' merge and the running update
    for (long g = 0; g < G; g++)
        for (int i = 0; i < od; i++) {
            const long b0 = g*ON_GROUP, b1 = b0 + ON_GROUP < B ? b0 + ON_GROUP : B;
            double* o = &grp[((size_t)g*od + i)*3];
            obs_group_merge<double>(part.data() + 2*i, 2L*od, rows, b0, b1, o[0], o[1], o[2]);
        }
    const double count0 = state[2*od];
    double count = count0;
    for (int i = 0; i < od; i++) {
        count = count0;
        obs_moment_update<double>(grp.data() + 3*i, 3L*od, G, rows, state[i], state[od + i], count);
    }
    state[2*od] = count;
}

// params / folded [P]; first[4]: offsets of pi_w0, pi_b0, vf_w0, vf_b0 in the block; norm [2 od] out
void on_fold(int od, int P, const int* first, const double* state, double epsilon, const float* params, float* folded, float* norm) {
    std::vector<double> inv(od);
    for (int i = 0; i < od; i++) { inv[i] = obs_inv_std<double>(state[od + i], epsilon); norm[i] = (float)state[i]; norm[od + i] = (float)inv[i]; }
    for (int p = 0; p < P; p++) folded[p] = params[p];
    for (int tw = 0; tw < 2; tw++) {
        const int oW = first[2*tw], oB = first[2*tw + 1];
        for (int j = 0; j < HID; j++) obs_fold_row<double>(od, params + oW + j*od, params[oB + j], state, inv.data(), folded + oW + j*od, folded[oB + j]);
    }
}

// out [n][od] = the learner's load of obs [n][od] under norm [2 od]
void on_normalize(long n, int od, const float* obs, const float* norm, float* out) {
    for (long r = 0; r < n; r++)
        for (int i = 0; i < od; i++) out[r*od + i] = obs_normalized(obs[r*od + i], norm[i], norm[od + i]);
}

}  // extern "C"

#ifdef OBSNORMCHECK_MAIN
// a stand-alone run for a host sanitizer: the header's known answer, then odd shapes (one row, a block and a remainder, several groups)
#include <stdio.h>
#include <math.h>
using namespace so100;
int main() {
    int bad = 0;
    {
        const float c[2*12] = { 1.f, 10.f, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3.f, 14.f, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        double st[5] = { 0.0, 0.0, 1.0, 1.0, 1e-4 };
        on_update(2, 2, 12, c, st);
        const double want[5] = { 1.9999000049997500, 11.999400029998500, 1.0001999800014999, 4.0070492875536214, 2.0001 };
        for (int i = 0; i < 5; i++) bad += fabs(st[i] - want[i]) > 1e-13*fabs(want[i]);
        // a "block" of P = 6 floats: w0 [1][2] at 0, b0 at 2, the second tower's at 3 and 5 (HID rows are read: keep to row 0 by hand)
        double inv[2] = { obs_inv_std<double>(st[2], 1e-8), obs_inv_std<double>(st[3], 1e-8) };
        const float w[2] = { 0.5f, -0.25f };
        float wo[2], bo;
        obs_fold_row<double>(2, w, 0.125f, st, inv, wo, bo);
        bad += fabs(wo[0] - 0.49995000999762556) > 6e-8 || fabs(wo[1] + 0.12489000009602631) > 2e-8 || fabs(bo - 0.62375504340489438) > 1.2e-7;
        bad += obs_normalized(3.0f, 1.0f, 0.5f) != 1.0f;
    }
    const long shapes[4] = { 1, 259, 64*256 + 5, 3*64*256 + 300 };
    for (long rows : shapes) {
        const int od = 15, row = 25, P = num_params(od);
        std::vector<float> c((size_t)rows*row);
        for (size_t i = 0; i < c.size(); i++) c[i] = (float)((i*2654435761u) % 1000u)/100.0f - 3.0f;
        std::vector<double> st(2*od + 1, 0.0);
        for (int i = 0; i < od; i++) st[od + i] = 1.0;
        st[2*od] = 1e-4;
        on_update(rows, od, row, c.data(), st.data());
        bad += fabs(st[2*od] - (1e-4 + (double)rows)) > 1e-9;
        for (int i = 0; i < od; i++) bad += !(st[i] > -3.1 && st[i] < 7.1) || !(st[od + i] >= 0.0);
        std::vector<float> prm(P), fol(P), norm(2*od);
        for (int p = 0; p < P; p++) prm[p] = (float)(p % 17)/17.0f - 0.5f;
        const int first[4] = { tensor_offset(T_pi_w0, od), tensor_offset(T_pi_b0, od), tensor_offset(T_vf_w0, od), tensor_offset(T_vf_b0, od) };
        on_fold(od, P, first, st.data(), 1e-8, prm.data(), fol.data(), norm.data());
        bad += fol[tensor_offset(T_pi_w1, od)] != prm[tensor_offset(T_pi_w1, od)] || fol[P - 1] != prm[P - 1];
        std::vector<float> out((size_t)od);
        on_normalize(1, od, c.data(), norm.data(), out.data());
        for (float v : out) bad += !(v == v);
    }
    printf("obsnormcheck selftest: %s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
#endif
