// Host program (float and double, pair form and one-vector-at-a-time form) of the arm dynamics in the DEVICE physics header, on a fixed
// list of joint states: the ones where a term that is wrongly treated as zero would show (base at rest, one joint moving alone, v = 0,
// v = -0.0, every joint at a limit) and 64 seeded random ones.  Built without FMA contraction.  Prints
//   S <state> <label> q[6] v[6]                       the state (float values, exactly representable in both types)
//   R <f|d> <pk 0|1> <state> <48 hex words>           the bit patterns of bias[6], M[21] (arm_mass) and the LDL^T factor[21] (arm_factor)
// tests/test_arm_zero_terms_cpu.py compares the lines with each other, with the committed output of an earlier commit and with the fp64
// oracle.  Not a product path: libso100sim.so never links this file.  No input, no state: the same lines on every run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../so100_mujoco_rl_amd/csrc/so100_physics.hpp"
using namespace so100;

struct State { const char* label; float q[6], v[6]; };

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double uni() {                                        // splitmix64 -> [0, 1): the same list of states on every platform
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30))*0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27))*0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11)*(1.0/9007199254740992.0);
}
static float lo(int i) { return (float)so100g::JNT_RANGE[i][0]; }
static float hi(int i) { return (float)so100g::JNT_RANGE[i][1]; }
static void random_q(State& s) { for (int i = 0; i < 6; i++) s.q[i] = (float)(lo(i) + (hi(i) - lo(i))*uni()); }
static void random_v(State& s) { for (int i = 0; i < 6; i++) s.v[i] = (float)(-4.0 + 8.0*uni()); }

static std::vector<State> states() {
    std::vector<State> out;
    for (int k = 0; k < 64; k++) { State s{"random", {}, {}}; random_q(s); random_v(s); out.push_back(s); }
    out.push_back(State{"rest", {}, {}});
    for (int k = 0; k < 4; k++) { State s{"v=0", {}, {}}; random_q(s); out.push_back(s); }
    for (int j = 0; j < 6; j++)
        for (int sg = -1; sg <= 1; sg += 2) { State s{"one_joint", {}, {}}; random_q(s); s.v[j] = (float)(sg*(0.5 + 3.5*uni())); out.push_back(s); }
    for (int k = 0; k < 4; k++) {                            // all low, all high, alternating, alternating the other way
        State s{"limits", {}, {}};
        for (int i = 0; i < 6; i++) s.q[i] = (k == 0 || (k == 2 && i % 2 == 0) || (k == 3 && i % 2 == 1)) ? lo(i) : hi(i);
        random_v(s); out.push_back(s);
    }
    for (int k = 0; k < 2; k++) {
        State s{"v=-0", {}, {}};
        if (k) random_q(s);
        for (int i = 0; i < 6; i++) s.v[i] = -0.0f;
        out.push_back(s);
    }
    return out;
}

static void word(float x)  { uint32_t u; std::memcpy(&u, &x, 4); std::printf(" %08x", u); }
static void word(double x) { uint64_t u; std::memcpy(&u, &x, 8); std::printf(" %016llx", (unsigned long long)u); }

template <typename T, bool PK> static void run(char type, int idx, const State& s) {
    T q[6], v[6];
    for (int i = 0; i < 6; i++) { q[i] = (T)s.q[i]; v[i] = (T)s.v[i]; }
    Arm<T> A{};
    arm_trig(q, A);
    arm_bias<T, PK, true>(v, A);                             // both forms with the known-zero terms left out (the product's scalar-form
    arm_mass<T, PK, true>(A);                                // kernels keep them: the text they had)
    T M[21];
    for (int i = 0; i < 21; i++) M[i] = A.M[i];
    arm_factor(0u, A);
    std::printf("R %c %d %d", type, PK ? 1 : 0, idx);
    for (int i = 0; i < 6; i++) word(A.bias[i]);
    for (int i = 0; i < 21; i++) word(M[i]);
    for (int i = 0; i < 21; i++) word(A.M[i]);
    std::printf("\n");
}

int main() {
    const std::vector<State> st = states();
    for (int k = 0; k < (int)st.size(); k++) {
        const State& s = st[k];
        std::printf("S %d %s", k, s.label);
        for (int i = 0; i < 6; i++) std::printf(" %.9g", (double)s.q[i]);
        for (int i = 0; i < 6; i++) std::printf(" %.9g", (double)s.v[i]);
        std::printf("\n");
        run<float, true>('f', k, s); run<float, false>('f', k, s);
        run<double, true>('d', k, s); run<double, false>('d', k, s);
    }
    return 0;
}
