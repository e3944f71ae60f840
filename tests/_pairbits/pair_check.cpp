// Host check that the pair form of the arm dynamics (V2 helpers, arm_bias / arm_mass / arm_trig_update with PK = true) computes every value by
// the same expression as the one-vector-at-a-time form (PK = false).  Built without FMA contraction, so both forms round
// identically and must agree bit for bit.  Prints one line per scalar type; exit status 1 on any mismatch.
#include <cstdio>
#include <cstring>
#include <random>
#include "../../so100_mujoco_rl_amd/csrc/so100_physics.hpp"
using namespace so100;

template <typename T> static int same(const T* a, const T* b, int n) { return std::memcmp(a, b, sizeof(T)*n) == 0; }

template <typename T> static int check(const char* name, int trials) {
    std::mt19937_64 rng(1234);
    std::uniform_real_distribution<double> ang(-3.2, 3.2), vel(-20.0, 20.0);
    int bad = 0;
    for (int t = 0; t < trials; t++) {
        T q[6], v[6];
        for (int i = 0; i < 6; i++) { q[i] = T(ang(rng)); v[i] = T(vel(rng)); }
        Arm<T> P{}, S{};
        arm_trig(q, P); arm_trig(q, S);
        arm_bias<T, true>(v, P); arm_bias<T, false>(v, S);
        arm_mass<T, true>(P); arm_mass<T, false>(S);
        if (!same(P.bias, S.bias, 6)) { bad++; if (bad < 4) std::printf("%s trial %d: arm_bias differs\n", name, t); }
        if (!same(P.M, S.M, 21)) { bad++; if (bad < 4) std::printf("%s trial %d: arm_mass differs\n", name, t); }
        T dq[6];
        for (int i = 0; i < 6; i++) dq[i] = T(0.002*vel(rng));
        arm_trig_update<T, true>(q, dq, P); arm_trig_update<T, false>(q, dq, S);
        if (!same(P.s, S.s, 6) || !same(P.c, S.c, 6)) { bad++; if (bad < 4) std::printf("%s trial %d: arm_trig_update differs\n", name, t); }
    }
    std::printf("%s: %d trials, %d mismatches\n", name, trials, bad);
    return bad;
}

int main() {
    const int bad = check<float>("float", 20000) + check<double>("double", 20000);
    return bad ? 1 : 0;
}
