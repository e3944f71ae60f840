// Host check that the pair form of the substep's solve path (so100_physics.hpp: arm_mass_p + ldl6_p, arm_tau_p, ldl6_forward_p + ldl6_back_p,
// arm_integrate_p) computes every value by the same expression as the scalar helpers (arm_mass + ldl6, arm_tau, ldl6_solve, arm_integrate).  Built without FMA contraction, so both
// forms round identically and must agree bit for bit.  Prints one line per scalar type; exit status 1 on any mismatch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include "../../so100_mujoco_rl_amd/csrc/so100_physics.hpp"
using namespace so100;

template <typename T> static int same(const T* a, const T* b, int n) { return std::memcmp(a, b, sizeof(T)*n) == 0; }
template <typename T> static void pack(const T a[6], V2<T> p[3]) { for (int j = 0; j < 3; j++) p[j] = V2<T>{ a[2*j], a[2*j + 1] }; }
template <typename T> static void packf(const T a[6], V2<T> p[3]) { for (int j = 0; j < 3; j++) p[j] = V2<T>{ a[2*j + 1], a[2*j] }; }      // the factor's order
template <typename T> static void unpackf(const V2<T> p[3], T a[6]) { for (int j = 0; j < 3; j++) { a[2*j + 1] = p[j].x; a[2*j] = p[j].y; } }
template <typename T> static void unpack(const V2<T> p[3], T a[6]) { for (int j = 0; j < 3; j++) { a[2*j] = p[j].x; a[2*j + 1] = p[j].y; } }

template <typename T> static int check(const char* name, int trials) {
    std::mt19937_64 rng(4321);
    std::uniform_real_distribution<double> ang(-3.2, 3.2), vel(-20.0, 20.0), near(-0.6, 0.6), bia(-6.0, 6.0), comp(-2e-7, 2e-7);
    int bad = 0, saturated = 0, free_ = 0;
    auto fail = [&](int t, const char* what) { bad++; if (bad < 6) std::printf("%s trial %d: %s differs\n", name, t, what); };
    for (int t = 0; t < trials; t++) {
        T q[6], v[6], ctrl[6], qc[6];
        for (int i = 0; i < 6; i++) {
            q[i] = T(ang(rng));
            v[i] = (t % 7 == 0 && i % 2 == 0) || t % 31 == 0 ? T(0) : T(vel(rng));           // both signs and zero
            ctrl[i] = t % 3 == 0 ? T(ang(rng)) : T(double(q[i]) + near(rng));                   // far targets saturate the force clamp, near ones do not
            qc[i] = T(comp(rng));                                                               // a running compensation that is not zero
        }
        Arm<T> A{};
        arm_trig(q, A);
        arm_mass<T, true>(A);                                   // M = arm_mass(q), armature on the diagonal
        for (int i = 0; i < 6; i++) A.bias[i] = T(bia(rng));
        // CRBA with the rows 5 | 4 and 3 | 2 left as pairs, then the factor on them.  The entries the pairs carry are NaN in the scalar array
        // on the way in: neither helper may read them there.
        Arm<T> B{};
        for (int i = 0; i < 6; i++) { B.s[i] = A.s[i]; B.c[i] = A.c[i]; }
        for (int i = 0; i < 21; i++) B.M[i] = std::numeric_limits<T>::quiet_NaN();
        V2<T> R5[4], R3[2];
        arm_mass_p<T>(B, R5, R3);
        T Mp[21];
        for (int i = 0; i < 21; i++) Mp[i] = B.M[i];
        for (int k = 0; k < 4; k++) { Mp[SO100_TRI(5, k)] = R5[k].x; Mp[SO100_TRI(4, k)] = R5[k].y; }
        for (int k = 0; k < 2; k++) { Mp[SO100_TRI(3, k)] = R3[k].x; Mp[SO100_TRI(2, k)] = R3[k].y; }
        if (!same(A.M, Mp, 21)) fail(t, "arm_mass_p");
        ldl6(A.M, A.Dinv);
        ldl6_p<T>(B.M, R5, R3, B.Dinv);
        if (!same(A.M, B.M, 21) || !same(A.Dinv, B.Dinv, 6)) fail(t, "factor");
        for (int k = 0; k < 4; k++) if (!same(&R5[k].x, &A.M[SO100_TRI(5, k)], 1) || !same(&R5[k].y, &A.M[SO100_TRI(4, k)], 1)) fail(t, "factor's pairs (5 | 4)");
        for (int k = 0; k < 2; k++) if (!same(&R3[k].x, &A.M[SO100_TRI(3, k)], 1) || !same(&R3[k].y, &A.M[SO100_TRI(2, k)], 1)) fail(t, "factor's pairs (3 | 2)");
        // tau: arm_tau's own servo expression, then its last line on the pairs
        T tau_s[6], servo[6];
        arm_tau(q, v, ctrl, A, tau_s);
        for (int i = 0; i < 6; i++) {
            const T u = tclamp(ctrl[i], T(-so100g::ACT_CTRL), T(so100g::ACT_CTRL));
            T f = T(so100g::ACT_KP)*u - T(so100g::ACT_KP)*q[i] - T(so100g::ACT_KV[i])*v[i];
            servo[i] = tclamp(f, T(-so100g::ACT_FORCE), T(so100g::ACT_FORCE));
            if (servo[i] == T(so100g::ACT_FORCE) || servo[i] == T(-so100g::ACT_FORCE)) saturated++; else free_++;
        }
        V2<T> sp[3], bp[3], xp[3];
        T tau_p[6];
        packf(servo, sp); packf(A.bias, bp);                  // the right-hand side in the order of the factor's pairs
        arm_tau_p<T>(sp, bp, xp);
        unpackf(xp, tau_p);
        if (!same(tau_s, tau_p, 6)) fail(t, "tau");
        // forward substitution alone (the scalar code's first loop), then the whole solve
        T fw_s[6], fw_p[6], acc_s[6], acc_p[6];
        for (int i = 0; i < 6; i++) { fw_s[i] = tau_s[i]; acc_s[i] = tau_s[i]; }
        for (int i = 1; i < 6; i++)
            for (int k = 0; k < i; k++) fw_s[i] -= A.M[SO100_TRI(i, k)]*fw_s[k];
        ldl6_forward_p<T>(A.M, xp);
        unpackf(xp, fw_p);
        if (!same(fw_s, fw_p, 6)) fail(t, "forward substitution");
        ldl6_solve(A.M, A.Dinv, acc_s);
        V2<T> ap[3];
        ldl6_back_p<T>(A.M, A.Dinv, xp, ap);                  // the solution as joint pairs
        unpack(ap, acc_p);
        pack(acc_s, xp);
        if (!same(acc_s, acc_p, 6)) fail(t, "solve");
        // integration; every 5th trial with a zero acceleration in some joints
        if (t % 5 == 0) { acc_s[1] = T(0); acc_s[4] = T(0); pack(acc_s, xp); }
        T q_s[6], v_s[6], c_s[6], d_s[6], q_p[6], v_p[6], c_p[6], d_p[6];
        for (int i = 0; i < 6; i++) { q_s[i] = q[i]; v_s[i] = v[i]; c_s[i] = qc[i]; }
        arm_integrate(q_s, v_s, c_s, acc_s, d_s);
        V2<T> qp[3], vp[3], cp[3], dp[3];
        pack(q, qp); pack(v, vp); pack(qc, cp);
        arm_integrate_p<T>(qp, vp, cp, xp, dp);
        unpack(qp, q_p); unpack(vp, v_p); unpack(cp, c_p); unpack(dp, d_p);
        if (!same(q_s, q_p, 6) || !same(v_s, v_p, 6) || !same(c_s, c_p, 6) || !same(d_s, d_p, 6)) fail(t, "integration");
        // a NaN in one joint's acceleration stays in that joint: the other half of its pair is the value it was
        const int j = t % 6;
        T acc_n[6];
        for (int i = 0; i < 6; i++) acc_n[i] = acc_s[i];
        acc_n[j] = std::numeric_limits<T>::quiet_NaN();
        pack(q, qp); pack(v, vp); pack(qc, cp); pack(acc_n, xp);
        arm_integrate_p<T>(qp, vp, cp, xp, dp);
        unpack(qp, q_p); unpack(vp, v_p); unpack(cp, c_p); unpack(dp, d_p);
        for (int i = 0; i < 6; i++) {
            if (i == j) { if (!std::isnan(q_p[i]) || !std::isnan(v_p[i])) fail(t, "NaN joint"); }
            else if (!same(q_s + i, q_p + i, 1) || !same(v_s + i, v_p + i, 1) || !same(c_s + i, c_p + i, 1) || !same(d_s + i, d_p + i, 1)) fail(t, "NaN neighbour");
        }
    }
    if (saturated == 0 || free_ == 0) { bad++; std::printf("%s: the force clamp was %s\n", name, saturated ? "always reached" : "never reached"); }
    std::printf("%s: %d trials, %d mismatches\n", name, trials, bad);
    return bad;
}

int main() {
    const int bad = check<float>("float", 20000) + check<double>("double", 20000);
    return bad ? 1 : 0;
}
