// so100_lqr.hpp -- the LQR query: the time-varying Riccati backward pass and the linear forward pass of an iLQR / LQR / MPC iteration on the
// linearisation the derivatives query gives (include/so100_query.h, so100_query_lqr).
//
// Templated on the scalar like so100_derivative.hpp: the pieces every form shares (the index map of the arm form, the 6 x 6 Cholesky and its
// solve) are used by the kernel (so100_query_lqr.hip) in float; lqr_problem, the whole recursion for one problem written element by element,
// is what the host twin (tests/_lqrcheck) instantiates in double and in float.  No physics: nothing of the model is read here.
//
// Per problem, horizon T, n = 24 (the full tangent state) or 12 (the arm block: tangent indices 0..5 and 12..17), 6 controls:
//     Vx = lx_T, Vxx = lxx_T;  for t = T-1 .. 0, with G = [A_t | B_t] (n x (n + 6)):
//         H = G' Vxx G + [lxx lux'; lux luu]        -> Qxx, Qux, Quu are its blocks
//         (Qx; Qu) = G' Vx + (lx; lu)
//         Quu_r = Quu + reg I = L L'                 (a pivot <= 0 or not finite: the problem fails at this t)
//         k = -Quu_r^-1 Qu,  K = -Quu_r^-1 Qux
//         dV1 += k'Qu,  dV2 += k'Quu k / 2          (the unregularised Quu, here and below)
//         Vx  = Qx  + K'(Quu k + Qu) + Qux'k
//         Vxx = Qxx + K'(Quu K + Qux) + Qux'K,  Vxx <- (Vxx + Vxx')/2
// and, if asked for, dx_0 = dx0, du_t = alpha k_t + K_t dx_t (with u: clamp(u_t + that, u_lo, u_hi) - u_t), dx_{t+1} = A_t dx_t + B_t du_t.
// lxx_T is symmetrised like every later Vxx.  A and B are always in the derivatives query's layout ([T][M][24][24], [T][M][24][6]); every
// other array is in the n of the call, problem-major.
// With a regulariser per problem (so100_query_lqr_reg, so100_query_reg_schedule): lqr_reg_raise, lqr_reg_again and lqr_reg_next
// are what the kernels, the twin (tests/_lqrregcheck) and the schedule share; lqr_reg_problem is the twin's retry loop round lqr_problem.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef SO100_HD
#if defined(__HIPCC__)
#define SO100_HD __host__ __device__ __forceinline__
#else
#define SO100_HD inline
#endif
#endif

namespace so100 {

constexpr int LQR_NU = 6;                                    // SO100_LQR_NU
constexpr int LQR_MAX_T = 4096;                              // SO100_LQR_MAX_T

template <typename T> struct LqrArgs {
    const T *A, *B, *lx, *lxx, *lu, *luu, *lux, *u, *dx0;
    int horizon;
    T reg, alpha, u_lo, u_hi;
    T *k, *K, *Vx0, *Vxx0, *dV, *du, *dx;
    int32_t* bad;
};

// index a of the call's state in the 24 of A and B
template <int N> SO100_HD constexpr int lqr_idx(int a) { return N == 24 ? a : (a < 6 ? a : a + 6); }

SO100_HD float  lqr_sqrt(float x)  { return __builtin_sqrtf(x); }
SO100_HD double lqr_sqrt(double x) { return __builtin_sqrt(x); }
template <typename T> SO100_HD bool lqr_finite(T x) { return x*T(0) == T(0); }
template <typename T> SO100_HD T lqr_nan() { return T(__builtin_nanf("")); }

// Q + reg I = L L' (the lower triangle of Q is read); inv: 1 / L_jj.  false where a pivot is <= 0 or not finite; the factor is then completed
// on a pivot of 1 so that every caller runs the same instructions (its result is not used).
template <typename T> SO100_HD bool lqr_chol6(const T Q[6][6], T reg, T L[6][6], T inv[6]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        T d = Q[j][j] + reg;
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[j][k]*L[j][k];
        if (!(d > T(0)) || !lqr_finite(d)) { ok = false; d = T(1); }
        const T s = lqr_sqrt(d);
        L[j][j] = s; inv[j] = T(1)/s;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            T v = Q[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k]*L[j][k];
            L[i][j] = v*inv[j];
        }
    }
    return ok;
}

// x = -(L L')^-1 b
template <typename T> SO100_HD void lqr_solve6(const T L[6][6], const T inv[6], const T b[6], T x[6]) {
    T y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        T v = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i][k]*y[k];
        y[i] = v*inv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        T v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v -= L[k][i]*x[k];
        x[i] = v*inv[i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = -x[i];
}

// A failed problem m of M: bad is written and every float output is NaN.
template <typename T, int N> inline void lqr_failed(const LqrArgs<T>& a, size_t M, size_t m, int bad) {
    constexpr int NU = LQR_NU;
    const int TT = a.horizon;
    const T nan = lqr_nan<T>();
    if (a.bad) a.bad[m] = bad;
    for (int t = 0; t <= TT; t++) {
        const size_t p = (size_t)t*M + m;
        if (a.dx) for (int i = 0; i < N; i++) a.dx[p*N + i] = nan;
        if (t == TT) break;
        if (a.k) for (int i = 0; i < NU; i++) a.k[p*NU + i] = nan;
        if (a.K) for (int i = 0; i < NU*N; i++) a.K[p*NU*N + i] = nan;
        if (a.du) for (int i = 0; i < NU; i++) a.du[p*NU + i] = nan;
    }
    if (a.Vx0) for (int i = 0; i < N; i++) a.Vx0[m*N + i] = nan;
    if (a.Vxx0) for (int i = 0; i < N*N; i++) a.Vxx0[m*(N*N) + i] = nan;
    if (a.dV) a.dV[2*m] = a.dV[2*m + 1] = nan;
}

// The whole query for problem m of M, element by element: the twin's form (the kernel deals the same arithmetic over a wave).  The inputs of
// step t are tested for finiteness as they are read: bad = T at the first step (from the end) that has one, bad = t where the factor fails.
// Returns bad.
template <typename T, int N> inline int lqr_problem(const LqrArgs<T>& a, size_t M, size_t m) {
    constexpr int NU = LQR_NU, NP = N + NU;
    const int TT = a.horizon;
    T Vx[N], Vxx[N][N], dV1 = T(0), dV2 = T(0);
    int bad = -1;
    bool fin = true;
    {
        const T* lx = a.lx + ((size_t)TT*M + m)*N; const T* lxx = a.lxx + ((size_t)TT*M + m)*(N*N);
        for (int i = 0; i < N; i++) { Vx[i] = lx[i]; fin = fin && lqr_finite(lx[i]); }
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) { Vxx[i][j] = T(0.5)*(lxx[i*N + j] + lxx[j*N + i]); fin = fin && lqr_finite(lxx[i*N + j]); }
        if (a.dx0) for (int i = 0; i < N; i++) fin = fin && lqr_finite(a.dx0[m*N + i]);
    }
    if (!fin) bad = TT;
    for (int t = TT - 1; t >= 0 && bad < 0; t--) {
        const size_t p = (size_t)t*M + m;
        const T* At = a.A + p*576; const T* Bt = a.B + p*144;
        T G[N][NP], C[NP][NP], c[NP];                        // the step's dynamics; its cost Hessian [lxx lux'; lux luu] and gradient (lx; lu)
        for (int i = 0; i < N; i++) {
            for (int j = 0; j < N; j++) G[i][j] = At[lqr_idx<N>(i)*24 + lqr_idx<N>(j)];
            for (int j = 0; j < NU; j++) G[i][N + j] = Bt[lqr_idx<N>(i)*NU + j];
        }
        for (int i = 0; i < NP; i++) {
            c[i] = i < N ? a.lx[p*N + i] : (a.lu ? a.lu[p*NU + (i - N)] : T(0));
            for (int j = 0; j < NP; j++)
                C[i][j] = i < N ? (j < N ? a.lxx[p*(N*N) + i*N + j] : T(0))
                                : (j < N ? (a.lux ? a.lux[(p*NU + (i - N))*N + j] : T(0)) : (a.luu ? a.luu[p*(NU*NU) + (i - N)*NU + (j - N)] : T(0)));
        }
        for (int i = 0; i < N; i++) for (int j = 0; j < NP; j++) fin = fin && lqr_finite(G[i][j]);
        for (int i = 0; i < NP; i++) { fin = fin && lqr_finite(c[i]); for (int j = 0; j < NP; j++) fin = fin && lqr_finite(C[i][j]); }
        if (a.u) for (int j = 0; j < NU; j++) fin = fin && lqr_finite(a.u[p*NU + j]);
        if (!fin) { bad = TT; break; }
        T W[N][NP], H[NP][NP], q[NP];
        for (int i = 0; i < N; i++)
            for (int j = 0; j < NP; j++) { T s = T(0); for (int k = 0; k < N; k++) s += Vxx[i][k]*G[k][j]; W[i][j] = s; }
        for (int i = 0; i < NP; i++) {
            for (int j = 0; j < NP; j++) { T s = T(0); for (int k = 0; k < N; k++) s += G[k][i]*W[k][j]; H[i][j] = s + C[i][j]; }
            T s = T(0); for (int k = 0; k < N; k++) s += G[k][i]*Vx[k];
            q[i] = s + c[i];
        }
        T Quu[6][6], Qu[6], L[6][6], inv[6], kk[6], Qk[6];
        for (int i = 0; i < NU; i++) { Qu[i] = q[N + i]; for (int j = 0; j < NU; j++) Quu[i][j] = H[N + i][N + j]; }
        if (!lqr_chol6(Quu, a.reg, L, inv)) { bad = t; break; }
        lqr_solve6(L, inv, Qu, kk);
        for (int i = 0; i < NU; i++) { T s = T(0); for (int j = 0; j < NU; j++) s += Quu[i][j]*kk[j]; Qk[i] = s; }
        { T s1 = T(0), s2 = T(0); for (int i = 0; i < NU; i++) { s1 += kk[i]*Qu[i]; s2 += kk[i]*Qk[i]; } dV1 += s1; dV2 += T(0.5)*s2; }
        T K[6][N], QK[6][N];
        for (int j = 0; j < N; j++) {
            T b[6], x[6];
            for (int i = 0; i < NU; i++) b[i] = H[N + i][j];
            lqr_solve6(L, inv, b, x);
            for (int i = 0; i < NU; i++) K[i][j] = x[i];
            for (int i = 0; i < NU; i++) { T s = T(0); for (int l = 0; l < NU; l++) s += Quu[i][l]*x[l]; QK[i][j] = s; }
        }
        T Vn[N][N];
        for (int j = 0; j < N; j++) {
            T s = q[j];
            for (int i = 0; i < NU; i++) s += K[i][j]*(Qk[i] + Qu[i]) + H[N + i][j]*kk[i];
            Vx[j] = s;
        }
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) {
                T s = H[i][j];
                for (int l = 0; l < NU; l++) s += K[l][i]*(QK[l][j] + H[N + l][j]) + H[N + l][i]*K[l][j];
                Vn[i][j] = s;
            }
        for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) Vxx[i][j] = T(0.5)*(Vn[i][j] + Vn[j][i]);
        if (a.k) for (int i = 0; i < NU; i++) a.k[p*NU + i] = kk[i];
        if (a.K) for (int i = 0; i < NU; i++) for (int j = 0; j < N; j++) a.K[(p*NU + i)*N + j] = K[i][j];
    }
    if (bad >= 0) { lqr_failed<T, N>(a, M, m, bad); return bad; }
    if (a.bad) a.bad[m] = bad;
    if (a.Vx0) for (int i = 0; i < N; i++) a.Vx0[m*N + i] = Vx[i];
    if (a.Vxx0) for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) a.Vxx0[m*(N*N) + i*N + j] = Vxx[i][j];
    if (a.dV) { a.dV[2*m] = dV1; a.dV[2*m + 1] = dV2; }
    if (!a.du && !a.dx) return bad;
    T dx[N];
    for (int i = 0; i < N; i++) dx[i] = a.dx0 ? a.dx0[m*N + i] : T(0);
    for (int t = 0; t < TT; t++) {
        const size_t p = (size_t)t*M + m;
        const T* At = a.A + p*576; const T* Bt = a.B + p*144;
        T du[6], nx[N];
        if (a.dx) for (int i = 0; i < N; i++) a.dx[p*N + i] = dx[i];
        for (int i = 0; i < NU; i++) {
            T d = a.alpha*a.k[p*NU + i];
            for (int j = 0; j < N; j++) d += a.K[(p*NU + i)*N + j]*dx[j];
            if (a.u) { const T u = a.u[p*NU + i]; T v = u + d; v = v < a.u_lo ? a.u_lo : v; v = v > a.u_hi ? a.u_hi : v; d = v - u; }
            du[i] = d;
            if (a.du) a.du[p*NU + i] = d;
        }
        for (int i = 0; i < N; i++) {
            T s = T(0);
            for (int j = 0; j < N; j++) s += At[lqr_idx<N>(i)*24 + lqr_idx<N>(j)]*dx[j];
            for (int j = 0; j < NU; j++) s += Bt[lqr_idx<N>(i)*NU + j]*du[j];
            nx[i] = s;
        }
        for (int i = 0; i < N; i++) dx[i] = nx[i];
    }
    if (a.dx) for (int i = 0; i < N; i++) a.dx[((size_t)TT*M + m)*N + i] = dx[i];
    return bad;
}

// ---- the regulariser per problem (so100_query_lqr_reg, so100_query_reg_schedule) ------------------------------------------------
constexpr int LQR_REG_MAX_TRIES = 16;                        // SO100_LQR_REG_MAX_TRIES

template <typename T> struct LqrRegArgs {
    const T* reg;                                            // [M] or null: LqrArgs::reg for every problem
    T reg_min, reg_max, reg_up;
    int tries;
    T* reg_used;                                             // [M] or null
    int32_t* tries_out;                                      // [M] or null
};

// the reg a failed pass goes on with: min(reg_max, max(reg_min, r reg_up)), the product rounded once; raise(0) = reg_min
template <typename T> SO100_HD T lqr_reg_raise(T r, T reg_min, T reg_max, T reg_up) {
    T v = r*reg_up;
    v = v > reg_min ? v : reg_min;
    return v < reg_max ? v : reg_max;
}
// a reg to start from: finite and >= 0
template <typename T> SO100_HD bool lqr_reg_valid(T r) { return r >= T(0) && lqr_finite(r); }
// whether a pass that ended with `bad` under r, the `pass`-th of `tries`, is followed by another: the factor failed (not an input) and there is room
template <typename T> SO100_HD bool lqr_reg_again(int bad, int horizon, int pass, int tries, T r, T reg_max) {
    return bad >= 0 && bad < horizon && pass < tries && r < reg_max;
}
// the line search's verdict on the reg a plan was made with (Tassa's schedule: a reg under reg_min becomes 0); r not finite or negative counts as 0
template <typename T> SO100_HD T lqr_reg_next(T r, bool improved, T reg_min, T reg_max, T reg_up, T reg_down) {
    if (!lqr_reg_valid(r)) r = T(0);
    if (!improved) return lqr_reg_raise(r, reg_min, reg_max, reg_up);
    const T v = r*reg_down;
    return v < reg_min ? T(0) : v;
}

// so100_query_lqr_reg for problem m of M, the twin's form: lqr_problem under r, again under raise(r) while the factor fails and there is room.
// A pass that fails leaves NaN behind it, the next one writes every row again, so what stands in the end is the last pass's.
template <typename T, int N> inline void lqr_reg_problem(const LqrArgs<T>& a, const LqrRegArgs<T>& g, size_t M, size_t m) {
    LqrArgs<T> b = a;
    T r = g.reg ? g.reg[m] : a.reg;
    int pass = 0;
    if (!lqr_reg_valid(r)) { lqr_failed<T, N>(a, M, m, a.horizon); r = lqr_nan<T>(); }
    else
        for (;;) {
            b.reg = r;
            const int bad = lqr_problem<T, N>(b, M, m);
            pass++;
            if (!lqr_reg_again(bad, a.horizon, pass, g.tries, r, g.reg_max)) break;
            r = lqr_reg_raise(r, g.reg_min, g.reg_max, g.reg_up);
        }
    if (g.reg_used) g.reg_used[m] = r;
    if (g.tries_out) g.tries_out[m] = pass;
}

}  // namespace so100
