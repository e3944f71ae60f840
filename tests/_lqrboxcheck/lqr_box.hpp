// lqr_box.hpp -- the control-limited (box-DDP) backward pass for the LQR query, test-side: the algorithm a kernel is to implement, written on
// so100_lqr.hpp's pieces (lqr_chol6, lqr_solve6, LqrArgs) and instantiated on the host by lqrboxcheck.cpp.  Nothing of the product includes this
// file.
#pragma once
#include "../../so100_mujoco_rl_amd/csrc/so100_lqr.hpp"

namespace so100 {

// ---- the control-limited step (box-DDP; Tassa, Mansard and Todorov 2014: boxQP) -----------------------------------------------------------------------
// The backward pass of so100_lqr.hpp knows nothing of the bounds the forward pass clamps to, so the gains of a saturated control are wrong.  Here every step
// solves  k = argmin x'Hx/2 + g'x over lo <= x <= hi  with H = Quu + reg I, g = Qu, lo_j = u_lo - u_tj, hi_j = u_hi - u_tj (each difference
// rounded once); K has zero rows for the controls clamped at k and K_f = -H_ff^-1 Qux_f on the free ones; the value update, dV1, dV2, the
// symmetrisation and the forward pass are so100_lqr.hpp's formulas, on these k and K.
// A set of clamped controls is one word: bit j: control j at its lower bound, bit 8 + j: at its upper bound (the layout of the clamped output).
constexpr int LQR_BOX_MAX_ITERS = 64;                        // projected-Newton iterations per step: 1..64
constexpr int LQR_BOX_SEARCH = 20;                           // step sizes 1, 0.6, 0.6^2, ... of the projected search
constexpr int32_t LQR_BOX_RAN_OUT = 1 << 16;                 // bit 16 of qp_used

// what the box step has beyond LqrArgs: the iterations allowed per step; clamped [T][M] the set at k_t; used [T][M] the iterations taken, with
// bit 16 where they ran out (both nullable, both 0 for every step of a failed problem)
struct LqrBoxArgs {
    int iters;
    int32_t *clamped, *used;
};

SO100_HD bool lqr_box_free(int32_t set, int j) { return ((set >> j) & 0x101) == 0; }

// H(i, j) of the box solve: the symmetric matrix whose lower triangle is that of Quu + reg I -- the triangle lqr_chol6 reads
template <typename T> SO100_HD T lqr_box_h(const T Q[6][6], T reg, int i, int j) { return i == j ? Q[i][i] + reg : (i > j ? Q[i][j] : Q[j][i]); }

// F H F + (I - F) = L L', F the indicator of the free controls of `set`: H's rows and columns of the clamped controls replaced by the identity's.
// The same lqr_chol6 on a masked copy, whatever the set: every caller runs the same instructions.  An empty set gives lqr_chol6(Q, reg)'s bits.
template <typename T> SO100_HD bool lqr_box_chol6(const T Q[6][6], T reg, int32_t set, T L[6][6], T inv[6]) {
    T Hm[6][6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const bool fi = lqr_box_free(set, i);
        Hm[i][i] = fi ? Q[i][i] + reg : T(1);
#pragma unroll
        for (int j = 0; j < i; j++) Hm[i][j] = (fi && lqr_box_free(set, j)) ? Q[i][j] : T(0);
    }
    return lqr_chol6(Hm, T(0), L, inv);
}

// x_f = -H_ff^-1 b_f on the free controls of `set` from its masked factor, exactly 0 on the clamped ones
template <typename T> SO100_HD void lqr_box_solve6(const T L[6][6], const T inv[6], int32_t set, const T b[6], T x[6]) {
    T bm[6];
#pragma unroll
    for (int j = 0; j < 6; j++) bm[j] = lqr_box_free(set, j) ? b[j] : T(0);
    lqr_solve6(L, inv, bm, x);
#pragma unroll
    for (int j = 0; j < 6; j++) x[j] = lqr_box_free(set, j) ? x[j] : T(0);
}

// grad = g + H x and the clamped set at x: j where (x_j == lo_j and grad_j > 0) or (x_j == hi_j and grad_j < 0).  A component of x that is zero adds
// nothing, not even +0 to a gradient of -0: from x = 0 the gradient is g to the bit.
template <typename T> SO100_HD int32_t lqr_box_grad6(const T Q[6][6], T reg, const T g[6], const T lo[6], const T hi[6], const T x[6], T grad[6]) {
    int32_t set = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        T s = g[i];
#pragma unroll
        for (int j = 0; j < 6; j++) s = x[j] == T(0) ? s : s + lqr_box_h(Q, reg, i, j)*x[j];
        grad[i] = s;
        if (x[i] == lo[i] && s > T(0)) set |= 1 << i;
        if (x[i] == hi[i] && s < T(0)) set |= 1 << (8 + i);
    }
    return set;
}

// x = argmin x'Hx/2 + g'x over lo <= x <= hi (lo <= hi), H = Quu + reg I, by this projected Newton iteration, which is the contract (every
// implementation is to give the same active sets): x = clamp(0, lo, hi) -- a u_t outside its bounds makes lo > 0 or hi < 0, and the start is
// then the bound nearest to it; then per iteration the gradient and the clamped set at x, the masked
// factor, the Newton direction on the free controls, and a projected search over s = 1, 0.6, 0.6^2, ... (at most LQR_BOX_SEARCH of them) that
// takes clamp(x + s d) once its true decrease is at least 0.1 of -grad'(clamp(x + s d) - x).  It ends -- with no tolerance -- when the set found
// at x equals the one the last step was taken on and that step had s = 1 and clipped nothing; or after `iters` steps, or where the search takes no
// step: bit 16 of `used` then.  L, inv: the masked factor of `set`, the set at the final x -- what the gains are solved against.  false: a factor
// failed (x, set and used are then not to be used).  Two things a caller must know beyond the issue's list.  (1) The search can take none of its
// steps (a direction that is no descent direction to working precision): the iteration then ends there, bit 16 set, like iterations running out.
// (2) Only the MASKED matrix is factored, so a Quu + reg I that is not positive definite fails the problem only if its free block is not: with a
// u_t outside its bounds the first set can be non-empty, and a bad pivot on a clamped control is never seen.  With u_t inside, the first set is
// empty and the whole matrix is factored first, as in so100_query_lqr.
template <typename T> SO100_HD bool lqr_boxqp6(const T Q[6][6], T reg, const T g[6], const T lo[6], const T hi[6], int iters,
                                               T x[6], T L[6][6], T inv[6], int32_t& set, int32_t& used) {
    T grad[6];
#pragma unroll
    for (int j = 0; j < 6; j++) { T v = T(0); v = v < lo[j] ? lo[j] : v; v = v > hi[j] ? hi[j] : v; x[j] = v; }
    int32_t taken_on = 0;
    int n = 0;
    bool full = false, done = false, stalled = false, ok = true;
#pragma unroll 1
    for (;;) {
        set = lqr_box_grad6(Q, reg, g, lo, hi, x, grad);
        if (full && set == taken_on) { done = true; break; }  // the factor in hand is this set's
        if (n == iters || stalled) break;
        ok = lqr_box_chol6(Q, reg, set, L, inv);
        if (!ok) break;
        T d[6], xn[6];
        lqr_box_solve6(L, inv, set, grad, d);
        T s = T(1);
        bool taken = false, clipped = false;
#pragma unroll 1
        for (int ls = 0; ls < LQR_BOX_SEARCH && !taken; ls++) {
            T p[6];
            clipped = false;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const T v = x[j] == T(0) ? s*d[j] : x[j] + s*d[j];      // from 0 the step itself, its zeros with their signs
                T w = v < lo[j] ? lo[j] : v; w = w > hi[j] ? hi[j] : w;
                clipped = clipped || !(w == v);
                xn[j] = w; p[j] = w - x[j];
            }
            T gp = T(0), php = T(0);
#pragma unroll
            for (int i = 0; i < 6; i++) {
                T hp = T(0);
#pragma unroll
                for (int j = 0; j < 6; j++) hp += lqr_box_h(Q, reg, i, j)*p[j];
                gp += grad[i]*p[i]; php += p[i]*hp;
            }
            taken = -(gp + T(0.5)*php) >= T(0.1)*-gp;
            full = taken && ls == 0 && !clipped;
            if (!taken) s *= T(0.6);
        }
        stalled = !taken;
        if (taken) {
#pragma unroll
            for (int j = 0; j < 6; j++) x[j] = xn[j];
        }
        taken_on = set;
        n++;
    }
    if (ok && !done) ok = lqr_box_chol6(Q, reg, set, L, inv);  // the steps ran out: the factor of the set the final x has
    used = n | (done ? 0 : LQR_BOX_RAN_OUT);
    return ok;
}

// The whole control-limited pass for problem m of M, element by element: so100_lqr.hpp's lqr_problem with the box step in place of the
// unconstrained one -- its text otherwise, line for line, so that bounds that never bind give its bits; a.u is required.  (A copy, because the
// product header is to stay as it is until a kernel uses this; it goes when the step moves there.)
template <typename T, int N> inline void lqr_box_problem(const LqrArgs<T>& a, size_t M, size_t m, const LqrBoxArgs* box) {
    constexpr int NU = LQR_NU, NP = N + NU;
    const int TT = a.horizon;
    const T nan = lqr_nan<T>();
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
        int32_t set = 0, used = 0;
        if (box) {                                           // lo and hi: the room u_t leaves, each difference rounded once
            T lo[6], hi[6];
            for (int i = 0; i < NU; i++) { lo[i] = a.u_lo - a.u[p*NU + i]; hi[i] = a.u_hi - a.u[p*NU + i]; }
            if (!lqr_boxqp6(Quu, a.reg, Qu, lo, hi, box->iters, kk, L, inv, set, used)) { bad = t; break; }
        } else {
            if (!lqr_chol6(Quu, a.reg, L, inv)) { bad = t; break; }
            lqr_solve6(L, inv, Qu, kk);
        }
        for (int i = 0; i < NU; i++) { T s = T(0); for (int j = 0; j < NU; j++) s += Quu[i][j]*kk[j]; Qk[i] = s; }
        { T s1 = T(0), s2 = T(0); for (int i = 0; i < NU; i++) { s1 += kk[i]*Qu[i]; s2 += kk[i]*Qk[i]; } dV1 += s1; dV2 += T(0.5)*s2; }
        T K[6][N], QK[6][N];
        for (int j = 0; j < N; j++) {
            T b[6], x[6];
            for (int i = 0; i < NU; i++) b[i] = H[N + i][j];
            if (box) lqr_box_solve6(L, inv, set, b, x); else lqr_solve6(L, inv, b, x);
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
        if (box && box->clamped) box->clamped[p] = set;
        if (box && box->used) box->used[p] = used;
    }
    if (a.bad) a.bad[m] = bad;
    if (bad >= 0) {                                          // every float output of a failed problem is NaN, its clamped and qp_used are 0
        for (int t = 0; t <= TT; t++) {
            const size_t p = (size_t)t*M + m;
            if (a.dx) for (int i = 0; i < N; i++) a.dx[p*N + i] = nan;
            if (t == TT) break;
            if (box && box->clamped) box->clamped[p] = 0;
            if (box && box->used) box->used[p] = 0;
            if (a.k) for (int i = 0; i < NU; i++) a.k[p*NU + i] = nan;
            if (a.K) for (int i = 0; i < NU*N; i++) a.K[p*NU*N + i] = nan;
            if (a.du) for (int i = 0; i < NU; i++) a.du[p*NU + i] = nan;
        }
        if (a.Vx0) for (int i = 0; i < N; i++) a.Vx0[m*N + i] = nan;
        if (a.Vxx0) for (int i = 0; i < N*N; i++) a.Vxx0[m*(N*N) + i] = nan;
        if (a.dV) a.dV[2*m] = a.dV[2*m + 1] = nan;
        return;
    }
    if (a.Vx0) for (int i = 0; i < N; i++) a.Vx0[m*N + i] = Vx[i];
    if (a.Vxx0) for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) a.Vxx0[m*(N*N) + i*N + j] = Vxx[i][j];
    if (a.dV) { a.dV[2*m] = dV1; a.dV[2*m + 1] = dV2; }
    if (!a.du && !a.dx) return;
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
}

}  // namespace so100
