// so100_cost.hpp -- the cost family of include/so100_query.h (so100_cost_def): what the cost-terms query and the cost-select query compute per
// state row, written once.  Per row (q, the arm's v, the target g):
//     r = point(q) - g
//     s = w_point (r0^2 + r1^2 + r2^2) + sum_j w_q[j] (q_j - q_nom_j)^2 + sum_j w_v[j] v_j^2               summed in that order, j ascending
// and the Gauss-Newton model of sigma s in the derivatives query's tangent (the point's second derivative is dropped):
//     lx[0..5]   = 2 sigma (w_point J'r + w_q o (q - q_nom))          lxx[0..5][0..5] = 2 sigma (w_point J'J + diag w_q)
//     lx[12..17] = 2 sigma w_v o v                                    lxx diagonal 12..17 = 2 sigma w_v
//     cube target, the cube's linear tangent 6..8 (dr/dx = -I):
//     lx[6..8]   = -2 sigma w_point r                                 lxx[0..5][6..8] = -2 sigma w_point J', lxx[6..8][6..8] = 2 sigma w_point I
// Nothing here restates the model: the point and its Jacobian are link_frames / link_point / point_jacobian of so100_query.hpp.
//
// The pieces.  cost_row() runs the chain of one state row and leaves a CostRow: J, r and the two weighted differences -- the numbers every entry of the
// row's lx and lxx is made of.  cost_lx() / cost_lxx() make ONE entry from a CostRow, addressed by its tangent index, so the kernel can hand the
// entries of a problem-major block to whichever lane stores them and the host twin can loop over them; lxx is symmetric to the bit because entry
// (i, j) is made from (min, max).  cost_state() is s alone (no Jacobian: what the select query sums), cost_control() the control term.
//
// Templated on the scalar T: float on the device; float / double host instantiations exist ONLY for the CPU-side tests in tests/_costcheck.
#pragma once
#include "so100_query.hpp"

namespace so100 {

constexpr int COST_TARGET_FIXED = 0, COST_TARGET_TRAJ = 1, COST_TARGET_CUBE = 2;
constexpr int COST_NU = 6;

template <typename T> struct CostDef {
    int link, target_mode;
    T o[3], w_point, w_q[6], q_nom[6], w_v[6], w_u[6], w_terminal;
};

// the tangent index (of the 24) of entry i of the n-form: n = 12 is the arm block, 0..5 and 12..17 (so100_lqr.hpp: lqr_idx)
SO100_HD constexpr int cost_idx(int n, int i) { return n == 24 ? i : (i < 6 ? i : i + 6); }
template <typename T> SO100_HD bool cost_finite(T x) { return x*T(0) == T(0); }

// what the entries of one state row's lx and lxx are made of; ok: every value the row's cost reads is finite
template <typename T> struct CostRow { T J[18], r[3], gq[6], gv[6]; bool ok; };

// r = point(q) - g and the frames it came from
template <typename T> SO100_HD void cost_residual(const CostDef<T>& c, const T q[6], const T g[3], LinkFrames<T>& F, T p[3], T r[3]) {
    Arm<T> A;
    arm_trig(q, A);
    link_frames(A.s, A.c, F);
    link_point(F, c.link, c.o, p);
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = p[i] - g[i];
}

template <typename T> SO100_HD bool cost_inputs_finite(const T q[6], const T v[6], const T g[3]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) ok = ok && cost_finite(q[j]) && cost_finite(v[j]);
#pragma unroll
    for (int i = 0; i < 3; i++) ok = ok && cost_finite(g[i]);
    return ok;
}

// s of one state row from its residual
template <typename T> SO100_HD T cost_sum(const CostDef<T>& c, const T q[6], const T v[6], const T r[3]) {
    T s = c.w_point*(r[0]*r[0] + r[1]*r[1] + r[2]*r[2]);
#pragma unroll
    for (int j = 0; j < 6; j++) { const T d = q[j] - c.q_nom[j]; s += c.w_q[j]*(d*d); }
#pragma unroll
    for (int j = 0; j < 6; j++) s += c.w_v[j]*(v[j]*v[j]);
    return s;
}

template <typename T> SO100_HD T cost_state(const CostDef<T>& c, const T q[6], const T v[6], const T g[3]) {
    LinkFrames<T> F;
    T p[3], r[3];
    cost_residual(c, q, g, F, p, r);
    return cost_sum(c, q, v, r);
}

template <typename T> SO100_HD T cost_control(const CostDef<T>& c, const T u[6]) {
    T s = T(0);
#pragma unroll
    for (int j = 0; j < 6; j++) s += c.w_u[j]*(u[j]*u[j]);
    return s;
}

template <typename T> SO100_HD void cost_row(const CostDef<T>& c, const T q[6], const T v[6], const T g[3], CostRow<T>& R) {
    LinkFrames<T> F;
    T p[3], jr[18];
    cost_residual(c, q, g, F, p, R.r);
    point_jacobian(F, c.link, p, R.J, jr);
#pragma unroll
    for (int j = 0; j < 6; j++) { R.gq[j] = c.w_q[j]*(q[j] - c.q_nom[j]); R.gv[j] = c.w_v[j]*v[j]; }
    R.ok = cost_inputs_finite(q, v, g);
}

// One entry of lx / lxx of the row, by TANGENT index (0..23); two_sigma = 2 sigma.  `row` gives the CostRow's numbers: row.J(a, k) = jacp[a][k],
// row.r(a), row.gq(k), row.gv(k) -- an accessor, so that the kernel reads them from LDS and the twin from the struct.
template <typename T, typename Row> SO100_HD T cost_lx(const CostDef<T>& c, const Row& row, T two_sigma, int i) {
    if (i < 6) return two_sigma*(c.w_point*(row.J(0, i)*row.r(0) + row.J(1, i)*row.r(1) + row.J(2, i)*row.r(2)) + row.gq(i));
    if (i < 9) return c.target_mode == COST_TARGET_CUBE ? -(two_sigma*(c.w_point*row.r(i - 6))) : T(0);
    if (i >= 12 && i < 18) return two_sigma*row.gv(i - 12);
    return T(0);
}
// w_q / w_v of joint k, selected (the arrays are launch arguments: an index would send them to scratch memory)
template <typename T> SO100_HD T cost_pick6(const T w[6], int k) {
    T x = w[0];
#pragma unroll
    for (int j = 1; j < 6; j++) x = k == j ? w[j] : x;
    return x;
}
template <typename T, typename Row> SO100_HD T cost_lxx(const CostDef<T>& c, const Row& row, T two_sigma, int i0, int j0) {
    const int i = i0 < j0 ? i0 : j0, j = i0 < j0 ? j0 : i0;
    if (j < 6) {
        const T jj = row.J(0, i)*row.J(0, j) + row.J(1, i)*row.J(1, j) + row.J(2, i)*row.J(2, j);
        return two_sigma*(c.w_point*jj + (i == j ? cost_pick6(c.w_q, i) : T(0)));
    }
    if (j < 9) {
        if (c.target_mode != COST_TARGET_CUBE) return T(0);
        if (i < 6) return -(two_sigma*(c.w_point*row.J(j - 6, i)));
        return i == j ? two_sigma*c.w_point : T(0);
    }
    if (i == j && j >= 12 && j < 18) return two_sigma*cost_pick6(c.w_v, j - 12);
    return T(0);
}

// the control's terms of step t: lu = 2 w_u o u, luu = diag(2 w_u)
template <typename T> SO100_HD T cost_lu(const CostDef<T>& c, const T u[6], int j) { return (T(2)*c.w_u[j])*u[j]; }
template <typename T> SO100_HD T cost_luu(const CostDef<T>& c, int i, int j) { return i == j ? T(2)*cost_pick6(c.w_u, i) : T(0); }

// the accessor over a CostRow in registers or host memory
template <typename T> struct CostRowRef {
    const CostRow<T>& R;
    SO100_HD T J(int a, int k) const { return R.J[6*a + k]; }
    SO100_HD T r(int a) const { return R.r[a]; }
    SO100_HD T gq(int k) const { return R.gq[k]; }
    SO100_HD T gv(int k) const { return R.gv[k]; }
};

// sigma of the state after step t of a horizon of `steps`
template <typename T> SO100_HD T cost_sigma(const CostDef<T>& c, int t, int steps) { return t == steps - 1 ? c.w_terminal : T(1); }

// the select query's total of one rollout: J = sum_t (c_t + sigma_t s_t), t ascending; src(t, q, v, u, g) loads step t's row
template <typename T, typename Src> SO100_HD T cost_total(const CostDef<T>& c, int steps, Src&& src) {
    T total = T(0);
    for (int t = 0; t < steps; t++) {
        T q[6], v[6], u[6], g[3];
        src(t, q, v, u, g);
        total += cost_control(c, u) + cost_sigma(c, t, steps)*cost_state(c, q, v, g);
    }
    return total;
}

// the line search's choice among L costs (+inf: not a candidate): the smallest, ties to the lowest index, -1 if none is below +inf
template <typename T, typename Get> SO100_HD int cost_argmin(int L, T inf, Get&& get, T& best_cost) {
    int best = -1;
    best_cost = inf;
    for (int a = 0; a < L; a++) { const T x = get(a); if (x < best_cost) { best_cost = x; best = a; } }
    return best;
}

}  // namespace so100
