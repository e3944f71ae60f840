// so100_forward.hpp -- the forward-dynamics query: for a given state, the contacts that exist, the force each carries and the acceleration the
// constraint solve settles on (MuJoCo: mj_forward, MjData.contact, mj_contactForce, qfrc_constraint, qacc).  include/so100_query.h,
// so100_query_forward; DESIGN.md section 12.
//
// Templated on the scalar like so100_query.hpp: float in the kernel (so100_query_forward.hip), double and float in the host twin
// (tests/_forwardcheck).  No second copy of the model or of the solver: the stages of one contact substep (so100_physics.hpp, so100_cube.hpp,
// so100_contact.hpp) are composed exactly as substep_with_pads / physics_phase_mw compose them, up to the point where those integrate --
// this code does not -- and then the forces are read off the solution.
//
// Cold start.  The step kernels warm-start from the previous substep; a query has none: zones = -1, no "previous" list (every record
// starts with all four edges), ff = fl = 0, cube.warm = 0, arm warm start = the unconstrained acceleration M^-1 tau.  The primal problem
// is strictly convex, so the converged answer does not depend on the start.
//
// Lanes.  Store::COOP = true: a group of `nparts` adjacent lanes holds one problem (so100_contact.hpp, "Cooperative lanes"): replicated
// arithmetic, records dealt out (record s belongs to lane s mod nparts), partial sums met by quad-permute DPP.  The list entries and forces
// of a record are written by the lane that owns it: the extraction costs no pass over foreign records.  The host twin is a group of one.
#pragma once
#include "so100_contact.hpp"

namespace so100 {

constexpr int FWD_MAXCON = MAXC;             // slots of the contact list (SO100_FWD_MAXCON)

// ---- the contact store of a query: [record][field][column] like ContactsLds, NCOL columns (problems) per image, plus the one thing a
// record does not keep -- the signed distance itself (C_KD holds K imp dist).  The step kernels' stores and contact_put stay as they are:
// the overload of contact_put below is chosen for THIS store type alone (it is the more specialised template), notes the distance and
// hands the record to the shared contact_put through the base type.
template <typename T, int NCOL, bool COOP_, int NPARTS> struct ForwardRecords {
    static constexpr bool COOP = COOP_;
    static constexpr int nparts = NPARTS;
    T* base; unsigned char* pbase; int col, part;            // col: the problem's column; part of nparts: this lane's share of it
    int n = 0, dropped = 0, prev_n = 0, sig = 0;
    SO100_HD T get(int s, int f) const { return base[(s*CF + f)*NCOL + col]; }
    SO100_HD void set(int s, int f, T v) { base[(s*CF + f)*NCOL + col] = v; }
    SO100_HD int getp(int k) const { return pbase[k*NCOL + col]; }
    SO100_HD void setp(int k, int v) { pbase[k*NCOL + col] = (unsigned char)v; }
};
template <typename T, int NCOL, bool COOP_, int NPARTS> struct ForwardStore : ForwardRecords<T, NCOL, COOP_, NPARTS> {
    T* dbase;                                                  // [record][column] signed distances
    SO100_HD ForwardStore(T* records, unsigned char* codes, T* dists, int col_, int part_)
        : ForwardRecords<T, NCOL, COOP_, NPARTS>{ records, codes, col_, part_ }, dbase(dists) {}
    SO100_HD T dist(int s) const { return dbase[s*NCOL + this->col]; }
};
template <typename T, int NCOL, bool COOP_, int NPARTS>
SO100_HD void contact_put(ForwardStore<T, NCOL, COOP_, NPARTS>& cs, int s, int kind, int id, const T p[3], const T n[3], T dist, const T vrel[3]) {
    cs.dbase[s*NCOL + cs.col] = dist;
    contact_put<T>(static_cast<ForwardRecords<T, NCOL, COOP_, NPARTS>&>(cs), s, kind, id, p, n, dist, vrel);
}

// the lanes of a group exchange records through the store: detection writes a record where the serial order puts it, the solve reads
// the records its lane owns.  A group lives inside one wavefront, whose LDS operations execute in order; the barrier keeps the compiler
// from moving a load over another lane's store.  Called where every lane of the workgroup arrives.
SO100_HD void forward_group_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

// kinds as the oracle's so100o_contact numbers them: 0 cube/floor, 1 pad/floor, 2 pad/cube, 3 proxy/floor, 4 proxy/cube
SO100_HD int forward_public_kind(int kind) { return kind == 0 ? 0 : kind <= 2 ? 1 : kind <= 4 ? 2 : kind == 5 ? 3 : 4; }

template <typename T> struct ForwardResult {
    T qacc[12];                // arm 6, cube linear (world frame), cube angular (body frame): MuJoCo's dof order
    T qfrc_constraint[12];
    T pad_force[8];            // normal force summed over each finger pad's records
    T residual;                // contact_solve's or arm_pgs's; cube_solve (the cube on its own) reports none
    int ncon, dropped;
};

// force of cube/floor row (S, E) at x = qacc - qacc_smooth: the terms cube_row_accum forms as jar and D
template <int E, typename T> SO100_HD T forward_cube_edge_force(const CubeRows<T>& r, int S, const T x[6]) {
    T ja[3]; cross(r.rl[S], r.dl[E], ja);
    T jar = r.b[S][E] + edge_dot<E>(x);
    jar += ja[0]*x[3]; jar += ja[1]*x[4]; jar += ja[2]*x[5];
    return jar < T(0) ? -jar*r.arinv[S][E] : T(0);
}

// mju_decodePyramid with mu = 1: edge forces (n + t1, n - t1, n + t2, n - t2) -> (normal, t1, t2)
template <typename T> SO100_HD void forward_decode(const T f[4], T force[3]) {
    force[0] = (f[0] + f[1]) + (f[2] + f[3]); force[1] = f[0] - f[1]; force[2] = f[2] - f[3];
}

// One problem.  qpos [13], qvel [12]: so100_get_state's layout; ctrl [6]: servo targets.  emit(slot, kind, feat, pos[3], frame[9], dist,
// force[3]) is called once for every slot 0 .. FWD_MAXCON - 1 that this lane owns (slots at or beyond ncon: zeros, feat = -1).
template <typename T, class Store, class Emit>
SO100_HD void forward_dynamics(const T qpos[13], const T qvel[12], const T ctrl[6], unsigned flags, int solver_iters, int contact_iters,
                               Store& cs, ForwardResult<T>& out, Emit emit) {
    // a non-finite input: no contacts, NaN accelerations (nothing below loops without a bound; this keeps the lists empty as well)
    T chk = T(0);
#pragma unroll
    for (int i = 0; i < 13; i++) chk += qpos[i]*T(0);
#pragma unroll
    for (int i = 0; i < 12; i++) chk += qvel[i]*T(0);
#pragma unroll
    for (int i = 0; i < 6; i++) chk += ctrl[i]*T(0);
    const bool bad = !(chk == T(0));

    T q[6], v[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { q[i] = qpos[i]; v[i] = qvel[i]; }
    Cube<T> cube;
#pragma unroll
    for (int i = 0; i < 3; i++) cube.pos[i] = qpos[6 + i];
#pragma unroll
    for (int i = 0; i < 4; i++) cube.quat[i] = qpos[9 + i];
#pragma unroll
    for (int i = 0; i < 6; i++) { cube.vel[i] = qvel[6 + i]; cube.warm[i] = T(0); }
    const bool cube_live = (flags & F_CUBE_PINNED) == 0u;

    // ---- smooth dynamics: M, bias, tau, the unconstrained acceleration
    Arm<T> A;
    arm_trig(q, A);
    arm_bias<T, false>(v, A);
    arm_mass<T, false>(A);
    T Marm[21];
#pragma unroll
    for (int i = 0; i < 21; i++) Marm[i] = A.M[i];
    arm_factor(flags, A);
    T tau[6], acc[6];
    arm_tau(q, v, ctrl, A, tau);
#pragma unroll
    for (int i = 0; i < 6; i++) acc[i] = tau[i];
    ldl6_solve(A.M, A.Dinv, acc);

    // ---- detection
    WorldFK<T> W;
    world_fk(A.s, A.c, W);
    T qn[4] = { cube.quat[0], cube.quat[1], cube.quat[2], cube.quat[3] };
    quat_normalize(qn);
    T Rc[9]; quat_to_mat(qn, Rc);
    cs.n = 0; cs.dropped = 0; cs.prev_n = 0; cs.sig = 0;
    bool coupled = false;
    if (!bad && (flags & F_ANY_CONTACT) != 0u) coupled = detect_pad_contacts(W, v, cube, Rc, flags, cube_live, cs);
    forward_group_sync();

    // ---- the constraint solve, as the step kernels pick it
    const T applied[3] = { T(0), T(0), T(0) };
    T xcube[6] = { T(0), T(0), T(0), T(0), T(0), T(0) }, res = T(0);
    bool cube_own = !coupled;                                  // the cube is solved on its own (so100_cube.hpp)
    if (cs.n > 0) {
        ArmRows<T> r;
        arm_row_consts(q, v, flags, r);
        int zones = -1;
        const T cwarm[6] = { T(0), T(0), T(0), T(0), T(0), T(0) };
        res = (flags & F_ANY_LINKS) != 0u ? contact_solve<true>(tau, r, Marm, W, cs, coupled, cube.pos, cwarm, Rc, applied, contact_iters, acc, xcube, &zones)
                                          : contact_solve<false>(tau, r, Marm, W, cs, coupled, cube.pos, cwarm, Rc, applied, contact_iters, acc, xcube, &zones);
    } else if ((flags & (F_FRICTIONLOSS | F_LIMITS)) != 0u) {
        ArmRows<T> r;
        T ff[6] = { T(0), T(0), T(0), T(0), T(0), T(0) }, fl[6] = { T(0), T(0), T(0), T(0), T(0), T(0) };
        arm_rows(q, v, tau, ff, fl, flags, A, r);
        arm_pgs(ff, fl, solver_iters, A, r, acc, res);
    }
    CubePrep<T> cp;
#pragma unroll
    for (int s = 0; s < 4; s++) cp.r.act[s] = false;
    if (cube_live && cube_own) {
        T al[3], aa[3];
        cube_prepare(cube, applied, flags, cp);
        cube_solve(cube, flags, contact_iters, cp, al, aa);
#pragma unroll
        for (int i = 0; i < 3; i++) { xcube[i] = al[i]; xcube[3 + i] = aa[i]; }
    }
    const bool own_rows = cube_live && cube_own && (flags & F_FLOOR) != 0u && !bad;      // cube/floor rows outside the store: listed after its records

    // ---- accelerations and constraint forces in joint space: qfrc_constraint = M qacc - qfrc_smooth
    const T nan = chk;                                         // NaN where an input was not finite, else 0
#pragma unroll
    for (int i = 0; i < 6; i++) {
        T t = T(0);
#pragma unroll
        for (int j = 0; j < 6; j++) t += sym6(Marm, i, j)*acc[j];
        out.qacc[i] = acc[i] + nan; out.qfrc_constraint[i] = (t - tau[i]) + nan;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const T a0 = i == 2 ? -T(so100g::GRAVITY) : T(0);
        out.qacc[6 + i] = cube_live ? xcube[i] + nan : T(0); out.qacc[9 + i] = cube_live ? xcube[3 + i] + nan : T(0);
        out.qfrc_constraint[6 + i] = cube_live ? T(so100g::CUBE_MASS)*(xcube[i] - a0) + nan : T(0);
        out.qfrc_constraint[9 + i] = cube_live ? T(so100g::CUBE_INERTIA)*xcube[3 + i] + nan : T(0);
    }
    out.residual = res + nan;
    out.dropped = cs.dropped;

    // ---- the list: the store's records (this lane's), then the cube's own floor rows, then empty slots
    T pf[8] = { T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0) };
#pragma unroll 1
    for (int s = cs.part; s < cs.n; s += cs.nparts) {
        const T p[3] = { cs.get(s, C_PX), cs.get(s, C_PY), cs.get(s, C_PZ) };
        const T n[3] = { cs.get(s, C_NX), cs.get(s, C_NY), cs.get(s, C_NZ) };
        const T kd = cs.get(s, C_KD), D = cs.get(s, C_RINV);
        const int code = (int)cs.get(s, C_KIND), kind = code & 7, id = (code >> 3) & 255;
        T t1[3], t2[3];
        contact_frame(n, t1, t2);
        // J x - aref of the four edge rows: the record's velocity term, the arm point's acceleration (geom1 in arm/cube pairs, geom2 against
        // the floor) and the cube point's (geom2, or the cube itself on the floor) -- PrimalProblem::eval's jar
        T w[3] = { cs.get(s, C_VX), cs.get(s, C_VY), cs.get(s, C_VZ) };
        const T sgn = contact_on_cube(kind) ? T(-1) : T(1);
        if (kind != 0) {
            const int link = contact_link(kind, id);
#pragma unroll
            for (int i = 0; i < 6; i++) {
                T col[3]; cross(W.z[i], p, col);
                const T xi = i <= link ? sgn*acc[i] : T(0);
#pragma unroll
                for (int k = 0; k < 3; k++) w[k] += xi*(col[k] + W.oz[i][k]);
            }
        }
        if (kind == 0 || contact_on_cube(kind)) { T ac[3]; cube_point_motion(Rc, cube.pos, xcube, p, ac); w[0] += ac[0]; w[1] += ac[1]; w[2] += ac[2]; }
        const T jn = dot(n, w) + kd, j1 = dot(t1, w), j2 = dot(t2, w);
        const T jar[4] = { jn + j1, jn - j1, jn + j2, jn - j2 };
        T f[4], force[3];
#pragma unroll
        for (int e = 0; e < 4; e++) f[e] = jar[e] < T(0) ? -jar[e]*D : T(0);
        forward_decode(f, force);
        if (kind >= 1 && kind <= 4) {
            const int g = (id & 63) >> 3;
#pragma unroll
            for (int k = 0; k < 8; k++) pf[k] += k == g ? force[0] : T(0);
        }
        const T frame[9] = { n[0], n[1], n[2], t1[0], t1[1], t1[2], t2[0], t2[1], t2[2] };
        emit(s, forward_public_kind(kind), id, p, frame, cs.dist(s), force);
    }
    int ncon = cs.n;
    if (own_rows) {
        const T hc[3] = { T(so100g::CUBE_HALF), T(so100g::CUBE_HALF), T(so100g::CUBE_HALF) };
        unsigned mask = plane_box_mask<T>(cube.pos, Rc, hc);       // which corners: the rows' slots are the hits in corner order
        const CubeRows<T>& r = cp.r;
#pragma unroll
        for (int S = 0; S < 4; S++) {
            if (!r.act[S]) continue;
            const int corner = mask != 0u ? __builtin_ctz(mask) : 0;
            mask &= mask - 1u;
            const int slot = cs.n + S;
            ncon = slot + 1;
            if (slot % cs.nparts != cs.part) continue;
            const T hs = T(so100g::CUBE_HALF);
            const T sx = (corner & 1) ? hs : -hs, sy = (corner & 2) ? hs : -hs, sz = (corner & 4) ? hs : -hs;
            const T dist = cube.pos[2] + (Rc[6]*sx + Rc[7]*sy + Rc[8]*sz);            // (cube_prepare's own expression)
            const T p[3] = { cube.pos[0] + Rc[0]*r.rl[S][0] + Rc[1]*r.rl[S][1] + Rc[2]*r.rl[S][2],
                             cube.pos[1] + Rc[3]*r.rl[S][0] + Rc[4]*r.rl[S][1] + Rc[5]*r.rl[S][2],
                             cube.pos[2] + Rc[6]*r.rl[S][0] + Rc[7]*r.rl[S][1] + Rc[8]*r.rl[S][2] };
            const T f[4] = { forward_cube_edge_force<0>(r, S, cube.warm), forward_cube_edge_force<1>(r, S, cube.warm),
                             forward_cube_edge_force<2>(r, S, cube.warm), forward_cube_edge_force<3>(r, S, cube.warm) };
            T force[3];
            forward_decode(f, force);
            const T frame[9] = { T(0), T(0), T(1), T(0), T(1), T(0), T(-1), T(0), T(0) };      // mju_makeFrame of +z (EdgeDir)
            emit(slot, 0, 128 + corner, p, frame, dist, force);
        }
    }
    out.ncon = ncon;
#pragma unroll
    for (int k = 0; k < 8; k++) out.pad_force[k] = coop_sum(cs, pf[k]) + nan;
    const T zero3[3] = { T(0), T(0), T(0) }, zero9[9] = { T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0) };
#pragma unroll 1
    for (int s = cs.part; s < FWD_MAXCON; s += cs.nparts)
        if (s >= ncon) emit(s, 0, -1, zero3, zero9, T(0), zero3);
}

}  // namespace so100
