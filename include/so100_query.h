/* so100_query.h -- model queries of libso100sim.so: what MuJoCo's users read from MjData or get from mj_jac, mj_fullM,
 * mj_inverse and mj_forward, for M independent problems at once, one GPU lane per problem (the forward query: four), and where M states
 * end up under M open-loop control sequences (the trajectory query), and the finite-difference linearisation of such a control step, one GPU
 * wave per problem (the derivatives query), the Riccati pass on such linearisations (the LQR query) and the rollouts under the feedback law it
 * gives, one GPU lane per rollout (the closed-loop query), and the cost of such plans: its quadratic model in the LQR query's input layout (the
 * cost-terms query) and the line search's choice among the closed-loop query's candidates (the cost-select query), and the two ends of a sampling
 * planner's step round the trajectory query: the candidate plans in its input layout (the plan-sample query) and their cost-weighted blend (the
 * cost-blend query).
 *
 * Additive to so100_sim.h (SO100_ABI_VERSION is unchanged) and under its conventions: extern "C"; `*_dev` pointers are DEVICE
 * pointers owned by the caller; 0 on success, a negative SO100_E_* code otherwise with the message in so100_last_error(); all
 * work goes to the caller's `hip_stream`; nothing allocates, frees or synchronises (hipGraph-capturable); a rejected call
 * enqueues nothing.  Every call only READS the handle's state matrix.
 *
 * Layout: every array is component-major (SoA) like so100_get_state: a quantity with k components is [k][M] floats, matrices
 * row-major in the leading index (xmat [6][9][M]: link, then the 9 row-major entries).  Links are numbered 0..5 as in
 * csrc/so100_model_def.h: link k is MuJoCo body k + 2 and hangs on hinge joint k.
 *
 * State defaults: q_dev == NULL reads rows q0..q5 of the handle's state matrix, and M must then be the handle's N.
 *
 * Argument errors (SO100_E_INVALID), in this order: a null handle or io; M < 1 (or M != N where the handle's state is read);
 * link outside 0..5; iters outside 1..1024; damping, tol or max_step not positive; a required pointer that is NULL; a call
 * that asks for no output.
 *
 * Reference files are cited as "ref:", as in so100_sim.h.
 */
#ifndef SO100_QUERY_H
#define SO100_QUERY_H
#include "so100_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the reference's end-effector point (ref: envs/env_base_01.py:118-127): on Fixed_Jaw, 10 cm along its -y axis */
#define SO100_EE_LINK 4
#define SO100_EE_OFFSET_Y (-0.1f)

/* Forward kinematics from q [6][M].  ref: the reads of data.body(...).xpos / .xmat, get_end_effector_pos and
 * data.camera(...).xpos / .xmat in the task code.  Every output is nullable; at least one is required. */
typedef struct {
    const float* q_dev;            /* [6][M] joint angles, or NULL (the handle's)                               */
    float*       xpos_dev;         /* [6][3][M] world position of each link frame (MjData.xpos[k + 2])          */
    float*       xmat_dev;         /* [6][9][M] world orientation of each link frame (MjData.xmat[k + 2])       */
    float*       ee_dev;           /* [3][M] xpos_FixedJaw + xmat_FixedJaw (0, -0.1, 0)                         */
    float*       cam_pos_dev;      /* [3][M] the wrist camera (MjData.cam_xpos)                                 */
    float*       cam_mat_dev;      /* [9][M] (MjData.cam_xmat)                                                  */
} so100_kinematics_io;

int so100_query_kinematics(so100_sim* sim, const so100_kinematics_io* io, int32_t M, void* hip_stream);

/* Jacobian of a point fixed to link `link` at `offset` in that link's frame, in the world frame and in mj_jac's convention:
 * column k is axis_k x (p - anchor_k) in jacp and axis_k in jacr for k <= link, zero for k > link.  link and offset are the
 * same for every problem of the call.  At least one output is required. */
typedef struct {
    const float* q_dev;            /* [6][M] or NULL (the handle's)                                             */
    int32_t      link;             /* 0..5                                                                      */
    const float* offset;           /* HOST pointer to 3 floats, or NULL: the link's default point -- the end-effector point
                                      (0, -0.1, 0) on link 4, the frame origin on every other link                */
    float*       jacp_dev;         /* [3][6][M] or NULL                                                         */
    float*       jacr_dev;         /* [3][6][M] or NULL                                                         */
} so100_jacobian_io;

int so100_query_jacobian(so100_sim* sim, const so100_jacobian_io* io, int32_t M, void* hip_stream);

/* Joint-space dynamics of the arm: M(q) as MuJoCo leaves it in qM (armature on the diagonal), bias = C(q, v) + g(q)
 * (MjData.qfrc_bias) and the inverse dynamics tau = M qacc + bias (mj_inverse without constraint or passive forces).
 * tau is written only when qacc_dev is given; at least one output (M, bias, or tau with qacc) is required. */
typedef struct {
    const float* q_dev;            /* [6][M] or NULL (the handle's)                                             */
    const float* v_dev;            /* [6][M] joint velocities, or NULL: zero -- or, with q_dev NULL too, the handle's */
    const float* qacc_dev;         /* [6][M] or NULL                                                            */
    float*       M_dev;            /* [36][M] full symmetric 6 x 6, row-major, or NULL                          */
    float*       bias_dev;         /* [6][M] or NULL                                                            */
    float*       tau_dev;          /* [6][M] or NULL                                                            */
} so100_dynamics_io;

int so100_query_dynamics(so100_sim* sim, const so100_dynamics_io* io, int32_t M, void* hip_stream);

/* Batched inverse kinematics: moves the point (link, offset: as in so100_jacobian_io) to target by damped least squares over
 * the joints 0..link; the joints behind the link keep q0's value.  Per problem:
 *     q = clamp(q0, joint range) on the joints 0..link
 *     for it = 0 .. iters:
 *         e = target - point(q);  r = |e|;   stop if r <= tol or it == iters
 *         J = jacp columns 0..link;   solve (J J' + damping^2 I) y = e;   dq = J' y
 *         s = min(1, max_step / max_i |dq_i|);   q = clamp(q + s dq, joint range)
 * Each lane stops when its own problem is done; the result is the same bits on every run.  q_dev may alias q0_dev.  target_dev
 * is required, every output is nullable, at least one output is required. */
#define SO100_IK_ITERS    64
#define SO100_IK_DAMPING  0.02f
#define SO100_IK_TOL      1e-4f    /* metres */
#define SO100_IK_MAX_STEP 0.3f     /* radians per iteration, largest joint */
typedef struct {
    const float* target_dev;       /* [3][M] world position                                                     */
    const float* q0_dev;           /* [6][M] start, or NULL (the handle's current joints)                       */
    int32_t      link;             /* 0..5                                                                      */
    const float* offset;           /* HOST pointer to 3 floats or NULL (so100_jacobian_io)                      */
    int32_t      iters;            /* 1..1024                                                                   */
    float        damping;          /* > 0                                                                       */
    float        tol;              /* > 0                                                                       */
    float        max_step;         /* > 0                                                                       */
    float*       q_dev;            /* [6][M] or NULL                                                            */
    float*       residual_dev;     /* [M] |target - point(q)| of the returned q, or NULL                        */
    int32_t*     iterations_dev;   /* [M] updates taken (0..iters), or NULL                                     */
    uint8_t*     converged_dev;    /* [M] residual <= tol, or NULL                                              */
} so100_ik_io;

int so100_query_ik(so100_sim* sim, const so100_ik_io* io, int32_t M, void* hip_stream);

/* Forward dynamics with constraints, without integrating: for each of M states the contacts that exist, the force each carries and the
 * acceleration the constraint solve settles on -- mj_forward, MjData.contact, mj_contactForce, qfrc_constraint and qacc.  The stages are
 * the ones a contact substep of so100_step runs (csrc/so100_forward.hpp), cold-started: no previous substep's forces or active set.
 *
 * State: qpos [13][M] and qvel [12][M] in so100_get_state's layout (arm 6, cube position 3, cube quaternion 4 / arm 6, cube linear 3 in
 * the world frame, cube angular 3 in the body frame).  Both NULL: the handle's rows, and M must be N.  qvel alone NULL: zero.
 * ctrl NULL: ctrl = q, the servo holds the pose (Env01's ctrl under a zero action).  No force is applied to the cube.
 * flags: SO100_F_*, decided per call (the handle's own flags are not consulted).
 *
 * The contact list has SO100_FWD_MAXCON slots per problem; slots at or beyond ncon are zeros with feat = -1.  It holds every contact of
 * the solve, the cube's own floor contacts included.  kind and feat are numbered as the oracle's so100o_contact: kind 0 cube/floor,
 * 1 pad/floor, 2 pad/cube, 3 link proxy/floor, 4 link proxy/cube; feat 8 pad + corner, 64 + 8 pad + manifold slot, 128 + corner,
 * 144 + 2 proxy + capsule end, 160 + proxy.  The order is the detection order: deterministic, otherwise not part of the contract -- match
 * by feat, which is unique within a problem.  frame rows: normal (geom1 -> geom2), t1, t2 (mju_makeFrame); force = mj_contactForce's first
 * three numbers, in that frame; dist < 0 in penetration.
 *
 * Argument errors, in this order: a null handle or io; M < 1 (or M != N where the state is read); qvel_dev without qpos_dev; flag bits
 * outside SO100_F_*; SO100_F_PADS_CUBE or SO100_F_LINKS_CUBE with SO100_F_CUBE_PINNED; an iteration count outside 1..64; no output.
 * residual is that of contact_solve or, without arm contact, of the block PGS; the cube's own floor solve (so100_cube.hpp, run when the
 * cube is not coupled to the arm) reports none, so residual = 0 says nothing about it -- it is bounded by contact_iters like the rest.
 * A non-finite input gives that problem ncon = 0 and NaN accelerations.  Every output is nullable; at least one is required. */
#define SO100_FWD_MAXCON        20
#define SO100_FWD_SOLVER_ITERS  64     /* block-PGS sweeps of a contact-free arm */
#define SO100_FWD_CONTACT_ITERS 64     /* Newton iterations (arm with contacts, cube on the floor) */
typedef struct {
    const float* qpos_dev;             /* [13][M] or NULL (with qvel_dev NULL: the handle's state)                 */
    const float* qvel_dev;             /* [12][M] or NULL                                                           */
    const float* ctrl_dev;             /* [6][M] servo targets (radians), or NULL: the joint angles                 */
    uint32_t     flags;                /* SO100_F_*                                                                 */
    int32_t      solver_iters;         /* 1..64                                                                     */
    int32_t      contact_iters;        /* 1..64                                                                     */
    float*       qacc_dev;             /* [12][M] arm 6, cube linear (world), cube angular (body): MuJoCo's dofs    */
    float*       qfrc_constraint_dev;  /* [12][M]                                                                   */
    int32_t*     ncon_dev;             /* [M]                                                                       */
    int32_t*     dropped_dev;          /* [M] contacts beyond the budget of 16 arm contacts, not simulated          */
    int32_t*     con_kind_dev;         /* [20][M]                                                                   */
    int32_t*     con_feat_dev;         /* [20][M]                                                                   */
    float*       con_pos_dev;          /* [20][3][M] world, midway between the surfaces                             */
    float*       con_frame_dev;        /* [20][9][M]                                                                */
    float*       con_dist_dev;         /* [20][M]                                                                   */
    float*       con_force_dev;        /* [20][3][M]                                                                */
    float*       pad_force_dev;        /* [8][M] normal force summed over each finger pad's contacts                */
    float*       residual_dev;         /* [M] of the arm's solve (with its contacts; coupled: the cube's too): 0 when it converged, else the size of its last step */
} so100_forward_io;

int so100_query_forward(so100_sim* sim, const so100_forward_io* io, int32_t M, void* hip_stream);

/* Open-loop trajectories: where M states end up under M control sequences of T control steps, nsub physics substeps each -- the physics of
 * T calls of the step function without its task layer (no reward, TimeLimit, reset, RNG or curriculum motion of the cube), in one launch, with the state in
 * registers from the first substep to the last.  The handle's simulation does not move.
 *
 * Start.  qpos [13][M] and qvel [12][M] in the state getter's layout; qvel alone NULL: zero.  An explicit state starts cold, as a freshly
 * reset env: no warm start (friction-loss and limit forces, the cube's and the contact Newton's), no Kahan compensation, no force on the cube.
 * Both NULL: the handle's state (M must be N) -- the query continues the handle's simulation: it also reads (and never writes) the
 * warm-start rows, the Kahan rows and the anti-gravity bit of `bits`.  Within a call the warm starts carry from substep to substep and from
 * step to step; the contact solve's active-set memory restarts at each control step, as it does at each env step.
 *
 * Controls.  ctrl [T][6][M].  SO100_TRAJ_TARGETS: the servo targets in radians, one set per control step.  SO100_TRAJ_ACTIONS: actions; the
 * targets of step t are q(start of step t) + 0.075 a, each operation rounded (the reach envs' law).
 * flags: SO100_F_*, decided per call (the handle's own flags are not consulted).  T in 1..4096, nsub in 1..1024, T * nsub <= 65 536.
 *
 * Outputs.  Row t is the state after control step t.  ee: the reference's end-effector point at that q (the fresh value the kinematics query
 * gives for it, not the step kernels' stale pose).  ncon / dropped / sig / residual: the contact_stat & 255, contact_stat >> 8, contact_sig
 * and solver_residual rows a step with these controls would leave: the most records in one substep, the contacts over the budget, the
 * signature of the last substep's set, the largest solver residual.  bad_step: the first control step whose controls or resulting state
 * are not finite (a non-finite start: 0), -1 if none; from that step on the problem is not advanced, its float rows (the final ones
 * included) are NaN and its int rows 0.  The other problems never see it.  Every output is nullable; at least one is required.
 *
 * Argument errors, in this order: a null handle or io; M < 1 (or M != N where the handle's state is read); qvel_dev without qpos_dev; a null
 * ctrl_dev; an unknown mode; T, nsub or T * nsub outside the limits; flag bits outside SO100_F_*; SO100_F_PADS_CUBE or SO100_F_LINKS_CUBE
 * with SO100_F_CUBE_PINNED; an iteration count outside 1..64; no output. */
#define SO100_TRAJ_TARGETS      0
#define SO100_TRAJ_ACTIONS      1
#define SO100_TRAJ_MAX_T        4096
#define SO100_TRAJ_MAX_NSUB     1024
#define SO100_TRAJ_MAX_SUBSTEPS 65536
typedef struct {
    const float* qpos_dev;             /* [13][M] or NULL (with qvel_dev NULL: the handle's state)                 */
    const float* qvel_dev;             /* [12][M] or NULL                                                           */
    const float* ctrl_dev;             /* [T][6][M] targets (radians) or actions, by mode                           */
    int32_t      mode;                 /* SO100_TRAJ_TARGETS or SO100_TRAJ_ACTIONS                                  */
    int32_t      T;                    /* control steps, 1..4096                                                    */
    int32_t      nsub;                 /* substeps per control step, 1..1024; T * nsub <= 65 536                    */
    uint32_t     flags;                /* SO100_F_*                                                                 */
    int32_t      solver_iters;         /* 1..64                                                                     */
    int32_t      contact_iters;        /* 1..64                                                                     */
    float*       qpos_traj_dev;        /* [T][13][M]                                                                */
    float*       qvel_traj_dev;        /* [T][12][M]                                                                */
    float*       ee_traj_dev;          /* [T][3][M]                                                                 */
    float*       qpos_final_dev;       /* [13][M] row T - 1 of qpos_traj                                            */
    float*       qvel_final_dev;       /* [12][M] row T - 1 of qvel_traj                                            */
    int32_t*     ncon_dev;             /* [T][M]                                                                    */
    int32_t*     dropped_dev;          /* [T][M]                                                                    */
    int32_t*     sig_dev;              /* [T][M]                                                                    */
    float*       residual_dev;         /* [T][M]                                                                    */
    int32_t*     bad_step_dev;         /* [M]                                                                       */
} so100_trajectory_io;

int so100_query_trajectory(so100_sim* sim, const so100_trajectory_io* io, int32_t M, void* hip_stream);

/* Derivatives of one control step: for each of M (state, control) pairs the matrices A = dx'/dx [24][24] and B = dx'/du [24][6] of the
 * step the trajectory query takes with T = 1 -- MuJoCo's mjd_transitionFD.  The handle's simulation does not move.
 *
 * The result is a CENTRED SECANT over +-eps, like mjd_transitionFD with centred differences: column c is (x'(+eps e_c) - x'(-eps e_c))/(2 eps),
 * from 60 perturbed evaluations of the step and the unperturbed one, all in one wave of the GPU per problem.  With friction loss, joint limits
 * or contacts the step is not smooth and the result depends on eps: measured on the CPU under SO100_F_FRICTIONLOSS | SO100_F_LIMITS, the
 * fp64 oracle's own secants at 2^-10 and at 1e-6 differ by up to 0.17 on entries of size 8.  Forward (one-sided) differences are not offered.
 *
 * Tangent state.  x = (dq [12], v [12]) in MuJoCo's dof order -- arm 6, cube linear 3 in the world frame, cube angular 3 in the BODY frame --
 * for the position tangent and for qvel alike; u = the 6 controls.  Columns 0..11 of A perturb the position, 12..23 the velocity.  Every
 * component is perturbed by one rounded add, x +- eps, except the cube's orientation: quat <- normalize(quat (x) (cos(eps/2), +-sin(eps/2) e_i))
 * (mj_integratePos).  Rows: (x'+ - x'-)/(2 eps), except the cube's rotation rows 9..11: the rotation vector of (quat'-)^-1 (x) quat'+
 * (mju_subQuat) over 2 eps.  SO100_TRAJ_ACTIONS: a perturbed arm angle moves that evaluation's targets with it (the reach envs' law,
 * d ctrl / d q = I included).
 *
 * Start, controls, flags and iteration counts: as in so100_trajectory_io with T = 1 (ctrl [6][M]; an explicit state starts cold, the handle's
 * state continues with its warm-start rows, Kahan rows and anti-gravity bit, the same for all 61 evaluations).
 *
 * Layout.  A_dev [M][24][24] and B_dev [M][24][6] are PROBLEM-major, each matrix row-major -- the one exception to this header's SoA rule: a
 * wave owns a problem.  qpos_next [13][M], qvel_next [12][M] (the unperturbed step: so100_trajectory_io's final rows) and bad [M] are SoA.
 * bad = 1 where the start or the controls are not finite or any of the 61 evaluations comes out not finite; that problem's float outputs
 * are then NaN.  The other problems never see it.  Every output is nullable; at least one is required.
 *
 * Argument errors, in this order: those of so100_query_trajectory up to the iteration counts (nsub alone outside 1..1024 in place of its
 * T / nsub check); eps not finite or not positive; no output. */
#define SO100_DERIV_NX  24
#define SO100_DERIV_NU  6
#define SO100_DERIV_EPS 0.015625f      /* 2^-6: the smallest worst error of the fp32 arithmetic against the fp64 derivative */
typedef struct {
    const float* qpos_dev;             /* [13][M] or NULL (with qvel_dev NULL: the handle's state)                 */
    const float* qvel_dev;             /* [12][M] or NULL                                                           */
    const float* ctrl_dev;             /* [6][M] targets (radians) or actions, by mode                              */
    int32_t      mode;                 /* SO100_TRAJ_TARGETS or SO100_TRAJ_ACTIONS                                  */
    int32_t      nsub;                 /* substeps of the control step, 1..1024                                     */
    uint32_t     flags;                /* SO100_F_*                                                                 */
    int32_t      solver_iters;         /* 1..64                                                                     */
    int32_t      contact_iters;        /* 1..64                                                                     */
    float        eps;                  /* finite and > 0; a power of two makes 1 / (2 eps) exact                    */
    float*       A_dev;                /* [M][24][24]                                                               */
    float*       B_dev;                /* [M][24][6]                                                                */
    float*       qpos_next_dev;        /* [13][M]                                                                   */
    float*       qvel_next_dev;        /* [12][M]                                                                   */
    int32_t*     bad_dev;              /* [M]                                                                       */
} so100_derivatives_io;

int so100_query_derivatives(so100_sim* sim, const so100_derivatives_io* io, int32_t M, void* hip_stream);

/* LQR: the time-varying Riccati backward pass, the feedback gains and the linear forward pass of one iLQR / LQR / MPC iteration, for M
 * independent problems in one launch, one GPU wave per problem -- the step between the linearisation (so100_query_derivatives) and a better
 * plan.  The handle is taken for the device, the error slot and the conventions: its state is NEVER read or written.
 *
 * Per problem: horizon T, state-tangent size n = nx, 6 controls, dx_{t+1} = A_t dx_t + B_t du_t and the quadratic model
 *     sum_{t<T} [lx_t.dx_t + dx_t' lxx_t dx_t / 2 + lu_t.du_t + du_t' luu_t du_t / 2 + du_t' lux_t dx_t] + lx_T.dx_T + dx_T' lxx_T dx_T / 2.
 * Backward pass.  Vx = lx_T, Vxx = lxx_T; for t = T-1 .. 0:
 *     Qx  = lx_t  + A'Vx            Qu  = lu_t  + B'Vx
 *     Qxx = lxx_t + A'Vxx A         Qux = lux_t + B'Vxx A        Quu = luu_t + B'Vxx B
 *     Quu_r = Quu + reg I           (6 x 6 Cholesky; a pivot that is <= 0 or not finite FAILS the problem at this t)
 *     k = -Quu_r^-1 Qu              K = -Quu_r^-1 Qux
 *     dV1 += k'Qu                   dV2 += k'Quu k / 2           (the unregularised Quu, here and below)
 *     Vx  = Qx  + K'Quu k + K'Qu  + Qux'k
 *     Vxx = Qxx + K'Quu K + K'Qux + Qux'K;   Vxx <- (Vxx + Vxx')/2
 * (Tassa's form, correct under reg > 0).  lxx_t and luu_t are symmetric matrices: lxx_T is symmetrised like every later Vxx, and the lower
 * triangle of Quu_r is what is factored.
 * Linear forward pass, run only if du or dx is asked for.  dx_0 = dx0 (NULL: 0);  du_t = alpha k_t + K_t dx_t, or with u (the nominal controls)
 * du_t = clamp(u_t + alpha k_t + K_t dx_t, u_lo, u_hi) - u_t;  dx_{t+1} = A_t dx_t + B_t du_t.  The bounds are used only with u.
 *
 * Forms.  nx = 24: the full tangent state of the derivatives query.  nx = 12: the arm block, tangent indices 0..5 and 12..17 -- what a planner
 * under SO100_F_CUBE_PINNED uses.  A [T][M][24][24] and B [T][M][24][6] are ALWAYS in the derivatives query's output layout: what
 * so100_query_derivatives writes for T * M problems ordered t-major; the arm form reads its 12 rows and columns out of them.  Everything else
 * is in the n of the call and PROBLEM-major (the exception the derivatives query makes: a wave owns a problem).
 *
 * bad [M]: -1 where the problem is fine; the t at which the Cholesky failed; T for a non-finite input.  The inputs of step t are tested as the
 * backward pass reads them, so of a non-finite input at one step and a failing factor at a LATER step the later step is what is reported.
 * Every float output of a failed problem is NaN; the other problems never see it.  du and dx need k and K (the call has no storage of its
 * own).  Every output is nullable; at least one is required.
 *
 * Argument errors, in this order: a null handle or io; M < 1; nx not 12 or 24; T outside 1..4096; a required pointer (A, B, lx, lxx) that is
 * NULL; reg negative or not finite, alpha not finite, u_lo > u_hi; du or dx without k and K; no output. */
#define SO100_LQR_NU    6
#define SO100_LQR_MAX_T 4096
typedef struct {
    int32_t      nx;                   /* 24 or 12                                                                  */
    int32_t      T;                    /* horizon, 1..4096                                                          */
    const float* A_dev;                /* [T][M][24][24]                                                            */
    const float* B_dev;                /* [T][M][24][6]                                                             */
    const float* lx_dev;               /* [T+1][M][n]                                                               */
    const float* lxx_dev;              /* [T+1][M][n][n]                                                            */
    const float* lu_dev;               /* [T][M][6] or NULL: zero                                                   */
    const float* luu_dev;              /* [T][M][6][6] or NULL: zero                                                */
    const float* lux_dev;              /* [T][M][6][n] or NULL: zero                                                */
    const float* u_dev;                /* [T][M][6] nominal controls, or NULL: no clamp                             */
    const float* dx0_dev;              /* [M][n] or NULL: zero                                                      */
    float        reg;                  /* finite and >= 0                                                           */
    float        alpha;                /* finite: the step on k                                                     */
    float        u_lo;                 /* u_lo <= u_hi; used only with u_dev                                        */
    float        u_hi;
    float*       k_dev;                /* [T][M][6]                                                                 */
    float*       K_dev;                /* [T][M][6][n]                                                              */
    float*       Vx0_dev;              /* [M][n]                                                                    */
    float*       Vxx0_dev;             /* [M][n][n]                                                                 */
    float*       dV_dev;               /* [M][2]: dV1, dV2                                                          */
    float*       du_dev;               /* [T][M][6]                                                                 */
    float*       dx_dev;               /* [T+1][M][n]                                                               */
    int32_t*     bad_dev;              /* [M]                                                                       */
} so100_lqr_io;

int so100_query_lqr(so100_sim* sim, const so100_lqr_io* io, int32_t M, void* hip_stream);

/* LQR with a regulariser PER PROBLEM and a retry inside the launch: so100_query_lqr whose reg is the problem's own and whose backward pass, where
 * the Cholesky of Quu + reg I fails, is run again under a raised reg without a look from the host -- what an iLQR does between a failed factor
 * and the next try (Tassa's iLQG, MJPC).  One wave per problem as before; a problem that retries costs only itself.
 *
 * Per problem m:
 *   Start.  r = reg_dev ? reg_dev[m] : base.reg.  An r that is not finite or is negative is a non-finite input: bad = T, tries = 0,
 *           reg_used = NaN, and no pass runs.
 *   Raise.  raise(r) = min(reg_max, max(reg_min, r * reg_up)), the product rounded once in fp32; raise(0) = reg_min.
 *   Pass a = 1, 2, ...: the backward pass of so100_query_lqr with reg = r, from the terminal cost, dV1 and dV2 restarted.
 *           It goes through: the problem is done, bad = -1, reg_used = r, tries = a.
 *           The Cholesky fails at step t, a < tries and r < reg_max: r = raise(r), the next pass.
 *           Otherwise the problem fails: bad = the t of this last pass, reg_used = r, tries = a, every float output NaN as in so100_query_lqr.
 *           A non-finite input (bad = T) is found by the first pass and never retried: tries = 1, reg_used = r.
 *   The linear forward pass runs after the pass that went through, the NaN fill after a final failure, both unchanged.  No row of k or K that
 *   a failed pass wrote survives: each is written again or NaN.
 * Identities, bit for bit.  reg_dev = NULL and tries = 1: every output is so100_query_lqr's.  A problem that succeeds: every float output is what
 * so100_query_lqr gives for that problem alone with reg = reg_used[m].
 *
 * reg_used [M]: the reg of the LAST pass run.  tries [M]: the backward passes run, 1..tries; 0 for a start that is no reg.  Both nullable; they
 * count as outputs.  so100_query_reg_schedule (below) turns reg_used and the line search's verdict into the next call's reg_dev.
 *
 * Argument errors, in this order: a null handle or io; those of so100_query_lqr on base, from M < 1 to du or dx without k and K (base.reg is
 * checked even where reg_dev is given); reg_min not finite or <= 0; reg_max not finite or < reg_min; reg_up not finite or <= 1; tries outside
 * 1..SO100_LQR_REG_MAX_TRIES; no output. */
#define SO100_LQR_REG_MAX_TRIES 16
typedef struct {
    so100_lqr_io base;                 /* everything of so100_query_lqr; base.reg is used where reg_dev is NULL      */
    const float* reg_dev;              /* [M] starting reg per problem, or NULL: base.reg for all                   */
    float        reg_min;              /* finite, > 0                                                               */
    float        reg_max;              /* finite, >= reg_min                                                        */
    float        reg_up;               /* finite, > 1                                                               */
    int32_t      tries;                /* 1..16: backward passes allowed per problem                                */
    float*       reg_used_dev;         /* [M] the reg of the LAST pass run, or NULL                                 */
    int32_t*     tries_dev;            /* [M] backward passes run (1..tries; 0 for a start that is no reg), or NULL */
} so100_lqr_reg_io;

int so100_query_lqr_reg(so100_sim* sim, const so100_lqr_reg_io* io, int32_t M, void* hip_stream);

/* The regulariser's schedule: the line search's verdict on each problem becomes its next reg, on the device, one GPU lane per problem (the
 * handle's state is never read or written).  Per problem m:
 *     r = reg_used[m]; a value that is not finite or is negative counts as 0
 *     improved = best[m] >= 0 && best[m] != keep       (so100_query_cost_select's best: -1 where no candidate got through; keep: the index of the
 *                                                       candidate that IS the old plan, alpha = 0, or -1 where there is none)
 *     improved:      r' = r * reg_down, and r' = 0 where r' < reg_min            (Tassa's rule: a reg under reg_min is 0)
 *     not improved:  r' = raise(r) of so100_query_lqr_reg
 *     reg[m] = r';  improved[m] = 1 or 0
 * reg_dev may be reg_used_dev.
 *
 * Argument errors, in this order: a null handle or io; M < 1; reg_used_dev, best_dev or reg_dev NULL; keep < -1; reg_min, reg_max, reg_up as in
 * so100_query_lqr_reg; reg_down not in (0, 1]. */
typedef struct {
    const float*   reg_used_dev;       /* [M] so100_query_lqr_reg's                                                 */
    const int32_t* best_dev;           /* [M] so100_query_cost_select's best                                        */
    int32_t        keep;               /* the candidate index that IS the old plan (alpha = 0), or -1: none         */
    float          reg_min;            /* as in so100_lqr_reg_io                                                    */
    float          reg_max;
    float          reg_up;
    float          reg_down;           /* finite, in (0, 1]                                                         */
    float*         reg_dev;            /* [M] the next reg; may alias reg_used_dev                                  */
    uint8_t*       improved_dev;       /* [M] or NULL                                                               */
} so100_reg_schedule_io;

int so100_query_reg_schedule(so100_sim* sim, const so100_reg_schedule_io* io, int32_t M, void* hip_stream);

/* Closed-loop trajectories: the trajectory query under a time-varying feedback law around a nominal plan -- the NONLINEAR forward pass of iLQR
 * at L step sizes at once (the line search's candidates), and LQR tracking of one plan from disturbed starts.  M problems with L candidates each
 * are M * L rollouts of T control steps, nsub substeps each, one GPU lane per rollout with the state in registers throughout.  The handle's
 * simulation does not move.
 *
 * Start (qpos_dev, qvel_dev; both NULL: the handle's state with its warm-start rows, Kahan rows and anti-gravity bit, M = N; an explicit state
 * starts cold), mode, T, nsub, flags, solver_iters, contact_iters and their limits: exactly as in so100_trajectory_io.  All L candidates of a
 * problem start from the same state.
 *
 * Nominal plan.  u [T][6][M] (SoA, the trajectory query's ctrl).  qpos_ref [T][13][M] and qvel_ref [T][12][M] hold in row t the nominal state
 * AFTER step t -- what so100_query_trajectory writes as qpos_traj / qvel_traj, passed straight in; the nominal state at the start of step
 * t >= 1 is row t - 1, and row T - 1 is never read (T = 1: the references may be NULL).  qpos_ref0 [13][M], qvel_ref0 [12][M]: the nominal
 * state at the start of step 0; both NULL: the start itself, dx_0 = 0 exactly (the iLQR case).
 * Gains.  nx = 24 or 12 (the arm block, tangent indices 0..5 and 12..17: the reference's cube rows are then never read).  k [T][M][6] and
 * K [T][M][6][nx] are PROBLEM-major, bit for bit what so100_query_lqr writes.  k NULL: zero.
 * Candidates.  L in 1..SO100_CL_MAX_L; alpha: a HOST pointer to L finite floats, copied into the launch.
 *
 * Law, per rollout at step t, from the state x_t the step starts from:
 *     dx  = x_t (-) xref_t       in the derivatives query's tangent: a rounded difference per row, the rotation vector of quat_ref^-1 (x) quat
 *                                (mju_subQuat) for the cube's rotation rows 9..11
 *     c_j = u_j + (alpha k_j + sum_i K_ji dx_i)       i ascending, the sum started from alpha k_j
 *     c_j = clamp(c_j, u_lo, u_hi)                    where clamp != 0
 * and c is the step's control as in so100_trajectory_io (SO100_TRAJ_ACTIONS: the targets are q(start of step t) + 0.075 c).
 *
 * Outputs.  SoA over the M * L rollouts, rollout (m, a) in column m L + a.  u_traj [T][6][ML]: the controls applied -- the chosen candidate's
 * column is the next plan.  The others: as in so100_trajectory_io; bad_step also fires at step t where a gain, a nominal control or a reference
 * row read at step t is not finite.  A failed rollout's float rows are NaN from that step on; no other rollout sees it.  Every output is
 * nullable; at least one is required.
 *
 * Argument errors, in this order: those of so100_query_trajectory up to the iteration counts (u_dev in ctrl_dev's place); nx not 12 or 24;
 * L outside 1..16 or M * L over INT32_MAX; a null alpha, K_dev, or (T > 1) qpos_ref_dev or qvel_ref_dev; exactly one of qpos_ref0_dev and
 * qvel_ref0_dev; an alpha that is not finite; clamp with u_lo > u_hi or a bound that is not finite; no output. */
#define SO100_CL_MAX_L 16
typedef struct {
    const float* qpos_dev;             /* [13][M] or NULL (with qvel_dev NULL: the handle's state)                 */
    const float* qvel_dev;             /* [12][M] or NULL                                                           */
    const float* u_dev;                /* [T][6][M] nominal controls: targets (radians) or actions, by mode         */
    int32_t      mode;                 /* SO100_TRAJ_TARGETS or SO100_TRAJ_ACTIONS                                  */
    int32_t      T;                    /* control steps, 1..4096                                                    */
    int32_t      nsub;                 /* substeps per control step, 1..1024; T * nsub <= 65 536                    */
    uint32_t     flags;                /* SO100_F_*                                                                 */
    int32_t      solver_iters;         /* 1..64                                                                     */
    int32_t      contact_iters;        /* 1..64                                                                     */
    const float* qpos_ref_dev;         /* [T][13][M] nominal state after step t (T = 1: may be NULL)                */
    const float* qvel_ref_dev;         /* [T][12][M]                                                                */
    const float* qpos_ref0_dev;        /* [13][M] nominal state at the start, or NULL: the start itself             */
    const float* qvel_ref0_dev;        /* [12][M] or NULL, together with qpos_ref0_dev                              */
    int32_t      nx;                   /* 24 or 12                                                                  */
    const float* k_dev;                /* [T][M][6] or NULL: zero                                                   */
    const float* K_dev;                /* [T][M][6][nx]                                                             */
    int32_t      L;                    /* candidates per problem, 1..16                                             */
    const float* alpha;                /* HOST pointer to L finite floats                                           */
    int32_t      clamp;                /* != 0: c is kept in [u_lo, u_hi]                                           */
    float        u_lo;
    float        u_hi;
    float*       u_traj_dev;           /* [T][6][ML] the controls applied                                           */
    float*       qpos_traj_dev;        /* [T][13][ML]                                                               */
    float*       qvel_traj_dev;        /* [T][12][ML]                                                               */
    float*       ee_traj_dev;          /* [T][3][ML]                                                                */
    float*       qpos_final_dev;       /* [13][ML] row T - 1 of qpos_traj                                           */
    float*       qvel_final_dev;       /* [12][ML] row T - 1 of qvel_traj                                           */
    int32_t*     ncon_dev;             /* [T][ML]                                                                   */
    int32_t*     dropped_dev;          /* [T][ML]                                                                   */
    int32_t*     sig_dev;              /* [T][ML]                                                                   */
    float*       residual_dev;         /* [T][ML]                                                                   */
    int32_t*     bad_step_dev;         /* [ML]                                                                      */
} so100_closed_loop_io;

int so100_query_closed_loop(so100_sim* sim, const so100_closed_loop_io* io, int32_t M, void* hip_stream);

/* The cost family of the two cost queries below: a tracked point drawn to a target, joint angles drawn to a nominal pose, joint velocities
 * and controls drawn to zero.  A HOST struct, copied into the launch.  Per state row (q, the arm's v, the target g):
 *     r = point(q) - g                                        point: link and offset exactly as in so100_jacobian_io
 *     s = w_point (r0^2 + r1^2 + r2^2) + sum_j w_q[j] (q_j - q_nom_j)^2 + sum_j w_v[j] v_j^2          summed in that order, j ascending
 * the control cost of step t is c_t = sum_j w_u[j] u_tj^2, and the total of a rollout of T steps
 *     J = sum_{t<T} (c_t + sigma_t s_t)                       t ascending; sigma_{T-1} = w_terminal, every other sigma_t = 1
 * with s_t taken at the state AFTER step t (row t of a trajectory): the start is not a decision variable and is not counted.
 * Target.  SO100_COST_TARGET_FIXED: target_dev [3][M], one point per problem.  SO100_COST_TARGET_TRAJ: target_dev [T][3][M], row t with the
 * state after step t.  SO100_COST_TARGET_CUBE: the cube's position, rows 6..8 of the same qpos row; target_dev is not read. */
#define SO100_COST_TARGET_FIXED 0
#define SO100_COST_TARGET_TRAJ  1
#define SO100_COST_TARGET_CUBE  2
typedef struct {
    int32_t      link;                 /* 0..5                                                                      */
    const float* offset;               /* HOST pointer to 3 finite floats or NULL (so100_jacobian_io)               */
    int32_t      target_mode;          /* SO100_COST_TARGET_*                                                       */
    float        w_point;              /* every weight finite and >= 0                                              */
    float        w_q[6];
    float        q_nom[6];             /* finite                                                                    */
    float        w_v[6];
    float        w_u[6];
    float        w_terminal;           /* multiplies the state terms of the LAST state row                          */
} so100_cost_def;

/* Cost terms: the quadratic model of that cost along M trajectories of T steps, written in the LQR query's input layout -- lx, lxx, lu and luu
 * are bit for bit what so100_query_lqr takes, with no operation in between.  The handle is taken for the device and the error slot: its state
 * is NEVER read or written.
 *
 * Inputs.  qpos_traj [T][13][M] and qvel_traj [T][12][M]: what the trajectory and closed-loop queries write (qvel_traj NULL: zero).  u [T][6][M]
 * (SoA, the trajectory query's ctrl).  nx = 24 or 12 (the arm block, tangent indices 0..5 and 12..17).
 * Outputs, with n = nx, PROBLEM-major like the LQR query's inputs.  Row 0 of lx and lxx is zero.  Row t + 1 is the model of sigma_t s_t at the state
 * after step t, in the derivatives query's tangent, with J = jacp of the point:
 *     lx[0..5]   = 2 sigma (w_point J'r + w_q o (q - q_nom))          lxx[0..5][0..5] = 2 sigma (w_point J'J + diag w_q)
 *     lx[12..17] = 2 sigma w_v o v   (6..11 where n = 12)             lxx diagonal 12..17 = 2 sigma w_v
 * This is the GAUSS-NEWTON model: the term of the point's second derivative, w_point sum_a r_a d2 p_a / dq2, is dropped.  With the cube target and
 * n = 24 the cube's world-frame linear tangent 6..8 enters with dr/dx = -I: lx[6..8] = -2 sigma w_point r, lxx[0..5][6..8] = -2 sigma w_point J'
 * and its transpose, lxx[6..8][6..8] = 2 sigma w_point I; with n = 12 those columns are dropped (the pinned-cube planner's case).  Every other
 * entry of lxx is zero, and lxx is symmetric to the bit: entry (i, j) is computed from (min, max).  lu_t = 2 w_u o u_t, luu_t = diag(2 w_u).
 * A value that is not finite among those a state row's cost reads (q, the arm's v, the target) makes that row's lx and lxx NaN -- all of
 * them -- and a u_t that is not finite makes lu_t and luu_t NaN; so100_query_lqr then reports bad = T for that problem.  No other problem sees it.
 * Every output is nullable; at least one is required.
 *
 * Argument errors, in this order: a null handle or io; M < 1; nx not 12 or 24; T outside 1..SO100_LQR_MAX_T; a null cost; link outside 0..5; an
 * offset that is not finite; an unknown target_mode; a weight that is negative or not finite or a q_nom that is not finite; a required pointer
 * (qpos_traj_dev, u_dev; target_dev unless the target is the cube) that is NULL; no output. */
typedef struct {
    const so100_cost_def* cost;        /* HOST pointer                                                              */
    const float* target_dev;           /* [3][M] or [T][3][M] by target_mode; not read with the cube target         */
    int32_t      nx;                   /* 24 or 12                                                                  */
    int32_t      T;                    /* horizon, 1..4096                                                          */
    const float* qpos_traj_dev;        /* [T][13][M] the state after step t                                         */
    const float* qvel_traj_dev;        /* [T][12][M] or NULL: zero                                                  */
    const float* u_dev;                /* [T][6][M]                                                                 */
    float*       lx_dev;               /* [T+1][M][n]                                                               */
    float*       lxx_dev;              /* [T+1][M][n][n]                                                            */
    float*       lu_dev;               /* [T][M][6]                                                                 */
    float*       luu_dev;              /* [T][M][6][6]                                                              */
} so100_cost_terms_io;

int so100_query_cost_terms(so100_sim* sim, const so100_cost_terms_io* io, int32_t M, void* hip_stream);

/* Cost select: the line search's decision on the closed-loop query's output -- the total cost J of each of M * L rollouts, per problem the
 * cheapest candidate, and its controls gathered as the next plan.  One GPU lane per rollout.  The handle's state is NEVER read or written.
 *
 * Inputs.  Rollout (m, a) is in column m L + a, the closed-loop query's output layout: qpos_traj [T][13][ML], qvel_traj [T][12][ML] (NULL: zero),
 * u_traj [T][6][ML] the controls applied, bad_step [ML] (NULL: none failed).  Targets are per PROBLEM, [3][M] or [T][3][M]: a problem's candidates
 * share them.  u_fallback [T][6][M] (nullable): the plan to keep where no candidate can be taken.
 * Outputs.  cost [ML]: J, or +inf where bad_step >= 0 or J is not finite.  best [M]: the candidate with the smallest cost, ties to the LOWEST
 * index, -1 if every candidate is +inf.  best_cost [M]: its cost, +inf where best = -1.  u_best [T][6][M]: the winner's column of u_traj; where
 * best = -1 the column of u_fallback, or NaN without one.  The result is the same bits on every run, whatever M, L and the problem's place.
 * Every output is nullable; at least one is required.
 *
 * Argument errors, in this order: a null handle or io; M < 1; T outside 1..SO100_LQR_MAX_T; L outside 1..SO100_CL_MAX_L or M * L over INT32_MAX;
 * then those of the cost as in so100_cost_terms_io (from the null cost to q_nom); a required pointer (qpos_traj_dev, u_traj_dev; target_dev unless
 * the target is the cube) that is NULL; no output. */
typedef struct {
    const so100_cost_def* cost;        /* HOST pointer                                                              */
    const float* target_dev;           /* [3][M] or [T][3][M] by target_mode; not read with the cube target         */
    int32_t      T;                    /* horizon, 1..4096                                                          */
    int32_t      L;                    /* candidates per problem, 1..16                                             */
    const float* qpos_traj_dev;        /* [T][13][ML]                                                               */
    const float* qvel_traj_dev;        /* [T][12][ML] or NULL: zero                                                 */
    const float* u_traj_dev;           /* [T][6][ML]                                                                */
    const int32_t* bad_step_dev;       /* [ML] or NULL                                                              */
    const float* u_fallback_dev;       /* [T][6][M] or NULL                                                         */
    float*       cost_dev;             /* [ML]                                                                      */
    int32_t*     best_dev;             /* [M]                                                                       */
    float*       best_cost_dev;        /* [M]                                                                       */
    float*       u_best_dev;           /* [T][6][M]                                                                 */
} so100_cost_select_io;

int so100_query_cost_select(so100_sim* sim, const so100_cost_select_io* io, int32_t M, void* hip_stream);

/* Plan sample: the candidates of a sampling planner (MPPI, CEM), K perturbed copies of each of N nominal plans, written in the trajectory
 * query's INPUT layout -- ctrl, qpos_rep and qvel_rep are bit for bit what so100_query_trajectory takes for M = N K problems, with no operation
 * in between.  One GPU lane per candidate.  The handle is taken for the device and the error slot: its state is NEVER read or written.
 *
 * Candidates.  plan [T][6][N] (SoA); candidate (n, k) is column n K + k of ctrl [T][6][NK]:
 *     ctrl[t][j][n K + k] = clamp(plan[t][j][n] + sigma[j] eps(n, k, t, j), u_lo, u_hi)       the product and the sum each rounded once
 * Candidate k = 0 has eps = 0 and a dimension with sigma[j] = 0 is never perturbed: both are clamp(plan) itself.  A plan entry that is not
 * finite is NaN in all K candidates (the trajectory query then reports bad_step for them).
 * Noise.  A function of (seed, draw, id_offset + n, k, t, j) alone, so a problem's candidates are the same bits whatever N is and wherever it
 * stands in the batch: for b in 0, 1 the Philox4x32-10 counter is (id_offset + n, draw, k, 0x4D500000 | t << 1 | b), the key (seed & 0xffffffff,
 * seed >> 32); words (2i, 2i + 1) of block b give eps[4b + 2i], eps[4b + 2i + 1] by the policy noise's Box-Muller transform (u1 = ((r_even >> 8) + 1) 2^-24,
 * u2 = (r_odd >> 8) 2^-24, rad = sqrt(-2 ln u1), ang = 2 pi u2 - pi, (rad cos ang, rad sin ang)); the first six of the eight are j = 0..5.
 * draw: the planner's call counter.  id_offset: the global index of problem 0 (a sharded caller draws what an unsharded one would).
 * Fan-out.  qpos_rep [13][NK] and qvel_rep [12][NK]: each problem's start copied to its K columns, bit for bit.
 * Every output is nullable; at least one is required.
 *
 * Argument errors, in this order: a null handle or io; N < 1; T outside 1..SO100_TRAJ_MAX_T; K outside 1..SO100_MPPI_MAX_K or N * K over
 * INT32_MAX; a sigma that is negative or not finite; u_lo or u_hi not finite or u_lo > u_hi; a null plan_dev; qvel_dev without qpos_dev;
 * qpos_rep_dev without qpos_dev or qvel_rep_dev without qvel_dev; no output. */
#define SO100_MPPI_MAX_K 4096
typedef struct {
    const float* plan_dev;             /* [T][6][N] the nominal controls                                            */
    float        sigma[6];             /* finite and >= 0; 0: that dimension is never perturbed                     */
    float        u_lo;                 /* finite, u_lo <= u_hi                                                      */
    float        u_hi;
    int32_t      K;                    /* candidates per problem, 1..4096; N * K <= INT32_MAX                       */
    int32_t      T;                    /* control steps, 1..4096                                                    */
    uint64_t     seed;
    uint32_t     draw;                 /* the planner's call counter                                                */
    uint32_t     id_offset;            /* the global index of problem 0                                             */
    const float* qpos_dev;             /* [13][N] or NULL                                                           */
    const float* qvel_dev;             /* [12][N] or NULL                                                           */
    float*       ctrl_dev;             /* [T][6][NK]                                                                */
    float*       qpos_rep_dev;         /* [13][NK]                                                                  */
    float*       qvel_rep_dev;         /* [12][NK]                                                                  */
} so100_plan_sample_io;

int so100_query_plan_sample(so100_sim* sim, const so100_plan_sample_io* io, int32_t N, void* hip_stream);

/* Cost blend: the sampling planner's decision on the trajectory query's output -- the total cost J of each of N * K rollouts (so100_cost_def,
 * exactly as so100_query_cost_select computes it), per problem the soft-min weights over its K candidates and the weighted mean of their controls
 * as the next plan.  One GPU workgroup per problem.  The handle's state is NEVER read or written.
 *
 * Inputs.  Those of so100_cost_select_io with K in place of L: rollout (n, k) in column n K + k of qpos_traj [T][13][NK], qvel_traj [T][12][NK]
 * (NULL: zero), u_traj [T][6][NK] the controls applied (so100_plan_sample_io's ctrl), bad_step [NK] (NULL: none failed); targets per PROBLEM;
 * u_fallback [T][6][N] (nullable).  temperature: lambda.
 * Outputs.  cost [NK], best [N], best_cost [N]: as in so100_cost_select_io.
 *     weight[n K + k] = exp(-(J_k - J_min) / lambda) / sum_k exp(-(J_k - J_min) / lambda)       0 where J_k = +inf; all 0 where best = -1
 *     ess[n]          = 1 / sum_k w_k^2   the effective sample size; 0 where best = -1
 *     blend[t][j]     = sum_k w_k u_traj[t][j][n K + k]       (a candidate of weight 0 is not read into it)
 * u_first [6][N]: row 0 of the blend, the control to execute now.  u_plan [T][6][N]: the blend; with shift = 1 row t holds blended row t + 1 and
 * row T - 1 is 0 (SO100_BLEND_TAIL_ZERO: the actions mode's "stay") or blended row T - 1 again (SO100_BLEND_TAIL_HOLD: servo targets) -- the
 * receding-horizon step.  Where best = -1 the blend is the column of u_fallback, or NaN without one, shifted the same way (a ZERO tail row is 0 there too).
 * J_min is an exact minimum and every sum over k is taken in one fixed order that depends on K alone: a problem's outputs are the same bits on
 * every run, whatever N is and wherever the problem stands, and each output is the same whether requested alone or with the others.  K = 1
 * returns w = 1 and its only candidate's controls, bit for bit.  Every output is nullable; at least one is required.
 *
 * Argument errors, in this order: a null handle or io; N < 1; T outside 1..SO100_TRAJ_MAX_T; K outside 1..SO100_MPPI_MAX_K or N * K over
 * INT32_MAX; those of the cost as in so100_cost_terms_io (from the null cost to q_nom); a temperature that is not finite or not positive;
 * shift not 0 or 1; an unknown tail; a required pointer (qpos_traj_dev, u_traj_dev; target_dev unless the target is the cube) that is NULL;
 * no output. */
#define SO100_BLEND_TAIL_ZERO 0
#define SO100_BLEND_TAIL_HOLD 1
typedef struct {
    const so100_cost_def* cost;        /* HOST pointer                                                              */
    const float* target_dev;           /* [3][N] or [T][3][N] by target_mode; not read with the cube target         */
    int32_t      T;                    /* horizon, 1..4096                                                          */
    int32_t      K;                    /* candidates per problem, 1..4096; N * K <= INT32_MAX                       */
    const float* qpos_traj_dev;        /* [T][13][NK]                                                               */
    const float* qvel_traj_dev;        /* [T][12][NK] or NULL: zero                                                 */
    const float* u_traj_dev;           /* [T][6][NK]                                                                */
    const int32_t* bad_step_dev;       /* [NK] or NULL                                                              */
    const float* u_fallback_dev;       /* [T][6][N] or NULL                                                         */
    float        temperature;          /* lambda, finite and > 0                                                    */
    int32_t      shift;                /* 0, or 1: u_plan is the blend moved up one step                            */
    int32_t      tail;                 /* SO100_BLEND_TAIL_*: row T - 1 of a shifted u_plan                         */
    float*       cost_dev;             /* [NK]                                                                      */
    int32_t*     best_dev;             /* [N]                                                                       */
    float*       best_cost_dev;        /* [N]                                                                       */
    float*       weight_dev;           /* [NK]                                                                      */
    float*       ess_dev;              /* [N]                                                                       */
    float*       u_plan_dev;           /* [T][6][N]                                                                 */
    float*       u_first_dev;          /* [6][N]                                                                    */
} so100_cost_blend_io;

int so100_query_cost_blend(so100_sim* sim, const so100_cost_blend_io* io, int32_t N, void* hip_stream);

/* Plan sample with a sigma per entry: so100_query_plan_sample with the noise scale read from the device, one per (step, joint, problem) -- what a
 * cross-entropy planner refits after every round (so100_query_cost_refit's sigma_out, passed on as it is).  Layout, noise counter words,
 * candidate 0, clamp, fan-out rows and the lane map are so100_query_plan_sample's:
 *     ctrl[t][j][n K + k] = clamp(plan[t][j][n] + sigma[t][j][n] eps(n, k, t, j), u_lo, u_hi)
 * With sigma[t][j][n] = s[j] the output equals so100_query_plan_sample's under sigma = s bit for bit.  An entry whose sigma is 0 is clamp(plan) in
 * every candidate.  An entry whose sigma is negative, NaN or infinite cannot be refused on the host: it is NaN in every candidate k >= 1 (the
 * trajectory query then reports bad_step for them); candidate 0 stays clamp(plan) and no other entry moves.
 *
 * Argument errors, in this order: those of so100_query_plan_sample with "a null sigma_dev" where the sigma check stands. */
typedef struct {
    const float* plan_dev;             /* [T][6][N] the nominal controls                                            */
    const float* sigma_dev;            /* [T][6][N] the noise scale per entry; 0: that entry is never perturbed     */
    float        u_lo;                 /* finite, u_lo <= u_hi                                                      */
    float        u_hi;
    int32_t      K;                    /* candidates per problem, 1..4096; N * K <= INT32_MAX                       */
    int32_t      T;                    /* control steps, 1..4096                                                    */
    uint64_t     seed;
    uint32_t     draw;                 /* the planner's call counter                                                */
    uint32_t     id_offset;            /* the global index of problem 0                                             */
    const float* qpos_dev;             /* [13][N] or NULL                                                           */
    const float* qvel_dev;             /* [12][N] or NULL                                                           */
    float*       ctrl_dev;             /* [T][6][NK]                                                                */
    float*       qpos_rep_dev;         /* [13][NK]                                                                  */
    float*       qvel_rep_dev;         /* [12][NK]                                                                  */
} so100_plan_sample_tv_io;

int so100_query_plan_sample_tv(so100_sim* sim, const so100_plan_sample_tv_io* io, int32_t N, void* hip_stream);

/* Cost refit: the cross-entropy planner's decision on the trajectory query's output -- the total cost J of each of N * K rollouts (exactly as
 * so100_query_cost_blend computes it), per problem the E cheapest candidates, and the mean and standard deviation of their controls, smoothed
 * against the old ones, as the next plan and the next sigma.  One GPU workgroup per problem.  The handle's state is NEVER read or written.
 *
 * Inputs.  so100_cost_blend_io's rollouts, cost, targets, bad_step and u_fallback, with the same meaning.  E: the number of elites.  alpha: the
 * smoothing factor; plan [T][6][N] and sigma [T][6][N]: the old mean and sigma (each nullable; both required with alpha > 0, neither read with
 * alpha = 0).  sigma_min[j] <= sigma_out <= sigma_max[j]; sigma_init[j]: the sigma of a row that has no history.
 * Outputs.  cost [NK], best [N], best_cost [N]: so100_cost_blend_io's, the same bits.
 *     order        candidate k stands before k' iff J_k < J_k' or (J_k = J_k' and k < k'); rank(k): the number of candidates before k
 *     elites       k is an elite iff rank(k) < E and J_k is finite (+inf: a failed or non-finite rollout);  n_elite[n] = min(E, finite costs)
 *     elite [N][E] the elites in ascending rank, -1 from slot n_elite on;  threshold[n]: the cost of the last elite, +inf where there is none
 *     per row (t, j), over the elites:   mu = (sum u_k) / n_elite;  var = (sum (u_k - mu)^2) / n_elite;  sd = sqrt(var)
 *     mean_new  = alpha plan + (1 - alpha) mu
 *     sigma_new = clamp(alpha sigma + (1 - alpha) sd, sigma_min[j], sigma_max[j])
 * The order is total, so the elite set is unique: the same on every run, whatever N, the problem's place, the outputs asked for and the way it
 * is found.  Both sums over the elites are taken in so100_cost_blend_io's one order over k = 0..K-1 with a non-elite's term left out (its
 * controls are never read into a sum and may be anything): the bits depend on K and the elite set alone.  The variance is the population
 * variance in two passes; every product is rounded once before it is added, each operation of the smoothing is rounded once, and with alpha = 0
 * the old value's term is not formed: mean_new is mu and sigma_new is clamp(sd) as they are.  n_elite = 1 gives sd = 0; E = K = 1 gives the
 * candidate's controls as mean, bit for bit.
 * u_first [6][N]: row 0 of mean_new before the shift.  mean [T][6][N]: mean_new, with shift = 1 moved up one step with the tail row as in
 * so100_cost_blend_io's u_plan.  sigma_out [T][6][N]: sigma_new, moved up the same way; its row T - 1 is then sigma_init[j] under either tail.
 * Where best = -1 (no finite cost): n_elite = 0, the elite slots are -1, threshold = +inf, mean is the column of u_fallback (or NaN without one)
 * shifted as in the blend, and sigma_out is sigma_init[j] in every row.
 * Every output is nullable; at least one is required; each is the same bits whether requested alone or with the others.
 *
 * Argument errors, in this order: those of so100_cost_blend_io up to and including the cost's; E outside 1..K; an alpha that is not finite or
 * outside [0, 1); a sigma_min, sigma_max or sigma_init entry that is not finite, negative, or sigma_min > sigma_max; shift not 0 or 1; an unknown
 * tail; a required pointer (qpos_traj_dev, u_traj_dev; target_dev unless the target is the cube; plan_dev and sigma_dev with alpha > 0) that is
 * NULL; no output. */
typedef struct {
    const so100_cost_def* cost;        /* HOST pointer                                                              */
    const float* target_dev;           /* [3][N] or [T][3][N] by target_mode; not read with the cube target         */
    int32_t      T;                    /* horizon, 1..4096                                                          */
    int32_t      K;                    /* candidates per problem, 1..4096; N * K <= INT32_MAX                       */
    const float* qpos_traj_dev;        /* [T][13][NK]                                                               */
    const float* qvel_traj_dev;        /* [T][12][NK] or NULL: zero                                                 */
    const float* u_traj_dev;           /* [T][6][NK]                                                                */
    const int32_t* bad_step_dev;       /* [NK] or NULL                                                              */
    const float* u_fallback_dev;       /* [T][6][N] or NULL                                                         */
    int32_t      E;                    /* elites per problem, 1..K                                                  */
    float        alpha;                /* smoothing: the old value's share, finite and in [0, 1)                    */
    const float* plan_dev;             /* [T][6][N] the old mean; required with alpha > 0                           */
    const float* sigma_dev;            /* [T][6][N] the old sigma; required with alpha > 0                          */
    float        sigma_min[6];         /* finite, 0 <= sigma_min <= sigma_max                                       */
    float        sigma_max[6];
    float        sigma_init[6];        /* finite and >= 0: row T - 1 of a shifted sigma_out; every row where best = -1 */
    int32_t      shift;                /* 0, or 1: mean and sigma_out are moved up one step                         */
    int32_t      tail;                 /* SO100_BLEND_TAIL_*: row T - 1 of a shifted mean                           */
    float*       cost_dev;             /* [NK]                                                                      */
    int32_t*     best_dev;             /* [N]                                                                       */
    float*       best_cost_dev;        /* [N]                                                                       */
    int32_t*     elite_dev;            /* [N][E]                                                                    */
    int32_t*     n_elite_dev;          /* [N]                                                                       */
    float*       threshold_dev;        /* [N]                                                                       */
    float*       mean_dev;             /* [T][6][N]                                                                 */
    float*       sigma_out_dev;        /* [T][6][N]                                                                 */
    float*       u_first_dev;          /* [6][N]                                                                    */
} so100_cost_refit_io;

int so100_query_cost_refit(so100_sim* sim, const so100_cost_refit_io* io, int32_t N, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SO100_QUERY_H */
