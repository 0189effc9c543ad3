/* include/osot_mi355x.h -- the drop-in C-ABI of the MI355X-native OpenSoT hot path.
 *
 * Plain C: opaque handles, POD structs, raw pointers + sizes, int error codes; no C++/Eigen/torch
 * types cross this boundary and no exception does.  Implemented by
 * opensot_amd/csrc/libosot_mi355x.so (hand-written HIP for gfx950).
 *
 * What each group replaces in the reference (ADVRHumanoids/OpenSoT @2024-10-24; paths relative to
 * the reference root):
 *
 *  osot_plan_desc ................ the *result* of the stack algebra (src/utils/AutoStack.cpp:7-331,
 *                                  examples/cpp/coman_ik.cpp:425-449): levels -> leaf task blocks,
 *                                  box-bound producers, global constraint-row producers.  Static.
 *  osot_stack_update ............. AutoStack::update()            src/utils/AutoStack.cpp:385-393
 *                                  (-> Task::update Task.h:375-400, tasks::Aggregated::_update
 *                                  src/tasks/Aggregated.cpp:92-132, constraints::Aggregated::update
 *                                  src/constraints/Aggregated.cpp:60-257 and the leaf _update()s)
 *  osot_ihqp_solve ............... Solver::solve() = iHQP::solve  src/solvers/iHQP.cpp:263-358
 *                                  (computeCostFunction :129-162, optimality rows :164-170,
 *                                  one BackEnd::solve per level, QPOasesBackEnd.cpp:248-307)
 *  osot_backend_* ................ the BackEnd plugin surface     include/OpenSoT/solvers/BackEnd.h:23-171
 *                                  and its C factory `create_instance`
 *                                  (src/solvers/QPOasesBackEnd.cpp:14-24), batch-of-one, host pointers
 *  osot_kinematics ............... batched frame poses / Jacobians / CoM: what the leaf _update()s fetch from
 *                                  XBot::ModelInterface (velocity/Cartesian.cpp:73-81, velocity/CoM.cpp:59-74)
 *  osot_allgather_dq ............. new surface (the reference has no multi-instance API): collects the
 *                                  per-rank dq shards; RCCL all-gather on the solve stream
 *
 * All batched arrays are INSTANCE-MAJOR, row-major inside an instance, fp64, resident in HBM:
 *   X[B][rows][n]  ->  element (i, r, c) at ((i*rows)+r)*n + c.
 * One wavefront solves one instance, so an instance's rows are a single contiguous, coalesced read.
 */
#ifndef OSOT_MI355X_H
#define OSOT_MI355X_H

#include <stddef.h>   /* size_t */

#ifdef __cplusplus
extern "C" {
#endif

#define OSOT_MAX_LEVELS 8
#define OSOT_MAX_TASKS 8      /* leaf task blocks per level   */
#define OSOT_MAX_BOUNDS 4     /* box-bound producers          */
#define OSOT_MAX_ROWBLOCKS 8  /* constraint-row blocks (global and task-local) */
#define OSOT_MAX_BAND_ROWS 6  /* rows of a task used as a constraint (TaskToConstraint error band) */
#define OSOT_MAX_VARS 64      /* one lane per variable        */
#define OSOT_MAX_QP_VARS 128  /* the explicit-QP surface (osot_qp_solve_batch, osot_backend_*): 65 .. 128 variables run one
                                 256-thread workgroup per QP instead of one wavefront (round 6; no graph capture; hot start through
                                 osot_qp_solve_batch_hot only -- osot_backend_solve starts cold above OSOT_MAX_VARS);
                                 plans: osot_solver_create (the wavefront route) stays at OSOT_MAX_VARS, osot_solver_create_wide
                                 takes up to OSOT_MAX_QP_VARS; nHQP / eHQP and the ADMM kernel stay at OSOT_MAX_VARS */

/* error codes (the reference returns bool / throws std::runtime_error) */
enum {
    OSOT_OK = 0,
    OSOT_ERR_INVALID = 1,      /* bad argument / size mismatch (BackEnd.cpp:23-27, :47-60)          */
    OSOT_ERR_UNSUPPORTED = 2,  /* plan uses something this build does not implement                 */
    OSOT_ERR_HIP = 3,          /* a HIP runtime call failed (osot_last_error() has the text)        */
    OSOT_ERR_NOT_SOLVED = 4,   /* batch-of-one back-end: QP infeasible / iteration limit            */
    OSOT_ERR_COMM = 5          /* RCCL failure                                                       */
};

/* per-instance status written by osot_ihqp_solve (the reference's `bool` per solve,
 * iHQP.cpp:279-347; failed instances return dq = 0 like examples/cpp/coman_ik.cpp:189-190) */
enum {
    OSOT_STATUS_SOLVED = 0,
    OSOT_STATUS_INFEASIBLE = 1,
    OSOT_STATUS_MAX_ITER = 2,
    OSOT_STATUS_NOT_PD = 3      /* Cholesky of H + eps I broke down */
};

/* ---- static stack plan ---------------------------------------------------------------------- */
typedef enum {
    OSOT_TASK_GENERIC = 0,   /* tasks::GenericTask (src/tasks/GenericTask.cpp:5-56): A and b supplied   */
    OSOT_TASK_CARTESIAN = 1, /* velocity::Cartesian (src/tasks/velocity/Cartesian.cpp:68-105, 279-285)  */
    OSOT_TASK_COM = 2,       /* velocity::CoM (src/tasks/velocity/CoM.cpp:59-74, 145-149)               */
    OSOT_TASK_POSTURAL = 3,  /* velocity::Postural (src/tasks/velocity/Postural.cpp:50-62, 97-100);
                                A = [I_rows 0] is implicit (never stored), rows <= n; must be the last block of
                                its level */
    /* inverse-dynamics formulation, x = [qddot; contact forces] (src/utils/InverseDynamics.cpp:12-28).  The
     * producer writes the task matrix ([J 0] ...) into A_k; the update computes b from the supplied errors. */
    OSOT_TASK_ACC_CARTESIAN = 4, /* acceleration::Cartesian (src/tasks/acceleration/Cartesian.cpp:127-180):
                                    b = a_ref + lambda2*Kd*vel_err + lambda*Kp*pose_err - Jdot*qdot (Kp = Kd = I
                                    unless osot_task_desc.acc_gain_matrices) */
    OSOT_TASK_ACC_COM = 5,       /* acceleration::CoM (src/tasks/acceleration/CoM.cpp:74-97), 3 rows */
    OSOT_TASK_ACC_POSTURAL = 6   /* acceleration::Postural (src/tasks/acceleration/Postural.cpp:135-163):
                                    A = [I_rows 0] implicit like OSOT_TASK_POSTURAL,
                                    b = qddot_ref + lambda2*(qdot_ref - qdot) + lambda*(q_ref - q) */
} osot_task_kind;

typedef struct {
    int kind;                /* osot_task_kind */
    int rows;                /* 6 / 3 / n / user-defined */
    double weight;           /* scalar on this block's W: `0.1*l_wrist` (AutoStack.cpp:16-47) */
    double lambda;           /* Task::setLambda; enters b only (Cartesian.cpp:284, CoM.cpp:148) */
    double orientation_gain; /* Cartesian::setOrientationErrorGain (Cartesian.cpp:283) */
    double lambda2;          /* velocity gain of the acceleration tasks (acceleration/Cartesian.cpp:158) */
    /* SubTask (src/tasks/SubTask.cpp:22-112, `task % {indices}`): this block keeps only some rows of a parent task.
     * row_mask bit i = row i of the parent is kept (0: not a sub-task); rows = popcount(row_mask); parent_rows = rows
     * of the parent (0: the kind's own size: 6 / 3 / n); b = sub_lambda * b_parent[kept rows] (SubTask.cpp:56-57);
     * the weight is the parent's scalar.  The producer writes the kept Jacobian rows; a Postural sub-task is NOT
     * implicit: its unit rows are stored like any other block's. */
    unsigned long long row_mask;
    int parent_rows;
    double sub_lambda;
    /* velocity::Cartesian with a BODY Jacobian (Cartesian::setIsBodyJacobian, src/tasks/velocity/Cartesian.cpp:93-100):
     * A and b are both rotated by Ad(R') with R the actual orientation.  The producer writes the rotated Jacobian
     * (osot_kin_desc.frame_body does); the update rotates b.  0 = world frame. */
    int body_frame;
    /* non-diagonal weight matrix (Task::setWeight(W) with a full W, include/OpenSoT/Task.h:273-300; in an aggregate the
     * level's W is blockdiag(weight_i * W_i), src/tasks/Aggregated.cpp:265-279).  1: the block's W_i [B][rows][rows]
     * comes with the leaf inputs (osot_leaf_ptrs.W); the update then forms W_k A_k and W_k b_k for the whole level
     * (osot_assembled_out.WA / Wb) and the cascade takes them as the left operand of H = A'(WA), g = -A'(Wb).  A
     * Postural block with dense_weight is stored like any other block (its unit rows are written by the producer). */
    int dense_weight;
    /* gain MATRICES of the acceleration tasks (acceleration::Cartesian::setGains(Kp, Kd), setKp / setKd,
     * src/tasks/acceleration/Cartesian.cpp:152-173; round 3 -- before: Kp = Kd = I).  1: the task's leaf array p0 carries
     * them per instance behind the errors, p0 = [pose_err (rows); vel_err (rows); Gp (rows x rows, row-major); Gd (rows x
     * rows)], and b = a_ref + lambda2 Gd vel_err + lambda Gp pose_err - Jdot qdot.
     *   GainType::Acceleration (:155-160): Gp = Kp, Gd = Kd, the same for every instance.
     *   GainType::Force        (:161-169): Gp = Mi Kp, Gd = Mi Kd with Mi = J B^-1 J' the inverse Cartesian inertia, and the
     *     virtual force enters as a_ref + Mi f -- osot_id_force_gains below writes all three from J, B^-1, Kp, Kd, f.
     * Only OSOT_TASK_ACC_CARTESIAN / OSOT_TASK_ACC_COM; 0 = scalar gains. */
    int acc_gain_matrices;
} osot_task_desc;

typedef struct {
    int n_tasks;
    osot_task_desc task[OSOT_MAX_TASKS]; /* tasks::Aggregated row order (Aggregated.cpp:113-132) */
} osot_level_desc;

typedef enum {
    OSOT_BOUND_GENERIC = 0,        /* l,u supplied */
    OSOT_BOUND_JOINT_LIMITS = 1,   /* velocity::JointLimits (src/constraints/velocity/JointLimits.cpp:37-58) */
    OSOT_BOUND_VELOCITY_LIMITS = 2,/* velocity::VelocityLimits (…/VelocityLimits.cpp:72-89) */
    /* velocity::JointLimitsInvariance (src/constraints/velocity/JointLimitsInvariance.cpp:47-206): the velocity-IK box that also
     * respects an acceleration limit.  dT = the control period dt (> 0), scaling = the step-ahead predictor p (0 < p <= 1,
     * setPStepAheadPredictor).  Per joint, with s = q_max - q, i = q_min - q (q = the leaf's q - q_neutral) and v = qdot_prev:
     *   ub = (v <= 0) ? min(s, dt^2 a + dt v) : min(via, dt^2 a + dt v), via = +-sqrt(|2 a dt^2 p s|) with the sign of s;
     *   lb the mirror image (v >= 0; -a; i); lb > ub swaps the two.  qdot_prev is the leaf p2: the caller advances it
     * (qdot_prev = dq / dt) between cycles, which is why osot_control_rollout refuses such a plan for steps > 1. */
    OSOT_BOUND_JOINT_LIMITS_INVARIANCE = 3
} osot_bound_kind;

typedef struct {
    int kind;       /* osot_bound_kind */
    double scaling; /* JointLimits boundScaling; JOINT_LIMITS_INVARIANCE: the step-ahead predictor p */
    double dT;      /* VelocityLimits dT; JOINT_LIMITS_INVARIANCE: dt */
} osot_bound_desc;

typedef enum {
    OSOT_ROWS_GENERIC = 0,  /* constraints::GenericConstraint / TaskToConstraint rows: C, lo, up supplied */
    OSOT_ROWS_COLLISION = 1,/* velocity::CollisionAvoidance rows (…/CollisionAvoidance.cpp:96-152):
                               -J_d dq <= max(0, s (d - d_min)) for pairs within the detection threshold */
    /* inverse-dynamics constraint rows on x = [qddot; forces] */
    OSOT_ROWS_DYN_FEASIBILITY = 2, /* acceleration::DynamicFeasibility as an equality (DynamicFeasibility.cpp:22-46):
                                      producer writes [B_u, -J_f'] (6 rows); lo = up = -h_u */
    OSOT_ROWS_TORQUE_LIMITS = 3,   /* acceleration::TorqueLimits (src/constraints/acceleration/TorqueLimits.cpp:25-46):
                                      producer writes [B, -Jc'] ; lo = -tau_max - h, up = tau_max - h */
    OSOT_ROWS_FRICTION_CONE = 4,   /* force::FrictionCone (src/constraints/force/FrictionCone.cpp:35-56): 5 rows per
                                      contact = pyramid(mu/sqrt2) * wRl' on the contact's 3 force columns,
                                      lo = -1e20, up = 0; rows = 5 * contacts, first_col = first force column */
    OSOT_ROWS_ACC_JOINT_LIMITS = 5,/* acceleration::JointLimits (src/constraints/acceleration/JointLimits.cpp:58-176):
                                      unit rows e_(first_col+i) (NOT stored), bounds from q, qdot, limits */
    OSOT_ROWS_ACC_VELOCITY_LIMITS = 6,/* acceleration::VelocityLimits (…/VelocityLimits.cpp:50-63): unit rows
                                      (NOT stored), (qdot_lim - qdot)/(dT*p) */
    /* constraints::TaskToConstraint (src/constraints/TaskToConstraint.cpp:25-68; `stack << l_sole` in
     * examples/cpp/coman_ik.cpp:430-449): the rows are the task's A (written by the producer into C, like the task's
     * Jacobian into A_k), the bounds are the task's b computed HERE from the task's leaf inputs, widened by the block's
     * error band: lo = b + err_lb, up = b + err_ub (0, 0: the task as an equality).  task_lambda /
     * task_orientation_gain are the task's gains. */
    OSOT_ROWS_TASK_CARTESIAN = 7,     /* velocity::Cartesian as a constraint: 6 rows; leaf as for OSOT_TASK_CARTESIAN */
    OSOT_ROWS_TASK_COM = 8,           /* velocity::CoM as a constraint: 3 rows; leaf as for OSOT_TASK_COM */
    OSOT_ROWS_UNIT_GENERIC = 9,       /* unit rows e_(first_col+i) (NOT stored), lo / up supplied: a box on a range of
                                         variables as rows.  With only_level = k + 1 this is a TASK-LOCAL BOUND
                                         (`task << joint_limits`: iHQP merges a level's own bounds into that level's
                                         box only, iHQP.cpp:190, 336-340).  force::WrenchLimits is such a block on
                                         a contact's 6 wrench columns (releaseContact: lo = up = 0) */
    /* surface contacts: `contacts` consecutive 6-D wrenches [f_x f_y f_z tau_x tau_y tau_z], the wrench of contact ct in
     * columns first_col + 6 ct .. + 5.  Stored rows (written into C by every update), lo = -1e20, up = 0.  Leaf p0 =
     * wRl [B][contacts][9] row-major (the contact link's rotation, as for OSOT_ROWS_FRICTION_CONE); Ad = blockdiag(wRl', wRl')
     * (_Ti.linear() of the contact pose T).  p1 = [B][contacts][4] (x_l, x_u, y_l, y_u): the X_Lims / Y_Lims of the foot. */
    OSOT_ROWS_WRENCH_FRICTION_CONE = 10, /* force::FrictionCone on a wrench (FrictionCone.cpp:35-56): 5 rows per contact,
                                            pyramid(mu/sqrt2) * wRl' on the force columns, 0 on the torque columns */
    OSOT_ROWS_COP = 11,               /* force::CoP (CoP.cpp:24-69): 4 rows per contact, Ai * Ad (the CoP inside the
                                         rectangle [x_l, x_u] x [y_l, y_u]) */
    OSOT_ROWS_NORMAL_TORQUE = 12,     /* force::NormalTorque (NormalTorque.cpp:5-69): 8 rows per contact, A0 * Ad2 * Ad
                                         with mu = the block's mu */
    /* (13, 14 and 15 are not kinds: both validators refuse them as "unknown row-block kind") */
    /* velocity::ConvexHull (src/constraints/velocity/ConvexHull.cpp:41-134, src/utils/convex_hull_utils.cpp:142-174): the CoM's
     * ground projection stays inside the support polygon of the contact points.  rows = P contact points (3 .. 16) = the fixed
     * number of rows (_C(links_in_contact.size(), 2)); bound_scaling = the safety margin in metres (setSafetyMargin).  Stored
     * rows, written by every update: the points are taken relative to the CoM and projected on z = 0, their convex hull is built
     * in fp64 (exact sign tests, no epsilon; duplicates of a lower-indexed point and points on a segment between two others are
     * no vertices), row r is the edge from the r-th hull vertex IN ORDER OF POINT INDEX to its counter-clockwise successor:
     * (a, b, c) of getLineCoefficients, C_r = +-(a J_com,x + b J_com,y), up_r = |c| - margin sqrt(a^2 + b^2) (the sign as
     * getConstraints picks it: c <= 0 keeps (a, b)), lo_r = -1e20.  Rows at or beyond the vertex count: C_r = 0, up_r = 1e10,
     * lo_r = -1e20 (the reference's A.setZero(), b = 1e10).  Fewer than three vertices (all points coincident or collinear): all
     * P rows are written that way -- the reference keeps its PREVIOUS hull there; the update is stateless. */
    OSOT_ROWS_CONVEX_HULL = 16,
    /* (17 is not a kind either) */
    /* The recursively feasible acceleration joint limits: unit rows e_(first_col+i) (NOT stored), like OSOT_ROWS_ACC_JOINT_LIMITS in
     * every generic respect (first_col, only_level).  q below is the leaf's ONE q - q_neutral (the convention of
     * OSOT_ROWS_ACC_JOINT_LIMITS): the reference takes the raw q in Viability's M2 / m2 and difference(q, neutral) elsewhere, which
     * differ only for a model whose neutral posture is not zero.  min / max are std::min / std::max, `(b < a) ? b : a` and
     * `(a < b) ? b : a`: a NaN second argument is ignored (a joint exactly on a limit at rest gives M2 = -0/0), unlike fmin / fmax. */
    OSOT_ROWS_ACC_JOINT_LIMITS_VIABILITY = 18, /* acceleration::JointLimitsViability (src/constraints/acceleration/
                                      JointLimitsViability.cpp:79-190): dt = dT*p (p >= 1 the step-ahead predictor, dT*p > 0);
                                      ub = min(pos, (qdot_max - qdot)/dt, viability, qddot_max), lb the mirror image, ub < lb swaps the
                                      two, then both are clamped into [-qddot_max, qddot_max] */
    OSOT_ROWS_ACC_JOINT_LIMITS_ECBF = 19,      /* acceleration::JointLimitsECBF (…/JointLimitsECBF.cpp:36-71): ub = min(-(a1 + a2) qdot
                                      + a1 a2 (q_max - q), a3 (qdot_max - qdot), qddot_max), lb the mirror image; swap and clamp as
                                      above; a1, a2, a3 per joint (setAlpha1/2/3); dT and p are not read */
    /* velocity::CartesianPositionConstraint (src/constraints/velocity/CartesianPositionConstraint.cpp:81-108): R half-spaces
     * A_c x <= b_c on the position x of a link (POSITION_CARTESIAN) or of the CoM (POSITION_COM).  rows = R (1 .. 16), STORED rows
     * written by every update: C = A_c J[0:3], up = (b_c - A_c x) * bound_scaling, lo = -1e20. */
    OSOT_ROWS_POSITION_CARTESIAN = 20,
    OSOT_ROWS_POSITION_COM = 21
    /* a kind added behind 21 needs its own branch in update_body (opensot_amd/csrc/osot_kernels.h): the update kernel hands every
     * kind from 18 upwards to limit_kind_rows, whose last branch is the position rows; the validators refuse 22 and above today */
} osot_rows_kind;

typedef struct {
    int kind;  /* osot_rows_kind */
    int rows;  /* for COLLISION: max_pairs; for CONVEX_HULL: contact points; for POSITION_*: half-spaces */
    double d_threshold, detection_threshold, bound_scaling;   /* bound_scaling of CONVEX_HULL: the safety margin (metres); of
                                                                 POSITION_*: CartesianPositionConstraint's boundScaling */
    int first_col;   /* unit-row / friction-cone / surface-contact blocks: column of the block's first variable */
    double dT, p;    /* acceleration limits: time step and horizon factor (dt = dT*p); VIABILITY: p >= 1; ECBF: not read */
    double mu;       /* friction coefficient */
    double task_lambda, task_orientation_gain;   /* OSOT_ROWS_TASK_*: gains of the underlying task */
    double err_lb[OSOT_MAX_BAND_ROWS], err_ub[OSOT_MAX_BAND_ROWS];   /* OSOT_ROWS_TASK_*: TaskToConstraint's error band,
                        one pair per row (err_lb / err_ub are vectors, src/constraints/TaskToConstraint.cpp:34-52, 61-68) */
    int task_body_frame;   /* OSOT_ROWS_TASK_CARTESIAN: the task has a body Jacobian (see osot_task_desc.body_frame) */
    int n_candidates;      /* OSOT_ROWS_COLLISION: collision pairs supplied per instance (0 = rows).  With more candidates
                              than rows the `rows` CLOSEST pairs are taken, in order of distance
                              (getOrderedCollisionPairIndices, src/constraints/velocity/CollisionAvoidance.cpp:120-131) */
    int only_level;  /* 0 = global rows: constrain every level (AutoStack `<<`, iHQP.cpp:191-193).  k + 1 = TASK-LOCAL
                        rows of level k (`task << constraint`, Task::getConstraints(), iHQP.cpp:190, 282-287): they
                        constrain the QP of level k only; at every other level they are absent */
} osot_rows_desc;

typedef struct {
    int n;         /* number of variables (<= OSOT_MAX_VARS) */
    int n_levels;
    osot_level_desc level[OSOT_MAX_LEVELS];
    int n_bounds;  /* 0 = no box (iHQP.cpp:340-344 then never calls updateBounds) */
    osot_bound_desc bound[OSOT_MAX_BOUNDS];
    int n_rowblocks;
    osot_rows_desc rowblock[OSOT_MAX_ROWBLOCKS];
    double eps_abs;  /* absolute epsilon on diag(H): 1e3 * 2.221e-16 * eps_factor
                        (QPOasesBackEnd.cpp:57,67; qpOASES Options.cpp:147) */
    int max_iter;    /* active-set iteration cap per level; 0 = default (the reference's nWSR is 13200,
                        QPOasesBackEnd.cpp:30) */
    /* user regularisation task (AutoStack::setRegularisationTask, include/OpenSoT/utils/AutoStack.h:78-92): iHQP adds
     * its cost to the cost of EVERY level, H += Hr, g += gr (iHQP.cpp:265-266, 274-278); it never becomes an
     * optimality row.  Supported: identity-Jacobian tasks A_r = [I_rows 0] with W_r = weight * I, i.e.
     * OSOT_TASK_GENERIC (b supplied: GenericTask(I, b) as in tests/solvers/TestiHQP.cpp:118-120, MinimumVelocity
     * with b = 0), OSOT_TASK_POSTURAL and OSOT_TASK_ACC_POSTURAL; row_mask must be 0.  Then Hr = weight * [I_rows 0;
     * 0 0] is folded into the diagonal and gr = -weight * b_r.  (A stored Jacobian: regularisation_dense below.) */
    int has_regularisation;
    osot_task_desc regularisation;
    /* regularisation task with a STORED Jacobian (round 3; iHQP.cpp:265-278 takes any task): 1 = A_r is the
     * [B][regularisation.rows][n] array osot_qp_batch.A_reg (written by the producer, like a level's A_k), W_r = weight * I,
     * b_r from the update like any task of its kind (TASK_GENERIC, TASK_CARTESIAN, TASK_COM); H += A_r'W_r A_r and
     * g -= A_r'W_r b_r at every level, never an optimality row.  0 = the identity-Jacobian form above. */
    int regularisation_dense;
} osot_plan_desc;

/* ---- assembled, batched QP data (device pointers) ------------------------------------------ */
typedef struct {
    int B;                              /* instances in this call (<= max_batch of the solver) */
    const double* A[OSOT_MAX_LEVELS];   /* [B][ma_k][n], ma_k = rows of the non-Postural blocks */
    const double* b[OSOT_MAX_LEVELS];   /* [B][m_k] */
    const double* w[OSOT_MAX_LEVELS];   /* [B][m_k] diagonal of W_k; NULL = identity */
    const double* c[OSOT_MAX_LEVELS];   /* [B][n] Task::getc(); NULL = 0 */
    const double* C;                    /* [B][nc_stored][n] global rows: the STORED row blocks stacked in plan
                                           order (unit-row blocks have no storage, see osot_plan_constraint_rows) */
    const double* lo;                   /* [B][nc] (all rows, stored or not) */
    const double* up;                   /* [B][nc] */
    const double* l;                    /* [B][n] merged box; NULL iff plan.n_bounds == 0 */
    const double* u;                    /* [B][n] */
    const unsigned char* level_active;  /* HOST pointer, [n_levels] iHQP::setActiveStack
                                           (iHQP.cpp:391-395); NULL = all active */
    double* dq;                         /* out [B][n]: x of the last active level (iHQP.cpp:349) */
    double* x_levels;                   /* out [B][n_levels][n], may be NULL */
    int* status;                        /* out [B] OSOT_STATUS_* */
    int* iterations;                    /* out [B] active-set iterations summed over levels; may be NULL */
    const double* b_reg;                /* [B][regularisation.rows] b of the regularisation task; NULL iff the plan
                                           has none */
    const double* WA[OSOT_MAX_LEVELS];  /* [B][ma_k][n] W_k A_k and                                              */
    const double* Wb[OSOT_MAX_LEVELS];  /* [B][m_k]     W_k b_k of a level with a non-diagonal W_k (written by
                                           osot_stack_update); NULL = diagonal W_k (w[k])                          */
    double* accepted_slack;             /* out [B], may be NULL: the largest constraint violation that a level of the
                                           instance accepted as round-off of the levels above it (no direction left and
                                           no multiplier to trade; at most min(1e-6 * max(1, |bound|), 1e-5)); 0 = none.
                                           The status stays OSOT_STATUS_SOLVED, like the reference's `true` when qpOASES
                                           stops inside its own tolerances */
    const double* A_reg;                /* [B][regularisation.rows][n] Jacobian of the regularisation task; read iff
                                           plan.regularisation_dense */
} osot_qp_batch;

/* ---- leaf inputs of AutoStack::update (device pointers) ------------------------------------ */
/* meaning of (p0, p1, p2) by kind:
 *   TASK_CARTESIAN : p0 = actual pose  [B][12] (R row-major 9, then p 3), p1 = desired pose [B][12],
 *                    p2 = desired twist [B][6] (NULL = 0)
 *   TASK_COM       : p0 = actual CoM [B][3], p1 = desired CoM [B][3], p2 = desired velocity [B][3] (NULL = 0)
 *   TASK_POSTURAL  : p0 = q [B][n], p1 = q_desired [B][n], p2 = v_desired [B][n] (NULL = 0)
 *   TASK_GENERIC   : p0 = b [B][rows] (copied);  p1, p2 unused
 *   BOUND_JOINT_LIMITS    : p0 = q - q_neutral [B][n], p1 = q_min [B][n], p2 = q_max [B][n]
 *   BOUND_VELOCITY_LIMITS : p0 = qdot_max [B][n]
 *   BOUND_GENERIC         : p0 = l [B][n], p1 = u [B][n]
 *   BOUND_JOINT_LIMITS_INVARIANCE : p0 = q - q_neutral [B][n], p1 = [q_min ; q_max ; qddot_max] [B][3*n], p2 = qdot_prev [B][n]
 *   ROWS_COLLISION : p0 = distance Jacobians J_d [B][rows][n] (ordered by distance), p1 = distances [B][rows]
 *   ROWS_GENERIC   : p0 = C [B][rows][n], p1 = lo [B][rows], p2 = up [B][rows]
 *   TASK_ACC_CARTESIAN / TASK_ACC_COM : p0 = [pose_err ; vel_err] [B][2*rows], p1 = Jdot*qdot [B][rows],
 *                    p2 = a_ref [B][rows] (NULL = 0)
 *   TASK_ACC_POSTURAL : p0 = [q_ref - q ; qdot_ref - qdot] [B][2*rows], p2 = qddot_ref [B][rows] (NULL = 0)
 *   ROWS_DYN_FEASIBILITY : p0 = h_u [B][6]            (the 6 x n rows are written by the producer into C)
 *   ROWS_TORQUE_LIMITS   : p0 = h [B][rows], p1 = tau_max [B][rows]   (rows written by the producer into C)
 *   ROWS_FRICTION_CONE   : p0 = contact rotations wRl [B][contacts][9] (row-major)
 *   ROWS_ACC_JOINT_LIMITS    : p0 = [q ; qdot] [B][2*rows], p1 = [q_min ; q_max] [B][2*rows], p2 = qddot_max [B][rows]
 *   ROWS_ACC_VELOCITY_LIMITS : p0 = qdot [B][rows], p1 = qdot_max [B][rows]
 *   ROWS_UNIT_GENERIC : p0 = lo [B][rows], p1 = up [B][rows]
 *   ROWS_TASK_CARTESIAN / ROWS_TASK_COM : as TASK_CARTESIAN / TASK_COM (the 6 / 3 rows are written by the producer into C)
 *   ROWS_COP / ROWS_NORMAL_TORQUE / ROWS_WRENCH_FRICTION_CONE : p0 = wRl [B][contacts][9], p1 = x / y limits [B][contacts][4]
 *   ROWS_CONVEX_HULL : p0 = CoM Jacobian [B][3][n] (rows 0 and 1 are read: what osot_kin_batch.com_J writes with
 *                    com_J_stride = 3 n), p1 = CoM [B][3], p2 = world positions of the contact points [B][rows][3]
 *                    (osot_kin_batch.points)
 *   ROWS_ACC_JOINT_LIMITS_VIABILITY : p0 = [q - q_neutral ; qdot] [B][2*rows], p1 = [q_min ; q_max] [B][2*rows],
 *                    p2 = [qdot_max ; qddot_max] [B][2*rows]
 *   ROWS_ACC_JOINT_LIMITS_ECBF : p0, p1 as above, p2 = [qdot_max ; qddot_max ; a1 ; a2 ; a3] [B][5*rows]
 *   ROWS_POSITION_CARTESIAN : p0 = the link's Jacobian [B][6][n] (rows 0 .. 2 are read: what osot_kin_batch.frame_J writes with
 *                    frame_J_stride = 6 n), p1 = the link's pose [B][12] ([R row-major | p]; p is read), p2 = [A_c (rows x 3
 *                    row-major) ; b_c (rows)] [B][4*rows]
 *   ROWS_POSITION_COM : p0 = CoM Jacobian [B][3][n], p1 = CoM [B][3], p2 as for ROWS_POSITION_CARTESIAN
 * Task Jacobians are NOT passed here: the producer writes them straight into their row range of
 * osot_qp_batch.A[k] (zero-copy stacking; the reference copies them twice through MatrixPiler,
 * src/tasks/Aggregated.cpp:113-132).
 *   any task with dense_weight : W = the block's weight matrix [B][rows][rows] (row-major) */
typedef struct { const double *p0, *p1, *p2, *W; } osot_leaf_ptrs;

typedef struct {
    int B;
    osot_leaf_ptrs task[OSOT_MAX_LEVELS][OSOT_MAX_TASKS];
    osot_leaf_ptrs bound[OSOT_MAX_BOUNDS];
    osot_leaf_ptrs rows[OSOT_MAX_ROWBLOCKS];
    osot_leaf_ptrs regularisation;      /* leaf inputs of the regularisation task (same meaning as for its kind) */
} osot_leaf_batch;

/* writable view of the assembled arrays that osot_stack_update fills (same shapes as osot_qp_batch) */
typedef struct {
    double* b[OSOT_MAX_LEVELS];
    double* w[OSOT_MAX_LEVELS];         /* NULL = leave the weights alone: for a DIAGONAL W_k with per-row entries
                                           (Task::setWeight(W), Aggregated.cpp:265-279) fill osot_qp_batch.w[k] once */
    double* C;
    double* lo;
    double* up;
    double* l;
    double* u;
    double* b_reg;                      /* [B][regularisation.rows]; NULL iff the plan has no regularisation task */
    double* WA[OSOT_MAX_LEVELS];        /* [B][ma_k][n], [B][m_k]: required for the levels that hold a dense_weight block  */
    double* Wb[OSOT_MAX_LEVELS];
    const double* A[OSOT_MAX_LEVELS];   /* the stacked Jacobians A_k the producer wrote (read to form W_k A_k); required for
                                           the same levels */
} osot_assembled_out;

typedef struct osot_solver osot_solver;

/* library / device */
const char* osot_version(void);
const char* osot_last_error(void);           /* thread-local text of the last failure */
int osot_device_count(int* count);

/* plan-derived sizes (host only, no GPU needed).
 * osot_plan_validate: the WAVEFRONT route (osot_solver_create): 1 <= n <= OSOT_MAX_VARS, one wavefront per instance.
 * osot_plan_validate_wide: the WORKGROUP route (osot_solver_create_wide): 1 <= n <= OSOT_MAX_QP_VARS with the same feature set
 * (every task kind, implicit and stored Postural blocks, diagonal and dense weights, c vectors, sub-tasks of parents of at most
 * 64 rows, body frames, gain matrices, both regularisation forms, every bound and row kind, global and task-local rows); the
 * rows of all levels and the constraint rows together at most 2048 (OSOT_ERR_UNSUPPORTED beyond), and the row table must fit
 * the LDS of a CU. */
int osot_plan_validate(const osot_plan_desc* plan);
int osot_plan_validate_wide(const osot_plan_desc* plan);
int osot_plan_level_rows(const osot_plan_desc* plan, int level, int* m_total, int* m_stored);
int osot_plan_constraint_rows(const osot_plan_desc* plan, int* nc);
int osot_plan_stored_constraint_rows(const osot_plan_desc* plan, int* nc_stored);

/* solver object: owns the per-plan device workspace for up to max_batch instances on `device` */
int osot_solver_create(const osot_plan_desc* plan, int max_batch, int device, osot_solver** out);
/* The same solver object for the WORKGROUP route (plans of 1 .. OSOT_MAX_QP_VARS variables; opensot_amd/csrc/osot_cascade_wide.h):
 * the iHQP cascade runs one 256-thread workgroup per instance on the dual active-set solver of osot_qp_solve_batch's wide path, the
 * grid capped at the workgroups the device holds at once, each with a slice of a workspace (2 n^2 doubles) allocated here, once:
 * no allocation per call, so osot_cycle on a wide handle can be captured into a HIP graph.  On a wide handle:
 *   osot_solver_destroy, osot_stack_update, osot_ihqp_solve, osot_solver_set_task_active, osot_solver_set_timing,
 *   osot_solver_kernel_time_ms .... as on the wavefront route (the timing brackets the cascade launch);
 *   osot_cycle ...................... TWO launches on the stream (osot_stack_update's kernel, then the cascade); results are
 *                                     bit-identical to the two calls;
 *   osot_solver_set_schedule, osot_solver_set_specialisation ... accepted, without effect (instances are dispatched in order);
 *   osot_solver_resident_waves ...... the instances in flight: resident workgroups of the wide kernel (one instance each);
 *                                     the cold kernel's figure -- a hot launch (below) never runs more workgroups than that;
 *   osot_ihqp_solve_hot, osot_cycle_hot ... the same two calls with every level's working set carried from cycle to cycle in a
 *                                     device array the CALLER owns (below); osot_solver_set_hotstart stays refused here;
 *   osot_nhqp_solve, osot_ehqp_solve, osot_control_cycle, osot_control_rollout, osot_solver_set_hotstart(s, 1),
 *   osot_solver_profile_phases, osot_solver_resident_waves_nhqp ... OSOT_ERR_UNSUPPORTED with a reason.
 * A level's status and accepted_slack follow the wavefront route's rules (round-off of the levels above: at most
 * min(1e-6 * max(1, |bound|), 1e-5), status SOLVED). */
int osot_solver_create_wide(const osot_plan_desc* plan, int max_batch, int device, osot_solver** out);
int osot_solver_destroy(osot_solver* s);

/* Hot start on the WORKGROUP route (reference: QPOasesBackEnd.cpp:258-285, SQProblem.cpp:149-193), with caller-owned state as in
 * osot_qp_solve_batch_hot.  hot_state: device int32 [B][n_levels][128] (osot_solver_hot_state_ints: n_levels * 128 per instance), row i
 * = instance i of the batch; an entry is 2 * position + (upper side ? 1 : 0) of a position in that LEVEL's row table -- position
 * < n: the box, n + r: constraint row r (global and task-local rows) -- or -1 for none.  Fill it with -1 before the first call (and
 * an instance's row whenever that robot is reset); several states (one per pipelined sub-batch) may be used with one solver.
 * Per instance, every ACTIVE level reads its list before its solve (re-adding the constraints as in osot_solver_set_hotstart) and
 * rewrites it, compacted, with the inequality working set it ended with; a level that fails records 128 x -1 and ends the instance,
 * the lists of the levels below it, and of levels switched off by level_active, are left as they are.  Entries that are no
 * inequality of the level (out of range, equality or optimality rows, infinite sides, rows of an inactive task) are skipped: any
 * content is safe.  The answer does not depend on the lists beyond round-off, only the iteration counts do.
 * hot_state == NULL: exactly osot_ihqp_solve / osot_cycle.  No allocation and no synchronisation: capturable into a HIP graph like
 * osot_cycle on a wide handle.  A handle of osot_solver_create: OSOT_ERR_UNSUPPORTED (use osot_solver_set_hotstart there). */
int osot_solver_hot_state_ints(osot_solver* s, int* ints_per_instance);
int osot_ihqp_solve_hot(osot_solver* s, const osot_qp_batch* batch, int* hot_state, void* hip_stream);
int osot_cycle_hot(osot_solver* s, const osot_leaf_batch* leaf, const osot_assembled_out* out, const osot_qp_batch* batch,
                   int* hot_state, void* hip_stream);

/* AutoStack::update() for B instances: leaf inputs -> b_k, w_k, merged box, constraint rows.
 * Stream-ordered on `hip_stream` (a hipStream_t passed as void*, NULL = default stream). */
int osot_stack_update(osot_solver* s, const osot_leaf_batch* leaf, const osot_assembled_out* out,
                      void* hip_stream);

/* Solver::solve() for B instances: the whole iHQP cascade in one launch. Stream-ordered. */
int osot_ihqp_solve(osot_solver* s, const osot_qp_batch* batch, void* hip_stream);

/* One control cycle in ONE launch: osot_stack_update followed by osot_ihqp_solve for the same B instances
 * (`stack->update(); solver->solve(dq)`, examples/cpp/coman_ik.cpp:186-192) with each instance's update and cascade run by
 * the same wavefront.  Results are identical to the two calls; the assembled arrays are still written. */
int osot_cycle(osot_solver* s, const osot_leaf_batch* leaf, const osot_assembled_out* out, const osot_qp_batch* batch,
               void* hip_stream);

/* average device time (ms) of the cascade kernel over the launches recorded since the last call
 * with reset != 0; measured with hipEvents on the launch stream. *launches receives the count. */
int osot_solver_kernel_time_ms(osot_solver* s, int reset, double* avg_ms, int* launches);
int osot_solver_set_timing(osot_solver* s, int enabled);   /* 0 off, 1 every launch, k > 1: every k-th launch (two event
                                                             * packets per timed launch sit in the stream's critical path) */
/* Dispatch order of the instances inside osot_ihqp_solve.  One wavefront solves one instance and the chip holds a
 * fixed number of them, so a batch runs in rounds and its tail is set by the slowest late starter.
 * OSOT_SCHEDULE_LONGEST_FIRST (default) dispatches in descending order of each instance's active-set iteration
 * count in the PREVIOUS solve of a batch of the same size on this solver (control loops are temporally coherent);
 * the first solve runs in order.  Results do not depend on the mode: the reference solves the robots of a batch
 * independently (one iHQP per robot, coman_ik.cpp:425-470). */
#define OSOT_SCHEDULE_IN_ORDER 0
#define OSOT_SCHEDULE_LONGEST_FIRST 1
int osot_solver_set_schedule(osot_solver* s, int mode);
/* Hot start of the working sets across control cycles (reference: QPOasesBackEnd.cpp:258-285 tries hotstart() first;
 * external/qpOASES-ext/src/SQProblem.cpp:149-193).  enabled != 0: every level of every instance records the inequality
 * working set it ends with, and the next osot_ihqp_solve / osot_cycle of THIS solver re-adds it before the first
 * violation scan (signed steps, then the constraints whose multipliers came out negative are taken out again); state is
 * per instance index, so instance i of consecutive batches should be the same robot.  Calling it (again) with
 * enabled != 0 forgets the recorded sets; 0 (default) = every solve is a cold start and nothing is recorded.  The answer
 * does not depend on the mode beyond round-off (each level's minimiser is unique); the iteration counts do: it pays
 * when the active sets persist from cycle to cycle and costs two iterations per constraint that has left the set.
 * The wavefront route only: a wide handle refuses enabled != 0 and hot-starts through osot_ihqp_solve_hot / osot_cycle_hot. */
int osot_solver_set_hotstart(osot_solver* s, int enabled);
/* Kernel instantiation by plan structure.  enabled != 0 (default): a plan WITHOUT constraint rows (the bounds l <= x <= u are
 * its only inequalities: a velocity stack with joint / velocity limits, BASELINE configs 2 and 3) of at most 32 variables runs
 * the instantiation of the cascade that carries no constraint-row code (row classification, row scans, row normals) -- and so
 * does, at every size up to 64 variables, a plan whose constraint rows are all TaskToConstraint blocks with a point band
 * (OSOT_ROWS_TASK_* with err_lb == err_ub: `stack << l_sole`, the feet of the reference's COMAN stacks,
 * examples/cpp/coman_ik.cpp:425-449): those rows are equalities of every level, the bounds stay the only inequalities;
 * 0: every plan runs the general instantiation.  The two are the same arithmetic in the same order: results are bit-identical
 * (tests/test_gpu_cascade.py), only the speed differs.  (The reference has nothing to mirror here: it is how one BackEnd
 * covers plans of different shape without paying for the features a plan does not use.) */
int osot_solver_set_specialisation(osot_solver* s, int enabled);
/* instances the device works on at once for this solver's plan (one wavefront each: CUs x resident wavefronts per CU, from
 * the kernel's register and LDS footprint): the dispatch order is planned for it, and batches that are a multiple of it
 * waste no round */
int osot_solver_resident_waves(osot_solver* s, int* waves);
/* Task::setActive (include/OpenSoT/Task.h:232-239, 375-400): an inactive task's A is zero -- it adds nothing to H and g
 * of its level and its optimality rows are void for the levels below.  The producer's Jacobian rows stay untouched in
 * A_k; the cascade ignores them.  Takes effect at the next osot_ihqp_solve / osot_cycle / osot_ehqp_solve (the equality-only
 * front-end gives the task's rows weight zero, i.e. treats the task as absent; a task beyond row 64 of its level is refused
 * there).  osot_nhqp_solve does not take inactive tasks.  (Column masks, Task::setActiveJointsMask, are the producer's:
 * osot_kin_desc.frame_col_mask.) */
int osot_solver_set_task_active(osot_solver* s, int level, int task, int active);
/* diagnostic: run the cascade once through the instrumented instantiation of the kernel and write, per
 * instance, OSOT_N_PHASES shader-clock cycle counts (H/g build, Cholesky, L^-1, substitution, equality
 * phase, inequality loop, optimality rhs, total, then four sub-phases of the equality adds: J'a,
 * reductions, step direction, Householder update; and six of the inequality loop: violation scan, d = J'n,
 * step direction z, dual direction r + step lengths, Householder add, drop) to cycles[B][OSOT_N_PHASES]
 * (device, int64). */
#define OSOT_N_PHASES 18
int osot_solver_profile_phases(osot_solver* s, const osot_qp_batch* batch, long long* cycles, void* hip_stream);

/* ---- the null-space front-end: OpenSoT::solvers::nHQP (src/solvers/nHQP.cpp:155-204, 236-317, 357-390) ----
 * Same stack, same assembled arrays as osot_ihqp_solve; per level the task is projected into the cumulated null space N of
 * the levels above, an SVD of A N drives the reference's A/b regularisation and yields the level's null space, the QP is
 * solved in the nf free coordinates (bounds become rows N z, compute_contraints :282-317) and q += N z, N <- N V2.  Three
 * launches per level (prepare, the batched QP kernel, accumulate).  n <= 64 (a level with min(rows, free variables) <= 32 goes
 * through a 32-wide eigen-decomposition; round 5: the others -- the reference's one-level stack S1, 50 rows in 35 variables --
 * through tridiagonalisation + QL on the full column-side Gram matrix), <= 64 rows per level, inactive tasks as zero rows and non-diagonal weights through level_W
 * (round 5), global rows and the box only (the reference refuses task-local constraints, nHQP.cpp:41-44). */
typedef struct {
    int free_vars[OSOT_MAX_LEVELS];      /* free variables of each level.  The reference fixes them in its constructor from the
                                            singular values of A N at construction (>= 1e-6 counts as rank, nHQP.cpp:88-103)
                                            and never changes them; 0 = default: n, then previous minus the rows of the level
                                            above (full row rank) */
    double min_sv_ratio;                 /* setMinSingularValueRatio (nHQP.cpp:342-355 accepts 0 <= s <= 1; 0 lifts nothing).
                                            A positive value is honoured as it is; 0 means DEFAULT_MIN_SV_RATIO = 0.05
                                            (nHQP.h:66), so that a zeroed struct is "the reference's defaults", UNLESS
                                            min_sv_ratio_is_set != 0, which makes 0 itself the value */
    int no_ab_regularization;            /* setPerformAbRegularization(false) */
    int no_selective_ns_regularization;  /* setPerformSelectiveNullSpaceRegularization(false) */
    int min_sv_ratio_is_set;             /* != 0: min_sv_ratio is the caller's value, 0 included (only needed to say 0) */
    /* per level (round 5; nHQP::setPerformAbRegularization(level, .), setPerformSelectiveNullSpaceRegularization(level, .),
       setMinSingularValueRatio(std::vector<double>): nHQP.cpp:127-152, 206-221).  A level's switch is OFF if the solver-wide one
       or its own says so; a level's ratio, where level_min_sv_ratio_is_set[k] != 0, replaces the solver-wide one. */
    int level_no_ab_regularization[OSOT_MAX_LEVELS];
    int level_no_selective_ns_regularization[OSOT_MAX_LEVELS];
    int level_min_sv_ratio_is_set[OSOT_MAX_LEVELS];
    double level_min_sv_ratio[OSOT_MAX_LEVELS];
    /* a level whose task(s) carry a NON-DIAGONAL weight (osot_task_desc.dense_weight; Task::setWeight(W)): the level's full weight
       matrix [B][m_k][m_k] (device; Task::getWeight() of the level: block diagonal over its tasks, symmetric), which nHQP.cpp:381-382
       multiplies the REGULARISED A N and b0 by -- so W A / W b (osot_qp_batch.WA / Wb, what iHQP and eHQP take) do not suffice.  NULL
       for a level with diagonal weights; a dense_weight level without it is refused. */
    const double* level_W[OSOT_MAX_LEVELS];
} osot_nhqp_options;
int osot_nhqp_solve(osot_solver* s, const osot_qp_batch* batch, const osot_nhqp_options* options, void* hip_stream);
/* instances the device works on at once in the null-space front-end's level preparation (the kernels a solve's time goes to; the
 * level with the fewest resident wavefronts counts): what a sub-batch size is chosen against, like osot_solver_resident_waves for
 * the cascade (opensot_amd/parallel.py: suggest_lanes).  opt: as for osot_nhqp_solve (its free_vars decide which kernel a level takes). */
int osot_solver_resident_waves_nhqp(osot_solver* s, const osot_nhqp_options* opt, int* waves);

/* ---- the equality-only front-end: OpenSoT::solvers::eHQP (src/solvers/eHQP.cpp:64-95, 124-146) -----------
 * Same stack, same assembled arrays (A_k, b_k, w_k or WA_k / Wb_k) as osot_ihqp_solve; the constraints and bounds of the
 * stack are NOT used (the reference's eHQP does not use them either: eHQP.cpp:45-47) and there is no active set: per level
 * JP = L'A P (W = L L'), x += JP^+ (L'b - L'A x) with the reference's damped pseudo-inverse, P <- P - V V' (thin right
 * singular vectors).  One launch for all levels.  sigma_min <= 0 = the reference's default 1e-12 (eHQP.cpp:56).
 * n <= 32; no regularisation task (the reference's eHQP has none); status is OSOT_STATUS_SOLVED for every instance
 * (eHQP::solve returns true). */
int osot_ehqp_solve(osot_solver* s, const osot_qp_batch* batch, double sigma_min, void* hip_stream);

/* ---- batch-of-one BackEnd surface (host pointers; mirrors BackEnd.h) ------------------------ */
typedef struct osot_backend osot_backend;
/* create_instance(number_of_variables, number_of_constraints, hessian_type, eps_regularisation)
 * (QPOasesBackEnd.cpp:14-24). eps_regularisation is the FACTOR; absolute eps = 2.221e-13 * factor.
 * number_of_variables <= OSOT_MAX_QP_VARS (128; see osot_qp_solve_batch for the path beyond 64). */
int osot_backend_create(int number_of_variables, int number_of_constraints, int hessian_type,
                        double eps_regularisation, osot_backend** out);
int osot_backend_destroy(osot_backend* be);
/* matrices row-major; A is nc x nv; l/u may be NULL (no box) */
int osot_backend_init_problem(osot_backend* be, const double* H, const double* g, const double* A,
                              const double* lA, const double* uA, const double* l, const double* u);
int osot_backend_update_task(osot_backend* be, const double* H, const double* g);
int osot_backend_update_constraints(osot_backend* be, const double* A, const double* lA,
                                    const double* uA, int number_of_constraints);
int osot_backend_update_bounds(osot_backend* be, const double* l, const double* u);
int osot_backend_solve(osot_backend* be);
int osot_backend_get_solution(osot_backend* be, double* x);
int osot_backend_get_objective(osot_backend* be, double* f);
/* BackEnd::getOptions / setOptions (include/OpenSoT/solvers/BackEnd.h:139-145; the qpOASES back-end hands out its
 * qpOASES::Options through boost::any, QPOasesBackEnd.cpp:309-318).  What this back-end has to set is the iteration cap of
 * the active-set loop (the counterpart of nWSR, QPOasesBackEnd.cpp:30: 0 = default 20 (n + nc) + 100); get also reports
 * the iteration count and OSOT_STATUS_* of the last solve.  INTEGRATION.md: the adapter carries this struct in the
 * boost::any. */
typedef struct { int max_iterations; int last_iterations; int last_status; } osot_backend_options;
int osot_backend_get_options(osot_backend* be, osot_backend_options* opt);
int osot_backend_set_options(osot_backend* be, const osot_backend_options* opt);
int osot_backend_set_eps_regularisation(osot_backend* be, double eps_abs);
int osot_backend_get_eps_regularisation(osot_backend* be, double* eps_abs);
int osot_backend_get_num_variables(osot_backend* be, int* nv);
int osot_backend_get_num_constraints(osot_backend* be, int* nc);

/* batched generic QP: B independent problems of the SAME shape in BackEnd convention, device
 * pointers, one wavefront each.  H: [B][n][n], g: [B][n], A: [B][nc][n], ...; x out [B][n].
 * n <= OSOT_MAX_QP_VARS (128).  Problems of 65 .. 128 variables -- wider than a wavefront: include/OpenSoT/Task.h:47-565 has no limit, a
 * 45-DoF robot or a floating-base inverse-dynamics stack with five contacts is such a problem -- run one 256-thread WORKGROUP per QP
 * (opensot_amd/csrc/osot_qp_big.h: the same dual active-set method; J in a stream-ordered device workspace of 2 n^2 doubles per
 * resident QP, R and the vectors in LDS; nc <= 2048).  Through this entry that path starts cold on every call (so does
 * osot_backend_solve: the plugin's hot-start record is for n <= 64; osot_qp_solve_batch_hot carries working sets at every size) and
 * allocates with hipMallocAsync on the caller's stream: do not capture it into a HIP graph. */
int osot_qp_solve_batch(int B, int n, int nc, const double* H, const double* g, const double* A,
                        const double* lA, const double* uA, const double* l, const double* u,
                        double eps_abs, int max_iter, double* x, int* status, int* iterations,
                        void* hip_stream);

/* HOT START for the call above: the working sets carried from call to call, as the reference's qpOASES back-end hot-starts every
 * solve from the previous one's (QPOasesBackEnd.cpp:258-285 -> SQProblem.cpp:149-193).  The state is a device array owned by the
 * caller, hot_state [B][ints] with ints from osot_qp_hot_state_ints(n) (32 for n <= 32, 64 for n <= 64, 128 for n <= 128;
 * OSOT_ERR_INVALID outside 1 .. OSOT_MAX_QP_VARS or with a null out pointer; host only, no GPU needed).  Row i belongs to INSTANCE i
 * of the call.  The kernel reads it before the solve and rewrites it after.  Entry -1 means "none": a state filled with 0xff bytes
 * (hipMemset) is a cold start: the same iterations as osot_qp_solve_batch (above 64 variables the same bits: the hot kernel runs the
 * cold kernel's instructions until it finds an entry).  Every other value is an opaque constraint code
 * of THIS library for THIS shape (n, nc): reset the state to 0xff when n or nc changes, and do not carry it to another version of the
 * library.  Whatever the state holds, the answer is the cold one up to round-off (the minimiser is unique; entries that name no
 * constraint of the problem, a constraint already in the set, an equality row, a side without a finite bound or a dependent normal
 * are skipped, stale ones are taken out again): what changes is the iteration count.
 * What a call leaves behind: an instance that ends OSOT_STATUS_SOLVED leaves the inequality part of its final working set compacted
 * to the front and -1 behind.  n > 64: an instance that does not end SOLVED leaves all -1.  n <= 64: an instance that fails in the
 * inequality loop (INFEASIBLE, MAX_ITER) leaves all -1; one that is refused before it (NOT_PD, or an inconsistent dependent equality
 * row: INFEASIBLE from the equality phase) leaves its row as it was -- harmless, see above.
 * hot_state == NULL is exactly osot_qp_solve_batch.  Same argument checks, same workspace rule above 64 variables (hipMallocAsync on
 * the caller's stream: not for HIP graph capture). */
int osot_qp_hot_state_ints(int n, int* ints);
int osot_qp_solve_batch_hot(int B, int n, int nc, const double* H, const double* g, const double* A,
                            const double* lA, const double* uA, const double* l, const double* u,
                            double eps_abs, int max_iter, double* x, int* status, int* iterations,
                            int* hot_state, void* hip_stream);

/* The same call through the SECOND back-end: an OSQP-convention ADMM solver -- the problem as
 * src/solvers/OSQPBackEnd.cpp poses it (P = H + eps I, one constraint matrix [A; I] with piled bounds, eps_abs = eps_rel =
 * 1e-5, sigma = 1e-6, alpha = 1.6, rho = 0.1 adaptive, 4000 iterations, "solved inaccurate" counts as solved: :25-49,
 * 198-226); osqp itself is not vendored in the reference, so this restates the published algorithm (parity vs osqp
 * unpinned) and is cross-checked against the active-set kernel.  eps_reg is the ABSOLUTE epsilon (the factory's factor
 * times 2.22e-13, OSQPBackEnd.cpp:8, 29).  max_iter 0 = 4000. */
int osot_qp_solve_batch_admm(int B, int n, int nc, const double* H, const double* g, const double* A,
                             const double* lA, const double* uA, const double* l, const double* u,
                             double eps_reg, int max_iter, double* x, int* status, int* iterations, void* hip_stream);

/* The same with osqp's settings exposed and WARM START: OSQPBackEnd keeps its osqp workspace between control cycles
 * (src/solvers/OSQPBackEnd.cpp:120-143 updates P, q, A and the bounds in place; :268-287), so every solve after the first
 * starts from the previous x and y with the rho the previous solve ended on (osqp's warm_start = 1).  Here the per-instance
 * state is three device arrays owned by the caller: warm_x [B][n], warm_y [B][nc + n] (the rows of A, then the box rows;
 * [B][nc] without l / u), warm_rho [B]; set warm_rho to 0 for "no state yet" (e.g. hipMemset the arrays once) -- an instance
 * whose solve fails is reset to that.  All three null = cold start.  opt null = the defaults below. */
typedef struct osot_admm_options {
    double eps_abs, eps_rel;     /* 0 = 1e-5 each (OSQPBackEnd.cpp:38-39) */
    double rho, sigma, alpha;    /* 0 = osqp's 0.1, 1e-6, 1.6 */
    int max_iter;                /* 0 = 4000 */
    int scaling;                 /* Ruiz equilibration passes: 0 = osqp's 10, negative = none */
    int check_every;             /* residual test period, 0 = 25 */
} osot_admm_options;
int osot_qp_solve_batch_admm_warm(int B, int n, int nc, const double* H, const double* g, const double* A,
                                  const double* lA, const double* uA, const double* l, const double* u,
                                  double eps_reg, const osot_admm_options* opt,
                                  double* warm_x, double* warm_y, double* warm_rho,
                                  double* x, int* status, int* iterations, void* hip_stream);

/* ---- batched kinematics producer ------------------------------------------------------
 * What the leaf tasks ask XBot::ModelInterface for every cycle: frame poses and 6 x n frame Jacobians
 * (velocity::Cartesian::_update, src/tasks/velocity/Cartesian.cpp:73-81: getJacobian / getPose), the centre
 * of mass and its 3 x n Jacobian (velocity::CoM::_update, src/tasks/velocity/CoM.cpp:59-74: getCOM /
 * getCOMJacobian).  xbot2_interface is not vendored in the reference, so this is an own implementation for a
 * kinematic TREE of revolute / prismatic joints (a floating base is the usual chain of three prismatic and three
 * revolute virtual joints); parity at this boundary is pinned by the CPU restatement in oracle/pykin.py and by
 * finite differences, not by the reference.  Convention: Jacobians are expressed in the world
 * frame (or the frame's base link frame: frame_base below), rows [linear; angular] of the frame origin, columns = joints; poses are [R row-major | p] (the Cartesian
 * leaf layout, osot_leaf_ptrs).  The Jacobians are written STRAIGHT into their row range of the stacked A_k. */
#define OSOT_KIN_MAX_JOINTS 64
#define OSOT_KIN_MAX_FRAMES 8
#define OSOT_KIN_MAX_PAIRS 32
#define OSOT_KIN_MAX_POINTS 16
#define OSOT_KIN_MAX_HULL_VERTICES 256
#define OSOT_KIN_MAX_HULL 32                 /* vertices of ONE hull */
#define OSOT_KIN_MAX_ROWSETS 8
enum { OSOT_JOINT_REVOLUTE = 0, OSOT_JOINT_PRISMATIC = 1 };
typedef struct {
    int n;                                   /* joints = generalised coordinates; tree order: parent[j] < j     */
    int parent[OSOT_KIN_MAX_JOINTS];         /* -1 = world                                                      */
    int type[OSOT_KIN_MAX_JOINTS];
    double axis[OSOT_KIN_MAX_JOINTS][3];     /* joint axis in the joint frame (unit)                            */
    double R0[OSOT_KIN_MAX_JOINTS][9];       /* fixed transform parent joint frame -> joint frame at q = 0      */
    double p0[OSOT_KIN_MAX_JOINTS][3];
    double mass[OSOT_KIN_MAX_JOINTS];        /* of the link the joint moves                                     */
    double com[OSOT_KIN_MAX_JOINTS][3];      /* its centre of mass in the joint frame                           */
    int n_frames;
    int frame_joint[OSOT_KIN_MAX_FRAMES];    /* joint whose link carries frame f                                */
    double frame_R[OSOT_KIN_MAX_FRAMES][9];  /* frame f in that joint frame                                     */
    double frame_p[OSOT_KIN_MAX_FRAMES][3];
    /* self-collision pairs: what velocity::CollisionAvoidance::update asks the (un-vendored) xbot2
     * collision module for every cycle, computeDistance / getDistanceJacobian
     * (src/constraints/velocity/CollisionAvoidance.cpp:96-118).  Each pair is two CAPSULES (segment + radius; a
     * segment of zero length is a sphere), each rigidly attached to a link.  Output per pair: the distance d between
     * the two surfaces and the row J_d with delta d = J_d dq, in the layout the OSOT_ROWS_COLLISION leaf expects. */
    int n_pairs;
    int pair_joint[OSOT_KIN_MAX_PAIRS][2];       /* joints whose links carry the two shapes                      */
    double pair_seg[OSOT_KIN_MAX_PAIRS][2][6];   /* capsule axis end points (a0, a1) in that joint's frame       */
    double pair_radius[OSOT_KIN_MAX_PAIRS][2];
    /* per-frame options of the Jacobian the producer writes (what Task::update applies after _update(), Task.h:375-400,
     * and Cartesian's own frame choice, Cartesian.cpp:73-100) */
    int frame_body[OSOT_KIN_MAX_FRAMES];         /* 1: BODY Jacobian Ad(R_f') J (Cartesian::setIsBodyJacobian,
                                                    Cartesian.cpp:93-100; pair with osot_task_desc.body_frame)       */
    unsigned long long frame_col_mask[OSOT_KIN_MAX_FRAMES]; /* Task::setActiveJointsMask (Task.h:129-139): bit j CLEAR =
                                                    column j of the frame's Jacobian is written as zero; 0 = no mask  */
    unsigned long long com_col_mask;             /* the same for the CoM Jacobian                                    */
    /* ---- environment shapes and boxes (reference: CollisionAvoidance::addCollisionShape /
     * moveCollisionShape / setLinksVsEnvironment, include/OpenSoT/constraints/velocity/CollisionAvoidance.h:115-144,
     * src/constraints/velocity/CollisionAvoidance.cpp:166-200; the shapes are XBot::Collision::Shape's sphere / capsule /
     * box).  Side a of a pair is a capsule (or sphere) on a link, as before.  Side b may be
     *   - carried by the WORLD: pair_joint[p][1] = -1 (a static world shape: its data are in world coordinates), and, with
     *     pair_env[p] = e + 1 > 0, placed by the RUNTIME pose osot_kin_batch.env_pose[e] (moveCollisionShape: the shape's
     *     data are then in the shape's own frame);
     *   - a BOX (pair_kind[p] = OSOT_SHAPE_BOX): half extents pair_box[p], box frame = carrier frame (link, world or
     *     env pose) composed with (pair_shape_R[p], pair_shape_p[p]) = link_T_shape; pair_seg[p][1] is unused and
     *     pair_radius[p][1] is a rounding radius (0 for a sharp box).
     * Distance = exact closest points of side a's axis segment and the box (piecewise-quadratic minimisation over the
     * segment parameter); a segment that touches or enters the box has no normal: distance -r_a - r_b, zero row (the
     * reference caps the bound at 0 there, CollisionAvoidance.cpp:141-146).  Box against box and every other pair of convex
     * shapes: the CONVEX SHAPES block below.
     * All zero (the value of a struct written before these fields existed) = capsule pairs on links only. */
    int pair_kind[OSOT_KIN_MAX_PAIRS];
    int pair_env[OSOT_KIN_MAX_PAIRS];
    double pair_box[OSOT_KIN_MAX_PAIRS][3];
    double pair_shape_R[OSOT_KIN_MAX_PAIRS][9];
    double pair_shape_p[OSOT_KIN_MAX_PAIRS][3];
    int n_env;                                   /* environment shapes with a runtime pose (env_pose entries)        */
    /* RELATIVE BASE LINK of a frame (round 6; velocity::Cartesian with base_link != "world", src/tasks/velocity/Cartesian.cpp:73-81:
     * getRelativeJacobian(distal, base, A) / getPose(distal, base, T); DefaultHumanoidStack's waist2LeftArm / waist2RightArm /
     * right2LeftLeg, tests/DefaultHumanoidStack.cpp:24-35, 52).  frame_base[f] = 0: the world (as before); g + 1 > 0: frame g
     * of this description is the base link frame (g != f; it may be a frame without outputs).  The producer then writes
     *   pose  = base_T_distal = [R_b'R_d | R_b'(p_d - p_b)],
     *   J     = R_b' (J_d - J_b shifted to the distal origin): column j = (anc_d(j) - anc_b(j)) [z_j x (p_d - p_j); z_j] rotated by
     *           R_b' (prismatic: [z_j; 0]) -- the twist of the distal frame relative to the base frame, in base coordinates; the
     *           joints both chains share drop out exactly, the joints of the base's own chain enter with a minus sign.
     * With frame_body[f] the rotation is R_d' instead (Ad(bR_d') after the R_b' of the relative Jacobian, Cartesian.cpp:93-100). */
    int frame_base[OSOT_KIN_MAX_FRAMES];
    /* CONVEX SHAPES on both sides of a pair (what CollisionAvoidance.cpp:96-200 takes from the URDF: boxes, cylinders, spheres
     * and meshes).  A shape is a convex CORE grown by the rounding radius pair_radius[p][side] >= 0:
     *   OSOT_SHAPE_CAPSULE  the segment pair_seg[p][side] (carrier frame); zero length = a sphere
     *   OSOT_SHAPE_BOX      size = half extents
     *   OSOT_SHAPE_CYLINDER size = (radius, unused, half length), axis = z of the shape frame
     *   OSOT_SHAPE_HULL     the convex hull of 1 .. 32 vertices hull_vertex[first .. first + count - 1] (shape frame): a convex
     *                       mesh.  Non-convex meshes are not offered.
     * SIDE A: pair_kind_a[p] (0 = the capsule of pair_seg[p][0], as before), pair_size_a, and link_T_shape =
     * (pair_shape_R_a[p], pair_shape_p_a[p]) in the frame of pair_joint[p][0]'s link.  SIDE B keeps pair_kind / pair_box (its size) /
     * pair_shape_R / pair_shape_p and its carriers (link, world, environment pose).  pair_hull[p][side] = {first vertex, count}.
     * A pair of capsule / capsule or capsule / box keeps its closed form, bit for bit.  Every other pair runs GJK on the two cores
     * in double precision (opensot_amd/csrc/osot_convex.h): distance = |ca - cb| - r_a - r_b with the witnesses ca, cb on the
     * cores; intersecting cores have no normal: distance -r_a - r_b, zero row, as for the segment inside a box above.  Such a
     * model is served by osot_kinematics; osot_control_cycle / osot_control_rollout refuse it when pair outputs are bound.
     * All zero = no convex pair.  (The block sits in front of the contact points, which stay the struct's last members.) */
    int pair_kind_a[OSOT_KIN_MAX_PAIRS];
    double pair_size_a[OSOT_KIN_MAX_PAIRS][3];
    double pair_shape_R_a[OSOT_KIN_MAX_PAIRS][9];
    double pair_shape_p_a[OSOT_KIN_MAX_PAIRS][3];
    int pair_hull[OSOT_KIN_MAX_PAIRS][2][2];
    int n_hull_vertices;                         /* 0 .. OSOT_KIN_MAX_HULL_VERTICES                                   */
    double hull_vertex[OSOT_KIN_MAX_HULL_VERTICES][3];
    /* ROW SETS (velocity::Contact, velocity::PureRolling / PureRollingPosition / PureRollingOrientation, floating_base::Contact,
     * constraints::velocity::OmniWheels4X): up to 6 rows derived from ONE frame, "a small pose-dependent matrix times the frame's
     * Jacobian", written per instance straight into a level's A_k or a row block's C (osot_kin_batch.rowset_A), as frame_J is.
     * rowset_row_mask: bit r set = row r of the kind is written; the rows are written COMPACTLY, in order (PureRollingPosition =
     * rows {0, 1[, 2]}, PureRollingOrientation = row {3} of OSOT_ROWSET_PURE_ROLLING, PureRolling.cpp:89-150).  All of them use the
     * frame's WORLD pose and world Jacobian [linear; angular], whatever frame_body / frame_col_mask say; a frame with
     * frame_base != 0 is refused.
     *   OSOT_ROWSET_CONTACT (src/tasks/velocity/Contact.cpp:19-33): A = K Ad(R_f') J_f, both 3-row blocks of J_f rotated by R_f'
     *     (XBot::Utils::rotate); K = rowset_param[0 .. 35], 6 x 6 row-major, row r of it is row r of the kind.  b = 0 is the
     *     caller's: the block is an OSOT_TASK_GENERIC.
     *     rowset_split = 1 (src/tasks/floating_base/Contact.cpp:47-67 with lambda = 0, the reference's default): the rows are
     *     written with SIX columns, A = (K Ad(R_f') J_f)[:, 0:6], for a 6-variable plan, and osot_kin_batch.rowset_b receives
     *     b = -(K Ad(R_f') J_f)[:, 6:] qdot[6:].  The lambda * error term of that task is NOT produced.  Needs n > 6.
     *   OSOT_ROWSET_PURE_ROLLING (src/tasks/velocity/PureRolling.cpp:50-77): 4 rows.  rowset_param = {radius r, outward normal
     *     n[3] (unit, world), S33[9] row-major}.  d = -r n; Jc = [J_lin + J_ang x d; J_ang], the Jacobian of the contact point
     *     p_f - r n; a = (R_f e_z) x n, normalised (the wheel spins about its local z); A = S Jc with S = [S33 0; 0 0 0 a'].
     *     S33 comes from osot_pure_rolling_s33 below.  NO GUARD for a wheel axis parallel to n: a is 0 / 0 there, as in the
     *     reference (PureRolling.cpp:64-65).
     *   OSOT_ROWSET_OMNI4X (src/constraints/velocity/OmniWheels4X.cpp:22-74): 3 rows.  rowset_param = {l1, l2, r}; rowset_wheel =
     *     the coordinates of the front-left, front-right, hind-left, hind-right wheel joints (each 6 .. n - 1); rowset_frame = the
     *     base link frame.  Columns 0 .. 5 are the constant selection (0,0) = (1,1) = (2,5) = 1; columns >= 6 are
     *     R_base (r / 4) v_j with v_j = 0 except fl: -(1, -1, -1/(l1+l2)), fr: -(1, 1, 1/(l1+l2)), hl: -(1, 1, -1/(l1+l2)),
     *     hr: -(1, -1, 1/(l1+l2)).  The caller puts the rows in an OSOT_ROWS_GENERIC block with lo = up = 0.
     * GAZE REFERENCES (src/tasks/velocity/Gaze.cpp:52-74, src/utils/cartesian_utils.cpp:27-35): per gaze g, with [R | p] the pose
     * frame gaze_frame[g] publishes (world, or relative to its frame_base) and the point osot_kin_batch.gaze_point[g]:
     * t = R'(point - p); where |t| >= 0.2 (GAZE_THRESHOLD) osot_kin_batch.gaze_ref[g] is overwritten with [RotZ(pan) RotY(-tilt) | 0],
     * pan = atan2(t_y, t_x), tilt = atan2(t_z, sqrt(t_y^2 + t_x^2)) (_bl_T_gaze_kdl is never set in the reference: the identity);
     * where |t| < 0.2 the buffer is left untouched, bit for bit: it is the previous reference.  The task itself is an
     * OSOT_TASK_CARTESIAN with the SubTask row mask {4, 5} reading gaze_ref as its reference pose.
     * A model with row sets or gaze references is served by osot_kinematics; osot_control_cycle / osot_control_rollout refuse it,
     * and so does osot_kinematics when convex (GJK) pair outputs are bound in the same call (OSOT_ERR_UNSUPPORTED).
     * All zero = none.  (Like the convex block, this one sits in front of the contact points, which stay the struct's last members.) */
    int n_rowsets;                               /* 0 .. OSOT_KIN_MAX_ROWSETS                                         */
    int rowset_kind[OSOT_KIN_MAX_ROWSETS];       /* OSOT_ROWSET_*                                                     */
    int rowset_frame[OSOT_KIN_MAX_ROWSETS];      /* 0 .. n_frames - 1                                                 */
    int rowset_row_mask[OSOT_KIN_MAX_ROWSETS];   /* rows of the kind (6 / 4 / 3) that are written; not empty          */
    int rowset_split[OSOT_KIN_MAX_ROWSETS];      /* OSOT_ROWSET_CONTACT only                                          */
    int rowset_wheel[OSOT_KIN_MAX_ROWSETS][4];   /* OSOT_ROWSET_OMNI4X only                                           */
    double rowset_param[OSOT_KIN_MAX_ROWSETS][36];
    int n_gaze;                                  /* 0 .. OSOT_KIN_MAX_FRAMES                                          */
    int gaze_frame[OSOT_KIN_MAX_FRAMES];         /* 0 .. n_frames - 1                                                 */
    /* CONTACT POINTS (velocity::ConvexHull: convex_hull::getSupportPolygonPoints asks the model for getPose(link).translation() of
     * every link in contact, src/utils/convex_hull_utils.cpp:142-174): point i is fixed at point_p[i] in the frame of joint
     * point_joint[i]'s link; the producer writes its world position to osot_kin_batch.points.  All zero = none. */
    int n_points;                                /* 0 .. OSOT_KIN_MAX_POINTS                                          */
    int point_joint[OSOT_KIN_MAX_POINTS];        /* 0 .. n - 1                                                        */
    double point_p[OSOT_KIN_MAX_POINTS][3];
} osot_kin_desc;
enum { OSOT_ROWSET_CONTACT = 1, OSOT_ROWSET_PURE_ROLLING = 2, OSOT_ROWSET_OMNI4X = 3 };
enum { OSOT_SHAPE_CAPSULE = 0, OSOT_SHAPE_BOX = 1, OSOT_SHAPE_CYLINDER = 2, OSOT_SHAPE_HULL = 3 };
#define OSOT_KIN_MAX_ENV 16
typedef struct {
    int B;
    const double* q;                               /* [B][n]                                                    */
    double* frame_pose[OSOT_KIN_MAX_FRAMES];       /* [B][12] or NULL                                           */
    double* frame_J[OSOT_KIN_MAX_FRAMES];          /* first of the 6 rows of frame f in instance 0, or NULL     */
    long long frame_J_stride[OSOT_KIN_MAX_FRAMES]; /* doubles from one instance to the next (ma_k * n)          */
    double* com;                                   /* [B][3] or NULL                                            */
    double* com_J;                                 /* first of the 3 rows in instance 0, or NULL                */
    long long com_J_stride;
    double* pair_dist;                             /* [B][n_pairs] surface distances (negative: penetration), or NULL */
    double* pair_J;                                /* first of the n_pairs rows J_d in instance 0, or NULL (the
                                                      OSOT_ROWS_COLLISION leaf p0: [B][rows][n])                */
    long long pair_J_stride;                       /* doubles from one instance to the next (rows * n)          */
    const double* env_pose;                        /* [n_env][12] world_T_shape = [R row-major | p] of the environment
                                                      shapes (moveCollisionShape), or NULL when n_env = 0           */
    long long env_pose_stride;                     /* 0: one world shared by all instances; 12 n_env: per instance  */
    double* pair_points;                           /* [B][n_pairs][6] the witness points of every pair, ca then cb, in the
                                                      world and ON THE CORES (the capsule axis, the box, the hull: not the
                                                      rounded surface) -- what the reference's collision module returns next to
                                                      the distance; or NULL                                          */
    /* row sets (osot_kin_desc.n_rowsets): all NULL / 0 = none written.  (In front of `points`, which stays the last member.) */
    double* rowset_A[OSOT_KIN_MAX_ROWSETS];          /* first written row of set s in instance 0, or NULL; row length n (6 with
                                                        rowset_split)                                                 */
    long long rowset_A_stride[OSOT_KIN_MAX_ROWSETS]; /* doubles from one instance to the next                         */
    double* rowset_b[OSOT_KIN_MAX_ROWSETS];          /* rowset_split only: first entry of b in instance 0, or NULL    */
    long long rowset_b_stride[OSOT_KIN_MAX_ROWSETS];
    const double* rowset_qdot;                       /* [B][n] joint velocities: required where a rowset_b is bound   */
    const double* gaze_point[OSOT_KIN_MAX_FRAMES];   /* [B][3] the point gaze g looks at, in the coordinates of the pose */
    double* gaze_ref[OSOT_KIN_MAX_FRAMES];           /* [B][12] read-modify-write: the Cartesian leaf's reference pose  */
    double* points;                                /* [B][n_points][3] world positions of the contact points (the
                                                      OSOT_ROWS_CONVEX_HULL leaf p2), or NULL                        */
} osot_kin_batch;
typedef struct osot_kin osot_kin;
int osot_kin_create(const osot_kin_desc* desc, int device, osot_kin** out);
int osot_kin_destroy(osot_kin* k);
int osot_kinematics(osot_kin* k, const osot_kin_batch* batch, void* hip_stream);
/* The 3 x 3 block S33 of OSOT_ROWSET_PURE_ROLLING for the outward normal n (HOST only, no device): PureRolling::setOutwardNormal
 * (src/tasks/velocity/PureRolling.cpp:19-47) as it is written.  uz = n / |n|; ux = e1, then e2 where |uz . e2| < |uz . ux|, then e3
 * where |uz . e3| < |uz . ux| with the ux chosen so far (a SEQUENTIAL choice); uy = uz x ux (ux is not made orthogonal to uz, so uy
 * is not a unit vector in general).  _local_R_world has the ROWS ux, uy, uz and _update() applies its transpose: S33's COLUMNS are
 * ux, uy, uz.  s33 [9] row-major; normal_unit [3] (may be NULL) receives uz.  OSOT_ERR_INVALID: a null or zero normal. */
int osot_pure_rolling_s33(const double* normal, double* s33, double* normal_unit);
/* Distance of two convex shapes ON THE HOST (no device is touched): the code the producer's lanes run, for a setup-time check
 * ("do my shapes overlap at q0?").  size as in the CONVEX SHAPES block above; a capsule: size[2] = half length along z of the shape frame;
 * world_T_a / world_T_b: [R row-major | p], 12 doubles.  Always GJK, also for the pairs the producer has a closed form for.
 * dist = |ca - cb| - r_a - r_b; ca, cb [3] on the cores (equal when the cores intersect); iterations: support evaluations.
 * dist, ca, cb, iterations may each be NULL. */
typedef struct {
    int kind;                    /* OSOT_SHAPE_*                                                                       */
    double size[3];
    double radius;               /* rounding radius >= 0                                                               */
    int n_vertices;              /* OSOT_SHAPE_HULL: 1 .. OSOT_KIN_MAX_HULL                                             */
    const double* vertices;      /* [n_vertices][3] in the shape frame                                                 */
} osot_shape;
int osot_shape_distance(const osot_shape* a, const double* world_T_a, const osot_shape* b, const double* world_T_b, double* dist,
                        double* ca, double* cb, int* iterations);

/* The body of the reference's control loop for B robots in ONE launch (examples/cpp/coman_ik.cpp:186-219:
 * `model.update(); stack->update(); solver->solve(dq); q = model.sum(q, dq)`): per instance the same wavefront runs
 * osot_kinematics (q -> frame poses, Jacobian rows, CoM, written where `kin_batch` says: the arrays the leaf inputs and A_k
 * point into), then osot_cycle (AutoStack::update + the iHQP cascade), then, when q_integrate is not NULL,
 * q_integrate[i] += dq[i] (usually kin_batch->q itself: the next call starts from the integrated posture).
 * Results are those of the three calls; every array they write is still written.  Not offered with the collision-pair
 * stage, dense weights, inactive tasks or the hot start (OSOT_ERR_UNSUPPORTED -- use the three calls).  It pays where several
 * sub-batches share the chip (a sub-batch's kinematics launch otherwise waits for wavefront slots the other's cascade holds).
 * Stream-ordered. */
int osot_control_cycle(osot_solver* s, osot_kin* k, const osot_kin_batch* kin_batch, const osot_leaf_batch* leaf,
                       const osot_assembled_out* out, const osot_qp_batch* batch, double* q_integrate, void* hip_stream);
/* A ROLLOUT (round 5): `steps` control cycles of every robot in ONE launch -- the loop of the reference's example
 * (examples/cpp/coman_ik.cpp:174-219: for every iteration model.update(); stack->update(); solver->solve(dq); q = model.sum(q, dq))
 * run by the robot's own wavefront, cycle after cycle, with the leaf inputs (references, gains) held fixed over the rollout.  The
 * robots are independent, so the results are those of `steps` osot_control_cycle calls (tested bit-identical) -- without a launch
 * per step and without every robot waiting, at every step, for the slowest robot of the batch.  What MPC rollouts and sample-based
 * planners ask for: B candidate roll-outs advanced K control cycles each.
 * q_integrate (required for steps > 1) is advanced by every cycle's dq; dq / status of the batch hold the LAST cycle's dq and the
 * FIRST non-zero status of the rollout (a failed cycle leaves the robot where it is: dq = 0, coman_ik.cpp:189-190);
 * dq_steps [steps][B][n] and status_steps [steps][B] (either may be NULL) receive every cycle's.  Stream-ordered.
 * A plan with an OSOT_BOUND_JOINT_LIMITS_INVARIANCE bound is refused for steps > 1 (OSOT_ERR_UNSUPPORTED): its qdot_prev leaf is
 * a held-fixed leaf input like any other, and the bound is only right when it follows every cycle's dq. */
int osot_control_rollout(osot_solver* s, osot_kin* k, const osot_kin_batch* kin_batch, const osot_leaf_batch* leaf,
                         const osot_assembled_out* out, const osot_qp_batch* batch, double* q_integrate, int steps,
                         double* dq_steps, int* status_steps, void* hip_stream);

/* ---- inverse-dynamics formulation (BASELINE config 5): x = [qddot (nv); contact forces / wrenches] -------------
 * (src/utils/InverseDynamics.cpp:12-28).  The matrices that are pure copies of model quantities are written by these
 * producers straight into their row ranges of the stacked A_k / C (zero-copy, like the kinematics producer's Jacobians);
 * the model quantities themselves (inertia matrix B, non-linear term h, contact Jacobians) come from the caller's
 * dynamics library, as they come from XBot::ModelInterface in the reference -- or from osot_dynamics / osot_kinematics below,
 * which write them into these arrays on the device. */
#define OSOT_ID_MAX_FORCE_VARS 48   /* eight surface contacts */
typedef struct {
    int B, nv, n_contacts, contact_dim;   /* contact_dim: 3 = point contact (force), 6 = surface contact (wrench)
                                             (InverseDynamics.cpp:16-27); nv + n_contacts * contact_dim <=
                                             OSOT_MAX_QP_VARS (128: the wide route) and n_contacts * contact_dim <=
                                             OSOT_ID_MAX_FORCE_VARS                                                      */
    const double* Bm;                     /* [B][nv][nv] inertia matrix (symmetric)                                      */
    const double* h;                      /* [B][nv] non-linear term                                                     */
    const double* Jc;                     /* [B][n_contacts][contact_dim][nv] first contact_dim rows of each contact's
                                             Jacobian                                                                    */
    int floating_base;                    /* computedTorque checks the first six rows of tau (InverseDynamics.cpp:83-92)  */
} osot_id_model;
/* rows [B_u, -J_f'] of acceleration::DynamicFeasibility (DynamicFeasibility.cpp:22-46; 6 rows) and [B, -Jc'] of
 * TorqueLimits (TorqueLimits.cpp:25-46; nv rows): C_dyn / C_tau point at the block's first row in instance 0 (either may
 * be NULL), *_stride = doubles from one instance to the next (nc_stored * n).  Plus n_tasks task matrices [J_i 0]
 * (acceleration::Cartesian / CoM, Cartesian.cpp:152-160): J[i] is [B][J_rows[i]][nv], A_dst[i] the block's first row in
 * instance 0 of A_k, A_stride[i] = ma_k * n. */
int osot_id_rows(const osot_id_model* m, double* C_dyn, long long dyn_stride, double* C_tau, long long tau_stride,
                 int n_tasks, const double* const* J, const int* J_rows, double* const* A_dst, const long long* A_stride,
                 void* hip_stream);
/* GainType::Force of acceleration::Cartesian (src/tasks/acceleration/Cartesian.cpp:161-169, 517-524): per instance
 * Mi = J Bi J' (compute_cartesian_inertia_inverse: Bi = the model's inverse inertia matrix, [B][nv][nv]; J [B][rows][nv]),
 * then Gp = Mi Kp, Gd = Mi Kd written into the task's leaf array p0 behind its 2 rows errors (see
 * osot_task_desc.acc_gain_matrices: p0_gains points at instance 0's Gp, p0_stride = 2 rows + 2 rows^2 doubles), and
 * a_ref[B][rows] += Mi f for a virtual force f [B][rows] (NULL: none).  Kp, Kd: HOST pointers to rows x rows row-major
 * matrices (the task's settings).  rows <= 6, nv <= OSOT_MAX_QP_VARS. */
int osot_id_force_gains(int B, int nv, int rows, const double* J, const double* Bi, const double* Kp, const double* Kd,
                        const double* f_virtual, double* p0_gains, long long p0_stride, double* a_ref, void* hip_stream);
/* InverseDynamics::computedTorque (InverseDynamics.cpp:57-96): tau[B][nv] = B qddot + h - sum_c Jc' F_c from the solved
 * x[B][n]; ok[B] (may be NULL) = 0 where a floating-base row of tau exceeds fb_tol (the reference uses 10e-3 and
 * returns false). */
int osot_computed_torque(const osot_id_model* m, const double* x, double* tau, int* ok, double fb_tol, void* hip_stream);

/* ---- batched rigid-body dynamics producer ------------------------------------------------------------------------
 * What the inverse-dynamics leaves ask XBot::ModelInterface for every cycle: computeInertiaMatrix (DynamicFeasibility.cpp:24,
 * TorqueLimits.cpp:27, variables/Torque.cpp:32), computeNonlinearTerm (DynamicFeasibility.cpp:25, TorqueLimits.cpp:28,
 * Torque.cpp:52), getJdotTimesV (acceleration/Cartesian.cpp:137, Contact.cpp:10) and getCOMJdotTimesV (acceleration/CoM.cpp:80),
 * for the tree of an osot_kin_desc plus the rotational inertia of its links.  Like the kinematics producer it is an own
 * implementation (xbot2_interface is not vendored); parity is pinned by a numpy restatement by another algorithm, by identities
 * against osot_kinematics and by finite differences.  Conventions:
 *   M qddot + h = tau + sum_c Jc' F_c: h holds the Coriolis, centrifugal AND gravity terms (computeNonlinearTerm); M and h are in
 *   the tree's generalised coordinates, so with the usual floating-base chain their first six rows are the floating base's;
 *   frame_Jdot_qdot = [classical acceleration of the frame origin; angular acceleration] at qddot = 0, world frame, such that
 *   d/dt (J qdot) = J qddot + Jdot qdot with the world-frame J osot_kinematics writes; com_Jdot_qdot likewise for the CoM.
 * M is written from one computed value per unordered pair (exactly symmetric).
 * Centroidal momentum (what tasks::velocity::AngularMomentum / LinearMomentum, tasks::acceleration::AngularMomentum and
 * tasks::force::CoM ask computeCentroidalMomentumMatrix / computeCentroidalMomentum for):
 *   the 6 x n matrix is [linear (3 rows); angular (3 rows)] -- the reference reads block(0,0,3,n) as linear and block(3,0,3,n)
 *   as angular -- in the WORLD axes about the instance's CENTRE OF MASS; its columns are the tree's generalised coordinates
 *   (the floating base of this project is three prismatic and three revolute virtual joints); momentum = matrix * qdot.
 *   cmm_lin and cmm_ang are two pointers so that the three rows of an AngularMomentum task land in a level's A_k next to
 *   other blocks: exactly n doubles per row are written, columns n .. ld-1 and the gaps between rows and instances are left
 *   alone, so with ld = the plan's n the rows [A_ang 0] of an inverse-dynamics level go into a zero-initialised A_k.
 *   ang_mom_b is the b of acceleration::AngularMomentum (AngularMomentum.cpp:31-60) with CMMdot * v = 0 as in the reference.
 *   The reference's tasks zero their references after every update; here the caller owns and rewrites the reference arrays.
 *   Like every model quantity here, parity with xbot2 is unpinned (xbot2_interface is not vendored). */
typedef struct {
    double inertia[OSOT_KIN_MAX_JOINTS][6];  /* Ixx Ixy Ixz Iyy Iyz Izz of the link joint j moves, about ITS CENTRE OF MASS
                                                (osot_kin_desc.com[j]), axes of the joint frame; all zero = point mass       */
    double gravity[3];                       /* world frame, e.g. (0, 0, -9.81)                                             */
} osot_dyn_desc;
typedef struct {
    int B;
    const double* q;                         /* [B][n]                                                                      */
    const double* qdot;                      /* [B][n], NULL = zero (h is then the gravity term)                            */
    double* M;                               /* first element of instance 0, or NULL                                        */
    long long M_stride;                      /* doubles from one instance to the next (n * n when dense)                    */
    double* h;                               /* [B][n] or NULL                                                              */
    double* frame_Jdot_qdot[OSOT_KIN_MAX_FRAMES];          /* [linear; angular] of frame f in instance 0, or NULL           */
    long long frame_Jdot_qdot_stride[OSOT_KIN_MAX_FRAMES]; /* doubles from one instance to the next (6 when dense): lets it
                                                              land in a task's leaf array p1                                */
    double* com_Jdot_qdot;                   /* 3 doubles per instance, or NULL                                             */
    long long com_Jdot_qdot_stride;          /* (3 when dense)                                                              */
    /* -- centroidal momentum (computeCentroidalMomentumMatrix / computeCentroidalMomentum); zero / NULL everywhere = none -- */
    double* cmm_lin;                         /* first of the 3 LINEAR rows of the momentum matrix in instance 0, or NULL     */
    long long cmm_lin_stride;                /* doubles from one instance to the next (>= 3 * ld)                            */
    int cmm_lin_ld;                          /* row length in doubles, 0 = n; exactly n doubles of each row are written      */
    double* cmm_ang;                         /* the 3 ANGULAR rows, likewise: e.g. a Generic block's rows in a level's A_k   */
    long long cmm_ang_stride;
    int cmm_ang_ld;
    double* momentum;                        /* [linear (3); angular (3)] per instance, or NULL; zeros when qdot is NULL     */
    long long momentum_stride;               /* (6 when dense)                                                              */
    double* ang_mom_b;                       /* 3 doubles per instance, or NULL: Ldot_d + lambda K (L_d - L_angular)         */
    long long ang_mom_b_stride;              /* (3 when dense): lets it land in a task's leaf array p0                       */
    const double* ang_mom_ref;               /* L_d [B][3]; NULL = L_d is the actual momentum (b = Ldot_d)                   */
    const double* ang_mom_rate_ref;          /* Ldot_d [B][3]; NULL = zero                                                   */
    double ang_mom_gain[9];                  /* K, row-major; all nine zero = the identity                                   */
    double ang_mom_lambda;
} osot_dyn_batch;
typedef struct osot_dyn osot_dyn;
/* tree: what osot_kin_create takes (frames included; collision pairs are ignored).  Refused with OSOT_ERR_INVALID before any
 * device is touched: joints out of tree order or out of range, axes that are not unit vectors, NaNs, negative masses, an
 * inertia tensor that is not positive semi-definite or violates the triangle inequalities of its principal moments. */
int osot_dyn_create(const osot_kin_desc* tree, const osot_dyn_desc* inertia, int device, osot_dyn** out);
int osot_dyn_destroy(osot_dyn* d);
/* Stream-ordered, no allocation, capturable.  Jdot qdot of a frame with frame_base != 0 or frame_body != 0 is refused
 * (OSOT_ERR_UNSUPPORTED; the reference leaves the relative case open as well, acceleration/Cartesian.cpp:144).  Refused with
 * OSOT_ERR_INVALID before any device is touched: a cmm row length below n, a cmm stride below 3 * ld, momentum_stride < 6,
 * ang_mom_b_stride < 3, ang_mom_ref / ang_mom_rate_ref without ang_mom_b, a non-finite ang_mom_gain or ang_mom_lambda. */
int osot_dynamics(osot_dyn* d, const osot_dyn_batch* batch, void* hip_stream);

/* ---- batched posture-gradient producer ---------------------------------------------------------------------------
 * The b of tasks::velocity::Manipulability (Manipulability.cpp:58-84) and tasks::velocity::MinimumEffort (MinimumEffort.cpp:51-77)
 * for the tree of an osot_kin_desc.  Per term and ACTIVE joint i, in the reference's order:
 *     grad[i] = (f(q + step e_i) - f(q - step e_i)) / (2 step),   0 for a joint that is not active
 *     b = lambda grad (manipulability),   b = -1.0 lambda grad (minimum effort)
 *     manipulability: f = sqrt(fabs(det(J W J'))), J = the 6 x n Jacobian of a frame (world, or relative to its frame_base), or the
 *                     3 x n Jacobian of the centre of mass (Manipulability.h:130-150)
 *     minimum effort: f = tau_g' W tau_g, tau_g = the gravity compensation over all n coordinates (MinimumEffort.h:89-96)
 * q + delta is plain addition: the floating base of this project is three prismatic and three revolute virtual joints.
 *   - The worker builds a FRESH Cartesian task on its own model copy, so frame_col_mask of the osot_kin_desc is NOT applied to J.
 *   - frame_body and the R_b' rotation of a relative Jacobian are orthogonal block transforms of J: the determinant does not see
 *     them, and the kernel skips them.
 *   - tau_g = -M_tot J_com' g, which is what osot_dynamics writes as h when qdot is NULL.
 * W is the worker's CONSTANT weight (setW); only its diagonal is offered (a dense W is not).  The tasks themselves have A = I, W = I:
 * b goes into the leaf of an implicit OSOT_TASK_POSTURAL block (p1 = p0, p2 = b) or of an OSOT_TASK_GENERIC block with stored unit
 * rows, by its own launch in front of osot_cycle / osot_control_cycle. */
enum { OSOT_GRAD_MANIPULABILITY_FRAME = 0, OSOT_GRAD_MANIPULABILITY_COM = 1, OSOT_GRAD_MIN_EFFORT = 2 };
#define OSOT_GRAD_MAX_TERMS 4
typedef struct {
    int n_terms;                                           /* 1 .. OSOT_GRAD_MAX_TERMS                                          */
    int kind[OSOT_GRAD_MAX_TERMS];
    int frame[OSOT_GRAD_MAX_TERMS];                        /* MANIPULABILITY_FRAME: a frame of the tree; its frame_base is honoured */
    double step[OSOT_GRAD_MAX_TERMS];                      /* finite, > 0; the reference's default is 1e-3                      */
    double lambda[OSOT_GRAD_MAX_TERMS];
    unsigned long long joint_mask[OSOT_GRAD_MAX_TERMS];    /* Task::getActiveJointsMask: bit i CLEAR = grad[i] is 0; 0 = all active */
    double W_diag[OSOT_GRAD_MAX_TERMS][OSOT_KIN_MAX_JOINTS]; /* diagonal of the worker's weight, one entry per coordinate        */
    double gravity[3];                                     /* world frame, e.g. (0, 0, -9.81)                                   */
} osot_grad_desc;
typedef struct {
    int B;
    const double* q;                                       /* [B][n]                                                            */
    double* b[OSOT_GRAD_MAX_TERMS];                        /* first of the n entries of instance 0, or NULL (then stride 0)     */
    long long b_stride[OSOT_GRAD_MAX_TERMS];               /* doubles from one instance to the next (>= n)                      */
    double* value[OSOT_GRAD_MAX_TERMS];                    /* [B]: ComputeManipulabilityIndex() / computeEffort() at q, or NULL */
} osot_grad_batch;
typedef struct osot_grad osot_grad;
/* Refused with OSOT_ERR_INVALID before any device is touched: what osot_dyn_create refuses of a tree, n_terms outside 1 .. 4, an
 * unknown kind, a frame out of range, a step that is not finite or not > 0, a lambda, W_diag or gravity that is not finite. */
int osot_grad_create(const osot_kin_desc* tree, const osot_grad_desc* desc, int device, osot_grad** out);
int osot_grad_destroy(osot_grad* g);
/* Stream-ordered, no allocation, capturable.  OSOT_ERR_INVALID: B < 0, q NULL, a NULL b with a stride, a stride below n, an output
 * bound to a term beyond n_terms.  B == 0 is a no-op. */
int osot_posture_gradient(osot_grad* g, const osot_grad_batch* batch, void* hip_stream);

/* ---- force-space tasks: contact-wrench stacks ----------------------------------------------------------------------
 * x = [w_0 .. w_{C-1} (6 each: force, torque) | optionally tau (nv - 6)]; wrench c starts at wrench_col[c], the torques at
 * torque_col.  osot_force_rows turns the model quantities osot_kinematics / osot_dynamics leave on the device into the matrices
 * and vectors of the reference's force tasks, written into OSOT_TASK_GENERIC / OSOT_ROWS_GENERIC blocks (no plan kind is added):
 *   force::CoM (src/tasks/force/CoM.cpp:106-134, 176-207, 266-279), 6 rows:
 *       block c of A = [I 0; P_c I], P_c = skew(p_c - com), p_c = the origin of contact c's frame;
 *       b = [m (a_d + lambda2 (v_d - v) + lambda (p_d - com) - g); Ldot_d + lambda_ang (L_d - L)],
 *       v = momentum[0:3] / m, L = momentum[3:6], m = mass
 *   force::FloatingBase (FloatingBase.cpp:58-76), 6 rows: block c of A = (Jc_c[:, 0:6])'.  b is the caller's floating_base_torque,
 *       a plain leaf: nothing is computed for it
 *   constraints::force::StaticConstraint (StaticConstraint.cpp:17-34), nv - 6 equality rows: block c = (Jc_c[:, 6:nv])', the
 *       identity on the torque columns (torque_col >= 0), beq = h_gravity[6:nv] - q_tau written to BOTH static_lo and static_up
 *   force::Cartesian (Cartesian.cpp:34-65), b only: b = Kp e + Kd (v_ref - J_f qdot) + f_des on contact cart_contact (its frame,
 *       its Jacobian, its wrench); A is the constant selection of the wrench's six columns (the caller's, written once).
 *       e = [p_ref - p; e_o], e_o = -2 x the quaternion error of include/OpenSoT/utils/cartesian_utils.h:144-164 (the one
 *       velocity::Cartesian uses, short path): it points from the actual to the reference orientation and is, to first order, the
 *       rotation vector of R_ref R' (exactly 2 sin(theta / 2) x the axis).  XBot::Utils::computeOrientationError is not vendored:
 *       parity with it is unpinned, as for every model quantity here.  cart_pose_error [B][6] replaces e for callers who bring
 *       their own error.
 *   force::Wrench / Wrenches (Force.cpp:5-26, 51-87) need no producer: A is the constant selection, b the reference.
 * Each destination row receives exactly the columns of the C wrench blocks (for the static rows also the nv - 6 torque columns);
 * every other column of the row, and the gaps between rows and instances, are left untouched (the cmm_ang convention of
 * osot_dynamics), so the rows land in a zero-initialised A_k or C next to other blocks.
 * enabled [B][C] (may be NULL = all): contact c of an instance with enabled == 0 gets an all-zero block in the CoM, FloatingBase
 * and static rows (written as zeros, so a contact may be released and taken up again from cycle to cycle).  For FloatingBase this
 * is setEnabledContacts.  For CoM it stands in for setLinksInContact: with lo = up = 0 wrench limits on the released contact the
 * QP is the same problem as the one over the shorter contact list. */
#define OSOT_FORCE_MAX_CONTACTS 8
typedef struct {
    int n_contacts;                          /* C, 1 .. OSOT_FORCE_MAX_CONTACTS                                              */
    int nv;                                  /* coordinates of the tree, 6 .. OSOT_KIN_MAX_JOINTS (the first six: floating base) */
    int n;                                   /* the plan's variable count, 1 .. OSOT_MAX_QP_VARS                             */
    int wrench_col[OSOT_FORCE_MAX_CONTACTS]; /* first of the six columns of wrench c                                         */
    int torque_col;                          /* first of the nv - 6 torque columns, -1 = x holds no torques                  */
    int cart_contact;                        /* the contact force::Cartesian is on                                           */
    double mass;                             /* total mass of the tree                                                       */
    double gravity[3];                       /* world frame, e.g. (0, 0, -9.81)                                              */
    double com_lambda, com_lambda2, com_lambda_ang;
    double cart_Kp[36], cart_Kd[36];         /* row-major 6 x 6                                                              */
} osot_force_model;
typedef struct {
    int B;
    const double* pose[OSOT_FORCE_MAX_CONTACTS]; /* [B][12] pose of contact c's frame as osot_kinematics writes it (R row-major; p) */
    const double* Jc;                        /* [B][C][6][nv] world Jacobians of the contact frames                          */
    const double* com;                       /* [B][3]                                                                       */
    const double* momentum;                  /* [B][6] centroidal momentum [linear; angular]                                 */
    const double* h_gravity;                 /* [B][nv] h of osot_dynamics with qdot = NULL                                  */
    const double* qdot;                      /* [B][nv], NULL = zero                                                         */
    const int* enabled;                      /* [B][C], NULL = every contact enabled                                         */
    double* com_A;                           /* first of the 6 rows of force::CoM in instance 0, or NULL                     */
    long long com_A_stride;                  /* doubles from one instance to the next (>= 6 * ld)                            */
    int com_A_ld;                            /* row length in doubles (>= n), 0 = n                                          */
    double* com_b;                           /* 6 doubles per instance, or NULL                                              */
    long long com_b_stride;                  /* (6 when dense)                                                               */
    const double* com_pos_ref;               /* p_d [B][3]; NULL = the actual CoM                                            */
    const double* com_vel_ref;               /* v_d [B][3]; NULL = zero                                                      */
    const double* com_acc_ref;               /* a_d [B][3]; NULL = zero                                                      */
    const double* ang_mom_ref;               /* L_d [B][3]; NULL = the actual momentum                                       */
    const double* ang_mom_rate_ref;          /* Ldot_d [B][3]; NULL = zero                                                   */
    double* fb_A;                            /* the 6 rows of force::FloatingBase, likewise                                  */
    long long fb_A_stride;
    int fb_A_ld;
    double* static_A;                        /* the nv - 6 rows of StaticConstraint, likewise (stride >= (nv - 6) * ld)      */
    long long static_A_stride;
    int static_A_ld;
    double* static_lo;                       /* nv - 6 doubles per instance each, both or neither                            */
    double* static_up;
    long long static_b_stride;               /* (nv - 6 when dense)                                                          */
    const double* static_q_tau;              /* [B][nv - 6] constant of the torque variable; NULL = zero                     */
    double* cart_b;                          /* 6 doubles per instance, or NULL                                              */
    long long cart_b_stride;
    const double* cart_pose_ref;             /* [B][12]                                                                      */
    const double* cart_vel_ref;              /* [B][6]; NULL = zero                                                          */
    const double* cart_f_des;                /* [B][6]; NULL = zero                                                          */
    const double* cart_pose_error;           /* [B][6]: replaces e (cart_pose_ref is then not read)                          */
} osot_force_batch;
/* Stream-ordered, no allocation, capturable; B == 0 is a no-op.  Refused with OSOT_ERR_INVALID before any device is touched
 * (osot_last_error() names the field): n_contacts outside 1 .. 8, nv below 6 or above 64, n out of range, static rows with
 * nv == 6, a wrench_col / torque_col range that leaves 0 .. n-1, overlapping column ranges, a row length below n, a stride below
 * rows * ld (below the vector's length for a b), references without the output they belong to, a non-finite gain, gravity or
 * mass, an output without the inputs it is computed from. */
int osot_force_rows(const osot_force_model* model, const osot_force_batch* batch, void* hip_stream);

/* ---- tasks driven by measurements: admittance, IMU, contact error, collision task ------------------------------------
 * osot_feedback turns sensor readings and the model quantities osot_kinematics / osot_dynamics leave on the device into the
 * references and rows of five reference classes, written into the leaves of existing kinds (no plan kind is added).  It is a
 * launch of its own in front of osot_cycle.  Every group below is optional: a group whose output is NULL is skipped.
 *   1. velocity::CartesianAdmittance (src/tasks/velocity/CartesianAdmittance.cpp:50-77), per term t < n_cart, R = cart_pose[t][0:9]:
 *        e = [R f; R m] of cart_wrench[t] = [f; m] measured in the sensor frame.  XBot::Utils::adjointFromRotation is not vendored:
 *        it is taken as blockdiag(R, R), parity with it is unpinned, as for every model quantity here.
 *        dead zone per channel (apply_deadzone, :303-320): e > dz -> e - dz, e < -dz -> e + dz, otherwise 0
 *        e -= cart_wrench_ref[t]
 *        y = filter(e)   (below)
 *        cart_twist_out[t] = cart_twist_in[t] + cart_C o y: the desired twist (p2) of the OSOT_TASK_CARTESIAN leaf
 *   2. velocity::JointAdmittance (JointAdmittance.cpp:28-44): u = joint_h - joint_tau, y = filter(u) with one set of
 *        coefficients, joint_qdot_out = C y, the desired velocity (p2) of the OSOT_TASK_POSTURAL leaf.  C = joint_C [nv][nv]
 *        row-major, one matrix for the batch (row i: an fma chain over j = 0 .. nv-1 from 0), or joint_C_scalar * I where joint_C
 *        is NULL (c * y_i).  With floating_base, entries 0 .. 5 are written as zeros.
 *   3. floating_base::IMU (src/tasks/floating_base/IMU.cpp:33-42): rows 0 .. 2 of imu_A are zeros, rows 3 .. 5 are
 *        imu_fb_J[3:6][0:6] (the floating-base link's frame_J); imu_b = [0; R_imu omega].  Columns 0 .. 5 only: any other column
 *        of a longer row, and the gaps between rows and instances, are left untouched (the cmm_ang convention of osot_dynamics).
 *   4. floating_base::Contact, the lambda * err term (src/tasks/floating_base/Contact.cpp:55-66):
 *        contact_b_out = contact_b_in + contact_lambda * [p_d - p; -e_o], contact_b_in = what rowset_b of osot_kinematics received,
 *        e_o = the quaternion error of include/OpenSoT/utils/cartesian_utils.h:144-164 on the short path, from contact_pose to
 *        contact_pose_ref: the 6-vector velocity::Cartesian's b holds at lambda = 1, orientation gain 1.
 *   5. tasks::velocity::CollisionAvoidance (src/tasks/velocity/CollisionAvoidance.cpp:17-47), per pair row i:
 *        err = ca_dist[i] - ca_threshold; err > 0: row i of ca_A (n columns) and ca_b[i] are written as zeros; otherwise
 *        ca_A[i] = -ca_J[i], ca_b[i] = err (err == 0 counts as violated).  ca_J / ca_dist are pair_J / pair_dist of osot_kinematics.
 * THE FILTER (SecondOrderFilter, include/OpenSoT/tasks/velocity/CartesianAdmittance.h:27-137): per channel
 *        a0 = 1 + 4 eps / (omega ts) + 4 / (omega ts)^2,  a1 = 2 - 8 / (omega ts)^2,  a2 = 1 + 4 / (omega ts)^2 - 4 eps / (omega ts)
 *        (computed on the host inside the call, with the reference's expression);
 *        shift ydd <- yd, yd <- y, udd <- ud, ud <- u, u <- input;  y = 1.0 / a0 * (u + 2 ud + 1 udd - a1 yd - a2 ydd), left to right.
 * THE STATE: state [B][count], count = osot_feedback_state_doubles, caller-owned, read and rewritten by every call that has
 * admittance terms.  Per instance: term t at 24 t as u[6], ud[6], y[6], yd[6]; the joint filter behind the last term as u[nv],
 * ud[nv], y[nv], yd[nv] (udd and ydd are overwritten before they are read: not stored).  All zeros is a fresh filter (the
 * reference's lazy reset(input * 0)); u = ud = y = yd = v is reset(v).  A term whose cart_twist_out is NULL keeps its state.
 * The filter recurrence, the rotations and item 4 are compiled with floating-point contraction off: the same bits wherever the
 * header is compiled. */
#define OSOT_FEEDBACK_MAX_CART 8
typedef struct {
    int nv;                                  /* coordinates of the tree, 1 .. OSOT_KIN_MAX_JOINTS                            */
    int floating_base;                       /* 0 / 1: the first six coordinates are the floating base                       */
    int n_cart;                              /* Cartesian admittance terms, 0 .. OSOT_FEEDBACK_MAX_CART                      */
    int joint;                               /* 0 / 1: the joint admittance filter exists                                    */
    int imu;                                 /* 0 / 1                                                                        */
    int n_pairs;                             /* collision pair rows, 0 .. OSOT_KIN_MAX_PAIRS                                 */
    int n;                                   /* row length of ca_J and ca_A, 1 .. OSOT_MAX_QP_VARS (read with n_pairs > 0)   */
    double cart_C[OSOT_FEEDBACK_MAX_CART * 6];        /* [t][6] compliance (diagonal)                                        */
    double cart_deadzone[OSOT_FEEDBACK_MAX_CART * 6]; /* [t][6], >= 0                                                        */
    double cart_omega[OSOT_FEEDBACK_MAX_CART * 6];    /* [t][6] natural frequency of each channel's filter, > 0              */
    double cart_damping[OSOT_FEEDBACK_MAX_CART * 6];  /* [t][6] damping ratio eps, >= 0                                      */
    double cart_ts[OSOT_FEEDBACK_MAX_CART];           /* [t] time step of the term's filters, > 0                            */
    double joint_omega, joint_damping, joint_ts, joint_C_scalar;
    double contact_lambda;
    double ca_threshold;
} osot_feedback_model;
typedef struct {
    int B;
    double* state;                                        /* [B][count]; required where n_cart + joint > 0               */
    const double* cart_pose[OSOT_FEEDBACK_MAX_CART];      /* [B][12] pose of the sensor frame as osot_kinematics writes it
                                                             (relative to a base link: the producer's frame_base)        */
    const double* cart_wrench[OSOT_FEEDBACK_MAX_CART];    /* [B][6] measured, in the sensor frame                         */
    const double* cart_wrench_ref[OSOT_FEEDBACK_MAX_CART];/* [B][6]; NULL = zero                                          */
    const double* cart_twist_in[OSOT_FEEDBACK_MAX_CART];  /* [B][6] the user's own desired twist; NULL = zero             */
    double* cart_twist_out[OSOT_FEEDBACK_MAX_CART];       /* [B][6]; must not alias cart_twist_in                         */
    const double* joint_tau;                              /* [B][nv] measured joint torques                               */
    const double* joint_h;                                /* [B][nv] h of osot_dynamics                                   */
    const double* joint_C;                                /* [nv][nv] row-major, one for the batch; NULL = joint_C_scalar I */
    double* joint_qdot_out;                               /* [B][nv]                                                      */
    const double* imu_fb_J;                               /* first of the 6 rows (length nv) of the floating-base link's
                                                             Jacobian in instance 0                                       */
    long long imu_fb_J_stride;                            /* doubles from one instance to the next (>= 6 nv)              */
    const double* imu_pose;                               /* [B][12] pose of the IMU's link                               */
    const double* imu_omega;                              /* [B][3] gyroscope reading, in the IMU's frame                 */
    double* imu_A;                                        /* first of the 6 rows in instance 0                            */
    long long imu_A_stride;                               /* (>= 6 ld)                                                    */
    int imu_A_ld;                                         /* row length in doubles (>= 6), 0 = 6                          */
    double* imu_b;                                        /* 6 doubles per instance                                       */
    long long imu_b_stride;                               /* (>= 6)                                                       */
    const double* contact_pose;                           /* [B][12]                                                      */
    const double* contact_pose_ref;                       /* [B][12] the desired contact pose                             */
    const double* contact_b_in;                           /* 6 doubles per instance                                       */
    long long contact_b_in_stride;                        /* (>= 6)                                                       */
    double* contact_b_out;                                /* 6 doubles per instance: the OSOT_TASK_GENERIC leaf; must not
                                                             alias contact_b_in (a repeated call gives the same result)   */
    long long contact_b_out_stride;                       /* (>= 6)                                                       */
    const double* ca_J;                                   /* first of the n_pairs rows (length n) in instance 0           */
    long long ca_J_stride;                                /* (>= n_pairs n)                                               */
    const double* ca_dist;                                /* [B][n_pairs]                                                 */
    double* ca_A;                                         /* first of the n_pairs rows in instance 0; must not be ca_J    */
    long long ca_A_stride;                                /* (>= n_pairs ld)                                              */
    int ca_A_ld;                                          /* row length in doubles (>= n), 0 = n                          */
    double* ca_b;                                         /* n_pairs doubles per instance                                 */
    long long ca_b_stride;                                /* (>= n_pairs)                                                 */
} osot_feedback_batch;
/* Stream-ordered, no allocation, capturable; B == 0 is a no-op.  Refused with OSOT_ERR_INVALID before any device is touched
 * (osot_last_error() names the field): a size out of range, a flag that is not 0 / 1, a filter constant that is not positive
 * and finite (damping and dead zone: negative), a non-finite gain, state NULL with n_cart + joint > 0, a pointer bound to a
 * term beyond n_cart or to a group the model does not have, an output without its inputs, an input without its output, an
 * output that aliases its input, a row length or a stride below what the rows need. */
int osot_feedback(const osot_feedback_model* model, const osot_feedback_batch* batch, void* hip_stream);
/* HOST only.  *count = doubles of filter state per instance: 4 (u, ud, y, yd) per channel, 6 n_cart channels, plus nv with joint. */
int osot_feedback_state_doubles(const osot_feedback_model* model, int* count);
/* HOST only.  CartesianAdmittance::computeParameters (CartesianAdmittance.cpp:171-199) as it is written: C = lambda K^-1,
 * M = (dt / lambda) D - (dt dt / lambda) C^-1, w = dt (C M)^-1 (w: the omega of the term's filters).  OSOT_ERR_INVALID where
 * D[i] <= K[i] dt / lambda for some i (nothing is written), or an argument is NULL. */
int osot_admittance_params(const double K[6], const double D[6], double lambda, double dt, double C[6], double M[6], double w[6]);

/* ---- acceleration task leaves: tracking errors, gain matrices and GainType::Force --------------------------------------
 * osot_acc_tasks turns the model quantities osot_kinematics / osot_dynamics leave on the device into the leaf arrays of the
 * acceleration kinds above (no plan kind is added).  It is a launch of its own between osot_dynamics and osot_id_rows:
 *     osot_kinematics -> osot_dynamics -> osot_acc_tasks -> osot_id_rows -> osot_cycle -> osot_computed_torque
 *   acceleration::Cartesian (src/tasks/acceleration/Cartesian.cpp:147-169), per term t < n_cart, into the leaf p0 of an
 *   OSOT_TASK_ACC_CARTESIAN block (a SubTask is the plan's business: the leaf has the parent's six rows):
 *       pose_err = [p_ref - p; cart_orientation_gain * e_o], e_o = -2 x the quaternion error of
 *                  include/OpenSoT/utils/cartesian_utils.h:144-164 on the short path, from the actual to the reference orientation
 *                  (the convention of force::Cartesian above).  XBot::Utils::computeOrientationError is not vendored: parity with
 *                  it is unpinned, as for every model quantity here.  The update kernel does not apply an orientation gain to a
 *                  supplied pose_err: it is applied here.
 *       vel_err  = vel_ref - J qdot
 *       cart_p0  = [pose_err; vel_err]            (12) without gain matrices and with the Acceleration type
 *                  [pose_err; vel_err; Gp; Gd]    (84) with cart_gain_matrices or the Force type: what acc_gain_matrices reads.
 *                  Acceleration type: Gp = Kp, Gd = Kd.  Force type (:161-169, 517-524): Gp = Mi Kp, Gd = Mi Kd, Mi = J M^-1 J'.
 *       cart_a_ref_out = cart_a_ref_in + Mi cart_f_virtual (Force type; otherwise a copy): the leaf p2 (p1 is Jdot qdot,
 *                  osot_dynamics').
 *   acceleration::CoM (CoM.cpp:74-97; it has no Force type): com_p0 = [com_ref - com; vel_ref - J_com qdot], behind them Kp and
 *       Kd (3 x 3 each) with com_gain_matrices.
 *   acceleration::Postural (Postural.cpp:135-163): post_p0 = [q_ref - q; qdot_ref - qdot] always, and
 *       post_qddot_out = qddot_ref + G (post_lambda2 Kd vel_err + post_lambda Kp pos_err), G = I (Acceleration) or M^-1 (Force).
 *       A stack with matrix gains or the Force type binds post_qddot_out as the block's p2 and sets the plan's lambda = lambda2 = 0
 *       on that block (the update then gives b = p2); with scalar gains and the Acceleration type it need not be bound.
 *   Minv: computeInertiaInverse, [nv][nv], exactly symmetric.
 * M = L L' is factored once per instance; Mi, M^-1 v and Minv all come from that factor by triangular solves (no inverse is
 * formed for the tasks).  Only the lower triangle of M is read, and only when a term is Force-type or Minv is bound.  A pivot
 * that is not finite or not above (nv + 1) 2^-52 x the largest diagonal entry of M counts as failed: ok = 0 for that instance,
 * its Force-type Gp, Gd, Mi and its Minv are written as zeros, cart_a_ref_out = cart_a_ref_in, post_qddot_out = qddot_ref (Force
 * type), its other outputs as usual; no NaN or Inf is written and the other instances are not affected. */
#define OSOT_ACC_MAX_CART 8
#define OSOT_ACC_GAIN_ACCELERATION 0
#define OSOT_ACC_GAIN_FORCE 1
typedef struct {
    int nv;                                       /* coordinates of the tree, 1 .. OSOT_KIN_MAX_JOINTS                       */
    int n_cart;                                   /* Cartesian terms, 0 .. OSOT_ACC_MAX_CART                                 */
    int cart_gain_type[OSOT_ACC_MAX_CART];        /* OSOT_ACC_GAIN_ACCELERATION / OSOT_ACC_GAIN_FORCE                        */
    int cart_gain_matrices[OSOT_ACC_MAX_CART];    /* 0 / 1: Kp, Kd are written behind the errors (implied by the Force type) */
    double cart_Kp[OSOT_ACC_MAX_CART * 36];       /* [t] row-major 6 x 6 (the reference's default: the identity)             */
    double cart_Kd[OSOT_ACC_MAX_CART * 36];
    double cart_orientation_gain[OSOT_ACC_MAX_CART];
    int has_com;                                  /* 0 / 1                                                                   */
    int com_gain_matrices;                        /* 0 / 1                                                                   */
    double com_Kp[9], com_Kd[9];                  /* row-major 3 x 3                                                         */
    int has_postural;                             /* 0 / 1                                                                   */
    int post_gain_type;
    int post_gain_matrices;                       /* 0 / 1: post_Kp / post_Kd are read (0: they must be NULL)                */
    double post_lambda, post_lambda2;
    const double* post_Kp;                        /* DEVICE [nv][nv] row-major, one for the batch; NULL = the identity       */
    const double* post_Kd;
} osot_acc_model;
typedef struct {
    int B;
    const double* q;                                   /* [B][nv] (read by the postural term)                                */
    const double* qdot;                                /* [B][nv]                                                            */
    const double* M;                                   /* first element of instance 0, as osot_dyn_batch.M writes it         */
    long long M_stride;                                /* doubles from one instance to the next (>= nv * nv)                 */
    const double* cart_J[OSOT_ACC_MAX_CART];           /* first of the 6 rows of term t in instance 0; may point into A_k or
                                                          Jc, where osot_kinematics wrote it                                 */
    long long cart_J_stride[OSOT_ACC_MAX_CART];        /* doubles from one instance to the next (>= 6 ld)                    */
    int cart_J_ld[OSOT_ACC_MAX_CART];                  /* row length in doubles (>= nv); columns nv .. ld-1 are not read     */
    const double* cart_pose[OSOT_ACC_MAX_CART];        /* [B][12] as osot_kinematics writes it (R row-major; p)              */
    const double* cart_pose_ref[OSOT_ACC_MAX_CART];    /* [B][12]                                                            */
    const double* cart_vel_ref[OSOT_ACC_MAX_CART];     /* [B][6]; NULL = zero                                                */
    const double* cart_f_virtual[OSOT_ACC_MAX_CART];   /* [B][6]; NULL = zero (Force type only)                              */
    const double* cart_a_ref_in[OSOT_ACC_MAX_CART];    /* [B][6]; NULL = zero                                                */
    double* cart_p0[OSOT_ACC_MAX_CART];                /* 12 or 84 doubles per instance, or NULL                             */
    long long cart_p0_stride[OSOT_ACC_MAX_CART];
    double* cart_a_ref_out[OSOT_ACC_MAX_CART];         /* [B][6] or NULL                                                     */
    double* cart_Mi[OSOT_ACC_MAX_CART];                /* [B][36] or NULL (Force type only)                                  */
    const double* com_J;                               /* first of the 3 rows in instance 0                                  */
    long long com_J_stride;                            /* (>= 3 ld)                                                          */
    int com_J_ld;                                      /* (>= nv)                                                            */
    const double* com;                                 /* [B][3]                                                             */
    const double* com_ref;                             /* [B][3]                                                             */
    const double* com_vel_ref;                         /* [B][3]; NULL = zero                                                */
    double* com_p0;                                    /* 6 or 24 doubles per instance, or NULL                              */
    long long com_p0_stride;
    const double* post_q_ref;                          /* [B][nv]                                                            */
    const double* post_qdot_ref;                       /* [B][nv]; NULL = zero                                               */
    const double* post_qddot_ref;                      /* [B][nv]; NULL = zero                                               */
    double* post_p0;                                   /* [B][2 nv] or NULL                                                  */
    double* post_qddot_out;                            /* [B][nv] or NULL                                                    */
    double* Minv;                                      /* first element of instance 0, or NULL                               */
    long long Minv_stride;                             /* (>= nv * nv)                                                       */
    int* ok;                                           /* [B] or NULL: 1 = the factorisation ran through (or was not needed) */
} osot_acc_batch;
/* Stream-ordered, no allocation, capturable; B == 0 is a no-op.  (The first launch on a device that needs more than 64 KB of LDS
 * -- nv near 64 with many terms or Minv -- raises the kernel's limit, a host-side setting made once; make that launch before a
 * capture.)  Refused with OSOT_ERR_INVALID before any device is touched
 * (osot_last_error() names the field): a size out of range, an unknown gain type, a flag that is not 0 / 1, a non-finite gain,
 * M NULL when it is needed, a required input that is NULL, a stride or row length below what the rows need, an output that
 * aliases an input of its term, a pointer bound to a term beyond n_cart or to a group the model lacks, post_Kp / post_Kd with
 * post_gain_matrices == 0, cart_Mi or cart_f_virtual on a term that is not Force-type, a reference without its output.  nv > 64: OSOT_ERR_UNSUPPORTED (beyond it the
 * Force-type gains are osot_id_force_gains' with an inverse inertia matrix of the caller's). */
int osot_acc_tasks(const osot_acc_model* model, const osot_acc_batch* batch, void* hip_stream);

/* ---- multipliers, active set and the backward pass of the batched explicit QP (opensot_amd/csrc/osot_qp_sens.h) ---------------
 * What QPOasesBackEnd keeps of every solve besides x: the dual solution (getDualSolution, QPOasesBackEnd.cpp:153-158, 291-296:
 * nV + nC entries, the bounds first) and the working set (getActiveBounds / getActiveConstraints, QPOasesBackEnd.h:163-172) --
 * recovered from the problem and a solution x, for B instances -- and, given grad_x = d loss / d x, the gradients of the loss
 * with respect to every input of the QP.  Per instance, with H~ = H + eps_abs I (only the LOWER triangle of H is read):
 *   candidates ... every equality (lA[r] == uA[r], l[i] == u[i]) and every finite side of a bound or row whose residual is within
 *                  active_tol max(1, |bound|); |v| >= 1e20 counts as absent.  At most 2n, in the order equalities (bounds, rows),
 *                  bounds, rows: an instance with more is DEGENERATE and processed on the first 2n.
 *   multipliers .. H~ x + g + C' lambda = 0 in the least-squares sense, by a column-pivoted Householder QR of L^-1 C' (H~ = L L').
 *                  A column whose pivot is below rank_tol times the first pivot is dependent and leaves the set (DEGENERATE).
 *                  An inequality with |lambda| <= dual_tol max(1, |lambda|_inf), or with the wrong sign, leaves the set and the
 *                  factorisation is redone once (DEGENERATE).
 *   y ............ qpOASES' convention, y = -lambda:  H~ x + g = y_b + A' y_c;  y > 0 on a lower side, y < 0 on an upper side;
 *                  [B][n + nc], the n bounds first.  active: 0, -1 lower, +1 upper, 2 equality, for the members of the final set.
 *   backward ..... [H~ C'; C 0] [dx; dlambda] = -[grad_x; 0]:  grad_g = dx, grad_H = (dx x' + x dx') / 2 (symmetric, written in
 *                  full), grad_A = dlambda_r x' + lambda_r dx' on the rows of the set (written in full, zeros elsewhere),
 *                  grad_lA / grad_uA / grad_l / grad_u = -dlambda on the side that is active (an equality: on the lower side, zero
 *                  on the upper: the sum over both is the derivative of a bound moved as one).  No gradient for eps_abs.
 * An instance whose status is not OSOT_STATUS_SOLVED, whose x is not finite, whose H~ is not positive definite (the pivot rule of
 * osot_acc_tasks) or whose results are not finite is SKIPPED: every output of it is zero.  Nothing non-finite is written. */
#define OSOT_SENS_OK         0   /* unique multipliers and derivative                                      */
#define OSOT_SENS_DEGENERATE 1   /* weakly active, dependent or > 2n candidates: a valid one-sided answer  */
#define OSOT_SENS_SKIPPED    2   /* status != SOLVED, non-finite x, or H + eps I not PD: all outputs zero   */
typedef struct osot_qp_sens_options { double active_tol, dual_tol, rank_tol; } osot_qp_sens_options;   /* 0 = 1e-8, 1e-9, 1e-11 */
typedef struct osot_qp_sens_batch {
    int B, n, nc;
    const double *H, *g, *A, *lA, *uA, *l, *u;          /* as osot_qp_solve_batch (A, lA, uA: nc > 0; l, u: both or neither)         */
    double eps_abs;
    const double* x;                                    /* [B][n]                                                                    */
    const int* status;                                  /* [B] OSOT_STATUS_* or NULL = all solved                                    */
    const double* grad_x;                               /* [B][n] or NULL: multipliers only                                          */
    double* y;                                          /* [B][n + nc] or NULL                                                       */
    int* active;                                        /* [B][n + nc] or NULL                                                       */
    double *grad_H, *grad_g, *grad_A, *grad_lA, *grad_uA, *grad_l, *grad_u;   /* shaped as the inputs; any may be NULL               */
    int* flag;                                          /* [B] OSOT_SENS_*                                                           */
} osot_qp_sens_batch;
/* Stream-ordered, no allocation, no synchronisation, capturable; B == 0 is a no-op.  (33 .. 64 variables need more than 64 KB of
 * LDS: the first such launch on a device raises the kernel's limit, a host-side setting made once; make that launch before a
 * capture.)  options NULL, or a tolerance of 0: the default.  Refused before any device is touched (osot_last_error() says why):
 * n > 64 with OSOT_ERR_UNSUPPORTED (65 .. 128 variables are not built); with OSOT_ERR_INVALID B < 0, n < 1, nc < 0, a negative
 * tolerance or eps_abs, H / g / x / flag NULL, nc > 0 with A NULL, A without lA and uA, l without u, a gradient output without
 * grad_x, an output that aliases an input. */
int osot_qp_sensitivity_batch(const osot_qp_sens_batch* b, const osot_qp_sens_options* opt, void* hip_stream);

/* The same call with a workspace of the caller's, for problems of up to OSOT_MAX_QP_VARS (128) variables
 * (opensot_amd/csrc/osot_qp_sens_big.h).  n <= 64 is exactly osot_qp_sensitivity_batch: the same kernel, the same bits, and the
 * workspace is not looked at (it may be NULL).  65 <= n <= 128 with nc <= 2048 runs one 256-thread workgroup per instance under
 * the contract above, word for word; min(B, slots) workgroups walk the batch, each on its own slice of the workspace, so the
 * workspace is sized by the slot count and not by B (n (2n + 2) doubles per slice).
 *   osot_qp_sens_workspace_bytes ... host only, no GPU needed: the bytes the call needs for (B, n, nc); 0 for n <= 64 or B == 0.
 *                                    OSOT_ERR_INVALID: bytes NULL, B < 0, n < 1, nc < 0; OSOT_ERR_UNSUPPORTED: n > 128, nc > 2048
 *                                    with n > 64.
 *   workspace ...................... device memory of the caller, 16-byte aligned, at least that many bytes; its content before
 *                                    the call does not matter and is undefined after it.  One workspace serves one call at a time.
 * Stream-ordered, no allocation, no synchronisation; B == 0 is a no-op.  The first launch on a device raises the kernel's LDS limit,
 * a host-side setting made once: make one eager call before a capture.  Refused before any device is touched (osot_last_error()
 * says why): everything osot_qp_sensitivity_batch refuses except 65 <= n <= 128; n > 128 and, with n > 64, nc > 2048
 * (OSOT_ERR_UNSUPPORTED); with n > 64 and B > 0 a workspace that is NULL, not 16-byte aligned or smaller than
 * osot_qp_sens_workspace_bytes, and an input or output whose first address lies inside the workspace (OSOT_ERR_INVALID). */
int osot_qp_sens_workspace_bytes(int B, int n, int nc, size_t* bytes);
int osot_qp_sensitivity_batch_ws(const osot_qp_sens_batch* b, const osot_qp_sens_options* opt, void* workspace, size_t workspace_bytes,
                                 void* hip_stream);

/* ---- the QP of every level of the batched iHQP cascade, its multipliers, active set and objective (opensot_amd/csrc/osot_ihqp_sens.h)
 * What iHQP exposes besides solve(): getBackEnd(i) (the level's H, g, A, lA, uA, l, u, iHQP.cpp:381-389, BackEnd.h), on the default
 * back-end the dual solution and the working set of that level (QPOasesBackEnd.h:163-172), and getObjective(i).  For handles of
 * osot_solver_create (the wavefront route, n <= 64: one wavefront per instance) and for handles of osot_solver_create_wide whose
 * plan has 65 .. 128 variables (one 256-thread workgroup per instance, opensot_amd/csrc/osot_ihqp_sens_wide.h, and
 * osot_qp_sensitivity_batch_ws's kernel for the multipliers): the same contract, the same results to the tolerances of the tests.
 * A handle of osot_solver_create_wide whose plan has n <= 64 is refused with OSOT_ERR_UNSUPPORTED before any device is touched:
 * such a plan belongs on osot_solver_create.
 *
 * THE LEVEL QP, for the inputs of an osot_qp_batch and the x_levels its solve left behind:
 *   H [B][n][n] ........ A_k' W_k A_k, full and symmetric to the bit, WITHOUT eps_abs: the stored rows (w[k] on the diagonal, or the
 *                        WA / Wb operands of a level with a non-diagonal weight), the rows of a regularisation task with a stored
 *                        Jacobian, then on the diagonal the weights of the level's implicit Postural block and of an
 *                        identity-Jacobian regularisation task.  The rows of an inactive task count with weight zero.
 *   g [B][n] ........... -A_k' W_k b_k (+ the regularisation task's) + c[k]
 *   A [B][rows][n], lA, uA [B][rows] with rows = nc + (task rows of the levels 0 .. level-1), osot_ihqp_level_rows:
 *     rows 0 .. nc-1 ... the plan's row blocks in plan order: stored rows from C, unit-row blocks as e_(first_col+i), lo / up clamped
 *                        to +-1e20; a task-local block (only_level) is a zero row with -1e20 / 1e20 at every level but its own.
 *     then, per level j < level in level order, its m_j task rows with lA = uA = a_r' x_j (x_j = x_levels[.][j]; one fma chain over
 *                        the columns in ascending order): stored rows from A[j], the implicit Postural block as e_i with the
 *                        bound x_j[i]; the rows of an inactive task are zero rows with -1e20 / 1e20; a level switched off by
 *                        level_active gives zero rows with -1 / 1 (iHQP.cpp:301-309).
 *   l, u [B][n] ........ the merged box clamped to +-1e20, or -1e20 / 1e20 where the plan has no bounds. */
typedef struct osot_level_qp { double *H, *g, *A, *lA, *uA, *l, *u; } osot_level_qp;   /* device pointers, all required */
/* rows of the QP of `level` (host only).  OSOT_ERR_INVALID: a null argument, level outside 0 .. n_levels-1. */
int osot_ihqp_level_rows(osot_solver* s, int level, int* rows);
/* One launch, stream-ordered, no allocation, capturable (a wide handle: after one eager call on the device -- the kernel's LDS,
 * 8 (64 (n | 1) + n) bytes, is 67 072 at n = 128, and the first call raises the limit, a host-side setting).  batch: as for osot_ihqp_solve, with x_levels (its level_active and the
 * handle's osot_solver_set_task_active flags are the ones of the solve).  OSOT_ERR_INVALID: a null argument or member of out, level
 * out of range, B outside 0 .. max_batch, what osot_ihqp_solve refuses of a batch, x_levels NULL for level > 0. */
int osot_ihqp_level_qp(osot_solver* s, const osot_qp_batch* batch, int level, const osot_level_qp* out, void* hip_stream);

/* Multipliers, active set, flag and objective of EVERY level, after a solve.  Per active level, from the last one down, three
 * launches on the stream: the level QP into the workspace, osot_qp_sensitivity_batch's kernel on it with x = x_levels[.][k]
 * (conventions, tolerances and flags: above), and the objective.
 *   qp ............ the batch of the solve just made; x_levels and status are required
 *   y[k] .......... [B][n + rows_k] qpOASES' sign, the n bounds first (rows_k: osot_ihqp_level_rows); active[k] likewise; flag[k] [B].
 *                   One pointer per level, each may be NULL.
 *   objective ..... [B][n_levels] or NULL: 1/2 x_k'(H_k + eps_abs I) x_k + g_k' x_k, qpOASES' getObjVal() of the level
 *   workspace ..... device memory of the caller, at least osot_ihqp_sens_workspace_bytes, 8-byte aligned (a wide handle: 16-byte)
 * An instance whose status is not OSOT_STATUS_SOLVED is OSOT_SENS_SKIPPED at every level (zeros); so is every instance at a level
 * that level_active switches off.  Nothing non-finite is written.
 * Stream-ordered, no allocation, no synchronisation, capturable (33 .. 64 variables: after one eager call on the device, see
 * osot_qp_sensitivity_batch; a wide handle: always after one eager call, which raises the LDS limits of the level kernel and of
 * osot_qp_sensitivity_batch_ws's kernel).  Refused before any device is touched (osot_last_error() says why): a wide handle whose
 * plan has n <= 64 (OSOT_ERR_UNSUPPORTED); with OSOT_ERR_INVALID a null argument, B outside 0 .. max_batch, what osot_ihqp_solve
 * refuses of qp, x_levels or status NULL, workspace NULL, misaligned or smaller than needed, a bad tolerance, an input inside the
 * workspace, an output that overlaps an input, the workspace or another output (the workspace by its byte range; the others by
 * their first address).  "Nothing non-finite is written" holds
 * for the outputs: the workspace of an instance that was not solved holds whatever x_levels held.
 *
 * BACKWARD (grad_dq given): the gradients of a loss with respect to the assembled inputs of the cascade, given grad_dq = d loss / d dq.
 * The levels run from the last active one down; level k's multiplier launch also solves its KKT system for gx_k (gx of the last
 * active level is grad_dq) and a pull-back launch per level hands the result on: with dx the level's grad_g, s_r = a_r'x_k and
 * t_r = a_r'dx on the task rows of level k,
 *   grad_b[k][r] = -w_r t_r, grad_w[k][r] = t_r (s_r - b_r), grad_c[k] = dx, grad_A[k][r] += w_r ((s_r - b_r) dx + t_r x_k);
 *   summed over the levels: grad_lo / grad_up += the QP's grad_lA / grad_uA on the global rows, grad_C += its grad_A on the stored
 *   global rows, grad_l / grad_u += its grad_l / grad_u; on the optimality block of level j < k, with rho = grad_lA + grad_uA:
 *   gx_j += A_j' rho, grad_A[j][r] += grad_A_qp[row] + rho_r x_j'.  (Implicit Postural rows have no storage: gx_j and grad_b / grad_w only.)
 * Every gradient output may be NULL; all are zeroed by the call first (stream-ordered fills), then accumulated.  grad_b[k], grad_w[k]
 * [B][m_k], grad_c[k] [B][n], grad_A[k] [B][ma_k][n], grad_C [B][nc_stored][n], grad_lo / grad_up [B][nc], grad_l / grad_u [B][n].
 * A DEGENERATE level gives the one-sided answer of osot_qp_sensitivity_batch (flag[k] says so); a SKIPPED instance zero gradients.
 * Refused: a gradient output without grad_dq (OSOT_ERR_INVALID); grad_dq on a plan with a dense-weight level or a regularisation
 * task (OSOT_ERR_UNSUPPORTED: forward works for them). */
typedef struct osot_ihqp_sens_batch {
    osot_qp_batch qp;
    double* y[OSOT_MAX_LEVELS];
    int* active[OSOT_MAX_LEVELS];
    int* flag[OSOT_MAX_LEVELS];
    double* objective;
    void* workspace;
    unsigned long long workspace_bytes;
    const double* grad_dq;                              /* [B][n] or NULL: forward only */
    double* grad_b[OSOT_MAX_LEVELS];
    double* grad_w[OSOT_MAX_LEVELS];
    double* grad_c[OSOT_MAX_LEVELS];
    double* grad_A[OSOT_MAX_LEVELS];
    double *grad_C, *grad_lo, *grad_up, *grad_l, *grad_u;
} osot_ihqp_sens_batch;
/* bytes of workspace for B instances (host only), rows = the last level's.  Forward: 8 (B (n n + rows n + 2 rows + 4 n) + (B + 1) / 2):
 * one level QP, x of the level and a flag per instance.  want_backward adds 8 B (3 n + 2 rows + L n) (dx, the QP's bound gradients,
 * gx of every level), want_grad_A (grad_A[k] or grad_C will be asked for) 8 B rows n more (the QP's grad_A).
 * A wide handle (65 .. 128 variables): that sum rounded up to 16 bytes, plus osot_qp_sens_workspace_bytes(B, n, rows) -- min(B, slots)
 * slices of 8 n (2n + 2) bytes for the multiplier kernel, slots = 256 (160 KiB / its LDS at (n, rows), at most 4); every level is
 * launched with that many workgroups (the last level has the most rows, so the fewest fit).  OSOT_ERR_UNSUPPORTED: a wide handle
 * whose plan has n <= 64. */
int osot_ihqp_sens_workspace_bytes(osot_solver* s, int B, int want_backward, int want_grad_A, unsigned long long* bytes);
int osot_ihqp_sensitivity(osot_solver* s, const osot_ihqp_sens_batch* b, const osot_qp_sens_options* opt, void* hip_stream);

/* ---- layout of the structs above as THIS library was compiled (for bindings that mirror them by hand: ctypes, cgo, JNI ...).
 * name = the typedef's name ("osot_plan_desc", "osot_qp_batch", ...).  *size = sizeof; the byte offset of every member, in
 * declaration order, goes to offsets[0 .. *n_fields) (at most max_fields are written; offsets may be NULL).  Unknown name:
 * OSOT_ERR_INVALID.  opensot_amd/abi.py is checked against it in tests/test_abi_host.py. */
int osot_abi_layout(const char* name, unsigned long long* size, unsigned long long* offsets, int max_fields, int* n_fields);

/* ---- multi-GPU: collect solved dq shards ---------------------------------------------------- */
typedef struct osot_comm osot_comm;
/* unique id exchange is the caller's job (e.g. torch.distributed broadcast of the 128-byte id) */
int osot_comm_unique_id(void* id128);
int osot_comm_create(const void* id128, int rank, int world, int device, osot_comm** out);
int osot_comm_destroy(osot_comm* c);
/* all ranks: recv[world*count] <- concat_r send_r[count] (fp64), on hip_stream */
int osot_allgather_dq(osot_comm* c, const double* send, double* recv, long long count, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
