// osot_plan_shape.h -- what the C-ABI plan says about sizes, offsets and switches, read ONCE for every route: the helpers that
// interpret a plan (implicit blocks, row counts, validation), the part of the kernel-argument plan that the wavefront route
// (DevPlan, osot_kernels.h) and the workgroup route (wide::Plan, osot_cascade_wide.h) share, and the check + copy of a call's
// batch pointers.  No HIP: the C-ABI header and the standard library only, so the host builds of tests/emu compile it as it is.
#pragma once
#include <cstddef>
#include <cstring>
#include <type_traits>
#include "../../include/osot_mi355x.h"   // OSOT_MAX_* (the C-ABI's limits are the kernels' limits)

#define OSOT_KMAX_LEVELS 8
#define OSOT_KMAX_TASKS 8
#define OSOT_KMAX_FLAT_TASKS 24
#define OSOT_KMAX_BOUNDS 4
#define OSOT_KMAX_ROWBLOCKS 8
#define OSOT_KMAX_FLAT_ROWS 256
static_assert(OSOT_KMAX_LEVELS == OSOT_MAX_LEVELS && OSOT_KMAX_TASKS == OSOT_MAX_TASKS && OSOT_KMAX_BOUNDS == OSOT_MAX_BOUNDS &&
              OSOT_KMAX_ROWBLOCKS == OSOT_MAX_ROWBLOCKS, "the kernels' limits are the C-ABI's");

namespace osot {

// a Postural block has A = [I 0] (Postural.cpp:37): implicit, never stored -- unless it is a SubTask of one
inline bool task_is_implicit(const osot_task_desc& t) {
    return (t.kind == OSOT_TASK_POSTURAL || t.kind == OSOT_TASK_ACC_POSTURAL) && t.row_mask == 0ull && !t.dense_weight;
}
// rows of the parent of a sub-task (the kind's own size unless given)
inline int task_parent_rows(const osot_task_desc& t, int n) {
    if (t.row_mask == 0ull) return t.rows;
    if (t.parent_rows > 0) return t.parent_rows;
    switch (t.kind) {
        case OSOT_TASK_CARTESIAN: case OSOT_TASK_ACC_CARTESIAN: return 6;
        case OSOT_TASK_COM: case OSOT_TASK_ACC_COM: return 3;
        case OSOT_TASK_POSTURAL: case OSOT_TASK_ACC_POSTURAL: return n;
        default: return 0;
    }
}

inline int plan_level_rows(const osot_plan_desc* p, int k, int* m_total, int* m_stored) {
    if (!p || k < 0 || k >= p->n_levels) return OSOT_ERR_INVALID;
    int m = 0, ma = 0;
    const osot_level_desc& lv = p->level[k];
    for (int j = 0; j < lv.n_tasks; ++j) {
        m += lv.task[j].rows;
        if (!task_is_implicit(lv.task[j])) ma += lv.task[j].rows;
    }
    if (m_total) *m_total = m;
    if (m_stored) *m_stored = ma;
    return OSOT_OK;
}

inline int plan_constraint_rows(const osot_plan_desc* p, int* nc) {
    if (!p) return OSOT_ERR_INVALID;
    int s = 0;
    for (int j = 0; j < p->n_rowblocks; ++j) s += p->rowblock[j].rows;
    if (nc) *nc = s;
    return OSOT_OK;
}

inline bool rows_are_implicit(int kind) {
    return kind == OSOT_ROWS_ACC_JOINT_LIMITS || kind == OSOT_ROWS_ACC_VELOCITY_LIMITS || kind == OSOT_ROWS_UNIT_GENERIC ||
           kind == OSOT_ROWS_ACC_JOINT_LIMITS_VIABILITY || kind == OSOT_ROWS_ACC_JOINT_LIMITS_ECBF;
}
// the plan holds a bound whose leaf is the PREVIOUS cycle's velocity (velocity::JointLimitsInvariance): a rollout of several steps
// cannot carry it, the leaf inputs are held fixed inside a launch
inline bool plan_has_invariance_bound(const osot_plan_desc& p) {
    for (int j = 0; j < p.n_bounds; ++j) if (p.bound[j].kind == OSOT_BOUND_JOINT_LIMITS_INVARIANCE) return true;
    return false;
}
// every constraint row of the plan is an EQUALITY by construction: TaskToConstraint blocks (`stack << l_sole`,
// TaskToConstraint.cpp:34-52) whose error band is a point -- the update writes lo = b + err_lb and up = b + err_ub, bit-equal
// then.  Such rows live in the equality phase of every level; the bounds are the only inequalities, which is what the BOX
// instantiation of the kernels assumes (a plan without rows is the trivial case).
inline bool plan_rows_all_equalities(const osot_plan_desc& p) {
    for (int j = 0; j < p.n_rowblocks; ++j) {
        const osot_rows_desc& rb = p.rowblock[j];
        if (rb.kind != OSOT_ROWS_TASK_CARTESIAN && rb.kind != OSOT_ROWS_TASK_COM) return false;
        for (int i = 0; i < rb.rows && i < OSOT_MAX_BAND_ROWS; ++i)
            if (!(rb.err_lb[i] == rb.err_ub[i])) return false;
    }
    return true;
}
inline int plan_stored_constraint_rows(const osot_plan_desc* p, int* nc_stored) {
    if (!p) return OSOT_ERR_INVALID;
    int s = 0;
    for (int j = 0; j < p->n_rowblocks; ++j) if (!rows_are_implicit(p->rowblock[j].kind)) s += p->rowblock[j].rows;
    if (nc_stored) *nc_stored = s;
    return OSOT_OK;
}

// wide = 0: the wavefront route (osot_plan_validate, osot_solver_create: n <= OSOT_MAX_VARS); 1: the workgroup route
// (osot_plan_validate_wide, osot_solver_create_wide: n <= OSOT_MAX_QP_VARS, osot_cascade_wide.h) -- the same feature set
inline int plan_validate(const osot_plan_desc* p, const char** why, int wide = 0) {
    static const char* ok = "";
    *why = ok;
    if (!p) { *why = "null plan"; return OSOT_ERR_INVALID; }
    if (!wide && (p->n < 1 || p->n > OSOT_MAX_VARS)) { *why = "n out of range (1..64)"; return OSOT_ERR_INVALID; }
    if (wide && (p->n < 1 || p->n > OSOT_MAX_QP_VARS)) { *why = "n out of range (1..128)"; return OSOT_ERR_INVALID; }
    if (p->n_levels < 1 || p->n_levels > OSOT_MAX_LEVELS) { *why = "n_levels out of range"; return OSOT_ERR_INVALID; }
    if (p->n_bounds < 0 || p->n_bounds > OSOT_MAX_BOUNDS) { *why = "n_bounds out of range"; return OSOT_ERR_INVALID; }
    if (p->n_rowblocks < 0 || p->n_rowblocks > OSOT_MAX_ROWBLOCKS) { *why = "n_rowblocks out of range"; return OSOT_ERR_INVALID; }
    if (!(p->eps_abs >= 0.0)) { *why = "negative eps"; return OSOT_ERR_INVALID; }
    int flat = 0;
    for (int k = 0; k < p->n_levels; ++k) {
        const osot_level_desc& lv = p->level[k];
        if (lv.n_tasks < 1 || lv.n_tasks > OSOT_MAX_TASKS) { *why = "n_tasks out of range"; return OSOT_ERR_INVALID; }
        flat += lv.n_tasks;
        for (int j = 0; j < lv.n_tasks; ++j) {
            const osot_task_desc& t = lv.task[j];
            if (t.rows < 1) { *why = "task with no rows"; return OSOT_ERR_INVALID; }
            if (t.row_mask != 0ull) {   // SubTask: rows = kept rows, all inside the parent
                const int pr = task_parent_rows(t, p->n);
                if (pr < 1 || pr > 64) { *why = "sub-task: parent rows out of range (1..64)"; return OSOT_ERR_INVALID; }
                if (__builtin_popcountll(t.row_mask) != t.rows) { *why = "sub-task: rows != popcount(row_mask)"; return OSOT_ERR_INVALID; }
                if (pr < 64 && (t.row_mask >> pr) != 0ull) { *why = "sub-task: row_mask selects rows beyond the parent"; return OSOT_ERR_INVALID; }
                if ((t.kind == OSOT_TASK_CARTESIAN || t.kind == OSOT_TASK_ACC_CARTESIAN) && pr != 6) { *why = "Cartesian parent has 6 rows"; return OSOT_ERR_INVALID; }
                if ((t.kind == OSOT_TASK_COM || t.kind == OSOT_TASK_ACC_COM) && pr != 3) { *why = "CoM parent has 3 rows"; return OSOT_ERR_INVALID; }
                if (t.kind < OSOT_TASK_GENERIC || t.kind > OSOT_TASK_ACC_POSTURAL) { *why = "unknown task kind"; return OSOT_ERR_UNSUPPORTED; }
                if (!(t.weight >= 0.0)) { *why = "negative task weight"; return OSOT_ERR_INVALID; }
                continue;
            }
            switch (t.kind) {
                case OSOT_TASK_GENERIC: break;
                case OSOT_TASK_CARTESIAN: case OSOT_TASK_ACC_CARTESIAN:
                    if (t.rows != 6) { *why = "Cartesian task must have 6 rows"; return OSOT_ERR_INVALID; } break;
                case OSOT_TASK_COM: case OSOT_TASK_ACC_COM:
                    if (t.rows != 3) { *why = "CoM task must have 3 rows"; return OSOT_ERR_INVALID; } break;
                case OSOT_TASK_POSTURAL: case OSOT_TASK_ACC_POSTURAL:
                    if (t.rows > p->n) { *why = "Postural task cannot have more than n rows"; return OSOT_ERR_INVALID; }
                    if (task_is_implicit(t) && j != lv.n_tasks - 1) { *why = "an implicit Postural block must be the last block of its level"; return OSOT_ERR_UNSUPPORTED; }
                    break;
                default: *why = "unknown task kind"; return OSOT_ERR_UNSUPPORTED;
            }
            if (!(t.weight >= 0.0)) { *why = "negative task weight"; return OSOT_ERR_INVALID; }
            if (t.body_frame && t.kind != OSOT_TASK_CARTESIAN) { *why = "body_frame is an option of velocity::Cartesian"; return OSOT_ERR_INVALID; }
            if (t.dense_weight && t.rows > 64) { *why = "dense weight: at most 64 rows per block"; return OSOT_ERR_INVALID; }
            if (t.acc_gain_matrices && t.kind != OSOT_TASK_ACC_CARTESIAN && t.kind != OSOT_TASK_ACC_COM) {
                *why = "gain matrices are an option of the acceleration Cartesian / CoM tasks"; return OSOT_ERR_INVALID; }
        }
    }
    if (p->has_regularisation) {   // identity-Jacobian regularisation only: Hr is folded into the diagonal
        const osot_task_desc& t = p->regularisation;
        if (p->regularisation_dense) {   // stored Jacobian A_r (osot_qp_batch.A_reg): any kind whose b the update forms without A
            if (t.kind != OSOT_TASK_GENERIC && t.kind != OSOT_TASK_CARTESIAN && t.kind != OSOT_TASK_COM) {
                *why = "regularisation task with a stored Jacobian: kinds GENERIC, CARTESIAN, COM"; return OSOT_ERR_UNSUPPORTED; }
            if (t.rows < 1 || t.rows > 64) { *why = "regularisation task: rows out of range (1..64)"; return OSOT_ERR_INVALID; }
        } else {
            if (t.kind != OSOT_TASK_GENERIC && t.kind != OSOT_TASK_POSTURAL && t.kind != OSOT_TASK_ACC_POSTURAL) {
                *why = "regularisation task without a stored Jacobian: identity-Jacobian kinds (generic b with A = [I 0], Postural)"; return OSOT_ERR_UNSUPPORTED; }
            if (t.rows < 1 || t.rows > p->n) { *why = "regularisation task: rows out of range (1..n)"; return OSOT_ERR_INVALID; }
        }
        if (t.row_mask != 0ull) { *why = "regularisation task cannot be a sub-task"; return OSOT_ERR_UNSUPPORTED; }
        if (t.dense_weight || t.body_frame) { *why = "regularisation task: scalar weight, no frame option"; return OSOT_ERR_UNSUPPORTED; }
        if (!(t.weight >= 0.0)) { *why = "negative task weight"; return OSOT_ERR_INVALID; }
        flat += 1;
    }
    if (flat > OSOT_KMAX_FLAT_TASKS) { *why = "too many leaf tasks in total"; return OSOT_ERR_UNSUPPORTED; }
    {
        int rows_total = p->has_regularisation ? p->regularisation.rows : 0;
        for (int k = 0; k < p->n_levels; ++k) for (int j = 0; j < p->level[k].n_tasks; ++j) rows_total += p->level[k].task[j].rows;
        if (rows_total > OSOT_KMAX_FLAT_ROWS) { *why = "more than 256 task rows in all levels together"; return OSOT_ERR_UNSUPPORTED; }
    }
    for (int j = 0; j < p->n_bounds; ++j) {
        const osot_bound_desc& bd = p->bound[j];
        if (bd.kind < 0 || bd.kind > OSOT_BOUND_JOINT_LIMITS_INVARIANCE) { *why = "unknown bound kind"; return OSOT_ERR_UNSUPPORTED; }
        if (bd.kind == OSOT_BOUND_JOINT_LIMITS_INVARIANCE && !(bd.dT > 0.0)) {
            *why = "joint limits invariance: dT (the control period) must be positive"; return OSOT_ERR_INVALID; }
        if (bd.kind == OSOT_BOUND_JOINT_LIMITS_INVARIANCE && !(bd.scaling > 0.0 && bd.scaling <= 1.0)) {   // setPStepAheadPredictor: p <= 1
            *why = "joint limits invariance: scaling (the step-ahead predictor p) must be in (0, 1]"; return OSOT_ERR_INVALID; }
    }
    for (int j = 0; j < p->n_rowblocks; ++j) {
        const osot_rows_desc& rb = p->rowblock[j];
        if ((rb.kind < 0 || rb.kind > OSOT_ROWS_NORMAL_TORQUE) && rb.kind != OSOT_ROWS_CONVEX_HULL &&
            (rb.kind < OSOT_ROWS_ACC_JOINT_LIMITS_VIABILITY || rb.kind > OSOT_ROWS_POSITION_COM)) { *why = "unknown row-block kind"; return OSOT_ERR_UNSUPPORTED; }
        if ((rb.kind == OSOT_ROWS_POSITION_CARTESIAN || rb.kind == OSOT_ROWS_POSITION_COM) && (rb.rows < 1 || rb.rows > 16)) {
            *why = "Cartesian position constraint: rows = half-spaces, 1..16"; return OSOT_ERR_INVALID; }
        if (rb.kind == OSOT_ROWS_ACC_JOINT_LIMITS_VIABILITY && !(rb.p >= 1.0)) {
            *why = "viability joint limits: p (the step-ahead predictor) must be at least 1"; return OSOT_ERR_INVALID; }
        if (rb.kind == OSOT_ROWS_CONVEX_HULL && (rb.rows < 3 || rb.rows > OSOT_KIN_MAX_POINTS)) {
            *why = "convex hull block: rows = contact points, 3..16"; return OSOT_ERR_INVALID; }
        if (rb.kind == OSOT_ROWS_TASK_CARTESIAN && rb.rows != 6) { *why = "a Cartesian task as a constraint has 6 rows"; return OSOT_ERR_INVALID; }
        if (rb.kind == OSOT_ROWS_TASK_COM && rb.rows != 3) { *why = "a CoM task as a constraint has 3 rows"; return OSOT_ERR_INVALID; }
        if (rb.kind == OSOT_ROWS_TASK_CARTESIAN || rb.kind == OSOT_ROWS_TASK_COM)
            for (int i = 0; i < rb.rows; ++i) if (!(rb.err_ub[i] >= rb.err_lb[i])) {
                *why = "Some components of err_ub are smaller than err_lb!!!"; return OSOT_ERR_INVALID; }   // TaskToConstraint.cpp:43
        if (rb.kind == OSOT_ROWS_COLLISION && (rb.n_candidates < 0 || rb.n_candidates > 256 || (rb.n_candidates > 0 && rb.n_candidates < rb.rows))) {
            *why = "collision block: n_candidates must be 0 or in rows..256"; return OSOT_ERR_INVALID; }
        if (rb.rows < 1 || rb.rows > 256) { *why = "row block size out of range (1..256)"; return OSOT_ERR_INVALID; }
        if (rb.kind == OSOT_ROWS_DYN_FEASIBILITY && rb.rows != 6) { *why = "DynamicFeasibility has 6 rows"; return OSOT_ERR_INVALID; }
        if (rb.kind == OSOT_ROWS_FRICTION_CONE && (rb.rows % 5 != 0 || rb.first_col < 0 || rb.first_col + 3 * (rb.rows / 5) > p->n)) {
            *why = "friction cone block: rows = 5*contacts and 3 force columns per contact inside x"; return OSOT_ERR_INVALID; }
        if (rb.kind >= OSOT_ROWS_WRENCH_FRICTION_CONE && rb.kind <= OSOT_ROWS_NORMAL_TORQUE) {   // 6 wrench columns per contact
            const int per = rb.kind == OSOT_ROWS_WRENCH_FRICTION_CONE ? 5 : (rb.kind == OSOT_ROWS_COP ? 4 : 8);
            if (rb.rows % per != 0 || rb.first_col < 0 || rb.first_col + 6 * (rb.rows / per) > p->n) {
                *why = rb.kind == OSOT_ROWS_WRENCH_FRICTION_CONE ? "wrench friction cone block: rows = 5*contacts and 6 wrench columns per contact inside x"
                     : (rb.kind == OSOT_ROWS_COP ? "CoP block: rows = 4*contacts and 6 wrench columns per contact inside x"
                                                 : "normal torque block: rows = 8*contacts and 6 wrench columns per contact inside x");
                return OSOT_ERR_INVALID;
            }
        }
        if (rows_are_implicit(rb.kind) && (rb.first_col < 0 || rb.first_col + rb.rows > p->n)) {
            *why = "unit-row block exceeds the variables"; return OSOT_ERR_INVALID; }
        if (rows_are_implicit(rb.kind) && rb.kind != OSOT_ROWS_UNIT_GENERIC && rb.kind != OSOT_ROWS_ACC_JOINT_LIMITS_ECBF && !(rb.dT * rb.p > 0.0)) { *why = "acceleration limits need dT*p > 0"; return OSOT_ERR_INVALID; }
        if (rb.only_level < 0 || rb.only_level > p->n_levels) { *why = "row block: only_level out of range (0..n_levels)"; return OSOT_ERR_INVALID; }
    }
    if (wide) {   // the workgroup solver's row limit (osot_qp_big.h: kMaxRows) holds the global rows and every level's optimality rows
        int nc = 0, rows = 0;
        plan_constraint_rows(p, &nc);
        for (int k = 0; k < p->n_levels; ++k) for (int j = 0; j < p->level[k].n_tasks; ++j) rows += p->level[k].task[j].rows;
        if (nc + rows > 2048) { *why = "wide route: more than 2048 constraint and task rows together"; return OSOT_ERR_UNSUPPORTED; }
    }
    return OSOT_OK;
}

// The kernel-argument structs of the two iHQP routes (DevPlan / DevBatch in osot_kernels.h, wide::Plan / wide::Batch in
// osot_cascade_wide.h) keep their own member order -- it fixes the kernels' scalar-load offsets, and with them the register
// allocation -- but name the shared members alike, so the two functions below fill either: make_plan_shape writes n, L, nc,
// nc_stored, m[], ma[], optoff[], nblocks, blk_rows/off/stored_off/implicit/first_col/level[], ntask[], task_off[][], inactive[],
// active_mask, max_iter, eps_abs, reg_rows, reg_w, reg_dense; fill_batch_ptrs writes B, A[], b[], w[], c[], WA[], Wb[], C, lo, up,
// l, u, b_reg, A_reg, dq, x_levels, accepted_slack, status, iterations.

// the single walk over levels, tasks and row blocks (and the call's level / task switches); zeroes S first
// task_active: [OSOT_MAX_LEVELS][OSOT_MAX_TASKS] flags (Task::setActive), null = all active
template <class Plan>
inline void make_plan_shape(const osot_plan_desc& p, const unsigned char* level_active, const unsigned char* task_active, Plan& S) {
    std::memset(&S, 0, sizeof(S));
    S.n = p.n;
    S.L = p.n_levels;
    S.nblocks = p.n_rowblocks;
    int off = 0, soff = 0;
    for (int j = 0; j < p.n_rowblocks; ++j) {
        const osot_rows_desc& rb = p.rowblock[j];
        S.blk_rows[j] = rb.rows;
        S.blk_off[j] = off;
        S.blk_stored_off[j] = soff;
        S.blk_implicit[j] = rows_are_implicit(rb.kind) ? 1 : 0;
        S.blk_first_col[j] = rb.first_col;
        S.blk_level[j] = rb.only_level;
        off += rb.rows;
        if (!S.blk_implicit[j]) soff += rb.rows;
    }
    S.nc = off;
    S.nc_stored = soff;
    for (int k = 0; k < p.n_levels; ++k) {
        const osot_level_desc& lv = p.level[k];
        int m = 0, ma = 0;
        S.ntask[k] = lv.n_tasks;
        for (int j = 0; j < lv.n_tasks; ++j) {
            S.task_off[k][j] = m;
            m += lv.task[j].rows;
            if (!task_is_implicit(lv.task[j])) ma += lv.task[j].rows;
            if (task_active && !task_active[k * OSOT_MAX_TASKS + j]) S.inactive[k] |= (1u << j);
        }
        S.task_off[k][lv.n_tasks] = m;
        S.m[k] = m;
        S.ma[k] = ma;
        S.optoff[k + 1] = S.optoff[k] + m;
        if (!level_active || level_active[k]) S.active_mask |= (1u << k);
    }
    // the iteration cap of every level's QP, both routes: 20 x (variables + constraint rows + all levels' rows) + 100
    S.max_iter = p.max_iter > 0 ? p.max_iter : 20 * (p.n + S.nc + S.optoff[p.n_levels]) + 100;
    S.eps_abs = p.eps_abs;
    S.reg_rows = p.has_regularisation ? p.regularisation.rows : 0;
    S.reg_w = p.has_regularisation ? p.regularisation.weight : 0.0;
    S.reg_dense = (p.has_regularisation && p.regularisation_dense) ? 1 : 0;
}

// doubles of a wavefront kernel's row table of capacity cap (even): rlo, rup, rptr (8 B per row each), rowstate and eqlist
// (4 B per row each), rsrc (1 B per row)
inline int row_table_doubles(int cap) { return 3 * cap + cap + (cap + 7) / 8; }

inline bool level_has_dense_weight(const osot_level_desc& lv) {
    for (int j = 0; j < lv.n_tasks; ++j) if (lv.task[j].dense_weight) return true;
    return false;
}
// the checks of a batch that every front-end makes (the null-check messages exist here only); each returns the reason, or null
inline const char* level_ptrs_missing(const osot_qp_batch& b, int k, int ma, bool dense) {
    if (ma > 0 && !b.A[k]) return "A[k] is null for a level with stored rows";
    if (!b.b[k]) return "b[k] is null";
    if (dense && (!b.WA[k] || !b.Wb[k])) return "level has a non-diagonal weight but WA[k] / Wb[k] is null";
    return nullptr;
}
inline const char* bounds_missing(const osot_plan_desc& p, const osot_qp_batch& b) {
    return (p.n_bounds > 0 && (!b.l || !b.u)) ? "plan has bounds but l/u is null" : nullptr;
}
inline const char* outputs_missing(const osot_qp_batch& b) { return (!b.dq || !b.status) ? "dq/status output is null" : nullptr; }

// the iHQP routes' check of a call's batch against the plan, and its copy into the kernel argument: a pointer the plan has no
// use for is NOT passed on (C without stored rows, l/u without bounds, b_reg / A_reg without the regularisation flags, WA/Wb
// on a level without a dense weight) -- the kernels read "null" as "absent".  D is expected zeroed.
// S: the plan argument make_plan_shape filled
template <class Plan, class Batch>
inline int fill_batch_ptrs(const osot_plan_desc& p, const Plan& S, const osot_qp_batch& b, Batch& D, const char** why) {
    D.B = b.B;
    for (int k = 0; k < p.n_levels; ++k) {
        const bool dense = level_has_dense_weight(p.level[k]);
        if ((*why = level_ptrs_missing(b, k, S.ma[k], dense))) return OSOT_ERR_INVALID;
        D.A[k] = b.A[k]; D.b[k] = b.b[k]; D.w[k] = b.w[k]; D.c[k] = b.c[k];
        if (dense) { D.WA[k] = b.WA[k]; D.Wb[k] = b.Wb[k]; }
    }
    if (S.nc > 0 && (!b.lo || !b.up)) { *why = "plan has constraint rows but lo/up is null"; return OSOT_ERR_INVALID; }
    if (S.nc_stored > 0 && !b.C) { *why = "plan has stored constraint rows but C is null"; return OSOT_ERR_INVALID; }
    if ((*why = bounds_missing(p, b))) return OSOT_ERR_INVALID;
    if ((*why = outputs_missing(b))) return OSOT_ERR_INVALID;
    if (p.has_regularisation && !b.b_reg) { *why = "plan has a regularisation task but b_reg is null"; return OSOT_ERR_INVALID; }
    if (S.reg_dense && !b.A_reg) { *why = "the regularisation task has a stored Jacobian but A_reg is null"; return OSOT_ERR_INVALID; }
    *why = "";
    D.C = S.nc_stored ? b.C : nullptr; D.lo = b.lo; D.up = b.up;
    D.l = p.n_bounds ? b.l : nullptr; D.u = p.n_bounds ? b.u : nullptr;
    D.b_reg = p.has_regularisation ? b.b_reg : nullptr;
    D.A_reg = S.reg_dense ? b.A_reg : nullptr;
    D.dq = b.dq; D.x_levels = b.x_levels; D.accepted_slack = b.accepted_slack;
    D.status = b.status; D.iterations = b.iterations;
    return OSOT_OK;
}

}  // namespace osot
