// osot_host_plan.h -- host-side translation of the C-ABI plan into kernel arguments (no HIP calls).  What a plan says is read
// in osot_plan_shape.h; here: the wavefront kernels' memory layout (lane layout, LDS carve-up) and the update kernel's arguments.
#pragma once
#include <initializer_list>
#include "osot_plan_shape.h"
#include "osot_kernels.h"

namespace osot {

// the lane layout of the wavefront kernels for n variables: 32; 40 (round 5: n <= 38, the reference's 35-coordinate COMAN -- two
// wavefronts per SIMD); 56: the 64-lane solver with the LDS of n <= 54, four wavefronts per CU instead of three (osot_qp_core.h,
// WaveCtx); 64
inline int pick_np(int n) {
    return (n <= 32) ? 32 : ((n <= WaveCtx<40>::NMAX) ? 40 : ((n <= WaveCtx<56>::NMAX) ? 56 : 64));
}
// doubles of M1, M2, V of one wave's LDS slice (sizes fixed by NP)
inline int wave_lds_doubles(int NP) {
    return NP == 32 ? WaveCtx<32>::LDS_DOUBLES : (NP == 40 ? WaveCtx<40>::LDS_DOUBLES : (NP == 56 ? WaveCtx<56>::LDS_DOUBLES : WaveCtx<64>::LDS_DOUBLES));
}

// LDS carve-up (doubles) of one wave's slice for padded size NP: M1, M2, V, then the row table (row_table_doubles).
// Returns the total in doubles.
inline int lds_layout(int NP, int n_rows, int* rows_off, int* rows_cap) {
    // (round 5: the phantom-lane layouts 40 and 56 too -- osot_qp_kernel<40> / <56> for the plugin route and nHQP's level QPs)
    int d = (wave_lds_doubles(NP) + 1) & ~1;
    *rows_off = d;
    const int cap = ((n_rows > 0 ? n_rows : 1) + 1) & ~1;
    *rows_cap = cap;
    d += row_table_doubles(cap);
    d = (d + 1) & ~1;
    return d;
}

// returns OSOT_OK and fills P, the padded size NP (pick_np) and the dynamic LDS bytes per workgroup (= wave)
// task_active: [OSOT_MAX_LEVELS][OSOT_MAX_TASKS] flags (Task::setActive), null = all active
inline int make_dev_plan(const osot_plan_desc& p, const unsigned char* level_active, DevPlan& P, int& NP,
                         size_t& lds_bytes, const unsigned char* task_active = nullptr) {
    std::memset(&P, 0, sizeof(P));
    make_plan_shape(p, level_active, task_active, P);
    for (int k = 0; k < p.n_levels; ++k) P.ident_rows[k] = P.m[k] - P.ma[k];
    NP = pick_np(p.n);
    // cascade layout: M1, M2, V | the row table of the global rows and every level's optimality rows.  (lds_layout rounds its
    // total up to an even number of doubles once more; this total is NOT rounded: eight bytes can move rows_in_global below)
    const int nrows_max = P.nc + P.optoff[p.n_levels];
    const int cap = ((nrows_max > 0 ? nrows_max : 1) + 1) & ~1;
    int total = (wave_lds_doubles(NP) + 1) & ~1;
    P.lds_rows_off = total;
    P.lds_rows_cap = cap;
    const int table = row_table_doubles(cap);
    P.rows_doubles = table;
    // NP = 64 (round 3): the row table lives in a per-instance slice of device memory (DevBatch.rows_scratch, served by the
    // CU's L1 / L2) whenever taking it out of LDS buys another resident wavefront per CU
    P.rows_in_global = 0;
    if (NP > 32) {
        const size_t with = (size_t)(total + table) * sizeof(double), without = (size_t)total * sizeof(double);
        if ((160 * 1024) / without > (160 * 1024) / with) P.rows_in_global = 1;
    }
    if (!P.rows_in_global) total += table;
    lds_bytes = (size_t)total * sizeof(double);
    return OSOT_OK;
}

// ---- which kernel an iHQP launch of the wavefront route runs ----
// The decision is a value: choose_kernel_variant computes it from plain facts, osot_mi355x.hip (with_ihqp_kernel) maps it to the
// instantiation -- for the launch, and over kernel_variants for the dynamic-LDS attribute at creation.
enum KernelFamily { KERNEL_CASCADE = 0, KERNEL_CYCLE = 1, KERNEL_CONTROL = 2 };   // osot_cascade_kernel / osot_cycle_kernel / osot_control_cycle_kernel
struct KernelVariant { int family; bool prof, extra, box, roll; };   // the instantiation's PROF / EXTRA / BOX / ROLL (false where the family has no such argument)
inline bool operator==(const KernelVariant& a, const KernelVariant& b) { return a.family == b.family && a.prof == b.prof && a.extra == b.extra && a.box == b.box && a.roll == b.roll; }
// (argument lists and defaults as the kernel templates have them after NP)
constexpr KernelVariant cascade_variant(bool prof, bool extra = false, bool box = false) { return {KERNEL_CASCADE, prof, extra, box, false}; }
constexpr KernelVariant cycle_variant(bool extra = false, bool box = false) { return {KERNEL_CYCLE, false, extra, box, false}; }
constexpr KernelVariant control_variant(bool extra = false, bool box = false, bool roll = false) { return {KERNEL_CONTROL, false, extra, box, roll}; }

// every variant of the lane layout T (13, 14 at T = 32): what osot_solver_create prepares.  -> their number
constexpr int kMaxKernelVariants = 14;
inline int kernel_variants(int T, KernelVariant* out) {
    int k = 0;
    out[k++] = cascade_variant(false); out[k++] = cascade_variant(true);
    out[k++] = cascade_variant(false, true); out[k++] = cascade_variant(false, false, true);
    if (T == 32) out[k++] = cascade_variant(true, false, true);   // PROF + BOX: compiled for the headline layout only
    out[k++] = cycle_variant(); out[k++] = cycle_variant(true); out[k++] = cycle_variant(false, true);
    for (const bool roll : {false, true}) { out[k++] = control_variant(false, false, roll); out[k++] = control_variant(true, false, roll); out[k++] = control_variant(false, true, roll); }
    return k;
}

struct LaunchFacts {
    int T, nc;                   // padded size (pick_np); constraint rows of the plan as this launch sees it (DevPlan.nc)
    bool fused, control, roll;   // the update half runs in this launch; so does the producer (osot_control.h); with the rollout loop
    bool pairs_out, prof;        // the model has collision pairs and the batch asks for their outputs; phase profiling
    bool plan_extra;             // an inactive task, a dense regularisation task or a level with a dense weight
    bool hotstart, force_extra, specialise, rows_all_equalities;   // solver state; OSOT_DEBUG_FORCE_EXTRA; osot_solver_set_specialisation; plan_rows_all_equalities
};
// -> OSOT_OK and the variant, or the refusal's code and text
inline int choose_kernel_variant(const LaunchFacts& f, KernelVariant& v, const char** why) {
    const bool hot_on = f.hotstart && !f.prof;   // (hot start: the EXTRA instantiation carries its code; never together with prof)
    // (the instrumented instantiation carries no dense-weight / inactive-task code: it would solve another problem)
    if (f.prof && !f.fused && f.plan_extra) { *why = "phase profiling is not available for plans with dense weights or inactive tasks"; return OSOT_ERR_UNSUPPORTED; }
    // the instantiation with the dense-weight / inactive-task code only where the plan or the solver state asks for it
    bool extra = f.plan_extra || hot_on;
    if (f.force_extra && !f.prof) extra = true;
    // plans without constraint rows (the bounds are the only inequalities): the BOX instantiation of the 32-column kernels
    // ... and plans whose rows are all equalities by construction (the feet as TaskToConstraint rows: the reference's COMAN stacks), at
    // every size -- but only where THIS launch's update half writes lo == up itself (fused): on the solve-only path lo / up are the
    // caller's arrays, and a row with lo < up would never be scanned by the BOX instantiation
    bool box = f.specialise && !extra && (f.nc == 0 ? f.T == 32 : (f.fused && f.rows_all_equalities));
    // the BOX instantiations of osot_control_cycle_kernel are compiled WITHOUT the collision-pair stage of the kinematics (PAIRS = !BOX):
    // a model with pairs whose batch asks for their outputs takes the general instantiation, whatever the plan's rows (such a
    // launch used to leave pair_dist / pair_J unwritten without an error)
    if (f.pairs_out) box = false;
    if (f.control && (f.prof || !f.fused)) { *why = "the fused control cycle carries no profiling code (use osot_kinematics + osot_cycle)"; return OSOT_ERR_UNSUPPORTED; }
    if (f.control) v = control_variant(extra, box, f.roll);   // (box only without extra, above)
    else if (box && (f.T == 32 || !f.prof)) v = f.fused ? cycle_variant(false, true) : cascade_variant(f.prof, false, true);
    else if (f.fused) v = cycle_variant(extra);
    else v = cascade_variant(f.prof, extra && !f.prof);
    return OSOT_OK;
}

// the static part of the update kernel's arguments (uploaded once per solver)
inline void make_update_plan(const osot_plan_desc& pl, DevUpdatePlan& U) {
    std::memset(&U, 0, sizeof(U));
    U.n = pl.n; U.L = pl.n_levels;
    plan_constraint_rows(&pl, &U.nc);
    plan_stored_constraint_rows(&pl, &U.nc_stored);
    int flat = 0;
    for (int k = 0; k < pl.n_levels; ++k) {
        plan_level_rows(&pl, k, &U.m[k], &U.ma[k]);
        int off = 0;
        for (int j = 0; j < pl.level[k].n_tasks; ++j) {
            const osot_task_desc& t = pl.level[k].task[j];
            DevTaskS& d = U.task[flat++];
            d.level = k; d.kind = t.kind; d.rows = t.rows; d.off = off;
            d.weight = t.weight; d.lambda = t.lambda; d.ogain = t.orientation_gain; d.lambda2 = t.lambda2;
            d.mask = t.row_mask; d.prow = task_parent_rows(t, pl.n); d.sublam = t.row_mask ? t.sub_lambda : 1.0;
            d.gains = t.acc_gain_matrices ? 1 : 0;
            d.body = t.body_frame; d.dense = t.dense_weight;
            if (t.dense_weight) U.dense_level[k] = 1;
            off += t.rows;
        }
    }
    if (pl.has_regularisation) {   // one more flat entry; its b goes to out->b_reg (level = -1)
        const osot_task_desc& t = pl.regularisation;
        DevTaskS& d = U.task[flat++];
        d.level = -1; d.kind = t.kind; d.rows = t.rows; d.off = 0;
        d.weight = t.weight; d.lambda = t.lambda; d.ogain = t.orientation_gain; d.lambda2 = t.lambda2;
        d.mask = 0ull; d.prow = t.rows; d.sublam = 1.0;
        d.gains = 0; d.body = 0; d.dense = 0;
    }
    U.ntasks = flat;
    {
        int fr = 0;
        for (int j = 0; j < flat; ++j)
            for (int r = 0; r < U.task[j].rows && fr < OSOT_KMAX_FLAT_ROWS; ++r, ++fr) { U.row_task[fr] = (unsigned char)j; U.row_in_task[fr] = (short)r; }
        U.total_rows = fr;
        for (int k = 0; k < pl.n_levels; ++k) if (U.dense_level[k]) U.any_dense = 1;
    }
    U.nbounds = pl.n_bounds;
    for (int j = 0; j < pl.n_bounds; ++j) {
        U.bound[j].kind = pl.bound[j].kind; U.bound[j].scaling = pl.bound[j].scaling; U.bound[j].dT = pl.bound[j].dT;
    }
    U.nrowblocks = pl.n_rowblocks;
    int roff = 0, soff = 0;
    for (int j = 0; j < pl.n_rowblocks; ++j) {
        const osot_rows_desc& r = pl.rowblock[j];
        DevRowBlockS& d = U.rowblock[j];
        d.kind = r.kind; d.rows = r.rows; d.off = roff; d.stored_off = soff; d.first_col = r.first_col;
        d.body = r.task_body_frame; d.ncand = r.n_candidates;
        d.dT = r.dT; d.p = r.p; d.mu = r.mu; d.lambda = r.task_lambda; d.ogain = r.task_orientation_gain;
        for (int i = 0; i < OSOT_MAX_BAND_ROWS; ++i) { d.err_lb[i] = r.err_lb[i]; d.err_ub[i] = r.err_ub[i]; }
        d.d_threshold = r.d_threshold; d.detection_threshold = r.detection_threshold; d.bound_scaling = r.bound_scaling;
        if (!rows_are_implicit(d.kind)) soff += d.rows;
        roff += d.rows;
    }
}

// the per-call part of the update kernel's arguments: leaf / output pointers, checked against the plan
inline int make_update_args(const osot_plan_desc& pl, const DevUpdatePlan& PL, const osot_leaf_batch* leaf,
                            const osot_assembled_out* out, const DevUpdatePlan* dev_plan, DevUpdate& U, const char** why) {
    std::memset(&U, 0, sizeof(U));
    U.B = leaf->B;
    U.plan = dev_plan;
    int flat = 0;
    for (int k = 0; k < pl.n_levels; ++k) {
        if (!out->b[k]) { *why = "out.b[k] is null"; return OSOT_ERR_INVALID; }
        U.b[k] = out->b[k]; U.w[k] = out->w[k];
        if (PL.dense_level[k]) {
            if (!out->WA[k] || !out->Wb[k] || (PL.ma[k] > 0 && !out->A[k]))
                { *why = "level has a non-diagonal weight: out.WA[k], out.Wb[k] and out.A[k] are required"; return OSOT_ERR_INVALID; }
            U.WA[k] = out->WA[k]; U.Wb[k] = out->Wb[k]; U.A[k] = out->A[k];
        }
        for (int j = 0; j < pl.level[k].n_tasks; ++j) {
            const osot_task_desc& t = pl.level[k].task[j];
            DevPtr4& d = U.task[flat++];
            d.p0 = leaf->task[k][j].p0; d.p1 = leaf->task[k][j].p1; d.p2 = leaf->task[k][j].p2; d.W = leaf->task[k][j].W;
            if (!d.p0) { *why = "leaf input p0 of a task is null"; return OSOT_ERR_INVALID; }
            if (t.kind != OSOT_TASK_GENERIC && t.kind != OSOT_TASK_ACC_POSTURAL && !d.p1)
                { *why = "leaf input p1 of a task is null"; return OSOT_ERR_INVALID; }
            if (t.dense_weight && !d.W) { *why = "task has dense_weight but its leaf W is null"; return OSOT_ERR_INVALID; }
        }
    }
    if (pl.has_regularisation) {   // one more flat entry; its b goes to out->b_reg (level = -1)
        const osot_task_desc& t = pl.regularisation;
        if (!out->b_reg) { *why = "out.b_reg is null"; return OSOT_ERR_INVALID; }
        DevPtr4& d = U.task[flat++];
        d.p0 = leaf->regularisation.p0; d.p1 = leaf->regularisation.p1; d.p2 = leaf->regularisation.p2; d.W = nullptr;
        if (!d.p0) { *why = "leaf input p0 of the regularisation task is null"; return OSOT_ERR_INVALID; }
        if (t.kind == OSOT_TASK_POSTURAL && !d.p1) { *why = "leaf input p1 of the regularisation task is null"; return OSOT_ERR_INVALID; }
        U.b_reg = out->b_reg;
    }
    for (int j = 0; j < pl.n_bounds; ++j) {
        DevPtr3& d = U.bound[j];
        const int kind = pl.bound[j].kind;
        d.p0 = leaf->bound[j].p0; d.p1 = leaf->bound[j].p1; d.p2 = leaf->bound[j].p2;
        if (!d.p0) { *why = "leaf input p0 of a bound is null"; return OSOT_ERR_INVALID; }
        if (kind == OSOT_BOUND_JOINT_LIMITS && (!d.p1 || !d.p2)) { *why = "joint limits need q, q_min, q_max"; return OSOT_ERR_INVALID; }
        if (kind == OSOT_BOUND_GENERIC && !d.p1) { *why = "generic bound needs l and u"; return OSOT_ERR_INVALID; }
        if (kind == OSOT_BOUND_JOINT_LIMITS_INVARIANCE && (!d.p1 || !d.p2))
            { *why = "joint limits invariance needs q (p0), [q_min; q_max; qddot_max] (p1) and qdot_prev (p2)"; return OSOT_ERR_INVALID; }
    }
    if (pl.n_bounds > 0 && (!out->l || !out->u)) { *why = "out.l/out.u is null"; return OSOT_ERR_INVALID; }
    U.l = out->l; U.u = out->u;
    for (int j = 0; j < pl.n_rowblocks; ++j) {
        DevPtr3& d = U.rows[j];
        const int kind = pl.rowblock[j].kind;
        d.p0 = leaf->rows[j].p0; d.p1 = leaf->rows[j].p1; d.p2 = leaf->rows[j].p2;
        if (!d.p0) { *why = "leaf input p0 of a row block is null"; return OSOT_ERR_INVALID; }
        if ((kind == OSOT_ROWS_GENERIC || kind == OSOT_ROWS_COLLISION || kind == OSOT_ROWS_TORQUE_LIMITS ||
             kind == OSOT_ROWS_ACC_JOINT_LIMITS || kind == OSOT_ROWS_ACC_VELOCITY_LIMITS ||
             kind == OSOT_ROWS_TASK_CARTESIAN || kind == OSOT_ROWS_TASK_COM || kind == OSOT_ROWS_UNIT_GENERIC) && !d.p1)
            { *why = "leaf input p1 of a row block is null"; return OSOT_ERR_INVALID; }
        if (kind == OSOT_ROWS_ACC_JOINT_LIMITS && !d.p2) { *why = "acceleration joint limits need qddot_max"; return OSOT_ERR_INVALID; }
        if (kind == OSOT_ROWS_GENERIC && !d.p2) { *why = "generic rows need C, lo, up"; return OSOT_ERR_INVALID; }
        if ((kind == OSOT_ROWS_COP || kind == OSOT_ROWS_NORMAL_TORQUE) && !d.p1)
            { *why = "CoP / normal torque rows need the contact's x / y limits (p1)"; return OSOT_ERR_INVALID; }
        if (kind == OSOT_ROWS_CONVEX_HULL && (!d.p1 || !d.p2))
            { *why = "convex hull rows need the CoM Jacobian (p0), the CoM (p1) and the contact points (p2)"; return OSOT_ERR_INVALID; }
        if ((kind == OSOT_ROWS_ACC_JOINT_LIMITS_VIABILITY || kind == OSOT_ROWS_ACC_JOINT_LIMITS_ECBF) && (!d.p1 || !d.p2))
            { *why = "viability / ECBF joint limits need [q; qdot] (p0), [q_min; q_max] (p1) and the velocity / acceleration limits (p2)"; return OSOT_ERR_INVALID; }
        if ((kind == OSOT_ROWS_POSITION_CARTESIAN || kind == OSOT_ROWS_POSITION_COM) && (!d.p1 || !d.p2))
            { *why = "Cartesian position rows need the Jacobian (p0), the pose / CoM (p1) and [A_c; b_c] (p2)"; return OSOT_ERR_INVALID; }
    }
    if (PL.nc > 0 && (!out->lo || !out->up)) { *why = "out.lo/up is null"; return OSOT_ERR_INVALID; }
    if (PL.nc_stored > 0 && !out->C) { *why = "out.C is null"; return OSOT_ERR_INVALID; }
    U.C = out->C; U.lo = out->lo; U.up = out->up;
    return OSOT_OK;
}

}  // namespace osot
