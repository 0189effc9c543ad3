// opensot_amd/csrc/osot_ihqp_sens.h -- the QP of every level of the batched iHQP cascade on the device, and from it the level's
// multipliers, active set and objective: what the reference's iHQP gives through getBackEnd(i) (iHQP.cpp:381-389: H, g, A, lA, uA,
// l, u of BackEnd.h), QPOasesBackEnd::getDualSolution / getActiveBounds / getActiveConstraints and getObjective(i).
// (include/osot_mi355x.h: osot_ihqp_level_qp and osot_ihqp_sensitivity have the contract.)
//
//   LevelPlan / LevelBatch ........ the plan shape (make_plan_shape) and the call's pointers (fill_batch_ptrs) of osot_plan_shape.h
//   level_qp_check, ihqp_sens_check  the argument checks, HIP-free: the host build runs them too
//   osot_ihqp_level_qp_kernel ..... one wavefront per instance: H, g, the row table [C; A_0 .. A_(k-1)] with its bounds, the box
//   osot_ihqp_objective_kernel .... one wavefront per instance: 1/2 x'(H + eps I)x + g'x of a materialised level (or, for a level
//                                   that is switched off, the zeros of a SKIPPED instance)
//   osot_ihqp_pullback_kernel ..... one wavefront per instance: the backward pass's link between the levels (below)
// The multipliers, and each level's KKT solve of the backward pass, are osot_qp_sens_kernel (osot_qp_sens.h), unchanged, on the
// materialised QP.  A handle of osot_solver_create_wide whose plan has 65 .. 128 variables passes the same checks and the same
// schedule (ihqp_sens_levels) with the workgroup kernels of osot_ihqp_sens_wide.h and osot_qp_sens_big_kernel; its workspace is
// ihqp_wide_workspace_bytes.  A wide handle whose plan has n <= 64 stays refused: such a plan belongs on osot_solver_create.
//
// THE ROUTE of the level kernel.  Rows are staged through LDS coalesced (lane = column) in tiles of kLevelTile rows (odd row
// stride: a lane-per-row walk at one column has no bank conflict).  H: lane = column j keeps column j of H in registers, entry
// (i, j) = sum_r L_r[max(i, j)] A_r[min(i, j)] with L_r = w_r A_r (or the row of WA): ONE product per unordered pair, so H is
// symmetric to the bit, and one fma chain over the rows in ascending order.  a_r'x_j of an optimality row: lane = row, one fma chain
// over the columns in ascending order, as osot_qp_sens_kernel forms a_r'x.  The kernel is bandwidth-shaped: it writes
// 8 (n n + rows n) bytes per instance in full 8 n-byte rows.
#pragma once
#include <cmath>
#include <osot_team.h>
#include <osot_mi355x.h>
#include "osot_plan_shape.h"
#include "osot_qp_sens.h"
#include "osot_qp_sens_big.h"   // sensbig::workspace_bytes, slots: the wide route's share of the workspace

namespace osot {

// the members make_plan_shape writes
struct LevelPlan {
    int n, L, nc, nc_stored, nblocks;
    int m[OSOT_KMAX_LEVELS], ma[OSOT_KMAX_LEVELS], optoff[OSOT_KMAX_LEVELS + 1];
    int blk_rows[OSOT_KMAX_ROWBLOCKS], blk_off[OSOT_KMAX_ROWBLOCKS], blk_stored_off[OSOT_KMAX_ROWBLOCKS];
    int blk_implicit[OSOT_KMAX_ROWBLOCKS], blk_first_col[OSOT_KMAX_ROWBLOCKS], blk_level[OSOT_KMAX_ROWBLOCKS];
    int ntask[OSOT_KMAX_LEVELS], task_off[OSOT_KMAX_LEVELS][OSOT_KMAX_TASKS + 1];
    unsigned inactive[OSOT_KMAX_LEVELS], active_mask;
    int max_iter, reg_rows, reg_dense;
    double eps_abs, reg_w;
};
// the members fill_batch_ptrs writes
struct LevelBatch {
    int B;
    const double *A[OSOT_KMAX_LEVELS], *b[OSOT_KMAX_LEVELS], *w[OSOT_KMAX_LEVELS], *c[OSOT_KMAX_LEVELS], *WA[OSOT_KMAX_LEVELS], *Wb[OSOT_KMAX_LEVELS];
    const double *C, *lo, *up, *l, *u, *b_reg, *A_reg;
    double *dq, *x_levels, *accepted_slack;
    int *status, *iterations;
};
struct LevelQpArgs {
    LevelPlan P;
    LevelBatch D;
    int level;
    osot_level_qp out;
    double* x_out;          // [B][n] x_levels[.][level] contiguous, for osot_qp_sens_kernel (null: not wanted)
};
struct ObjectiveArgs {
    int B, n, L, level, rows;
    int level_off;          // 1: the level is switched off -- y, active, flag, objective of a SKIPPED instance are written, nothing is read
    const double *H, *g, *x;
    double eps_abs;
    const int* status;
    double* objective;      // [B][L] or null
    double* y; int* active; int* flag;   // level_off only; any may be null
};
static_assert(std::is_trivially_copyable<LevelQpArgs>::value && std::is_trivially_copyable<ObjectiveArgs>::value, "kernel arguments");

constexpr int kLevelTile = 32;   // rows of a staged tile
inline int level_qp_lds_bytes(int n) { return (2 * kLevelTile * (n | 1) + n) * (int)sizeof(double); }   // 33 792 bytes at n = 64

__host__ __device__ inline int level_qp_rows(const LevelPlan& P, int level) { return P.nc + P.optoff[level]; }
__host__ __device__ inline double level_clamp(double v) { return v < -1e20 ? -1e20 : (v > 1e20 ? 1e20 : v); }
// row r of level k belongs to a task that Task::setActive(false) switched off
__host__ __device__ inline bool level_row_off(const LevelPlan& P, int k, int r) {
    const unsigned inact = P.inactive[k];
    bool off = false;
    if (inact)
        for (int j = 0; j < P.ntask[k]; ++j) off = off || (((inact >> j) & 1u) && r >= P.task_off[k][j] && r < P.task_off[k][j + 1]);
    return off;
}


// the workspace of osot_ihqp_sensitivity for B instances: offsets in doubles.  back: dx, the QP's bound gradients and gx [L][B][n]
// (one [B][n] slice per level: osot_qp_sens_kernel takes grad_x contiguous); grad_A: the QP's grad_A
struct IhqpSensWorkspace { long long H, g, A, lA, uA, l, u, x, flag, dx, glA, guA, gl, gu, gx, gA, total; };
inline IhqpSensWorkspace ihqp_sens_workspace(const LevelPlan& P, long long B, bool back = false, bool grad_A = false) {
    IhqpSensWorkspace W;
    const long long n = P.n, rows = level_qp_rows(P, P.L - 1);
    W.H = 0; W.g = W.H + B * n * n; W.A = W.g + B * n; W.lA = W.A + B * rows * n; W.uA = W.lA + B * rows;
    W.l = W.uA + B * rows; W.u = W.l + B * n; W.x = W.u + B * n; W.flag = W.x + B * n;
    W.dx = W.flag + (B + 1) / 2;
    W.glA = W.dx + (back ? B * n : 0); W.guA = W.glA + (back ? B * rows : 0); W.gl = W.guA + (back ? B * rows : 0);
    W.gu = W.gl + (back ? B * n : 0); W.gx = W.gu + (back ? B * n : 0); W.gA = W.gx + (back ? P.L * B * n : 0);
    W.total = W.gA + ((back && grad_A) ? B * rows * n : 0);
    return W;
}

// The workspace of osot_ihqp_sensitivity on a wide handle, in bytes: the arrays of ihqp_sens_workspace (the level QP, x, the flags,
// with grad_dq the level's gradients), rounded up to 16 bytes, then the Y slices of osot_qp_sens_big_kernel,
// sensbig::workspace_bytes(B, n, rows of the last level) -- min(B, slots(n, rows_last)) slices of n (2n + 2) doubles.  The last level
// has the most rows, hence the largest LDS block and the fewest slots: every level is launched with that many workgroups.
inline unsigned long long ihqp_wide_front_bytes(const LevelPlan& P, long long B, bool back, bool grad_A) {
    return (((unsigned long long)ihqp_sens_workspace(P, B, back, grad_A).total * sizeof(double)) + 15ull) & ~15ull;
}
inline unsigned long long ihqp_wide_workspace_bytes(const LevelPlan& P, long long B, bool back, bool grad_A) {
    return ihqp_wide_front_bytes(P, B, back, grad_A) + (unsigned long long)sensbig::workspace_bytes((int)B, P.n, level_qp_rows(P, P.L - 1));
}
// workgroups of every osot_qp_sens_big_kernel launch of a call
inline int ihqp_wide_sens_grid(const LevelPlan& P, int B) {
    const int s = sensbig::slots(P.n, level_qp_rows(P, P.L - 1));
    return B < s ? B : s;
}

// the gradient outputs of a call (osot_ihqp_sens_batch's)
struct IhqpGrads { double *b[OSOT_KMAX_LEVELS], *w[OSOT_KMAX_LEVELS], *c[OSOT_KMAX_LEVELS], *A[OSOT_KMAX_LEVELS], *C, *lo, *up, *l, *u; };
struct PullbackArgs {
    LevelPlan P;
    LevelBatch D;
    int level;
    const double *dx, *glA, *guA, *gl, *gu, *gA;   // of the level's QP: [B][n], [B][rows_k] x 2, [B][n] x 2, [B][rows_k][n] or null
    double* gx;                                    // [L][B][n]
    const int* flag;                               // [B] OSOT_SENS_* of the level's multiplier launch: a SKIPPED instance is left alone
    IhqpGrads G;
};
static_assert(std::is_trivially_copyable<PullbackArgs>::value, "kernel arguments");
inline int pullback_lds_bytes(int n) { return (kLevelTile * (n | 1) + 2 * n + 2 * kLevelTile) * (int)sizeof(double); }

inline IhqpGrads ihqp_grads(const osot_ihqp_sens_batch& b) {
    IhqpGrads G;
    for (int k = 0; k < OSOT_KMAX_LEVELS; ++k) { G.b[k] = b.grad_b[k]; G.w[k] = b.grad_w[k]; G.c[k] = b.grad_c[k]; G.A[k] = b.grad_A[k]; }
    G.C = b.grad_C; G.lo = b.grad_lo; G.up = b.grad_up; G.l = b.grad_l; G.u = b.grad_u;
    return G;
}
inline bool ihqp_wants_grad_A(const osot_ihqp_sens_batch& b, int L) {
    bool w = b.grad_C != nullptr;
    for (int k = 0; k < L; ++k) w = w || b.grad_A[k] != nullptr;
    return w;
}

// task_active: the handle's Task::setActive flags (null: all active), as make_plan_shape takes them
inline int level_qp_check(const osot_plan_desc& plan, int wide, int max_batch, const unsigned char* task_active, const osot_qp_batch* b, int level,
                          const osot_level_qp* out, LevelQpArgs& Q, const char** why) {
    if (wide && plan.n <= OSOT_MAX_VARS) { *why = "the level QPs are built for handles of osot_solver_create (one wavefront per instance, n <= 64), not for the wide route"; return OSOT_ERR_UNSUPPORTED; }
    if (!b || !out) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (level < 0 || level >= plan.n_levels) { *why = "level out of range"; return OSOT_ERR_INVALID; }
    if (b->B < 0 || b->B > max_batch) { *why = "batch size exceeds max_batch"; return OSOT_ERR_INVALID; }
    if (!out->H || !out->g || !out->A || !out->lA || !out->uA || !out->l || !out->u) { *why = "a member of the output is null"; return OSOT_ERR_INVALID; }
    make_plan_shape(plan, b->level_active, task_active, Q.P);
    std::memset(&Q.D, 0, sizeof(Q.D));
    const int rc = fill_batch_ptrs(plan, Q.P, *b, Q.D, why);
    if (rc != OSOT_OK) return rc;
    if (level > 0 && !b->x_levels) { *why = "x_levels is null"; return OSOT_ERR_INVALID; }
    Q.level = level;
    Q.out = *out;
    Q.x_out = nullptr;
    return OSOT_OK;
}

// the checks of osot_ihqp_sensitivity; Q receives the plan shape's batch pointers
inline int ihqp_sens_check(const osot_plan_desc& plan, int wide, int max_batch, const unsigned char* task_active, const osot_ihqp_sens_batch* b,
                           const osot_qp_sens_options* o, LevelQpArgs& Q, const char** why) {
    if (wide && plan.n <= OSOT_MAX_VARS) { *why = "per-level multipliers are built for handles of osot_solver_create (one wavefront per instance, n <= 64), not for the wide route"; return OSOT_ERR_UNSUPPORTED; }
    if (!b) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (b->qp.B < 0 || b->qp.B > max_batch) { *why = "batch size exceeds max_batch"; return OSOT_ERR_INVALID; }
    if (o) {
        const double t[3] = {o->active_tol, o->dual_tol, o->rank_tol};
        for (double v : t) if (!(v >= 0.0) || !sens_finite(v)) { *why = "a tolerance is negative or not finite"; return OSOT_ERR_INVALID; }
    }
    const osot_qp_batch& q = b->qp;
    const int L = plan.n_levels;
    // the outputs, each with the first address alone (their sizes depend on the plan; the workspace's range is known)
    const void* outp[6 + 7 * OSOT_MAX_LEVELS] = {b->objective, b->grad_C, b->grad_lo, b->grad_up, b->grad_l, b->grad_u};
    int no = 6;
    for (int k = 0; k < L; ++k) {
        outp[no++] = b->y[k]; outp[no++] = b->active[k]; outp[no++] = b->flag[k];
        outp[no++] = b->grad_b[k]; outp[no++] = b->grad_w[k]; outp[no++] = b->grad_c[k]; outp[no++] = b->grad_A[k];
    }
    bool any_grad = false;
    for (int a = 1; a < 6; ++a) any_grad = any_grad || outp[a];
    for (int k = 0; k < L; ++k) any_grad = any_grad || b->grad_b[k] || b->grad_w[k] || b->grad_c[k] || b->grad_A[k];
    if (any_grad && !b->grad_dq) { *why = "a gradient output without grad_dq"; return OSOT_ERR_INVALID; }
    if (b->grad_dq) {
        bool dense = false;
        for (int k = 0; k < L; ++k) dense = dense || level_has_dense_weight(plan.level[k]);
        if (dense) { *why = "the backward pass is not built for plans with a dense-weight level (forward works for them)"; return OSOT_ERR_UNSUPPORTED; }
        if (plan.has_regularisation) { *why = "the backward pass is not built for plans with a regularisation task (forward works for them)"; return OSOT_ERR_UNSUPPORTED; }
    }
    make_plan_shape(plan, q.level_active, task_active, Q.P);
    std::memset(&Q.D, 0, sizeof(Q.D));
    const int rc = fill_batch_ptrs(plan, Q.P, q, Q.D, why);
    if (rc != OSOT_OK) return rc;
    if (!q.x_levels || !q.status) { *why = "x_levels / status of the solve is null"; return OSOT_ERR_INVALID; }
    if (!b->workspace) { *why = "workspace is null"; return OSOT_ERR_INVALID; }
    const unsigned long long need = wide ? ihqp_wide_workspace_bytes(Q.P, q.B, b->grad_dq != nullptr, ihqp_wants_grad_A(*b, L))
                                         : (unsigned long long)ihqp_sens_workspace(Q.P, q.B, b->grad_dq != nullptr, ihqp_wants_grad_A(*b, L)).total * sizeof(double);
    if (b->workspace_bytes < need) { *why = "workspace is smaller than osot_ihqp_sens_workspace_bytes"; return OSOT_ERR_INVALID; }
    if (!wide && reinterpret_cast<unsigned long long>(b->workspace) % sizeof(double)) { *why = "workspace is not 8-byte aligned"; return OSOT_ERR_INVALID; }
    if (wide && reinterpret_cast<unsigned long long>(b->workspace) % 16) { *why = "workspace is not 16-byte aligned"; return OSOT_ERR_INVALID; }
    const void* in[16 + 6 * OSOT_MAX_LEVELS] = {q.C, q.lo, q.up, q.l, q.u, q.dq, q.x_levels, q.status, q.iterations, q.b_reg, q.accepted_slack, q.A_reg, b->grad_dq};
    int ni = 13;
    for (int k = 0; k < L; ++k) { in[ni++] = q.A[k]; in[ni++] = q.b[k]; in[ni++] = q.w[k]; in[ni++] = q.c[k]; in[ni++] = q.WA[k]; in[ni++] = q.Wb[k]; }
    const char* w0 = static_cast<const char*>(b->workspace);
    const char* w1 = w0 + b->workspace_bytes;
    auto in_workspace = [&](const void* p) { return p && static_cast<const char*>(p) >= w0 && static_cast<const char*>(p) < w1; };
    for (int i = 0; i < ni; ++i) if (in_workspace(in[i])) { *why = "an input lies inside the workspace"; return OSOT_ERR_INVALID; }
    for (int a = 0; a < no; ++a) {
        if (!outp[a]) continue;
        if (in_workspace(outp[a])) { *why = "an output lies inside the workspace"; return OSOT_ERR_INVALID; }
        for (int i = 0; i < ni; ++i) if (outp[a] == in[i]) { *why = "an output aliases an input"; return OSOT_ERR_INVALID; }
        for (int c = 0; c < a; ++c) if (outp[a] == outp[c]) { *why = "two outputs alias"; return OSOT_ERR_INVALID; }
    }
    return OSOT_OK;
}

// The launches of osot_ihqp_sensitivity on a checked batch (Q: from ihqp_sens_check), from the last level down: the level QP into
// the workspace, the multipliers (with grad_dq: and the level's KKT solve for gx_k), the objective, with grad_dq the pull-back.
// go.level_qp(Q), go.sens(S) -> code, go.objective(O), go.pullback(R) launch the kernels, go.zero(p, bytes) and go.copy(dst, src,
// bytes) are stream-ordered fills and copies (the device library on a stream, the host build through the emulation).  The zero
// fill of the accumulating outputs and the accumulation are separate operations on the stream: no fence inside a kernel.
template <class Launch>
inline int ihqp_sens_levels(LevelQpArgs& Q, const osot_ihqp_sens_batch* b, Launch&& go) {
    const int B = b->qp.B, n = Q.P.n, L = Q.P.L;
    const bool back = b->grad_dq != nullptr, want_A = ihqp_wants_grad_A(*b, L);
    double* ws = static_cast<double*>(b->workspace);
    const IhqpSensWorkspace W = ihqp_sens_workspace(Q.P, B, back, want_A);
    Q.out = osot_level_qp{ws + W.H, ws + W.g, ws + W.A, ws + W.lA, ws + W.uA, ws + W.l, ws + W.u};
    Q.x_out = ws + W.x;
    const size_t vec = (size_t)B * n * sizeof(double);
    if (back) {
        const IhqpGrads G = ihqp_grads(*b);
        for (int k = 0; k < L; ++k) {
            if (G.b[k]) go.zero(G.b[k], (size_t)B * Q.P.m[k] * sizeof(double));
            if (G.w[k]) go.zero(G.w[k], (size_t)B * Q.P.m[k] * sizeof(double));
            if (G.c[k]) go.zero(G.c[k], vec);
            if (G.A[k]) go.zero(G.A[k], vec * Q.P.ma[k]);
        }
        if (G.C) go.zero(G.C, vec * Q.P.nc_stored);
        if (G.lo) go.zero(G.lo, (size_t)B * Q.P.nc * sizeof(double));
        if (G.up) go.zero(G.up, (size_t)B * Q.P.nc * sizeof(double));
        if (G.l) go.zero(G.l, vec);
        if (G.u) go.zero(G.u, vec);
        go.zero(ws + W.gx, vec * L);
        for (int k = L - 1; k >= 0; --k)
            if ((Q.P.active_mask >> k) & 1u) { go.copy(ws + W.gx + (long long)k * B * n, b->grad_dq, vec); break; }
    }
    for (int k = L - 1; k >= 0; --k) {
        const int rows = level_qp_rows(Q.P, k);
        ObjectiveArgs O;
        std::memset(&O, 0, sizeof(O));
        O.B = B; O.n = n; O.L = L; O.level = k; O.rows = rows; O.eps_abs = Q.P.eps_abs;
        O.H = Q.out.H; O.g = Q.out.g; O.x = Q.x_out; O.status = b->qp.status; O.objective = b->objective;
        O.level_off = ((Q.P.active_mask >> k) & 1u) ? 0 : 1;
        if (O.level_off) {
            O.y = b->y[k]; O.active = b->active[k]; O.flag = b->flag[k];
            if (O.y || O.active || O.flag || O.objective) go.objective(O);
            continue;
        }
        Q.level = k;
        go.level_qp(Q);
        osot_qp_sens_batch S;
        std::memset(&S, 0, sizeof(S));
        S.B = B; S.n = n; S.nc = rows; S.H = Q.out.H; S.g = Q.out.g; S.l = Q.out.l; S.u = Q.out.u; S.eps_abs = Q.P.eps_abs;
        if (rows > 0) { S.A = Q.out.A; S.lA = Q.out.lA; S.uA = Q.out.uA; }
        S.x = Q.x_out; S.status = b->qp.status; S.y = b->y[k]; S.active = b->active[k];
        S.flag = b->flag[k] ? b->flag[k] : reinterpret_cast<int*>(ws + W.flag);
        if (back) {      // only what the pull-back reads; never grad_H (sym(dx x'): n^2 per instance for nothing)
            S.grad_x = ws + W.gx + (long long)k * B * n;
            S.grad_g = ws + W.dx; S.grad_l = ws + W.gl; S.grad_u = ws + W.gu;
            if (rows > 0) { S.grad_lA = ws + W.glA; S.grad_uA = ws + W.guA; if (want_A) S.grad_A = ws + W.gA; }
        }
        if (const int r = go.sens(S)) return r;
        if (O.objective) go.objective(O);
        if (back) {
            PullbackArgs R;
            std::memset(&R, 0, sizeof(R));
            R.P = Q.P; R.D = Q.D; R.level = k;
            R.dx = S.grad_g; R.glA = S.grad_lA; R.guA = S.grad_uA; R.gl = S.grad_l; R.gu = S.grad_u; R.gA = S.grad_A;
            R.gx = ws + W.gx; R.flag = S.flag; R.G = ihqp_grads(*b);
            go.pullback(R);
        }
    }
    return OSOT_OK;
}

template <int NP>
__global__ void __launch_bounds__(64) osot_ihqp_level_qp_kernel(const LevelQpArgs A_) {
    OSOT_DYNAMIC_LDS(level_smem);                              // level_qp_lds_bytes(n)
    const LevelQpArgs* Q = OSOT_KERNARG_PTR(LevelQpArgs, A_);
    const LevelPlan& P = Q->P;
    const LevelBatch& D = Q->D;
    const long long inst = blockIdx.x;
    const int lane = threadIdx.x;
    if (inst >= D.B) return;
    const int n = P.n < NP ? P.n : NP;                         // (n <= NP by the launch layer)
    const int k = Q->level, ld = n | 1;
    const bool col = lane < n;
    double* At = reinterpret_cast<double*>(level_smem);        // the tile of A (right operand; the rows whose a'x is formed)
    double* Lt = At + kLevelTile * ld;                         // the tile of W A (left operand)
    double* xs = Lt + kLevelTile * ld;
    const osot_level_qp& O = Q->out;

    // ---- 1. H and g: column `lane` of H in registers
    double acc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) acc[i] = 0.0;
    double gacc = 0.0;
    const int m = P.m[k], ma = P.ma[k];
    // Ar: count rows [.][n]; left operand: the rows of Wr (non-diagonal weight) or wv[r] * Ar (wv null: ws); right-hand side bv
    // (for a non-diagonal weight: W b); lvl >= 0: the rows of that level's inactive tasks count as zero rows
    auto add_rows = [&](const double* Ar, const double* Wr, const double* wv, double ws, const double* bv, int count, int lvl) {
        for (int r0 = 0; r0 < count; r0 += kLevelTile) {
            const int rows = count - r0 < kLevelTile ? count - r0 : kLevelTile;
            for (int rr = 0; rr < rows; ++rr) {
                const int r = r0 + rr;
                const bool off = lvl >= 0 && level_row_off(P, lvl, r);
                if (col) {
                    const double a = off ? 0.0 : Ar[(long long)r * n + lane];
                    const double l = Wr ? (off ? 0.0 : Wr[(long long)r * n + lane]) : (wv ? wv[r] : ws) * a;
                    At[rr * ld + lane] = a;
                    Lt[rr * ld + lane] = l;
                    gacc = fma(Wr ? -a : -l, bv[r], gacc);
                }
            }
            wave_sync();
            if (col)
                for (int rr = 0; rr < rows; ++rr) {
                    const double a = At[rr * ld + lane], l = Lt[rr * ld + lane];
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        if (i < n) acc[i] = (lane >= i) ? fma(l, At[rr * ld + i], acc[i]) : fma(Lt[rr * ld + i], a, acc[i]);
                }
            wave_sync();
        }
    };
    const double* bk = D.b[k] + inst * m;
    const double* wk = D.w[k] ? D.w[k] + inst * m : nullptr;
    if (ma > 0)
        add_rows(D.A[k] + inst * ma * n, D.WA[k] ? D.WA[k] + inst * ma * n : nullptr, wk, 1.0, D.WA[k] ? D.Wb[k] + inst * m : bk, ma, k);
    if (D.b_reg && P.reg_dense)
        add_rows(D.A_reg + inst * (long long)P.reg_rows * n, nullptr, nullptr, P.reg_w, D.b_reg + inst * P.reg_rows, P.reg_rows, -1);
    // the diagonal: the implicit Postural block A = [I 0] and an identity-Jacobian regularisation task
    double dv = 0.0, g = gacc;
    if (col) {
        const int npost = m - ma;
        if (lane < npost) {
            const double wp = level_row_off(P, k, ma + lane) ? 0.0 : (wk ? wk[ma + lane] : 1.0);
            dv = wp;
            g = fma(-wp, bk[ma + lane], g);
        }
        if (D.b_reg && !P.reg_dense && lane < P.reg_rows) {
            dv += P.reg_w;
            g = fma(-P.reg_w, D.b_reg[inst * P.reg_rows + lane], g);
        }
        if (D.c[k]) g += D.c[k][inst * n + lane];
        O.g[inst * n + lane] = g;
        O.l[inst * n + lane] = D.l ? level_clamp(D.l[inst * n + lane]) : -1e20;
        O.u[inst * n + lane] = D.u ? level_clamp(D.u[inst * n + lane]) : 1e20;
        if (Q->x_out) Q->x_out[inst * n + lane] = D.x_levels[(inst * P.L + k) * n + lane];
        double* Ho = O.H + inst * n * n;
#pragma unroll
        for (int i = 0; i < NP; ++i)
            if (i < n) Ho[i * n + lane] = acc[i] + (i == lane ? dv : 0.0);
    }

    // ---- 2. the global rows, in plan order
    const long long rows_k = level_qp_rows(P, k);
    double* Ao = O.A + inst * rows_k * n;
    double* lAo = O.lA + inst * rows_k;
    double* uAo = O.uA + inst * rows_k;
    for (int j = 0; j < P.nblocks; ++j) {
        const bool on = P.blk_level[j] == 0 || P.blk_level[j] - 1 == k;     // a task-local block is absent at a foreign level
        const int r0 = P.blk_off[j];
        for (int q = 0; q < P.blk_rows[j]; ++q) {
            if (!col) continue;
            double v = 0.0;
            if (on) v = P.blk_implicit[j] ? (lane == P.blk_first_col[j] + q ? 1.0 : 0.0)
                                          : D.C[(inst * P.nc_stored + P.blk_stored_off[j] + q) * n + lane];
            Ao[(long long)(r0 + q) * n + lane] = v;
        }
        for (int q = lane; q < P.blk_rows[j]; q += 64) {
            lAo[r0 + q] = on ? level_clamp(D.lo[inst * P.nc + r0 + q]) : -1e20;
            uAo[r0 + q] = on ? level_clamp(D.up[inst * P.nc + r0 + q]) : 1e20;
        }
    }

    // ---- 3. the optimality rows of the levels above: A_j x = A_j x_j
    for (int j = 0; j < k; ++j) {
        const int off = P.nc + P.optoff[j], mj = P.m[j], maj = P.ma[j];
        if (!((P.active_mask >> j) & 1u)) {        // a level that is switched off: 0 x in [-1, 1] (iHQP.cpp:301-309)
            for (int q = 0; q < mj; ++q) if (col) Ao[(long long)(off + q) * n + lane] = 0.0;
            for (int q = lane; q < mj; q += 64) { lAo[off + q] = -1.0; uAo[off + q] = 1.0; }
            continue;
        }
        wave_sync();                               // (everybody has read the previous level's xs)
        if (col) xs[lane] = D.x_levels[(inst * P.L + j) * n + lane];
        const double* Aj = maj > 0 ? D.A[j] + inst * maj * n : nullptr;
        for (int r0 = 0; r0 < maj; r0 += kLevelTile) {
            const int rows = maj - r0 < kLevelTile ? maj - r0 : kLevelTile;
            for (int rr = 0; rr < rows; ++rr) {
                if (!col) continue;
                const double a = level_row_off(P, j, r0 + rr) ? 0.0 : Aj[(long long)(r0 + rr) * n + lane];
                At[rr * ld + lane] = a;
                Ao[(long long)(off + r0 + rr) * n + lane] = a;
            }
            wave_sync();
            if (lane < rows) {
                double ax = 0.0;
                for (int c = 0; c < n; ++c) ax = fma(At[lane * ld + c], xs[c], ax);
                const bool v = level_row_off(P, j, r0 + lane);          // an inactive task: no row
                lAo[off + r0 + lane] = v ? -1e20 : ax;
                uAo[off + r0 + lane] = v ? 1e20 : ax;
            }
            wave_sync();
        }
        for (int q = maj; q < mj; ++q) {           // the implicit Postural block: e_(q - ma) x = x_j[q - ma]
            const bool v = level_row_off(P, j, q);
            if (col) Ao[(long long)(off + q) * n + lane] = (!v && lane == q - maj) ? 1.0 : 0.0;
        }
        for (int q = maj + lane; q < mj; q += 64) {
            const bool v = level_row_off(P, j, q);
            lAo[off + q] = v ? -1e20 : xs[q - maj];
            uAo[off + q] = v ? 1e20 : xs[q - maj];
        }
    }
}

// objective[inst][level] = 1/2 x'(H + eps I)x + g'x: lane = column j forms (H x)_j as one fma chain over the rows (H is symmetric
// to the bit), the n terms are added in ascending order by one lane
__global__ void __launch_bounds__(64) osot_ihqp_objective_kernel(const ObjectiveArgs A_) {
    OSOT_DYNAMIC_LDS(obj_smem);                                // n doubles
    const ObjectiveArgs* Q = OSOT_KERNARG_PTR(ObjectiveArgs, A_);
    const long long inst = blockIdx.x;
    const int lane = threadIdx.x;
    if (inst >= Q->B) return;
    const int n = Q->n;
    if (Q->level_off) {
        const long long mt = n + Q->rows;
        for (long long e = lane; e < mt; e += 64) {
            if (Q->y) Q->y[inst * mt + e] = 0.0;
            if (Q->active) Q->active[inst * mt + e] = 0;
        }
        if (lane == 0) {
            if (Q->flag) Q->flag[inst] = OSOT_SENS_SKIPPED;
            if (Q->objective) Q->objective[inst * Q->L + Q->level] = 0.0;
        }
        return;
    }
    if (!Q->objective) return;
    double* term = reinterpret_cast<double*>(obj_smem);
    const bool solved = Q->status[inst] == OSOT_STATUS_SOLVED;
    if (solved && lane < n) {
        const double* H = Q->H + inst * n * n;
        const double* x = Q->x + inst * n;
        double hx = 0.0;
        for (int i = 0; i < n; ++i) hx = fma(H[i * n + lane], x[i], hx);
        hx = fma(Q->eps_abs, x[lane], hx);
        term[lane] = x[lane] * fma(0.5, hx, Q->g[inst * n + lane]);
    }
    wave_sync();
    if (lane == 0) {
        double f = 0.0;
        if (solved) for (int i = 0; i < n; ++i) f += term[i];
        Q->objective[inst * Q->L + Q->level] = sens_finite(f) ? f : 0.0;
    }
}

// The pull-back of level k: from dx = the level QP's grad_g and its bound / row gradients to the gradients of the cascade's own
// inputs and to gx_j of the levels above (include/osot_mi355x.h has the formulas).  One wavefront per instance; every output of an
// instance is owned by its wavefront and was zeroed before the first pull-back of the call, so the sums are plain read-add-writes.
// Rows are staged as in the level kernel; s_r = a_r'x_k and t_r = a_r'dx are one fma chain each over the columns, lane = row.
__global__ void __launch_bounds__(64) osot_ihqp_pullback_kernel(const PullbackArgs A_) {
    OSOT_DYNAMIC_LDS(pull_smem);                               // pullback_lds_bytes(n)
    const PullbackArgs* Q = OSOT_KERNARG_PTR(PullbackArgs, A_);
    const LevelPlan& P = Q->P;
    const LevelBatch& D = Q->D;
    const IhqpGrads& G = Q->G;
    const long long inst = blockIdx.x;
    const int lane = threadIdx.x;
    if (inst >= D.B) return;
    // not solved, x not finite or H~ not positive definite: the level's gradients are zeros (the fill), and x_k may hold anything
    if (Q->flag[inst] == OSOT_SENS_SKIPPED) return;
    const int n = P.n, k = Q->level, ld = n | 1;
    const bool col = lane < n;
    double* At = reinterpret_cast<double*>(pull_smem);
    double* xs = At + kLevelTile * ld;
    double* dxs = xs + n;
    double* sv = dxs + n;               // w_r (s_r - b_r) of the tile's rows
    double* tv = sv + kLevelTile;       // w_r t_r
    if (col) { xs[lane] = D.x_levels[(inst * P.L + k) * n + lane]; dxs[lane] = Q->dx[inst * n + lane]; }
    wave_sync();

    // ---- 1. the cost of level k
    const int m = P.m[k], ma = P.ma[k];
    const double* bk = D.b[k] + inst * m;
    const double* wk = D.w[k] ? D.w[k] + inst * m : nullptr;
    const double* Ak = ma > 0 ? D.A[k] + inst * ma * n : nullptr;
    for (int r0 = 0; r0 < ma; r0 += kLevelTile) {
        const int rows = ma - r0 < kLevelTile ? ma - r0 : kLevelTile;
        for (int rr = 0; rr < rows; ++rr)
            if (col) At[rr * ld + lane] = level_row_off(P, k, r0 + rr) ? 0.0 : Ak[(long long)(r0 + rr) * n + lane];
        wave_sync();
        if (lane < rows) {
            const int r = r0 + lane;
            double s = 0.0, t = 0.0;
            for (int c = 0; c < n; ++c) { const double a = At[lane * ld + c]; s = fma(a, xs[c], s); t = fma(a, dxs[c], t); }
            const bool off = level_row_off(P, k, r);
            const double w = off ? 0.0 : (wk ? wk[r] : 1.0), e = s - bk[r];
            sv[lane] = w * e; tv[lane] = w * t;
            if (G.b[k]) G.b[k][inst * m + r] = -(w * t);
            if (G.w[k]) G.w[k][inst * m + r] = off ? 0.0 : t * e;
        }
        wave_sync();
        if (G.A[k] && col)
            for (int rr = 0; rr < rows; ++rr) {
                double* ga = G.A[k] + (inst * ma + r0 + rr) * n + lane;
                *ga += fma(sv[rr], dxs[lane], tv[rr] * xs[lane]);
            }
        wave_sync();
    }
    for (int q = ma + lane; q < m; q += 64) {       // the implicit Postural block: s = x_k[i], t = dx[i]
        const int i = q - ma;
        const bool off = level_row_off(P, k, q);
        const double w = off ? 0.0 : (wk ? wk[q] : 1.0), e = xs[i] - bk[q], t = dxs[i];
        if (G.b[k]) G.b[k][inst * m + q] = -(w * t);
        if (G.w[k]) G.w[k][inst * m + q] = off ? 0.0 : t * e;
    }
    if (G.c[k] && col) G.c[k][inst * n + lane] = dxs[lane];

    // ---- 2. the global rows and the box
    const long long rows_k = level_qp_rows(P, k);
    const double* glA = Q->glA ? Q->glA + inst * rows_k : nullptr;
    const double* guA = Q->guA ? Q->guA + inst * rows_k : nullptr;
    const double* gA = Q->gA ? Q->gA + inst * rows_k * n : nullptr;
    for (int q = lane; q < P.nc; q += 64) {
        if (G.lo) G.lo[inst * P.nc + q] += glA[q];
        if (G.up) G.up[inst * P.nc + q] += guA[q];
    }
    if (G.C && gA && col)
        for (int j = 0; j < P.nblocks; ++j) {
            if (P.blk_implicit[j]) continue;
            for (int q = 0; q < P.blk_rows[j]; ++q)
                G.C[(inst * P.nc_stored + P.blk_stored_off[j] + q) * n + lane] += gA[(long long)(P.blk_off[j] + q) * n + lane];
        }
    if (col) {
        if (G.l) G.l[inst * n + lane] += Q->gl[inst * n + lane];
        if (G.u) G.u[inst * n + lane] += Q->gu[inst * n + lane];
    }

    // ---- 3. the optimality blocks of the levels above: gx_j += A_j' rho, grad_A[j] += grad_A_qp + rho x_j'
    for (int j = 0; j < k; ++j) {
        if (!((P.active_mask >> j) & 1u)) continue;
        const int off = P.nc + P.optoff[j], mj = P.m[j], maj = P.ma[j];
        wave_sync();                                           // (everybody has read the previous xs)
        if (col) xs[lane] = D.x_levels[(inst * P.L + j) * n + lane];
        wave_sync();
        const double* Aj = maj > 0 ? D.A[j] + inst * maj * n : nullptr;
        double acc = 0.0;
        if (col) {
            for (int q = 0; q < maj; ++q) {
                if (level_row_off(P, j, q)) continue;          // an inactive task: a void row
                const double rho = glA[off + q] + guA[off + q];
                acc = fma(Aj[(long long)q * n + lane], rho, acc);
                if (G.A[j]) {
                    double* ga = G.A[j] + (inst * maj + q) * n + lane;
                    *ga += fma(rho, xs[lane], gA[(long long)(off + q) * n + lane]);
                }
            }
            if (lane < mj - maj && !level_row_off(P, j, maj + lane)) acc += glA[off + maj + lane] + guA[off + maj + lane];
            Q->gx[((long long)j * D.B + inst) * n + lane] += acc;
        }
    }
}

}  // namespace osot
