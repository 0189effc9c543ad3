// opensot_amd/csrc/osot_cascade_wide.h -- Solver::solve() = iHQP::solve (src/solvers/iHQP.cpp:263-358) for plans of 1 .. 128
// variables: the cascade of osot_kernels.h (cascade_body) on the workgroup solver of osot_qp_big.h.  What osot_solver_create_wide
// builds and osot_ihqp_solve / osot_cycle run on a wide handle.
//
// One 256-thread WORKGROUP per instance; a launch of G workgroups (G = what the device holds at once) walks the batch with stride G,
// each workgroup on its own slice of the solver's workspace (2 n^2 doubles: L and J of osot_qp_big.h), allocated once with the solver.
// Per active level k, in the same launch:
//   1. the cost H_k = A_k'(W_k A_k) + implicit Postural diagonal + regularisation + (eps I, added by big::solve), lower triangle,
//      written straight into the slot's L; g_k = -A_k'(W_k b_k) + c_k (+ g_r) in LDS.  Rows of A_k are staged kStage at a time in LDS
//      (coalesced loads), every thread accumulates its elements of the packed lower triangle (v_fma_f64).
//   2. the constraint rows are a TABLE in LDS (bounds, row address or unit-row code, optimality flag), as the wavefront kernel's rptr:
//      global rows, this level's task-local rows (absent = infinite bounds at the other levels), the optimality rows A_j x = A_j x_j of
//      every active level j < k (an implicit Postural block gives unit rows; an inactive task void rows; iHQP.cpp:164-170, 282-333).
//      Optimality rows are taken relative to the previous level's solution x_prev: a'(x - x_prev) = 0 (x_prev satisfies a'x = a'x_j).
//   3. big::solve with the table as its row source and the cascade switch on: round-off inconsistency of dependent optimality rows
//      (at most min(1e-6 max(1, |bound|), 1e-5)) is accepted and reported in accepted_slack, the status stays SOLVED.
//   4. a failed level ends the instance: status = that level's status, dq = 0 (coman_ik.cpp:189-190).
// The body is written against the two-member team of osot_qp_big.h, so the same source compiles for the host (tests/emu).
#pragma once
#include <cstring>
#include "osot_plan_shape.h"
#include "osot_qp_big.h"

namespace osot {
namespace wide {

constexpr int kL = OSOT_MAX_LEVELS, kT = OSOT_MAX_TASKS, kRB = OSOT_MAX_ROWBLOCKS;
constexpr int kStage = 8;   // rows of A staged in LDS per pass of the H build

struct Plan {
    int n, L, nc, nc_stored;
    int nrows;                          // table capacity: nc + the rows of every level but the last (whose optimality rows no level uses)
    int big_bytes;                      // LDS of the solver (big::shared_bytes for the table's capacity), 16-byte aligned
    int m[kL], ma[kL], optoff[kL + 1];
    int nblocks;
    int blk_rows[kRB], blk_off[kRB], blk_stored_off[kRB], blk_implicit[kRB], blk_first_col[kRB], blk_level[kRB];
    int ntask[kL];
    int task_off[kL][kT + 1];
    unsigned inactive[kL];              // Task::setActive(false): bit j = task j of level k
    unsigned active_mask;               // iHQP::setActiveStack
    int max_iter;
    double eps_abs;
    int reg_rows, reg_dense;
    double reg_w;
};

struct Batch {
    int B;
    const double *A[kL], *b[kL], *w[kL], *c[kL], *WA[kL], *Wb[kL];
    const double *C, *lo, *up, *l, *u, *b_reg, *A_reg;
    double *dq, *x_levels, *accepted_slack;
    int *status, *iterations;
    double* work;                       // [grid][2][n][n]
};
static_assert(std::is_trivially_copyable<Plan>::value && std::is_trivially_copyable<Batch>::value, "kernel arguments, zeroed with memset");

// host side: the plan (and the call's level / task switches) -> kernel argument
inline void make_plan(const osot_plan_desc& p, const unsigned char* level_active, const unsigned char* task_active, Plan& P) {
    std::memset(&P, 0, sizeof(P));
    make_plan_shape(p, level_active, task_active, P);
    P.nrows = P.nc + P.optoff[p.n_levels - 1];
    P.big_bytes = (int)((big::shared_bytes(p.n, P.nrows) + 15) & ~(size_t)15);
}

// LDS of one workgroup: the solver's (big::shared_bytes for the table's capacity), then x_prev, x_k, g, the box (relaxed where a level
// accepts a bound's violation as round-off), the staging buffers, the row table (rlo, rup, rptr: 8 B per row; ropt: 4 B per row) and
// three scalars.  nrows = Plan::nrows
inline size_t shared_bytes(int n, int nrows) {
    const size_t big_b = (big::shared_bytes(n, nrows) + 15) & ~(size_t)15;
    const size_t dbl = 5 * (size_t)n + 2 * (size_t)kStage * n + 2 * kStage + 3 * (size_t)nrows + 2;
    return big_b + 8 * dbl + 4 * ((size_t)nrows + 4);
}

// the solver's row source: the table (see osot_qp_big.h: DenseRows)
struct TableRows {
    double *rlo, *rup;                // (relaxed where a level accepts a row's violation as round-off: for the rest of the instance)
    const unsigned long long* rptr;   // row address, or (col << 1) | 1 for the unit row e_col
    const int* ropt;                  // 1: optimality row, a'(x - x_prev) = 0
    const double* xprev;
    int n;
    OSOT_BIG_FN double lo(int r) const { return rlo[r]; }
    OSOT_BIG_FN double up(int r) const { return rup[r]; }
    OSOT_BIG_FN int unit(int r) const { const unsigned long long p = rptr[r]; return (p & 1ull) ? (int)(p >> 1) : -1; }
    OSOT_BIG_FN const double* row(int r) const { return reinterpret_cast<const double*>(rptr[r]); }
    OSOT_BIG_FN void relax(int r, int side, double v) const { if (side > 0) rlo[r] -= v; else rup[r] += v; }
    OSOT_BIG_FN double dot(int r, const double* x) const {
        const unsigned long long p = rptr[r];
        const bool opt = ropt[r] != 0;
        if (p & 1ull) { const int col = (int)(p >> 1); return opt ? x[col] - xprev[col] : x[col]; }
        const double* ar = reinterpret_cast<const double*>(p);
        double acc = 0.0;
        if (opt) for (int i = 0; i < n; ++i) acc += ar[i] * (x[i] - xprev[i]);
        else for (int i = 0; i < n; ++i) acc += ar[i] * x[i];
        return acc;
    }
};

OSOT_BIG_FN unsigned long long unit_code(int col) { return ((unsigned long long)col << 1) | 1ull; }

// one instance by the whole team; smem = shared_bytes(P.n, P.nrows), slot = 2 n^2 doubles
// HOT: every active level's solve is big::solve<true> on its own list of the caller's state, hot [B][P.L][big::kHotLen] (osot_ihqp_solve_hot):
// row inst belongs to instance inst of the batch, whichever workgroup solves it.  Level k's list holds positions in level k's row table
// (box, global rows, this level's task-local rows), read before the level's solve and rewritten after it -- all -1 where the level
// fails; the list of a level that is switched off, or that a failure above keeps from running, is not touched.  The cold
// instantiation carries none of it.
template <bool HOT = false, class Team>
OSOT_BIG_FN void cascade_instance(const Team& tm, const Plan& P, const Batch& D, const long long inst, char* smem, double* slot, int* hot = nullptr) {
    const int n = P.n, R = P.nrows;
    const bool t0 = tm.tid == 0;
    const big::Shared sh = big::carve(smem, n, R);
    double* xprev = reinterpret_cast<double*>(smem + P.big_bytes);
    double* xk = xprev + n;
    double* gl = xk + n;
    double* lb = gl + n;                  // [n] the box, relaxed where a level accepts a bound's violation
    double* ub = lb + n;
    double* sa = ub + n;                  // [kStage][n] rows of A
    double* sl = sa + kStage * n;         // [kStage][n] rows of W A (left operand)
    double* sb = sl + kStage * n;         // [kStage] b_r, or (W b)_r
    double* sw = sb + kStage;             // [kStage] (unused slot kept for alignment of the table)
    double* rlo = sw + kStage;
    double* rup = rlo + R;
    unsigned long long* rptr = reinterpret_cast<unsigned long long*>(rup + R);
    double* slack = reinterpret_cast<double*>(rptr + R);
    double* pad = slack + 1; (void)pad;
    int* ropt = reinterpret_cast<int*>(slack + 2);
    int* lst = ropt + R;                  // [0] status of the level, [1] its iterations
    double* Lw = slot;
    double* Jw = slot + (size_t)n * n;
    const TableRows rows{rlo, rup, rptr, ropt, xprev, n};

    // global rows: bounds and addresses (task-local blocks get their bounds per level)
    for (int j = 0; j < P.nblocks; ++j) {
        OSOT_BIG_FOR(q, P.blk_rows[j]) {
            const int r = P.blk_off[j] + q;
            rlo[r] = big::clamp_inf(D.lo[inst * P.nc + r]);
            rup[r] = big::clamp_inf(D.up[inst * P.nc + r]);
            rptr[r] = P.blk_implicit[j] ? unit_code(P.blk_first_col[j] + q)
                                        : reinterpret_cast<unsigned long long>(D.C + (inst * P.nc_stored + P.blk_stored_off[j] + q) * n);
            ropt[r] = 0;
        }
    }
    OSOT_BIG_FOR(i, n) {
        xprev[i] = 0.0;
        lb[i] = D.l ? D.l[inst * n + i] : -kInfty;
        ub[i] = D.u ? D.u[inst * n + i] : kInfty;
    }
    if (t0) *slack = 0.0;
    tm.sync();

    const bool regd = P.reg_dense && D.b_reg != nullptr;
    int status = big::ST_SOLVED, iters_total = 0;
    bool any = false;
    for (int k = 0; k < P.L; ++k) {
        if (!((P.active_mask >> k) & 1u)) {
            // inactive level: its optimality rows are void for the levels below (iHQP.cpp:301-309)
            if (k + 1 < P.L) {
                OSOT_BIG_FOR(q, P.m[k]) {
                    const int r = P.nc + P.optoff[k] + q;
                    rlo[r] = -kInfty; rup[r] = kInfty; rptr[r] = unit_code(0); ropt[r] = 0;
                }
                tm.sync();
            }
            continue;
        }
        // task-local row blocks: their bounds at their own level, absent (infinite bounds) at every other level
        for (int j = 0; j < P.nblocks; ++j) {
            if (P.blk_level[j] == 0) continue;
            const bool on = P.blk_level[j] - 1 == k;
            OSOT_BIG_FOR(q, P.blk_rows[j]) {
                const int r = P.blk_off[j] + q;
                rlo[r] = on ? big::clamp_inf(D.lo[inst * P.nc + r]) : -kInfty;
                rup[r] = on ? big::clamp_inf(D.up[inst * P.nc + r]) : kInfty;
            }
        }
        const int m = P.m[k], ma = P.ma[k], npost = m - ma;
        const unsigned inact = P.inactive[k];
        auto row_off = [&](int r) -> bool {
            if (!inact) return false;
            for (int j = 0; j < P.ntask[k]; ++j)
                if (((inact >> j) & 1u) && r >= P.task_off[k][j] && r < P.task_off[k][j + 1]) return true;
            return false;
        };
        const double* Ak = D.A[k] ? D.A[k] + inst * (long long)ma * n : nullptr;
        const double* bk = D.b[k] + inst * m;
        const double* wk = D.w[k] ? D.w[k] + inst * m : nullptr;
        const bool dense = D.WA[k] != nullptr;
        const double* WAk = dense ? D.WA[k] + inst * (long long)ma * n : nullptr;
        const double* Wbk = dense ? D.Wb[k] + inst * m : nullptr;
        const double* ck = D.c[k] ? D.c[k] + inst * n : nullptr;

        // ---- 1. H_k (lower triangle, into L) and g_k (LDS)
        const int ntri = n * (n + 1) / 2;
        OSOT_BIG_FOR(e, n * n) Lw[e] = 0.0;   // (big::solve adds eps to every element of the square it is handed; the upper triangle stays unread)
        OSOT_BIG_FOR(i, n) {
            double gi = ck ? ck[i] : 0.0;
            if (i < npost) gi -= (row_off(ma + i) ? 0.0 : (wk ? wk[ma + i] : 1.0)) * bk[ma + i];
            if (D.b_reg && !regd && i < P.reg_rows) gi -= P.reg_w * D.b_reg[inst * P.reg_rows + i];
            gl[i] = gi;
        }
        // rows [0, cnt) of a row source, kStage at a time: H += L'A (L = W A), g -= A'(W b) (dense W) or (W A)'b (diagonal W)
        auto accumulate = [&](const double* As, const double* WAs, const double* bs, const double* ws, double wconst, int cnt, bool use_off) {
            for (int r0 = 0; r0 < cnt; r0 += kStage) {
                tm.sync();                                   // (the previous stage has been consumed)
                OSOT_BIG_FOR(e, kStage * n) {
                    const int rr = e / n, col = e - rr * n, r = r0 + rr;
                    const bool in = r < cnt && !(use_off && row_off(r));
                    const double av = in ? As[(size_t)r * n + col] : 0.0;
                    sa[e] = av;
                    sl[e] = WAs ? (in ? WAs[(size_t)r * n + col] : 0.0) : (in ? (ws ? ws[r] : wconst) : 0.0) * av;
                }
                OSOT_BIG_FOR(rr, kStage) { const int r = r0 + rr; sb[rr] = (r < cnt) ? bs[r] : 0.0; }
                tm.sync();
                OSOT_BIG_FOR(e, ntri) {
                    int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
                    if ((i + 1) * (i + 2) / 2 <= e) ++i;
                    if (i * (i + 1) / 2 > e) --i;
                    const int j = e - i * (i + 1) / 2;
                    double acc = Lw[i * n + j];
                    for (int rr = 0; rr < kStage; ++rr) acc = fma(sl[rr * n + i], sa[rr * n + j], acc);
                    Lw[i * n + j] = acc;
                }
                OSOT_BIG_FOR(i, n) {
                    double gi = gl[i];
                    for (int rr = 0; rr < kStage; ++rr) gi -= (WAs ? sa[rr * n + i] : sl[rr * n + i]) * sb[rr];
                    gl[i] = gi;
                }
            }
        };
        if (ma > 0) accumulate(Ak, WAk, dense ? Wbk : bk, wk, 1.0, ma, true);
        if (regd) accumulate(D.A_reg + inst * (long long)P.reg_rows * n, nullptr, D.b_reg + inst * P.reg_rows, nullptr, P.reg_w, P.reg_rows, false);
        tm.sync();
        OSOT_BIG_FOR(i, n) {   // the implicit Postural block and the identity regularisation task: diagonal
            double dv = 0.0;
            if (i < npost) dv += row_off(ma + i) ? 0.0 : (wk ? wk[ma + i] : 1.0);
            if (D.b_reg && !regd && i < P.reg_rows) dv += P.reg_w;
            Lw[i * n + i] += dv;
        }
        tm.sync();

        // ---- 2. + 3. the level's QP on the row table
        big::Args a;
        a.n = n; a.nc = P.nc + P.optoff[k]; a.max_iter = P.max_iter; a.eps = P.eps_abs;
        a.H = Lw; a.g = gl; a.A = nullptr; a.lA = nullptr; a.uA = nullptr;
        a.l = D.l ? lb : nullptr; a.u = D.u ? ub : nullptr;
        a.lmut = lb; a.umut = ub;
        a.x = xk; a.status = lst; a.iters = lst + 1;
        a.Lw = Lw; a.J = Jw;
        a.accept_slack = true; a.slack = slack;
        if constexpr (HOT) {
            // (a null state: the level starts cold and records nothing.  The launch layer hands a null state to the cold kernel, so
            // the test is never false on the device; with it the kernel allocates 124 VGPRs, without it 130 -- one workgroup per CU
            // less: profiles/wide_hot_codegen.txt)
            if (hot) a.hot_in = a.hot_out = hot + ((size_t)inst * P.L + k) * big::kHotLen;
            big::solve<true>(tm, a, sh, rows);
        } else {
            (void)hot;
            big::solve(tm, a, sh, rows);
        }
        const int st = lst[0];
        iters_total += lst[1];
        tm.sync();                                           // (everybody has read the level's status before the next one)
        if (st != big::ST_SOLVED) { status = st; break; }
        any = true;
        OSOT_BIG_FOR(i, n) {
            xprev[i] = xk[i];
            if (D.x_levels) D.x_levels[(inst * P.L + k) * n + i] = xk[i];
        }
        // ---- optimality rows A_k x = A_k x_k for the levels below -> table
        if (k + 1 < P.L) {
            OSOT_BIG_FOR(q, m) {
                const int r = P.nc + P.optoff[k] + q;
                const bool void_row = row_off(q);            // inactive task: 0 x = 0 (Task.h:383-387), i.e. no row
                rlo[r] = void_row ? -kInfty : 0.0;
                rup[r] = void_row ? kInfty : 0.0;
                ropt[r] = void_row ? 0 : 1;
                rptr[r] = void_row ? unit_code(0)
                        : (q < ma) ? reinterpret_cast<unsigned long long>(Ak + (size_t)q * n) : unit_code(q - ma);   // Postural: e_(q-ma)
            }
        }
        tm.sync();
    }
    OSOT_BIG_FOR(i, n) D.dq[inst * n + i] = (status == big::ST_SOLVED && any) ? xprev[i] : 0.0;
    if (t0) {
        D.status[inst] = status;
        if (D.iterations) D.iterations[inst] = iters_total;
        if (D.accepted_slack) D.accepted_slack[inst] = *slack;
    }
    tm.sync();
}

}  // namespace wide

#if defined(__HIPCC__) && !defined(OSOT_BIG_HOST) && !defined(OSOT_EMULATION)
// one 256-thread workgroup per instance; the grid is capped at the resident workgroups and walks the batch with stride gridDim.x
__global__ void __launch_bounds__(256) osot_cascade_wide_kernel(const wide::Plan P, const wide::Batch D) {
    extern __shared__ __attribute__((aligned(16))) char osot_wide_smem[];
    const BigTeamDev tm{(int)threadIdx.x, (int)blockDim.x};
    double* slot = D.work + (size_t)blockIdx.x * 2 * (size_t)P.n * P.n;
    for (long long inst = blockIdx.x; inst < D.B; inst += gridDim.x) {
        wide::cascade_instance(tm, P, D, inst, osot_wide_smem, slot);
    }
}
// the same walk with every level's working set carried from call to call (osot_ihqp_solve_hot / osot_cycle_hot): same LDS, same
// workspace slot; the state is indexed by the INSTANCE, never by the workgroup
__global__ void __launch_bounds__(256) osot_cascade_wide_hot_kernel(const wide::Plan P, const wide::Batch D, int* const hot) {
    extern __shared__ __attribute__((aligned(16))) char osot_wide_smem[];
    const BigTeamDev tm{(int)threadIdx.x, (int)blockDim.x};
    double* slot = D.work + (size_t)blockIdx.x * 2 * (size_t)P.n * P.n;
    for (long long inst = blockIdx.x; inst < D.B; inst += gridDim.x) {
        wide::cascade_instance<true>(tm, P, D, inst, osot_wide_smem, slot, hot);
    }
}
#endif
}  // namespace osot
