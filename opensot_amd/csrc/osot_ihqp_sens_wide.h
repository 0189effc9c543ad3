// opensot_amd/csrc/osot_ihqp_sens_wide.h -- the level QPs, objectives and the backward pass's pull-back of the batched iHQP cascade
// for plans of 65 .. 128 variables (handles of osot_solver_create_wide): the three kernels of osot_ihqp_sens.h where the problem is
// wider than the 64 lanes of a wavefront.  The contracts are those kernels', word for word (include/osot_mi355x.h: osot_ihqp_level_qp,
// osot_ihqp_sensitivity); the argument structs, the checks and the schedule (ihqp_sens_levels) are osot_ihqp_sens.h's.
//
//   ihqpwide::level_qp ........ H, g, the row table [C; A_0 .. A_(k-1)] with its bounds, the box, of one instance
//   ihqpwide::objective ....... 1/2 x'(H + eps I)x + g'x of a materialised level (or the zeros of a level that is switched off)
//   ihqpwide::pullback ........ the backward pass's link between the levels
//   osot_ihqp_*_wide_kernel ... each of them as one 256-thread workgroup per instance
// The multipliers, and each level's KKT solve of the backward pass, are osot_qp_sens_big_kernel (osot_qp_sens_big.h), unchanged, on
// the materialised QP; it takes its per-slot Y slices from the tail of the caller's workspace.
//
// Each function is written against a team { tid, nt, sync() } as osot_qp_big.h and osot_qp_sens_big.h are: the SAME source is a
// workgroup on the device and, on the host, a team of one thread and a turn-taking team of several.  THE REPRODUCIBILITY RULE of
// osot_qp_sens_big.h holds: every scalar is ONE fma chain in one fixed order computed by its owner, there is no cross-thread
// reduction and no atomic, so the bits do not depend on the size of the team.  Every section that reads what another thread wrote
// is fenced by sync(); every loop that holds a sync() has bounds that depend on the plan alone, so every thread reaches every barrier.
//
// WHERE THE DATA LIVES (level_qp).  The work on H is cut into kThreads = 256 OWNERS: owner o has column j = o % 128 and the rows
// i = 64 (o / 128) .. + 63 of H, up to 64 accumulators that stay in registers over the whole row loop (entry (i, j) = sum_r
// L_r[max(i, j)] A_r[min(i, j)], L_r = w_r A_r or the row of W A: ONE product per unordered pair, one fma chain over the rows in
// ascending order: H is symmetric to the bit).  A thread of the device team is one owner (Team::kOwners = 1, Team::nt = 256 at compile
// time); a host thread plays the owners tid, tid + nt, ... with one accumulator set each (Team::kOwners = 256).  The owners of the
// first half also carry g_j.  Rows are staged through LDS in coalesced tiles of kTile = 32 rows, both operands, with the odd row
// stride n | 1 (a thread-per-row walk at one column has no bank conflict): level_lds_bytes(n) = (64 (n | 1) + n) 8 bytes, 33 800 at
// n = 65 and 67 072 at n = 128.  a_r'x_j of an optimality row: thread = row, one fma chain over the columns in ascending order.
// The kernel is bandwidth-shaped: it writes 8 (n n + rows n) bytes per instance and level.
//
// 67 072 bytes are above the 64 KB a kernel may ask for by default, and osot_qp_sens_big_kernel needs up to 145 KB: the host layer
// raises both limits once per device, on the first call.  hipFuncSetAttribute is not a stream operation, so ONE EAGER CALL must come
// before a capture of osot_ihqp_level_qp / osot_ihqp_sensitivity on a wide handle (as for osot_qp_sensitivity_batch at n > 32).
#pragma once
#include "osot_ihqp_sens.h"
#include "osot_qp_sens_big.h"

namespace osot {
namespace ihqpwide {

constexpr int kMinVars = sensbig::kMinVars;       // 65; below: the wavefront kernels of osot_ihqp_sens.h
constexpr int kMaxVars = sensbig::kMaxVars;       // 128
constexpr int kThreads = 256;
constexpr int kTile = 32;                         // rows of a staged tile
constexpr int kHalf = 64;                         // rows of H of one owner
constexpr int kOwners = 2 * kMaxVars;             // (column, half of the rows)
static_assert(kOwners == kThreads && 2 * kHalf == kMaxVars, "one owner per thread of the device team");

inline int level_lds_bytes(int n) { return (2 * kTile * (n | 1) + n) * (int)sizeof(double); }
inline int objective_lds_bytes(int n) { return n * (int)sizeof(double); }
inline int pullback_lds_bytes(int n) { return (kTile * (n | 1) + 2 * n + 2 * kTile) * (int)sizeof(double); }

// a plan of the wide route that these kernels serve
inline bool serves(const osot_plan_desc& plan, int wide) { return wide && plan.n >= kMinVars && plan.n <= kMaxVars; }

#if defined(__HIPCC__) && !defined(OSOT_EMULATION)
#define OSOT_IHQPWIDE_FN __device__ inline
#else
#define OSOT_IHQPWIDE_FN inline
#endif
#define OSOT_IHQPWIDE_FOR(i, N) for (int i = tm.tid; i < (N); i += tm.nt)

// Team: { int tid; nt; static constexpr int kOwners (the most owners one thread plays); void sync() const; } -- every thread of the
// team calls with the same arguments; lds: level_lds_bytes(n)
template <class Team>
OSOT_IHQPWIDE_FN void level_qp(const Team& tm, const LevelQpArgs& Q, long long inst, char* lds) {
    const LevelPlan& P = Q.P;
    const LevelBatch& D = Q.D;
    const int n = P.n, k = Q.level, ld = n | 1;
    double* At = reinterpret_cast<double*>(lds);               // the tile of A (right operand; the rows whose a'x is formed)
    double* Lt = At + kTile * ld;                              // the tile of W A (left operand)
    double* xs = Lt + kTile * ld;
    const osot_level_qp& O = Q.out;

    // ---- 1. H and g: owner o keeps H[64 (o / 128) ..][o % 128] in registers
    double acc[Team::kOwners][kHalf];
    double gacc[Team::kOwners];
#pragma unroll
    for (int s = 0; s < Team::kOwners; ++s) {
        gacc[s] = 0.0;
#pragma unroll
        for (int ii = 0; ii < kHalf; ++ii) acc[s][ii] = 0.0;
    }
    const int m = P.m[k], ma = P.ma[k];
    // Ar: count rows [.][n]; left operand: the rows of Wr (non-diagonal weight) or wv[r] * Ar (wv null: ws); right-hand side bv
    // (for a non-diagonal weight: W b); lvl >= 0: the rows of that level's inactive tasks count as zero rows
    auto add_rows = [&](const double* Ar, const double* Wr, const double* wv, double ws, const double* bv, int count, int lvl) {
        for (int r0 = 0; r0 < count; r0 += kTile) {
            const int rows = count - r0 < kTile ? count - r0 : kTile;
            OSOT_IHQPWIDE_FOR(e, rows * n) {
                const int rr = e / n, c = e - rr * n, r = r0 + rr;
                const bool off = lvl >= 0 && level_row_off(P, lvl, r);
                const double a = off ? 0.0 : Ar[(long long)r * n + c];
                At[rr * ld + c] = a;
                Lt[rr * ld + c] = Wr ? (off ? 0.0 : Wr[(long long)r * n + c]) : (wv ? wv[r] : ws) * a;
            }
            tm.sync();
#pragma unroll
            for (int s = 0; s < Team::kOwners; ++s) {
                const int o = tm.tid + s * tm.nt;
                const int j = o & (kMaxVars - 1), i0 = (o >> 7) * kHalf;
                if (o >= kOwners || j >= n || i0 >= n) continue;
                for (int rr = 0; rr < rows; ++rr) {
                    const double a = At[rr * ld + j], l = Lt[rr * ld + j];
                    if (i0 == 0) gacc[s] = fma(Wr ? -a : -l, bv[r0 + rr], gacc[s]);
#pragma unroll
                    for (int ii = 0; ii < kHalf; ++ii) {
                        const int i = i0 + ii;
                        if (i < n) acc[s][ii] = (j >= i) ? fma(l, At[rr * ld + i], acc[s][ii]) : fma(Lt[rr * ld + i], a, acc[s][ii]);
                    }
                }
            }
            tm.sync();
        }
    };
    const double* bk = D.b[k] + inst * m;
    const double* wk = D.w[k] ? D.w[k] + inst * m : nullptr;
    if (ma > 0)
        add_rows(D.A[k] + inst * ma * n, D.WA[k] ? D.WA[k] + inst * ma * n : nullptr, wk, 1.0, D.WA[k] ? D.Wb[k] + inst * m : bk, ma, k);
    if (D.b_reg && P.reg_dense)
        add_rows(D.A_reg + inst * (long long)P.reg_rows * n, nullptr, nullptr, P.reg_w, D.b_reg + inst * P.reg_rows, P.reg_rows, -1);
    // the diagonal (the implicit Postural block A = [I 0] and an identity-Jacobian regularisation task), g, the box, H
#pragma unroll
    for (int s = 0; s < Team::kOwners; ++s) {
        const int o = tm.tid + s * tm.nt;
        const int j = o & (kMaxVars - 1), i0 = (o >> 7) * kHalf;
        if (o >= kOwners || j >= n || i0 >= n) continue;
        double dv = 0.0, g = gacc[s];
        const int npost = m - ma;
        if (j < npost) {
            const double wp = level_row_off(P, k, ma + j) ? 0.0 : (wk ? wk[ma + j] : 1.0);
            dv = wp;
            g = fma(-wp, bk[ma + j], g);
        }
        if (D.b_reg && !P.reg_dense && j < P.reg_rows) {
            dv += P.reg_w;
            g = fma(-P.reg_w, D.b_reg[inst * P.reg_rows + j], g);
        }
        if (i0 == 0) {
            if (D.c[k]) g += D.c[k][inst * n + j];
            O.g[inst * n + j] = g;
            O.l[inst * n + j] = D.l ? level_clamp(D.l[inst * n + j]) : -1e20;
            O.u[inst * n + j] = D.u ? level_clamp(D.u[inst * n + j]) : 1e20;
            if (Q.x_out) Q.x_out[inst * n + j] = D.x_levels[(inst * P.L + k) * n + j];
        }
        double* Ho = O.H + inst * n * n;
#pragma unroll
        for (int ii = 0; ii < kHalf; ++ii) {
            const int i = i0 + ii;
            if (i < n) Ho[(long long)i * n + j] = acc[s][ii] + (i == j ? dv : 0.0);
        }
    }

    // ---- 2. the global rows, in plan order
    const long long rows_k = level_qp_rows(P, k);
    double* Ao = O.A + inst * rows_k * n;
    double* lAo = O.lA + inst * rows_k;
    double* uAo = O.uA + inst * rows_k;
    for (int j = 0; j < P.nblocks; ++j) {
        const bool on = P.blk_level[j] == 0 || P.blk_level[j] - 1 == k;     // a task-local block is absent at a foreign level
        const int r0 = P.blk_off[j];
        OSOT_IHQPWIDE_FOR(e, P.blk_rows[j] * n) {
            const int q = e / n, c = e - q * n;
            double v = 0.0;
            if (on) v = P.blk_implicit[j] ? (c == P.blk_first_col[j] + q ? 1.0 : 0.0)
                                          : D.C[(inst * P.nc_stored + P.blk_stored_off[j] + q) * n + c];
            Ao[(long long)(r0 + q) * n + c] = v;
        }
        OSOT_IHQPWIDE_FOR(q, P.blk_rows[j]) {
            lAo[r0 + q] = on ? level_clamp(D.lo[inst * P.nc + r0 + q]) : -1e20;
            uAo[r0 + q] = on ? level_clamp(D.up[inst * P.nc + r0 + q]) : 1e20;
        }
    }

    // ---- 3. the optimality rows of the levels above: A_j x = A_j x_j
    for (int j = 0; j < k; ++j) {
        const int off = P.nc + P.optoff[j], mj = P.m[j], maj = P.ma[j];
        if (!((P.active_mask >> j) & 1u)) {        // a level that is switched off: 0 x in [-1, 1] (iHQP.cpp:301-309)
            OSOT_IHQPWIDE_FOR(e, mj * n) Ao[(long long)off * n + e] = 0.0;
            OSOT_IHQPWIDE_FOR(q, mj) { lAo[off + q] = -1.0; uAo[off + q] = 1.0; }
            continue;
        }
        tm.sync();                                 // (everybody has read the previous level's xs and the last tile)
        OSOT_IHQPWIDE_FOR(c, n) xs[c] = D.x_levels[(inst * P.L + j) * n + c];
        const double* Aj = maj > 0 ? D.A[j] + inst * maj * n : nullptr;
        for (int r0 = 0; r0 < maj; r0 += kTile) {
            const int rows = maj - r0 < kTile ? maj - r0 : kTile;
            OSOT_IHQPWIDE_FOR(e, rows * n) {
                const int rr = e / n, c = e - rr * n;
                const double a = level_row_off(P, j, r0 + rr) ? 0.0 : Aj[(long long)(r0 + rr) * n + c];
                At[rr * ld + c] = a;
                Ao[(long long)(off + r0 + rr) * n + c] = a;
            }
            tm.sync();
            OSOT_IHQPWIDE_FOR(rr, rows) {
                double ax = 0.0;
                for (int c = 0; c < n; ++c) ax = fma(At[rr * ld + c], xs[c], ax);
                const bool v = level_row_off(P, j, r0 + rr);            // an inactive task: no row
                lAo[off + r0 + rr] = v ? -1e20 : ax;
                uAo[off + r0 + rr] = v ? 1e20 : ax;
            }
            tm.sync();
        }
        if (maj == 0) tm.sync();                   // (xs is read below)
        OSOT_IHQPWIDE_FOR(e, (mj - maj) * n) {     // the implicit Postural block: e_(q - ma) x = x_j[q - ma]
            const int q = e / n, c = e - q * n;
            Ao[(long long)(off + maj + q) * n + c] = (!level_row_off(P, j, maj + q) && c == q) ? 1.0 : 0.0;
        }
        OSOT_IHQPWIDE_FOR(q, mj - maj) {
            const bool v = level_row_off(P, j, maj + q);
            lAo[off + maj + q] = v ? -1e20 : xs[q];
            uAo[off + maj + q] = v ? 1e20 : xs[q];
        }
    }
}

// objective[inst][level] = 1/2 x'(H + eps I)x + g'x with the chains of osot_ihqp_objective_kernel: thread = column j forms (H x)_j as
// one fma chain over the rows (H is symmetric to the bit), the n terms are added in ascending order by thread 0.  lds: n doubles
template <class Team>
OSOT_IHQPWIDE_FN void objective(const Team& tm, const ObjectiveArgs& Q, long long inst, char* lds) {
    const int n = Q.n;
    if (Q.level_off) {
        const long long mt = n + Q.rows;
        OSOT_IHQPWIDE_FOR(e, (int)mt) {
            if (Q.y) Q.y[inst * mt + e] = 0.0;
            if (Q.active) Q.active[inst * mt + e] = 0;
        }
        if (tm.tid == 0) {
            if (Q.flag) Q.flag[inst] = OSOT_SENS_SKIPPED;
            if (Q.objective) Q.objective[inst * Q.L + Q.level] = 0.0;
        }
        return;
    }
    if (!Q.objective) return;
    double* term = reinterpret_cast<double*>(lds);
    const bool solved = Q.status[inst] == OSOT_STATUS_SOLVED;
    if (solved) {
        const double* H = Q.H + inst * n * n;
        const double* x = Q.x + inst * n;
        OSOT_IHQPWIDE_FOR(j, n) {
            double hx = 0.0;
            for (int i = 0; i < n; ++i) hx = fma(H[i * n + j], x[i], hx);
            hx = fma(Q.eps_abs, x[j], hx);
            term[j] = x[j] * fma(0.5, hx, Q.g[inst * n + j]);
        }
    }
    tm.sync();
    if (tm.tid == 0) {
        double f = 0.0;
        if (solved) for (int i = 0; i < n; ++i) f += term[i];
        Q.objective[inst * Q.L + Q.level] = sens_finite(f) ? f : 0.0;
    }
}

// The pull-back of level k with the formulas of osot_ihqp_pullback_kernel (include/osot_mi355x.h has them).  Every output of an
// instance is owned by its team and was zeroed by a stream-ordered fill before the first pull-back of the call, so the sums are
// plain read-add-writes, each entry by one thread.  s_r = a_r'x_k and t_r = a_r'dx are one fma chain each over the columns, thread =
// row; (A_j' rho)_c is one fma chain over the rows, thread = column.  lds: pullback_lds_bytes(n)
template <class Team>
OSOT_IHQPWIDE_FN void pullback(const Team& tm, const PullbackArgs& Q, long long inst, char* lds) {
    const LevelPlan& P = Q.P;
    const LevelBatch& D = Q.D;
    const IhqpGrads& G = Q.G;
    // not solved, x not finite or H~ not positive definite: the level's gradients are zeros (the fill), and x_k may hold anything.
    // (The flag is an input here: the whole team leaves.)
    if (Q.flag[inst] == OSOT_SENS_SKIPPED) return;
    const int n = P.n, k = Q.level, ld = n | 1;
    double* At = reinterpret_cast<double*>(lds);
    double* xs = At + kTile * ld;
    double* dxs = xs + n;
    double* sv = dxs + n;               // w_r (s_r - b_r) of the tile's rows
    double* tv = sv + kTile;            // w_r t_r
    OSOT_IHQPWIDE_FOR(c, n) { xs[c] = D.x_levels[(inst * P.L + k) * n + c]; dxs[c] = Q.dx[inst * n + c]; }
    tm.sync();

    // ---- 1. the cost of level k
    const int m = P.m[k], ma = P.ma[k];
    const double* bk = D.b[k] + inst * m;
    const double* wk = D.w[k] ? D.w[k] + inst * m : nullptr;
    const double* Ak = ma > 0 ? D.A[k] + inst * ma * n : nullptr;
    for (int r0 = 0; r0 < ma; r0 += kTile) {
        const int rows = ma - r0 < kTile ? ma - r0 : kTile;
        OSOT_IHQPWIDE_FOR(e, rows * n) {
            const int rr = e / n, c = e - rr * n;
            At[rr * ld + c] = level_row_off(P, k, r0 + rr) ? 0.0 : Ak[(long long)(r0 + rr) * n + c];
        }
        tm.sync();
        OSOT_IHQPWIDE_FOR(rr, rows) {
            const int r = r0 + rr;
            double s = 0.0, t = 0.0;
            for (int c = 0; c < n; ++c) { const double a = At[rr * ld + c]; s = fma(a, xs[c], s); t = fma(a, dxs[c], t); }
            const bool off = level_row_off(P, k, r);
            const double w = off ? 0.0 : (wk ? wk[r] : 1.0), e = s - bk[r];
            sv[rr] = w * e; tv[rr] = w * t;
            if (G.b[k]) G.b[k][inst * m + r] = -(w * t);
            if (G.w[k]) G.w[k][inst * m + r] = off ? 0.0 : t * e;
        }
        tm.sync();
        if (G.A[k])
            OSOT_IHQPWIDE_FOR(e, rows * n) {
                const int rr = e / n, c = e - rr * n;
                double* ga = G.A[k] + (inst * ma + r0 + rr) * n + c;
                *ga += fma(sv[rr], dxs[c], tv[rr] * xs[c]);
            }
        tm.sync();
    }
    OSOT_IHQPWIDE_FOR(i, m - ma) {                  // the implicit Postural block: s = x_k[i], t = dx[i]
        const int q = ma + i;
        const bool off = level_row_off(P, k, q);
        const double w = off ? 0.0 : (wk ? wk[q] : 1.0), e = xs[i] - bk[q], t = dxs[i];
        if (G.b[k]) G.b[k][inst * m + q] = -(w * t);
        if (G.w[k]) G.w[k][inst * m + q] = off ? 0.0 : t * e;
    }
    if (G.c[k]) OSOT_IHQPWIDE_FOR(c, n) G.c[k][inst * n + c] = dxs[c];

    // ---- 2. the global rows and the box
    const long long rows_k = level_qp_rows(P, k);
    const double* glA = Q.glA ? Q.glA + inst * rows_k : nullptr;
    const double* guA = Q.guA ? Q.guA + inst * rows_k : nullptr;
    const double* gA = Q.gA ? Q.gA + inst * rows_k * n : nullptr;
    OSOT_IHQPWIDE_FOR(q, P.nc) {
        if (G.lo) G.lo[inst * P.nc + q] += glA[q];
        if (G.up) G.up[inst * P.nc + q] += guA[q];
    }
    if (G.C && gA)
        for (int j = 0; j < P.nblocks; ++j) {
            if (P.blk_implicit[j]) continue;
            OSOT_IHQPWIDE_FOR(e, P.blk_rows[j] * n)
                G.C[(inst * P.nc_stored + P.blk_stored_off[j]) * n + e] += gA[(long long)P.blk_off[j] * n + e];
        }
    OSOT_IHQPWIDE_FOR(c, n) {
        if (G.l) G.l[inst * n + c] += Q.gl[inst * n + c];
        if (G.u) G.u[inst * n + c] += Q.gu[inst * n + c];
    }

    // ---- 3. the optimality blocks of the levels above: gx_j += A_j' rho, grad_A[j] += grad_A_qp + rho x_j'
    for (int j = 0; j < k; ++j) {
        if (!((P.active_mask >> j) & 1u)) continue;
        const int off = P.nc + P.optoff[j], mj = P.m[j], maj = P.ma[j];
        tm.sync();                                             // (everybody has read the previous xs)
        OSOT_IHQPWIDE_FOR(c, n) xs[c] = D.x_levels[(inst * P.L + j) * n + c];
        tm.sync();
        const double* Aj = maj > 0 ? D.A[j] + inst * maj * n : nullptr;
        OSOT_IHQPWIDE_FOR(c, n) {
            double acc = 0.0;
            for (int q = 0; q < maj; ++q) {
                if (level_row_off(P, j, q)) continue;          // an inactive task: a void row
                acc = fma(Aj[(long long)q * n + c], glA[off + q] + guA[off + q], acc);
            }
            if (c < mj - maj && !level_row_off(P, j, maj + c)) acc += glA[off + maj + c] + guA[off + maj + c];
            Q.gx[((long long)j * D.B + inst) * n + c] += acc;
        }
        if (G.A[j])
            OSOT_IHQPWIDE_FOR(e, maj * n) {
                const int q = e / n, c = e - q * n;
                if (level_row_off(P, j, q)) continue;
                const double rho = glA[off + q] + guA[off + q];
                G.A[j][(inst * maj + q) * n + c] += fma(rho, xs[c], gA[(long long)(off + q) * n + c]);
            }
    }
}

}  // namespace ihqpwide

#if defined(__HIPCC__) && !defined(OSOT_EMULATION)
// ---- the device side: one 256-thread workgroup per instance
struct IhqpWideTeamDev {
    int tid;
    static constexpr int nt = ihqpwide::kThreads;
    static constexpr int kOwners = 1;
    __device__ void sync() const { __syncthreads(); }
};
__global__ void __launch_bounds__(256) osot_ihqp_level_qp_wide_kernel(const LevelQpArgs A_) {
    OSOT_DYNAMIC_LDS(level_wide_smem);                         // ihqpwide::level_lds_bytes(n)
    const LevelQpArgs* Q = OSOT_KERNARG_PTR(LevelQpArgs, A_);
    if ((long long)blockIdx.x >= Q->D.B) return;
    ihqpwide::level_qp(IhqpWideTeamDev{(int)threadIdx.x}, *Q, blockIdx.x, level_wide_smem);
}
__global__ void __launch_bounds__(256) osot_ihqp_objective_wide_kernel(const ObjectiveArgs A_) {
    OSOT_DYNAMIC_LDS(obj_wide_smem);                           // ihqpwide::objective_lds_bytes(n)
    const ObjectiveArgs* Q = OSOT_KERNARG_PTR(ObjectiveArgs, A_);
    if ((long long)blockIdx.x >= Q->B) return;
    ihqpwide::objective(IhqpWideTeamDev{(int)threadIdx.x}, *Q, blockIdx.x, obj_wide_smem);
}
__global__ void __launch_bounds__(256) osot_ihqp_pullback_wide_kernel(const PullbackArgs A_) {
    OSOT_DYNAMIC_LDS(pull_wide_smem);                          // ihqpwide::pullback_lds_bytes(n)
    const PullbackArgs* Q = OSOT_KERNARG_PTR(PullbackArgs, A_);
    if ((long long)blockIdx.x >= Q->D.B) return;
    ihqpwide::pullback(IhqpWideTeamDev{(int)threadIdx.x}, *Q, blockIdx.x, pull_wide_smem);
}
#endif

}  // namespace osot
