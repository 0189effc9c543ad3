// osot_qp_core.h -- device-side dense QP core: Cholesky, J = L^-T, dual active set; one wavefront per QP.
//
// Solves   min 1/2 x'(H + eps I)x + g'x   s.t.  lo_r <= a_r'x <= up_r  (general rows),  lb <= x <= ub
// which is the problem every level of the cascade hands to OpenSoT's BackEnd
// (include/OpenSoT/solvers/BackEnd.h:125-150; convention SURVEY.md 8b).  H + eps I is strictly convex,
// so the minimiser is unique and any exact method reproduces the reference qpOASES x up to round-off.
//
// Method: Goldfarb-Idnani dual active set (the algorithm of the reference's eiQuadProg back-end,
// external/eiQuadProg-ext/include/eiquadprog.hpp) re-designed for a wavefront:
//   * the n-1 sequential Givens rotations of every constraint addition are replaced by ONE Householder
//     reflection = one rank-1 update of J, fully lane-parallel (w = J2 v comes for free from z);
//   * bilateral rows and the box are native (no [I;-I;A;-A] expansion, eiQuadProgBackEnd.cpp:40-66);
//     box normals are +-e_i, so d = J'n is a row read of J, not a mat-vec;
//   * equalities (lo == up: TaskToConstraint rows and the iHQP optimality rows A_j x = A_j x_j,
//     iHQP.cpp:164-170) are eliminated first and never enter the ratio test; their multipliers are
//     not formed;
//   * the triangular solve r = R^-1 d1 only runs over the inequality part of the working set.
//
// Lane layout (osot_team.h): lane = c + LW*h, LW = 32 or 64 lanes per half, HV = 64/LW halves; NP = padded size: 32, 64, or
// 56 = the 64-lane layout on a shorter LDS slice (WaveCtx below).  Vectors are
// one element per lane, replicated over h; for NP = 32 the halves split the inner range of every mat-vec.
// LDS per wave (doubles, zero-padded beyond n, compile-time row stride S = NP+1 so that row- and column-
// walks are bank-conflict free for ds_read_b64 and every inner-loop offset is an instruction immediate):
//     M1 (packed) L (Cholesky factor, written from registers) -> R (working-set factor, upper triangular, by columns)
//     M2[NP][S]  JT, JT[j][k] = J[k][j]  (starts as L^-1; or the closed-form J of a low-rank level, or the
//                H-orthonormal null-space basis of the equality rows under a diagonal Hessian)
// H itself never sits in LDS: it is built and factorised in registers (NP = 32: in the accumulator layout of
// v_mfma_f64_16x16x4_f64, factor_tiles32; NP > 32: the upper triangle of 16 x 16 tiles, factor_tiles_wide).
//     V[4][LW]   staging vectors for broadcasts
// All control flow is wave-uniform.
#pragma once
#include <osot_team.h>  // resolved through -I: csrc/ for the product, tests/emu/ for the host emulation
#include "osot_qp_tol.h" // kInfty, kViolTol, ... : the active-set tolerances, shared with osot_qp_big.h

namespace osot {

#ifndef OSOT_FEAS_MARGIN
#define OSOT_FEAS_MARGIN 0.0
#endif
constexpr double kFeasMargin = OSOT_FEAS_MARGIN;  // cascade levels below the first: every inequality that the previous level's solution
                                       // x_prev satisfies with less slack than this (or violates at round-off level: a level ends
                                       // when no violation exceeds kViolTol) has its bound moved to x_prev -+ margin before the
                                       // level is solved.  With the optimality rows posed relative to x_prev (see gi_solve) x_prev
                                       // is then a point that satisfies all equalities exactly and all inequalities strictly, so a
                                       // dual method can only meet its infeasibility certificate (normal in the span of the
                                       // working set, no multiplier to trade) through round-off, not because the stacked problem
                                       // is feasible to 1e-13 only.  Same magnitude as qpOASES' boundTolerance under OpenSoT's
                                       // options (1e6 * EPS, external/qpOASES-ext/src/Options.cpp:191-218).

enum { QP_SOLVED = 0, QP_INFEASIBLE = 1, QP_MAX_ITER = 2, QP_NOT_PD = 3 };

// R (the triangular factor of the working set; upper Hessenberg for a moment while a constraint is being dropped) lives in
// M1, PACKED by columns, column j holding rows 0 .. j+1 at offset j (j + 3) / 2 (NP = 64, round 3: 17 KB instead of 33, and
// the row table moved out of LDS: 52 KB per wave, three waves per CU instead of two).  NP = 32: 560 doubles instead of 1056: the 4 KB that let ten
// waves (instead of eight) share a CU's 160 KB of LDS, i.e. 2560 instead of 2048 instances in flight.  (At BASELINE
// config 3 a batch of 4096 then is 1.6 instead of 2 jobs per slot: the long jobs get a slot to themselves and the launch
// ends with its longest instance instead of with a late-started short one; tools/prof_cycle.py shows the timeline.)  A
// column's rows are contiguous, so lane-per-row accesses of one column are conflict-free and the column offset is uniform.
template <int NP>
__device__ __forceinline__ int ridx(int i, int j) { return ((j * (j + 3)) >> 1) + i; }   // (round 3: packed for NP = 64 as well)
template <int NP>
struct WaveCtx {
    // NP = padded problem size: 32 (two lanes per column), 64, or 56 -- the 64-lane solver with its LDS cut to what n <= 54
    // needs, so that FOUR wavefronts (one per SIMD) fit the CU's 160 KB instead of three.  There the lanes 56 .. 63 all take
    // the column index 56: a phantom all-zero column that lives in the padding element of every row (S = 57) and in one
    // phantom row of M2, so every address formed from c stays in bounds, every value those lanes hold is the zero a
    // padded column holds anyway, and no reduction has to know about them.  "Lane = row" loops use the physical lane.
    static constexpr int LW = (NP <= 32) ? 32 : 64;        // lanes per half
    static constexpr int HV = 64 / LW;
    static constexpr int S = NP + 1;
    // PH ("phantom" layouts, NP = 56 and -- round 5 -- NP = 40 for n <= 38: the reference's own 35-coordinate COMAN; its 80-register
    // factorisation arrays and 22 KB LDS slice run at TWO wavefronts per SIMD where the 56-lane layout runs at one)
    static constexpr bool PH = (NP > 32 && NP < 64);
    static constexpr int ROWS = PH ? NP + 1 : NP;          // rows of M2 that exist
    static constexpr int NMAX = PH ? NP - 2 : NP;          // largest n of this instantiation
    // packed R: 560 doubles for NP = 32, 2144 for NP = 64; the phantom layouts keep the NP (NP + 1) / 2 of the packed Cholesky
    // factor of round 3's register row sweep (in the history): 1596 for NP = 56, where R of n <= 54 columns needs 1539
    static constexpr int M1_DOUBLES = PH ? (NP * (NP + 1)) / 2 : NP * (NP + 3) / 2;
    // elements in flight per trip of the mat-vec passes / the stored-row walk (divisors of NP, multiples of 4)
#ifndef OSOT_DOT_CH40
#define OSOT_DOT_CH40 8     // round 5, A/B on one box with the tile factorisation in (COMAN35 S1..S4, M solves/s): 8 -> 19.9 / 8.37 / 6.58 / 4.33 with 222
                            // registers and NO spill; 20 (round 4's value) -> 19.6 / 8.33 / 6.52 / 4.32 with 26 spilled registers
#endif
#ifndef OSOT_DOT2_CH40
#define OSOT_DOT2_CH40 8    // the two-product passes (jt_rows_dot2 / jt_cols_dot2) hold three arrays per trip: at 20 elements their 120 registers were
                            // the NP = 40 kernels' peak
#endif
    static constexpr int DOT_CH = (NP == 56) ? 28 : ((NP == 40) ? OSOT_DOT_CH40 : 16);
    static constexpr int LDS_DOUBLES = M1_DOUBLES + ROWS * S + 4 * LW;   // M1, M2, V (four staging vectors of LW)
    __device__ static __forceinline__ int col_of(int lane) { return PH ? ((lane < NP) ? lane : NP) : lane % NP; }
    __device__ static __forceinline__ int half_of(int lane) { return PH ? 0 : lane / NP; }
    // the wavefront position of lane (c, h): recomputed from the coordinates where they determine it (no extra live register)
    __device__ static __forceinline__ int lane_of(int c, int h) { return PH ? phys_lane() : c + LW * h; }
    int c, h;       // column index and half of this lane
    int n;
    double* M1;
    double* M2;
    double* V;      // 4*LW
    // general-row table of the current QP, built in LDS by the calling kernel (one entry per row):
    double* rlo;                  // lower bound (already clamped to +-1e20)
    double* rup;                  // upper bound
    unsigned long long* rptr;     // address of the row's n doubles in HBM, or (index << 1) | 1 for the unit row e_index
    int* rowstate;                // 0 free, 1 lower active, 2 upper active, 3 equality
    int* eqlist;                  // indices of the equality rows, in row order
    signed char* rsrc;            // -1: bounds are rlo/rup (global row);  -2: the same, but a TASK-LOCAL row of the level being
                                  // solved (the previous level's solution need not satisfy it);  j >= 0: optimality row of
                                  // level j, the equality a'x = a'x_j (iHQP.cpp:164-170), posed as a'x = a'x_prev with x_prev
                                  // the solution of the last level solved (which satisfies a'x_prev = a'x_j); rlo = rup = 0
    unsigned long long safe_row;  // address of n readable doubles in HBM (dummy target of unit-row loads)
};

// a_r[col] for lane-column col (0 beyond n).  Branch-free: a unit row reads a harmless valid address
// (safe_row) and discards the value; the load is a global_load (address space 1), not a flat one.
template <int NP>
__device__ __forceinline__ double row_elem_p(const WaveCtx<NP>& w, unsigned long long p, int col) {   // (p = the row's table entry)
    const bool unit = (p & 1ull) != 0ull;
    const unsigned long long addr = unit ? w.safe_row : p;
    const double v = OSOT_GLOBAL_F64(addr)[(col < w.n) ? col : 0];
    const double uv = (col == (int)(p >> 1)) ? 1.0 : 0.0;
    return unit ? uv : ((col < w.n) ? v : 0.0);
}
template <int NP>
__device__ __forceinline__ double row_elem(const WaveCtx<NP>& w, int r, int col) {
    const unsigned long long p = w.rptr[r];
    const bool unit = (p & 1ull) != 0ull;
    const unsigned long long addr = unit ? w.safe_row : p;
    const int cc = (col < w.n) ? col : 0;
    const double v = OSOT_GLOBAL_F64(addr)[cc];
    const double uv = (col == (int)(p >> 1)) ? 1.0 : 0.0;
    return unit ? uv : ((col < w.n) ? v : 0.0);
}

// LEAN (NP = 32; osot_kernels.h, lean_plan): the instantiation for full-width, box-only plans -- n = 32 exactly, no constraint rows,
// every level active, diagonal weights, no linear term, no regularisation task.  Two things are then known at compile time:
//   * there is no padding: every "c < n" is true, every clamped column index is the index itself;
//   * the row table is IMPLICIT: the rows a level sees are exactly the optimality rows of the levels above it, in the table's
//     order -- row optoff[j] + q is row q of level j: the stored row A_j + q n, or the unit row e_(q - ma_j) of a Postural block; its
//     bounds are lo = up = 0, every row is an equality that x_prev satisfies (rsrc = j >= 0).  No rlo / rup / rptr / rowstate /
//     eqlist / rsrc traffic, no classification; a row's address comes from (j, q).
// The arithmetic, its order and the order of the rows are those of the general body: the results are the same bits.
struct LeanRows {
    const int* optoff;          // the plan's prefix sums of m[], m[] and ma[]
    const int* m;
    const int* ma;
    const double* const* A;     // the batch's level Jacobians (null where ma = 0)
    long long inst;
    int nlev;                   // levels above the one being solved: rows 0 .. optoff[nlev] - 1 are visible
};
// row `row` of the implicit table: the address of its 32 doubles (safe for a unit row) and the unit row's column (-1: stored)
__device__ __forceinline__ void lean_row(const LeanRows& lr, int row, unsigned long long safe, unsigned long long& addr, int& ucol) {
    addr = safe; ucol = -1;
    for (int j = 0; j < lr.nlev; ++j) {
        const int q = row - lr.optoff[j], maj = lr.ma[j];
        const bool in = q >= 0 && q < lr.m[j];
        const bool stored = q < maj;
        const unsigned long long a = reinterpret_cast<unsigned long long>(lr.A[j]) + (unsigned long long)(((lr.inst * maj + q) * 32) * 8);
        if (in) { addr = stored ? a : safe; ucol = stored ? -1 : q - maj; }
    }
}
// The same for N rows of a LANE's own (0 <= row[i] < optoff[nlev]): ONE loop over the levels around the rows.  What a level contributes is
// wave-uniform -- the address of its stored row q = row - optoff[j] is A_j + ((inst ma_j + q) 32) 8 = base_j + 256 row with base_j a
// scalar, and its unit rows start at table row optoff[j] + ma_j -- so a row costs one compare and the selects of (base, first unit row)
// per level BOUNDARY and one multiply-add at the end, instead of the whole address arithmetic per level.  Same addresses, same ucol.
// PRECONDITION (what lean_row does not need): every row[i] IS a row of the table, i.e. optoff[nlev] > 0 and optoff = the prefix sums of
// m -- a row at or beyond optoff[nlev] would come out as a row of the last level instead of (safe, -1).  The one caller passes
// min(row, 0 if row >= n_eq) with 8 <= n_eq <= optoff[nlev] (gi_solve takes the elimination only from 8 equalities on).
template <int N>
__device__ __forceinline__ void lean_rows(const LeanRows& lr, const int (&row)[N], unsigned long long safe, unsigned long long (&addr)[N], int (&ucol)[N]) {
    auto level_base = [&](int j) {
        return reinterpret_cast<unsigned long long>(lr.A[j]) + (unsigned long long)(((lr.inst * lr.ma[j] - lr.optoff[j]) * 32) * 8);
    };
    const bool none = lr.nlev <= 0;
    unsigned long long base[N];
    int ufirst[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { base[i] = level_base(0); ufirst[i] = lr.optoff[0] + lr.ma[0]; }
    for (int j = 1; j < lr.nlev; ++j) {
        const int o = lr.optoff[j], uj = o + lr.ma[j];
        const unsigned long long bj = level_base(j);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const bool at = row[i] >= o;
            base[i] = at ? bj : base[i];
            ufirst[i] = at ? uj : ufirst[i];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool unit = row[i] >= ufirst[i];
        addr[i] = (unit || none) ? safe : base[i] + 256ull * (unsigned long long)row[i];
        ucol[i] = (unit && !none) ? row[i] - ufirst[i] : -1;
    }
}
__device__ __forceinline__ double lean_row_elem(const LeanRows& lr, int row, unsigned long long safe, int col) {   // (row is wave-uniform)
    unsigned long long addr; int ucol;
    lean_row(lr, row, safe, addr, ucol);
    const double v = OSOT_GLOBAL_F64(addr)[col];
    return (ucol >= 0) ? ((col == ucol) ? 1.0 : 0.0) : v;
}

__device__ __forceinline__ double clamp_inf(double v) {
    return v < -kInfty ? -kInfty : (v > kInfty ? kInfty : v);
}

// d_c = sum_k JT[c][k] * vec[k]   (row walk, k split over the halves).  All LDS reads of a chunk are issued
// before the first FMA (one LDS round trip per chunk) and four accumulators break the dependent chain.
template <int NP>
__device__ __forceinline__ double jt_rows_dot(const WaveCtx<NP>& w, const double* vec) {
#ifndef OSOT_DOT_CH
#define OSOT_DOT_CH 16
#endif
#ifndef OSOT_DOT_CH56
#define OSOT_DOT_CH56 28    // elements in flight per trip of the 56-row layout (a divisor of 56, a multiple of 4): one wavefront per
                            // SIMD hides an LDS round trip with loads in flight only -- 8 per trip: 579 us per config-5 launch, 28: 562
#endif
    constexpr int HV = WaveCtx<NP>::HV, S = WaveCtx<NP>::S, CH = (NP % 16 == 0) ? OSOT_DOT_CH : ((NP == 56) ? OSOT_DOT_CH56 : WaveCtx<NP>::DOT_CH);
    const double* row = w.M2 + w.c * S + w.h;
    const double* v = vec + w.h;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
#pragma unroll
    for (int k0 = 0; k0 < NP / HV; k0 += CH) {
        double a[CH], b[CH];
#pragma unroll
        for (int t = 0; t < CH; ++t) a[t] = row[(k0 + t) * HV];
#pragma unroll
        for (int t = 0; t < CH; ++t) b[t] = v[(k0 + t) * HV];
#pragma unroll
        for (int t = 0; t < CH; t += 4) {
            acc0 = fma(a[t], b[t], acc0); acc1 = fma(a[t + 1], b[t + 1], acc1);
            acc2 = fma(a[t + 2], b[t + 2], acc2); acc3 = fma(a[t + 3], b[t + 3], acc3);
        }
    }
    return halfsum<NP>((acc0 + acc1) + (acc2 + acc3));
}
// z_c = sum_j JT[j][c] * vec[j]   (column walk, j split over the halves)
template <int NP>
__device__ __forceinline__ double jt_cols_dot(const WaveCtx<NP>& w, const double* vec) {
    constexpr int HV = WaveCtx<NP>::HV, S = WaveCtx<NP>::S, CH = (NP % 16 == 0) ? OSOT_DOT_CH : ((NP == 56) ? OSOT_DOT_CH56 : WaveCtx<NP>::DOT_CH);
    const double* col = w.M2 + w.h * S + w.c;
    const double* v = vec + w.h;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
#pragma unroll
    for (int j0 = 0; j0 < NP / HV; j0 += CH) {
        double a[CH], b[CH];
#pragma unroll
        for (int t = 0; t < CH; ++t) a[t] = col[(j0 + t) * HV * S];
#pragma unroll
        for (int t = 0; t < CH; ++t) b[t] = v[(j0 + t) * HV];
#pragma unroll
        for (int t = 0; t < CH; t += 4) {
            acc0 = fma(a[t], b[t], acc0); acc1 = fma(a[t + 1], b[t + 1], acc1);
            acc2 = fma(a[t + 2], b[t + 2], acc2); acc3 = fma(a[t + 3], b[t + 3], acc3);
        }
    }
    return halfsum<NP>((acc0 + acc1) + (acc2 + acc3));
}

// TWO products in one pass over JT (the equality phase adds its rows in pairs: gi_solve): the reads of JT -- what a pass costs,
// above all at one wavefront per SIMD -- are shared, each element feeds two accumulator sets.
template <int NP>
__device__ __forceinline__ void jt_rows_dot2(const WaveCtx<NP>& w, const double* va, const double* vb, double& da, double& db) {
    constexpr int HV = WaveCtx<NP>::HV, S = WaveCtx<NP>::S, CH = (NP == 32) ? 8 : ((NP == 40) ? OSOT_DOT2_CH40 : WaveCtx<NP>::DOT_CH);
    const double* row = w.M2 + w.c * S + w.h;
    const double* pa = va + w.h;
    const double* pb = vb + w.h;
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
#pragma unroll
    for (int k0 = 0; k0 < NP / HV; k0 += CH) {
        double m[CH], xa[CH], xb[CH];
#pragma unroll
        for (int t = 0; t < CH; ++t) m[t] = row[(k0 + t) * HV];
#pragma unroll
        for (int t = 0; t < CH; ++t) { xa[t] = pa[(k0 + t) * HV]; xb[t] = pb[(k0 + t) * HV]; }
#pragma unroll
        for (int t = 0; t < CH; t += 2) {
            a0 = fma(m[t], xa[t], a0); a1 = fma(m[t + 1], xa[t + 1], a1);
            b0 = fma(m[t], xb[t], b0); b1 = fma(m[t + 1], xb[t + 1], b1);
        }
    }
    da = halfsum<NP>(a0 + a1);
    db = halfsum<NP>(b0 + b1);
}
template <int NP>
__device__ __forceinline__ void jt_cols_dot2(const WaveCtx<NP>& w, const double* va, const double* vb, double& za, double& zb) {
    constexpr int HV = WaveCtx<NP>::HV, S = WaveCtx<NP>::S, CH = (NP == 32) ? 8 : ((NP == 40) ? OSOT_DOT2_CH40 : WaveCtx<NP>::DOT_CH);
    const double* col = w.M2 + w.h * S + w.c;
    const double* pa = va + w.h;
    const double* pb = vb + w.h;
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
#pragma unroll
    for (int j0 = 0; j0 < NP / HV; j0 += CH) {
        double m[CH], xa[CH], xb[CH];
#pragma unroll
        for (int t = 0; t < CH; ++t) m[t] = col[(j0 + t) * HV * S];
#pragma unroll
        for (int t = 0; t < CH; ++t) { xa[t] = pa[(j0 + t) * HV]; xb[t] = pb[(j0 + t) * HV]; }
#pragma unroll
        for (int t = 0; t < CH; t += 2) {
            a0 = fma(m[t], xa[t], a0); a1 = fma(m[t + 1], xa[t + 1], a1);
            b0 = fma(m[t], xb[t], b0); b1 = fma(m[t + 1], xb[t + 1], b1);
        }
    }
    za = halfsum<NP>(a0 + a1);
    zb = halfsum<NP>(b0 + b1);
}
// the rank-2 form of householder_add's update: rows j >= iq of JT lose  va[j] wa[c] + vb[j] wb[c]  (va = beta_a v_a in one staging
// vector, vb = beta_b v_b in another, both zero below their pivot; wa = J2 v_a, wb = (J2 H_a) v_b at my column)
template <int NP>
__device__ __forceinline__ void householder_apply2(const WaveCtx<NP>& w, const double* va, const double* vb, double wa, double wb, int iq) {
    constexpr int HV = WaveCtx<NP>::HV, S = WaveCtx<NP>::S;
    const int c = w.c, h = w.h, n = w.n;
    constexpr int RT = (NP == 64) ? 16 : (WaveCtx<NP>::PH ? 8 : 4);
    constexpr int TRIP = RT * HV;
    for (int jj = iq & ~(TRIP - 1); jj < n; jj += TRIP) {
        double* mrow = w.M2 + (jj + h) * S + c;
        const double* pa = va + jj + h;
        const double* pb = vb + jj + h;
        double m[RT], xa[RT], xb[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) m[t] = mrow[t * HV * S];
#pragma unroll
        for (int t = 0; t < RT; ++t) { xa[t] = pa[t * HV]; xb[t] = pb[t * HV]; }
#pragma unroll
        for (int t = 0; t < RT; ++t) mrow[t * HV * S] = fma(-xb[t], wb, fma(-xa[t], wa, m[t]));
    }
    wave_sync();
}

// the same product when vec is known to vanish below row j0 (z = J2 d2 with a large working set), NP = 64: only
// the rows from j0 rounded down to a multiple of sixteen are read (measured: -3 % on the 50-variable stack; for
// NP = 32 the fixed, fully unrolled walk above is faster)
template <int NP>
__device__ __forceinline__ double jt_cols_dot_tail64(const WaveCtx<NP>& w, const double* vec, int j0) {
    constexpr int S = WaveCtx<NP>::S, RT = (NP % 16 == 0) ? 16 : 8;
    double acc0 = 0.0, acc1 = 0.0;
    for (int jj = j0 & ~(RT - 1); jj < NP; jj += RT) {
        const double* col = w.M2 + jj * S + w.c;
        const double* v = vec + jj;
        double a[RT], b[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) a[t] = col[t * S];
#pragma unroll
        for (int t = 0; t < RT; ++t) b[t] = v[t];
#pragma unroll
        for (int t = 0; t < RT; t += 2) { acc0 = fma(a[t], b[t], acc0); acc1 = fma(a[t + 1], b[t + 1], acc1); }
    }
    return acc0 + acc1;
}

// One Householder reflection that maps d2 = d[iq:] onto alpha*e_iq, applied to the columns iq.. of J
// (rows iq.. of JT); appends (d1; alpha) as column iq of R.  z = J2 d2 is an input.
template <int NP, bool WRITE_R>
__device__ __forceinline__ void householder_add(const WaveCtx<NP>& w, double d, double d2, double z,
                                                double nd2, int iq) {
    constexpr int HV = WaveCtx<NP>::HV, S = WaveCtx<NP>::S;
    const int c = w.c, h = w.h, n = w.n;
    double* V2 = w.V + 2 * WaveCtx<NP>::LW;
    const double d_iq = bcast(d, iq);
    double nrm, rnrm;
    fast_sqrt_rsqrt(nd2, nrm, rnrm);
    const double alpha = (d_iq > 0.0) ? -nrm : nrm;
    const double v = (c > iq) ? d2 : ((c == iq) ? d_iq - alpha : 0.0);
    const double beta = fast_rcp(nd2 - alpha * d_iq);
    if (h == 0) V2[c] = v * beta;
    wave_sync();
    const double wv = z - alpha * w.M2[iq * S + c];   // w = J2 v
    wave_sync();   // both halves have read row iq before half 0 rewrites it
    // rows j >= iq of JT, split over the halves, RT rows per half and trip (NP = 64 runs one wave per SIMD:
    // only loads in flight hide the LDS latency there, and it has the registers for 16).  The start is rounded
    // DOWN to a multiple of the trip size: the extra rows j < iq have V2[j] = 0 (exact no-op) and every access
    // stays inside the NP rows of M2, so the loop needs no predicates and its LDS reads overlap.
    constexpr int RT = (NP == 64) ? 16 : (WaveCtx<NP>::PH ? 8 : 4);
    constexpr int TRIP = RT * HV;
    for (int jj = iq & ~(TRIP - 1); jj < n; jj += TRIP) {
        double* mrow = w.M2 + (jj + h) * S + c;
        const double* vrow = V2 + jj + h;
        double m[RT], vb[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) m[t] = mrow[t * HV * S];
#pragma unroll
        for (int t = 0; t < RT; ++t) vb[t] = vrow[t * HV];
#pragma unroll
        for (int t = 0; t < RT; ++t) mrow[t * HV * S] = fma(-vb[t], wv, m[t]);
    }
    if (WRITE_R && h == 0) {
        if (c < iq) w.M1[ridx<NP>(c, iq)] = d;
        else if (c == iq) w.M1[ridx<NP>(iq, iq)] = alpha;
    }
    wave_sync();
}

// Remove working-set position qq: shift R, re-triangularise with Givens rotations applied to the rows
// of R and to the matching columns of J (eiquadprog.hpp:551-617 does the same on its storage).
template <int NP>
__device__ __forceinline__ void drop_constraint(const WaveCtx<NP>& w, int qq, int& iq, int& Aq, double& uq) {
    constexpr int S = WaveCtx<NP>::S;
    const int c = w.c, h = w.h, n = w.n;
    const int An = shift_down_i<NP>(Aq);
    const double un = shift_down<NP>(uq);
    if (c >= qq && c < iq - 1) { Aq = An; uq = un; }
    if (h == 0 && c < n) {
        for (int q = qq; q < iq - 1; ++q)
            if (c <= q + 1) w.M1[ridx<NP>(c, q)] = w.M1[ridx<NP>(c, q + 1)];
    }
    wave_sync();
    iq--;
    for (int j = qq; j < iq; ++j) {
        const double a = w.M1[ridx<NP>(j, j)], b = w.M1[ridx<NP>(j + 1, j)];
        wave_sync();   // every lane has read the pivot pair before lane j overwrites it
        const double hh = a * a + b * b;
        if (hh == 0.0) continue;
        double s_, rs_;
        fast_sqrt_rsqrt(hh, s_, rs_);
        const double cg = a * rs_, sg = b * rs_;
        if (h == 0) {
            if (c >= j && c < iq) {
                const int o1 = ridx<NP>(j, c);            // (rows j, j+1 of column c: adjacent in the packed form)
                const int o2 = ridx<NP>(j + 1, c);
                const double r1 = w.M1[o1], r2 = w.M1[o2];
                w.M1[o1] = cg * r1 + sg * r2;
                w.M1[o2] = cg * r2 - sg * r1;
            }
            if (c < n) {
                const double j1 = w.M2[j * S + c], j2 = w.M2[(j + 1) * S + c];
                w.M2[j * S + c] = cg * j1 + sg * j2;
                w.M2[(j + 1) * S + c] = cg * j2 - sg * j1;
            }
        }
        wave_sync();
    }
}

// The general rows come from the LDS row table in WaveCtx (rlo/rup/rptr, nrows entries).

// ---------------------------------------------------------------------------------------------------------
// NP = 32 production path: BLOCKED right-looking Cholesky + inverse on the fp64 MATRIX CORE, panel width 4.
//
// H + eps I and L^-1 live in the accumulator layout of v_mfma_f64_16x16x4_f64: lane l = (a, q) = (l & 15, l >> 4),
// tile (I, C), element r holds M[16 I + q + 4 r][16 C + a]; as a flat array Ht[4 (2 I + C) + r] (sixteen fp64
// registers, the same count as the column layout).  Panel p is the four columns 4p .. 4p+3.
//   * By symmetry of the trailing matrix the panel IS a register: column 4p+q at rows 16 X + a equals row 4p+q at
//     columns 16 X + a, which is element r = p & 3 of the tiles (I = p >> 2, X) at lane (a, q).  No data movement.
//   * Inside the panel (VALU): per column one pivot broadcast + sqrt/rsqrt chain; the 3+2+1 rank-1 updates of the
//     later panel columns take their operands through ds_bpermute (lane (a, q) <- lane (a, qq): LDS crossbar,
//     no VALU time).  The four rows 4p .. 4p+3 of L^-1 (the same register of the L^-1 tiles) are finalised with the
//     same multipliers.
//   * Trailing updates (matrix core):  H(I,C) -= Lp(I) Lp(C)',  Linv(I,C) -= Lp(I) Linv_rows(C): the panel register
//     is the A operand (m = row-in-tile, k = panel column) AND the B operand of every tile.  13 + 13 MFMAs per
//     factorisation replace 32 x (16 LDS broadcasts + 32 VALU FMAs).  The (1,0) tile of H is never needed.
//   * L itself is never stored whole (M1 is the packed R of the working set, 560 doubles): the forward substitution
//     L y = -g rides along, one panel at a time -- the finished panel goes through a 4 x 32 staging buffer (the head of M1,
//     idle during the factorisation) so that lane c picks up its row's four entries L[c][4p .. 4p+3]; the backward
//     substitution L'x = y is the product x = (L^-1)'y with the rows of L^-1 that have just been stored.
// In : Ht (H + eps I with a unit diagonal beyond n), g by lane c.   Out: M2 = JT = L^-1, x = -(H+eps I)^-1 g; M1 clobbered.
// SKIP (round 6, nullspace_dense_wide's borrowed context: a reduced Hessian of 14 .. 24 columns): panels that lie wholly in the identity
// padding beyond n run under a uniform guard -- the padding factorises to itself, its off-diagonal entries are zero, so skipping them is
// exact (factor_tiles_wide does the same).  The cascade's own calls keep SKIP = false: no branch in the headline's panel sequence.
template <bool TT = false, bool SKIP = false, bool LEAN = false>
__device__ inline int factor_tiles32(const WaveCtx<32>& w, double (&Hf)[16], double g, double& x_out, long long* tt = nullptr) {
    long long tt0 = TT ? (long long)clock64() : 0;
#define OSOT_TT(i) do { if (TT) { const long long t_ = (long long)clock64(); tt[i] += t_ - tt0; tt0 = t_; } } while (0)
    constexpr int S = WaveCtx<32>::S;
    const int c = w.c, n = LEAN ? 32 : w.n;
    const int lane = c + 32 * w.h;
    const int ta = lane & 15, tq = lane >> 4;
    const bool valid = LEAN || c < n;
    double* PB = w.M1;   // [4][32] staging of the finished panel: PB[q * 32 + i] = L[i][4p + q]
    double* M2 = w.M2;
    double rhs = valid ? -g : 0.0;   // forward substitution, lane c = row c (replicated over the halves)
    v4f64 H00 = {Hf[0], Hf[1], Hf[2], Hf[3]}, H01 = {Hf[4], Hf[5], Hf[6], Hf[7]}, H11 = {Hf[12], Hf[13], Hf[14], Hf[15]};
    v4f64 L00, L10 = {0.0, 0.0, 0.0, 0.0}, L11;
#pragma unroll
    for (int r = 0; r < 4; ++r) { L00[r] = (ta == tq + 4 * r) ? 1.0 : 0.0; L11[r] = L00[r]; }
    bool bad = false;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int Ip = p >> 2, rp = p & 3;
        if (SKIP && 4 * p >= n) continue;
        // panel columns (as rows, by symmetry) and the matching rows of L^-1
        double Pn[2], Rp[2];
        double rsq[4];                         // 1 / L[j][j] of the panel's four columns (uniform)
        Pn[0] = Ip ? 0.0 : H00[rp];            // rows 0..15 of a column >= 16 are zero (above the diagonal)
        Pn[1] = Ip ? H11[rp] : H01[rp];
        Rp[0] = Ip ? L10[rp] : L00[rp];
        Rp[1] = Ip ? L11[rp] : 0.0;            // rows < 16 of L^-1 have no entries in columns >= 16
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int j = 4 * p + qq;
            const int lj = (4 * rp + qq) + 16 * qq;   // lane (a = j & 15, q = qq) holds H[j][j] in Pn[Ip]
            double piv = bcast(Pn[Ip], lj);
            bad = bad || !(piv > 0.0);      // (a non-positive or NaN pivot poisons what follows; the routine returns NOT_PD and x = 0 then)
            double sq, rs;
            fast_sqrt_rsqrt(piv, sq, rs);
            rsq[qq] = rs;
            const bool mine = (tq == qq);
            // Round 6 (instruction diet): the column's quarter-row is scaled by ONE masked multiplier (1 / L[j][j] in the lanes that hold
            // it, 1 elsewhere) instead of three selects per register.  The entries on and above the diagonal are NOT cleared here -- by
            // symmetry they hold the upper triangle of the trailing matrix, which nothing below reads: the later columns of the panel take
            // L[4p + q][j] from BELOW the diagonal, the trailing products mask the rows of the panel, and the forward substitution's
            // staging clears them once per panel (below).  The entries below the diagonal get the same bits as before.
            const double mul = mine ? rs : 1.0;
#pragma unroll
            for (int X = 0; X < 2; ++X) {
                if (!(Ip == 1 && X == 0)) Pn[X] *= mul;
                if (!(Ip == 0 && X == 1)) Rp[X] *= mul;
            }
            if (qq < 3) {
                const int src = ta + 16 * qq;                     // lane (a, qq): same row, column j
                const double ljj = __shfl(Pn[Ip], (4 * rp + tq) + 16 * qq, 64);   // L[4p + q][j] for my column 4p + q
                const bool later = (tq > qq);
#pragma unroll
                for (int X = 0; X < 2; ++X) {
                    if (!(Ip == 1 && X == 0)) {
                        const double colj = __shfl(Pn[X], src, 64);
                        Pn[X] = later ? fma(-colj, ljj, Pn[X]) : Pn[X];
                    }
                    if (!(Ip == 0 && X == 1)) {
                        const double rowj = __shfl(Rp[X], src, 64);
                        Rp[X] = later ? fma(-ljj, rowj, Rp[X]) : Rp[X];
                    }
                }
            }
        }
        // finished panel (zeros above the diagonal included) -> staging; final rows of L^-1 back into their tiles
        // staged with zeros ON and above the diagonal (column 4p + tq at rows ta, 16 + ta): a step of the substitution below is then a
        // plain fma in every lane -- rows at or above the column see a zero and keep their residual
        PB[tq * 32 + ta] = (Ip == 0 && ta > 4 * p + tq) ? Pn[0] : 0.0;
        PB[tq * 32 + 16 + ta] = (16 + ta > 4 * p + tq) ? Pn[1] : 0.0;
        if (Ip) { L10[rp] = Rp[0]; L11[rp] = Rp[1]; } else { L00[rp] = Rp[0]; }
        wave_sync();
        {   // forward substitution through the panel's four columns: y_j = rhs_j / L[j][j], rhs_i -= L[i][j] y_j below it
            double lrow[4];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) lrow[qq] = PB[qq * 32 + c];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int j = 4 * p + qq;
                const double yj = bcast(rhs, j) * rsq[qq];
                rhs = fma(-lrow[qq], yj, rhs);      // (lane j keeps its residual: y_j = rhs_j / L[j][j] is formed from it at the end)
            }
        }
        wave_sync();   // the staging buffer is free for the next panel
        // trailing updates on the matrix core; the A operand is the panel restricted to the rows below it
        const double A0 = (ta > 4 * p + 3) ? -Pn[0] : 0.0;          // rows 0..15
        const double A1 = (16 + ta > 4 * p + 3) ? -Pn[1] : 0.0;     // rows 16..31
        if (p < 3) {
            H00 = mfma_f64_16x16x4(A0, -A0, H00);
            H01 = mfma_f64_16x16x4(A0, -A1, H01);
            L00 = mfma_f64_16x16x4(A0, Rp[0], L00);
        }
        if (p < 7) {
            H11 = mfma_f64_16x16x4(A1, -A1, H11);
            L10 = mfma_f64_16x16x4(A1, Rp[0], L10);
            if (p >= 4) L11 = mfma_f64_16x16x4(A1, Rp[1], L11);
        }
    }
    OSOT_TT(0);   // panels
    // JT = L^-1 (the upper right tile is zero)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        M2[(tq + 4 * r) * S + ta] = L00[r];
        M2[(tq + 4 * r) * S + 16 + ta] = 0.0;
        M2[(16 + tq + 4 * r) * S + ta] = L10[r];
        M2[(16 + tq + 4 * r) * S + 16 + ta] = L11[r];
    }
    wave_sync();
    if (bad) { x_out = 0.0; return QP_NOT_PD; }
    OSOT_TT(1);   // L^-1 store
    OSOT_TT(2);   // (forward substitution: done panel by panel above)
    // L'x = y:  x_c = sum_j (L^-1)[j][c] y_j  (rhs holds y; rows of L^-1 = rows of JT)
    // y_c = (residual of row c) / L[c][c]: the reciprocal is the diagonal of L^-1 that has just been stored -- the very value the
    // substitution multiplied by when it broadcast y_c (a row of L^-1 starts as a unit row, is scaled once, by 1 / L[c][c], and no
    // later update reaches its diagonal: exact)
    rhs *= M2[c * S + c];
    if (w.h == 0) w.V[c] = valid ? rhs : 0.0;
    wave_sync();
    const double x = jt_cols_dot<32>(w, w.V);
    wave_sync();
    OSOT_TT(3);   // backward substitution
#undef OSOT_TT
    x_out = valid ? x : 0.0;
    return QP_SOLVED;
}

// ---------------------------------------------------------------------------------------------------------
// Round 5: the SAME blocked factorisation for the 64-lane layouts (NP = 40 / 56 / 64: 33 .. 64 variables) on T x T tiles of
// 16 x 16 (T = 3 covers 48 columns, T = 4 covers 64).  H + eps I arrives as the UPPER triangle of tiles (T (T + 1) / 2 of them,
// tile_u), L^-1 is built as the LOWER triangle (tile_l): 24 + 24 fp64 registers for T = 3, 40 + 40 for T = 4, where the
// register-resident row sweep it replaced (in the history) held NP-register arrays whose fully unrolled sweeps the allocator
// answered with 50 .. 300 spilled registers (profiles/r05_v1_kernel_resources.txt).  Panel p = columns 4p .. 4p+3 is element p & 3 of the
// tiles (p >> 2, X), X >= p >> 2; the trailing updates are one MFMA per live tile.  Panels that lie entirely in the identity
// padding beyond n (only possible from p = 8 on: these layouts serve n > 32) are skipped under a uniform guard: the padding
// factorises to itself and no earlier panel reaches it (its off-diagonal entries are zero).
// In : Hf[4 tile_u(I, C) + r] = (H + eps I)[16 I + q + 4 r][16 C + a] with a unit diagonal beyond n, lane (a, q) = (lane & 15,
// lane >> 4) of the PHYSICAL lane; g by lane = column.  Out: M2 = JT = L^-1 (identity on the padding n .. NP-1, nothing at or
// beyond NP), x = -(H + eps I)^-1 g by substitution (forward panel by panel, backward as (L^-1)'y); M1 clobbered.
constexpr int wide_tiles(int np) { return np <= 48 ? 3 : 4; }      // 16 x 16 tiles per side: NP = 40 -> 3, NP = 56 / 64 -> 4
template <int P, int N, class F>
__device__ __forceinline__ void static_for(F& f) {       // f(integral_constant<int, P>) for P = P .. N-1, each a compile-time call
    if constexpr (P < N) { f(std::integral_constant<int, P>{}); static_for<P + 1, N>(f); }
}
template <int T> __device__ __forceinline__ constexpr int tile_u(int I, int C) { return I * T - (I * (I - 1)) / 2 + (C - I); }   // I <= C
__device__ __forceinline__ constexpr int tile_l(int I, int C) { return (I * (I + 1)) / 2 + C; }                                  // C <= I
template <int NP, int T>
__device__ __forceinline__ int factor_tiles_wide(const WaveCtx<NP>& w, double (&Hf)[NP], double g, double& x_out) {
    static_assert(NP > 32 && 16 * T >= NP && 4 * (T * (T + 1)) / 2 <= NP, "tile count against the register array of the caller");
    constexpr int S = WaveCtx<NP>::S, NT = (T * (T + 1)) / 2, PBS = 16 * T;
    const int n = w.n;
    const int lane = phys_lane();
    const int ta = lane & 15, tq = lane >> 4;
    double* PB = w.M1;   // [4][16 T] staging of the finished panel: PB[q * PBS + i] = L[i][4p + q]
    double* M2 = w.M2;
    double rhs = (lane < n) ? -g : 0.0;   // forward substitution, lane = row
    v4f64 Hu[NT], Ll[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) Hu[t] = v4f64{Hf[4 * t], Hf[4 * t + 1], Hf[4 * t + 2], Hf[4 * t + 3]};
#pragma unroll
    for (int I = 0; I < T; ++I)
#pragma unroll
        for (int C = 0; C <= I; ++C)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ll[tile_l(I, C)][r] = (I == C && ta == tq + 4 * r) ? 1.0 : 0.0;
    bool bad = false;
    const int prow = (lane < PBS) ? lane : 0;   // my row of the staged panel (lanes beyond the tiles read a harmless entry)
    auto panel = [&](auto pc) {
        constexpr int p = decltype(pc)::value;
        constexpr int Ip = p >> 2, rp = p & 3;
        if (p >= 8 && 4 * p >= n) return;      // identity padding
        double Pn[T], Rp[T], rsq[4];
#pragma unroll
        for (int X = 0; X < T; ++X) {
            Pn[X] = (X < Ip) ? 0.0 : Hu[tile_u<T>(Ip, (X < Ip) ? Ip : X)][rp];      // rows above the panel's tile row: zero
            Rp[X] = (X <= Ip) ? Ll[tile_l(Ip, (X <= Ip) ? X : 0)][rp] : 0.0;         // L^-1 has no entries right of the diagonal tile
        }
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int j = 4 * p + qq;
            const int lj = (4 * rp + qq) + 16 * qq;   // lane (a = j & 15, q = qq) holds H[j][j] in Pn[Ip]
            double piv = bcast(Pn[Ip], lj);
            if (!(piv > 0.0)) { bad = true; piv = 1.0; }
            double sq, rs;
            fast_sqrt_rsqrt(piv, sq, rs);
            rsq[qq] = rs;
            const bool mine = (tq == qq);
#pragma unroll
            for (int X = Ip; X < T; ++X) {
                const int i = 16 * X + ta;
                const double scaled = (i > j) ? Pn[X] * rs : ((i == j) ? sq : 0.0);
                Pn[X] = mine ? scaled : Pn[X];
            }
#pragma unroll
            for (int X = 0; X <= Ip; ++X) Rp[X] = mine ? Rp[X] * rs : Rp[X];
            if (qq < 3) {
                const int src = ta + 16 * qq;                                       // lane (a, qq): same row, column j
                const double ljj = __shfl(Pn[Ip], (4 * rp + tq) + 16 * qq, 64);     // L[4p + q][j] for my column 4p + q
                const bool later = (tq > qq);
#pragma unroll
                for (int X = Ip; X < T; ++X) {
                    const double colj = __shfl(Pn[X], src, 64);
                    Pn[X] = later ? fma(-colj, ljj, Pn[X]) : Pn[X];
                }
#pragma unroll
                for (int X = 0; X <= Ip; ++X) {
                    const double rowj = __shfl(Rp[X], src, 64);
                    Rp[X] = later ? fma(-ljj, rowj, Rp[X]) : Rp[X];
                }
            }
        }
        // finished panel (zeros above the diagonal included) -> staging; final rows of L^-1 back into their tiles
#pragma unroll
        for (int X = 0; X < T; ++X) PB[tq * PBS + 16 * X + ta] = Pn[X];
#pragma unroll
        for (int X = 0; X <= Ip; ++X) Ll[tile_l(Ip, X)][rp] = Rp[X];
        wave_sync();
        {   // forward substitution through the panel's four columns
            double lrow[4];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) lrow[qq] = PB[qq * PBS + prow];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int j = 4 * p + qq;
                const double yj = bcast(rhs, j) * rsq[qq];
                rhs = (lane == j) ? yj : ((lane > j && lane < PBS) ? fma(-lrow[qq], yj, rhs) : rhs);
            }
        }
        wave_sync();   // the staging buffer is free for the next panel
        // trailing updates on the matrix core; the A operand is the panel restricted to the rows below it
        double Am[T];
#pragma unroll
        for (int X = 0; X < T; ++X) Am[X] = (X >= Ip && 16 * X + ta > 4 * p + 3) ? -Pn[X] : 0.0;
#pragma unroll
        for (int I = Ip; I < T; ++I) {
            if (p < 4 * I + 3) {           // tile row I still has rows below the panel
#pragma unroll
                for (int C = I; C < T; ++C) Hu[tile_u<T>(I, C)] = mfma_f64_16x16x4(Am[I], -Am[C], Hu[tile_u<T>(I, C)]);
#pragma unroll
                for (int C = 0; C <= Ip; ++C) Ll[tile_l(I, C)] = mfma_f64_16x16x4(Am[I], Rp[C], Ll[tile_l(I, C)]);
            }
        }
    };
    static_for<0, 4 * T>(panel);
    // JT = L^-1 (zero right of the diagonal tiles; rows / columns at or beyond NP do not exist in the slice)
#pragma unroll
    for (int I = 0; I < T; ++I)
#pragma unroll
        for (int C = 0; C < T; ++C)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + tq + 4 * r, col = 16 * C + ta;
                if (row < NP && col < NP) M2[row * S + col] = (C <= I) ? Ll[tile_l(I, (C <= I) ? C : 0)][r] : 0.0;
            }
    wave_sync();
    if (bad) { x_out = 0.0; return QP_NOT_PD; }
    w.V[lane] = (lane < n) ? rhs : 0.0;
    wave_sync();
    const double x = jt_cols_dot<NP>(w, w.V);
    wave_sync();
    x_out = (w.c < n) ? x : 0.0;
    return QP_SOLVED;
}

// phase cycle counters of the profiling instantiation (PROF = true): indices into prof[]
enum { PH_HBUILD = 0, PH_CHOL = 1, PH_INV = 2, PH_SUBST = 3, PH_EQ = 4, PH_INEQ = 5, PH_OPT = 6, PH_TOTAL = 7,
       PH_EQ_D = 8, PH_EQ_RED = 9, PH_EQ_Z = 10, PH_EQ_HH = 11,
       PH_IN_SCAN = 12, PH_IN_D = 13, PH_IN_Z = 14, PH_IN_R = 15, PH_IN_HH = 16, PH_IN_DROP = 17, PH_COUNT = 18 };
#define OSOT_SUB_BEGIN() long long sub_t0_ = PROF ? (long long)clock64() : 0
#define OSOT_SUB_END(idx) do { if (PROF) { const long long t_ = (long long)clock64(); prof[idx] += t_ - sub_t0_; sub_t0_ = t_; } } while (0)
#define OSOT_SUB_RESET() do { if (PROF) sub_t0_ = (long long)clock64(); } while (0)      /* behind a callee that keeps its own sub-phase clock */
#define OSOT_PH_BEGIN() long long ph_t0_ = PROF ? (long long)clock64() : 0
#define OSOT_PH_END(idx) do { if (PROF) { const long long t_ = (long long)clock64(); prof[idx] += t_ - ph_t0_; ph_t0_ = t_; } } while (0)

// ---------------------------------------------------------------------------------------------------------
// Null-space elimination of MANY equalities under a DIAGONAL Hessian (NP = 32).
//
// The last level of a velocity stack is a Postural task: H = diag(h) and its equalities are the optimality
// rows of every level above, E x = E x_prev (27 rows in 32 variables at BASELINE config 3), all satisfied by
// the previous level's solution x_prev.  Adding them one by one costs a rank-1 update of the full 32x32 J
// each.  Here instead:  (1) Gauss-Jordan with column pivoting brings E (held in registers, lane = column,
// rows split over the halves) to reduced echelon form -> basic / free columns and Z = [-E_B^-1 E_N ; I];
// (2) modified Gram-Schmidt in the H metric turns the nf = n - rank columns of Z into J2 (J2' H J2 = I);
// (3) x = x_prev - J2 J2'(H x_prev + g).  Any H-orthonormal basis of null(E) is a valid J2 for the dual
// active-set loop that follows, and the equality part of J is never read again.  Work ~ me^2 n / 2 instead of
// me n^2; linearly dependent (necessarily consistent) rows simply produce no pivot.
// Returns the rank (= number of equality positions in the working set), or -1 if nf > kNullMax (caller then
// takes the generic path; M2 = JT is as it was on entry in that case).
constexpr int kNullMax = 8;
template <bool PROF, bool LEAN = false>
__device__ inline int nullspace_equalities32(const WaveCtx<32>& w, int n_eq, double hdiag, double g, double xprev,
                                             double& x_out, long long* prof, const LeanRows& lr = LeanRows()) {
    OSOT_SUB_BEGIN();
    constexpr int S = WaveCtx<32>::S;
    const int c = w.c, h = w.h, n = LEAN ? 32 : w.n;
    const int lane = c + 32 * h;
    const bool valid = LEAN || c < n;
    double* M2 = w.M2;
    // ---- E -> registers in the ACCUMULATOR-TILE layout of v_mfma_f64_16x16x4: lane l = (ta, tq) = (l & 15, l >> 4), tile
    // (I, C) element r holds E[16 I + tq + 4 r][16 C + ta] (the layout of factor_tiles32).  All sixteen row pointers first,
    // then all loads (unconditional: a unit row reads the harmless safe_row), then the selects: ONE memory round trip.
    const int ta = lane & 15, tq = lane >> 4;
    v4f64 Et[4];   // Et[2 I + C]
    double emax = 0.0;
    {
        unsigned long long rp[8];   // the row's address (LEAN: safe_row for a unit row), or its table entry
        int uc[8];                  // LEAN: the unit row's column, -1 for a stored row
        double ld[16];
        if constexpr (LEAN) {           // (the list is the table itself; n_eq = optoff[nlev] rows)
            int rw[8];
#pragma unroll
            for (int I = 0; I < 2; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) { const int row = 16 * I + tq + 4 * r; rw[4 * I + r] = (row < n_eq) ? row : 0; }
            lean_rows<8>(lr, rw, w.safe_row, rp, uc);
        } else {
#pragma unroll
            for (int I = 0; I < 2; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * I + tq + 4 * r;
                    rp[4 * I + r] = w.rptr[w.eqlist[(row < n_eq) ? row : 0]]; uc[4 * I + r] = 0;
                }
        }
        const int c0 = (LEAN || ta < n) ? ta : 0, c1 = (LEAN || 16 + ta < n) ? 16 + ta : 0;
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned long long pr = rp[4 * I + r];
                const auto* base = OSOT_GLOBAL_F64((!LEAN && (pr & 1ull)) ? w.safe_row : pr);
                ld[8 * I + 2 * r] = base[c0];
                ld[8 * I + 2 * r + 1] = base[c1];
            }
        OSOT_KEEP16(ld);
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned long long pr = rp[4 * I + r];
                const bool unit = LEAN ? (uc[4 * I + r] >= 0) : ((pr & 1ull) != 0ull);
                const int ucol = LEAN ? uc[4 * I + r] : (int)(pr >> 1);
                const bool in = (16 * I + tq + 4 * r) < n_eq;
#pragma unroll
                for (int C = 0; C < 2; ++C) {
                    const int col = 16 * C + ta;
                    const double v = unit ? ((col == ucol) ? 1.0 : 0.0) : ((LEAN || col < n) ? ld[8 * I + 2 * r + C] : 0.0);
                    const double e = in ? v : 0.0;
                    Et[2 * I + C][r] = e;
                    emax = fmax(emax, fabs(e));
                }
            }
    }
    emax = colmax<64>(emax);
    const double tol = 1.0e-9 * emax;
    OSOT_SUB_END(PH_EQ_D);      // (profiling slots reused: load + scale)
    // ---- Gauss-Jordan with column pivoting, FOUR ROWS AT A TIME.  Panel p = rows 4p .. 4p+3 = element p & 3 of the tiles
    // (p >> 2, C) -- one register per tile column, lane (ta, tq) holding row 4p + tq at columns 16 C + ta: no data movement
    // to take it out.  (a) The four rows are reduced against each other in that form.  Pivot of a row = its largest entry among
    // the non-basic columns: the candidates travel as |value| in fp32 bits with the column packed into the five low bits
    // (non-negative floats order like unsigned integers), so ONE 16-lane integer DPP max + v_readlane yields value and
    // column; ties and values within 2^-18 of each other go to the lower column.  (b) Every other row i then needs
    // E[i] -= sum_q E[i][p_q] Rhat[q], the Schur form of eliminating the panel's four pivot columns with the ORIGINAL column
    // entries as multipliers: a rank-4 update, i.e. ONE v_mfma_f64_16x16x4 per tile.  The reduced panel in its quarter-row
    // form IS the B operand (lane (n, k) = Rhat[k][16 C + n]); the A operand (lane (m, k) = E[16 I + m][p_k]) goes through
    // LDS: every lane stores its sixteen entries of E by columns when the panel starts (asynchronously) and reads its two
    // after the panel, at the column its quarter-row's pivot fell on.
    unsigned basicmask = 0u;     // bit c: column c has become a pivot (basic) column
    double* colstore = M2;                                      // E by columns, stride 33 (M2 is idle: it is zeroed below)
    int* pivcol = reinterpret_cast<int*>(w.M1);                 // pivot column of each row (32 ints); M1 is idle too
    const unsigned tolbits = uniform_u32(f32_bits((float)tol));
    const int ta4 = ta << 2, rowbase4 = (lane & 48) << 2;       // byte addresses for ds_bpermute
    bool nb0 = LEAN || ta < n, nb1 = LEAN || 16 + ta < n;       // my columns are (still) non-basic
    int mypk = -1;                                              // lane k: pivot column of row k
    auto panel = [&](auto pc) {
        constexpr int p = decltype(pc)::value;
        constexpr int Ip = p >> 2, rq = p & 3;
        if (4 * p >= n_eq) return;
        // E as it is at the start of the panel -> LDS by columns (asynchronous: the stores drain under the first pivot search)
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int C = 0; C < 2; ++C)
#pragma unroll
                for (int r = 0; r < 4; ++r) colstore[(16 * C + ta) * 33 + 16 * I + tq + 4 * r] = Et[2 * I + C][r];
        double Pr0 = Et[2 * Ip][rq], Pr1 = Et[2 * Ip + 1][rq];
        int pcq = 0;                                            // pivot column of MY panel row (row 4p + tq); -1: none
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 4 * p + q;
            if (k < n_eq) {
                // branch-free: a row without a pivot (every candidate below tol: a dependent row, consistent because x_prev
                // satisfies every row) goes through the same arithmetic with a zero reciprocal, which zeroes the row and
                // leaves the others as they are
                const double r0raw = permute_f64(Pr0, ta4 + 64 * q), r1raw = permute_f64(Pr1, ta4 + 64 * q);   // row k at my columns
                const unsigned c0 = nb0 ? ((f32_bits((float)fabs(Pr0)) & ~31u) | (unsigned)(31 - ta)) : 0u;
                const unsigned c1 = nb1 ? ((f32_bits((float)fabs(Pr1)) & ~31u) | (unsigned)(15 - ta)) : 0u;
                const unsigned s = bcast_u32(row16_max_u32(umax(c0, c1)), 16 * q);
                const bool ok = (s & ~31u) > tolbits;
                const int pcol = 31 - (int)(s & 31u);
                const int ap = pcol & 15;
                const double fsel = (pcol >> 4) ? Pr1 : Pr0;              // the register that holds column pcol
                const double piv = bcast(fsel, ap + 16 * q);
                const double ipv = ok ? fast_rcp(piv) : 0.0;
                const double f = permute_f64(fsel, (ap << 2) + rowbase4);  // my panel row's entry at the pivot column
                const double r0 = r0raw * ipv, r1 = r1raw * ipv;           // the scaled pivot row at my columns
                const bool myrow = (tq == q);
                Pr0 = myrow ? r0 : fma(-f, r0, Pr0);
                Pr1 = myrow ? r1 : fma(-f, r1, Pr1);
                const int pk = ok ? pcol : -1;
                basicmask |= ok ? (1u << pcol) : 0u;
                nb0 = nb0 && (ta != pk);
                nb1 = nb1 && (16 + ta != pk);
                pcq = myrow ? pk : pcq;
                mypk = (lane == k) ? pk : mypk;
            } else {
                pcq = (tq == q) ? -1 : pcq;
            }
        }
        wave_sync();
        // A operand of the trailing update: lane (m, k) = (ta, tq) <- -E[16 I + m][p_k] as stored above; zero for the panel's own
        // rows and for a row without a pivot
        double FA[2];
#pragma unroll
        for (int I = 0; I < 2; ++I) {
            const double v = colstore[(pcq < 0 ? 0 : pcq) * 33 + 16 * I + ta];
            const bool own = (I == Ip) && ((ta >> 2) == rq);
            FA[I] = (pcq >= 0 && !own) ? -v : 0.0;
        }
        Et[0] = mfma_f64_16x16x4(FA[0], Pr0, Et[0]);
        Et[1] = mfma_f64_16x16x4(FA[0], Pr1, Et[1]);
        Et[2] = mfma_f64_16x16x4(FA[1], Pr0, Et[2]);
        Et[3] = mfma_f64_16x16x4(FA[1], Pr1, Et[3]);
        Et[2 * Ip][rq] = Pr0;                 // the reduced panel back into its register
        Et[2 * Ip + 1][rq] = Pr1;
        wave_sync();                          // the column store is free for the next panel
    };
    panel(std::integral_constant<int, 0>{}); panel(std::integral_constant<int, 1>{});
    panel(std::integral_constant<int, 2>{}); panel(std::integral_constant<int, 3>{});
    panel(std::integral_constant<int, 4>{}); panel(std::integral_constant<int, 5>{});
    panel(std::integral_constant<int, 6>{}); panel(std::integral_constant<int, 7>{});
    if (lane < 32) pivcol[lane] = mypk;
    wave_sync();
    OSOT_SUB_END(PH_EQ_RED);    // Gauss-Jordan
    const bool basic = valid && ((basicmask >> c) & 1u);
    const unsigned long long fmask = wave_ballot(valid && !basic && h == 0);
    const int nf = __builtin_popcountll(fmask);
    if (nf > kNullMax) {   // the caller goes on with the generic path: JT = diag(1 / sqrt(h)) back into M2 (it held the column store)
        for (int e = lane; e < 32 * S; e += 64) M2[e] = 0.0;
        wave_sync();
        if (h == 0 && valid) { double sq, rs; fast_sqrt_rsqrt(hdiag, sq, rs); M2[c * S + c] = rs; }
        wave_sync();
        return -1;
    }
    const bool is_free = valid && !basic;
    const int t = __builtin_popcountll(fmask & ((1ull << c) - 1ull));   // index of my column among the free ones
    const int me = n - nf;
    // ---- Z' rows into M2[me + t][:]:  Z[pivcol(row)][free column] = -E_reduced[row][free column]
    for (int e = lane; e < 32 * S; e += 64) M2[e] = 0.0;
    wave_sync();
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * I + tq + 4 * r;
            const int pk = (row < n_eq) ? pivcol[row] : -1;
#pragma unroll
            for (int C = 0; C < 2; ++C) {
                const int col = 16 * C + ta;
                const bool colfree = (LEAN || col < n) && !((basicmask >> col) & 1u);
                if (colfree && pk >= 0) {
                    const int tc = __builtin_popcountll(fmask & ((1ull << col) - 1ull));
                    M2[(me + tc) * S + pk] = -Et[2 * I + C][r];
                }
            }
        }
    if (is_free && h == 0) M2[(me + t) * S + c] = 1.0;
    wave_sync();
    // ---- modified Gram-Schmidt in the H metric: rows me.. of M2 become J2' -------------------------------
    const double hc = valid ? hdiag : 0.0;
    double zr[kNullMax];
#pragma unroll
    for (int s = 0; s < kNullMax; ++s) zr[s] = (s < nf) ? M2[(me + s) * S + c] : 0.0;
#pragma unroll
    for (int s = 0; s < kNullMax; ++s) {
        if (s < nf) {
#pragma unroll
            for (int q = 0; q < s; ++q) {
                const double rq = colsum<32>(hc * zr[q] * zr[s]);
                zr[s] = fma(-rq, zr[q], zr[s]);
            }
            const double nn = colsum<32>(hc * zr[s] * zr[s]);
            double sq, rs;
            fast_sqrt_rsqrt(nn, sq, rs);
            zr[s] *= rs;
            if (h == 0) M2[(me + s) * S + c] = zr[s];
        }
    }
    OSOT_SUB_END(PH_EQ_Z);      // Z extraction + Gram-Schmidt
    // ---- x = x_prev - J2 J2' (H x_prev + g) -----------------------------------------------------------------
    const double grad = valid ? fma(hc, xprev, g) : 0.0;
    double x = valid ? xprev : 0.0;
#pragma unroll
    for (int s = 0; s < kNullMax; s += 2) {
        if (s < nf) {
            double d0, d1;
            colsum2<32>(zr[s] * grad, (s + 1 < kNullMax) ? zr[s + 1] * grad : 0.0, d0, d1);
            x = fma(-d0, zr[s], x);
            if (s + 1 < kNullMax) x = fma(-d1, zr[s + 1], x);
        }
    }
    wave_sync();
    OSOT_SUB_END(PH_EQ_HH);     // projection
    x_out = x;
    return me;
}

// ---------------------------------------------------------------------------------------------------------
// Round 6: the SAME null-space elimination for the 40-lane layout (33 .. 38 variables: the reference's own 35-coordinate COMAN).
// There the last level of every published stack (examples/cpp/coman_ik.cpp:425-449) is the Postural task under 27 equality rows --
// the feet as TaskToConstraint rows (12), the CoM level (3) and the wrists (12) -- and until now each of them was one Householder
// reflection of the full 40 x 40 J: 159 k of an S3 solve's 550 k clocks (profiles/r06_phase_cycles_COMAN35.txt).  E lives in
// 2 x 3 tiles of 16 x 16 (rows <= 32, columns <= 48, zero beyond n), the panel step is nullspace_equalities32's with three
// column registers per quarter-row and six trailing products per panel; the column store (48 columns, stride 33) fits the idle M2
// (41 x 41).  Phantom lanes (40 .. 63 of the layout) hold tile columns like every other lane here: the tile coordinates come from the
// PHYSICAL lane, the vector phases behind the elimination from the layout's column index as everywhere else.
// (the elimination itself: shared by the diagonal-Hessian form below and the dense-level form, nullspace_dense_wide)
template <int NP, bool PROF>
// with_rhs: the rows' right-hand sides (rlo = rup of an equality row) ride along as tile column 47 -- never a pivot candidate (it lies beyond
// n), reduced with the rest: after the elimination row k reads x_(pivot k) + sum_free E'[k][f] x_f = E'[k][47]
__device__ inline void gj_reduce_wide(const WaveCtx<NP>& w, int n_eq, v4f64 (&Et)[6], unsigned long long& basicmask_out, long long* prof,
                                      bool with_rhs = false) {
    static_assert(NP == 40, "three column tiles: the 40-lane layout (n <= 38)");
    OSOT_SUB_BEGIN();
    constexpr int S = WaveCtx<NP>::S;
    constexpr int TC = 3;
    const int n = w.n;
    const int lane = phys_lane();
    double* M2 = w.M2;
    const int ta = lane & 15, tq = lane >> 4;
    // Et[TC I + C]: tile (I, C) element r holds E[16 I + tq + 4 r][16 C + ta]
    double emax = 0.0;
    {
        unsigned long long rp[8];
        double ld[8 * TC];
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + tq + 4 * r;
                rp[4 * I + r] = w.rptr[w.eqlist[(row < n_eq) ? row : 0]];
            }
        int cc[TC];
#pragma unroll
        for (int C = 0; C < TC; ++C) cc[C] = (16 * C + ta < n) ? 16 * C + ta : 0;
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned long long pr = rp[4 * I + r];
                const auto* base = OSOT_GLOBAL_F64((pr & 1ull) ? w.safe_row : pr);
#pragma unroll
                for (int C = 0; C < TC; ++C) ld[TC * (4 * I + r) + C] = base[cc[C]];
            }
        // (all 24 loads in flight before the first select: see OSOT_KEEP16)
        OSOT_KEEP12(ld, 0);
        OSOT_KEEP12(ld, 12);
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned long long pr = rp[4 * I + r];
                const bool unit = (pr & 1ull) != 0ull;
                const int ucol = (int)(pr >> 1);
                const bool in = (16 * I + tq + 4 * r) < n_eq;
#pragma unroll
                for (int C = 0; C < TC; ++C) {
                    const int col = 16 * C + ta;
                    const double v = unit ? ((col == ucol) ? 1.0 : 0.0) : ((col < n) ? ld[TC * (4 * I + r) + C] : 0.0);
                    const double e = in ? v : 0.0;
                    Et[TC * I + C][r] = e;
                    emax = fmax(emax, fabs(e));
                }
                if (with_rhs && ta == 15 && in) Et[TC * I + 2][r] = w.rlo[w.eqlist[16 * I + tq + 4 * r]];     // column 47
            }
    }
    emax = colmax<64>(emax);
    const double tol = 1.0e-9 * emax;
    OSOT_SUB_END(PH_EQ_D);
    // ---- Gauss-Jordan with column pivoting, four rows at a time (nullspace_equalities32's panel step; the column of a candidate is
    // packed into the SIX low bits of its fp32 magnitude: 48 columns)
    unsigned long long basicmask = 0ull;
    double* colstore = M2;                                      // E by columns, stride 33: 48 x 33 doubles of the 41 x 41 M2
    int* pivcol = reinterpret_cast<int*>(w.M1);
    const unsigned tolbits = uniform_u32(f32_bits((float)tol));
    const int ta4 = ta << 2, rowbase4 = (lane & 48) << 2;
    bool nb[TC];
#pragma unroll
    for (int C = 0; C < TC; ++C) nb[C] = 16 * C + ta < n;
    int mypk = -1;
    auto panel = [&](auto pc) {
        constexpr int p = decltype(pc)::value;
        constexpr int Ip = p >> 2, rq = p & 3;
        if (4 * p >= n_eq) return;
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int C = 0; C < TC; ++C)
#pragma unroll
                for (int r = 0; r < 4; ++r) colstore[(16 * C + ta) * 33 + 16 * I + tq + 4 * r] = Et[TC * I + C][r];
        double Pr[TC];
#pragma unroll
        for (int C = 0; C < TC; ++C) Pr[C] = Et[TC * Ip + C][rq];
        int pcq = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 4 * p + q;
            if (k < n_eq) {
                double rraw[TC];
                unsigned cand = 0u;
#pragma unroll
                for (int C = 0; C < TC; ++C) {
                    rraw[C] = permute_f64(Pr[C], ta4 + 64 * q);                                  // row k at my columns
                    const unsigned cb = nb[C] ? ((f32_bits((float)fabs(Pr[C])) & ~63u) | (unsigned)(47 - 16 * C - ta)) : 0u;
                    cand = umax(cand, cb);
                }
                const unsigned s = bcast_u32(row16_max_u32(cand), 16 * q);
                const bool ok = (s & ~63u) > tolbits;
                const int pcol = 47 - (int)(s & 63u);
                const int ap = pcol & 15, pt = pcol >> 4;
                const double fsel = (pt == 0) ? Pr[0] : ((pt == 1) ? Pr[1] : Pr[2]);              // the register that holds column pcol
                const double piv = bcast(fsel, ap + 16 * q);
                const double ipv = ok ? fast_rcp(piv) : 0.0;
                const double f = permute_f64(fsel, (ap << 2) + rowbase4);                        // my panel row's entry at the pivot column
                const bool myrow = (tq == q);
                const int pk = ok ? pcol : -1;
#pragma unroll
                for (int C = 0; C < TC; ++C) {
                    const double rs = rraw[C] * ipv;                                             // the scaled pivot row at my columns
                    Pr[C] = myrow ? rs : fma(-f, rs, Pr[C]);
                    nb[C] = nb[C] && (16 * C + ta != pk);
                }
                basicmask |= ok ? (1ull << pcol) : 0ull;
                pcq = myrow ? pk : pcq;
                mypk = (lane == k) ? pk : mypk;
            } else {
                pcq = (tq == q) ? -1 : pcq;
            }
        }
        wave_sync();
        double FA[2];
#pragma unroll
        for (int I = 0; I < 2; ++I) {
            const double v = colstore[(pcq < 0 ? 0 : pcq) * 33 + 16 * I + ta];
            const bool own = (I == Ip) && ((ta >> 2) == rq);
            FA[I] = (pcq >= 0 && !own) ? -v : 0.0;
        }
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int C = 0; C < TC; ++C) Et[TC * I + C] = mfma_f64_16x16x4(FA[I], Pr[C], Et[TC * I + C]);
#pragma unroll
        for (int C = 0; C < TC; ++C) Et[TC * Ip + C][rq] = Pr[C];      // the reduced panel back into its registers
        wave_sync();
    };
    panel(std::integral_constant<int, 0>{}); panel(std::integral_constant<int, 1>{});
    panel(std::integral_constant<int, 2>{}); panel(std::integral_constant<int, 3>{});
    panel(std::integral_constant<int, 4>{}); panel(std::integral_constant<int, 5>{});
    panel(std::integral_constant<int, 6>{}); panel(std::integral_constant<int, 7>{});
    if (lane < 32) pivcol[lane] = mypk;
    wave_sync();
    OSOT_SUB_END(PH_EQ_RED);
    basicmask_out = basicmask;
}

template <int NP, bool PROF>
__device__ inline int nullspace_equalities_wide(const WaveCtx<NP>& w, int n_eq, double hdiag, double g, double xprev,
                                                double& x_out, long long* prof) {
    static_assert(NP == 40, "three column tiles: the 40-lane layout (n <= 38)");
    OSOT_SUB_BEGIN();
    constexpr int S = WaveCtx<NP>::S;
    constexpr int TC = 3;
    const int c = w.c, n = w.n;
    const int lane = phys_lane();
    const bool valid = c < n;
    double* M2 = w.M2;
    const int ta = lane & 15, tq = lane >> 4;
    v4f64 Et[2 * TC];
    unsigned long long basicmask = 0ull;
    gj_reduce_wide<NP, PROF>(w, n_eq, Et, basicmask, prof);
    OSOT_SUB_RESET();
    int* pivcol = reinterpret_cast<int*>(w.M1);
    const bool basic = valid && ((basicmask >> c) & 1ull);
    const unsigned long long fmask = wave_ballot(valid && !basic && lane < NP);
    const int nf = __builtin_popcountll(fmask);
    if (nf > kNullMax) {   // the caller goes on with the generic path: JT = diag(1 / sqrt(h)) back into M2 (it held the column store)
        for (int e = lane; e < WaveCtx<NP>::ROWS * S; e += 64) M2[e] = 0.0;
        wave_sync();
        if (valid && lane < NP) { double sq, rs; fast_sqrt_rsqrt(hdiag, sq, rs); M2[c * S + c] = rs; }
        wave_sync();
        return -1;
    }
    const bool is_free = valid && !basic && lane < NP;
    const int t = __builtin_popcountll(fmask & ((1ull << c) - 1ull));
    const int me = n - nf;
    for (int e = lane; e < WaveCtx<NP>::ROWS * S; e += 64) M2[e] = 0.0;
    wave_sync();
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * I + tq + 4 * r;
            const int pk = (row < n_eq) ? pivcol[row] : -1;
#pragma unroll
            for (int C = 0; C < TC; ++C) {
                const int col = 16 * C + ta;
                const bool colfree = (col < n) && !((basicmask >> col) & 1ull);
                if (colfree && pk >= 0) {
                    const int tc = __builtin_popcountll(fmask & ((1ull << col) - 1ull));
                    M2[(me + tc) * S + pk] = -Et[TC * I + C][r];
                }
            }
        }
    if (is_free) M2[(me + t) * S + c] = 1.0;
    wave_sync();
    // ---- modified Gram-Schmidt in the H metric: rows me.. of M2 become J2' (phantom lanes read the zero padding column)
    const double hc = valid ? hdiag : 0.0;
    double zr[kNullMax];
#pragma unroll
    for (int s = 0; s < kNullMax; ++s) zr[s] = (s < nf) ? M2[(me + s) * S + c] : 0.0;
#pragma unroll
    for (int s = 0; s < kNullMax; ++s) {
        if (s < nf) {
#pragma unroll
            for (int q = 0; q < s; ++q) {
                const double rq = colsum<NP>(hc * zr[q] * zr[s]);
                zr[s] = fma(-rq, zr[q], zr[s]);
            }
            const double nn = colsum<NP>(hc * zr[s] * zr[s]);
            double sq, rs;
            fast_sqrt_rsqrt(nn, sq, rs);
            zr[s] *= rs;
            if (lane < NP) M2[(me + s) * S + c] = zr[s];
        }
    }
    OSOT_SUB_END(PH_EQ_Z);
    // ---- x = x_prev - J2 J2' (H x_prev + g)
    const double grad = valid ? fma(hc, xprev, g) : 0.0;
    double x = valid ? xprev : 0.0;
#pragma unroll
    for (int s = 0; s < kNullMax; s += 2) {
        if (s < nf) {
            double d0, d1;
            colsum2<NP>(zr[s] * grad, (s + 1 < kNullMax) ? zr[s + 1] * grad : 0.0, d0, d1);
            x = fma(-d0, zr[s], x);
            if (s + 1 < kNullMax) x = fma(-d1, zr[s + 1], x);
        }
    }
    wave_sync();
    OSOT_SUB_END(PH_EQ_HH);
    x_out = x;
    return me;
}

// ---------------------------------------------------------------------------------------------------------
// Round 6: a DENSE level under many equality rows, 40-lane layout (the reference's COMAN stacks, examples/cpp/coman_ik.cpp:425-449:
// every task level below the first sits under the feet's 12 TaskToConstraint rows plus the optimality rows of the levels above --
// 15 rows at S3's wrist level, 15 and 21 at S4's -- and each of them was one Householder reflection of the full 40 x 40 J BEHIND a
// 40-column Cholesky + inverse: 45 % of an S3 / S4 solve, profiles/r06_phase_cycles_COMAN35.txt).  The null-space method instead,
// for rows that x_prev satisfies (global equality rows and optimality rows do):
//   Z = null(E)                      gj_reduce_wide, the elimination of the Postural level (n x nf, nf = n - rank <= 24)
//   H = A'WA + D  (D diagonal: eps, a Postural block's weights, the regularisation task; A the level's <= 24 stored rows)
//   G = Z'HZ = (W^1/2 A Z)'(W^1/2 A Z) + Z'DZ,   t = Z'(H x_prev + g) = (W^1/2 A Z)'W^1/2 (A x_prev - b) + Z'(D x_prev + c)   [no H, no g: the
//                                    method runs AHEAD of the level's H build and takes its place]
//                                    two tile products on the matrix core: x_prev rides along as column nf of Z, so t is column nf of G
//   G = L L',  y = -G^-1 t           factor_tiles32<SKIP> on a BORROWED 32-lane context laid over the idle M1 / M2 (substitution included)
//   x = x_prev + Z y,   J2 = Z L^-T  (J2'HJ2 = I, E J2 = 0: what the dual active-set loop needs; the equality part of J is never read)
// The dual loop then runs as after the diagonal-level elimination: iq = rank, the equality rows of J zero, and the dependency test
// measured against n'(J2 J2')n -- for a bound exactly the diagonal entry sum_s J2[c][s]^2, returned as hinv.
// Returns the rank, or -1 (nothing the generic path relies on has been touched: it overwrites M1 and M2 itself) when more than
// kDenseNullFree columns stay free, none does, or G is not positive definite.
constexpr int kDenseNullFree = 24;   // free columns carried (registers: the lane's row of Z)
constexpr int kDenseNullRows = 24;   // stored rows of the level (their products with Z are staged in M1: 24 x 33 doubles)
template <int NP, bool PROF>
__device__ inline int nullspace_dense_wide(const WaveCtx<NP>& w, int n_eq, const double* Ak, const double* bk, const double* wk, int ma, double dcol,
                                           double clin, bool have_prev, double xprev_in, double& x_out, double& hinv_out, long long* prof) {
    static_assert(NP == 40, "the 40-lane layout (n <= 38)");
    OSOT_SUB_BEGIN();
    constexpr int S = WaveCtx<NP>::S, TC = 3, NF = kDenseNullFree;
    const int c = w.c, n = w.n;
    const int lane = phys_lane();
    const bool valid = c < n;
    double* M1 = w.M1;
    double* M2 = w.M2;
    double* V0 = w.V;
    double* V1 = w.V + WaveCtx<NP>::LW;
    double* V2 = w.V + 2 * WaveCtx<NP>::LW;
    double* V3 = w.V + 3 * WaveCtx<NP>::LW;
    const int ta = lane & 15, tq = lane >> 4;
    v4f64 Et[2 * TC];
    unsigned long long basicmask = 0ull;
    // (the FIRST level has no x_prev: its equality rows are global rows with their own right-hand sides, which ride along in the
    //  elimination -- a particular solution then is "basic variables = the reduced right-hand sides, free variables = 0")
    gj_reduce_wide<NP, PROF>(w, n_eq, Et, basicmask, prof, !have_prev);
    OSOT_SUB_RESET();
    int* pivcol = reinterpret_cast<int*>(M1);
    const bool basic = valid && ((basicmask >> c) & 1ull);
    const unsigned long long fmask = wave_ballot(valid && !basic && lane < NP);
    const int nf = __builtin_popcountll(fmask);
    if (nf > NF || nf < 1) return -1;
    double xprev = xprev_in;
    if (!have_prev) {
        bool inconsistent = false;
        if (lane < NP) V2[c] = 0.0;
        wave_sync();
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + tq + 4 * r;
                if (ta == 15 && row < n_eq) {
                    const int pk = pivcol[row];
                    const double rv = Et[TC * I + 2][r];
                    if (pk >= 0) V2[pk] = rv;
                    else inconsistent = inconsistent || (fabs(rv) > kEqTol);      // a dependent row that its partners do not imply: the generic path reports it
                }
            }
        if (wave_ballot(inconsistent) != 0ull) return -1;
        wave_sync();
        xprev = (basic && lane < NP) ? V2[c] : 0.0;
        wave_sync();
    }
    const bool is_free = valid && !basic && lane < NP;
    const int t = __builtin_popcountll(fmask & ((1ull << c) - 1ull));
    const int me = n - nf;
    // ---- Z' rows into M2[me + t][:] as after the diagonal-level elimination; row me + nf = x_prev (column nf of the products below)
    for (int e = lane; e < WaveCtx<NP>::ROWS * S; e += 64) M2[e] = 0.0;
    wave_sync();
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * I + tq + 4 * r;
            const int pk = (row < n_eq) ? pivcol[row] : -1;
#pragma unroll
            for (int C = 0; C < TC; ++C) {
                const int col = 16 * C + ta;
                const bool colfree = (col < n) && !((basicmask >> col) & 1ull);
                if (colfree && pk >= 0) {
                    const int tc = __builtin_popcountll(fmask & ((1ull << col) - 1ull));
                    M2[(me + tc) * S + pk] = -Et[TC * I + C][r];
                }
            }
        }
    if (is_free) M2[(me + t) * S + c] = 1.0;
    if (lane < NP) {
        M2[(me + nf) * S + c] = valid ? xprev : 0.0;
        V0[c] = valid ? dcol : 0.0;                          // D
        V1[c] = valid ? fma(dcol, xprev, clin) : 0.0;        // D x_prev + the linear term beside the stored rows' (-A'Wb is column nf of Ys'Ys)
    }
    wave_sync();     // (pivcol, at the head of M1, is dead from here on: M1 takes the staged products)
    double zr[NF];   // my row of Z
#pragma unroll
    for (int s2 = 0; s2 < NF; ++s2) zr[s2] = (s2 < nf) ? M2[(me + s2) * S + c] : 0.0;
    OSOT_SUB_END(PH_EQ_Z);
    // ---- Yt = A [Z | x_prev]  (ma x 32): A operand lane (m = ta, k = tq) = A[16 I + ta][4 kk + tq] straight from HBM / L2 (the H build
    // has just read these rows), B operand lane (k = tq, n = ta) = Z[4 kk + tq][16 J + ta] from the Z' rows in LDS
    const int ksteps = (n + 3) >> 2;
    const bool two_row_tiles = ma > 16;
    v4f64 Yt[2][2];
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J) Yt[I][J] = v4f64{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < ksteps; k0 += 5) {
        double a0[5], a1[5];
#pragma unroll
        for (int u = 0; u < 5; ++u) {       // (five steps of loads in flight before their products)
            const int j = 4 * (k0 + u) + tq;
            const bool jin = (k0 + u < ksteps) && j < n;
            a0[u] = Ak[((ta < ma) ? ta : 0) * n + (jin ? j : 0)];
            a1[u] = two_row_tiles ? Ak[((16 + ta < ma) ? 16 + ta : 0) * n + (jin ? j : 0)] : 0.0;
            a0[u] = (jin && ta < ma) ? a0[u] : 0.0;
            a1[u] = (jin && 16 + ta < ma) ? a1[u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            if (k0 + u < ksteps) {
                const int j = 4 * (k0 + u) + tq;
                const int jj = (j < n) ? j : 0;
                const double b0 = (ta <= nf && j < n) ? M2[(me + ta) * S + jj] : 0.0;
                const double b1 = (16 + ta <= nf && j < n) ? M2[(me + ((16 + ta <= nf) ? 16 + ta : 0)) * S + jj] : 0.0;
                Yt[0][0] = mfma_f64_16x16x4(a0[u], b0, Yt[0][0]);
                Yt[0][1] = mfma_f64_16x16x4(a0[u], b1, Yt[0][1]);
                if (two_row_tiles) {
                    Yt[1][0] = mfma_f64_16x16x4(a1[u], b0, Yt[1][0]);
                    Yt[1][1] = mfma_f64_16x16x4(a1[u], b1, Yt[1][1]);
                }
            }
        }
    }
    // Ys = W^1/2 Yt -> M1 (row i, column s at i * 33 + s; rows 0 .. 23)
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * I + tq + 4 * r;
            if (i < kDenseNullRows) {
                const double wi = (i < ma) ? (wk ? wk[i] : 1.0) : 0.0;
                const double bi = (i < ma) ? bk[i] : 0.0;
                double sw, isw;
                fast_sqrt_rsqrt((wi > 0.0) ? wi : 1.0, sw, isw);
                sw = (wi > 0.0) ? sw : 0.0;
#pragma unroll
                for (int J = 0; J < 2; ++J) {
                    // column nf: the level's residual at x_prev, A x_prev - b (so that column nf of G below is Z'(A'W(A x_prev - b) + ...))
                    const double yv = (16 * J + ta == nf) ? Yt[I][J][r] - bi : Yt[I][J][r];
                    M1[i * 33 + 16 * J + ta] = sw * yv;
                }
            }
        }
    wave_sync();
    // ---- G (rows s, columns s') = Ys'Ys + Z'[D Z | D x_prev + g]: the first sum runs over the level's rows, the second over the variables
    v4f64 Gt[2][2];
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J) Gt[I][J] = v4f64{0.0, 0.0, 0.0, 0.0};
    const int rsteps = ((ma < kDenseNullRows ? ma : kDenseNullRows) + 3) >> 2;
    for (int kk = 0; kk < rsteps; ++kk) {
        const int i = 4 * kk + tq;
        const double y0 = M1[i * 33 + ta], y1 = M1[i * 33 + 16 + ta];
        Gt[0][0] = mfma_f64_16x16x4(y0, y0, Gt[0][0]);
        Gt[0][1] = mfma_f64_16x16x4(y0, y1, Gt[0][1]);
        Gt[1][0] = mfma_f64_16x16x4(y1, y0, Gt[1][0]);
        Gt[1][1] = mfma_f64_16x16x4(y1, y1, Gt[1][1]);
    }
    for (int kk = 0; kk < ksteps; ++kk) {
        const int j = 4 * kk + tq;
        const int jj = (j < n) ? j : 0;
        const bool jin = j < n;
        const double z0 = (ta < nf && jin) ? M2[(me + ta) * S + jj] : 0.0;
        const double z1 = (16 + ta < nf && jin) ? M2[(me + ((16 + ta < nf) ? 16 + ta : 0)) * S + jj] : 0.0;
        const double dj = jin ? V0[jj] : 0.0, hj = jin ? V1[jj] : 0.0;
        const double b0 = (ta < nf) ? dj * z0 : ((ta == nf) ? hj : 0.0);
        const double b1 = (16 + ta < nf) ? dj * z1 : ((16 + ta == nf) ? hj : 0.0);
        Gt[0][0] = mfma_f64_16x16x4(z0, b0, Gt[0][0]);
        Gt[0][1] = mfma_f64_16x16x4(z0, b1, Gt[0][1]);
        Gt[1][0] = mfma_f64_16x16x4(z1, b0, Gt[1][0]);
        Gt[1][1] = mfma_f64_16x16x4(z1, b1, Gt[1][1]);
    }
    // t = column nf of G (rows s < nf) -> V2; G itself masked to nf x nf with a unit diagonal beyond (the padding factor_tiles32 expects)
    double Hf[16];
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int srow = 16 * I + tq + 4 * r, scol = 16 * J + ta;
                const double v = Gt[I][J][r];
                if (scol == nf && srow < nf) V2[srow] = v;
                Hf[4 * (2 * I + J) + r] = (srow < nf && scol < nf) ? v : ((srow == scol) ? 1.0 : 0.0);
            }
    wave_sync();
    const int c32 = lane & 31;
    const double t32 = (c32 < nf) ? V2[c32] : 0.0;
    wave_sync();
    OSOT_SUB_END(PH_EQ_D);
    // ---- G = L L', y = -G^-1 t on a borrowed 32-lane context: its 32 x 33 J' (= L^-1) over the head of M2 (the Z' rows are in registers
    // by now), its panel staging over the head of M1, its staging vector the fourth of V
    WaveCtx<32> w32;
    w32.c = c32; w32.h = lane >> 5; w32.n = nf;
    w32.M1 = M1; w32.M2 = M2; w32.V = V3;
    w32.rlo = nullptr; w32.rup = nullptr; w32.rptr = nullptr; w32.rowstate = nullptr; w32.eqlist = nullptr; w32.rsrc = nullptr; w32.safe_row = 0ull;
    double y32 = 0.0;
    const int stf = uniform_i(factor_tiles32<false, true>(w32, Hf, t32, y32));
    if (stf != QP_SOLVED) return -1;
    OSOT_SUB_END(PH_CHOL);
    // ---- x = x_prev + Z y
    double x = valid ? xprev : 0.0;
#pragma unroll
    for (int s2 = 0; s2 < NF; ++s2) { if (s2 < nf) x = fma(zr[s2], bcast(y32, s2), x); }
    // ---- J2' = L^-1 Z', IN PLACE in the lane's registers, last row first (row s2 needs the rows t2 <= s2 of Z' only), THEN -- behind a
    // synchronisation: the rows of J2' land on top of the borrowed L^-1 -- into M2[(me + s2) S ..]
    double hacc2 = 0.0;
#pragma unroll
    for (int s2 = NF - 1; s2 >= 0; --s2) {
        if (s2 < nf) {
            double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
            for (int t2 = 0; t2 <= s2; t2 += 2) {
                acc0 = fma(M2[s2 * 33 + t2], zr[t2], acc0);
                if (t2 + 1 <= s2) acc1 = fma(M2[s2 * 33 + t2 + 1], zr[t2 + 1], acc1);
            }
            zr[s2] = acc0 + acc1;
            hacc2 = fma(zr[s2], zr[s2], hacc2);
        }
    }
    wave_sync();
#pragma unroll
    for (int s2 = 0; s2 < NF; ++s2) { if (s2 < nf) M2[(me + s2) * S + c] = zr[s2]; }      // (phantom lanes: zeros -> the padding column stays zero)
    wave_sync();
    // the equality part of J', the borrowed context's remains below it, and the x_prev row: zero
    for (int e = lane; e < me * S; e += 64) M2[e] = 0.0;
    if (lane <= NP) M2[n * S + lane] = 0.0;
    wave_sync();
    OSOT_SUB_END(PH_EQ_HH);
    x_out = x;
    hinv_out = valid ? hacc2 : 0.0;
    return me;
}

// Is the part d2 = J2'n of a constraint normal outside the span of the working set a DIRECTION or round-off?
// nd2 = |d2|^2, dd = |d|^2 (both uniform); d2 = this lane's component (0 below iq); nv = this lane's entry of the
// normal n.  Second tier, per FREE COLUMN c of J: d2_c^2 / (|J_c|^2 |n|^2) = cos^2 of the angle between n and that
// column; the normal counts as a direction if it makes a usable angle with at least one of them.  (Per column, not
// against |J2|_F: at the default eps the null directions of H give columns of norm 1e5 next to columns of norm 1.)
template <int NP>
__device__ inline bool direction_is_independent(const WaveCtx<NP>& w, double nd2, double dd, double d2, double nv, int iq) {
    if (nd2 > 1.0e-12 * dd) return true;           // the usual case: one compare
    if (!(nd2 > kDepTol2 * dd)) return false;
    constexpr int S = WaveCtx<NP>::S;
    const int c = w.c, n = w.n;
    double cn = 0.0;                                // |J[:, c]|^2 of my column, if it is a free one
    if (c >= iq && c < n)
        for (int i = 0; i < n; ++i) { const double v = w.M2[c * S + i]; cn = fma(v, v, cn); }
    const double cos2 = (cn > 0.0) ? d2 * d2 / cn : 0.0;
    const double best = uniform_d(colmax<NP>(cos2));
    const double nn = uniform_d(colsum<NP>(nv * nv));
    return best > kDepFloor2 * nn;
}


// ITERATIVE REFINEMENT OF THE ITERATE ONTO THE WORKING SET (round 5).  x is built up as x0 + sum t z, and at the reference's
// default eps (J spans ten decades) the equalities it is supposed to satisfy -- the optimality rows A_j x = A_j x_prev above all --
// are met to ~1e-11 only; when those rows leave little or no freedom that residual, divided by their smallest singular value,
// is a displacement of 1e-6 .. 1e-5, and an inequality that was ACTIVE at the level above re-appears violated by that much with
// its normal in the span of the working set (tests/golden/default_eps_accepted_slack_instance.npz: 25 optimality rows in 25
// variables, 4.2e-7).  In exact arithmetic that cannot happen (x_prev is feasible and satisfies every equality), so before a
// level accepts such a violation as round-off it takes the round-off out: the residuals rho_q of all iq members of the working
// set at the current x (equalities: lo - a'x, or a'(x_prev - x) for an optimality row; active inequalities: minus their
// slack), R'y = rho by forward substitution, x += J1 y -- the minimum-H-norm correction onto the manifold.  Cold path: a few
// instances per thousand at the default eps, none at the benchmark's.
template <int NP, bool BOX, bool LEAN = false>
__device__ __forceinline__ double refine_on_working_set(const WaveCtx<NP>& w, double x, int iq, int Aq, double lb, double ub, double xprev,
                                                        const LeanRows& lr = LeanRows()) {
    const int c = w.c, h = w.h, n = LEAN ? 32 : w.n;
    double rho = 0.0;
#pragma unroll 1
    for (int q = 0; q < iq; ++q) {
        const int code = bcast_i(Aq, q);
        double rq;
        if (code <= -2) {
            const int r = -2 - code;
            if constexpr (LEAN) {   // an optimality row: a'(x_prev - x) against lo = 0
                const double a = lean_row_elem(lr, r, w.safe_row, c);
                rq = 0.0 + uniform_d(colsum<NP>(a * (xprev - x)));
            } else {
            const double a = row_elem<NP>(w, r, c);
            const double xref = (uniform_i(w.rsrc[r]) >= 0) ? xprev : 0.0;
            rq = uniform_d(w.rlo[r]) + uniform_d(colsum<NP>(a * (xref - x)));
            }
        } else if (BOX || code < 2 * n) {
            const int var = (code < n) ? code : code - n;
            rq = bcast((code < n) ? (lb - x) : (x - ub), var);
        } else {
            const int r = (code - 2 * n) >> 1;
            const double a = row_elem<NP>(w, r, c);
            const double ax = uniform_d(colsum<NP>(a * x));
            rq = (code & 1) ? (ax - uniform_d(w.rup[r])) : (uniform_d(w.rlo[r]) - ax);
        }
        if (c == q) rho = rq;
    }
    const bool in = c < iq;
    double e = in ? rho : 0.0, y = 0.0;
    const double rinv = in ? fast_rcp(w.M1[ridx<NP>(c, c)]) : 0.0;
#pragma unroll 1
    for (int i = 0; i < iq; ++i) {
        const double yi = bcast(e * rinv, i);
        if (c == i) y = yi;
        if (in && c > i) e = fma(-w.M1[ridx<NP>(i, c)], yi, e);
    }
    // dx = J1 y, one column of J per trip (cold path: no unrolled LDS batches -- their registers would be the hot kernels')
    double dx = 0.0;
#pragma unroll 1
    for (int j = 0; j < iq; ++j) dx = fma(w.M2[j * WaveCtx<NP>::S + c], bcast(y, j), dx);
    return (LEAN || c < n) ? x + dx : x;
}

// BOX: the instantiation for problems whose ONLY inequalities are the bounds l <= x <= u (a plan without constraint rows: every
// row of the table is an optimality row, i.e. an equality -- BASELINE configs 2 and 3): the candidate of a trip is a bound
// by construction, so the row classification, the unit-row and stored-row scans, the fetch of a row normal and every
// "bound or row?" branch of the trip are not compiled in (measured: +9 % on the headline batch)
template <int NP, bool PROF, bool BOX, bool LEAN = false>
__device__ int gi_inequalities(const WaveCtx<NP>& w, int nrows, double x, int iq, const int me, int Aq, double uq,
                               int iters, bool has_box, double& lb, double& ub, int max_iter, bool diag_dd, double hinv,
                               bool have_prev, double xprev, double& slack_out, double& x_out, int& iters_out, long long* prof,
                               int hotcode, int* hot_out, const LeanRows& lr = LeanRows());

// ---------------------------------------------------------------------------------------------------------
// Low-rank level (NP = 32):  H + eps I = D + A'WA with D diagonal and at most kLowRankMax stored rows
// (a CoM task: 3 rows in 32 variables; the Postural weights of the level, if any, and eps are D).
// Goldfarb-Idnani only needs SOME J with J J' = (H + eps I)^-1, not the Cholesky one.  In the scaled variables
// xh = D^1/2 x the Hessian is I + Ah'Ah, Ah = W^1/2 A D^-1/2 = Rh Qh (modified Gram-Schmidt of the m rows,
// Qh orthonormal rows, Rh lower triangular m x m), so with M = Rh'Rh and I + M = Lh Lh':
//     (I + Ah'Ah)^-1 = (I - Qh'Qh) + Qh'(I + M)^-1 Qh      and      Jh = I + Qh'(Lh^-T - I) Qh  satisfies Jh Jh' = that,
//     J = D^-1/2 Jh,     xh = -(I - Qh'Qh) ch + Qh'(I + M)^-1 (Rh' W^1/2 b - Qh ch),    ch = D^-1/2 c
// (c collects the level's linear term and the Postural rows' -w_i b_i).  No cancellation: the b part never forms
// A'Wb.  Cost: m(m+1)/2 reductions, an m x m Cholesky in uniform scalars and a rank-m update of the identity,
// instead of the n x n x m product and a 32-column factorisation.  A numerically dependent row is dropped.
// Out: M2 = JT (M2[j][c] = J[c][j]), x; M1 is used as staging.
#ifndef OSOT_LOWRANK_MAX
#define OSOT_LOWRANK_MAX 6      // round 5: one Cartesian task (six rows) next to a Postural block -- BASELINE config 2 -- takes the closed form too
#endif
constexpr int kLowRankMax = OSOT_LOWRANK_MAX;
// MM = compile-time bound on the rows (3 for a CoM task, else kLowRankMax): the m x m algebra is fully unrolled
// (round 6: NP = 32 as before, and NP = 40 -- the CoM level of the reference's COMAN stacks on its own 35-coordinate robot)
template <int NP, int MM, bool LEAN = false>
__device__ inline void lowrank_prepare(const WaveCtx<NP>& w, const double* Ak, const double* bk, const double* wk,
                                         int m, double dcol, double cvec, bool has_c, double& x_out) {
    constexpr int S = WaveCtx<NP>::S, HV = WaveCtx<NP>::HV;
    static_assert(MM * S <= WaveCtx<NP>::M1_DOUBLES, "the rows are staged in M1");
    const int c = w.c, h = w.h, n = LEAN ? 32 : w.n;
    const bool valid = LEAN || c < n;
    double* M1 = w.M1;
    double* M2 = w.M2;
    double dsq, dis;   // sqrt(d_c), 1 / sqrt(d_c)
    fast_sqrt_rsqrt(valid ? dcol : 1.0, dsq, dis);
    double q[MM], bt[MM], Rm[MM][MM];
#pragma unroll
    for (int r = 0; r < MM; ++r) {
        const int rr = (r < m) ? r : 0;
        const double wr = wk ? wk[rr] : 1.0;
        double sw, isw;
        fast_sqrt_rsqrt((wr > 0.0) ? wr : 1.0, sw, isw);
        sw = (wr > 0.0 && r < m) ? sw : 0.0;
        q[r] = valid ? sw * Ak[rr * n + c] * dis : 0.0;
        bt[r] = sw * bk[rr];
#pragma unroll
        for (int s2 = 0; s2 < MM; ++s2) Rm[r][s2] = 0.0;
    }
    // modified Gram-Schmidt of the rows (lane = column, replicated over the halves)
#pragma unroll
    for (int r = 0; r < MM; ++r) {
        if (r < m) {
            double v = q[r];
            const double n0 = colsum<NP>(v * v);
#pragma unroll
            for (int s2 = 0; s2 < r; ++s2) {
                const double d = colsum<NP>(q[s2] * v);
                Rm[r][s2] = d;
                v = fma(-d, q[s2], v);
            }
            const double nn = (r == 0) ? n0 : colsum<NP>(v * v);
            if (nn > 1.0e-24 * n0 && nn > 0.0) {
                double sq, rs;
                fast_sqrt_rsqrt(nn, sq, rs);
                Rm[r][r] = sq;
                q[r] = v * rs;
            } else {
                q[r] = 0.0;   // dependent (or zero) row: nothing new in its direction
            }
        } else {
            q[r] = 0.0;
        }
    }
    // I + M = Lh Lh'  (uniform scalars);  Y = Lh^-T;  Dh = Y - I
    double Lh[MM][MM], Y[MM][MM];
#pragma unroll
    for (int i = 0; i < MM; ++i)
#pragma unroll
        for (int j = 0; j < MM; ++j) {
            double acc = (i == j) ? 1.0 : 0.0;
            if (j <= i) {
#pragma unroll
                for (int r = 0; r < MM; ++r) acc = fma(Rm[r][i], Rm[r][j], acc);   // (I + Rh'Rh)[i][j]
            }
            Lh[i][j] = (j <= i) ? acc : 0.0;
        }
    double ild[MM];   // 1 / Lh[i][i]
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        double sq, rs;
        fast_sqrt_rsqrt(Lh[j][j], sq, rs);   // >= 1
        Lh[j][j] = sq;
        ild[j] = rs;
#pragma unroll
        for (int i = j + 1; i < MM; ++i) Lh[i][j] *= rs;
#pragma unroll
        for (int i = j + 1; i < MM; ++i)
#pragma unroll
            for (int k = j + 1; k <= i; ++k) Lh[i][k] = fma(-Lh[i][j], Lh[k][j], Lh[i][k]);
    }
    // Y = Lh^-T (upper triangular): column by column of Lh^-1, transposed
#pragma unroll
    for (int i = 0; i < MM; ++i)
#pragma unroll
        for (int j = 0; j < MM; ++j) Y[i][j] = 0.0;
#pragma unroll
    for (int col = 0; col < MM; ++col) {      // Linv[:, col] by forward substitution; Y[col][i] = Linv[i][col]
#pragma unroll
        for (int i = col; i < MM; ++i) {
            double acc = (i == col) ? 1.0 : 0.0;
#pragma unroll
            for (int k = col; k < i; ++k) acc = fma(-Lh[i][k], Y[col][k], acc);
            Y[col][i] = acc * ild[i];
        }
    }
    // t = Rh' bt - Qh ch;  u = (I + M)^-1 t = Y (Y' t)
    const double ch = valid ? cvec * dis : 0.0;
    double Qc[MM], t[MM], u[MM];
#pragma unroll
    for (int s2 = 0; s2 < MM; ++s2) {
        Qc[s2] = (has_c && s2 < m) ? colsum<NP>(q[s2] * ch) : 0.0;
        double acc = -Qc[s2];
#pragma unroll
        for (int r = 0; r < MM; ++r) acc = fma(Rm[r][s2], bt[r], acc);
        t[s2] = acc;
    }
    {
        double yt[MM];
#pragma unroll
        for (int i = 0; i < MM; ++i) {      // yt = Y' t   (Y' = Lh^-1, lower triangular: Y'[i][k] = Y[k][i])
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k <= i; ++k) acc = fma(Y[k][i], t[k], acc);
            yt[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < MM; ++i) {      // u = Y yt
            double acc = 0.0;
#pragma unroll
            for (int k = i; k < MM; ++k) acc = fma(Y[i][k], yt[k], acc);
            u[i] = acc;
        }
    }
    double xh = -ch;
#pragma unroll
    for (int s2 = 0; s2 < MM; ++s2) xh = fma(q[s2], u[s2] + Qc[s2], xh);
    x_out = valid ? xh * dis : 0.0;
    // J: F[s](c) = sum_r q[r](c) (Y - I)[r][s];  JT[j][c] = J[c][j] = dis_c (delta_cj + sum_s F[s](c) q[s](j))
    double F[MM];
#pragma unroll
    for (int s2 = 0; s2 < MM; ++s2) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < MM; ++r) acc = fma(q[r], Y[r][s2] - ((r == s2) ? 1.0 : 0.0), acc);
        F[s2] = acc * dis;
    }
    wave_sync();
    if (h == 0) {
#pragma unroll
        for (int s2 = 0; s2 < MM; ++s2) M1[s2 * S + c] = q[s2];
    }
    wave_sync();
#pragma unroll
    for (int jj = 0; jj < NP / HV; ++jj) {
        const int j = HV * jj + h;
        double acc = (j == c) ? dis : 0.0;
#pragma unroll
        for (int s2 = 0; s2 < MM; ++s2) acc = fma(F[s2], M1[s2 * S + j], acc);
        M2[j * S + c] = acc;
    }
    wave_sync();
}

// Pre (general H):  Hc = the accumulator tiles of H + eps I (NP = 32: factor_tiles32; NP > 32: the upper triangle of tiles, factor_tiles_wide),
// M1 is scratch.
template <int NP, bool PROF, bool BOX = false, bool LEAN = false>
__device__ int gi_solve(const WaveCtx<NP>& w_in, int nrows, double g, bool diag_h,
                        double hdiag, double (&Hc)[NP / WaveCtx<NP>::HV], bool has_box, double& lb, double& ub, int max_iter,
                        bool have_prev, double xprev, double& x_out, int& iters_out, long long* prof,
                        double& slack_out, bool prepared = false, double xprep = 0.0, int hotcode = -1, int* hot_out = nullptr,
                        int dense_rank_in = -1, int dense_neq_in = 0, double dense_x_in = 0.0, double dense_hinv_in = 0.0,
                        const LeanRows& lr = LeanRows()) {
    static_assert(!LEAN || (NP == 32 && BOX), "the lean path is a path of the 32-lane BOX instantiation");
    constexpr int HV = WaveCtx<NP>::HV, S = WaveCtx<NP>::S;
    const int n = LEAN ? 32 : w_in.n;
    double* M1 = w_in.M1;
    double* M2 = w_in.M2;
    double* V0 = w_in.V;
    double* V1 = w_in.V + WaveCtx<NP>::LW;
    lb = clamp_inf(lb);
    ub = clamp_inf(ub);
    double x;
    OSOT_PH_BEGIN();
    // round 6, 40-lane layout: a DENSE level under many equality rows that x_prev satisfies has taken the null-space method INSTEAD of
    // the H build, the factorisation and the row-by-row reflections (nullspace_dense_wide, called by the cascade AHEAD of the H build: its
    // rank, the number of equality rows it eliminated, the equality-constrained minimiser and diag(J2 J2') arrive here)
    const bool dense_ns = (NP == 40) && dense_rank_in >= 0;
    const int dense_rank = dense_rank_in, dense_neq = dense_neq_in;
    const double dense_hinv = dense_hinv_in;
    if (dense_ns) x = dense_x_in;
    {   // ---------------- factorisation phase (own scope: see the launder_i note below) ----------------
    WaveCtx<NP> w1 = w_in;
    { const int l1 = launder_i(WaveCtx<NP>::lane_of(w_in.c, w_in.h)); w1.c = WaveCtx<NP>::col_of(l1); w1.h = WaveCtx<NP>::half_of(l1); }
    if constexpr (LEAN) w1.n = 32;
    const WaveCtx<NP>& w = w1;
    const int c = w.c, h = w.h;
    const bool valid = LEAN || c < n;

    if (dense_ns) {
        // (nothing to factorise: J2' is in M2, x is the equality-constrained minimiser)
    } else if (prepared) {
        // JT is in M2 and the unconstrained minimiser is known already (lowrank_prepare32)
        x = xprep;
        OSOT_PH_END(PH_CHOL);
    } else if (diag_h) {
        // H + eps I diagonal (a level made of a Postural block only): L = sqrt(diag), JT = diag(1/L)
        const bool okd = !valid || (hdiag > 0.0);
        if (uniform_d(colsum<NP>(okd ? 0.0 : 1.0)) != 0.0) { x_out = 0.0; iters_out = 0; return QP_NOT_PD; }
        double sq = 1.0, rs = 1.0;
        if (valid) fast_sqrt_rsqrt(hdiag, sq, rs);
        for (int e = WaveCtx<NP>::lane_of(c, h); e < WaveCtx<NP>::ROWS * S; e += 64) M2[e] = 0.0;
        wave_sync();
        if (h == 0 && valid) M2[c * S + c] = rs;
        x = valid ? -g * rs * rs : 0.0;
        wave_sync();
        OSOT_PH_END(PH_CHOL);
    } else {
        int stf;
        if constexpr (NP > 32) {
            stf = factor_tiles_wide<NP, wide_tiles(NP)>(w, Hc, g, x);
        } else stf = factor_tiles32<false, false, LEAN>(w, Hc, g, x);
        stf = uniform_i(stf);
        if (stf != QP_SOLVED) { x_out = 0.0; iters_out = 0; return stf; }
        OSOT_PH_END(PH_CHOL);
        // (the substitution, NOT x = -J J'g: with H = A'A + eps I rank deficient, g lies in range(A') and the
        //  substitution keeps the exact cancellation in the eps-pivots that the explicit inverse loses -- the
        //  reference's own known-answer test TestQPOases.cpp:274-340 needs it at 1e-6)
    }

    }   // end of the factorisation phase
    // (the lane coordinates are re-derived here so that nothing computed for the factorisation stays live)
    WaveCtx<NP> w2 = w_in;
    { const int l2 = launder_i(WaveCtx<NP>::lane_of(w_in.c, w_in.h)); w2.c = WaveCtx<NP>::col_of(l2); w2.h = WaveCtx<NP>::half_of(l2); }
    if constexpr (LEAN) w2.n = 32;
    const WaveCtx<NP>& w = w2;
    const int c = w.c, h = w.h;
    const bool valid = LEAN || c < n;
    int iq = 0;          // size of the working set (wave-uniform)
    int Aq = -1;         // lane q < iq: code of the constraint at working-set position q
    double uq = 0.0;     // lane q < iq: its multiplier (inequalities only)
    int iters = 0;

    // ---- equalities first --------------------------------------------------------------------------
    // classify all rows in parallel (lane = row), then walk the equality rows with the next row's
    // elements already in flight (one HBM/L2 round trip per row would otherwise sit on the critical path)
    int n_eq = LEAN ? nrows : 0;   // (LEAN: every row of the implicit table is an equality, and the list is the table)
    bool local_eq = false;   // an equality among the level's task-local rows: x_prev does not satisfy it
    for (int r0 = 0; r0 < ((dense_ns || LEAN) ? 0 : nrows); r0 += 64) {
        const int r = r0 + WaveCtx<NP>::lane_of(c, h);
        bool is_eq = false, is_loc = false;
        if (r < nrows) {
            const double lo = w.rlo[r], up = w.rup[r];
            is_eq = (lo == up) && (lo > -kInfty) && (lo < kInfty);
            is_loc = is_eq && (w.rsrc[r] == -2);
            w.rowstate[r] = is_eq ? 3 : 0;
        }
        local_eq = local_eq || (wave_ballot(is_loc) != 0ull);
        const unsigned long long mask = wave_ballot(is_eq);
        if (is_eq) w.eqlist[n_eq + lanes_below(mask)] = r;
        n_eq += __builtin_popcountll(mask);
    }
    if constexpr (!LEAN) wave_sync();
    // many equalities under a diagonal Hessian, ALL satisfied by the previous level's solution (optimality rows and
    // global equality rows are; a task-local equality of this level is not: then the generic path runs): null-space
    // elimination instead of n_eq Householder updates of the full J (see nullspace_equalities32)
    bool used_nullspace = false;
    if (dense_ns) {
        // the rows' states as the walk above would have left them (the list itself was built ahead of the factorisation)
        for (int r0 = 0; r0 < nrows; r0 += 64) {
            const int r = r0 + WaveCtx<NP>::lane_of(c, h);
            if (r < nrows) {
                const double lo = w.rlo[r], up = w.rup[r];
                w.rowstate[r] = ((lo == up) && (lo > -kInfty) && (lo < kInfty)) ? 3 : 0;
            }
        }
        wave_sync();
        iq = dense_rank; iters += dense_neq; used_nullspace = true;
    }
    if (NP == 32 && diag_h && have_prev && !local_eq && n_eq >= 8 && n_eq <= 32 && n - n_eq <= kNullMax) {
        const int r_ns = uniform_i(nullspace_equalities32<PROF, LEAN>(reinterpret_cast<const WaveCtx<32>&>(w), n_eq, hdiag, g, xprev, x, prof, lr));
        if (r_ns >= 0) { iq = r_ns; iters += n_eq; used_nullspace = true; n_eq = 0; }
    }
    if constexpr (NP == 40) {     // round 6: the 40-lane layout (the reference's 35-coordinate COMAN) takes the same route
        if (diag_h && have_prev && !local_eq && n_eq >= 8 && n_eq <= 32 && n - n_eq <= kNullMax) {
            const int r_ns = uniform_i(nullspace_equalities_wide<NP, PROF>(w, n_eq, hdiag, g, xprev, x, prof));
            if (r_ns >= 0) { iq = r_ns; iters += n_eq; used_nullspace = true; n_eq = 0; }
        }
    }
    // (uniform_i / uniform_d below: table entries and reduction results ARE wave-uniform, said so that the loop's control flow
    // and its counters stay on the scalar unit -- see osot_team.h)
    // The equality rows are added IN PAIRS wherever two consecutive rows are both (clearly) independent of the working set: a pass
    // over JT is what an addition costs (above all at one wavefront per SIMD: an LDS sweep nothing hides), and a pair needs
    // three of them instead of six --
    //   d_a = J'a and d_b = J'b in one pass (jt_rows_dot2);
    //   b after a's reflection H_a = I - beta_a v_a v_a' without touching J: d_b' = H_a d_b is lane-local after one reduction,
    //   its slack loses t_a (b'z_a) = t_a (d_b . d2_a), and z_b = (J2 H_a) d2_b' = J2 d2_b' - beta_a (v_a . d2_b') (J2 v_a): so
    //   z_a = J2 d2_a and J2 d2_b' in one pass over the UNCHANGED J (jt_cols_dot2), the correction lane-local;
    //   both reflections as one rank-2 update (householder_apply2), with w_b = (J2 H_a) v_b from z_b and row iq+1 of JT.
    // A row that is dependent, or a pair of which either row is not WELL clear of the dependency threshold (nd2 <= 1e-6 dd: the finer
    // tests look at J as it is AFTER the partner's reflection, and an ill-conditioned level needs the one-row path's accuracy), goes
    // through the one-row path as before.
    constexpr double kPairTol = 1.0e-6;
    double* V2p = w.V + 2 * WaveCtx<NP>::LW;
    double* V3p = w.V + 3 * WaveCtx<NP>::LW;
    double rq[4];    // rows e .. e+3 of the list at my column, requested ahead of their use
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (LEAN) rq[i] = (i < n_eq) ? lean_row_elem(lr, i, w.safe_row, c) : 0.0;
        else rq[i] = (i < n_eq) ? row_elem<NP>(w, uniform_i(w.eqlist[i]), c) : 0.0;
    }
    for (int e = 0; e < n_eq;) {
        // (the 64-lane layouts only: at NP = 32 -- two wavefronts per SIMD, three such rows at config 3 -- the pair's code and registers
        //  cost more than its passes save: measured -1.4 % on the headline batch with pairs on)
        const bool have_b = (NP > 32) && e + 1 < n_eq;
        const int r = LEAN ? e : uniform_i(w.eqlist[e]);
        const int rb = LEAN ? e : uniform_i(w.eqlist[have_b ? e + 1 : e]);
        const double a = rq[0], b = have_b ? rq[1] : 0.0;
        const double lo = LEAN ? 0.0 : uniform_d(w.rlo[r]), lob = LEAN ? 0.0 : uniform_d(w.rlo[rb]);
        const int src = LEAN ? 0 : uniform_i(w.rsrc[r]), srcb = LEAN ? 0 : uniform_i(w.rsrc[rb]);   // (LEAN: optimality rows all)
        // right-hand side relative to x: lo - a'x, or a'(x_prev - x) for an optimality row (x_prev, the solution of the
        // last level solved, satisfies a'x_prev = a'x_j for the rows of every level j above it)
        const double xref = (src >= 0) ? xprev : 0.0, xrefb = (srcb >= 0) ? xprev : 0.0;
        OSOT_SUB_BEGIN();
        if (h == 0) { V0[c] = a; V3p[c] = b; }
        wave_sync();
        double d, db;
        if (have_b) jt_rows_dot2<NP>(w, V0, V3p, d, db);
        else { d = jt_rows_dot<NP>(w, V0); db = 0.0; }
        OSOT_SUB_END(PH_EQ_D);
        const double d2 = (c >= iq) ? d : 0.0;
        double dd, nd2;
        colsum2<NP>(d * d, d2 * d2, dd, nd2);
        dd = uniform_d(dd); nd2 = uniform_d(nd2);
        double ra, rbx;      // a'(xref - x) and b'(xrefb - x)
        colsum2<NP>(a * (xref - x), b * (xrefb - x), ra, rbx);
        const double resid = lo + uniform_d(ra);
        OSOT_SUB_END(PH_EQ_RED);
        int adv = 1;
        const bool ok_a = direction_is_independent<NP>(w, nd2, dd, d2, a, iq);
        if (!ok_a) {   // row is (numerically) a combination of the rows already in
            // an optimality row of an upper level (src >= 0) is consistent BY CONSTRUCTION (x of that level
            // satisfies all of them, iHQP.cpp:164-170): a residual there is round-off of an ill-conditioned level
            // (default eps 4.4e-11: O(1e-16 / eps)), never infeasibility
            if (!(src >= 0 || fabs(resid) <= kEqTol * fmax(1.0, fabs(lo)))) { x_out = x; iters_out = iters; return QP_INFEASIBLE; }
            // redundant and consistent: nothing to add
        } else {
            // the reflection of a (householder_add's scalars)
            const double d_iq = bcast(d, iq);
            double nrm, rnrm;
            fast_sqrt_rsqrt(nd2, nrm, rnrm);
            const double alpha = (d_iq > 0.0) ? -nrm : nrm;
            const double va = (c > iq) ? d2 : ((c == iq) ? d_iq - alpha : 0.0);
            const double beta = fast_rcp(nd2 - alpha * d_iq);
            const double ta = resid * fast_rcp(nd2);
            bool pair = false;
            double d2b = 0.0, ddb = 0.0, nd2b = 0.0, dbp = 0.0, residb = 0.0;
            if (have_b) {
                // b against the working set WITH a: d_b' = H_a d_b; slack of b at x + t_a z_a
                double sab, bza;
                colsum2<NP>(va * db, db * d2, sab, bza);      // v_a . d_b  and  b'z_a = d_b . d2_a
                sab = uniform_d(sab); bza = uniform_d(bza);
                dbp = fma(-beta * sab, va, db);
                d2b = (c >= iq + 1) ? dbp : 0.0;
                colsum2<NP>(dbp * dbp, d2b * d2b, ddb, nd2b);
                ddb = uniform_d(ddb); nd2b = uniform_d(nd2b);
                residb = lob + uniform_d(rbx) - ta * bza;
                // (well clear of the dependency threshold, BOTH of them: on an ill-conditioned level -- the default eps, where
                //  J spans ten decades -- the pair's extra algebra costs accuracy that the one-row path keeps; there the rows go
                //  one by one as they always did: default_eps_stuck_instances, hardware)
                pair = (nd2 > kPairTol * dd) && (nd2b > kPairTol * ddb);
            }
            if (pair) {
                const double d_iqb = bcast(dbp, iq + 1);
                double nrmb, rnrmb;
                fast_sqrt_rsqrt(nd2b, nrmb, rnrmb);
                const double alphab = (d_iqb > 0.0) ? -nrmb : nrmb;
                const double vb = (c > iq + 1) ? d2b : ((c == iq + 1) ? d_iqb - alphab : 0.0);
                const double betab = fast_rcp(nd2b - alphab * d_iqb);
                const double tb = residb * fast_rcp(nd2b);
                // z_b = (J2 H_a) d2_b' = J2 d2_b' - beta_a (v_a . d2_b') (J2 v_a): the product with the UNCHANGED J takes the columns from
                // iq + 1 on only (d2_b' is zero at iq), the correction is the rank-1 term the reflection of a would have put into J
                const double s2 = uniform_d(colsum<NP>(va * d2b));
                const double va_next = bcast(va, iq + 1);        // v_a[iq + 1]
                const double m_iq = M2[iq * S + c], m_iq1 = M2[(iq + 1) * S + c];
                if (h == 0) { V1[c] = d2; V3p[c] = d2b; V2p[c] = va * beta; V0[c] = vb * betab; }
                wave_sync();
                double z, zb;
                jt_cols_dot2<NP>(w, V1, V3p, z, zb);
                const double wa = z - alpha * m_iq;                                              // J2 v_a
                zb = fma(-beta * s2, wa, zb);
                x += ta * z;
                x += tb * zb;
                OSOT_SUB_END(PH_EQ_Z);
                const double wb = zb - alphab * fma(-beta * va_next, wa, m_iq1);                   // (J2 H_a) v_b
                householder_apply2<NP>(w, V2p, V0, wa, wb, iq);
                if (h == 0) {   // the pair's two columns of R (refine_on_working_set)
                    if (c < iq) { M1[ridx<NP>(c, iq)] = d; M1[ridx<NP>(c, iq + 1)] = dbp; }
                    else if (c == iq) { M1[ridx<NP>(iq, iq)] = alpha; M1[ridx<NP>(iq, iq + 1)] = dbp; }
                    else if (c == iq + 1) M1[ridx<NP>(iq + 1, iq + 1)] = alphab;
                }
                OSOT_SUB_END(PH_EQ_HH);
                if (c == iq) Aq = -2 - r;
                if (c == iq + 1) Aq = -2 - rb;
                iq += 2;
                iters += 2;
                adv = 2;
            } else {
                if (h == 0) V1[c] = d2;
                wave_sync();
                const double z = jt_cols_dot<NP>(w, V1);
                x += ta * z;
                OSOT_SUB_END(PH_EQ_Z);
                householder_add<NP, true>(w, d, d2, z, nd2, iq);    // (the equality columns of R: read by refine_on_working_set only)
                OSOT_SUB_END(PH_EQ_HH);
                if (c == iq) Aq = -2 - r;
                iq++;
                iters++;
            }
        }
        // the rows ahead: shift the queue by what was consumed and request the missing ones
        // (rows go in pairs -- adv == 2 -- in the 64-lane layouts only; LEAN is NP = 32, see the static_assert above: the pair arm,
        //  which reads the list the lean path never fills, is not compiled into it)
        if (LEAN || adv == 1) {
            rq[0] = rq[1]; rq[1] = rq[2]; rq[2] = rq[3];
            if constexpr (LEAN) rq[3] = (e + 4 < n_eq) ? lean_row_elem(lr, e + 4, w.safe_row, c) : 0.0;
            else rq[3] = (e + 4 < n_eq) ? row_elem<NP>(w, uniform_i(w.eqlist[e + 4]), c) : 0.0;
        } else {
            rq[0] = rq[2]; rq[1] = rq[3];
            rq[2] = (e + 4 < n_eq) ? row_elem<NP>(w, uniform_i(w.eqlist[e + 4]), c) : 0.0;
            rq[3] = (e + 5 < n_eq) ? row_elem<NP>(w, uniform_i(w.eqlist[e + 5]), c) : 0.0;
        }
        e += adv;
    }
    const int me = iq;
    wave_sync();
    OSOT_PH_END(PH_EQ);

    // ---- inequality loop -----------------------------------------------------------------------------
    WaveCtx<NP> w3 = w_in;
    { const int l3 = launder_i(WaveCtx<NP>::lane_of(w_in.c, w_in.h)); w3.c = WaveCtx<NP>::col_of(l3); w3.h = WaveCtx<NP>::half_of(l3); }
    if constexpr (LEAN) w3.n = 32;
    // after the null-space path the equality rows of J are zero, so |J'n|^2 no longer measures n'H^-1 n;
    // the diagonal of H^-1 does (hinv > 0 selects that in the dependency test)
    const double hinv = dense_ns ? dense_hinv : ((used_nullspace && valid) ? fast_rcp(hdiag) : 0.0);
    return gi_inequalities<NP, PROF, BOX, LEAN>(w3, nrows, x, iq, me, Aq, uq, iters, has_box, lb, ub, max_iter, used_nullspace, hinv,
                                     have_prev, xprev, slack_out, x_out, iters_out, prof, hotcode, hot_out, lr);
}

template <int NP, bool PROF, bool BOX, bool LEAN>
__device__ int gi_inequalities(const WaveCtx<NP>& w, int nrows, double x, int iq, const int me, int Aq, double uq,
                               int iters, bool has_box, double& lb, double& ub, int max_iter, bool diag_dd, double hinv,
                               bool have_prev, double xprev, double& slack_out, double& x_out, int& iters_out, long long* prof,
                               int hotcode, int* hot_out, const LeanRows& lr) {
    static_assert(!LEAN || (NP == 32 && BOX), "the lean path is a path of the 32-lane BOX instantiation");
    constexpr int S = WaveCtx<NP>::S;
    const int c = w.c, h = w.h, n = LEAN ? 32 : w.n;
    const bool valid = LEAN || c < n;
    double* M1 = w.M1;
    double* M2 = w.M2;
    double* V0 = w.V;
    double* V1 = w.V + WaveCtx<NP>::LW;
    int box_state = 0;   // lane c: 0 free, 1 lower bound active, 2 upper bound active
    OSOT_PH_BEGIN();
    // the stored rows that can ever be violated (not equalities, at least one finite bound), in row order;
    // the equality list is dead by now, its LDS array is reused
    int n_gen = 0;
    bool any_unit = false;   // is there a unit row that can ever be violated?  (none: its pass is skipped)
    for (int r0 = 0; r0 < (BOX ? 0 : nrows); r0 += 64) {
        const int r = r0 + WaveCtx<NP>::lane_of(c, h);
        bool is_gen = false, is_unit = false;
        if (r < nrows) {
            const double lo = w.rlo[r], up = w.rup[r];
            const bool live = (w.rowstate[r] != 3) && ((lo > -kInfty) || (up < kInfty));
            const bool unit = (w.rptr[r] & 1ull) != 0ull;
            is_gen = live && !unit;
            is_unit = live && unit;
        }
        wave_sync();
        const unsigned long long mask = wave_ballot(is_gen);
        if (is_gen) w.eqlist[n_gen + lanes_below(mask)] = r;
        n_gen += __builtin_popcountll(mask);
        any_unit = any_unit || (wave_ballot(is_unit) != 0ull);
    }
    wave_sync();
    int status = QP_SOLVED;
    const int kNone = 0x7fffffff;
    // first trip of a cascade level below the first: the scan below runs once on x_prev and, instead of looking for
    // violations, gives every inequality the feasibility margin described at kFeasMargin (task-local rows of this level
    // excepted: x_prev owes them nothing).  The moved bounds stay moved for the lower levels of the instance.
    bool margin_pass = have_prev;
    if (margin_pass && has_box && valid) {
        if (lb > -kInfty) lb = fmin(lb, xprev - kFeasMargin * fmax(1.0, fabs(lb)));
        if (ub < kInfty) ub = fmax(ub, xprev + kFeasMargin * fmax(1.0, fabs(ub)));
    }
    // HOT START (the reference's qpOASES back-end keeps its working set from one control cycle to the next:
    // QPOasesBackEnd.cpp:258-285 hotstart -> SQProblem.cpp:149-193).  hotcode = lane q's entry of the inequality working set
    // this level ended with at the instance's previous solve (-1: none).  Those constraints are re-added first, each as if it
    // were an equality (a SIGNED step onto its boundary, multipliers updated by the same dual direction, no scan and no
    // ratio test); then every constraint whose multiplier came out negative is taken out again by the reverse of an
    // addition (x' = x - u_k z, u' = u + u_k r with z, r of the normal against the factors of the set without it).  Each
    // removal moves to the minimiser over a subset, f strictly decreases, so the phase ends; what is left is an S-pair
    // (x minimises f on the working set, all multipliers >= 0) -- a valid state of the dual method, which then goes on
    // as from a cold start.  The minimiser is unique, so the answer is the cold one up to round-off; what changes is the
    // number of iterations (no add-then-drop churn, no scans for the constraints that stay active from cycle to cycle).
    int hot_n = __builtin_popcountll(wave_ballot(hotcode >= 0 && h == 0));
    int hot_i = 0;
    bool hot_check = false;     // hot additions were made: their multipliers have to be looked at
    // A STALE hot list must not cost more than it can save (round 4; the launch is its longest instance): the multipliers are looked
    // at after every kHotBatch additions, and when at least kHotAbandon of them AND a quarter of the additions made so far are negative
    // the rest of the list is not tried -- the instance takes out what does not belong (below) and goes on as from a cold start from
    // the S-pair it has reached.  Nothing is removed at such a look: a PARTIAL working set can show a negative multiplier that the
    // complete one does not (on an exact repeat of a cycle the whole list goes in, as before).
    constexpr int kHotBatch = 4, kHotAbandon = 3;
    int hot_since_check = 0, hot_added = 0;
    // table entries of the hot list's rows, lane q = entry q, fetched in ONE round trip when the first hot trip starts (the
    // table may live in device memory: bound, state and row address were three dependent loads in front of every hot trip)
    bool hm_loaded = false;
    double hm_bnd = 0.0;
    int hm_state = 0;
    unsigned long long hm_ptr = 0ull;
    int refine_left = kRefineMax;
    constexpr double kHotDropTol = 1.0e-13;   // a multiplier below -kHotDropTol max|u| is negative (above: round-off of zero)
    for (;;) {
        OSOT_SUB_BEGIN();
        // trip kind: 0 = scan for the most violated constraint (the dual method proper), 1 = re-add the next constraint of the
        // previous cycle's working set, 2 = take out a hot constraint whose multiplier is negative
        int mode = 0;
        double cand = 0.0;
        int code = kNone;
        double u_rev = 0.0;
        unsigned long long hot_ptr = 0ull;    // mode 1, a row: its table entry (from the list's metadata)
        const bool hot_check_now = hot_check && (hot_i >= hot_n || hot_since_check >= kHotBatch);
        if (!margin_pass && hot_i < hot_n && !hot_check_now) {
            if (!hm_loaded) {
                hm_loaded = true;
                if (hotcode >= 2 * n && hotcode < 2 * n + 2 * nrows) {
                    const int rq = (hotcode - 2 * n) >> 1;
                    hm_bnd = (hotcode & 1) ? w.rup[rq] : w.rlo[rq];
                    hm_state = w.rowstate[rq];
                    hm_ptr = w.rptr[rq];
                }
            }
            const int hq = hot_i;      // (entry hq lives in lane hq)
            code = bcast_i(hotcode, hot_i);
            hot_i++;
            mode = 1;
            // still a constraint of this level's problem, with a finite bound on that side, and not in the working set?
            bool okc = false;
            if (code >= 0 && code < 2 * n) {
                const int var = (code < n) ? code : code - n;
                const double bnd = bcast((code < n) ? lb : ub, var);
                okc = has_box && (bcast_i(box_state, var) == 0) && ((code < n) ? (bnd > -kInfty) : (bnd < kInfty));
            } else if (code >= 2 * n && code < 2 * n + 2 * nrows) {
                const double bnd = bcast(hm_bnd, hq);
                okc = (bcast_i(hm_state, hq) == 0) && ((code & 1) ? (bnd < kInfty) : (bnd > -kInfty));
                hot_ptr = ((unsigned long long)(unsigned)bcast_i((int)(hm_ptr >> 32), hq) << 32) | (unsigned long long)(unsigned)bcast_i((int)(hm_ptr & 0xffffffffull), hq);
            }
            if (!okc) continue;
        } else if (!margin_pass && hot_check) {
            const bool mine = (c >= me && c < iq);
            double um = mine ? uq : INFINITY;
            int pos = c;
            const double uabs = uniform_d(colmax<NP>(mine ? fabs(uq) : 0.0));
            if (hot_i < hot_n) {      // a look in the middle of the list: count, do not remove
                const int nneg = __builtin_popcountll(wave_ballot(mine && h == 0 && uq < -kHotDropTol * uabs));
                hot_since_check = 0;
                if (nneg >= kHotAbandon && 4 * nneg >= hot_added) hot_n = hot_i;
                continue;
            }
            colargmin<NP>(um, pos);
            pos = uniform_i(pos);
            um = bcast(um, 0);
            if (!(um < -kHotDropTol * uabs)) { hot_check = false; hot_since_check = 0; continue; }
            mode = 2;
            u_rev = um;
            code = bcast_i(Aq, pos);
            if (code < 2 * n) { if (c == (code < n ? code : code - n)) box_state = 0; }
            else { if (c == 0 && h == 0) w.rowstate[(code - 2 * n) >> 1] = 0; }
            drop_constraint<NP>(w, pos, iq, Aq, uq);
            wave_sync();
        } else {
        // most violated constraint outside the working set (eiquadprog.hpp:300-315 picks the same)
        if (has_box && valid) {
            if (box_state != 1 && lb > -kInfty) {
                const double s = x - lb;
                if (s < -kViolTol * fmax(1.0, fabs(lb)) && s < cand) { cand = s; code = c; }
            }
            if (box_state != 2 && ub < kInfty) {
                const double s = ub - x;
                if (s < -kViolTol * fmax(1.0, fabs(ub)) && s < cand) { cand = s; code = n + c; }
            }
        }
        // unit rows (implicit e_i rows: acceleration joint/velocity limits) are checked 64 rows at a time,
        // lane = row, against a staged copy of x: they cost no reduction at all
        if (any_unit || n_gen > 0) {
            if (h == 0) V0[c] = margin_pass ? xprev : x;
            wave_sync();
        }
        if (any_unit) {
            const int lane = WaveCtx<NP>::lane_of(c, h);
            for (int r0 = 0; r0 < nrows; r0 += 64) {
                const int r = r0 + lane;
                if (r < nrows) {
                    const unsigned long long pr = w.rptr[r];
                    const int st = w.rowstate[r];
                    const int idx = (int)(pr >> 1);
                    if ((pr & 1ull) && st != 3 && idx < n) {
                        const double lo = w.rlo[r], up = w.rup[r];
                        const double ax = V0[idx];
                        if (margin_pass) {
                            if (w.rsrc[r] != -2) {
                                if (lo > -kInfty) w.rlo[r] = fmin(lo, ax - kFeasMargin * fmax(1.0, fabs(lo)));
                                if (up < kInfty) w.rup[r] = fmax(up, ax + kFeasMargin * fmax(1.0, fabs(up)));
                            }
                        } else {
                        if (st != 1 && lo > -kInfty) {
                            const double s = ax - lo;
                            if (s < -kViolTol * fmax(1.0, fabs(lo)) && s < cand) { cand = s; code = 2 * n + 2 * r; }
                        }
                        if (st != 2 && up < kInfty) {
                            const double s = up - ax;
                            if (s < -kViolTol * fmax(1.0, fabs(up)) && s < cand) { cand = s; code = 2 * n + 2 * r + 1; }
                        }
                        }
                    }
                }
            }
        }
        // stored inequality rows, lane = row, 64 rows at a time: each lane walks its own row against the staged
        // x (no cross-lane reduction at all).  Consecutive elements of a row share a cache line, so after the
        // first touch the walk is served from the CU's vector L1.
        // Few stored rows (round 5; BASELINE config 4's sixteen collision rows): FOUR lanes per row, each a quarter of the columns --
        // the walk is one round trip of NP / 4 loads per lane and a two-stage quad reduction where lane = row needs two round
        // trips of sixteen (the scan is a chain of L1 / L2 latencies: 2.7 k cycles per scan at config 4, 14 % of its job)
        const bool quad_scan = NP == 32 && n_gen > 0 && n_gen <= 16;
        if (quad_scan) {
            const int lane = WaveCtx<NP>::lane_of(c, h);
            const int gi = lane >> 2, part = lane & 3;
            const bool on = gi < n_gen;
            const int r = w.eqlist[on ? gi : 0];
            const auto* row = OSOT_GLOBAL_F64(w.rptr[r]);
            constexpr int QC = NP / 4;
            double e[QC];
#pragma unroll
            for (int t = 0; t < QC; ++t) { const int col = part * QC + t; e[t] = row[(col < n) ? col : 0]; }
            double a0 = 0.0, a1 = 0.0;
#pragma unroll
            for (int t = 0; t < QC; t += 2) {
                const int col = part * QC + t;
                a0 = fma((col < n) ? e[t] : 0.0, V0[col], a0);
                a1 = fma((col + 1 < n) ? e[t + 1] : 0.0, V0[col + 1], a1);
            }
            const double ax = quad_sum(a0 + a1);
            if (on && part == 0) {
                const int st = w.rowstate[r];
                const double lo = w.rlo[r], up = w.rup[r];
                if (margin_pass) {
                    if (w.rsrc[r] != -2) {
                        if (lo > -kInfty) w.rlo[r] = fmin(lo, ax - kFeasMargin * fmax(1.0, fabs(lo)));
                        if (up < kInfty) w.rup[r] = fmax(up, ax + kFeasMargin * fmax(1.0, fabs(up)));
                    }
                } else {
                    if (st != 1 && lo > -kInfty) {
                        const double s = ax - lo;
                        if (s < -kViolTol * fmax(1.0, fabs(lo)) && s < cand) { cand = s; code = 2 * n + 2 * r; }
                    }
                    if (st != 2 && up < kInfty) {
                        const double s = up - ax;
                        if (s < -kViolTol * fmax(1.0, fabs(up)) && s < cand) { cand = s; code = 2 * n + 2 * r + 1; }
                    }
                }
            }
        }
        for (int g0 = 0; g0 < (quad_scan ? 0 : n_gen); g0 += 64) {
            const int gi = g0 + WaveCtx<NP>::lane_of(c, h);
            if (gi < n_gen) {
                const int r = w.eqlist[gi];
                const auto* row = OSOT_GLOBAL_F64(w.rptr[r]);
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                int cc = 0;
                // SC loads per trip: the walk is a chain of L1/L2 round trips, only loads in flight shorten it
#ifndef OSOT_SCAN_SC
#define OSOT_SCAN_SC 16
#endif
#ifndef OSOT_SCAN_SC40
#define OSOT_SCAN_SC40 20
#endif
#ifndef OSOT_SCAN_SC56
#define OSOT_SCAN_SC56 28   // (the 56-row layout: 28 loads per trip of the row walk -- two trips for n = 50 instead of four: 565 -> 546-553 us per config-5 launch; 52: 572)
#endif
                constexpr int SC = (NP == 56) ? OSOT_SCAN_SC56 : ((NP == 40) ? OSOT_SCAN_SC40 : OSOT_SCAN_SC);
                for (; cc + SC <= n; cc += SC) {
                    double e[SC];
#pragma unroll
                    for (int t = 0; t < SC; ++t) e[t] = row[cc + t];
#pragma unroll
                    for (int t = 0; t < SC; t += 4) {
                        a0 = fma(e[t], V0[cc + t], a0); a1 = fma(e[t + 1], V0[cc + t + 1], a1);
                        a2 = fma(e[t + 2], V0[cc + t + 2], a2); a3 = fma(e[t + 3], V0[cc + t + 3], a3);
                    }
                }
                if (cc < n) {   // the ragged tail in one more round trip (clamped addresses, masked terms)
                    double e[SC];
#pragma unroll
                    for (int t = 0; t < SC; ++t) e[t] = row[(cc + t < n) ? cc + t : n - 1];
#pragma unroll
                    for (int t = 0; t < SC; t += 4) {
                        a0 = fma((cc + t < n) ? e[t] : 0.0, V0[cc + t], a0);
                        a1 = fma((cc + t + 1 < n) ? e[t + 1] : 0.0, V0[cc + t + 1], a1);
                        a2 = fma((cc + t + 2 < n) ? e[t + 2] : 0.0, V0[cc + t + 2], a2);
                        a3 = fma((cc + t + 3 < n) ? e[t + 3] : 0.0, V0[cc + t + 3], a3);
                    }
                }
                const double ax = (a0 + a1) + (a2 + a3);
                const int st = w.rowstate[r];
                const double lo = w.rlo[r], up = w.rup[r];
                if (margin_pass) {
                    if (w.rsrc[r] != -2) {
                        if (lo > -kInfty) w.rlo[r] = fmin(lo, ax - kFeasMargin * fmax(1.0, fabs(lo)));
                        if (up < kInfty) w.rup[r] = fmax(up, ax + kFeasMargin * fmax(1.0, fabs(up)));
                    }
                } else {
                if (st != 1 && lo > -kInfty) {
                    const double s = ax - lo;
                    if (s < -kViolTol * fmax(1.0, fabs(lo)) && s < cand) { cand = s; code = 2 * n + 2 * r; }
                }
                if (st != 2 && up < kInfty) {
                    const double s = up - ax;
                    if (s < -kViolTol * fmax(1.0, fabs(up)) && s < cand) { cand = s; code = 2 * n + 2 * r + 1; }
                }
                }
            }
        }
        if (margin_pass) { margin_pass = false; wave_sync(); continue; }   // bounds moved: now the real scan
        // all 64 lanes when the unit-row / stored-row passes ran (they hold different rows in the two halves);
        // box candidates alone are replicated over the halves, so the 32-lane network does
        if (any_unit || n_gen > 0 || NP > 32) colargmin<64>(cand, code);
        else colargmin<NP>(cand, code);
        code = uniform_i(code);
        OSOT_SUB_END(PH_IN_SCAN);
        if (code == kNone) break;   // primal feasible: optimal
        }   // (end of the scan trip)
        if (++iters > max_iter) { status = QP_MAX_ITER; break; }

        const int ip = uniform_i(code);
        double s_ip = bcast(cand, 0);
        double u_new = 0.0;
        const bool ip_box = BOX || ip < 2 * n;
        const int ip_var = ip_box ? (ip < n ? ip : ip - n) : 0;
        const int ip_row = ip_box ? 0 : (ip - 2 * n) >> 1;
        const double ip_sgn = ip_box ? (ip < n ? 1.0 : -1.0) : ((ip & 1) ? -1.0 : 1.0);
        double np = 0.0;   // lane-distributed normal (general rows only)
        const unsigned long long ip_ptr = ip_box ? 0ull : ((mode == 1) ? hot_ptr : w.rptr[ip_row]);
        if (!ip_box) np = ip_sgn * row_elem_p<NP>(w, ip_ptr, c);
        const bool ip_unit = uniform_b(!ip_box && (ip_ptr & 1ull));      // unit row e_i: d = J'n is a row read, like a bound
        const int ip_uidx = uniform_i(ip_unit ? (int)(ip_ptr >> 1) : 0);
        if (mode == 1) {   // slack of the hot constraint at the current iterate (either sign)
            if (ip_box) s_ip = bcast((ip < n) ? (x - lb) : (ub - x), ip_var);
            else {
                const double ax = colsum<NP>(np * x);   // = sgn * a'x
                s_ip = bcast((ip & 1) ? (w.rup[ip_row] + ax) : (ax - w.rlo[ip_row]), 0);
            }
        }

        bool failed = false, degenerate_done = false;
        for (;;) {
            // d = J' n
            double d;
            if (ip_box) {
                d = ip_sgn * M2[c * S + ip_var];
            } else if (ip_unit) {
                d = ip_sgn * M2[c * S + ip_uidx];
            } else {
                if (h == 0) V0[c] = np;
                wave_sync();
                d = jt_rows_dot<NP>(w, V0);
            }
            const double d2 = (c >= iq) ? d : 0.0;
            double dd, nd2;
            if (diag_dd) {   // n' H^-1 n from the diagonal of H^-1
                nd2 = uniform_d(colsum<NP>(d2 * d2));
                dd = ip_box ? bcast(hinv, ip_var) : (ip_unit ? bcast(hinv, ip_uidx) : uniform_d(colsum<NP>(np * np * hinv)));
            } else {
                colsum2<NP>(d * d, d2 * d2, dd, nd2);
                dd = uniform_d(dd); nd2 = uniform_d(nd2);
            }
            const bool z_ok = direction_is_independent<NP>(w, nd2, dd, d2,
                                                           ip_box ? ((c == ip_var) ? 1.0 : 0.0) : (ip_unit ? ((c == ip_uidx) ? 1.0 : 0.0) : np), iq);
            OSOT_SUB_END(PH_IN_D);
            // z = J2 d2 : primal step direction
            if (h == 0) V1[c] = d2;
            wave_sync();
            double z;
            if constexpr (NP > 32) z = (iq >= 16) ? jt_cols_dot_tail64<NP>(w, V1, iq) : jt_cols_dot<NP>(w, V1);   // d2 = 0 below iq
            else z = jt_cols_dot<NP>(w, V1);
            OSOT_SUB_END(PH_IN_Z);
            // r = R^-1 d1 restricted to the inequality part [me, iq): dual step direction.  The reciprocals of
            // the diagonal are formed lane-parallel up front and the columns of R are fetched four steps
            // ahead, so that a step of the serial chain is readlane -> mul -> fma only.
            double rr = 0.0;
            double rmax = 0.0;   // max |r_j| (uniform): picked up on the way, every r_j passes through a broadcast
            if (iq > me) {       // (no inequality in the working set yet -- the first addition of most levels: no dual direction)
                // the residual is carried SCALED by the reciprocal diagonal, e_c = d1_c / R_cc, and so are the column entries
                // (off the chain: the columns are fetched four steps ahead): a step of the serial chain is then
                // readlane -> fma only (the unscaled form had a multiplication by 1 / R_jj in front of every broadcast)
                const bool mine = (c >= me && c < iq);
                const double rinv = mine ? fast_rcp(M1[ridx<NP>(c, c)]) : 0.0;
                double e = mine ? d * rinv : 0.0;
                const int rrow = mine ? c : 0;                                  // in-range row for idle lanes
                for (int j0 = iq - 1; j0 >= me; j0 -= 4) {
                    double rc[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {     // R[c][j] is only used for c < j: rows above the diagonal exist in every column
                        const int jj = (j0 - t >= 0) ? j0 - t : 0;
                        rc[t] = M1[ridx<NP>((rrow <= jj) ? rrow : 0, jj)] * rinv;
                    }
                    // TWO columns per step of the chain: r_j = e_j and r_(j-1) = e_(j-1) - Rhat[j-1][j] r_j come from three
                    // independent broadcasts and one uniform fma (the very operation lane j-1 would do on itself: bit-identical),
                    // then every lane applies both columns -- one broadcast latency per pair instead of one per column
                    // (measured +1.5 % on the headline batch; preparing the reflection of the trip under its z pass instead of
                    // after the step decision was measured too and lost 2 %: a third of the passes end in a partial step)
#pragma unroll
                    for (int t = 0; t < 4; t += 2) {
                        const int j = j0 - t;
                        if (j >= me) {
                            const double rj = bcast(e, j);
                            rmax = fmax(rmax, fabs(rj));
                            if (c == j) rr = rj;
                            if (j - 1 >= me) {
                                const double rjm1 = fma(-bcast(rc[t], j - 1), rj, bcast(e, j - 1));
                                rmax = fmax(rmax, fabs(rjm1));
                                if (c == j - 1) rr = rjm1;
                                if (mine && c < j - 1) e = fma(-rc[t + 1], rjm1, fma(-rc[t], rj, e));
                            }
                        }
                    }
                }
            }
            // step lengths (eiquadprog.hpp:343-366).  An entry of r counts as positive only above round-off of the largest
            // one (kRatioTol): r = R^-1 d1 carries ~1e-16 cond(R) of noise, and a noise-level "positive" entry that happens to
            // be the only one gives a dual step of u / r ~ 1e8 that wrecks every multiplier (seen in the closed-loop sweep at
            // the default eps; qpOASES guards its ratio tests the same way, epsNum / epsDen in Constants.hpp)
            if (mode == 2) {   // reverse of the addition of a hot constraint whose multiplier u_rev is negative
                if (z_ok) x -= u_rev * z;
                if (c >= me && c < iq) uq += u_rev * rr;
                OSOT_SUB_END(PH_IN_DROP);
                break;
            }
            if (mode == 1 && !z_ok) break;   // in the span of the working set by now: left to the scan
            double t1 = INFINITY;
            int lpos = c;
            if (mode == 0 && iq > me) {
                t1 = (c >= me && c < iq && rr > kRatioTol * rmax) ? fast_div(fmax(uq, 0.0), rr) : INFINITY;
                colargmin<NP>(t1, lpos);
                lpos = uniform_i(lpos);
                t1 = bcast(t1, 0);
            }
            const double t2 = z_ok ? (-s_ip * fast_rcp(nd2)) : INFINITY;   // (mode 1: a signed step onto the boundary)
            OSOT_SUB_END(PH_IN_R);
#ifdef OSOT_TRACE_TRIPS   // developer knob: one line per pass of the inner loop (GPU or emulator; run ONE instance)
            if (WaveCtx<NP>::lane_of(c, h) == 0)
                printf("TRIP it %d iq %d me %d ip %d s_ip %.3e nd2 %.3e dd %.3e z_ok %d rmax %.3e t1 %.3e t2 %.3e mode %d\n", iters, iq, me, ip, s_ip, nd2, dd,
                       (int)z_ok, rmax, t1, t2, mode);
#endif
            // A TINY VIOLATION WITH THE NORMAL IN THE SPAN OF THE WORKING SET, AHEAD OF A DUAL EXCHANGE (round 5).  No primal direction,
            // a multiplier to trade: in exact arithmetic the exchange is the dual method's step.  But at the reference's default eps a
            // violation of 1e-9 is what the working set's own round-off implies, and the exchange it triggers goes through a direction
            // that is barely independent -- seen on hardware only (tests/golden/default_eps_roundoff_exchange_instance.npz, closed-loop
            // seed 44): a bound 3.5e-9 outside was traded against a member of the set along |d2|^2 = 8e-7 |d|^2, another bound ended
            // 1.6e-6 outside with nothing left to trade, and the level was called INFEASIBLE where both witnesses solve it.  So:
            //   below kSpanAccept (1e-8 relative: a tenth of the 1e-7 the acceptance rule of DESIGN section 5 asks of a feasible point, far
            //   inside qpOASES' own termination tolerance of 2.2e-7) the constraint counts as satisfied -- its bound is relaxed by the
            //   violation for the rest of the cascade and the accepted slack is reported;
            //   up to kSlackTol the round-off of the ITERATE is taken out first (refine_on_working_set) and the scan runs again; a
            //   violation that survives is exchanged as before.
            if (mode == 0 && !z_ok && t1 < INFINITY) {
                const double bmag0 = ip_box ? fabs(bcast((ip < n) ? lb : ub, ip_var))
                                            : fabs(uniform_d((ip & 1) ? w.rup[ip_row] : w.rlo[ip_row]));
                if (-s_ip <= kSpanAccept * fmax(1.0, bmag0)) {
                    const double relax = -1.001 * s_ip;
                    if (ip_box) { if (c == ip_var) { if (ip < n) lb -= relax; else ub += relax; } }
                    else if (c == 0 && h == 0) { if (ip & 1) w.rup[ip_row] += relax; else w.rlo[ip_row] -= relax; }
                    wave_sync();
                    slack_out = fmax(slack_out, -s_ip);
                    degenerate_done = true; break;
                }
                if (!diag_dd && refine_left > 0 && -s_ip <= kSlackTol * fmax(1.0, bmag0)) {
                    refine_left--;
                    x = refine_on_working_set<NP, BOX, LEAN>(w, x, iq, Aq, lb, ub, xprev, lr);
                    degenerate_done = true; break;
                }
            }
            if (!(t1 < INFINITY) && !(t2 < INFINITY)) {
                // no primal direction left and no inequality to trade.  If the most violated constraint is
                // violated only at round-off level (an active inequality of an upper level re-appearing when the
                // optimality rows leave no freedom: slack = O(eps * cond)), the point is optimal; otherwise the
                // QP is infeasible (eiquadprog.hpp:376-382).
                const double bmag = ip_box ? fabs(bcast((ip < n) ? lb : ub, ip_var))
                                           : fabs(uniform_d((ip & 1) ? w.rup[ip_row] : w.rlo[ip_row]));
                if (-s_ip <= fmin(kSlackTol * fmax(1.0, bmag), kSlackCap)) {
                    if (!diag_dd && refine_left > 0 && -s_ip > kRefineFloor * fmax(1.0, bmag)) {
                        // round-off of the iterate, not of the problem: put x back onto the working set and scan again
                        refine_left--;
                        x = refine_on_working_set<NP, BOX, LEAN>(w, x, iq, Aq, lb, ub, xprev, lr);
                        degenerate_done = true; break;
                    }
                    // accepted as satisfied: the LOWER levels must accept the same point (their optimality rows pin x
                    // to it), so the bound is relaxed by what was accepted for the rest of this instance's cascade --
                    // otherwise they find the constraint violated by that much, trade it against a bound and end
                    // INFEASIBLE (tests/stress_closed_loop.py at the default eps)
                    const double relax = -1.001 * s_ip;
                    if (ip_box) { if (c == ip_var) { if (ip < n) lb -= relax; else ub += relax; } }
                    else if (c == 0 && h == 0) { if (ip & 1) w.rup[ip_row] += relax; else w.rlo[ip_row] -= relax; }
                    wave_sync();
                    slack_out = fmax(slack_out, -s_ip);
                    degenerate_done = true; break;   // this constraint now counts as satisfied; the scan goes on
                }
                failed = true; break;
            }
            if (t2 <= t1) {
                // full step: constraint ip becomes active
                x += t2 * z;
                if (c >= me && c < iq) uq -= t2 * rr;
                u_new += t2;
                householder_add<NP, true>(w, d, d2, z, nd2, iq);
                if (c == iq) { Aq = ip; uq = u_new; }
                if (ip_box) { if (c == ip_var) box_state = (ip < n) ? 1 : 2; }
                else { if (c == 0 && h == 0) w.rowstate[ip_row] = (ip & 1) ? 2 : 1; }
                iq++;
                if (mode == 1) { hot_check = true; hot_since_check++; hot_added++; }
                wave_sync();
                OSOT_SUB_END(PH_IN_HH);
                break;
            }
            // partial step (or pure dual step when z == 0): drop the blocking constraint
            if (z_ok) x += t1 * z;
            if (c >= me && c < iq) uq -= t1 * rr;
            u_new += t1;
            const int cdrop = bcast_i(Aq, lpos);
            if (cdrop < 2 * n) { if (c == (cdrop < n ? cdrop : cdrop - n)) box_state = 0; }
            else { if (c == 0 && h == 0) w.rowstate[(cdrop - 2 * n) >> 1] = 0; }
            drop_constraint<NP>(w, lpos, iq, Aq, uq);
            if (z_ok) {
                if (ip_box) s_ip = bcast((ip < n) ? (x - lb) : (ub - x), ip_var);
                else {
                    const double ax = colsum<NP>(np * x);   // = sgn * a'x
                    s_ip = (ip & 1) ? (w.rup[ip_row] + ax) : (ax - w.rlo[ip_row]);
                    s_ip = bcast(s_ip, 0);
                }
            }
            OSOT_SUB_END(PH_IN_DROP);
            if (++iters > max_iter) { status = QP_MAX_ITER; failed = true; break; }
        }
        if (failed) { if (status == QP_SOLVED) status = QP_INFEASIBLE; break; }
        if (degenerate_done) continue;   // (bounded: every trip of the outer loop counts against max_iter)
    }
    OSOT_PH_END(PH_INEQ);
    if (hot_out) {   // the inequality part of the working set, compacted to the front, for the next solve of this instance
        const bool act = (status == QP_SOLVED) && c >= me && c < iq;
        const int slot = (c >= me) ? c - me : c + NP - me;
        if (h == 0 && c < NP) hot_out[slot] = act ? Aq : -1;
    }
    x_out = x;
    iters_out = iters;
    return status;
}

}  // namespace osot
