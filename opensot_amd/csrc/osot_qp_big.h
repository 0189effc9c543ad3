// opensot_amd/csrc/osot_qp_big.h -- the BackEnd-convention QP (BackEnd.h:125-150: H, g, lA <= A x <= uA, l <= x <= u) for 65 .. 128
// variables: what osot_qp_solve_batch and the osot_backend_* plugin surface run when the problem is wider than the 64 lanes of a
// wavefront (a 45-DoF robot, a 38-DoF floating-base inverse-dynamics stack with five 6-D contacts: include/OpenSoT/Task.h has no limit).
//
// One WORKGROUP of 256 threads per QP instead of one wavefront.  Same method as the wavefront core (osot_qp_core.h): Goldfarb-Idnani
// dual active set (the reference's eiQuadProg back-end, external/eiQuadProg-ext/include/eiquadprog.hpp), H + eps I = L L', J = L^-T
// explicit, every addition ONE Householder reflection of J2 (the new column of R is [d1; alpha]), removals by Givens rotations of R and
// the matching columns of J, bilateral rows and box bounds native, equality rows (lA == uA) eliminated first and never dropped.
// Data: J (n x n) and the Cholesky factor live in a per-workgroup slice of device memory (256 KB at n = 128: L2-resident; every pass
// over them is a parallel loop with coalesced or row-private accesses), the packed triangular R of the working set, the iterate and the
// work vectors in LDS.  The n^2 work of an iteration (d = J'n, z = J2 d2, the reflection / the rotations of J, the row scan) is spread
// over the threads; the iq^2 work on R (back substitution, re-triangularisation after a removal) and the scalar decisions run on thread 0
// out of LDS; a workgroup barrier separates the sections.  This is the coverage path for wide problems, not a tuned kernel: see DESIGN.md.
//
// The body is written against a two-member "team" (thread id, thread count, barrier) so that the SAME source compiles for the host
// with a team of one (tests/emu: the parity tests of this file run it on the CPU against the oracle; a section is then a plain loop).
#pragma once
#include <cmath>
#include <cstddef>
#include "osot_qp_tol.h"   // kInfty, kViolTol, kEqTol, ...: the wavefront core's tolerances, by the same names

#if defined(__HIPCC__) && !defined(OSOT_BIG_HOST)
#define OSOT_BIG_FN __device__ inline
#else
#define OSOT_BIG_FN inline
#endif

namespace osot {
namespace big {

constexpr int kMaxVars = 128;
constexpr int kMaxRows = 2048;
enum { ST_SOLVED = 0, ST_INFEASIBLE = 1, ST_MAX_ITER = 2, ST_NOT_PD = 3 };   // = OSOT_STATUS_*

struct Args {                         // one instance
    int n, nc, max_iter;
    double eps;
    const double *H, *g, *A, *lA, *uA, *l, *u;   // l / u null: no box.  H may be Lw itself (built in place by the caller)
    double* x;
    int* status;
    int* iters;                       // may be null
    double* Lw;                       // workspace [n][n]: H + eps I -> its Cholesky factor (lower triangle)
    double* J;                        // workspace [n][n]: J = L^-T, rotated / reflected as the working set changes
    // cascade switch (osot_cascade_wide.h; the explicit-QP path leaves it off and keeps its statuses): a dependent equality that is
    // inconsistent, or a violated constraint with no direction left and no multiplier to trade, is accepted as round-off of the levels
    // above when the violation is at most min(kSlackTol max(1, |bound|), kSlackCap); the largest one goes to *slack (thread 0)
    // With the switch on, the rest of the wavefront cascade's rule (osot_qp_core.h, gi_inequalities) comes along: an accepted bound or
    // row is RELAXED by 1.001 x the violation for the rest of the instance's cascade (lmut / umut: the box the cascade hands in as l / u;
    // rows: Rows::relax), so that the levels below accept the same point; a violation of at most kSpanAccept with its normal in the span
    // of the working set is accepted ahead of a dual exchange; and up to kRefineMax times per level the round-off of the ITERATE is taken
    // out first (x += J1 y with R'y = the working set's residuals) before a violation up to kSlackTol is accepted.
    bool accept_slack = false;
    double* slack = nullptr;
    double *lmut = nullptr, *umut = nullptr;
    // hot start (solve<true> only; the cold instantiation reads neither): kHotLen codes in global memory each, hot_code() of the
    // inequality working set this problem ended with last time, -1 = none.  Both null: cold.  They may be the same array (the list is
    // read before it is written).  (A cascade would hand in one list per level: the codes are positions in THIS level's rows.)
    const int* hot_in = nullptr;
    int* hot_out = nullptr;
};

// The constraint rows as the solver sees them.  DenseRows: the explicit QP's A [nc][n] with lA <= A x <= uA.  A row source must
// give the clamped bounds, a'x, and either the row's n coefficients or the variable of a unit row e_col (osot_cascade_wide.h: rows
// described by a table, optimality rows taken relative to the previous level's solution).
struct DenseRows {
    const double *A, *lA, *uA;
    int n;
    OSOT_BIG_FN double lo(int r) const;
    OSOT_BIG_FN double up(int r) const;
    OSOT_BIG_FN int unit(int) const { return -1; }
    OSOT_BIG_FN const double* row(int r) const { return A + (size_t)r * n; }
    OSOT_BIG_FN void relax(int, int, double) const {}   // (the explicit QP never accepts a violation)
    OSOT_BIG_FN double dot(int r, const double* x) const {
        const double* ar = A + (size_t)r * n;
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += ar[i] * x[i];
        return acc;
    }
};
enum { SI_IQ = 0, SI_ME, SI_IP, SI_SIDE, SI_ACT, SI_L, SI_ST, SI_ITERS, SI_DONE, SI_REFINE, SI_HOTQ, SI_HOTN, SI_HOTSINCE, SI_HOTADDED, SI_COUNT = 16 };
enum { SD_T = 0, SD_ND2, SD_DD, SD_ALPHA, SD_BETA, SD_SIP, SD_PIV, SD_BND, SD_SLACK, SD_COUNT = 16 };
struct Shared {                       // LDS on the device, heap on the host
    double* R;                        // packed upper triangle of the working set's factor: R(i, j) at j (j + 1) / 2 + i, i <= j
    double *x, *np, *d, *z, *r, *e;   // [n] each: iterate, normal, d = J'n, z = J2 d2, r = R^-1 d1, scratch
    double* u;                        // [n + 1] multipliers by position (+ the candidate's)
    double* cval;                     // [n + nc] violation of each inactive constraint (0: none)
    double *cs_c, *cs_s;              // [n] the rotations of a removal
    double* sc;                       // [SD_COUNT] shared scalars (written by thread 0 between two barriers)
    int *aset, *aside;                // [n] working set by position: constraint code (variable k, or n + row), side (+1 lower, -1 upper)
    int *bstate;                      // [n] 0 free, 1 lower active, 2 upper active
    int *rstate;                      // [nc] 0 inactive, 1 lower active, 2 upper active, 3 equality (in the set for good, or dependent and consistent)
    int* cside;                       // [n + nc]
    int* si;                          // [SI_COUNT]
};
inline size_t shared_doubles(int n, int nc) {
    return (size_t)n * (n + 1) / 2 + 6 * (size_t)n + (n + 1) + (size_t)(n + nc) + 2 * (size_t)n + SD_COUNT;
}
inline size_t shared_ints(int n, int nc) { return 3 * (size_t)n + nc + (size_t)(n + nc) + SI_COUNT; }
inline size_t shared_bytes(int n, int nc) { return 8 * ((shared_doubles(n, nc) + 1) & ~(size_t)1) + 4 * shared_ints(n, nc); }
OSOT_BIG_FN Shared carve(void* base, int n, int nc) {
    Shared s;
    double* p = reinterpret_cast<double*>(base);
    s.R = p; p += (size_t)n * (n + 1) / 2;
    s.x = p; p += n; s.np = p; p += n; s.d = p; p += n; s.z = p; p += n; s.r = p; p += n; s.e = p; p += n;
    s.u = p; p += n + 1;
    s.cval = p; p += n + nc;
    s.cs_c = p; p += n; s.cs_s = p; p += n;
    s.sc = p; p += SD_COUNT;
    if ((p - reinterpret_cast<double*>(base)) & 1) ++p;
    int* q = reinterpret_cast<int*>(p);
    s.aset = q; q += n; s.aside = q; q += n; s.bstate = q; q += n;
    s.rstate = q; q += nc;
    s.cside = q; q += n + nc;
    s.si = q;
    return s;
}

OSOT_BIG_FN double clamp_inf(double v) { return v >= kInfty ? kInfty : (v <= -kInfty ? -kInfty : v); }
OSOT_BIG_FN int ridx(int i, int j) { return ((j * (j + 1)) >> 1) + i; }
OSOT_BIG_FN double DenseRows::lo(int r) const { return clamp_inf(lA[r]); }
OSOT_BIG_FN double DenseRows::up(int r) const { return clamp_inf(uA[r]); }

// ---- hot start: the list of a previous solve's inequality working set (Args::hot_in / hot_out)
constexpr int kHotLen = kMaxVars;         // entries per list
// the stale-list guard and the negative-multiplier threshold of the wavefront route, restated (osot_qp_core.h, gi_inequalities: the
// constants of the same names are local to that function; tests/test_qp_hot_host.py compares the two texts)
constexpr int kHotBatch = 4;              // the multipliers are looked at after every kHotBatch hot additions ...
constexpr int kHotAbandon = 3;            // ... and with at least kHotAbandon negative, and a quarter of the additions so far, the rest of the list is not tried
// (The guard counts negative multipliers only.  An entry that passes the validity checks but whose normal turns out dependent on the
// set costs one compute_d -- an n^2 pass and three barriers -- and is neither an addition nor an iteration: a foreign list of
// dependent normals gets up to kHotLen such trips past the guard and past max_iter.  The list's length is the bound.)
constexpr double kHotDropTol = 1.0e-13;   // a multiplier below -kHotDropTol max|u| is negative (above: round-off of zero)
// one list entry: constraint code (variable k, or n + row) and side (+1 lower, -1 upper); decoded as code = e >> 1, side from e & 1
OSOT_BIG_FN int hot_code(int code, int side) { return 2 * code + ((side < 0) ? 1 : 0); }

#define OSOT_BIG_FOR(i, N) for (int i = tm.tid; i < (N); i += tm.nt)

// Team: { int tid, nt; void sync() const; }  -- every thread of the team calls solve() with the same arguments
// HOT: the instantiation that carries the hot-start code (Args::hot_in / hot_out); the plain one carries none of it
template <bool HOT = false, class Team, class Rows>
OSOT_BIG_FN void solve(const Team& tm, const Args& a, const Shared& s, const Rows& rows) {
    const int n = a.n, nc = a.nc;
    const bool t0 = tm.tid == 0;
    const bool has_box = a.l != nullptr;
    double* L = a.Lw;
    double* J = a.J;
    double* Rp = s.R;
    // ---- H + eps I -> L, state
    OSOT_BIG_FOR(e2, n * n) { const int i = e2 / n, j = e2 - i * n; L[e2] = a.H[e2] + ((i == j) ? a.eps : 0.0); }
    OSOT_BIG_FOR(i, n) { s.bstate[i] = 0; s.x[i] = 0.0; s.u[i] = 0.0; s.aset[i] = -1; s.aside[i] = 0; s.d[i] = -a.g[i]; }
    OSOT_BIG_FOR(r, nc) s.rstate[r] = 0;
    if (t0) { s.si[SI_IQ] = 0; s.si[SI_ME] = 0; s.si[SI_ST] = ST_SOLVED; s.si[SI_ITERS] = 0; s.si[SI_DONE] = 0; s.si[SI_REFINE] = kRefineMax; s.u[n] = 0.0; s.sc[SD_SLACK] = 0.0; }
    tm.sync();
    auto finish = [&]() {              // (called by every thread, behind a barrier)
        const int st = s.si[SI_ST];
        OSOT_BIG_FOR(i, n) a.x[i] = (st == ST_SOLVED) ? s.x[i] : 0.0;
        if (t0) { *a.status = st; if (a.iters) *a.iters = s.si[SI_ITERS]; if (a.slack) *a.slack = fmax(*a.slack, s.sc[SD_SLACK]); }
        if constexpr (HOT) {           // the inequality part of the working set, compacted to the front, for this problem's next solve
            if (a.hot_out) {
                const int me0 = s.si[SI_ME], cnt = (st == ST_SOLVED) ? s.si[SI_IQ] - me0 : 0;
                OSOT_BIG_FOR(q, kHotLen) a.hot_out[q] = (q < cnt) ? hot_code(s.aset[me0 + q], s.aside[me0 + q]) : -1;
            }
        }
        tm.sync();
    };
    // ---- Cholesky of H + eps I, right-looking, in place (lower triangle of L)
    for (int k = 0; k < n; ++k) {
        if (t0) {
            const double p = L[k * n + k];
            if (!(p > 0.0) || !(p < INFINITY)) s.si[SI_ST] = ST_NOT_PD;
            else { const double sq = sqrt(p); L[k * n + k] = sq; s.sc[SD_PIV] = 1.0 / sq; s.d[k] *= 1.0 / sq; }      // (y_k: final)
        }
        tm.sync();
        if (s.si[SI_ST] != ST_SOLVED) { finish(); return; }
        const double ip = s.sc[SD_PIV];
        const int m = n - k - 1;
        const double yk = s.d[k];
        OSOT_BIG_FOR(i2, m) { const int i = k + 1 + i2; const double lik = L[i * n + k] * ip; L[i * n + k] = lik; s.d[i] -= lik * yk; }
        tm.sync();
        OSOT_BIG_FOR(e2, m * m) {
            const int ii = e2 / m, jj = e2 - ii * m;
            if (jj <= ii) { const int i = k + 1 + ii, j = k + 1 + jj; L[i * n + j] -= L[i * n + k] * L[j * n + k]; }
        }
        tm.sync();
    }
    // ---- J = L^-T: thread j computes column j of L^-1 by forward substitution = row j of J
    OSOT_BIG_FOR(j, n) {
        double* row = J + (size_t)j * n;
        for (int i = 0; i < j; ++i) row[i] = 0.0;
        row[j] = 1.0 / L[j * n + j];
        for (int i = j + 1; i < n; ++i) {
            double acc = 0.0;
            for (int k = j; k < i; ++k) acc += L[i * n + k] * row[k];
            row[i] = -acc / L[i * n + i];
        }
    }
    tm.sync();
    // ---- unconstrained minimiser: L y = -g rode along with the factorisation (s.d = y), x = L^-T y = J y.  (Forward SUBSTITUTION, not
    // J'g: on a rank-deficient H + eps I with g in range(H) it keeps the cancellation in the eps-pivots -- the explicit inverse put 1e-6 of
    // null-space noise into x where substitution leaves 5e-8: tests/stress_qp.py "wide", the known-answer structure of TestQPOases.cpp:274-340)
    OSOT_BIG_FOR(i, n) { double acc = 0.0; for (int j = i; j < n; ++j) acc += J[i * n + j] * s.d[j]; s.x[i] = acc; }
    tm.sync();

    // d = J'n for the constraint (code, side), |d|^2 and |d2|^2, z = J2 d2.  Ends behind a barrier.
    auto compute_d = [&](int code, int side) {
        const int iq = s.si[SI_IQ];
        const int ucol = (code < n) ? code : rows.unit(code - n);
        if (ucol >= 0) {
            OSOT_BIG_FOR(j, n) s.d[j] = side * J[ucol * n + j];
        } else {
            const double* ar = rows.row(code - n);
            OSOT_BIG_FOR(i, n) s.np[i] = side * ar[i];
            tm.sync();
            OSOT_BIG_FOR(j, n) { double acc = 0.0; for (int i = 0; i < n; ++i) acc += J[i * n + j] * s.np[i]; s.d[j] = acc; }
        }
        tm.sync();
        if (t0) {
            double dd = 0.0, nd2 = 0.0;
            for (int j = 0; j < n; ++j) { const double v = s.d[j] * s.d[j]; dd += v; if (j >= iq) nd2 += v; }
            s.sc[SD_DD] = dd; s.sc[SD_ND2] = nd2;
        }
        OSOT_BIG_FOR(i, n) { double acc = 0.0; const double* row = J + (size_t)i * n; for (int j = iq; j < n; ++j) acc += row[j] * s.d[j]; s.z[i] = acc; }
        tm.sync();
        // cascade: a normal at 1e-6 of the span of the working set is a direction on paper only -- taking it puts |d2| on the diagonal
        // of R and moves x by violation / |d2|.  Per FREE column c of J: d_c^2 / (|J_c|^2 |n|^2) = cos^2 of its angle with the normal;
        // no usable angle with any of them: dependent (osot_qp_core.h: direction_is_independent)
        if (a.accept_slack && !(s.sc[SD_ND2] > 1.0e-12 * s.sc[SD_DD]) && s.sc[SD_ND2] > kDepTol2 * s.sc[SD_DD]) {
            OSOT_BIG_FOR(c, n) {
                double cos2 = 0.0;
                if (c >= iq) {
                    double cn = 0.0;
                    for (int i = 0; i < n; ++i) { const double v = J[(size_t)i * n + c]; cn += v * v; }
                    cos2 = (cn > 0.0) ? s.d[c] * s.d[c] / cn : 0.0;
                }
                s.e[c] = cos2;
            }
            tm.sync();
            if (t0) {
                double best = 0.0, nn = 1.0;
                for (int c = iq; c < n; ++c) best = fmax(best, s.e[c]);
                if (ucol < 0) { nn = 0.0; for (int i = 0; i < n; ++i) nn += s.np[i] * s.np[i]; }
                if (!(best > kDepFloor2 * nn)) s.sc[SD_ND2] = 0.0;
            }
            tm.sync();
        }
    };
    // the constraint whose d, z are current enters the working set at position iq: one Householder reflection of J2.  Ends behind a barrier.
    auto add_constraint = [&](int code, int side) {
        const int iq = s.si[SI_IQ];
        if (t0) {
            const double nd2 = s.sc[SD_ND2], d0 = s.d[iq];
            const double nrm = sqrt(nd2), alpha = (d0 > 0.0) ? -nrm : nrm;
            s.sc[SD_ALPHA] = alpha; s.sc[SD_BETA] = 1.0 / (nd2 - alpha * d0);
            for (int i = 0; i < iq; ++i) Rp[ridx(i, iq)] = s.d[i];
            Rp[ridx(iq, iq)] = alpha;
            s.aset[iq] = code; s.aside[iq] = side;
            if (code < n) s.bstate[code] = (side > 0) ? 1 : 2;
            else if (s.rstate[code - n] != 3) s.rstate[code - n] = (side > 0) ? 1 : 2;
        }
        tm.sync();
        const double alpha = s.sc[SD_ALPHA], beta = s.sc[SD_BETA];
        const double v0 = s.d[iq] - alpha;
        OSOT_BIG_FOR(i, n) {
            double* row = J + (size_t)i * n;
            const double bw = beta * (s.z[i] - alpha * row[iq]);      // J2 v = J2 d2 - alpha J[:, iq]
            row[iq] -= bw * v0;
            for (int j = iq + 1; j < n; ++j) row[j] -= bw * s.d[j];
        }
        if (t0) s.si[SI_IQ] = iq + 1;
        tm.sync();
    };
    // the constraint at position l leaves the working set: column l out of R, Givens rotations restore the triangle (thread 0, column
    // by column through a scratch vector: the packed storage has no room for the sub-diagonal), the same rotations on the columns of J.
    auto drop_constraint = [&](int l) {
        const int iq = s.si[SI_IQ];
        tm.sync();                                       // (everybody has read iq before thread 0 moves it)
        if (t0) {
            const int code = s.aset[l];
            if (code < n) s.bstate[code] = 0; else s.rstate[code - n] = 0;
            double* e = s.e;
            for (int k = l; k < iq - 1; ++k) {
                for (int i = 0; i <= k + 1; ++i) e[i] = Rp[ridx(i, k + 1)];
                for (int j = l; j < k; ++j) {
                    const double c = s.cs_c[j], sn = s.cs_s[j], a0 = e[j], b0 = e[j + 1];
                    e[j] = c * a0 + sn * b0; e[j + 1] = -sn * a0 + c * b0;
                }
                const double a0 = e[k], b0 = e[k + 1];
                const double h = sqrt(a0 * a0 + b0 * b0);
                double c = 1.0, sn = 0.0;
                if (h > 0.0) { c = a0 / h; sn = b0 / h; }
                s.cs_c[k] = c; s.cs_s[k] = sn;
                e[k] = h;
                for (int i = 0; i <= k; ++i) Rp[ridx(i, k)] = e[i];
                s.aset[k] = s.aset[k + 1]; s.aside[k] = s.aside[k + 1]; s.u[k] = s.u[k + 1];
            }
            s.u[iq - 1] = s.u[iq]; s.u[iq] = 0.0;       // (the candidate's multiplier follows the set)
            s.aset[iq - 1] = -1;
            s.si[SI_IQ] = iq - 1;
        }
        tm.sync();
        OSOT_BIG_FOR(i, n) {
            double* row = J + (size_t)i * n;
            for (int j = l; j < iq - 1; ++j) {
                const double c = s.cs_c[j], sn = s.cs_s[j], a0 = row[j], b0 = row[j + 1];
                row[j] = c * a0 + sn * b0; row[j + 1] = -sn * a0 + c * b0;
            }
        }
        tm.sync();
    };

    // ---- equality rows first (lA == uA after the clamp): a signed step onto each, no multipliers, never dropped
    for (int r = 0; r < nc; ++r) {
        const double lo = rows.lo(r), up = rows.up(r);
        if (!(lo == up)) continue;
        tm.sync();                                       // (the scalars of the previous row have been read by everybody)
        if (t0) { s.sc[SD_SIP] = rows.dot(r, s.x) - lo; s.rstate[r] = 3; }
        compute_d(n + r, +1);
        const double nd2 = s.sc[SD_ND2], dd = s.sc[SD_DD], sip = s.sc[SD_SIP];
        if (!(nd2 > kDepTol2 * dd)) {                    // a combination of the rows already in
            if (fabs(sip) > kEqTol * fmax(1.0, fabs(lo))) {
                if (a.accept_slack && fabs(sip) <= fmin(kSlackTol * fmax(1.0, fabs(lo)), kSlackCap)) {   // round-off of the levels above
                    tm.sync();
                    if (t0) s.sc[SD_SLACK] = fmax(s.sc[SD_SLACK], fabs(sip));
                    continue;
                }
                tm.sync(); if (t0) s.si[SI_ST] = ST_INFEASIBLE; tm.sync(); finish(); return;
            }
            continue;                                    // redundant and consistent
        }
        const double t = -sip / nd2;
        OSOT_BIG_FOR(i, n) s.x[i] += t * s.z[i];
        add_constraint(n + r, +1);
        if (t0) s.si[SI_ITERS] += 1;
    }
    tm.sync();
    if (t0) s.si[SI_ME] = s.si[SI_IQ];
    tm.sync();
    const int me = s.si[SI_ME];

    // ---- HOT START (the method of the wavefront route, osot_qp_core.h gi_inequalities, restated for the team; the reference's
    // qpOASES back-end keeps its working set from one control cycle to the next, QPOasesBackEnd.cpp:258-285).  The constraints of the
    // list are re-added first, each as if it were an equality: a SIGNED full step onto its boundary, the multipliers updated by the
    // same dual direction, no scan and no ratio test.  Then every constraint whose multiplier came out negative is taken out again by
    // the reverse of an addition (x' = x - u_k z, u' = u + u_k r with z, r of its normal against the factors of the set without it):
    // each removal moves to the minimiser over a subset, f strictly decreases, so the phase ends in an S-pair (x minimises f on the
    // working set, all multipliers >= 0) -- a valid state of the dual method, which goes on below as from a cold start.  The minimiser
    // is unique: the answer is the cold one up to round-off, what changes is the number of iterations.  A STALE list must not cost
    // more than it can save: see kHotBatch / kHotAbandon.  Thread 0 walks the list and takes the scalar decisions;
    // d, z, the reflection and the rotations are the team's, as in the dual loop.
    if constexpr (HOT) {
        if (a.hot_in) {
            if (t0) { s.si[SI_HOTQ] = 0; s.si[SI_HOTN] = kHotLen; s.si[SI_HOTSINCE] = 0; s.si[SI_HOTADDED] = 0; }
            // the list comes into LDS in one parallel pass (thread 0 walking it in global memory is a chain of 128 round trips); it
            // borrows the scan's violation array, which nothing reads before the first scan rewrites it.  What does not fit
            // (n + nc < 64) thread 0 reads where it is.
            int* hl = reinterpret_cast<int*>(s.cval);
            const int nst = (2 * (n + nc) < kHotLen) ? 2 * (n + nc) : kHotLen;
            OSOT_BIG_FOR(q, nst) hl[q] = a.hot_in[q];
            // thread 0: largest |u| and the most negative u over the inequality positions; the count of negative ones
            auto look = [&](int& lmin, int& nneg) {
                const int iq = s.si[SI_IQ];
                double umax = 0.0, umin = 0.0;
                for (int k = me; k < iq; ++k) umax = fmax(umax, fabs(s.u[k]));
                lmin = -1; nneg = 0;
                for (int k = me; k < iq; ++k)
                    if (s.u[k] < -kHotDropTol * umax) { ++nneg; if (s.u[k] < umin) { umin = s.u[k]; lmin = k; } }
            };
            for (;;) {                                   // additions
                tm.sync();                               // (the scalars of the previous entry have been read by everybody)
                if (t0) {
                    int q = s.si[SI_HOTQ], hn = s.si[SI_HOTN];
                    int act = 0;
                    while (q < hn) {
                        if (s.si[SI_HOTSINCE] >= kHotBatch) {        // a look in the middle of the list: count, do not remove (a PARTIAL
                            int lmin, nneg;                          // set can show a negative multiplier that the complete one does not)
                            look(lmin, nneg);
                            s.si[SI_HOTSINCE] = 0;
                            if (nneg >= kHotAbandon && 4 * nneg >= s.si[SI_HOTADDED]) { hn = q; break; }
                        }
                        const int enc = (q < nst) ? hl[q] : a.hot_in[q];
                        ++q;
                        if (enc < 0) continue;
                        const int code = enc >> 1, side = (enc & 1) ? -1 : +1;
                        if (code >= n + nc) continue;                // not a constraint of this problem
                        double bnd;
                        if (code < n) {
                            if (!has_box || s.bstate[code] != 0) continue;               // in the working set already
                            bnd = (side > 0) ? clamp_inf(a.l[code]) : clamp_inf(a.u[code]);
                        } else {
                            if (s.rstate[code - n] != 0) continue;                       // in the set already, or an equality row
                            bnd = (side > 0) ? rows.lo(code - n) : rows.up(code - n);
                        }
                        if ((side > 0) ? !(bnd > -kInfty) : !(bnd < kInfty)) continue;   // no bound on that side
                        s.si[SI_IP] = code; s.si[SI_SIDE] = side; s.sc[SD_BND] = bnd;
                        act = 1;
                        break;
                    }
                    s.si[SI_HOTQ] = q; s.si[SI_HOTN] = hn; s.si[SI_ACT] = act;
                }
                tm.sync();
                if (s.si[SI_ACT] == 0) break;
                const int ip = s.si[SI_IP], side = s.si[SI_SIDE];
                compute_d(ip, side);
                if (!(s.sc[SD_ND2] > kDepTol2 * s.sc[SD_DD])) continue;                  // dependent on the set: not taken
                if (t0) {
                    const int iq = s.si[SI_IQ];
                    for (int j = iq - 1; j >= 0; --j) {              // r = R^-1 d1
                        double acc = s.d[j];
                        for (int k = j + 1; k < iq; ++k) acc -= Rp[ridx(j, k)] * s.r[k];
                        s.r[j] = acc / Rp[ridx(j, j)];
                    }
                    const double ax = (ip < n) ? s.x[ip] : rows.dot(ip - n, s.x);
                    const double t = -(side * (ax - s.sc[SD_BND])) / s.sc[SD_ND2];       // onto the boundary, either sign
                    for (int k = 0; k < iq; ++k) s.u[k] -= t * s.r[k];
                    s.u[iq] = t;
                    s.sc[SD_T] = t;
                    s.si[SI_HOTSINCE] += 1; s.si[SI_HOTADDED] += 1;
                    s.si[SI_ACT] = (++s.si[SI_ITERS] > a.max_iter) ? 4 : 1;
                }
                tm.sync();
                if (s.si[SI_ACT] == 4) { if (t0) s.si[SI_ST] = ST_MAX_ITER; tm.sync(); finish(); return; }
                const double t = s.sc[SD_T];
                OSOT_BIG_FOR(i, n) s.x[i] += t * s.z[i];
                add_constraint(ip, side);
            }
            for (;;) {                                   // removals: the most negative multiplier, while there is one
                tm.sync();
                if (t0) {
                    int lmin = -1, nneg = 0;
                    if (s.si[SI_HOTADDED] > 0) look(lmin, nneg);
                    int act = 0;
                    if (lmin >= 0) {
                        s.si[SI_L] = lmin; s.si[SI_IP] = s.aset[lmin]; s.si[SI_SIDE] = s.aside[lmin]; s.sc[SD_T] = s.u[lmin];
                        act = (++s.si[SI_ITERS] > a.max_iter) ? 4 : 2;
                    }
                    s.si[SI_ACT] = act;
                }
                tm.sync();
                if (s.si[SI_ACT] == 0) break;
                if (s.si[SI_ACT] == 4) { if (t0) s.si[SI_ST] = ST_MAX_ITER; tm.sync(); finish(); return; }
                const int l = s.si[SI_L], ip = s.si[SI_IP], side = s.si[SI_SIDE];
                const double uk = s.sc[SD_T];
                drop_constraint(l);
                compute_d(ip, side);                     // (against the factors of the set without it)
                if (t0) {
                    const int iq = s.si[SI_IQ];
                    for (int j = iq - 1; j >= 0; --j) {
                        double acc = s.d[j];
                        for (int k = j + 1; k < iq; ++k) acc -= Rp[ridx(j, k)] * s.r[k];
                        s.r[j] = acc / Rp[ridx(j, j)];
                    }
                    for (int k = 0; k < iq; ++k) s.u[k] += uk * s.r[k];
                    s.u[iq] = 0.0;
                }
                OSOT_BIG_FOR(i, n) s.x[i] -= uk * s.z[i];
            }
        }
    }

    // ---- the dual loop
    for (;;) {
        // most violated inactive constraint
        OSOT_BIG_FOR(k, n) {
            double v = 0.0; int sd = 0;
            if (has_box && s.bstate[k] == 0) {
                const double lo = clamp_inf(a.l[k]), up = clamp_inf(a.u[k]), xk = s.x[k];
                if (lo > -kInfty) { const double vi = lo - xk; if (vi > kViolTol * fmax(1.0, fabs(lo)) && vi > v) { v = vi; sd = +1; } }
                if (up < kInfty) { const double vi = xk - up; if (vi > kViolTol * fmax(1.0, fabs(up)) && vi > v) { v = vi; sd = -1; } }
            }
            s.cval[k] = v; s.cside[k] = sd;
        }
        OSOT_BIG_FOR(r, nc) {
            double v = 0.0; int sd = 0;
            if (s.rstate[r] == 0) {
                const double lo = rows.lo(r), up = rows.up(r);
                if (lo > -kInfty || up < kInfty) {
                    const double ax = rows.dot(r, s.x);
                    if (lo > -kInfty) { const double vi = lo - ax; if (vi > kViolTol * fmax(1.0, fabs(lo)) && vi > v) { v = vi; sd = +1; } }
                    if (up < kInfty) { const double vi = ax - up; if (vi > kViolTol * fmax(1.0, fabs(up)) && vi > v) { v = vi; sd = -1; } }
                }
            }
            s.cval[n + r] = v; s.cside[n + r] = sd;
        }
        tm.sync();
        if (t0) {
            double best = 0.0; int ip = -1;
            for (int k = 0; k < n + nc; ++k) if (s.cval[k] > best) { best = s.cval[k]; ip = k; }
            if (ip < 0) s.si[SI_DONE] = 1;
            else {
                const int sd = s.cside[ip];
                s.si[SI_IP] = ip; s.si[SI_SIDE] = sd; s.sc[SD_SIP] = -best;
                s.sc[SD_BND] = (ip < n) ? ((sd > 0) ? clamp_inf(a.l[ip]) : clamp_inf(a.u[ip])) : ((sd > 0) ? rows.lo(ip - n) : rows.up(ip - n));
                s.u[s.si[SI_IQ]] = 0.0;
            }
        }
        tm.sync();
        if (s.si[SI_DONE]) break;
        const int ip = s.si[SI_IP], side = s.si[SI_SIDE];
        // the step(s) that bring constraint ip in
        for (;;) {
            compute_d(ip, side);
            if (t0) {
                const int iq = s.si[SI_IQ];
                for (int j = iq - 1; j >= 0; --j) {              // r = R^-1 d1
                    double acc = s.d[j];
                    for (int k = j + 1; k < iq; ++k) acc -= Rp[ridx(j, k)] * s.r[k];
                    s.r[j] = acc / Rp[ridx(j, j)];
                }
                double rmax = 0.0;
                for (int k = me; k < iq; ++k) rmax = fmax(rmax, fabs(s.r[k]));
                double t1 = INFINITY; int l = -1;
                for (int k = me; k < iq; ++k)
                    if (s.r[k] > kRatioTol * rmax && s.r[k] > 0.0) { const double q = s.u[k] / s.r[k]; if (q < t1) { t1 = q; l = k; } }
                const double nd2 = s.sc[SD_ND2], dd = s.sc[SD_DD], sip = s.sc[SD_SIP];
                const bool has_dir = nd2 > kDepTol2 * dd;
                const double t2 = has_dir ? -sip / nd2 : INFINITY;
                int act; double t = 0.0;
                const double viol = -sip, bmag = fmax(1.0, fabs(s.sc[SD_BND]));
                const bool refine = a.accept_slack && s.si[SI_REFINE] > 0;
                if (a.accept_slack && !has_dir && t1 < INFINITY && viol <= kSpanAccept * bmag) act = 5;     // round-off ahead of an exchange: accept
                else if (refine && !has_dir && t1 < INFINITY && viol <= kSlackTol * bmag) act = 6;          // ... or refine the iterate first
                else if (!(t1 < INFINITY) && !(t2 < INFINITY)) {                                           // no step at all: infeasible, or
                    act = 0;                                                                                // round-off of the levels above
                    if (a.accept_slack && viol <= fmin(kSlackTol * bmag, kSlackCap)) act = (refine && viol > kRefineFloor * bmag) ? 6 : 5;
                }
                else if (t2 <= t1) { act = 2; t = t2; }                                    // full step: ip enters
                else if (!has_dir) { act = 1; t = t1; }                                    // dual step only: l leaves
                else { act = 3; t = t1; }                                                  // partial step: l leaves
                if (act >= 1 && act <= 3) {
                    for (int k = 0; k < iq; ++k) s.u[k] -= t * s.r[k];
                    s.u[iq] += t;
                }
                if (act == 5) {                                  // accepted: relaxed for the rest of the cascade, reported
                    const double rx = 1.001 * viol;
                    if (ip < n) { if (side > 0) a.lmut[ip] -= rx; else a.umut[ip] += rx; }
                    else rows.relax(ip - n, side, rx);
                    s.sc[SD_SLACK] = fmax(s.sc[SD_SLACK], viol);
                }
                if (act == 6) {                                  // refinement: residuals of the working set, R'y = rho into s.r
                    s.si[SI_REFINE] -= 1;
                    for (int q = 0; q < iq; ++q) {
                        const int code = s.aset[q], sd = s.aside[q];
                        double rq;
                        if (code < n) rq = (sd > 0) ? (clamp_inf(a.l[code]) - s.x[code]) : (s.x[code] - clamp_inf(a.u[code]));
                        else {
                            const int r = code - n;
                            const double ax = rows.dot(r, s.x);
                            rq = (s.rstate[r] == 3 || sd > 0) ? (rows.lo(r) - ax) : (ax - rows.up(r));
                        }
                        double acc = rq;
                        for (int i = 0; i < q; ++i) acc -= Rp[ridx(i, q)] * s.r[i];
                        s.r[q] = acc / Rp[ridx(q, q)];
                    }
                }
                if (++s.si[SI_ITERS] > a.max_iter) act = 4;
                s.si[SI_ACT] = act; s.si[SI_L] = l; s.sc[SD_T] = t;
            }
            tm.sync();
            const int act = s.si[SI_ACT];
            const double t = s.sc[SD_T];
            if (act == 5) break;                                 // (the scan goes on)
            if (act == 6) {                                      // x += J1 y, then scan again
                const int iq = s.si[SI_IQ];
                OSOT_BIG_FOR(i, n) { double dx = 0.0; const double* row = J + (size_t)i * n; for (int j = 0; j < iq; ++j) dx += row[j] * s.r[j]; s.x[i] += dx; }
                tm.sync();
                break;
            }
            if (act == 0 || act == 4) { if (t0) s.si[SI_ST] = (act == 0) ? ST_INFEASIBLE : ST_MAX_ITER; tm.sync(); finish(); return; }
            if (act >= 2) { OSOT_BIG_FOR(i, n) s.x[i] += t * s.z[i]; }
            tm.sync();
            if (act == 2) { add_constraint(ip, side); break; }
            drop_constraint(s.si[SI_L]);
            if (act == 3) {                                      // the candidate's slack at the new x
                if (t0) {
                    double ax;
                    if (ip < n) ax = s.x[ip];
                    else ax = rows.dot(ip - n, s.x);
                    s.sc[SD_SIP] = side * (ax - s.sc[SD_BND]);
                }
                tm.sync();
            }
        }
    }
    finish();
}
// the explicit QP: dense rows A [nc][n]
template <bool HOT = false, class Team>
OSOT_BIG_FN void solve(const Team& tm, const Args& a, const Shared& s) { solve<HOT>(tm, a, s, DenseRows{a.A, a.lA, a.uA, a.n}); }

}  // namespace big

#if defined(__HIPCC__) && !defined(OSOT_BIG_HOST) && !defined(OSOT_EMULATION)
// ---- the device side: one 256-thread workgroup per QP; a launch of G workgroups walks the batch with stride G, each workgroup on its
// own slice of the workspace (2 n^2 doubles)
struct DevQPBig {
    int B, n, nc, max_iter;
    double eps_abs;
    const double *H, *g, *A, *lA, *uA, *l, *u;
    double* x;
    int* status;
    int* iterations;
    double* work;                     // [gridDim.x][2][n][n]
};
struct BigTeamDev {
    int tid, nt;
    __device__ void sync() const { __syncthreads(); }
};
__global__ void __launch_bounds__(256) osot_qp_big_kernel(const DevQPBig Q) {
    extern __shared__ __attribute__((aligned(16))) char osot_big_smem[];
    const int n = Q.n, nc = Q.nc;
    const big::Shared sh = big::carve(osot_big_smem, n, nc);
    const BigTeamDev tm{(int)threadIdx.x, (int)blockDim.x};
    double* slot = Q.work + (size_t)blockIdx.x * 2 * (size_t)n * n;
    for (long long inst = blockIdx.x; inst < Q.B; inst += gridDim.x) {
        big::Args a;
        a.n = n; a.nc = nc; a.max_iter = Q.max_iter; a.eps = Q.eps_abs;
        a.H = Q.H + inst * (long long)n * n; a.g = Q.g + inst * n;
        a.A = nc ? Q.A + inst * (long long)nc * n : nullptr;
        a.lA = nc ? Q.lA + inst * nc : nullptr; a.uA = nc ? Q.uA + inst * nc : nullptr;
        a.l = Q.l ? Q.l + inst * n : nullptr; a.u = Q.u ? Q.u + inst * n : nullptr;
        a.x = Q.x + inst * n; a.status = Q.status + inst; a.iters = Q.iterations ? Q.iterations + inst : nullptr;
        a.Lw = slot; a.J = slot + (size_t)n * n;
        big::solve(tm, a, sh);
        __syncthreads();
    }
}
// the same walk with the working sets carried from call to call (osot_qp_solve_batch_hot): row inst of hot belongs to instance inst of
// the batch, whichever workgroup solves it; read before the solve, rewritten after it.  (A copy of the walk above, on purpose: with
// both kernels calling one function template over HOT the cold kernel came out 20 bytes longer and with other SGPR spills than its
// parent's -- profiles/qp_hot_codegen.txt -- and the cold kernel's code is not to move for a feature it does not run.)
struct DevQPBigHot {
    DevQPBig q;
    int* hot;                         // [B][big::kHotLen]
};
__global__ void __launch_bounds__(256) osot_qp_big_hot_kernel(const DevQPBigHot QH) {
    extern __shared__ __attribute__((aligned(16))) char osot_big_smem[];
    const DevQPBig& Q = QH.q;
    const int n = Q.n, nc = Q.nc;
    const big::Shared sh = big::carve(osot_big_smem, n, nc);
    const BigTeamDev tm{(int)threadIdx.x, (int)blockDim.x};
    double* slot = Q.work + (size_t)blockIdx.x * 2 * (size_t)n * n;
    for (long long inst = blockIdx.x; inst < Q.B; inst += gridDim.x) {
        big::Args a;
        a.n = n; a.nc = nc; a.max_iter = Q.max_iter; a.eps = Q.eps_abs;
        a.H = Q.H + inst * (long long)n * n; a.g = Q.g + inst * n;
        a.A = nc ? Q.A + inst * (long long)nc * n : nullptr;
        a.lA = nc ? Q.lA + inst * nc : nullptr; a.uA = nc ? Q.uA + inst * nc : nullptr;
        a.l = Q.l ? Q.l + inst * n : nullptr; a.u = Q.u ? Q.u + inst * n : nullptr;
        a.x = Q.x + inst * n; a.status = Q.status + inst; a.iters = Q.iterations ? Q.iterations + inst : nullptr;
        a.Lw = slot; a.J = slot + (size_t)n * n;
        a.hot_in = QH.hot + inst * big::kHotLen; a.hot_out = QH.hot + inst * big::kHotLen;
        big::solve<true>(tm, a, sh);
        __syncthreads();
    }
}
#endif
}  // namespace osot
