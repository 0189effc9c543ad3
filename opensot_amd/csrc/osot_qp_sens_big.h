// opensot_amd/csrc/osot_qp_sens_big.h -- multipliers, active set and the backward pass of the batched explicit QP for 65 .. 128
// variables: the contract of osot_qp_sensitivity_batch (include/osot_mi355x.h, osot_qp_sens.h) word for word -- the candidates, their
// capacity 2n and order, least-squares multipliers by a column-pivoted Householder QR of Y = L^-1 C', rank_tol and dual_tol, one
// redo, y = -lambda, active, the seven gradients, SKIPPED / DEGENERATE, nothing non-finite written -- where the problem is wider
// than the 64 lanes of a wavefront.  Reached through osot_qp_sensitivity_batch_ws, which takes the caller's workspace.
//
//   sens_ws_check ............. the argument checks of osot_qp_sensitivity_batch_ws, HIP-free: the host build runs them too
//   sensbig::run .............. one instance, written against a team { tid, nt, sync() } as osot_qp_big.h is: the SAME source is
//                               a 256-thread workgroup on the device and a team of one (or a turn-taking team) on the host
//   osot_qp_sens_big_kernel ... G = min(B, slots) workgroups walk the batch with stride G, each on its own slice of the workspace
//
// WHERE THE DATA LIVES.  L (n x (n | 1) doubles, 132 096 bytes at n = 128) and every vector and list are in LDS; Y, (2n + 2) columns
// of n, is in the workgroup's slice of the workspace, ROW-major (entry i of column c at i (2n + 2) + c): a thread walks its own
// column and the threads of a wavefront touch neighbouring addresses.  At n = 128 the two cannot share the 160 KB of a CU
// (132 KB + 258 KB).
//
// THE REPRODUCIBILITY RULE.  Every scalar -- a row's a_r'x, an entry of L, of Y, a column norm, a reflector's dot product, an entry
// of a triangular solve -- is ONE fma chain in one fixed order computed by one thread (or by every thread alike from the same
// operands); there is no cross-thread reduction tree and no atomic.  Work is spread by ownership: thread = variable, row or column
// (columns c = tid, tid + nt).  Decisions (the pivot, the rank test, who is weakly active) are made by thread 0 and published
// through LDS between two barriers.  Hence the results do not depend on the size of the team, which is how the host build finds a
// missing barrier: a team of several threads taking turns in two opposite orders must give the bits of the team of one.
//
// Every section that reads what another thread wrote is fenced by sync(), and every thread of the team reaches every barrier:
// what an instance does depends only on flags read from LDS after a barrier (a SKIPPED instance takes no early return).
// Each output entry is written once, by its owner: a map from constraint index to set member, built in LDS, makes the zero and
// the value the same store.
#pragma once
#include <cstddef>
#include <cstdint>
#include "osot_qp_sens.h"   // SensArgs, sens_side, sens_present, sens_finite, sens_options, sens_check; acc_pivot_rel

namespace osot {
namespace sensbig {

constexpr int kMinVars = OSOT_MAX_VARS + 1;       // below: osot_qp_sens_kernel
constexpr int kMaxVars = OSOT_MAX_QP_VARS;        // 128
constexpr int kMaxRows = 2048;
constexpr int kThreads = 256;
constexpr int kLdsLimit = 160 * 1024;             // of a CU
constexpr int kComputeUnits = 256;                // of the MI355X: the slot count is a host-side constant (no device is asked)

enum { SI_SKIP = 0, SI_BAD, SI_K, SI_OVER, SI_P, SI_STOP, SI_DEP, SI_WEAK, SI_COUNT = 8 };
enum { SD_S = 0, SD_FIRST, SD_COUNT = 2 };

// the workgroup's LDS: offsets in doubles, then the int part (offsets in ints from its start)
struct Layout { int ldl, ldc, cap, L, xs, hv, zv, dxs, rd, hb, h0, dg, lam, dlam, nrm, sc, ints, cidx, cside, cstate, piv, map, si, bytes; };
__host__ __device__ inline Layout layout(int n, int nc) {
    Layout a;
    a.ldl = n | 1; a.cap = 2 * n; a.ldc = a.cap + 2;
    a.L = 0;
    a.xs = a.L + n * a.ldl;
    a.hv = a.xs + n; a.zv = a.hv + n; a.dxs = a.zv + n; a.rd = a.dxs + n; a.hb = a.rd + n; a.h0 = a.hb + n; a.dg = a.h0 + n;
    a.lam = a.dg + n; a.dlam = a.lam + n;
    a.nrm = a.dlam + n;                            // 2n
    a.sc = a.nrm + a.cap;
    a.ints = a.sc + SD_COUNT;
    a.cidx = 0; a.cside = a.cap; a.cstate = 2 * a.cap;
    a.piv = 3 * a.cap;                             // n
    a.map = a.piv + n;                             // n + nc: the sides of every bound and row, later constraint -> set member
    a.si = a.map + n + nc;
    a.bytes = a.ints * (int)sizeof(double) + (a.si + SI_COUNT) * (int)sizeof(int);
    return a;
}
inline size_t lds_bytes(int n, int nc) { return (size_t)layout(n, nc).bytes; }
// the slice of the workspace one workgroup works on: Y, n rows of 2n + 2 (a multiple of 16 bytes)
inline size_t slice_bytes(int n) { return (size_t)n * (2 * (size_t)n + 2) * sizeof(double); }
// workgroups in flight: what the LDS lets a CU hold (at most 4: 16 wavefronts), on every CU
inline int slots(int n, int nc) {
    int per_cu = (int)((size_t)kLdsLimit / lds_bytes(n, nc));
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    return kComputeUnits * per_cu;
}
inline size_t workspace_bytes(int B, int n, int nc) {
    if (n < kMinVars || B <= 0) return 0;
    const int s = slots(n, nc);
    return (size_t)(B < s ? B : s) * slice_bytes(n);
}

// The column a thread works on in its pass t (slot = tid + nt t).  With more columns than threads (258 at n = 128) the two
// right-hand sides, columns 2n and 2n + 1, take the slots of the last two threads in the FIRST pass: they do not queue behind a
// candidate column of their thread (sens_col does the same at 64 lanes).  Which thread works on a column does not change its bits.
__host__ __device__ inline int col_of(int slot, int cap, int ncol, int nt) {
    if (ncol <= nt || nt < 2) return slot;
    return slot == nt - 1 ? cap : (slot == nt - 2 ? cap + 1 : (slot < nt - 2 ? slot : slot - 2));
}

// an inequality of the set whose multiplier is within `small` of zero or has the wrong sign
__host__ __device__ inline bool weak_member(int side, double v, double small) {
    return side != 2 && (fabs(v) <= small || (side == -1 ? v > 0.0 : v < 0.0));
}

#if defined(__HIPCC__) && !defined(OSOT_EMULATION)
#define OSOT_SENSBIG_FN __device__ inline
#else
#define OSOT_SENSBIG_FN inline
#endif
#define OSOT_SENSBIG_FOR(i, N) for (int i = tm.tid; i < (N); i += tm.nt)

// Team: { int tid, nt; void sync() const; } -- every thread of the team calls run() with the same arguments.
// P.b is the batch, inst the instance, lds the workgroup's LDS (lds_bytes(n, nc)), Y its slice of the workspace (slice_bytes(n)).
template <class Team>
OSOT_SENSBIG_FN void run(const Team& tm, const SensArgs& P, long long inst, char* lds, double* Y) {
    const osot_qp_sens_batch& b = P.b;
    const int n = b.n, nc = b.nc;
    const bool back = b.grad_x != nullptr;
    const Layout Ly = layout(n, nc);
    const int ldl = Ly.ldl, ldc = Ly.ldc, cap = Ly.cap, ncol = cap + 2;
    double* S = reinterpret_cast<double*>(lds);
    double *Ls = S + Ly.L, *xs = S + Ly.xs, *hv = S + Ly.hv, *zv = S + Ly.zv, *dxs = S + Ly.dxs, *rd = S + Ly.rd, *hb = S + Ly.hb, *h0 = S + Ly.h0,
           *Dg = S + Ly.dg, *lam = S + Ly.lam, *dlam = S + Ly.dlam, *nrm = S + Ly.nrm, *sc = S + Ly.sc;
    int* I = reinterpret_cast<int*>(S + Ly.ints);
    int *cidx = I + Ly.cidx, *cside = I + Ly.cside, *cstate = I + Ly.cstate, *piv = I + Ly.piv, *map = I + Ly.map, *si = I + Ly.si;
    double* tcol = Y + cap;                  // column 2n: -(L'x + L^-1 g), then Q't        (entry i at tcol[i ldc])
    double* wcol = Y + cap + 1;              // column 2n + 1: L^-1 grad_x, then Q'w
    const double* Hg = b.H + inst * n * n;
    const double* Ag = nc > 0 ? b.A + inst * nc * n : nullptr;
    const long long m = n + nc;

    // ---- 0. an instance that was not solved, or whose x is not finite, is skipped
    if (tm.tid == 0) {
        for (int q = 0; q < SI_COUNT; ++q) si[q] = 0;
        si[SI_SKIP] = (b.status != nullptr && b.status[inst] != OSOT_STATUS_SOLVED) ? 1 : 0;
    }
    tm.sync();
    OSOT_SENSBIG_FOR(i, n) {
        const double v = b.x[inst * n + i];
        xs[i] = v;
        if (!sens_finite(v)) si[SI_SKIP] = 1;
    }
    tm.sync();
    bool bad = si[SI_SKIP] != 0;
    bool degenerate = false;
    int r = 0;

    if (!bad) {
        // ---- 1. the lower triangle of H + eps I
        OSOT_SENSBIG_FOR(e, n * n) {
            const int row = e / n, c = e - row * n;
            if (c <= row) Ls[row * ldl + c] = Hg[e] + (c == row ? b.eps_abs : 0.0);
        }
        // ---- 2. the candidates: thread = variable, thread = row (a_r'x is one chain over the row)
        OSOT_SENSBIG_FOR(i, n) map[i] = b.l ? sens_side(xs[i], b.l[inst * n + i], b.u[inst * n + i], P.active_tol) : 0;
        OSOT_SENSBIG_FOR(row, nc) {
            const double* ar = Ag + (long long)row * n;
            double ax = 0.0;
            for (int q = 0; q < n; ++q) ax = fma(ar[q], xs[q], ax);
            int rs = sens_side(ax, b.lA[inst * nc + row], b.uA[inst * nc + row], P.active_tol);
            if (!sens_finite(ax)) rs = 0;
            map[n + row] = rs;
        }
        tm.sync();
        // the list, in the order equalities (bounds, rows), bounds, rows, cut at 2n
        if (tm.tid == 0) {
            int cnt[4] = {0, 0, 0, 0};
            for (int e = 0; e < n + nc; ++e) {
                const int s = map[e];
                if (s != 0) ++cnt[(s == 2 ? 0 : 2) + (e < n ? 0 : 1)];
            }
            int at[4] = {0, cnt[0], cnt[0] + cnt[1], cnt[0] + cnt[1] + cnt[2]};
            for (int e = 0; e < n + nc; ++e) {
                const int s = map[e];
                if (s == 0) continue;
                const int p = at[(s == 2 ? 0 : 2) + (e < n ? 0 : 1)]++;
                if (p < cap) { cidx[p] = e; cside[p] = s; }
            }
            const int total = cnt[0] + cnt[1] + cnt[2] + cnt[3];
            si[SI_K] = total < cap ? total : cap;
            si[SI_OVER] = total > cap ? 1 : 0;
            for (int c = 0; c < cap; ++c) cstate[c] = 0;
        }
        tm.sync();
    }
    const int k = bad ? 0 : si[SI_K];
    if (!bad) degenerate = si[SI_OVER] != 0;

    // ---- 3. H~ = L L': thread = row, column by column; the diagonal of L goes to Dg (every thread forms the pivot alike)
    if (!bad) {
        double dmax = Ls[0];
        for (int i = 1; i < n; ++i) { const double v = Ls[i * ldl + i]; dmax = (v > dmax || v != v) ? v : dmax; }
        const double thr = acc_pivot_rel(n) * dmax;
        for (int j = 0; j < n; ++j) {
            double d = Ls[j * ldl + j];
            for (int q = 0; q < j; ++q) { const double v = Ls[j * ldl + q]; d = fma(-v, v, d); }
            if (!(d > thr) || !(d <= 1.7976931348623157e308)) { bad = true; break; }
            const double ljj = sqrt(d);
            if (tm.tid == 0) Dg[j] = ljj;
            for (int i = j + 1 + tm.tid; i < n; i += tm.nt) {
                double s = Ls[i * ldl + j];
                for (int q = 0; q < j; ++q) s = fma(-Ls[i * ldl + q], Ls[j * ldl + q], s);
                Ls[i * ldl + j] = s / ljj;
            }
            tm.sync();
        }
    }
    tm.sync();

    for (int pass = 0; pass < 2 && !bad; ++pass) {
        // ---- 4. the columns of Y = L^-1 C' of the candidates still in the set, and the two right-hand sides
        OSOT_SENSBIG_FOR(e, k * n) {
            const int c = e / n, i = e - c * n;
            if (cstate[c] != 0) continue;
            const int idx = cidx[c];
            Y[(size_t)i * ldc + c] = idx < n ? (i == idx ? 1.0 : 0.0) : Ag[(long long)(idx - n) * n + i];
        }
        OSOT_SENSBIG_FOR(i, n) {
            tcol[(size_t)i * ldc] = b.g[inst * n + i];
            wcol[(size_t)i * ldc] = back ? b.grad_x[inst * n + i] : 0.0;
        }
        tm.sync();
        for (int slot = tm.tid; slot < ncol; slot += tm.nt) {
            const int c = col_of(slot, cap, ncol, tm.nt);
            if (c < cap && (c >= k || cstate[c] != 0)) continue;
            double* y = Y + c;
            const int q0 = (c < cap && cidx[c] < n) ? cidx[c] : 0;      // a unit vector: zeros above its one stay zeros
            for (int q = q0; q < n; ++q) {
                double v = y[(size_t)q * ldc];
                for (int j = q0; j < q; ++j) v = fma(-Ls[q * ldl + j], y[(size_t)j * ldc], v);
                y[(size_t)q * ldc] = v / Dg[q];
            }
        }
        tm.sync();
        // t = -(L'x + L^-1 g): thread = entry
        OSOT_SENSBIG_FOR(i, n) {
            double s = fma(Dg[i], xs[i], tcol[(size_t)i * ldc]);
            for (int q = i + 1; q < n; ++q) s = fma(Ls[q * ldl + i], xs[q], s);
            tcol[(size_t)i * ldc] = -s;
        }
        tm.sync();

        // ---- 5. Householder QR with column pivoting over every column at once
        r = 0;
        for (int j = 0; j < n; ++j) {
            OSOT_SENSBIG_FOR(c, k) {
                if (cstate[c] != 0) continue;
                double s = 0.0;
                for (int i = j; i < n; ++i) { const double v = Y[(size_t)i * ldc + c]; s = fma(v, v, s); }
                nrm[c] = s;
            }
            tm.sync();
            // the first largest remaining norm in ascending column order; thread 0 decides and publishes
            if (tm.tid == 0) {
                int p = -1;
                double best = -1.0;
                for (int c = 0; c < k; ++c) if (cstate[c] == 0 && nrm[c] > best) { best = nrm[c]; p = c; }
                bool stop = p < 0;
                if (!stop) {
                    const double norm = sqrt(best);
                    if (j == 0) sc[SD_FIRST] = norm;                    // the first pivot
                    stop = !(norm > 0.0) || !sens_finite(norm) || norm < P.rank_tol * sc[SD_FIRST];
                    if (!stop) {
                        const double x0 = Y[(size_t)j * ldc + p];
                        const double alpha = x0 >= 0.0 ? -norm : norm;
                        rd[j] = alpha; hb[j] = 1.0 / fma(norm, fabs(x0), best); h0[j] = x0 - alpha;     // hb: 2 / v'v
                        piv[j] = p; cstate[p] = 1;
                    }
                }
                si[SI_P] = p; si[SI_STOP] = stop ? 1 : 0;
            }
            tm.sync();
            if (si[SI_STOP] != 0) break;
            const int p = si[SI_P];
            for (int i = j + tm.tid; i < n; i += tm.nt) hv[i] = i == j ? h0[j] : Y[(size_t)i * ldc + p];
            tm.sync();
            const double beta = hb[j];
            for (int slot = tm.tid; slot < ncol; slot += tm.nt) {
                const int c = col_of(slot, cap, ncol, tm.nt);
                if (c < cap && (c >= k || cstate[c] != 0)) continue;
                double* y = Y + c;
                double s = 0.0;
                for (int i = j; i < n; ++i) s = fma(hv[i], y[(size_t)i * ldc], s);
                s *= beta;
                for (int i = j; i < n; ++i) y[(size_t)i * ldc] = fma(-s, hv[i], y[(size_t)i * ldc]);
            }
            tm.sync();
            r = j + 1;
        }
        // what is left in the set is dependent on the pivots
        if (tm.tid == 0) {
            int dependent = 0;
            for (int c = 0; c < k; ++c) if (cstate[c] == 0) { dependent = 1; cstate[c] = 2; }
            si[SI_DEP] = dependent;
        }

        // ---- 6. R lambda = Q1't and R dlambda = -Q1'w, column-wise: thread = row of R (the running right-hand sides in hv, zv)
        OSOT_SENSBIG_FOR(i, r) { hv[i] = tcol[(size_t)i * ldc]; zv[i] = -wcol[(size_t)i * ldc]; }
        for (int j = r - 1; j >= 0; --j) {
            if (tm.tid == j % tm.nt) { lam[j] = hv[j] / rd[j]; dlam[j] = zv[j] / rd[j]; }
            tm.sync();
            OSOT_SENSBIG_FOR(i, j) {
                const double rij = Y[(size_t)i * ldc + piv[j]];
                hv[i] = fma(-rij, lam[j], hv[i]);
                zv[i] = fma(-rij, dlam[j], zv[i]);
            }
        }
        tm.sync();

        // ---- 7. weakly active or wrong-signed inequalities leave the set, once
        if (tm.tid == 0) {
            double linf = 0.0;
            for (int j = 0; j < r; ++j) { const double a = fabs(lam[j]); linf = (a > linf || a != a) ? a : linf; }
            const double small = P.dual_tol * fmax(1.0, linf);
            int any_weak = 0;
            for (int j = 0; j < r; ++j) any_weak |= weak_member(cside[piv[j]], lam[j], small) ? 1 : 0;
            if (pass == 0 && any_weak) {
                for (int c = 0; c < k; ++c) if (cstate[c] != 3) cstate[c] = 0;
                for (int j = 0; j < r; ++j) if (weak_member(cside[piv[j]], lam[j], small)) cstate[piv[j]] = 3;
            }
            si[SI_WEAK] = any_weak;
        }
        tm.sync();
        const bool any_weak = si[SI_WEAK] != 0;
        degenerate = degenerate || si[SI_DEP] != 0 || any_weak;
        if (pass == 0 && any_weak) continue;
        break;
    }

    // ---- 8. the backward pass: z = Q [0; (Q'w)_(r..)] from the reflectors, dx = -L^-T z
    if (!bad && back) {
        OSOT_SENSBIG_FOR(i, n) zv[i] = i < r ? 0.0 : wcol[(size_t)i * ldc];
        tm.sync();
        for (int j = r - 1; j >= 0; --j) {
            const double* v = Y + piv[j];
            if (tm.tid == 0) {
                double s = h0[j] * zv[j];
                for (int i = j + 1; i < n; ++i) s = fma(v[(size_t)i * ldc], zv[i], s);
                sc[SD_S] = s * hb[j];
            }
            tm.sync();
            const double s = sc[SD_S];
            for (int i = j + tm.tid; i < n; i += tm.nt) zv[i] = fma(-s, i == j ? h0[j] : v[(size_t)i * ldc], zv[i]);
            tm.sync();
        }
        for (int q = n - 1; q >= 0; --q) {
            if (tm.tid == q % tm.nt) dxs[q] = -(zv[q] / Dg[q]);
            tm.sync();
            OSOT_SENSBIG_FOR(i, q) zv[i] = fma(Ls[q * ldl + i], dxs[q], zv[i]);
        }
        tm.sync();
    }
    // ---- 9. nothing non-finite leaves
    if (!bad) {
        OSOT_SENSBIG_FOR(j, r) if (!sens_finite(lam[j]) || (back && !sens_finite(dlam[j]))) si[SI_BAD] = 1;
        if (back) OSOT_SENSBIG_FOR(i, n) if (!sens_finite(dxs[i])) si[SI_BAD] = 1;
    }
    OSOT_SENSBIG_FOR(e, n + nc) map[e] = -1;
    tm.sync();
    bad = bad || si[SI_BAD] != 0;
    // ---- 10. the outputs, each entry once by its owner: constraint -> member of the set, then whole rows
    if (!bad) OSOT_SENSBIG_FOR(j, r) map[cidx[piv[j]]] = j;
    tm.sync();
    OSOT_SENSBIG_FOR(e, n + nc) {
        const int j = map[e];
        if (b.y) b.y[inst * m + e] = j >= 0 ? -lam[j] : 0.0;
        if (b.active) b.active[inst * m + e] = j >= 0 ? cside[piv[j]] : 0;
    }
    OSOT_SENSBIG_FOR(i, n) {
        const int j = map[i];
        const bool upper = j >= 0 && cside[piv[j]] == 1;
        if (b.grad_g) b.grad_g[inst * n + i] = bad ? 0.0 : dxs[i];
        if (b.grad_l) b.grad_l[inst * n + i] = (j >= 0 && !upper) ? -dlam[j] : 0.0;
        if (b.grad_u) b.grad_u[inst * n + i] = upper ? -dlam[j] : 0.0;
    }
    OSOT_SENSBIG_FOR(row, nc) {
        const int j = map[n + row];
        const bool upper = j >= 0 && cside[piv[j]] == 1;
        if (b.grad_lA) b.grad_lA[inst * nc + row] = (j >= 0 && !upper) ? -dlam[j] : 0.0;
        if (b.grad_uA) b.grad_uA[inst * nc + row] = upper ? -dlam[j] : 0.0;
    }
    if (b.grad_A) {
        double* G = b.grad_A + inst * nc * n;
        OSOT_SENSBIG_FOR(e, nc * n) {
            const int row = e / n, i = e - row * n;
            const int j = map[n + row];
            G[e] = j >= 0 ? fma(dlam[j], xs[i], lam[j] * dxs[i]) : 0.0;
        }
    }
    if (b.grad_H) {
        double* G = b.grad_H + inst * n * n;
        OSOT_SENSBIG_FOR(e, n * n) {       // (the pair in one order for both triangles: symmetric to the bit)
            const int row = e / n, c = e - row * n;
            const int lo = row < c ? row : c, hi = row < c ? c : row;
            G[e] = bad ? 0.0 : 0.5 * fma(dxs[lo], xs[hi], xs[lo] * dxs[hi]);
        }
    }
    if (tm.tid == 0) b.flag[inst] = bad ? OSOT_SENS_SKIPPED : (degenerate ? OSOT_SENS_DEGENERATE : OSOT_SENS_OK);
    tm.sync();                              // (the next instance of this workgroup reuses the LDS and the slice)
}

}  // namespace sensbig

// the size of the workspace of osot_qp_sensitivity_batch_ws (include/osot_mi355x.h: osot_qp_sens_workspace_bytes); *why names the field
inline int sens_ws_bytes_check(int B, int n, int nc, const size_t* bytes, const char** why) {
    if (!bytes) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (B < 0) { *why = "B is negative"; return OSOT_ERR_INVALID; }
    if (n < 1) { *why = "n is below 1"; return OSOT_ERR_INVALID; }
    if (n > sensbig::kMaxVars) { *why = "n is above 128"; return OSOT_ERR_UNSUPPORTED; }
    if (nc < 0) { *why = "nc is negative"; return OSOT_ERR_INVALID; }
    if (n > OSOT_MAX_VARS && nc > sensbig::kMaxRows) { *why = "nc is above 2048 with n above 64"; return OSOT_ERR_UNSUPPORTED; }
    return OSOT_OK;
}

// the checks of osot_qp_sensitivity_batch_ws: sens_check's, with n up to 128 and the workspace's
inline int sens_ws_check(const osot_qp_sens_batch* b, const osot_qp_sens_options* o, const void* workspace, size_t workspace_bytes, const char** why) {
    if (!b || b->n <= OSOT_MAX_VARS) return sens_check(b, o, why);      // n <= 64: the same call; the workspace is not looked at
    if (b->B >= 0 && b->n > sensbig::kMaxVars) { *why = "n is above 128 (one workgroup per instance takes 65 .. 128 variables)"; return OSOT_ERR_UNSUPPORTED; }
    osot_qp_sens_batch c = *b;
    c.n = OSOT_MAX_VARS;                                                // (no other check of sens_check depends on n)
    const int rc = sens_check(&c, o, why);
    if (rc != OSOT_OK) return rc;
    if (b->nc > sensbig::kMaxRows) { *why = "nc is above 2048 with n above 64"; return OSOT_ERR_UNSUPPORTED; }
    if (b->B == 0) return OSOT_OK;
    if (!workspace) { *why = "the workspace is null (n above 64 needs osot_qp_sens_workspace_bytes of device memory)"; return OSOT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) { *why = "the workspace is not 16-byte aligned"; return OSOT_ERR_INVALID; }
    if (workspace_bytes < sensbig::workspace_bytes(b->B, b->n, b->nc)) { *why = "the workspace is too small (osot_qp_sens_workspace_bytes gives the size)"; return OSOT_ERR_INVALID; }
    const void* all[20] = {b->H, b->g, b->A, b->lA, b->uA, b->l, b->u, b->x, b->status, b->grad_x,
                           b->y, b->active, b->grad_H, b->grad_g, b->grad_A, b->grad_lA, b->grad_uA, b->grad_l, b->grad_u, b->flag};
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(workspace);
    for (const void* q : all) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(q);
        if (q && a >= w0 && a - w0 < workspace_bytes) { *why = "an input or output lies inside the workspace"; return OSOT_ERR_INVALID; }
    }
    return OSOT_OK;
}

#if defined(__HIPCC__) && !defined(OSOT_EMULATION)
// ---- the device side: one 256-thread workgroup per instance; a launch of G = min(B, slots) workgroups walks the batch with stride G
struct SensBigArgs {
    SensArgs s;
    double* work;                          // [gridDim.x][n][2n + 2]
};
struct SensBigTeamDev {
    int tid, nt;
    __device__ void sync() const { __syncthreads(); }
};
__global__ void __launch_bounds__(256) osot_qp_sens_big_kernel(const SensBigArgs A_) {
    OSOT_DYNAMIC_LDS(sens_big_smem);       // sensbig::lds_bytes(n, nc)
    const SensBigTeamDev tm{(int)threadIdx.x, (int)blockDim.x};
    const SensBigArgs* P = OSOT_KERNARG_PTR(SensBigArgs, A_);
    const int n = P->s.b.n;
    double* slice = P->work + (size_t)blockIdx.x * (size_t)n * (2 * (size_t)n + 2);
    for (long long inst = blockIdx.x; inst < P->s.b.B; inst += gridDim.x) sensbig::run(tm, P->s, inst, sens_big_smem, slice);
}
#endif

}  // namespace osot
