// opensot_amd/csrc/osot_qp_sens.h -- multipliers, active set and the backward pass of the batched explicit QP
//     min 1/2 x'Hx + g'x   s.t.  lA <= A x <= uA,  l <= x <= u        (BackEnd.h:125-150)
// from the problem and a solution x that osot_qp_solve_batch (or anybody else) has left on the device: what the reference keeps as
// QPOasesBackEnd::getDualSolution (src/solvers/QPOasesBackEnd.cpp:153-158, 291-296) and getActiveBounds / getActiveConstraints
// (include/OpenSoT/solvers/QPOasesBackEnd.h:163-172), and the vector-Jacobian product of x with respect to H, g, A, lA, uA, l, u
// (include/osot_mi355x.h: osot_qp_sensitivity_batch has the contract).
//
//   sens_check ............ the argument checks of osot_qp_sensitivity_batch, HIP-free: the host build runs them too
//   osot_qp_sens_kernel ... one wavefront per instance, n <= 64 (NP = 32: n <= 32, NP = 64 above), any nc
//
// THE ROUTE.  H~ = H + eps I = L L' (lane = row, left-looking, the pivot rule of osot_acc.h).  The candidates -- every equality,
// every finite side whose residual is within active_tol max(1, |bound|) -- are found in one pass: the bounds by lane = variable, the
// rows of A in tiles that are staged coalesced (lane = column) and then read lane = row, so that a_r'x is one fma chain in one order
// (a cross-lane tree would not be reproducible on the host).  Only the candidates' rows are staged again, as the columns of
// Y = L^-1 C' (ONE LANE PER COLUMN through the factor, L read as LDS broadcasts), with -(L'x + L^-1 g) and L^-1 grad_x as two
// more columns.  A Householder QR with column pivoting (the largest remaining column norm, recomputed at every step as one fma
// chain per column) runs over all columns at once, the right-hand sides included: after r steps the first r entries of the two
// extra columns are Q1't and Q1'w, the multipliers are R^-1 of the first, d lambda = -R^-1 of the second, and
// w + Y d lambda = (I - Q1 Q1') w = Q [0; (Q'w)_(r..)] is put together from the reflectors, which stay where the pivot columns
// were.  dx = -L^-T of that.  A weakly active or wrong-signed inequality leaves the set and the whole of this is redone ONCE.
//
// LDS: L is n x (n | 1), Y is (2n + 2) x (n | 1) doubles (odd row strides: a lane-per-row walk at one column has no bank
// conflict, see osot_acc.h), 12 n doubles of vectors and 13 n ints of lists: 30 608 bytes at n = 32, 110 352 at n = 64 (sens_lds_bytes).
// Every sum is an explicit fma chain in one order on the device and in the host build; square roots and divisions are IEEE on both.
// Nothing non-finite is written: an instance whose x, factor or results are not finite is SKIPPED with zeros.
#pragma once
#include <cmath>
#include <cstdlib>
#include <osot_team.h>
#include <osot_mi355x.h>
#include "osot_acc.h"   // acc_pivot_rel

namespace osot {

struct SensArgs { osot_qp_sens_batch b; double active_tol, dual_tol, rank_tol; };

// stores of the zero fill are complete before the scatter over them starts (the same wave, other lanes)
#ifdef OSOT_EMULATION
inline void sens_store_fence() {}
#else
__device__ __forceinline__ void sens_store_fence() { __threadfence(); }
#endif

__host__ __device__ inline bool sens_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
__host__ __device__ inline bool sens_present(double v) { return fabs(v) < 1e20; }   // NaN: absent

// the wave's LDS slice: offsets in doubles (ints: in ints from the start of the int part)
struct SensLayout { int ldl, ldy, cap, L, Y, xs, hv, zv, dxs, rd, hb, h0, dg, lam, dlam, nrm, ints, total; };
__host__ __device__ inline SensLayout sens_layout(int n) {
    SensLayout a;
    a.ldl = n | 1; a.ldy = n | 1; a.cap = 2 * n;
    a.L = 0;
    a.Y = a.L + n * a.ldl;
    a.xs = a.Y + (a.cap + 2) * a.ldy;
    a.hv = a.xs + n; a.zv = a.hv + n; a.dxs = a.zv + n; a.rd = a.dxs + n; a.hb = a.rd + n; a.h0 = a.hb + n; a.dg = a.h0 + n;
    a.lam = a.dg + n; a.dlam = a.lam + n;
    a.nrm = a.dlam + n;                        // 2n
    a.ints = a.nrm + a.cap;                    // cidx, cside, cstate, erow, irow, iside: 2n each; piv: n
    a.total = a.ints + (13 * n + 1) / 2;
    return a;
}
inline int sens_lds_bytes(int n) { return sens_layout(n).total * (int)sizeof(double); }

inline void sens_options(const osot_qp_sens_options* o, double* active_tol, double* dual_tol, double* rank_tol) {
    *active_tol = (o && o->active_tol != 0.0) ? o->active_tol : 1e-8;
    *dual_tol = (o && o->dual_tol != 0.0) ? o->dual_tol : 1e-9;
    *rank_tol = (o && o->rank_tol != 0.0) ? o->rank_tol : 1e-11;
}

// the checks of osot_qp_sensitivity_batch (include/osot_mi355x.h); *why names the field
inline int sens_check(const osot_qp_sens_batch* b, const osot_qp_sens_options* o, const char** why) {
    if (!b) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (b->B < 0) { *why = "B is negative"; return OSOT_ERR_INVALID; }
    if (b->n < 1) { *why = "n is below 1"; return OSOT_ERR_INVALID; }
    if (b->n > OSOT_MAX_VARS) { *why = "n is above 64 (the sensitivity kernel is one wavefront per instance; 65 .. 128 variables are not built)"; return OSOT_ERR_UNSUPPORTED; }
    if (b->nc < 0) { *why = "nc is negative"; return OSOT_ERR_INVALID; }
    if (o) {
        const double t[3] = {o->active_tol, o->dual_tol, o->rank_tol};
        for (double v : t) if (!(v >= 0.0) || !sens_finite(v)) { *why = "a tolerance is negative or not finite"; return OSOT_ERR_INVALID; }
    }
    if (!(b->eps_abs >= 0.0) || !sens_finite(b->eps_abs)) { *why = "eps_abs is negative or not finite"; return OSOT_ERR_INVALID; }
    if (b->B == 0) return OSOT_OK;
    if (!b->H || !b->g || !b->x) { *why = "H / g / x is null"; return OSOT_ERR_INVALID; }
    if (!b->flag) { *why = "flag is null"; return OSOT_ERR_INVALID; }
    if (b->nc > 0 && !b->A) { *why = "nc is above 0 but A is null"; return OSOT_ERR_INVALID; }
    if (b->nc > 0 && (!b->lA || !b->uA)) { *why = "A without its bounds lA / uA"; return OSOT_ERR_INVALID; }
    if ((b->l == nullptr) != (b->u == nullptr)) { *why = "l and u must both be given or both be null"; return OSOT_ERR_INVALID; }
    const bool any_grad = b->grad_H || b->grad_g || b->grad_A || b->grad_lA || b->grad_uA || b->grad_l || b->grad_u;
    if (any_grad && !b->grad_x) { *why = "a gradient output without grad_x"; return OSOT_ERR_INVALID; }
    const void* in[10] = {b->H, b->g, b->A, b->lA, b->uA, b->l, b->u, b->x, b->status, b->grad_x};
    const void* out[10] = {b->y, b->active, b->grad_H, b->grad_g, b->grad_A, b->grad_lA, b->grad_uA, b->grad_l, b->grad_u, b->flag};
    for (const void* q : out)
        for (const void* i : in)
            if (q && q == i) { *why = "an output aliases an input"; return OSOT_ERR_INVALID; }
    return OSOT_OK;
}

// 0: not a candidate, -1 / +1: the lower / upper side is within tol, 2: an equality
__host__ __device__ inline int sens_side(double v, double lo, double up, double tol) {
    const bool flo = sens_present(lo), fup = sens_present(up);
    if (flo && fup && lo == up) return 2;
    if (flo && fabs(v - lo) <= tol * fmax(1.0, fabs(lo))) return -1;
    if (fup && fabs(v - up) <= tol * fmax(1.0, fabs(up))) return 1;
    return 0;
}

// The column a lane works on in its pass t (slot = lane + 64 t).  With more than 64 columns the two right-hand sides, columns 2n
// and 2n + 1, take the slots of lanes 63 and 62 in the FIRST pass: the candidates fill the lanes from 0 upwards and are rarely
// more than 62, so the right-hand sides do not queue behind a candidate column of their lane.
__host__ __device__ inline int sens_col(int slot, int cap, int ncol) {
    if (ncol <= 64) return slot;
    return slot == 63 ? cap : (slot == 62 ? cap + 1 : (slot < 62 ? slot : slot - 2));
}

// every output of the instance is zero (what a SKIPPED instance leaves; the zero fill of the others)
__device__ inline void sens_zero_outputs(const osot_qp_sens_batch& b, long long inst, int lane, int n, int nc) {
    const long long m = n + nc;
    for (long long e = lane; e < m; e += 64) {
        if (b.y) b.y[inst * m + e] = 0.0;
        if (b.active) b.active[inst * m + e] = 0;
    }
    for (int e = lane; e < n; e += 64) {
        if (b.grad_g) b.grad_g[inst * n + e] = 0.0;
        if (b.grad_l) b.grad_l[inst * n + e] = 0.0;
        if (b.grad_u) b.grad_u[inst * n + e] = 0.0;
    }
    for (long long e = lane; e < nc; e += 64) {
        if (b.grad_lA) b.grad_lA[inst * nc + e] = 0.0;
        if (b.grad_uA) b.grad_uA[inst * nc + e] = 0.0;
    }
    if (b.grad_A) for (long long e = lane; e < (long long)nc * n; e += 64) b.grad_A[inst * nc * n + e] = 0.0;
}

template <int NP>
__global__ void __launch_bounds__(64) osot_qp_sens_kernel(const SensArgs A_) {
    OSOT_DYNAMIC_LDS(sens_smem);                               // sens_lds_bytes(n)
    const SensArgs* P = OSOT_KERNARG_PTR(SensArgs, A_);
    const osot_qp_sens_batch& b = P->b;
    const long long inst = blockIdx.x;
    const int lane = threadIdx.x;
    if (inst >= b.B) return;
    const int n = b.n < NP ? b.n : NP;                         // (n <= NP by the launch layer)
    const int nc = b.nc;
    const bool back = b.grad_x != nullptr;
    const SensLayout Ly = sens_layout(n);
    const int ldl = Ly.ldl, ldy = Ly.ldy, cap = Ly.cap, ncol = cap + 2;
    double* S = reinterpret_cast<double*>(sens_smem);
    double *Ls = S + Ly.L, *Y = S + Ly.Y, *xs = S + Ly.xs, *hv = S + Ly.hv, *zv = S + Ly.zv, *dxs = S + Ly.dxs, *rd = S + Ly.rd, *hb = S + Ly.hb,
           *h0 = S + Ly.h0, *Dg = S + Ly.dg, *lam = S + Ly.lam, *dlam = S + Ly.dlam, *nrm = S + Ly.nrm;
    int* I = reinterpret_cast<int*>(S + Ly.ints);
    int *cidx = I, *cside = I + cap, *cstate = I + 2 * cap, *erow = I + 3 * cap, *irow = I + 4 * cap, *iside = I + 5 * cap, *piv = I + 6 * cap;
    double* tcol = Y + cap * ldy;            // -(L'x + L^-1 g), then Q't
    double* wcol = Y + (cap + 1) * ldy;      // L^-1 grad_x, then Q'w
    const double* Hg = b.H + inst * n * n;
    const double* Ag = nc > 0 ? b.A + inst * nc * n : nullptr;

    // ---- 0. an instance that was not solved, or whose x is not finite, is skipped
    const double xv = (lane < n) ? b.x[inst * n + lane] : 0.0;
    bool skip = b.status != nullptr && b.status[inst] != OSOT_STATUS_SOLVED;
    skip = skip || wave_ballot(!sens_finite(xv)) != 0ull;
    if (uniform_b(skip)) {
        sens_zero_outputs(b, inst, lane, n, nc);
        if (b.grad_H) for (int e = lane; e < n * n; e += 64) b.grad_H[inst * n * n + e] = 0.0;
        if (lane == 0) b.flag[inst] = OSOT_SENS_SKIPPED;
        return;
    }

    // ---- 1. stage x and the lower triangle of H + eps I
    if (lane < n) xs[lane] = xv;
    for (int r = 0; r < n; ++r) if (lane <= r) Ls[r * ldl + lane] = Hg[r * n + lane] + (lane == r ? b.eps_abs : 0.0);
    wave_sync();

    // ---- 2. the candidates.  Bounds: lane = variable
    int bs = 0;
    if (b.l && lane < n) bs = sens_side(xv, b.l[inst * n + lane], b.u[inst * n + lane], P->active_tol);
    const unsigned long long mEb = wave_ballot(bs == 2), mIb = wave_ballot(bs == 1 || bs == -1);
    const int neb = __builtin_popcountll(mEb), nib = __builtin_popcountll(mIb);
    // rows: tiles of tr rows staged into Y's place (lane = column), then lane = row
    int ner = 0, nir = 0;
    const int tr = ncol < 64 ? ncol : 64;
    for (int t0 = 0; t0 < nc; t0 += tr) {
        const int rows = nc - t0 < tr ? nc - t0 : tr;
        for (int rr = 0; rr < rows; ++rr) if (lane < n) Y[rr * ldy + lane] = Ag[(long long)(t0 + rr) * n + lane];
        wave_sync();
        int rs = 0;
        if (lane < rows) {
            double ax = 0.0;
            for (int k = 0; k < n; ++k) ax = fma(Y[lane * ldy + k], xs[k], ax);
            rs = sens_side(ax, b.lA[inst * nc + t0 + lane], b.uA[inst * nc + t0 + lane], P->active_tol);
            if (!sens_finite(ax)) rs = 0;
        }
        const unsigned long long mE = wave_ballot(rs == 2), mI = wave_ballot(rs == 1 || rs == -1);
        const int pe = ner + lanes_below(mE), pi = nir + lanes_below(mI);
        if (rs == 2 && pe < cap) erow[pe] = t0 + lane;
        if ((rs == 1 || rs == -1) && pi < cap) { irow[pi] = t0 + lane; iside[pi] = rs; }
        ner += __builtin_popcountll(mE); nir += __builtin_popcountll(mI);
        if (ner > cap) ner = cap + 1;          // (more than the capacity is all that matters: no overflow of the counts)
        if (nir > cap) nir = cap + 1;
        wave_sync();
    }
    // the list, in the order equalities (bounds, rows), bounds, rows, cut at 2n
    const int total = neb + ner + nib + nir;
    const int k = total < cap ? total : cap;
    bool degenerate = total > cap;
    {
        if (bs == 2) { const int p = lanes_below(mEb); if (p < cap) { cidx[p] = lane; cside[p] = 2; } }
        for (int j = lane; j < ner && j < cap; j += 64) { const int p = neb + j; if (p < cap) { cidx[p] = n + erow[j]; cside[p] = 2; } }
        if (bs == 1 || bs == -1) { const int p = neb + ner + lanes_below(mIb); if (p < cap) { cidx[p] = lane; cside[p] = bs; } }
        for (int j = lane; j < nir && j < cap; j += 64) { const int p = neb + ner + nib + j; if (p < cap) { cidx[p] = n + irow[j]; cside[p] = iside[j]; } }
        for (int c = lane; c < cap; c += 64) cstate[c] = 0;
    }
    wave_sync();

    // ---- 3. H~ = L L': lane = row, column by column; the diagonal of L goes to Dg
    bool bad = false;
    {
        double dmax = Ls[0];
        for (int i = 1; i < n; ++i) { const double v = Ls[i * ldl + i]; dmax = (v > dmax || v != v) ? v : dmax; }
        const double thr = acc_pivot_rel(n) * dmax;
        for (int j = 0; j < n; ++j) {
            double d = Ls[j * ldl + j];
            for (int q = 0; q < j; ++q) { const double v = Ls[j * ldl + q]; d = fma(-v, v, d); }
            if (uniform_b(!(d > thr) || !(d <= 1.7976931348623157e308))) { bad = true; break; }
            const double ljj = sqrt(d);
            if (lane == 0) Dg[j] = ljj;
            if (lane > j && lane < n) {
                double s = Ls[lane * ldl + j];
                for (int q = 0; q < j; ++q) s = fma(-Ls[lane * ldl + q], Ls[j * ldl + q], s);
                Ls[lane * ldl + j] = s / ljj;
            }
            wave_sync();
        }
    }
    wave_sync();

    int r = 0;
    for (int pass = 0; pass < 2 && !bad; ++pass) {
        // ---- 4. the columns of Y = L^-1 C' of the candidates still in the set, and the two right-hand sides
        for (int c = 0; c < k; ++c) {
            if (cstate[c] != 0) continue;
            const int idx = cidx[c];
            if (lane < n) Y[c * ldy + lane] = idx < n ? (lane == idx ? 1.0 : 0.0) : Ag[(long long)(idx - n) * n + lane];
        }
        if (lane < n) {
            tcol[lane] = b.g[inst * n + lane];
            wcol[lane] = back ? b.grad_x[inst * n + lane] : 0.0;
        }
        wave_sync();
        for (int slot = lane; slot < ncol; slot += 64) {
            const int c = sens_col(slot, cap, ncol);
            if (c < cap && (c >= k || cstate[c] != 0)) continue;
            double* y = Y + c * ldy;
            const int q0 = (c < cap && cidx[c] < n) ? cidx[c] : 0;      // a unit vector: zeros above its one stay zeros
            for (int q = q0; q < n; ++q) {
                double v = y[q];
                for (int j = q0; j < q; ++j) v = fma(-Ls[q * ldl + j], y[j], v);
                y[q] = v / Dg[q];
            }
        }
        wave_sync();
        // t = -(L'x + L^-1 g): lane = entry
        if (lane < n) {
            double s = fma(Dg[lane], xs[lane], tcol[lane]);
            for (int i = lane + 1; i < n; ++i) s = fma(Ls[i * ldl + lane], xs[i], s);
            tcol[lane] = -s;
        }
        wave_sync();

        // ---- 5. Householder QR with column pivoting over every column at once
        double first = 0.0;
        r = 0;
        for (int j = 0; j < n; ++j) {
            for (int c = lane; c < k; c += 64) {
                if (cstate[c] != 0) continue;
                double s = 0.0;
                for (int i = j; i < n; ++i) { const double v = Y[c * ldy + i]; s = fma(v, v, s); }
                nrm[c] = s;
            }
            wave_sync();
            int p = -1;
            double best = -1.0;
            for (int c = 0; c < k; ++c) if (cstate[c] == 0 && nrm[c] > best) { best = nrm[c]; p = c; }
            p = uniform_i(p);
            if (p < 0) break;
            const double norm = sqrt(best);
            if (j == 0) first = norm;
            if (uniform_b(!(norm > 0.0) || !sens_finite(norm) || norm < P->rank_tol * first)) break;
            const double x0 = Y[p * ldy + j];
            const double alpha = x0 >= 0.0 ? -norm : norm;
            const double v0 = x0 - alpha;
            const double beta = 1.0 / fma(norm, fabs(x0), best);       // 2 / v'v
            wave_sync();                                                // (everybody has read cstate and nrm)
            if (lane >= j && lane < n) hv[lane] = lane == j ? v0 : Y[p * ldy + lane];
            if (lane == 0) { rd[j] = alpha; hb[j] = beta; h0[j] = v0; piv[j] = p; cstate[p] = 1; }
            wave_sync();
            for (int slot = lane; slot < ncol; slot += 64) {
                const int c = sens_col(slot, cap, ncol);
                if (c < cap && (c >= k || cstate[c] != 0)) continue;
                double* y = Y + c * ldy;
                double s = 0.0;
                for (int i = j; i < n; ++i) s = fma(hv[i], y[i], s);
                s *= beta;
                for (int i = j; i < n; ++i) y[i] = fma(-s, hv[i], y[i]);
            }
            wave_sync();
            r = j + 1;
        }
        // what is left in the set is dependent on the pivots
        bool dependent = false;
        for (int c = 0; c < k; ++c) dependent = dependent || cstate[c] == 0;
        wave_sync();
        for (int c = lane; c < k; c += 64) if (cstate[c] == 0) cstate[c] = 2;

        // ---- 6. R lambda = Q1't and R dlambda = -Q1'w, column-wise: lane = row of R
        {
            double tv = (lane < r) ? tcol[lane] : 0.0, wv = (lane < r) ? -wcol[lane] : 0.0;
            for (int j = r - 1; j >= 0; --j) {
                if (lane == j) { lam[j] = tv / rd[j]; dlam[j] = wv / rd[j]; }
                wave_sync();
                if (lane < j) {
                    const double rij = Y[piv[j] * ldy + lane];
                    tv = fma(-rij, lam[j], tv);
                    wv = fma(-rij, dlam[j], wv);
                }
            }
        }
        wave_sync();

        // ---- 7. weakly active or wrong-signed inequalities leave the set, once
        double linf = 0.0;
        for (int j = 0; j < r; ++j) { const double a = fabs(lam[j]); linf = (a > linf || a != a) ? a : linf; }
        bool weak = false;
        if (lane < r) {
            const int side = cside[piv[lane]];
            const double v = lam[lane];
            weak = side != 2 && (fabs(v) <= P->dual_tol * fmax(1.0, linf) || (side == -1 ? v > 0.0 : v < 0.0));
        }
        const bool any_weak = wave_ballot(weak) != 0ull;
        degenerate = degenerate || dependent || any_weak;
        if (pass == 0 && any_weak) {
            wave_sync();
            for (int c = lane; c < k; c += 64) if (cstate[c] != 3) cstate[c] = 0;
            wave_sync();
            if (weak) cstate[piv[lane]] = 3;
            wave_sync();
            continue;
        }
        break;
    }

    // ---- 8. the backward pass: z = Q [0; (Q'w)_(r..)] from the reflectors, dx = -L^-T z
    if (!bad && back) {
        if (lane < n) zv[lane] = lane < r ? 0.0 : wcol[lane];
        wave_sync();
        for (int j = r - 1; j >= 0; --j) {
            const double* v = Y + piv[j] * ldy;
            double s = h0[j] * zv[j];
            for (int i = j + 1; i < n; ++i) s = fma(v[i], zv[i], s);
            s *= hb[j];
            wave_sync();
            if (lane >= j && lane < n) zv[lane] = fma(-s, lane == j ? h0[j] : v[lane], zv[lane]);
            wave_sync();
        }
        double yv = (lane < n) ? zv[lane] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            if (lane == q) dxs[q] = -(yv / Dg[q]);
            wave_sync();
            if (lane < q) yv = fma(Ls[q * ldl + lane], dxs[q], yv);
        }
        wave_sync();
    }
    // ---- 9. nothing non-finite leaves
    if (!bad) {
        bool fin = true;
        for (int j = 0; j < r; ++j) fin = fin && sens_finite(lam[j]) && (!back || sens_finite(dlam[j]));
        if (back) for (int i = 0; i < n; ++i) fin = fin && sens_finite(dxs[i]);
        bad = !fin;
    }
    bad = uniform_b(bad);

    // ---- 10. the outputs: zeros everywhere, then the set's entries over them
    sens_zero_outputs(b, inst, lane, n, nc);
    if (b.grad_H) {
        double* G = b.grad_H + inst * n * n;
        for (int i = 0; i < n; ++i) {      // (the pair in one order for both triangles: symmetric to the bit)
            if (lane >= n) continue;
            const int lo = i < lane ? i : lane, hi = i < lane ? lane : i;
            G[i * n + lane] = bad ? 0.0 : 0.5 * fma(dxs[lo], xs[hi], xs[lo] * dxs[hi]);
        }
    }
    if (!bad) {
        sens_store_fence();
        wave_sync();
        if (b.grad_g && lane < n) b.grad_g[inst * n + lane] = dxs[lane];
        const long long m = n + nc;
        if (lane < r) {
            const int c = piv[lane], idx = cidx[c], side = cside[c];
            if (b.y) b.y[inst * m + idx] = -lam[lane];
            if (b.active) b.active[inst * m + idx] = side;
            if (back) {
                const double v = -dlam[lane];
                if (idx < n) {
                    if (side == 1) { if (b.grad_u) b.grad_u[inst * n + idx] = v; }
                    else if (b.grad_l) b.grad_l[inst * n + idx] = v;
                } else {
                    if (side == 1) { if (b.grad_uA) b.grad_uA[inst * nc + idx - n] = v; }
                    else if (b.grad_lA) b.grad_lA[inst * nc + idx - n] = v;
                }
            }
        }
        if (b.grad_A)
            for (int j = 0; j < r; ++j) {
                const int idx = cidx[piv[j]];
                if (idx >= n && lane < n) b.grad_A[(inst * nc + (idx - n)) * n + lane] = fma(dlam[j], xs[lane], lam[j] * dxs[lane]);
            }
    }
    if (lane == 0) b.flag[inst] = bad ? OSOT_SENS_SKIPPED : (degenerate ? OSOT_SENS_DEGENERATE : OSOT_SENS_OK);
}

}  // namespace osot
