// opensot_amd/csrc/osot_grad.h -- batched posture-gradient producer: the b of tasks::velocity::Manipulability and
// tasks::velocity::MinimumEffort (src/tasks/velocity/Manipulability.cpp:58-84, MinimumEffort.cpp:51-77; the workers in
// include/OpenSoT/tasks/velocity/Manipulability.h:130-150 and MinimumEffort.h:89-96).
//
// Per term and active joint i the reference evaluates a cost f at q + step e_i and q - step e_i -- two whole model updates per joint --
// and writes grad[i] = (f+ - f-) / (2 step), b = lambda grad (manipulability) or b = -1.0 lambda grad (minimum effort), with
//   manipulability: f = sqrt(fabs(det(J W J'))), J the 6 x n Jacobian of a frame (world, or relative to its frame_base) or the 3 x n
//                   Jacobian of the centre of mass;
//   minimum effort: f = tau_g' W tau_g, tau_g the gravity compensation over all n coordinates.
// model.sum(q, delta) is plain addition (the floating base is three prismatic and three revolute virtual joints).
//
// One wavefront per instance, LANE = PERTURBED JOINT i.  The forward kinematics run ONCE (kin_instance with no output bound); perturbing
// joint i is a rigid motion G_i of everything attached to the links of sub(i): a rotation by +-step about the axis (z_i, p_i), or a
// translation by +-step z_i for a prismatic joint, applied to the world quantities in LDS.  A uniform loop over the columns l reads
// z_l, p_l and the subtree aggregates S_l = sum over sub(l) of m [c, 1] as LDS broadcasts; the lane moves them when l is in sub(i), and for
// an ancestor l of i the aggregate becomes S_l - S_i + G(S_i).  Every lane accumulates its own 21 (frame) or 6 (CoM) entries of
// J W J', or sum_l w_l tau_l^2: no cross-lane reduction.  The determinant is a fully unrolled symmetric elimination without pivoting
// (static indices: registers, no scratch); a pivot that is exactly zero gives index 0.
//
// Three facts about the reference that shape this:
//   * a worker builds a FRESH Cartesian task on its own model copy (Manipulability.h:110-111), so the frame_col_mask of the original
//     task is not applied to J;
//   * frame_body and the R_b' rotation of a relative Jacobian are orthogonal block transforms diag(R', R') of J: det(J W J') does not
//     change, so the kernel skips them (the sign of a column of the base chain drops out of col col' as well);
//   * tau_g = -M_tot J_com' g: what osot_dynamics writes as h when qdot is NULL (the tests cross-check the two).
// W is the worker's CONSTANT weight; only its diagonal is offered.
#pragma once
#include <cmath>
#include <cstring>
#include "osot_kin.h"

namespace osot {

struct DevGrad {           // the tree with its tables and the terms, in device memory
    DevKin k;
    int n_terms;
    int kind[OSOT_GRAD_MAX_TERMS];
    int frame[OSOT_GRAD_MAX_TERMS];
    double step[OSOT_GRAD_MAX_TERMS];
    double sin_step[OSOT_GRAD_MAX_TERMS];                  // sin(step)
    double ver_step[OSOT_GRAD_MAX_TERMS];                  // 1 - cos(step) = 2 sin^2(step / 2): no cancellation
    double lambda[OSOT_GRAD_MAX_TERMS];
    unsigned long long joint_mask[OSOT_GRAD_MAX_TERMS];    // bit i set: joint i is active (all ones where the description said 0)
    double W[OSOT_GRAD_MAX_TERMS][OSOT_KIN_MAX_JOINTS];
    double gravity[3];
};

// osot_grad_create's checks and the device image (no device is touched): shared with the host build of the kernel
// (tests/emu/grad_host.cpp)
inline int grad_build(const osot_kin_desc* t, const osot_grad_desc* in, DevGrad& h, const char** why) {
    if (!t || !in) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (t->n < 1 || t->n > OSOT_KIN_MAX_JOINTS) { *why = "joint count out of range"; return OSOT_ERR_INVALID; }
    if (t->n_frames < 0 || t->n_frames > OSOT_KIN_MAX_FRAMES) { *why = "frame count out of range"; return OSOT_ERR_INVALID; }
    for (int j = 0; j < t->n; ++j) {
        if (t->parent[j] >= j || t->parent[j] < -1) { *why = "joints must be in tree order (parent[j] < j)"; return OSOT_ERR_INVALID; }
        if (t->type[j] != OSOT_JOINT_REVOLUTE && t->type[j] != OSOT_JOINT_PRISMATIC) { *why = "unknown joint type"; return OSOT_ERR_INVALID; }
        double a2 = 0.0;
        bool finite = std::isfinite(t->mass[j]);
        for (int i = 0; i < 3; ++i) { a2 += t->axis[j][i] * t->axis[j][i]; finite = finite && std::isfinite(t->p0[j][i]) && std::isfinite(t->com[j][i]); }
        for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(t->R0[j][i]);
        if (!finite || !std::isfinite(a2)) { *why = "the model holds a NaN or an infinity"; return OSOT_ERR_INVALID; }
        if (!(std::fabs(a2 - 1.0) <= 1.0e-9)) { *why = "joint axes must be unit vectors"; return OSOT_ERR_INVALID; }
        if (!(t->mass[j] >= 0.0)) { *why = "negative link mass"; return OSOT_ERR_INVALID; }
    }
    {
        const int rc = kin_check_frames(t, why);
        if (rc != OSOT_OK) return rc;
    }
    for (int f = 0; f < t->n_frames; ++f) {
        bool finite = true;
        for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(t->frame_R[f][i]);
        for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(t->frame_p[f][i]);
        if (!finite) { *why = "the model holds a NaN or an infinity"; return OSOT_ERR_INVALID; }
    }
    if (in->n_terms < 1 || in->n_terms > OSOT_GRAD_MAX_TERMS) { *why = "term count out of range (1..4)"; return OSOT_ERR_INVALID; }
    for (int k = 0; k < in->n_terms; ++k) {
        if (in->kind[k] != OSOT_GRAD_MANIPULABILITY_FRAME && in->kind[k] != OSOT_GRAD_MANIPULABILITY_COM && in->kind[k] != OSOT_GRAD_MIN_EFFORT) {
            *why = "unknown gradient kind"; return OSOT_ERR_INVALID;
        }
        if (in->kind[k] == OSOT_GRAD_MANIPULABILITY_FRAME && (in->frame[k] < 0 || in->frame[k] >= t->n_frames)) {
            *why = "manipulability of a frame the model does not have"; return OSOT_ERR_INVALID;
        }
        if (!std::isfinite(in->step[k]) || !(in->step[k] > 0.0)) { *why = "the finite-difference step must be finite and positive"; return OSOT_ERR_INVALID; }
        if (!std::isfinite(in->lambda[k])) { *why = "lambda is not finite"; return OSOT_ERR_INVALID; }
        for (int j = 0; j < t->n; ++j) if (!std::isfinite(in->W_diag[k][j])) { *why = "W_diag is not finite"; return OSOT_ERR_INVALID; }
    }
    for (int i = 0; i < 3; ++i) if (!std::isfinite(in->gravity[i])) { *why = "gravity is not finite"; return OSOT_ERR_INVALID; }
    std::memset(&h, 0, sizeof(h));
    h.k.d = *t;
    h.k.d.n_pairs = 0;
    h.k.d.n_points = 0;
    kin_build_tables(h.k);
    h.n_terms = in->n_terms;
    for (int k = 0; k < in->n_terms; ++k) {
        h.kind[k] = in->kind[k];
        h.frame[k] = in->kind[k] == OSOT_GRAD_MANIPULABILITY_FRAME ? in->frame[k] : 0;
        h.step[k] = in->step[k];
        h.sin_step[k] = std::sin(in->step[k]);
        const double sh = std::sin(0.5 * in->step[k]);
        h.ver_step[k] = 2.0 * sh * sh;
        h.lambda[k] = in->lambda[k];
        h.joint_mask[k] = in->joint_mask[k] ? in->joint_mask[k] : ~0ull;
        for (int j = 0; j < t->n; ++j) h.W[k][j] = in->W_diag[k][j];
    }
    for (int i = 0; i < 3; ++i) h.gravity[i] = in->gravity[i];
    return OSOT_OK;
}

// osot_posture_gradient's checks of a batch against the tree and the terms
inline int grad_check_batch(int n, int n_terms, const osot_grad_batch* b, const char** why) {
    if (!b) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (b->B < 0) { *why = "negative batch"; return OSOT_ERR_INVALID; }
    for (int k = 0; k < OSOT_GRAD_MAX_TERMS; ++k) {
        if (!b->b[k] && b->b_stride[k] != 0) { *why = "b is null but its stride is not zero"; return OSOT_ERR_INVALID; }
        if ((b->b[k] || b->value[k]) && k >= n_terms) { *why = "output bound to a term the producer does not have"; return OSOT_ERR_INVALID; }
        if (b->b[k] && b->b_stride[k] < n) { *why = "b_stride is below n"; return OSOT_ERR_INVALID; }
    }
    if (b->B == 0) return OSOT_OK;
    if (!b->q) { *why = "q is null"; return OSOT_ERR_INVALID; }
    return OSOT_OK;
}

// the kinematics batch the kernel hands to kin_instance: same B and q, no output
inline osot_kin_batch grad_kin_batch(const osot_grad_batch& b) {
    osot_kin_batch kb;
    std::memset(&kb, 0, sizeof(kb));
    kb.B = b.B;
    kb.q = b.q;
    return kb;
}

// det of the symmetric N x N matrix whose lower triangle is a[r (r + 1) / 2 + c] (c <= r), by elimination without pivoting: every index
// is a compile-time constant once the loops are unrolled, so the triangle stays in registers.  A pivot that is exactly zero (or below
// the smallest normal number) ends it with 0: no Inf, no NaN.
template <int N>
__device__ __forceinline__ double sym_det(double (&a)[N * (N + 1) / 2]) {
    double det = 1.0;
    bool zero = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double d = a[k * (k + 1) / 2 + k];
        zero = zero || !(fabs(d) >= 2.2250738585072014e-308);
        const double inv = zero ? 0.0 : 1.0 / d;
        det *= d;
#pragma unroll
        for (int r = k + 1; r < N; ++r) {
            const double lrk = a[r * (r + 1) / 2 + k] * inv;
#pragma unroll
            for (int c = k + 1; c <= r; ++c) a[r * (r + 1) / 2 + c] -= lrk * a[c * (c + 1) / 2 + k];
        }
    }
    return zero ? 0.0 : det;
}

// LDS of one instance, in doubles: the kinematics stages' slice, the subtree aggregates [JMAX][4] and one term's weights [JMAX]
template <int JMAX> constexpr int grad_lds_doubles() { return kin_lds_doubles<JMAX>(false) + JMAX * 4 + JMAX; }

template <int JMAX>
__device__ __forceinline__ void grad_instance(const DevGrad* __restrict__ G, const osot_grad_batch& Bt, const osot_kin_batch& Kb,
                                              const long long inst, const bool live, const int j, double* lds) {
    constexpr int TS = OSOT_KIN_TS;
    const DevKin* __restrict__ K = &G->k;
    const int n = K->d.n;
    const int jc = (j < n) ? j : 0;
    const int type_j = K->d.type[jc], dfs_j = K->dfs_pos[jc], end_j = K->sub_end[jc];
    const double grav[3] = {G->gravity[0], G->gravity[1], G->gravity[2]};
    const double iM = 1.0 / K->total_mass;
    // ---- the kinematics producer's own stages with no output bound: they leave the world [R | p] of every joint and of every frame,
    // the world axes, m [c, 1] of every link at its depth-first position and the ancestor masks in LDS (kin_instance's layout)
    kin_instance<false, JMAX>(K, Kb, inst, live, j, lds);
    static_assert(kin_lds_doubles<JMAX>(false) == JMAX * TS + JMAX * 3 + JMAX * 4 + JMAX + (JMAX + 1) / 2 + OSOT_KIN_MAX_FRAMES * (14 + 1),
                  "osot_grad.h restates the LDS layout of kin_instance (osot_kin.h): update both");
    const double* Tw = lds;
    const double* Zw = lds + JMAX * TS;
    double* Cw = lds + JMAX * TS + JMAX * 3;
    const unsigned long long* Anc = reinterpret_cast<const unsigned long long*>(Cw + JMAX * 4);
    const int* Par = reinterpret_cast<const int*>(Anc + JMAX);
    const double* Fw = reinterpret_cast<const double*>(Par + 2 * ((JMAX + 1) / 2));
    double* Sg = lds + kin_lds_doubles<JMAX>(false);      // subtree aggregates [sum m c, sum m] of every joint
    double* Wl = Sg + JMAX * 4;                           // the weights of the term at hand
    const bool valid = j < n && live;
    const bool rev_i = valid && type_j == OSOT_JOINT_REVOLUTE;
    const unsigned long long rev_mask = wave_ballot(rev_i);
    wave_sync();
    // ---- subtree aggregates: inclusive prefix sums of m [c, 1] over the depth-first order, then a difference per joint (as the centre-of-mass
    // stage of the kinematics producer does)
    {
        double a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = Cw[j * 4 + i];
#pragma unroll
        for (int d = 1; d < JMAX; d <<= 1) {
            double t[4];
            const int src = (j >= d) ? j - d : 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) t[i] = Cw[src * 4 + i];
            wave_sync();
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] += (j >= d) ? t[i] : 0.0; Cw[j * 4 + i] = a[i]; }
            wave_sync();
        }
    }
    double pi[3], zi[3], Si[4];
    {
        const int hi = valid ? end_j - 1 : 0, lo = (valid && dfs_j > 0) ? dfs_j - 1 : 0;
        const bool from0 = !(valid && dfs_j > 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double ph = Cw[hi * 4 + i], pl = Cw[lo * 4 + i];
            Si[i] = valid ? ph - (from0 ? 0.0 : pl) : 0.0;
            Sg[j * 4 + i] = Si[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { pi[i] = valid ? Tw[j * TS + 9 + i] : 0.0; zi[i] = valid ? Zw[j * 3 + i] : 0.0; }
    }
    const unsigned long long anc_i = valid ? Anc[j] : 0ull;
    const int nt = G->n_terms;
    for (int t = 0; t < nt; ++t) {
        double* bt = Bt.b[t];
        double* vt = Bt.value[t];
        if (!bt && !vt) continue;
        const int kind = G->kind[t];
        const double step = G->step[t], sin_step = G->sin_step[t], ver_step = G->ver_step[t], lambda = G->lambda[t];
        const unsigned long long active = G->joint_mask[t];
        const double wj = G->W[t][jc];
        wave_sync();                     // the previous term's loop has read its weights (and, first, the aggregates are written)
        Wl[j] = (j < n) ? wj : 0.0;
        wave_sync();
        // the frame of a manipulability term: its world origin, the joints of its own chain and of its base link's chain
        int jf = 0, jb = 0;
        bool has_base = false;
        double pf[3] = {0.0, 0.0, 0.0};
        if (kind == OSOT_GRAD_MANIPULABILITY_FRAME) {
            const int f = G->frame[t];
            jf = (int)Fw[f * 14 + 12];
            const int bf = ((int)Fw[f * 14 + 13] >> 1) - 1;
            has_base = bf >= 0;
            jb = has_base ? (int)Fw[bf * 14 + 12] : 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) pf[i] = Fw[f * 14 + 9 + i];
        }
        const unsigned long long anc_f = Anc[jf], anc_b = has_base ? Anc[jb] : 0ull;
        double fv[3] = {0.0, 0.0, 0.0};          // f(q + step e_i), f(q - step e_i), f(q)
        const int passes = vt ? 3 : 2;
        for (int pass = 0; pass < passes; ++pass) {
            const bool act = pass < 2 && valid;
            const double sgn = pass == 0 ? 1.0 : -1.0;
            const double sn = sgn * sin_step, tr = sgn * step;
            // the lane's rigid motion: a direction x -> R x, a point x -> p_i + R (x - p_i)  (revolute; R = E + sn [z]x + ver [z]x^2, i.e.
            // R x = x + sn z x x + ver (z (z . x) - x)),  or x -> x, x -> x + tr z_i  (prismatic)
            auto rot = [&](const double* x, double* o) {
                double zx[3];
                cross3(zi, x, zx);
                const double zd = zi[0] * x[0] + zi[1] * x[1] + zi[2] * x[2];
#pragma unroll
                for (int i = 0; i < 3; ++i) o[i] = rev_i ? x[i] + (sn * zx[i] + ver_step * (zi[i] * zd - x[i])) : x[i];
            };
            auto mov = [&](const double* x, double* o) {
                const double d[3] = {x[0] - pi[0], x[1] - pi[1], x[2] - pi[2]};
                double r[3];
                rot(d, r);
#pragma unroll
                for (int i = 0; i < 3; ++i) o[i] = rev_i ? pi[i] + r[i] : x[i] + tr * zi[i];
            };
            double f = 0.0;
            if (kind == OSOT_GRAD_MANIPULABILITY_FRAME) {
                double pe[3];
                {
                    double pm[3];
                    mov(pf, pm);
                    const bool moved = act && ((anc_f >> j) & 1ull) != 0ull;
#pragma unroll
                    for (int i = 0; i < 3; ++i) pe[i] = moved ? pm[i] : pf[i];
                }
                double A[21];
#pragma unroll
                for (int i = 0; i < 21; ++i) A[i] = 0.0;
                for (int l = 0; l < n; ++l) {
                    const bool in_d = ((anc_f >> l) & 1ull) != 0ull, in_b = ((anc_b >> l) & 1ull) != 0ull;
                    const double w = Wl[l];
                    if (in_d == in_b || w == 0.0) continue;        // (uniform: the joint moves both links or neither, or has no weight)
                    const bool moved = act && ((Anc[l] >> j) & 1ull) != 0ull;     // l is in sub(i)
                    const bool rev_l = ((rev_mask >> l) & 1ull) != 0ull;
                    const double zl[3] = {Zw[l * 3], Zw[l * 3 + 1], Zw[l * 3 + 2]};
                    const double pl[3] = {Tw[l * TS + 9], Tw[l * TS + 10], Tw[l * TS + 11]};
                    double zm[3], pm[3], z[3], dlt[3], col[6];
                    rot(zl, zm);
                    mov(pl, pm);
#pragma unroll
                    for (int i = 0; i < 3; ++i) { z[i] = moved ? zm[i] : zl[i]; dlt[i] = pe[i] - (moved ? pm[i] : pl[i]); }
                    cross3(z, dlt, col);
#pragma unroll
                    for (int i = 0; i < 3; ++i) { col[i] = rev_l ? col[i] : z[i]; col[3 + i] = rev_l ? z[i] : 0.0; }
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        const double wc = w * col[r];
#pragma unroll
                        for (int c = 0; c <= r; ++c) A[r * (r + 1) / 2 + c] = fma(wc, col[c], A[r * (r + 1) / 2 + c]);
                    }
                }
                f = sqrt(fabs(sym_det<6>(A)));
            } else {
                // centre of mass / gravity torques: the column of joint l is u_l = z_l x (Sc_l - Sm_l p_l) (revolute) or Sm_l z_l (prismatic)
                // from the aggregates of sub(l); J_com = u / M, tau_g = -g . u
                double dS[3];                       // G(Sc_i) - Sc_i: what the motion adds to the aggregate of every ancestor of i
                {
                    double sm[3];
                    if (rev_i) {
                        const double d[3] = {Si[0] - Si[3] * pi[0], Si[1] - Si[3] * pi[1], Si[2] - Si[3] * pi[2]};
                        double r[3];
                        rot(d, r);
#pragma unroll
                        for (int i = 0; i < 3; ++i) sm[i] = Si[3] * pi[i] + r[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < 3; ++i) sm[i] = Si[i] + Si[3] * (tr * zi[i]);
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i) dS[i] = act ? sm[i] - Si[i] : 0.0;
                }
                double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                double eff = 0.0;
                for (int l = 0; l < n; ++l) {
                    const double w = Wl[l];
                    if (w == 0.0) continue;
                    const bool in_sub = act && ((Anc[l] >> j) & 1ull) != 0ull;                 // l is in sub(i): the whole column moves
                    const bool above = act && !in_sub && ((anc_i >> l) & 1ull) != 0ull;        // l is a strict ancestor of i
                    const bool rev_l = ((rev_mask >> l) & 1ull) != 0ull;
                    const double zl[3] = {Zw[l * 3], Zw[l * 3 + 1], Zw[l * 3 + 2]};
                    const double pl[3] = {Tw[l * TS + 9], Tw[l * TS + 10], Tw[l * TS + 11]};
                    const double sm = Sg[l * 4 + 3];
                    double dlt[3], u[3], um[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) dlt[i] = (Sg[l * 4 + i] + (above ? dS[i] : 0.0)) - sm * pl[i];
                    cross3(zl, dlt, u);
#pragma unroll
                    for (int i = 0; i < 3; ++i) u[i] = rev_l ? u[i] : sm * zl[i];
                    rot(u, um);
#pragma unroll
                    for (int i = 0; i < 3; ++i) u[i] = in_sub ? um[i] : u[i];
                    if (kind == OSOT_GRAD_MANIPULABILITY_COM) {
                        const double col[3] = {u[0] * iM, u[1] * iM, u[2] * iM};
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const double wc = w * col[r];
#pragma unroll
                            for (int c = 0; c <= r; ++c) A[r * (r + 1) / 2 + c] = fma(wc, col[c], A[r * (r + 1) / 2 + c]);
                        }
                    } else {
                        const double tau = -(grav[0] * u[0] + grav[1] * u[1] + grav[2] * u[2]);
                        eff = fma(w * tau, tau, eff);
                    }
                }
                f = kind == OSOT_GRAD_MANIPULABILITY_COM ? sqrt(fabs(sym_det<3>(A))) : eff;
            }
            fv[0] = pass == 0 ? f : fv[0];
            fv[1] = pass == 1 ? f : fv[1];
            fv[2] = pass == 2 ? f : fv[2];
        }
        if (bt && valid) {
            const double grad = ((active >> j) & 1ull) ? (fv[0] - fv[1]) / (2.0 * step) : 0.0;
            bt[inst * Bt.b_stride[t] + j] = kind == OSOT_GRAD_MIN_EFFORT ? -1.0 * lambda * grad : lambda * grad;
        }
        if (vt && live && j == 0) vt[inst] = fv[2];
    }
}

template <int JMAX>
__global__ void __launch_bounds__(64) osot_grad_kernel(const DevGrad* __restrict__ G, const osot_grad_batch Bt, const osot_kin_batch Kb) {
    OSOT_STATIC_LDS(double, grad_lds, grad_lds_doubles<JMAX>());
    const int j = (int)threadIdx.x;
    const long long inst = (long long)blockIdx.x;
    grad_instance<JMAX>(G, Bt, Kb, inst, inst < Bt.B, j, grad_lds);
}

}  // namespace osot
