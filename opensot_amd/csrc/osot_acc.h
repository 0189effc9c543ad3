// opensot_amd/csrc/osot_acc.h -- device side of the ACCELERATION task leaves: from the model quantities osot_kinematics /
// osot_dynamics leave on the device to the leaf arrays of OSOT_TASK_ACC_CARTESIAN, OSOT_TASK_ACC_COM and OSOT_TASK_ACC_POSTURAL,
// GainType::Force included
//   acceleration::Cartesian ... src/tasks/acceleration/Cartesian.cpp:127-180, 517-524   [pose_err; vel_err; Gp; Gd], a_ref + Mi f
//   acceleration::CoM ......... src/tasks/acceleration/CoM.cpp:74-97                    [com_ref - com; vel_ref - J_com qdot; Kp; Kd]
//   acceleration::Postural .... src/tasks/acceleration/Postural.cpp:135-163             [q_ref - q; qdot_ref - qdot], qddot_d
// (include/osot_mi355x.h: osot_acc_tasks has the formulas and the layouts).
//
//   acc_check ............. the argument checks of osot_acc_tasks, HIP-free: the host build runs them before any device is touched
//   osot_acc_tasks_kernel . one wavefront per instance, every term in one pass.
//
// FACTOR ONCE.  No inverse of M is formed for the tasks.  M = L L' is factored once per instance in LDS (lane = row, left-looking,
// one wave_sync per column; every lane evaluates the pivot's own fma chain, so the pivot test is wave-uniform without a broadcast).
// Every right-hand side of the instance then goes through that one factor, ONE LANE PER COLUMN with L read as LDS broadcasts:
// the 6 columns of J' of every Force-type Cartesian term (<= 48) and the postural vector (<= 49 of the 64 lanes).
//     Mi = J M^-1 J' = Y'Y with L Y = J'   (each entry once per unordered pair: exactly symmetric)
//     M^-1 v = L^-T (L^-1 v)               (the back substitution runs column-wise over all lanes)
// Minv (computeInertiaInverse) is a second pass of nv columns through the same factor: Z = L^-1, Minv = Z'Z.
// The staged rows of J serve twice: J qdot of every term (lane = row), and in place as the right-hand sides.  Row strides in LDS
// are odd (nv | 1): a lane-per-row walk at one column is then free of bank conflicts (64 banks of 4 bytes: each group of 32 lanes
// of a 64-bit read lands on 32 different bank pairs; an even stride would fold them).
//
// THE PIVOT RULE.  The computed pivot d_j = m_jj - sum_k l_jk^2 carries an absolute error of at most gamma_(j+1) m_jj <=
// (nv + 1) u max_i m_ii (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (10.5) with Theorem 10.7: Cholesky
// runs to completion exactly when the scaled matrix is further than that from singular).  A pivot that is not finite, or not
// above  acc_pivot_rel(nv) = (nv + 1) 2^-52  times the largest diagonal entry of M (2 u = 2^-52: gamma_k <= 2 k u here), is not
// distinguishable from zero and counts as failed: ok = 0, the instance's Force-type Gp, Gd, Mi and Minv are zeros, a_ref_out and
// qddot_out pass the references through, and nothing non-finite is written.
//
// Every sum is an explicit fma chain in one order on the device and in the host build; the orientation error (osot_force.h) is
// compiled with contraction off.  Square roots and divisions are IEEE on both.
#pragma once
#include <cmath>
#include <cstdlib>
#include <osot_team.h>
#include <osot_mi355x.h>
#include "osot_force.h"   // force_orientation_error

namespace osot {

// both structs travel as ONE by-value kernel argument (5.7 KB: the gain matrices of eight terms are 4.5 KB of it) and are read
// through the kernarg pointer, so that a lane-dependent term index is a load and not a copy of the argument to scratch
struct AccArgs { osot_acc_model M; osot_acc_batch Bt; };

__host__ __device__ inline double acc_pivot_rel(int nv) { return (double)(nv + 1) * 0x1p-52; }

// the wave's LDS slice, in doubles
struct AccLayout { int ldl, jld, jrows, qd, pe, ve, xs, dg, mi, js, ls, total; };
__host__ __device__ inline AccLayout acc_layout(int nv, int n_cart, bool factor, bool minv) {
    AccLayout a;
    a.ldl = nv | 1; a.jld = nv | 1;
    a.jrows = 6 * n_cart + 4;                 // 6 per Cartesian term, 3 of the CoM, the postural vector
    if (minv && nv > a.jrows) a.jrows = nv;   // the second pass: nv columns
    a.qd = 0; a.pe = nv; a.ve = 2 * nv; a.xs = 3 * nv; a.dg = 4 * nv;
    a.mi = 5 * nv;
    a.js = a.mi + 36 * n_cart;
    a.ls = a.js + a.jrows * a.jld;
    a.total = a.ls + (factor ? nv * a.ldl : 0);
    return a;
}

__host__ __device__ inline bool acc_is_force(const osot_acc_model& m, int t) { return m.cart_gain_type[t] == OSOT_ACC_GAIN_FORCE; }
__host__ __device__ inline bool acc_has_gains(const osot_acc_model& m, int t) { return m.cart_gain_matrices[t] != 0 || acc_is_force(m, t); }
__host__ __device__ inline bool acc_post_force(const osot_acc_model& m) { return m.has_postural != 0 && m.post_gain_type == OSOT_ACC_GAIN_FORCE; }
// M is read (and factored) exactly when a term is Force-type or Minv is bound
__host__ __device__ inline bool acc_needs_M(const osot_acc_model& m, const osot_acc_batch& b) {
    bool f = acc_post_force(m) || b.Minv != nullptr;
    for (int t = 0; t < m.n_cart; ++t) f = f || acc_is_force(m, t);
    return f;
}
inline int acc_lds_bytes(const osot_acc_model* m, const osot_acc_batch* b) {
    return acc_layout(m->nv, m->n_cart, acc_needs_M(*m, *b), b->Minv != nullptr).total * (int)sizeof(double);
}

// the largest slice any model and batch can ask for (nv = 64, eight terms, Minv): what the launch layer raises the kernel's limit to, once
inline int acc_lds_bytes_max() { return acc_layout(OSOT_KIN_MAX_JOINTS, OSOT_ACC_MAX_CART, true, true).total * (int)sizeof(double); }

// the checks of osot_acc_tasks (include/osot_mi355x.h); *why names the field
inline int acc_check(const osot_acc_model* m, const osot_acc_batch* b, const char** why) {
    if (!m || !b) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (m->nv < 1) { *why = "nv is below 1"; return OSOT_ERR_INVALID; }
    if (m->nv > OSOT_KIN_MAX_JOINTS) {
        *why = "nv is above 64 (beyond it: osot_id_force_gains with an inverse inertia matrix of the caller's)";
        return OSOT_ERR_UNSUPPORTED;
    }
    if (m->n_cart < 0 || m->n_cart > OSOT_ACC_MAX_CART) { *why = "n_cart is outside 0 .. 8"; return OSOT_ERR_INVALID; }
    if (b->B < 0) { *why = "B is negative"; return OSOT_ERR_INVALID; }
    const int nv = m->nv, nc = m->n_cart;
    const auto flag = [](int v) { return v == 0 || v == 1; };
    const auto type = [](int v) { return v == OSOT_ACC_GAIN_ACCELERATION || v == OSOT_ACC_GAIN_FORCE; };
    if (!flag(m->has_com) || !flag(m->has_postural)) { *why = "has_com / has_postural is not 0 or 1"; return OSOT_ERR_INVALID; }
    if (!flag(m->com_gain_matrices) || !flag(m->post_gain_matrices)) { *why = "com_gain_matrices / post_gain_matrices is not 0 or 1"; return OSOT_ERR_INVALID; }
    for (int t = 0; t < nc; ++t) {
        if (!type(m->cart_gain_type[t])) { *why = "cart_gain_type is neither OSOT_ACC_GAIN_ACCELERATION nor OSOT_ACC_GAIN_FORCE"; return OSOT_ERR_INVALID; }
        if (!flag(m->cart_gain_matrices[t])) { *why = "cart_gain_matrices is not 0 or 1"; return OSOT_ERR_INVALID; }
        if (!std::isfinite(m->cart_orientation_gain[t])) { *why = "cart_orientation_gain is not finite"; return OSOT_ERR_INVALID; }
        for (int i = 0; i < 36; ++i)
            if (!std::isfinite(m->cart_Kp[36 * t + i]) || !std::isfinite(m->cart_Kd[36 * t + i])) { *why = "cart_Kp / cart_Kd is not finite"; return OSOT_ERR_INVALID; }
    }
    if (m->has_com)
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(m->com_Kp[i]) || !std::isfinite(m->com_Kd[i])) { *why = "com_Kp / com_Kd is not finite"; return OSOT_ERR_INVALID; }
    if (m->has_postural) {
        if (!type(m->post_gain_type)) { *why = "post_gain_type is neither OSOT_ACC_GAIN_ACCELERATION nor OSOT_ACC_GAIN_FORCE"; return OSOT_ERR_INVALID; }
        if (!std::isfinite(m->post_lambda) || !std::isfinite(m->post_lambda2)) { *why = "post_lambda / post_lambda2 is not finite"; return OSOT_ERR_INVALID; }
    }
    // pointers bound to a term beyond n_cart, or to a group the model does not have
    for (int t = nc; t < OSOT_ACC_MAX_CART; ++t)
        if (b->cart_J[t] || b->cart_pose[t] || b->cart_pose_ref[t] || b->cart_vel_ref[t] || b->cart_f_virtual[t] || b->cart_a_ref_in[t] ||
            b->cart_p0[t] || b->cart_a_ref_out[t] || b->cart_Mi[t]) { *why = "a cart_ pointer is bound to a term beyond n_cart"; return OSOT_ERR_INVALID; }
    if (!m->has_com && (b->com_J || b->com || b->com_ref || b->com_vel_ref || b->com_p0))
        { *why = "com_J / com / com_ref / com_vel_ref / com_p0 is bound, but the model has no CoM term (has_com)"; return OSOT_ERR_INVALID; }
    if (!m->has_postural && (b->post_q_ref || b->post_qdot_ref || b->post_qddot_ref || b->post_p0 || b->post_qddot_out))
        { *why = "a post_ pointer is bound, but the model has no postural term (has_postural)"; return OSOT_ERR_INVALID; }
    if (!m->has_postural && (m->post_Kp || m->post_Kd)) { *why = "post_Kp / post_Kd is bound, but the model has no postural term (has_postural)"; return OSOT_ERR_INVALID; }
    if (m->has_postural && !m->post_gain_matrices && (m->post_Kp || m->post_Kd)) { *why = "post_Kp / post_Kd is bound, but post_gain_matrices is 0"; return OSOT_ERR_INVALID; }
    // inputs
    if ((nc > 0 || m->has_com || m->has_postural) && !b->qdot) { *why = "qdot is null"; return OSOT_ERR_INVALID; }
    if (m->has_postural && !b->q) { *why = "q is null (the postural term reads it)"; return OSOT_ERR_INVALID; }
    if (acc_needs_M(*m, *b)) {
        if (!b->M) { *why = "M is null (a Force-type term or Minv reads it)"; return OSOT_ERR_INVALID; }
        if (b->M_stride < (long long)nv * nv) { *why = "M_stride is below nv * nv"; return OSOT_ERR_INVALID; }
    }
    for (int t = 0; t < nc; ++t) {
        if (!b->cart_J[t] || !b->cart_pose[t] || !b->cart_pose_ref[t]) { *why = "cart_J / cart_pose / cart_pose_ref of a term is null"; return OSOT_ERR_INVALID; }
        if (b->cart_J_ld[t] < nv) { *why = "cart_J_ld is below nv"; return OSOT_ERR_INVALID; }
        if (b->cart_J_stride[t] < 6LL * b->cart_J_ld[t]) { *why = "cart_J_stride is below 6 * cart_J_ld"; return OSOT_ERR_INVALID; }
        if (b->cart_p0[t] && b->cart_p0_stride[t] < (acc_has_gains(*m, t) ? 84 : 12))
            { *why = "cart_p0_stride is below 12 (84 with gain matrices or the Force type)"; return OSOT_ERR_INVALID; }
        if (!acc_is_force(*m, t) && (b->cart_Mi[t] || b->cart_f_virtual[t]))
            { *why = "cart_Mi / cart_f_virtual is bound to a term whose cart_gain_type is not OSOT_ACC_GAIN_FORCE"; return OSOT_ERR_INVALID; }
        if (b->cart_f_virtual[t] && !b->cart_a_ref_out[t]) { *why = "cart_f_virtual without cart_a_ref_out to add Mi f to"; return OSOT_ERR_INVALID; }
        if (b->cart_a_ref_in[t] && !b->cart_a_ref_out[t]) { *why = "cart_a_ref_in without cart_a_ref_out"; return OSOT_ERR_INVALID; }
        const void* in[6] = {b->cart_J[t], b->cart_pose[t], b->cart_pose_ref[t], b->cart_vel_ref[t], b->cart_f_virtual[t], b->cart_a_ref_in[t]};
        const void* out[3] = {b->cart_p0[t], b->cart_a_ref_out[t], b->cart_Mi[t]};
        for (const void* o : out)
            for (const void* i : in)
                if (o && o == i) { *why = "cart_p0 / cart_a_ref_out / cart_Mi aliases an input of its term"; return OSOT_ERR_INVALID; }
    }
    if (m->has_com) {
        if (!b->com_J || !b->com || !b->com_ref) { *why = "com_J / com / com_ref is null"; return OSOT_ERR_INVALID; }
        if (b->com_J_ld < nv) { *why = "com_J_ld is below nv"; return OSOT_ERR_INVALID; }
        if (b->com_J_stride < 3LL * b->com_J_ld) { *why = "com_J_stride is below 3 * com_J_ld"; return OSOT_ERR_INVALID; }
        if (b->com_p0 && b->com_p0_stride < (m->com_gain_matrices ? 24 : 6)) { *why = "com_p0_stride is below 6 (24 with gain matrices)"; return OSOT_ERR_INVALID; }
        const void* in[4] = {b->com_J, b->com, b->com_ref, b->com_vel_ref};
        for (const void* i : in) if (b->com_p0 && b->com_p0 == i) { *why = "com_p0 aliases an input of the CoM term"; return OSOT_ERR_INVALID; }
    }
    if (m->has_postural) {
        if (!b->post_q_ref) { *why = "post_q_ref is null"; return OSOT_ERR_INVALID; }
        const void* in[5] = {b->q, b->qdot, b->post_q_ref, b->post_qdot_ref, b->post_qddot_ref};
        const void* out[2] = {b->post_p0, b->post_qddot_out};
        for (const void* o : out)
            for (const void* i : in)
                if (o && o == i) { *why = "post_p0 / post_qddot_out aliases an input of the postural term"; return OSOT_ERR_INVALID; }
    }
    if (b->Minv) {
        if (b->Minv_stride < (long long)nv * nv) { *why = "Minv_stride is below nv * nv"; return OSOT_ERR_INVALID; }
        if (b->Minv == b->M) { *why = "Minv aliases M"; return OSOT_ERR_INVALID; }
    }
    return OSOT_OK;
}

__global__ void __launch_bounds__(64) osot_acc_tasks_kernel(const AccArgs A) {
    OSOT_DYNAMIC_LDS(acc_smem);                                // acc_lds_bytes(model, batch)
    const AccArgs* P = OSOT_KERNARG_PTR(AccArgs, A);
    const osot_acc_model& M = P->M;
    const osot_acc_batch& Bt = P->Bt;
    const long long inst = blockIdx.x;
    const int lane = threadIdx.x;
    if (inst >= Bt.B) return;
    const int nv = M.nv, nc = M.n_cart;
    const bool factor = acc_needs_M(M, Bt), post_force = acc_post_force(M) && Bt.post_qddot_out;
    const AccLayout Ly = acc_layout(nv, nc, factor, Bt.Minv != nullptr);
    double* S = reinterpret_cast<double*>(acc_smem);
    double *qd = S + Ly.qd, *pe = S + Ly.pe, *ve = S + Ly.ve, *xs = S + Ly.xs, *Dg = S + Ly.dg, *MiS = S + Ly.mi, *JS = S + Ly.js, *Ls = S + Ly.ls;
    const int jld = Ly.jld, ldl = Ly.ldl;
    const int com_row = 6 * nc, post_row = 6 * nc + 3;

    // ---- 1. stage: qdot, the joint errors, the rows of every J (coalesced row loads), the lower triangle of M
    if (lane < nv) {
        qd[lane] = Bt.qdot ? Bt.qdot[inst * nv + lane] : 0.0;
        if (M.has_postural) {
            const double e = Bt.post_q_ref[inst * nv + lane] - Bt.q[inst * nv + lane];
            const double v = (Bt.post_qdot_ref ? Bt.post_qdot_ref[inst * nv + lane] : 0.0) - Bt.qdot[inst * nv + lane];
            pe[lane] = e; ve[lane] = v;
            if (Bt.post_p0) { Bt.post_p0[inst * 2 * nv + lane] = e; Bt.post_p0[inst * 2 * nv + nv + lane] = v; }
        }
    }
    for (int r = 0; r < 6 * nc; ++r) {
        const int t = r / 6;
        const double* Jr = Bt.cart_J[t] + inst * Bt.cart_J_stride[t] + (long long)(r - 6 * t) * Bt.cart_J_ld[t];
        if (lane < nv) JS[r * jld + lane] = Jr[lane];
    }
    if (M.has_com)
        for (int r = 0; r < 3; ++r)
            if (lane < nv) JS[(com_row + r) * jld + lane] = Bt.com_J[inst * Bt.com_J_stride + (long long)r * Bt.com_J_ld + lane];
    if (factor) {
        const double* Mg = Bt.M + inst * Bt.M_stride;
        for (int r = 0; r < nv; ++r) if (lane <= r) Ls[r * ldl + lane] = Mg[r * nv + lane];
    }
    wave_sync();

    // ---- 2. J qdot of this lane's row (Cartesian rows 6 t + d, behind them the three of the CoM)
    double jq = 0.0;
    if (lane < 6 * nc + (M.has_com ? 3 : 0))
        for (int k = 0; k < nv; ++k) jq = fma(JS[lane * jld + k], qd[k], jq);

    // ---- 3. the errors.  Cartesian: lane = 6 t + d writes entry d of both errors and column d of the copied gains
    if (lane < 6 * nc) {
        const int t = lane / 6, d = lane - 6 * t;
        if (Bt.cart_p0[t]) {
            const double* Ta = Bt.cart_pose[t] + inst * 12;
            const double* Tr = Bt.cart_pose_ref[t] + inst * 12;
            double e;
            if (d < 3) e = Tr[9 + d] - Ta[9 + d];
            else {
                double eo[3];
                force_orientation_error(Ta, Tr, eo);
                e = M.cart_orientation_gain[t] * (d == 3 ? eo[0] : d == 4 ? eo[1] : eo[2]);
            }
            double* p0 = Bt.cart_p0[t] + inst * Bt.cart_p0_stride[t];
            p0[d] = e;
            p0[6 + d] = (Bt.cart_vel_ref[t] ? Bt.cart_vel_ref[t][inst * 6 + d] : 0.0) - jq;
            if (acc_has_gains(M, t) && !acc_is_force(M, t))
                for (int i = 0; i < 6; ++i) {
                    p0[12 + 6 * i + d] = M.cart_Kp[36 * t + 6 * i + d];
                    p0[48 + 6 * i + d] = M.cart_Kd[36 * t + 6 * i + d];
                }
        }
    } else if (M.has_com && lane < 6 * nc + 3 && Bt.com_p0) {
        const int i = lane - com_row;
        double* p0 = Bt.com_p0 + inst * Bt.com_p0_stride;
        p0[i] = Bt.com_ref[inst * 3 + i] - Bt.com[inst * 3 + i];
        p0[3 + i] = (Bt.com_vel_ref ? Bt.com_vel_ref[inst * 3 + i] : 0.0) - jq;
        if (M.com_gain_matrices)
            for (int r = 0; r < 3; ++r) { p0[6 + 3 * r + i] = M.com_Kp[3 * r + i]; p0[15 + 3 * r + i] = M.com_Kd[3 * r + i]; }
    }
    // the postural vector v = lambda Kp pos_err + lambda2 Kd vel_err: row i by lane i, into the row the solves take it from
    double pv = 0.0;
    if (M.has_postural && Bt.post_qddot_out && lane < nv) {
        double kp = pe[lane], kd = ve[lane];
        if (M.post_Kp) { kp = 0.0; for (int j = 0; j < nv; ++j) kp = fma(M.post_Kp[lane * nv + j], pe[j], kp); }
        if (M.post_Kd) { kd = 0.0; for (int j = 0; j < nv; ++j) kd = fma(M.post_Kd[lane * nv + j], ve[j], kd); }
        pv = fma(M.post_lambda, kp, M.post_lambda2 * kd);
        JS[post_row * jld + lane] = pv;
    }

    // ---- 4. M = L L': lane = row, column by column; the diagonal of L goes to Dg, M's own stays where it was
    bool bad = false;
    if (factor) {
        double dmax = Ls[0];
        for (int i = 1; i < nv; ++i) { const double x = Ls[i * ldl + i]; dmax = (x > dmax || x != x) ? x : dmax; }
        const double thr = acc_pivot_rel(nv) * dmax;
        for (int j = 0; j < nv; ++j) {
            double d = Ls[j * ldl + j];
            for (int k = 0; k < j; ++k) { const double l = Ls[j * ldl + k]; d = fma(-l, l, d); }
            if (uniform_b(!(d > thr) || !(d <= 1.7976931348623157e308))) { bad = true; break; }
            const double ljj = sqrt(d);
            if (lane == 0) Dg[j] = ljj;
            if (lane > j && lane < nv) {
                double s = Ls[lane * ldl + j];
                for (int k = 0; k < j; ++k) s = fma(-Ls[lane * ldl + k], Ls[j * ldl + k], s);
                Ls[lane * ldl + j] = s / ljj;
            }
            wave_sync();
        }
    }
    wave_sync();

    // ---- 5. L Y = [J' of the Force-type terms | v]: lane = column, in place in the column's staged row
    const bool col_cart = lane < 6 * nc && acc_is_force(M, lane < 6 * nc ? lane / 6 : 0);
    const bool col_post = lane == post_row && post_force;
    if (factor && !bad && (col_cart || col_post)) {
        double* y = JS + lane * jld;
        for (int k = 0; k < nv; ++k) {
            double v = y[k];
            for (int j = 0; j < k; ++j) v = fma(-Ls[k * ldl + j], y[j], v);
            y[k] = v / Dg[k];
        }
    }
    wave_sync();

    // ---- 6. Mi = Y'Y, each entry once per unordered pair
    if (col_cart) {
        const int t = lane / 6, b = lane - 6 * t;
        for (int a = 0; a <= b; ++a) {
            double acc = 0.0;
            if (!bad) for (int k = 0; k < nv; ++k) acc = fma(JS[(6 * t + a) * jld + k], JS[lane * jld + k], acc);
            MiS[36 * t + 6 * a + b] = acc;
            MiS[36 * t + 6 * b + a] = acc;
        }
    }
    // ---- 7. x = L^-T y of the postural vector, column-wise: x_k = y_k / l_kk, then y_j -= l_kj x_k for every j < k at once
    if (post_force && !bad) {
        double yv = (lane < nv) ? JS[post_row * jld + lane] : 0.0;
        for (int k = nv - 1; k >= 0; --k) {
            if (lane == k) xs[k] = yv / Dg[k];
            wave_sync();
            if (lane < k) yv = fma(-Ls[k * ldl + lane], xs[k], yv);
        }
    }
    wave_sync();
    if (M.has_postural && Bt.post_qddot_out && lane < nv) {
        const double ref = Bt.post_qddot_ref ? Bt.post_qddot_ref[inst * nv + lane] : 0.0;
        const double add = acc_post_force(M) ? (bad ? 0.0 : xs[lane]) : pv;
        Bt.post_qddot_out[inst * nv + lane] = acc_post_force(M) && bad ? ref : ref + add;
    }

    // ---- 8. the Force-type outputs of the Cartesian terms: lane = 6 t + d writes column d of Gp, Gd, Mi and entry d of a_ref_out
    if (lane < 6 * nc) {
        const int t = lane / 6, d = lane - 6 * t;
        const double* Mi = MiS + 36 * t;
        if (acc_is_force(M, t)) {
            if (Bt.cart_p0[t]) {
                double* p0 = Bt.cart_p0[t] + inst * Bt.cart_p0_stride[t];
                for (int i = 0; i < 6; ++i) {
                    double gp = 0.0, gd = 0.0;
                    for (int k = 0; k < 6; ++k) { gp = fma(Mi[6 * i + k], M.cart_Kp[36 * t + 6 * k + d], gp); gd = fma(Mi[6 * i + k], M.cart_Kd[36 * t + 6 * k + d], gd); }
                    p0[12 + 6 * i + d] = bad ? 0.0 : gp;
                    p0[48 + 6 * i + d] = bad ? 0.0 : gd;
                }
            }
            if (Bt.cart_Mi[t]) for (int i = 0; i < 6; ++i) Bt.cart_Mi[t][inst * 36 + 6 * i + d] = Mi[6 * i + d];
        }
        if (Bt.cart_a_ref_out[t]) {
            double acc = Bt.cart_a_ref_in[t] ? Bt.cart_a_ref_in[t][inst * 6 + d] : 0.0;
            if (acc_is_force(M, t) && Bt.cart_f_virtual[t] && !bad)
                for (int k = 0; k < 6; ++k) acc = fma(Mi[6 * d + k], Bt.cart_f_virtual[t][inst * 6 + k], acc);
            Bt.cart_a_ref_out[t][inst * 6 + d] = acc;
        }
    }

    // ---- 9. Minv = Z'Z, Z = L^-1: nv columns through the same factor (the staged rows are free by now)
    if (Bt.Minv) {
        double* Mo = Bt.Minv + inst * Bt.Minv_stride;
        wave_sync();
        if (!bad && lane < nv) {
            double* z = JS + lane * jld;
            for (int k = 0; k < lane; ++k) z[k] = 0.0;
            for (int k = lane; k < nv; ++k) {
                double v = (k == lane) ? 1.0 : 0.0;
                for (int j = lane; j < k; ++j) v = fma(-Ls[k * ldl + j], z[j], v);
                z[k] = v / Dg[k];
            }
        }
        wave_sync();
        // (L is not read any more: both halves of the result are put together in its place, so that every row of Minv leaves as
        // one coalesced store instead of a column walk with a stride of nv)
        for (int a = 0; a < nv; ++a) {
            if (lane < a || lane >= nv) continue;
            double acc = 0.0;
            if (!bad) for (int k = lane; k < nv; ++k) acc = fma(JS[a * jld + k], JS[lane * jld + k], acc);
            Ls[a * ldl + lane] = acc;
            Ls[lane * ldl + a] = acc;
        }
        wave_sync();
        for (int r = 0; r < nv; ++r) if (lane < nv) Mo[r * nv + lane] = Ls[r * ldl + lane];
    }
    if (Bt.ok && lane == 0) Bt.ok[inst] = bad ? 0 : 1;
}

}  // namespace osot
