// opensot_amd/csrc/osot_force.h -- device side of the force-space task family, x = [w_0 .. w_{C-1} (6 each) | optionally tau (nv - 6)]:
// from the model quantities osot_kinematics / osot_dynamics leave on the device to the A, b, Aeq, beq of
//   force::CoM ............ src/tasks/force/CoM.cpp:106-134, 176-207, 266-279        6 rows [I 0; P_c I] per contact, and b
//   force::FloatingBase ... src/tasks/force/FloatingBase.cpp:58-76                   6 rows (Jc_c[:, 0:6])'
//   StaticConstraint ...... src/constraints/force/StaticConstraint.cpp:17-34         nv - 6 rows (Jc_c[:, 6:nv])', I on tau, beq
//   force::Cartesian ...... src/tasks/force/Cartesian.cpp:34-65                      b = Kp e + Kd (v_ref - J_f qdot) + f_des
// (include/osot_mi355x.h: osot_force_rows has the formulas, the conventions of the enabled mask and of the orientation error).
//
//   force_check ............. the argument checks of osot_force_rows, HIP-free: the host build runs them before any device is touched
//   osot_force_rows_kernel .. one wavefront per instance, LANE = COLUMN of x (columns lane, lane + 64 for n <= 128, as
//                             osot_id_rows_kernel): every output row is one coalesced store of the columns the row owns (the
//                             wrench blocks, for the static rows also the torque columns); every other column of the destination,
//                             and the gaps between rows and instances, are left untouched.  The contact Jacobians are staged
//                             through LDS once (their transposes are what the rows need), with a row stride of 65 doubles: a
//                             transposed read walks the rows at one column, and a stride of 64 would put all of them on one bank.
// HBM-bound by construction: reads C * 6 * nv + 12 C + 9 + 2 nv doubles, writes (12 + nv - 6) * 6 C + (nv - 6) * (nv - 6 + 2) + 12.
// Every b is evaluated in ONE order on the device and in the host build: sums are explicit fma chains, and the orientation error,
// whose products could be contracted either way, is compiled with contraction off.
#pragma once
#include <cmath>
#include <cstdlib>
#include <osot_team.h>
#include <osot_mi355x.h>
#include "osot_kernels.h"   // rot_to_quat

namespace osot {

constexpr int kForceStageLd = 65;   // row stride of the staged contact Jacobians (doubles)

inline int force_ld(int ld, int n) { return ld == 0 ? n : ld; }
// dynamic LDS of osot_force_rows_kernel (bytes): the staged rows of the model's C contacts (two contacts: 6.3 KB, eight: 25 KB --
// sized by the model, so that a two-contact stack keeps its resident waves) behind the six doubles of J_f qdot
inline int force_lds_bytes(int n_contacts) { return (6 + 6 * n_contacts * kForceStageLd) * (int)sizeof(double); }

// the checks of osot_force_rows (include/osot_mi355x.h); *why names the field
inline int force_check(const osot_force_model* m, const osot_force_batch* b, const char** why) {
    if (!m || !b) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (m->n_contacts < 1 || m->n_contacts > OSOT_FORCE_MAX_CONTACTS) { *why = "n_contacts is outside 1 .. 8"; return OSOT_ERR_INVALID; }
    if (m->nv < 6) { *why = "nv is below 6 (the first six coordinates are the floating base)"; return OSOT_ERR_INVALID; }
    if (m->nv > OSOT_KIN_MAX_JOINTS) { *why = "nv is above 64"; return OSOT_ERR_INVALID; }
    if (m->n < 1 || m->n > OSOT_MAX_QP_VARS) { *why = "n is outside 1 .. 128"; return OSOT_ERR_INVALID; }
    if (b->B < 0) { *why = "B is negative"; return OSOT_ERR_INVALID; }
    const int C = m->n_contacts, na = m->nv - 6;
    const bool wants_static = b->static_A || b->static_lo || b->static_up;
    if (wants_static && na == 0) { *why = "static rows asked with nv == 6 (static_A / static_lo / static_up: no actuated coordinate)"; return OSOT_ERR_INVALID; }
    for (int c = 0; c < C; ++c)
        if (m->wrench_col[c] < 0 || m->wrench_col[c] + 6 > m->n) { *why = "a wrench_col range leaves 0 .. n-1"; return OSOT_ERR_INVALID; }
    if (m->torque_col < -1 || (m->torque_col >= 0 && m->torque_col + na > m->n)) { *why = "the torque_col range leaves 0 .. n-1"; return OSOT_ERR_INVALID; }
    for (int c = 0; c < C; ++c) {
        for (int e = 0; e < c; ++e)
            if (std::abs(m->wrench_col[c] - m->wrench_col[e]) < 6) { *why = "two wrench_col ranges overlap"; return OSOT_ERR_INVALID; }
        if (m->torque_col >= 0 && m->wrench_col[c] + 6 > m->torque_col && m->torque_col + na > m->wrench_col[c])
            { *why = "the torque_col range overlaps a wrench_col range"; return OSOT_ERR_INVALID; }
    }
    const struct { const double* p; long long stride; int ld, rows; const char* ld_why; const char* stride_why; } blocks[3] = {
        {b->com_A, b->com_A_stride, b->com_A_ld, 6, "com_A_ld is below n", "com_A_stride is below 6 * ld"},
        {b->fb_A, b->fb_A_stride, b->fb_A_ld, 6, "fb_A_ld is below n", "fb_A_stride is below 6 * ld"},
        {b->static_A, b->static_A_stride, b->static_A_ld, na, "static_A_ld is below n", "static_A_stride is below (nv - 6) * ld"}};
    for (const auto& k : blocks) {
        if (!k.p) continue;
        if (k.ld != 0 && k.ld < m->n) { *why = k.ld_why; return OSOT_ERR_INVALID; }
        if (k.stride < (long long)k.rows * force_ld(k.ld, m->n)) { *why = k.stride_why; return OSOT_ERR_INVALID; }
    }
    if (b->com_b && b->com_b_stride < 6) { *why = "com_b_stride is below 6"; return OSOT_ERR_INVALID; }
    if (b->cart_b && b->cart_b_stride < 6) { *why = "cart_b_stride is below 6"; return OSOT_ERR_INVALID; }
    if ((b->static_lo == nullptr) != (b->static_up == nullptr)) { *why = "static_lo and static_up go together"; return OSOT_ERR_INVALID; }
    if (b->static_lo && b->static_b_stride < na) { *why = "static_b_stride is below nv - 6"; return OSOT_ERR_INVALID; }
    // references without the output they belong to
    if (!b->com_b && (b->com_pos_ref || b->com_vel_ref || b->com_acc_ref || b->ang_mom_ref || b->ang_mom_rate_ref))
        { *why = "com_pos_ref / com_vel_ref / com_acc_ref / ang_mom_ref / ang_mom_rate_ref without com_b"; return OSOT_ERR_INVALID; }
    if (!b->static_lo && b->static_q_tau) { *why = "static_q_tau without static_lo / static_up"; return OSOT_ERR_INVALID; }
    if (!b->cart_b && (b->cart_pose_ref || b->cart_vel_ref || b->cart_f_des || b->cart_pose_error))
        { *why = "cart_pose_ref / cart_vel_ref / cart_f_des / cart_pose_error without cart_b"; return OSOT_ERR_INVALID; }
    // gains and mass
    if (!std::isfinite(m->mass)) { *why = "mass is not finite"; return OSOT_ERR_INVALID; }
    if (!std::isfinite(m->com_lambda) || !std::isfinite(m->com_lambda2) || !std::isfinite(m->com_lambda_ang))
        { *why = "com_lambda / com_lambda2 / com_lambda_ang is not finite"; return OSOT_ERR_INVALID; }
    for (int i = 0; i < 3; ++i) if (!std::isfinite(m->gravity[i])) { *why = "gravity is not finite"; return OSOT_ERR_INVALID; }
    for (int i = 0; i < 36; ++i)
        if (!std::isfinite(m->cart_Kp[i]) || !std::isfinite(m->cart_Kd[i])) { *why = "cart_Kp / cart_Kd is not finite"; return OSOT_ERR_INVALID; }
    // an output without the inputs it is computed from
    if ((b->fb_A || b->static_A) && !b->Jc) { *why = "Jc is null (fb_A / static_A read it)"; return OSOT_ERR_INVALID; }
    if (b->com_A) {
        if (!b->com) { *why = "com is null (com_A reads it)"; return OSOT_ERR_INVALID; }
        for (int c = 0; c < C; ++c) if (!b->pose[c]) { *why = "a pose is null (com_A reads the pose of every contact)"; return OSOT_ERR_INVALID; }
    }
    if (b->com_b) {
        if (!b->com || !b->momentum) { *why = "com / momentum is null (com_b reads them)"; return OSOT_ERR_INVALID; }
        if (!(m->mass > 0.0)) { *why = "mass is not positive (com_b divides the linear momentum by it)"; return OSOT_ERR_INVALID; }
    }
    if (b->static_lo && !b->h_gravity) { *why = "h_gravity is null (static_lo / static_up read it)"; return OSOT_ERR_INVALID; }
    if (b->cart_b) {
        if (m->cart_contact < 0 || m->cart_contact >= C) { *why = "cart_contact is not a contact"; return OSOT_ERR_INVALID; }
        if (b->qdot && !b->Jc) { *why = "Jc is null (cart_b reads it with qdot)"; return OSOT_ERR_INVALID; }
        if (!b->cart_pose_error && (!b->cart_pose_ref || !b->pose[m->cart_contact]))
            { *why = "cart_b needs cart_pose_error, or cart_pose_ref and the pose of cart_contact"; return OSOT_ERR_INVALID; }
    }
    return OSOT_OK;
}

// e_o of force::Cartesian: -2 x the quaternion error of cartesian_utils.h:144-164 on the short path, from the actual (Ta) to the
// reference (Tr) orientation.  Contraction is off: the same IEEE operations, in this order, wherever it is compiled.
__device__ inline void force_orientation_error(const double* Ta, const double* Tr, double* eo) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double q[4], qd[4];
    rot_to_quat(Ta, q);
    rot_to_quat(Tr, qd);
    const double dot = ((q[0] * qd[0] + q[1] * qd[1]) + q[2] * qd[2]) + q[3] * qd[3];
    const double sg = (dot < 0.0) ? -1.0 : 1.0;
    const double qx = sg * q[0], qy = sg * q[1], qz = sg * q[2], qw = sg * q[3];
    eo[0] = -2.0 * ((qd[3] * qx - qw * qd[0]) + (qd[1] * qz - qd[2] * qy));
    eo[1] = -2.0 * ((qd[3] * qy - qw * qd[1]) + (qd[2] * qx - qd[0] * qz));
    eo[2] = -2.0 * ((qd[3] * qz - qw * qd[2]) + (qd[0] * qy - qd[1] * qx));
}

// what a lane's column is: d in 0 .. 5 of wrench ct, or torque index tq, or neither (ct = tq = -1)
struct ForceCol { int ct, d, tq; };
__device__ inline ForceCol force_col(const osot_force_model& M, int col) {
    ForceCol k = {-1, 0, -1};
    if (col >= M.n) return k;
    for (int c = 0; c < M.n_contacts; ++c)
        if (col >= M.wrench_col[c] && col < M.wrench_col[c] + 6) { k.ct = c; k.d = col - M.wrench_col[c]; }
    if (M.torque_col >= 0 && col >= M.torque_col && col < M.torque_col + (M.nv - 6)) k.tq = col - M.torque_col;
    return k;
}

__global__ void __launch_bounds__(64) osot_force_rows_kernel(const osot_force_model M, const osot_force_batch Bt) {
    OSOT_DYNAMIC_LDS(force_smem);                              // force_lds_bytes(C)
    double* jq = reinterpret_cast<double*>(force_smem);        // J_f qdot of force::Cartesian
    double* JcS = jq + 6;                                      // row 6 c + d = row d of contact c, nv columns
    const long long inst = blockIdx.x;
    const int lane = threadIdx.x;
    if (inst >= Bt.B) return;
    const int nv = M.nv, n = M.n, C = M.n_contacts, na = nv - 6;
    const bool wants_Jc = Bt.fb_A || Bt.static_A || (Bt.cart_b && Bt.qdot);
    if (wants_Jc) {
        const double* Jc = Bt.Jc + inst * (6 * C) * nv;
        for (int r = 0; r < 6 * C; ++r) if (lane < nv) JcS[r * kForceStageLd + lane] = Jc[r * nv + lane];   // coalesced row loads
        wave_sync();
    }
    // the two columns of this lane, and whether their contact is enabled
    ForceCol col[2] = {force_col(M, lane), force_col(M, lane + 64)};
    bool on[2];
    for (int h = 0; h < 2; ++h) on[h] = col[h].ct >= 0 && (!Bt.enabled || Bt.enabled[inst * C + col[h].ct] != 0);

    if (Bt.com_A) {   // block c = [I 0; P_c I], P_c = skew(t), t = p_c - com (CoM.cpp:188-203)
        const int ld = Bt.com_A_ld ? Bt.com_A_ld : n;
        double* A = Bt.com_A + inst * Bt.com_A_stride;
        for (int h = 0; h < 2; ++h) {
            if (col[h].ct < 0) continue;
            const int cc = lane + 64 * h, d = col[h].d;
            double t[3] = {0.0, 0.0, 0.0};
            if (d < 3) for (int i = 0; i < 3; ++i) t[i] = Bt.pose[col[h].ct][inst * 12 + 9 + i] - Bt.com[inst * 3 + i];
            // column d < 3 of P: (0, t2, -t1), (-t2, 0, t0), (t1, -t0, 0); the reference fills the lower triangle as the negated upper
            const double p0 = (d == 1) ? -t[2] : (d == 2) ? t[1] : 0.0;
            const double p1 = (d == 0) ? -(-t[2]) : (d == 2) ? -t[0] : 0.0;
            const double p2 = (d == 0) ? -t[1] : (d == 1) ? -(-t[0]) : 0.0;
            const double pcol[3] = {p0, p1, p2};
            for (int r = 0; r < 6; ++r) {
                double v = (r < 3) ? ((d == r) ? 1.0 : 0.0) : ((d < 3) ? pcol[r - 3] : ((d == r) ? 1.0 : 0.0));
                A[r * ld + cc] = on[h] ? v : 0.0;
            }
        }
    }
    if (Bt.fb_A) {    // block c = (Jc_c[:, 0:6])' (FloatingBase.cpp:68-70)
        const int ld = Bt.fb_A_ld ? Bt.fb_A_ld : n;
        double* A = Bt.fb_A + inst * Bt.fb_A_stride;
        for (int r = 0; r < 6; ++r)
            for (int h = 0; h < 2; ++h)
                if (col[h].ct >= 0) A[r * ld + lane + 64 * h] = on[h] ? JcS[(6 * col[h].ct + col[h].d) * kForceStageLd + r] : 0.0;
    }
    if (Bt.static_A) {   // block c = (Jc_c[:, 6:nv])', the identity on the torque columns (StaticConstraint.cpp:21-27)
        const int ld = Bt.static_A_ld ? Bt.static_A_ld : n;
        double* A = Bt.static_A + inst * Bt.static_A_stride;
        for (int r = 0; r < na; ++r)
            for (int h = 0; h < 2; ++h) {
                if (col[h].ct >= 0) A[r * ld + lane + 64 * h] = on[h] ? JcS[(6 * col[h].ct + col[h].d) * kForceStageLd + 6 + r] : 0.0;
                else if (col[h].tq >= 0) A[r * ld + lane + 64 * h] = (col[h].tq == r) ? 1.0 : 0.0;
            }
    }
    if (Bt.static_lo && lane < na) {   // beq = gcomp.tail(na) - q (StaticConstraint.cpp:32)
        const double v = Bt.h_gravity[inst * nv + 6 + lane] - (Bt.static_q_tau ? Bt.static_q_tau[inst * na + lane] : 0.0);
        Bt.static_lo[inst * Bt.static_b_stride + lane] = v;
        Bt.static_up[inst * Bt.static_b_stride + lane] = v;
    }
    if (Bt.com_b && lane < 6) {   // CoM::update_b (CoM.cpp:266-279)
        double v;
        if (lane < 3) {
            const int i = lane;
            const double com = Bt.com[inst * 3 + i];
            const double vel = Bt.momentum[inst * 6 + i] / M.mass;
            const double ev = (Bt.com_vel_ref ? Bt.com_vel_ref[inst * 3 + i] : 0.0) - vel;
            const double ep = Bt.com_pos_ref ? Bt.com_pos_ref[inst * 3 + i] - com : 0.0;
            const double acc = fma(M.com_lambda, ep, fma(M.com_lambda2, ev, Bt.com_acc_ref ? Bt.com_acc_ref[inst * 3 + i] : 0.0));
            v = M.mass * (acc - M.gravity[i]);
        } else {
            const int i = lane - 3;
            const double eL = Bt.ang_mom_ref ? Bt.ang_mom_ref[inst * 3 + i] - Bt.momentum[inst * 6 + 3 + i] : 0.0;
            v = fma(M.com_lambda_ang, eL, Bt.ang_mom_rate_ref ? Bt.ang_mom_rate_ref[inst * 3 + i] : 0.0);
        }
        Bt.com_b[inst * Bt.com_b_stride + lane] = v;
    }
    if (Bt.cart_b) {   // Cartesian::_update (force/Cartesian.cpp:47-61)
        if (lane < 6) {
            double acc = 0.0;
            if (Bt.qdot) for (int k = 0; k < nv; ++k) acc = fma(JcS[(6 * M.cart_contact + lane) * kForceStageLd + k], Bt.qdot[inst * nv + k], acc);
            jq[lane] = acc;
        }
        wave_sync();
        if (lane < 6) {
            double e[6];
            if (Bt.cart_pose_error) {
                for (int j = 0; j < 6; ++j) e[j] = Bt.cart_pose_error[inst * 6 + j];
            } else {
                const double* Ta = Bt.pose[M.cart_contact] + inst * 12;
                const double* Tr = Bt.cart_pose_ref + inst * 12;
                for (int j = 0; j < 3; ++j) e[j] = Tr[9 + j] - Ta[9 + j];
                force_orientation_error(Ta, Tr, e + 3);
            }
            double acc = Bt.cart_f_des ? Bt.cart_f_des[inst * 6 + lane] : 0.0;
            for (int j = 0; j < 6; ++j) acc = fma(M.cart_Kp[lane * 6 + j], e[j], acc);
            for (int j = 0; j < 6; ++j) acc = fma(M.cart_Kd[lane * 6 + j], (Bt.cart_vel_ref ? Bt.cart_vel_ref[inst * 6 + j] : 0.0) - jq[j], acc);
            Bt.cart_b[inst * Bt.cart_b_stride + lane] = acc;
        }
    }
}

}  // namespace osot
