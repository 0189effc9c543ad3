// opensot_amd/csrc/osot_feedback.h -- device side of the tasks driven by MEASUREMENTS (force/torque sensor, joint torques, IMU, pair
// distances): from what the sensors and osot_kinematics / osot_dynamics leave on the device to the references and rows of
//   velocity::CartesianAdmittance ... src/tasks/velocity/CartesianAdmittance.cpp:50-77, 303-320, filter CartesianAdmittance.h:27-137
//                                     desired twist of an OSOT_TASK_CARTESIAN leaf; adjointFromRotation taken as blockdiag(R, R)
//   velocity::JointAdmittance ....... src/tasks/velocity/JointAdmittance.cpp:28-44     desired velocity of an OSOT_TASK_POSTURAL leaf
//   floating_base::IMU .............. src/tasks/floating_base/IMU.cpp:33-42            6 rows over the six base columns, and b
//   floating_base::Contact .......... src/tasks/floating_base/Contact.cpp:55-66        the lambda * err term added to rowset_b
//   tasks::velocity::CollisionAvoidance  src/tasks/velocity/CollisionAvoidance.cpp:17-47  A = -J, b = err on the violated pairs
// (include/osot_mi355x.h: osot_feedback has the formulas and the layout of the filter state).
//
//   feedback_check ........ the argument checks of osot_feedback, HIP-free: the host build runs them before any device is touched
//   feedback_coeffs ....... the filter coefficients of a model (host: computeCoeff, CartesianAdmittance.h:115-124, as it is written)
//   osot_feedback_kernel .. one wavefront per instance.  Cartesian terms: lane = 6 t + channel, all terms in one pass.  Joint filter:
//                           lane = coordinate; y goes through LDS, the dense compliance is staged through LDS by coalesced rows (row
//                           stride 65 doubles, as in osot_force.h) and lane i forms row i of C y.  IMU and collision rows: lane =
//                           column (lane, lane + 64), one coalesced store per row.  The filter state is read once, written once.
//                           Collision rows go eight to a trip (their loads in flight before the first store).
// HBM-bound by construction, per instance 8 (2 count + 24 n_cart (+ 12 n_cart with references) + 3 nv + n_pairs (2 n + 2) + 93)
// bytes with every group bound (93: the IMU and contact groups); the dense compliance is one matrix for the batch and stays in
// the caches.  Measured: profiles/feedback_rows.txt.
// Every sum is evaluated in ONE order on the device and in the host build: C y is an explicit fma chain, everything else is compiled
// with contraction off (the same IEEE operations, in this order, wherever it is compiled).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <osot_team.h>
#include <osot_mi355x.h>
#include "osot_kernels.h"   // rot_to_quat

namespace osot {

constexpr int kFeedbackStageLd = 65;   // row stride of the staged compliance (doubles)

// a0, a1, a2 of every filter, and 1.0 / a0 (the reference forms this quotient first in every process()): passed by value
struct FeedbackCoeffs {
    double cart[OSOT_FEEDBACK_MAX_CART * 6][3];   // {1 / a0, a1, a2}
    double joint[3];
};
static_assert(sizeof(osot_feedback_model) + sizeof(osot_feedback_batch) + sizeof(FeedbackCoeffs) <= 4096, "kernel arguments are limited to 4 KB");

// SecondOrderFilter::computeCoeff (CartesianAdmittance.h:115-124), b1 = 2, b2 = 1: c = {1 / a0, a1, a2}, *a0_out = a0
inline void feedback_filter_coeff(double omega, double eps, double ts, double* c, double* a0_out = nullptr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a0 = 1.0 + 4.0 * eps / (omega * ts) + 4.0 / std::pow(omega * ts, 2.0);
    const double a1 = 2 - 8.0 / std::pow(omega * ts, 2.0);
    const double a2 = 1.0 + 4.0 / std::pow(omega * ts, 2.0) - 4.0 * eps / (omega * ts);
    c[0] = 1.0 / a0; c[1] = a1; c[2] = a2;
    if (a0_out) *a0_out = a0;
}

inline void feedback_coeffs(const osot_feedback_model* m, FeedbackCoeffs* k) {
    memset(k, 0, sizeof(*k));
    for (int t = 0; t < m->n_cart; ++t)
        for (int c = 0; c < 6; ++c)
            feedback_filter_coeff(m->cart_omega[6 * t + c], m->cart_damping[6 * t + c], m->cart_ts[t], k->cart[6 * t + c]);
    if (m->joint) feedback_filter_coeff(m->joint_omega, m->joint_damping, m->joint_ts, k->joint);
}

inline int feedback_state_count(const osot_feedback_model* m) { return 4 * (6 * m->n_cart + (m->joint ? m->nv : 0)); }
inline int feedback_ld(int ld, int n) { return ld == 0 ? n : ld; }
// dynamic LDS of osot_feedback_kernel (bytes): y of the joint filter, behind it the staged compliance where it is dense
inline int feedback_lds_bytes(const osot_feedback_model* m, const osot_feedback_batch* b) {
    return (64 + ((m->joint && b->joint_C) ? m->nv * kFeedbackStageLd : 0)) * (int)sizeof(double);
}

// do [p, p + (B - 1) sp + w) and [q, q + (B - 1) sq + w) share a double?  Equal strides: entries interleaved in one buffer do not.
inline bool feedback_overlap(const double* p, long long sp, const double* q, long long sq, int B, int w) {
    if (B < 1) return false;
    const std::intptr_t a = (std::intptr_t)p / 8, c = (std::intptr_t)q / 8;
    const std::intptr_t a1 = a + (std::intptr_t)(B - 1) * sp + w, c1 = c + (std::intptr_t)(B - 1) * sq + w;
    if (a1 <= c || c1 <= a) return false;
    if (sp != sq || sp < 2 * w) return true;
    const std::intptr_t d = ((a - c) % sp + sp) % sp;
    return d < w || d > sp - w;
}

// the checks of osot_feedback (include/osot_mi355x.h); *why names the field
inline int feedback_check(const osot_feedback_model* m, const osot_feedback_batch* b, const char** why) {
    if (!m || !b) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (m->nv < 1 || m->nv > OSOT_KIN_MAX_JOINTS) { *why = "nv is outside 1 .. 64"; return OSOT_ERR_INVALID; }
    if (m->floating_base != 0 && m->floating_base != 1) { *why = "floating_base is not 0 or 1"; return OSOT_ERR_INVALID; }
    if (m->n_cart < 0 || m->n_cart > OSOT_FEEDBACK_MAX_CART) { *why = "n_cart is outside 0 .. 8"; return OSOT_ERR_INVALID; }
    if (m->joint != 0 && m->joint != 1) { *why = "joint is not 0 or 1"; return OSOT_ERR_INVALID; }
    if (m->imu != 0 && m->imu != 1) { *why = "imu is not 0 or 1"; return OSOT_ERR_INVALID; }
    if (m->n_pairs < 0 || m->n_pairs > OSOT_KIN_MAX_PAIRS) { *why = "n_pairs is outside 0 .. 32"; return OSOT_ERR_INVALID; }
    if (m->n_pairs > 0 && (m->n < 1 || m->n > OSOT_MAX_QP_VARS)) { *why = "n is outside 1 .. 128"; return OSOT_ERR_INVALID; }
    if (b->B < 0) { *why = "B is negative"; return OSOT_ERR_INVALID; }
    const int nv = m->nv, B = b->B;
    // the constants
    for (int t = 0; t < m->n_cart; ++t) {
        if (!std::isfinite(m->cart_ts[t]) || !(m->cart_ts[t] > 0.0)) { *why = "a cart_ts is not positive and finite"; return OSOT_ERR_INVALID; }
        for (int c = 6 * t; c < 6 * t + 6; ++c) {
            if (!std::isfinite(m->cart_C[c])) { *why = "a cart_C is not finite"; return OSOT_ERR_INVALID; }
            if (!std::isfinite(m->cart_deadzone[c]) || m->cart_deadzone[c] < 0.0) { *why = "a cart_deadzone is negative or not finite"; return OSOT_ERR_INVALID; }
            if (!std::isfinite(m->cart_omega[c]) || !(m->cart_omega[c] > 0.0)) { *why = "a cart_omega is not positive and finite"; return OSOT_ERR_INVALID; }
            if (!std::isfinite(m->cart_damping[c]) || m->cart_damping[c] < 0.0) { *why = "a cart_damping is negative or not finite"; return OSOT_ERR_INVALID; }
        }
    }
    if (m->joint) {
        if (!std::isfinite(m->joint_ts) || !(m->joint_ts > 0.0)) { *why = "joint_ts is not positive and finite"; return OSOT_ERR_INVALID; }
        if (!std::isfinite(m->joint_omega) || !(m->joint_omega > 0.0)) { *why = "joint_omega is not positive and finite"; return OSOT_ERR_INVALID; }
        if (!std::isfinite(m->joint_damping) || m->joint_damping < 0.0) { *why = "joint_damping is negative or not finite"; return OSOT_ERR_INVALID; }
        if (!std::isfinite(m->joint_C_scalar)) { *why = "joint_C_scalar is not finite"; return OSOT_ERR_INVALID; }
    }
    if (!std::isfinite(m->contact_lambda)) { *why = "contact_lambda is not finite"; return OSOT_ERR_INVALID; }
    if (m->n_pairs > 0 && !std::isfinite(m->ca_threshold)) { *why = "ca_threshold is not finite"; return OSOT_ERR_INVALID; }
    // the state
    if (m->n_cart + m->joint > 0 && !b->state) { *why = "state is null (the model has admittance terms)"; return OSOT_ERR_INVALID; }
    // Cartesian admittance terms
    for (int t = 0; t < OSOT_FEEDBACK_MAX_CART; ++t) {
        const bool any_in = b->cart_pose[t] || b->cart_wrench[t] || b->cart_wrench_ref[t] || b->cart_twist_in[t];
        if (t >= m->n_cart) {
            if (any_in || b->cart_twist_out[t]) { *why = "a cart_* pointer is bound to a term beyond n_cart"; return OSOT_ERR_INVALID; }
            continue;
        }
        if (!b->cart_twist_out[t]) {
            if (any_in) { *why = "cart_pose / cart_wrench / cart_wrench_ref / cart_twist_in without cart_twist_out"; return OSOT_ERR_INVALID; }
            continue;
        }
        if (!b->cart_pose[t] || !b->cart_wrench[t]) { *why = "cart_pose / cart_wrench is null (cart_twist_out reads them)"; return OSOT_ERR_INVALID; }
        if (b->cart_twist_in[t] && feedback_overlap(b->cart_twist_in[t], 6, b->cart_twist_out[t], 6, B, 6))
            { *why = "cart_twist_out aliases cart_twist_in"; return OSOT_ERR_INVALID; }
    }
    // joint admittance
    if (b->joint_qdot_out) {
        if (!m->joint) { *why = "joint_qdot_out with joint == 0"; return OSOT_ERR_INVALID; }
        if (!b->joint_tau || !b->joint_h) { *why = "joint_tau / joint_h is null (joint_qdot_out reads them)"; return OSOT_ERR_INVALID; }
    } else if (b->joint_tau || b->joint_h || b->joint_C) { *why = "joint_tau / joint_h / joint_C without joint_qdot_out"; return OSOT_ERR_INVALID; }
    // IMU
    if (b->imu_A || b->imu_b) {
        if (!m->imu) { *why = "imu_A / imu_b with imu == 0"; return OSOT_ERR_INVALID; }
        if (nv < 6) { *why = "imu rows asked with nv below 6 (the first six coordinates are the floating base)"; return OSOT_ERR_INVALID; }
    }
    if (b->imu_A) {
        if (!b->imu_fb_J) { *why = "imu_fb_J is null (imu_A reads it)"; return OSOT_ERR_INVALID; }
        if (b->imu_fb_J_stride < 6LL * nv) { *why = "imu_fb_J_stride is below 6 * nv"; return OSOT_ERR_INVALID; }
        if (b->imu_A_ld != 0 && b->imu_A_ld < 6) { *why = "imu_A_ld is below 6"; return OSOT_ERR_INVALID; }
        if (b->imu_A_stride < 6LL * feedback_ld(b->imu_A_ld, 6)) { *why = "imu_A_stride is below 6 * ld"; return OSOT_ERR_INVALID; }
    } else if (b->imu_fb_J) { *why = "imu_fb_J without imu_A"; return OSOT_ERR_INVALID; }
    if (b->imu_b) {
        if (!b->imu_pose || !b->imu_omega) { *why = "imu_pose / imu_omega is null (imu_b reads them)"; return OSOT_ERR_INVALID; }
        if (b->imu_b_stride < 6) { *why = "imu_b_stride is below 6"; return OSOT_ERR_INVALID; }
    } else if (b->imu_pose || b->imu_omega) { *why = "imu_pose / imu_omega without imu_b"; return OSOT_ERR_INVALID; }
    // contact error
    if (b->contact_b_out) {
        if (!b->contact_pose || !b->contact_pose_ref || !b->contact_b_in)
            { *why = "contact_pose / contact_pose_ref / contact_b_in is null (contact_b_out reads them)"; return OSOT_ERR_INVALID; }
        if (b->contact_b_in_stride < 6) { *why = "contact_b_in_stride is below 6"; return OSOT_ERR_INVALID; }
        if (b->contact_b_out_stride < 6) { *why = "contact_b_out_stride is below 6"; return OSOT_ERR_INVALID; }
        if (feedback_overlap(b->contact_b_in, b->contact_b_in_stride, b->contact_b_out, b->contact_b_out_stride, B, 6))
            { *why = "contact_b_out aliases contact_b_in"; return OSOT_ERR_INVALID; }
    } else if (b->contact_pose || b->contact_pose_ref || b->contact_b_in)
        { *why = "contact_pose / contact_pose_ref / contact_b_in without contact_b_out"; return OSOT_ERR_INVALID; }
    // collision task
    if (b->ca_A || b->ca_b) {
        if (m->n_pairs < 1) { *why = "ca_A / ca_b with n_pairs == 0"; return OSOT_ERR_INVALID; }
        if (!b->ca_dist) { *why = "ca_dist is null (ca_A / ca_b read it)"; return OSOT_ERR_INVALID; }
    } else if (b->ca_dist || b->ca_J) { *why = "ca_dist / ca_J without ca_A / ca_b"; return OSOT_ERR_INVALID; }
    if (b->ca_A) {
        if (!b->ca_J) { *why = "ca_J is null (ca_A reads it)"; return OSOT_ERR_INVALID; }
        if (b->ca_J == b->ca_A) { *why = "ca_A aliases ca_J"; return OSOT_ERR_INVALID; }
        if (b->ca_J_stride < (long long)m->n_pairs * m->n) { *why = "ca_J_stride is below n_pairs * n"; return OSOT_ERR_INVALID; }
        if (b->ca_A_ld != 0 && b->ca_A_ld < m->n) { *why = "ca_A_ld is below n"; return OSOT_ERR_INVALID; }
        if (b->ca_A_stride < (long long)m->n_pairs * feedback_ld(b->ca_A_ld, m->n)) { *why = "ca_A_stride is below n_pairs * ld"; return OSOT_ERR_INVALID; }
    } else if (b->ca_J) { *why = "ca_J without ca_A"; return OSOT_ERR_INVALID; }
    if (b->ca_b && b->ca_b_stride < m->n_pairs) { *why = "ca_b_stride is below n_pairs"; return OSOT_ERR_INVALID; }
    return OSOT_OK;
}

// osot_admittance_params (include/osot_mi355x.h): CartesianAdmittance::computeParameters as it is written
inline int feedback_admittance_params(const double* K, const double* D, double lambda, double dt, double* C, double* M, double* w, const char** why) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!K || !D || !C || !M || !w) { *why = "null argument"; return OSOT_ERR_INVALID; }
    for (int i = 0; i < 6; ++i)
        if (!(D[i] > (K[i] * dt) / lambda)) { *why = "D[i] <= K[i] * dt / lambda"; return OSOT_ERR_INVALID; }
    for (int i = 0; i < 6; ++i) {
        C[i] = lambda * (1.0 / K[i]);
        M[i] = (dt / lambda) * D[i] - ((dt * dt) / lambda) * (1.0 / C[i]);
        w[i] = dt * (1.0 / (C[i] * M[i]));
    }
    return OSOT_OK;
}

// one step of SecondOrderFilter::process (CartesianAdmittance.h:62-77) on the stored (u, ud, y, yd): s = {u, ud, y, yd} is rewritten,
// the new y returned.  udd and ydd live only inside the step (the reference overwrites them before it reads them).
__device__ inline double feedback_filter_step(double* s, double input, const double* k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ydd = s[3], yd = s[2], udd = s[1], ud = s[0], u = input;
    const double y = k[0] * ((((u + 2.0 * ud) + 1.0 * udd) - k[1] * yd) - k[2] * ydd);
    s[0] = u; s[1] = ud; s[2] = y; s[3] = yd;
    return y;
}

// apply_deadzone (CartesianAdmittance.cpp:303-320), one channel
__device__ inline double feedback_deadzone(double v, double dz) {
    if (v > dz) return v - dz;
    if (v < -dz) return v + dz;
    return 0.0;
}

// [p_d - p; -e_o] of floating_base::Contact (Contact.cpp:60-63): e_o = the quaternion error of cartesian_utils.h:144-164 on the
// short path, from the actual (Ta) to the reference (Tr) pose.  Contraction is off, as in force_orientation_error.
__device__ inline void feedback_contact_error(const double* Ta, const double* Tr, double* e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double q[4], qd[4];
    rot_to_quat(Ta, q);
    rot_to_quat(Tr, qd);
    const double dot = ((q[0] * qd[0] + q[1] * qd[1]) + q[2] * qd[2]) + q[3] * qd[3];
    const double sg = (dot < 0.0) ? -1.0 : 1.0;
    const double qx = sg * q[0], qy = sg * q[1], qz = sg * q[2], qw = sg * q[3];
    for (int i = 0; i < 3; ++i) e[i] = Tr[9 + i] - Ta[9 + i];
    e[3] = -((qd[3] * qx - qw * qd[0]) + (qd[1] * qz - qd[2] * qy));
    e[4] = -((qd[3] * qy - qw * qd[1]) + (qd[2] * qx - qd[0] * qz));
    e[5] = -((qd[3] * qz - qw * qd[2]) + (qd[0] * qy - qd[1] * qx));
}

__global__ void __launch_bounds__(64) osot_feedback_kernel(const osot_feedback_model M, const osot_feedback_batch Bt, const FeedbackCoeffs K) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    OSOT_DYNAMIC_LDS(feedback_smem);                           // feedback_lds_bytes
    double* ys = reinterpret_cast<double*>(feedback_smem);     // y of the joint filter
    double* Cs = ys + 64;                                      // row i of the dense compliance at i * kFeedbackStageLd
    const long long inst = blockIdx.x;
    const int lane = threadIdx.x;
    if (inst >= Bt.B) return;
    const int nv = M.nv, count = 4 * (6 * M.n_cart + (M.joint ? nv : 0));
    double* state = Bt.state ? Bt.state + inst * count : nullptr;

    // 1. CartesianAdmittance::_update: lane = 6 t + channel
    if (lane < 6 * M.n_cart) {
        const int t = lane / 6, c = lane - 6 * t, r = (c < 3) ? c : c - 3, h = (c < 3) ? 0 : 3;
        double* out = Bt.cart_twist_out[t];
        if (out) {
            const double* T = Bt.cart_pose[t] + inst * 12;
            const double* w = Bt.cart_wrench[t] + inst * 6 + h;
            const double* wr = Bt.cart_wrench_ref[t];
            const double* tin = Bt.cart_twist_in[t];
            double* s = state + 24 * t + c;                    // u, ud, y, yd of the term's six channels: 6 doubles apart
            double st[4] = {s[0], s[6], s[12], s[18]};
            double e = (T[3 * r] * w[0] + T[3 * r + 1] * w[1]) + T[3 * r + 2] * w[2];
            e = feedback_deadzone(e, M.cart_deadzone[lane]);
            e -= wr ? wr[inst * 6 + c] : 0.0;
            const double y = feedback_filter_step(st, e, K.cart[lane]);
            s[0] = st[0]; s[6] = st[1]; s[12] = st[2]; s[18] = st[3];
            out[inst * 6 + c] = (tin ? tin[inst * 6 + c] : 0.0) + M.cart_C[lane] * y;
        }
    }

    // 2. JointAdmittance::_update: lane = coordinate
    if (Bt.joint_qdot_out) {
        const bool dense = Bt.joint_C != nullptr;
        double y = 0.0;
        if (lane < nv) {
            double* s = state + 24 * M.n_cart + lane;          // u, ud, y, yd: nv doubles apart
            double st[4] = {s[0], s[nv], s[2 * nv], s[3 * nv]};
            y = feedback_filter_step(st, Bt.joint_h[inst * nv + lane] - Bt.joint_tau[inst * nv + lane], K.joint);
            s[0] = st[0]; s[nv] = st[1]; s[2 * nv] = st[2]; s[3 * nv] = st[3];
            ys[lane] = y;
        }
        if (dense) {
            for (int r = 0; r < nv; ++r) if (lane < nv) Cs[r * kFeedbackStageLd + lane] = Bt.joint_C[r * nv + lane];   // coalesced row loads
            wave_sync();
        }
        if (lane < nv) {
            double v;
            if (dense) {
                v = 0.0;
                for (int j = 0; j < nv; ++j) v = fma(Cs[lane * kFeedbackStageLd + j], ys[j], v);
            } else {
                v = M.joint_C_scalar * y;
            }
            if (M.floating_base && lane < 6) v = 0.0;
            Bt.joint_qdot_out[inst * nv + lane] = v;
        }
    }

    // 3. floating_base::IMU::_update: lane = column 0 .. 5
    if (Bt.imu_A && lane < 6) {
        const int ld = Bt.imu_A_ld ? Bt.imu_A_ld : 6;
        double* A = Bt.imu_A + inst * Bt.imu_A_stride;
        const double* J = Bt.imu_fb_J + inst * Bt.imu_fb_J_stride;
        for (int r = 0; r < 3; ++r) A[r * ld + lane] = 0.0;
        for (int r = 3; r < 6; ++r) A[r * ld + lane] = J[r * nv + lane];
    }
    if (Bt.imu_b && lane < 6) {
        double v = 0.0;
        if (lane >= 3) {
            const double* R = Bt.imu_pose + inst * 12 + 3 * (lane - 3);
            const double* w = Bt.imu_omega + inst * 3;
            v = (R[0] * w[0] + R[1] * w[1]) + R[2] * w[2];
        }
        Bt.imu_b[inst * Bt.imu_b_stride + lane] = v;
    }

    // 4. floating_base::Contact: b_out = b_in + lambda [p_d - p; -e_o]
    if (Bt.contact_b_out && lane < 6) {
        double e[6];
        feedback_contact_error(Bt.contact_pose + inst * 12, Bt.contact_pose_ref + inst * 12, e);
        double el = e[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) if (lane == i) el = e[i];
        Bt.contact_b_out[inst * Bt.contact_b_out_stride + lane] = Bt.contact_b_in[inst * Bt.contact_b_in_stride + lane] + M.contact_lambda * el;
    }

    // 5. tasks::velocity::CollisionAvoidance::_update: lane = column
    if (Bt.ca_A) {
        const int n = M.n, ld = Bt.ca_A_ld ? Bt.ca_A_ld : n;
        double* A = Bt.ca_A + inst * Bt.ca_A_stride;
        const double* J = Bt.ca_J + inst * Bt.ca_J_stride;
        const double* dist = Bt.ca_dist + inst * M.n_pairs;
        const int P = M.n_pairs, c0 = lane, c1 = lane + 64;
        // eight rows a trip: the destination may alias anything as far as the compiler knows, so a row-by-row loop is one memory
        // round trip per row; here the loads of a batch are all in flight before its first store
        for (int i0 = 0; i0 < P; i0 += 8) {
            double err[8], v0[8], v1[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = i0 + k;
                err[k] = 1.0; v0[k] = 0.0; v1[k] = 0.0;
                if (i < P) {
                    err[k] = dist[i] - M.ca_threshold;
                    if (c0 < n) v0[k] = J[i * n + c0];
                    if (c1 < n) v1[k] = J[i * n + c1];
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = i0 + k;
                if (i < P) {
                    if (c0 < n) A[i * ld + c0] = (err[k] > 0.0) ? 0.0 : -v0[k];
                    if (c1 < n) A[i * ld + c1] = (err[k] > 0.0) ? 0.0 : -v1[k];
                }
            }
        }
    }
    if (Bt.ca_b && lane < M.n_pairs) {
        const double err = Bt.ca_dist[inst * M.n_pairs + lane] - M.ca_threshold;
        Bt.ca_b[inst * Bt.ca_b_stride + lane] = (err > 0.0) ? 0.0 : err;
    }
}

}  // namespace osot
