// osot_mi355x.hip -- implementation of the C-ABI in include/osot_mi355x.h for gfx950 (MI355X).
//
// Host side: argument checking with the reference's error behaviour (size mismatches are refused like
// BackEnd::updateTask/updateConstraints do, src/solvers/BackEnd.cpp:19-93), translation of the static
// plan into kernel arguments, stream-ordered launches, hipEvent timing, RCCL all-gather.
// Device side: osot_kernels.h / osot_qp_core.h.  There is no CPU code path in this library.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "osot_host_plan.h"
#include "osot_kin.h"
#include "osot_dyn.h"
#include "osot_grad.h"
#include "osot_control.h"
#include "osot_ehqp.h"
#include "osot_id.h"
#include "osot_force.h"
#include "osot_feedback.h"
#include "osot_acc.h"
#include "osot_qp_sens.h"
#include "osot_qp_sens_big.h"
#include "osot_ihqp_sens.h"
#include "osot_ihqp_sens_wide.h"
#include "osot_nhqp_host.h"
#include "osot_admm.h"
#include "osot_qp_big.h"
#include "osot_cascade_wide.h"

using namespace osot;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(OSOT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

// Every entry point that touches a device runs under this guard: the calling thread's current device is saved, the
// object's device made current, and the caller's restored on the way out (several solvers on different GPUs may live
// in one process; the caller's current device is never changed).
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) ok = (hipSetDevice(device) == hipSuccess);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

template <class K>
int ensure_lds(K kernel, size_t bytes) {
    if (bytes > 160 * 1024) return fail(OSOT_ERR_UNSUPPORTED, "problem does not fit the 160 KiB LDS of a CU");
    if (bytes > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return OSOT_OK;
}

}  // namespace

// calls f with the padded size of the cascade instantiation as a compile-time constant (make_dev_plan picks it: 32, 56 or 64)
template <typename F>
static inline auto by_np(int T, F&& f) {
#ifdef OSOT_ONLY_NP32      // developer builds (tools/build_variant.sh NAME -DOSOT_ONLY_NP32): the 32-lane instantiations only -- a fifth of the
    (void)T;               // compile time for A/B runs of the headline kernel; every other layout would run THIS one: never shipped
    return f(std::integral_constant<int, 32>{});
#endif
    if (T == 32) return f(std::integral_constant<int, 32>{});
    if (T == 40) return f(std::integral_constant<int, 40>{});
    if (T == 56) return f(std::integral_constant<int, 56>{});
    return f(std::integral_constant<int, 64>{});
}

// calls f with the instantiation of variant v (osot_host_plan.h: choose_kernel_variant, kernel_variants) at padded size NP: the one place
// that names them, for the launch, the dynamic-LDS attribute and the occupancy query alike.  (In the order the code object holds them.)
template <int NP, class F>
static int with_ihqp_kernel(const KernelVariant& v, F&& f) {
    if (v == cascade_variant(false)) return f(osot_cascade_kernel<NP, false>);
    if (v == cascade_variant(true)) return f(osot_cascade_kernel<NP, true>);
    if (v == cycle_variant(false)) return f(osot_cycle_kernel<NP, false>);
    if (v == cycle_variant(true)) return f(osot_cycle_kernel<NP, true>);
    if (v == cascade_variant(false, true)) return f(osot_cascade_kernel<NP, false, true>);
    if (v == cascade_variant(false, false, true)) return f(osot_cascade_kernel<NP, false, false, true>);
    if (v == cycle_variant(false, true)) return f(osot_cycle_kernel<NP, false, true>);
    if (v == control_variant(false, true)) return f(osot_control_cycle_kernel<NP, false, true>);
    if (v == control_variant(false, true, true)) return f(osot_control_cycle_kernel<NP, false, true, true>);
    if (v == control_variant(false, false)) return f(osot_control_cycle_kernel<NP, false, false>);
    if (v == control_variant(false, false, true)) return f(osot_control_cycle_kernel<NP, false, false, true>);
    if (v == control_variant(true, false)) return f(osot_control_cycle_kernel<NP, true, false>);
    if (v == control_variant(true, false, true)) return f(osot_control_cycle_kernel<NP, true, false, true>);
    if constexpr (NP == 32) if (v == cascade_variant(true, false, true)) return f(osot_cascade_kernel<32, true, false, true>);
    return fail(OSOT_ERR_UNSUPPORTED, "no kernel instantiation for this variant and lane layout");
}

// calls f(kernel, its dynamic LDS bytes) with the preparation kernel of an nHQP level of m rows and nf free variables among n
template <class F>
static int with_nhqp_prepare_kernel(int m, int nf, int n, F&& f) {
    if (nhqp_level_is_wide(m, nf)) return f(osot_nhqp_prepare_wide_kernel, nhqp_prepare_wide_lds_bytes(m, n));   // min(rows, free variables) > 32: the full column-side Gram matrix (sym_eig_wide)
    if (n > 32)     // 33 .. 64 variables: the 64-column kernel (dynamic LDS beyond the 64 KB default: raised once per solver)
        return m <= 32 ? f(osot_nhqp_prepare64_kernel<32>, nhqp_prepare64_lds_bytes(32, n)) : f(osot_nhqp_prepare64_kernel<64>, nhqp_prepare64_lds_bytes(64, n));
    return m <= 32 ? f(osot_nhqp_prepare_kernel<32>, (size_t)0) : f(osot_nhqp_prepare_kernel<64>, (size_t)0);
}

struct osot_solver {
    osot_plan_desc plan;
    int max_batch;
    int device;
    bool timing;
    int timing_stride = 1, timing_count = 0;   // every timing_stride-th launch is bracketed by events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;   // recorded, not yet accumulated
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    // longest-first dispatch (order_body in osot_kernels.h): cost estimates of the previous solves and the order built from them
    int schedule = 1;        // 0: in order, 1: longest first
    int* d_cost = nullptr;   // [2][max_batch]: the launches alternate (read one, write the other)
    int* d_order = nullptr;  // [2][max_batch]: likewise (use one, the launch's order workgroup fills the other)
    int flip = 0;            // which halves the next launch writes
    int order_B = -1;        // batch size the order the next launch reads is valid for (-1: none yet)
    // d_cost / d_order are stream-ordered state shared by consecutive solves.  A solver is meant to be driven from one
    // thread on one stream (like the reference's Solver: no locks, SURVEY 8b "threading"); a solve that arrives on a
    // DIFFERENT stream than the previous one first waits (host side, rare) for that stream, so that it never reads
    // d_order while the previous launch's order workgroup is still writing it.  No event traffic on the common path.
    hipStream_t order_stream = nullptr;
    DevUpdatePlan* d_uplan = nullptr;   // static part of the update kernel's arguments, uploaded at creation
    DevUpdatePlan h_uplan;
    unsigned char task_active[OSOT_MAX_LEVELS * OSOT_MAX_TASKS];   // Task::setActive flags
    bool any_inactive = false;
    int slots = 1;      // wavefronts of the cascade kernel the device holds at once (CUs x resident workgroups per CU)
    NhqpWorkspace nhqp; // scratch of the null-space front-end, allocated at its first use
    bool nhqp_ready = false;
    bool nhqp_lds_ready = false;
    // hot start (osot_solver_set_hotstart): the inequality working set each level of each instance ended with
    double* d_rows = nullptr;   // [max_batch][rows_doubles] row tables (plans whose 64-lane kernels keep them out of LDS)
    int hotstart = 0;
    int specialise = 1;         // osot_solver_set_specialisation: the BOX instantiation for plans without constraint rows
    int* d_hot = nullptr;    // [max_batch][n_levels][T] constraint codes, -1 = none (allocated when first switched on)
    int hot_T = 0;
    // the workgroup route (osot_solver_create_wide, osot_cascade_wide.h): one 256-thread workgroup per instance
    int wide = 0;
    double* d_work = nullptr;   // [wide_grid][2][n][n]: L and J of every resident workgroup, allocated once
    int wide_grid = 0;          // workgroups of a launch: the resident ones, at most max_batch
    int wide_grid_hot = 0;      // the same for osot_cascade_wide_hot_kernel (by its own occupancy; never more than wide_grid: the workspace)
    size_t wide_lds = 0;
};

// entries that the workgroup route does not carry
static int refuse_wide(const osot_solver* s, const char* what) {
    if (s && s->wide) return fail(OSOT_ERR_UNSUPPORTED, std::string(what) + " is not available on the wide route (osot_solver_create_wide)");
    return OSOT_OK;
}

extern "C" {

const char* osot_version(void) { return "osot-mi355x 0.1 (gfx950)"; }
const char* osot_last_error(void) { return g_err.c_str(); }

int osot_abi_layout(const char* name, unsigned long long* size, unsigned long long* offsets, int max_fields, int* n_fields) {
    if (!name || !size) return fail(OSOT_ERR_INVALID, "null name/size");
    std::vector<unsigned long long> off;
    unsigned long long sz = 0;
    const std::string nm(name);
#define OSOT_LAYOUT_BEGIN(T) if (nm == #T) { typedef T osot_layout_t; sz = sizeof(T);
#define OSOT_F(f) off.push_back((unsigned long long)offsetof(osot_layout_t, f));
#define OSOT_LAYOUT_END() }
    OSOT_LAYOUT_BEGIN(osot_task_desc) OSOT_F(kind) OSOT_F(rows) OSOT_F(weight) OSOT_F(lambda) OSOT_F(orientation_gain) OSOT_F(lambda2)
        OSOT_F(row_mask) OSOT_F(parent_rows) OSOT_F(sub_lambda) OSOT_F(body_frame) OSOT_F(dense_weight) OSOT_F(acc_gain_matrices) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_level_desc) OSOT_F(n_tasks) OSOT_F(task) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_bound_desc) OSOT_F(kind) OSOT_F(scaling) OSOT_F(dT) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_rows_desc) OSOT_F(kind) OSOT_F(rows) OSOT_F(d_threshold) OSOT_F(detection_threshold) OSOT_F(bound_scaling)
        OSOT_F(first_col) OSOT_F(dT) OSOT_F(p) OSOT_F(mu) OSOT_F(task_lambda) OSOT_F(task_orientation_gain) OSOT_F(err_lb) OSOT_F(err_ub)
        OSOT_F(task_body_frame) OSOT_F(n_candidates) OSOT_F(only_level) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_plan_desc) OSOT_F(n) OSOT_F(n_levels) OSOT_F(level) OSOT_F(n_bounds) OSOT_F(bound) OSOT_F(n_rowblocks)
        OSOT_F(rowblock) OSOT_F(eps_abs) OSOT_F(max_iter) OSOT_F(has_regularisation) OSOT_F(regularisation) OSOT_F(regularisation_dense) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_qp_batch) OSOT_F(B) OSOT_F(A) OSOT_F(b) OSOT_F(w) OSOT_F(c) OSOT_F(C) OSOT_F(lo) OSOT_F(up) OSOT_F(l) OSOT_F(u)
        OSOT_F(level_active) OSOT_F(dq) OSOT_F(x_levels) OSOT_F(status) OSOT_F(iterations) OSOT_F(b_reg) OSOT_F(WA) OSOT_F(Wb)
        OSOT_F(accepted_slack) OSOT_F(A_reg) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_leaf_ptrs) OSOT_F(p0) OSOT_F(p1) OSOT_F(p2) OSOT_F(W) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_leaf_batch) OSOT_F(B) OSOT_F(task) OSOT_F(bound) OSOT_F(rows) OSOT_F(regularisation) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_assembled_out) OSOT_F(b) OSOT_F(w) OSOT_F(C) OSOT_F(lo) OSOT_F(up) OSOT_F(l) OSOT_F(u) OSOT_F(b_reg) OSOT_F(WA)
        OSOT_F(Wb) OSOT_F(A) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_backend_options) OSOT_F(max_iterations) OSOT_F(last_iterations) OSOT_F(last_status) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_nhqp_options) OSOT_F(free_vars) OSOT_F(min_sv_ratio) OSOT_F(no_ab_regularization)
        OSOT_F(no_selective_ns_regularization) OSOT_F(min_sv_ratio_is_set) OSOT_F(level_no_ab_regularization)
        OSOT_F(level_no_selective_ns_regularization) OSOT_F(level_min_sv_ratio_is_set) OSOT_F(level_min_sv_ratio) OSOT_F(level_W) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_admm_options) OSOT_F(eps_abs) OSOT_F(eps_rel) OSOT_F(rho) OSOT_F(sigma) OSOT_F(alpha) OSOT_F(max_iter)
        OSOT_F(scaling) OSOT_F(check_every) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_id_model) OSOT_F(B) OSOT_F(nv) OSOT_F(n_contacts) OSOT_F(contact_dim) OSOT_F(Bm) OSOT_F(h) OSOT_F(Jc)
        OSOT_F(floating_base) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_kin_desc) OSOT_F(n) OSOT_F(parent) OSOT_F(type) OSOT_F(axis) OSOT_F(R0) OSOT_F(p0) OSOT_F(mass) OSOT_F(com)
        OSOT_F(n_frames) OSOT_F(frame_joint) OSOT_F(frame_R) OSOT_F(frame_p) OSOT_F(n_pairs) OSOT_F(pair_joint) OSOT_F(pair_seg)
        OSOT_F(pair_radius) OSOT_F(frame_body) OSOT_F(frame_col_mask) OSOT_F(com_col_mask) OSOT_F(pair_kind) OSOT_F(pair_env)
        OSOT_F(pair_box) OSOT_F(pair_shape_R) OSOT_F(pair_shape_p) OSOT_F(n_env) OSOT_F(frame_base)
        OSOT_F(pair_kind_a) OSOT_F(pair_size_a) OSOT_F(pair_shape_R_a) OSOT_F(pair_shape_p_a) OSOT_F(pair_hull) OSOT_F(n_hull_vertices)
        OSOT_F(hull_vertex) OSOT_F(n_rowsets) OSOT_F(rowset_kind) OSOT_F(rowset_frame) OSOT_F(rowset_row_mask) OSOT_F(rowset_split)
        OSOT_F(rowset_wheel) OSOT_F(rowset_param) OSOT_F(n_gaze) OSOT_F(gaze_frame) OSOT_F(n_points) OSOT_F(point_joint) OSOT_F(point_p) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_kin_batch) OSOT_F(B) OSOT_F(q) OSOT_F(frame_pose) OSOT_F(frame_J) OSOT_F(frame_J_stride) OSOT_F(com)
        OSOT_F(com_J) OSOT_F(com_J_stride) OSOT_F(pair_dist) OSOT_F(pair_J) OSOT_F(pair_J_stride) OSOT_F(env_pose) OSOT_F(env_pose_stride)
        OSOT_F(pair_points) OSOT_F(rowset_A) OSOT_F(rowset_A_stride) OSOT_F(rowset_b) OSOT_F(rowset_b_stride)
        OSOT_F(rowset_qdot) OSOT_F(gaze_point) OSOT_F(gaze_ref) OSOT_F(points) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_shape) OSOT_F(kind) OSOT_F(size) OSOT_F(radius) OSOT_F(n_vertices) OSOT_F(vertices) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_dyn_desc) OSOT_F(inertia) OSOT_F(gravity) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_dyn_batch) OSOT_F(B) OSOT_F(q) OSOT_F(qdot) OSOT_F(M) OSOT_F(M_stride) OSOT_F(h) OSOT_F(frame_Jdot_qdot)
        OSOT_F(frame_Jdot_qdot_stride) OSOT_F(com_Jdot_qdot) OSOT_F(com_Jdot_qdot_stride) OSOT_F(cmm_lin) OSOT_F(cmm_lin_stride)
        OSOT_F(cmm_lin_ld) OSOT_F(cmm_ang) OSOT_F(cmm_ang_stride) OSOT_F(cmm_ang_ld) OSOT_F(momentum) OSOT_F(momentum_stride)
        OSOT_F(ang_mom_b) OSOT_F(ang_mom_b_stride) OSOT_F(ang_mom_ref) OSOT_F(ang_mom_rate_ref) OSOT_F(ang_mom_gain)
        OSOT_F(ang_mom_lambda) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_grad_desc) OSOT_F(n_terms) OSOT_F(kind) OSOT_F(frame) OSOT_F(step) OSOT_F(lambda) OSOT_F(joint_mask)
        OSOT_F(W_diag) OSOT_F(gravity) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_grad_batch) OSOT_F(B) OSOT_F(q) OSOT_F(b) OSOT_F(b_stride) OSOT_F(value) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_force_model) OSOT_F(n_contacts) OSOT_F(nv) OSOT_F(n) OSOT_F(wrench_col) OSOT_F(torque_col) OSOT_F(cart_contact)
        OSOT_F(mass) OSOT_F(gravity) OSOT_F(com_lambda) OSOT_F(com_lambda2) OSOT_F(com_lambda_ang) OSOT_F(cart_Kp) OSOT_F(cart_Kd) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_force_batch) OSOT_F(B) OSOT_F(pose) OSOT_F(Jc) OSOT_F(com) OSOT_F(momentum) OSOT_F(h_gravity) OSOT_F(qdot)
        OSOT_F(enabled) OSOT_F(com_A) OSOT_F(com_A_stride) OSOT_F(com_A_ld) OSOT_F(com_b) OSOT_F(com_b_stride) OSOT_F(com_pos_ref)
        OSOT_F(com_vel_ref) OSOT_F(com_acc_ref) OSOT_F(ang_mom_ref) OSOT_F(ang_mom_rate_ref) OSOT_F(fb_A) OSOT_F(fb_A_stride) OSOT_F(fb_A_ld)
        OSOT_F(static_A) OSOT_F(static_A_stride) OSOT_F(static_A_ld) OSOT_F(static_lo) OSOT_F(static_up) OSOT_F(static_b_stride)
        OSOT_F(static_q_tau) OSOT_F(cart_b) OSOT_F(cart_b_stride) OSOT_F(cart_pose_ref) OSOT_F(cart_vel_ref) OSOT_F(cart_f_des)
        OSOT_F(cart_pose_error) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_feedback_model) OSOT_F(nv) OSOT_F(floating_base) OSOT_F(n_cart) OSOT_F(joint) OSOT_F(imu) OSOT_F(n_pairs) OSOT_F(n)
        OSOT_F(cart_C) OSOT_F(cart_deadzone) OSOT_F(cart_omega) OSOT_F(cart_damping) OSOT_F(cart_ts) OSOT_F(joint_omega) OSOT_F(joint_damping)
        OSOT_F(joint_ts) OSOT_F(joint_C_scalar) OSOT_F(contact_lambda) OSOT_F(ca_threshold) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_feedback_batch) OSOT_F(B) OSOT_F(state) OSOT_F(cart_pose) OSOT_F(cart_wrench) OSOT_F(cart_wrench_ref)
        OSOT_F(cart_twist_in) OSOT_F(cart_twist_out) OSOT_F(joint_tau) OSOT_F(joint_h) OSOT_F(joint_C) OSOT_F(joint_qdot_out)
        OSOT_F(imu_fb_J) OSOT_F(imu_fb_J_stride) OSOT_F(imu_pose) OSOT_F(imu_omega) OSOT_F(imu_A) OSOT_F(imu_A_stride) OSOT_F(imu_A_ld)
        OSOT_F(imu_b) OSOT_F(imu_b_stride) OSOT_F(contact_pose) OSOT_F(contact_pose_ref) OSOT_F(contact_b_in) OSOT_F(contact_b_in_stride)
        OSOT_F(contact_b_out) OSOT_F(contact_b_out_stride) OSOT_F(ca_J) OSOT_F(ca_J_stride) OSOT_F(ca_dist) OSOT_F(ca_A) OSOT_F(ca_A_stride)
        OSOT_F(ca_A_ld) OSOT_F(ca_b) OSOT_F(ca_b_stride) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_acc_model) OSOT_F(nv) OSOT_F(n_cart) OSOT_F(cart_gain_type) OSOT_F(cart_gain_matrices) OSOT_F(cart_Kp) OSOT_F(cart_Kd)
        OSOT_F(cart_orientation_gain) OSOT_F(has_com) OSOT_F(com_gain_matrices) OSOT_F(com_Kp) OSOT_F(com_Kd) OSOT_F(has_postural)
        OSOT_F(post_gain_type) OSOT_F(post_gain_matrices) OSOT_F(post_lambda) OSOT_F(post_lambda2) OSOT_F(post_Kp) OSOT_F(post_Kd) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_acc_batch) OSOT_F(B) OSOT_F(q) OSOT_F(qdot) OSOT_F(M) OSOT_F(M_stride) OSOT_F(cart_J) OSOT_F(cart_J_stride)
        OSOT_F(cart_J_ld) OSOT_F(cart_pose) OSOT_F(cart_pose_ref) OSOT_F(cart_vel_ref) OSOT_F(cart_f_virtual) OSOT_F(cart_a_ref_in)
        OSOT_F(cart_p0) OSOT_F(cart_p0_stride) OSOT_F(cart_a_ref_out) OSOT_F(cart_Mi) OSOT_F(com_J) OSOT_F(com_J_stride) OSOT_F(com_J_ld)
        OSOT_F(com) OSOT_F(com_ref) OSOT_F(com_vel_ref) OSOT_F(com_p0) OSOT_F(com_p0_stride) OSOT_F(post_q_ref) OSOT_F(post_qdot_ref)
        OSOT_F(post_qddot_ref) OSOT_F(post_p0) OSOT_F(post_qddot_out) OSOT_F(Minv) OSOT_F(Minv_stride) OSOT_F(ok) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_qp_sens_options) OSOT_F(active_tol) OSOT_F(dual_tol) OSOT_F(rank_tol) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_qp_sens_batch) OSOT_F(B) OSOT_F(n) OSOT_F(nc) OSOT_F(H) OSOT_F(g) OSOT_F(A) OSOT_F(lA) OSOT_F(uA) OSOT_F(l) OSOT_F(u)
        OSOT_F(eps_abs) OSOT_F(x) OSOT_F(status) OSOT_F(grad_x) OSOT_F(y) OSOT_F(active) OSOT_F(grad_H) OSOT_F(grad_g) OSOT_F(grad_A)
        OSOT_F(grad_lA) OSOT_F(grad_uA) OSOT_F(grad_l) OSOT_F(grad_u) OSOT_F(flag) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_level_qp) OSOT_F(H) OSOT_F(g) OSOT_F(A) OSOT_F(lA) OSOT_F(uA) OSOT_F(l) OSOT_F(u) OSOT_LAYOUT_END()
    OSOT_LAYOUT_BEGIN(osot_ihqp_sens_batch) OSOT_F(qp) OSOT_F(y) OSOT_F(active) OSOT_F(flag) OSOT_F(objective) OSOT_F(workspace)
        OSOT_F(workspace_bytes) OSOT_F(grad_dq) OSOT_F(grad_b) OSOT_F(grad_w) OSOT_F(grad_c) OSOT_F(grad_A) OSOT_F(grad_C) OSOT_F(grad_lo)
        OSOT_F(grad_up) OSOT_F(grad_l) OSOT_F(grad_u) OSOT_LAYOUT_END()
#undef OSOT_LAYOUT_BEGIN
#undef OSOT_F
#undef OSOT_LAYOUT_END
    if (sz == 0) return fail(OSOT_ERR_INVALID, std::string("osot_abi_layout: unknown struct ") + name);
    *size = sz;
    if (n_fields) *n_fields = (int)off.size();
    if (offsets) for (int i = 0; i < (int)off.size() && i < max_fields; ++i) offsets[i] = off[i];
    return OSOT_OK;
}

int osot_device_count(int* count) {
    if (!count) return fail(OSOT_ERR_INVALID, "null count");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; return fail(OSOT_ERR_HIP, hipGetErrorString(e)); }
    *count = c;
    return OSOT_OK;
}

int osot_plan_validate(const osot_plan_desc* plan) {
    const char* why;
    int rc = plan_validate(plan, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    return OSOT_OK;
}
int osot_plan_validate_wide(const osot_plan_desc* plan) {
    const char* why;
    int rc = plan_validate(plan, &why, 1);
    if (rc != OSOT_OK) return fail(rc, why);
    wide::Plan P;
    wide::make_plan(*plan, nullptr, nullptr, P);
    if (wide::shared_bytes(plan->n, P.nrows) > 160 * 1024)
        return fail(OSOT_ERR_UNSUPPORTED, "wide route: the row table of this plan does not fit the 160 KiB LDS of a CU");
    return OSOT_OK;
}
int osot_plan_level_rows(const osot_plan_desc* plan, int level, int* m_total, int* m_stored) {
    int rc = plan_level_rows(plan, level, m_total, m_stored);
    return rc == OSOT_OK ? rc : fail(rc, "bad plan/level");
}
int osot_plan_constraint_rows(const osot_plan_desc* plan, int* nc) {
    int rc = plan_constraint_rows(plan, nc);
    return rc == OSOT_OK ? rc : fail(rc, "bad plan");
}
int osot_plan_stored_constraint_rows(const osot_plan_desc* plan, int* nc_stored) {
    int rc = plan_stored_constraint_rows(plan, nc_stored);
    return rc == OSOT_OK ? rc : fail(rc, "bad plan");
}

}  // extern "C"

// what the two routes' constructors share: the handle with its plan and the host copy of the update plan ...
static osot_solver* solver_new(const osot_plan_desc& plan, int max_batch, int device) {
    osot_solver* s = new osot_solver();
    s->plan = plan;
    s->max_batch = max_batch;
    s->device = device;
    s->timing = false;
    std::memset(s->task_active, 1, sizeof(s->task_active));
    make_update_plan(plan, s->h_uplan);
    return s;
}
// ... and, after the route's own allocations (allocated: they succeeded), the update plan's upload.  The static update plan lives
// with the solver from the start (no lazy allocation on whatever device is current).  One clean-up path: osot_solver_destroy
static int solver_finish(osot_solver* s, bool allocated, osot_solver** out) {
    if (!allocated || hipMalloc(&s->d_uplan, sizeof(DevUpdatePlan)) != hipSuccess ||
        hipMemcpy(s->d_uplan, &s->h_uplan, sizeof(DevUpdatePlan), hipMemcpyHostToDevice) != hipSuccess) {
        osot_solver_destroy(s);
        return fail(OSOT_ERR_HIP, "device allocation for the solver failed");
    }
    *out = s;
    return OSOT_OK;
}

extern "C" {

int osot_solver_create(const osot_plan_desc* plan, int max_batch, int device, osot_solver** out) {
    if (!out) return fail(OSOT_ERR_INVALID, "null out");
    *out = nullptr;
    int rc = osot_plan_validate(plan);
    if (rc != OSOT_OK) return rc;
    if (max_batch < 1) return fail(OSOT_ERR_INVALID, "max_batch < 1");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    DevPlan P; int T; size_t lds;
    make_dev_plan(*plan, nullptr, P, T, lds);
    // every variant a launch can ask for goes through the mapping the launch uses: none is launchable without being prepared
    const size_t lds_control = lds > control_kin_lds_bytes(T) ? lds : control_kin_lds_bytes(T);
    KernelVariant all[kMaxKernelVariants];
    const int n_all = kernel_variants(T, all);
    rc = by_np(T, [&](auto np) {
        int r = OSOT_OK;
        for (int i = 0; i < n_all && r == OSOT_OK; ++i)
            r = with_ihqp_kernel<decltype(np)::value>(all[i], [&](auto kernel) { return ensure_lds(kernel, all[i].family == KERNEL_CONTROL ? lds_control : lds); });
        return r;
    });
    if (rc != OSOT_OK) return rc;
    osot_solver* s = solver_new(*plan, max_batch, device);
    {   // resident workgroups: what the longest-first dispatch order is planned for (order_body)
        int per_cu = 0, cus = 0;
        const int e1 = by_np(T, [&](auto np) {
            return with_ihqp_kernel<decltype(np)::value>(cycle_variant(), [&](auto kernel) { return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, lds); });
        });
        hipError_t e2 = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        s->slots = (e1 == hipSuccess && e2 == hipSuccess && per_cu > 0 && cus > 0) ? per_cu * cus : 2048;
    }
    if (P.rows_in_global && hipMalloc(&s->d_rows, sizeof(double) * (size_t)max_batch * (size_t)P.rows_doubles) != hipSuccess) {
        osot_solver_destroy(s);
        return fail(OSOT_ERR_HIP, "device allocation for the row tables failed");
    }
    // the dispatch-order state lives with the solver from the start too
    const bool allocated =
        hipMalloc(&s->d_cost, sizeof(int) * 2 * (size_t)max_batch) == hipSuccess &&
        hipMemset(s->d_cost, 0, sizeof(int) * 2 * (size_t)max_batch) == hipSuccess &&
        hipMalloc(&s->d_order, sizeof(int) * 2 * (size_t)max_batch) == hipSuccess &&
        [&] {   // both halves of the order buffer start as the identity permutation: a half that no launch has written yet
                // (a graph capture that failed half-way leaves the host-side flip ahead of the device) is still a valid order
            std::vector<int> id(2 * (size_t)max_batch);
            for (int i = 0; i < 2 * max_batch; ++i) id[i] = i % max_batch;
            return hipMemcpy(s->d_order, id.data(), sizeof(int) * id.size(), hipMemcpyHostToDevice) == hipSuccess;
        }();
    return solver_finish(s, allocated, out);
}

int osot_solver_create_wide(const osot_plan_desc* plan, int max_batch, int device, osot_solver** out) {
    if (!out) return fail(OSOT_ERR_INVALID, "null out");
    *out = nullptr;
    int rc = osot_plan_validate_wide(plan);
    if (rc != OSOT_OK) return rc;
    if (max_batch < 1) return fail(OSOT_ERR_INVALID, "max_batch < 1");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    wide::Plan P;
    wide::make_plan(*plan, nullptr, nullptr, P);
    const size_t lds = wide::shared_bytes(P.n, P.nrows);
    rc = ensure_lds(osot_cascade_wide_kernel, lds);
    if (rc != OSOT_OK) return rc;
    int per_cu = 0, cus = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, osot_cascade_wide_kernel, 256, lds));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (per_cu < 1 || cus < 1) return fail(OSOT_ERR_UNSUPPORTED, "the wide cascade kernel does not fit a CU for this plan");
    // the hot kernel (osot_ihqp_solve_hot / osot_cycle_hot): same LDS, its own occupancy
    rc = ensure_lds(osot_cascade_wide_hot_kernel, lds);
    if (rc != OSOT_OK) return rc;
    int per_cu_hot = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_hot, osot_cascade_wide_hot_kernel, 256, lds));
    if (per_cu_hot < 1) return fail(OSOT_ERR_UNSUPPORTED, "the wide cascade kernel does not fit a CU for this plan");
    osot_solver* s = solver_new(*plan, max_batch, device);
    s->wide = 1;
    s->wide_lds = lds;
    s->slots = per_cu * cus;
    s->wide_grid = max_batch < s->slots ? max_batch : s->slots;
    s->wide_grid_hot = per_cu_hot * cus < s->wide_grid ? per_cu_hot * cus : s->wide_grid;
    return solver_finish(s, hipMalloc(&s->d_work, sizeof(double) * 2 * (size_t)P.n * P.n * (size_t)s->wide_grid) == hipSuccess, out);
}

int osot_solver_destroy(osot_solver* s) {
    if (!s) return OSOT_OK;
    DeviceGuard guard(s->device);
    if (s->d_work) hipFree(s->d_work);
    for (auto& p : s->events) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    for (auto& p : s->pool) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    if (s->d_cost) hipFree(s->d_cost);
    if (s->d_order) hipFree(s->d_order);
    if (s->d_uplan) hipFree(s->d_uplan);
    if (s->d_hot) hipFree(s->d_hot);
    if (s->d_rows) hipFree(s->d_rows);
    if (s->nhqp_ready) {
        void* ptrs[] = {s->nhqp.N[0], s->nhqp.N[1], s->nhqp.q0, s->nhqp.H, s->nhqp.g, s->nhqp.R, s->nhqp.rlo, s->nhqp.rup, s->nhqp.z,
                        s->nhqp.V2, s->nhqp.qp_status, s->nhqp.qp_iters};
        for (void* q : ptrs) if (q) hipFree(q);
    }
    delete s;
    return OSOT_OK;
}

int osot_solver_set_schedule(osot_solver* s, int mode) {
    if (!s) return fail(OSOT_ERR_INVALID, "null solver");
    if (mode != OSOT_SCHEDULE_IN_ORDER && mode != OSOT_SCHEDULE_LONGEST_FIRST) return fail(OSOT_ERR_INVALID, "unknown schedule mode");
    s->schedule = mode;
    s->order_B = -1;
    return OSOT_OK;
}

int osot_solver_set_specialisation(osot_solver* s, int enabled) {
    if (!s) return fail(OSOT_ERR_INVALID, "null solver");
    s->specialise = enabled ? 1 : 0;
    return OSOT_OK;
}

int osot_solver_set_hotstart(osot_solver* s, int enabled) {
    if (!s) return fail(OSOT_ERR_INVALID, "null solver");
    if (enabled && s->wide) return refuse_wide(s, "hot start");
    DeviceGuard guard(s->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    if (enabled) {
        DevPlan P; int T; size_t lds;
        make_dev_plan(s->plan, nullptr, P, T, lds);
        const size_t bytes = sizeof(int) * (size_t)s->max_batch * (size_t)s->plan.n_levels * (size_t)(T <= 32 ? 32 : 64);   // (WaveCtx::LW entries per level)
        if (!s->d_hot) {
            if (hipMalloc(&s->d_hot, bytes) != hipSuccess) { s->d_hot = nullptr; return fail(OSOT_ERR_HIP, "device allocation for the hot-start state failed"); }
            s->hot_T = T;
        }
        // (re-)enabling forgets what was recorded: every instance starts cold once.  Device-wide synchronous, like the
        // allocation: this is a configuration call, not part of a control cycle
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemset(s->d_hot, 0xff, bytes));
    }
    s->hotstart = enabled ? 1 : 0;
    return OSOT_OK;
}

int osot_solver_set_task_active(osot_solver* s, int level, int task, int active) {
    if (!s) return fail(OSOT_ERR_INVALID, "null solver");
    if (level < 0 || level >= s->plan.n_levels || task < 0 || task >= s->plan.level[level].n_tasks)
        return fail(OSOT_ERR_INVALID, "no such task");
    s->task_active[level * OSOT_MAX_TASKS + task] = active ? 1 : 0;
    s->any_inactive = false;
    for (int k = 0; k < s->plan.n_levels; ++k)
        for (int j = 0; j < s->plan.level[k].n_tasks; ++j)
            if (!s->task_active[k * OSOT_MAX_TASKS + j]) s->any_inactive = true;
    return OSOT_OK;
}

int osot_solver_set_timing(osot_solver* s, int enabled) {
    if (!s) return fail(OSOT_ERR_INVALID, "null solver");
    s->timing = enabled != 0;
    s->timing_stride = enabled > 1 ? enabled : 1;
    s->timing_count = 0;
    if (s->timing) {   // the event pairs exist before the first timed launch: creating them costs more than recording them
        DeviceGuard guard(s->device);
        if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
        while (s->pool.size() < 64) {
            std::pair<hipEvent_t, hipEvent_t> ev;
            HIP_TRY(hipEventCreate(&ev.first));
            HIP_TRY(hipEventCreate(&ev.second));
            s->pool.push_back(ev);
        }
    }
    return OSOT_OK;
}

int osot_ehqp_solve(osot_solver* s, const osot_qp_batch* b, double sigma_min, void* hip_stream) {
    if (!s || !b) return fail(OSOT_ERR_INVALID, "null solver/batch");
    if (s->wide) return refuse_wide(s, "the eHQP front-end");
    if (b->B < 0 || b->B > s->max_batch) return fail(OSOT_ERR_INVALID, "batch size exceeds max_batch");
    if (b->B == 0) return OSOT_OK;
    if (const char* w = outputs_missing(*b)) return fail(OSOT_ERR_INVALID, w);
    const osot_plan_desc& pl = s->plan;
    DevEhqp Q;
    const char* why = "";
    int rc = ehqp_args(pl, b, sigma_min, s->any_inactive ? s->task_active : nullptr, Q, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    DeviceGuard guard(s->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    if (Q.use_qr) {
        const int NPq = Q.n <= 32 ? 32 : 64;
        const size_t lds = ehqp_qr_lds_bytes(NPq, Q.rows8);
        rc = NPq == 32 ? ensure_lds(osot_ehqp_qr_kernel<32>, lds) : ensure_lds(osot_ehqp_qr_kernel<64>, lds);
        if (rc != OSOT_OK) return rc;
        if (NPq == 32) hipLaunchKernelGGL(osot_ehqp_qr_kernel<32>, dim3((unsigned)b->B), dim3(64), lds, (hipStream_t)hip_stream, Q);
        else hipLaunchKernelGGL(osot_ehqp_qr_kernel<64>, dim3((unsigned)b->B), dim3(64), lds, (hipStream_t)hip_stream, Q);
    } else {
        hipLaunchKernelGGL(osot_ehqp_kernel, dim3((unsigned)b->B), dim3(64), 0, (hipStream_t)hip_stream, Q);
    }
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

int osot_nhqp_solve(osot_solver* s, const osot_qp_batch* b, const osot_nhqp_options* opt, void* hip_stream) {
    if (!s || !b) return fail(OSOT_ERR_INVALID, "null solver/batch");
    if (s->wide) return refuse_wide(s, "the nHQP front-end");
    if (b->B < 0 || b->B > s->max_batch) return fail(OSOT_ERR_INVALID, "batch size exceeds max_batch");
    if (b->B == 0) return OSOT_OK;
    if (const char* w = outputs_missing(*b)) return fail(OSOT_ERR_INVALID, w);
    DeviceGuard guard(s->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    const osot_plan_desc& pl = s->plan;
    if (b->level_active)     // (iHQP::setActiveStack: the reference's nHQP has no such switch, nHQP.h)
        for (int k = 0; k < pl.n_levels; ++k)
            if (!b->level_active[k]) return fail(OSOT_ERR_UNSUPPORTED, "nHQP front-end: level_active is iHQP's setActiveStack; nHQP has no such switch");
    {
        int fv[OSOT_MAX_LEVELS]; const char* why = "";
        int rc = nhqp_validate(pl, opt, fv, &why);
        if (rc != OSOT_OK) return fail(rc, why);
        for (int k = 0; k < pl.n_levels; ++k) {
            int m, ma; plan_level_rows(&pl, k, &m, &ma);
            if (const char* w = level_ptrs_missing(*b, k, ma, false)) return fail(OSOT_ERR_INVALID, w);
        }
        int nc = 0; plan_constraint_rows(&pl, &nc);
        if (nc > 0 && (!b->C || !b->lo || !b->up)) return fail(OSOT_ERR_INVALID, "plan has constraint rows but C/lo/up is null");
        if (const char* w = bounds_missing(pl, *b)) return fail(OSOT_ERR_INVALID, w);
    }
    if (!s->nhqp_ready) {
        const NhqpSizes z = nhqp_sizes(pl, s->max_batch);
        NhqpWorkspace& w = s->nhqp;
        std::memset(&w, 0, sizeof(w));
        auto dm = [](double** p, size_t cnt) { return hipMalloc((void**)p, sizeof(double) * (cnt ? cnt : 1)) == hipSuccess; };
        bool ok = dm(&w.N[0], z.N) && dm(&w.N[1], z.N) && dm(&w.q0, z.q0) && dm(&w.H, z.H) && dm(&w.g, z.g) && dm(&w.R, z.R) &&
                  dm(&w.rlo, z.rl) && dm(&w.rup, z.rl) && dm(&w.z, z.z) && dm(&w.V2, z.V2) &&
                  hipMalloc((void**)&w.qp_status, sizeof(int) * z.st) == hipSuccess && hipMalloc((void**)&w.qp_iters, sizeof(int) * z.st) == hipSuccess;
        if (!ok) return fail(OSOT_ERR_HIP, "device allocation for the nHQP workspace failed");
        s->nhqp_ready = true;
    }
    if (pl.n > 32) {    // the 64-column preparation kernels' dynamic LDS, once per solver and with its error reported (a
                        // failed attribute call used to skip the launch silently and the solve went on with a stale workspace)
        if (!s->nhqp_lds_ready) {
            const int m_nf[3][2] = {{32, 32}, {64, 32}, {64, 64}};   // the 64-column kernel of either row count and the wide kernel, at their largest
            for (const auto& c : m_nf)
                if (const int r = with_nhqp_prepare_kernel(c[0], c[1], pl.n, [](auto kernel, size_t lds) { return ensure_lds(kernel, lds); })) return r;
            s->nhqp_lds_ready = true;
        }
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const unsigned grid = (unsigned)b->B;
    const char* why = "";
    int rc = nhqp_run(pl, b, opt, s->nhqp,
        [&](const DevNhqp& Q) {
            with_nhqp_prepare_kernel(Q.m, Q.nf, Q.n, [&](auto kernel, size_t lds) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, st, Q); return 0; });
        },
        [&](int B, int n, int nc, const double* H, const double* g, const double* A, const double* lA, const double* uA,
            const double* l, const double* u, double eps, double* x, int* status, int* iters) {
            return osot_qp_solve_batch(B, n, nc, H, g, A, lA, uA, l, u, eps, 0, x, status, iters, hip_stream);
        },
        [&](const DevNhqpAcc& A) { hipLaunchKernelGGL(osot_nhqp_accumulate_kernel, dim3(grid), dim3(64), 0, st, A); }, &why,
        s->any_inactive ? s->task_active : nullptr);
    if (rc != OSOT_OK) return fail(rc, why);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

int osot_solver_resident_waves(osot_solver* s, int* waves) {
    if (!s || !waves) return fail(OSOT_ERR_INVALID, "null argument");
    *waves = s->slots;
    return OSOT_OK;
}

// the same for the null-space front-end: its level-preparation kernels are what a solve's time goes to, and the one with the fewest
// resident wavefronts sets the round (static 25 KB of LDS at n <= 32: six per CU; the 64-column and wide kernels by the plan's sizes)
int osot_solver_resident_waves_nhqp(osot_solver* s, const osot_nhqp_options* opt, int* waves) {
    if (!s || !waves) return fail(OSOT_ERR_INVALID, "null argument");
    if (s->wide) return refuse_wide(s, "the nHQP front-end");
    DeviceGuard guard(s->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    const osot_plan_desc& pl = s->plan;
    int fv[OSOT_MAX_LEVELS]; const char* why = "";
    int rc = nhqp_validate(pl, opt, fv, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
    int least = 1 << 30;
    for (int k = 0; k < pl.n_levels; ++k) {
        int m, ma; plan_level_rows(&pl, k, &m, &ma);
        int per_cu = 0;
        const int e = with_nhqp_prepare_kernel(m, fv[k], pl.n, [&](auto kernel, size_t lds) { return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, lds); });
        if (e != hipSuccess || per_cu < 1) return fail(OSOT_ERR_HIP, "occupancy query of a preparation kernel failed");
        if (per_cu * cus < least) least = per_cu * cus;
    }
    *waves = least;
    return OSOT_OK;
}

int osot_solver_kernel_time_ms(osot_solver* s, int reset, double* avg_ms, int* launches) {
    if (!s) return fail(OSOT_ERR_INVALID, "null solver");
    double total = 0.0;
    int cnt = 0;
    for (auto& p : s->events) {
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        total += ms;
        cnt++;
    }
    if (avg_ms) *avg_ms = cnt ? total / cnt : 0.0;
    if (launches) *launches = cnt;
    if (reset) {
        for (auto& p : s->events) s->pool.push_back(p);
        s->events.clear();
    }
    return OSOT_OK;
}

// wide_hot: the caller's hot-start state of osot_ihqp_solve_hot / osot_cycle_hot (wide handles only)
static int ihqp_launch(osot_solver* s, const osot_qp_batch* b, void* hip_stream, long long* prof, const DevUpdate* fused = nullptr,
                       const DevControl* control = nullptr, int* wide_hot = nullptr);

int osot_ihqp_solve(osot_solver* s, const osot_qp_batch* b, void* hip_stream) {
    return ihqp_launch(s, b, hip_stream, nullptr);
}

// osot_cycle and osot_cycle_hot: the update's arguments, then the launch (hot_state: wide handles only, null = cold)
static int cycle_impl(osot_solver* s, const osot_leaf_batch* leaf, const osot_assembled_out* out, const osot_qp_batch* b,
                      int* hot_state, void* hip_stream) {
    if (!s || !leaf || !out || !b) return fail(OSOT_ERR_INVALID, "null argument");
    if (leaf->B != b->B) return fail(OSOT_ERR_INVALID, "leaf and batch disagree on B");
    if (leaf->B < 0 || leaf->B > s->max_batch) return fail(OSOT_ERR_INVALID, "batch size exceeds max_batch");
    if (leaf->B == 0) return OSOT_OK;
    DevUpdate U;
    const char* why = "";
    int rc = make_update_args(s->plan, s->h_uplan, leaf, out, s->d_uplan, U, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    // developer knob: OSOT_DEBUG_CYCLE_PROF=<device pointer, hex> receives [B][2] int64 cycle counts (update, cascade)
    static const char* dbg = getenv("OSOT_DEBUG_CYCLE_PROF");
    return ihqp_launch(s, b, hip_stream, dbg ? (long long*)strtoull(dbg, nullptr, 16) : nullptr, &U, nullptr, hot_state);
}

int osot_cycle(osot_solver* s, const osot_leaf_batch* leaf, const osot_assembled_out* out, const osot_qp_batch* b,
               void* hip_stream) {
    return cycle_impl(s, leaf, out, b, nullptr, hip_stream);
}

// the hot calls are the wide route's: the wavefront route keeps its state in the solver
static int refuse_wavefront_hot(const osot_solver* s, const char* what) {
    if (s && !s->wide) return fail(OSOT_ERR_UNSUPPORTED, std::string(what) + " takes a handle of osot_solver_create_wide; the wavefront route hot-starts through osot_solver_set_hotstart");
    return OSOT_OK;
}

int osot_solver_hot_state_ints(osot_solver* s, int* ints_per_instance) {
    if (!s || !ints_per_instance) return fail(OSOT_ERR_INVALID, "null argument");
    if (const int r = refuse_wavefront_hot(s, "osot_solver_hot_state_ints")) return r;
    *ints_per_instance = s->plan.n_levels * big::kHotLen;
    return OSOT_OK;
}

int osot_ihqp_solve_hot(osot_solver* s, const osot_qp_batch* b, int* hot_state, void* hip_stream) {
    if (const int r = refuse_wavefront_hot(s, "osot_ihqp_solve_hot")) return r;
    return ihqp_launch(s, b, hip_stream, nullptr, nullptr, nullptr, hot_state);
}

int osot_cycle_hot(osot_solver* s, const osot_leaf_batch* leaf, const osot_assembled_out* out, const osot_qp_batch* b,
                   int* hot_state, void* hip_stream) {
    if (const int r = refuse_wavefront_hot(s, "osot_cycle_hot")) return r;
    return cycle_impl(s, leaf, out, b, hot_state, hip_stream);
}

int osot_solver_profile_phases(osot_solver* s, const osot_qp_batch* b, long long* cycles, void* hip_stream) {
    if (!cycles) return fail(OSOT_ERR_INVALID, "null cycles");
    if (s && s->wide) return refuse_wide(s, "phase profiling");
    return ihqp_launch(s, b, hip_stream, cycles);
}

// the event bracket of a timed launch (osot_solver_set_timing: every timing_stride-th one): timed_begin takes a pair from the pool
// and records its first event, timed_end records the second and queues the pair for osot_solver_kernel_time_ms.  timed_begin
// comes after the LAST early return of a launch function
struct TimedLaunch { bool timed = false; std::pair<hipEvent_t, hipEvent_t> ev; };
static int timed_begin(osot_solver* s, hipStream_t st, TimedLaunch& t) {
    t.timed = s->timing && (s->timing_count++ % s->timing_stride) == 0;
    if (!t.timed) return OSOT_OK;
    if (!s->pool.empty()) { t.ev = s->pool.back(); s->pool.pop_back(); }
    else { HIP_TRY(hipEventCreate(&t.ev.first)); HIP_TRY(hipEventCreate(&t.ev.second)); }
    HIP_TRY(hipEventRecord(t.ev.first, st));
    return OSOT_OK;
}
static int timed_end(osot_solver* s, hipStream_t st, const TimedLaunch& t) {
    if (!t.timed) return OSOT_OK;
    HIP_TRY(hipEventRecord(t.ev.second, st));
    s->events.push_back(t.ev);
    return OSOT_OK;
}

// the workgroup route: osot_ihqp_solve, and osot_cycle as TWO launches on the stream (osot_update_kernel, then the cascade)
// hot: [B][n_levels][big::kHotLen] device ints of the caller (osot_ihqp_solve_hot) -> the hot kernel; null -> the cold one
static int wide_launch(osot_solver* s, const osot_qp_batch* b, void* hip_stream, long long* prof, const DevUpdate* fused, const DevControl* control, int* hot) {
    if (prof) return refuse_wide(s, "phase profiling");
    if (control) return refuse_wide(s, "the fused control cycle / rollout");
    const osot_plan_desc& pl = s->plan;
    wide::Plan P;
    wide::make_plan(pl, b->level_active, s->any_inactive ? s->task_active : nullptr, P);
    wide::Batch D;
    std::memset(&D, 0, sizeof(D));
    const char* why = "";
    const int rc = fill_batch_ptrs(pl, P, *b, D, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    D.work = s->d_work;
    hipStream_t st = (hipStream_t)hip_stream;
    if (fused) {
        hipLaunchKernelGGL(osot_update_kernel, dim3((unsigned)b->B), dim3(64), 0, st, *fused);
        HIP_TRY(hipGetLastError());
    }
    TimedLaunch tl;
    if (int r = timed_begin(s, st, tl)) return r;
    const int cap = hot ? s->wide_grid_hot : s->wide_grid;
    const unsigned grid = (unsigned)(b->B < cap ? b->B : cap);
    if (hot) hipLaunchKernelGGL(osot_cascade_wide_hot_kernel, dim3(grid), dim3(256), s->wide_lds, st, P, D, hot);
    else hipLaunchKernelGGL(osot_cascade_wide_kernel, dim3(grid), dim3(256), s->wide_lds, st, P, D);
    HIP_TRY(hipGetLastError());
    if (int r = timed_end(s, st, tl)) return r;
    return OSOT_OK;
}

// hipLaunchKernelGGL of the kernel that with_ihqp_kernel hands over, with its family's argument list
struct IhqpLaunch {
    unsigned grid; size_t lds; hipStream_t st; const DevPlan& P; const DevBatch& D; const DevUpdate* fused; const DevControl* control;
    int operator()(void (*k)(DevPlan, DevBatch)) const { hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, P, D); return OSOT_OK; }
    int operator()(void (*k)(DevUpdate, DevPlan, DevBatch)) const { hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, *fused, P, D); return OSOT_OK; }
    int operator()(void (*k)(DevUpdate, DevPlan, DevBatch, DevControl)) const { hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, st, *fused, P, D, *control); return OSOT_OK; }
};

static int ihqp_launch(osot_solver* s, const osot_qp_batch* b, void* hip_stream, long long* prof, const DevUpdate* fused, const DevControl* control, int* wide_hot) {
    if (!s || !b) return fail(OSOT_ERR_INVALID, "null solver/batch");
    if (b->B < 0 || b->B > s->max_batch) return fail(OSOT_ERR_INVALID, "batch size exceeds max_batch");
    if (b->B == 0) return OSOT_OK;   // empty batch: nothing to do
    DeviceGuard guard(s->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    if (s->wide) return wide_launch(s, b, hip_stream, prof, fused, control, wide_hot);
    const osot_plan_desc& pl = s->plan;
    DevPlan P; int T; size_t lds;
    make_dev_plan(pl, b->level_active, P, T, lds, s->any_inactive ? s->task_active : nullptr);
    {   // developer knob: extra dynamic LDS per wave (lowers the occupancy; used to measure how the kernel responds to it)
        static const char* extra = getenv("OSOT_DEBUG_EXTRA_LDS");
        if (extra) lds += (size_t)atoi(extra);
    }
    if (control && lds < control_kin_lds_bytes(T)) lds = control_kin_lds_bytes(T);
    DevBatch D;
    std::memset(&D, 0, sizeof(D));
    const char* why = "";
    const int rc = fill_batch_ptrs(pl, P, *b, D, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    D.prof = prof;
    D.hot = (s->hotstart && !prof) ? s->d_hot : nullptr;
    D.rows_scratch = s->d_rows;
    hipStream_t st = (hipStream_t)hip_stream;
    if (s->schedule == 1) {
        if (s->order_B >= 0 && s->order_stream != st) HIP_TRY(hipStreamSynchronize(s->order_stream));
        const size_t mb = (size_t)s->max_batch;
        D.order = (s->order_B == b->B) ? s->d_order + (size_t)(s->flip ^ 1) * mb : nullptr;
        D.cost_in = s->d_cost + (size_t)(s->flip ^ 1) * mb;
        D.cost_out = s->d_cost + (size_t)s->flip * mb;
        D.order_next = s->d_order + (size_t)s->flip * mb;
        D.slots = s->slots;
    }
    const unsigned grid = (unsigned)b->B + (D.order_next ? 1u : 0u);   // (+ the order workgroup, block 0)
    static const char* force = getenv("OSOT_DEBUG_FORCE_EXTRA");   // developer knob: the EXTRA instantiation for every launch (A/B of the two register allocations)
    LaunchFacts facts;
    facts.T = T; facts.nc = P.nc; facts.fused = fused != nullptr; facts.control = control != nullptr; facts.prof = prof != nullptr;
    facts.roll = control && (control->steps > 1 || control->dq_steps || control->status_steps);
    facts.pairs_out = control && control->K_pairs > 0 && (control->Bt.pair_dist || control->Bt.pair_J || control->Bt.pair_points);
    facts.plan_extra = s->any_inactive || (pl.has_regularisation && pl.regularisation_dense);
    for (int k = 0; k < pl.n_levels; ++k) facts.plan_extra = facts.plan_extra || (s->h_uplan.dense_level[k] != 0);
    facts.hotstart = s->hotstart != 0; facts.force_extra = force && force[0] == '1'; facts.specialise = s->specialise != 0;
    facts.rows_all_equalities = plan_rows_all_equalities(pl);
    KernelVariant v;
    if (const int r = choose_kernel_variant(facts, v, &why)) return fail(r, why);
    TimedLaunch tl;   // (after EVERY early return: nothing is taken from the pool for a launch that does not happen)
    if (int r = timed_begin(s, st, tl)) return r;
    const IhqpLaunch launch{grid, lds, st, P, D, fused, control};
    if (const int r = by_np(T, [&](auto np) { return with_ihqp_kernel<decltype(np)::value>(v, launch); })) return r;
    HIP_TRY(hipGetLastError());
    if (int r = timed_end(s, st, tl)) return r;
    if (s->schedule == 1) {   // this launch's order workgroup has written the order for the next solve of a batch of this size
        s->flip ^= 1;
        s->order_B = b->B;
        s->order_stream = st;
    }
    return OSOT_OK;
}

int osot_stack_update(osot_solver* s, const osot_leaf_batch* leaf, const osot_assembled_out* out, void* hip_stream) {
    if (!s || !leaf || !out) return fail(OSOT_ERR_INVALID, "null argument");
    if (leaf->B < 0 || leaf->B > s->max_batch) return fail(OSOT_ERR_INVALID, "batch size exceeds max_batch");
    if (leaf->B == 0) return OSOT_OK;
    DeviceGuard guard(s->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    const osot_plan_desc& pl = s->plan;
    const DevUpdatePlan& PL = s->h_uplan;
    DevUpdate U;
    const char* why = "";
    int rc = make_update_args(pl, PL, leaf, out, s->d_uplan, U, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    hipLaunchKernelGGL(osot_update_kernel, dim3((unsigned)leaf->B), dim3(64), 0, (hipStream_t)hip_stream, U);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

// the argument checks of the explicit-QP entries (n_max: the entry's own size limit); an empty batch passes whatever its pointers
static int qp_args_check(int B, int n, int n_max, int nc, const double* H, const double* g, const double* A, const double* lA,
                         const double* uA, const double* l, const double* u, const double* x, const int* status) {
    if (B < 0 || n < 1 || n > n_max || nc < 0) return fail(OSOT_ERR_INVALID, "bad sizes");
    if (B == 0) return OSOT_OK;
    if (!H || !g || !x || !status) return fail(OSOT_ERR_INVALID, "null H/g/x/status");
    if (nc > 0 && (!A || !lA || !uA)) return fail(OSOT_ERR_INVALID, "nc > 0 but A/lA/uA is null");
    if ((l == nullptr) != (u == nullptr)) return fail(OSOT_ERR_INVALID, "l and u must both be given or both be null");
    return OSOT_OK;
}

// hot: [B][osot_qp_hot_state_ints(n)] device ints (n <= 64: DevQP.hot; above: DevQPBigHot.hot) or null
static int qp_solve_batch_impl(int B, int n, int nc, const double* H, const double* g, const double* A,
                               const double* lA, const double* uA, const double* l, const double* u,
                               double eps_abs, int max_iter, double* x, int* status, int* iterations,
                               void* hip_stream, int* hot) {
    if (const int r = qp_args_check(B, n, OSOT_MAX_QP_VARS, nc, H, g, A, lA, uA, l, u, x, status)) return r;
    if (B == 0) return OSOT_OK;
    if (n > OSOT_MAX_VARS) {
        // wider than a wavefront (65 .. 128 variables): one 256-thread workgroup per QP (osot_qp_big.h).  hot: the instantiation
        // that carries the hot-start code, else the plain one.  Stream-ordered workspace: not for HIP graph capture.
        if (nc > big::kMaxRows) return fail(OSOT_ERR_UNSUPPORTED, "more than 2048 constraint rows with more than 64 variables");
        DevQPBig Q;
        std::memset(&Q, 0, sizeof(Q));
        Q.B = B; Q.n = n; Q.nc = nc;
        Q.max_iter = max_iter > 0 ? max_iter : 20 * (n + nc) + 100;
        Q.eps_abs = eps_abs;
        Q.H = H; Q.g = g; Q.A = A; Q.lA = lA; Q.uA = uA; Q.l = l; Q.u = u;
        Q.x = x; Q.status = status; Q.iterations = iterations;
        const size_t lds = big::shared_bytes(n, nc);
        int r = hot ? ensure_lds(osot_qp_big_hot_kernel, lds) : ensure_lds(osot_qp_big_kernel, lds);
        if (r != OSOT_OK) return r;
        // (workgroups in flight: 30 KB of LDS at n = 70 lets five share a CU, 82 KB at n = 128 one; the workspace is 2 n^2 doubles each)
        const unsigned cap = n <= 96 ? 1024u : 512u;
        const unsigned grid = (unsigned)B < cap ? (unsigned)B : cap;
        const size_t wbytes = (size_t)grid * 2 * (size_t)n * n * sizeof(double);
        HIP_TRY(hipMallocAsync((void**)&Q.work, wbytes, (hipStream_t)hip_stream));
        if (hot) hipLaunchKernelGGL(osot_qp_big_hot_kernel, dim3(grid), dim3(256), lds, (hipStream_t)hip_stream, DevQPBigHot{Q, hot});
        else hipLaunchKernelGGL(osot_qp_big_kernel, dim3(grid), dim3(256), lds, (hipStream_t)hip_stream, Q);
        const hipError_t le = hipGetLastError();
        HIP_TRY(hipFreeAsync(Q.work, (hipStream_t)hip_stream));
        HIP_TRY(le);
        return OSOT_OK;
    }
    DevQP Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.B = B; Q.n = n; Q.nc = nc;
    Q.max_iter = max_iter > 0 ? max_iter : 20 * (n + nc) + 100;
    Q.eps_abs = eps_abs;
    Q.H = H; Q.g = g; Q.A = A; Q.lA = lA; Q.uA = uA; Q.l = l; Q.u = u;
    Q.x = x; Q.status = status; Q.iterations = iterations;
    const int T = pick_np(n);   // the lane layout of the cascade kernels
    const size_t lds = (size_t)lds_layout(T, nc, &Q.lds_rows_off, &Q.lds_rows_cap) * sizeof(double);
    Q.hot = hot;
    const unsigned grid = (unsigned)B;
    const int rc = by_np(T, [&](auto np) -> int {
        constexpr int NP = decltype(np)::value;
        const auto kernel = hot ? osot_qp_kernel<NP, true> : osot_qp_kernel<NP, false>;
        const int r = ensure_lds(kernel, lds);
        if (r == OSOT_OK) hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, (hipStream_t)hip_stream, Q);
        return r;
    });
    if (rc != OSOT_OK) return rc;
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

int osot_qp_solve_batch(int B, int n, int nc, const double* H, const double* g, const double* A,
                        const double* lA, const double* uA, const double* l, const double* u,
                        double eps_abs, int max_iter, double* x, int* status, int* iterations,
                        void* hip_stream) {
    return qp_solve_batch_impl(B, n, nc, H, g, A, lA, uA, l, u, eps_abs, max_iter, x, status, iterations, hip_stream, nullptr);
}

int osot_qp_hot_state_ints(int n, int* ints) {
    if (!ints) return fail(OSOT_ERR_INVALID, "null out");
    if (n < 1 || n > OSOT_MAX_QP_VARS) return fail(OSOT_ERR_INVALID, "n out of range (1..128)");
    *ints = n <= 32 ? 32 : (n <= OSOT_MAX_VARS ? 64 : big::kHotLen);   // (n <= 64: WaveCtx<NP>::LW of the lane layout pick_np(n) selects)
    return OSOT_OK;
}

int osot_qp_solve_batch_hot(int B, int n, int nc, const double* H, const double* g, const double* A,
                            const double* lA, const double* uA, const double* l, const double* u,
                            double eps_abs, int max_iter, double* x, int* status, int* iterations,
                            int* hot_state, void* hip_stream) {
    return qp_solve_batch_impl(B, n, nc, H, g, A, lA, uA, l, u, eps_abs, max_iter, x, status, iterations, hip_stream, hot_state);
}

int osot_qp_solve_batch_admm_warm(int B, int n, int nc, const double* H, const double* g, const double* A,
                                  const double* lA, const double* uA, const double* l, const double* u,
                                  double eps_reg, const osot_admm_options* opt, double* warm_x, double* warm_y, double* warm_rho,
                                  double* x, int* status, int* iterations, void* hip_stream) {
    if (const int r = qp_args_check(B, n, OSOT_MAX_VARS, nc, H, g, A, lA, uA, l, u, x, status)) return r;
    if (B == 0) return OSOT_OK;
    const bool has_y = (nc + (l ? n : 0)) > 0;
    if ((warm_x == nullptr) != (warm_rho == nullptr) || (warm_x && has_y && !warm_y) || (!warm_x && warm_y))
        return fail(OSOT_ERR_INVALID, "warm_x, warm_y and warm_rho must be given together (or all be null)");
    const DevAdmm Q = admm_args(B, n, nc, H, g, A, lA, uA, l, u, eps_reg, opt, warm_x, warm_y, warm_rho, x, status, iterations);
    const size_t lds = admm_lds_bytes(n, nc, l != nullptr);
    int rc = ensure_lds(osot_admm_kernel, lds);
    if (rc != OSOT_OK) return rc;
    hipLaunchKernelGGL(osot_admm_kernel, dim3((unsigned)B), dim3(64), lds, (hipStream_t)hip_stream, Q);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

int osot_qp_solve_batch_admm(int B, int n, int nc, const double* H, const double* g, const double* A,
                             const double* lA, const double* uA, const double* l, const double* u,
                             double eps_reg, int max_iter, double* x, int* status, int* iterations, void* hip_stream) {
    osot_admm_options opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.max_iter = max_iter;
    return osot_qp_solve_batch_admm_warm(B, n, nc, H, g, A, lA, uA, l, u, eps_reg, &opt, nullptr, nullptr, nullptr, x, status, iterations, hip_stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// batch-of-one BackEnd surface (host pointers).  Mirrors OpenSoT::solvers::BackEnd
// (include/OpenSoT/solvers/BackEnd.h:23-171, src/solvers/BackEnd.cpp:19-104) and the qpOASES
// back-end's re-allocation on a changed row count (QPOasesBackEnd.cpp:229-244).
// ---------------------------------------------------------------------------------------------------
struct osot_backend {
    int nv, nc;
    int hessian_type;
    double eps_abs;
    bool inited, has_bounds;
    int device;         // the device that was current when the back-end was created
    std::vector<double> H, g, A, lA, uA, l, u, x;
    double* d_buf;      // device arena
    size_t d_cap;
    int* d_status;
    int last_status, last_iters;
    int max_iterations = 0;   // osot_backend_options: active-set iteration cap (0: the kernel's default, 20 (n + nc) + 100)
    // hot start across solve() calls (QPOasesBackEnd::solve hot-starts every call, QPOasesBackEnd.cpp:258-285): the inequality
    // working set of the previous solve, 64 constraint codes on the device; forgotten (cold start) by initProblem and whenever
    // the row count changes (the reference re-creates its SQProblem then, QPOasesBackEnd.cpp:229-244)
    int* d_hot = nullptr;
    int hot_nc = -1;          // row count the recorded set belongs to (-1: nothing recorded)
};

namespace {
int backend_run(osot_backend* be) {
    const int n = be->nv, nc = be->nc;
    DeviceGuard guard(be->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    const size_t need = (size_t)n * n + n + (size_t)nc * n + 2 * (size_t)nc + 2 * (size_t)n + n;
    if (need > be->d_cap) {
        if (be->d_buf) hipFree(be->d_buf);
        be->d_buf = nullptr;
        HIP_TRY(hipMalloc((void**)&be->d_buf, need * sizeof(double)));
        be->d_cap = need;
    }
    if (!be->d_status) HIP_TRY(hipMalloc((void**)&be->d_status, 2 * sizeof(int)));
    double* dH = be->d_buf;
    double* dg = dH + (size_t)n * n;
    double* dA = dg + n;
    double* dlA = dA + (size_t)nc * n;
    double* duA = dlA + nc;
    double* dl = duA + nc;
    double* du = dl + n;
    double* dx = du + n;
    HIP_TRY(hipMemcpy(dH, be->H.data(), sizeof(double) * n * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dg, be->g.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    if (nc) {
        HIP_TRY(hipMemcpy(dA, be->A.data(), sizeof(double) * nc * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dlA, be->lA.data(), sizeof(double) * nc, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(duA, be->uA.data(), sizeof(double) * nc, hipMemcpyHostToDevice));
    }
    if (be->has_bounds) {
        HIP_TRY(hipMemcpy(dl, be->l.data(), sizeof(double) * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(du, be->u.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    }
    if (!be->d_hot) HIP_TRY(hipMalloc((void**)&be->d_hot, 64 * sizeof(int)));
    if (be->hot_nc != nc) {   // nothing recorded for this problem shape: cold start
        HIP_TRY(hipMemset(be->d_hot, 0xff, 64 * sizeof(int)));
        be->hot_nc = nc;
    }
    int rc = qp_solve_batch_impl(1, n, nc, dH, dg, nc ? dA : nullptr, nc ? dlA : nullptr, nc ? duA : nullptr,
                                 be->has_bounds ? dl : nullptr, be->has_bounds ? du : nullptr, be->eps_abs, be->max_iterations,
                                 dx, be->d_status, be->d_status + 1, nullptr,
                                 n > OSOT_MAX_VARS ? nullptr : be->d_hot);   // (above 64 variables the plugin starts cold: its record is 64 codes)
    if (rc != OSOT_OK) return rc;
    int st[2];
    HIP_TRY(hipMemcpy(st, be->d_status, 2 * sizeof(int), hipMemcpyDeviceToHost));
    be->last_status = st[0];
    be->last_iters = st[1];
    if (st[0] != OSOT_STATUS_SOLVED) return fail(OSOT_ERR_NOT_SOLVED, "QP not solved (infeasible / iteration limit / H not PD)");
    HIP_TRY(hipMemcpy(be->x.data(), dx, sizeof(double) * n, hipMemcpyDeviceToHost));
    return OSOT_OK;
}
}  // namespace

extern "C" {

int osot_backend_create(int number_of_variables, int number_of_constraints, int hessian_type,
                        double eps_regularisation, osot_backend** out) {
    if (!out) return fail(OSOT_ERR_INVALID, "null out");
    *out = nullptr;
    if (number_of_variables < 1 || number_of_variables > OSOT_MAX_QP_VARS)
        return fail(OSOT_ERR_INVALID, "number_of_variables out of range (1..128)");
    if (number_of_constraints < 0) return fail(OSOT_ERR_INVALID, "negative number_of_constraints");
    if (eps_regularisation < 0) return fail(OSOT_ERR_INVALID, "Negative eps is not allowed!");
    osot_backend* be = new osot_backend();
    be->nv = number_of_variables; be->nc = number_of_constraints; be->hessian_type = hessian_type;
    be->eps_abs = 1.0e3 * 2.221e-16 * eps_regularisation;   // QPOasesBackEnd.cpp:57,67
    be->inited = false; be->has_bounds = false;
    be->d_buf = nullptr; be->d_cap = 0; be->d_status = nullptr;
    be->last_status = 0; be->last_iters = 0;
    if (hipGetDevice(&be->device) != hipSuccess) be->device = 0;
    be->x.assign(be->nv, 0.0);
    *out = be;
    return OSOT_OK;
}

int osot_backend_destroy(osot_backend* be) {
    if (!be) return OSOT_OK;
    DeviceGuard guard(be->device);
    if (be->d_buf) hipFree(be->d_buf);
    if (be->d_status) hipFree(be->d_status);
    if (be->d_hot) hipFree(be->d_hot);
    delete be;
    return OSOT_OK;
}

int osot_backend_update_task(osot_backend* be, const double* H, const double* g) {
    if (!be || !H || !g) return fail(OSOT_ERR_INVALID, "null argument");
    be->H.assign(H, H + (size_t)be->nv * be->nv);
    be->g.assign(g, g + be->nv);
    return OSOT_OK;
}

int osot_backend_update_constraints(osot_backend* be, const double* A, const double* lA, const double* uA,
                                    int number_of_constraints) {
    if (!be || number_of_constraints < 0) return fail(OSOT_ERR_INVALID, "bad argument");
    if (number_of_constraints > 0 && (!A || !lA || !uA)) return fail(OSOT_ERR_INVALID, "null A/lA/uA");
    // validate first, commit after: a refused update leaves the previous problem intact (BackEnd::updateConstraints,
    // BackEnd.cpp:47-71)
    for (int i = 0; i < number_of_constraints; ++i)
        if (lA[i] > uA[i]) return fail(OSOT_ERR_INVALID, "lA > uA");
    be->nc = number_of_constraints;   // a changed row count re-allocates (QPOasesBackEnd.cpp:229-244)
    be->A.assign(A, A + (size_t)be->nc * be->nv);
    be->lA.assign(lA, lA + be->nc);
    be->uA.assign(uA, uA + be->nc);
    return OSOT_OK;
}

int osot_backend_update_bounds(osot_backend* be, const double* l, const double* u) {
    if (!be) return fail(OSOT_ERR_INVALID, "null backend");
    if (!l && !u) { be->has_bounds = false; be->l.clear(); be->u.clear(); return OSOT_OK; }
    if (!l || !u) return fail(OSOT_ERR_INVALID, "l and u must both be given");
    for (int i = 0; i < be->nv; ++i)
        if (l[i] > u[i]) return fail(OSOT_ERR_INVALID, "l > u");   // BackEnd.cpp:76-84
    be->l.assign(l, l + be->nv);
    be->u.assign(u, u + be->nv);
    be->has_bounds = true;
    return OSOT_OK;
}

int osot_backend_init_problem(osot_backend* be, const double* H, const double* g, const double* A,
                              const double* lA, const double* uA, const double* l, const double* u) {
    if (!be) return fail(OSOT_ERR_INVALID, "null backend");
    // every argument is checked before anything is committed: a refused initProblem leaves the object as it was
    if (!H || !g) return fail(OSOT_ERR_INVALID, "null argument");
    if (be->nc > 0 && (!A || !lA || !uA)) return fail(OSOT_ERR_INVALID, "null A/lA/uA");
    for (int i = 0; i < be->nc; ++i)
        if (lA[i] > uA[i]) return fail(OSOT_ERR_INVALID, "lA > uA");
    if ((l == nullptr) != (u == nullptr)) return fail(OSOT_ERR_INVALID, "l and u must both be given");
    if (l) for (int i = 0; i < be->nv; ++i)
        if (l[i] > u[i]) return fail(OSOT_ERR_INVALID, "l > u");
    int rc = osot_backend_update_task(be, H, g);
    if (rc != OSOT_OK) return rc;
    rc = osot_backend_update_constraints(be, A, lA, uA, be->nc);
    if (rc != OSOT_OK) return rc;
    rc = osot_backend_update_bounds(be, l, u);
    if (rc != OSOT_OK) return rc;
    be->hot_nc = -1;          // initProblem is a cold start (QPOasesBackEnd::initProblem -> SQProblem::init)
    rc = backend_run(be);
    be->inited = (rc == OSOT_OK);
    return rc;
}

int osot_backend_solve(osot_backend* be) {
    if (!be) return fail(OSOT_ERR_INVALID, "null backend");
    if (be->H.empty()) return fail(OSOT_ERR_INVALID, "solve() before initProblem()");
    return backend_run(be);
}

int osot_backend_get_solution(osot_backend* be, double* x) {
    if (!be || !x) return fail(OSOT_ERR_INVALID, "null argument");
    std::memcpy(x, be->x.data(), sizeof(double) * be->nv);
    return OSOT_OK;
}

int osot_backend_get_objective(osot_backend* be, double* f) {
    if (!be || !f) return fail(OSOT_ERR_INVALID, "null argument");
    if (be->H.empty()) return fail(OSOT_ERR_INVALID, "no problem");
    const int n = be->nv;
    double v = 0.0;
    for (int i = 0; i < n; ++i) {
        double hx = 0.0;
        for (int j = 0; j < n; ++j) hx += be->H[(size_t)i * n + j] * be->x[j];
        v += be->x[i] * (0.5 * (hx + be->eps_abs * be->x[i]) + be->g[i]);
    }
    *f = v;
    return OSOT_OK;
}

int osot_backend_get_options(osot_backend* be, osot_backend_options* opt) {
    if (!be || !opt) return fail(OSOT_ERR_INVALID, "null argument");
    opt->max_iterations = be->max_iterations;
    opt->last_iterations = be->last_iters;
    opt->last_status = be->last_status;
    return OSOT_OK;
}
int osot_backend_set_options(osot_backend* be, const osot_backend_options* opt) {
    if (!be || !opt) return fail(OSOT_ERR_INVALID, "null argument");
    if (opt->max_iterations < 0) return fail(OSOT_ERR_INVALID, "negative iteration cap");
    be->max_iterations = opt->max_iterations;
    return OSOT_OK;
}

int osot_backend_set_eps_regularisation(osot_backend* be, double eps_abs) {
    if (!be) return fail(OSOT_ERR_INVALID, "null backend");
    if (eps_abs < 0.0) return fail(OSOT_ERR_INVALID, "Negative eps is not allowed!");   // QPOasesBackEnd.cpp:358-366
    be->eps_abs = eps_abs;
    return OSOT_OK;
}
int osot_backend_get_eps_regularisation(osot_backend* be, double* eps_abs) {
    if (!be || !eps_abs) return fail(OSOT_ERR_INVALID, "null argument");
    *eps_abs = be->eps_abs;
    return OSOT_OK;
}
int osot_backend_get_num_variables(osot_backend* be, int* nv) {
    if (!be || !nv) return fail(OSOT_ERR_INVALID, "null argument");
    *nv = be->nv;
    return OSOT_OK;
}
int osot_backend_get_num_constraints(osot_backend* be, int* nc) {
    if (!be || !nc) return fail(OSOT_ERR_INVALID, "null argument");
    *nc = be->nc;
    return OSOT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// batched kinematics producer
// ---------------------------------------------------------------------------------------------------
struct osot_kin {
    DevKin* dev;
    int n, n_frames, n_pairs, n_env, device;
    int n_rowsets, n_gaze, n_split;      // row sets, gaze references, split contact row sets (osot_kin_desc.rowset_*, gaze_*)
    int n_convex;      // pairs that are not capsule / capsule or capsule / box: served by the CONVEX instantiation of the producer alone
};

namespace {
// a pair of the closed forms (osot_kin.h, stage 5)?
bool pair_is_closed_form(const osot_kin_desc* d, int p) {
    return d->pair_kind_a[p] == OSOT_SHAPE_CAPSULE && (d->pair_kind[p] == OSOT_SHAPE_CAPSULE || d->pair_kind[p] == OSOT_SHAPE_BOX);
}
// one side of a pair beyond the capsule: sizes, link_T_shape, the hull's vertex range
int check_pair_shape(const osot_kin_desc* d, int kind, const double* size, double radius, const double* R, const int* hull, const char** why) {
    if ((*why = convex_check_size(kind, size, radius)) != nullptr) return OSOT_ERR_INVALID;
    if ((*why = convex_check_rotation(R)) != nullptr) return OSOT_ERR_INVALID;
    if (kind == OSOT_SHAPE_HULL) {
        if (hull[1] < 1 || hull[1] > OSOT_KIN_MAX_HULL) { *why = "a hull has 1 .. 32 vertices"; return OSOT_ERR_INVALID; }
        if (hull[0] < 0 || hull[0] > d->n_hull_vertices - hull[1]) { *why = "hull vertex range outside n_hull_vertices"; return OSOT_ERR_INVALID; }
    }
    return OSOT_OK;
}
}  // namespace

extern "C" {

int osot_kin_create(const osot_kin_desc* d, int device, osot_kin** out) {
    if (!d || !out) return fail(OSOT_ERR_INVALID, "null argument");
    if (d->n < 1 || d->n > OSOT_KIN_MAX_JOINTS) return fail(OSOT_ERR_INVALID, "joint count out of range");
    if (d->n_frames < 0 || d->n_frames > OSOT_KIN_MAX_FRAMES) return fail(OSOT_ERR_INVALID, "frame count out of range");
    DevKin h;
    std::memset(&h, 0, sizeof(h));
    h.d = *d;
    for (int j = 0; j < d->n; ++j) {
        if (d->parent[j] >= j || d->parent[j] < -1) return fail(OSOT_ERR_INVALID, "joints must be in tree order (parent[j] < j)");
        if (d->type[j] != OSOT_JOINT_REVOLUTE && d->type[j] != OSOT_JOINT_PRISMATIC) return fail(OSOT_ERR_INVALID, "unknown joint type");
    }
    kin_build_tables(h);
    {
        const char* why = "";
        const int rc = kin_check_frames(d, &why);
        if (rc != OSOT_OK) return fail(rc, why);
    }
    if (d->n_pairs < 0 || d->n_pairs > OSOT_KIN_MAX_PAIRS) return fail(OSOT_ERR_INVALID, "collision pair count out of range");
    if (d->n_env < 0 || d->n_env > OSOT_KIN_MAX_ENV) return fail(OSOT_ERR_INVALID, "environment shape count out of range");
    {
        const char* why = "";
        const int rc = kin_check_points(d, &why);
        if (rc != OSOT_OK) return fail(rc, why);
    }
    {
        const char* why = "";
        const int rc = kin_check_rowsets(d, &why);
        if (rc != OSOT_OK) return fail(rc, why);
    }
    if (d->n_hull_vertices < 0 || d->n_hull_vertices > OSOT_KIN_MAX_HULL_VERTICES) return fail(OSOT_ERR_INVALID, "hull vertex count out of range (0..256)");
    for (int v = 0; v < d->n_hull_vertices; ++v)
        for (int i = 0; i < 3; ++i)
            if (!(fabs(d->hull_vertex[v][i]) <= 1.0e300)) return fail(OSOT_ERR_INVALID, "hull vertices must be finite");
    int n_convex = 0;
    for (int p = 0; p < d->n_pairs; ++p) {
        if (d->pair_joint[p][0] < 0 || d->pair_joint[p][0] >= d->n) return fail(OSOT_ERR_INVALID, "collision shape attached to a joint out of range");
        if (d->pair_joint[p][1] < -1 || d->pair_joint[p][1] >= d->n)      // (-1: side b is a world / environment shape)
            return fail(OSOT_ERR_INVALID, "collision shape attached to a joint out of range");
        if (!(d->pair_radius[p][0] >= 0.0) || !(d->pair_radius[p][1] >= 0.0)) return fail(OSOT_ERR_INVALID, "negative capsule radius");
        if (d->pair_kind[p] < OSOT_SHAPE_CAPSULE || d->pair_kind[p] > OSOT_SHAPE_HULL || d->pair_kind_a[p] < OSOT_SHAPE_CAPSULE ||
            d->pair_kind_a[p] > OSOT_SHAPE_HULL)
            return fail(OSOT_ERR_UNSUPPORTED, "unknown collision shape kind");
        if (d->pair_env[p] < 0 || d->pair_env[p] > d->n_env) return fail(OSOT_ERR_INVALID, "pair refers to an environment shape out of range");
        if (d->pair_env[p] > 0 && d->pair_joint[p][1] != -1) return fail(OSOT_ERR_INVALID, "an environment shape is carried by the world (joint -1)");
        if (pair_is_closed_form(d, p)) {
            if (d->pair_kind[p] == OSOT_SHAPE_BOX)
                for (int i = 0; i < 3; ++i) if (!(d->pair_box[p][i] > 0.0)) return fail(OSOT_ERR_INVALID, "box half extents must be positive");
            continue;
        }
        const char* why = "";
        int rc = OSOT_OK;
        if (d->pair_kind_a[p] != OSOT_SHAPE_CAPSULE)
            rc = check_pair_shape(d, d->pair_kind_a[p], d->pair_size_a[p], d->pair_radius[p][0], d->pair_shape_R_a[p], d->pair_hull[p][0], &why);
        if (rc == OSOT_OK && d->pair_kind[p] != OSOT_SHAPE_CAPSULE)
            rc = check_pair_shape(d, d->pair_kind[p], d->pair_box[p], d->pair_radius[p][1], d->pair_shape_R[p], d->pair_hull[p][1], &why);
        if (rc != OSOT_OK) return fail(rc, why);
        ++n_convex;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    osot_kin* k = new osot_kin();
    k->n = d->n; k->n_frames = d->n_frames; k->n_pairs = d->n_pairs; k->n_env = d->n_env; k->device = device;
    k->n_convex = n_convex;
    k->n_rowsets = d->n_rowsets; k->n_gaze = d->n_gaze; k->n_split = 0;
    for (int s = 0; s < d->n_rowsets; ++s) k->n_split |= d->rowset_split[s] ? (1 << s) : 0;
    hipError_t e = hipMalloc(&k->dev, sizeof(DevKin));
    if (e == hipSuccess) e = hipMemcpy(k->dev, &h, sizeof(DevKin), hipMemcpyHostToDevice);
    if (e != hipSuccess) { delete k; return fail(OSOT_ERR_HIP, hipGetErrorString(e)); }
    *out = k;
    return OSOT_OK;
}

int osot_kin_destroy(osot_kin* k) {
    if (!k) return OSOT_OK;
    DeviceGuard guard(k->device);
    if (k->dev) hipFree(k->dev);
    delete k;
    return OSOT_OK;
}

int osot_kinematics(osot_kin* k, const osot_kin_batch* b, void* hip_stream) {
    if (!k || !b) return fail(OSOT_ERR_INVALID, "null argument");
    if (b->B < 0) return fail(OSOT_ERR_INVALID, "negative batch");
    if (b->B == 0) return OSOT_OK;
    if (!b->q) return fail(OSOT_ERR_INVALID, "q is null");
    DeviceGuard guard(k->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    const bool pairs = k->n_pairs > 0 && (b->pair_dist || b->pair_J || b->pair_points);
    if (pairs && k->n_env > 0 && !b->env_pose) return fail(OSOT_ERR_INVALID, "the model has environment shapes but env_pose is null");
    const bool convex = pairs && k->n_convex > 0;      // the instantiation with the per-lane GJK: only where a pair needs it
    // row sets and gaze references: their own instantiation, only where the call binds one
    bool rows = false;
    for (int s = 0; s < OSOT_KIN_MAX_ROWSETS; ++s) {
        const bool bound_b = b->rowset_b[s] != nullptr;
        if (s >= k->n_rowsets) {
            if (b->rowset_A[s] || bound_b) return fail(OSOT_ERR_INVALID, "a row set output is bound beyond the model's n_rowsets");
            continue;
        }
        if (bound_b && !((k->n_split >> s) & 1)) return fail(OSOT_ERR_INVALID, "rowset_b is the output of a split contact row set only");
        if (bound_b && !b->rowset_qdot) return fail(OSOT_ERR_INVALID, "rowset_b is bound but rowset_qdot is null");
        if (bound_b && b->rowset_b_stride[s] < 1) return fail(OSOT_ERR_INVALID, "rowset_b is bound without a stride");
        rows = rows || b->rowset_A[s] || bound_b;
    }
    for (int g = 0; g < OSOT_KIN_MAX_FRAMES; ++g) {
        if (!b->gaze_ref[g] && !b->gaze_point[g]) continue;
        if (g >= k->n_gaze) return fail(OSOT_ERR_INVALID, "a gaze buffer is bound beyond the model's n_gaze");
        if (!b->gaze_ref[g] || !b->gaze_point[g]) return fail(OSOT_ERR_INVALID, "a gaze needs both gaze_point and gaze_ref");
        rows = true;
    }
    if (rows && convex)
        return fail(OSOT_ERR_UNSUPPORTED, "row sets / gaze references with convex collision pairs: two osot_kinematics calls (pair outputs in one, row sets in the other)");
    const dim3 grid((unsigned)(k->n <= 32 ? (b->B + 1) / 2 : b->B)), block(64);   // <= 32 joints: two instances per wavefront
    hipStream_t st = (hipStream_t)hip_stream;
    const DevKin* dk = (const DevKin*)k->dev;
    if (rows) {
        if (k->n <= 32) {
            if (pairs) hipLaunchKernelGGL((osot_kin_kernel<true, 32, false, true>), grid, block, 0, st, dk, *b);
            else hipLaunchKernelGGL((osot_kin_kernel<false, 32, false, true>), grid, block, 0, st, dk, *b);
        } else {
            if (pairs) hipLaunchKernelGGL((osot_kin_kernel<true, 64, false, true>), grid, block, 0, st, dk, *b);
            else hipLaunchKernelGGL((osot_kin_kernel<false, 64, false, true>), grid, block, 0, st, dk, *b);
        }
    } else if (k->n <= 32) {
        if (convex) hipLaunchKernelGGL((osot_kin_kernel<true, 32, true>), grid, block, 0, st, dk, *b);
        else if (pairs) hipLaunchKernelGGL((osot_kin_kernel<true, 32>), grid, block, 0, st, dk, *b);
        else hipLaunchKernelGGL((osot_kin_kernel<false, 32>), grid, block, 0, st, dk, *b);
    } else {
        if (convex) hipLaunchKernelGGL((osot_kin_kernel<true, 64, true>), grid, block, 0, st, dk, *b);
        else if (pairs) hipLaunchKernelGGL((osot_kin_kernel<true, 64>), grid, block, 0, st, dk, *b);
        else hipLaunchKernelGGL((osot_kin_kernel<false, 64>), grid, block, 0, st, dk, *b);
    }
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

int osot_pure_rolling_s33(const double* normal, double* s33, double* normal_unit) {
    if (kin_pure_rolling_s33(normal, s33, normal_unit) != OSOT_OK) return fail(OSOT_ERR_INVALID, "pure rolling: a null or zero outward normal");
    return OSOT_OK;
}

// the producer's convex-shape code on the host: no device, no handle
int osot_shape_distance(const osot_shape* a, const double* world_T_a, const osot_shape* b, const double* world_T_b, double* dist,
                        double* ca, double* cb, int* iterations) {
    if (!a || !b || !world_T_a || !world_T_b) return fail(OSOT_ERR_INVALID, "null argument");
    ConvexCore C[2];
    for (int sd = 0; sd < 2; ++sd) {
        const osot_shape* s = sd == 0 ? a : b;
        const double* T = sd == 0 ? world_T_a : world_T_b;
        if (s->kind < OSOT_SHAPE_CAPSULE || s->kind > OSOT_SHAPE_HULL) return fail(OSOT_ERR_UNSUPPORTED, "unknown collision shape kind");
        if (const char* why = convex_check_size(s->kind, s->size, s->radius)) return fail(OSOT_ERR_INVALID, why);
        for (int i = 0; i < 12; ++i) if (!(fabs(T[i]) <= 1.0e300)) return fail(OSOT_ERR_INVALID, "collision shape: the pose must be finite");
        if (const char* why = convex_check_rotation(T)) return fail(OSOT_ERR_INVALID, why);
        if (s->kind == OSOT_SHAPE_HULL) {
            if (s->n_vertices < 1 || s->n_vertices > OSOT_KIN_MAX_HULL) return fail(OSOT_ERR_INVALID, "a hull has 1 .. 32 vertices");
            if (!s->vertices) return fail(OSOT_ERR_INVALID, "a hull without vertices");
            for (int i = 0; i < 3 * s->n_vertices; ++i)
                if (!(fabs(s->vertices[i]) <= 1.0e300)) return fail(OSOT_ERR_INVALID, "hull vertices must be finite");
        }
        if (s->kind == OSOT_SHAPE_CAPSULE) {      // axis = z of the shape frame, centred
            const double h = s->size[2];
            const double e0[3] = {T[9] - h * T[2], T[10] - h * T[5], T[11] - h * T[8]}, e1[3] = {T[9] + h * T[2], T[10] + h * T[5], T[11] + h * T[8]};
            convex_segment(C[sd], e0, e1);
        } else {
            C[sd].kind = s->kind;
            for (int i = 0; i < 9; ++i) C[sd].R[i] = T[i];
            for (int i = 0; i < 3; ++i) { C[sd].p[i] = T[9 + i]; C[sd].s[i] = s->size[i]; }
            C[sd].v = s->vertices; C[sd].nv = s->n_vertices;
        }
    }
    GjkResult r;
    gjk_closest(C[0], C[1], r);
    if (dist) *dist = r.len - a->radius - b->radius;
    for (int i = 0; i < 3; ++i) { if (ca) ca[i] = r.ca[i]; if (cb) cb[i] = r.cb[i]; }
    if (iterations) *iterations = r.iterations;
    return OSOT_OK;
}

// batched rigid-body dynamics producer (osot_dyn.h): M(q), h(q, qdot), Jdot qdot of frames and of the centre of mass
struct osot_dyn {
    DevDyn* dev;
    osot_kin_desc tree;
    int device;
};

int osot_dyn_create(const osot_kin_desc* tree, const osot_dyn_desc* inertia, int device, osot_dyn** out) {
    if (!tree || !inertia || !out) return fail(OSOT_ERR_INVALID, "null argument");
    std::vector<DevDyn> image(1);    // (70 KB: not on the stack)
    DevDyn& h = image[0];
    const char* why = "";
    const int rc = dyn_build(tree, inertia, h, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    osot_dyn* d = new osot_dyn();
    d->tree = h.k.d; d->device = device; d->dev = nullptr;
    hipError_t e = hipMalloc(&d->dev, sizeof(DevDyn));
    if (e == hipSuccess) e = hipMemcpy(d->dev, &h, sizeof(DevDyn), hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (d->dev) hipFree(d->dev); delete d; return fail(OSOT_ERR_HIP, hipGetErrorString(e)); }
    *out = d;
    return OSOT_OK;
}

int osot_dyn_destroy(osot_dyn* d) {
    if (!d) return OSOT_OK;
    DeviceGuard guard(d->device);
    if (d->dev) hipFree(d->dev);
    delete d;
    return OSOT_OK;
}

int osot_dynamics(osot_dyn* d, const osot_dyn_batch* b, void* hip_stream) {
    if (!d || !b) return fail(OSOT_ERR_INVALID, "null argument");
    const char* why = "";
    const int rc = dyn_check_batch(d->tree, b, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    if (b->B == 0) return OSOT_OK;
    DeviceGuard guard(d->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    // a batch that binds no momentum output runs the instantiation without stage 5a
    if (dyn_wants_momentum(*b))
        hipLaunchKernelGGL((osot_dyn_kernel<64, DYN_MOMENTUM>), dim3((unsigned)b->B), dim3(64), 0, (hipStream_t)hip_stream, (const DevDyn*)d->dev, *b, dyn_kin_batch(*b));
    else
        hipLaunchKernelGGL((osot_dyn_kernel<64, DYN_PLAIN>), dim3((unsigned)b->B), dim3(64), 0, (hipStream_t)hip_stream, (const DevDyn*)d->dev, *b, dyn_kin_batch(*b));
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

// batched posture-gradient producer (osot_grad.h): the b of velocity::Manipulability and velocity::MinimumEffort
struct osot_grad {
    DevGrad* dev;
    int n, n_terms;
    int device;
};

int osot_grad_create(const osot_kin_desc* tree, const osot_grad_desc* desc, int device, osot_grad** out) {
    if (!tree || !desc || !out) return fail(OSOT_ERR_INVALID, "null argument");
    std::vector<DevGrad> image(1);   // (not on the stack)
    DevGrad& h = image[0];
    const char* why = "";
    const int rc = grad_build(tree, desc, h, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    osot_grad* g = new osot_grad();
    g->n = h.k.d.n; g->n_terms = h.n_terms; g->device = device; g->dev = nullptr;
    hipError_t e = hipMalloc(&g->dev, sizeof(DevGrad));
    if (e == hipSuccess) e = hipMemcpy(g->dev, &h, sizeof(DevGrad), hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (g->dev) hipFree(g->dev); delete g; return fail(OSOT_ERR_HIP, hipGetErrorString(e)); }
    *out = g;
    return OSOT_OK;
}

int osot_grad_destroy(osot_grad* g) {
    if (!g) return OSOT_OK;
    DeviceGuard guard(g->device);
    if (g->dev) hipFree(g->dev);
    delete g;
    return OSOT_OK;
}

int osot_posture_gradient(osot_grad* g, const osot_grad_batch* b, void* hip_stream) {
    if (!g || !b) return fail(OSOT_ERR_INVALID, "null argument");
    const char* why = "";
    const int rc = grad_check_batch(g->n, g->n_terms, b, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    if (b->B == 0) return OSOT_OK;
    DeviceGuard guard(g->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    hipLaunchKernelGGL((osot_grad_kernel<64>), dim3((unsigned)b->B), dim3(64), 0, (hipStream_t)hip_stream, (const DevGrad*)g->dev, *b, grad_kin_batch(*b));
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

static int control_launch(osot_solver* s, osot_kin* k, const osot_kin_batch* kb, const osot_leaf_batch* leaf, const osot_assembled_out* out,
                          const osot_qp_batch* b, double* q_integrate, int steps, double* dq_steps, int* status_steps, void* hip_stream);

int osot_control_cycle(osot_solver* s, osot_kin* k, const osot_kin_batch* kb, const osot_leaf_batch* leaf, const osot_assembled_out* out,
                       const osot_qp_batch* b, double* q_integrate, void* hip_stream) {
    return control_launch(s, k, kb, leaf, out, b, q_integrate, 1, nullptr, nullptr, hip_stream);
}

int osot_control_rollout(osot_solver* s, osot_kin* k, const osot_kin_batch* kb, const osot_leaf_batch* leaf, const osot_assembled_out* out,
                         const osot_qp_batch* b, double* q_integrate, int steps, double* dq_steps, int* status_steps, void* hip_stream) {
    if (s && s->wide) return refuse_wide(s, "the fused control cycle / rollout");
    if (steps < 1) return fail(OSOT_ERR_INVALID, "a rollout has at least one step");
    if (steps > 1 && !q_integrate) return fail(OSOT_ERR_INVALID, "a rollout of several steps integrates q (q_integrate is null: every step would solve the same problem)");
    if (s && steps > 1 && plan_has_invariance_bound(s->plan))
        return fail(OSOT_ERR_UNSUPPORTED, "a rollout of several steps cannot carry OSOT_BOUND_JOINT_LIMITS_INVARIANCE: its qdot_prev leaf is not advanced inside a launch (use osot_control_cycle per step)");
    return control_launch(s, k, kb, leaf, out, b, q_integrate, steps, dq_steps, status_steps, hip_stream);
}

static int control_launch(osot_solver* s, osot_kin* k, const osot_kin_batch* kb, const osot_leaf_batch* leaf, const osot_assembled_out* out,
                          const osot_qp_batch* b, double* q_integrate, int steps, double* dq_steps, int* status_steps, void* hip_stream) {
    if (!s || !k || !kb || !leaf || !out || !b) return fail(OSOT_ERR_INVALID, "null argument");
    if (s->wide) return refuse_wide(s, "the fused control cycle / rollout");
    if (leaf->B != b->B || kb->B != b->B) return fail(OSOT_ERR_INVALID, "kinematics batch, leaf batch and qp batch disagree on B");
    if (leaf->B < 0 || leaf->B > s->max_batch) return fail(OSOT_ERR_INVALID, "batch size exceeds max_batch");
    if (leaf->B == 0) return OSOT_OK;
    if (!kb->q) return fail(OSOT_ERR_INVALID, "q is null");
    if (k->device != s->device) return fail(OSOT_ERR_INVALID, "the model and the solver live on different devices");
    if (k->n != s->plan.n) return fail(OSOT_ERR_INVALID, "the model's joint count is not the plan's variable count");
    if (k->n_pairs > 0 && (kb->pair_dist || kb->pair_J) && k->n_env > 0 && !kb->env_pose)
        return fail(OSOT_ERR_INVALID, "the model has environment shapes but env_pose is null");
    // (the fused kernels carry the closed-form pair stage only: no instantiation of theirs runs GJK)
    if (k->n_convex > 0 && (kb->pair_dist || kb->pair_J || kb->pair_points))
        return fail(OSOT_ERR_UNSUPPORTED, "convex collision pairs: use osot_kinematics + osot_cycle");
    if (k->n_rowsets > 0 || k->n_gaze > 0)
        return fail(OSOT_ERR_UNSUPPORTED, "row sets / gaze references: use osot_kinematics + osot_cycle");
    DevUpdate U;
    const char* why = "";
    int rc = make_update_args(s->plan, s->h_uplan, leaf, out, s->d_uplan, U, &why);
    if (rc != OSOT_OK) return fail(rc, why);
    DevControl C;
    C.K = (const DevKin*)k->dev;
    C.K_pairs = k->n_pairs;
    C.Bt = *kb;
    C.q_int = q_integrate;
    C.steps = steps; C.dq_steps = dq_steps; C.status_steps = status_steps;
    return ihqp_launch(s, b, hip_stream, nullptr, &U, &C);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// inverse-dynamics producers and computedTorque (osot_id.h)
// ---------------------------------------------------------------------------------------------------
namespace {
int id_model_check(const osot_id_model* m, int* n_out) {
    if (!m) return fail(OSOT_ERR_INVALID, "null model");
    if (m->B < 0 || m->nv < 1 || m->n_contacts < 0) return fail(OSOT_ERR_INVALID, "bad sizes");
    if (m->contact_dim != 3 && m->contact_dim != 6) return fail(OSOT_ERR_INVALID, "Unsupported  contact model");   // InverseDynamics.cpp:27
    const int nf = m->n_contacts * m->contact_dim;
    if (nf > OSOT_ID_MAX_FORCE_VARS || m->nv + nf > OSOT_MAX_QP_VARS) return fail(OSOT_ERR_UNSUPPORTED, "nv + force variables exceed 128 (or forces exceed 48)");
    if (!m->Bm || (nf > 0 && !m->Jc)) return fail(OSOT_ERR_INVALID, "null B / Jc");
    *n_out = m->nv + nf;
    return OSOT_OK;
}
}  // namespace

extern "C" {

int osot_id_rows(const osot_id_model* m, double* C_dyn, long long dyn_stride, double* C_tau, long long tau_stride,
                 int n_tasks, const double* const* J, const int* J_rows, double* const* A_dst, const long long* A_stride,
                 void* hip_stream) {
    int n = 0;
    int rc = id_model_check(m, &n);
    if (rc != OSOT_OK) return rc;
    if (m->B == 0) return OSOT_OK;
    if (n_tasks < 0 || n_tasks > OSOT_MAX_TASKS) return fail(OSOT_ERR_INVALID, "n_tasks out of range");
    if (n_tasks > 0 && (!J || !J_rows || !A_dst || !A_stride)) return fail(OSOT_ERR_INVALID, "null task arrays");
    if (C_dyn && m->nv < 6) return fail(OSOT_ERR_INVALID, "DynamicFeasibility needs a floating base (nv >= 6)");
    DevIdRows R;
    std::memset(&R, 0, sizeof(R));
    R.B = m->B; R.nv = m->nv; R.n_contacts = m->n_contacts; R.cdim = m->contact_dim; R.n = n;
    R.Bm = m->Bm; R.Jc = m->Jc;
    R.C_dyn = C_dyn; R.dyn_stride = dyn_stride; R.C_tau = C_tau; R.tau_stride = tau_stride;
    R.n_tasks = n_tasks;
    for (int i = 0; i < n_tasks; ++i) {
        if (!J[i] || !A_dst[i] || J_rows[i] < 1) return fail(OSOT_ERR_INVALID, "bad task block");
        R.J[i] = J[i]; R.J_rows[i] = J_rows[i]; R.A_dst[i] = A_dst[i]; R.A_stride[i] = A_stride[i];
    }
    hipLaunchKernelGGL(osot_id_rows_kernel, dim3((unsigned)m->B), dim3(64), 0, (hipStream_t)hip_stream, R);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

// force-space task rows (osot_force.h): force::CoM, force::FloatingBase, StaticConstraint, force::Cartesian
int osot_force_rows(const osot_force_model* m, const osot_force_batch* b, void* hip_stream) {
    const char* why = "";
    const int rc = force_check(m, b, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_force_rows: ") + why);
    if (b->B == 0) return OSOT_OK;
    hipLaunchKernelGGL(osot_force_rows_kernel, dim3((unsigned)b->B), dim3(64), force_lds_bytes(m->n_contacts), (hipStream_t)hip_stream, *m, *b);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

// tasks driven by measurements (osot_feedback.h): CartesianAdmittance, JointAdmittance, IMU, the contact error, the collision task
int osot_feedback(const osot_feedback_model* m, const osot_feedback_batch* b, void* hip_stream) {
    const char* why = "";
    const int rc = feedback_check(m, b, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_feedback: ") + why);
    if (b->B == 0) return OSOT_OK;
    FeedbackCoeffs k;
    feedback_coeffs(m, &k);
    hipLaunchKernelGGL(osot_feedback_kernel, dim3((unsigned)b->B), dim3(64), feedback_lds_bytes(m, b), (hipStream_t)hip_stream, *m, *b, k);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

// acceleration task leaves (osot_acc.h): acceleration::Cartesian / CoM / Postural with gain matrices and GainType::Force, Minv
int osot_acc_tasks(const osot_acc_model* m, const osot_acc_batch* b, void* hip_stream) {
    const char* why = "";
    int rc = acc_check(m, b, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_acc_tasks: ") + why);
    if (b->B == 0) return OSOT_OK;
    const size_t lds = (size_t)acc_lds_bytes(m, b);   // 1.5 KB at nv = 7 with one term, 71 KB at nv = 64 with eight and Minv
    if (lds > 64 * 1024) {
        // the limit is raised to the largest slice there is, ONCE per device: later launches, captured ones included, only launch
        static unsigned long long raised = 0ull;     // bit d: done on device d (benign if two threads both do it)
        int device = 0;
        HIP_TRY(hipGetDevice(&device));
        if (device < 0 || device >= 64 || !((raised >> device) & 1ull)) {
            rc = ensure_lds(osot_acc_tasks_kernel, (size_t)acc_lds_bytes_max());
            if (rc != OSOT_OK) return rc;
            if (device >= 0 && device < 64) raised |= 1ull << device;
        }
    }
    AccArgs A;
    A.M = *m; A.Bt = *b;
    hipLaunchKernelGGL(osot_acc_tasks_kernel, dim3((unsigned)b->B), dim3(64), lds, (hipStream_t)hip_stream, A);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

// multipliers, active set and backward pass of the explicit QP (osot_qp_sens.h): one wavefront per instance, n <= 64
static int sens_launch(const osot_qp_sens_batch* b, const osot_qp_sens_options* opt, void* hip_stream);
int osot_qp_sensitivity_batch(const osot_qp_sens_batch* b, const osot_qp_sens_options* opt, void* hip_stream) {
    const char* why = "";
    int rc = sens_check(b, opt, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_qp_sensitivity_batch: ") + why);
    if (b->B == 0) return OSOT_OK;
    return sens_launch(b, opt, hip_stream);
}
// the launch of osot_qp_sens_kernel on a checked batch (osot_ihqp_sensitivity launches it once per level)
static int sens_launch(const osot_qp_sens_batch* b, const osot_qp_sens_options* opt, void* hip_stream) {
    int rc = OSOT_OK;
    const size_t lds = (size_t)sens_lds_bytes(b->n);   // 29.9 KB at n = 32, 107.8 KB at n = 64
    if (lds > 64 * 1024) {
        // the limit is raised to the largest slice there is, ONCE per device: later launches, captured ones included, only launch
        static unsigned long long raised = 0ull;     // bit d: done on device d (benign if two threads both do it)
        int device = 0;
        HIP_TRY(hipGetDevice(&device));
        if (device < 0 || device >= 64 || !((raised >> device) & 1ull)) {
            rc = ensure_lds(osot_qp_sens_kernel<64>, (size_t)sens_lds_bytes(OSOT_MAX_VARS));
            if (rc != OSOT_OK) return rc;
            if (device >= 0 && device < 64) raised |= 1ull << device;
        }
    }
    SensArgs S;
    S.b = *b;
    sens_options(opt, &S.active_tol, &S.dual_tol, &S.rank_tol);
    if (b->n <= 32) hipLaunchKernelGGL(osot_qp_sens_kernel<32>, dim3((unsigned)b->B), dim3(64), lds, (hipStream_t)hip_stream, S);
    else hipLaunchKernelGGL(osot_qp_sens_kernel<64>, dim3((unsigned)b->B), dim3(64), lds, (hipStream_t)hip_stream, S);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

// the same call with the caller's workspace: n <= 64 is the launch above, 65 .. 128 variables run one 256-thread workgroup per
// instance (osot_qp_sens_big.h), min(B, slots) of them walking the batch, each on its own slice of the workspace
int osot_qp_sens_workspace_bytes(int B, int n, int nc, size_t* bytes) {
    const char* why = "";
    const int rc = sens_ws_bytes_check(B, n, nc, bytes, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_qp_sens_workspace_bytes: ") + why);
    *bytes = sensbig::workspace_bytes(B, n, nc);
    return OSOT_OK;
}
// the launch of osot_qp_sens_big_kernel on a checked batch of 65 .. 128 variables: `grid` workgroups (at most slots(n, nc)) walk the
// batch, each on its own slice of `workspace` (osot_ihqp_sensitivity on a wide handle launches it once per level)
static int sens_big_launch(const osot_qp_sens_batch* b, const osot_qp_sens_options* opt, void* workspace, unsigned grid, void* hip_stream) {
    int rc = OSOT_OK;
    // 41.3 KiB of LDS at (65, 40) lets three workgroups share a CU, 145.1 KiB at (128, 24) one (derived: sensbig::lds_bytes).  The limit is
    // raised to the largest there is, ONCE per device: later launches, captured ones included, only launch
    const size_t lds = sensbig::lds_bytes(b->n, b->nc);
    if (lds > 64 * 1024) {
        static unsigned long long raised = 0ull;     // bit d: done on device d (benign if two threads both do it)
        int device = 0;
        HIP_TRY(hipGetDevice(&device));
        if (device < 0 || device >= 64 || !((raised >> device) & 1ull)) {
            rc = ensure_lds(osot_qp_sens_big_kernel, sensbig::lds_bytes(sensbig::kMaxVars, sensbig::kMaxRows));
            if (rc != OSOT_OK) return rc;
            if (device >= 0 && device < 64) raised |= 1ull << device;
        }
    }
    SensBigArgs S;
    S.s.b = *b;
    sens_options(opt, &S.s.active_tol, &S.s.dual_tol, &S.s.rank_tol);
    S.work = static_cast<double*>(workspace);
    hipLaunchKernelGGL(osot_qp_sens_big_kernel, dim3(grid), dim3(sensbig::kThreads), lds, (hipStream_t)hip_stream, S);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}
int osot_qp_sensitivity_batch_ws(const osot_qp_sens_batch* b, const osot_qp_sens_options* opt, void* workspace, size_t workspace_bytes,
                                 void* hip_stream) {
    const char* why = "";
    const int rc = sens_ws_check(b, opt, workspace, workspace_bytes, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_qp_sensitivity_batch_ws: ") + why);
    if (b->B == 0) return OSOT_OK;
    if (b->n <= OSOT_MAX_VARS) return sens_launch(b, opt, hip_stream);
    const int slots = sensbig::slots(b->n, b->nc);
    return sens_big_launch(b, opt, workspace, (unsigned)(b->B < slots ? b->B : slots), hip_stream);
}

// ---- the level QPs of the cascade, their multipliers, active sets and objectives (osot_ihqp_sens.h) -------------------------------
int osot_ihqp_level_rows(osot_solver* s, int level, int* rows) {
    if (!s || !rows) return fail(OSOT_ERR_INVALID, "osot_ihqp_level_rows: null argument");
    if (level < 0 || level >= s->plan.n_levels) return fail(OSOT_ERR_INVALID, "osot_ihqp_level_rows: level out of range");
    LevelPlan P;
    make_plan_shape(s->plan, nullptr, nullptr, P);
    *rows = level_qp_rows(P, level);
    return OSOT_OK;
}

// the wide route (65 .. 128 variables, osot_ihqp_sens_wide.h): one 256-thread workgroup per instance.  The level kernel's LDS is
// 67 072 bytes at n = 128, above the default limit: it is raised to that, ONCE per device, on the first call -- one eager call must
// come before a capture (osot_qp_sens_big_kernel's limit is raised the same way by sens_big_launch)
static int level_qp_wide_launch(const LevelQpArgs& Q, hipStream_t st) {
    const size_t lds = (size_t)ihqpwide::level_lds_bytes(Q.P.n);
    if (lds > 64 * 1024) {
        static unsigned long long raised = 0ull;     // bit d: done on device d (benign if two threads both do it)
        int device = 0;
        HIP_TRY(hipGetDevice(&device));
        if (device < 0 || device >= 64 || !((raised >> device) & 1ull)) {
            const int rc = ensure_lds(osot_ihqp_level_qp_wide_kernel, (size_t)ihqpwide::level_lds_bytes(ihqpwide::kMaxVars));
            if (rc != OSOT_OK) return rc;
            if (device >= 0 && device < 64) raised |= 1ull << device;
        }
    }
    hipLaunchKernelGGL(osot_ihqp_level_qp_wide_kernel, dim3((unsigned)Q.D.B), dim3(ihqpwide::kThreads), lds, st, Q);
    return OSOT_OK;
}

static void level_qp_launch(const LevelQpArgs& Q, hipStream_t st) {
    const size_t lds = (size_t)level_qp_lds_bytes(Q.P.n);     // at most 33 792 bytes: below the default limit
    if (Q.P.n <= 32) hipLaunchKernelGGL(osot_ihqp_level_qp_kernel<32>, dim3((unsigned)Q.D.B), dim3(64), lds, st, Q);
    else hipLaunchKernelGGL(osot_ihqp_level_qp_kernel<64>, dim3((unsigned)Q.D.B), dim3(64), lds, st, Q);
}

int osot_ihqp_level_qp(osot_solver* s, const osot_qp_batch* b, int level, const osot_level_qp* out, void* hip_stream) {
    if (!s) return fail(OSOT_ERR_INVALID, "osot_ihqp_level_qp: null solver");
    LevelQpArgs Q;
    const char* why = "";
    const int rc = level_qp_check(s->plan, s->wide, s->max_batch, s->any_inactive ? s->task_active : nullptr, b, level, out, Q, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_ihqp_level_qp: ") + why);
    if (b->B == 0) return OSOT_OK;
    DeviceGuard guard(s->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    if (s->wide) {
        const int r = level_qp_wide_launch(Q, (hipStream_t)hip_stream);
        if (r != OSOT_OK) return r;
    } else {
        level_qp_launch(Q, (hipStream_t)hip_stream);
    }
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

int osot_ihqp_sens_workspace_bytes(osot_solver* s, int B, int want_backward, int want_grad_A, unsigned long long* bytes) {
    if (!s || !bytes) return fail(OSOT_ERR_INVALID, "osot_ihqp_sens_workspace_bytes: null argument");
    if (s->wide && s->plan.n <= OSOT_MAX_VARS) return fail(OSOT_ERR_UNSUPPORTED, "osot_ihqp_sens_workspace_bytes: per-level multipliers are built for handles of osot_solver_create, not for the wide route");
    if (B < 0 || B > s->max_batch) return fail(OSOT_ERR_INVALID, "osot_ihqp_sens_workspace_bytes: batch size exceeds max_batch");
    LevelPlan P;
    make_plan_shape(s->plan, nullptr, nullptr, P);
    *bytes = s->wide ? ihqp_wide_workspace_bytes(P, B, want_backward != 0, want_grad_A != 0)
                     : (unsigned long long)ihqp_sens_workspace(P, B, want_backward != 0, want_grad_A != 0).total * sizeof(double);
    return OSOT_OK;
}

int osot_ihqp_sensitivity(osot_solver* s, const osot_ihqp_sens_batch* b, const osot_qp_sens_options* opt, void* hip_stream) {
    if (!s) return fail(OSOT_ERR_INVALID, "osot_ihqp_sensitivity: null solver");
    LevelQpArgs Q;
    const char* why = "";
    const int rc = ihqp_sens_check(s->plan, s->wide, s->max_batch, s->any_inactive ? s->task_active : nullptr, b, opt, Q, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_ihqp_sensitivity: ") + why);
    if (b->qp.B == 0) return OSOT_OK;
    DeviceGuard guard(s->device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    struct {
        hipStream_t st; const osot_qp_sens_options* opt;
        void level_qp(const LevelQpArgs& q) { level_qp_launch(q, st); }
        int sens(const osot_qp_sens_batch& S) { return sens_launch(&S, opt, st); }
        void objective(const ObjectiveArgs& O) { hipLaunchKernelGGL(osot_ihqp_objective_kernel, dim3((unsigned)O.B), dim3(64), (size_t)O.n * sizeof(double), st, O); }
        void pullback(const PullbackArgs& R) { hipLaunchKernelGGL(osot_ihqp_pullback_kernel, dim3((unsigned)R.D.B), dim3(64), (size_t)pullback_lds_bytes(R.P.n), st, R); }
        void zero(void* p, size_t bytes) { if (bytes) (void)hipMemsetAsync(p, 0, bytes, st); }
        void copy(void* dst, const void* src, size_t bytes) { (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st); }
    } go{(hipStream_t)hip_stream, opt};
    if (s->wide) {
        // the same schedule with the workgroup kernels; the Y slices of osot_qp_sens_big_kernel follow the schedule's arrays
        struct {
            hipStream_t st; const osot_qp_sens_options* opt; void* slices; unsigned grid; int rc;
            void level_qp(const LevelQpArgs& q) { const int r = level_qp_wide_launch(q, st); if (rc == OSOT_OK) rc = r; }
            int sens(const osot_qp_sens_batch& S) { return rc != OSOT_OK ? rc : sens_big_launch(&S, opt, slices, grid, st); }
            void objective(const ObjectiveArgs& O) { hipLaunchKernelGGL(osot_ihqp_objective_wide_kernel, dim3((unsigned)O.B), dim3(ihqpwide::kThreads), (size_t)ihqpwide::objective_lds_bytes(O.n), st, O); }
            void pullback(const PullbackArgs& R) { hipLaunchKernelGGL(osot_ihqp_pullback_wide_kernel, dim3((unsigned)R.D.B), dim3(ihqpwide::kThreads), (size_t)ihqpwide::pullback_lds_bytes(R.P.n), st, R); }
            void zero(void* p, size_t bytes) { if (bytes) (void)hipMemsetAsync(p, 0, bytes, st); }
            void copy(void* dst, const void* src, size_t bytes) { (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st); }
        } wgo{(hipStream_t)hip_stream, opt,
              static_cast<char*>(b->workspace) + ihqp_wide_front_bytes(Q.P, b->qp.B, b->grad_dq != nullptr, ihqp_wants_grad_A(*b, Q.P.L)),
              (unsigned)ihqp_wide_sens_grid(Q.P, b->qp.B), OSOT_OK};
        if (const int r = ihqp_sens_levels(Q, b, wgo)) return r;
    } else if (const int r = ihqp_sens_levels(Q, b, go)) return r;
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

int osot_feedback_state_doubles(const osot_feedback_model* m, int* count) {
    if (!m || !count) return fail(OSOT_ERR_INVALID, "osot_feedback_state_doubles: null argument");
    if (m->nv < 1 || m->nv > OSOT_KIN_MAX_JOINTS || m->n_cart < 0 || m->n_cart > OSOT_FEEDBACK_MAX_CART || (m->joint != 0 && m->joint != 1))
        return fail(OSOT_ERR_INVALID, "osot_feedback_state_doubles: nv, n_cart or joint is out of range");
    *count = feedback_state_count(m);
    return OSOT_OK;
}

int osot_admittance_params(const double K[6], const double D[6], double lambda, double dt, double C[6], double M[6], double w[6]) {
    const char* why = "";
    const int rc = feedback_admittance_params(K, D, lambda, dt, C, M, w, &why);
    if (rc != OSOT_OK) return fail(rc, std::string("osot_admittance_params: ") + why);
    return OSOT_OK;
}

int osot_id_force_gains(int B, int nv, int rows, const double* J, const double* Bi, const double* Kp, const double* Kd,
                        const double* f_virtual, double* p0_gains, long long p0_stride, double* a_ref, void* hip_stream) {
    if (B < 0 || nv < 1 || nv > OSOT_MAX_QP_VARS || rows < 1 || rows > 6) return fail(OSOT_ERR_INVALID, "force gains: sizes out of range (nv <= 128, rows <= 6)");
    if (B == 0) return OSOT_OK;
    if (!J || !Bi || !Kp || !Kd || !p0_gains) return fail(OSOT_ERR_INVALID, "force gains: null argument");
    if (f_virtual && !a_ref) return fail(OSOT_ERR_INVALID, "force gains: a virtual force needs a_ref to add Mi f to");
    DevForceGains F;
    std::memset(&F, 0, sizeof(F));
    F.B = B; F.nv = nv; F.rows = rows; F.J = J; F.Bi = Bi; F.f = f_virtual; F.G = p0_gains; F.G_stride = p0_stride; F.a_ref = a_ref;
    for (int i = 0; i < rows * rows; ++i) { F.Kp[i] = Kp[i]; F.Kd[i] = Kd[i]; }
    if (nv <= 64) hipLaunchKernelGGL(osot_force_gains_kernel<64>, dim3((unsigned)B), dim3(64), 0, (hipStream_t)hip_stream, F);
    else hipLaunchKernelGGL(osot_force_gains_kernel<OSOT_MAX_QP_VARS>, dim3((unsigned)B), dim3(64), 0, (hipStream_t)hip_stream, F);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

int osot_computed_torque(const osot_id_model* m, const double* x, double* tau, int* ok, double fb_tol, void* hip_stream) {
    int n = 0;
    int rc = id_model_check(m, &n);
    if (rc != OSOT_OK) return rc;
    if (m->B == 0) return OSOT_OK;
    if (!m->h || !x || !tau) return fail(OSOT_ERR_INVALID, "null h / x / tau");
    DevTorque T;
    std::memset(&T, 0, sizeof(T));
    T.B = m->B; T.nv = m->nv; T.n_contacts = m->n_contacts; T.cdim = m->contact_dim; T.n = n; T.floating_base = m->floating_base;
    T.Bm = m->Bm; T.h = m->h; T.Jc = m->Jc; T.x = x; T.tau = tau; T.ok = ok; T.fb_tol = fb_tol;
    hipLaunchKernelGGL(osot_torque_kernel, dim3((unsigned)m->B), dim3(64), 0, (hipStream_t)hip_stream, T);
    HIP_TRY(hipGetLastError());
    return OSOT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// multi-GPU: one RCCL all-gather of the solved dq shards (instances are independent)
// ---------------------------------------------------------------------------------------------------
struct osot_comm {
    ncclComm_t comm;
    int rank, world;
};

extern "C" {

int osot_comm_unique_id(void* id128) {
    if (!id128) return fail(OSOT_ERR_INVALID, "null id");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(OSOT_ERR_COMM, ncclGetErrorString(r));
    std::memcpy(id128, &id, sizeof(id));
    return OSOT_OK;
}

int osot_comm_create(const void* id128, int rank, int world, int device, osot_comm** out) {
    if (!id128 || !out || world < 1 || rank < 0 || rank >= world) return fail(OSOT_ERR_INVALID, "bad argument");
    *out = nullptr;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(OSOT_ERR_HIP, "hipSetDevice failed");
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    ncclComm_t c;
    ncclResult_t r = ncclCommInitRank(&c, world, id, rank);
    if (r != ncclSuccess) return fail(OSOT_ERR_COMM, ncclGetErrorString(r));
    osot_comm* oc = new osot_comm();
    oc->comm = c; oc->rank = rank; oc->world = world;
    *out = oc;
    return OSOT_OK;
}

int osot_comm_destroy(osot_comm* c) {
    if (!c) return OSOT_OK;
    ncclCommDestroy(c->comm);
    delete c;
    return OSOT_OK;
}

int osot_allgather_dq(osot_comm* c, const double* send, double* recv, long long count, void* hip_stream) {
    if (!c || !send || !recv || count < 0) return fail(OSOT_ERR_INVALID, "bad argument");
    ncclResult_t r = ncclAllGather(send, recv, (size_t)count, ncclDouble, c->comm, (hipStream_t)hip_stream);
    if (r != ncclSuccess) return fail(OSOT_ERR_COMM, ncclGetErrorString(r));
    return OSOT_OK;
}

}  // extern "C"
