"""ctypes mirror of include/osot_mi355x.h (structs, enums, prototypes).

Host-side plumbing only: the product's arithmetic lives in opensot_amd/csrc (HIP, gfx950).
"""
import ctypes as C
import os

MAX_LEVELS, MAX_TASKS, MAX_BOUNDS, MAX_ROWBLOCKS, MAX_VARS = 8, 8, 4, 8, 64
MAX_QP_VARS = 128      # the explicit-QP surface (osot_qp_solve_batch, osot_backend_*): OSOT_MAX_QP_VARS
MAX_BAND_ROWS, ID_MAX_FORCE_VARS = 6, 48

OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_HIP, ERR_NOT_SOLVED, ERR_COMM = range(6)
STATUS_SOLVED, STATUS_INFEASIBLE, STATUS_MAX_ITER, STATUS_NOT_PD = range(4)
TASK_GENERIC, TASK_CARTESIAN, TASK_COM, TASK_POSTURAL, TASK_ACC_CARTESIAN, TASK_ACC_COM, TASK_ACC_POSTURAL = range(7)
BOUND_GENERIC, BOUND_JOINT_LIMITS, BOUND_VELOCITY_LIMITS = range(3)
# velocity::JointLimitsInvariance: dT = dt, scaling = the step-ahead predictor p (0 < p <= 1); leaf p2 = the previous cycle's velocity
BOUND_JOINT_LIMITS_INVARIANCE = 3
(ROWS_GENERIC, ROWS_COLLISION, ROWS_DYN_FEASIBILITY, ROWS_TORQUE_LIMITS, ROWS_FRICTION_CONE,
 ROWS_ACC_JOINT_LIMITS, ROWS_ACC_VELOCITY_LIMITS, ROWS_TASK_CARTESIAN, ROWS_TASK_COM, ROWS_UNIT_GENERIC) = range(10)
# surface contacts: 6-D wrenches, 5 / 4 / 8 stored rows per contact (force::FrictionCone, force::CoP, force::NormalTorque)
ROWS_WRENCH_FRICTION_CONE, ROWS_COP, ROWS_NORMAL_TORQUE = 10, 11, 12
# velocity::ConvexHull: rows = contact points (3 .. 16), built on the device from the CoM, its Jacobian and the points.  13 .. 15 are
# not kinds (the validators refuse them as unknown)
ROWS_CONVEX_HULL = 16
# acceleration::JointLimitsViability / JointLimitsECBF: unit rows (not stored), like ROWS_ACC_JOINT_LIMITS; 17 is not a kind
ROWS_ACC_JOINT_LIMITS_VIABILITY, ROWS_ACC_JOINT_LIMITS_ECBF = 18, 19
# velocity::CartesianPositionConstraint on a link / on the CoM: rows = half-spaces (1 .. 16), stored rows built on the device
ROWS_POSITION_CARTESIAN, ROWS_POSITION_COM = 20, 21
MAX_POSITION_ROWS = 16
# OpenSoT::HessianType (include/OpenSoT/Task.h:33-41)
HST_UNDEFINED, HST_ZERO, HST_IDENTITY, HST_POSDEF, HST_POSDEF_NULLSPACE, HST_SEMIDEF, HST_UNKNOWN = range(7)

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)


class TaskDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("rows", C.c_int), ("weight", C.c_double),
                ("lambda_", C.c_double), ("orientation_gain", C.c_double), ("lambda2", C.c_double),
                ("row_mask", C.c_ulonglong), ("parent_rows", C.c_int), ("sub_lambda", C.c_double),
                ("body_frame", C.c_int), ("dense_weight", C.c_int), ("acc_gain_matrices", C.c_int)]


class LevelDesc(C.Structure):
    _fields_ = [("n_tasks", C.c_int), ("task", TaskDesc * MAX_TASKS)]


class BoundDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("scaling", C.c_double), ("dT", C.c_double)]


class RowsDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("rows", C.c_int), ("d_threshold", C.c_double),
                ("detection_threshold", C.c_double), ("bound_scaling", C.c_double),
                ("first_col", C.c_int), ("dT", C.c_double), ("p", C.c_double), ("mu", C.c_double),
                ("task_lambda", C.c_double), ("task_orientation_gain", C.c_double),
                ("err_lb", C.c_double * MAX_BAND_ROWS), ("err_ub", C.c_double * MAX_BAND_ROWS),
                ("task_body_frame", C.c_int), ("n_candidates", C.c_int), ("only_level", C.c_int)]


class PlanDesc(C.Structure):
    _fields_ = [("n", C.c_int), ("n_levels", C.c_int), ("level", LevelDesc * MAX_LEVELS),
                ("n_bounds", C.c_int), ("bound", BoundDesc * MAX_BOUNDS),
                ("n_rowblocks", C.c_int), ("rowblock", RowsDesc * MAX_ROWBLOCKS),
                ("eps_abs", C.c_double), ("max_iter", C.c_int),
                ("has_regularisation", C.c_int), ("regularisation", TaskDesc), ("regularisation_dense", C.c_int)]


class QpBatch(C.Structure):
    _fields_ = [("B", C.c_int),
                ("A", C.c_void_p * MAX_LEVELS), ("b", C.c_void_p * MAX_LEVELS),
                ("w", C.c_void_p * MAX_LEVELS), ("c", C.c_void_p * MAX_LEVELS),
                ("C", C.c_void_p), ("lo", C.c_void_p), ("up", C.c_void_p),
                ("l", C.c_void_p), ("u", C.c_void_p),
                ("level_active", C.c_void_p),
                ("dq", C.c_void_p), ("x_levels", C.c_void_p),
                ("status", C.c_void_p), ("iterations", C.c_void_p), ("b_reg", C.c_void_p),
                ("WA", C.c_void_p * MAX_LEVELS), ("Wb", C.c_void_p * MAX_LEVELS),
                ("accepted_slack", C.c_void_p), ("A_reg", C.c_void_p)]


class LeafPtrs(C.Structure):
    _fields_ = [("p0", C.c_void_p), ("p1", C.c_void_p), ("p2", C.c_void_p), ("W", C.c_void_p)]


class LeafBatch(C.Structure):
    _fields_ = [("B", C.c_int),
                ("task", (LeafPtrs * MAX_TASKS) * MAX_LEVELS),
                ("bound", LeafPtrs * MAX_BOUNDS),
                ("rows", LeafPtrs * MAX_ROWBLOCKS), ("regularisation", LeafPtrs)]


class AssembledOut(C.Structure):
    _fields_ = [("b", C.c_void_p * MAX_LEVELS), ("w", C.c_void_p * MAX_LEVELS),
                ("C", C.c_void_p), ("lo", C.c_void_p), ("up", C.c_void_p),
                ("l", C.c_void_p), ("u", C.c_void_p), ("b_reg", C.c_void_p),
                ("WA", C.c_void_p * MAX_LEVELS), ("Wb", C.c_void_p * MAX_LEVELS), ("A", C.c_void_p * MAX_LEVELS)]


class BackendOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("last_iterations", C.c_int), ("last_status", C.c_int)]


class NhqpOptions(C.Structure):
    _fields_ = [("free_vars", C.c_int * MAX_LEVELS), ("min_sv_ratio", C.c_double),
                ("no_ab_regularization", C.c_int), ("no_selective_ns_regularization", C.c_int),
                ("min_sv_ratio_is_set", C.c_int),
                ("level_no_ab_regularization", C.c_int * MAX_LEVELS), ("level_no_selective_ns_regularization", C.c_int * MAX_LEVELS),
                ("level_min_sv_ratio_is_set", C.c_int * MAX_LEVELS), ("level_min_sv_ratio", C.c_double * MAX_LEVELS),
                ("level_W", C.c_void_p * MAX_LEVELS)]


class AdmmOptions(C.Structure):
    _fields_ = [("eps_abs", C.c_double), ("eps_rel", C.c_double), ("rho", C.c_double), ("sigma", C.c_double),
                ("alpha", C.c_double), ("max_iter", C.c_int), ("scaling", C.c_int), ("check_every", C.c_int)]


class IdModel(C.Structure):
    _fields_ = [("B", C.c_int), ("nv", C.c_int), ("n_contacts", C.c_int), ("contact_dim", C.c_int),
                ("Bm", C.c_void_p), ("h", C.c_void_p), ("Jc", C.c_void_p), ("floating_base", C.c_int)]


# every symbol include/osot_mi355x.h declares (tests/test_abi_symbols.py checks the .so exports all)
KIN_MAX_JOINTS, KIN_MAX_FRAMES, KIN_MAX_PAIRS = 64, 8, 32
KIN_MAX_ENV = 16
KIN_MAX_POINTS = 16
KIN_MAX_HULL_VERTICES, KIN_MAX_HULL = 256, 32      # hull vertices of a model / of one hull
SHAPE_CAPSULE, SHAPE_BOX, SHAPE_CYLINDER, SHAPE_HULL = 0, 1, 2, 3
JOINT_REVOLUTE, JOINT_PRISMATIC = 0, 1
KIN_MAX_ROWSETS = 8
ROWSET_CONTACT, ROWSET_PURE_ROLLING, ROWSET_OMNI4X = 1, 2, 3
ROWSET_ROWS = {ROWSET_CONTACT: 6, ROWSET_PURE_ROLLING: 4, ROWSET_OMNI4X: 3}      # rows of a kind before its row_mask


class KinDesc(C.Structure):
    _fields_ = [("n", C.c_int), ("parent", C.c_int * KIN_MAX_JOINTS), ("type", C.c_int * KIN_MAX_JOINTS),
                ("axis", (C.c_double * 3) * KIN_MAX_JOINTS), ("R0", (C.c_double * 9) * KIN_MAX_JOINTS),
                ("p0", (C.c_double * 3) * KIN_MAX_JOINTS), ("mass", C.c_double * KIN_MAX_JOINTS),
                ("com", (C.c_double * 3) * KIN_MAX_JOINTS), ("n_frames", C.c_int),
                ("frame_joint", C.c_int * KIN_MAX_FRAMES), ("frame_R", (C.c_double * 9) * KIN_MAX_FRAMES),
                ("frame_p", (C.c_double * 3) * KIN_MAX_FRAMES), ("n_pairs", C.c_int),
                ("pair_joint", (C.c_int * 2) * KIN_MAX_PAIRS), ("pair_seg", ((C.c_double * 6) * 2) * KIN_MAX_PAIRS),
                ("pair_radius", (C.c_double * 2) * KIN_MAX_PAIRS),
                ("frame_body", C.c_int * KIN_MAX_FRAMES), ("frame_col_mask", C.c_ulonglong * KIN_MAX_FRAMES),
                ("com_col_mask", C.c_ulonglong),
                ("pair_kind", C.c_int * KIN_MAX_PAIRS), ("pair_env", C.c_int * KIN_MAX_PAIRS),
                ("pair_box", (C.c_double * 3) * KIN_MAX_PAIRS), ("pair_shape_R", (C.c_double * 9) * KIN_MAX_PAIRS),
                ("pair_shape_p", (C.c_double * 3) * KIN_MAX_PAIRS), ("n_env", C.c_int),
                ("frame_base", C.c_int * KIN_MAX_FRAMES),
                ("pair_kind_a", C.c_int * KIN_MAX_PAIRS), ("pair_size_a", (C.c_double * 3) * KIN_MAX_PAIRS),
                ("pair_shape_R_a", (C.c_double * 9) * KIN_MAX_PAIRS), ("pair_shape_p_a", (C.c_double * 3) * KIN_MAX_PAIRS),
                ("pair_hull", ((C.c_int * 2) * 2) * KIN_MAX_PAIRS), ("n_hull_vertices", C.c_int),
                ("hull_vertex", (C.c_double * 3) * KIN_MAX_HULL_VERTICES),
                ("n_rowsets", C.c_int), ("rowset_kind", C.c_int * KIN_MAX_ROWSETS), ("rowset_frame", C.c_int * KIN_MAX_ROWSETS),
                ("rowset_row_mask", C.c_int * KIN_MAX_ROWSETS), ("rowset_split", C.c_int * KIN_MAX_ROWSETS),
                ("rowset_wheel", (C.c_int * 4) * KIN_MAX_ROWSETS), ("rowset_param", (C.c_double * 36) * KIN_MAX_ROWSETS),
                ("n_gaze", C.c_int), ("gaze_frame", C.c_int * KIN_MAX_FRAMES),
                ("n_points", C.c_int), ("point_joint", C.c_int * KIN_MAX_POINTS), ("point_p", (C.c_double * 3) * KIN_MAX_POINTS)]


class KinBatch(C.Structure):
    _fields_ = [("B", C.c_int), ("q", C.c_void_p), ("frame_pose", C.c_void_p * KIN_MAX_FRAMES),
                ("frame_J", C.c_void_p * KIN_MAX_FRAMES), ("frame_J_stride", C.c_longlong * KIN_MAX_FRAMES),
                ("com", C.c_void_p), ("com_J", C.c_void_p), ("com_J_stride", C.c_longlong),
                ("pair_dist", C.c_void_p), ("pair_J", C.c_void_p), ("pair_J_stride", C.c_longlong),
                ("env_pose", C.c_void_p), ("env_pose_stride", C.c_longlong), ("pair_points", C.c_void_p),
                ("rowset_A", C.c_void_p * KIN_MAX_ROWSETS), ("rowset_A_stride", C.c_longlong * KIN_MAX_ROWSETS),
                ("rowset_b", C.c_void_p * KIN_MAX_ROWSETS), ("rowset_b_stride", C.c_longlong * KIN_MAX_ROWSETS),
                ("rowset_qdot", C.c_void_p), ("gaze_point", C.c_void_p * KIN_MAX_FRAMES), ("gaze_ref", C.c_void_p * KIN_MAX_FRAMES),
                ("points", C.c_void_p)]


class Shape(C.Structure):
    _fields_ = [("kind", C.c_int), ("size", C.c_double * 3), ("radius", C.c_double), ("n_vertices", C.c_int), ("vertices", dp)]


class DynDesc(C.Structure):
    _fields_ = [("inertia", (C.c_double * 6) * KIN_MAX_JOINTS), ("gravity", C.c_double * 3)]


class DynBatch(C.Structure):
    _fields_ = [("B", C.c_int), ("q", C.c_void_p), ("qdot", C.c_void_p), ("M", C.c_void_p), ("M_stride", C.c_longlong),
                ("h", C.c_void_p), ("frame_Jdot_qdot", C.c_void_p * KIN_MAX_FRAMES),
                ("frame_Jdot_qdot_stride", C.c_longlong * KIN_MAX_FRAMES),
                ("com_Jdot_qdot", C.c_void_p), ("com_Jdot_qdot_stride", C.c_longlong),
                ("cmm_lin", C.c_void_p), ("cmm_lin_stride", C.c_longlong), ("cmm_lin_ld", C.c_int),
                ("cmm_ang", C.c_void_p), ("cmm_ang_stride", C.c_longlong), ("cmm_ang_ld", C.c_int),
                ("momentum", C.c_void_p), ("momentum_stride", C.c_longlong),
                ("ang_mom_b", C.c_void_p), ("ang_mom_b_stride", C.c_longlong),
                ("ang_mom_ref", C.c_void_p), ("ang_mom_rate_ref", C.c_void_p),
                ("ang_mom_gain", C.c_double * 9), ("ang_mom_lambda", C.c_double)]


GRAD_MANIPULABILITY_FRAME, GRAD_MANIPULABILITY_COM, GRAD_MIN_EFFORT = range(3)
GRAD_MAX_TERMS = 4


class GradDesc(C.Structure):
    _fields_ = [("n_terms", C.c_int), ("kind", C.c_int * GRAD_MAX_TERMS), ("frame", C.c_int * GRAD_MAX_TERMS),
                ("step", C.c_double * GRAD_MAX_TERMS), ("lambda_", C.c_double * GRAD_MAX_TERMS),
                ("joint_mask", C.c_ulonglong * GRAD_MAX_TERMS), ("W_diag", (C.c_double * KIN_MAX_JOINTS) * GRAD_MAX_TERMS),
                ("gravity", C.c_double * 3)]


class GradBatch(C.Structure):
    _fields_ = [("B", C.c_int), ("q", C.c_void_p), ("b", C.c_void_p * GRAD_MAX_TERMS), ("b_stride", C.c_longlong * GRAD_MAX_TERMS),
                ("value", C.c_void_p * GRAD_MAX_TERMS)]


FORCE_MAX_CONTACTS = 8


class ForceModel(C.Structure):
    _fields_ = [("n_contacts", C.c_int), ("nv", C.c_int), ("n", C.c_int), ("wrench_col", C.c_int * FORCE_MAX_CONTACTS),
                ("torque_col", C.c_int), ("cart_contact", C.c_int), ("mass", C.c_double), ("gravity", C.c_double * 3),
                ("com_lambda", C.c_double), ("com_lambda2", C.c_double), ("com_lambda_ang", C.c_double),
                ("cart_Kp", C.c_double * 36), ("cart_Kd", C.c_double * 36)]


class ForceBatch(C.Structure):
    _fields_ = [("B", C.c_int), ("pose", C.c_void_p * FORCE_MAX_CONTACTS), ("Jc", C.c_void_p), ("com", C.c_void_p),
                ("momentum", C.c_void_p), ("h_gravity", C.c_void_p), ("qdot", C.c_void_p), ("enabled", C.c_void_p),
                ("com_A", C.c_void_p), ("com_A_stride", C.c_longlong), ("com_A_ld", C.c_int),
                ("com_b", C.c_void_p), ("com_b_stride", C.c_longlong),
                ("com_pos_ref", C.c_void_p), ("com_vel_ref", C.c_void_p), ("com_acc_ref", C.c_void_p),
                ("ang_mom_ref", C.c_void_p), ("ang_mom_rate_ref", C.c_void_p),
                ("fb_A", C.c_void_p), ("fb_A_stride", C.c_longlong), ("fb_A_ld", C.c_int),
                ("static_A", C.c_void_p), ("static_A_stride", C.c_longlong), ("static_A_ld", C.c_int),
                ("static_lo", C.c_void_p), ("static_up", C.c_void_p), ("static_b_stride", C.c_longlong),
                ("static_q_tau", C.c_void_p),
                ("cart_b", C.c_void_p), ("cart_b_stride", C.c_longlong),
                ("cart_pose_ref", C.c_void_p), ("cart_vel_ref", C.c_void_p), ("cart_f_des", C.c_void_p),
                ("cart_pose_error", C.c_void_p)]


FEEDBACK_MAX_CART = 8


class FeedbackModel(C.Structure):
    _fields_ = [("nv", C.c_int), ("floating_base", C.c_int), ("n_cart", C.c_int), ("joint", C.c_int), ("imu", C.c_int),
                ("n_pairs", C.c_int), ("n", C.c_int),
                ("cart_C", C.c_double * (6 * FEEDBACK_MAX_CART)), ("cart_deadzone", C.c_double * (6 * FEEDBACK_MAX_CART)),
                ("cart_omega", C.c_double * (6 * FEEDBACK_MAX_CART)), ("cart_damping", C.c_double * (6 * FEEDBACK_MAX_CART)),
                ("cart_ts", C.c_double * FEEDBACK_MAX_CART),
                ("joint_omega", C.c_double), ("joint_damping", C.c_double), ("joint_ts", C.c_double), ("joint_C_scalar", C.c_double),
                ("contact_lambda", C.c_double), ("ca_threshold", C.c_double)]


class FeedbackBatch(C.Structure):
    _fields_ = [("B", C.c_int), ("state", C.c_void_p),
                ("cart_pose", C.c_void_p * FEEDBACK_MAX_CART), ("cart_wrench", C.c_void_p * FEEDBACK_MAX_CART),
                ("cart_wrench_ref", C.c_void_p * FEEDBACK_MAX_CART), ("cart_twist_in", C.c_void_p * FEEDBACK_MAX_CART),
                ("cart_twist_out", C.c_void_p * FEEDBACK_MAX_CART),
                ("joint_tau", C.c_void_p), ("joint_h", C.c_void_p), ("joint_C", C.c_void_p), ("joint_qdot_out", C.c_void_p),
                ("imu_fb_J", C.c_void_p), ("imu_fb_J_stride", C.c_longlong), ("imu_pose", C.c_void_p), ("imu_omega", C.c_void_p),
                ("imu_A", C.c_void_p), ("imu_A_stride", C.c_longlong), ("imu_A_ld", C.c_int),
                ("imu_b", C.c_void_p), ("imu_b_stride", C.c_longlong),
                ("contact_pose", C.c_void_p), ("contact_pose_ref", C.c_void_p), ("contact_b_in", C.c_void_p),
                ("contact_b_in_stride", C.c_longlong), ("contact_b_out", C.c_void_p), ("contact_b_out_stride", C.c_longlong),
                ("ca_J", C.c_void_p), ("ca_J_stride", C.c_longlong), ("ca_dist", C.c_void_p),
                ("ca_A", C.c_void_p), ("ca_A_stride", C.c_longlong), ("ca_A_ld", C.c_int),
                ("ca_b", C.c_void_p), ("ca_b_stride", C.c_longlong)]


ACC_MAX_CART = 8
ACC_GAIN_ACCELERATION, ACC_GAIN_FORCE = 0, 1


class AccModel(C.Structure):
    _fields_ = [("nv", C.c_int), ("n_cart", C.c_int), ("cart_gain_type", C.c_int * ACC_MAX_CART),
                ("cart_gain_matrices", C.c_int * ACC_MAX_CART), ("cart_Kp", C.c_double * (36 * ACC_MAX_CART)),
                ("cart_Kd", C.c_double * (36 * ACC_MAX_CART)), ("cart_orientation_gain", C.c_double * ACC_MAX_CART),
                ("has_com", C.c_int), ("com_gain_matrices", C.c_int), ("com_Kp", C.c_double * 9), ("com_Kd", C.c_double * 9),
                ("has_postural", C.c_int), ("post_gain_type", C.c_int), ("post_gain_matrices", C.c_int),
                ("post_lambda", C.c_double), ("post_lambda2", C.c_double), ("post_Kp", C.c_void_p), ("post_Kd", C.c_void_p)]


class AccBatch(C.Structure):
    _fields_ = [("B", C.c_int), ("q", C.c_void_p), ("qdot", C.c_void_p), ("M", C.c_void_p), ("M_stride", C.c_longlong),
                ("cart_J", C.c_void_p * ACC_MAX_CART), ("cart_J_stride", C.c_longlong * ACC_MAX_CART), ("cart_J_ld", C.c_int * ACC_MAX_CART),
                ("cart_pose", C.c_void_p * ACC_MAX_CART), ("cart_pose_ref", C.c_void_p * ACC_MAX_CART),
                ("cart_vel_ref", C.c_void_p * ACC_MAX_CART), ("cart_f_virtual", C.c_void_p * ACC_MAX_CART),
                ("cart_a_ref_in", C.c_void_p * ACC_MAX_CART), ("cart_p0", C.c_void_p * ACC_MAX_CART),
                ("cart_p0_stride", C.c_longlong * ACC_MAX_CART), ("cart_a_ref_out", C.c_void_p * ACC_MAX_CART),
                ("cart_Mi", C.c_void_p * ACC_MAX_CART),
                ("com_J", C.c_void_p), ("com_J_stride", C.c_longlong), ("com_J_ld", C.c_int),
                ("com", C.c_void_p), ("com_ref", C.c_void_p), ("com_vel_ref", C.c_void_p),
                ("com_p0", C.c_void_p), ("com_p0_stride", C.c_longlong),
                ("post_q_ref", C.c_void_p), ("post_qdot_ref", C.c_void_p), ("post_qddot_ref", C.c_void_p),
                ("post_p0", C.c_void_p), ("post_qddot_out", C.c_void_p),
                ("Minv", C.c_void_p), ("Minv_stride", C.c_longlong), ("ok", C.c_void_p)]


SENS_OK, SENS_DEGENERATE, SENS_SKIPPED = 0, 1, 2


class QpSensOptions(C.Structure):
    _fields_ = [("active_tol", C.c_double), ("dual_tol", C.c_double), ("rank_tol", C.c_double)]


class QpSensBatch(C.Structure):
    _fields_ = [("B", C.c_int), ("n", C.c_int), ("nc", C.c_int),
                ("H", C.c_void_p), ("g", C.c_void_p), ("A", C.c_void_p), ("lA", C.c_void_p), ("uA", C.c_void_p), ("l", C.c_void_p), ("u", C.c_void_p),
                ("eps_abs", C.c_double), ("x", C.c_void_p), ("status", C.c_void_p), ("grad_x", C.c_void_p), ("y", C.c_void_p), ("active", C.c_void_p),
                ("grad_H", C.c_void_p), ("grad_g", C.c_void_p), ("grad_A", C.c_void_p), ("grad_lA", C.c_void_p), ("grad_uA", C.c_void_p),
                ("grad_l", C.c_void_p), ("grad_u", C.c_void_p), ("flag", C.c_void_p)]


class LevelQp(C.Structure):
    _fields_ = [("H", C.c_void_p), ("g", C.c_void_p), ("A", C.c_void_p), ("lA", C.c_void_p), ("uA", C.c_void_p), ("l", C.c_void_p), ("u", C.c_void_p)]


class IhqpSensBatch(C.Structure):
    _fields_ = [("qp", QpBatch), ("y", C.c_void_p * MAX_LEVELS), ("active", C.c_void_p * MAX_LEVELS), ("flag", C.c_void_p * MAX_LEVELS),
                ("objective", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_ulonglong),
                ("grad_dq", C.c_void_p), ("grad_b", C.c_void_p * MAX_LEVELS), ("grad_w", C.c_void_p * MAX_LEVELS),
                ("grad_c", C.c_void_p * MAX_LEVELS), ("grad_A", C.c_void_p * MAX_LEVELS), ("grad_C", C.c_void_p), ("grad_lo", C.c_void_p),
                ("grad_up", C.c_void_p), ("grad_l", C.c_void_p), ("grad_u", C.c_void_p)]


SYMBOLS = [
    "osot_version", "osot_last_error", "osot_device_count",
    "osot_plan_validate", "osot_plan_validate_wide", "osot_solver_create_wide", "osot_plan_level_rows", "osot_plan_constraint_rows",
    "osot_plan_stored_constraint_rows",
    "osot_solver_create", "osot_solver_destroy", "osot_stack_update", "osot_ihqp_solve", "osot_cycle", "osot_nhqp_solve", "osot_ehqp_solve",
    "osot_solver_kernel_time_ms", "osot_solver_set_timing", "osot_solver_set_schedule", "osot_solver_set_hotstart", "osot_solver_set_specialisation", "osot_solver_set_task_active", "osot_solver_resident_waves", "osot_solver_resident_waves_nhqp",
    "osot_id_rows", "osot_force_rows", "osot_acc_tasks", "osot_feedback", "osot_feedback_state_doubles", "osot_admittance_params", "osot_id_force_gains", "osot_computed_torque", "osot_kin_create", "osot_kin_destroy", "osot_kinematics", "osot_pure_rolling_s33", "osot_shape_distance", "osot_dyn_create", "osot_dyn_destroy", "osot_dynamics",
    "osot_grad_create", "osot_grad_destroy", "osot_posture_gradient", "osot_control_cycle", "osot_control_rollout", "osot_solver_profile_phases",
    "osot_backend_create", "osot_backend_destroy", "osot_backend_init_problem",
    "osot_backend_update_task", "osot_backend_update_constraints", "osot_backend_update_bounds",
    "osot_backend_solve", "osot_backend_get_solution", "osot_backend_get_objective",
    "osot_backend_get_options", "osot_backend_set_options",
    "osot_backend_set_eps_regularisation", "osot_backend_get_eps_regularisation",
    "osot_backend_get_num_variables", "osot_backend_get_num_constraints",
    "osot_qp_solve_batch", "osot_qp_solve_batch_admm", "osot_qp_solve_batch_admm_warm",
    "osot_qp_hot_state_ints", "osot_qp_solve_batch_hot", "osot_qp_sensitivity_batch",
    "osot_qp_sens_workspace_bytes", "osot_qp_sensitivity_batch_ws",
    "osot_ihqp_level_rows", "osot_ihqp_level_qp", "osot_ihqp_sens_workspace_bytes", "osot_ihqp_sensitivity",
    "osot_solver_hot_state_ints", "osot_ihqp_solve_hot", "osot_cycle_hot",
    "osot_comm_unique_id", "osot_comm_create", "osot_comm_destroy", "osot_allgather_dq", "osot_abi_layout",
]

# the header's typedef name of every struct mirrored above (osot_abi_layout: tests/test_abi_host.py checks size and every offset)
STRUCTS = {"osot_task_desc": TaskDesc, "osot_level_desc": LevelDesc, "osot_bound_desc": BoundDesc, "osot_rows_desc": RowsDesc,
           "osot_plan_desc": PlanDesc, "osot_qp_batch": QpBatch, "osot_leaf_ptrs": LeafPtrs, "osot_leaf_batch": LeafBatch,
           "osot_assembled_out": AssembledOut, "osot_backend_options": BackendOptions, "osot_nhqp_options": NhqpOptions,
           "osot_admm_options": AdmmOptions, "osot_id_model": IdModel, "osot_kin_desc": KinDesc, "osot_kin_batch": KinBatch,
           "osot_dyn_desc": DynDesc, "osot_dyn_batch": DynBatch, "osot_grad_desc": GradDesc, "osot_grad_batch": GradBatch, "osot_shape": Shape,
           "osot_force_model": ForceModel, "osot_force_batch": ForceBatch,
           "osot_feedback_model": FeedbackModel, "osot_feedback_batch": FeedbackBatch,
           "osot_acc_model": AccModel, "osot_acc_batch": AccBatch,
           "osot_qp_sens_options": QpSensOptions, "osot_qp_sens_batch": QpSensBatch,
           "osot_level_qp": LevelQp, "osot_ihqp_sens_batch": IhqpSensBatch}

_HERE = os.path.dirname(os.path.abspath(__file__))
# (OSOT_MI355X_LIB: developer override, to A/B two builds of the HIP library on the GPU box)
LIB_PATH = os.environ.get("OSOT_MI355X_LIB") or os.path.join(_HERE, "csrc", "libosot_mi355x.so")
_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def lib():
    """Load the HIP library.  There is NO fallback: a missing .so is a hard error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). opensot_amd has no CPU fallback.")
    # torch bundles its own libamdhip64/librccl; import it FIRST so that our library binds to the same
    # (single) HIP runtime instance whose streams and allocations we are handed.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.osot_version.restype = C.c_char_p
    L.osot_last_error.restype = C.c_char_p
    L.osot_device_count.argtypes = [ip]
    L.osot_plan_validate.argtypes = [C.POINTER(PlanDesc)]
    L.osot_plan_validate_wide.argtypes = [C.POINTER(PlanDesc)]   # the workgroup route: 1 <= n <= MAX_QP_VARS
    L.osot_solver_create_wide.argtypes = [C.POINTER(PlanDesc), C.c_int, C.c_int, C.POINTER(vp)]
    L.osot_plan_level_rows.argtypes = [C.POINTER(PlanDesc), C.c_int, ip, ip]
    L.osot_plan_constraint_rows.argtypes = [C.POINTER(PlanDesc), ip]
    L.osot_plan_stored_constraint_rows.argtypes = [C.POINTER(PlanDesc), ip]
    L.osot_solver_create.argtypes = [C.POINTER(PlanDesc), C.c_int, C.c_int, C.POINTER(vp)]
    L.osot_solver_destroy.argtypes = [vp]
    L.osot_stack_update.argtypes = [vp, C.POINTER(LeafBatch), C.POINTER(AssembledOut), vp]
    L.osot_ihqp_solve.argtypes = [vp, C.POINTER(QpBatch), vp]
    L.osot_nhqp_solve.argtypes = [vp, C.POINTER(QpBatch), C.POINTER(NhqpOptions), vp]
    L.osot_ehqp_solve.argtypes = [vp, C.POINTER(QpBatch), C.c_double, vp]
    L.osot_cycle.argtypes = [vp, C.POINTER(LeafBatch), C.POINTER(AssembledOut), C.POINTER(QpBatch), vp]
    L.osot_solver_kernel_time_ms.argtypes = [vp, C.c_int, dp, ip]
    L.osot_solver_set_timing.argtypes = [vp, C.c_int]
    L.osot_solver_set_schedule.argtypes = [vp, C.c_int]
    L.osot_solver_set_hotstart.argtypes = [vp, C.c_int]
    L.osot_solver_hot_state_ints.argtypes = [vp, ip]
    L.osot_ihqp_solve_hot.argtypes = [vp, C.POINTER(QpBatch), vp, vp]
    L.osot_cycle_hot.argtypes = [vp, C.POINTER(LeafBatch), C.POINTER(AssembledOut), C.POINTER(QpBatch), vp, vp]
    L.osot_solver_set_specialisation.argtypes = [vp, C.c_int]
    L.osot_solver_set_task_active.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.osot_solver_resident_waves.argtypes = [vp, ip]
    L.osot_solver_resident_waves_nhqp.argtypes = [vp, vp, ip]
    L.osot_id_force_gains.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, dp, dp, vp, vp, C.c_longlong, vp, vp]
    L.osot_id_rows.argtypes = [C.POINTER(IdModel), vp, C.c_longlong, vp, C.c_longlong, C.c_int, vp, vp, vp, vp, vp]
    L.osot_force_rows.argtypes = [C.POINTER(ForceModel), C.POINTER(ForceBatch), vp]
    L.osot_feedback.argtypes = [C.POINTER(FeedbackModel), C.POINTER(FeedbackBatch), vp]
    L.osot_acc_tasks.argtypes = [C.POINTER(AccModel), C.POINTER(AccBatch), vp]
    L.osot_feedback_state_doubles.argtypes = [C.POINTER(FeedbackModel), ip]
    L.osot_admittance_params.argtypes = [dp, dp, C.c_double, C.c_double, dp, dp, dp]
    L.osot_computed_torque.argtypes = [C.POINTER(IdModel), vp, vp, vp, C.c_double, vp]
    L.osot_kin_create.argtypes = [C.POINTER(KinDesc), C.c_int, C.POINTER(vp)]
    L.osot_kin_destroy.argtypes = [vp]
    L.osot_kinematics.argtypes = [vp, C.POINTER(KinBatch), vp]
    L.osot_pure_rolling_s33.argtypes = [dp, dp, dp]
    L.osot_shape_distance.argtypes = [C.POINTER(Shape), dp, C.POINTER(Shape), dp, dp, dp, dp, ip]
    L.osot_dyn_create.argtypes = [C.POINTER(KinDesc), C.POINTER(DynDesc), C.c_int, C.POINTER(vp)]
    L.osot_dyn_destroy.argtypes = [vp]
    L.osot_dynamics.argtypes = [vp, C.POINTER(DynBatch), vp]
    L.osot_grad_create.argtypes = [C.POINTER(KinDesc), C.POINTER(GradDesc), C.c_int, C.POINTER(vp)]
    L.osot_grad_destroy.argtypes = [vp]
    L.osot_posture_gradient.argtypes = [vp, C.POINTER(GradBatch), vp]
    L.osot_control_cycle.argtypes = [vp, vp, C.POINTER(KinBatch), C.POINTER(LeafBatch), C.POINTER(AssembledOut), C.POINTER(QpBatch), vp, vp]
    L.osot_control_rollout.argtypes = [vp, vp, C.POINTER(KinBatch), C.POINTER(LeafBatch), C.POINTER(AssembledOut), C.POINTER(QpBatch), vp, C.c_int, vp, vp, vp]
    L.osot_solver_profile_phases.argtypes = [vp, C.POINTER(QpBatch), vp, vp]
    L.osot_backend_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(vp)]
    L.osot_backend_destroy.argtypes = [vp]
    L.osot_backend_init_problem.argtypes = [vp, dp, dp, dp, dp, dp, dp, dp]
    L.osot_backend_update_task.argtypes = [vp, dp, dp]
    L.osot_backend_update_constraints.argtypes = [vp, dp, dp, dp, C.c_int]
    L.osot_backend_update_bounds.argtypes = [vp, dp, dp]
    L.osot_backend_solve.argtypes = [vp]
    L.osot_backend_get_solution.argtypes = [vp, dp]
    L.osot_backend_get_objective.argtypes = [vp, dp]
    L.osot_backend_get_options.argtypes = [vp, C.POINTER(BackendOptions)]
    L.osot_backend_set_options.argtypes = [vp, C.POINTER(BackendOptions)]
    L.osot_backend_set_eps_regularisation.argtypes = [vp, C.c_double]
    L.osot_backend_get_eps_regularisation.argtypes = [vp, dp]
    L.osot_backend_get_num_variables.argtypes = [vp, ip]
    L.osot_backend_get_num_constraints.argtypes = [vp, ip]
    L.osot_qp_solve_batch.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                      C.c_double, C.c_int, vp, vp, vp, vp]
    L.osot_qp_hot_state_ints.argtypes = [C.c_int, ip]
    L.osot_qp_solve_batch_hot.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                          C.c_double, C.c_int, vp, vp, vp, vp, vp]
    L.osot_qp_solve_batch_admm.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                           C.c_double, C.c_int, vp, vp, vp, vp]
    L.osot_qp_solve_batch_admm_warm.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                                C.c_double, C.POINTER(AdmmOptions), vp, vp, vp, vp, vp, vp, vp]
    L.osot_qp_sensitivity_batch.argtypes = [C.POINTER(QpSensBatch), C.POINTER(QpSensOptions), vp]
    L.osot_qp_sens_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    L.osot_qp_sensitivity_batch_ws.argtypes = [C.POINTER(QpSensBatch), C.POINTER(QpSensOptions), vp, C.c_size_t, vp]
    L.osot_ihqp_level_rows.argtypes = [vp, C.c_int, ip]
    L.osot_ihqp_level_qp.argtypes = [vp, C.POINTER(QpBatch), C.c_int, C.POINTER(LevelQp), vp]
    L.osot_ihqp_sens_workspace_bytes.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
    L.osot_ihqp_sensitivity.argtypes = [vp, C.POINTER(IhqpSensBatch), C.POINTER(QpSensOptions), vp]
    L.osot_comm_unique_id.argtypes = [vp]
    L.osot_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.osot_comm_destroy.argtypes = [vp]
    L.osot_allgather_dq.argtypes = [vp, vp, vp, C.c_longlong, vp]
    _lib = L
    return L


def check(rc, what=""):
    if rc != OK:
        msg = lib().osot_last_error()
        raise RuntimeError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
