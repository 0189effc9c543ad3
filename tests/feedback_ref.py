"""tests/feedback_ref.py -- TEST INFRASTRUCTURE ONLY: what the tests of the measurement-driven producer (osot_feedback) share.

  * the recipe of the host build tests/emu/feedback_host.cpp (osot_feedback_kernel through the lock-step emulation, with the checks of
    osot_feedback and its host helpers), built with native_build's flags, staleness rule and write-then-rename rule; and of the same
    file as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (statically linked runtimes, its own main);
  * the numpy restatement of the five formulas of include/osot_mi355x.h (osot_feedback), written from the formulas, twice: in float64
    in the reference's order (one IEEE operation per operator: what the kernel must reproduce bit for bit, the dense C y aside), and
    in numpy.longdouble returning the TERMS of every sum, from which the tests take the value and the forward-error bound;
  * random cases, sentinel-filled destinations with gaps between rows and instances, and the run of a case through anything that
    takes the two structs (the host build here, the device library in tests/test_feedback_gpu.py).
"""
import ctypes as C
import math
import os

import numpy as np

from opensot_amd import abi
import native_build
import force_ref
from force_ref import SENTINEL, U, random_pose, rot_to_quat   # noqa: F401

EMU = os.path.join(native_build.ROOT, "tests", "emu")
SOURCE = "feedback_host.cpp"
LIBRARY = "libosot_feedback_host.so"
PROGRAM = "feedback_asan"
SANITIZED = ["g++", "-O1", "-g", "-std=c++17", "-DOSOT_EMULATION", "-DOSOT_FEEDBACK_MAIN", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I."] + native_build.INCLUDES
LD = np.longdouble


# ---- 1. the host builds --------------------------------------------------------------------------------------------------------------
def _ensure(output, command):
    out = os.path.join(EMU, output)
    if native_build.is_stale(out, out + ".d", EMU, recipe=os.path.abspath(__file__)) or \
            os.path.getmtime(native_build.RECIPE) > os.path.getmtime(out):
        import shlex
        import subprocess
        tmp = f"{output}.tmp.{os.getpid()}"
        cmd = command + [SOURCE, "-MMD", "-MF", output + ".d", "-o", tmp]
        print(shlex.join(cmd), flush=True)
        try:
            subprocess.check_call(cmd, cwd=EMU)
            os.replace(os.path.join(EMU, tmp), out)
        finally:
            if os.path.exists(os.path.join(EMU, tmp)):
                os.remove(os.path.join(EMU, tmp))
    return out


def ensure():
    """build tests/emu/libosot_feedback_host.so if it is stale (native_build.is_stale), to a temporary name first"""
    return _ensure(LIBRARY, native_build.LOCKSTEP)


def ensure_sanitized():
    """the stand-alone program of the same file (-DOSOT_FEEDBACK_MAIN) under ASan + UBSan"""
    return _ensure(PROGRAM, SANITIZED)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(ensure())
        mp, bp = C.POINTER(abi.FeedbackModel), C.POINTER(abi.FeedbackBatch)
        _lib.feedback_host_check.argtypes = [mp, bp, C.POINTER(C.c_char_p)]
        _lib.feedback_host_run.argtypes = [mp, bp]
        _lib.feedback_host_coeff.argtypes = [C.c_double, C.c_double, C.c_double, abi.dp]
        _lib.feedback_host_coeff.restype = None
        _lib.feedback_host_state_doubles.argtypes = [mp]
        _lib.feedback_host_admittance_params.argtypes = [abi.dp, abi.dp, C.c_double, C.c_double, abi.dp, abi.dp, abi.dp, C.POINTER(C.c_char_p)]
    return _lib


def host_check(model, batch):
    """osot_feedback's answer to its arguments, from the host build -> (code, reason)"""
    why = C.c_char_p()
    rc = lib().feedback_host_check(C.byref(model), C.byref(batch), C.byref(why))
    return rc, (why.value or b"").decode()


def host_coeff(omega, eps, ts):
    """(a0, a1, a2, 1 / a0) as osot_feedback computes them on the host"""
    out = np.zeros(4)
    lib().feedback_host_coeff(omega, eps, ts, out.ctypes.data_as(abi.dp))
    return out


def host_admittance_params(K, D, lam, dt):
    """osot_admittance_params from the host build -> (code, reason, C, M, w)"""
    K, D = np.ascontiguousarray(K, dtype=float), np.ascontiguousarray(D, dtype=float)
    Cc, M, w = np.full(6, SENTINEL), np.full(6, SENTINEL), np.full(6, SENTINEL)
    why = C.c_char_p()
    p = lambda a: a.ctypes.data_as(abi.dp)
    rc = lib().feedback_host_admittance_params(p(K), p(D), lam, dt, p(Cc), p(M), p(w), C.byref(why))
    return rc, (why.value or b"").decode(), Cc, M, w


# ---- 2. cases ------------------------------------------------------------------------------------------------------------------------
def make_case(B, nv, n_cart=0, n_pairs=0, n=None, dense=False, joint=True, floating_base=1, imu=True, contact=True, seed=0, refs=True):
    """the inputs of one osot_feedback call as host arrays"""
    rng = np.random.default_rng(seed)
    n = nv if n is None else n
    c = dict(B=B, nv=nv, floating_base=floating_base, n_cart=n_cart, joint=int(joint), imu=int(imu and nv >= 6), n_pairs=n_pairs, n=n,
             contact=contact,
             cart_C=rng.uniform(1e-4, 1e-2, (n_cart, 6)), cart_deadzone=rng.uniform(0.0, 0.5, (n_cart, 6)),
             cart_omega=rng.uniform(5.0, 60.0, (n_cart, 6)), cart_damping=rng.uniform(0.5, 1.5, (n_cart, 6)),
             cart_ts=rng.uniform(0.001, 0.01, n_cart),
             joint_omega=2.0 * math.pi * 8.0, joint_damping=1.0, joint_ts=0.002, joint_C_scalar=0.00015,
             contact_lambda=float(rng.uniform(0.1, 1.0)), ca_threshold=0.01)
    c["cart_pose"] = [np.stack([random_pose(rng) for _ in range(B)]) for _ in range(n_cart)]
    c["cart_wrench"] = [rng.uniform(-2.0, 2.0, (B, 6)) for _ in range(n_cart)]
    c["cart_wrench_ref"] = [rng.uniform(-0.5, 0.5, (B, 6)) if refs else None for _ in range(n_cart)]
    c["cart_twist_in"] = [rng.uniform(-0.1, 0.1, (B, 6)) if refs else None for _ in range(n_cart)]
    c["joint_tau"], c["joint_h"] = rng.uniform(-30.0, 30.0, (B, nv)), rng.uniform(-30.0, 30.0, (B, nv))
    c["joint_C"] = rng.uniform(-1e-3, 1e-3, (nv, nv)) if dense else None
    c["imu_fb_J"] = rng.uniform(-1.0, 1.0, (B, 6, nv))
    c["imu_pose"] = np.stack([random_pose(rng) for _ in range(B)])
    c["imu_omega"] = rng.uniform(-2.0, 2.0, (B, 3))
    c["contact_pose"] = np.stack([random_pose(rng) for _ in range(B)])
    c["contact_pose_ref"] = np.stack([random_pose(rng) for _ in range(B)])
    c["contact_pose"][:, 9:] *= 2.0
    c["contact_pose_ref"][:, 9:] *= 2.0
    c["contact_b_in"] = rng.uniform(-1.0, 1.0, (B, 6))
    c["ca_J"] = rng.uniform(-1.0, 1.0, (B, max(n_pairs, 1), n))[:, :n_pairs].copy()
    d = rng.uniform(-0.05, 0.08, (B, max(n_pairs, 1)))[:, :n_pairs].copy()
    d.reshape(-1)[::3] = c["ca_threshold"]              # err == 0 exactly on every third pair
    c["ca_dist"] = d
    return c


def state_count(case):
    return 4 * (6 * case["n_cart"] + (case["nv"] if case["joint"] else 0))


class Outputs:
    """sentinel-filled destinations: the row blocks with a spare row in front of and behind them and `pad` spare columns, the strided
    vectors with a spare entry around them (the blocks start at row 1 / entry 1, the strides span the spares); the dense outputs
    (twists, joint velocities) are written whole"""

    def __init__(self, case, pad=0):
        B, nv, P = case["B"], case["nv"], case["n_pairs"]
        full = lambda *s: np.full(s, SENTINEL)
        self.pad, self.ld, self.imu_ld = pad, case["n"] + pad, 6 + pad
        self.cart_twist_out = [full(B, 6) for _ in range(case["n_cart"])]
        self.joint_qdot_out = full(B, nv)
        self.imu_A, self.imu_b = full(B, 8, self.imu_ld), full(B, 8)
        self.contact_b_out = full(B, 8)
        self.ca_A, self.ca_b = full(B, P + 2, self.ld), full(B, P + 2)

    def arrays(self):
        d = {k: getattr(self, k) for k in ("joint_qdot_out", "imu_A", "imu_b", "contact_b_out", "ca_A", "ca_b")}
        d.update({f"cart_twist_out{t}": a for t, a in enumerate(self.cart_twist_out)})
        return d


def model_struct(case):
    m = abi.FeedbackModel()
    for k in ("nv", "floating_base", "n_cart", "joint", "imu", "n_pairs", "n"):
        setattr(m, k, int(case[k]))
    for k in ("cart_C", "cart_deadzone", "cart_omega", "cart_damping"):
        for i, v in enumerate(np.asarray(case[k]).reshape(-1)):
            getattr(m, k)[i] = float(v)
    for t in range(case["n_cart"]):
        m.cart_ts[t] = float(case["cart_ts"][t])
    for k in ("joint_omega", "joint_damping", "joint_ts", "joint_C_scalar", "contact_lambda", "ca_threshold"):
        setattr(m, k, float(case[k]))
    return m


def structs(case, out, state, address):
    """(abi.FeedbackModel, abi.FeedbackBatch) of a case, its Outputs and its state; address(array) -> the address the kernel is given"""
    m, b = model_struct(case), abi.FeedbackBatch()
    b.B, nv, P = case["B"], case["nv"], case["n_pairs"]
    if state is not None and state.size:
        b.state = address(state)
    for t in range(case["n_cart"]):
        b.cart_pose[t], b.cart_wrench[t], b.cart_twist_out[t] = address(case["cart_pose"][t]), address(case["cart_wrench"][t]), address(out.cart_twist_out[t])
        if case["cart_wrench_ref"][t] is not None:
            b.cart_wrench_ref[t] = address(case["cart_wrench_ref"][t])
        if case["cart_twist_in"][t] is not None:
            b.cart_twist_in[t] = address(case["cart_twist_in"][t])
    if case["joint"]:
        b.joint_tau, b.joint_h, b.joint_qdot_out = address(case["joint_tau"]), address(case["joint_h"]), address(out.joint_qdot_out)
        if case["joint_C"] is not None:
            b.joint_C = address(case["joint_C"])
    if case["imu"]:
        b.imu_fb_J, b.imu_fb_J_stride, b.imu_pose, b.imu_omega = address(case["imu_fb_J"]), 6 * nv, address(case["imu_pose"]), address(case["imu_omega"])
        b.imu_A, b.imu_A_stride, b.imu_A_ld = address(out.imu_A) + 8 * out.imu_ld, 8 * out.imu_ld, out.imu_ld
        b.imu_b, b.imu_b_stride = address(out.imu_b) + 8, 8
    if case["contact"]:
        b.contact_pose, b.contact_pose_ref = address(case["contact_pose"]), address(case["contact_pose_ref"])
        b.contact_b_in, b.contact_b_in_stride = address(case["contact_b_in"]), 6
        b.contact_b_out, b.contact_b_out_stride = address(out.contact_b_out) + 8, 8
    if P > 0:
        b.ca_J, b.ca_J_stride, b.ca_dist = address(case["ca_J"]), P * case["n"], address(case["ca_dist"])
        b.ca_A, b.ca_A_stride, b.ca_A_ld = address(out.ca_A) + 8 * out.ld, (P + 2) * out.ld, out.ld
        b.ca_b, b.ca_b_stride = address(out.ca_b) + 8, P + 2
    return m, b


def run_host(case, state, pad=0, calls=1):
    """the case through the emulated kernel `calls` times; state [B][count] is advanced in place -> Outputs"""
    out = Outputs(case, pad)
    m, b = structs(case, out, state, lambda a: a.ctypes.data)
    for _ in range(calls):
        assert lib().feedback_host_run(C.byref(m), C.byref(b)) == abi.OK
    return out


# ---- 3. the restatement --------------------------------------------------------------------------------------------------------------
def filter_coeff(omega, eps, ts, dtype=np.float64):
    """computeCoeff (CartesianAdmittance.h:115-124) -> (a0, a1, a2); arrays or scalars of `dtype`"""
    omega, eps, ts = (np.asarray(v, dtype=dtype) for v in (omega, eps, ts))
    one, two, four, eight = (dtype(v) for v in (1.0, 2.0, 4.0, 8.0))
    p = np.power(omega * ts, two) if dtype is not np.float64 else np.vectorize(math.pow)(omega * ts, 2.0)
    a0 = one + four * eps / (omega * ts) + four / p
    a1 = two - eight / p
    a2 = one + four / p - four * eps / (omega * ts)
    return a0, a1, a2


def filter_step(s, e, a0, a1, a2):
    """one process() on the stored (u, ud, y, yd), float64, the reference's order: -> (new (u, ud, y, yd), y)"""
    u, ud, y, yd = s
    ydd, yd, udd, ud = yd, y, ud, u
    ynew = (1.0 / a0) * ((((e + 2.0 * ud) + 1.0 * udd) - a1 * yd) - a2 * ydd)
    return (e, ud, ynew, yd), ynew


def filter_terms(s, e, a0, a1, a2):
    """the same step in longdouble from the float64 state and coefficients: the 5 terms of a0 * y"""
    u, ud, y, yd = (np.asarray(v, dtype=LD) for v in s)
    a0, a1, a2, e = (np.asarray(v, dtype=LD) for v in (a0, a1, a2, e))
    return [e, LD(2.0) * u, LD(1.0) * ud, -a1 * y, -a2 * yd], a0


def deadzone(e, dz):
    return np.where(e > dz, e - dz, np.where(e < -dz, e + dz, 0.0))


def rotate_wrench(pose, w):
    """[R f; R m], each entry (R_r0 v_0 + R_r1 v_1) + R_r2 v_2"""
    R = pose[:, :9].reshape(-1, 3, 3)
    rot = lambda v: (R[:, :, 0] * v[:, 0:1] + R[:, :, 1] * v[:, 1:2]) + R[:, :, 2] * v[:, 2:3]
    return np.concatenate([rot(w[:, :3]), rot(w[:, 3:])], axis=1)


def contact_error(Ta, Tr):
    """[p_d - p; -e_o], float64 in the kernel's order"""
    q, qd = rot_to_quat(Ta[:9]), rot_to_quat(Tr[:9])
    dot = ((q[0] * qd[0] + q[1] * qd[1]) + q[2] * qd[2]) + q[3] * qd[3]
    sg = -1.0 if dot < 0.0 else 1.0
    qx, qy, qz, qw = sg * q[0], sg * q[1], sg * q[2], sg * q[3]
    return np.array([Tr[9] - Ta[9], Tr[10] - Ta[10], Tr[11] - Ta[11],
                     -((qd[3] * qx - qw * qd[0]) + (qd[1] * qz - qd[2] * qy)),
                     -((qd[3] * qy - qw * qd[1]) + (qd[2] * qx - qd[0] * qz)),
                     -((qd[3] * qz - qw * qd[2]) + (qd[0] * qy - qd[1] * qx))])


def _quat_ld(R):
    """Eigen's Quaterniond(Matrix3d) in longdouble"""
    R = [LD(v) for v in R]
    q = [LD(0.0)] * 4
    t = R[0] + R[4] + R[8]
    if t > 0:
        t = np.sqrt(t + LD(1.0))
        q[3] = LD(0.5) * t
        t = LD(0.5) / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + LD(1.0))
        q[i] = LD(0.5) * t
        t = LD(0.5) / t
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def contact_error_ld(Ta, Tr):
    """the same 6-vector in longdouble"""
    q, qd = _quat_ld(Ta[:9]), _quat_ld(Tr[:9])
    sg = LD(-1.0) if sum(a * b for a, b in zip(q, qd)) < 0 else LD(1.0)
    x, y, z, w = (sg * v for v in q)
    eo = [qd[3] * x - w * qd[0] + (qd[1] * z - qd[2] * y), qd[3] * y - w * qd[1] + (qd[2] * x - qd[0] * z), qd[3] * z - w * qd[2] + (qd[0] * y - qd[1] * x)]
    return np.array([LD(Tr[9 + i]) - LD(Ta[9 + i]) for i in range(3)] + [-v for v in eo], dtype=LD)


def cart_views(case, state):
    """term t -> its (u, ud, y, yd) as [B][6] views of state"""
    return [tuple(state[:, 24 * t + 6 * k:24 * t + 6 * k + 6] for k in range(4)) for t in range(case["n_cart"])]


def joint_views(case, state):
    nv, o = case["nv"], 24 * case["n_cart"]
    return tuple(state[:, o + nv * k:o + nv * (k + 1)] for k in range(4))


def step(case, state):
    """one osot_feedback call in float64, the reference's order; state [B][count] is advanced in place -> dict of the outputs (dense
    blocks: cart_twist_out[t] [B][6], joint_qdot_out [B][nv], imu_A [B][6][6], imu_b, contact_b_out [B][6], ca_A [B][P][n], ca_b)"""
    B, nv, r = case["B"], case["nv"], {}
    r["cart_twist_out"] = []
    for t, views in enumerate(cart_views(case, state)):
        e = deadzone(rotate_wrench(case["cart_pose"][t], case["cart_wrench"][t]), case["cart_deadzone"][t][None, :])
        e = e - (case["cart_wrench_ref"][t] if case["cart_wrench_ref"][t] is not None else 0.0)
        a0, a1, a2 = filter_coeff(case["cart_omega"][t], case["cart_damping"][t], case["cart_ts"][t])
        new, y = filter_step(tuple(v.copy() for v in views), e, a0[None, :], a1[None, :], a2[None, :])
        for v, nw in zip(views, new):
            v[...] = nw
        tin = case["cart_twist_in"][t]
        r["cart_twist_out"].append((tin if tin is not None else 0.0) + case["cart_C"][t][None, :] * y)
    if case["joint"]:
        views = joint_views(case, state)
        a0, a1, a2 = (float(v) for v in filter_coeff(case["joint_omega"], case["joint_damping"], case["joint_ts"]))
        new, y = filter_step(tuple(v.copy() for v in views), case["joint_h"] - case["joint_tau"], a0, a1, a2)
        for v, nw in zip(views, new):
            v[...] = nw
        r["joint_y"] = y
        # dense: NOT the kernel's bits (the kernel's row is one fma chain); the tests bound it through joint_terms
        qd = case["joint_C_scalar"] * y if case["joint_C"] is None else y @ case["joint_C"].T
        if case["floating_base"]:
            qd[:, :6] = 0.0
        r["joint_qdot_out"] = qd
    if case["imu"]:
        A = np.zeros((B, 6, 6))
        A[:, 3:6, :] = case["imu_fb_J"][:, 3:6, 0:6]
        R, w = case["imu_pose"][:, :9].reshape(B, 3, 3), case["imu_omega"]
        r["imu_A"] = A
        r["imu_b"] = np.concatenate([np.zeros((B, 3)), (R[:, :, 0] * w[:, 0:1] + R[:, :, 1] * w[:, 1:2]) + R[:, :, 2] * w[:, 2:3]], axis=1)
    if case["contact"]:
        err = np.stack([contact_error(case["contact_pose"][i], case["contact_pose_ref"][i]) for i in range(B)])
        r["contact_b_out"] = case["contact_b_in"] + case["contact_lambda"] * err
    if case["n_pairs"] > 0:
        err = case["ca_dist"] - case["ca_threshold"]
        r["ca_A"] = np.where((err > 0.0)[:, :, None], 0.0, -case["ca_J"])
        r["ca_b"] = np.where(err > 0.0, 0.0, err)
    return r


def joint_terms(case, y):
    """dense C y: the nv terms C_ij y_j of row i, each [B][nv] (index i), longdouble"""
    Cm, y = np.asarray(case["joint_C"], dtype=LD), np.asarray(y, dtype=LD)
    return [Cm[None, :, j] * y[:, j:j + 1] for j in range(case["nv"])]


def check_outputs(got, ref, case, what=("cart", "joint", "imu", "contact", "ca")):
    """an Outputs against step()'s dict: the written entries bit for bit (the dense C y aside: left to the caller), the sentinels of
    every column, row gap and instance gap that is not written still in place"""
    P, n = case["n_pairs"], case["n"]
    if "cart" in what:
        for t in range(case["n_cart"]):
            assert np.array_equal(got.cart_twist_out[t], ref["cart_twist_out"][t]), ("cart_twist_out", t)
    if "joint" in what and case["joint"] and case["joint_C"] is None:
        assert np.array_equal(got.joint_qdot_out, ref["joint_qdot_out"]), "joint_qdot_out"
    if case["imu"] and "imu" in what:
        assert np.array_equal(got.imu_A[:, 1:7, 0:6], ref["imu_A"]), "imu_A"
        a = got.imu_A.copy()
        a[:, 1:7, 0:6] = SENTINEL
        assert (a == SENTINEL).all(), "imu_A: a sentinel was overwritten"
        assert np.array_equal(got.imu_b[:, 1:7], ref["imu_b"]), "imu_b"
        assert (got.imu_b[:, [0, 7]] == SENTINEL).all(), "imu_b: a sentinel was overwritten"
    else:
        assert (got.imu_A == SENTINEL).all() and (got.imu_b == SENTINEL).all()
    if case["contact"] and "contact" in what:
        assert np.array_equal(got.contact_b_out[:, 1:7], ref["contact_b_out"]), "contact_b_out"
        assert (got.contact_b_out[:, [0, 7]] == SENTINEL).all(), "contact_b_out: a sentinel was overwritten"
    if P > 0 and "ca" in what:
        assert np.array_equal(got.ca_A[:, 1:1 + P, :n], ref["ca_A"]), "ca_A"
        a = got.ca_A.copy()
        a[:, 1:1 + P, :n] = SENTINEL
        assert (a == SENTINEL).all(), "ca_A: a sentinel was overwritten"
        assert np.array_equal(got.ca_b[:, 1:1 + P], ref["ca_b"]), "ca_b"
        assert (got.ca_b[:, [0, P + 1]] == SENTINEL).all(), "ca_b: a sentinel was overwritten"
