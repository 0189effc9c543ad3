"""tests/force_ref.py -- TEST INFRASTRUCTURE ONLY: what the force-row tests share.

  * the recipe of the host build tests/emu/force_rows_host.cpp (osot_force_rows_kernel through the lock-step emulation, with the
    checks of osot_force_rows), built with native_build's flags, staleness rule and write-then-rename rule; and of the same file
    as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (statically linked runtimes, its own main);
  * a numpy restatement of the five formulas of include/osot_mi355x.h (osot_force_rows), written from the formulas: matrices as
    dense arrays, every b as the list of the TERMS of its sum in numpy.longdouble, from which the tests take the value and the
    forward-error bound (k + 2) 2^-53 sum |terms|, k = the number of terms;
  * random cases, sentinel-filled destinations with gaps between rows and instances, and the run of a case through anything that
    takes the two structs (the host build here, the device library in tests/test_force_rows_gpu.py).
"""
import ctypes as C
import math
import os
import shlex
import subprocess

import numpy as np

from opensot_amd import abi
import native_build

EMU = os.path.join(native_build.ROOT, "tests", "emu")
SOURCE = "force_rows_host.cpp"
LIBRARY = "libosot_force_rows_host.so"
PROGRAM = "force_rows_asan"
SANITIZED = ["g++", "-O1", "-g", "-std=c++17", "-DOSOT_EMULATION", "-DOSOT_FORCE_ROWS_MAIN", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I."] + native_build.INCLUDES
SENTINEL = -7.25e300
U = 2.0 ** -53


# ---- 1. the host builds --------------------------------------------------------------------------------------------------------------
def _ensure(output, command):
    out = os.path.join(EMU, output)
    if native_build.is_stale(out, out + ".d", EMU, recipe=os.path.abspath(__file__)) or \
            os.path.getmtime(native_build.RECIPE) > os.path.getmtime(out):
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
    """build tests/emu/libosot_force_rows_host.so if it is stale (native_build.is_stale), to a temporary name first"""
    return _ensure(LIBRARY, native_build.LOCKSTEP)


def ensure_sanitized():
    """the stand-alone program of the same file (-DOSOT_FORCE_ROWS_MAIN) under ASan + UBSan"""
    return _ensure(PROGRAM, SANITIZED)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(ensure())
        _lib.force_host_check.argtypes = [C.POINTER(abi.ForceModel), C.POINTER(abi.ForceBatch), C.POINTER(C.c_char_p)]
        _lib.force_host_rows.argtypes = [C.POINTER(abi.ForceModel), C.POINTER(abi.ForceBatch)]
    return _lib


def host_check(model, batch):
    """osot_force_rows' answer to its arguments, from the host build -> (code, reason)"""
    why = C.c_char_p()
    rc = lib().force_host_check(C.byref(model), C.byref(batch), C.byref(why))
    return rc, (why.value or b"").decode()


# ---- 2. cases ------------------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    """Rodrigues' formula, row-major 3 x 3"""
    a = np.asarray(axis, dtype=float)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def random_pose(rng, max_angle=math.pi):
    return np.concatenate([rotation(rng.standard_normal(3), rng.uniform(-max_angle, max_angle)).reshape(9), rng.uniform(-1.0, 1.0, 3)])


def make_case(B, C_, nv, wrench_col, torque_col, n, seed=0, enabled="random", refs=True, pose_error=False, qdot=True):
    """the inputs of one osot_force_rows call as host arrays (poses: pose[c] is [B][12])"""
    rng = np.random.default_rng(seed)
    na = nv - 6
    c = dict(B=B, C=C_, nv=nv, n=n, wrench_col=list(wrench_col), torque_col=torque_col, cart_contact=C_ - 1,
             mass=float(rng.uniform(5.0, 80.0)), gravity=np.array([0.0, 0.0, -9.81]),
             com_lambda=float(rng.uniform(1.0, 100.0)), com_lambda2=float(rng.uniform(0.5, 20.0)), com_lambda_ang=float(rng.uniform(0.1, 2.0)),
             cart_Kp=rng.uniform(-50.0, 50.0, (6, 6)), cart_Kd=rng.uniform(-5.0, 5.0, (6, 6)))
    c["pose"] = [np.stack([random_pose(rng) for _ in range(B)]) for _ in range(C_)]
    c["Jc"] = rng.uniform(-1.0, 1.0, (B, C_, 6, nv))
    c["com"] = rng.uniform(-1.0, 1.0, (B, 3))
    c["momentum"] = rng.uniform(-10.0, 10.0, (B, 6))
    c["h_gravity"] = rng.uniform(-100.0, 100.0, (B, nv))
    c["qdot"] = rng.uniform(-1.0, 1.0, (B, nv)) if qdot else None
    if isinstance(enabled, str):
        c["enabled"] = {"random": (rng.uniform(size=(B, C_)) < 0.7).astype(np.int32), "all": np.ones((B, C_), dtype=np.int32), "none": None}[enabled]
    else:
        c["enabled"] = None if enabled is None else np.ascontiguousarray(enabled, dtype=np.int32)
    for name, w in (("com_pos_ref", 3), ("com_vel_ref", 3), ("com_acc_ref", 3), ("ang_mom_ref", 3), ("ang_mom_rate_ref", 3),
                    ("cart_vel_ref", 6), ("cart_f_des", 6)):
        c[name] = rng.uniform(-2.0, 2.0, (B, w)) if refs else None
    c["static_q_tau"] = rng.uniform(-10.0, 10.0, (B, max(na, 1)))[:, :na].copy() if refs else None
    c["cart_pose_ref"] = np.stack([random_pose(rng) for _ in range(B)])
    c["cart_pose_error"] = rng.uniform(-0.5, 0.5, (B, 6)) if pose_error else None
    return c


# the three shapes at which the kernel can go wrong (C, nv, wrench columns, torque column, n, ld):
#   one static row; both column halves with the staging array full; non-contiguous wrench columns off zero with ld > n
SHAPES = {
    "C1_nv7": dict(C_=1, nv=7, wrench_col=[0], torque_col=6, n=7, ld=7),
    "C8_nv64": dict(C_=8, nv=64, wrench_col=[0, 6, 12, 18, 24, 30, 36, 42], torque_col=48, n=106, ld=106),
    "C3_nv35": dict(C_=3, nv=35, wrench_col=[40, 3, 21], torque_col=47, n=80, ld=85),
}


def shape_case(name, B, seed=0, **kw):
    s = dict(SHAPES[name])
    ld = s.pop("ld")
    return make_case(B, seed=seed, **s, **kw), ld


class Outputs:
    """sentinel-filled destinations with a spare row in front of and behind every block, a spare entry around every vector: the
    blocks start at row 1 / entry 1, the strides span the spares"""

    def __init__(self, case, ld, want=("com_A", "com_b", "fb_A", "static_A", "static_b", "cart_b")):
        B, na = case["B"], case["nv"] - 6
        full = lambda *s: np.full(s, SENTINEL)
        self.ld, self.want = ld, tuple(w for w in want if na > 0 or not w.startswith("static"))
        self.com_A, self.fb_A, self.static_A = full(B, 8, ld), full(B, 8, ld), full(B, na + 2, ld)
        self.com_b, self.cart_b = full(B, 8), full(B, 8)
        self.static_lo, self.static_up = full(B, na + 2), full(B, na + 2)

    def arrays(self):
        return {k: getattr(self, k) for k in ("com_A", "fb_A", "static_A", "com_b", "cart_b", "static_lo", "static_up")}


def structs(case, out, address):
    """(abi.ForceModel, abi.ForceBatch) of a case and its Outputs; address(array) -> the address the kernel is given for it"""
    m, b = abi.ForceModel(), abi.ForceBatch()
    m.n_contacts, m.nv, m.n, m.torque_col, m.cart_contact = case["C"], case["nv"], case["n"], case["torque_col"], case["cart_contact"]
    for i, w in enumerate(case["wrench_col"]):
        m.wrench_col[i] = w
    m.mass, m.com_lambda, m.com_lambda2, m.com_lambda_ang = case["mass"], case["com_lambda"], case["com_lambda2"], case["com_lambda_ang"]
    for i in range(3):
        m.gravity[i] = float(case["gravity"][i])
    for i in range(36):
        m.cart_Kp[i], m.cart_Kd[i] = float(case["cart_Kp"].reshape(36)[i]), float(case["cart_Kd"].reshape(36)[i])
    b.B = case["B"]
    for i, p in enumerate(case["pose"]):
        b.pose[i] = address(p)
    for name in ("Jc", "com", "momentum", "h_gravity", "qdot", "enabled"):
        if case[name] is not None:
            setattr(b, name, address(case[name]))
    ld, na = out.ld, case["nv"] - 6
    if "com_A" in out.want:
        b.com_A, b.com_A_stride, b.com_A_ld = address(out.com_A) + 8 * ld, 8 * ld, ld
    if "fb_A" in out.want:
        b.fb_A, b.fb_A_stride, b.fb_A_ld = address(out.fb_A) + 8 * ld, 8 * ld, ld
    if "static_A" in out.want:
        b.static_A, b.static_A_stride, b.static_A_ld = address(out.static_A) + 8 * ld, (na + 2) * ld, ld
    if "static_b" in out.want:
        b.static_lo, b.static_up, b.static_b_stride = address(out.static_lo) + 8, address(out.static_up) + 8, na + 2
        if case["static_q_tau"] is not None:
            b.static_q_tau = address(case["static_q_tau"])
    if "com_b" in out.want:
        b.com_b, b.com_b_stride = address(out.com_b) + 8, 8
        for name in ("com_pos_ref", "com_vel_ref", "com_acc_ref", "ang_mom_ref", "ang_mom_rate_ref"):
            if case[name] is not None:
                setattr(b, name, address(case[name]))
    if "cart_b" in out.want:
        b.cart_b, b.cart_b_stride = address(out.cart_b) + 8, 8
        for name in ("cart_vel_ref", "cart_f_des", "cart_pose_error"):
            if case[name] is not None:
                setattr(b, name, address(case[name]))
        if case["cart_pose_error"] is None:
            b.cart_pose_ref = address(case["cart_pose_ref"])
    return m, b


def run_host(case, ld, want=None):
    """the case through the emulated kernel -> Outputs"""
    out = Outputs(case, ld) if want is None else Outputs(case, ld, want)
    m, b = structs(case, out, lambda a: a.ctypes.data)
    assert lib().force_host_rows(C.byref(m), C.byref(b)) == abi.OK
    return out


# ---- 3. the restatement --------------------------------------------------------------------------------------------------------------
def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def _on(case, i, c):
    return case["enabled"] is None or case["enabled"][i, c] != 0


def written_columns(case, static):
    """the columns of x a destination row receives: the wrench blocks, for the static rows also the torque columns"""
    cols = [w + d for w in case["wrench_col"] for d in range(6)]
    if static and case["torque_col"] >= 0:
        cols += list(range(case["torque_col"], case["torque_col"] + case["nv"] - 6))
    return sorted(cols)


def com_A(case):
    """force::CoM: block c = [I 0; skew(p_c - com) I]"""
    G = np.zeros((case["B"], 6, case["n"]))
    for i in range(case["B"]):
        for c, w in enumerate(case["wrench_col"]):
            if _on(case, i, c):
                G[i, :, w:w + 6] = np.block([[np.eye(3), np.zeros((3, 3))], [skew(case["pose"][c][i, 9:12] - case["com"][i]), np.eye(3)]])
    return G


def fb_A(case):
    """force::FloatingBase: block c = (Jc_c[:, 0:6])'"""
    G = np.zeros((case["B"], 6, case["n"]))
    for i in range(case["B"]):
        for c, w in enumerate(case["wrench_col"]):
            if _on(case, i, c):
                G[i, :, w:w + 6] = case["Jc"][i, c][:, 0:6].T
    return G


def static_A(case):
    """StaticConstraint: block c = (Jc_c[:, 6:nv])', the identity on the torque columns"""
    nv, na, tq = case["nv"], case["nv"] - 6, case["torque_col"]
    G = np.zeros((case["B"], na, case["n"]))
    for i in range(case["B"]):
        for c, w in enumerate(case["wrench_col"]):
            if _on(case, i, c):
                G[i, :, w:w + 6] = case["Jc"][i, c][:, 6:nv].T
        if tq >= 0:
            G[i, :, tq:tq + na] = np.eye(na)
    return G


def static_b(case):
    q = case["static_q_tau"]
    return case["h_gravity"][:, 6:] - (0.0 if q is None else q)


def value_and_bound(terms):
    """terms: a list of longdouble arrays of one shape -> (their sum, (k + 2) 2^-53 sum |terms|)"""
    k = len(terms)
    return sum(terms), (k + 2) * U * sum(np.abs(t) for t in terms)


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def com_b_terms(case):
    """[m (a_d + lambda2 (v_d - v) + lambda (p_d - com) - g); Ldot_d + lambda_ang (L_d - L)] -> (terms of rows 0..2, of rows 3..5),
    each term [B][3]; m v is the linear momentum"""
    m, l1, l2, la = (np.longdouble(case[k]) for k in ("mass", "com_lambda", "com_lambda2", "com_lambda_ang"))
    mom = _ld(case["momentum"])
    lin = [-l2 * mom[:, :3], -m * _ld(case["gravity"])[None, :] * np.ones((case["B"], 1), dtype=np.longdouble)]
    if case["com_acc_ref"] is not None:
        lin.append(m * _ld(case["com_acc_ref"]))
    if case["com_vel_ref"] is not None:
        lin.append(m * l2 * _ld(case["com_vel_ref"]))
    if case["com_pos_ref"] is not None:
        lin += [m * l1 * _ld(case["com_pos_ref"]), -m * l1 * _ld(case["com"])]
    ang = [np.zeros((case["B"], 3), dtype=np.longdouble)]
    if case["ang_mom_rate_ref"] is not None:
        ang.append(_ld(case["ang_mom_rate_ref"]))
    if case["ang_mom_ref"] is not None:
        ang += [la * _ld(case["ang_mom_ref"]), -la * mom[:, 3:]]
    return lin, ang


def rot_to_quat(R):
    """Eigen's Quaterniond(Matrix3d), R row-major [9] -> (x, y, z, w); python floats, one IEEE operation per operator"""
    R = [float(v) for v in R]
    q = [0.0] * 4
    t = R[0] + R[4] + R[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def orientation_error(Ta, Tr):
    """e_o = -2 x (qd.w eps - q.w eps_d + eps_d x eps) on the short path: from the actual to the reference orientation"""
    q, qd = rot_to_quat(Ta[:9]), rot_to_quat(Tr[:9])
    dot = ((q[0] * qd[0] + q[1] * qd[1]) + q[2] * qd[2]) + q[3] * qd[3]
    sg = -1.0 if dot < 0.0 else 1.0
    qx, qy, qz, qw = sg * q[0], sg * q[1], sg * q[2], sg * q[3]
    return np.array([-2.0 * ((qd[3] * qx - qw * qd[0]) + (qd[1] * qz - qd[2] * qy)),
                     -2.0 * ((qd[3] * qy - qw * qd[1]) + (qd[2] * qx - qd[0] * qz)),
                     -2.0 * ((qd[3] * qz - qw * qd[2]) + (qd[0] * qy - qd[1] * qx))])


def pose_error(case):
    """e = [p_ref - p; e_o] of force::Cartesian [B][6] (float64), or the caller's"""
    if case["cart_pose_error"] is not None:
        return case["cart_pose_error"]
    Ta, Tr = case["pose"][case["cart_contact"]], case["cart_pose_ref"]
    return np.stack([np.concatenate([Tr[i, 9:12] - Ta[i, 9:12], orientation_error(Ta[i], Tr[i])]) for i in range(case["B"])])


def cart_b_terms(case):
    """Kp e + Kd (v_ref - J_f qdot) + f_des: the terms of row r, each [B][6] (index r); e is taken as given (float64)"""
    B, nv = case["B"], case["nv"]
    Kp, Kd, e = _ld(case["cart_Kp"]), _ld(case["cart_Kd"]), _ld(pose_error(case))
    terms = [Kp[None, :, j] * e[:, None, j] for j in range(6)]
    if case["cart_f_des"] is not None:
        terms.append(_ld(case["cart_f_des"]))
    if case["cart_vel_ref"] is not None:
        terms += [Kd[None, :, j] * _ld(case["cart_vel_ref"])[:, None, j] for j in range(6)]
    if case["qdot"] is not None:
        J, qd = _ld(case["Jc"][:, case["cart_contact"]]), _ld(case["qdot"])
        terms += [-Kd[None, :, j] * (J[:, j, k] * qd[:, k])[:, None] for j in range(6) for k in range(nv)]
    return terms


# ---- 4. the synth stacks assembled on the host ---------------------------------------------------------------------------------------
def stack_quantities(leaf, model, gravity=(0.0, 0.0, -9.81)):
    """what the producers write for a synth force stack, on the host: the stack's own (no tree) or, for a tree at rest, from
    oracle/pykin.py -- poses and world Jacobians of the contact frames, the CoM, zero momentum, gravity term -M Jcom' g"""
    from oracle import pykin
    f = leaf["force"]
    if model is None:
        return f["quantities"]
    B, nv = leaf["B"], f["nv"]
    assert not np.any(leaf["state"]["qdot0"]), "the host assembly is for a tree at rest"
    frames = [model.frame_index(c) for c in f["contacts"]]
    Q = {"pose": [np.zeros((B, 12)) for _ in frames], "Jc": np.zeros((B, len(frames), 6, nv)), "com": np.zeros((B, 3)),
         "momentum": np.zeros((B, 6)), "h_gravity": np.zeros((B, nv))}
    for i in range(B):
        fk = pykin.forward(model, leaf["state"]["q0"][i])
        for c, fr in enumerate(frames):
            Q["pose"][c][i] = np.concatenate([fk["frame_R"][fr].reshape(9), fk["frame_p"][fr]])
            Q["Jc"][i, c] = fk["J"][fr]
        Q["com"][i] = fk["com"]
        Q["h_gravity"][i] = -f["mass"] * fk["Jcom"].T @ np.asarray(gravity)
    return Q


def stack_case(leaf, Q, n, gravity=(0.0, 0.0, -9.81)):
    """the osot_force_rows case (make_case's layout) of a synth force stack and its model quantities, as ForceStep binds it"""
    f = leaf["force"]
    B = leaf["B"]
    lam, lam2, lam_ang = f["com_gains"]
    z3 = np.zeros((B, 3))
    return dict(B=B, C=len(f["wrench_col"]), nv=f["nv"], n=n, wrench_col=f["wrench_col"], torque_col=f["torque_col"], cart_contact=0,
                mass=f["mass"], gravity=np.asarray(gravity), com_lambda=lam, com_lambda2=lam2, com_lambda_ang=lam_ang,
                cart_Kp=np.eye(6), cart_Kd=np.eye(6), pose=Q["pose"], Jc=Q["Jc"], com=Q["com"], momentum=Q["momentum"],
                h_gravity=Q["h_gravity"], qdot=None, enabled=None, com_pos_ref=Q["com"], com_vel_ref=z3,
                com_acc_ref=f.get("com_acc_ref") if f.get("com_acc_ref") is not None else z3, ang_mom_ref=z3, ang_mom_rate_ref=z3,
                static_q_tau=None, cart_vel_ref=None, cart_f_des=None, cart_pose_ref=None, cart_pose_error=None)


def assemble_stack(plan, leaf, model):
    """the leaf of a synth force stack with every force block filled on the host by the restatement -> (leaf, case)"""
    f = leaf["force"]
    case = stack_case(leaf, stack_quantities(leaf, model), plan.n)
    out = dict(leaf)
    out["A"] = [a.copy() if a is not None else None for a in leaf["A"]]
    out["task"] = [list(lev) for lev in leaf["task"]]
    out["rows"] = list(leaf["rows"])
    lvl, row = f["task"]
    if f["form"] == "com":
        out["A"][lvl][:, row:row + 6] = com_A(case)
        lin, ang = com_b_terms(case)
        b = np.concatenate([sum(lin), sum(ang)], axis=1).astype(np.float64)
    else:
        out["A"][lvl][:, row:row + 6] = fb_A(case)
        b = case["h_gravity"][:, :6].copy()
    out["task"][lvl][f["task_index"]] = (b, None, None)
    if f["static_block"] is not None:
        out["rows"][f["static_block"]] = (static_A(case), static_b(case), static_b(case))
    return out, case
