"""tests/acc_ref.py -- TEST INFRASTRUCTURE ONLY: what the acceleration-leaf tests share.

  * the recipe of the host build tests/emu/acc_tasks_host.cpp (osot_acc_tasks_kernel through the lock-step emulation, with the
    checks of osot_acc_tasks), built with native_build's flags, staleness rule and write-then-rename rule; and of the same file as
    a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (statically linked runtimes, its own main);
  * a numpy restatement of the formulas of include/osot_mi355x.h (osot_acc_tasks) by the SAME ROUTE (M = L L', triangular solves,
    Mi = Y'Y, Minv = Z'Z), in any dtype: float64 is the restatement, numpy.longdouble the arbiter;
  * cases (M from tests/dyn_ref.py on the trees of tests/tree_cases.py, or a synthetic SPD matrix of a given condition number),
    sentinel-fenced destinations, NaN in everything that must not be read, and the run of a case through anything that takes the
    two structs (the host build here, the device library in tests/test_acc_tasks_gpu.py).

THE TOLERANCE of every output that comes from the Cholesky factor (Mi, Gp, Gd, a_ref_out, qddot_out, Minv): the deviation from the
arbiter is stated as  max|X - X*| / (cond2(M) max|X*|)  per instance and output.  RESTATEMENT_WORST is the worst such figure of the
float64 restatement over the committed cases (measured here on the CPU by `python tests/acc_ref.py`), CHOLESKY_TOL is 10 x that:
the margin PARITY_TOL of the posture gradient takes for a different summation order.  EMULATED_WORST is what the emulated kernel
showed in the same run (fma chains: fewer roundings than numpy's dot products)."""
import ctypes as C
import os
import shlex
import subprocess

import numpy as np

from opensot_amd import abi
import native_build
from force_ref import SENTINEL, U, orientation_error, random_pose, value_and_bound  # noqa: F401  (shared with the tests)

EMU = os.path.join(native_build.ROOT, "tests", "emu")
SOURCE = "acc_tasks_host.cpp"
LIBRARY = "libosot_acc_tasks_host.so"
PROGRAM = "acc_tasks_asan"
SANITIZED = ["g++", "-O1", "-g", "-std=c++17", "-DOSOT_EMULATION", "-DOSOT_ACC_TASKS_MAIN", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I."] + native_build.INCLUDES
ACC, FORCE = abi.ACC_GAIN_ACCELERATION, abi.ACC_GAIN_FORCE

# measured on the CPU over CASES (python tests/acc_ref.py prints both), in units of cond2(M) max|X*|
RESTATEMENT_WORST = 3.93e-16
EMULATED_WORST = 2.74e-16
CHOLESKY_TOL = 10.0 * RESTATEMENT_WORST


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
    """build tests/emu/libosot_acc_tasks_host.so if it is stale (native_build.is_stale), to a temporary name first"""
    return _ensure(LIBRARY, native_build.LOCKSTEP)


def ensure_sanitized():
    """the stand-alone program of the same file (-DOSOT_ACC_TASKS_MAIN) under ASan + UBSan"""
    return _ensure(PROGRAM, SANITIZED)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(ensure())
        _lib.acc_host_check.argtypes = [C.POINTER(abi.AccModel), C.POINTER(abi.AccBatch), C.POINTER(C.c_char_p)]
        _lib.acc_host_tasks.argtypes = [C.POINTER(abi.AccModel), C.POINTER(abi.AccBatch)]
        _lib.acc_host_pivot_rel.argtypes = [C.c_int]
        _lib.acc_host_pivot_rel.restype = C.c_double
    return _lib


def host_check(model, batch):
    """osot_acc_tasks' answer to its arguments, from the host build -> (code, reason)"""
    why = C.c_char_p()
    rc = lib().acc_host_check(C.byref(model), C.byref(batch), C.byref(why))
    return rc, (why.value or b"").decode()


def pivot_rel(nv):
    """the relative pivot threshold of osot_acc.h: (nv + 1) 2^-52"""
    return (nv + 1) * 2.0 ** -52


# ---- 2. cases ------------------------------------------------------------------------------------------------------------------------
def tree_M(nv, B, topology="random", seed=0):
    """[B][nv][nv] inertia matrices of a tree of tests/tree_cases.py at B postures, by the restatement tests/dyn_ref.py"""
    import dyn_ref
    import tree_cases
    m = tree_cases.tree_case(nv, topology, seed)
    q = tree_cases.draw_q(m, B, seed)
    M = np.stack([dyn_ref.Ref(m, q[i]).inertia_matrix() for i in range(B)])
    return 0.5 * (M + np.transpose(M, (0, 2, 1)))


def spd_M(nv, B, cond, seed=0):
    """[B][nv][nv] Q diag(s) Q' with singular values log-spaced from 1 to 1 / cond: cond2 = cond up to rounding"""
    rng = np.random.default_rng([nv, seed, 91])
    out = np.zeros((B, nv, nv))
    for i in range(B):
        Q, _ = np.linalg.qr(rng.standard_normal((nv, nv)))
        s = np.logspace(0.0, -np.log10(cond), nv) if nv > 1 else np.ones(1)
        M = (Q * s) @ Q.T
        out[i] = 0.5 * (M + M.T)
    return out


def make_case(B, nv, cart=(), com=None, post=None, M=None, minv=False, ld_pad=0, seed=0, refs=True):
    """the inputs of one osot_acc_tasks call as host arrays.
    cart: one (gain_type, gain_matrices) per term; com: None or gain_matrices; post: None or (gain_type, gain_matrices);
    ld_pad: the Jacobian rows are ld = nv + ld_pad long and lie at row 1 of an 8-row (CoM: 5-row) block, as inside a wider A_k;
    refs=False: every optional input is left out (NULL)"""
    rng = np.random.default_rng([B, nv, len(cart), seed])
    ld = nv + ld_pad

    def jac(rows):
        J = rng.uniform(-1.0, 1.0, (B, rows + 2, ld))
        J[:, :, nv:] = np.nan                      # columns nv .. ld-1 are not read
        return J

    c = dict(B=B, nv=nv, ld=ld, minv=minv, q=rng.uniform(-1.0, 1.0, (B, nv)), qdot=rng.uniform(-1.0, 1.0, (B, nv)), M=M, cart=[], com=None, post=None)
    opt = (lambda a: a) if refs else (lambda a: None)
    for gt, gm in cart:
        c["cart"].append(dict(gain_type=gt, gain_matrices=gm, Kp=rng.uniform(-50.0, 50.0, (6, 6)), Kd=rng.uniform(-5.0, 5.0, (6, 6)),
                              og=float(rng.uniform(0.2, 2.0)), J=jac(6), pose=np.stack([random_pose(rng) for _ in range(B)]),
                              pose_ref=np.stack([random_pose(rng) for _ in range(B)]), vel_ref=opt(rng.uniform(-2.0, 2.0, (B, 6))),
                              f_virtual=opt(rng.uniform(-20.0, 20.0, (B, 6))) if gt == FORCE else None,
                              a_ref_in=opt(rng.uniform(-2.0, 2.0, (B, 6)))))
    if com is not None:
        c["com"] = dict(gain_matrices=com, Kp=rng.uniform(-50.0, 50.0, (3, 3)), Kd=rng.uniform(-5.0, 5.0, (3, 3)), J=jac(3),
                        com=rng.uniform(-1.0, 1.0, (B, 3)), com_ref=rng.uniform(-1.0, 1.0, (B, 3)), vel_ref=opt(rng.uniform(-1.0, 1.0, (B, 3))))
    if post is not None:
        gt, gm = post
        c["post"] = dict(gain_type=gt, gain_matrices=gm, lam=float(rng.uniform(1.0, 100.0)), lam2=float(rng.uniform(0.5, 20.0)),
                         Kp=rng.uniform(-5.0, 5.0, (nv, nv)) if gm and refs else None, Kd=rng.uniform(-1.0, 1.0, (nv, nv)) if gm and refs else None,
                         q_ref=rng.uniform(-1.0, 1.0, (B, nv)), qdot_ref=opt(rng.uniform(-1.0, 1.0, (B, nv))),
                         qddot_ref=opt(rng.uniform(-1.0, 1.0, (B, nv))))
    return c


def needs_M(case):
    return case["minv"] or any(t["gain_type"] == FORCE for t in case["cart"]) or (case["post"] is not None and case["post"]["gain_type"] == FORCE)


def has_gains(term):
    return bool(term["gain_matrices"]) or term["gain_type"] == FORCE


# the shapes at which the kernel can go wrong: name -> (B, make_case arguments, the source of M)
#   nv = 1 postural only; nv = 7; nv = 35 (COMAN's size); nv = 64 with the most right-hand sides (8 x 6 + 1) and the full second
#   pass; B = 1, 3, 257; rows inside a wider A_k; NULL optional inputs; once cond2(M) = 1e8
F1, A1, A0 = (FORCE, 1), (ACC, 1), (ACC, 0)
CASES = {
    "nv1_postural": dict(B=3, nv=1, post=F1, minv=True, M=("tree", "chain")),
    "nv7": dict(B=257, nv=7, cart=[F1, A0], com=0, post=F1, minv=True, ld_pad=3, M=("tree", "chain")),
    "nv7_null_inputs": dict(B=1, nv=7, cart=[F1, A1], com=1, post=A1, refs=False, M=("tree", "star")),
    "nv35": dict(B=3, nv=35, cart=[A0, F1, A1], com=1, post=F1, minv=True, ld_pad=13, M=("tree", "random")),
    "nv35_cond1e8": dict(B=3, nv=35, cart=[F1], post=F1, minv=True, M=("spd", 1e8)),
    "nv64_full": dict(B=3, nv=64, cart=[F1] * 8, com=1, post=F1, minv=True, M=("tree", "forest")),
    "nv64_no_M": dict(B=1, nv=64, cart=[A1, A0], com=0, post=A1, M=None),
}


def named_case(name):
    s = dict(CASES[name])
    src = s.pop("M")
    M = None
    if src is not None:
        M = tree_M(s["nv"], s["B"], src[1]) if src[0] == "tree" else spd_M(s["nv"], s["B"], src[1])
    return make_case(M=M, **s)


# ---- 3. destinations, structs, the run ------------------------------------------------------------------------------------------------
PAD = 2


class Outputs:
    """sentinel-filled destinations: PAD spare doubles in front of and behind every instance of a strided output, and around the
    whole of a dense one; `want` names the outputs that are bound (the others stay NULL and must stay sentinels)"""

    ALL = ("cart_p0", "cart_a_ref_out", "cart_Mi", "com_p0", "post_p0", "post_qddot_out", "Minv", "ok")

    def __init__(self, case, want=ALL):
        B, nv = case["B"], case["nv"]
        full = lambda *s: np.full(s, SENTINEL)
        self.want = tuple(want)
        self.cart_p0 = [full(B, (84 if has_gains(t) else 12) + 2 * PAD) for t in case["cart"]]
        self.cart_a_ref_out = [full(B * 6 + 2 * PAD) for _ in case["cart"]]
        self.cart_Mi = [full(B * 36 + 2 * PAD) for _ in case["cart"]]
        self.com_p0 = full(B, (24 if case["com"] and case["com"]["gain_matrices"] else 6) + 2 * PAD)
        self.post_p0 = full(B * 2 * nv + 2 * PAD)
        self.post_qddot_out = full(B * nv + 2 * PAD)
        self.Minv = full(B, nv * nv + 2 * PAD)
        self.ok = np.full(B + 2, -7, dtype=np.int32)

    def arrays(self):
        return [self.com_p0, self.post_p0, self.post_qddot_out, self.Minv, self.ok] + self.cart_p0 + self.cart_a_ref_out + self.cart_Mi

    # the written parts
    def p0(self, t):
        return self.cart_p0[t][:, PAD:-PAD]

    def a_ref_out(self, t):
        return self.cart_a_ref_out[t][PAD:-PAD].reshape(-1, 6)

    def Mi(self, t):
        return self.cart_Mi[t][PAD:-PAD].reshape(-1, 6, 6)

    def com(self):
        return self.com_p0[:, PAD:-PAD]

    def post(self, nv):
        return self.post_p0[PAD:-PAD].reshape(-1, 2 * nv)

    def qddot(self, nv):
        return self.post_qddot_out[PAD:-PAD].reshape(-1, nv)

    def minv(self, nv):
        return self.Minv[:, PAD:-PAD].reshape(-1, nv, nv)

    def fences_intact(self):
        """every spare double (and ok's spare ints) still holds the sentinel"""
        ok = all(np.all(a[:, :PAD] == SENTINEL) and np.all(a[:, -PAD:] == SENTINEL) for a in self.cart_p0 + [self.com_p0, self.Minv])
        ok = ok and all(np.all(a[:PAD] == SENTINEL) and np.all(a[-PAD:] == SENTINEL)
                        for a in self.cart_a_ref_out + self.cart_Mi + [self.post_p0, self.post_qddot_out])
        return ok and self.ok[0] == -7 and self.ok[-1] == -7


def device_M(case):
    """M as the kernel is given it: the lower triangle, NaN above it (only the lower triangle is read)"""
    M = case["M"].copy()
    iu = np.triu_indices(case["nv"], 1)
    M[:, iu[0], iu[1]] = np.nan
    return M


def structs(case, out, address, keep):
    """(abi.AccModel, abi.AccBatch) of a case and its Outputs; address(array) -> the address the kernel is given for it (host: the
    array's own; device: its copy's).  Arrays made here are appended to `keep`."""
    m, b = abi.AccModel(), abi.AccBatch()
    B, nv, ld = case["B"], case["nv"], case["ld"]
    m.nv, m.n_cart = nv, len(case["cart"])
    b.B = B
    b.q, b.qdot = address(case["q"]), address(case["qdot"])
    if case["M"] is not None:
        Md = device_M(case)
        keep.append(Md)
        b.M, b.M_stride = address(Md), nv * nv
    for t, term in enumerate(case["cart"]):
        m.cart_gain_type[t], m.cart_gain_matrices[t], m.cart_orientation_gain[t] = term["gain_type"], term["gain_matrices"], term["og"]
        for i in range(36):
            m.cart_Kp[36 * t + i], m.cart_Kd[36 * t + i] = float(term["Kp"].reshape(36)[i]), float(term["Kd"].reshape(36)[i])
        b.cart_J[t], b.cart_J_stride[t], b.cart_J_ld[t] = address(term["J"]) + 8 * ld, 8 * ld, ld
        b.cart_pose[t], b.cart_pose_ref[t] = address(term["pose"]), address(term["pose_ref"])
        for name in ("vel_ref", "f_virtual", "a_ref_in"):
            if term[name] is not None:
                getattr(b, "cart_" + name)[t] = address(term[name])
        if "cart_p0" in out.want:
            b.cart_p0[t], b.cart_p0_stride[t] = address(out.cart_p0[t]) + 8 * PAD, out.cart_p0[t].shape[1]
        if "cart_a_ref_out" in out.want:
            b.cart_a_ref_out[t] = address(out.cart_a_ref_out[t]) + 8 * PAD
        if "cart_Mi" in out.want and term["gain_type"] == FORCE:
            b.cart_Mi[t] = address(out.cart_Mi[t]) + 8 * PAD
    if case["com"] is not None:
        k = case["com"]
        m.has_com, m.com_gain_matrices = 1, k["gain_matrices"]
        for i in range(9):
            m.com_Kp[i], m.com_Kd[i] = float(k["Kp"].reshape(9)[i]), float(k["Kd"].reshape(9)[i])
        b.com_J, b.com_J_stride, b.com_J_ld = address(k["J"]) + 8 * ld, 5 * ld, ld
        b.com, b.com_ref = address(k["com"]), address(k["com_ref"])
        if k["vel_ref"] is not None:
            b.com_vel_ref = address(k["vel_ref"])
        if "com_p0" in out.want:
            b.com_p0, b.com_p0_stride = address(out.com_p0) + 8 * PAD, out.com_p0.shape[1]
    if case["post"] is not None:
        p = case["post"]
        m.has_postural, m.post_gain_type, m.post_gain_matrices, m.post_lambda, m.post_lambda2 = 1, p["gain_type"], p["gain_matrices"], p["lam"], p["lam2"]
        if p["Kp"] is not None:
            m.post_Kp, m.post_Kd = address(p["Kp"]), address(p["Kd"])
        b.post_q_ref = address(p["q_ref"])
        for name in ("qdot_ref", "qddot_ref"):
            if p[name] is not None:
                setattr(b, "post_" + name, address(p[name]))
        if "post_p0" in out.want:
            b.post_p0 = address(out.post_p0) + 8 * PAD
        if "post_qddot_out" in out.want:
            b.post_qddot_out = address(out.post_qddot_out) + 8 * PAD
    if case["minv"] and "Minv" in out.want:
        b.Minv, b.Minv_stride = address(out.Minv) + 8 * PAD, out.Minv.shape[1]
    if "ok" in out.want:
        b.ok = address(out.ok) + 4
    return m, b


def run_host(case, want=Outputs.ALL):
    """the case through the emulated kernel -> Outputs"""
    out, keep = Outputs(case, want), []
    m, b = structs(case, out, lambda a: a.ctypes.data, keep)
    assert lib().acc_host_tasks(C.byref(m), C.byref(b)) == abi.OK
    return out


# ---- 4. the restatement ----------------------------------------------------------------------------------------------------------------
def cholesky(M, T, thr_rel):
    """M = L L' column by column in dtype T -> (L, ok); ok = False at the first pivot that is not finite or not above thr_rel x the
    largest diagonal entry (L is then not to be used)"""
    n = M.shape[0]
    A = np.tril(M).astype(T)
    L = np.zeros((n, n), dtype=T)
    thr = T(thr_rel) * np.max(np.diag(A))
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not (np.isfinite(d) and d > thr):
            return L, False
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, True


def solve_lower(L, Bm):
    """L Y = Bm by forward substitution"""
    Y = np.zeros_like(Bm)
    for k in range(L.shape[0]):
        Y[k] = (Bm[k] - L[k, :k] @ Y[:k]) / L[k, k]
    return Y


def solve_upper_t(L, Y):
    """L' X = Y by back substitution"""
    X = np.zeros_like(Y)
    for k in range(L.shape[0] - 1, -1, -1):
        X[k] = (Y[k] - L[k + 1:, k] @ X[k + 1:]) / L[k, k]
    return X


def pose_error(term, i):
    """[p_ref - p; orientation_gain e_o] of instance i in float64, one IEEE operation per operator (the bit-exact group)"""
    Ta, Tr = term["pose"][i], term["pose_ref"][i]
    return np.concatenate([Tr[9:12] - Ta[9:12], term["og"] * orientation_error(Ta, Tr)])


def restate(case, T=np.float64):
    """every output of osot_acc_tasks for the case in dtype T (the errors that are single float64 operations stay float64) ->
    dict(ok [B], cart=[dict(pose_err, vel_err, Gp, Gd, Mi, a_ref_out)], com=dict(err, vel_err), post=dict(pe, ve, qddot_out), Minv)"""
    B, nv = case["B"], case["nv"]
    z = lambda a, s: np.zeros(s) if a is None else a
    R = dict(ok=np.ones(B, dtype=np.int32), cart=[], com=None, post=None, Minv=np.zeros((B, nv, nv), dtype=T))
    fac = []
    if needs_M(case):
        for i in range(B):
            L, ok = cholesky(case["M"][i], T, pivot_rel(nv))
            R["ok"][i] = int(ok)
            fac.append(L if ok else None)
            if ok and case["minv"]:
                Z = solve_lower(L, np.eye(nv, dtype=T))
                R["Minv"][i] = Z.T @ Z
    qd = case["qdot"].astype(T)
    for term in case["cart"]:
        J = term["J"][:, 1:7, :nv].astype(T)
        o = dict(pose_err=np.stack([pose_error(term, i) for i in range(B)]),
                 vel_err=z(term["vel_ref"], (B, 6)).astype(T) - np.einsum("brk,bk->br", J, qd),
                 Gp=np.zeros((B, 6, 6), dtype=T), Gd=np.zeros((B, 6, 6), dtype=T), Mi=np.zeros((B, 6, 6), dtype=T),
                 a_ref_out=z(term["a_ref_in"], (B, 6)).astype(T))
        for i in range(B):
            if term["gain_type"] == FORCE:
                if fac[i] is not None:
                    Y = solve_lower(fac[i], J[i].T.copy())
                    o["Mi"][i] = Y.T @ Y
                    o["Gp"][i], o["Gd"][i] = o["Mi"][i] @ term["Kp"].astype(T), o["Mi"][i] @ term["Kd"].astype(T)
                    if term["f_virtual"] is not None:
                        o["a_ref_out"][i] = o["a_ref_out"][i] + o["Mi"][i] @ term["f_virtual"][i].astype(T)
            else:
                o["Gp"][i], o["Gd"][i] = term["Kp"], term["Kd"]
        R["cart"].append(o)
    if case["com"] is not None:
        k = case["com"]
        R["com"] = dict(err=k["com_ref"] - k["com"],
                        vel_err=z(k["vel_ref"], (B, 3)).astype(T) - np.einsum("brk,bk->br", k["J"][:, 1:4, :nv].astype(T), qd))
    if case["post"] is not None:
        p = case["post"]
        pe, ve = p["q_ref"] - case["q"], z(p["qdot_ref"], (B, nv)) - case["qdot"]
        Kp = np.eye(nv) if p["Kp"] is None else p["Kp"]
        Kd = np.eye(nv) if p["Kd"] is None else p["Kd"]
        v = T(p["lam"]) * (pe.astype(T) @ Kp.astype(T).T) + T(p["lam2"]) * (ve.astype(T) @ Kd.astype(T).T)
        out = z(p["qddot_ref"], (B, nv)).astype(T)
        for i in range(B):
            if p["gain_type"] == FORCE:
                if fac[i] is not None:
                    out[i] = out[i] + solve_upper_t(fac[i], solve_lower(fac[i], v[i]))
            else:
                out[i] = out[i] + v[i]
        R["post"] = dict(pe=pe, ve=ve, qddot_out=out)
    return R


def chol_outputs(case, got, ref):
    """(name, instance, X, X*) of every Cholesky-based output: got an Outputs or a restate() result, ref a restate() result"""
    nv = case["nv"]
    as_ref = isinstance(got, dict)
    for i in range(case["B"]):
        for t, term in enumerate(case["cart"]):
            if term["gain_type"] != FORCE:
                continue
            r = ref["cart"][t]
            if as_ref:
                g = got["cart"][t]
                trip = (("Mi", g["Mi"][i], r["Mi"][i]), ("Gp", g["Gp"][i], r["Gp"][i]), ("Gd", g["Gd"][i], r["Gd"][i]),
                        ("a_ref_out", g["a_ref_out"][i], r["a_ref_out"][i]))
            else:
                p0 = got.p0(t)[i]
                trip = (("Mi", got.Mi(t)[i], r["Mi"][i]), ("Gp", p0[12:48].reshape(6, 6), r["Gp"][i]), ("Gd", p0[48:84].reshape(6, 6), r["Gd"][i]),
                        ("a_ref_out", got.a_ref_out(t)[i], r["a_ref_out"][i]))
            for name, x, xs in trip:
                yield f"cart{t}.{name}", i, x, xs
        if case["post"] is not None and case["post"]["gain_type"] == FORCE:
            yield "qddot_out", i, (got["post"]["qddot_out"][i] if as_ref else got.qddot(nv)[i]), ref["post"]["qddot_out"][i]
        if case["minv"]:
            yield "Minv", i, (got["Minv"][i] if as_ref else got.minv(nv)[i]), ref["Minv"][i]


def worst_deviation(case, got, arbiter):
    """max over outputs and instances of max|X - X*| / (cond2(M) max|X*|) -> (figure, the output's name, instance)"""
    cond = [np.linalg.cond(case["M"][i]) for i in range(case["B"])]
    worst = (0.0, "", -1)
    for name, i, x, xs in chol_outputs(case, got, arbiter):
        err, scale = np.max(np.abs(np.asarray(x, dtype=np.longdouble) - xs)), np.max(np.abs(xs))
        dev = float(err / (cond[i] * scale)) if scale > 0 else (0.0 if err == 0 else np.inf)    # an all-zero X*: X is to be zero too
        if dev > worst[0]:
            worst = (dev, name, i)
    return worst

# ---- 5. the batch with a failed pivot ----------------------------------------------------------------------------------------------------
def singular_case(case, instance=1):
    """the case with an exact zero row and column in M of one instance"""
    M = case["M"].copy()
    z = case["nv"] // 2
    M[instance, z, :] = 0.0
    M[instance, :, z] = 0.0
    return dict(case, M=M)


def views(out, case):
    """the written part of every output, one row per instance"""
    nv, T = case["nv"], range(len(case["cart"]))
    return [out.p0(t) for t in T] + [out.a_ref_out(t) for t in T] + [out.Mi(t) for t in T] + \
        [out.com(), out.post(nv), out.qddot(nv), out.minv(nv), out.ok[1:-1]]


def check_failed_pivot(out, good, case, bad=1):
    """out: the Outputs of the batch whose instance `bad` has a singular M; good: of the same batch without it.  ok, the Force
    outputs of that instance as osot_acc_tasks documents them, nothing non-finite; its other outputs and the other instances bit
    for bit as in `good`"""
    nv, B = case["nv"], case["B"]
    assert list(out.ok[1:-1]) == [int(i != bad) for i in range(B)]
    assert out.fences_intact()
    for a in views(out, case):
        assert np.all(np.isfinite(a.astype(float)))
    for t, term in enumerate(case["cart"]):
        if term["gain_type"] == FORCE:
            assert np.all(out.p0(t)[bad, 12:84] == 0.0) and np.all(out.Mi(t)[bad] == 0.0)
            assert np.array_equal(out.a_ref_out(t)[bad], term["a_ref_in"][bad])
            assert np.array_equal(out.p0(t)[bad, :12], good.p0(t)[bad, :12])
        else:
            assert np.array_equal(out.p0(t)[bad], good.p0(t)[bad]) and np.array_equal(out.a_ref_out(t)[bad], good.a_ref_out(t)[bad])
    assert np.all(out.minv(nv)[bad] == 0.0)
    assert np.array_equal(out.qddot(nv)[bad], case["post"]["qddot_ref"][bad])
    assert np.array_equal(out.post(nv)[bad], good.post(nv)[bad]) and np.array_equal(out.com()[bad], good.com()[bad])
    others = [i for i in range(B) if i != bad]
    for a, b in zip(views(out, case), views(good, case)):
        assert np.array_equal(a[others], b[others])

# ---- 6. the tracking stack of synth.make_coman_id_tracking_stack on the host ---------------------------------------------------------------
def tracking_quantities(model, leaf, q, qd):
    """what the producers leave for dynamics.IdTrackingStep, from tests/dyn_ref.py: make_coman_id_stack's (test_dynamics_host) and the
    hand's Jacobian, pose and Jdot qdot"""
    import dyn_ref
    from test_dynamics_host import GRAVITY, coman_quantities
    Q = coman_quantities(model, q, qd, "ref")
    f = model.frame_index(leaf["state"]["tracking"]["hand"])
    B = q.shape[0]
    Q.update(Jhand=np.zeros((B, 6, model.n)), hand_pose=np.zeros((B, 12)), hand_jdq=np.zeros((B, 6)))
    for i in range(B):
        r = dyn_ref.Ref(model, q[i], qd[i], GRAVITY)
        Q["Jhand"][i], Q["hand_jdq"][i] = r.frame_jacobian(f), r.frame_jdot_qdot(f)
        Q["hand_pose"][i] = np.concatenate([np.asarray(r.fk["frame_R"][f]).reshape(9), r.fk["frame_p"][f]])
    return Q


def tracking_case(leaf, Q, q, qd, com_ref, hand_ref):
    """the osot_acc_tasks case (make_case's layout) of one step of the tracking stack, as IdTrackingStep binds it"""
    tr = leaf["state"]["tracking"]
    B, nv = q.shape

    def block(J):                                   # the rows at row 1 of a block two rows taller (structs' convention)
        out = np.zeros((B, J.shape[1] + 2, nv))
        out[:, 1:-1] = J
        return out
    return dict(B=B, nv=nv, ld=nv, minv=False, q=np.ascontiguousarray(q), qdot=np.ascontiguousarray(qd), M=0.5 * (Q["M"] + np.transpose(Q["M"], (0, 2, 1))),
                cart=[dict(gain_type=tr["gain_type"], gain_matrices=1, Kp=tr["Kp"], Kd=tr["Kd"], og=tr["orientation_gain"], J=block(Q["Jhand"]),
                           pose=np.ascontiguousarray(Q["hand_pose"]), pose_ref=np.ascontiguousarray(hand_ref), vel_ref=tr["vel_ref"],
                           f_virtual=tr["f_virtual"], a_ref_in=None)],
                com=dict(gain_matrices=0, Kp=np.eye(3), Kd=np.eye(3), J=block(Q["Jcom"]), com=np.ascontiguousarray(Q["com"]),
                         com_ref=np.ascontiguousarray(com_ref), vel_ref=None),
                post=dict(gain_type=tr["gain_type"], gain_matrices=1, lam=tr["post_lam"], lam2=tr["post_lam2"], Kp=tr["post_Kp"], Kd=tr["post_Kd"],
                          q_ref=np.ascontiguousarray(leaf["state"]["q_ref"]), qdot_ref=None, qddot_ref=None))


def tracking_leaf(leaf, Q, p0_hand, a_ref, p0_com, p0_post, qddot_d):
    """the leaf of the tracking stack for this step (numpy) from the producer's outputs: test_dynamics_host.coman_fill_leaf's A_0,
    C and rows, the hand's rows in A_1"""
    from test_dynamics_host import coman_fill_leaf
    B, nv = Q["M"].shape[0], Q["M"].shape[1]
    out = coman_fill_leaf(leaf, Q, np.zeros((B, nv)), np.zeros((B, nv)), Q["com"])
    A1 = np.zeros((B, 6, nv + 12))
    A1[:, :, :nv] = Q["Jhand"]
    out["A"] = [out["A"][0], A1, None]
    lvl0 = out["task"][0]
    out["task"] = [[lvl0[0], lvl0[1], (np.ascontiguousarray(p0_com), Q["com_jdq"], None)],
                   [(np.ascontiguousarray(p0_hand), Q["hand_jdq"], np.ascontiguousarray(a_ref))],
                   [(np.ascontiguousarray(p0_post), None, np.ascontiguousarray(qddot_d))]]
    return out


def tracking_b(plan, Q, R):
    """b of the three acceleration blocks from the reference formulas (Cartesian.cpp:147-169, CoM.cpp:86-92, Postural.cpp:145-158) and
    a restate() result R, in R's dtype -> (b_hand [B][6], b_com [B][3], b_post [B][nv], scale_hand [B]: the size of b_hand's terms)"""
    c, T = R["cart"][0], R["Minv"].dtype.type
    com_t = plan.levels[0][2]
    pe, ve = c["pose_err"].astype(T), c["vel_err"]
    b_hand = c["a_ref_out"] + np.einsum("bij,bj->bi", c["Gd"], ve) + np.einsum("bij,bj->bi", c["Gp"], pe) - Q["hand_jdq"]
    scale = np.abs(c["a_ref_out"]).max(axis=1) + 6 * np.abs(c["Gd"]).max(axis=(1, 2)) * np.abs(ve).max(axis=1) + \
        6 * np.abs(c["Gp"]).max(axis=(1, 2)) * np.abs(pe).max(axis=1) + np.abs(Q["hand_jdq"]).max(axis=1)
    b_com = T(com_t.lam2) * R["com"]["vel_err"] + T(com_t.lam) * R["com"]["err"].astype(T) - Q["com_jdq"]
    return b_hand, b_com, R["post"]["qddot_out"], scale


if __name__ == "__main__":
    for name in CASES:
        if CASES[name]["M"] is None:
            continue
        case = named_case(name)
        arb = restate(case, np.longdouble)
        print(f"{name:18s} cond2 <= {max(np.linalg.cond(M) for M in case['M']):9.3e}  restatement {worst_deviation(case, restate(case), arb)}"
              f"  emulated {worst_deviation(case, run_host(case), arb)}")
