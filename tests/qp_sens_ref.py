"""tests/qp_sens_ref.py -- TEST INFRASTRUCTURE ONLY: what the tests of osot_qp_sensitivity_batch share.

  * the recipe of the host build tests/emu/qp_sens_host.cpp (osot_qp_sens_kernel through the lock-step emulation, with the checks of
    osot_qp_sensitivity_batch), built with native_build's flags, staleness rule and write-then-rename rule; and of the same file as a
    stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (statically linked runtimes, its own main: nothing is
    loaded into Python under a sanitizer);
  * a numpy restatement of the contract of include/osot_mi355x.h (osot_qp_sensitivity_batch) by the SAME ROUTE (Cholesky of H + eps I,
    column-pivoted Householder QR of L^-1 C'), in any dtype: float64 is the restatement, numpy.longdouble the arbiter; and, for the
    gradients, the arbiter's DENSE KKT solve (Gaussian elimination with partial pivoting in longdouble on the arbiter's set);
  * the cases: the fixture tests/golden/qp_sens.npz (inputs of helpers.random_qp, x and y of the reference's qpOASES, a seeded
    grad_x; tests/golden/make_qp_sens_golden.py) and the edges, whose solution and multipliers are known by construction;
  * sentinel-fenced destinations and the run of a case through anything that takes the struct (the host build here, the device
    library in tests/test_qp_sens_gpu.py).

THE TOLERANCE.  The deviation of an output from the arbiter is stated as  max|X - X*| / (cond2(H + eps I) max|X*|)  per instance and
output.  `python tests/qp_sens_ref.py` measures, over the fixture, REFERENCE_WORST (the reference's own y), RESTATEMENT_WORST (y and
the seven gradients of the float64 restatement) and, for the record, EMULATED_WORST (the emulated kernel).  SENS_TOL is 10 x the
larger of the first two: the margin acc_ref.CHOLESKY_TOL gives a different summation order.  It is measured on the reference and
the restatement, never on the kernel under test."""
import ctypes as C
import os
import shlex
import subprocess
import sys

import numpy as np

if __name__ == "__main__":     # `python tests/qp_sens_ref.py`: the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opensot_amd import abi
from opensot_amd.plan import eps_abs_from_factor
import native_build

EMU = os.path.join(native_build.ROOT, "tests", "emu")
GOLDEN = os.path.join(native_build.ROOT, "tests", "golden", "qp_sens.npz")
SOURCE = "qp_sens_host.cpp"
LIBRARY = "libosot_qp_sens_host.so"
PROGRAM = "qp_sens_asan"
SANITIZED = ["g++", "-O1", "-g", "-std=c++17", "-DOSOT_EMULATION", "-DOSOT_QP_SENS_MAIN", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I."] + native_build.INCLUDES
SENTINEL = -7.25e300
OK, DEGENERATE, SKIPPED = abi.SENS_OK, abi.SENS_DEGENERATE, abi.SENS_SKIPPED
DEFAULTS = (1e-8, 1e-9, 1e-11)          # active_tol, dual_tol, rank_tol
EPS_ABS = eps_abs_from_factor(2e2)
# the fixture's shapes (n, nc, n_eq, B); the last is box only
SHAPES = ((7, 9, 0, 8), (32, 40, 3, 4), (33, 20, 0, 4), (64, 24, 2, 2), (12, 0, 0, 4))
GRADS = ("grad_H", "grad_g", "grad_A", "grad_lA", "grad_uA", "grad_l", "grad_u")

# measured on the CPU over the fixture (python tests/qp_sens_ref.py prints them), in units of cond2(H + eps I) max|X*|
REFERENCE_WORST = 6.09e-17
RESTATEMENT_WORST = 7.10e-17
EMULATED_WORST = 8.66e-17
SENS_TOL = 10.0 * max(REFERENCE_WORST, RESTATEMENT_WORST)


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
    """build tests/emu/libosot_qp_sens_host.so if it is stale (native_build.is_stale), to a temporary name first"""
    return _ensure(LIBRARY, native_build.LOCKSTEP)


def ensure_sanitized():
    """the stand-alone program of the same file (-DOSOT_QP_SENS_MAIN) under ASan + UBSan"""
    return _ensure(PROGRAM, SANITIZED)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(ensure())
        _lib.sens_host_check.argtypes = [C.POINTER(abi.QpSensBatch), C.POINTER(abi.QpSensOptions), C.POINTER(C.c_char_p)]
        _lib.sens_host_run.argtypes = [C.POINTER(abi.QpSensBatch), C.POINTER(abi.QpSensOptions)]
        _lib.sens_host_lds_bytes.argtypes = [C.c_int]
    return _lib


def host_check(batch, options=None):
    """osot_qp_sensitivity_batch's answer to its arguments, from the host build -> (code, reason)"""
    why = C.c_char_p()
    rc = lib().sens_host_check(C.byref(batch), None if options is None else C.byref(options), C.byref(why))
    return rc, (why.value or b"").decode()


# ---- 2. cases ------------------------------------------------------------------------------------------------------------------------
def problem(H, g, A=None, lA=None, uA=None, l=None, u=None, eps_abs=EPS_ABS):
    """B QPs as contiguous host arrays (A.. and l, u optional)"""
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    B, n = g.shape
    return dict(B=B, n=n, nc=0 if A is None else A.shape[1], H=c(H), g=c(g), A=c(A), lA=c(lA), uA=c(uA), l=c(l), u=c(u), eps_abs=float(eps_abs))


def fixture():
    """[(problem, x_ref, y_ref, grad_x)] of tests/golden/qp_sens.npz, one per shape of SHAPES"""
    out = []
    with np.load(GOLDEN) as z:
        for s, (n, nc, n_eq, B) in enumerate(SHAPES):
            get = lambda k: z[f"s{s}_{k}"] if f"s{s}_{k}" in z.files else None
            p = problem(get("H"), get("g"), get("A"), get("lA"), get("uA"), get("l"), get("u"), float(z["eps_abs"]))
            assert (p["B"], p["n"], p["nc"]) == (B, n, nc)
            out.append((p, get("x"), get("y"), get("grad_x")))
    return out


def reference_active(p, y_ref):
    """the reference's set from its multipliers: 0, -1 lower (y > 0), +1 upper (y < 0), 2 where the two sides are equal"""
    B, n, nc = p["B"], p["n"], p["nc"]
    act = np.where(y_ref > 0, -1, np.where(y_ref < 0, 1, 0)).astype(np.int32)
    if p["l"] is not None:
        act[:, :n][p["l"] == p["u"]] = 2
    if nc:
        act[:, n:][p["lA"] == p["uA"]] = 2
    return act


def margins_ok(A, lA, uA, l, u, x, y, MARGIN=1e-6):
    """non-degenerate by the reference alone: |y| >= MARGIN on every active inequality, a gap >= MARGIN on every inactive side"""
    n = len(x)
    v = x if A is None else np.concatenate([x, A @ x])
    lo = l if A is None else np.concatenate([l, lA])
    up = u if A is None else np.concatenate([u, uA])
    for k in range(len(v)):
        if lo[k] == up[k]:
            continue
        if y[k] != 0.0:
            if abs(y[k]) < MARGIN:
                return False
            side = lo[k] if y[k] > 0 else up[k]
            other = up[k] if y[k] > 0 else lo[k]
            if abs(v[k] - side) > 1e-9 * max(1.0, abs(side)) or (np.isfinite(other) and abs(v[k] - other) < MARGIN):
                return False
        else:
            if (np.isfinite(lo[k]) and v[k] - lo[k] < MARGIN) or (np.isfinite(up[k]) and up[k] - v[k] < MARGIN):
                return False
    return True


def constructed(B, n, nc, box=True, shape=None, post=None, seed=0, eps_abs=EPS_ABS):
    """B QPs whose solution and multipliers are known by construction: x and the active sides are chosen (shape(i, bside, rside) marks
    them: 0, -1, +1, 2), y is drawn with the right signs, g = -H~x + y_b + A'y_c; post(i, q) may edit the instance's arrays (a dict)
    before g is formed.  -> (problem, x, y)"""
    rng = np.random.default_rng([B, n, nc, seed, 77])
    H, g, x, y = np.zeros((B, n, n)), np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n + nc))
    A, lA, uA = np.zeros((B, nc, n)), np.zeros((B, nc)), np.zeros((B, nc))
    l, u = np.zeros((B, n)), np.zeros((B, n))
    for i in range(B):
        M = rng.normal(size=(n + 3, n))
        q = dict(H=M.T @ M, A=rng.normal(size=(nc, n)), x=rng.uniform(-0.3, 0.3, n))
        bside, rside = np.zeros(n, dtype=int), np.zeros(nc, dtype=int)
        if shape is not None:
            shape(i, bside, rside)
        if not box:
            bside[:] = 0
        ax = q["A"] @ q["x"]
        q["l"] = q["x"] - np.where((bside == -1) | (bside == 2), 0.0, 0.5)
        q["u"] = q["x"] + np.where((bside == 1) | (bside == 2), 0.0, 0.5)
        q["lA"] = ax - np.where((rside == -1) | (rside == 2), 0.0, 0.5)
        q["uA"] = np.where(rside == 2, q["lA"], ax + np.where(rside == 1, 0.0, 0.5))
        sign = lambda s: np.where(s == 1, -1.0, np.where(s == 0, 0.0, 1.0))
        q["yb"] = sign(bside) * rng.uniform(0.5, 1.5, n)
        q["yc"] = sign(rside) * rng.uniform(0.5, 1.5, nc)
        if post is not None:
            post(i, q)
        H[i], A[i], x[i], l[i], u[i], lA[i], uA[i] = q["H"], q["A"], q["x"], q["l"], q["u"], q["lA"], q["uA"]
        y[i] = np.concatenate([q["yb"], q["yc"]])
        g[i] = -(q["H"] + eps_abs * np.eye(n)) @ q["x"] + q["yb"] + q["A"].T @ q["yc"]
    p = problem(H, g, A if nc else None, lA if nc else None, uA if nc else None, l if box else None, u if box else None, eps_abs)
    return p, x, y


# ---- 3. destinations, the struct, the run --------------------------------------------------------------------------------------------
PAD = 2


class Outputs:
    """sentinel-filled destinations with PAD spare entries in front of and behind each; `want` names the outputs that are bound (the
    others stay NULL and must stay sentinels)"""

    ALL = ("y", "active", "flag") + GRADS

    def __init__(self, p, want=ALL):
        B, n, nc = p["B"], p["n"], p["nc"]
        self.want = tuple(want)
        self.shapes = dict(y=(B, n + nc), active=(B, n + nc), flag=(B,), grad_H=(B, n, n), grad_g=(B, n), grad_A=(B, nc, n), grad_lA=(B, nc),
                           grad_uA=(B, nc), grad_l=(B, n), grad_u=(B, n))
        self.raw = {}
        for k, s in self.shapes.items():
            ints = k in ("active", "flag")
            self.raw[k] = np.full(int(np.prod(s)) + 2 * PAD, -7 if ints else SENTINEL, dtype=np.int32 if ints else np.float64)

    def __getattr__(self, k):
        if k in self.__dict__.get("shapes", {}):
            return self.raw[k][PAD:len(self.raw[k]) - PAD].reshape(self.shapes[k])
        raise AttributeError(k)

    def fences_intact(self):
        """every spare entry, and the whole of an output that was not bound, still holds the sentinel"""
        for k, a in self.raw.items():
            s = -7 if a.dtype == np.int32 else SENTINEL
            part = a if k not in self.want else np.concatenate([a[:PAD], a[-PAD:]])
            if not np.all(part == s):
                return False
        return True


def structs(p, x, out, address, keep, gx=None, status=None):
    """abi.QpSensBatch of a case and its Outputs; address(array) -> the address the kernel is given for it (host: the array's own;
    device: its copy's).  Arrays made here are appended to `keep`."""
    b = abi.QpSensBatch()
    b.B, b.n, b.nc, b.eps_abs = p["B"], p["n"], p["nc"], p["eps_abs"]
    for k in ("H", "g", "A", "lA", "uA", "l", "u"):
        if p[k] is not None:
            setattr(b, k, address(p[k]))
    x = np.ascontiguousarray(x, dtype=np.float64)
    keep.append(x)
    b.x = address(x)
    if gx is not None:
        gx = np.ascontiguousarray(gx, dtype=np.float64)
        keep.append(gx)
        b.grad_x = address(gx)
    if status is not None:
        status = np.ascontiguousarray(status, dtype=np.int32)
        keep.append(status)
        b.status = address(status)
    for k in out.want:
        a = out.raw[k]
        if k in ("grad_A", "grad_lA", "grad_uA") and p["nc"] == 0:
            continue
        if k in ("grad_l", "grad_u") and p["l"] is None:
            continue
        setattr(b, k, address(a) + PAD * a.itemsize)
    return b


def options(active_tol=0.0, dual_tol=0.0, rank_tol=0.0):
    o = abi.QpSensOptions()
    o.active_tol, o.dual_tol, o.rank_tol = active_tol, dual_tol, rank_tol
    return o


def run_host(p, x, gx=None, status=None, want=None, opts=None):
    """the case through the emulated kernel -> Outputs"""
    if want is None:
        want = Outputs.ALL if gx is not None else ("y", "active", "flag")
    out, keep = Outputs(p, want), []
    b = structs(p, x, out, lambda a: a.ctypes.data, keep, gx, status)
    assert lib().sens_host_run(C.byref(b), None if opts is None else C.byref(opts)) == abi.OK
    return out


# ---- 4. the restatement --------------------------------------------------------------------------------------------------------------
def pivot_rel(n):
    return (n + 1) * 2.0 ** -52


def cholesky(M, T, thr_rel):
    """M = L L' column by column in dtype T from M's lower triangle -> (L, ok) (the pivot rule of osot_acc.h)"""
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
    Y = np.zeros_like(Bm)
    for k in range(L.shape[0]):
        Y[k] = (Bm[k] - L[k, :k] @ Y[:k]) / L[k, k]
    return Y


def solve_upper_t(L, Y):
    X = np.zeros_like(Y)
    for k in range(L.shape[0] - 1, -1, -1):
        X[k] = (Y[k] - L[k + 1:, k] @ X[k + 1:]) / L[k, k]
    return X


def _sides(v, lo, up, tol, T):
    """0, -1, +1, 2 of every entry: the candidate rule"""
    out = np.zeros(len(v), dtype=int)
    for i in range(len(v)):
        flo, fup = abs(lo[i]) < 1e20, abs(up[i]) < 1e20
        if flo and fup and lo[i] == up[i]:
            out[i] = 2
        elif flo and abs(v[i] - T(lo[i])) <= T(tol) * max(T(1), abs(T(lo[i]))):
            out[i] = -1
        elif fup and abs(v[i] - T(up[i])) <= T(tol) * max(T(1), abs(T(up[i]))):
            out[i] = 1
    return out


def restate_one(H, g, A, lA, uA, l, u, eps_abs, x, gx=None, T=np.float64, tols=DEFAULTS):
    """one instance by the kernel's route in dtype T -> dict(flag, y, active, the seven gradients, set=[(index, side, lambda, dlambda)],
    dx); index < n: a bound, else n + the row"""
    n = len(g)
    nc = 0 if A is None else A.shape[0]
    active_tol, dual_tol, rank_tol = tols
    R = dict(flag=SKIPPED, y=np.zeros(n + nc, dtype=T), active=np.zeros(n + nc, dtype=np.int32), grad_H=np.zeros((n, n), dtype=T),
             grad_g=np.zeros(n, dtype=T), grad_A=np.zeros((nc, n), dtype=T), grad_lA=np.zeros(nc, dtype=T), grad_uA=np.zeros(nc, dtype=T),
             grad_l=np.zeros(n, dtype=T), grad_u=np.zeros(n, dtype=T), set=[], dx=np.zeros(n, dtype=T))
    if not np.all(np.isfinite(x)):
        return R
    xT, gT = x.astype(T), g.astype(T)
    AT = None if A is None else A.astype(T)
    L, ok = cholesky(np.tril(H).astype(T) + T(eps_abs) * np.eye(n, dtype=T), T, pivot_rel(n))
    if not ok:
        return R
    bs = _sides(xT, l, u, active_tol, T) if l is not None else np.zeros(n, dtype=int)
    rs = _sides(AT @ xT, lA, uA, active_tol, T) if nc else np.zeros(0, dtype=int)
    cand = [(i, 2) for i in range(n) if bs[i] == 2] + [(n + r, 2) for r in range(nc) if rs[r] == 2] + \
        [(i, int(bs[i])) for i in range(n) if abs(bs[i]) == 1] + [(n + r, int(rs[r])) for r in range(nc) if abs(rs[r]) == 1]
    degenerate = len(cand) > 2 * n
    cand = cand[:2 * n]
    state = np.zeros(len(cand), dtype=int)
    normal = lambda idx: np.eye(n, dtype=T)[idx] if idx < n else AT[idx - n]
    have_gx = gx is not None
    w0 = solve_lower(L, gx.astype(T)) if have_gx else np.zeros(n, dtype=T)
    for sweep in range(2):
        pool = [c for c in range(len(cand)) if state[c] == 0]
        kp = len(pool)
        M = np.zeros((n, kp + 2), dtype=T)
        if kp:
            M[:, :kp] = solve_lower(L, np.stack([normal(cand[c][0]) for c in pool], axis=1))
        M[:, kp] = -(L.T @ xT + solve_lower(L, gT))
        M[:, kp + 1] = w0
        remaining, piv, rd, refl = list(range(kp)), [], [], []
        first = T(0)
        for j in range(n):
            if not remaining:
                break
            n2 = np.sum(M[j:, remaining] ** 2, axis=0)
            a = int(np.argmax(n2))
            best = n2[a]
            norm = np.sqrt(best)
            if j == 0:
                first = norm
            if not (norm > 0) or not np.isfinite(norm) or norm < T(rank_tol) * first:
                break
            pc = remaining.pop(a)
            x0 = M[j, pc]
            alpha = -norm if x0 >= 0 else norm
            v = M[j:, pc].copy()
            v[0] = x0 - alpha
            beta = T(1) / (best + norm * abs(x0))
            cols = remaining + [kp, kp + 1]
            s = beta * (v @ M[j:, cols])
            M[j:, cols] -= np.outer(v, s)
            piv.append(pc); rd.append(alpha); refl.append((v, beta))
        r = len(piv)
        dependent = len(remaining) > 0
        lam, dlam = np.zeros(r, dtype=T), np.zeros(r, dtype=T)
        tv, wv = M[:r, kp].copy(), -M[:r, kp + 1].copy()
        for j in range(r - 1, -1, -1):
            lam[j], dlam[j] = tv[j] / rd[j], wv[j] / rd[j]
            tv[:j] -= M[:j, piv[j]] * lam[j]
            wv[:j] -= M[:j, piv[j]] * dlam[j]
        linf = max([abs(v) for v in lam], default=T(0))
        weak = [cand[pool[piv[j]]][1] != 2 and (abs(lam[j]) <= T(dual_tol) * max(T(1), linf) or
                                                 (lam[j] > 0 if cand[pool[piv[j]]][1] == -1 else lam[j] < 0)) for j in range(r)]
        degenerate = degenerate or dependent or any(weak)
        if sweep == 0 and any(weak):
            state[:] = 0
            for j in range(r):
                if weak[j]:
                    state[pool[piv[j]]] = 3
            continue
        break
    z = M[:, kp + 1].copy()
    z[:r] = 0
    for j in range(r - 1, -1, -1):
        v, beta = refl[j]
        z[j:] -= (beta * (v @ z[j:])) * v
    dx = -solve_upper_t(L, z)
    if not (np.all(np.isfinite(lam)) and np.all(np.isfinite(dlam)) and np.all(np.isfinite(dx))):
        return R
    R["flag"] = DEGENERATE if degenerate else OK
    for j in range(r):
        idx, side = cand[pool[piv[j]]]
        R["set"].append((idx, side, lam[j], dlam[j]))
    _fill(R, n, xT, dx if have_gx else None)
    return R


def _fill(R, n, xT, dx):
    """y, active and the gradients of R from its set (and dx, with a backward pass)"""
    for idx, side, lam, dlam in R["set"]:
        R["y"][idx], R["active"][idx] = -lam, side
        if dx is None:
            continue
        name = ("grad_u" if side == 1 else "grad_l") if idx < n else ("grad_uA" if side == 1 else "grad_lA")
        R[name][idx if idx < n else idx - n] = -dlam
        if idx >= n:
            R["grad_A"][idx - n] = dlam * xT + lam * dx
    if dx is not None:
        R["dx"], R["grad_g"] = dx, dx.copy()
        R["grad_H"] = (np.outer(dx, xT) + np.outer(xT, dx)) / 2


def ge_solve(K, rhs):
    """K z = rhs by Gaussian elimination with partial pivoting, in K's dtype"""
    K, z = K.copy(), rhs.copy()
    m = len(z)
    for c in range(m):
        p = c + int(np.argmax(np.abs(K[c:, c])))
        if p != c:
            K[[c, p]], z[[c, p]] = K[[p, c]], z[[p, c]]
        f = K[c + 1:, c] / K[c, c]
        K[c + 1:, c:] -= np.outer(f, K[c, c:])
        z[c + 1:] -= f * z[c]
    for c in range(m - 1, -1, -1):
        z[c] = (z[c] - K[c, c + 1:] @ z[c + 1:]) / K[c, c]
    return z


def dense_kkt_gradients(R, H, A, eps_abs, x, gx):
    """the gradients of an arbiter result R (restate_one in longdouble) recomputed from a DENSE solve of
    [H~ C'; C 0] [dx; dlambda] = -[grad_x; 0] on R's set -> a copy of R with them"""
    T = np.longdouble
    n = len(x)
    if R["flag"] == SKIPPED:
        return R
    Ht = np.tril(H).astype(T)
    Ht = Ht + np.tril(Ht, -1).T + T(eps_abs) * np.eye(n, dtype=T)
    k = len(R["set"])
    Cm = np.zeros((k, n), dtype=T)
    for j, (idx, _, _, _) in enumerate(R["set"]):
        Cm[j] = np.eye(n, dtype=T)[idx] if idx < n else A[idx - n].astype(T)
    K = np.zeros((n + k, n + k), dtype=T)
    K[:n, :n], K[:n, n:], K[n:, :n] = Ht, Cm.T, Cm
    z = ge_solve(K, -np.concatenate([gx.astype(T), np.zeros(k, dtype=T)]))
    out = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in R.items()}
    for name in GRADS:
        out[name] = np.zeros_like(R[name])
    out["set"] = [(idx, side, lam, z[n + j]) for j, (idx, side, lam, _) in enumerate(R["set"])]
    _fill(out, n, x.astype(T), z[:n])
    return out


def _inst(p, i):
    o = lambda k: None if p[k] is None else p[k][i]
    return o("H"), o("g"), o("A"), o("lA"), o("uA"), o("l"), o("u"), p["eps_abs"]


def restate(p, x, gx=None, T=np.float64, tols=DEFAULTS, status=None):
    """every instance of a case -> list of restate_one results (an instance whose status is not SOLVED: skipped)"""
    out = []
    for i in range(p["B"]):
        xi = x[i] if status is None or status[i] == 0 else np.full(p["n"], np.nan)
        out.append(restate_one(*_inst(p, i), xi, None if gx is None else gx[i], T, tols))
    return out


def arbiter(p, x, gx=None, tols=DEFAULTS, status=None):
    """the longdouble restatement, its gradients from the dense KKT solve"""
    res = restate(p, x, gx, np.longdouble, tols, status)
    if gx is None:
        return res
    return [dense_kkt_gradients(res[i], p["H"][i], None if p["A"] is None else p["A"][i], p["eps_abs"], x[i], gx[i]) for i in range(p["B"])]


def cond_H(p):
    return [float(np.linalg.cond(np.tril(p["H"][i]) + np.tril(p["H"][i], -1).T + p["eps_abs"] * np.eye(p["n"]))) for i in range(p["B"])]


def worst_deviation(p, got, arb, names=("y",) + GRADS):
    """max over the named outputs and the instances of max|X - X*| / (cond2(H~) max|X*|) -> (figure, the output's name, instance).
    got: an Outputs, a list of restate_one results or a dict name -> [B][...] array"""
    cond = cond_H(p)
    worst = (0.0, "", -1)
    for name in names:
        for i in range(p["B"]):
            xs = arb[i][name]
            if isinstance(got, list):
                xg = got[i][name]
            else:
                xg = (got[name] if isinstance(got, dict) else getattr(got, name))[i]
            if xs.size == 0:
                continue
            err, scale = np.max(np.abs(np.asarray(xg, dtype=np.longdouble) - xs)), np.max(np.abs(xs))
            dev = float(err / (cond[i] * scale)) if scale > 0 else (0.0 if err == 0 else np.inf)   # an all-zero X*: X is to be zero too
            if dev > worst[0]:
                worst = (dev, name, i)
    return worst


if __name__ == "__main__":
    ref_w = res_w = emu_w = 0.0
    for p, x, y_ref, gx in fixture():
        arb = arbiter(p, x, gx)
        assert all(a["flag"] == OK for a in arb)
        a = worst_deviation(p, dict(y=y_ref), arb, names=("y",))
        b = worst_deviation(p, restate(p, x, gx), arb)
        c = worst_deviation(p, run_host(p, x, gx), arb)
        print(f"n = {p['n']:2d} nc = {p['nc']:2d} B = {p['B']}  cond2 <= {max(cond_H(p)):9.3e}  reference {a}  restatement {b}  emulated {c}")
        ref_w, res_w, emu_w = max(ref_w, a[0]), max(res_w, b[0]), max(emu_w, c[0])
    print(f"REFERENCE_WORST = {ref_w:.2e}\nRESTATEMENT_WORST = {res_w:.2e}\nEMULATED_WORST = {emu_w:.2e}")
