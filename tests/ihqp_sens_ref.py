"""tests/ihqp_sens_ref.py -- TEST INFRASTRUCTURE ONLY: what the tests of osot_ihqp_level_qp / osot_ihqp_sensitivity share.

  * the recipe of the host build tests/emu/ihqp_sens_host.cpp (the level-QP kernel, osot_qp_sens_kernel, the objective kernel and
    the pull-back kernel through the lock-step emulation, with the argument checks), built with native_build's flags, staleness rule and
    write-then-rename rule; and of the same file as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
    (statically linked runtimes, its own main: nothing is loaded into Python under a sanitizer);
  * the cases (a) .. (e): plans, switches and a seeded generator of their inputs; the fixture tests/golden/ihqp_sens.npz holds the
    inputs that were drawn, and per level x, y and the objective of the reference's own qpOASES (tests/golden/make_ihqp_sens_golden.py);
  * a numpy restatement of the level QP of include/osot_mi355x.h (osot_ihqp_level_qp) in any dtype, with the sums of absolute
    terms that bound what another summation order may change;
  * the struct of a case over host arrays or device tensors, sentinel-fenced destinations, and the run through the host build.

THE TOLERANCES.
  level QP ...... A, l, u and every bound that is copied are compared bit for bit.  An entry of H, of g or an optimality bound is a sum
                  of K products; any two summation orders (and any use of fma) are each within gamma_K = K u / (1 - K u), u = 2^-53,
                  of the exact sum times the sum of the absolute terms, so they differ by at most 2 gamma_K sum|terms|: that figure
                  is the bound, against the restatement in longdouble (whose own error is 2^-11 of that).  It is derived, not measured.
  y, active ..... in the units of qp_sens_ref: max|y - y*| / (cond2(H~) max|y*|) against its longdouble arbiter on the restated level
                  QP, with qp_sens_ref.SENS_TOL (the per-level kernel is the one measured there).  `python tests/ihqp_sens_ref.py`
                  measures the reference's own deviation on THIS fixture (REFERENCE_WORST below, printout in profiles/ihqp_sens.txt):
                  SENS_TOL here is the larger of qp_sens_ref.SENS_TOL and ten times that.  Never measured on the kernel under test.
  objective ..... relative 1e-12 against the restatement (longdouble); against the reference's getObjVal() ten times the
                  reference's own measured deviation from the restatement at ITS x (REFERENCE_OBJECTIVE_WORST).
  gradients ..... against the longdouble chain backward_arbiter: max|X - X*| <= SENS_TOL max|X*| times the product of cond2(H~_k) over
                  the levels traversed on the way to the output, plus the floor n u max|grad_dq| (assert_gradients says why)."""
import ctypes as C
import os
import shlex
import subprocess
import sys

import numpy as np

if __name__ == "__main__":     # `python tests/ihqp_sens_ref.py`: the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opensot_amd import abi
from opensot_amd.plan import Bound, Rows, StackPlan, Task, eps_abs_from_factor
import native_build
import qp_sens_ref

EMU = qp_sens_ref.EMU
GOLDEN = os.path.join(native_build.ROOT, "tests", "golden", "ihqp_sens.npz")
SOURCE = "ihqp_sens_host.cpp"
LIBRARY = "libosot_ihqp_sens_host.so"
PROGRAM = "ihqp_sens_asan"
SANITIZED = [w.replace("OSOT_QP_SENS_MAIN", "OSOT_IHQP_SENS_MAIN") for w in qp_sens_ref.SANITIZED]
SENTINEL = qp_sens_ref.SENTINEL
OK, DEGENERATE, SKIPPED = abi.SENS_OK, abi.SENS_DEGENERATE, abi.SENS_SKIPPED
EPS_FACTOR = 1e6
EPS_ABS = eps_abs_from_factor(EPS_FACTOR)
U = 2.0 ** -53

# measured on the CPU over the fixture (python tests/ihqp_sens_ref.py prints them; profiles/ihqp_sens.txt has the printout)
REFERENCE_WORST = 7.00e-16              # the reference's y, in units of cond2(H~) max|y*| (case b, level 2; qp_sens_ref's fixture: 6.09e-17)
REFERENCE_OBJECTIVE_WORST = 1.07e-15    # |getObjVal() - restated objective at the reference's x| / max(1, |objective|)
SENS_TOL = max(qp_sens_ref.SENS_TOL, 10.0 * REFERENCE_WORST)
OBJECTIVE_REL = 1e-12
OBJECTIVE_REF_TOL = 10.0 * REFERENCE_OBJECTIVE_WORST


# ---- 1. the host builds --------------------------------------------------------------------------------------------------------------
def _ensure(output, command):
    """native_build's staleness rule (this file and native_build.py are the recipe) and its write-then-rename rule"""
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
    """build tests/emu/libosot_ihqp_sens_host.so if it is stale, to a temporary name first"""
    return _ensure(LIBRARY, native_build.LOCKSTEP)


def ensure_sanitized():
    """the stand-alone program of the same file (-DOSOT_IHQP_SENS_MAIN) under ASan + UBSan"""
    return _ensure(PROGRAM, SANITIZED)


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(ensure())
        pp, cp = C.POINTER(abi.PlanDesc), C.POINTER(C.c_char_p)
        L.ihqp_host_level_rows.argtypes = [pp, C.c_int, C.POINTER(C.c_int)]
        L.ihqp_host_workspace_bytes.argtypes = [pp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
        L.ihqp_host_level_qp.argtypes = [pp, C.c_int, C.c_int, C.c_void_p, C.POINTER(abi.QpBatch), C.c_int, C.POINTER(abi.LevelQp), C.c_int, cp]
        L.ihqp_host_sensitivity.argtypes = [pp, C.c_int, C.c_int, C.c_void_p, C.POINTER(abi.IhqpSensBatch), C.POINTER(abi.QpSensOptions),
                                            C.c_int, cp]
        _lib = L
    return _lib


# ---- 2. the cases --------------------------------------------------------------------------------------------------------------------
class Case:
    """a plan, its batch size and switches: level_active (list of bool or None), task_active ({(level, task): bool} or None)"""

    def __init__(self, name, plan, B, level_active=None, task_active=None, box=0.6, b_scale=0.3, with_c=False):
        self.name, self.plan, self.B, self.level_active, self.task_active = name, plan, B, level_active, task_active
        self.box, self.b_scale = box, b_scale       # the generator's: l, u = -+ uniform(box / 2, box), b = b_scale N(0, 1)
        self.with_c = with_c                        # Task::getc() on the odd levels

    def active(self, k):
        return self.level_active is None or bool(self.level_active[k])

    def row_off(self, k):
        """[m_k] bool: the row belongs to a task that is switched off"""
        off = np.zeros(self.plan.m(k), dtype=bool)
        for j, t in enumerate(self.plan.levels[k]):
            if self.task_active is not None and not self.task_active.get((k, j), True):
                o = self.plan.task_row_offset(k, j)
                off[o:o + t.rows] = True
        return off

    def rows(self, k):
        return self.plan.nc + sum(self.plan.m(j) for j in range(k))

    def task_flags(self):
        import helpers
        return helpers.task_active_flags(self.task_active)


def _generic(rows, weight=1.0):
    return Task(abi.TASK_GENERIC, rows, weight=weight)


def cases():
    box = [Bound(abi.BOUND_GENERIC)]
    n = 33
    return {
        # n = 7, two levels of 3 and 4 rows, one stored row block, a box
        "a": Case("a", StackPlan(7, [[_generic(3)], [_generic(4)]], box, [Rows(abi.ROWS_GENERIC, 2)], eps_abs=EPS_ABS), 8),
        # the C3 shape on the NP = 32 layout: 3 / 24 / an implicit Postural block over every variable, box only
        "b": Case("b", StackPlan(32, [[_generic(3)], [_generic(24)], [Task(abi.TASK_POSTURAL, 32)]], box, [], eps_abs=EPS_ABS), 4),
        # the NP = 64 layout with a stored block, a unit-row block that is local to level 1 (only_level = 2), one inactive task and
        # level 1 switched off
        "c": Case("c", StackPlan(n, [[_generic(4), _generic(3, 0.5)], [_generic(5)], [_generic(6), Task(abi.TASK_POSTURAL, n)]], box,
                                 [Rows(abi.ROWS_GENERIC, 3), Rows(abi.ROWS_UNIT_GENERIC, 4, first_col=5, level=1)], eps_abs=EPS_ABS), 4,
                  level_active=[True, False, True], task_active={(0, 1): False}, b_scale=0.6),
        "d": Case("d", StackPlan(64, [[_generic(12)], [_generic(6), Task(abi.TASK_POSTURAL, 64)]], box, [Rows(abi.ROWS_GENERIC, 24)],
                                 eps_abs=EPS_ABS), 2, b_scale=0.6),
        # OSOT_MAX_LEVELS levels of one row: the chain's depth.  From level 6 on the optimality rows are dependent (n = 5).  A bound
        # that is active at one level stays tight, with a zero multiplier, once the rows above leave no freedom: with five variables
        # that is every instance, so this case's box is loose enough to stay inactive
        "e": Case("e", StackPlan(5, [[_generic(1)] for _ in range(abi.MAX_LEVELS)], box, [], eps_abs=EPS_ABS), 4, box=8.0),
    }


def extra_cases():
    """what the level QP holds besides the fixture's shapes; not in the fixture (the level QP alone is compared, at a seeded x)"""
    return {
        # a level with a non-diagonal weight, an identity-Jacobian regularisation task, c, a global unit-row block, no box
        "dense": Case("dense", StackPlan(9, [[Task(abi.TASK_GENERIC, 4, dense_weight=True)], [_generic(3), Task(abi.TASK_POSTURAL, 9)]], [],
                                         [Rows(abi.ROWS_UNIT_GENERIC, 2, first_col=1)], eps_abs=EPS_ABS,
                                         regularisation=Task(abi.TASK_GENERIC, 5, weight=0.3)), 3, with_c=True),
        # a regularisation task with a stored Jacobian; more stored rows than one tile holds
        "reg": Case("reg", StackPlan(34, [[_generic(40)], [_generic(2)]], [Bound(abi.BOUND_GENERIC)], [], eps_abs=EPS_ABS,
                                     regularisation=Task(abi.TASK_GENERIC, 3, weight=0.7), regularisation_dense=True), 2),
    }


def draw(case, rng, B):
    """the seeded inputs of B instances of a case: A[k], b[k], w[k] per level, C (the STORED rows), lo, up, l, u.  x = 0 is feasible."""
    p, n = case.plan, case.plan.n
    inp = dict(A=[], b=[], w=[])
    for k in range(p.L):
        inp["A"].append(rng.normal(size=(B, p.ma(k), n)) if p.ma(k) else None)
        inp["b"].append(case.b_scale * rng.normal(size=(B, p.m(k))))
        w = rng.uniform(0.5, 1.5, size=(B, p.m(k)))
        for j, t in enumerate(p.levels[k]):
            o = p.task_row_offset(k, j)
            w[:, o:o + t.rows] *= t.weight
        inp["w"].append(w)
    inp["C"] = 0.3 * rng.normal(size=(B, p.nc_stored, n)) if p.nc_stored else None
    inp["lo"] = -rng.uniform(0.3, 1.0, size=(B, p.nc)) if p.nc else None
    inp["up"] = rng.uniform(0.3, 1.0, size=(B, p.nc)) if p.nc else None
    inp["l"] = -rng.uniform(0.5 * case.box, case.box, size=(B, n)) if p.bounds else None
    inp["u"] = rng.uniform(0.5 * case.box, case.box, size=(B, n)) if p.bounds else None
    if any(p.dense_level(k) for k in range(p.L)):      # W_k A_k and W_k b_k of the levels with a non-diagonal weight (W_k = M M' + I)
        inp["WA"], inp["Wb"] = [None] * p.L, [None] * p.L
        for k in range(p.L):
            if p.dense_level(k):
                M = rng.normal(size=(B, p.m(k), p.m(k)))
                W = M @ np.transpose(M, (0, 2, 1)) + np.eye(p.m(k))
                inp["WA"][k] = W[:, :p.ma(k), :p.ma(k)] @ inp["A"][k]
                inp["Wb"][k] = np.einsum("brs,bs->br", W, inp["b"][k])
    if p.regularisation is not None:
        inp["reg"] = dict(b=rng.normal(size=(B, p.regularisation.rows)),
                          A=rng.normal(size=(B, p.regularisation.rows, n)) if p.regularisation_dense else None)
    if case.with_c:
        inp["c"] = [0.1 * rng.normal(size=(B, n)) if k % 2 else None for k in range(p.L)]
    return inp


def fixture():
    """{name: dict(inp, x_levels [B][L][n], y [k] -> [B][n + rows_k], objective [B][L], grad_dq [B][n])} of tests/golden/ihqp_sens.npz
    (grad_dq: a seeded upstream gradient, kept with the inputs for a backward pass through the cascade; no test reads it yet)"""
    out = {}
    with np.load(GOLDEN) as z:
        assert float(z["eps_abs"]) == EPS_ABS
        for name, case in cases().items():
            p = case.plan
            get = lambda k: z[f"{name}_{k}"] if f"{name}_{k}" in z.files else None
            inp = dict(A=[get(f"A{k}") for k in range(p.L)], b=[get(f"b{k}") for k in range(p.L)], w=[get(f"w{k}") for k in range(p.L)],
                       C=get("C"), lo=get("lo"), up=get("up"), l=get("l"), u=get("u"))
            assert inp["l"].shape == (case.B, p.n)
            out[name] = dict(inp=inp, x_levels=get("x_levels"), y=[get(f"y{k}") for k in range(p.L)], objective=get("objective"),
                             grad_dq=get("grad_dq"))
    return out


# ---- 3. the restatement of the level QP ----------------------------------------------------------------------------------------------
def restate_level_qp(case, inp, i, k, x_levels, T=np.float64):
    """the QP of level k of instance i (include/osot_mi355x.h: osot_ihqp_level_qp) in dtype T -> dict(H, g, A, lA, uA, l, u) and, for
    the tolerance, Habs / gabs / babs (the sums of the absolute terms of every entry of H, g and of every optimality bound) and
    K (the longest sum).  x_levels: [L][n] of the instance"""
    p, n = case.plan, case.plan.n
    m, ma = p.m(k), p.ma(k)
    off = case.row_off(k)
    w = inp["w"][k][i].astype(T) * ~off
    b = inp["b"][k][i].astype(T)
    H, g = np.zeros((n, n), dtype=T), np.zeros(n, dtype=T)
    Habs, gabs = np.zeros((n, n), dtype=T), np.zeros(n, dtype=T)
    if ma:
        A = inp["A"][k][i].astype(T) * ~off[:ma, None]
        if inp.get("WA") is not None and inp["WA"][k] is not None:       # a non-diagonal weight: W_k A_k and W_k b_k are inputs
            WA, Wb = inp["WA"][k][i].astype(T) * ~off[:ma, None], inp["Wb"][k][i].astype(T)
            g -= A.T @ Wb[:ma]
            gabs += np.abs(A).T @ np.abs(Wb[:ma])
        else:
            WA = w[:ma, None] * A
            g -= WA.T @ b[:ma]
            gabs += np.abs(WA).T @ np.abs(b[:ma])
        H += np.tril(WA.T @ A) + np.tril(WA.T @ A, -1).T                 # (i, j) = sum_r WA[r][max(i, j)] A[r][min(i, j)]
        Habs += np.tril(np.abs(WA).T @ np.abs(A)) + np.tril(np.abs(WA).T @ np.abs(A), -1).T
    reg = inp.get("reg")
    if reg is not None:                         # the regularisation task, at every level
        wr, br = T(p.regularisation.weight), reg["b"][i].astype(T)
        if reg.get("A") is not None:
            Ar = reg["A"][i].astype(T)
            H += wr * (Ar.T @ Ar)
            g -= wr * (Ar.T @ br)
            Habs += wr * (np.abs(Ar).T @ np.abs(Ar))
            gabs += wr * (np.abs(Ar).T @ np.abs(br))
        else:
            idx = np.arange(p.regularisation.rows)
            H[idx, idx] += wr
            g[idx] -= wr * br
            Habs[idx, idx] += wr
            gabs[idx] += np.abs(wr * br)
    if inp.get("c") is not None and inp["c"][k] is not None:
        g += inp["c"][k][i].astype(T)
        gabs += np.abs(inp["c"][k][i])
    npost = m - ma
    if npost:                                   # the implicit Postural block: A = [I 0]
        idx = np.arange(npost)
        H[idx, idx] += w[ma:]
        g[:npost] -= w[ma:] * b[ma:]
        Habs[idx, idx] += np.abs(w[ma:])
        gabs[:npost] += np.abs(w[ma:] * b[ma:])
    rows = case.rows(k)
    A_, lA, uA, babs = np.zeros((rows, n), dtype=T), np.full(rows, -1e20, dtype=T), np.full(rows, 1e20, dtype=T), np.zeros(rows, dtype=T)
    r = s = 0
    for blk in p.rowblocks:                     # the global rows in plan order
        on = blk.level is None or blk.level == k
        stored = blk.kind not in (abi.ROWS_UNIT_GENERIC,)
        for q in range(blk.rows):
            if on:
                if stored:
                    A_[r] = inp["C"][i, s + q]
                else:
                    A_[r, blk.first_col + q] = 1.0
                lA[r], uA[r] = np.clip(inp["lo"][i, r], -1e20, 1e20), np.clip(inp["up"][i, r], -1e20, 1e20)
            r += 1
        if stored:
            s += blk.rows
    for j in range(k):                          # the optimality rows of the levels above
        mj, maj = p.m(j), p.ma(j)
        if not case.active(j):
            lA[r:r + mj], uA[r:r + mj] = -1.0, 1.0
            r += mj
            continue
        offj = case.row_off(j)
        xj = x_levels[j].astype(T)
        Aj = np.zeros((mj, n), dtype=T)
        if maj:
            Aj[:maj] = inp["A"][j][i]
        Aj[np.arange(maj, mj), np.arange(mj - maj)] = 1.0
        for q in range(mj):
            if not offj[q]:
                A_[r + q] = Aj[q]
                lA[r + q] = uA[r + q] = Aj[q] @ xj
                babs[r + q] = np.abs(Aj[q]) @ np.abs(xj)
        r += mj
    assert r == rows
    l = np.full(n, -1e20, dtype=T) if inp["l"] is None else np.clip(inp["l"][i], -1e20, 1e20).astype(T)
    u = np.full(n, 1e20, dtype=T) if inp["u"] is None else np.clip(inp["u"][i], -1e20, 1e20).astype(T)
    K = max(ma + (p.regularisation.rows if reg is not None else 0) + 4, n) + 2
    return dict(H=H, g=g, A=A_, lA=lA, uA=uA, l=l, u=u, Habs=Habs, gabs=gabs, babs=babs, K=K)


def gamma(K):
    return K * U / (1.0 - K * U)


def objective_of(qp, x, eps_abs=EPS_ABS, T=np.longdouble):
    x = x.astype(T)
    return float(0.5 * x @ ((qp["H"].astype(T) + T(eps_abs) * np.eye(len(x), dtype=T)) @ x) + qp["g"].astype(T) @ x)


def level_problem(case, inp, k, x_levels, T=np.float64):
    """the restated QPs of level k of every instance as a qp_sens_ref problem"""
    B = x_levels.shape[0]
    qs = [restate_level_qp(case, inp, i, k, x_levels[i], T) for i in range(B)]
    st = lambda key: np.stack([q[key] for q in qs]).astype(np.float64)
    rows = case.rows(k)
    return qp_sens_ref.problem(st("H"), st("g"), st("A") if rows else None, st("lA") if rows else None, st("uA") if rows else None,
                               st("l"), st("u"), EPS_ABS)


# ---- 4. the struct of a case, destinations, the host run ---------------------------------------------------------------------------------
PAD = 2


def qp_batch(case, arrays, address, B):
    """abi.QpBatch over `arrays` (A, b, w lists; C, lo, up, l, u, dq, x_levels, status; numpy arrays or device tensors);
    address(a) -> the pointer the kernels are given.  The caller keeps `arrays` alive."""
    qb = abi.QpBatch()
    qb.B = B
    for k in range(case.plan.L):
        for name in ("A", "b", "w", "c", "WA", "Wb"):
            if arrays.get(name) is not None and arrays[name][k] is not None:
                getattr(qb, name)[k] = address(arrays[name][k])
    for name in ("C", "lo", "up", "l", "u", "dq", "x_levels", "status"):
        if arrays.get(name) is not None:
            setattr(qb, name, address(arrays[name]))
    if arrays.get("reg") is not None:
        qb.b_reg = address(arrays["reg"]["b"])
        if arrays["reg"].get("A") is not None:
            qb.A_reg = address(arrays["reg"]["A"])
    if case.level_active is not None:
        act = (C.c_ubyte * case.plan.L)(*[1 if a else 0 for a in case.level_active])
        arrays["_level_active"] = act
        qb.level_active = C.addressof(act)
    return qb


def host_arrays(case, inp, x_levels, status=None):
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    B = x_levels.shape[0]
    conv = lambda v: [c(a) for a in v] if isinstance(v, list) else ({kk: c(a) for kk, a in v.items()} if isinstance(v, dict) else c(v))
    arr = {k: conv(v) for k, v in inp.items()}
    arr["x_levels"] = c(x_levels)
    arr["dq"] = c(x_levels[:, -1])
    arr["status"] = np.zeros(B, dtype=np.int32) if status is None else np.ascontiguousarray(status, dtype=np.int32)
    return arr


class Fenced:
    """a sentinel-filled destination with PAD spare entries in front of and behind it"""

    def __init__(self, shape, ints=False):
        self.sentinel = -7 if ints else SENTINEL
        self.raw = np.full(int(np.prod(shape)) + 2 * PAD, self.sentinel, dtype=np.int32 if ints else np.float64)
        self.shape = tuple(shape)

    @property
    def value(self):
        return self.raw[PAD:len(self.raw) - PAD].reshape(self.shape)

    @property
    def address(self):
        return self.raw.ctypes.data + PAD * self.raw.itemsize

    def intact(self):
        return bool(np.all(self.raw[:PAD] == self.sentinel) and np.all(self.raw[-PAD:] == self.sentinel))

    def untouched(self):
        return bool(np.all(self.raw == self.sentinel))


def host_level_rows(case, k):
    rows = C.c_int(-1)
    pd = case.plan.to_c()
    assert lib().ihqp_host_level_rows(C.byref(pd), k, C.byref(rows)) == abi.OK
    return rows.value


def host_workspace_bytes(case, B, backward=False, grad_A=False):
    v = C.c_ulonglong(0)
    pd = case.plan.to_c()
    assert lib().ihqp_host_workspace_bytes(C.byref(pd), B, int(backward), int(grad_A), C.byref(v)) == abi.OK
    return v.value


def host_level_qp(case, inp, k, x_levels):
    """osot_ihqp_level_qp through the emulated kernel -> dict of Fenced (H, g, A, lA, uA, l, u)"""
    B, n, rows = x_levels.shape[0], case.plan.n, case.rows(k)
    arr = host_arrays(case, inp, x_levels)
    qb = qp_batch(case, arr, lambda a: a.ctypes.data, B)
    out = dict(H=Fenced((B, n, n)), g=Fenced((B, n)), A=Fenced((B, rows, n)), lA=Fenced((B, rows)), uA=Fenced((B, rows)), l=Fenced((B, n)),
               u=Fenced((B, n)))
    lq = abi.LevelQp()
    for key, f in out.items():
        setattr(lq, key, f.address)
    why = C.c_char_p()
    pd = case.plan.to_c()
    ta = case.task_flags()
    rc = lib().ihqp_host_level_qp(C.byref(pd), 0, B, None if ta is None else ta.ctypes.data, C.byref(qb), k, C.byref(lq), 1, C.byref(why))
    assert rc == abi.OK, why.value
    return out


class SensOutputs:
    """the destinations of osot_ihqp_sensitivity for a case, fenced; want: the names that are bound ("y", "active", "flag",
    "objective")"""

    def __init__(self, case, B, want=("y", "active", "flag", "objective"), workspace_bytes=None, fenced=Fenced):
        p, n = case.plan, case.plan.n
        self.want = tuple(want)
        self.y = [fenced((B, n + case.rows(k))) for k in range(p.L)]
        self.active = [fenced((B, n + case.rows(k)), ints=True) for k in range(p.L)]
        self.flag = [fenced((B,), ints=True) for k in range(p.L)]
        self.objective = fenced((B, p.L))
        self.workspace = fenced((workspace_bytes // 8,)) if workspace_bytes is not None else None

    def struct(self, qb):
        s = abi.IhqpSensBatch()
        s.qp = qb
        for k in range(len(self.y)):
            if "y" in self.want:
                s.y[k] = self.y[k].address
            if "active" in self.want:
                s.active[k] = self.active[k].address
            if "flag" in self.want:
                s.flag[k] = self.flag[k].address
        if "objective" in self.want:
            s.objective = self.objective.address
        if self.workspace is not None:
            s.workspace, s.workspace_bytes = self.workspace.address, self.workspace.value.size * 8
        return s

    def fences_intact(self):
        every = self.y + self.active + self.flag + [self.objective] + ([self.workspace] if self.workspace is not None else [])
        bound = lambda f: (any(f is a for a in self.y) and "y" in self.want) or (any(f is a for a in self.active) and "active" in self.want) or \
            (any(f is a for a in self.flag) and "flag" in self.want) or (f is self.objective and "objective" in self.want) or f is self.workspace
        return all(f.intact() if bound(f) else f.untouched() for f in every)


def host_check(case, sens, opts=None, wide=0, max_batch=None):
    """osot_ihqp_sensitivity's answer to its arguments, from the host build -> (code, reason)"""
    why = C.c_char_p()
    pd = case.plan.to_c()
    ta = case.task_flags()
    rc = lib().ihqp_host_sensitivity(C.byref(pd), wide, sens.qp.B if max_batch is None else max_batch, None if ta is None else ta.ctypes.data,
                                     C.byref(sens), None if opts is None else C.byref(opts), 0, C.byref(why))
    return rc, (why.value or b"").decode()


def host_sensitivity(case, inp, x_levels, status=None, want=("y", "active", "flag", "objective")):
    """osot_ihqp_sensitivity through the emulated kernels -> SensOutputs"""
    B = x_levels.shape[0]
    arr = host_arrays(case, inp, x_levels, status)
    qb = qp_batch(case, arr, lambda a: a.ctypes.data, B)
    out = SensOutputs(case, B, want, host_workspace_bytes(case, B))
    s = out.struct(qb)
    why = C.c_char_p()
    pd = case.plan.to_c()
    ta = case.task_flags()
    rc = lib().ihqp_host_sensitivity(C.byref(pd), 0, B, None if ta is None else ta.ctypes.data, C.byref(s), None, 1, C.byref(why))
    assert rc == abi.OK, why.value
    return out


# ---- 5. the comparisons (shared by the host and the device tests) -----------------------------------------------------------------------
def assert_level_qp(case, inp, k, x_levels, got):
    """got: dict name -> [B][...] arrays of the materialised level QP"""
    worst = 0.0
    for i in range(x_levels.shape[0]):
        q = restate_level_qp(case, inp, i, k, x_levels[i], np.longdouble)
        g2 = 2.0 * gamma(q["K"])
        for name in ("A", "l", "u"):
            assert np.array_equal(got[name][i], q[name].astype(np.float64)), (case.name, k, i, name)
        copied = q["babs"] == 0                  # every bound that is copied or set: bit for bit
        for name in ("lA", "uA"):
            assert np.array_equal(got[name][i][copied], q[name].astype(np.float64)[copied]), (case.name, k, i, name)
            err, bound = np.abs(got[name][i][~copied] - q[name][~copied]), g2 * q["babs"][~copied]
            assert np.all(err <= bound), (case.name, k, i, name, float(np.max(err / bound)))
            worst = max(worst, float(np.max(err / bound, initial=0.0)))
        for name, ab in (("H", "Habs"), ("g", "gabs")):
            err, bound = np.abs(got[name][i] - q[name]), g2 * q[ab]
            assert np.all(err <= bound), (case.name, k, i, name, float(np.max(err - bound)))
            worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0))))
        assert np.array_equal(got["H"][i], got["H"][i].T)                 # symmetric to the bit
    return worst


def stationarity(p, i, x, y):
    """|H~ x + g - y_b - A'y_c|_inf of instance i of a qp_sens_ref problem, in longdouble, and the scale sum|terms|_inf"""
    T = np.longdouble
    n = p["n"]
    Ht = p["H"][i].astype(T) + T(p["eps_abs"]) * np.eye(n, dtype=T)
    r = Ht @ x.astype(T) + p["g"][i].astype(T) - y[:n].astype(T)
    scale = np.abs(Ht) @ np.abs(x.astype(T)) + np.abs(p["g"][i]) + np.abs(y[:n])
    if p["nc"]:
        r -= p["A"][i].astype(T).T @ y[n:].astype(T)
        scale += np.abs(p["A"][i]).T @ np.abs(y[n:])
    return float(np.max(np.abs(r))), float(np.max(scale))


def assert_multipliers(case, inp, x_levels, status, y, active, flag, objective, require_ok=True):
    """y / active / flag per level and objective [B][L] against the arbiter on the restated level QPs.  Where the arbiter's set is
    unique (flag OK) y and the set are compared; where it says DEGENERATE (dependent optimality rows: the multipliers are not
    unique) the flag is compared and y by the stationarity residual |H~x + g - y_b - A'y_c| <= cond2(H~) SENS_TOL sum|terms|.
    -> the worst deviation in units of SENS_TOL"""
    p, B = case.plan, x_levels.shape[0]
    worst = 0.0
    solved = np.ones(B, dtype=bool) if status is None else (np.asarray(status) == 0)
    for k in range(p.L):
        if not case.active(k):
            assert np.all(flag[k] == SKIPPED) and np.all(y[k] == 0.0) and np.all(active[k] == 0) and np.all(objective[:, k] == 0.0)
            continue
        prob = level_problem(case, inp, k, x_levels)
        arb = qp_sens_ref.arbiter(prob, x_levels[:, k], status=None if status is None else np.asarray(status))
        cond = qp_sens_ref.cond_H(prob)
        for i in range(B):
            if not solved[i]:
                assert flag[k][i] == SKIPPED and np.all(y[k][i] == 0.0) and np.all(active[k][i] == 0) and objective[i, k] == 0.0
                continue
            assert flag[k][i] == arb[i]["flag"], (case.name, k, i, flag[k][i], arb[i]["flag"])
            if require_ok:
                assert arb[i]["flag"] == OK, (case.name, k, i)
            if arb[i]["flag"] == OK:
                ys = arb[i]["y"]
                dev = float(np.max(np.abs(y[k][i] - ys)) / (cond[i] * max(float(np.max(np.abs(ys))), 1e-300)))
                assert np.array_equal(active[k][i], arb[i]["active"]), (case.name, k, i)
            else:
                res, scale = stationarity(prob, i, x_levels[i, k], y[k][i])
                dev = res / (cond[i] * scale)
            worst = max(worst, dev / SENS_TOL)
            assert dev <= SENS_TOL, (case.name, k, i, dev, SENS_TOL)
            f = objective_of(restate_level_qp(case, inp, i, k, x_levels[i], np.longdouble), x_levels[i, k])
            assert abs(objective[i, k] - f) <= OBJECTIVE_REL * max(1.0, abs(f)), (case.name, k, i, objective[i, k], f)
    return worst


# ---- 6. the backward pass ----------------------------------------------------------------------------------------------------------------
GRAD_LEVEL = ("b", "w", "c", "A")              # one per level
GRAD_GLOBAL = ("C", "lo", "up", "l", "u")


class GradOutputs:
    """fenced destinations of the gradient outputs of a case; want: names of GRAD_LEVEL + GRAD_GLOBAL that are bound"""

    def __init__(self, case, B, want=GRAD_LEVEL + GRAD_GLOBAL, fenced=Fenced):
        p, n = case.plan, case.plan.n
        self.want = tuple(want)
        self.b = [fenced((B, p.m(k))) for k in range(p.L)]
        self.w = [fenced((B, p.m(k))) for k in range(p.L)]
        self.c = [fenced((B, n)) for k in range(p.L)]
        self.A = [fenced((B, p.ma(k), n)) if p.ma(k) else None for k in range(p.L)]
        self.C = fenced((B, p.nc_stored, n)) if p.nc_stored else None
        self.lo = fenced((B, p.nc)) if p.nc else None
        self.up = fenced((B, p.nc)) if p.nc else None
        self.l, self.u = fenced((B, n)), fenced((B, n))

    def every(self):
        out = []
        for name in GRAD_LEVEL:
            out += [(name, f) for f in getattr(self, name) if f is not None]
        return out + [(name, getattr(self, name)) for name in GRAD_GLOBAL if getattr(self, name) is not None]

    def bind(self, s):
        for k in range(len(self.b)):
            for name in GRAD_LEVEL:
                f = getattr(self, name)[k]
                if name in self.want and f is not None:
                    getattr(s, "grad_" + name)[k] = f.address
        for name in GRAD_GLOBAL:
            f = getattr(self, name)
            if name in self.want and f is not None:
                setattr(s, "grad_" + name, f.address)

    def wants_A(self):
        return ("A" in self.want and any(f is not None for f in self.A)) or ("C" in self.want and self.C is not None)

    def fences_intact(self):
        return all(f.intact() if name in self.want else f.untouched() for name, f in self.every())

    def values(self):
        """dict name -> list per level (GRAD_LEVEL) or array (GRAD_GLOBAL); None where there is no such buffer"""
        v = {name: [None if f is None else f.value for f in getattr(self, name)] for name in GRAD_LEVEL}
        v.update({name: (None if getattr(self, name) is None else getattr(self, name).value) for name in GRAD_GLOBAL})
        return v


def host_backward(case, inp, x_levels, grad_dq, status=None, want=GRAD_LEVEL + GRAD_GLOBAL):
    """osot_ihqp_sensitivity with grad_dq through the emulated kernels -> (SensOutputs, GradOutputs)"""
    B = x_levels.shape[0]
    arr = host_arrays(case, inp, x_levels, status)
    qb = qp_batch(case, arr, lambda a: a.ctypes.data, B)
    grads = GradOutputs(case, B, want)
    out = SensOutputs(case, B, workspace_bytes=host_workspace_bytes(case, B, True, grads.wants_A()))
    s = out.struct(qb)
    gdq = np.ascontiguousarray(grad_dq, dtype=np.float64)
    s.grad_dq = gdq.ctypes.data
    grads.bind(s)
    why = C.c_char_p()
    pd = case.plan.to_c()
    ta = case.task_flags()
    rc = lib().ihqp_host_sensitivity(C.byref(pd), 0, B, None if ta is None else ta.ctypes.data, C.byref(s), None, 1, C.byref(why))
    assert rc == abi.OK, why.value
    return out, grads


def _level_rows_matrix(case, inp, i, j, T):
    """A_j of instance i in full ([m_j][n], the implicit Postural block as unit rows, the rows of an inactive task zero)"""
    p, n = case.plan, case.plan.n
    mj, maj = p.m(j), p.ma(j)
    Aj = np.zeros((mj, n), dtype=T)
    if maj:
        Aj[:maj] = inp["A"][j][i]
    Aj[np.arange(maj, mj), np.arange(mj - maj)] = 1.0
    Aj[case.row_off(j)] = 0.0
    return Aj


def backward_arbiter(case, inp, i, x_levels, grad_dq):
    """the longdouble chain of instance i: per level, from the last active one down, qp_sens_ref's longdouble arbiter on the restated
    level QP with grad_x = gx_k and its DENSE KKT solve for the gradients, linked by the formulas of include/osot_mi355x.h
    -> (dict of gradients as GradOutputs.values() of one instance, [flag per level], [cond2(H~_k) per level, 0 for a level that is off])"""
    T = np.longdouble
    p, n, L = case.plan, case.plan.n, case.plan.L
    G = dict(b=[np.zeros(p.m(k), dtype=T) for k in range(L)], w=[np.zeros(p.m(k), dtype=T) for k in range(L)],
             c=[np.zeros(n, dtype=T) for k in range(L)], A=[np.zeros((p.ma(k), n), dtype=T) if p.ma(k) else None for k in range(L)],
             C=np.zeros((p.nc_stored, n), dtype=T) if p.nc_stored else None, lo=np.zeros(p.nc, dtype=T) if p.nc else None,
             up=np.zeros(p.nc, dtype=T) if p.nc else None, l=np.zeros(n, dtype=T), u=np.zeros(n, dtype=T))
    gx = np.zeros((L, n), dtype=T)
    live = [k for k in range(L) if case.active(k)]
    gx[live[-1]] = grad_dq
    flags, conds = [SKIPPED] * L, [0.0] * L
    stored_rows = []                       # QP row of every stored global row, in the order of C
    r = 0
    for blk in p.rowblocks:
        if blk.kind != abi.ROWS_UNIT_GENERIC:
            stored_rows += list(range(r, r + blk.rows))
        r += blk.rows
    for k in reversed(live):
        q = restate_level_qp(case, inp, i, k, x_levels, T)
        rows = case.rows(k)
        xk = x_levels[k].astype(T)
        args = (q["H"], q["g"], q["A"] if rows else None, q["lA"] if rows else None, q["uA"] if rows else None, q["l"], q["u"], EPS_ABS)
        R = qp_sens_ref.restate_one(*args, xk, gx[k], T)
        R = qp_sens_ref.dense_kkt_gradients(R, q["H"], q["A"] if rows else None, EPS_ABS, xk, gx[k])
        flags[k] = R["flag"]
        conds[k] = float(np.linalg.cond((q["H"] + T(EPS_ABS) * np.eye(n, dtype=T)).astype(np.float64)))
        dx = R["grad_g"]
        Ak = _level_rows_matrix(case, inp, i, k, T)
        w = inp["w"][k][i].astype(T) * ~case.row_off(k)
        s, t = Ak @ xk, Ak @ dx
        e = s - inp["b"][k][i].astype(T)
        G["b"][k] = -w * t
        G["w"][k] = np.where(case.row_off(k), 0, t * e)
        G["c"][k] = dx.copy()
        if p.ma(k):
            ma = p.ma(k)
            G["A"][k] += (w[:ma] * e[:ma])[:, None] * dx[None, :] + (w[:ma] * t[:ma])[:, None] * xk[None, :]
        if p.nc:
            G["lo"] += R["grad_lA"][:p.nc]
            G["up"] += R["grad_uA"][:p.nc]
        if p.nc_stored:
            G["C"] += R["grad_A"][stored_rows]
        G["l"] += R["grad_l"]
        G["u"] += R["grad_u"]
        off = p.nc
        for j in range(k):
            mj, maj = p.m(j), p.ma(j)
            if case.active(j):
                rho = R["grad_lA"][off:off + mj] + R["grad_uA"][off:off + mj]
                gx[j] += _level_rows_matrix(case, inp, i, j, T).T @ rho
                if maj:
                    G["A"][j] += R["grad_A"][off:off + maj] + rho[:maj, None] * x_levels[j].astype(T)[None, :]
            off += mj
    return G, flags, conds


def assert_gradients(case, inp, x_levels, grad_dq, got, flag, status=None):
    """got: GradOutputs.values() of all instances; flag: per level [B].  Every gradient against the longdouble chain:
    max|X - X*| <= SENS_TOL max|X*| prod cond2(H~_k) over the levels ACTUALLY TRAVERSED on the way to it -- the active levels from the
    last one down to the level the output belongs to (the summed outputs C, lo, up, l, u: down to the first active level).  Where the
    rows above leave a level no freedom (case e from level 5 on) the exact gradient is ZERO and the arbiter's is its own round-off
    (1e-28): a relative bound means nothing there, so every bound carries the absolute floor n u max|grad_dq|, u = 2^-53 -- n
    rounding units of the upstream gradient, below which a float64 result computed from grad_dq is zero to its inputs' resolution.  An
    instance that was not solved: zero gradients.  -> (the worst |X - X*| / bound, its name, level, instance)"""
    p, B = case.plan, x_levels.shape[0]
    worst = (0.0, "", -1, -1)
    for i in range(B):
        if status is not None and status[i] != 0:
            for name in GRAD_LEVEL:
                assert all(np.all(g[i] == 0.0) for g in got[name] if g is not None), (name, i)
            assert all(np.all(got[name][i] == 0.0) for name in GRAD_GLOBAL if got[name] is not None), i
            continue
        G, flags, conds = backward_arbiter(case, inp, i, x_levels[i], grad_dq[i])
        live = [k for k in range(p.L) if case.active(k)]
        for k in live:
            assert flag[k][i] == flags[k], (case.name, k, i, flag[k][i], flags[k])
        through = lambda k: float(np.prod([conds[j] for j in live if j >= k]))
        floor = p.n * U * float(np.max(np.abs(grad_dq[i])))
        checks = [(name, k, got[name][k][i], G[name][k], through(k)) for name in GRAD_LEVEL for k in range(p.L) if G[name][k] is not None]
        checks += [(name, -1, got[name][i], G[name], through(live[0])) for name in GRAD_GLOBAL if G[name] is not None]
        for name, k, x, xs, cond in checks:
            if k >= 0 and not case.active(k):
                assert np.all(x == 0.0), (name, k, i)
                continue
            err, scale = float(np.max(np.abs(x - xs), initial=0.0)), float(np.max(np.abs(xs), initial=0.0))
            bound = SENS_TOL * cond * scale + floor
            assert err <= bound, (case.name, name, k, i, err, bound)
            if bound > 0 and err / bound > worst[0]:
                worst = (err / bound, name, k, i)
    return worst


if __name__ == "__main__":
    ref_w = obj_w = emu_w = 0.0
    for name, fx in fixture().items():
        case = cases()[name]
        for k in range(case.plan.L):
            if not case.active(k):
                continue
            prob = level_problem(case, fx["inp"], k, fx["x_levels"])
            arb = qp_sens_ref.arbiter(prob, fx["x_levels"][:, k])
            ok = [i for i in range(case.B) if arb[i]["flag"] == OK]
            pk ={key: (v[ok] if isinstance(v, np.ndarray) else v) for key, v in prob.items()}
            pk["B"] = len(ok)
            a = qp_sens_ref.worst_deviation(pk, dict(y=fx["y"][k][ok]), [arb[i] for i in ok], names=("y",)) if ok else (0.0, "", -1)
            o = max(abs(fx["objective"][i, k] - objective_of(restate_level_qp(case, fx["inp"], i, k, fx["x_levels"][i], np.longdouble),
                                                             fx["x_levels"][i, k])) / max(1.0, abs(fx["objective"][i, k])) for i in range(case.B))
            print(f"case {name} level {k}: n = {case.plan.n:2d} rows = {case.rows(k):3d} unique sets {len(ok)}/{case.B} "
                  f"cond2 <= {max(qp_sens_ref.cond_H(prob)):9.3e}  reference y {a[0]:.3e}  reference objective {o:.3e}")
            ref_w, obj_w = max(ref_w, a[0]), max(obj_w, o)
        out = host_sensitivity(case, fx["inp"], fx["x_levels"])
        emu_w = max(emu_w, SENS_TOL * assert_multipliers(case, fx["inp"], fx["x_levels"], None, [f.value for f in out.y],
                                                         [f.value for f in out.active], [f.value for f in out.flag], out.objective.value,
                                                         require_ok=name != "e"))
    print(f"REFERENCE_WORST = {ref_w:.2e}\nREFERENCE_OBJECTIVE_WORST = {obj_w:.2e}\nEMULATED_WORST = {emu_w:.2e} (for the record)\n"
          f"qp_sens_ref.SENS_TOL = {qp_sens_ref.SENS_TOL:.2e}  SENS_TOL = {SENS_TOL:.2e}")
