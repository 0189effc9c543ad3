"""tests/ihqp_sens_wide_ref.py -- TEST INFRASTRUCTURE ONLY: what the tests of osot_ihqp_level_qp / osot_ihqp_sensitivity on a handle of
osot_solver_create_wide (65 .. 128 variables) share.

  * the recipe of the host build tests/emu/ihqp_sens_wide_host.cpp (the level-QP, objective and pull-back functions of
    opensot_amd/csrc/osot_ihqp_sens_wide.h and sensbig::run, as a team of one thread or a turn-taking team of several, with the
    checks of the two entries), built with native_build's flags, staleness rule and write-then-rename rule; and of the same file as a
    stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (statically linked runtimes, its own main: nothing is
    loaded into Python under a sanitizer);
  * the cases (p) .. (t) and the n = 65 twins of ihqp_sens_ref's extra cases; the fixture tests/golden/ihqp_sens_wide.npz
    (tests/golden/make_ihqp_sens_wide_golden.py) and the runs through the host build.

Case, draw, the restatement of the level QP, the longdouble arbiters (assert_multipliers, backward_arbiter, assert_gradients), the
structs and the fenced destinations are ihqp_sens_ref's: they do not depend on the width.

THE TOLERANCES are ihqp_sens_ref's, stated there.  SENS_TOL is the largest of ihqp_sens_ref.SENS_TOL, qp_sens_big_ref.SENS_BIG_TOL and
ten times the reference's own deviation measured on THIS fixture (`python tests/ihqp_sens_wide_ref.py` prints REFERENCE_WORST and
REFERENCE_OBJECTIVE_WORST; profiles/ihqp_sens_wide.txt has the printout); ten is the margin this project gives a different summation
order.  Never measured on the kernel under test.  assert_multipliers and assert_gradients of ihqp_sens_ref carry ihqp_sens_ref.SENS_TOL:
the assertion below holds them to this file's figure."""
import ctypes as C
import os
import shlex
import subprocess
import sys

import numpy as np

if __name__ == "__main__":     # `python tests/ihqp_sens_wide_ref.py`: the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opensot_amd import abi
from opensot_amd.plan import Bound, Rows, StackPlan, Task
import native_build
import ihqp_sens_ref as R
import qp_sens_big_ref
import qp_sens_ref
from ihqp_sens_ref import (Case, draw, restate_level_qp, backward_arbiter, assert_gradients, assert_multipliers, assert_level_qp,   # noqa: F401
                           level_problem, objective_of, qp_batch, host_arrays, Fenced, SensOutputs, GradOutputs, GRAD_LEVEL, GRAD_GLOBAL,
                           EPS_FACTOR, EPS_ABS, OK, DEGENERATE, SKIPPED, OBJECTIVE_REL)

EMU = R.EMU
GOLDEN = os.path.join(native_build.ROOT, "tests", "golden", "ihqp_sens_wide.npz")
SOURCE = "ihqp_sens_wide_host.cpp"
LIBRARY = "libosot_ihqp_sens_wide_host.so"
PROGRAM = "ihqp_sens_wide_asan"
SHARED = native_build.LOCKSTEP + ["-pthread"]
SANITIZED = ["g++", "-O1", "-g", "-std=c++17", "-DOSOT_EMULATION", "-DOSOT_IHQP_SENS_WIDE_MAIN", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-pthread", "-I."] + native_build.INCLUDES

# measured on the CPU over the fixture (python tests/ihqp_sens_wide_ref.py prints them; profiles/ihqp_sens_wide.txt has the printout)
REFERENCE_WORST = 6.31e-16              # the reference's y, in units of cond2(H~) max|y*| (case q, level 2)
REFERENCE_OBJECTIVE_WORST = 1.68e-15    # |getObjVal() - restated objective at the reference's x| / max(1, |objective|) (case s, level 1)
SENS_TOL = max(R.SENS_TOL, qp_sens_big_ref.SENS_BIG_TOL, 10.0 * REFERENCE_WORST)
OBJECTIVE_REF_TOL = 10.0 * REFERENCE_OBJECTIVE_WORST
assert SENS_TOL == R.SENS_TOL, "ihqp_sens_ref's comparisons carry its SENS_TOL: this fixture needs a wider one, pass it through"


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
    """build tests/emu/libosot_ihqp_sens_wide_host.so if it is stale, to a temporary name first"""
    return _ensure(LIBRARY, SHARED)


def ensure_sanitized():
    """the stand-alone program of the same file (-DOSOT_IHQP_SENS_WIDE_MAIN) under ASan + UBSan"""
    return _ensure(PROGRAM, SANITIZED)


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(ensure())
        pp, cp, pu = C.POINTER(abi.PlanDesc), C.POINTER(C.c_char_p), C.POINTER(C.c_ulonglong)
        L.ihqp_wide_host_level_lds_bytes.argtypes = [C.c_int]
        L.ihqp_wide_host_pullback_lds_bytes.argtypes = [C.c_int]
        L.ihqp_wide_host_workspace_bytes.argtypes = [pp, C.c_int, C.c_int, C.c_int, pu, pu]
        L.ihqp_wide_host_level_qp.argtypes = [pp, C.c_int, C.c_int, C.c_void_p, C.POINTER(abi.QpBatch), C.c_int, C.POINTER(abi.LevelQp),
                                              C.c_int, C.c_int, C.c_int, cp]
        L.ihqp_wide_host_sensitivity.argtypes = [pp, C.c_int, C.c_int, C.c_void_p, C.POINTER(abi.IhqpSensBatch), C.POINTER(abi.QpSensOptions),
                                                 C.c_int, C.c_int, C.c_int, cp]
        _lib = L
    return _lib


# ---- 2. the cases --------------------------------------------------------------------------------------------------------------------
def _generic(rows, weight=1.0):
    return Task(abi.TASK_GENERIC, rows, weight=weight)


def cases():
    """the smallest shapes at which the wide kernels can go wrong; p .. t, so that the seeds differ from ihqp_sens_ref's a .. e"""
    box = [Bound(abi.BOUND_GENERIC)]
    return {
        # the first wide size (n | 1 = n): two levels of 3 and 4 rows, one stored row block
        "p": Case("p", StackPlan(65, [[_generic(3)], [_generic(4)]], box, [Rows(abi.ROWS_GENERIC, 2)], eps_abs=EPS_ABS), 4),
        # n | 1 != n; the C3 shape: 3 / 24 / an implicit Postural block over every variable, box only
        "q": Case("q", StackPlan(66, [[_generic(3)], [_generic(24)], [Task(abi.TASK_POSTURAL, 66)]], box, [], eps_abs=EPS_ABS), 2),
        # 40 rows: more than one 32-row tile and no multiple of it; a stored block, a unit-row block that is local to level 1, one
        # inactive task and level 1 switched off
        "r": Case("r", StackPlan(72, [[_generic(4), _generic(3, 0.5)], [_generic(5)], [_generic(40), Task(abi.TASK_POSTURAL, 72)]], box,
                                 [Rows(abi.ROWS_GENERIC, 3), Rows(abi.ROWS_UNIT_GENERIC, 4, first_col=5, level=1)], eps_abs=EPS_ABS), 2,
                  level_active=[True, False, True], task_active={(0, 1): False}, b_scale=0.6),
        # the maximum: the full ownership map, the largest LDS blocks
        "s": Case("s", StackPlan(128, [[_generic(12)], [_generic(6), Task(abi.TASK_POSTURAL, 128)]], box, [Rows(abi.ROWS_GENERIC, 24)],
                                 eps_abs=EPS_ABS), 2, b_scale=0.6),
        # OSOT_MAX_LEVELS levels of one row: the chain's depth for the pull-back
        "t": Case("t", StackPlan(65, [[_generic(1)] for _ in range(abi.MAX_LEVELS)], box, [], eps_abs=EPS_ABS), 2, box=8.0),
    }


def extra_cases():
    """the n = 65 twins of ihqp_sens_ref.extra_cases(): not in the fixture (the level QP alone is compared, at a seeded x)"""
    return {
        # a level with a non-diagonal weight, an identity-Jacobian regularisation task, c, a global unit-row block, no box
        "dense": Case("dense", StackPlan(65, [[Task(abi.TASK_GENERIC, 4, dense_weight=True)], [_generic(3), Task(abi.TASK_POSTURAL, 65)]], [],
                                         [Rows(abi.ROWS_UNIT_GENERIC, 2, first_col=1)], eps_abs=EPS_ABS,
                                         regularisation=Task(abi.TASK_GENERIC, 5, weight=0.3)), 3, with_c=True),
        # a regularisation task with a stored Jacobian; more stored rows than one tile holds
        "reg": Case("reg", StackPlan(65, [[_generic(40)], [_generic(2)]], [Bound(abi.BOUND_GENERIC)], [], eps_abs=EPS_ABS,
                                     regularisation=Task(abi.TASK_GENERIC, 3, weight=0.7), regularisation_dense=True), 2),
    }


def fixture():
    """{name: dict(inp, x_levels [B][L][n], y [k] -> [B][n + rows_k], objective [B][L], grad_dq [B][n])} of
    tests/golden/ihqp_sens_wide.npz"""
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


# ---- 3. the runs through the host build ------------------------------------------------------------------------------------------------
def host_workspace_bytes(case, B, backward=False, grad_A=False):
    """osot_ihqp_sens_workspace_bytes of a wide handle -> (bytes, the part in front of the Y slices)"""
    v, f = C.c_ulonglong(0), C.c_ulonglong(0)
    pd = case.plan.to_c()
    assert lib().ihqp_wide_host_workspace_bytes(C.byref(pd), B, int(backward), int(grad_A), C.byref(v), C.byref(f)) == abi.OK
    return v.value, f.value


def host_level_qp(case, inp, k, x_levels, nthreads=1, t0_last=0):
    """osot_ihqp_level_qp of a wide handle through the host build -> dict of Fenced (H, g, A, lA, uA, l, u)"""
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
    rc = lib().ihqp_wide_host_level_qp(C.byref(pd), 1, B, None if ta is None else ta.ctypes.data, C.byref(qb), k, C.byref(lq), 1, nthreads,
                                       t0_last, C.byref(why))
    assert rc == abi.OK, why.value
    return out


def host_check(case, sens, opts=None, wide=1, max_batch=None):
    """osot_ihqp_sensitivity's answer to its arguments, from the host build -> (code, reason)"""
    why = C.c_char_p()
    pd = case.plan.to_c()
    ta = case.task_flags()
    rc = lib().ihqp_wide_host_sensitivity(C.byref(pd), wide, sens.qp.B if max_batch is None else max_batch,
                                          None if ta is None else ta.ctypes.data, C.byref(sens), None if opts is None else C.byref(opts), 0, 1, 0,
                                          C.byref(why))
    return rc, (why.value or b"").decode()


def _run(case, s, B, nthreads, t0_last):
    why = C.c_char_p()
    pd = case.plan.to_c()
    ta = case.task_flags()
    rc = lib().ihqp_wide_host_sensitivity(C.byref(pd), 1, B, None if ta is None else ta.ctypes.data, C.byref(s), None, 1, nthreads, t0_last,
                                          C.byref(why))
    assert rc == abi.OK, why.value


def host_sensitivity(case, inp, x_levels, status=None, want=("y", "active", "flag", "objective"), nthreads=1, t0_last=0):
    """osot_ihqp_sensitivity of a wide handle through the host build -> SensOutputs (the workspace fenced, 16-byte aligned)"""
    B = x_levels.shape[0]
    arr = host_arrays(case, inp, x_levels, status)
    qb = qp_batch(case, arr, lambda a: a.ctypes.data, B)
    out = SensOutputs(case, B, want, host_workspace_bytes(case, B)[0])
    assert out.workspace.address % 16 == 0
    _run(case, out.struct(qb), B, nthreads, t0_last)
    return out


def host_backward(case, inp, x_levels, grad_dq, status=None, want=GRAD_LEVEL + GRAD_GLOBAL, nthreads=1, t0_last=0):
    """osot_ihqp_sensitivity with grad_dq through the host build -> (SensOutputs, GradOutputs)"""
    B = x_levels.shape[0]
    arr = host_arrays(case, inp, x_levels, status)
    qb = qp_batch(case, arr, lambda a: a.ctypes.data, B)
    grads = GradOutputs(case, B, want)
    out = SensOutputs(case, B, workspace_bytes=host_workspace_bytes(case, B, True, grads.wants_A())[0])
    assert out.workspace.address % 16 == 0
    s = out.struct(qb)
    gdq = np.ascontiguousarray(grad_dq, dtype=np.float64)
    s.grad_dq = gdq.ctypes.data
    grads.bind(s)
    _run(case, s, B, nthreads, t0_last)
    return out, grads


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
            pk = {key: (v[ok] if isinstance(v, np.ndarray) else v) for key, v in prob.items()}
            pk["B"] = len(ok)
            a = qp_sens_ref.worst_deviation(pk, dict(y=fx["y"][k][ok]), [arb[i] for i in ok], names=("y",)) if ok else (0.0, "", -1)
            o = max(abs(fx["objective"][i, k] - objective_of(restate_level_qp(case, fx["inp"], i, k, fx["x_levels"][i], np.longdouble),
                                                             fx["x_levels"][i, k])) / max(1.0, abs(fx["objective"][i, k])) for i in range(case.B))
            print(f"case {name} level {k}: n = {case.plan.n:3d} rows = {case.rows(k):3d} unique sets {len(ok)}/{case.B} "
                  f"cond2 <= {max(qp_sens_ref.cond_H(prob)):9.3e}  reference y {a[0]:.3e}  reference objective {o:.3e}")
            ref_w, obj_w = max(ref_w, a[0]), max(obj_w, o)
        out = host_sensitivity(case, fx["inp"], fx["x_levels"])
        emu_w = max(emu_w, R.SENS_TOL * assert_multipliers(case, fx["inp"], fx["x_levels"], None, [f.value for f in out.y],
                                                           [f.value for f in out.active], [f.value for f in out.flag], out.objective.value,
                                                           require_ok=False))
    print(f"REFERENCE_WORST = {ref_w:.2e}\nREFERENCE_OBJECTIVE_WORST = {obj_w:.2e}\nHOST_BUILD_WORST = {emu_w:.2e} (for the record)\n"
          f"ihqp_sens_ref.SENS_TOL = {R.SENS_TOL:.2e}  qp_sens_big_ref.SENS_BIG_TOL = {qp_sens_big_ref.SENS_BIG_TOL:.2e}  "
          f"SENS_TOL = {max(R.SENS_TOL, qp_sens_big_ref.SENS_BIG_TOL, 10.0 * ref_w):.2e}")
