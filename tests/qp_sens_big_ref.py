"""tests/qp_sens_big_ref.py -- TEST INFRASTRUCTURE ONLY: what the tests of osot_qp_sensitivity_batch_ws (65 .. 128 variables) share.

  * the recipe of the host build tests/emu/qp_sens_big_host.cpp (sensbig::run of opensot_amd/csrc/osot_qp_sens_big.h as a team of
    one thread or a turn-taking team of several, with the checks of osot_qp_sensitivity_batch_ws), built with native_build's flags,
    staleness rule and write-then-rename rule; and of the same file as a stand-alone program under AddressSanitizer and
    UndefinedBehaviorSanitizer (statically linked runtimes, its own main: nothing is loaded into Python under a sanitizer);
  * the fixture tests/golden/qp_sens_big.npz (tests/golden/make_qp_sens_big_golden.py) and the run of a case through the host build.

The restatement, the longdouble arbiter, Outputs, structs, constructed() and worst_deviation are qp_sens_ref's: they do not depend
on the shape.

THE TOLERANCE.  `python tests/qp_sens_big_ref.py` measures, over the new fixture only and in the units of
qp_sens_ref.worst_deviation, REFERENCE_WORST (the reference's own y against the arbiter), RESTATEMENT_WORST (y and the seven
gradients of the float64 restatement against the arbiter) and, for the record, EMULATED_WORST (the emulated kernel).  The tests'
tolerance is SENS_BIG_TOL = max(qp_sens_ref.SENS_TOL, 10 x the larger of the first two): ten is the margin this project gives a
different summation order.  It is measured on the reference and the restatement, never on the kernel under test."""
import ctypes as C
import os
import shlex
import subprocess
import sys

import numpy as np

if __name__ == "__main__":     # `python tests/qp_sens_big_ref.py`: the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from opensot_amd import abi
import native_build
import qp_sens_ref as R

EMU = R.EMU
GOLDEN = os.path.join(native_build.ROOT, "tests", "golden", "qp_sens_big.npz")
SOURCE = "qp_sens_big_host.cpp"
LIBRARY = "libosot_qp_sens_big_host.so"
PROGRAM = "qp_sens_big_asan"
SHARED = native_build.LOCKSTEP + ["-pthread"]
SANITIZED = ["g++", "-O1", "-g", "-std=c++17", "-DOSOT_EMULATION", "-DOSOT_QP_SENS_BIG_MAIN", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-pthread", "-I."] + native_build.INCLUDES
# the fixture's shapes (n, nc, n_eq, B); the last is box only
SHAPES = ((65, 40, 3, 2), (128, 24, 2, 1), (100, 0, 0, 1))

# measured on the CPU over the fixture (python tests/qp_sens_big_ref.py prints them), in units of cond2(H + eps I) max|X*|
REFERENCE_WORST = 1.73e-17
RESTATEMENT_WORST = 1.09e-18
EMULATED_WORST = 2.28e-18
SENS_BIG_TOL = max(R.SENS_TOL, 10.0 * max(REFERENCE_WORST, RESTATEMENT_WORST))


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
    """build tests/emu/libosot_qp_sens_big_host.so if it is stale (native_build.is_stale), to a temporary name first"""
    return _ensure(LIBRARY, SHARED)


def ensure_sanitized():
    """the stand-alone program of the same file (-DOSOT_QP_SENS_BIG_MAIN) under ASan + UBSan"""
    return _ensure(PROGRAM, SANITIZED)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(ensure())
        pb, po = C.POINTER(abi.QpSensBatch), C.POINTER(abi.QpSensOptions)
        _lib.sens_big_host_check.argtypes = [pb, po, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
        _lib.sens_big_host_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
        _lib.sens_big_host_run.argtypes = [pb, po, C.c_int, C.c_int, C.c_int]
        _lib.sens_big_host_lds_bytes.argtypes = [C.c_int, C.c_int]
        _lib.sens_big_host_lds_bytes.restype = C.c_size_t
        _lib.sens_big_host_slice_bytes.argtypes = [C.c_int]
        _lib.sens_big_host_slice_bytes.restype = C.c_size_t
        _lib.sens_big_host_slots.argtypes = [C.c_int, C.c_int]
    return _lib


def host_check(batch, options=None, workspace=None, workspace_bytes=0):
    """osot_qp_sensitivity_batch_ws's answer to its arguments, from the host build -> (code, reason)"""
    why = C.c_char_p()
    rc = lib().sens_big_host_check(C.byref(batch), None if options is None else C.byref(options), workspace, workspace_bytes, C.byref(why))
    return rc, (why.value or b"").decode()


def workspace_bytes(B, n, nc):
    """osot_qp_sens_workspace_bytes from the host build -> (code, bytes, reason)"""
    why, out = C.c_char_p(), C.c_size_t(0)
    rc = lib().sens_big_host_workspace_bytes(B, n, nc, C.byref(out), C.byref(why))
    return rc, out.value, (why.value or b"").decode()


# ---- 2. the fixture and the run --------------------------------------------------------------------------------------------------------
def fixture():
    """[(problem, x_ref, y_ref, grad_x)] of tests/golden/qp_sens_big.npz, one per shape of SHAPES"""
    out = []
    with np.load(GOLDEN) as z:
        for s, (n, nc, n_eq, B) in enumerate(SHAPES):
            get = lambda k: z[f"s{s}_{k}"] if f"s{s}_{k}" in z.files else None
            p = R.problem(get("H"), get("g"), get("A"), get("lA"), get("uA"), get("l"), get("u"), float(z["eps_abs"]))
            assert (p["B"], p["n"], p["nc"]) == (B, n, nc)
            out.append((p, get("x"), get("y"), get("grad_x")))
    return out


def run_host(p, x, gx=None, status=None, want=None, opts=None, groups=2, nthreads=1, t0_last=0):
    """the case through the host build -> Outputs.  groups workgroups walk the batch; nthreads = 1: the team of one, above: the
    turn-taking team with thread 0 first (t0_last = 0) or last (1)"""
    if want is None:
        want = R.Outputs.ALL if gx is not None else ("y", "active", "flag")
    out, keep = R.Outputs(p, want), []
    b = R.structs(p, x, out, lambda a: a.ctypes.data, keep, gx, status)
    assert lib().sens_big_host_run(C.byref(b), None if opts is None else C.byref(opts), groups, nthreads, t0_last) == abi.OK
    return out


if __name__ == "__main__":
    ref_w = res_w = emu_w = 0.0
    for p, x, y_ref, gx in fixture():
        arb = R.arbiter(p, x, gx)
        assert all(a["flag"] == R.OK for a in arb)
        a = R.worst_deviation(p, dict(y=y_ref), arb, names=("y",))
        b = R.worst_deviation(p, R.restate(p, x, gx), arb)
        c = R.worst_deviation(p, run_host(p, x, gx), arb)
        print(f"n = {p['n']:3d} nc = {p['nc']:2d} B = {p['B']}  cond2 <= {max(R.cond_H(p)):9.3e}  reference {a}  restatement {b}  emulated {c}")
        ref_w, res_w, emu_w = max(ref_w, a[0]), max(res_w, b[0]), max(emu_w, c[0])
    print(f"REFERENCE_WORST = {ref_w:.2e}\nRESTATEMENT_WORST = {res_w:.2e}\nEMULATED_WORST = {emu_w:.2e}")
    print(f"qp_sens_ref.SENS_TOL = {R.SENS_TOL:.2e}, 10 x the larger of the first two = {10.0 * max(ref_w, res_w):.2e}")
