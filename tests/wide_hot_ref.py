"""tests/wide_hot_ref.py -- TEST INFRASTRUCTURE ONLY: the host build of the wide cascade's HOT instantiation
(tests/emu/cascade_wide_hot_host.cpp) and what the hot-start tests of the wide route share: the call, the drift of a stack between
control cycles, the fixtures.

The two artifacts are built here with native_build's flags, staleness rule and write-then-rename rule (its table of names is pinned
by tests/test_native_build_host.py): the library the tests load with the flags of "wide_host", and the same file as a stand-alone
program with the flags of "big_hot_asan" (AddressSanitizer + UndefinedBehaviorSanitizer, runtimes linked statically), which is run
as a child process: nothing sanitised is loaded into the interpreter."""
import ctypes as C
import os
import shlex
import subprocess

import numpy as np

from opensot_amd import abi, synth
from opensot_amd.solver import stored_rows
import native_build

EMU = os.path.join(native_build.ROOT, "tests", "emu")
SOURCE = "cascade_wide_hot_host.cpp"
LIBRARY = "libosot_wide_hot_host.so"
PROGRAM = "wide_hot_asan"
HOT_LEN = 128


def _flags(name, drop=()):
    return [w for w in native_build.ARTIFACTS[name].command if w not in drop]


COMMANDS = {LIBRARY: native_build.TEAM_OF_ONE + ["-pthread"] + native_build.INCLUDES,
            PROGRAM: _flags("big_hot_asan", drop=("-DOSOT_BIG_HOT_MAIN",)) + ["-DOSOT_WIDE_HOT_MAIN"]}


def ensure(output):
    """build tests/emu/<output> if it is stale (native_build.is_stale), to a temporary name first"""
    out = os.path.join(EMU, output)
    if native_build.is_stale(out, out + ".d", EMU, recipe=os.path.abspath(__file__)) or \
            os.path.getmtime(native_build.RECIPE) > os.path.getmtime(out):
        tmp = f"{output}.tmp.{os.getpid()}"
        cmd = COMMANDS[output] + [SOURCE, "-MMD", "-MF", output + ".d", "-o", tmp]
        print(shlex.join(cmd), flush=True)
        try:
            subprocess.check_call(cmd, cwd=EMU)
            os.replace(os.path.join(EMU, tmp), out)
        finally:
            if os.path.exists(os.path.join(EMU, tmp)):
                os.remove(os.path.join(EMU, tmp))
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(ensure(LIBRARY))
        _lib.wide_host_ihqp_hot.argtypes = [C.POINTER(abi.PlanDesc), C.POINTER(abi.QpBatch), C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return _lib


def run_sanitizer_program():
    """the stand-alone program under ASan + UBSan as a child process -> CompletedProcess"""
    return subprocess.run([ensure(PROGRAM)], capture_output=True, text=True, timeout=600)


def new_state(B, L):
    return np.full((B, L * HOT_LEN), -1, dtype=np.int32)


def wide_host_hot(plan, asm, hot, active=None, task_active=None, nthreads=1, t0_last=False):
    """the wide cascade on host arrays (asm: oracle layout), every level starting from its list of `hot` (int32 (B, L * 128),
    rewritten in place; None: the cold instantiation) -> dq, x_levels, status, iterations, accepted_slack"""
    B, n, L = asm["B"], asm["n"], asm["L"]
    qb = abi.QpBatch()
    qb.B = B
    keep = []

    def put(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data
    for k in range(L):
        for name in ("A", "b", "w", "c", "WA", "Wb"):
            if name in asm and asm[name][k] is not None:
                getattr(qb, name)[k] = put(asm[name][k])
    if asm["C"] is not None:
        Cs = stored_rows(plan, asm["C"])
        if Cs.shape[1]:
            qb.C = put(Cs)
    for name in ("lo", "up", "l", "u"):
        if asm[name] is not None:
            setattr(qb, name, put(asm[name]))
    if asm.get("reg") is not None:
        qb.b_reg = put(asm["reg"]["b"])
        if asm["reg"].get("A") is not None:
            qb.A_reg = put(asm["reg"]["A"])
    dq = np.zeros((B, n)); xl = np.zeros((B, L, n)); slack = np.zeros(B)
    st = np.full(B, -1, dtype=np.int32); it = np.zeros(B, dtype=np.int32)
    qb.dq, qb.x_levels, qb.status, qb.iterations = dq.ctypes.data, xl.ctypes.data, st.ctypes.data, it.ctypes.data
    qb.accepted_slack = slack.ctypes.data
    if active is not None:
        act = (C.c_ubyte * L)(*[1 if a else 0 for a in active])
        keep.append(act)
        qb.level_active = C.addressof(act)
    ta = None
    if task_active:
        ta = (C.c_ubyte * (abi.MAX_LEVELS * abi.MAX_TASKS))(*([1] * (abi.MAX_LEVELS * abi.MAX_TASKS)))
        for (k, j), on in task_active.items():
            ta[k * abi.MAX_TASKS + j] = 1 if on else 0
    if hot is not None:
        assert hot.dtype == np.int32 and hot.flags.c_contiguous and hot.shape == (B, L * HOT_LEN)
    pd = plan.to_c()
    rc = lib().wide_host_ihqp_hot(C.byref(pd), C.byref(qb), C.cast(ta, C.c_void_p) if ta is not None else None,
                                  nthreads, 1 if t0_last else 0, hot.ctypes.data if hot is not None else None)
    assert rc == 0
    return dq, xl, st, it, slack


def drifted(asm, cycle, rel=0.01):
    """the assembled stack of control cycle `cycle` (0: asm itself): every task's b, the constraint rows' bounds and the box scaled by
    one factor per instance and array within 1 +- rel, drawn anew per cycle.  Both sides of a row are scaled by the SAME factor, so
    a row with lo == up stays an equality and an infinite side stays infinite; a scaled feasible set that held 0 still holds it"""
    if cycle == 0:
        return asm
    rng = np.random.default_rng(1000 + cycle)
    B = asm["B"]
    out = dict(asm)
    out["b"] = [None if b is None else b * (1.0 + rel * rng.uniform(-1, 1, size=(B, 1))) for b in asm["b"]]
    if asm["lo"] is not None:
        f = 1.0 + rel * rng.uniform(-1, 1, size=(B, 1))
        out["lo"], out["up"] = _scaled(asm["lo"], f), _scaled(asm["up"], f)
    if asm["l"] is not None:
        f = 1.0 + rel * rng.uniform(-1, 1, size=(B, 1))
        out["l"], out["u"] = _scaled(asm["l"], f), _scaled(asm["u"], f)
    return out


def _scaled(a, f):
    return np.where(np.abs(a) >= 1e20, a, a * f)


def scaled_diff(a, b):
    """the worst |a - b| over the batch, relative to max(1, |b|)"""
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def tight_stack(B):
    """a tight box under many inequality rows: the hot phase both adds and removes (test_wide_cascade_team_of_four_equals_team_of_one)"""
    return synth.make_generic_stack(B, 72, [30, 40], n_ineq=120, box=0.05, seed=0)
