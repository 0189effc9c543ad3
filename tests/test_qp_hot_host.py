"""Hot start of the wide explicit QP (65 .. 128 variables, opensot_amd/csrc/osot_qp_big.h, big::solve<true>) on the host: the SAME
source the product runs as a 256-thread workgroup, compiled by tests/native_build.py (big_hot_host) with a team of one thread and with the
turn-taking team of tests/emu/cascade_wide_host.cpp.  No GPU.

Problems: random_qp(default_rng(31), 6, n, nc, n_eq, box=True) with g *= 4, eps 1e-9, at (n, nc, n_eq) = (65, 10, 0), (72, 24, 4),
(128, 40, 0): the cold solver takes 45 .. 150 iterations on them for 27 .. 64 active constraints.
Bound for "the same answer": |x_hot - x_cold| <= 1e-10 max(1, |x|), the bound tests/test_gpu_backend.py uses for the same property."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import native_build
from helpers import ROOT, big_host_solve, kkt_check, random_qp

EPS = 1e-9
HOT_LEN = 128
SHAPES = [(65, 10, 0), (72, 24, 4), (128, 40, 0)]

_lib = None


def _build(what):
    """the library the tests load ("lib") or the stand-alone sanitizer program ("asan"), rebuilt when stale"""
    return native_build.ensure("big_hot_host" if what == "lib" else "big_hot_asan")


def hot_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(_build("lib"))
    return _lib


def empty_list():
    return np.full(HOT_LEN, -1, dtype=np.int32)


def big_hot_host_solve(H, g, A, lA, uA, l, u, eps_abs, hot, max_iter=0, nthreads=1, t0_last=False):
    """one QP through big::solve<true> with the caller's list.  Returns (status, x, iterations, recorded list)."""
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int)
    n = H.shape[0]
    nc = 0 if A is None else A.shape[0]
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (H, g, A, lA, uA, l, u)]
    ptr = [None if a is None else a.ctypes.data_as(dp) for a in keep]
    hin = np.ascontiguousarray(hot, dtype=np.int32).copy()
    assert hin.shape == (HOT_LEN,)
    hout = np.full(HOT_LEN, 12345, dtype=np.int32)
    x = np.zeros(n)
    st, it = C.c_int(-1), C.c_int(0)
    rc = hot_lib().osot_big_hot_host_solve(n, nc, *ptr, C.c_double(eps_abs), int(max_iter), x.ctypes.data_as(dp), C.byref(st), C.byref(it),
                                           hin.ctypes.data_as(ip), hout.ctypes.data_as(ip), int(nthreads), int(bool(t0_last)))
    assert rc == 0, "osot_big_hot_host_solve refused the arguments"
    return st.value, x, it.value, hout


def problems(n, nc, n_eq, seed=31):
    H, g, A, lA, uA, l, u = random_qp(np.random.default_rng(seed), 6, n, nc, n_eq, box=True)
    g = g * 4.0
    return [(H[b], g[b], A[b], lA[b], uA[b], l[b], u[b]) for b in range(6)]


def close(x, ref):
    return np.abs(x - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


def as_set(lst):
    return set(int(v) for v in lst if v >= 0)


_cold = {}


def cold(shape, seed=31):
    """the parent's cold solver on the six problems of a shape, and the empty-list solve of the hot instantiation; computed once"""
    key = (shape, seed)
    if key not in _cold:
        out = []
        for q in problems(*shape, seed=seed):
            st, x, it = big_host_solve(*q, EPS)
            assert st == 0
            out.append((q, x, it, big_hot_host_solve(*q, EPS, empty_list())))
        _cold[key] = out
    return _cold[key]


def test_hot_constants_are_the_wavefront_routes():
    """kHotBatch, kHotAbandon, kHotDropTol as big::solve sees them = the values written in osot_qp_core.h (gi_inequalities)"""
    text = open(os.path.join(ROOT, "opensot_amd", "csrc", "osot_qp_core.h")).read()
    m = re.search(r"constexpr int kHotBatch = (\d+), kHotAbandon = (\d+);", text)
    d = re.search(r"constexpr double kHotDropTol = ([0-9.eE+-]+);", text)
    assert m and d
    out = (C.c_double * 4)()
    hot_lib().osot_big_hot_constants(out)
    assert (out[0], out[1], out[2]) == (float(m.group(1)), float(m.group(2)), float(d.group(1)))
    assert out[3] == HOT_LEN


@pytest.mark.parametrize("shape", SHAPES)
def test_empty_list_is_the_cold_solve(shape):
    n = shape[0]
    for q, xc, itc, (st, x, it, rec) in cold(shape):
        assert st == 0 and it == itc
        assert np.array_equal(x, xc), "an empty list must give the cold solve bit for bit"
        cnt = int((rec >= 0).sum())
        assert cnt <= n
        assert (rec[:cnt] >= 0).all() and (rec[cnt:] == -1).all(), "the recorded list is compacted to the front, -1 behind"
        assert len(as_set(rec)) == cnt


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_repeat(shape):
    for q, xc, itc, (_, _, _, rec) in cold(shape):
        st, x, it, rec2 = big_hot_host_solve(*q, EPS, rec)
        print(f"{shape}: cold {itc} iterations, hot {it}, {len(as_set(rec))} active")
        assert st == 0
        assert close(x, xc)
        assert kkt_check(*q, x, EPS) < 1e-7
        assert it < itc
        assert as_set(rec2) == as_set(rec)


@pytest.mark.parametrize("shape", SHAPES)
def test_drift(shape):
    rng = np.random.default_rng(5)
    tot_hot = tot_cold = 0
    for q, xc, itc, (_, _, _, rec) in cold(shape):
        H, g, A, lA, uA, l, u = q
        lst = rec
        for cycle in range(3):
            g = g * (1.0 + 0.01 * rng.normal(size=g.shape))
            q2 = (H, g, A, lA, uA, l, u)
            stc, x2c, it2c = big_host_solve(*q2, EPS)
            st, x, it, lst = big_hot_host_solve(*q2, EPS, lst)
            assert stc == 0 and st == 0
            assert close(x, x2c), f"cycle {cycle}"
            if cycle == 0:
                tot_hot += it; tot_cold += it2c
    print(f"{shape}: drifted g, summed iterations over six instances: hot {tot_hot}, cold {tot_cold}")
    assert tot_hot < tot_cold


def corrupt_lists(shape):
    """lists that are not this problem's: every one must leave the cold answer"""
    n, nc, n_eq = shape
    other = cold(shape, seed=32)[0][3][3]                      # another seed's list
    lows = np.full(HOT_LEN, -1, dtype=np.int32); lows[:n] = 2 * np.arange(n)          # every lower bound
    rng = np.random.default_rng(9)
    wild = empty_list(); wild[0] = 10**6; wild[1] = -7; wild[2:40] = rng.integers(-50, 4 * (n + nc), size=38); wild[40] = 2**31 - 1; wild[41] = -2**31
    dup = empty_list(); dup[:] = np.tile(np.array([2 * 3, 2 * 3, 2 * 3 + 1, 2 * (n + nc - 2), 2 * (n + nc - 2) + 1, 2 * 5 + 1, 2 * 5 + 1, 2 * 3], dtype=np.int32), HOT_LEN // 8)
    eq = empty_list(); eq[0] = 2 * n; eq[1] = 2 * n + 1; eq[2] = 2 * (n + 1)           # rows 0, 1: equality rows where n_eq > 0
    inf = empty_list(); inf[0] = 2 * (n + nc - 1); inf[1] = 2 * (n + nc - 1) + 1       # the last row has no lower bound (random_qp)
    return {"other seed": other, "all lower bounds": lows, "out of range": wild, "duplicates": dup, "equality row": eq, "infinite side": inf}


@pytest.mark.parametrize("shape", SHAPES)
def test_foreign_and_corrupt_lists(shape):
    for q, xc, itc, _ in cold(shape)[:3]:
        for name, lst in corrupt_lists(shape).items():
            st, x, it, rec = big_hot_host_solve(*q, EPS, lst)
            assert st == 0, name
            assert close(x, xc), name
            assert kkt_check(*q, x, EPS) < 1e-7


@pytest.mark.parametrize("shape", SHAPES)
def test_corrupt_lists_under_sanitizers(shape, tmp_path):
    """the same case as a stand-alone program built with -fsanitize=address,undefined, the runtimes linked statically (its own main;
    nothing is loaded into Python, and the child runs in this process's environment as it is)"""
    exe = _build("asan")
    n, nc, _ = shape
    q, xc, itc, _ = cold(shape)[0]
    lists = list(corrupt_lists(shape).values()) + [cold(shape)[0][3][3], empty_list()]
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        np.array([n, nc, 1, len(lists), 0], dtype=np.int32).tofile(f)
        np.array([EPS]).tofile(f)
        for a in q:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        for lst in lists:
            np.ascontiguousarray(lst, dtype=np.int32).tofile(f)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(lists)
    for line in lines:
        tok = line.split()
        assert int(tok[0]) == 0
        x = np.array([float(t) for t in tok[2:2 + n]])
        assert close(x, xc)
        assert len(tok) == 2 + n + HOT_LEN
    tok = lines[-1].split()                                   # the empty list: the cold solve
    assert int(tok[1]) == itc and np.array_equal(np.array([float(t) for t in tok[2:2 + n]]), xc)


def test_failures_record_nothing():
    n, nc, n_eq = 72, 24, 4
    q, xc, itc, (_, _, _, rec) = cold((n, nc, n_eq))[0]
    H, g, A, lA, uA, l, u = q
    A2, lA2, uA2 = A.copy(), lA.copy(), uA.copy()
    A2[1] = A2[0]; lA2[1] = uA2[1] = lA2[0] + 1.0             # two contradictory equality rows
    for lst in (empty_list(), rec):
        st, _, _, out = big_hot_host_solve(H, g, A2, lA2, uA2, l, u, EPS, lst)
        assert st == 1 and (out == -1).all()
        st, _, it, out2 = big_hot_host_solve(*q, EPS, lst, max_iter=2)
        assert st == 2 and (out2 == -1).all()
        for left in (out, out2):                               # a good problem with what a failure left: the cold solve
            st, x, it, _ = big_hot_host_solve(*q, EPS, left)
            assert st == 0 and it == itc and np.array_equal(x, xc)


@pytest.mark.parametrize("t0_last", [False, True])
@pytest.mark.parametrize("shape", [(65, 10, 0), (72, 24, 4)])
def test_teams(shape, t0_last):
    """five threads taking turns, thread 0 first or last: x, iterations and the recorded list are those of the team of one"""
    for q, xc, itc, (_, x1, it1, rec1) in cold(shape)[:2]:
        st, x, it, rec = big_hot_host_solve(*q, EPS, empty_list(), nthreads=5, t0_last=t0_last)
        assert st == 0 and it == it1 and np.array_equal(x, x1) and np.array_equal(rec, rec1)
        _, xr1, itr1, recr1 = big_hot_host_solve(*q, EPS, rec1)
        st, x, it, rec = big_hot_host_solve(*q, EPS, rec1, nthreads=5, t0_last=t0_last)
        assert st == 0 and it == itr1 and np.array_equal(x, xr1) and np.array_equal(rec, recr1)
