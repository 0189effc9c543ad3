"""sensbig::run (opensot_amd/csrc/osot_qp_sens_big.h: multipliers, active set and backward pass of the explicit QP for 65 .. 128
variables) through its host build tests/emu/qp_sens_big_host.cpp: the fixture tests/golden/qp_sens_big.npz against the longdouble
arbiter of tests/qp_sens_ref.py and the reference's own multipliers, the turn-taking team of several threads against the team of
one, the edges at the smallest sizes where the wide route can differ from the wavefront route, every refusal of
osot_qp_sensitivity_batch_ws, the workspace's size, and the same file as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer.  No GPU needed."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from opensot_amd import abi
import qp_sens_ref as R
import qp_sens_big_ref as BG

TOL = BG.SENS_BIG_TOL


@functools.lru_cache(maxsize=None)
def fixture():
    return BG.fixture()


@functools.lru_cache(maxsize=None)
def fixture_arbiter(s):
    p, x, _, gx = fixture()[s]
    return R.arbiter(p, x, gx)


@functools.lru_cache(maxsize=None)
def fixture_team_of_one(s):
    p, x, _, gx = fixture()[s]
    return BG.run_host(p, x, gx)


def assert_matches_arbiter(p, out, arb, names=("y",) + R.GRADS):
    for name in names:
        dev = R.worst_deviation(p, out, arb, names=(name,))
        print(f"  {name:8s} worst deviation {dev[0]:.3e} (instance {dev[2]}), SENS_BIG_TOL {TOL:.3e}")
        assert dev[0] <= TOL, dev
    assert [int(f) for f in out.flag] == [a["flag"] for a in arb]
    assert np.array_equal(out.active, np.stack([a["active"] for a in arb]))


def test_tolerance_is_the_recorded_one():
    assert TOL == max(R.SENS_TOL, 10.0 * max(BG.REFERENCE_WORST, BG.RESTATEMENT_WORST))


@pytest.mark.parametrize("s", range(len(BG.SHAPES)))
def test_fixture_multipliers_and_gradients(s):
    """x = the reference's x: y within SENS_BIG_TOL of the arbiter, the set the reference's, every flag OK, the seven gradients
    within SENS_BIG_TOL of the arbiter's dense KKT solve, grad_H symmetric to the bit, sentinels intact"""
    p, x, y_ref, gx = fixture()[s]
    arb = fixture_arbiter(s)
    out = fixture_team_of_one(s)
    assert out.fences_intact()
    assert np.all(out.flag == R.OK)
    assert np.array_equal(out.active, R.reference_active(p, y_ref))
    assert_matches_arbiter(p, out, arb)
    assert np.array_equal(out.grad_H, np.transpose(out.grad_H, (0, 2, 1)))
    print("  reference's y:", R.worst_deviation(p, dict(y=y_ref), arb, names=("y",)))


def test_multipliers_only_leaves_gradients_alone():
    p, x, _, gx = fixture()[0]
    full = fixture_team_of_one(0)
    only = BG.run_host(p, x)
    assert only.fences_intact()
    assert np.array_equal(only.y, full.y) and np.array_equal(only.active, full.active) and np.array_equal(only.flag, full.flag)


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("t0_last", [0, 1])
def test_turn_taking_team_gives_the_bits_of_the_team_of_one(s, t0_last):
    """7 threads, one at a time in a fixed order, thread 0 first or last in every section: a value read in the section that
    writes it (a missing barrier) comes out differently under one of the two orders"""
    p, x, _, gx = fixture()[s]
    one = fixture_team_of_one(s)
    seven = BG.run_host(p, x, gx, nthreads=7, t0_last=t0_last)
    assert seven.fences_intact()
    for k in R.Outputs.ALL:
        assert np.array_equal(getattr(seven, k), getattr(one, k)), k


def test_one_workgroup_walks_the_batch():
    """the stride walk: one workgroup over both instances (the LDS and the slice reused) gives the bits of two workgroups"""
    p, x, _, gx = fixture()[0]
    walked = BG.run_host(p, x, gx, groups=1)
    for k in R.Outputs.ALL:
        assert np.array_equal(getattr(walked, k), getattr(fixture_team_of_one(0), k)), k


# ---- the edges, each at B = 2 (the failed instance: B = 3, it lies between two good ones) ---------------------------------------------
def run_edge(p, x, seed=5, status=None, want=None, with_arbiter=True):
    gx = np.random.default_rng([p["n"], seed]).normal(size=(p["B"], p["n"]))
    out = BG.run_host(p, x, gx, status=status, want=want)
    assert out.fences_intact()
    for k in out.want:
        assert np.all(np.isfinite(getattr(out, k).astype(float)))
    return out, gx, (R.arbiter(p, x, gx, status=status) if with_arbiter else None)


def assert_y_constructed(p, out, y):
    """the multipliers the instance was constructed with come back (to the conditioning of H~)"""
    cond = R.cond_H(p)
    for i in range(p["B"]):
        assert np.max(np.abs(out.y[i] - y[i])) <= 1e3 * 2.0 ** -53 * cond[i] * max(1.0, np.abs(y[i]).max()) * p["n"]


def test_edge_no_candidate():
    p, x, _ = R.constructed(2, 65, 5)
    out, gx, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb)
    assert np.all(out.flag == R.OK) and np.all(out.y == 0.0) and np.all(out.active == 0)
    cond = R.cond_H(p)
    for i in range(2):
        dx = -np.linalg.solve(p["H"][i] + p["eps_abs"] * np.eye(65), gx[i])
        assert np.max(np.abs(out.grad_g[i] - dx)) <= TOL * cond[i] * np.abs(dx).max()


def test_edge_all_bounds_active():
    def shape(i, bs, rs):
        bs[:] = [1 if (k + i) % 2 else -1 for k in range(len(bs))]
    p, x, y = R.constructed(2, 65, 4, shape=shape)
    out, _, arb = run_edge(p, x)
    # (dx is exactly zero: the arbiter's elimination leaves rounding noise there, which is no scale to compare against)
    assert_matches_arbiter(p, out, arb, names=("y", "grad_A", "grad_lA", "grad_uA", "grad_l", "grad_u"))
    assert np.all(out.flag == R.OK)
    assert np.all(out.grad_g == 0.0) and np.all(out.grad_H == 0.0)
    assert_y_constructed(p, out, y)


def test_edge_no_rows_no_box():
    p, x, _ = R.constructed(2, 66, 0, box=False)
    assert p["A"] is None and p["l"] is None
    out, _, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb, names=("y", "grad_H", "grad_g"))
    assert np.all(out.flag == R.OK)


def test_edge_active_rows_on_both_sides_of_row_256():
    """nc = 300: the row scan takes more than one pass of 256 threads; active rows in the first pass, at its last row, and beyond"""
    def shape(i, bs, rs):
        rs[3], rs[255], rs[256 + i], rs[299] = 1, -1, 1, 2
        bs[64] = -1
    p, x, y = R.constructed(2, 65, 300, shape=shape)
    out, _, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb)
    assert np.all(out.flag == R.OK)
    for i in range(2):
        assert sorted(np.flatnonzero(out.active[i])) == sorted([64, 65 + 3, 65 + 255, 65 + 256 + i, 65 + 299])
        assert out.active[i, 65 + 299] == 2 and out.active[i, 65 + 255] == -1 and out.active[i, 65 + 256 + i] == 1
    assert_y_constructed(p, out, y)


def test_edge_full_capacity_128_bounds_and_128_rows():
    """n = 128 with every bound active and 128 candidate rows: 2n candidates, the full capacity of 258 columns.  At most n of them
    are independent: DEGENERATE, at most n nonzero multipliers, and they satisfy stationarity (C' has full row rank)"""
    def shape(i, bs, rs):
        bs[:] = [1 if (k + i) % 2 else -1 for k in range(128)]
        rs[:] = [1 if k % 2 else -1 for k in range(128)]
    p, x, _ = R.constructed(2, 128, 128, shape=shape)
    out, _, _ = run_edge(p, x, with_arbiter=False)
    assert np.all(out.flag == R.DEGENERATE)
    cond = R.cond_H(p)
    for i in range(2):
        Hx = (p["H"][i] + p["eps_abs"] * np.eye(128)) @ x[i]
        res = Hx + p["g"][i] - out.y[i, :128] - p["A"][i].T @ out.y[i, 128:]
        print(f"  instance {i}: {np.count_nonzero(out.y[i])} nonzero multipliers, residual {np.max(np.abs(res)):.3e}, "
              f"bound {TOL * cond[i] * max(np.abs(Hx).max(), np.abs(p['g'][i]).max()):.3e}")
        assert np.max(np.abs(res)) <= TOL * cond[i] * max(np.abs(Hx).max(), np.abs(p["g"][i]).max())
        assert np.count_nonzero(out.y[i]) <= 128


def test_edge_more_than_2n_candidates():
    def shape(i, bs, rs):
        bs[:] = -1
        rs[:68] = 1
    p, x, _ = R.constructed(2, 65, 70, shape=shape)
    out, _, arb = run_edge(p, x)
    assert np.all(out.flag == R.DEGENERATE)
    assert [a["flag"] for a in arb] == [R.DEGENERATE] * 2
    assert np.count_nonzero(out.active) <= 2 * 65
    assert np.array_equal(out.active, np.stack([a["active"] for a in arb]))


def test_edge_equal_bounds():
    def shape(i, bs, rs):
        bs[i], bs[64], rs[1] = 2, 2, 2
    p, x, y = R.constructed(2, 65, 3, shape=shape)
    out, _, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb)
    assert np.all(out.flag == R.OK)
    for i in range(2):
        assert out.active[i, i] == 2 and out.active[i, 64] == 2 and out.active[i, 65 + 1] == 2
        assert out.grad_u[i, i] == 0.0 and out.grad_uA[i, 1] == 0.0      # an equality: the lower side carries the derivative
    assert_y_constructed(p, out, y)


def test_edge_one_sided_row():
    def shape(i, bs, rs):
        rs[8], rs[2] = 1, -1

    def post(i, q):
        q["lA"][8], q["uA"][2] = -np.inf, np.inf
    p, x, y = R.constructed(2, 65, 9, shape=shape, post=post)
    out, _, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb)
    assert np.all(out.flag == R.OK)
    assert np.all(out.active[:, 65 + 8] == 1) and np.all(out.active[:, 65 + 2] == -1)
    assert np.all(out.grad_lA[:, 8] == 0.0) and np.all(out.grad_uA[:, 2] == 0.0)
    assert_y_constructed(p, out, y)


def test_edge_row_repeats_an_active_bound():
    def shape(i, bs, rs):
        bs[2], rs[1] = -1, -1

    def post(i, q):
        q["A"][1] = np.eye(65)[2]
        q["lA"][1], q["uA"][1] = q["x"][2], q["x"][2] + 0.5
    p, x, _ = R.constructed(2, 65, 4, shape=shape, post=post)
    out, _, arb = run_edge(p, x)
    assert np.all(out.flag == R.DEGENERATE)
    assert [a["flag"] for a in arb] == [R.DEGENERATE] * 2
    cond = R.cond_H(p)
    for i in range(2):
        Hx = (p["H"][i] + p["eps_abs"] * np.eye(65)) @ x[i]
        res = Hx + p["g"][i] - out.y[i, :65] - p["A"][i].T @ out.y[i, 65:]
        assert np.max(np.abs(res)) <= TOL * cond[i] * max(np.abs(Hx).max(), np.abs(p["g"][i]).max())
        assert np.count_nonzero(out.y[i]) <= 65


def mixed(i, bs, rs):
    for k in range(0, len(bs), 3):
        bs[k] = 1 if (k + i) % 2 else -1
    for r in range(0, min(len(rs), len(bs) // 2), 2):
        rs[r] = 1 if r % 4 else -1


def test_edge_failed_instance_is_skipped():
    """a failed / NaN instance between two good ones (one workgroup walks all three): SKIPPED with all zeros, the neighbours unchanged"""
    p, x, _ = R.constructed(3, 65, 9, shape=mixed)
    good, _, _ = run_edge(p, x, with_arbiter=False)
    xbad = x.copy()
    xbad[1] = np.nan
    gx = np.random.default_rng([65, 5]).normal(size=(3, 65))
    status = np.array([0, abi.STATUS_MAX_ITER, 0], dtype=np.int32)
    for groups in (1, 2):
        out = BG.run_host(p, xbad, gx, status=status, groups=groups)
        assert out.fences_intact()
        assert list(out.flag) == [R.OK, R.SKIPPED, R.OK]
        for k in out.want:
            a, b = getattr(out, k), getattr(good, k)
            assert np.all(np.isfinite(a.astype(float)))
            if k != "flag":
                assert np.all(a[1] == 0)
            assert np.array_equal(a[[0, 2]], b[[0, 2]])
    # NaN in x alone (status says solved), and a status alone
    out2, _, _ = run_edge(p, xbad, with_arbiter=False)
    out3, _, _ = run_edge(p, x, status=np.array([0, abi.STATUS_INFEASIBLE, 0], dtype=np.int32), with_arbiter=False)
    for o in (out2, out3):
        assert list(o.flag) == [R.OK, R.SKIPPED, R.OK] and np.all(o.y[1] == 0.0) and np.all(o.grad_A[1] == 0.0) and np.all(o.grad_H[1] == 0.0)


def test_larger_tolerance_takes_a_near_active_row():
    """active_tol from the options reaches the kernel: a row 1e-6 inside its bound is a candidate at 1e-5 and not at the default"""
    def post(i, q):
        q["uA"][0] = q["A"][0] @ q["x"] + 1e-6
    p, x, _ = R.constructed(2, 65, 3, post=post)
    gx = np.ones((2, 65))
    assert np.all(BG.run_host(p, x, gx).flag == R.OK)
    wide = BG.run_host(p, x, gx, opts=R.options(active_tol=1e-5))
    assert np.all(wide.flag == R.DEGENERATE)          # its multiplier is zero: weakly active, it leaves the set again


# ---- the entry's checks --------------------------------------------------------------------------------------------------------------
def valid_batch(keep, n=65, nc=3):
    p, x, _ = R.constructed(2, n, nc)
    out = R.Outputs(p)
    keep += [p, out]
    return R.structs(p, x, out, lambda a: a.ctypes.data, keep, gx=np.ones((2, n)))


def workspace_for(b, keep, spare=0):
    rc, nbytes, _ = BG.workspace_bytes(b.B, b.n, b.nc)
    assert rc == abi.OK
    buf = np.zeros(nbytes // 8 + 2 + spare, dtype=np.float64)
    keep.append(buf)
    addr = buf.ctypes.data
    return addr + (-addr) % 16, nbytes


SMALL_EDITS = [
    lambda b: None,
    lambda b: setattr(b, "B", -1), lambda b: setattr(b, "n", 0), lambda b: setattr(b, "nc", -1), lambda b: setattr(b, "eps_abs", -1.0),
    lambda b: setattr(b, "H", None), lambda b: setattr(b, "flag", None), lambda b: setattr(b, "A", None), lambda b: setattr(b, "lA", None),
    lambda b: setattr(b, "u", None), lambda b: setattr(b, "grad_x", None), lambda b: setattr(b, "grad_g", b.g), lambda b: setattr(b, "y", b.x),
    lambda b: setattr(b, "B", 0),
]


def test_ws_entry_at_64_and_below_answers_as_sens_check():
    """n <= 64: the answer of osot_qp_sensitivity_batch to the same arguments, code and text, with a NULL workspace; and the same bits"""
    keep = []
    for n in (5, 64):
        for edit in SMALL_EDITS:
            b = valid_batch(keep, n=n)
            edit(b)
            assert BG.host_check(b, None, None, 0) == R.host_check(b)
    o = R.options()
    o.dual_tol = -1e-9
    assert BG.host_check(valid_batch(keep, n=64), o, None, 0) == R.host_check(valid_batch(keep, n=64), o)
    assert BG.host_check(valid_batch(keep, n=64), None, None, 0) == (abi.OK, "")
    p, x, _ = R.constructed(2, 64, 7, shape=mixed)
    gx = np.ones((2, 64))
    small, ws = R.run_host(p, x, gx), BG.run_host(p, x, gx)
    for k in R.Outputs.ALL:
        assert np.array_equal(getattr(small, k), getattr(ws, k)), k


def test_every_refusal_of_the_ws_entry():
    keep = []
    b = valid_batch(keep)
    ws, nbytes = workspace_for(b, keep)
    assert nbytes > 0 and BG.host_check(b, None, ws, nbytes) == (abi.OK, "")
    # what sens_check refuses is refused above 64 too, with its text
    cases = [
        (lambda b: setattr(b, "B", -1), abi.ERR_INVALID, "B is negative"),
        (lambda b: setattr(b, "nc", -1), abi.ERR_INVALID, "nc is negative"),
        (lambda b: setattr(b, "eps_abs", float("nan")), abi.ERR_INVALID, "eps_abs"),
        (lambda b: setattr(b, "H", None), abi.ERR_INVALID, "H / g / x is null"),
        (lambda b: setattr(b, "flag", None), abi.ERR_INVALID, "flag is null"),
        (lambda b: setattr(b, "A", None), abi.ERR_INVALID, "A is null"),
        (lambda b: setattr(b, "uA", None), abi.ERR_INVALID, "A without its bounds"),
        (lambda b: setattr(b, "l", None), abi.ERR_INVALID, "l and u"),
        (lambda b: setattr(b, "grad_x", None), abi.ERR_INVALID, "a gradient output without grad_x"),
        (lambda b: setattr(b, "y", b.x), abi.ERR_INVALID, "aliases"),
        # the checks that are new
        (lambda b: setattr(b, "n", 129), abi.ERR_UNSUPPORTED, "n is above 128"),
        (lambda b: setattr(b, "nc", 2049), abi.ERR_UNSUPPORTED, "nc is above 2048"),
    ]
    for edit, code, text in cases:
        b = valid_batch(keep)
        edit(b)
        rc, why = BG.host_check(b, None, ws, nbytes)
        assert rc == code and text in why, (rc, why, text)
    o = R.options()
    o.rank_tol = -1e-9
    rc, why = BG.host_check(valid_batch(keep), o, ws, nbytes)
    assert rc == abi.ERR_INVALID and "tolerance" in why
    # the workspace
    b = valid_batch(keep)
    for args, text in (((None, nbytes), "the workspace is null"), ((ws + 8, nbytes), "not 16-byte aligned"), ((ws, nbytes - 1), "too small"),
                       ((ws, 0), "too small")):
        rc, why = BG.host_check(b, None, *args)
        assert rc == abi.ERR_INVALID and text in why, (rc, why, text)
    # an input or an output that starts inside the workspace: at its first byte, at its last, and not one byte behind it
    for field in ("H", "x", "grad_x", "y", "grad_A", "flag", "active"):
        for at, refused in ((ws, True), (ws + nbytes - 1, True), (ws + nbytes, False)):
            b = valid_batch(keep)
            setattr(b, field, at)
            rc, why = BG.host_check(b, None, ws, nbytes)
            assert (rc == abi.ERR_INVALID and "inside the workspace" in why) if refused else (rc, why) == (abi.OK, ""), (field, at - ws, rc, why)
    # an empty batch passes whatever its pointers and its workspace; the run is a no-op
    b = abi.QpSensBatch()
    b.n = 100
    assert BG.host_check(b, None, None, 0) == (abi.OK, "")
    assert BG.lib().sens_big_host_run(C.byref(b), None, 1, 1, 0) == abi.OK
    # the sizes osot_qp_sens_workspace_bytes refuses
    for args, code, text in (((-1, 65, 0), abi.ERR_INVALID, "B is negative"), ((1, 0, 0), abi.ERR_INVALID, "n is below 1"),
                             ((1, 129, 0), abi.ERR_UNSUPPORTED, "n is above 128"), ((1, 65, -1), abi.ERR_INVALID, "nc is negative"),
                             ((1, 65, 2049), abi.ERR_UNSUPPORTED, "nc is above 2048")):
        rc, _, why = BG.workspace_bytes(*args)
        assert rc == code and text in why, (args, rc, why)
    assert BG.workspace_bytes(4, 64, 5000)[:2] == (abi.OK, 0)          # (n <= 64 has no row limit and no workspace)


def test_product_entry_refuses_before_any_device_is_touched():
    """libosot_mi355x.so itself, where no GPU is present: the new symbols answer through C, the refusals carry the entry's name and
    the reason, and the workspace's size is the host build's"""
    import os
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = abi.lib()
    keep = []
    b = valid_batch(keep)
    assert lib.osot_qp_sensitivity_batch_ws(C.byref(b), None, None, 0, None) == abi.ERR_INVALID
    assert b"osot_qp_sensitivity_batch_ws: the workspace is null" in lib.osot_last_error()
    b.n = 129
    assert lib.osot_qp_sensitivity_batch_ws(C.byref(b), None, None, 0, None) == abi.ERR_UNSUPPORTED
    assert b"n is above 128" in lib.osot_last_error()
    assert lib.osot_qp_sensitivity_batch(C.byref(valid_batch(keep)), None, None) == abi.ERR_UNSUPPORTED
    assert b"n is above 64" in lib.osot_last_error()
    empty = abi.QpSensBatch()
    empty.n = 100
    assert lib.osot_qp_sensitivity_batch_ws(C.byref(empty), None, None, 0, None) == abi.OK
    nbytes = C.c_size_t(7)
    for B, n, nc in ((1, 64, 9), (2, 65, 40), (5000, 128, 24), (0, 100, 0)):
        assert lib.osot_qp_sens_workspace_bytes(B, n, nc, C.byref(nbytes)) == abi.OK
        assert nbytes.value == BG.workspace_bytes(B, n, nc)[1]
    assert lib.osot_qp_sens_workspace_bytes(1, 129, 0, C.byref(nbytes)) == abi.ERR_UNSUPPORTED
    assert b"osot_qp_sens_workspace_bytes: n is above 128" in lib.osot_last_error()
    assert lib.osot_qp_sens_workspace_bytes(1, 65, 0, None) == abi.ERR_INVALID


def test_workspace_is_sized_by_the_slots_and_the_lds_fits():
    """one slice is Y, n rows of 2n + 2 doubles; the workspace grows with B up to the slot count and no further; the LDS slice --
    L padded, ten n of vectors, 2n norms, the lists and the map (DESIGN.md states these figures) -- fits a CU at the largest shape"""
    lib = BG.lib()
    for n, nc in ((65, 40), (100, 0), (128, 24), (128, 2048)):
        slots, one = lib.sens_big_host_slots(n, nc), lib.sens_big_host_slice_bytes(n)
        assert one == 8 * n * (2 * n + 2) and one % 16 == 0
        lds = lib.sens_big_host_lds_bytes(n, nc)
        assert lds == 8 * (n * (n | 1) + 10 * n + 2 * n + 2) + 4 * (3 * 2 * n + n + (n + nc) + 8)
        assert lds <= 160 * 1024
        assert slots == 256 * max(1, min(4, (160 * 1024) // lds))
        for B, groups in ((0, 0), (1, 1), (slots - 1, slots - 1), (slots, slots), (slots + 1, slots), (100 * slots, slots)):
            assert BG.workspace_bytes(B, n, nc)[:2] == (abi.OK, groups * one)
    assert lib.sens_big_host_slots(65, 40) == 3 * 256 and lib.sens_big_host_slots(128, 24) == 256


def test_sanitized_program():
    """the same file as a stand-alone program under ASan + UBSan, over the same edges: exits 0"""
    exe = BG.ensure_sanitized()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert "qp_sens_big: ok" in r.stdout
