"""osot_qp_sens_kernel through the host lock-step emulation (tests/emu/qp_sens_host.cpp): multipliers, active set and backward pass
of the explicit QP against the longdouble arbiter of tests/qp_sens_ref.py, the reference's own multipliers (tests/golden/qp_sens.npz),
central finite differences through the CPU oracle's QP solve, the edges, every refusal of sens_check, and the same file as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU needed."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from opensot_amd import abi
import qp_sens_ref as R


@functools.lru_cache(maxsize=None)
def fixture():
    return R.fixture()


@functools.lru_cache(maxsize=None)
def fixture_arbiter(s):
    p, x, _, gx = fixture()[s]
    return R.arbiter(p, x, gx)


def assert_matches_arbiter(p, out, arb, names=("y",) + R.GRADS):
    for name in names:
        dev = R.worst_deviation(p, out, arb, names=(name,))
        print(f"  {name:8s} worst deviation {dev[0]:.3e} (instance {dev[2]}), SENS_TOL {R.SENS_TOL:.3e}")
        assert dev[0] <= R.SENS_TOL, dev
    assert [int(f) for f in out.flag] == [a["flag"] for a in arb]
    assert np.array_equal(out.active, np.stack([a["active"] for a in arb]))


@pytest.mark.parametrize("s", range(len(R.SHAPES)))
def test_fixture_multipliers_and_gradients(s):
    """x = the reference's x: y within SENS_TOL of the arbiter, the set the reference's, every flag OK, the seven gradients within
    SENS_TOL of the arbiter's dense KKT solve"""
    p, x, y_ref, gx = fixture()[s]
    arb = fixture_arbiter(s)
    out = R.run_host(p, x, gx)
    assert out.fences_intact()
    assert np.all(out.flag == R.OK)
    assert np.array_equal(out.active, R.reference_active(p, y_ref))
    assert_matches_arbiter(p, out, arb)
    assert np.array_equal(out.grad_H, np.transpose(out.grad_H, (0, 2, 1)))          # symmetric to the bit
    # the reference's own multipliers, for the record of the run (REFERENCE_WORST is the worst of these)
    print("  reference's y:", R.worst_deviation(p, dict(y=y_ref), arb, names=("y",)))


def test_multipliers_only_leaves_gradients_alone():
    p, x, _, gx = fixture()[0]
    full = R.run_host(p, x, gx)
    only = R.run_host(p, x)
    assert only.fences_intact()
    assert np.array_equal(only.y, full.y) and np.array_equal(only.active, full.active) and np.array_equal(only.flag, full.flag)


# ---- finite differences ------------------------------------------------------------------------------------------------------------
FD_STEP = 1e-6


def fd_bound(p, i, x, gx):
    """What central differences of l = grad_x . x(theta) with step h can show on instance i.  Inside one active set x(theta) is a
    smooth (rational) function of the data, linear in g and the bounds.
      rounding:   each solve carries |dx| <= n u cond2(H~) max|x| (a backward-stable solve of the reduced system), so the quotient
                  is off by at most |grad_x|_1 n u cond2(H~) max|x| / h;
      truncation: h^2 / 6 times the third derivative, which for an entry of H or A is at most 6 |H~^-1|^3 |grad_x| (|g| + |y|_1 + |x|)
                  (three factors of the inverse of the reduced matrix, each bounded by |H~^-1|_2).
    The bound is ten times their sum (the margin this project gives such estimates)."""
    n = p["n"]
    Ht = p["H"][i] + p["eps_abs"] * np.eye(n)
    cond, inv = np.linalg.cond(Ht), np.linalg.norm(np.linalg.inv(Ht), 2)
    rounding = np.abs(gx).sum() * n * 2.0 ** -53 * cond * np.abs(x).max() / FD_STEP
    truncation = FD_STEP ** 2 * inv ** 3 * np.linalg.norm(gx) * (np.abs(p["g"][i]).max() + 2.0 * n + np.abs(x).max())
    return 10.0 * (rounding + truncation)


def test_gradients_against_finite_differences(oracle):
    """an independent check on the (7, 9) case: central differences of grad_x . x through the CPU oracle's QP solve, against the
    emulated kernel's gradients, for every entry of g, H (moved symmetrically), A and every finite bound.  The step h = FD_STEP =
    1e-6 is the margin the fixture's generator asserts of every gap and multiplier (a step moves a residual by at most h, |x| <= 0.5
    in this case), so that a perturbation stays inside the active set; one that did not would show here as a failure.  The bound:
    fd_bound."""
    p, x_ref, _, gx = fixture()[0]
    n, nc = p["n"], p["nc"]
    out = R.run_host(p, x_ref, gx)

    def loss(i, q):
        ok, x, _ = oracle.backend_solve(q["H"], q["g"], q["A"], q["lA"], q["uA"], q["l"], q["u"], p["eps_abs"])
        assert ok
        return float(gx[i] @ x)

    worst = 0.0
    for i in range(p["B"]):
        bound = fd_bound(p, i, x_ref[i], gx[i])
        base = {k: p[k][i].copy() for k in ("H", "g", "A", "lA", "uA", "l", "u")}

        def quotient(name, idx, mirror=None):
            vals = []
            for sgn in (1.0, -1.0):
                q = {k: v.copy() for k, v in base.items()}
                q[name][idx] += sgn * FD_STEP
                if mirror is not None:
                    q[name][mirror] += sgn * FD_STEP
                vals.append(loss(i, q))
            return (vals[0] - vals[1]) / (2.0 * FD_STEP)

        checks = [("g", (k,), None, out.grad_g[i, k]) for k in range(n)]
        checks += [("H", (a, b), None if a == b else (b, a), out.grad_H[i, a, b] + (0.0 if a == b else out.grad_H[i, b, a]))
                   for a in range(n) for b in range(a + 1)]
        checks += [("A", (r, k), None, out.grad_A[i, r, k]) for r in range(nc) for k in range(n)]
        for name, got in (("lA", out.grad_lA), ("uA", out.grad_uA), ("l", out.grad_l), ("u", out.grad_u)):
            checks += [(name, (k,), None, got[i, k]) for k in range(base[name].shape[0]) if np.isfinite(base[name][k])]
        for name, idx, mirror, got in checks:
            fd = quotient(name, idx, mirror)
            worst = max(worst, abs(fd - got) / bound)
            assert abs(fd - got) <= bound, (i, name, idx, fd, got, bound)
    print(f"  worst |fd - grad| / bound = {worst:.3e}")


# ---- the edges, each at B = 3 --------------------------------------------------------------------------------------------------------
def run_edge(p, x, seed=5, status=None, want=None):
    gx = np.random.default_rng([p["n"], seed]).normal(size=(p["B"], p["n"]))
    out = R.run_host(p, x, gx, status=status, want=want)
    assert out.fences_intact()
    for k in out.want:
        assert np.all(np.isfinite(getattr(out, k).astype(float)))
    return out, gx, R.arbiter(p, x, gx, status=status)


def assert_y_constructed(p, out, y):
    """the multipliers the instance was constructed with come back (to the conditioning of H~)"""
    cond = R.cond_H(p)
    for i in range(p["B"]):
        assert np.max(np.abs(out.y[i] - y[i])) <= 1e3 * 2.0 ** -53 * cond[i] * max(1.0, np.abs(y[i]).max()) * p["n"]


def test_edge_n1():
    def shape(i, bs, rs):
        if i == 1:
            bs[0] = -1
        if i == 2:
            rs[1] = 1
    p, x, y = R.constructed(3, 1, 2, shape=shape)
    out, _, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb)
    assert np.all(out.flag == R.OK)
    assert_y_constructed(p, out, y)


def test_edge_no_candidate():
    p, x, _ = R.constructed(3, 9, 5)
    out, gx, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb)
    assert np.all(out.flag == R.OK) and np.all(out.y == 0.0) and np.all(out.active == 0)
    cond = R.cond_H(p)
    for i in range(3):
        dx = -np.linalg.solve(p["H"][i] + p["eps_abs"] * np.eye(9), gx[i])
        assert np.max(np.abs(out.grad_g[i] - dx)) <= R.SENS_TOL * cond[i] * np.abs(dx).max()


def test_edge_all_bounds_active():
    def shape(i, bs, rs):
        bs[:] = [1 if (k + i) % 2 else -1 for k in range(len(bs))]
    p, x, y = R.constructed(3, 7, 4, shape=shape)
    out, _, arb = run_edge(p, x)
    # (dx is exactly zero: the arbiter's elimination leaves rounding noise of 1e-20 there, which is no scale to compare against)
    assert_matches_arbiter(p, out, arb, names=("y", "grad_A", "grad_lA", "grad_uA", "grad_l", "grad_u"))
    assert np.all(out.flag == R.OK)
    assert np.all(out.grad_g == 0.0) and np.all(out.grad_H == 0.0)
    assert_y_constructed(p, out, y)


def test_edge_no_rows_no_box():
    p, x, _ = R.constructed(3, 12, 0, box=False)
    assert p["A"] is None and p["l"] is None
    out, _, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb, names=("y", "grad_H", "grad_g"))
    assert np.all(out.flag == R.OK)


def test_edge_one_sided_row():
    def shape(i, bs, rs):
        rs[8], rs[2] = 1, -1

    def post(i, q):
        q["lA"][8], q["uA"][2] = -np.inf, np.inf
    p, x, y = R.constructed(3, 7, 9, shape=shape, post=post)
    out, _, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb)
    assert np.all(out.flag == R.OK)
    assert np.all(out.active[:, 7 + 8] == 1) and np.all(out.active[:, 7 + 2] == -1)
    assert np.all(out.grad_lA[:, 8] == 0.0) and np.all(out.grad_uA[:, 2] == 0.0)
    assert_y_constructed(p, out, y)


def test_edge_equal_bounds():
    def shape(i, bs, rs):
        bs[i], rs[1] = 2, 2
    p, x, y = R.constructed(3, 7, 3, shape=shape)
    out, _, arb = run_edge(p, x)
    assert_matches_arbiter(p, out, arb)
    assert np.all(out.flag == R.OK)
    for i in range(3):
        assert out.active[i, i] == 2 and out.active[i, 7 + 1] == 2
        assert out.grad_u[i, i] == 0.0 and out.grad_uA[i, 1] == 0.0      # an equality: the lower side carries the derivative
    assert_y_constructed(p, out, y)


def mixed(i, bs, rs):
    for k in range(0, len(bs), 3):
        bs[k] = 1 if (k + i) % 2 else -1
    for r in range(0, min(len(rs), len(bs) // 2), 2):
        rs[r] = 1 if r % 4 else -1


def test_edge_failed_instance_is_skipped():
    p, x, _ = R.constructed(3, 7, 9, shape=mixed)
    good, _, _ = run_edge(p, x)
    xbad = x.copy()
    xbad[1] = np.nan
    out, _, arb = run_edge(p, xbad, status=np.array([0, abi.STATUS_MAX_ITER, 0], dtype=np.int32))
    assert list(out.flag) == [R.OK, R.SKIPPED, R.OK]
    for k in out.want:
        a, b = getattr(out, k), getattr(good, k)
        if k != "flag":
            assert np.all(a[1] == 0)
        assert np.array_equal(a[[0, 2]], b[[0, 2]])
    # NaN in x alone (status says solved), and a status alone
    out2, _, _ = run_edge(p, xbad)
    out3, _, _ = run_edge(p, x, status=np.array([0, abi.STATUS_INFEASIBLE, 0], dtype=np.int32))
    for o in (out2, out3):
        assert list(o.flag) == [R.OK, R.SKIPPED, R.OK] and np.all(o.y[1] == 0.0) and np.all(o.grad_A[1] == 0.0)


def test_edge_row_repeats_an_active_bound():
    def shape(i, bs, rs):
        bs[2], rs[1] = -1, -1

    def post(i, q):
        q["A"][1] = np.eye(7)[2]
        q["lA"][1], q["uA"][1] = q["x"][2], q["x"][2] + 0.5
    p, x, _ = R.constructed(3, 7, 4, shape=shape, post=post)
    out, _, arb = run_edge(p, x)
    assert np.all(out.flag == R.DEGENERATE)
    assert [a["flag"] for a in arb] == [R.DEGENERATE] * 3
    cond = R.cond_H(p)
    for i in range(3):
        Hx = (p["H"][i] + p["eps_abs"] * np.eye(7)) @ x[i]
        res = Hx + p["g"][i] - out.y[i, :7] - p["A"][i].T @ out.y[i, 7:]
        assert np.max(np.abs(res)) <= R.SENS_TOL * cond[i] * max(np.abs(Hx).max(), np.abs(p["g"][i]).max())
        assert np.count_nonzero(out.y[i]) <= 7


def test_edge_more_than_2n_candidates():
    def shape(i, bs, rs):
        bs[:] = -1
        rs[:6] = 1
    p, x, _ = R.constructed(3, 5, 8, shape=shape)
    out, _, arb = run_edge(p, x)
    assert np.all(out.flag == R.DEGENERATE)
    assert np.count_nonzero(out.active) <= 3 * 5


def test_larger_tolerance_takes_a_near_active_row():
    """active_tol from the options reaches the kernel: a row 1e-6 inside its bound is a candidate at 1e-5 and not at the default"""
    def post(i, q):
        q["uA"][0] = q["A"][0] @ q["x"] + 1e-6
    p, x, _ = R.constructed(3, 7, 3, post=post)
    gx = np.ones((3, 7))
    assert np.all(R.run_host(p, x, gx).flag == R.OK)
    wide = R.run_host(p, x, gx, opts=R.options(active_tol=1e-5))
    assert np.all(wide.flag == R.DEGENERATE)          # its multiplier is zero: weakly active, it leaves the set again


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def valid_batch(keep):
    p, x, _ = R.constructed(2, 5, 3)
    out = R.Outputs(p)
    keep += [p, out]
    return R.structs(p, x, out, lambda a: a.ctypes.data, keep, gx=np.ones((2, 5)))


def test_every_refusal_of_sens_check():
    keep = []
    assert R.host_check(valid_batch(keep)) == (abi.OK, "")
    cases = [
        (lambda b: setattr(b, "B", -1), abi.ERR_INVALID, "B is negative"),
        (lambda b: setattr(b, "n", 0), abi.ERR_INVALID, "n is below 1"),
        (lambda b: setattr(b, "n", 65), abi.ERR_UNSUPPORTED, "n is above 64"),
        (lambda b: setattr(b, "nc", -1), abi.ERR_INVALID, "nc is negative"),
        (lambda b: setattr(b, "eps_abs", -1.0), abi.ERR_INVALID, "eps_abs"),
        (lambda b: setattr(b, "eps_abs", float("nan")), abi.ERR_INVALID, "eps_abs"),
        (lambda b: setattr(b, "H", None), abi.ERR_INVALID, "H / g / x is null"),
        (lambda b: setattr(b, "g", None), abi.ERR_INVALID, "H / g / x is null"),
        (lambda b: setattr(b, "x", None), abi.ERR_INVALID, "H / g / x is null"),
        (lambda b: setattr(b, "flag", None), abi.ERR_INVALID, "flag is null"),
        (lambda b: setattr(b, "A", None), abi.ERR_INVALID, "A is null"),
        (lambda b: setattr(b, "lA", None), abi.ERR_INVALID, "A without its bounds"),
        (lambda b: setattr(b, "uA", None), abi.ERR_INVALID, "A without its bounds"),
        (lambda b: setattr(b, "l", None), abi.ERR_INVALID, "l and u"),
        (lambda b: setattr(b, "u", None), abi.ERR_INVALID, "l and u"),
        (lambda b: setattr(b, "grad_x", None), abi.ERR_INVALID, "a gradient output without grad_x"),
        (lambda b: setattr(b, "grad_g", b.g), abi.ERR_INVALID, "aliases"),
        (lambda b: setattr(b, "y", b.x), abi.ERR_INVALID, "aliases"),
    ]
    for edit, code, text in cases:
        b = valid_batch(keep)
        edit(b)
        rc, why = R.host_check(b)
        assert rc == code and text in why, (rc, why, text)
    for field in ("active_tol", "dual_tol", "rank_tol"):
        o = R.options()
        setattr(o, field, -1e-9)
        rc, why = R.host_check(valid_batch(keep), o)
        assert rc == abi.ERR_INVALID and "tolerance" in why
    # an empty batch passes whatever its pointers; a gradient output alone without grad_x does not
    b = abi.QpSensBatch()
    b.n = 3
    assert R.host_check(b)[0] == abi.OK
    assert R.lib().sens_host_run(C.byref(b), None) == abi.OK


def test_lds_slice():
    """the slice the launch asks for: L, Y with 2n + 2 columns, twelve n of vectors and the lists (DESIGN.md 4.10 states these figures)"""
    assert R.lib().sens_host_lds_bytes(32) == 8 * (32 * 33 + 66 * 33 + 12 * 32 + (13 * 32 + 1) // 2)
    assert R.lib().sens_host_lds_bytes(64) == 8 * (64 * 65 + 130 * 65 + 12 * 64 + (13 * 64 + 1) // 2)
    assert R.lib().sens_host_lds_bytes(64) <= 160 * 1024


def test_sanitized_program():
    """the same file as a stand-alone program under ASan + UBSan, over the same edges: exits 0"""
    exe = R.ensure_sanitized()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "qp_sens: ok" in r.stdout
