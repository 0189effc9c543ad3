"""The level QPs of the iHQP cascade, their multipliers, active sets and objectives (osot_ihqp_level_qp, osot_ihqp_sensitivity) through
the host lock-step emulation (tests/emu/ihqp_sens_host.cpp): the level QP against the numpy restatement of tests/ihqp_sens_ref.py and
against the reference's qpOASES, y / active / objective against the longdouble arbiter and the reference's own numbers
(tests/golden/ihqp_sens.npz), the backward pass against a longdouble chain through the levels and against central differences of a
longdouble cascade, failed instances, optional outputs, every refusal, and the same file as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU needed.  The tolerances: tests/ihqp_sens_ref.py."""
import ctypes as C
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

from opensot_amd import abi
from oracle import pyref
import helpers
import ihqp_sens_ref as R
import qp_sens_ref

CASES = tuple(R.cases())


@functools.lru_cache(maxsize=None)
def fixture():
    return R.fixture()


def values(fenced):
    return [f.value for f in fenced]


# ---- the level QP --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_level_qp_equals_the_restatement(name):
    """every level of every case, a level that is switched off included: A, l, u and every copied bound bit for bit, H, g and the
    optimality bounds within 2 gamma_K sum|terms| of the longdouble restatement"""
    case, fx = R.cases()[name], fixture()[name]
    for k in range(case.plan.L):
        assert R.host_level_rows(case, k) == case.rows(k)
        out = R.host_level_qp(case, fx["inp"], k, fx["x_levels"])
        assert all(f.intact() for f in out.values())
        worst = R.assert_level_qp(case, fx["inp"], k, fx["x_levels"], {key: f.value for key, f in out.items()})
        print(f"  case {name} level {k}: worst |difference| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", tuple(R.extra_cases()))
def test_level_qp_with_dense_weights_and_regularisation(name):
    """WA / Wb operands, the regularisation task (identity and stored Jacobian), c, a global unit-row block, no box, more stored rows
    than a tile: the level QP at a seeded x"""
    case = R.extra_cases()[name]
    rng = np.random.default_rng([len(name), 31])
    inp = R.draw(case, rng, case.B)
    xl = rng.uniform(-0.5, 0.5, size=(case.B, case.plan.L, case.plan.n))
    for k in range(case.plan.L):
        out = R.host_level_qp(case, inp, k, xl)
        assert all(f.intact() for f in out.values())
        R.assert_level_qp(case, inp, k, xl, {key: f.value for key, f in out.items()})


@pytest.mark.skipif(not pyref.available(), reason="the reference's qpOASES build (oracle/_ref) is not present")
@pytest.mark.parametrize("name", CASES)
def test_reference_solves_the_materialised_level_qps(name):
    """the materialised level QPs handed to the reference's back-end give the fixture's x_k within the project's parity bound 1e-6"""
    case, fx = R.cases()[name], fixture()[name]
    n = case.plan.n
    for k in range(case.plan.L):
        if not case.active(k):
            continue
        rows = case.rows(k)
        out = {key: f.value for key, f in R.host_level_qp(case, fx["inp"], k, fx["x_levels"]).items()}
        for i in range(case.B):
            be = pyref.RefBackEnd(n, rows, pyref.HST_SEMIDEF, R.EPS_FACTOR)
            assert be.initProblem(out["H"][i], out["g"][i], out["A"][i] if rows else None, out["lA"][i] if rows else None,
                                  out["uA"][i] if rows else None, out["l"][i], out["u"][i])
            assert np.max(np.abs(be.getSolution() - fx["x_levels"][i, k])) <= 1e-6, (name, k, i)


# ---- multipliers, active set, objective ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_multipliers_active_set_and_objective(name):
    case, fx = R.cases()[name], fixture()[name]
    out = R.host_sensitivity(case, fx["inp"], fx["x_levels"])
    assert out.fences_intact()
    y, active, flag, objective = values(out.y), values(out.active), values(out.flag), out.objective.value
    worst = R.assert_multipliers(case, fx["inp"], fx["x_levels"], None, y, active, flag, objective, require_ok=name != "e")
    print(f"  case {name}: worst deviation {worst:.3f} SENS_TOL (SENS_TOL = {R.SENS_TOL:.2e} cond2 max|y*|)")
    for k in range(case.plan.L):
        if not case.active(k):
            continue
        # the reference's own set and objective
        prob = R.level_problem(case, fx["inp"], k, fx["x_levels"])
        unique = flag[k] == R.OK
        assert np.array_equal(active[k][unique], qp_sens_ref.reference_active(prob, fx["y"][k])[unique]), (name, k)
        ref = fx["objective"][:, k]
        assert np.all(np.abs(objective[:, k] - ref) <= R.OBJECTIVE_REF_TOL * np.maximum(1.0, np.abs(ref))), (name, k)
    if name == "e":      # six and seven rows in five variables: dependent, flagged, and still a valid answer (assert_multipliers)
        assert np.all(flag[6] == R.DEGENERATE) and np.all(flag[7] == R.DEGENERATE) and all(np.all(flag[k] == R.OK) for k in range(5))
    else:
        assert all(np.all(flag[k] == R.OK) for k in range(case.plan.L) if case.active(k))


def test_failed_instances_are_skipped_at_every_level():
    """(f): shape (b) solved by the emulated cascade with max_iter = 1 -- some instances fail: those are SKIPPED with zeros at every
    level, the others are as the arbiter says; nothing non-finite is written and the fences are intact"""
    case, fx = R.cases()["b"], fixture()["b"]
    inp = fx["inp"]
    plan = dataclasses.replace(case.plan, max_iter=1)
    asm = dict(B=case.B, n=plan.n, L=plan.L, A=inp["A"], b=inp["b"], w=inp["w"], C=None, lo=None, up=None, l=inp["l"], u=inp["u"])
    _, xl, status, _ = helpers.emu_cascade(plan, asm)
    assert np.any(status != 0) and np.any(status == 0), status
    xl[status != 0] = np.nan            # whatever a failed solve left behind must not matter
    out = R.host_sensitivity(case, inp, xl, status)
    assert out.fences_intact()
    y, active, flag, objective = values(out.y), values(out.active), values(out.flag), out.objective.value
    assert all(np.all(np.isfinite(a)) for a in y) and np.all(np.isfinite(objective))
    R.assert_multipliers(case, inp, np.where(np.isnan(xl), 0.0, xl), status, y, active, flag, objective, require_ok=False)
    for k in range(plan.L):
        assert np.all(flag[k][status != 0] == R.SKIPPED) and np.all(flag[k][status == 0] != R.SKIPPED)


def test_every_output_is_optional():
    case, fx = R.cases()["a"], fixture()["a"]
    full = R.host_sensitivity(case, fx["inp"], fx["x_levels"])
    for want in (("y",), ("active",), ("flag",), ("objective",), ()):
        part = R.host_sensitivity(case, fx["inp"], fx["x_levels"], want=want)
        assert part.fences_intact(), want
        for key in want:
            a, b = getattr(part, key), getattr(full, key)
            assert all(np.array_equal(p.value, q.value) for p, q in (zip(a, b) if isinstance(a, list) else [(a, b)])), key


def test_workspace_formula():
    """forward 8 (B (n n + rows n + 2 rows + 4 n) + (B + 1) / 2) bytes, rows = the last level's; the backward pass 8 B (3 n + 2 rows + L n)
    more, grad_A / grad_C 8 B rows n more"""
    for case in R.cases().values():
        n, rows, L = case.plan.n, case.rows(case.plan.L - 1), case.plan.L
        for B in (1, 3, case.B):
            fwd = 8 * (B * (n * n + rows * n + 2 * rows + 4 * n) + (B + 1) // 2)
            assert R.host_workspace_bytes(case, B) == fwd == R.host_workspace_bytes(case, B, False, True)
            assert R.host_workspace_bytes(case, B, True) == fwd + 8 * B * (3 * n + 2 * rows + L * n)
            assert R.host_workspace_bytes(case, B, True, True) == fwd + 8 * B * (3 * n + 2 * rows + L * n + rows * n)


# ---- the backward pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_gradients_against_the_longdouble_chain(name):
    """every gradient output of the emulated kernels against the arbiter's chain (R.backward_arbiter: qp_sens_ref's longdouble
    arbiter and dense KKT solve per level, linked by the pull-back formulas), within SENS_TOL times the product of the condition
    numbers of the levels traversed (R.assert_gradients states the bound); the flags are the arbiter's; the fences are intact"""
    case, fx = R.cases()[name], fixture()[name]
    out, grads = R.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"])
    assert out.fences_intact() and grads.fences_intact()
    worst = R.assert_gradients(case, fx["inp"], fx["x_levels"], fx["grad_dq"], grads.values(), values(out.flag))
    print(f"  case {name}: worst |X - X*| / bound = {worst[0]:.3e} (grad_{worst[1]}, level {worst[2]}, instance {worst[3]})")
    fwd = R.host_sensitivity(case, fx["inp"], fx["x_levels"])       # the forward outputs do not depend on the backward pass
    assert all(np.array_equal(a.value, b.value) for a, b in zip(out.y + out.active + out.flag, fwd.y + fwd.active + fwd.flag))
    assert np.array_equal(out.objective.value, fwd.objective.value)


def test_gradient_outputs_are_optional():
    case, fx = R.cases()["a"], fixture()["a"]
    _, full = R.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"])
    for want in (("b",), ("lo", "u"), ("A",), ("C", "w"), ()):
        _, part = R.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"], want=want)
        assert part.fences_intact(), want
        for (name, a), (_, b) in zip(part.every(), full.every()):
            if name in want:
                assert np.array_equal(a.value, b.value), (want, name)


def test_failed_instances_have_zero_gradients():
    """(f) again: the instances the cascade could not solve contribute zeros, the others are as the arbiter says"""
    case, fx = R.cases()["b"], fixture()["b"]
    inp = fx["inp"]
    plan = dataclasses.replace(case.plan, max_iter=1)
    asm = dict(B=case.B, n=plan.n, L=plan.L, A=inp["A"], b=inp["b"], w=inp["w"], C=None, lo=None, up=None, l=inp["l"], u=inp["u"])
    _, xl, status, _ = helpers.emu_cascade(plan, asm)
    xl[status != 0] = np.nan
    out, grads = R.host_backward(case, inp, xl, fx["grad_dq"], status)
    assert out.fences_intact() and grads.fences_intact()
    assert all(np.all(np.isfinite(f.value)) for _, f in grads.every())
    R.assert_gradients(case, inp, np.where(np.isnan(xl), 0.0, xl), fx["grad_dq"], grads.values(), values(out.flag), status)


FD_STEP = 1e-4


def test_gradients_against_finite_differences():
    """An independent check on case (a): central differences of grad_dq . dq through a longdouble cascade whose active sets are held
    fixed (each level: the dense KKT system of the restated level QP on the arbiter's set, with the bound values on the right-hand
    side), for every entry of b, w, lo, up, l, u and three random entries of each A[k] and of C.  Stated against the step h = 1e-4:
    the quotient's own error is taken from the longdouble cascade itself as ten times |FD(h) - FD(h / 2)| (three quarters of the
    h^2 truncation term plus the rounding of both), and the emulated float64 gradient gets 1e-6 max(1, max|gradient|) = 100 h^2 --
    far inside the bound against the arbiter (SENS_TOL times two condition numbers of 1e8)."""
    T = np.longdouble
    case, fx = R.cases()["a"], fixture()["a"]
    p, n = case.plan, case.plan.n
    _, grads = R.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"])
    got = grads.values()
    rng = np.random.default_rng(17)
    worst = 0.0
    for i in range(3):
        base = {k: ([None if a is None else a[i:i + 1].astype(T) for a in v] if isinstance(v, list) else (None if v is None else v[i:i + 1].astype(T)))
                for k, v in fx["inp"].items()}
        sets = []
        for k in range(p.L):
            prob = R.level_problem(case, fx["inp"], k, fx["x_levels"][i:i + 1] if False else fx["x_levels"])
            arb = qp_sens_ref.arbiter(prob, fx["x_levels"][:, k])[i]
            assert arb["flag"] == R.OK
            sets.append([(idx, side) for idx, side, _, _ in arb["set"]])

        def loss(inp1):
            xl = np.zeros((p.L, n), dtype=T)
            for k in range(p.L):
                q = R.restate_level_qp(case, inp1, 0, k, xl, T)
                m = len(sets[k])
                K, rhs = np.zeros((n + m, n + m), dtype=T), np.zeros(n + m, dtype=T)
                K[:n, :n] = q["H"] + T(R.EPS_ABS) * np.eye(n, dtype=T)
                rhs[:n] = -q["g"]
                for c, (idx, side) in enumerate(sets[k]):
                    K[n + c, :n] = np.eye(n, dtype=T)[idx] if idx < n else q["A"][idx - n]
                    lo, up = (q["l"][idx], q["u"][idx]) if idx < n else (q["lA"][idx - n], q["uA"][idx - n])
                    rhs[n + c] = up if side == 1 else lo
                K[:n, n:] = K[n:, :n].T
                xl[k] = qp_sens_ref.ge_solve(K, rhs)[:n]
            return fx["grad_dq"][i].astype(T) @ xl[-1]

        x_check = np.zeros((p.L, n), dtype=T)       # the fixed-set cascade reproduces the fixture's solution at the unperturbed inputs
        entries = []
        for k in range(p.L):
            entries += [("b", k, (0, r)) for r in range(p.m(k))] + [("w", k, (0, r)) for r in range(p.m(k))]
            entries += [("A", k, (0, int(rng.integers(p.ma(k))), int(rng.integers(n)))) for _ in range(3)]
        entries += [(name, None, (0, r)) for name in ("lo", "up") for r in range(p.nc)] + [(name, None, (0, c)) for name in ("l", "u") for c in range(n)]
        entries += [("C", None, (0, int(rng.integers(p.nc_stored)), int(rng.integers(n)))) for _ in range(3)]
        scale = max(1.0, max(float(np.max(np.abs(f.value[i]))) for _, f in grads.every()))
        for name, k, idx in entries:
            def quotient(h):
                vals = []
                for sgn in (1, -1):
                    q = {key: (list(v) if isinstance(v, list) else v) for key, v in base.items()}
                    arr = (q[name][k] if k is not None else q[name]).copy()
                    arr[idx] += sgn * T(h)
                    if k is not None:
                        q[name][k] = arr
                    else:
                        q[name] = arr
                    vals.append(loss(q))
                return (vals[0] - vals[1]) / (2 * T(h))
            fd, fd2 = quotient(FD_STEP), quotient(FD_STEP / 2)
            g = (got[name][k] if k is not None else got[name])[(i,) + idx[1:]]
            tol = 10.0 * abs(float(fd - fd2)) + 1e-6 * scale
            worst = max(worst, abs(float(fd2) - g) / tol)
            assert abs(float(fd2) - g) <= tol, (i, name, k, idx, float(fd2), g, tol)
    print(f"  worst |fd - grad| / tolerance = {worst:.3e}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def sens_struct(case, fx):
    arr = R.host_arrays(case, fx["inp"], fx["x_levels"])
    qb = R.qp_batch(case, arr, lambda a: a.ctypes.data, case.B)
    out = R.SensOutputs(case, case.B, workspace_bytes=R.host_workspace_bytes(case, case.B))
    return out.struct(qb), (arr, out)


def test_refusals_of_the_sensitivity_entry():
    case, fx = R.cases()["a"], fixture()["a"]
    s, keep = sens_struct(case, fx)
    assert R.host_check(case, s) == (abi.OK, "")
    rc, why = R.host_check(case, s, wide=1)
    assert rc == abi.ERR_UNSUPPORTED and "wide route" in why
    for name in ("x_levels", "status"):
        s, keep = sens_struct(case, fx)
        setattr(s.qp, name, None)
        rc, why = R.host_check(case, s)
        assert rc == abi.ERR_INVALID and ("x_levels / status" in why or "dq/status" in why), (name, why)
    s, keep = sens_struct(case, fx)
    s.workspace = None
    assert R.host_check(case, s) == (abi.ERR_INVALID, "workspace is null")
    s, keep = sens_struct(case, fx)
    s.workspace_bytes -= 8
    assert R.host_check(case, s) == (abi.ERR_INVALID, "workspace is smaller than osot_ihqp_sens_workspace_bytes")
    s, keep = sens_struct(case, fx)
    s.workspace += 4
    assert R.host_check(case, s) == (abi.ERR_INVALID, "workspace is not 8-byte aligned")
    s, keep = sens_struct(case, fx)
    s.y[1] = s.qp.x_levels
    assert R.host_check(case, s) == (abi.ERR_INVALID, "an output aliases an input")
    for inside in (0, 8 * 11):                # the workspace by its byte range: its first address and somewhere in its middle
        s, keep = sens_struct(case, fx)
        s.objective = s.workspace + inside
        assert R.host_check(case, s) == (abi.ERR_INVALID, "an output lies inside the workspace")
    s, keep = sens_struct(case, fx)
    s.qp.lo = s.workspace + 16
    assert R.host_check(case, s) == (abi.ERR_INVALID, "an input lies inside the workspace")
    # the backward pass: a gradient output without grad_dq; a workspace sized for the forward pass alone
    gdq = np.zeros((case.B, case.plan.n))
    dest = np.zeros(case.B * case.plan.n * 8)
    for name in ("grad_l", "grad_C"):
        s, keep = sens_struct(case, fx)
        setattr(s, name, dest.ctypes.data)
        assert R.host_check(case, s) == (abi.ERR_INVALID, "a gradient output without grad_dq")
    s, keep = sens_struct(case, fx)
    s.grad_b[1] = dest.ctypes.data
    assert R.host_check(case, s) == (abi.ERR_INVALID, "a gradient output without grad_dq")
    s, keep = sens_struct(case, fx)
    s.grad_dq = gdq.ctypes.data
    assert R.host_check(case, s) == (abi.ERR_INVALID, "workspace is smaller than osot_ihqp_sens_workspace_bytes")
    s, keep = sens_struct(case, fx)
    s.grad_dq = gdq.ctypes.data
    s.grad_l = s.grad_dq
    assert R.host_check(case, s)[0] == abi.ERR_INVALID
    s, keep = sens_struct(case, fx)
    s.y[0] = s.y[1]
    assert R.host_check(case, s) == (abi.ERR_INVALID, "two outputs alias")
    s, keep = sens_struct(case, fx)
    assert R.host_check(case, s, max_batch=case.B - 1) == (abi.ERR_INVALID, "batch size exceeds max_batch")
    rc, why = R.host_check(case, s, opts=qp_sens_ref.options(active_tol=-1.0))
    assert rc == abi.ERR_INVALID and "tolerance" in why
    s, keep = sens_struct(case, fx)
    s.qp.lo = None
    assert R.host_check(case, s) == (abi.ERR_INVALID, "plan has constraint rows but lo/up is null")
    s, keep = sens_struct(case, fx)
    s.qp.B = 0
    assert R.host_check(case, s) == (abi.OK, "")


@pytest.mark.parametrize("name", tuple(R.extra_cases()))
def test_backward_is_refused_on_dense_weight_and_regularised_plans(name):
    """forward works for them (test_level_qp_with_dense_weights_and_regularisation); grad_dq is refused with the reason"""
    case = R.extra_cases()[name]
    rng = np.random.default_rng(3)
    inp = R.draw(case, rng, case.B)
    xl = np.zeros((case.B, case.plan.L, case.plan.n))
    arr = R.host_arrays(case, inp, xl)
    out = R.SensOutputs(case, case.B, workspace_bytes=R.host_workspace_bytes(case, case.B, True, True))
    s = out.struct(R.qp_batch(case, arr, lambda a: a.ctypes.data, case.B))
    assert R.host_check(case, s) == (abi.OK, "")
    gdq = np.zeros((case.B, case.plan.n))
    s.grad_dq = gdq.ctypes.data
    rc, why = R.host_check(case, s)
    assert rc == abi.ERR_UNSUPPORTED and "backward pass is not built for plans with a" in why and "forward works" in why


def test_refusals_of_the_level_qp_entry():
    case, fx = R.cases()["a"], fixture()["a"]
    arr = R.host_arrays(case, fx["inp"], fx["x_levels"])
    pd = case.plan.to_c()
    dest = np.zeros(case.B * (case.plan.n + case.rows(1)) * case.plan.n)

    def answer(level=1, wide=0, max_batch=case.B, edit=None, null_out=None):
        qb = R.qp_batch(case, arr, lambda a: a.ctypes.data, case.B)
        lq = abi.LevelQp()
        for key in ("H", "g", "A", "lA", "uA", "l", "u"):
            setattr(lq, key, None if key == null_out else dest.ctypes.data)
        if edit:
            edit(qb)
        why = C.c_char_p()
        rc = R.lib().ihqp_host_level_qp(C.byref(pd), wide, max_batch, None, C.byref(qb), level, C.byref(lq), 0, C.byref(why))
        return rc, (why.value or b"").decode()

    assert answer() == (abi.OK, "")
    for level in (-1, 2):
        assert answer(level=level) == (abi.ERR_INVALID, "level out of range")
    rc, why = answer(wide=1)
    assert rc == abi.ERR_UNSUPPORTED and "wide route" in why
    assert answer(max_batch=case.B - 1) == (abi.ERR_INVALID, "batch size exceeds max_batch")
    assert answer(null_out="lA") == (abi.ERR_INVALID, "a member of the output is null")
    assert answer(edit=lambda qb: setattr(qb, "x_levels", None)) == (abi.ERR_INVALID, "x_levels is null")
    assert answer(level=0, edit=lambda qb: setattr(qb, "x_levels", None)) == (abi.OK, "")
    assert answer(edit=lambda qb: setattr(qb, "C", None)) == (abi.ERR_INVALID, "plan has stored constraint rows but C is null")


# ---- the sanitized stand-alone program -----------------------------------------------------------------------------------------------
def test_sanitized_program():
    """tests/emu/ihqp_sens_host.cpp with its own main under ASan + UBSan over the smallest case: exact-size heap arrays, sentinels
    around the outputs and the workspace"""
    res = subprocess.run([R.ensure_sanitized()], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0 and "ihqp_sens: ok" in res.stdout
