"""The level QPs of the iHQP cascade, their multipliers, active sets, objectives and the backward pass on the wide route (65 .. 128
variables: osot_ihqp_level_qp / osot_ihqp_sensitivity with a handle of osot_solver_create_wide) through the host build
tests/emu/ihqp_sens_wide_host.cpp: the level QP against the numpy restatement, y / active / objective against the longdouble arbiter
and the reference's own numbers (tests/golden/ihqp_sens_wide.npz), the gradients against the longdouble chain and against central
differences of a longdouble cascade, the turn-taking team of 7 threads in both orders against the team of one, failed instances,
sentinels around every output and the workspace, the workspace formula, every refusal, and the same file as a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU needed.  The tolerances: tests/ihqp_sens_wide_ref.py."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from opensot_amd import abi
import ihqp_sens_ref as R
import ihqp_sens_wide_ref as W
import qp_sens_big_ref
import qp_sens_ref

CASES = tuple(W.cases())


@functools.lru_cache(maxsize=None)
def fixture():
    return W.fixture()


def values(fenced):
    return [f.value for f in fenced]


# ---- the level QP --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_level_qp_equals_the_restatement(name):
    """every level of every case, a level that is switched off included: A, l, u and every copied bound bit for bit, H (symmetric to
    the bit), g and the optimality bounds within 2 gamma_K sum|terms| of the longdouble restatement; the fences are intact"""
    case, fx = W.cases()[name], fixture()[name]
    for k in range(case.plan.L):
        out = W.host_level_qp(case, fx["inp"], k, fx["x_levels"])
        assert all(f.intact() for f in out.values())
        worst = W.assert_level_qp(case, fx["inp"], k, fx["x_levels"], {key: f.value for key, f in out.items()})
        print(f"  case {name} level {k}: worst |difference| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", tuple(W.extra_cases()))
def test_level_qp_with_dense_weights_and_regularisation(name):
    """WA / Wb operands, the regularisation task (identity and stored Jacobian), c, a global unit-row block, no box, more stored rows
    than a tile, at n = 65: the level QP at a seeded x"""
    case = W.extra_cases()[name]
    rng = np.random.default_rng([len(name), 65])
    inp = W.draw(case, rng, case.B)
    xl = rng.uniform(-0.5, 0.5, size=(case.B, case.plan.L, case.plan.n))
    for k in range(case.plan.L):
        out = W.host_level_qp(case, inp, k, xl)
        assert all(f.intact() for f in out.values())
        W.assert_level_qp(case, inp, k, xl, {key: f.value for key, f in out.items()})


# ---- multipliers, active set, objective ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_multipliers_active_set_and_objective(name):
    case, fx = W.cases()[name], fixture()[name]
    out = W.host_sensitivity(case, fx["inp"], fx["x_levels"])
    assert out.fences_intact()
    y, active, flag, objective = values(out.y), values(out.active), values(out.flag), out.objective.value
    worst = W.assert_multipliers(case, fx["inp"], fx["x_levels"], None, y, active, flag, objective)
    print(f"  case {name}: worst deviation {worst:.3f} SENS_TOL (SENS_TOL = {W.SENS_TOL:.2e} cond2 max|y*|)")
    for k in range(case.plan.L):
        if not case.active(k):
            continue
        prob = W.level_problem(case, fx["inp"], k, fx["x_levels"])      # the reference's own set and objective
        assert np.all(flag[k] == W.OK)
        assert np.array_equal(active[k], qp_sens_ref.reference_active(prob, fx["y"][k])), (name, k)
        ref = fx["objective"][:, k]
        assert np.all(np.abs(objective[:, k] - ref) <= W.OBJECTIVE_REF_TOL * np.maximum(1.0, np.abs(ref))), (name, k)


def test_active_sets_of_the_fixture_are_not_trivial():
    """what the cases are for: bounds and rows are active at the last level of q, r and s"""
    fx = fixture()
    for name, k in (("q", 2), ("r", 2), ("s", 1)):
        n = W.cases()[name].plan.n
        for y in fx[name]["y"][k]:
            assert np.count_nonzero(y[:n]) >= 4 and np.count_nonzero(y[n:]) >= 4, name


def test_failed_instances_are_skipped_with_zero_gradients():
    """an instance the cascade did not solve (whatever its x holds) is SKIPPED with zeros at every level and contributes zero gradients;
    the others are as the arbiter says; nothing non-finite is written"""
    case, fx = W.cases()["p"], fixture()["p"]
    status = np.array([0, 3, 0, 0], dtype=np.int32)
    xl = fx["x_levels"].copy()
    xl[1] = np.nan
    out, grads = W.host_backward(case, fx["inp"], xl, fx["grad_dq"], status)
    assert out.fences_intact() and grads.fences_intact()
    y, active, flag, objective = values(out.y), values(out.active), values(out.flag), out.objective.value
    assert all(np.all(np.isfinite(a)) for a in y) and np.all(np.isfinite(objective))
    assert all(np.all(np.isfinite(f.value)) for _, f in grads.every())
    xl0 = np.where(np.isnan(xl), 0.0, xl)
    W.assert_multipliers(case, fx["inp"], xl0, status, y, active, flag, objective)
    W.assert_gradients(case, fx["inp"], xl0, fx["grad_dq"], grads.values(), flag, status)
    for k in range(case.plan.L):
        assert flag[k][1] == W.SKIPPED and np.all(np.delete(flag[k], 1) == W.OK)


def test_every_output_is_optional():
    case, fx = W.cases()["p"], fixture()["p"]
    full = W.host_sensitivity(case, fx["inp"], fx["x_levels"])
    for want in (("y",), ("active", "flag"), ("objective",), ()):
        part = W.host_sensitivity(case, fx["inp"], fx["x_levels"], want=want)
        assert part.fences_intact(), want
        for key in want:
            a, b = getattr(part, key), getattr(full, key)
            assert all(np.array_equal(p.value, q.value) for p, q in (zip(a, b) if isinstance(a, list) else [(a, b)])), key


def test_workspace_formula():
    """the wavefront route's formula (ihqp_sens_host's), rounded up to 16 bytes, plus osot_qp_sens_workspace_bytes(B, n, rows of the
    last level): min(B, slots) slices of n (2n + 2) doubles"""
    for case in W.cases().values():
        n, rows = case.plan.n, case.rows(case.plan.L - 1)
        for B in (1, 3, case.B, 2000):
            rc, slices, _ = qp_sens_big_ref.workspace_bytes(B, n, rows)
            assert rc == abi.OK and slices == min(B, qp_sens_big_ref.lib().sens_big_host_slots(n, rows)) * 8 * n * (2 * n + 2)
            for back, grad_A in ((False, False), (True, False), (True, True)):
                front = (R.host_workspace_bytes(case, B, back, grad_A) + 15) // 16 * 16
                assert W.host_workspace_bytes(case, B, back, grad_A) == (front + slices, front)
    assert W.lib().ihqp_wide_host_level_lds_bytes(65) == 33800 and W.lib().ihqp_wide_host_level_lds_bytes(128) == 67072
    assert W.lib().ihqp_wide_host_pullback_lds_bytes(128) == 35584


# ---- the backward pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_gradients_against_the_longdouble_chain(name):
    """every gradient output against the arbiter's chain (R.backward_arbiter), within SENS_TOL times the product of the condition
    numbers of the levels traversed plus the floor (R.assert_gradients states the bound); the flags are the arbiter's; the fences are
    intact; the forward outputs do not depend on the backward pass"""
    case, fx = W.cases()[name], fixture()[name]
    out, grads = W.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"])
    assert out.fences_intact() and grads.fences_intact()
    worst = W.assert_gradients(case, fx["inp"], fx["x_levels"], fx["grad_dq"], grads.values(), values(out.flag))
    print(f"  case {name}: worst |X - X*| / bound = {worst[0]:.3e} (grad_{worst[1]}, level {worst[2]}, instance {worst[3]})")
    fwd = W.host_sensitivity(case, fx["inp"], fx["x_levels"])
    assert all(np.array_equal(a.value, b.value) for a, b in zip(out.y + out.active + out.flag, fwd.y + fwd.active + fwd.flag))
    assert np.array_equal(out.objective.value, fwd.objective.value)


def test_gradient_outputs_are_optional():
    case, fx = W.cases()["p"], fixture()["p"]
    _, full = W.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"])
    for want in (("b",), ("lo", "u"), ("A",), ("C", "w"), ()):
        _, part = W.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"], want=want)
        assert part.fences_intact(), want
        for (name, a), (_, b) in zip(part.every(), full.every()):
            if name in want:
                assert np.array_equal(a.value, b.value), (want, name)


FD_STEP = 1e-4


def test_gradients_against_finite_differences():
    """An independent check on case (p): central differences of grad_dq . dq through a longdouble cascade whose active sets are held
    fixed (each level: the dense KKT system of the restated level QP on the arbiter's set, with the bound values on the right-hand
    side), for every entry of b, w, lo, up and three random entries of each A[k], of C, of l and of u.  Stated against the step
    h = 1e-4: the quotient's own error is taken from the longdouble cascade itself as ten times |FD(h) - FD(h / 2)|, and the float64
    gradient gets 1e-6 max(1, max|gradient|) = 100 h^2, as tests/test_ihqp_sens_host.py gives it -- far inside the bound against the
    arbiter (SENS_TOL times two condition numbers of 5e8)."""
    T = np.longdouble
    case, fx = W.cases()["p"], fixture()["p"]
    p, n = case.plan, case.plan.n
    _, grads = W.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"])
    got = grads.values()
    rng = np.random.default_rng(65)
    worst = 0.0
    for i in range(2):
        base = {k: ([None if a is None else a[i:i + 1].astype(T) for a in v] if isinstance(v, list) else (None if v is None else v[i:i + 1].astype(T)))
                for k, v in fx["inp"].items()}
        sets = []
        for k in range(p.L):
            arb = qp_sens_ref.arbiter(W.level_problem(case, fx["inp"], k, fx["x_levels"]), fx["x_levels"][:, k])[i]
            assert arb["flag"] == W.OK
            sets.append([(idx, side) for idx, side, _, _ in arb["set"]])

        def cascade(inp1):
            xl = np.zeros((p.L, n), dtype=T)
            for k in range(p.L):
                q = W.restate_level_qp(case, inp1, 0, k, xl, T)
                m = len(sets[k])
                K, rhs = np.zeros((n + m, n + m), dtype=T), np.zeros(n + m, dtype=T)
                K[:n, :n] = q["H"] + T(W.EPS_ABS) * np.eye(n, dtype=T)
                rhs[:n] = -q["g"]
                for c, (idx, side) in enumerate(sets[k]):
                    K[n + c, :n] = np.eye(n, dtype=T)[idx] if idx < n else q["A"][idx - n]
                    lo, up = (q["l"][idx], q["u"][idx]) if idx < n else (q["lA"][idx - n], q["uA"][idx - n])
                    rhs[n + c] = up if side == 1 else lo
                K[:n, n:] = K[n:, :n].T
                xl[k] = qp_sens_ref.ge_solve(K, rhs)[:n]
            return xl

        # the fixed-set cascade reproduces the fixture's solution at the unperturbed inputs, within the project's parity bound
        assert float(np.max(np.abs(cascade(base) - fx["x_levels"][i]))) <= 1e-6
        loss = lambda inp1: fx["grad_dq"][i].astype(T) @ cascade(inp1)[-1]
        entries = []
        for k in range(p.L):
            entries += [("b", k, (0, r)) for r in range(p.m(k))] + [("w", k, (0, r)) for r in range(p.m(k))]
            entries += [("A", k, (0, int(rng.integers(p.ma(k))), int(rng.integers(n)))) for _ in range(3)]
        entries += [(name, None, (0, r)) for name in ("lo", "up") for r in range(p.nc)]
        entries += [(name, None, (0, int(rng.integers(n)))) for name in ("l", "u") for _ in range(3)]
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


# ---- the team: a missing barrier ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("r", "s"))
def test_turn_taking_team_gives_the_bits_of_the_team_of_one(name):
    """7 threads taking turns, thread 0 first and thread 0 last: the level QP of every level, y, active, flag, objective and every
    gradient are the team of one's, bit for bit (7 divides neither 256 owners nor a tile: every ownership loop wraps unevenly)"""
    case, fx = W.cases()[name], fixture()[name]
    one_qp = [W.host_level_qp(case, fx["inp"], k, fx["x_levels"]) for k in range(case.plan.L)]
    one, one_g = W.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"])
    for t0_last in (0, 1):
        for k in range(case.plan.L):
            got = W.host_level_qp(case, fx["inp"], k, fx["x_levels"], nthreads=7, t0_last=t0_last)
            assert all(f.intact() and np.array_equal(f.value, one_qp[k][key].value) for key, f in got.items()), (k, t0_last)
        out, grads = W.host_backward(case, fx["inp"], fx["x_levels"], fx["grad_dq"], nthreads=7, t0_last=t0_last)
        assert out.fences_intact() and grads.fences_intact()
        for a, b in zip(out.y + out.active + out.flag + [out.objective], one.y + one.active + one.flag + [one.objective]):
            assert np.array_equal(a.value, b.value), t0_last
        for (gname, a), (_, b) in zip(grads.every(), one_g.every()):
            assert np.array_equal(a.value, b.value), (gname, t0_last)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def sens_struct(case, fx, backward=False):
    arr = W.host_arrays(case, fx["inp"], fx["x_levels"])
    qb = W.qp_batch(case, arr, lambda a: a.ctypes.data, case.B)
    out = W.SensOutputs(case, case.B, workspace_bytes=W.host_workspace_bytes(case, case.B, backward)[0])
    return out.struct(qb), (arr, out)


def test_refusals_of_the_sensitivity_entry():
    case, fx = W.cases()["p"], fixture()["p"]
    s, keep = sens_struct(case, fx)
    assert W.host_check(case, s) == (abi.OK, "")
    # a wide handle whose plan has n <= 64 belongs on osot_solver_create: refused as before, whatever the workspace
    small, sfx = R.cases()["a"], R.fixture()["a"]
    ss, skeep = sens_struct(small, sfx)
    rc, why = W.host_check(small, ss)
    assert rc == abi.ERR_UNSUPPORTED and "wide route" in why and "osot_solver_create" in why
    s, keep = sens_struct(case, fx)
    s.workspace = None
    assert W.host_check(case, s) == (abi.ERR_INVALID, "workspace is null")
    s, keep = sens_struct(case, fx)
    s.workspace_bytes -= 8
    assert W.host_check(case, s) == (abi.ERR_INVALID, "workspace is smaller than osot_ihqp_sens_workspace_bytes")
    s, keep = sens_struct(case, fx)      # the wavefront route's size is too small here: the Y slices are missing
    s.workspace_bytes = R.host_workspace_bytes(case, case.B)
    assert W.host_check(case, s) == (abi.ERR_INVALID, "workspace is smaller than osot_ihqp_sens_workspace_bytes")
    s, keep = sens_struct(case, fx)
    s.workspace += 8                     # 8-byte aligned is enough on the wavefront route, not here
    s.workspace_bytes += 8
    assert W.host_check(case, s) == (abi.ERR_INVALID, "workspace is not 16-byte aligned")
    for name in ("x_levels", "status"):
        s, keep = sens_struct(case, fx)
        setattr(s.qp, name, None)
        rc, why = W.host_check(case, s)
        assert rc == abi.ERR_INVALID and ("x_levels / status" in why or "dq/status" in why), (name, why)
    s, keep = sens_struct(case, fx)
    s.y[1] = s.qp.x_levels
    assert W.host_check(case, s) == (abi.ERR_INVALID, "an output aliases an input")
    for inside in (0, 8 * 11, s.workspace_bytes - 8):      # the workspace by its byte range: first address, middle, the last Y slice
        s, keep = sens_struct(case, fx)
        s.objective = s.workspace + inside
        assert W.host_check(case, s) == (abi.ERR_INVALID, "an output lies inside the workspace")
    s, keep = sens_struct(case, fx)
    s.qp.lo = s.workspace + s.workspace_bytes - 16
    assert W.host_check(case, s) == (abi.ERR_INVALID, "an input lies inside the workspace")
    gdq = np.zeros((case.B, case.plan.n))
    dest = np.zeros(case.B * case.plan.n * 8)
    s, keep = sens_struct(case, fx)
    s.grad_l = dest.ctypes.data
    assert W.host_check(case, s) == (abi.ERR_INVALID, "a gradient output without grad_dq")
    s, keep = sens_struct(case, fx)      # a workspace sized for the forward pass alone
    s.grad_dq = gdq.ctypes.data
    assert W.host_check(case, s) == (abi.ERR_INVALID, "workspace is smaller than osot_ihqp_sens_workspace_bytes")
    s, keep = sens_struct(case, fx, backward=True)
    s.grad_dq = gdq.ctypes.data
    assert W.host_check(case, s) == (abi.OK, "")
    s, keep = sens_struct(case, fx)
    s.y[0] = s.y[1]
    assert W.host_check(case, s) == (abi.ERR_INVALID, "two outputs alias")
    s, keep = sens_struct(case, fx)
    assert W.host_check(case, s, max_batch=case.B - 1) == (abi.ERR_INVALID, "batch size exceeds max_batch")
    rc, why = W.host_check(case, s, opts=qp_sens_ref.options(active_tol=-1.0))
    assert rc == abi.ERR_INVALID and "tolerance" in why
    s, keep = sens_struct(case, fx)
    s.qp.B = 0
    assert W.host_check(case, s) == (abi.OK, "")


@pytest.mark.parametrize("name", tuple(W.extra_cases()))
def test_backward_is_refused_on_dense_weight_and_regularised_plans(name):
    """forward works for them (test_level_qp_with_dense_weights_and_regularisation); grad_dq is refused with the reason"""
    case = W.extra_cases()[name]
    inp = W.draw(case, np.random.default_rng(3), case.B)
    xl = np.zeros((case.B, case.plan.L, case.plan.n))
    arr = W.host_arrays(case, inp, xl)
    out = W.SensOutputs(case, case.B, workspace_bytes=W.host_workspace_bytes(case, case.B, True, True)[0])
    s = out.struct(W.qp_batch(case, arr, lambda a: a.ctypes.data, case.B))
    assert W.host_check(case, s) == (abi.OK, "")
    gdq = np.zeros((case.B, case.plan.n))
    s.grad_dq = gdq.ctypes.data
    rc, why = W.host_check(case, s)
    assert rc == abi.ERR_UNSUPPORTED and "backward pass is not built for plans with a" in why and "forward works" in why


def test_refusals_of_the_level_qp_entry():
    case, fx = W.cases()["p"], fixture()["p"]
    dest = np.zeros(case.B * (case.plan.n + case.rows(1)) * case.plan.n)

    def answer(case=case, fx=fx, level=1, wide=1, max_batch=None, edit=None, null_out=None):
        arr = W.host_arrays(case, fx["inp"], fx["x_levels"])
        pd = case.plan.to_c()
        qb = W.qp_batch(case, arr, lambda a: a.ctypes.data, case.B)
        lq = abi.LevelQp()
        for key in ("H", "g", "A", "lA", "uA", "l", "u"):
            setattr(lq, key, None if key == null_out else dest.ctypes.data)
        if edit:
            edit(qb)
        why = C.c_char_p()
        rc = W.lib().ihqp_wide_host_level_qp(C.byref(pd), wide, case.B if max_batch is None else max_batch, None, C.byref(qb), level, C.byref(lq),
                                             0, 1, 0, C.byref(why))
        return rc, (why.value or b"").decode()

    assert answer() == (abi.OK, "")
    rc, why = answer(case=R.cases()["a"], fx=R.fixture()["a"])        # a wide handle with n <= 64
    assert rc == abi.ERR_UNSUPPORTED and "wide route" in why
    for level in (-1, 2):
        assert answer(level=level) == (abi.ERR_INVALID, "level out of range")
    assert answer(max_batch=case.B - 1) == (abi.ERR_INVALID, "batch size exceeds max_batch")
    assert answer(null_out="lA") == (abi.ERR_INVALID, "a member of the output is null")
    assert answer(edit=lambda qb: setattr(qb, "x_levels", None)) == (abi.ERR_INVALID, "x_levels is null")
    assert answer(level=0, edit=lambda qb: setattr(qb, "x_levels", None)) == (abi.OK, "")
    assert answer(edit=lambda qb: setattr(qb, "C", None)) == (abi.ERR_INVALID, "plan has stored constraint rows but C is null")


# ---- the sanitized stand-alone program -----------------------------------------------------------------------------------------------
def test_sanitized_program():
    """tests/emu/ihqp_sens_wide_host.cpp with its own main under ASan + UBSan over the shape of case p: exact-size heap arrays and LDS
    blocks, sentinels around the outputs and the workspace, the team of one and the team of 7"""
    res = subprocess.run([W.ensure_sanitized()], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0 and "ihqp_sens_wide: ok" in res.stdout
