"""The recursively feasible joint limits (acceleration::JointLimitsViability, JointLimitsECBF, velocity::JointLimitsInvariance) and
velocity::CartesianPositionConstraint, CPU side: row kinds 18 .. 21 and bound kind 3 through both validators, the leaf checks and the
update kernel's host builds (tests/emu: emu_stack_update and the surface / wide build) -- against the numpy restatement of the
reference in tests/limits_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from opensot_amd import abi, synth
from opensot_amd.plan import Bound, Rows, StackPlan, Task

from helpers import emu_lib
from limits_ref import (LO, RECORDED_SENSITIVITY, acc_closed_loop, host_update, invariance_block, invariance_closed_loop, limit_block,
                        position_block, tolerance)
from surface_ref import surface_lib

ATOL = 1e-13      # stored rows of O(1) entries (tests/test_convex_hull_host.py:19)
VIA, ECBF = abi.ROWS_ACC_JOINT_LIMITS_VIABILITY, abi.ROWS_ACC_JOINT_LIMITS_ECBF
WIDE_LONGDOUBLE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
# (dT, qdot_max, qddot_max, p, steps per half, snapshots every): the two settings measured for the issue, and the p = 2 of the GPU loop.
# Every setting keeps 24 snapshots of its loop: every 25th state of the 600-step loop of check 5, and -- the same loop in physical time at
# dT = 1e-3, 6000 steps -- every 250th there (24 x 16 x 70 = the 26 880 sampled states the issue counts its at-limit joints in).
VIABILITY_SETTINGS = ((1e-3, np.pi, 20.0, 2.0, 3000, 250), (1e-2, 2.0, 12.0, 1.0, 300, 25), (1e-2, 2.0, 12.0, 2.0, 300, 25))


def _validate(fn, pd):
    return getattr(abi.lib(), fn)(C.byref(pd))


def update(plan, leaf):
    """the update kernel's host build under the validator of the plan's route (n <= 64: both builds must agree)"""
    rc, res = host_update(surface_lib().surf_stack_update, plan, leaf, 1)
    if plan.n <= abi.MAX_VARS:
        rc2, res2 = host_update(emu_lib().emu_stack_update, plan, leaf)
        assert rc2 == rc
        if rc == abi.OK:
            for k in ("C", "lo", "up", "l", "u"):
                np.testing.assert_array_equal(res[k], res2[k])
    return rc, res


def limit_plan(n, kind, rows=None, first_col=0, dT=0.01, p=1.0):
    rows = n - first_col if rows is None else rows
    return StackPlan(n=n, levels=[[Task(abi.TASK_GENERIC, 1, name="t")]], rowblocks=[Rows(kind, rows, first_col=first_col, dT=dT, p=p, name="joint_limits")])


def limit_leaf(B, n, p0, p1, p2):
    return {"B": B, "A": [np.zeros((B, 1, n))], "task": [[(np.zeros((B, 1)), None, None)]], "bound": [], "rows": [(p0, p1, p2)], "C": [None]}


def invariance_plan(n, dt=1e-3, p=0.9, with_velocity_limits=False):
    bounds = ([Bound(abi.BOUND_VELOCITY_LIMITS, dT=dt)] if with_velocity_limits else []) + [Bound(abi.BOUND_JOINT_LIMITS_INVARIANCE, scaling=p, dT=dt)]
    return StackPlan(n=n, levels=[[Task(abi.TASK_GENERIC, 1, name="t")]], bounds=bounds)


def invariance_leaf(B, n, p0, p1, p2, vmax=None):
    bl = ([(np.full((B, n), vmax), None, None)] if vmax is not None else []) + [(p0, p1, p2)]
    return {"B": B, "A": [np.zeros((B, 1, n))], "task": [[(np.zeros((B, 1)), None, None)]], "bound": bl, "rows": [], "C": []}


def position_plan(n, kind, R, scaling=1.0):
    return StackPlan(n=n, levels=[[Task(abi.TASK_GENERIC, 1, name="t")]], rowblocks=[Rows(kind, R, bound_scaling=scaling, name="position_constraint")])


# ---- inputs: states the restatement's own closed loop visits (computed once per size) ---------------------------------------------------
def limits_of(n, seed=0):
    half = np.random.default_rng(1000 + n + seed).uniform(0.5, 2.5, size=(16, n))
    return -half, half


@functools.lru_cache(maxsize=None)
def viability_inputs(n):
    """per setting: (dT, p, p0 [K * 16][2 n], p1, p2) from the numpy loop of check 5, every `every`-th state"""
    qmin, qmax = limits_of(n)
    out = []
    for dT, vmax, amax, p, steps, every in VIABILITY_SETTINGS:
        r = acc_closed_loop(VIA, qmin, qmax, dT, vmax, amax, p=p, steps=(steps, steps), keep_every=every)
        assert r["violation"] <= 1e-4 and r["active"] == 1.0      # the restatement's own loop, under the reference test's EPS
        K = r["q"].shape[0]
        tile = lambda a: np.tile(a, (K, 1))
        p0 = np.concatenate([r["q"].reshape(K * 16, n), r["qdot"].reshape(K * 16, n)], axis=1)
        out.append((dT, p, p0, tile(np.concatenate([qmin, qmax], axis=1)), np.concatenate([np.full((K * 16, n), vmax), np.full((K * 16, n), amax)], axis=1)))
    return out


@functools.lru_cache(maxsize=None)
def ecbf_inputs(n):
    """the closed loop's states (it never swaps) and one batch of the near-limit sampler (which does) -> p0, p1, p2"""
    qmin, qmax = limits_of(n)
    vmax, amax, alpha = 2.0, 12.0, 15.0
    r = acc_closed_loop(ECBF, qmin, qmax, 1e-2, vmax, amax, alpha=alpha, keep_every=25)
    assert r["violation"] <= 1e-4 and r["active"] == 1.0
    qs, qds = synth.near_limit_states(np.random.default_rng(7), 16, n, qmin, qmax, amax)
    q = np.concatenate([r["q"].reshape(-1, n), qs]); qd = np.concatenate([r["qdot"].reshape(-1, n), qds])
    K = q.shape[0] // 16
    lim = [np.full(q.shape, v) for v in (vmax, amax, alpha, alpha, alpha)]
    return np.concatenate([q, qd], axis=1), np.tile(np.concatenate([qmin, qmax], axis=1), (K, 1)), np.concatenate(lim, axis=1)


@functools.lru_cache(maxsize=None)
def invariance_inputs(n):
    qmin, qmax = limits_of(n)
    r = invariance_closed_loop(qmin, qmax, 1e-3, 2.0, 20.0, 0.9, keep_every=25)
    assert r["violation"] <= np.deg2rad(0.01) and r["acc_excess"] <= 1e-9
    K = r["q"].shape[0]
    return r["q"].reshape(K * 16, n), np.tile(np.concatenate([qmin, qmax, np.full((16, n), 20.0)], axis=1), (K, 1)), r["qdot"].reshape(K * 16, n)


def check_bounds(lo, up, rb_or_bd, p0, p1, p2, recorded, name, block=limit_block):
    """device (or emulated) bounds against the restatement, under the allowance measured on these very inputs -> (lb, ub, swapped)"""
    lb, ub, sw = block(rb_or_bd, p0, p1, p2)
    lbw, ubw, _ = block(rb_or_bd, p0, p1, p2, dtype=np.longdouble)
    assert not np.isnan(lo).any() and not np.isnan(up).any() and not np.isnan(lb).any() and not np.isnan(ub).any()
    assert (lo <= up).all()
    for got, ref, wide, side in ((lo, lb, lbw, "lb"), (up, ub, ubw, "ub")):
        tol, sens = tolerance(ref, wide, recorded, ref)
        err = np.abs(got - ref)
        print(f"{name} {side}: max|device - restatement| = {err.max():.3e}, sensitivity max|fp64 - longdouble| = {sens:.3e}"
              + ("" if WIDE_LONGDOUBLE else " (RECORDED: np.longdouble is no wider than float64 here)"))
        assert (err <= tol).all(), (name, side, float(err.max()))
    return lb, ub, sw


# ---- 1. validators and leaf checks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn,n", [("osot_plan_validate", 12), ("osot_plan_validate", 64), ("osot_plan_validate_wide", 70), ("osot_plan_validate_wide", 128)])
def test_validators_ranges_and_unknown_kinds(fn, n):
    L = abi.lib()
    err = L.osot_last_error
    for kind in (VIA, ECBF):
        plan = limit_plan(n, kind, rows=n - 2, first_col=2)
        assert _validate(fn, plan.to_c()) == abi.OK, err()
        pd = plan.to_c(); pd.rowblock[0].first_col = 3
        assert _validate(fn, pd) == abi.ERR_INVALID and b"unit-row block exceeds the variables" in err()
        pd = plan.to_c(); pd.rowblock[0].first_col = -1
        assert _validate(fn, pd) == abi.ERR_INVALID and b"unit-row block exceeds the variables" in err()
        pd = plan.to_c(); pd.rowblock[0].only_level = 2
        assert _validate(fn, pd) == abi.ERR_INVALID and b"only_level" in err()
        pd = plan.to_c(); pd.rowblock[0].only_level = 1
        assert _validate(fn, pd) == abi.OK
    # Viability: p >= 1 and dT * p > 0
    for dT, p, msg in ((0.01, 0.5, b"viability joint limits: p"), (0.01, float("nan"), b"viability joint limits: p"), (0.0, 1.0, b"dT*p > 0"), (-0.01, 2.0, b"dT*p > 0")):
        pd = limit_plan(n, VIA).to_c()
        pd.rowblock[0].dT, pd.rowblock[0].p = dT, p
        assert _validate(fn, pd) == abi.ERR_INVALID and msg in err(), (dT, p, err())
    # ECBF reads neither: exempt
    pd = limit_plan(n, ECBF).to_c()
    pd.rowblock[0].dT, pd.rowblock[0].p = 0.0, 0.0
    assert _validate(fn, pd) == abi.OK, err()
    # position rows: 1 <= R <= 16
    for kind in (abi.ROWS_POSITION_CARTESIAN, abi.ROWS_POSITION_COM):
        for R, want in ((0, abi.ERR_INVALID), (17, abi.ERR_INVALID), (1, abi.OK), (16, abi.OK)):
            pd = position_plan(n, kind, 5).to_c()
            pd.rowblock[0].rows = R
            assert _validate(fn, pd) == want, (kind, R)
            assert want == abi.OK or b"Cartesian position constraint" in err()
    # the invariance bound: 0 < p <= 1 and dT > 0
    assert _validate(fn, invariance_plan(n, p=1.0).to_c()) == abi.OK, err()
    for dt, p, msg in ((1e-3, 0.0, b"step-ahead predictor"), (1e-3, 1.5, b"step-ahead predictor"), (1e-3, float("nan"), b"step-ahead predictor"),
                       (0.0, 0.9, b"control period"), (-1e-3, 0.9, b"control period")):
        pd = invariance_plan(n).to_c()
        pd.bound[0].dT, pd.bound[0].scaling = dt, p
        assert _validate(fn, pd) == abi.ERR_INVALID and msg in err(), (dt, p, err())
    # what is still no kind
    for kind in (13, 14, 15, 17, 22):
        pd = limit_plan(n, VIA).to_c()
        pd.rowblock[0].kind = kind
        assert _validate(fn, pd) == abi.ERR_UNSUPPORTED and b"unknown row-block kind" in err(), kind
    pd = invariance_plan(n).to_c()
    pd.bound[0].kind = 4
    assert _validate(fn, pd) == abi.ERR_UNSUPPORTED and b"unknown bound kind" in err()
    # the dataclasses refuse the same
    for bad in (lambda: position_plan(n, abi.ROWS_POSITION_COM, 0), lambda: position_plan(n, abi.ROWS_POSITION_CARTESIAN, 17),
                lambda: limit_plan(n, VIA, p=0.5), lambda: limit_plan(n, VIA, dT=0.0), lambda: limit_plan(n, ECBF, rows=n, first_col=1),
                lambda: invariance_plan(n, p=0.0), lambda: invariance_plan(n, p=1.5), lambda: invariance_plan(n, dt=0.0)):
        with pytest.raises(AssertionError):
            bad().to_c()


def test_row_counts_stored_and_not():
    plan = StackPlan(n=12, levels=[[Task(abi.TASK_GENERIC, 1)]],
                     rowblocks=[Rows(VIA, 7, first_col=2, dT=0.01, p=2.0), Rows(abi.ROWS_POSITION_CARTESIAN, 5), Rows(ECBF, 12), Rows(abi.ROWS_POSITION_COM, 16)])
    pd = plan.to_c()
    nc, ncs = C.c_int(0), C.c_int(0)
    assert abi.lib().osot_plan_constraint_rows(C.byref(pd), C.byref(nc)) == abi.OK and nc.value == 40 == plan.nc
    assert abi.lib().osot_plan_stored_constraint_rows(C.byref(pd), C.byref(ncs)) == abi.OK and ncs.value == 21 == plan.nc_stored
    assert plan.rows_stored_offset(3) == 5 and plan.rows_offset(3) == 24


@pytest.mark.parametrize("missing", [0, 1, 2])
def test_update_refuses_a_missing_leaf(missing):
    rng = np.random.default_rng(3)
    B, n, R = 2, 12, 4
    entries = (emu_lib().emu_stack_update, ()), (surface_lib().surf_stack_update, (1,))
    drop = lambda full: [None if i == missing else a for i, a in enumerate(full)]
    for kind, k2 in ((VIA, 2), (ECBF, 5)):
        full = (rng.normal(size=(B, 2 * n)), np.concatenate([-np.ones((B, n)), np.ones((B, n))], axis=1), np.ones((B, k2 * n)))
        for fn, extra in entries:
            assert host_update(fn, limit_plan(n, kind), limit_leaf(B, n, *drop(full)), *extra)[0] == abi.ERR_INVALID, kind
        assert update(limit_plan(n, kind), limit_leaf(B, n, *full))[0] == abi.OK
    for kind, rows in ((abi.ROWS_POSITION_CARTESIAN, 6), (abi.ROWS_POSITION_COM, 3)):
        full = (rng.normal(size=(B, rows, n)), rng.normal(size=(B, 12 if rows == 6 else 3)), rng.normal(size=(B, 4 * R)))
        for fn, extra in entries:
            assert host_update(fn, position_plan(n, kind, R), limit_leaf(B, n, *drop(full)), *extra)[0] == abi.ERR_INVALID, kind
        assert update(position_plan(n, kind, R), limit_leaf(B, n, *full))[0] == abi.OK
    full = (np.zeros((B, n)), np.concatenate([-np.ones((B, n)), np.ones((B, n)), np.full((B, n), 20.0)], axis=1), np.zeros((B, n)))
    for fn, extra in entries:
        assert host_update(fn, invariance_plan(n), invariance_leaf(B, n, *drop(full)), *extra)[0] == abi.ERR_INVALID
    assert update(invariance_plan(n), invariance_leaf(B, n, *full))[0] == abi.OK


# ---- 2. bounds against the restatement, on closed-loop states ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 64, 70])
def test_viability_bounds_on_closed_loop_states(n):
    for dT, p, p0, p1, p2 in viability_inputs(n):
        plan = limit_plan(n, VIA, dT=dT, p=p)
        B = p0.shape[0]
        rc, res = update(plan, limit_leaf(B, n, p0, p1, p2))
        assert rc == abi.OK
        lb, ub, sw = check_bounds(res["lo"], res["up"], plan.rowblocks[0], p0, p1, p2, RECORDED_SENSITIVITY[("viability", dT)], f"viability n={n} dT={dT} p={p}")
        amax = p2[:, n:]
        fl, fu = (np.abs(lb) < amax).mean(), (np.abs(ub) < amax).mean()
        at_limit = int(((p0[:, :n] == p1[:, :n]) | (p0[:, :n] == p1[:, n:])).sum())
        print(f"viability n={n} dT={dT} p={p}: interior lb {fl:.2f}, ub {fu:.2f}, swaps {int(sw.sum())}, states exactly on a limit {at_limit} of {lb.size}")
        # the conditions on the inputs, for EVERY setting by itself
        assert fl >= 0.3 and fu >= 0.3 and sw.sum() >= 1
        # ... except that only a predictor p > 1 lands joints exactly on a limit: with p = 1 the numpy loop never does (0 of 26 880 sampled
        # states at n = 70), so the M2 = -0/0 states come from the two p = 2 settings, each by itself
        assert at_limit >= 1 or p == 1.0


@pytest.mark.parametrize("n", [7, 64, 70])
def test_ecbf_bounds_on_closed_loop_and_near_limit_states(n):
    p0, p1, p2 = ecbf_inputs(n)
    plan = limit_plan(n, ECBF, dT=0.0, p=0.0)
    rc, res = update(plan, limit_leaf(p0.shape[0], n, p0, p1, p2))
    assert rc == abi.OK
    lb, ub, sw = check_bounds(res["lo"], res["up"], plan.rowblocks[0], p0, p1, p2, RECORDED_SENSITIVITY["ecbf"], f"ecbf n={n}")
    amax = p2[:, n:2 * n]
    fl, fu = (np.abs(lb) < amax).mean(), (np.abs(ub) < amax).mean()
    print(f"ecbf n={n}: interior lb {fl:.2f}, ub {fu:.2f}, swaps {int(sw.sum())}")
    assert fl >= 0.3 and fu >= 0.3 and sw.sum() >= 1


@pytest.mark.parametrize("n", [7, 64, 70])
def test_invariance_bound_on_closed_loop_states(n):
    p0, p1, p2 = invariance_inputs(n)
    B = p0.shape[0]
    plan = invariance_plan(n)
    rc, res = update(plan, invariance_leaf(B, n, p0, p1, p2))
    assert rc == abi.OK
    lb, ub, sw = check_bounds(res["l"], res["u"], plan.bounds[0], p0, p1, p2, RECORDED_SENSITIVITY["invariance"], f"invariance n={n}", block=invariance_block)
    print(f"invariance n={n}: swaps {int(sw.sum())} of {lb.size}")
    assert sw.sum() >= 1
    # the merged box is still max l / min u over all bounds of the plan
    plan2 = invariance_plan(n, with_velocity_limits=True)
    rc, res2 = update(plan2, invariance_leaf(B, n, p0, p1, p2, vmax=2.0))
    assert rc == abi.OK
    np.testing.assert_array_equal(res2["l"], np.maximum(res["l"], -2.0 * 1e-3))
    np.testing.assert_array_equal(res2["u"], np.minimum(res["u"], 2.0 * 1e-3))
    assert (res2["l"] != res["l"]).any() and (res2["l"] == res["l"]).any()


def test_limit_block_on_a_column_range():
    """first_col / rows: the block's leaf is indexed by row, whatever columns the rows sit on; other blocks keep their offsets"""
    n, c0, r = 12, 3, 7
    _, _, p0, p1, p2 = viability_inputs(7)[1]
    p0, p1, p2 = p0[:32], p1[:32], p2[:32]
    plan = StackPlan(n=n, levels=[[Task(abi.TASK_GENERIC, 1)]],
                     rowblocks=[Rows(abi.ROWS_UNIT_GENERIC, 2, first_col=0), Rows(VIA, r, first_col=c0, dT=1e-2, p=1.0), Rows(ECBF, r, first_col=c0 + 1)])
    e0, e1, e2 = (a[:32] for a in ecbf_inputs(7))
    leaf = limit_leaf(32, n, None, None, None)
    leaf["rows"] = [(np.full((32, 2), -3.0), np.full((32, 2), 4.0), None), (p0, p1, p2), (e0, e1, e2)]
    leaf["C"] = [None] * 3
    rc, res = update(plan, leaf)
    assert rc == abi.OK
    lv, uv, _ = limit_block(plan.rowblocks[1], p0, p1, p2)
    le, ue, _ = limit_block(plan.rowblocks[2], e0, e1, e2)
    np.testing.assert_array_equal(res["lo"][:, :2], -3.0); np.testing.assert_array_equal(res["up"][:, :2], 4.0)
    np.testing.assert_allclose(res["lo"][:, 2:9], lv, rtol=0, atol=1e-10); np.testing.assert_allclose(res["up"][:, 2:9], uv, rtol=0, atol=1e-10)
    np.testing.assert_allclose(res["lo"][:, 9:], le, rtol=0, atol=1e-12); np.testing.assert_allclose(res["up"][:, 9:], ue, rtol=0, atol=1e-12)


def test_nan_quirk_joint_on_its_limit_at_rest():
    """q == q_max, qdot == 0: M2 = -0/0.  std::min(M1, NaN) is M1 = -0: the reference's bound is [-qddot_max .. 0], not NaN"""
    n = 7
    q = np.zeros((2, n)); q[0] = 1.0; q[1] = -1.0
    p0 = np.concatenate([q, np.zeros((2, n))], axis=1)
    p1 = np.concatenate([-np.ones((2, n)), np.ones((2, n))], axis=1)
    p2 = np.concatenate([np.full((2, n), 2.0), np.full((2, n), 12.0)], axis=1)
    plan = limit_plan(n, VIA, dT=0.01, p=1.0)
    rc, res = update(plan, limit_leaf(2, n, p0, p1, p2))
    assert rc == abi.OK
    lb, ub, _ = limit_block(plan.rowblocks[0], p0, p1, p2)
    np.testing.assert_array_equal(res["lo"], lb); np.testing.assert_array_equal(res["up"], ub)
    assert (res["up"][0] == 0.0).all() and (res["lo"][0] == -12.0).all() and (res["lo"][1] == 0.0).all() and (res["up"][1] == 12.0).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(-(p0[0, n:] * p0[0, n:]) / (2.0 * (p1[0, n:] - p0[0, :n]))).all()      # M2 is NaN there ...
        assert np.isnan(np.minimum(-0.0, np.float64("nan")))                                  # ... and np.minimum would hand it on


# ---- 3. position rows -----------------------------------------------------------------------------------------------------------------
def position_inputs(rng, B, n, R, cart, dyadic=False):
    rows = 6 if cart else 3
    if dyadic:
        d = lambda *sh: rng.integers(-64, 65, size=sh) / 64.0
        J, Ac, bc, x = d(B, rows, n), d(B, R, 3), d(B, R), d(B, 3)
        R9 = np.tile(np.eye(3).reshape(9), (B, 1))
    else:
        J, Ac, bc, x = rng.uniform(-2.0, 2.0, size=(B, rows, n)), rng.normal(size=(B, R, 3)), rng.uniform(-1.0, 1.0, size=(B, R)), rng.uniform(-1.0, 1.0, size=(B, 3))
        Ac /= np.linalg.norm(Ac, axis=2, keepdims=True)
        R9 = synth._rot_exp(rng.normal(0.0, 0.5, size=(B, 3))).reshape(B, 9)
    p1 = np.concatenate([R9, x], axis=1) if cart else x
    return J, p1, np.concatenate([Ac.reshape(B, 3 * R), bc], axis=1)


@pytest.mark.parametrize("kind", [abi.ROWS_POSITION_CARTESIAN, abi.ROWS_POSITION_COM])
@pytest.mark.parametrize("n", [7, 64, 70])
@pytest.mark.parametrize("R", [1, 5, 16])
def test_position_rows_against_the_reference_restatement(kind, n, R):
    B = 8
    cart = kind == abi.ROWS_POSITION_CARTESIAN
    rng = np.random.default_rng(100 * n + R + kind)
    for dyadic, scaling in ((False, 0.7), (True, 0.5)):
        p0, p1, p2 = position_inputs(rng, B, n, R, cart, dyadic)
        plan = position_plan(n, kind, R, scaling)
        rc, res = update(plan, limit_leaf(B, n, p0, p1, p2))      # C is pre-filled with 7.0: every stored entry must be written
        assert rc == abi.OK
        Cw, lo, up = position_block(plan.rowblocks[0], p0, p1, p2, n)
        assert (res["lo"] == LO).all() and (lo == LO).all()
        if dyadic:      # multiples of 2^-6, three-term sums: every operation is exact
            np.testing.assert_array_equal(res["C"], Cw); np.testing.assert_array_equal(res["up"], up)
        else:
            np.testing.assert_allclose(res["C"], Cw, rtol=0, atol=ATOL); np.testing.assert_allclose(res["up"], up, rtol=0, atol=ATOL)
        assert (np.abs(Cw).max(axis=2) > 0.0).all() and (res["C"] != 7.0).all()


def test_position_block_among_other_stored_blocks():
    """stored offset: the position rows land behind a generic block's rows and leave them alone"""
    B, n, R = 4, 12, 3
    rng = np.random.default_rng(8)
    p0, p1, p2 = position_inputs(rng, B, n, R, True)
    g = (rng.normal(size=(B, 2, n)), -np.ones((B, 2)), np.ones((B, 2)))
    plan = StackPlan(n=n, levels=[[Task(abi.TASK_GENERIC, 1)]], rowblocks=[Rows(abi.ROWS_GENERIC, 2), Rows(abi.ROWS_POSITION_CARTESIAN, R, bound_scaling=2.0)])
    leaf = limit_leaf(B, n, None, None, None)
    leaf["rows"], leaf["C"] = [g, (p0, p1, p2)], [None, None]
    rc, res = update(plan, leaf)
    assert rc == abi.OK
    Cw, lo, up = position_block(plan.rowblocks[1], p0, p1, p2, n)
    np.testing.assert_array_equal(res["C"][:, :2], g[0])
    np.testing.assert_allclose(res["C"][:, 2:], Cw, rtol=0, atol=ATOL); np.testing.assert_allclose(res["up"][:, 2:], up, rtol=0, atol=ATOL)
    np.testing.assert_array_equal(res["up"][:, :2], 1.0)


# ---- 4. CartesianVelocity is a TaskToConstraint ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task_kind", [abi.ROWS_TASK_COM, abi.ROWS_TASK_CARTESIAN])
def test_cartesian_velocity_rows_equal_a_generic_band(task_kind):
    """constraints::velocity::CartesianVelocity (CartesianVelocity.cpp:77-96): -v dT <= J dq <= v dT, whatever the pose and its reference.
    (This mapping needs no new kind: the test documents it.)"""
    B, n, dT = 4, 12, 0.005
    rng = np.random.default_rng(21)
    rows = 3 if task_kind == abi.ROWS_TASK_COM else 6
    v = np.array([0.3, 0.2, 0.1] if rows == 3 else [0.3, 0.2, 0.1, 1e3, 1e3, 1e3])
    rb = synth.cartesian_velocity_rows(task_kind, v, dT)
    assert rb.lam == 0.0 and rb.rows == rows
    J = rng.normal(size=(B, rows, n))
    if rows == 3:
        tl = (rng.normal(size=(B, 3)), rng.normal(size=(B, 3)), None)
    else:
        tl = synth._cartesian_leaf(rng, B)
    base = dict(B=B, A=[np.zeros((B, 1, n))], task=[[(np.zeros((B, 1)), None, None)]], bound=[])
    rc, res = update(StackPlan(n=n, levels=[[Task(abi.TASK_GENERIC, 1)]], rowblocks=[rb]), dict(base, rows=[tl], C=[J]))
    assert rc == abi.OK
    band = np.tile(v * dT, (B, 1))
    rc, gen = update(StackPlan(n=n, levels=[[Task(abi.TASK_GENERIC, 1)]], rowblocks=[Rows(abi.ROWS_GENERIC, rows)]), dict(base, rows=[(J, -band, band)], C=[None]))
    assert rc == abi.OK
    for k in ("C", "lo", "up"):
        np.testing.assert_array_equal(res[k], gen[k])
    with pytest.raises(AssertionError):
        synth.cartesian_velocity_rows(abi.ROWS_GENERIC, 0.1, dT)


# ---- 5. the generators ------------------------------------------------------------------------------------------------------------------------
def test_generators_validate_on_both_routes():
    for plan in (synth.make_viability_stack(4, 7, VIA, seed=1, p=2.0)[0], synth.make_viability_stack(4, 7, ECBF, seed=1)[0],
                 synth.make_viability_stack(4, 12, VIA, seed=1, first_col=3, rows=5)[0], synth.make_invariance_stack(4, 7, seed=1)[0],
                 synth.make_position_stack(4, 32, 5, seed=1)[0], synth.make_position_stack(4, 32, 16, seed=1, kind=abi.ROWS_POSITION_COM)[0],
                 synth.make_coman_position_stack(4, seed=1)[0]):
        for fn in ("osot_plan_validate", "osot_plan_validate_wide"):
            assert _validate(fn, plan.to_c()) == abi.OK, abi.lib().osot_last_error()
    plan = synth.make_viability_stack(4, 70, VIA, seed=1)[0]
    assert _validate("osot_plan_validate_wide", plan.to_c()) == abi.OK and _validate("osot_plan_validate", plan.to_c()) == abi.ERR_INVALID
    assert plan.nc == 70 and plan.nc_stored == 0
