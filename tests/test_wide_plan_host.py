"""Batched iHQP plans of 65 .. 128 variables, CPU side: the validator of the workgroup route (osot_plan_validate_wide) and the wide
cascade source (opensot_amd/csrc/osot_cascade_wide.h) compiled for the host (tests/emu/cascade_wide_host.cpp) -- with a team of one
thread against the oracle, and with a turn-taking team of four threads against the team of one under two schedules."""
import ctypes as C
import os

import numpy as np
import pytest

from opensot_amd import abi, synth
from opensot_amd.solver import stored_rows
import native_build
from helpers import null_batch_pointer
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_wide = None


def wide_lib():
    global _wide
    if _wide is None:
        _wide = native_build.load("wide_host")
        _wide.wide_host_ihqp.argtypes = [C.POINTER(abi.PlanDesc), C.POINTER(abi.QpBatch), C.c_void_p, C.c_int, C.c_int]
        _wide.wide_host_tolerances.argtypes = [C.POINTER(C.c_double)]
        _wide.wide_host_tolerances.restype = None
    return _wide


def wide_host(plan, asm, active=None, task_active=None, nthreads=1, t0_last=False, drop=None):
    """the wide cascade on host arrays (asm: oracle layout) -> dq, x_levels, status, iterations, accepted_slack
    drop: (name, level or None) of a batch pointer to hand over as null -- the return code alone comes back"""
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
    pd = plan.to_c()
    if drop is not None:
        null_batch_pointer(qb, *drop)
    rc = wide_lib().wide_host_ihqp(C.byref(pd), C.byref(qb), C.cast(ta, C.c_void_p) if ta is not None else None,
                                   nthreads, 1 if t0_last else 0)
    if drop is not None:
        return rc
    assert rc == 0
    return dq, xl, st, it, slack


def generic_wide(B, n, seed, **kw):
    """two generic levels + an implicit Postural block, equality / inequality / task-local rows, a box as unit rows and a generic box"""
    args = dict(level_rows=[12, 20], n_eq=6, n_ineq=24, n_local=6, local_level=1, unit_box=(None, 0.6), seed=seed)
    args.update(kw)
    return synth.make_generic_stack(B, n, **args)


def oracle_solve(asm, active=None):
    return pyoracle.ihqp_solve_batch(asm, pyoracle.BE_EIQP_EQ, nthreads=4, active=active)


def close(a, b, tol=1e-8):
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# ---- the batch check of osot_ihqp_solve (fill_batch_ptrs, osot_plan_shape.h) is the one the host build runs -----------------------
MISSING_POINTERS = [("b", 1), ("A", 0), ("lo", None), ("up", None), ("l", None), ("u", None), ("dq", None), ("b_reg", None)]


@pytest.mark.parametrize("drop", MISSING_POINTERS, ids=lambda d: d[0] if d[1] is None else f"{d[0]}{d[1]}")
def test_missing_batch_pointer_is_refused(drop):
    """a null b[k], a null A[k] on a level with stored rows, lo/up missing with constraint rows, l/u missing with bounds, a null dq,
    b_reg missing with a regularisation task: OSOT_ERR_INVALID, as from osot_ihqp_solve on a wide handle -- not a fault of the process"""
    plan, leaf = generic_wide(2, 70, seed=3)
    synth.add_regularisation(plan, leaf, kind=abi.TASK_GENERIC, rows=None, weight=1e-2, seed=3)
    assert plan.nc > 0 and plan.bounds and plan.ma(0) > 0 and plan.regularisation is not None
    asm = pyoracle.assemble(plan, leaf)
    assert wide_host(plan, asm, drop=drop) == abi.ERR_INVALID
    assert (wide_host(plan, asm)[2] == 0).all()      # (the complete batch is solved)


def test_wide_route_tolerances_are_the_specified_ones():
    """the active-set tolerances as the wide route's own code sees them (osot_qp_tol.h, read from inside namespace big) are the literals
    the rule was specified with -- exact equality: a private copy in osot_qp_big.h with another number would show here"""
    out = (C.c_double * 11)()
    wide_lib().wide_host_tolerances(out)
    names = ("violation", "equality", "dependence", "dependence floor", "ratio", "slack", "slack cap", "span accept",
             "refine floor", "refinements", "infinity")
    spec = (1e-11, 1e-9, 1e-24, 1e-13, 1e-14, 1e-6, 1e-5, 1e-8, 1e-9, 2.0, 1e20)
    assert dict(zip(names, out)) == dict(zip(names, spec))


# ---- validator of the workgroup route ------------------------------------------------------------------------------------------
def _validate(fn, plan):
    pd = plan.to_c()
    return getattr(abi.lib(), fn)(C.byref(pd))


@pytest.mark.parametrize("n", [65, 100, 128])
def test_validate_wide_accepts_up_to_128(n):
    plan, _ = generic_wide(2, n, seed=1)
    assert _validate("osot_plan_validate_wide", plan) == abi.OK
    assert _validate("osot_plan_validate", plan) == abi.ERR_INVALID      # the wavefront route keeps n <= 64
    plan, _ = synth.make_wide_robot_stack(2, n, seed=1)
    assert _validate("osot_plan_validate_wide", plan) == abi.OK


def test_validate_wide_refusals():
    plan, _ = generic_wide(2, 128, seed=1)
    pd = plan.to_c()
    pd.n = 129
    assert abi.lib().osot_plan_validate_wide(C.byref(pd)) == abi.ERR_INVALID
    assert b"1..128" in abi.lib().osot_last_error()
    # a sub-task of a parent wider than the 64-bit row mask
    plan, _ = generic_wide(2, 100, seed=1)
    pd = plan.to_c()
    t = pd.level[0].task[0]
    t.row_mask, t.parent_rows, t.rows = 0b111, 80, 3
    assert abi.lib().osot_plan_validate_wide(C.byref(pd)) == abi.ERR_INVALID
    # more rows than the workgroup solver takes: 8 blocks of 256 rows and the task rows
    plan, _ = synth.make_generic_stack(1, 100, [20, 20], n_ineq=256, seed=1)
    pd = plan.to_c()
    for j in range(1, 8):
        pd.rowblock[j] = pd.rowblock[0]
    pd.n_rowblocks = 8
    assert abi.lib().osot_plan_validate_wide(C.byref(pd)) == abi.ERR_UNSUPPORTED
    assert b"2048" in abi.lib().osot_last_error()
    # a row table that does not fit the LDS of a CU at n = 128 (inside the 2048-row limit)
    plan, _ = synth.make_generic_stack(1, 128, [20, 20], n_ineq=256, seed=1)
    pd = plan.to_c()
    for j in range(1, 7):
        pd.rowblock[j] = pd.rowblock[0]
    pd.n_rowblocks = 7
    assert abi.lib().osot_plan_validate_wide(C.byref(pd)) == abi.ERR_UNSUPPORTED
    assert b"LDS" in abi.lib().osot_last_error()


# ---- the cascade source on the host against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 80, 100, 128])
def test_wide_cascade_host_matches_oracle(n):
    B = 4
    plan, leaf = generic_wide(B, n, seed=n)
    asm = pyoracle.assemble(plan, leaf)
    dq, xl, st, it, slack = wide_host(plan, asm)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all() and (st == 0).all()
    assert close(dq, ref["dq"]) and close(xl, ref["x_levels"])
    assert (it > 0).all() and (slack <= 1e-5).all()


@pytest.mark.parametrize("n", [80, 128])
def test_wide_cascade_host_inactive_level_and_task(n):
    B = 3
    plan, leaf = synth.make_generic_stack(B, n, [10, 8, 14], n_ineq=20, unit_box=(None, 0.6), seed=3 * n)
    plan.levels[1].append(synth.Task(abi.TASK_GENERIC, 5, name="extra"))
    leaf["A"][1] = np.concatenate([leaf["A"][1], np.random.default_rng(1).normal(0, 0.4, size=(B, 5, n))], axis=1)
    leaf["task"][1].append((np.random.default_rng(2).normal(0, 0.05, size=(B, 5)), None, None))
    ta = {(1, 1): False}
    asm = pyoracle.assemble(plan, leaf, task_active=ta)
    act = [True, False, True, True]
    dq, xl, st, _, _ = wide_host(plan, asm, active=act, task_active=ta)
    ref = oracle_solve(asm, active=act)
    assert (ref["status"] == 1).all() and (st == 0).all()
    assert close(dq, ref["dq"])
    for k in (0, 2, 3):
        assert close(xl[:, k], ref["x_levels"][:, k])


def test_wide_robot_stack_host_matches_oracle():
    plan, leaf = synth.make_wide_robot_stack(3, 96, levels=3, seed=5)
    asm = pyoracle.assemble(plan, leaf)
    dq, xl, st, _, _ = wide_host(plan, asm)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all() and (st == 0).all()
    assert close(dq, ref["dq"]) and close(xl, ref["x_levels"])


def test_wide_cascade_host_small_plan_matches_oracle():
    """the workgroup route at any n (BatchedStack(route="wide")): a 48-variable plan"""
    plan, leaf = generic_wide(3, 48, seed=4)
    asm = pyoracle.assemble(plan, leaf)
    dq, _, st, _, _ = wide_host(plan, asm)
    ref = oracle_solve(asm)
    assert (st == 0).all() and close(dq, ref["dq"])


# ---- a team of four threads against the team of one ---------------------------------------------------------------------------
@pytest.mark.parametrize("t0_last", [False, True])
def test_wide_cascade_team_of_four_equals_team_of_one(t0_last):
    """sections of the team run one thread at a time, thread 0 first or last: the same x and iteration counts as a team of one.
    (Thread 0 first reproduces the race of drop_constraint, osot_qp_big.h, without its barrier: the other threads then read the
    working-set size thread 0 has already decremented and skip the last rotation of their rows of J.)"""
    B = 2   # (a tight box under many inequality rows: the dual loop drops constraints from the working set)
    plan, leaf = synth.make_generic_stack(B, 72, [30, 40], n_ineq=120, box=0.05, seed=0)
    asm = pyoracle.assemble(plan, leaf)
    one = wide_host(plan, asm)
    if pyoracle.ref_available():   # (the eiQuadProg restatement stops on this instance; the reference's qpOASES solves it)
        rq = pyoracle.ihqp_solve_batch(asm, pyoracle.BE_QPOASES_REF, nthreads=1)
        assert (rq["status"] == 1).all() and close(one[0], rq["dq"], 1e-9)
    four = wide_host(plan, asm, nthreads=4, t0_last=t0_last)
    assert (one[2] == 0).all()
    assert np.array_equal(one[0], four[0]) and np.array_equal(one[1], four[1])
    assert np.array_equal(one[2], four[2]) and np.array_equal(one[3], four[3])


# ---- the golden inverse-dynamics levels (tests/golden/wide_id_levels.npz: the reference's own qpOASES answers) -------------------
def golden_plan(c):
    """case c of wide_id_levels.npz posed as a two-level PLAN: level 0 = a GENERIC task of 15 rows (A0 = the last 15 rows of the
    second level's constraint matrix, i.e. the first level's optimality rows; b0 from A0'b0 = -g0), level 1 = an implicit Postural
    block over the nv accelerations (H1 = diag(I_nv, 0), b = qref = -g1[:nv]), the first level's constraint rows as global GENERIC
    rows, a GENERIC box.  Returns (plan, asm, x0 exact, x1 exact)."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "wide_id_levels.npz"))
    g = lambda k, nm: d[f"c{c}_k{k}_{nm}"]
    H0, g0, Cg, lo, up, l, u = g(0, "H"), g(0, "g"), g(0, "A"), g(0, "lA"), g(0, "uA"), g(0, "l"), g(0, "u")
    n, nc = H0.shape[0], Cg.shape[0]
    A0 = g(1, "A")[-15:]
    b0 = np.linalg.lstsq(A0.T, -g0, rcond=None)[0]
    nv = int(round(np.trace(g(1, "H"))))
    qref = -g(1, "g")[:nv]
    eps = 2.221e-13 * float(d["eps_factor"])
    plan = synth.StackPlan(n=n, levels=[[synth.Task(abi.TASK_GENERIC, 15, name="id")], [synth.Task(abi.TASK_POSTURAL, nv, name="post")]],
                           bounds=[synth.Bound(abi.BOUND_GENERIC, name="box")], rowblocks=[synth.Rows(abi.ROWS_GENERIC, nc, name="rows")],
                           eps_abs=eps)
    asm = {"B": 1, "n": n, "L": 2, "eps_abs": eps, "m": [15, nv], "ma": [15, 0], "nc": nc,
           "A": [A0[None], None], "b": [b0[None], qref[None]], "w": [None, None], "c": [None, None],
           "C": Cg[None], "lo": lo[None], "up": up[None], "l": l[None], "u": u[None], "reg": None}
    return plan, asm, g(0, "x_qpoases_exact"), g(1, "x_qpoases_exact")


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_wide_cascade_host_golden_id_levels(c):
    plan, asm, x0, x1 = golden_plan(c)
    dq, xl, st, _, _ = wide_host(plan, asm)
    assert st[0] == 0
    assert np.abs(xl[0, 0] - x0).max() < 1e-6 and np.abs(dq[0] - x1).max() < 1e-6


# ---- options beyond the generic stacks: dense weights, c vectors, both regularisation forms, body frames, sub-tasks -------------
def with_dense_operands(plan, asm):
    """W_k A_k and W_k b_k of the levels with a non-diagonal weight (what osot_stack_update writes) from the oracle's level weights"""
    asm = dict(asm)
    asm["WA"] = [None] * plan.L
    asm["Wb"] = [None] * plan.L
    for k, W in enumerate(asm.get("Wdense") or []):
        if W is not None:
            ma = plan.ma(k)
            asm["WA"][k] = W[:, :, :ma] @ asm["A"][k] if ma else None
            asm["Wb"][k] = (W @ asm["b"][k][..., None])[..., 0]
    return asm


@pytest.mark.parametrize("n,reg", [(70, None), (100, "identity"), (100, "dense")])
def test_wide_cascade_host_feature_stack(n, reg):
    B = 3
    plan, leaf = synth.make_feature_stack(B, n=n, seed=n)
    if reg is not None:
        plan, leaf = synth.add_regularisation(plan, leaf, kind=abi.TASK_GENERIC if reg == "dense" else abi.TASK_POSTURAL,
                                              rows=6 if reg == "dense" else n, seed=2, dense=(reg == "dense"))
    asm = pyoracle.assemble(plan, leaf)
    asm = with_dense_operands(plan, asm)
    assert any(w is not None for w in asm["WA"])
    dq, xl, st, _, _ = wide_host(plan, asm)
    assert (st == 0).all()
    ref = oracle_solve(asm)
    ok = ref["status"] == 1
    if ok.any():
        assert close(dq[ok], ref["dq"][ok]) and close(xl[ok], ref["x_levels"][ok])
    solved_by_one = ok.copy()
    if pyoracle.ref_available():    # (each witness stops on some of these instances: every instance against the ones that solve it)
        rq = pyoracle.ihqp_solve_batch(asm, pyoracle.BE_QPOASES_REF, nthreads=1, termination_tolerance=10 * 2.221e-16)
        okq = rq["status"] == 1
        if okq.any():
            assert np.abs(dq[okq] - rq["dq"][okq]).max() < 1e-7
        solved_by_one |= okq
    assert solved_by_one.all()


def test_wide_cascade_host_c_vectors():
    B, n = 3, 90
    plan, leaf = generic_wide(B, n, seed=7)
    asm = pyoracle.assemble(plan, leaf)
    rng = np.random.default_rng(1)
    asm["c"] = [rng.normal(0.0, 0.01, size=(B, n)) for _ in range(plan.L)]     # Task::getc()
    dq, xl, st, _, _ = wide_host(plan, asm)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all() and (st == 0).all()
    assert close(dq, ref["dq"]) and close(xl, ref["x_levels"])


# ---- the default-eps regression fixtures of the wavefront route (degenerate closed-loop instances at iHQP's default eps) ------
def _witnesses(asm):
    re_ = pyoracle.ihqp_solve_batch(asm, pyoracle.BE_EIQP_EQ, nthreads=1)
    wit = [("eiQuadProg", re_)]
    if pyoracle.ref_available():
        wit += [("qpOASES exact", pyoracle.ihqp_solve_batch(asm, pyoracle.BE_QPOASES_REF, nthreads=1, termination_tolerance=10 * 2.221e-16)),
                ("qpOASES", pyoracle.ihqp_solve_batch(asm, pyoracle.BE_QPOASES_REF, nthreads=1))]
    return wit


def _pick(asm, i):
    B = asm["B"]
    sub = {k: (v[i:i + 1] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == B else v) for k, v in asm.items()}
    for k in ("A", "b", "w", "c"):
        sub[k] = [None if v is None else v[i:i + 1] for v in asm[k]]
    sub["B"] = 1
    return sub


# (tasks, 5): the sixth instance of the fixture ends SOLVED 3e-2 from every witness, lexicographically worse at level 1 -- a known
# limitation of the wide route; strict, so that the fix shows
STUCK = [("tasks", i) for i in range(5)] + [pytest.param("tasks", 5, marks=pytest.mark.xfail(strict=True, reason="known: DESIGN.md 4.6")),
                                             ("ttc", 0), ("ttc_exchange", 0)]


@pytest.mark.parametrize("mode,i", STUCK)
def test_wide_cascade_host_default_eps_stuck_instances(mode, i):
    from helpers import answer_is_acceptable, default_eps_stuck_instances
    plan, asm = default_eps_stuck_instances(mode)
    asm = _pick(asm, i)
    dq, _, st, _, slack = wide_host(plan, asm)
    assert st[0] == 0 and slack[0] <= 1e-7
    wit = _witnesses(asm)
    ok, why = answer_is_acceptable(asm, 0, dq[0], [(nm, r["dq"][0], r["status"][0] == 1) for nm, r in wit])
    assert ok, why


def test_wide_cascade_host_accepted_slack_instance():
    from helpers import accepted_slack_instance, answer_is_acceptable
    plan, asm, wit = accepted_slack_instance()
    dq, _, st, _, slack = wide_host(plan, asm)
    assert st[0] == 0
    ok, why = answer_is_acceptable(asm, 0, dq[0], wit)
    assert ok, why
    assert slack[0] <= 1.0e-7
