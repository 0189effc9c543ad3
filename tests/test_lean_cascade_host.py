"""The lean path of the 32-lane BOX instantiation (osot_kernels.h: lean_plan, cascade_body<32, ., false, true, true>) on the host
emulation: for a full-width, box-only plan the BOX kernel takes a body without padding guards and without the row table; every
other plan takes the body it always took.  Either way the BOX kernel must give the bits of the general instantiation -- dq, every
level's x, status and iteration counts.  WHICH body ran is not observable through the emulation library's entries (emu_ihqp_solve
reports that the BOX kernel ran, not which of its bodies): the plans below are chosen by lean_plan's facts, read off the source."""
import ctypes as C

import numpy as np
import pytest

from helpers import default_eps_stuck_instances, emu_lib, fill_level_ptrs
from opensot_amd import abi, synth
from opensot_amd.solver import stored_rows
from oracle import pyoracle


def batch_of(plan, asm, want_levels=True, active=None):
    """the osot_qp_batch of helpers.emu_cascade, with x_levels optional -> qb, outputs, the arrays to keep alive"""
    B, n, L = asm["B"], asm["n"], asm["L"]
    qb = abi.QpBatch()
    qb.B = B
    keep = []
    fill_level_ptrs(qb, asm, ("A", "b", "w", "c"), keep)
    for name in ("C", "lo", "up", "l", "u"):
        a = asm[name]
        if a is not None:
            if name == "C":
                a = stored_rows(plan, a)
                if a.shape[1] == 0:
                    continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            setattr(qb, name, a.ctypes.data)
    if asm.get("reg") is not None:
        a = np.ascontiguousarray(asm["reg"]["b"], dtype=np.float64)
        keep.append(a)
        qb.b_reg = a.ctypes.data
    out = {"dq": np.zeros((B, n)), "x_levels": np.zeros((B, L, n)), "status": np.full(B, -1, dtype=np.int32),
           "iterations": np.zeros(B, dtype=np.int32), "accepted_slack": np.zeros(B)}
    for name, a in out.items():
        if name != "x_levels" or want_levels:
            setattr(qb, name, a.ctypes.data)
    if active is not None:
        act = (C.c_ubyte * L)(*[1 if a else 0 for a in active])
        keep.append(act)
        qb.level_active = C.addressof(act)
    return qb, out, keep


def run_both(plan, asm, monkeypatch, want_levels=True, active=None):
    """general instantiation, then the BOX one, on the same arrays -> (general, box, did the BOX kernel run)"""
    res = []
    for box in (False, True):
        if box:
            monkeypatch.setenv("OSOT_EMU_BOX", "1")
        else:
            monkeypatch.delenv("OSOT_EMU_BOX", raising=False)
        qb, out, keep = batch_of(plan, asm, want_levels, active)
        pd = plan.to_c()
        rc = emu_lib().emu_ihqp_solve(C.byref(pd), C.byref(qb), None, None)
        assert rc in (0, 100)
        res.append((out, rc == 100))
    assert not res[0][1]
    return res[0][0], res[1][0], res[1][1]


def assert_same_bits(full, box):
    for name in ("dq", "x_levels", "status", "iterations", "accepted_slack"):
        assert np.array_equal(full[name], box[name]), name


@pytest.mark.parametrize("cfg", ["C3", "C2"])
def test_lean_body_gives_the_general_bits(cfg, monkeypatch):
    plan, leaf = synth.make_velocity_stack(cfg, 16, seed=311)
    asm = pyoracle.assemble(plan, leaf)
    full, box, ran_box = run_both(plan, asm, monkeypatch)
    assert ran_box
    assert_same_bits(full, box)
    assert (box["status"] == 0).all() and (box["iterations"] > 0).any()


def test_lean_body_without_level_outputs(monkeypatch):
    plan, leaf = synth.make_velocity_stack("C3", 16, seed=312)
    asm = pyoracle.assemble(plan, leaf)
    full, box, ran_box = run_both(plan, asm, monkeypatch, want_levels=False)
    assert ran_box
    assert_same_bits(full, box)
    assert (box["x_levels"] == 0.0).all() and (box["status"] == 0).all()
    withl = run_both(plan, asm, monkeypatch)[1]
    assert np.array_equal(withl["dq"], box["dq"]) and np.array_equal(withl["iterations"], box["iterations"])


def test_lean_body_at_the_default_eps(monkeypatch):
    """iHQP's default eps factor 2e2: J spans ten decades, the refinement and the accepted-slack rules come into play"""
    plan, leaf = synth.make_velocity_stack("C3", 16, seed=313, eps_factor=2e2)
    asm = pyoracle.assemble(plan, leaf)
    full, box, ran_box = run_both(plan, asm, monkeypatch)
    assert ran_box
    assert_same_bits(full, box)


def test_stuck_instances_fixture_is_not_a_box_only_plan(monkeypatch):
    """tests/golden/default_eps_stuck_instances.npz carries sixteen collision rows: it loads as a plan WITH constraint rows, so the
    BOX instantiation (and with it the lean path) does not take it (one instance, through both requests)"""
    plan, asm = default_eps_stuck_instances("tasks")
    assert plan.n == 32 and plan.nc > 0
    one = dict(asm, B=1, A=[None if a is None else a[:1] for a in asm["A"]], b=[a[:1] for a in asm["b"]], w=[a[:1] for a in asm["w"]],
               **{k: asm[k][:1] for k in ("C", "lo", "up", "l", "u")})
    full, box, ran_box = run_both(plan, one, monkeypatch)
    assert not ran_box
    assert_same_bits(full, box)


def rank_deficient_stack(B=6, box=0.5):
    """32 variables, levels of 6 and 20 generic rows and a Postural: the last row of each generic level is a combination of two others.
    Level 1 meets level 0's dependent row on the one-row path; the Postural level eliminates 26 rows of rank 24 (null-space path:
    two rows without a pivot, eight free columns)"""
    plan, leaf = synth.make_generic_stack(B, 32, [6, 20], seed=41, box=box)
    leaf["A"][0][:, 5] = leaf["A"][0][:, 0] + leaf["A"][0][:, 1]
    leaf["A"][1][:, 19] = leaf["A"][1][:, 2] - leaf["A"][1][:, 3]
    return plan, leaf


def test_lean_body_on_rank_deficient_levels(monkeypatch):
    plan, leaf = rank_deficient_stack()
    asm = pyoracle.assemble(plan, leaf)
    # the construction: level 0 has rank 5 of 6 rows, the 26 rows the Postural level sees have rank 24 -- eight free columns
    for i in range(asm["B"]):
        assert np.linalg.matrix_rank(asm["A"][0][i]) == 5
        assert np.linalg.matrix_rank(np.concatenate([asm["A"][0][i], asm["A"][1][i]])) == 24
    full, box, ran_box = run_both(plan, asm, monkeypatch)
    assert ran_box
    assert_same_bits(full, box)
    assert (box["status"] == 0).all()
    for k in (0, 1):   # the answer keeps the levels above: their optimality rows hold
        r = np.einsum("bmn,bn->bm", asm["A"][k], box["x_levels"][:, k] - box["dq"])
        assert np.abs(r).max() < 1e-7


def test_rank_deficient_levels_take_the_dependent_row_and_no_pivot_branches(monkeypatch):
    """the same stack under a box so wide that no bound is ever violated: the iteration count is then the count of the equality phase
    alone, and it says which branches ran.  Level 0 sees no rows: 0.  Level 1 walks level 0's six rows one by one and counts a row
    when it enters the working set: the dependent row does not, 5.  The Postural level counts all 26 rows it hands to the null-space
    elimination (iters += n_eq) -- and takes that route only if at most eight columns stay free, i.e. with rank 24 exactly: the two
    dependent rows found no pivot (row by row it would count the 24 that enter)."""
    plan, leaf = rank_deficient_stack(box=1.0e3)
    asm = pyoracle.assemble(plan, leaf)
    full, box, ran_box = run_both(plan, asm, monkeypatch)
    assert ran_box
    assert_same_bits(full, box)
    assert (box["status"] == 0).all()
    assert (box["iterations"] == 0 + 5 + 26).all()


def refused_plans():
    p31, l31 = synth.make_generic_stack(6, 31, [5, 9], seed=42)
    yield "n31", p31, pyoracle.assemble(p31, l31), None
    pc, lc = synth.make_velocity_stack("C3", 6, seed=314)
    ac = pyoracle.assemble(pc, lc)
    rng = np.random.default_rng(5)
    ac["c"] = [rng.normal(0.0, 0.01, size=(6, 32)) for _ in range(ac["L"])]
    yield "linear_term", pc, ac, None
    pr, lr = synth.add_regularisation(*synth.make_velocity_stack("C3", 6, seed=315))
    yield "regularisation", pr, pyoracle.assemble(pr, lr), None
    pi, li = synth.make_velocity_stack("C3", 6, seed=316)
    yield "inactive_level", pi, pyoracle.assemble(pi, li), [True, False, True]


@pytest.mark.parametrize("case", ["n31", "linear_term", "regularisation", "inactive_level"])
def test_plans_the_predicate_refuses_keep_the_general_bits(case, monkeypatch):
    """plans the BOX kernel takes but lean_plan refuses (n = 31; a linear term c; a regularisation task; an inactive level): the BOX
    kernel's answer is still the general instantiation's, bit for bit"""
    name, plan, asm, active = next(c for c in refused_plans() if c[0] == case)
    full, box, ran_box = run_both(plan, asm, monkeypatch, active=active)
    assert ran_box
    assert_same_bits(full, box)
    assert (box["status"] == 0).all()
