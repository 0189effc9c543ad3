"""The synth force stacks (synth.make_coman_force_stack, make_wide_force_stack) on the host: every force block assembled by the numpy
restatement of tests/force_ref.py, and the oracle's cascade ALONE solves every instance the GPU tests use -- so no instance needs
excusing there.  No GPU needed."""
import numpy as np
import pytest

from opensot_amd import abi, synth
from oracle import pyoracle

import force_ref as fr
from surface_ref import generic_twin
from test_wide_plan_host import oracle_solve

# (name, maker, B): the inputs of the stack-parity tests of tests/test_force_rows_gpu.py
STACKS = [("coman_com", lambda B: synth.make_coman_force_stack(B, "com"), 32),
          ("coman_static", lambda B: synth.make_coman_force_stack(B, "static"), 32),
          ("wide_static", lambda B: synth.make_wide_force_stack(B), 8)]


@pytest.fixture(scope="module", params=STACKS, ids=[s[0] for s in STACKS])
def solved(request):
    name, make, B = request.param
    plan, leaf, model = make(B)
    full, case = fr.assemble_stack(plan, leaf, model)
    twin, tleaf = generic_twin(plan, full)
    asm = pyoracle.assemble(twin, tleaf)
    return name, plan, full, case, asm, oracle_solve(asm)


def test_shapes(solved):
    name, plan, leaf, case, asm, ref = solved
    assert plan.n == {"coman_com": 12, "coman_static": 41, "wide_static": 106}[name]
    assert all(t.kind == abi.TASK_GENERIC for lev in plan.levels for t in lev)
    assert all(rb.kind in (abi.ROWS_GENERIC, abi.ROWS_UNIT_GENERIC, abi.ROWS_WRENCH_FRICTION_CONE, abi.ROWS_COP) for rb in plan.rowblocks)


def test_the_oracle_alone_solves_every_instance(solved):
    name, plan, leaf, case, asm, ref = solved
    assert (ref["status"] == 1).all(), ref["status"]


def test_the_solution_is_a_wrench_distribution(solved):
    """level 0 is met (the residual of force::CoM / force::FloatingBase is round-off of the QP), the static equalities hold, and the
    wrenches are inside their cones and CoP rectangles"""
    name, plan, leaf, case, asm, ref = solved
    x = ref["dq"]
    r0 = np.einsum("brn,bn->br", asm["A"][0], x) - asm["b"][0]
    assert np.abs(r0).max() <= 1e-6 * max(1.0, np.abs(asm["b"][0]).max()), np.abs(r0).max()
    Cx = np.einsum("brn,bn->br", asm["C"], x)
    assert (Cx >= asm["lo"] - 1e-6).all() and (Cx <= asm["up"] + 1e-6).all()
    assert (x[:, 2:6 * case["C"]:6] > 1.0).all()     # every sole pushes
