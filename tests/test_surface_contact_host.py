"""Surface contacts, CPU side: the row kinds OSOT_ROWS_WRENCH_FRICTION_CONE / COP / NORMAL_TORQUE (force::FrictionCone on a wrench,
force::CoP, force::NormalTorque) through both validators and the update kernel, the inverse-dynamics producers beyond 64 variables
(contact_dim = 6), and whole solves of surface inverse-dynamics stacks on both routes' host builds against the oracle on the generic
twin (tests/surface_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from opensot_amd import abi, synth
from opensot_amd.solver import stored_rows
from oracle import pyoracle

from helpers import emu_cascade, emu_lib
from surface_ref import SURFACE_KINDS, generic_twin, host_update, id_model, surface_block, surface_lib, torque
from test_wide_plan_host import _pick, _witnesses, close, oracle_solve, wide_host

SIZES = {56: (32, 4), 68: (44, 4), 86: (56, 5), 128: (80, 8)}


def stack(B, n, seed):
    nv, nc = SIZES[n]
    return synth.make_surface_id_stack(B, seed=seed, nv=nv, n_contacts=nc)


def _validate(fn, pd):
    return getattr(abi.lib(), fn)(C.byref(pd))


# ---- validators ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fn", [(56, "osot_plan_validate"), (56, "osot_plan_validate_wide"), (68, "osot_plan_validate_wide"),
                                  (128, "osot_plan_validate_wide")])
def test_validators_accept_surface_kinds(n, fn):
    plan, _ = stack(2, n, seed=1)
    assert {rb.kind for rb in plan.rowblocks} >= set(SURFACE_KINDS)
    assert _validate(fn, plan.to_c()) == abi.OK, abi.lib().osot_last_error()


@pytest.mark.parametrize("fn,n", [("osot_plan_validate", 56), ("osot_plan_validate_wide", 86)])
@pytest.mark.parametrize("kind", sorted(SURFACE_KINDS))
def test_validators_refuse_bad_surface_blocks(fn, n, kind):
    plan, _ = stack(2, n, seed=1)
    j = [rb.kind for rb in plan.rowblocks].index(kind)
    per, nc = SURFACE_KINDS[kind], SIZES[n][1]
    for rows, first_col in ((per * nc + 1, plan.n - 6 * nc),      # not a multiple of the rows per contact
                            (per * nc, plan.n - 6 * nc + 1),      # the last wrench ends beyond x
                            (per * (nc + 1), plan.n - 6 * nc),    # one contact too many
                            (per * nc, -1)):                      # before the first column
        pd = plan.to_c()
        pd.rowblock[j].rows, pd.rowblock[j].first_col = rows, first_col
        assert _validate(fn, pd) == abi.ERR_INVALID, (rows, first_col)
        assert b"6 wrench columns per contact" in abi.lib().osot_last_error()
    pd = plan.to_c()
    pd.rowblock[j].kind = abi.ROWS_NORMAL_TORQUE + 1
    assert _validate(fn, pd) == abi.ERR_UNSUPPORTED and b"unknown row-block kind" in abi.lib().osot_last_error()


@pytest.mark.parametrize("kind", [abi.ROWS_COP, abi.ROWS_NORMAL_TORQUE])
def test_update_refuses_missing_foot_limits(kind):
    plan, leaf = stack(2, 56, seed=2)
    j = [rb.kind for rb in plan.rowblocks].index(kind)
    leaf["rows"][j] = (leaf["rows"][j][0], None, None)
    rc, _ = host_update(emu_lib().emu_stack_update, plan, leaf)
    assert rc == abi.ERR_INVALID
    rc, _ = host_update(surface_lib().surf_stack_update, plan, leaf, 1)
    assert rc == abi.ERR_INVALID
    # the friction cone on wrenches needs no p1
    plan, leaf = stack(2, 56, seed=2)
    j = [rb.kind for rb in plan.rowblocks].index(abi.ROWS_WRENCH_FRICTION_CONE)
    assert leaf["rows"][j][1] is None
    assert host_update(emu_lib().emu_stack_update, plan, leaf)[0] == abi.OK


# ---- the update kernel against numpy ------------------------------------------------------------------------------------------
def _check_surface_rows(plan, leaf, res):
    """the stored rows and bounds of every surface block in res (update output) against the numpy restatement"""
    seen = 0
    for j, rb in enumerate(plan.rowblocks):
        if rb.kind not in SURFACE_KINDS:
            continue
        p0, p1, _ = leaf["rows"][j]
        Cw, lo, up = surface_block(rb, p0, p1, plan.n)
        o, r0 = plan.rows_stored_offset(j), plan.rows_offset(j)
        np.testing.assert_allclose(res["C"][:, o:o + rb.rows], Cw, rtol=0, atol=1e-13)
        np.testing.assert_array_equal(res["lo"][:, r0:r0 + rb.rows], lo)
        np.testing.assert_array_equal(res["up"][:, r0:r0 + rb.rows], up)
        seen += 1
    assert seen == 3


def test_update_writes_surface_rows_wavefront_build():
    B = 5
    plan, leaf = stack(B, 56, seed=3)
    rc, res = host_update(emu_lib().emu_stack_update, plan, leaf)
    assert rc == abi.OK
    _check_surface_rows(plan, leaf, res)
    # everything else as the oracle assembles the generic twin
    twin, tleaf = generic_twin(plan, leaf)
    asm = pyoracle.assemble(twin, tleaf)
    np.testing.assert_allclose(res["C"], stored_rows(plan, asm["C"]), rtol=0, atol=1e-13)
    np.testing.assert_allclose(res["lo"], asm["lo"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["up"], asm["up"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("n", [68, 86, 128])
def test_wide_update_and_id_producers(n):
    """osot_update_kernel under the wide validator, osot_id_rows_kernel, osot_torque_kernel at nv + 6 contacts > 64"""
    B = 3
    plan, leaf = stack(B, n, seed=n)
    nv = leaf["model"]["nv"]
    L = surface_lib()
    assert host_update(L.surf_stack_update, plan, leaf, 0)[0] == abi.ERR_INVALID     # the wavefront route keeps n <= 64
    bare = dict(leaf); bare["C"] = [None] * len(plan.rowblocks)
    rc, res = host_update(L.surf_stack_update, plan, bare, 1)
    assert rc == abi.OK
    _check_surface_rows(plan, leaf, res)
    # the producer writes [B_u, -J_f'], [B, -Jc'] into C and the [J 0] rows into A_0
    keep = []
    m = id_model(leaf, keep)
    vp = C.c_void_p
    Cst = res["C"]
    A0 = np.full((B, plan.ma(0), n), 7.0)
    Js = [np.ascontiguousarray(leaf["A"][0][:, o:o + r, :nv]) for o, r in ((0, 3), (3, 6), (9, 6))]
    Jp = (vp * 3)(*[j.ctypes.data for j in Js]); Jr = (C.c_int * 3)(3, 6, 6)
    Ad = (vp * 3)(*[A0.ctypes.data + 8 * o * n for o in (0, 3, 9)]); As = (C.c_longlong * 3)(*[plan.ma(0) * n] * 3)
    o_dyn, o_tau = plan.rows_stored_offset(0), plan.rows_stored_offset(4)
    assert L.surf_id_rows(C.byref(m), Cst.ctypes.data + 8 * o_dyn * n, plan.nc_stored * n, Cst.ctypes.data + 8 * o_tau * n,
                          plan.nc_stored * n, 3, Jp, Jr, Ad, As) == 0
    np.testing.assert_array_equal(Cst[:, o_dyn:o_dyn + 6], leaf["C"][0])
    np.testing.assert_array_equal(Cst[:, o_tau:o_tau + nv], leaf["C"][4])
    np.testing.assert_array_equal(A0, leaf["A"][0])
    # tau with contact_dim = 6 at the nominal point and at a random x
    for x in (leaf["nominal"], np.random.default_rng(n).normal(0.0, 5.0, size=(B, n))):
        x = np.ascontiguousarray(x)
        tau = np.zeros((B, nv)); ok = np.full(B, -1, dtype=np.int32)
        assert L.surf_computed_torque(C.byref(m), x.ctypes.data, tau.ctypes.data, ok.ctypes.data, 1e-2) == 0
        np.testing.assert_allclose(tau, torque(leaf, x), rtol=0, atol=1e-10)
        np.testing.assert_allclose(tau, synth.computed_torque(leaf, x), rtol=0, atol=1e-10)
        assert (ok == (np.abs(tau[:, :6]).max(axis=1) <= 1e-2)).all()
    assert np.abs(torque(leaf, leaf["nominal"])[:, :6]).max() < 1e-10


def test_id_producers_take_up_to_128_variables():
    """osot_id_rows / osot_computed_torque: nv + forces <= 128 and forces <= 48 (the size checks run before any launch: B = 0)"""
    plan, leaf = stack(1, 128, seed=1)
    keep = []
    m = id_model(leaf, keep, B=0)
    L = abi.lib()
    x = np.zeros((1, 129)); tau = np.zeros((1, 81))
    assert L.osot_computed_torque(C.byref(m), x.ctypes.data, tau.ctypes.data, None, 1e-2, None) == abi.OK   # 80 + 8 x 6
    m.nv = 81                                   # 129 variables
    assert L.osot_computed_torque(C.byref(m), x.ctypes.data, tau.ctypes.data, None, 1e-2, None) == abi.ERR_UNSUPPORTED
    assert L.osot_id_rows(C.byref(m), None, 0, None, 0, 0, None, None, None, None, None) == abi.ERR_UNSUPPORTED
    m.nv, m.n_contacts = 40, 9                  # 54 force variables
    assert L.osot_computed_torque(C.byref(m), x.ctypes.data, tau.ctypes.data, None, 1e-2, None) == abi.ERR_UNSUPPORTED
    assert abi.ID_MAX_FORCE_VARS == 48
    Kp = np.eye(6)
    dp = Kp.ctypes.data_as(abi.dp)
    assert L.osot_id_force_gains(0, 128, 6, None, None, dp, dp, None, None, 0, None, None) == abi.OK
    assert L.osot_id_force_gains(0, 129, 6, None, None, dp, dp, None, None, 0, None, None) == abi.ERR_INVALID


@pytest.mark.parametrize("nv", [40, 100, 128])
def test_force_gains_beyond_64_joints(nv):
    B, rows = 3, 6
    rng = np.random.default_rng(nv)
    J = rng.normal(0.0, 0.3, size=(B, rows, nv))
    Lm = rng.normal(0.0, 0.3, size=(B, nv, nv))
    Bi = np.linalg.inv(Lm @ np.transpose(Lm, (0, 2, 1)) + np.eye(nv))
    Bi = np.ascontiguousarray((Bi + np.transpose(Bi, (0, 2, 1))) / 2)
    Kp, Kd = np.diag(rng.uniform(1, 10, rows)), np.diag(rng.uniform(1, 5, rows))
    f = rng.normal(size=(B, rows))
    G = np.zeros((B, 2 * rows * rows)); a_ref = rng.normal(size=(B, rows)); a0 = a_ref.copy()
    assert surface_lib().surf_force_gains(B, nv, rows, J.ctypes.data, Bi.ctypes.data, Kp.ctypes.data, Kd.ctypes.data, f.ctypes.data,
                                          G.ctypes.data, 2 * rows * rows, a_ref.ctypes.data) == 0
    Mi = J @ Bi @ np.transpose(J, (0, 2, 1))
    np.testing.assert_allclose(G[:, :rows * rows].reshape(B, rows, rows), Mi @ Kp, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(G[:, rows * rows:].reshape(B, rows, rows), Mi @ Kd, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a_ref, a0 + np.einsum("brs,bs->br", Mi, f), rtol=1e-12, atol=1e-12)


# ---- whole solves on the host against the oracle on the generic twin -----------------------------------------------------------
def _judge(asm, dq, st):
    """SOLVED, and every instance within the parity tolerance of the oracle -- or, where it is not, acceptable to the lexicographic
    rule against the witnesses (helpers.answer_is_acceptable)"""
    from helpers import answer_is_acceptable
    assert (st == 0).all()
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all()
    for i in range(asm["B"]):
        if close(dq[i], ref["dq"][i]):
            continue
        sub = _pick(asm, i)
        ok, why = answer_is_acceptable(sub, 0, dq[i], [(nm, r["dq"][0], r["status"][0] == 1) for nm, r in _witnesses(sub)])
        assert ok, (i, why)


def _assembled(plan, leaf):
    """the oracle's assembly of the generic twin, checked against what the update kernel writes for the surface plan itself"""
    twin, tleaf = generic_twin(plan, leaf)
    asm = pyoracle.assemble(twin, tleaf)
    rc, res = host_update(surface_lib().surf_stack_update, plan, leaf, 1)
    assert rc == abi.OK
    np.testing.assert_allclose(res["C"], stored_rows(plan, asm["C"]), rtol=0, atol=1e-13)
    np.testing.assert_allclose(res["lo"], asm["lo"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["up"], asm["up"], rtol=0, atol=1e-12)
    for k in range(plan.L):
        np.testing.assert_allclose(res["b"][k], asm["b"][k], rtol=0, atol=1e-12)
    return asm


def test_surface_id_solve_wavefront_build():
    B = 4
    plan, leaf = stack(B, 56, seed=11)
    asm = _assembled(plan, leaf)
    dq, _, st, _ = emu_cascade(plan, asm)   # the surface plan itself: its blocks are stored rows to the cascade
    _judge(asm, dq, st)
    tau = torque(leaf, dq)
    assert np.abs(tau[:, :6]).max() < 1e-8 and np.abs(tau[:, 6:]).max() <= 30.0 + 1e-8


@pytest.mark.parametrize("n", [68, 86])
def test_surface_id_solve_wide_build(n):
    B = 3
    plan, leaf = stack(B, n, seed=n + 1)
    asm = _assembled(plan, leaf)
    dq, _, st, _, slack = wide_host(plan, asm)
    _judge(asm, dq, st)
    assert (slack <= 1e-7).all()
    tau = torque(leaf, dq)
    assert np.abs(tau[:, :6]).max() < 1e-8 and np.abs(tau[:, 6:]).max() <= 30.0 + 1e-8
