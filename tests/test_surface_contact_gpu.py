"""Surface contacts on the device: the row kinds OSOT_ROWS_WRENCH_FRICTION_CONE / COP / NORMAL_TORQUE through osot_stack_update on both
routes, and the whole inverse-dynamics control step with 6-D wrenches -- osot_id_rows, update + cascade (osot_cycle), osot_computed_torque
-- at n = 56 (wavefront route) and 68 / 86 / 128 (wide route), against numpy and the oracle on the generic twin
(tests/surface_ref.py)."""
import numpy as np
import pytest
import torch

from opensot_amd import synth
from opensot_amd.dynamics import IdModel, force_gains
from opensot_amd.solver import BatchedStack
from oracle import pyoracle

from surface_ref import SURFACE_KINDS, generic_twin, surface_block, torque
from test_wide_plan_host import _pick, _witnesses, close, oracle_solve

pytestmark = pytest.mark.gpu

SIZES = {56: (32, 4), 68: (44, 4), 86: (56, 5), 128: (80, 8)}


def stack(B, n, seed):
    nv, nc = SIZES[n]
    return synth.make_surface_id_stack(B, seed=seed, nv=nv, n_contacts=nc)


@pytest.mark.parametrize("n,route", [(56, "wavefront"), (56, "wide"), (86, "wide")])
def test_stack_update_surface_rows_gpu(n, route, gpu_device):
    B = 32
    plan, leaf = stack(B, n, seed=n)
    st = BatchedStack(plan, B, device=0, route=route)
    dev = st.load_leaf(leaf)
    st.C.fill_(7.0)
    st.update(dev)
    torch.cuda.synchronize()
    Cd, lo, up = st.C[:B].cpu().numpy(), st.lo[:B].cpu().numpy(), st.up[:B].cpu().numpy()
    for j, rb in enumerate(plan.rowblocks):
        if rb.kind not in SURFACE_KINDS:
            continue
        p0, p1, _ = leaf["rows"][j]
        Cw, lw, uw = surface_block(rb, p0, p1, n)
        o, r0 = plan.rows_stored_offset(j), plan.rows_offset(j)
        np.testing.assert_allclose(Cd[:, o:o + rb.rows], Cw, rtol=0, atol=1e-13)
        np.testing.assert_array_equal(lo[:, r0:r0 + rb.rows], lw)
        np.testing.assert_array_equal(up[:, r0:r0 + rb.rows], uw)


def _twin_device(plan, leaf, route):
    twin, tleaf = generic_twin(plan, leaf)
    B = leaf["B"]
    st = BatchedStack(twin, B, device=0, route=route)
    dev = st.load_leaf(tleaf)
    st.update(dev)
    st.solve(B)
    torch.cuda.synchronize()
    assert (st.status[:B].cpu().numpy() == 0).all()
    return twin, tleaf, st.dq[:B].cpu().numpy()


@pytest.mark.parametrize("n", [56, 68, 86, 128])
def test_surface_id_control_step_gpu(n, gpu_device):
    """osot_id_rows -> osot_cycle -> osot_computed_torque, everything model-derived written on the device"""
    from helpers import answer_is_acceptable
    B = 32
    plan, leaf = stack(B, n, seed=100 + n)
    nv = leaf["model"]["nv"]
    st = BatchedStack(plan, B, device=0)
    assert st.route == ("wavefront" if n <= 64 else "wide")
    bare = dict(leaf); bare["A"] = [np.zeros_like(leaf["A"][0]), None]; bare["C"] = [None] * len(plan.rowblocks)
    dev = st.load_leaf(bare)
    md = IdModel(leaf["model"]["B"], leaf["model"]["h"], leaf["model"]["Jc"], device=0)
    assert md.cdim == 6 and md.n == n
    J = [torch.as_tensor(np.ascontiguousarray(leaf["A"][0][:, o:o + r, :nv])).to(st.device) for o, r in ((0, 3), (3, 6), (9, 6))]
    md.write_rows(st, dyn_block=0, tau_block=4, tasks=[(0, 0, J[0]), (0, 3, J[1]), (0, 9, J[2])])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(st.A[0][:B].cpu().numpy(), leaf["A"][0])
    o_dyn, o_tau = plan.rows_stored_offset(0), plan.rows_stored_offset(4)
    np.testing.assert_array_equal(st.C[:B, o_dyn:o_dyn + 6].cpu().numpy(), leaf["C"][0])
    np.testing.assert_array_equal(st.C[:B, o_tau:o_tau + nv].cpu().numpy(), leaf["C"][4])
    st.cycle(dev)
    tau_d, ok_d = md.computed_torque(st.dq[:B])
    torch.cuda.synchronize()
    assert (st.status[:B].cpu().numpy() == 0).all()
    x = st.dq[:B].cpu().numpy()
    tau = tau_d.cpu().numpy()
    np.testing.assert_allclose(tau, torque(leaf, x), rtol=0, atol=1e-10)
    assert (ok_d.cpu().numpy() == 1).all() and np.abs(tau[:, :6]).max() < 1e-8
    assert np.abs(tau[:, 6:]).max() <= 30.0 + 1e-8
    # the generic twin: solved on the device through the same route, and by the oracle
    twin, tleaf, x_twin = _twin_device(plan, leaf, st.route)
    assert np.abs(x - x_twin).max() <= 1e-9 * max(1.0, np.abs(x_twin).max())
    asm = pyoracle.assemble(twin, tleaf)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all()
    for i in range(B):
        if close(x[i], ref["dq"][i]):
            continue
        sub = _pick(asm, i)
        ok, why = answer_is_acceptable(sub, 0, x[i], [(nm, r["dq"][0], r["status"][0] == 1) for nm, r in _witnesses(sub)])
        assert ok, (i, why)


def test_wide_cycle_with_surface_rows_graph_replay(gpu_device):
    B = 64
    plan, leaf = stack(B, 86, seed=7)
    st = BatchedStack(plan, B, device=0)
    assert st.route == "wide"
    dev = st.load_leaf(leaf)
    st.cycle(dev)
    torch.cuda.synchronize()
    dq0 = st.dq.clone()
    assert (st.status[:B] == 0).all()
    s = torch.cuda.Stream()
    st.stream = s
    with torch.cuda.stream(s):
        st.cycle(dev)
    torch.cuda.synchronize()
    assert torch.equal(dq0, st.dq)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        st.cycle(dev)
    st.dq.zero_()
    o, r = plan.rows_stored_offset(1), sum(rb.rows for rb in plan.rowblocks if rb.kind in SURFACE_KINDS)
    st.C[:, o:o + r].zero_()          # the surface rows: rewritten by the update inside the graph
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(dq0, st.dq)


@pytest.mark.parametrize("nv", [100, 128])
def test_force_gains_beyond_64_joints_gpu(nv, gpu_device):
    B, rows = 32, 6
    rng = np.random.default_rng(nv)
    J = rng.normal(0.0, 0.3, size=(B, rows, nv))
    Lm = rng.normal(0.0, 0.3, size=(B, nv, nv))
    Bi = np.linalg.inv(Lm @ np.transpose(Lm, (0, 2, 1)) + np.eye(nv))
    Bi = (Bi + np.transpose(Bi, (0, 2, 1))) / 2
    Kp, Kd = np.diag(rng.uniform(1, 10, rows)), np.diag(rng.uniform(1, 5, rows))
    f = rng.normal(size=(B, rows))
    f64 = dict(dtype=torch.float64, device="cuda:0")
    p0 = torch.zeros((B, 2 * rows + 2 * rows * rows), **f64)
    a_ref = torch.zeros((B, rows), **f64)
    force_gains(torch.as_tensor(J, **f64).contiguous(), torch.as_tensor(Bi, **f64).contiguous(), Kp, Kd, p0, rows,
                f_virtual=torch.as_tensor(f, **f64).contiguous(), a_ref=a_ref)
    torch.cuda.synchronize()
    Mi = J @ Bi @ np.transpose(J, (0, 2, 1))
    G = p0[:, 2 * rows:].cpu().numpy()
    np.testing.assert_allclose(G[:, :rows * rows].reshape(B, rows, rows), Mi @ Kp, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(G[:, rows * rows:].reshape(B, rows, rows), Mi @ Kd, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a_ref.cpu().numpy(), np.einsum("brs,bs->br", Mi, f), rtol=1e-12, atol=1e-12)
