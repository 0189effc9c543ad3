"""velocity::ConvexHull on the device: the row kind OSOT_ROWS_CONVEX_HULL through osot_stack_update on both routes, whole solves of
the balance stack against its generic twin and the oracle, the fused paths (osot_cycle, osot_control_cycle, osot_control_rollout) on
the COMAN variant whose CoM, CoM Jacobian and contact points come from the kinematics producer, and the producer's contact points
-- against the numpy restatement of the reference in tests/hull_ref.py."""
import numpy as np
import pytest
import torch

from opensot_amd import abi, synth
from opensot_amd import kinematics as kin
from opensot_amd.solver import BatchedStack
from oracle import pyoracle

from hull_ref import INACTIVE_UP, LO, dyadic_batch, generic_twin, hull_block
from test_convex_hull_host import ATOL, general_position, hull_leaf, hull_plan
from test_wide_plan_host import _pick, _witnesses, close, oracle_solve

pytestmark = pytest.mark.gpu


def device_rows(plan, leaf):
    """osot_stack_update on the device (the route the plan's size picks) -> C, lo, up"""
    B = leaf["B"]
    st = BatchedStack(plan, B, device=0)
    assert st.route == ("wavefront" if plan.n <= abi.MAX_VARS else "wide")
    dev = st.load_leaf(leaf)
    st.C.fill_(7.0)
    st.update(dev)
    torch.cuda.synchronize()
    return st.C[:B].cpu().numpy(), st.lo[:B].cpu().numpy(), st.up[:B].cpu().numpy()


def check_rows(plan, leaf, exact=False):
    Cd, lo, up = device_rows(plan, leaf)
    Cw, lw, uw, act = hull_block(plan.rowblocks[0], *leaf["rows"][0], plan.n)
    np.testing.assert_array_equal(lo, lw)
    for i in range(leaf["B"]):
        a = act[i]
        if exact:
            np.testing.assert_array_equal(Cd[i], Cw[i]); np.testing.assert_array_equal(up[i], uw[i])
        np.testing.assert_allclose(Cd[i, :a], Cw[i, :a], rtol=0, atol=ATOL)
        np.testing.assert_allclose(up[i, :a], uw[i, :a], rtol=0, atol=ATOL)
        np.testing.assert_array_equal(Cd[i, a:], 0.0)                        # inactive rows: exact
        np.testing.assert_array_equal(up[i, a:], INACTIVE_UP)
    return act, Cd, up


# ---- 1. osot_stack_update ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", [(7, 3), (64, 8), (70, 16)])
def test_stack_update_hull_rows_gpu(n, P, gpu_device):
    B = 8
    rng = np.random.default_rng(100 * n + P)
    J, com, pts = general_position(rng, B, n, P)
    act, _, _ = check_rows(hull_plan(n, P, margin=0.01), hull_leaf(B, n, J, com, pts))
    assert ((act >= 3) & (act <= P)).all() and (P == 3 or (act < P).any())


@pytest.mark.parametrize("n", [7, 70])
def test_stack_update_degenerate_dyadic_batch_gpu(n, gpu_device):
    P = 8
    rng = np.random.default_rng(5)
    for margin, cases in dyadic_batch(P).items():
        B = len(cases)
        pts = np.stack([c[1] for c in cases]); com = np.stack([c[2] for c in cases])
        J = rng.integers(-64, 65, size=(B, 3, n)) / 32.0
        act, Cd, up = check_rows(hull_plan(n, P, margin), hull_leaf(B, n, J, com, pts), exact=True)
        assert list(act) == [c[3] for c in cases]


def test_lifted_foot_workaround_gpu(gpu_device):
    """contact sets that differ per instance: a lifted foot's points are replaced by copies of a stance point -- duplicates of a
    lower-indexed point are dropped, so the rows are those of the stance foot's polygon alone"""
    B = 4
    _, leaf, model = synth.make_coman_balance_stack(B, seed=2)
    n, q = model.n, leaf["state"]["q0"]
    pts = np.stack([model.points_world(q[i]) for i in range(B)])             # l_sole corners 0..3, r_sole corners 4..7
    rng = np.random.default_rng(9)
    com = pts.mean(axis=1) + rng.normal(0.0, 0.01, size=(B, 3))
    J = rng.uniform(-2.0, 2.0, size=(B, 3, n))
    one = pts.copy()
    one[:, 4:] = one[:, :1]                                                  # the right foot is in the air
    act8, C8, up8 = check_rows(hull_plan(n, 8, 0.01), hull_leaf(B, n, J, com, one))
    act4, C4, up4 = check_rows(hull_plan(n, 4, 0.01), hull_leaf(B, n, J, com, pts[:, :4]))
    assert (act8 == 4).all() and (act4 == 4).all()
    np.testing.assert_array_equal(C8[:, :4], C4); np.testing.assert_array_equal(up8[:, :4], up4)
    act2, _, _ = check_rows(hull_plan(n, 8, 0.01), hull_leaf(B, n, J, com, pts))
    assert (act2 >= 4).all() and (act2 <= 6).all()                           # both feet: the hull of two rectangles


# ---- 2. solve parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,P", [(16, 32, 8), (4, 70, 16)])
def test_balance_stack_solve_parity_gpu(B, n, P, gpu_device):
    from helpers import answer_is_acceptable
    plan, leaf = synth.make_balance_stack(B, seed=3, n=n, P=P)
    st = BatchedStack(plan, B, device=0)
    assert st.route == ("wavefront" if n <= abi.MAX_VARS else "wide")
    dev = st.load_leaf(leaf)
    st.update(dev)
    st.solve(B)
    torch.cuda.synchronize()
    assert (st.status[:B].cpu().numpy() == 0).all()
    dq = st.dq[:B].cpu().numpy()
    # the generic twin on the same device, through the same route
    twin, tleaf = generic_twin(plan, leaf)
    tw = BatchedStack(twin, B, device=0, route=st.route)
    tdev = tw.load_leaf(tleaf)
    tw.update(tdev)
    tw.solve(B)
    torch.cuda.synchronize()
    assert (tw.status[:B].cpu().numpy() == 0).all()
    dq_twin = tw.dq[:B].cpu().numpy()
    err = np.abs(dq - dq_twin).max()
    print(f"max|dq - dq_twin| = {err:.3e}")
    assert err <= 1e-9 * max(1.0, np.abs(dq_twin).max())
    # the twin against the oracle, under the suite's rule: the parity tolerance, or the lexicographic rule against the witnesses
    asm = pyoracle.assemble(twin, tleaf)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all()
    for i in range(B):
        if close(dq_twin[i], ref["dq"][i]):
            continue
        sub = _pick(asm, i)
        ok, why = answer_is_acceptable(sub, 0, dq_twin[i], [(nm, r["dq"][0], r["status"][0] == 1) for nm, r in _witnesses(sub)])
        assert ok, (i, why)
    # the CoM step stays inside the margin-shrunk polygon (up to what the solver accepted as round-off), and the polygon matters
    Cw, _, up, act = hull_block(plan.rowblocks[0], *leaf["rows"][0], n)
    res = np.einsum("bpn,bn->bp", Cw, dq) - up
    slack = st.accepted_slack[:B].cpu().numpy()
    print(f"max hull residual = {res.max():.3e}, accepted slack max = {slack.max():.3e}")
    assert (res.max(axis=1) <= slack + 1e-10).all()
    assert ((np.abs(res) <= 1e-9).sum(axis=1) >= 1).any(), "no hull row active at any solution"


# ---- 3. fused paths on the COMAN variant ----------------------------------------------------------------------------------------------
def coman(B, K=None):
    plan, leaf, model = synth.make_coman_balance_stack(B, seed=5)
    K = K or kin.Kinematics(model, device=0)
    st = BatchedStack(plan, B, device=0, want_levels=False)
    dev, kb, q = synth.bind_balance(st, K, leaf)
    kw = dict(com=dev["rows"][0][1], com_J=(st.A[0], 0), points=dev["rows"][0][2])
    return st, K, dev, kb, q, kw


def test_fused_paths_bit_identical_on_coman_gpu(gpu_device):
    B, steps = 4, 3
    sa, K, da, _, qa, kwa = coman(B)                 # three calls: kinematics, update, solve
    sb, _, db, _, qb, kwb = coman(B, K)              # kinematics + osot_cycle
    sc, _, dc, kbc, qc, _ = coman(B, K)              # osot_control_cycle
    sd, _, dd, kbd, qd, _ = coman(B, K)              # osot_control_rollout
    dq_steps = torch.zeros((steps, B, sa.plan.n), dtype=torch.float64, device=sa.device)
    st_steps = torch.full((steps, B), -1, dtype=torch.int32, device=sa.device)
    sd.control_rollout(K, kbd, dd, qd, steps, dq_steps=dq_steps, status_steps=st_steps)
    ups, Cs = [], []
    for t in range(steps):
        K.forward(qa, **kwa); sa.update(da); sa.solve(B); qa += sa.dq[:B]
        K.forward(qb, **kwb); sb.cycle(db); qb += sb.dq[:B]
        sc.control_cycle(K, kbc, dc, q_integrate=qc)
        torch.cuda.synchronize()
        for s in (sa, sb, sc):
            assert (s.status[:B] == 0).all()
        assert torch.equal(sa.dq[:B], sb.dq[:B]), f"osot_cycle differs from update + solve at step {t}"
        assert torch.equal(sa.dq[:B], sc.dq[:B]), f"osot_control_cycle differs from kinematics + update + solve at step {t}"
        assert torch.equal(sa.C[:B], sb.C[:B]) and torch.equal(sa.C[:B], sc.C[:B])
        assert torch.equal(sa.up[:B], sb.up[:B]) and torch.equal(sa.up[:B], sc.up[:B])
        assert torch.equal(qa, qb) and torch.equal(qa, qc)
        assert torch.equal(dq_steps[t], sc.dq[:B]), f"osot_control_rollout differs from the control cycles at step {t}"
        ups.append(sc.up[:B].clone()); Cs.append(sc.C[:B].clone())
    assert (st_steps == 0).all() and torch.equal(qd, qc) and torch.equal(sd.up[:B], sc.up[:B]) and torch.equal(sd.C[:B], sc.C[:B])
    # the polygon follows the posture: the rows of step 3 are not those of step 1
    assert not torch.equal(ups[0], ups[2]) and not torch.equal(Cs[0], Cs[2])
    assert float((ups[0] - ups[2]).abs().max()) > 1e-6
    # and the rows are the reference's for the posture the last cycle saw
    Cw, lo, up, act = hull_block(sa.plan.rowblocks[0], sa.A[0][:B].cpu().numpy(), da["rows"][0][1].cpu().numpy(), da["rows"][0][2].cpu().numpy(), sa.plan.n)
    assert ((act >= 4) & (act <= 6)).all()
    np.testing.assert_allclose(sa.C[:B].cpu().numpy(), Cw, rtol=0, atol=ATOL)
    np.testing.assert_allclose(sa.up[:B].cpu().numpy()[up < INACTIVE_UP], up[up < INACTIVE_UP], rtol=0, atol=ATOL)
    assert (sa.lo[:B].cpu().numpy() == LO).all()
    res = torch.einsum("bpn,bn->bp", sa.C[:B], sa.dq[:B]) - sa.up[:B]
    print(f"COMAN: hull rows active at the last step: {int((res.abs() <= 1e-9).sum())}, max residual {float(res.max()):.3e}")
    assert float(res.max()) <= float(sa.accepted_slack[:B].max()) + 1e-10


# ---- 4. the producer's contact points -----------------------------------------------------------------------------------------------
def test_kinematics_points_gpu(gpu_device):
    B = 4
    _, leaf, model = synth.make_coman_balance_stack(B, seed=2)
    q = leaf["state"]["q0"] + np.random.default_rng(4).normal(0.0, 0.3, size=(B, model.n))
    K = kin.Kinematics(model, device=0)
    f64 = dict(dtype=torch.float64, device="cuda:0")
    tq = torch.as_tensor(q, **f64).contiguous()
    pts = torch.full((B + 1, 8, 3), 7.0, **f64)
    com = torch.zeros((B, 3), **f64)
    K.forward(tq, com=com, points=pts)
    torch.cuda.synchronize()
    ref = np.stack([model.points_world(q[i]) for i in range(B)])
    np.testing.assert_allclose(pts[:B].cpu().numpy(), ref, rtol=0, atol=1e-12)
    assert (pts[B] == 7.0).all()
    com2 = torch.zeros((B, 3), **f64)
    K.forward(tq, com=com2)                           # points = NULL: the other outputs are what they were
    torch.cuda.synchronize()
    assert torch.equal(com, com2)
