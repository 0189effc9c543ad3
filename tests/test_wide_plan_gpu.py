"""Batched iHQP plans of 65 .. 128 variables on the GPU: osot_solver_create_wide + osot_ihqp_solve / osot_stack_update / osot_cycle
(one 256-thread workgroup per instance, opensot_amd/csrc/osot_cascade_wide.h) against the oracle, the host build of the same source
(tests/test_wide_plan_host.py), the wavefront route, and the reference's qpOASES answers in tests/golden/wide_id_levels.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

from opensot_amd import abi, synth
from opensot_amd.solver import BatchedStack
from oracle import pyoracle
from test_wide_plan_host import close, generic_wide, golden_plan, oracle_solve, wide_host

pytestmark = pytest.mark.gpu


def _solve(plan, asm, route="wide", active=None, task_active=None):
    B = asm["B"]
    st = BatchedStack(plan, B, device=0, route=route)
    st.load_assembled(asm)
    for (k, j), on in (task_active or {}).items():
        st.set_task_active(k, j, on)
    st.level_active = active
    st.solve(B)
    torch.cuda.synchronize()
    return (st.dq[:B].cpu().numpy(), st.x_levels[:B].cpu().numpy(), st.status[:B].cpu().numpy(),
            st.iterations[:B].cpu().numpy(), st.accepted_slack[:B].cpu().numpy())


@pytest.mark.parametrize("n", [65, 80, 100, 128])
def test_wide_route_matches_oracle_and_host_build(n, gpu_device):
    B = 16
    plan, leaf = generic_wide(B, n, seed=n)
    asm = pyoracle.assemble(plan, leaf)
    dq, xl, st, it, slack = _solve(plan, asm)
    ref = oracle_solve(asm)
    assert (st == 0).all() and (ref["status"] == 1).all()
    assert close(dq, ref["dq"]) and close(xl, ref["x_levels"])
    assert (slack >= 0).all() and (slack <= 1e-5).all()
    h = wide_host(plan, asm)
    assert np.abs(dq - h[0]).max() <= 1e-9 * max(1.0, np.abs(h[0]).max())
    assert np.array_equal(it, h[3]) and np.array_equal(st, h[2])


def test_wide_route_inactive_level_and_task(gpu_device):
    B, n = 8, 100
    plan, leaf = synth.make_generic_stack(B, n, [10, 8, 14], n_ineq=20, unit_box=(None, 0.6), seed=3 * n)
    plan.levels[1].append(synth.Task(abi.TASK_GENERIC, 5, name="extra"))
    leaf["A"][1] = np.concatenate([leaf["A"][1], np.random.default_rng(1).normal(0, 0.4, size=(B, 5, n))], axis=1)
    leaf["task"][1].append((np.random.default_rng(2).normal(0, 0.05, size=(B, 5)), None, None))
    ta = {(1, 1): False}
    asm = pyoracle.assemble(plan, leaf, task_active=ta)
    act = [True, False, True, True]
    dq, xl, st, _, _ = _solve(plan, asm, active=act, task_active=ta)
    ref = oracle_solve(asm, active=act)
    assert (st == 0).all() and close(dq, ref["dq"])
    for k in (0, 2, 3):
        assert close(xl[:, k], ref["x_levels"][:, k])


def test_wide_route_grid_loops_over_the_batch(gpu_device):
    """B = 2048 at n = 96: more instances than the grid holds -- every workgroup solves several, each one equal to the host build"""
    B = 2048
    plan, leaf = synth.make_wide_robot_stack(B, 96, levels=3, seed=9)
    asm = pyoracle.assemble(plan, leaf)
    stk = BatchedStack(plan, B, device=0)
    assert stk.route == "wide" and stk.resident_waves() < B
    stk.load_assembled(asm)
    stk.solve(B)
    torch.cuda.synchronize()
    dq, it = stk.dq.cpu().numpy(), stk.iterations.cpu().numpy()
    assert (stk.status.cpu().numpy() == 0).all()
    h = wide_host(plan, asm)
    assert np.abs(dq - h[0]).max() <= 1e-9 * max(1.0, np.abs(h[0]).max())
    assert np.array_equal(it, h[3])


@pytest.mark.parametrize("case", ["C3", "generic48"])
def test_cross_route_wide_equals_wavefront(case, gpu_device):
    B = 256
    if case == "C3":
        plan, leaf = synth.make_velocity_stack("C3", B, seed=17)
    else:
        plan, leaf = generic_wide(B, 48, seed=48)
    asm = pyoracle.assemble(plan, leaf)
    w = _solve(plan, asm, route="wide")
    f = _solve(plan, asm, route="wavefront")
    assert np.array_equal(w[2], f[2]) and (w[2] == 0).all()
    rel = np.abs(w[0] - f[0]).max(axis=1) / np.maximum(1.0, np.abs(f[0]).max(axis=1))
    beyond = np.nonzero(rel > 1e-9)[0]
    # (an instance at a degenerate vertex may differ by more: the lexicographic judge of the stress sweeps decides, oracle/lexcheck.py)
    if len(beyond):
        from helpers import answer_is_acceptable
        ref = oracle_solve(asm)
        for i in beyond:
            ok, why = answer_is_acceptable(asm, i, w[0][i], [("oracle", ref["dq"][i], ref["status"][i] == 1), ("wavefront", f[0][i], True)])
            assert ok, f"instance {i}: {why}"
    print(f"{case}: {len(beyond)} of {B} instances beyond 1e-9 judged by the lexicographic rule")


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_wide_route_golden_id_levels(c, gpu_device):
    plan, asm, x0, x1 = golden_plan(c)
    dq, xl, st, _, _ = _solve(plan, asm)
    assert st[0] == 0
    assert np.abs(xl[0, 0] - x0).max() < 1e-6 and np.abs(dq[0] - x1).max() < 1e-6


def test_wide_update_matches_oracle_assembly(gpu_device):
    plan, leaf = synth.make_wide_robot_stack(32, 100, levels=3, seed=5)
    asm = pyoracle.assemble(plan, leaf)
    st = BatchedStack(plan, 32, device=0)
    st.update(st.load_leaf(leaf))
    torch.cuda.synchronize()
    for k in range(plan.L):   # (b as in test_update_kernel_matches_oracle_assembly: the device's fma against numpy's rounding)
        np.testing.assert_allclose(st.b[k].cpu().numpy(), asm["b"][k], rtol=0, atol=1e-15)
        np.testing.assert_array_equal(st.w[k].cpu().numpy(), asm["w"][k])
    np.testing.assert_array_equal(st.l.cpu().numpy(), asm["l"])
    np.testing.assert_array_equal(st.u.cpu().numpy(), asm["u"])
    np.testing.assert_array_equal(st.C.cpu().numpy(), asm["C"])
    np.testing.assert_array_equal(st.lo.cpu().numpy(), asm["lo"])
    np.testing.assert_array_equal(st.up.cpu().numpy(), asm["up"])


def test_wide_cycle_equals_update_and_solve_and_graph_replay(gpu_device):
    B = 512
    plan, leaf = synth.make_wide_robot_stack(B, 70, levels=2, seed=3)
    st = BatchedStack(plan, B, device=0)
    dev = st.load_leaf(leaf)
    st.update(dev)
    st.solve(B)
    torch.cuda.synchronize()
    dq0, s0 = st.dq.clone(), st.status.clone()
    assert (s0 == 0).all()
    st.dq.zero_()
    st.cycle(dev)
    torch.cuda.synchronize()
    assert torch.equal(dq0, st.dq) and torch.equal(s0, st.status)
    # one stream, captured once, replayed
    s = torch.cuda.Stream()
    st.stream = s
    with torch.cuda.stream(s):
        st.cycle(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        st.cycle(dev)
    st.dq.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(dq0, st.dq)


def test_wide_route_refusals(gpu_device):
    L = abi.lib()
    plan, leaf = synth.make_wide_robot_stack(4, 80, seed=1)
    st = BatchedStack(plan, 4, device=0)
    h = st._h
    qb = st._qp_batch(4)
    assert L.osot_nhqp_solve(h, C.byref(qb), None, None) == abi.ERR_UNSUPPORTED
    assert L.osot_ehqp_solve(h, C.byref(qb), 0.0, None) == abi.ERR_UNSUPPORTED
    assert L.osot_solver_set_hotstart(h, 1) == abi.ERR_UNSUPPORTED and b"wide route" in L.osot_last_error()
    assert L.osot_solver_set_hotstart(h, 0) == abi.OK
    cyc = (C.c_longlong * (4 * 18))()
    assert L.osot_solver_profile_phases(h, C.byref(qb), C.cast(cyc, C.c_void_p), None) == abi.ERR_UNSUPPORTED
    lb, out = st._update_args(st.load_leaf(leaf))
    kb = abi.KinBatch(); kb.B = 4
    assert L.osot_control_cycle(h, C.c_void_p(1), C.byref(kb), C.byref(lb), C.byref(out), C.byref(qb), None, None) == abi.ERR_UNSUPPORTED
    assert L.osot_control_rollout(h, C.c_void_p(1), C.byref(kb), C.byref(lb), C.byref(out), C.byref(qb), None, 2, None, None, None) == abi.ERR_UNSUPPORTED
    assert L.osot_solver_set_schedule(h, 0) == abi.OK and L.osot_solver_set_timing(h, 1) == abi.OK
    with pytest.raises(RuntimeError, match="wide route"):
        st.set_hotstart(True)
    # the wavefront route keeps its limit
    pd = plan.to_c()
    hh = C.c_void_p()
    assert L.osot_solver_create(C.byref(pd), 4, 0, C.byref(hh)) == abi.ERR_INVALID


from test_wide_plan_host import _pick, _witnesses, oracle_solve as _oracle   # noqa: E402

# (tasks, 2) on the device: SOLVED 7e-5 from every witness, lexicographically worse at level 1 -- the known limitation of DESIGN.md 4.6
# (on the host build it is instance 5: the rounding of the two builds differs at these degenerate vertices); strict, so the fix shows
STUCK_GPU = [("tasks", i) for i in (0, 1, 3, 4, 5)] + [pytest.param("tasks", 2, marks=pytest.mark.xfail(strict=True, reason="known: DESIGN.md 4.6")),
                                                       ("ttc", 0), ("ttc_exchange", 0)]


@pytest.mark.parametrize("mode,i", STUCK_GPU)
def test_wide_route_default_eps_stuck_instances(mode, i, gpu_device):
    """the wavefront route's default-eps regression fixtures (test_default_eps_stuck_instances_gpu) through route="wide": SOLVED,
    acceptable by the lexicographic rule, what was accepted reported and below 1e-7"""
    from helpers import answer_is_acceptable, default_eps_stuck_instances
    plan, asm = default_eps_stuck_instances(mode)
    asm = _pick(asm, i)
    dq, _, st, _, slack = _solve(plan, asm, route="wide")
    assert st[0] == 0 and slack[0] <= 1e-7
    ok, why = answer_is_acceptable(asm, 0, dq[0], [(nm, r["dq"][0], r["status"][0] == 1) for nm, r in _witnesses(asm)])
    assert ok, why


def test_wide_route_accepted_slack_instance(gpu_device):
    from helpers import accepted_slack_instance, answer_is_acceptable
    plan, asm, wit = accepted_slack_instance()
    dq, _, st, _, slack = _solve(plan, asm, route="wide")
    assert st[0] == 0
    ok, why = answer_is_acceptable(asm, 0, dq[0], wit)
    assert ok, why
    assert slack[0] <= 1.0e-7


def test_wide_update_and_cascade_feature_stack(gpu_device):
    """make_feature_stack at n = 100: dense weight (WA / Wb), body frame, error bands, collision rows among more candidates, more than
    four row blocks -- the update against pyoracle.assemble (W_k A_k, W_k b_k included), the cascade against the oracle"""
    B, n = 32, 100
    plan, leaf = synth.make_feature_stack(B, n=n, seed=3)
    asm = pyoracle.assemble(plan, leaf)
    st = BatchedStack(plan, B, device=0)
    st.update(st.load_leaf(leaf))
    torch.cuda.synchronize()
    for k in range(plan.L):
        np.testing.assert_allclose(st.b[k].cpu().numpy(), asm["b"][k], rtol=0, atol=1e-15)
        np.testing.assert_array_equal(st.w[k].cpu().numpy(), asm["w"][k])
        W = asm["Wdense"][k] if asm.get("Wdense") else None
        if W is not None:
            ma = plan.ma(k)
            np.testing.assert_allclose(st.WA[k].cpu().numpy(), W[:, :, :ma] @ asm["A"][k], rtol=0, atol=1e-13)
            np.testing.assert_allclose(st.Wb[k].cpu().numpy(), (W @ asm["b"][k][..., None])[..., 0], rtol=0, atol=1e-13)
    np.testing.assert_array_equal(st.l.cpu().numpy(), asm["l"])
    np.testing.assert_array_equal(st.u.cpu().numpy(), asm["u"])
    np.testing.assert_array_equal(st.C.cpu().numpy(), asm["C"])
    np.testing.assert_array_equal(st.lo.cpu().numpy(), asm["lo"])
    np.testing.assert_array_equal(st.up.cpu().numpy(), asm["up"])
    st.solve(B)
    torch.cuda.synchronize()
    dq, status = st.dq.cpu().numpy(), st.status.cpu().numpy()
    ref = _oracle(asm)
    ok = ref["status"] == 1
    assert (status == 0).all() and ok.any()
    assert close(dq[ok], ref["dq"][ok])
