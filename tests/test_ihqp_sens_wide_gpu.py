"""osot_ihqp_level_qp / osot_ihqp_sensitivity on the device for plans of 65 .. 128 variables (BatchedStack(route="auto") picks the wide
route), with x_levels from the device's own cascade: the cases (p) .. (t) of tests/test_ihqp_sens_wide_host.py through BatchedStack
with the same comparisons and tolerances (tests/ihqp_sens_wide_ref.py); the level QP and the objective bit for bit against the host
build of the same source; the backward pass and torch_api.ihqp_layer against the longdouble chain; torch_api.iHQP's getters; one
eager call, then a HIP graph capture and replay."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from opensot_amd import abi, torch_api
from opensot_amd.solver import BatchedStack

import ihqp_sens_wide_ref as W

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture():
    return W.fixture()


def load(st, case, inp, B):
    """the inputs of a case into the stack's buffers, its switches onto the stack"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(st.device)
    for k in range(case.plan.L):
        if st.A[k] is not None:
            st.A[k][:B].copy_(t(inp["A"][k]))
        st.b[k][:B].copy_(t(inp["b"][k]))
        st.w[k][:B].copy_(t(inp["w"][k]))
    for name in ("C", "lo", "up", "l", "u"):
        if inp[name] is not None:
            getattr(st, name)[:B].copy_(t(inp[name]))
    st.level_active = case.level_active
    for (k, j), on in (case.task_active or {}).items():
        st.set_task_active(k, j, on)


def solved_stack(case, inp):
    st = BatchedStack(case.plan, case.B, route="auto")
    assert st.route == "wide"
    load(st, case, inp, case.B)
    st.solve(case.B)
    torch.cuda.synchronize()
    return st, st.x_levels[:case.B].cpu().numpy(), st.status[:case.B].cpu().numpy()


def cpu(v):
    return [t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()


@pytest.mark.parametrize("name", tuple(W.cases()))
def test_cases_on_the_device(gpu_device, name):
    """the device's cascade on the wide route, then every level's QP against the restatement at the device's x_levels and against the
    host build's bits, the multipliers, sets, flags and objectives against the arbiter there, the objective against the host build's
    bits and the reference's getObjVal()"""
    case, fx = W.cases()[name], fixture()[name]
    st, xl, status = solved_stack(case, fx["inp"])
    assert np.all(status == abi.STATUS_SOLVED)
    live = [k for k in range(case.plan.L) if case.active(k)]
    print(f"  case {name}: max|x_levels - the reference's| = {np.max(np.abs(xl[:, live] - fx['x_levels'][:, live])):.3e}")
    assert np.max(np.abs(xl[:, live] - fx["x_levels"][:, live])) <= 1e-6
    for k in range(case.plan.L):
        assert st.level_rows(k) == case.rows(k)
        qp = {key: cpu(t) for key, t in st.level_qp(k, case.B).items()}
        W.assert_level_qp(case, fx["inp"], k, xl, qp)
        host = W.host_level_qp(case, fx["inp"], k, xl)
        for key, f in host.items():
            assert np.array_equal(qp[key], f.value), (name, k, key)
    m = st.multipliers(case.B)
    torch.cuda.synchronize()
    y, active, flag, objective = cpu(m["y"]), cpu(m["active"]), cpu(m["flag"]), cpu(m["objective"])
    worst = W.assert_multipliers(case, fx["inp"], xl, None, y, active, flag, objective)
    print(f"  case {name}: worst deviation {worst:.3f} SENS_TOL")
    # the reference's getObjVal() is at ITS x: the device's x is within 1e-6 of it and the objective is stationary at the minimiser
    # on the feasible set (1e-8 max(1, |f|): tests/test_ihqp_sens_gpu.py has the estimate)
    ref = fx["objective"][:, live]
    assert np.all(np.abs(objective[:, live] - ref) <= (W.OBJECTIVE_REF_TOL + 1e-8) * np.maximum(1.0, np.abs(ref)))
    host = W.host_sensitivity(case, fx["inp"], xl)
    assert np.array_equal(objective, host.objective.value)
    same = all(np.array_equal(a, b.value) for a, b in zip(y + active + flag, host.y + host.active + host.flag))
    print(f"  case {name}: y, active, flag equal the host build's bits: {same}; max|y - host's| = "
          f"{max(float(np.max(np.abs(a - b.value))) for a, b in zip(y, host.y)):.3e}")


@pytest.mark.parametrize("name", ("p", "r"))
def test_gradients_on_the_device(gpu_device, name):
    """BatchedStack.backward at the device's own x_levels against the longdouble chain there (the bound of assert_gradients); the
    flags are those of the forward-only call"""
    case, fx = W.cases()[name], fixture()[name]
    st, xl, status = solved_stack(case, fx["inp"])
    fwd = st.multipliers(case.B)
    g = st.backward(case.B, torch.from_numpy(fx["grad_dq"]).cuda(), want_A=True)
    torch.cuda.synchronize()
    got = {key: [None if t is None else cpu(t) for t in g[key]] for key in W.GRAD_LEVEL}
    got.update({key: None if g[key] is None else cpu(g[key]) for key in W.GRAD_GLOBAL})
    flag = cpu(g["flag"])
    assert all(np.array_equal(a, b) for a, b in zip(flag, cpu(fwd["flag"])))
    worst = W.assert_gradients(case, fx["inp"], xl, fx["grad_dq"], got, flag)
    print(f"  case {name}: worst |X - X*| / bound = {worst[0]:.3e} (grad_{worst[1]}, level {worst[2]}, instance {worst[3]})")
    _, host = W.host_backward(case, fx["inp"], xl, fx["grad_dq"])
    hv = host.values()
    pairs = [(got[key][k], hv[key][k]) for key in W.GRAD_LEVEL for k in range(case.plan.L) if hv[key][k] is not None]
    pairs += [(got[key], hv[key]) for key in W.GRAD_GLOBAL if hv[key] is not None]
    print(f"  case {name}: the gradients equal the host build's bits: {all(np.array_equal(a, b) for a, b in pairs)}")


@pytest.mark.parametrize("name", ("p", "r"))
def test_ihqp_layer_against_the_arbiter(gpu_device, name):
    """torch_api.ihqp_layer on a wide stack: loss = sum(grad_dq * dq), loss.backward(); the gradients autograd hands back for b, w, A,
    C, lo, up, l are the longdouble chain's at the layer's own x_levels (the bound of assert_gradients); u, which does not require a
    gradient, gets none; .last holds the status and the levels' flags"""
    case, fx = W.cases()[name], fixture()[name]
    inp, B, L = fx["inp"], case.B, case.plan.L
    st = BatchedStack(case.plan, B, route="auto")
    load(st, case, inp, B)                     # (the switches; the layer copies the tensors)
    t = lambda a, rg=True: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(rg)
    b, w, A = [t(a) for a in inp["b"]], [t(a) for a in inp["w"]], [None if a is None else t(a) for a in inp["A"]]
    lo, up, l, u, Cm = t(inp["lo"]), t(inp["up"]), t(inp["l"]), t(inp["u"], False), t(inp["C"])
    dq = torch_api.ihqp_layer(st, b, w, lo, up, l, u, A, Cm)
    assert torch.all(torch_api.ihqp_layer.last.status == abi.STATUS_SOLVED) and torch_api.ihqp_layer.last.flag is None
    (dq * torch.from_numpy(fx["grad_dq"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert u.grad is None
    xl = st.x_levels[:B].cpu().numpy()
    flag = cpu(torch_api.ihqp_layer.last.flag)
    got = dict(b=[x.grad.cpu().numpy() for x in b], w=[x.grad.cpu().numpy() for x in w],
               A=[None if x is None else x.grad.cpu().numpy() for x in A], c=[None] * L, C=Cm.grad.cpu().numpy(),
               lo=lo.grad.cpu().numpy(), up=up.grad.cpu().numpy(), l=l.grad.cpu().numpy(), u=None)
    # (c and u are not inputs that asked for a gradient here: their slots are filled from BatchedStack.backward on the same state)
    g = st.backward(B, torch.from_numpy(fx["grad_dq"]).cuda())
    got["c"], got["u"] = cpu(g["c"]), cpu(g["u"])
    worst = W.assert_gradients(case, inp, xl, fx["grad_dq"], got, flag)
    print(f"  ihqp_layer, case {name}: worst |X - X*| / bound = {worst[0]:.3e} (grad_{worst[1]})")


def test_ihqp_getters(gpu_device):
    """torch_api.iHQP on case (p): getObjective, getDualSolution, getActiveSet, getSensitivityFlag and getLevelQP of every level are
    BatchedStack's on the same state, and the arbiter's"""
    case, fx = W.cases()["p"], fixture()["p"]
    ih = torch_api.iHQP(dataclasses.replace(case.plan), case.B, eps_regularisation=W.EPS_FACTOR)
    assert ih.stack.route == "wide"
    load(ih.stack, case, fx["inp"], case.B)
    with pytest.raises(RuntimeError):
        ih.getObjective(0)
    ih.solve(B=case.B)
    torch.cuda.synchronize()
    xl = ih.stack.x_levels[:case.B].cpu().numpy()
    L, n = case.plan.L, case.plan.n
    y, active = [cpu(ih.getDualSolution(k)) for k in range(L)], [cpu(ih.getActiveSet(k)) for k in range(L)]
    flag = [cpu(ih.getSensitivityFlag(k)) for k in range(L)]
    objective = np.stack([cpu(ih.getObjective(k)) for k in range(L)], axis=1)
    assert all(a.shape == (case.B, n + case.rows(k)) for k, a in enumerate(y))
    W.assert_multipliers(case, fx["inp"], xl, None, y, active, flag, objective)
    for k in range(L):
        W.assert_level_qp(case, fx["inp"], k, xl, {key: cpu(t) for key, t in ih.getLevelQP(k).items()})
    with pytest.raises(IndexError):
        ih.getObjective(L)


def test_graph_replay_gives_the_eager_bits(gpu_device):
    """case (q): one eager call (it raises the LDS limits of the level kernel and of the multiplier kernel on the device), then the
    same call captured into a HIP graph and replayed into cleared outputs"""
    case, fx = W.cases()["q"], fixture()["q"]
    st, _, _ = solved_stack(case, fx["inp"])
    eager = st.multipliers(case.B)
    torch.cuda.synchronize()
    keep = {key: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for key, v in eager.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            st.multipliers(case.B, out=eager)
    for v in eager.values():
        for t in (v if isinstance(v, list) else [v]):
            t.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    for key, v in eager.items():
        for a, b in zip(v if isinstance(v, list) else [v], keep[key] if isinstance(v, list) else [keep[key]]):
            assert torch.equal(a, b), key


def test_a_wide_stack_of_a_narrow_plan_is_still_refused(gpu_device):
    """n <= 64 on the wide route: the texts of the parent"""
    import ihqp_sens_ref as R
    case = R.cases()["b"]
    st = BatchedStack(case.plan, case.B, route="wide")
    gdq = torch.zeros((case.B, case.plan.n), dtype=torch.float64, device="cuda")
    for call in (lambda: st.multipliers(case.B), lambda: st.level_qp(0, case.B), lambda: st.sens_workspace(case.B),
                 lambda: st.backward(case.B, gdq)):
        with pytest.raises(RuntimeError, match="wide route"):
            call()
    with pytest.raises(ValueError, match="wide stack"):
        torch_api.ihqp_layer(st, [torch.zeros((case.B, case.plan.m(0)), dtype=torch.float64, device="cuda"), None, None])
