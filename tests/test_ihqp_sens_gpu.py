"""osot_ihqp_level_qp / osot_ihqp_sensitivity on the device, with x_levels from the device's own cascade: the cases (a) .. (f) of
tests/test_ihqp_sens_host.py through the C-ABI (sentinel-fenced device buffers) and through BatchedStack, with the same comparisons
and tolerances (tests/ihqp_sens_ref.py), forward and with the backward pass; torch_api.ihqp_layer against the longdouble chain; a HIP
graph replay; torch_api.iHQP's getObjective against osot_backend_get_objective on the materialised level QP; the refusals."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from opensot_amd import abi, torch_api
from opensot_amd.solver import BackEnd, BatchedStack

import ihqp_sens_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture():
    return R.fixture()


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


def solved_stack(case, inp, plan=None):
    st = BatchedStack(plan or case.plan, case.B, route="wavefront")
    load(st, case, inp, case.B)
    st.solve(case.B)
    torch.cuda.synchronize()
    return st, st.x_levels[:case.B].cpu().numpy(), st.status[:case.B].cpu().numpy()


class DeviceFenced(R.Fenced):
    """R.Fenced mirrored on the device: the kernels get the device copy's address, download() brings it back"""

    def __init__(self, shape, ints=False):
        super().__init__(shape, ints)
        self.dev = torch.from_numpy(self.raw.copy()).cuda()

    @property
    def address(self):
        return self.dev.data_ptr() + R.PAD * self.raw.itemsize

    def download(self):
        self.raw[...] = self.dev.cpu().numpy()


def sensitivity_through_the_abi(st, case, B, grad_dq=None):
    """osot_ihqp_sensitivity on the stack's handle and batch into fenced device buffers -> R.SensOutputs (downloaded)"""
    nbytes = C.c_ulonglong(0)
    back = grad_dq is not None
    abi.check(abi.lib().osot_ihqp_sens_workspace_bytes(st._h, B, int(back), int(back), C.byref(nbytes)), "osot_ihqp_sens_workspace_bytes")
    assert nbytes.value == R.host_workspace_bytes(case, B, back, back)
    out = R.SensOutputs(case, B, workspace_bytes=nbytes.value, fenced=DeviceFenced)
    s = out.struct(st._qp_batch(B))
    grads = None
    if back:
        gdq = torch.from_numpy(np.ascontiguousarray(grad_dq)).cuda()
        s.grad_dq = gdq.data_ptr()
        grads = R.GradOutputs(case, B, fenced=DeviceFenced)
        grads.bind(s)
    abi.check(abi.lib().osot_ihqp_sensitivity(st._h, C.byref(s), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "osot_ihqp_sensitivity")
    torch.cuda.synchronize()
    for f in out.y + out.active + out.flag + [out.objective, out.workspace] + ([f for _, f in grads.every()] if back else []):
        f.download()
    return (out, grads) if back else out


def values(fenced):
    return [f.value for f in fenced]


@pytest.mark.parametrize("name", tuple(R.cases()))
def test_cases_on_the_device(gpu_device, name):
    """the device's cascade, then every level's QP against the restatement at the device's x_levels and the multipliers, sets, flags
    and objectives against the arbiter there: through the C-ABI with fences and through BatchedStack, bit for bit the same"""
    case, fx = R.cases()[name], fixture()[name]
    st, xl, status = solved_stack(case, fx["inp"])
    assert np.all(status == abi.STATUS_SOLVED)
    live = [k for k in range(case.plan.L) if case.active(k)]
    print(f"  case {name}: max|x_levels - the reference's| = {np.max(np.abs(xl[:, live] - fx['x_levels'][:, live])):.3e}")
    assert np.max(np.abs(xl[:, live] - fx["x_levels"][:, live])) <= 1e-6
    for k in range(case.plan.L):
        assert st.level_rows(k) == case.rows(k)
        qp = {key: t.cpu().numpy() for key, t in st.level_qp(k, case.B).items()}
        R.assert_level_qp(case, fx["inp"], k, xl, qp)
    out = sensitivity_through_the_abi(st, case, case.B)
    assert out.fences_intact()
    y, active, flag, objective = values(out.y), values(out.active), values(out.flag), out.objective.value
    worst = R.assert_multipliers(case, fx["inp"], xl, None, y, active, flag, objective, require_ok=name != "e")
    print(f"  case {name}: worst deviation {worst:.3f} SENS_TOL")
    # the reference's getObjVal() is at ITS x: the device's x is within 1e-6 of it and the objective is stationary at the minimiser
    # on the feasible set (1e-8 max(1, |f|): test_ihqp_get_objective_against_the_backend has the estimate)
    ref = fx["objective"][:, live]
    assert np.all(np.abs(objective[:, live] - ref) <= (R.OBJECTIVE_REF_TOL + 1e-8) * np.maximum(1.0, np.abs(ref)))
    m = st.multipliers(case.B)
    torch.cuda.synchronize()
    for k in range(case.plan.L):
        assert np.array_equal(m["y"][k].cpu().numpy(), y[k]) and np.array_equal(m["active"][k].cpu().numpy(), active[k])
        assert np.array_equal(m["flag"][k].cpu().numpy(), flag[k])
    assert np.array_equal(m["objective"].cpu().numpy(), objective)
    emu = R.host_sensitivity(case, fx["inp"], xl)
    print("  device - emulation, y:", max(float(np.max(np.abs(a - b.value))) for a, b in zip(y, emu.y)))


def test_failed_instances_on_the_device(gpu_device):
    """(f): shape (b) with max_iter = 1: the instances the device could not solve are SKIPPED with zeros at every level"""
    case, fx = R.cases()["b"], fixture()["b"]
    st, xl, status = solved_stack(case, fx["inp"], dataclasses.replace(case.plan, max_iter=1))
    assert np.any(status != 0) and np.any(status == 0), status
    out = sensitivity_through_the_abi(st, case, case.B)
    assert out.fences_intact()
    y, active, flag, objective = values(out.y), values(out.active), values(out.flag), out.objective.value
    assert all(np.all(np.isfinite(a)) for a in y) and np.all(np.isfinite(objective))
    R.assert_multipliers(case, fx["inp"], xl, status, y, active, flag, objective, require_ok=False)
    for k in range(case.plan.L):
        assert np.all(flag[k][status != 0] == R.SKIPPED) and np.all(flag[k][status == 0] != R.SKIPPED)


@pytest.mark.parametrize("name", tuple(R.cases()))
def test_gradients_on_the_device(gpu_device, name):
    """the backward pass at the device's own x_levels against the longdouble chain there, through the C-ABI with fences and through
    BatchedStack.backward, bit for bit the same; the forward outputs are those of the forward-only call"""
    case, fx = R.cases()[name], fixture()[name]
    st, xl, status = solved_stack(case, fx["inp"])
    fwd = sensitivity_through_the_abi(st, case, case.B)
    out, grads = sensitivity_through_the_abi(st, case, case.B, fx["grad_dq"])
    assert out.fences_intact() and grads.fences_intact()
    assert all(np.array_equal(a.value, b.value) for a, b in zip(out.y + out.active + out.flag, fwd.y + fwd.active + fwd.flag))
    got = grads.values()
    worst = R.assert_gradients(case, fx["inp"], xl, fx["grad_dq"], got, values(out.flag))
    print(f"  case {name}: worst |X - X*| / bound = {worst[0]:.3e} (grad_{worst[1]}, level {worst[2]}, instance {worst[3]})")
    g = st.backward(case.B, torch.from_numpy(fx["grad_dq"]).cuda(), want_A=True)
    torch.cuda.synchronize()
    for k in range(case.plan.L):
        for key in ("b", "w", "c", "A"):
            if got[key][k] is not None:
                assert np.array_equal(g[key][k].cpu().numpy(), got[key][k]), (key, k)
    for key in ("C", "lo", "up", "l", "u"):
        if got[key] is not None:
            assert np.array_equal(g[key].cpu().numpy(), got[key]), key


def test_failed_instances_have_zero_gradients_on_the_device(gpu_device):
    case, fx = R.cases()["b"], fixture()["b"]
    st, xl, status = solved_stack(case, fx["inp"], dataclasses.replace(case.plan, max_iter=1))
    assert np.any(status != 0) and np.any(status == 0), status
    out, grads = sensitivity_through_the_abi(st, case, case.B, fx["grad_dq"])
    assert out.fences_intact() and grads.fences_intact()
    assert all(np.all(np.isfinite(f.value)) for _, f in grads.every())
    R.assert_gradients(case, fx["inp"], xl, fx["grad_dq"], grads.values(), values(out.flag), status)


def test_ihqp_layer_against_the_arbiter(gpu_device):
    """torch_api.ihqp_layer on shape (a): loss = sum(grad_dq * dq), loss.backward(); the gradients autograd hands back for b, w, lo, up,
    l, u, A and C are the longdouble chain's at the layer's own x_levels (the bound of R.assert_gradients); an input that does not
    require a gradient gets none; .last holds the status and the levels' flags"""
    case, fx = R.cases()["a"], fixture()["a"]
    inp, B, L = fx["inp"], case.B, case.plan.L
    st = BatchedStack(case.plan, B, route="wavefront")
    t = lambda a, rg=True: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(rg)
    b, w, A = [t(a) for a in inp["b"]], [t(a) for a in inp["w"]], [t(a) for a in inp["A"]]
    lo, up, l, u, Cm = t(inp["lo"]), t(inp["up"]), t(inp["l"]), t(inp["u"], False), t(inp["C"])
    dq = torch_api.ihqp_layer(st, b, w, lo, up, l, u, A, Cm)
    assert torch.all(torch_api.ihqp_layer.last.status == abi.STATUS_SOLVED) and torch_api.ihqp_layer.last.flag is None
    (dq * torch.from_numpy(fx["grad_dq"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert u.grad is None
    xl = st.x_levels[:B].cpu().numpy()
    flag = [f.cpu().numpy() for f in torch_api.ihqp_layer.last.flag]
    got = dict(b=[x.grad.cpu().numpy() for x in b], w=[x.grad.cpu().numpy() for x in w], A=[x.grad.cpu().numpy() for x in A],
               c=[None] * L, C=Cm.grad.cpu().numpy(), lo=lo.grad.cpu().numpy(), up=up.grad.cpu().numpy(), l=l.grad.cpu().numpy(), u=None)
    # (c and u are not inputs that asked for a gradient here: their slots are filled from BatchedStack.backward on the same state)
    g = st.backward(B, torch.from_numpy(fx["grad_dq"]).cuda())
    got["c"], got["u"] = [x.cpu().numpy() for x in g["c"]], g["u"].cpu().numpy()
    worst = R.assert_gradients(case, inp, xl, fx["grad_dq"], got, flag)
    print(f"  ihqp_layer: worst |X - X*| / bound = {worst[0]:.3e} (grad_{worst[1]})")


def test_ihqp_layer_raises_before_solving(gpu_device):
    case = R.cases()["a"]
    wide = BatchedStack(case.plan, case.B, route="wide")
    b0 = torch.zeros((case.B, case.plan.m(0)), dtype=torch.float64, device="cuda")
    wide.status.fill_(-5)
    with pytest.raises(ValueError, match="wide stack"):
        torch_api.ihqp_layer(wide, [b0, None])
    assert torch.all(wide.status == -5)                     # nothing was solved
    dense = R.extra_cases()["dense"]
    st = BatchedStack(dense.plan, dense.B, route="wavefront")
    with pytest.raises(ValueError, match="dense-weight level or a regularisation task"):
        torch_api.ihqp_layer(st, [torch.zeros((dense.B, dense.plan.m(0)), dtype=torch.float64, device="cuda"), None])
    with pytest.raises(RuntimeError, match="not built for plans with a"):
        st.backward(dense.B, torch.zeros((dense.B, dense.plan.n), dtype=torch.float64, device="cuda"))


def test_graph_replay_gives_the_eager_bits(gpu_device):
    """case (c), 33 variables: one eager call (it raises the multiplier kernel's LDS limit on the device), then the same call
    captured into a HIP graph and replayed into cleared outputs"""
    case, fx = R.cases()["c"], fixture()["c"]
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


def test_ihqp_get_objective_against_the_backend(gpu_device):
    """torch_api.iHQP.getObjective(i) against osot_backend_get_objective of a BackEnd that solves the materialised level QP itself.
    Both x are within the parity bound 1e-6 of the level's minimiser; the objective is stationary there on the feasible set, so the
    two differ by at most 1/2 |H~| 1e-12 plus |y| times a feasibility residual of 1e-9: 1e-8 max(1, |f|) carries a factor ten."""
    case, fx = R.cases()["a"], fixture()["a"]
    ih = torch_api.iHQP(dataclasses.replace(case.plan), case.B, eps_regularisation=R.EPS_FACTOR)
    load(ih.stack, case, fx["inp"], case.B)
    with pytest.raises(RuntimeError):
        ih.getObjective(0)
    ih.solve(B=case.B)
    n = case.plan.n
    for k in range(case.plan.L):
        f = ih.getObjective(k).cpu().numpy()
        y, flag = ih.getDualSolution(k), ih.getSensitivityFlag(k)
        assert tuple(y.shape) == (case.B, n + case.rows(k)) and tuple(ih.getActiveSet(k).shape) == tuple(y.shape) and torch.all(flag == R.OK)
        qp = {key: t.cpu().numpy() for key, t in ih.getLevelQP(k).items()}
        for i in range(2):
            be = BackEnd(n, case.rows(k), eps_regularisation=R.EPS_FACTOR)
            assert be.initProblem(qp["H"][i], qp["g"][i], qp["A"][i], qp["lA"][i], qp["uA"][i], qp["l"][i], qp["u"][i])
            assert abs(be.getObjective() - f[i]) <= 1e-8 * max(1.0, abs(f[i])), (k, i, be.getObjective(), f[i])
    with pytest.raises(IndexError):
        ih.getObjective(case.plan.L)


def test_a_wide_stack_is_refused(gpu_device):
    case = R.cases()["a"]
    st = BatchedStack(case.plan, case.B, route="wide")
    gdq = torch.zeros((case.B, case.plan.n), dtype=torch.float64, device="cuda")
    for call in (lambda: st.multipliers(case.B), lambda: st.level_qp(0, case.B), lambda: st.sens_workspace(case.B),
                 lambda: st.backward(case.B, gdq)):
        with pytest.raises(RuntimeError, match="wide route"):
            call()
    assert st.level_rows(1) == case.rows(1)
