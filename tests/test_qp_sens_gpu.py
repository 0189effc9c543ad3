"""osot_qp_sensitivity_batch on the device: the fixture against the longdouble arbiter (and, for the record, the host emulation), end to
end behind osot_qp_solve_batch against the float64 restatement, the multipliers against the reference's qpOASES live, and the tensor
entries torch_api.qp_multipliers / qp_layer (finite differences through the device solve, NULL gradient outputs, a failed instance,
HIP graph replay)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from opensot_amd import abi, torch_api
from oracle import pyref

import helpers
import qp_sens_ref as R
from test_qp_sens_host import FD_STEP, assert_matches_arbiter, fd_bound

pytestmark = pytest.mark.gpu


class DeviceArrays:
    """host arrays mirrored on the device: address(a) uploads a once; download(arrays) brings the mirrored ones back"""

    def __init__(self):
        self.mirror = {}

    def address(self, a):
        if id(a) not in self.mirror:
            assert a.flags["C_CONTIGUOUS"]
            self.mirror[id(a)] = (a, torch.from_numpy(a.copy()).cuda())
        return self.mirror[id(a)][1].data_ptr()

    def download(self, arrays):
        for a in arrays:
            if id(a) in self.mirror:
                a[...] = self.mirror[id(a)][1].cpu().numpy()


def run_device(p, x, gx=None, status=None, want=None):
    """the case through libosot_mi355x.so -> Outputs"""
    if want is None:
        want = R.Outputs.ALL if gx is not None else ("y", "active", "flag")
    out, keep, dv = R.Outputs(p, want), [], DeviceArrays()
    b = R.structs(p, x, out, dv.address, keep, gx, status)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().osot_qp_sensitivity_batch(C.byref(b), None, st), "osot_qp_sensitivity_batch")
    torch.cuda.synchronize()
    dv.download(out.raw.values())
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    return R.fixture()


def tensors(p, device="cuda"):
    return {k: (None if p[k] is None else torch.from_numpy(p[k]).to(device)) for k in ("H", "g", "A", "lA", "uA", "l", "u")}


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(len(R.SHAPES)))
def test_fixture_on_the_device(gpu_device, s):
    """the assertions of tests/test_qp_sens_host.py on the device's results; the difference to the emulation is printed"""
    p, x, y_ref, gx = fixture()[s]
    arb = R.arbiter(p, x, gx)
    out = run_device(p, x, gx)
    assert out.fences_intact()
    assert np.all(out.flag == R.OK)
    assert np.array_equal(out.active, R.reference_active(p, y_ref))
    assert_matches_arbiter(p, out, arb)
    emu = R.run_host(p, x, gx)
    for k in ("y",) + R.GRADS:
        a, b = getattr(out, k), getattr(emu, k)
        print(f"  device - emulation, {k:8s}: {np.max(np.abs(a - b)) if a.size else 0.0:.3e}")


# ---- 2. end to end behind the product's own solve ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nc,n_eq,B", [(32, 40, 3, 64), (64, 24, 0, 16)])
def test_end_to_end_against_restatement(gpu_device, n, nc, n_eq, B):
    """osot_qp_solve_batch, then the new call on the product's own x, against the float64 restatement on that x.  Both are within
    SENS_TOL of the arbiter (the restatement by measurement, the kernel by the fixture test), so they are within 2 SENS_TOL of each
    other, in the units of qp_sens_ref."""
    rng = np.random.default_rng([n, nc, B, 31])
    p = R.problem(*helpers.random_qp(rng, B, n, nc, n_eq=n_eq))
    gx = rng.normal(size=(B, n))
    t = tensors(p)
    x, status, _ = torch_api.qp_solve(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"])
    assert torch.all(status == abi.STATUS_SOLVED)
    x = x.cpu().numpy()
    out = run_device(p, x, gx, status=status.cpu().numpy())
    assert out.fences_intact()
    ref = R.restate(p, x, gx)
    assert [int(f) for f in out.flag] == [r["flag"] for r in ref]
    assert np.array_equal(out.active, np.stack([r["active"] for r in ref]))
    for name in ("y",) + R.GRADS:
        dev = R.worst_deviation(p, out, ref, names=(name,))
        print(f"  {name:8s} worst deviation from the restatement {dev[0]:.3e} (instance {dev[2]}), bound {2 * R.SENS_TOL:.3e}")
        assert dev[0] <= 2.0 * R.SENS_TOL, dev


# ---- 3. the reference's multipliers, live ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not pyref.available(), reason="the reference's qpOASES build (oracle/_ref) is not present")
def test_multipliers_against_reference_live(gpu_device):
    """64 fresh random_qp draws at (32, 40): the device's y at the reference's x against RefBackEnd.getDual().  Each is within
    SENS_TOL of the arbiter at that x (SENS_TOL is ten times the reference's worst over the fixture): 2 SENS_TOL between them.
    Instances whose reference margins are below 1e-6 are left out, at most 5 %."""
    n, nc, B = 32, 40, 64
    rng = np.random.default_rng([n, nc, B, 99])
    p = R.problem(*helpers.random_qp(rng, B, n, nc, n_eq=3))
    xr, yr, keep = np.zeros((B, n)), np.zeros((B, n + nc)), []
    for i in range(B):
        be = pyref.RefBackEnd(n, nc, pyref.HST_SEMIDEF, 2e2)
        ok = be.initProblem(p["H"][i], p["g"][i], p["A"][i], np.clip(p["lA"][i], -1e20, 1e20), np.clip(p["uA"][i], -1e20, 1e20), p["l"][i], p["u"][i])
        xr[i], yr[i] = be.getSolution(), be.getDual()
        if ok and R.margins_ok(p["A"][i], p["lA"][i], p["uA"][i], p["l"][i], p["u"][i], xr[i], yr[i]):
            keep.append(i)
    assert len(keep) >= 0.95 * B, f"{B - len(keep)} of {B} instances are near-degenerate by the reference's own margins"
    out = run_device(p, xr)
    cond = R.cond_H(p)
    worst = 0.0
    for i in keep:
        dev = np.max(np.abs(out.y[i] - yr[i])) / (cond[i] * np.max(np.abs(yr[i])))
        worst = max(worst, dev)
        assert out.flag[i] == R.OK and dev <= 2.0 * R.SENS_TOL, (i, dev)
    assert np.array_equal(out.active[keep], R.reference_active(p, yr)[keep])
    print(f"  {len(keep)} of {B} instances, worst deviation of y from the reference {worst:.3e}, bound {2 * R.SENS_TOL:.3e}")


# ---- 4. the tensor entries ---------------------------------------------------------------------------------------------------------------
def layer_problem(B=4):
    p, x, _, gx = fixture()[0]
    q = {k: p[k][:B] for k in ("H", "g", "A", "lA", "uA", "l", "u")}
    return dict(q, B=B, n=p["n"], nc=p["nc"], eps_abs=p["eps_abs"]), x[:B], gx[:B]


def test_qp_layer_against_finite_differences(gpu_device):
    """gradcheck-style at (7, 9, B = 4): H = S + S' with S the parameter; central differences (the step and the bound of
    tests/test_qp_sens_host.py; an entry of S moves two entries of H, or one by 2 h: twice the bound) of grad_x . x through the
    device's own solve, one entry of all four instances per pair of launches"""
    p, x_ref, gx = layer_problem()
    B, n = p["B"], p["n"]
    t = tensors(p)
    S = (0.5 * t["H"]).clone().requires_grad_(True)
    leaves = dict(S=S, **{k: t[k].clone().requires_grad_(True) for k in ("g", "A", "lA", "uA", "l", "u")})
    w = torch.from_numpy(gx).cuda()

    def solve(v):
        H = (v["S"] + v["S"].transpose(1, 2)).contiguous()
        return torch_api.qp_layer(H, v["g"], v["A"], v["lA"], v["uA"], v["l"], v["u"])

    loss = (solve(leaves) * w).sum()
    loss.backward()
    last = torch_api.qp_layer.last
    assert torch.all(last.status == abi.STATUS_SOLVED) and torch.all(last.flag == R.OK)
    assert sorted(last.bound) == sorted(["H", "g", "A", "lA", "uA", "l", "u"])
    bound = np.array([fd_bound(p, i, x_ref[i], gx[i]) for i in range(B)])
    worst = 0.0
    with torch.no_grad():
        for name, leaf in leaves.items():
            grad = leaf.grad.cpu().numpy().reshape(B, -1)
            flat = leaf.detach().reshape(B, -1)
            for e in range(flat.shape[1]):
                if not torch.all(torch.isfinite(flat[:, e])):
                    assert np.all(grad[:, e] == 0.0)
                    continue
                vals = []
                for sgn in (1.0, -1.0):
                    v = {k: a.detach().clone() for k, a in leaves.items()}
                    v[name].reshape(B, -1)[:, e] += sgn * FD_STEP
                    vals.append((solve(v) * w).sum(dim=1))
                fd = ((vals[0] - vals[1]) / (2.0 * FD_STEP)).cpu().numpy()
                ratio = np.abs(fd - grad[:, e]) / ((2.0 if name == "S" else 1.0) * bound)
                worst = max(worst, ratio.max())
                assert np.all(ratio <= 1.0), (name, e, fd, grad[:, e], bound)
    print(f"  worst |fd - grad| / bound = {worst:.3e}")


def test_qp_layer_binds_only_what_needs_a_gradient(gpu_device):
    p, _, gx = layer_problem()
    t = tensors(p)
    t["g"].requires_grad_(True)
    t["lA"].requires_grad_(True)
    x = torch_api.qp_layer(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"])
    (x * torch.from_numpy(gx).cuda()).sum().backward()
    assert sorted(torch_api.qp_layer.last.bound) == ["g", "lA"]
    assert t["g"].grad is not None and t["lA"].grad is not None
    assert all(t[k].grad is None for k in ("H", "A", "uA", "l", "u"))
    # box only, no rows
    p12 = fixture()[4][0]
    t = tensors(p12)
    t["H"].requires_grad_(True)
    x = torch_api.qp_layer(t["H"], t["g"], l=t["l"], u=t["u"])
    x.sum().backward()
    assert torch_api.qp_layer.last.bound == ["H"] and torch.all(torch.isfinite(t["H"].grad))
    assert torch.equal(t["H"].grad, t["H"].grad.transpose(1, 2))


def test_qp_layer_unsolved_instance_gives_zero_gradient(gpu_device):
    p, _, gx = layer_problem()
    t = tensors(p)
    for k in ("H", "g", "A", "lA", "uA", "l", "u"):
        t[k].requires_grad_(True)
    x = torch_api.qp_layer(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], max_iter=1)
    (x * torch.from_numpy(gx).cuda()).sum().backward()
    last = torch_api.qp_layer.last
    failed = last.status != abi.STATUS_SOLVED
    assert torch.any(last.status == abi.STATUS_MAX_ITER)
    assert torch.all(last.flag[failed] == R.SKIPPED)
    for k in ("H", "g", "A", "lA", "uA", "l", "u"):
        assert torch.all(t[k].grad[failed] == 0.0) and torch.all(torch.isfinite(t[k].grad))


def test_qp_multipliers_shapes_and_dtypes(gpu_device):
    p, x, y_ref, _ = fixture()[0]
    t = tensors(p)
    xs, status, _ = torch_api.qp_solve(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"])
    y, active, flag = torch_api.qp_multipliers(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], xs, status)
    B, n, nc = p["B"], p["n"], p["nc"]
    assert y.shape == (B, n + nc) and y.dtype == torch.float64 and y.is_cuda
    assert active.shape == (B, n + nc) and active.dtype == torch.int32
    assert flag.shape == (B,) and flag.dtype == torch.int32 and torch.all(flag == R.OK)
    assert np.array_equal(active.cpu().numpy(), R.reference_active(p, y_ref))
    with pytest.raises(RuntimeError, match="above 64"):
        torch_api.qp_multipliers(torch.eye(65, dtype=torch.float64, device="cuda")[None], torch.zeros((1, 65), dtype=torch.float64, device="cuda"),
                                 None, None, None, None, None, torch.zeros((1, 65), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="64 variables"):
        torch_api.qp_layer(torch.eye(65, dtype=torch.float64, device="cuda")[None], torch.zeros((1, 65), dtype=torch.float64, device="cuda"))


def test_graph_replay_gives_the_same_bits(gpu_device):
    """the call allocates nothing and synchronises nothing: captured into a HIP graph, its replay gives the bits of the eager run"""
    p, x, _, gx = fixture()[1]
    t = tensors(p)
    xs = torch.from_numpy(x).cuda()
    eager = torch_api.qp_multipliers(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], xs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch_api.qp_multipliers(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = torch_api.qp_multipliers(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], xs)
    for _ in range(2):
        for o in captured:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(a, b)
