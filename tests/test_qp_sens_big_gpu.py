"""osot_qp_sensitivity_batch_ws on the device for 65 .. 128 variables: the fixture tests/golden/qp_sens_big.npz against the longdouble
arbiter (and, for the record, the host build of the same source), end to end behind osot_qp_solve_batch against the float64
restatement, the multipliers against the reference's qpOASES live, the tensor entries torch_api.qp_multipliers / qp_layer with
workspace = qp_sens_workspace(...) (finite differences through the device solve, NULL gradient outputs, a failed instance, HIP
graph replay), and n <= 64 through the new entry against osot_qp_sensitivity_batch bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from opensot_amd import abi, torch_api
from oracle import pyref

import helpers
import qp_sens_ref as R
import qp_sens_big_ref as BG
from test_qp_sens_host import FD_STEP, fd_bound
from test_qp_sens_big_host import TOL, assert_matches_arbiter, mixed

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


def run_device(p, x, gx=None, status=None, want=None, workspace="sized"):
    """the case through libosot_mi355x.so -> Outputs.  workspace: "sized" = qp_sens_workspace's, None = NULL through the new entry,
    "old" = osot_qp_sensitivity_batch"""
    if want is None:
        want = R.Outputs.ALL if gx is not None else ("y", "active", "flag")
    out, keep, dv = R.Outputs(p, want), [], DeviceArrays()
    b = R.structs(p, x, out, dv.address, keep, gx, status)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if workspace == "old":
        abi.check(abi.lib().osot_qp_sensitivity_batch(C.byref(b), None, st), "osot_qp_sensitivity_batch")
    else:
        ws = torch_api.qp_sens_workspace(p["B"], p["n"], p["nc"]) if workspace == "sized" else None
        abi.check(abi.lib().osot_qp_sensitivity_batch_ws(C.byref(b), None, None if ws is None or ws.numel() == 0 else ws.data_ptr(),
                                                         0 if ws is None else ws.numel(), st), "osot_qp_sensitivity_batch_ws")
    torch.cuda.synchronize()
    dv.download(out.raw.values())
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    return BG.fixture()


def tensors(p, device="cuda"):
    return {k: (None if p[k] is None else torch.from_numpy(p[k]).to(device)) for k in ("H", "g", "A", "lA", "uA", "l", "u")}


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(len(BG.SHAPES)))
def test_fixture_on_the_device(gpu_device, s):
    """the assertions of tests/test_qp_sens_big_host.py on the device's results; the difference to the host build is printed"""
    p, x, y_ref, gx = fixture()[s]
    arb = R.arbiter(p, x, gx)
    out = run_device(p, x, gx)
    assert out.fences_intact()
    assert np.all(out.flag == R.OK)
    assert np.array_equal(out.active, R.reference_active(p, y_ref))
    assert_matches_arbiter(p, out, arb)
    assert np.array_equal(out.grad_H, np.transpose(out.grad_H, (0, 2, 1)))
    emu = BG.run_host(p, x, gx)
    for k in ("y",) + R.GRADS:
        a, b = getattr(out, k), getattr(emu, k)
        print(f"  device - emulation, {k:8s}: {np.max(np.abs(a - b)) if a.size else 0.0:.3e}")


# ---- 2. end to end behind the product's own solve ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nc,n_eq,B", [(65, 40, 3, 8), (128, 24, 0, 4)])
def test_end_to_end_against_restatement(gpu_device, n, nc, n_eq, B):
    """osot_qp_solve_batch, then the new call on the product's own x, against the float64 restatement on that x.  Both are within
    SENS_BIG_TOL of the arbiter (the restatement by measurement, the kernel by the fixture test), so they are within twice that of
    each other, in the units of qp_sens_ref."""
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
        print(f"  {name:8s} worst deviation from the restatement {dev[0]:.3e} (instance {dev[2]}), bound {2 * TOL:.3e}")
        assert dev[0] <= 2.0 * TOL, dev


# ---- 3. the reference's multipliers, live ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not pyref.available(), reason="the reference's qpOASES build (oracle/_ref) is not present")
def test_multipliers_against_reference_live(gpu_device):
    """16 fresh random_qp draws at (96, 48): the device's y at the reference's x against RefBackEnd.getDual().  Each is within
    SENS_BIG_TOL of the arbiter at that x (the tolerance is at least ten times the reference's worst over the fixture): twice that
    between them.  Instances whose reference margins are below 1e-6 are left out, at most 1 of 16 (with this seed the reference
    alone keeps 16 of 16)."""
    n, nc, B = 96, 48, 16
    rng = np.random.default_rng([n, nc, B, 99])
    p = R.problem(*helpers.random_qp(rng, B, n, nc, n_eq=0))
    xr, yr, keep = np.zeros((B, n)), np.zeros((B, n + nc)), []
    for i in range(B):
        be = pyref.RefBackEnd(n, nc, pyref.HST_SEMIDEF, 2e2)
        ok = be.initProblem(p["H"][i], p["g"][i], p["A"][i], np.clip(p["lA"][i], -1e20, 1e20), np.clip(p["uA"][i], -1e20, 1e20), p["l"][i], p["u"][i])
        xr[i], yr[i] = be.getSolution(), be.getDual()
        if ok and R.margins_ok(p["A"][i], p["lA"][i], p["uA"][i], p["l"][i], p["u"][i], xr[i], yr[i]):
            keep.append(i)
    assert len(keep) >= B - 1, f"{B - len(keep)} of {B} instances are near-degenerate by the reference's own margins"
    out = run_device(p, xr)
    assert out.fences_intact()
    cond = R.cond_H(p)
    worst = 0.0
    for i in keep:
        dev = np.max(np.abs(out.y[i] - yr[i])) / (cond[i] * np.max(np.abs(yr[i])))
        worst = max(worst, dev)
        assert out.flag[i] == R.OK and dev <= 2.0 * TOL, (i, dev)
    assert np.array_equal(out.active[keep], R.reference_active(p, yr)[keep])
    print(f"  {len(keep)} of {B} instances, worst deviation of y from the reference {worst:.3e}, bound {2 * TOL:.3e}")


# ---- 4. the tensor entries ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_problem():
    """(65, 10, B = 2), solution and multipliers known by construction: every active multiplier is at least 0.5 and every inactive
    side 0.5 away, so a step of FD_STEP stays inside the active set"""
    p, x, _ = R.constructed(2, 65, 10, shape=mixed)
    gx = np.random.default_rng([65, 10, 3]).normal(size=(2, 65))
    return p, x, gx


def test_qp_layer_against_finite_differences(gpu_device):
    """gradcheck-style at (65, 10, B = 2): H = S + S' with S the parameter; central differences (the step and the bound of
    tests/test_qp_sens_host.py; an entry of S moves two entries of H, or one by 2 h: twice the bound) of grad_x . x through the
    device's own solve, on a seeded sample of 24 entries per input, one entry of both instances per pair of launches"""
    p, x_ref, gx = layer_problem()
    B, n, nc = p["B"], p["n"], p["nc"]
    t = tensors(p)
    ws = torch_api.qp_sens_workspace(B, n, nc)
    assert ws.is_cuda and ws.dtype == torch.uint8 and ws.numel() == B * 8 * n * (2 * n + 2)
    S = (0.5 * t["H"]).clone().requires_grad_(True)
    leaves = dict(S=S, **{k: t[k].clone().requires_grad_(True) for k in ("g", "A", "lA", "uA", "l", "u")})
    w = torch.from_numpy(gx).cuda()

    def solve(v, workspace=None):
        H = (v["S"] + v["S"].transpose(1, 2)).contiguous()
        return torch_api.qp_layer(H, v["g"], v["A"], v["lA"], v["uA"], v["l"], v["u"], workspace=workspace)

    xs = solve(leaves, ws)
    assert np.max(np.abs(xs.detach().cpu().numpy() - x_ref)) <= 1e-9          # (the constructed solution is the solve's)
    (xs * w).sum().backward()
    last = torch_api.qp_layer.last
    assert torch.all(last.status == abi.STATUS_SOLVED) and torch.all(last.flag == R.OK)
    assert sorted(last.bound) == sorted(["H", "g", "A", "lA", "uA", "l", "u"])
    bound = np.array([fd_bound(p, i, x_ref[i], gx[i]) for i in range(B)])
    rng = np.random.default_rng([n, nc, 24])
    worst = 0.0
    with torch.no_grad():
        for name, leaf in leaves.items():
            grad = leaf.grad.cpu().numpy().reshape(B, -1)
            assert np.all(np.isfinite(grad))
            size = grad.shape[1]
            for e in sorted(rng.choice(size, size=min(24, size), replace=False)):
                vals = []
                for sgn in (1.0, -1.0):
                    v = {k: a.detach().clone() for k, a in leaves.items()}
                    v[name].reshape(B, -1)[:, e] += sgn * FD_STEP
                    vals.append((torch_api.qp_solve((v["S"] + v["S"].transpose(1, 2)).contiguous(), v["g"], v["A"], v["lA"], v["uA"], v["l"], v["u"])[0] * w).sum(dim=1))
                fd = ((vals[0] - vals[1]) / (2.0 * FD_STEP)).cpu().numpy()
                ratio = np.abs(fd - grad[:, e]) / ((2.0 if name == "S" else 1.0) * bound)
                worst = max(worst, ratio.max())
                assert np.all(ratio <= 1.0), (name, e, fd, grad[:, e], bound)
    print(f"  worst |fd - grad| / bound = {worst:.3e}")


def test_qp_layer_binds_only_what_needs_a_gradient(gpu_device):
    p, _, gx = layer_problem()
    t = tensors(p)
    ws = torch_api.qp_sens_workspace(p["B"], p["n"], p["nc"])
    t["g"].requires_grad_(True)
    t["lA"].requires_grad_(True)
    x = torch_api.qp_layer(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], workspace=ws)
    (x * torch.from_numpy(gx).cuda()).sum().backward()
    assert sorted(torch_api.qp_layer.last.bound) == ["g", "lA"]
    assert t["g"].grad is not None and t["lA"].grad is not None
    assert all(t[k].grad is None for k in ("H", "A", "uA", "l", "u"))
    # box only, no rows
    p100 = fixture()[2][0]
    t = tensors(p100)
    t["H"].requires_grad_(True)
    x = torch_api.qp_layer(t["H"], t["g"], l=t["l"], u=t["u"], workspace=torch_api.qp_sens_workspace(p100["B"], p100["n"], 0))
    x.sum().backward()
    assert torch_api.qp_layer.last.bound == ["H"] and torch.all(torch.isfinite(t["H"].grad))
    assert torch.equal(t["H"].grad, t["H"].grad.transpose(1, 2))


def test_qp_layer_unsolved_instance_gives_zero_gradient(gpu_device):
    p, _, gx = layer_problem()
    t = tensors(p)
    for k in ("H", "g", "A", "lA", "uA", "l", "u"):
        t[k].requires_grad_(True)
    ws = torch_api.qp_sens_workspace(p["B"], p["n"], p["nc"])
    x = torch_api.qp_layer(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], max_iter=1, workspace=ws)
    (x * torch.from_numpy(gx).cuda()).sum().backward()
    last = torch_api.qp_layer.last
    failed = last.status != abi.STATUS_SOLVED
    assert torch.any(last.status == abi.STATUS_MAX_ITER)
    assert torch.all(last.flag[failed] == R.SKIPPED)
    for k in ("H", "g", "A", "lA", "uA", "l", "u"):
        assert torch.all(t[k].grad[failed] == 0.0) and torch.all(torch.isfinite(t[k].grad))


def test_qp_multipliers_with_a_workspace(gpu_device):
    """shapes, dtypes and the reference's set at (65, 40); without the keyword the call is refused as before, and the text names it"""
    p, x, y_ref, _ = fixture()[0]
    t = tensors(p)
    B, n, nc = p["B"], p["n"], p["nc"]
    ws = torch_api.qp_sens_workspace(B, n, nc)
    xs, status, _ = torch_api.qp_solve(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"])
    y, active, flag = torch_api.qp_multipliers(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], xs, status, workspace=ws)
    assert y.shape == (B, n + nc) and y.dtype == torch.float64 and y.is_cuda
    assert active.shape == (B, n + nc) and active.dtype == torch.int32
    assert flag.shape == (B,) and flag.dtype == torch.int32 and torch.all(flag == R.OK)
    assert np.array_equal(active.cpu().numpy(), R.reference_active(p, y_ref))
    with pytest.raises(RuntimeError, match="above 64.*workspace="):
        torch_api.qp_multipliers(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], xs, status)
    with pytest.raises(ValueError, match="64 variables.*workspace="):
        torch_api.qp_layer(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"])
    with pytest.raises(RuntimeError, match="too small"):
        torch_api.qp_multipliers(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], xs, status, workspace=ws[:-16])
    assert torch_api.qp_sens_workspace(4, 64, 10).numel() == 0


def test_graph_replay_gives_the_same_bits(gpu_device):
    """the call allocates nothing and synchronises nothing: captured into a HIP graph after one eager call, its replay gives the
    bits of the eager run"""
    p, x, _, gx = fixture()[0]
    t = tensors(p)
    xs = torch.from_numpy(x).cuda()
    ws = torch_api.qp_sens_workspace(p["B"], p["n"], p["nc"])
    call = lambda: torch_api.qp_multipliers(t["H"], t["g"], t["A"], t["lA"], t["uA"], t["l"], t["u"], xs, workspace=ws)
    eager = call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call()
    for _ in range(2):
        for o in captured:
            o.fill_(7)
        ws.fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(a, b)


# ---- 5. the small sizes through the new entry ------------------------------------------------------------------------------------------
def test_ws_entry_at_32_gives_the_bits_of_the_old_entry(gpu_device):
    """(32, 40) with a NULL workspace: the same kernel, the same bits as osot_qp_sensitivity_batch"""
    p, x, _, gx = R.fixture()[1]
    assert (p["n"], p["nc"]) == (32, 40)
    old = run_device(p, x, gx, workspace="old")
    new = run_device(p, x, gx, workspace=None)
    assert new.fences_intact()
    for k in R.Outputs.ALL:
        assert np.array_equal(getattr(old, k), getattr(new, k)), k
