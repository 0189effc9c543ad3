"""Hot start of the batched explicit QP on the device (osot_qp_solve_batch_hot, torch_api.qp_solve(hot=...)): the working sets carried
from call to call in a caller-owned state, at every size of the surface -- 65 .. 128 variables on the workgroup route
(osot_qp_big_hot_kernel), up to 64 on the wavefront route (osot_qp_kernel<NP, true>, until now reachable through the plugin only).

Problems: helpers.random_qp with g *= 4 (about half of the constraints end active), eps 1e-9.  "The same answer" is
|x_hot - x_cold| <= 1e-10 max(1, |x|), the bound tests/test_gpu_backend.py uses for a hot-started repeat."""
import ctypes as C

import numpy as np
import pytest

from opensot_amd import abi
from helpers import random_qp

pytestmark = pytest.mark.gpu
EPS = 1e-9


def _problems(n, nc, n_eq, B, seed=None):
    H, g, A, lA, uA, l, u = random_qp(np.random.default_rng(n + nc if seed is None else seed), B, n, nc, n_eq)
    return [H, g * 4.0, A, lA, uA, l, u]


def _one(args, i):
    return tuple(None if a is None else a[i] for a in args)


def _dev(args):
    import torch
    dev = torch.device("cuda", 0)
    return [None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev).contiguous() for a in args]


def _state(B, n):
    from opensot_amd import torch_api as ta
    return ta.qp_hot_state(B, n)


def _solve(ts, B, n, nc, hot=None, max_iter=0):
    """osot_qp_solve_batch (hot None) or osot_qp_solve_batch_hot on device tensors; returns numpy x, status, iterations"""
    import torch
    dev = ts[0].device
    x = torch.zeros((B, n), dtype=torch.float64, device=dev)
    st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    it = torch.zeros((B,), dtype=torch.int32, device=dev)
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = abi.lib()
    if hot is None:
        rc = L.osot_qp_solve_batch(B, n, nc, *[p(a) for a in ts], EPS, max_iter, p(x), p(st), p(it), stream)
    else:
        rc = L.osot_qp_solve_batch_hot(B, n, nc, *[p(a) for a in ts], EPS, max_iter, p(x), p(st), p(it), p(hot), stream)
    assert rc == abi.OK, L.osot_last_error()
    torch.cuda.synchronize()
    return x.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()


def _close(x, ref):
    return np.abs(x - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


def _compacted(row):
    cnt = int((row >= 0).sum())
    return (row[:cnt] >= 0).all() and (row[cnt:] == -1).all()


@pytest.mark.parametrize("n,nc,n_eq,B", [(65, 10, 2, 40), (72, 24, 4, 33), (128, 40, 0, 9), (66, 4, 1, 600)])
def test_hot_batch_wider_than_64(n, nc, n_eq, B, gpu_device):
    """B = 600: more QPs than workgroups in the launch -- the state is per instance, not per workgroup"""
    from test_qp_hot_host import as_set, big_hot_host_solve, empty_list
    args = _problems(n, nc, n_eq, B)
    ts = _dev(args)
    xc, stc, itc = _solve(ts, B, n, nc)
    assert (stc == 0).all()
    hot = _state(B, n)
    assert tuple(hot.shape) == (B, 128)
    x1, st1, it1 = _solve(ts, B, n, nc, hot)
    assert np.array_equal(x1, xc) and np.array_equal(st1, stc) and np.array_equal(it1, itc), "an empty state is the cold call, bit for bit"
    rec1 = hot.cpu().numpy().copy()
    assert all(_compacted(r) for r in rec1) and ((rec1 >= 0).sum(axis=1) <= n).all()
    x2, st2, it2 = _solve(ts, B, n, nc, hot)
    rec2 = hot.cpu().numpy()
    print(f"n={n} nc={nc} B={B}: iterations cold mean {itc.mean():.1f} max {itc.max()}, hot mean {it2.mean():.1f} max {it2.max()}")
    assert (st2 == 0).all()
    for i in range(B):
        assert _close(x2[i], xc[i]), i
    assert (it2 <= itc).all() and it2.sum() < itc.sum()
    for i in range(0, B, max(1, B // 8)):          # the same source on the host, one thread: same path
        q = _one(args, i)
        sth, xh, ith, rech = big_hot_host_solve(*q, EPS, empty_list())
        assert sth == 0 and ith == it1[i] and as_set(rech) == as_set(rec1[i])
        sth, xh, ith, rech2 = big_hot_host_solve(*q, EPS, rech)
        assert sth == 0 and ith == it2[i] and as_set(rech2) == as_set(rec2[i])
        assert _close(x2[i], xh)


@pytest.mark.parametrize("n,nc", [(24, 10), (36, 12), (50, 14)])
def test_hot_batch_up_to_64(n, nc, gpu_device):
    """the wavefront route through the new entry; instance 0 is what the plugin (BackEnd: the same kernel with a batch of one and a
    state of its own) computes on the same problem, cold and hot -- same code, same input, same bits"""
    from opensot_amd.solver import BackEnd
    B = 64
    args = _problems(n, nc, 2, B)
    ts = _dev(args)
    xc, stc, itc = _solve(ts, B, n, nc)
    assert (stc == 0).all()
    hot = _state(B, n)
    assert tuple(hot.shape) == (B, 32 if n <= 32 else 64)
    x1, st1, it1 = _solve(ts, B, n, nc, hot)
    assert np.array_equal(it1, itc) and all(_close(x1[i], xc[i]) for i in range(B))     # (two instantiations: the same path)
    x2, st2, it2 = _solve(ts, B, n, nc, hot)
    print(f"n={n} nc={nc} B={B}: iterations cold {itc.sum()}, hot {it2.sum()}; empty state bit-identical to cold: {np.array_equal(x1, xc)}")
    assert (st2 == 0).all()
    for i in range(B):
        assert _close(x2[i], xc[i]), i
    assert it2.sum() < itc.sum()
    qp = BackEnd(n, nc, abi.HST_SEMIDEF, 1.0)
    assert qp.setEpsRegularisation(EPS)
    assert qp.initProblem(*_one(args, 0))
    assert np.array_equal(qp.getSolution(), x1[0]) and qp.getOptions()["last_iterations"] == it1[0]
    assert qp.solve()
    assert np.array_equal(qp.getSolution(), x2[0]) and qp.getOptions()["last_iterations"] == it2[0]


def test_failed_instance_leaves_no_state(gpu_device):
    """33 QPs of 72 variables, the one in the middle infeasible (two contradictory equality rows): its state comes back empty, and
    the others are what they are in the batch without it"""
    n, nc, n_eq, B, bad = 72, 24, 4, 33, 16
    args = _problems(n, nc, n_eq, B)
    args[2][bad, 1] = args[2][bad, 0]
    args[3][bad, 1] = args[4][bad, 1] = args[3][bad, 0] + 1.0
    keep = [i for i in range(B) if i != bad]
    ts, ts_good = _dev(args), _dev([a[keep] for a in args])
    hot, hot_good = _state(B, n), _state(B - 1, n)
    for cycle in range(2):
        x, st, it = _solve(ts, B, n, nc, hot)
        xg, stg, itg = _solve(ts_good, B - 1, n, nc, hot_good)
        rec, recg = hot.cpu().numpy(), hot_good.cpu().numpy()
        assert st[bad] == 1 and not x[bad].any() and (rec[bad] == -1).all()
        assert (stg == 0).all() and np.array_equal(st[keep], stg)
        assert np.array_equal(x[keep], xg) and np.array_equal(it[keep], itg) and np.array_equal(rec[keep], recg)
    # every instance at the iteration cap: nothing recorded either
    x, st, it = _solve(ts_good, B - 1, n, nc, hot_good, max_iter=2)
    assert (st == 2).all() and (hot_good.cpu().numpy() == -1).all()


def test_torch_api_hot_over_drifting_cycles(gpu_device):
    import torch
    from opensot_amd import torch_api as ta
    n, nc, n_eq, B = 72, 24, 4, 33
    factor = EPS / 2.221e-13
    args = _problems(n, nc, n_eq, B)
    H, g, A, lA, uA, l, u = _dev(args)
    hot = ta.qp_hot_state(B, n)
    assert hot.dtype == torch.int32 and tuple(hot.shape) == (B, 128) and bool((hot == -1).all())
    gen = torch.Generator(device="cpu").manual_seed(3)
    tot_hot = tot_cold = 0
    for cycle in range(4):          # (cycle 0 fills the state)
        if cycle:
            g = g * (1.0 + 0.01 * torch.randn(g.shape, generator=gen, dtype=torch.float64).to(g.device))
        xc, stc, itc = ta.qp_solve(H, g, A, lA, uA, l, u, eps_regularisation=factor)
        xh, sth, ith = ta.qp_solve(H, g, A, lA, uA, l, u, eps_regularisation=factor, hot=hot)
        torch.cuda.synchronize()
        assert bool((stc == 0).all()) and bool((sth == 0).all())
        xc, xh = xc.cpu().numpy(), xh.cpu().numpy()
        for i in range(B):
            assert _close(xh[i], xc[i]), (cycle, i)
        if cycle:
            tot_hot += int(ith.sum()); tot_cold += int(itc.sum())
    print(f"three drifting cycles, n={n} B={B}: iterations hot {tot_hot}, cold {tot_cold}")
    assert tot_hot < tot_cold
    with pytest.raises(TypeError):
        ta.qp_solve(H, g, A, lA, uA, l, u, hot=hot.to(torch.int64))
    with pytest.raises(TypeError):
        ta.qp_solve(H, g, A, lA, uA, l, u, hot=hot.cpu())
    with pytest.raises(ValueError):
        ta.qp_solve(H, g, A, lA, uA, l, u, hot=hot[:, :64].contiguous())
    with pytest.raises(ValueError):
        ta.qp_solve(H, g, A, lA, uA, l, u, hot=hot[: B - 1].contiguous())
    with pytest.raises(ValueError):
        ta.qp_solve(H[:, :40, :40].contiguous(), g[:, :40].contiguous(), be_solver=ta.solver_back_ends.OSQP, hot=ta.qp_hot_state(B, 40))
    with pytest.raises(ValueError, match="hot"):
        ta.qp_solve(H[:, :40, :40].contiguous(), g[:, :40].contiguous(), warm=ta.admm_state(B, 40, 0, box=False))
