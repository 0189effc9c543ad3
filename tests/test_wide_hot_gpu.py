"""Hot start of the working sets on the wide route, on the GPU: osot_ihqp_solve_hot / osot_cycle_hot (osot_cascade_wide_hot_kernel,
opensot_amd/csrc/osot_cascade_wide.h) with a caller-owned state against the cold calls of the same handle, the oracle, a batch larger
than the grid (the state is indexed by the instance) and a captured graph.  The CPU side of the same source: test_wide_hot_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from opensot_amd import abi
from opensot_amd.solver import BatchedStack, _stream_ptr
from oracle import pyoracle

import test_surface_contact_host as surf
from test_wide_plan_host import close, generic_wide, oracle_solve
from wide_hot_ref import HOT_LEN, drifted, scaled_diff, tight_stack

pytestmark = pytest.mark.gpu

# Worst scaled |dq_hot - dq_cold| with every list at -1 against the cold call, MI355X (test_empty_lists_against_the_cold_call prints
# it per fixture): 0 on all four fixtures -- the hot kernel from empty lists gives the cold kernel's bits.
HOT_VS_COLD_DEVICE_MEASURED = 0.0
HOT_VS_COLD_DEVICE = min(100 * HOT_VS_COLD_DEVICE_MEASURED, 1e-8)

FIXTURES = ["surface68", "tight72", "generic128", "generic20"]
FEWER = ("surface68", "tight72")


@functools.lru_cache(maxsize=None)
def fixture(name):
    if name == "surface68":
        plan, leaf = surf.stack(3, 68, 69)
        return plan, surf._assembled(plan, leaf)
    if name == "tight72":
        plan, leaf = tight_stack(4)
    elif name == "generic128":
        plan, leaf = generic_wide(4, 128, seed=128)
    else:
        plan, leaf = generic_wide(4, 20, seed=3, level_rows=[4, 6], n_eq=2, n_ineq=6, n_local=2)
    return plan, pyoracle.assemble(plan, leaf)


def results(st, B):
    torch.cuda.synchronize()
    return (st.dq[:B].cpu().numpy(), st.x_levels[:B].cpu().numpy(), st.status[:B].cpu().numpy(),
            st.iterations[:B].cpu().numpy(), st.accepted_slack[:B].cpu().numpy())


def solve(st, B, hot=None):
    for t in (st.dq, st.x_levels, st.accepted_slack):
        t.fill_(float("nan"))
    st.status.fill_(-1); st.iterations.fill_(-1)
    st.solve(B, hot=hot)
    return results(st, B)


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- (a) (b) the cold kernel through the new entry; empty lists ---------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_null_state_is_the_cold_call(name, gpu_device):
    plan, asm = fixture(name)
    B = asm["B"]
    st = BatchedStack(plan, B, device=0, route="wide")
    st.load_assembled(asm)
    cold = solve(st, B)
    for t in (st.dq, st.x_levels):
        t.fill_(float("nan"))
    qb = st._qp_batch(B)
    abi.check(abi.lib().osot_ihqp_solve_hot(st._h, C.byref(qb), None, _stream_ptr(st.device)), "osot_ihqp_solve_hot")
    assert (cold[2] == 0).all()
    assert same_bits(results(st, B), cold)


@pytest.mark.parametrize("name", FIXTURES)
def test_empty_lists_against_the_cold_call(name, gpu_device):
    plan, asm = fixture(name)
    B = asm["B"]
    st = BatchedStack(plan, B, device=0, route="wide")
    st.load_assembled(asm)
    cold = solve(st, B)
    state = st.hot_state()
    assert state.shape == (B, plan.L * HOT_LEN) and state.dtype == torch.int32 and bool((state == -1).all())
    hot = solve(st, B, hot=state)
    d = max(scaled_diff(hot[0], cold[0]), scaled_diff(hot[1], cold[1]))
    print(f"{name}: scaled |hot - cold| from empty lists {d:.3g}; bit-identical: {same_bits(hot, cold)}")
    assert np.array_equal(hot[2], cold[2]) and np.array_equal(hot[3], cold[3]) and (hot[2] == 0).all()
    assert d <= HOT_VS_COLD_DEVICE
    assert bool((state >= 0).any())      # (something was recorded)


# ---- (c) exact repeat and three drifted cycles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_repeat_and_drifted_cycles(name, gpu_device):
    plan, asm = fixture(name)
    B = asm["B"]
    st = BatchedStack(plan, B, device=0, route="wide")
    state = st.hot_state(B)
    for step, cycle in enumerate((0, 0, 1, 2, 3)):
        a = drifted(asm, cycle)
        st.load_assembled(a)
        cold = solve(st, B)
        dq, xl, status, it, slack = solve(st, B, hot=state)
        print(f"{name} step {step}: cold {cold[3].tolist()} hot {it.tolist()} scaled |hot - cold| {scaled_diff(dq, cold[0]):.3g}")
        assert (status == 0).all() and (cold[2] == 0).all()
        assert close(dq, cold[0])       # (two solves of one strictly convex problem: the parity rule the oracle checks below use)
        if step == 0:
            continue
        if name.startswith("surface"):
            surf._judge(a, dq, status)
        elif name == "tight72":        # (the eiQuadProg restatement stops on this stack; the reference's qpOASES solves it)
            if pyoracle.ref_available():
                rq = pyoracle.ihqp_solve_batch(a, pyoracle.BE_QPOASES_REF, nthreads=1)
                assert (rq["status"] == 1).all() and close(dq, rq["dq"], 1e-9)
            else:
                print(f"{name}: the reference's qpOASES build is absent -- this stack's hot answers are judged against the cold call alone")
        else:
            ref = oracle_solve(a)
            assert (ref["status"] == 1).all() and close(dq, ref["dq"]) and close(xl, ref["x_levels"])
        if step == 1:
            assert (it <= cold[3]).all()
            if name in FEWER:
                assert (it < cold[3]).all()


# ---- (d) more instances than workgroups: the state belongs to the instance ---------------------------------------------------------
def tiled(asm, B):
    reps = -(-B // asm["B"])
    t = lambda a: None if a is None else np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:B])
    out = dict(asm)
    out["B"] = B
    for k in ("A", "b", "w", "c"):
        out[k] = [t(a) for a in asm[k]]
    for k in ("C", "lo", "up", "l", "u"):
        out[k] = t(asm[k])
    return out


def test_state_is_indexed_by_the_instance(gpu_device):
    plan, asm = fixture("tight72")
    probe = BatchedStack(plan, 4, device=0, route="wide")
    B = probe.resident_waves() + 3
    del probe
    st = BatchedStack(plan, B, device=0, route="wide")
    assert st.resident_waves() < B
    state = st.hot_state()
    for cycle in (0, 1):
        st.load_assembled(tiled(drifted(asm, cycle), B))
        dq, _, status, it, _ = solve(st, B, hot=state)
        assert (status == 0).all()
    s = state.cpu().numpy()
    src = np.arange(B) % 4
    assert np.array_equal(dq, dq[src]) and np.array_equal(it, it[src]) and np.array_equal(s, s[src])
    assert (s >= 0).any(axis=1).all()


# ---- (e) osot_cycle_hot captured into a graph --------------------------------------------------------------------------------------
def test_cycle_hot_graph_replay_equals_plain_launches(gpu_device):
    B = 4
    plan, leaf = tight_stack(B)
    st = BatchedStack(plan, B, device=0, route="wide")
    dev = st.load_leaf(leaf)
    # the leaf buffers a cycle drifts, in place: b of the generic tasks, both bounds of the generic rows (one factor), the box
    drift_sets = [[t[0]] for lev_plan, lev in zip(plan.levels, dev["task"]) for task, t in zip(lev_plan, lev) if task.kind == abi.TASK_GENERIC]
    drift_sets += [[t[1], t[2]] for rb, t in zip(plan.rowblocks, dev["rows"]) if rb.kind == abi.ROWS_GENERIC]
    drift_sets += [[t[0], t[1]] for bd, t in zip(plan.bounds, dev["bound"]) if bd.kind == abi.BOUND_GENERIC]
    keep = [[t.clone() for t in ts] for ts in drift_sets]
    gen = torch.Generator(device="cpu").manual_seed(3)
    factors = [[(1.0 + 0.01 * (2.0 * torch.rand((B, 1), generator=gen, dtype=torch.float64) - 1.0)).to(st.device) for _ in drift_sets]
               for _ in range(3)]

    def restore():
        for ts, ks in zip(drift_sets, keep):
            for t, k in zip(ts, ks):
                t.copy_(k)

    def drift(c):
        for ts, f in zip(drift_sets, factors[c]):
            for t in ts:
                t.mul_(f)

    s = torch.cuda.Stream()
    st.stream = s
    plain, state = [], st.hot_state()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for c in range(3):
            drift(c)
            st.cycle(dev, hot=state)
            s.synchronize()
            plain.append((st.dq.clone(), st.iterations.clone(), st.status.clone(), state.clone()))
        restore()
        state.fill_(-1)
        st.cycle(dev, hot=state)            # (the kernels are loaded before the capture)
        s.synchronize()
        restore()
        state.fill_(-1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        st.cycle(dev, hot=state)
    torch.cuda.synchronize()
    assert bool((state == -1).all())        # (a capture runs nothing)
    for c in range(3):
        with torch.cuda.stream(s):
            drift(c)
            st.dq.zero_()
        s.synchronize()
        g.replay()
        torch.cuda.synchronize()
        dq, it, status, hs = plain[c]
        assert bool((status == 0).all())
        assert torch.equal(st.dq, dq) and torch.equal(st.iterations, it) and torch.equal(st.status, status) and torch.equal(state, hs)
    assert bool((plain[2][1] < plain[0][1]).all())      # (the later cycles did start hot)


# ---- (f) refusals and errors -------------------------------------------------------------------------------------------------------
def test_hot_calls_refusals(gpu_device):
    L = abi.lib()
    plan, asm = fixture("generic20")
    B = asm["B"]
    wave = BatchedStack(plan, B, device=0, route="wavefront")
    wave.load_assembled(asm)
    dev = torch.full((B, plan.L * HOT_LEN), -1, dtype=torch.int32, device=wave.device)
    qb = wave._qp_batch(B)
    v = C.c_int(0)
    stream = _stream_ptr(wave.device)
    assert L.osot_solver_hot_state_ints(wave._h, C.byref(v)) == abi.ERR_UNSUPPORTED and b"osot_solver_set_hotstart" in L.osot_last_error()
    assert L.osot_ihqp_solve_hot(wave._h, C.byref(qb), C.c_void_p(dev.data_ptr()), stream) == abi.ERR_UNSUPPORTED
    assert b"osot_solver_set_hotstart" in L.osot_last_error()
    lb, out = wave._update_args(wave.load_leaf(generic_wide(4, 20, seed=3, level_rows=[4, 6], n_eq=2, n_ineq=6, n_local=2)[1]))
    assert L.osot_cycle_hot(wave._h, C.byref(lb), C.byref(out), C.byref(qb), C.c_void_p(dev.data_ptr()), stream) == abi.ERR_UNSUPPORTED
    assert b"osot_solver_set_hotstart" in L.osot_last_error()
    with pytest.raises(RuntimeError, match="osot_solver_set_hotstart"):
        wave.hot_state()
    with pytest.raises(RuntimeError, match="osot_solver_set_hotstart"):
        wave.solve(B, hot=dev)
    torch.cuda.synchronize()
    assert bool((dev == -1).all())
    # a wide handle
    wide = BatchedStack(plan, B, device=0, route="wide")
    wide.load_assembled(asm)
    assert L.osot_solver_hot_state_ints(wide._h, C.byref(v)) == abi.OK and v.value == plan.L * HOT_LEN
    qb = wide._qp_batch(B + 1)
    big = torch.full((B + 1, plan.L * HOT_LEN), -1, dtype=torch.int32, device=wide.device)
    assert L.osot_ihqp_solve_hot(wide._h, C.byref(qb), C.c_void_p(big.data_ptr()), stream) == abi.ERR_INVALID
    assert b"max_batch" in L.osot_last_error()
    lb, out = wide._update_args(wide.load_leaf(generic_wide(4, 20, seed=3, level_rows=[4, 6], n_eq=2, n_ineq=6, n_local=2)[1]))
    lb.B = B + 1
    assert L.osot_cycle_hot(wide._h, C.byref(lb), C.byref(out), C.byref(qb), C.c_void_p(big.data_ptr()), stream) == abi.ERR_INVALID
    with pytest.raises(ValueError, match="hot_state"):
        wide.solve(B, hot=big[:, :HOT_LEN])             # one level's worth of columns
    with pytest.raises(ValueError, match="hot_state"):
        wide.solve(B, hot=big[:B - 1])                  # fewer rows than instances
    torch.cuda.synchronize()
    assert bool((big == -1).all())
