"""The posture-gradient producer on the device (osot_posture_gradient, opensot_amd/csrc/osot_grad.h): parity with the reference's loop by
brute force (tests/gradient_ref.py) at the shapes of the host tests and at B = 257, the output written straight into the leaf of the
block that carries the task (bit-identical assembled b_k on the Postural and on the Generic route, 64-lane and wide solver), graph
capture, the closed loops of the reference's own tests (TestMinimumEffort.cpp:121-171, TestManipulability.cpp:111-219) and one
whole solve against the oracle.

The tolerance is the host tests' constant (gradient_cases.PARITY_TOL: 10 x the worst deviation from the long-double arbiter, measured
on the host; unit: |lambda| x the cancellation scale of the instance).  The device's FMA contraction differs from the host build by
rounding only.  The restatement runs its "batched" engine here (one pass over all 2 n B perturbed postures; the host tests pin it to
oracle.pykin.forward): 2 n B calls of pykin.forward take 5 .. 50 s per shape."""
import numpy as np
import pytest
import torch

from opensot_amd import abi, synth
from opensot_amd import kinematics as kin
from opensot_amd.gradient import PostureGradient
from opensot_amd.solver import BatchedStack
from oracle import pykin, pyoracle

import gradient_cases as gc
import gradient_ref as gref
from test_wide_plan_host import _pick, _witnesses, close, oracle_solve

pytestmark = pytest.mark.gpu
F64 = dict(dtype=torch.float64, device="cuda:0")
# W_diag scale of the minimum-effort loop: the reference's own 1e-5 I (TestMinimumEffort.cpp:104).  With it the numpy restatement driving
# the oracle solver lowers the effort in every one of the 200 cycles (per-cycle decrease >= 2e-7 of an effort of 0.95) -- verified on
# the CPU; 3e-6 and 1e-6 do as well
EFFORT_W_SCALE = 1e-5
# cycles of the manipulability loop: with the restatement driving the oracle solver on the CPU the indices rise from 0.0797 .. 0.0839 to
# 0.0829 .. 0.0871 within 40 cycles (the steps fall below 1.1e-3 by then) and the wrists stay within 1e-7 of their start
MANIP_CYCLES = 40


def run_producer(model, terms, q, pad=0):
    """osot_posture_gradient on the device -> (b [T][B][n], value [T][B]) as numpy; pad: extra columns around every b (they must stay)"""
    B, n = q.shape
    T = len(terms)
    g = PostureGradient(model, terms, device=0, gravity=gc.GRAVITY)
    qd = torch.as_tensor(q, **F64).contiguous()
    outs = [torch.full((B, n + 2 * pad), 7.0, **F64) for _ in range(T)]
    vals = [torch.full((B,), 7.0, **F64) for _ in range(T)]
    g.forward(qd, b={t: (outs[t], pad) for t in range(T)}, value={t: vals[t] for t in range(T)})
    torch.cuda.synchronize()
    full = np.stack([o.cpu().numpy() for o in outs])
    if pad:
        assert np.all(full[:, :, :pad] == 7.0) and np.all(full[:, :, pad + n:] == 7.0)
    return full[:, :, pad:pad + n], np.stack([v.cpu().numpy() for v in vals])


@pytest.mark.parametrize("name", gc.SHAPES)
def test_parity_with_the_restatement_gpu(name, gpu_device):
    m, terms, q = gc.case(name)
    b, value = run_producer(m, terms, q, pad=3 if name == "chain7" else 0)
    ref = gc.reference(name, "batched")
    dev, vdev = gc.deviation(b, ref), gc.value_deviation(value, ref)
    print(f"{name}: b {dev}  value {vdev}")
    assert (dev <= gc.PARITY_TOL).all(), (name, dev)
    assert (vdev <= gc.PARITY_TOL).all(), (name, vdev)


def test_parity_odd_batch_of_257_gpu(gpu_device):
    """every instance of an odd batch beyond one wavefront's worth of workgroups"""
    m, terms, q = gc.case("humanoid32_b257")
    assert q.shape[0] == 257
    b, value = run_producer(m, terms, q)
    ref = gc.reference("humanoid32_b257", "batched")
    per_instance = np.array([np.abs(b[t] - ref["b"][t]).max(axis=1) / (abs(ref["lam"][t]) * ref["scale"][t]) for t in range(len(terms))])
    print(f"B = 257: worst per term {per_instance.max(axis=1)}")
    assert (per_instance <= gc.PARITY_TOL).all(), np.argwhere(per_instance > gc.PARITY_TOL)
    assert (gc.value_deviation(value, ref) <= gc.PARITY_TOL).all()


# ---- wiring: the producer's b is the assembled b_k, bit for bit ------------------------------------------------------------------------
def effort_setup(B, route="auto"):
    plan, leaf, model, terms = synth.make_min_effort_stack(B, seed=3, w_scale=EFFORT_W_SCALE)
    st = BatchedStack(plan, B, device=0, route=route)
    g = PostureGradient(model, terms, device=0, gravity=gc.GRAVITY)
    dev, gb, _, q = synth.bind_posture_gradient(st, g, leaf)
    return plan, leaf, model, terms, st, g, dev, gb, q


def manip_setup(B, route="auto"):
    plan, leaf, model, terms = synth.make_coman_manipulability_stack(B, seed=4)
    st = BatchedStack(plan, B, device=0, route=route, want_levels=False)
    K = kin.Kinematics(model, device=0)
    g = PostureGradient(model, terms, device=0, gravity=gc.GRAVITY)
    dev, gb, kb, q = synth.bind_posture_gradient(st, g, leaf, kin=K)
    return plan, leaf, model, terms, st, g, K, dev, gb, kb, q


@pytest.mark.parametrize("route", ["wavefront", "wide"])
def test_assembled_b_is_the_producers_output_gpu(route, gpu_device):
    B = 5
    # Postural route: p1 = p0 = q, p2 = the producer's b
    plan, leaf, model, terms, st, g, dev, gb, q = effort_setup(B, route)
    assert st.route == route
    dense = torch.zeros((B, model.n), **F64)
    g.forward(q, b={0: dense})
    g.forward(q, batch=gb)                               # straight into the leaf array
    st.b[0].fill_(7.0)
    st.update(dev)
    torch.cuda.synchronize()
    assert dense.abs().max() > 0 and torch.equal(dev["task"][0][0][2], dense)
    assert torch.equal(st.b[0][:B], dense)
    # Generic route: stored unit rows next to an implicit Postural block
    plan, leaf, model, terms, st, g, K, dev, gb, kb, q = manip_setup(B, route)
    n = model.n
    dl, dr = torch.zeros((B, n), **F64), torch.zeros((B, n), **F64)
    g.forward(q, b={0: dl, 1: dr})
    g.forward(q, batch=gb)
    st.b[1].fill_(7.0)
    st.update(dev)
    torch.cuda.synchronize()
    assert dl.abs().max() > 0 and dr.abs().max() > 0 and not torch.equal(dl, dr)
    assert torch.equal(st.b[1][:B, :n], dl) and torch.equal(st.b[1][:B, n:2 * n], dr)
    assert torch.equal(st.b[1][:B, 2 * n:], torch.zeros((B, n), **F64))      # the Postural block: lambda (q_ref - q) at the start
    assert torch.equal(st.A[1][:B, :n], torch.eye(n, **F64).expand(B, n, n)) and torch.equal(st.A[1][:B, n:], st.A[1][:B, :n])


def test_graph_capture_replays_the_same_bits_gpu(gpu_device):
    m, terms, q = gc.case("coman35")
    B, n = q.shape
    g = PostureGradient(m, terms, device=0, gravity=gc.GRAVITY)
    qd = torch.as_tensor(q, **F64).contiguous()
    outs = [torch.zeros((B, n), **F64) for _ in terms]
    vals = [torch.zeros((B,), **F64) for _ in terms]
    gb = g.batch_args(qd, b=dict(enumerate(outs)), value=dict(enumerate(vals)))
    g.forward(qd, batch=gb)
    torch.cuda.synchronize()
    want = [t.clone() for t in outs + vals]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.forward(qd, batch=gb)                          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g.forward(qd, batch=gb)
    for t in outs + vals:
        t.fill_(-3.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(want, outs + vals):
        assert torch.equal(a, b)


# ---- closed loops ------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_minimum_effort_gpu(gpu_device):
    """TestMinimumEffort.cpp:121-171 on COMAN: producer -> osot_cycle -> q += dq; the effort never rises, and ends below its start"""
    B, cycles = 4, 200
    plan, leaf, model, terms, st, g, dev, gb, q = effort_setup(B)
    eff = torch.zeros((cycles + 1, B), **F64)
    b = dev["task"][0][0][2]
    batches = [g.batch_args(q, b={0: b}, value={0: eff[c]}) for c in range(cycles + 1)]
    for c in range(cycles):
        g.forward(q, batch=batches[c])
        st.cycle(dev)
        q.add_(st.dq[:B])
    g.forward(q, batch=batches[cycles])
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all()
    e = eff.cpu().numpy()
    print(f"effort: start {e[0]}  end {e[-1]}  largest step {np.diff(e, axis=0).max():.3e}")
    assert (np.diff(e, axis=0) <= 0.0).all()
    assert (e[-1] < e[0]).all()
    want = gref.costs(model, q.cpu().numpy(), terms, gc.GRAVITY)[0]
    assert (np.abs(e[-1] - want) <= gc.PARITY_TOL * np.abs(want)).all()


def test_closed_loop_manipulability_gpu(gpu_device):
    """TestManipulability.cpp:111-219 on COMAN: the wrists (relative to the waist) hold their poses while the bottom level climbs the two
    manipulability indices: producer -> osot_control_cycle (kinematics, update, cascade, q += dq) per cycle"""
    B = 4
    plan, leaf, model, terms, st, g, K, dev, gb, kb, q = manip_setup(B)
    idx = torch.zeros((2, 2, B), **F64)
    first = g.batch_args(q, b={0: dev["task"][1][0][0], 1: dev["task"][1][1][0]}, value={0: idx[0, 0], 1: idx[0, 1]})
    last = g.batch_args(q, value={0: idx[1, 0], 1: idx[1, 1]})
    poses0 = [dev["task"][0][i][0].clone() for i in range(2)]
    for c in range(MANIP_CYCLES):
        g.forward(q, batch=first if c == 0 else gb)
        st.control_cycle(K, kb, dev, q_integrate=q)
    g.forward(q, batch=last)
    K.forward(q, frame_pose={f: dev["task"][0][i][0] for i, f in enumerate(leaf["state"]["frames"])})
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all()
    i0, i1 = idx[0].cpu().numpy(), idx[1].cpu().numpy()
    moved = max((dev["task"][0][i][0] - poses0[i]).abs().max().item() for i in range(2))
    print(f"index: start {i0.tolist()}  end {i1.tolist()}  wrists moved {moved:.3e}  max|q - q0| {np.abs(q.cpu().numpy() - leaf['state']['q0']).max():.3e}")
    assert moved <= 1e-3
    assert (i1 >= i0).all()
    assert (i1 > i0).any()


# ---- one whole solve against the oracle ---------------------------------------------------------------------------------------------------
def accept(asm, dq, ref):
    """the suite's rule (tests/test_limit_kinds_gpu.py): the parity tolerance, or the lexicographic rule against the witnesses"""
    from helpers import answer_is_acceptable
    for i in range(asm["B"]):
        if close(dq[i], ref["dq"][i]):
            continue
        sub = _pick(asm, i)
        ok, why = answer_is_acceptable(sub, 0, dq[i], [(nm, r["dq"][0], r["status"][0] == 1) for nm, r in _witnesses(sub)])
        assert ok, (i, why)


def test_solve_parity_minimum_effort_gpu(gpu_device):
    B = 4
    plan, leaf, model, terms, st, g, dev, gb, q = effort_setup(B)
    g.forward(q, batch=gb)
    st.cycle(dev)
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all()
    ref_b = gref.gradients(model, leaf["state"]["q0"], terms, gc.GRAVITY, np.float64, "batched")["b"][0]
    leaf["task"][0][0] = (leaf["state"]["q0"], leaf["state"]["q0"], np.ascontiguousarray(ref_b))
    asm = pyoracle.assemble(plan, leaf)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all()
    dq = st.dq[:B].cpu().numpy()
    print(f"max|dq - dq_oracle| = {np.abs(dq - ref['dq']).max():.3e}  max|dq| = {np.abs(dq).max():.3e}")
    accept(asm, dq, ref)


def test_solve_parity_manipulability_gpu(gpu_device):
    B = 4
    plan, leaf, model, terms, st, g, K, dev, gb, kb, q = manip_setup(B)
    g.forward(q, batch=gb)
    st.control_cycle(K, kb, dev)
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all()
    # the same cycle on the CPU: oracle.pykin for the wrists, the restatement for the two b, the oracle for the solve
    q0, (fl, fr), fw = leaf["state"]["q0"], leaf["state"]["frames"], model.frame_index("Waist")
    poses, J = [[], []], []
    for i in range(B):
        fk = pykin.forward(model, q0[i])
        rows = []
        for k, f in enumerate((fl, fr)):
            R, p, Jr = pykin.relative(fk, f, fw)
            poses[k].append(np.concatenate([R.reshape(9), p])); rows.append(Jr)
        J.append(np.concatenate(rows, axis=0))
    ref_b = gref.gradients(model, q0, terms, gc.GRAVITY, np.float64, "batched")["b"]
    leaf["A"][0] = np.array(J)
    for k in range(2):
        leaf["task"][0][k] = (np.array(poses[k]), np.array(poses[k]), None)
        leaf["task"][1][k] = (np.ascontiguousarray(ref_b[k]), None, None)
    asm = pyoracle.assemble(plan, leaf)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all()
    dq = st.dq[:B].cpu().numpy()
    print(f"max|dq - dq_oracle| = {np.abs(dq - ref['dq']).max():.3e}  max|dq| = {np.abs(dq).max():.3e}")
    accept(asm, dq, ref)
