"""The force-space row producer on the device: osot_force_rows against its host emulation and the numpy restatement
(tests/force_ref.py) at the shapes where the kernel can go wrong, the three synth force stacks through BatchedStack.cycle against the
oracle's cascade, and dynamics.ForceStep (three eager steps, then a captured graph)."""
import ctypes as C

import numpy as np
import pytest
import torch

from opensot_amd import abi, synth
from opensot_amd.dynamics import ForceStep
from oracle import pyoracle

import force_ref as fr
from surface_ref import generic_twin
from test_force_rows_host import check_b
from test_force_stacks_host import STACKS
from test_wide_plan_host import _pick, _witnesses, close, oracle_solve

pytestmark = pytest.mark.gpu


def run_device(case, ld):
    """the case through osot_force_rows on cuda:0 -> Outputs (downloaded)"""
    out = fr.Outputs(case, ld)
    dev = {}

    def address(a):
        if id(a) not in dev:
            dev[id(a)] = (torch.as_tensor(a).to("cuda:0").contiguous(), a)
        return dev[id(a)][0].data_ptr()
    m, b = fr.structs(case, out, address)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().osot_force_rows(C.byref(m), C.byref(b), st), "osot_force_rows")
    torch.cuda.synchronize()
    for host in out.arrays().values():
        if id(host) in dev:
            host[...] = dev[id(host)][0].cpu().numpy()
    return out


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_device_against_emulation(shape, B, gpu_device):
    case, ld = fr.shape_case(shape, B, seed=100 + B)
    emu, got = fr.run_host(case, ld), run_device(case, ld)
    na = case["nv"] - 6
    # matrices and the static bounds: copies, transposes, negations, one subtraction per entry -- the same bits, and the sentinels
    # of every entry that is not written (rows and columns between the blocks, gaps between instances) still in place
    for name in ("com_A", "fb_A", "static_A", "static_lo", "static_up"):
        assert np.array_equal(getattr(got, name), getattr(emu, name)), name
    for name, ref, rows, static in (("com_A", fr.com_A(case), 6, False), ("fb_A", fr.fb_A(case), 6, False),
                                    ("static_A", fr.static_A(case), na, True)):
        cols = fr.written_columns(case, static)
        a = getattr(got, name).copy()
        assert np.array_equal(a[:, 1:1 + rows, cols], ref[:, :, cols]), name
        a[:, 1:1 + rows, cols] = fr.SENTINEL
        assert (a == fr.SENTINEL).all(), name
    # every b: the host's bound, against the longdouble evaluation; around them the sentinels
    lin, ang = fr.com_b_terms(case)
    check_b(got.com_b[:, 1:4], lin, "com_b linear")
    check_b(got.com_b[:, 4:7], ang, "com_b angular")
    check_b(got.cart_b[:, 1:7], fr.cart_b_terms(case), "cart_b")
    for name in ("com_b", "cart_b"):
        a = getattr(got, name)
        assert (a[:, 0] == fr.SENTINEL).all() and (a[:, 7] == fr.SENTINEL).all(), name
        print(f"{name}: device and emulation differ in {int((a != getattr(emu, name)).sum())} entries")


def test_device_orientation_error_is_the_restated_sequence(gpu_device):
    """Kp = I, Kd = 0: cart_b is e; the quaternion error is compiled without contraction, so the device gives the restatement's bits"""
    case, ld = fr.shape_case("C3_nv35", 65, seed=5)
    case["cart_Kp"], case["cart_Kd"], case["cart_f_des"] = np.eye(6), np.zeros((6, 6)), None
    assert np.array_equal(run_device(case, ld).cart_b[:, 1:7], fr.pose_error(case))


def test_device_refuses_what_the_host_refuses(gpu_device):
    case, ld = fr.shape_case("C3_nv35", 2, seed=0)
    out = fr.Outputs(case, ld)
    m, b = fr.structs(case, out, lambda a: a.ctypes.data)      # (never launched: the check comes first)
    m.n_contacts = 9
    assert abi.lib().osot_force_rows(C.byref(m), C.byref(b), None) == abi.ERR_INVALID
    assert b"n_contacts is outside 1 .. 8" in abi.lib().osot_last_error()


# ---- the synth stacks: producers + osot_force_rows + osot_cycle against the oracle's cascade -------------------------------------------
def device_leaf(step, leaf):
    """the leaf as the device assembled it: every force block downloaded from where osot_force_rows wrote it"""
    f, B = leaf["force"], leaf["B"]
    full = dict(leaf)
    full["A"] = [None if a is None else a[:B].cpu().numpy() for a in step.st.A]
    full["task"] = [list(lev) for lev in leaf["task"]]
    full["task"][f["task"][0]][f["task_index"]] = (step.b0[:B].cpu().numpy(), None, None)
    full["rows"] = list(leaf["rows"])
    if f["static_block"] is not None:
        full["rows"][f["static_block"]] = tuple(t[:B].cpu().numpy() for t in step.dev["rows"][f["static_block"]])
    return full


@pytest.fixture(scope="module", params=STACKS, ids=[s[0] for s in STACKS])
def stepped(request, gpu_device):
    name, make, B = request.param
    plan, leaf, model = make(B)
    step = ForceStep(plan, leaf, model, device=0)
    xs = []
    for _ in range(3):
        step.step()
        torch.cuda.synchronize()
        xs.append(step.st.dq[:B].cpu().numpy())
    return name, plan, leaf, model, step, xs


def test_force_blocks_match_the_host_assembly(stepped):
    """what the three launches wrote is the host assembly of the same stack: bit for bit where the quantities are the stack's own,
    to the producers' round-off (1e-12 of a Jacobian entry, a lever arm, a gravity torque) where they come from the tree"""
    name, plan, leaf, model, step, xs = stepped
    host, _ = fr.assemble_stack(plan, leaf, model)
    dev = device_leaf(step, leaf)
    f = leaf["force"]
    pairs = [(dev["A"][0], host["A"][0]), (dev["task"][0][0][0], host["task"][0][0][0])]
    if f["static_block"] is not None:
        pairs += list(zip(dev["rows"][f["static_block"]], host["rows"][f["static_block"]]))
    for d, h in pairs:
        if model is None:
            assert np.array_equal(d, h)
        else:
            assert np.abs(d - h).max() <= 1e-12 * max(1.0, np.abs(h).max())
    assert np.array_equal(dev["A"][1], host["A"][1])      # force::Wrenches: the constant selection, untouched


def test_stack_parity_with_the_oracle(stepped):
    from helpers import answer_is_acceptable
    name, plan, leaf, model, step, xs = stepped
    B = leaf["B"]
    assert step.st.route == ("wide" if plan.n > 64 else "wavefront")
    assert (step.st.status[:B].cpu().numpy() == 0).all()
    twin, tleaf = generic_twin(plan, device_leaf(step, leaf))
    asm = pyoracle.assemble(twin, tleaf)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all()
    x = xs[-1]
    for i in range(B):
        if close(x[i], ref["dq"][i]):
            continue
        sub = _pick(asm, i)
        ok, why = answer_is_acceptable(sub, 0, x[i], [(nm, r["dq"][0], r["status"][0] == 1) for nm, r in _witnesses(sub)])
        assert ok, (i, why)


def test_three_steps_and_level_zero(stepped):
    """three eager steps give one answer (the stack is at rest), and level 0 holds: |G x - b| of force::CoM / force::FloatingBase is
    within the residual the oracle's own solution of the same data shows (the regularisation's), plus the forward-error bound of
    the product G x"""
    name, plan, leaf, model, step, xs = stepped
    B = leaf["B"]
    assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[1], xs[2])
    twin, tleaf = generic_twin(plan, device_leaf(step, leaf))
    asm = pyoracle.assemble(twin, tleaf)
    ref = oracle_solve(asm)
    G, b = asm["A"][0].astype(np.longdouble), asm["b"][0].astype(np.longdouble)
    r_dev = np.abs(np.einsum("brn,bn->br", G, xs[-1].astype(np.longdouble)) - b)
    r_ref = np.abs(np.einsum("brn,bn->br", G, ref["dq"].astype(np.longdouble)) - b)
    bound = (plan.n + 2) * fr.U * np.einsum("brn,bn->br", np.abs(G), np.abs(xs[-1]).astype(np.longdouble))
    print(f"{name}: max |G x - b| device {float(r_dev.max()):.6e}, oracle {float(r_ref.max()):.6e}, forward-error bound {float(bound.max()):.3e}")
    assert (r_dev.max(axis=1) <= r_ref.max(axis=1) + bound.max(axis=1)).all()


def test_captured_graph_replays_to_the_same_bits(stepped):
    name, plan, leaf, model, step, xs = stepped
    B = leaf["B"]
    s = torch.cuda.Stream()
    step.st.stream = s
    with torch.cuda.stream(s):
        step.step()
    torch.cuda.synchronize()
    eager = step.st.dq.clone()
    assert np.array_equal(eager[:B].cpu().numpy(), xs[-1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step.step()
    step.st.dq.zero_()
    step.st.A[0].zero_()          # the force block's rows: rewritten inside the graph
    step.b0.zero_()
    g.replay()
    torch.cuda.synchronize()
    step.st.stream = None
    assert torch.equal(eager, step.st.dq)
