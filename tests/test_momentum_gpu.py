"""The centroidal momentum outputs of the dynamics producer on the GPU (osot_dyn_batch.cmm_lin / cmm_ang / momentum / ang_mom_b through
opensot_amd.dynamics.Dynamics): the device build against the host build of the same kernel source, the rows written straight into a
stack's A_k on both routes, graph capture, one whole solve per stack against the oracle, and the closed loops of the two momentum
stacks (synth.make_coman_momentum_stack, synth.make_coman_id_momentum_stack) with and without the momentum task.

Both closed loops were driven on the CPU first (tests/momentum_cases.py: restatements + the oracle solver, same seeds):
  velocity, B = 4, 40 cycles: max|A_ang dq| with the task at most 2.8e-11, without it at least 2.7e-5 (strictly below in every cycle
      and instance, worst ratio 2.1e-8); the soles moved 1.7e-8 / 7.8e-9
  inverse dynamics, B = 2, 30 steps: largest |angular momentum| with the block 1.2e-6, without it 1.1e-2
Measured on an MI355X: velocity 7.8e-19 .. 2.8e-11 with the task, 2.7e-5 .. 1.5e-2 without, soles moved 1.7e-8 / 7.8e-9; inverse
dynamics 1.2e-6 with the block, 1.1e-2 without; device against host build at worst 9.1e-15 (cmm_ang, humanoid32 at B = 257)."""
import numpy as np
import pytest
import torch

from opensot_amd import abi, synth
from opensot_amd.dynamics import Dynamics, IdMomentumStep
from opensot_amd.kinematics import Kinematics
from opensot_amd.plan import StackPlan, Task
from opensot_amd.solver import BatchedStack

import momentum_cases as mc
import test_momentum_host as tmh
from test_dynamics_gpu import DEVICE_TOL
from test_dynamics_host import GRAVITY, rel
from test_posture_gradient_gpu import accept
from test_wide_plan_host import oracle_solve

pytestmark = pytest.mark.gpu
F64 = dict(dtype=torch.float64, device="cuda:0")
VEL_CYCLES, ID_STEPS = 40, 30


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), **F64)


def run_device(m, q, qd, new=True, ang=None):
    """osot_dynamics with every existing output and (new=True) every momentum output -> dict of device tensors"""
    B, n, F = q.shape[0], m.n, len(m.frames)
    dyn = Dynamics(m, 0, GRAVITY)
    full = lambda *s: torch.full(s, 7.0, **F64)
    out = dict(M=full(B, n * n), h=full(B, n), jdq=full(B, 6 * max(F, 1)), com_jdq=full(B, 3), cmm_lin=full(B, 3, n), cmm_ang=full(B, 3, n),
               momentum=full(B, 6), ang_mom_b=full(B, 3))
    kw = {}
    if new:
        kw = dict(cmm_lin=out["cmm_lin"], cmm_ang=out["cmm_ang"], momentum=out["momentum"])
        if ang is not None:
            kw["ang_mom_b"] = dict(out=out["ang_mom_b"], ref=dev(ang["ref"]), rate_ref=dev(ang["rate_ref"]), K=ang["K"], lam=ang["lam"])
    dyn.forward(dev(q), dev(qd), M=out["M"], h=out["h"], frame_jdotqdot={f: (out["jdq"], 6 * f) for f in range(F)},
                com_jdotqdot=out["com_jdq"], **kw)
    torch.cuda.synchronize()
    return out


# ---- 1. device build against host build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [(nm, None) for nm in sorted(tmh.MODELS)] + [("humanoid32", 257)])
def test_device_build_against_host_build(name, B, gpu_device):
    m, q, qd, rng = tmh.sample(name, B)
    B = len(q)
    ang = dict(ref=rng.uniform(-1, 1, (B, 3)), rate_ref=rng.uniform(-3, 3, (B, 3)), K=rng.uniform(-2, 2, (3, 3)), lam=0.7)
    got, ref = run_device(m, q, qd, ang=ang), tmh.emu_momentum(m, q, qd, ang=ang)
    for k in ("cmm_lin", "cmm_ang", "momentum", "ang_mom_b"):
        d = rel(got[k].cpu().numpy(), ref[k])
        print(f"{name} B={B} {k}: device vs host rel {d:.3e}")
        assert d <= DEVICE_TOL, (name, k, d)
    plain = run_device(m, q, qd, new=False)
    for k in ("M", "h", "jdq", "com_jdq"):
        assert torch.equal(got[k], plain[k]), (name, k)             # the existing outputs do not see the new ones
    for k in ("cmm_lin", "cmm_ang", "momentum", "ang_mom_b"):
        assert torch.all(plain[k] == 7.0)


# ---- 2. rows straight into a stack --------------------------------------------------------------------------------------------------------
def velocity_setup(B, route="auto", seed=5, **kw):
    plan, leaf, model = synth.make_coman_momentum_stack(B, seed=seed, **kw)
    st = BatchedStack(plan, B, device=0, route=route, want_levels=False)
    K, D = Kinematics(model, device=0), Dynamics(model, 0, GRAVITY)
    dv, kb, db, q = synth.bind_momentum(st, K, D, leaf)
    return plan, leaf, model, st, K, D, dv, kb, db, q


def test_velocity_rows_land_in_the_stack_gpu(gpu_device):
    B = 5
    for linear in (False, True):
        plan, leaf, model, st, K, D, dv, kb, db, q = velocity_setup(B, "wavefront", linear_momentum=linear)
        assert st.route == "wavefront"
        n = model.n
        dl, da = torch.zeros((B, 3, n), **F64), torch.zeros((B, 3, n), **F64)
        D.forward(q, cmm_lin=dl, cmm_ang=da)
        st.A[1].fill_(0.0)
        dv["task"][1][0][0].copy_(dev(np.arange(3 * B).reshape(B, 3) * 0.25))       # the leaf's reference (the caller's b)
        K.forward(q, batch=kb); D.forward(q, batch=db)
        st.b[1].fill_(7.0)
        st.update(dv)
        torch.cuda.synchronize()
        assert da.abs().max() > 0 and torch.equal(st.A[1][:B], da)
        assert torch.equal(st.b[1][:B], dv["task"][1][0][0])
        if linear:
            assert torch.equal(st.A[0][:B, 12:15], dl) and torch.equal(st.b[0][:B, 12:15], torch.zeros((B, 3), **F64))
        assert st.A[0][:B, :12].abs().max() > 0                     # the soles' Jacobians are where they were


def id_step(B, seed=31, momentum=True):
    make = synth.make_coman_id_momentum_stack if momentum else synth.make_coman_id_stack
    plan, leaf, model = make(B, seed=seed)
    return IdMomentumStep(plan, leaf, model, device=0), plan, leaf, model


def test_id_rows_land_in_the_stack_gpu(gpu_device):
    B = 3
    loop, plan, leaf, model = id_step(B)
    nv, n = model.n, plan.n
    assert n == 47 and loop.st.route == "wavefront"
    loop.qdot.copy_(dev(np.random.default_rng(3).uniform(-1, 1, (B, nv))))           # so that the momentum, hence b, is not zero
    loop.L_ref.copy_(dev(np.random.default_rng(4).uniform(-1, 1, (B, 3))))
    da, db_ = torch.zeros((B, 3, nv), **F64), torch.zeros((B, 3), **F64)
    loop.dyn.forward(loop.q, loop.qdot, cmm_ang=da, ang_mom_b=dict(out=db_, ref=loop.L_ref, rate_ref=loop.Ldot_ref, K=np.eye(3), lam=1.0))
    loop.st.b[1].fill_(7.0)
    loop.produce()
    loop.st.update(loop.dev)
    torch.cuda.synchronize()
    assert da.abs().max() > 0 and db_.abs().max() > 0
    assert torch.equal(loop.st.A[1][:B, :, :nv], da) and torch.all(loop.st.A[1][:B, :, nv:] == 0.0)
    assert torch.equal(loop.st.b[1][:B], db_)
    want = loop.L_ref - loop.momentum[:, 3:]                         # lambda = 1, K = I, Ldot_d = 0
    assert (db_ - want).abs().max() <= 4 * np.spacing(want.abs().max().item())


def test_rows_land_in_a_wide_stack_gpu(gpu_device):
    """above 64 variables: synth.make_surface_id_stack (n = 68) with a 3-row momentum block appended to its first level; the tree is
    COMAN's (35 coordinates), so the rows are [A_ang 0] with 33 untouched columns"""
    B = 3
    plan0, leaf = synth.make_surface_id_stack(B, seed=9)
    n = plan0.n
    assert n > 64
    levels = [list(plan0.levels[0]) + [Task(abi.TASK_GENERIC, 3, name="angular_momentum")], plan0.levels[1]]
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=plan0.rowblocks, eps_abs=plan0.eps_abs)
    leaf["A"] = [np.concatenate([leaf["A"][0], np.zeros((B, 3, n))], axis=1), None]
    leaf["task"] = [list(leaf["task"][0]) + [(np.zeros((B, 3)), None, None)], leaf["task"][1]]
    st = BatchedStack(plan, B, device=0, route="wide")
    assert st.route == "wide"
    dv = st.load_leaf(leaf)
    m, q, qd, rng = tmh.sample("coman35", B)
    nv = m.n
    D = Dynamics(m, 0, GRAVITY)
    qt, qdt, Ld = dev(q), dev(qd), dev(rng.uniform(-1, 1, (B, 3)))
    da, db_ = torch.zeros((B, 3, nv), **F64), torch.zeros((B, 3), **F64)
    ang = lambda out: dict(out=out, ref=Ld, K=np.eye(3), lam=2.0)
    D.forward(qt, qdt, cmm_ang=da, ang_mom_b=ang(db_))
    before = st.A[0][:B, :15].clone()
    D.forward(qt, qdt, cmm_ang=(st.A[0], 15), ang_mom_b=ang(dv["task"][0][3][0]))
    st.b[0].fill_(7.0)
    st.update(dv)
    torch.cuda.synchronize()
    assert torch.equal(st.A[0][:B, 15:, :nv], da) and torch.all(st.A[0][:B, 15:, nv:] == 0.0) and torch.equal(st.A[0][:B, :15], before)
    assert db_.abs().max() > 0 and torch.equal(st.b[0][:B, 15:], db_)
    st.solve(B)
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all()


# ---- 3. graph capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_same_bits_gpu(gpu_device):
    B = 4
    plan, leaf, model, st, K, D, dv, kb, _, q = velocity_setup(B)
    qdot = dev(np.random.default_rng(8).uniform(-1, 1, (B, model.n)))
    mom = torch.zeros((B, 6), **F64)
    db = D.batch_args(q, qdot, cmm_ang=(st.A[1], 0), momentum=mom)

    def cycle():
        K.forward(q, batch=kb); D.forward(q, batch=db); st.cycle(dv)
    cycle()
    torch.cuda.synchronize()
    outs = (st.dq, st.A[0], st.A[1], mom)
    want = [t.clone() for t in outs]
    assert (st.status[:B] == 0).all() and mom.abs().max() > 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cycle()                                          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cycle()
    for _ in range(2):                                   # twice from the same q
        for t in outs:
            t.fill_(-3.0)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(want, outs):
            assert torch.equal(a, b)


# ---- 4. one whole solve per stack against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("linear", [False, True])
def test_solve_parity_velocity_gpu(linear, gpu_device):
    B = 4
    plan, leaf, model, st, K, D, dv, kb, db, q = velocity_setup(B, linear_momentum=linear)
    K.forward(q, batch=kb); D.forward(q, batch=db); st.cycle(dv)
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all()
    lf, _, _ = mc.velocity_fill(plan, leaf, model, leaf["state"]["q0"])
    from oracle import pyoracle
    asm = pyoracle.assemble(plan, lf)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all()
    dq = st.dq[:B].cpu().numpy()
    print(f"max|dq - dq_oracle| = {np.abs(dq - ref['dq']).max():.3e}  max|dq| = {np.abs(dq).max():.3e}")
    accept(asm, dq, ref)


def test_solve_parity_inverse_dynamics_gpu(gpu_device):
    B = 4
    loop, plan, leaf, model = id_step(B)
    qd0 = np.random.default_rng(12).uniform(-0.2, 0.2, (B, model.n))               # a moving start: the block's b is not zero
    loop.qdot.copy_(dev(qd0))
    loop.produce(); loop.consume()
    torch.cuda.synchronize()
    assert (loop.st.status[:B] == 0).all()
    lf, mom, _ = mc.id_fill(plan, leaf, model, leaf["state"]["q0"], qd0, None)
    assert np.abs(mom[:, 3:]).max() > 1e-3
    asm = mc.id_assemble(plan, lf)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all()
    x = loop.st.dq[:B].cpu().numpy()
    print(f"max|x - x_oracle| = {np.abs(x - ref['dq']).max():.3e}  max|x| = {np.abs(x).max():.3e}")
    accept(asm, x, ref)


# ---- 5. closed loop, velocity ------------------------------------------------------------------------------------------------------------------
def velocity_loop(B, momentum):
    """kinematics -> dynamics -> cycle -> q += dq: (max|A_ang dq| [cycles][B], how far the soles moved); without the momentum level the
    producer writes A_ang into a spare tensor"""
    plan, leaf, model, st, K, D, dv, kb, db, q = velocity_setup(B, momentum=momentum)
    if momentum:
        Aang = st.A[1]
    else:
        assert db is None and plan.L == 2
        Aang = torch.zeros((B, 3, model.n), **F64)
        db = D.batch_args(q, cmm_ang=Aang)
    norms = torch.zeros((VEL_CYCLES, B), **F64)
    refs = [dv["task"][0][i][1] for i in range(2)]
    for c in range(VEL_CYCLES):
        K.forward(q, batch=kb); D.forward(q, batch=db); st.cycle(dv)
        norms[c] = torch.einsum("brn,bn->br", Aang[:B], st.dq[:B]).abs().amax(dim=1)
        assert (st.status[:B] == 0).all(), c
        q.add_(st.dq[:B])
    K.forward(q, batch=kb)
    torch.cuda.synchronize()
    moved = max((dv["task"][0][i][0] - refs[i]).abs().max().item() for i in range(2))
    return norms.cpu().numpy(), moved


def test_closed_loop_velocity_gpu(gpu_device):
    """B = 4, 40 cycles, the same seed and references with and without velocity::AngularMomentum above the swinging Postural task.
    On the CPU (restatements + oracle solver): max|A_ang dq| at most 2.8e-11 with the task, at least 2.7e-5 without."""
    B = 4
    a, ma = velocity_loop(B, True)
    b, mb = velocity_loop(B, False)
    print(f"max|A_ang dq|: with the task {a.min():.3e} .. {a.max():.3e}, without {b.min():.3e} .. {b.max():.3e}; soles moved {ma:.3e} / {mb:.3e}")
    assert (a < b).all()
    assert ma <= 1e-3 and mb <= 1e-3


# ---- 6. closed loop, inverse dynamics ------------------------------------------------------------------------------------------------------------
def id_loop(B, momentum):
    loop, plan, leaf, model = id_step(B, momentum=momentum)
    worst = torch.zeros((ID_STEPS, B), **F64)
    for s in range(ID_STEPS):
        loop.produce(); loop.consume()
        worst[s] = loop.momentum[:, 3:].abs().amax(dim=1)
        assert (loop.st.status[:B] == 0).all() and (loop.ok == 1).all(), s
        loop.integrate()
    torch.cuda.synchronize()
    return worst.cpu().numpy()


def test_closed_loop_inverse_dynamics_gpu(gpu_device):
    """B = 2, 30 steps of 1 ms with and without acceleration::AngularMomentum.  On the CPU (restatements + oracle solver): the largest
    |angular momentum| over the run is 1.2e-6 with the block, 1.1e-2 without."""
    B = 2
    a, b = id_loop(B, True), id_loop(B, False)
    print(f"largest |angular momentum|: with the block {a.max():.3e}, without {b.max():.3e}")
    assert a.max() < b.max()
