"""The rigid-body dynamics producer on the GPU (osot_dyn_create / osot_dynamics through opensot_amd.dynamics.Dynamics): the device
build against the host build of the same kernel source, the refusals that need a handle, strided outputs that land in other
producers' arrays (IdModel.Bm / h / Jc, a task's leaf array), and a captured kinematics + dynamics + computed-torque sequence."""
import ctypes as C

import numpy as np
import pytest
import torch

from opensot_amd import abi
from opensot_amd.dynamics import Dynamics, IdModel
from opensot_amd.kinematics import Kinematics

from test_dynamics_host import GRAVITY, MODELS, chain3_model, coman_model, emu_dynamics, rel

pytestmark = pytest.mark.gpu
DEVICE_TOL = 1e-13      # host build against device build: fma contraction is the only licensed difference


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def run_device(m, q, qd, M_extra=0):
    B, n, F = q.shape[0], m.n, len(m.frames)
    dyn = Dynamics(m, 0, GRAVITY)
    M = torch.full((B, n * n + M_extra), 7.0, dtype=torch.float64, device="cuda")
    h = torch.full((B, n), 7.0, dtype=torch.float64, device="cuda")
    jd = torch.full((B, 6 * F), 7.0, dtype=torch.float64, device="cuda")
    cj = torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda")
    dyn.forward(dev(q), None if qd is None else dev(qd), M=M, h=h, frame_jdotqdot={f: (jd, 6 * f) for f in range(F)}, com_jdotqdot=cj)
    torch.cuda.synchronize()
    return dict(M=M.cpu().numpy(), h=h.cpu().numpy(), jdq=jd.cpu().numpy().reshape(B, F, 6), com_jdq=cj.cpu().numpy())


@pytest.mark.parametrize("name", sorted(MODELS))
def test_device_build_against_host_build(name):
    make = MODELS[name][0]
    m, lo, up = make()
    rng = np.random.default_rng(400 + len(name))
    B = 256
    q, qd = rng.uniform(lo, up, (B, m.n)), rng.uniform(-2.0, 2.0, (B, m.n))
    got, ref = run_device(m, q, qd), emu_dynamics(m, q, qd)
    got["M"] = got["M"].reshape(B, m.n, m.n)
    for k in ("M", "h", "jdq", "com_jdq"):
        d = rel(got[k], ref[k])
        print(f"{name} {k}: device vs host rel {d:.3e}")
        assert d <= DEVICE_TOL, (name, k, d)
    for i in range(B):
        assert np.array_equal(got["M"][i], got["M"][i].T)
        np.linalg.cholesky(got["M"][i])
    g0 = run_device(m, q, None)                     # qdot = NULL
    assert rel(g0["h"], emu_dynamics(m, q, None)["h"]) <= DEVICE_TOL and np.all(g0["jdq"] == 0.0)


def test_refusals_with_a_handle():
    m, q, qd, = chain3_model()[0], None, None
    m.frame_body = {0: True}
    m.frame_base = {1: 0}
    dyn = Dynamics(m, 0)
    lib = abi.lib()
    B = 4
    qt = torch.zeros((B, m.n), dtype=torch.float64, device="cuda")
    out = torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for f in (0, 1):
        b = dyn.batch_args(qt, frame_jdotqdot={f: out})
        assert lib.osot_dynamics(dyn._h, C.byref(b), st) == abi.ERR_UNSUPPORTED
        assert b"world frames only" in lib.osot_last_error()
    M = torch.zeros((B, m.n * m.n), dtype=torch.float64, device="cuda")
    b = dyn.batch_args(qt, M=M); b.M_stride = m.n * m.n - 1
    assert lib.osot_dynamics(dyn._h, C.byref(b), st) == abi.ERR_INVALID and b"M_stride" in lib.osot_last_error()
    b = dyn.batch_args(qt, M=M); b.q = None
    assert lib.osot_dynamics(dyn._h, C.byref(b), st) == abi.ERR_INVALID
    b = dyn.batch_args(qt, M=M); b.frame_Jdot_qdot[5] = out.data_ptr(); b.frame_Jdot_qdot_stride[5] = 6
    assert lib.osot_dynamics(dyn._h, C.byref(b), st) == abi.ERR_INVALID
    b = dyn.batch_args(qt, com_jdotqdot=out); b.com_Jdot_qdot_stride = 2
    assert lib.osot_dynamics(dyn._h, C.byref(b), st) == abi.ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)                    # nothing was launched
    dyn.forward(qt, M=M)                            # M and h are offered for this model
    torch.cuda.synchronize()


def test_strided_outputs_into_other_producers_arrays():
    """M with a gap behind every instance, Jdot qdot into the p1 array of an acceleration task, the producers' outputs straight
    into an IdModel (Bm, h from osot_dynamics; Jc from osot_kinematics' frame_J): the gaps keep their sentinel"""
    m, lo, up = coman_model()
    rng = np.random.default_rng(77)
    B, n = 32, m.n
    q, qd = rng.uniform(lo, up, (B, n)), rng.uniform(-2.0, 2.0, (B, n))
    ref = emu_dynamics(m, q, qd)
    got = run_device(m, q, qd, M_extra=9)
    assert np.all(got["M"][:, n * n:] == 7.0) and rel(got["M"][:, :n * n].reshape(B, n, n), ref["M"]) <= DEVICE_TOL
    ls, rs = m.frame_index("l_sole"), m.frame_index("r_sole")
    model = IdModel.empty(B, n, 2, 6)
    kin, dyn = Kinematics(m, 0), Dynamics(m, 0, GRAVITY)
    p1 = torch.full((B, 2, 10), 7.0, dtype=torch.float64, device="cuda")      # two tasks' leaves with room around the 6 rows
    qt, qdt = dev(q), dev(qd)
    kin.forward(qt, frame_J={ls: model.contact_rows(0), rs: model.contact_rows(1)})
    dyn.forward(qt, qdt, M=model.Bm, h=model.h, frame_jdotqdot={ls: (p1.view(B, 20), 2), rs: (p1.view(B, 20), 12)})
    torch.cuda.synchronize()
    assert rel(model.Bm.cpu().numpy(), ref["M"]) <= DEVICE_TOL and rel(model.h.cpu().numpy(), ref["h"]) <= DEVICE_TOL
    P = p1.cpu().numpy()
    assert np.all(P[:, :, :2] == 7.0) and np.all(P[:, :, 8:] == 7.0)
    assert rel(P[:, 0, 2:8], ref["jdq"][:, ls]) <= DEVICE_TOL and rel(P[:, 1, 2:8], ref["jdq"][:, rs]) <= DEVICE_TOL
    # Jc is the kinematics producer's Jacobian of the two soles, and the pieces are consistent: d/dt (Jc qdot) = Jc qddot + Jdot qdot
    from helpers import emu_kinematics
    _, J, _ = emu_kinematics(m, q)
    Jc = model.Jc.cpu().numpy()
    assert rel(Jc[:, 0], J[:, 6 * ls:6 * ls + 6]) <= DEVICE_TOL and rel(Jc[:, 1], J[:, 6 * rs:6 * rs + 6]) <= DEVICE_TOL
    # computed torque from the in-place model: tau = M qddot + h - Jc' F
    x = dev(rng.uniform(-1.0, 1.0, (B, n + 12)))
    tau, _ = model.computed_torque(x)
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    want = np.einsum("bij,bj->bi", ref["M"], xh[:, :n]) + ref["h"] - np.einsum("bcij,bci->bj", Jc, xh[:, n:].reshape(B, 2, 6))
    assert rel(tau.cpu().numpy(), want) <= 1e-12


def test_graph_capture_replays_bit_for_bit():
    """kinematics + dynamics + computed torque captured into one graph: the replay equals the stream-launched sequence"""
    m, lo, up = coman_model()
    rng = np.random.default_rng(78)
    B, n = 64, m.n
    qt, qdt = dev(rng.uniform(lo, up, (B, n))), dev(rng.uniform(-2.0, 2.0, (B, n)))
    x = dev(rng.uniform(-1.0, 1.0, (B, n + 12)))
    ls, rs = m.frame_index("l_sole"), m.frame_index("r_sole")
    kin, dyn = Kinematics(m, 0), Dynamics(m, 0, GRAVITY)
    model = IdModel.empty(B, n, 2, 6)
    jd = torch.zeros((B, 12), dtype=torch.float64, device="cuda")
    cj = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
    tau = torch.zeros((B, n), dtype=torch.float64, device="cuda")
    mc = model._c()
    lib = abi.lib()

    def step():
        kin.forward(qt, frame_J={ls: model.contact_rows(0), rs: model.contact_rows(1)})
        dyn.forward(qt, qdt, M=model.Bm, h=model.h, frame_jdotqdot={ls: (jd, 0), rs: (jd, 6)}, com_jdotqdot=cj)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        abi.check(lib.osot_computed_torque(C.byref(mc), C.c_void_p(x.data_ptr()), C.c_void_p(tau.data_ptr()), None, 10e-3, st))
    step()
    torch.cuda.synchronize()
    want = [t.clone() for t in (model.Bm, model.h, model.Jc, jd, cj, tau)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                      # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    for t in (model.Bm, model.h, model.Jc, jd, cj, tau):
        t.fill_(-3.0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for t in (model.Bm, model.h, model.Jc, jd, cj, tau):
        t.fill_(-3.0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(want, (model.Bm, model.h, model.Jc, jd, cj, tau)):
        assert torch.equal(a, b)


# ---- the COMAN inverse-dynamics stack on the producers ------------------------------------------------------------------------
# Worst |q_device - q_host| over the 50 steps and 64 instances measured on an MI355X (device run: every model quantity from
# osot_kinematics / osot_dynamics; host run: from tests/dyn_ref.py, uploaded): TRAJ_MEASURED.  The assertion is 100x that, capped
# at 1e-6 (active-set changes amplify round-off of the inputs, so the bound is measured, not derived).  No instance is excluded.
TRAJ_MEASURED = 3.331e-16
TRAJ_CAP = 1e-6


def _coman_loop(B, seed):
    from opensot_amd import synth
    from opensot_amd.dynamics import IdStep
    plan, leaf, model = synth.make_coman_id_stack(B, seed=seed)
    return IdStep(plan, leaf, model, device=0), model


def _check_step(loop):
    """every instance SOLVED, computed torque ok, and |M qddot + h - Jc' F - tau| at round-off from the tensors on the device"""
    B, nv = loop.B, loop.nv
    assert (loop.st.status[:B] == 0).all() and (loop.ok == 1).all()
    x = loop.st.dq[:B].cpu().numpy()
    M, h, Jc = loop.model.Bm.cpu().numpy(), loop.model.h.cpu().numpy(), loop.model.Jc.cpu().numpy()
    want = np.einsum("bij,bj->bi", M, x[:, :nv]) + h - np.einsum("bcij,bci->bj", Jc, x[:, nv:].reshape(B, 2, 6))
    tau = loop.tau.cpu().numpy()
    assert np.abs(tau - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    assert np.abs(tau[:, :6]).max() <= 1e-8 and np.abs(tau[:, 6:]).max() <= 60.0 + 1e-8


def test_coman_id_closed_loop_device_against_host_quantities():
    """B = 64, 50 steps of 1 ms on synth.make_coman_id_stack, q and qdot integrated explicitly with the solved qddot.  Run 1: the
    producers on the device.  Run 2: M, h, Jc, Jdot qdot, CoM and its Jacobian from tests/dyn_ref.py on the host, uploaded into the
    same tensors.  (The seeds were pre-checked through the host builds: tests/test_dynamics_host.py.)"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    from test_dynamics_host import coman_quantities_parallel
    B, steps, seed = 64, 50, 31
    dev_loop, model = _coman_loop(B, seed)
    traj_dev = []
    for _ in range(steps):
        dev_loop.produce(); dev_loop.consume()
        torch.cuda.synchronize()
        _check_step(dev_loop)
        dev_loop.integrate()
        traj_dev.append(dev_loop.q.cpu().numpy())
    host_loop, _ = _coman_loop(B, seed)
    traj_host = []
    with ProcessPoolExecutor(8, mp_context=mp.get_context("spawn")) as pool:
        for _ in range(steps):
            Q = coman_quantities_parallel(pool, model, host_loop.q.cpu().numpy(), host_loop.qdot.cpu().numpy())
            host_loop.model.Bm.copy_(dev(Q["M"])); host_loop.model.h.copy_(dev(Q["h"])); host_loop.model.Jc.copy_(dev(Q["Jc"]))
            host_loop.jdq_l.copy_(dev(Q["jdq"][:, 0])); host_loop.jdq_r.copy_(dev(Q["jdq"][:, 1])); host_loop.jdq_com.copy_(dev(Q["com_jdq"]))
            host_loop.Jcom.copy_(dev(Q["Jcom"])); host_loop.com.copy_(dev(Q["com"]))
            host_loop.consume()
            torch.cuda.synchronize()
            _check_step(host_loop)
            host_loop.integrate()
            traj_host.append(host_loop.q.cpu().numpy())
    d = np.abs(np.array(traj_dev) - np.array(traj_host))
    moved = np.abs(np.array(traj_dev)[-1] - np.array(traj_dev)[0]).max()
    print(f"coman closed loop: worst |q_dev - q_host| {d.max():.3e} (worst instance {d.max(axis=(0, 2)).argmax()}), the posture moved {moved:.3e}")
    assert moved > 1e-4                                # the loop does something
    assert TRAJ_MEASURED is not None
    assert d.max() <= min(100.0 * TRAJ_MEASURED, TRAJ_CAP)


def test_captured_id_step_replays_bit_for_bit():
    """the whole step -- osot_kinematics, osot_dynamics, leaf errors, osot_id_rows, osot_cycle, osot_computed_torque, integration --
    captured into one graph: three replays equal three stream-launched steps bit for bit"""
    B, seed = 64, 31
    a, _ = _coman_loop(B, seed)
    a.step(); torch.cuda.synchronize()                 # (fixes com_ref)
    want = []
    for _ in range(3):
        a.step(); torch.cuda.synchronize()
        want.append([t.clone() for t in (a.q, a.qdot, a.st.dq[:B], a.tau, a.model.Bm, a.model.h, a.model.Jc)])
    b, _ = _coman_loop(B, seed)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b.step()                                       # the same first step, on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    keep = (b.q.clone(), b.qdot.clone())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                # (the stream the solver was last used on: it orders its calls across streams)
        b.step()
    torch.cuda.synchronize()
    b.q.copy_(keep[0]); b.qdot.copy_(keep[1])          # capture does not execute; start the replays from the state after step 1
    for k in range(3):
        g.replay(); torch.cuda.synchronize()
        got = (b.q, b.qdot, b.st.dq[:B], b.tau, b.model.Bm, b.model.h, b.model.Jc)
        for x, y in zip(want[k], got):
            assert torch.equal(x, y), k
    assert (b.st.status[:B] == 0).all() and (b.ok == 1).all()
