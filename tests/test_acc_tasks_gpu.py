"""osot_acc_tasks on the device against its host lock-step emulation (tests/acc_ref.py) and the numpy.longdouble arbiter."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from opensot_amd import abi
from opensot_amd.acceleration import FORCE, AccModel, AccTasks
from opensot_amd.dynamics import Dynamics

import acc_ref as ar

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


def run_device(case, want=ar.Outputs.ALL):
    """the case through libosot_mi355x.so -> Outputs"""
    out, keep, dv = ar.Outputs(case, want), [], DeviceArrays()
    m, b = ar.structs(case, out, dv.address, keep)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().osot_acc_tasks(C.byref(m), C.byref(b), st), "osot_acc_tasks")
    torch.cuda.synchronize()
    dv.download(out.arrays())
    return out


@functools.lru_cache(maxsize=None)
def host(name):
    case = ar.named_case(name)
    return case, ar.run_host(case)


# ---- 1. the shapes against the emulation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ar.CASES))
def test_device_against_emulation_and_arbiter(name):
    case, emu = host(name)
    dev = run_device(case)
    B, nv = case["B"], case["nv"]
    assert dev.fences_intact() and np.array_equal(dev.ok, emu.ok)
    # single operations, the orientation error (contraction off) and copies: the same bits
    for t, term in enumerate(case["cart"]):
        assert np.array_equal(dev.p0(t)[:, 0:6], emu.p0(t)[:, 0:6]), (name, t)
        if term["gain_type"] != FORCE:
            assert np.array_equal(dev.p0(t)[:, 12:], emu.p0(t)[:, 12:]) and np.array_equal(dev.a_ref_out(t), emu.a_ref_out(t))
        elif term["f_virtual"] is None:
            assert np.array_equal(dev.a_ref_out(t), emu.a_ref_out(t))
    if case["com"] is not None:
        assert np.array_equal(dev.com()[:, 0:3], emu.com()[:, 0:3]) and np.array_equal(dev.com()[:, 6:], emu.com()[:, 6:])
    if case["post"] is not None:
        assert np.array_equal(dev.post(nv), emu.post(nv))
    # fma chains: the same order on both sides -- within the bound of the sum of either, and in practice the same bits
    for t, term in enumerate(case["cart"]):
        scale = np.abs(term["J"][:, 1:7, :nv]).sum(axis=2) * np.abs(case["qdot"]).max() + 2.0
        assert np.all(np.abs(dev.p0(t)[:, 6:12] - emu.p0(t)[:, 6:12]) <= 2 * (nv + 2) * ar.U * scale), (name, t)
    if case["com"] is not None:
        scale = np.abs(case["com"]["J"][:, 1:4, :nv]).sum(axis=2) * np.abs(case["qdot"]).max() + 1.0
        assert np.all(np.abs(dev.com()[:, 3:6] - emu.com()[:, 3:6]) <= 2 * (nv + 2) * ar.U * scale), name
    p = case["post"]
    if p is not None and p["gain_type"] != FORCE:
        # qddot_out = qddot_ref + lambda2 Kd vel_err + lambda Kp pos_err: 2 nv + 1 terms, each side within (k + 2) u sum|terms|
        pe, ve = np.abs(emu.post(nv)[:, :nv]), np.abs(emu.post(nv)[:, nv:])
        Kp = np.eye(nv) if p["Kp"] is None else np.abs(p["Kp"])
        Kd = np.eye(nv) if p["Kd"] is None else np.abs(p["Kd"])
        scale = p["lam"] * pe @ Kp.T + p["lam2"] * ve @ Kd.T + (0.0 if p["qddot_ref"] is None else np.abs(p["qddot_ref"]))
        assert np.all(np.abs(dev.qddot(nv) - emu.qddot(nv)) <= 2 * (2 * nv + 3) * ar.U * scale), name
    # everything out of the Cholesky factor: the tolerance of the host test, against the arbiter
    if case["M"] is not None:
        worst = ar.worst_deviation(case, dev, ar.restate(case, np.longdouble))
        print(name, "device:", worst)
        assert worst[0] <= ar.CHOLESKY_TOL, worst
        for t, term in enumerate(case["cart"]):
            if term["gain_type"] == FORCE:
                assert np.array_equal(dev.Mi(t), np.transpose(dev.Mi(t), (0, 2, 1)))
        if case["minv"]:
            assert np.array_equal(dev.minv(nv), np.transpose(dev.minv(nv), (0, 2, 1)))
    same = all(np.array_equal(a, b) for a, b in zip(dev.arrays(), emu.arrays()))
    print(name, "every output bit-identical to the emulation:", same)


# ---- 2. captured with the dynamics producer ------------------------------------------------------------------------------------------------
def test_graph_of_dynamics_and_acc_tasks_replays_bit_for_bit():
    """osot_dynamics -> osot_acc_tasks on one stream, captured; two replays with changed q equal the eager calls bit for bit"""
    import tree_cases
    m = tree_cases.tree_case(7, "chain", 0)
    B, nv = 33, m.n
    rng = np.random.default_rng(5)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    qs = [dev(tree_cases.draw_q(m, B, seed)) for seed in (1, 2, 3)]
    q, qdot = qs[0].clone(), dev(tree_cases.draw_qdot(m, B, 1))
    M, Minv, ok = z(B, nv, nv), z(B, nv, nv), torch.zeros((B,), dtype=torch.int32, device="cuda")
    J, pose, pose_ref = dev(rng.uniform(-1, 1, (B, 6, nv))), dev(np.stack([ar.random_pose(rng) for _ in range(B)])), dev(np.stack([ar.random_pose(rng) for _ in range(B)]))
    fv, p0, aout, Mi = dev(rng.uniform(-5, 5, (B, 6))), z(B, 84), z(B, 6), z(B, 36)
    q_ref, pp0, qdd = dev(rng.uniform(-1, 1, (B, nv))), z(B, 2 * nv), z(B, nv)
    dyn = Dynamics(m, 0)
    acc = AccTasks(AccModel(nv, cart=[dict(gain_type=FORCE, Kp=rng.uniform(-5, 5, (6, 6)), Kd=rng.uniform(-1, 1, (6, 6)))],
                            postural=dict(gain_type=FORCE, gain_matrices=True, lam=20.0, lam2=3.0, Kp=rng.uniform(-1, 1, (nv, nv)))))
    db = dyn.batch_args(q, qdot, M=M)
    ab = acc.batch_args(B, q=q, qdot=qdot, M=M, cart=[dict(J=J, pose=pose, pose_ref=pose_ref, f_virtual=fv, p0=p0, a_ref_out=aout, Mi=Mi)],
                        postural=dict(q_ref=q_ref, p0=pp0, qddot_out=qdd), Minv=Minv, ok=ok)
    outs = (M, Minv, p0, aout, Mi, pp0, qdd)

    def step():
        dyn.forward(q, batch=db)
        acc.forward(ab)
    want = []
    for k in range(3):
        q.copy_(qs[k]); step(); torch.cuda.synchronize()
        want.append([t.clone() for t in outs])
        assert (ok == 1).all()
    assert not torch.equal(want[1][1], want[2][1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    for k in (1, 2):
        for t in outs:
            t.fill_(-3.0)
        q.copy_(qs[k])
        g.replay(); torch.cuda.synchronize()
        for a, b in zip(want[k], outs):
            assert torch.equal(a, b), k


def test_the_largest_shape_replays_from_a_graph_after_one_eager_launch():
    """nv = 64, eight terms, Minv: 71 KB of LDS.  The first launch raises the kernel's limit (a host-side setting, made once per
    device); a capture made after it replays with the bits of the eager launch"""
    case, _ = host("nv64_full")
    out, keep, dv = ar.Outputs(case), [], DeviceArrays()
    m, b = ar.structs(case, out, dv.address, keep)
    lib = abi.lib()
    launch = lambda: abi.check(lib.osot_acc_tasks(C.byref(m), C.byref(b), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "osot_acc_tasks")
    launch()
    torch.cuda.synchronize()
    dv.download(out.arrays())
    eager = [v.copy() for v in ar.views(out, case)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    for a in out.arrays():
        dv.mirror[id(a)][1].zero_()               # (fences included: only what the kernel writes is compared below)
    g.replay()
    torch.cuda.synchronize()
    dv.download(out.arrays())
    assert not np.all(eager[-2] == 0.0)
    for x, y in zip(ar.views(out, case), eager):
        assert np.array_equal(x, y)


# ---- 3. the tracking stack in closed loop ----------------------------------------------------------------------------------------------------
# x and tau of the step whose leaves the CPU computed (acc_ref.restate from the downloaded M, J and poses) against the step whose
# leaves osot_acc_tasks wrote, both solved by the same device cycle from the same producer tensors (the scheme of
# tests/test_dynamics_gpu.py: host quantities uploaded into the tensors the step reads).  As there, the bound is 100 x the worst
# deviation measured on an MI355X (both variants, 8 instances, 5 steps), relative to max(1, max|.|); no instance is excluded.  The
# torque identity of every step is test_dynamics_gpu._check_step's, at its 1e-11.
X_MEASURED = 7.4e-16
TAU_MEASURED = 2.0e-14
CLOSED_LOOP_TOL = {"x": 100.0 * X_MEASURED, "tau": 100.0 * TAU_MEASURED}


@pytest.mark.parametrize("gain_type", [ar.ACC, FORCE])
def test_tracking_closed_loop_against_cpu_leaves(gain_type):
    from opensot_amd import synth
    from opensot_amd.dynamics import IdTrackingStep
    from test_dynamics_gpu import _check_step
    B, steps = 8, 5
    plan, leaf, model = synth.make_coman_id_tracking_stack(B, gain_type=gain_type, seed=31)
    loop, twin = IdTrackingStep(plan, leaf, model, device=0), IdTrackingStep(plan, leaf, model, device=0)
    dn = lambda t: t.cpu().numpy()
    up = lambda t, a: t.copy_(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64))
    nv, track = model.n, []
    shared = ("q", "qdot", "Jcom", "com", "com_ref", "Jhand", "hand_pose", "hand_ref", "jdq_l", "jdq_r", "jdq_com", "jdq_hand")
    for k in range(steps):
        loop.produce(); loop.consume()
        torch.cuda.synchronize()
        _check_step(loop)
        assert (loop.acc_ok == 1).all()
        track.append(np.linalg.norm(dn(loop.hand_ref)[:, 9:12] - dn(loop.hand_pose)[:, 9:12], axis=1))
        # the same step with the leaves from the CPU
        for name in shared:
            getattr(twin, name).copy_(getattr(loop, name))
        for name in ("Bm", "h", "Jc"):
            getattr(twin.model, name).copy_(getattr(loop.model, name))
        Q = dict(M=dn(loop.model.Bm), Jhand=dn(loop.Jhand), hand_pose=dn(loop.hand_pose), Jcom=dn(loop.Jcom), com=dn(loop.com))
        case = ar.tracking_case(leaf, Q, dn(loop.q), dn(loop.qdot), dn(loop.com_ref), dn(loop.hand_ref))
        R = ar.restate(case)
        c = R["cart"][0]
        up(twin.p0_hand, np.concatenate([c["pose_err"], c["vel_err"], c["Gp"].reshape(B, 36), c["Gd"].reshape(B, 36)], axis=1))
        up(twin.a_ref_hand, c["a_ref_out"])
        up(twin.p0_com, np.concatenate([R["com"]["err"], R["com"]["vel_err"]], axis=1))
        up(twin.p0_post, np.concatenate([R["post"]["pe"], R["post"]["ve"]], axis=1))
        up(twin.qddot_d, R["post"]["qddot_out"])
        twin.solve()
        torch.cuda.synchronize()
        assert (twin.st.status[:B] == 0).all() and (twin.ok == 1).all()
        for name, a, b in (("x", dn(loop.st.dq[:B]), dn(twin.st.dq[:B])), ("tau", dn(loop.tau), dn(twin.tau))):
            d = np.abs(a - b).max() / max(1.0, np.abs(b).max())
            print(f"step {k} {name}: device leaves against CPU leaves {d:.3e}")
            assert d <= CLOSED_LOOP_TOL[name], (k, name, d)
        loop.integrate()
    track = np.array(track)
    print("hand tracking error per step, worst instance:", track.max(axis=1))
    assert np.all(np.diff(track, axis=0) < 0.0)          # every instance, every step


# ---- 4. the batch with a singular M ---------------------------------------------------------------------------------------------------------
def test_a_failed_pivot_on_the_device():
    """a numerical path, not a fault: ok = [1, 0, 1], zeros and pass-throughs in the instance, the neighbours as without it, and the
    same bits as the emulation in every output"""
    good_case, _ = host("nv35")
    case = ar.singular_case(good_case)
    dev, good = run_device(case), run_device(good_case)
    ar.check_failed_pivot(dev, good, case)
    emu = ar.run_host(case)
    assert np.array_equal(dev.ok, emu.ok)
    for a, b in zip(ar.views(dev, case), ar.views(emu, case)):
        assert np.array_equal(a[1], b[1])         # the failed instance holds no arithmetic of the factor: bit for bit
