"""The measurement-driven producer on the device: osot_feedback against its host emulation and the numpy restatement
(tests/feedback_ref.py) at the shapes where the kernel can go wrong, a captured graph against eager calls, and the three synth
stacks (Cartesian admittance, joint admittance, base estimation with the IMU) through BatchedStack.cycle in closed loop against the
CPU loop: oracle/pykin.py and tests/dyn_ref.py for the model quantities, feedback_ref for the producer, the oracle's cascade for the
solve.  The CPU loop reads the posture the device's loop has reached at every step and carries its OWN filter state from step to
step, so every step compares one cycle's answer on the same posture while the filter history is restated independently."""
import ctypes as C

import numpy as np
import pytest
import torch

from opensot_amd import abi, kinematics as kin, synth
from opensot_amd.dynamics import Dynamics
from opensot_amd.feedback import Feedback, FeedbackModel
from opensot_amd.solver import BatchedStack
from oracle import pykin, pyoracle

import dyn_ref
import feedback_ref as fb
import kin_rows_ref as kr
from test_wide_plan_host import _pick, _witnesses, close, oracle_solve

pytestmark = pytest.mark.gpu
F64 = dict(dtype=torch.float64, device="cuda:0")


def run_device(case, state, pad=0, calls=1):
    """the case through osot_feedback on cuda:0 `calls` times; state is advanced in place -> Outputs (downloaded)"""
    out = fb.Outputs(case, pad)
    dev = {}

    def address(a):
        if id(a) not in dev:
            dev[id(a)] = (torch.as_tensor(a).to("cuda:0").contiguous(), a)
        return dev[id(a)][0].data_ptr()
    m, b = fb.structs(case, out, state, address)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(calls):
        abi.check(abi.lib().osot_feedback(C.byref(m), C.byref(b), st), "osot_feedback")
    torch.cuda.synchronize()
    for host in list(out.arrays().values()) + [state]:
        if id(host) in dev:
            host[...] = dev[id(host)][0].cpu().numpy()
    return out


# nv, n_cart, n_pairs, n, pad, dense: every value of the issue's lists, the staging array full (nv = 64 dense), both column halves
SHAPES = {
    "nv6_c1_p1_n7_scalar": (6, 1, 1, 7, 3, False),
    "nv7_c8_p32_n64_dense": (7, 8, 32, 64, 1, True),
    "nv35_c1_p32_n106_dense": (35, 1, 32, 106, 5, True),
    "nv64_c8_p1_n106_scalar": (64, 8, 1, 106, 2, False),
    "nv64_c8_p32_n64_dense": (64, 8, 32, 64, 0, True),
}


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_against_emulation(shape, B, gpu_device):
    """every output and the state after 3 calls are the emulation's bits, sentinels included; the restatement agrees"""
    nv, n_cart, n_pairs, n, pad, dense = SHAPES[shape]
    case = fb.make_case(B, nv, n_cart=n_cart, n_pairs=n_pairs, n=n, dense=dense, seed=100 + B)
    s_emu = np.zeros((B, fb.state_count(case)))
    s_dev, s_ref = s_emu.copy(), s_emu.copy()
    emu, got = fb.run_host(case, s_emu, pad=pad, calls=3), run_device(case, s_dev, pad=pad, calls=3)
    assert np.array_equal(s_dev, s_emu), "state"
    for name, a in got.arrays().items():
        assert np.array_equal(a, emu.arrays()[name]), name
    for _ in range(2):
        fb.step(case, s_ref)
    fb.check_outputs(got, fb.step(case, s_ref), case)
    assert np.array_equal(s_dev, s_ref)


def test_device_refuses_what_the_host_refuses(gpu_device):
    case = fb.make_case(2, 35, n_cart=2, n_pairs=4, n=35, seed=0)
    out = fb.Outputs(case)
    state = np.zeros((2, fb.state_count(case)))
    m, b = fb.structs(case, out, state, lambda a: a.ctypes.data)      # (never launched: the check comes first)
    m.n_cart = 9
    assert abi.lib().osot_feedback(C.byref(m), C.byref(b), None) == abi.ERR_INVALID
    assert b"n_cart is outside 0 .. 8" in abi.lib().osot_last_error()
    m.n_cart, b.B = 2, 0
    assert abi.lib().osot_feedback(C.byref(m), C.byref(b), None) == abi.OK      # B == 0: a no-op
    assert (state == 0.0).all()


def _admittance_feedback(B, seed):
    """a Feedback with two Cartesian terms and the dense joint filter, and its bound tensors"""
    nv = 35
    rng = np.random.default_rng(seed)
    model = FeedbackModel(nv, floating_base=True)
    for _ in range(2):
        t = model.add_cartesian_admittance(**FeedbackModel.cartesian_admittance_defaults())
        model.set_raw_params(t, rng.uniform(1e-4, 1e-3, 6), rng.uniform(20.0, 60.0, 6), 0, 0.002)
    model.set_joint_admittance(**FeedbackModel.joint_admittance_defaults())
    f = Feedback(model, B, device=0)
    tn = lambda a: torch.as_tensor(a, **F64).contiguous()
    pose = [tn(np.stack([fb.random_pose(rng) for _ in range(B)])) for _ in range(2)]
    wrench = [tn(rng.uniform(-2.0, 2.0, (B, 6))) for _ in range(2)]
    twist = [torch.zeros((B, 6), **F64) for _ in range(2)]
    tau, h, qd = tn(rng.uniform(-30.0, 30.0, (B, nv))), tn(rng.uniform(-30.0, 30.0, (B, nv))), torch.zeros((B, nv), **F64)
    Cm = tn(rng.uniform(-1e-3, 1e-3, (nv, nv)))
    f.bind(cart=[dict(pose=pose[t], wrench=wrench[t], twist_out=twist[t]) for t in range(2)], joint=dict(tau=tau, h=h, qdot_out=qd, C=Cm))
    return f, twist, qd


def test_captured_graph_advances_the_state_as_eager_calls_do(gpu_device):
    """one call captured once in a torch.cuda.graph and replayed twice = two eager calls: outputs and state, bit for bit"""
    B = 9
    eager, tw_e, qd_e = _admittance_feedback(B, seed=7)
    eager.launch()
    eager.launch()
    torch.cuda.synchronize()
    assert eager.count == 4 * (12 + 35) and (eager.state != 0.0).any()
    graphed, tw_g, qd_g = _admittance_feedback(B, seed=7)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        graphed.launch()                      # (the kernel is loaded before the capture)
    torch.cuda.synchronize()
    graphed.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        graphed.launch()
    assert (graphed.state == 0.0).all()       # capturing runs nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.state, eager.state)
    assert torch.equal(qd_g, qd_e) and all(torch.equal(a, b) for a, b in zip(tw_g, tw_e))
    graphed.reset(0.5)
    assert (graphed.state == 0.5).all()


# ---- the synth stacks in closed loop against the CPU loop -----------------------------------------------------------------------------
STEPS, SB = 5, 8


def accept(plan, leaf_cpu, dq, what):
    """the suite's rule: the parity tolerance against the oracle's cascade on the CPU-assembled leaf, or the lexicographic rule against
    the witnesses"""
    from helpers import answer_is_acceptable
    asm = pyoracle.assemble(plan, leaf_cpu)
    ref = oracle_solve(asm)
    assert (ref["status"] == 1).all(), what
    worst = 0.0
    for i in range(leaf_cpu["B"]):
        worst = max(worst, float(np.abs(dq[i] - ref["dq"][i]).max()))
        if close(dq[i], ref["dq"][i]):
            continue
        sub = _pick(asm, i)
        ok, why = answer_is_acceptable(sub, 0, dq[i], [(nm, r["dq"][0], r["status"][0] == 1) for nm, r in _witnesses(sub)])
        assert ok, (what, i, why)
    return worst, ref["dq"]


def model_case(fmodel, B, **arrays):
    """a feedback_ref case from a feedback.FeedbackModel and the arrays of the groups in use"""
    m = fmodel._m
    nc = m.n_cart
    case = dict(B=B, nv=m.nv, floating_base=m.floating_base, n_cart=nc, joint=m.joint, imu=0, contact=False, n_pairs=0, n=m.n,
                cart_C=np.array(m.cart_C[:6 * nc]).reshape(nc, 6), cart_deadzone=np.array(m.cart_deadzone[:6 * nc]).reshape(nc, 6),
                cart_omega=np.array(m.cart_omega[:6 * nc]).reshape(nc, 6), cart_damping=np.array(m.cart_damping[:6 * nc]).reshape(nc, 6),
                cart_ts=np.array(m.cart_ts[:nc]), joint_omega=m.joint_omega, joint_damping=m.joint_damping, joint_ts=m.joint_ts,
                joint_C_scalar=m.joint_C_scalar, contact_lambda=m.contact_lambda, ca_threshold=m.ca_threshold,
                cart_wrench_ref=[None] * nc, cart_twist_in=[None] * nc, joint_C=None)
    case.update(arrays)
    return case


def spring_wrench(pose, x_wall, k, xp):
    """the virtual spring on the wrist position, f = k (x_wall - x) expressed in the sensor frame (R' f), and a moment 0.02 x the
    force's entries shifted by one; xp = numpy or torch"""
    R = pose[:, :9].reshape(-1, 3, 3)
    fw = k * (x_wall - pose[:, 9:])
    f = (R * fw[:, :, None]).sum(1)                        # R' f_world
    return xp.cat([f, 0.02 * xp.roll(f, 1, 1)], 1) if xp is torch else np.concatenate([f, 0.02 * np.roll(f, 1, 1)], 1)


def test_cartesian_admittance_stack_closed_loop(gpu_device):
    plan, leaf, model, fmodel = synth.make_cartesian_admittance_stack(SB)
    s, B, n = leaf["state"], SB, plan.n
    K = kin.Kinematics(model, device=0)
    st = BatchedStack(plan, B, device=0, want_levels=False)
    fbk = Feedback(fmodel, B, device=0)
    dev, kb, q, wrench = synth.bind_cartesian_admittance(st, K, fbk, leaf)
    f = model.frame_index(s["frame"])
    pose = dev["task"][0][0][0]
    x_wall = pose[:, 9:].clone() + torch.as_tensor(s["wall"], **F64)
    # the CPU side: its own reference pose, wall and filter state
    fk0 = [pykin.forward(model, s["q0"][i]) for i in range(B)]
    pose_ref = np.stack([np.concatenate([fk["frame_R"][f].reshape(9), fk["frame_p"][f]]) for fk in fk0])
    wall_cpu = pose_ref[:, 9:] + s["wall"]
    state_cpu = np.zeros((B, fbk.count))
    for k in range(STEPS):
        q_now = q.cpu().numpy().copy()
        K.forward(q, batch=kb)
        wrench.copy_(spring_wrench(pose, x_wall, s["stiffness"], torch))
        fbk.launch()
        st.cycle(dev)
        torch.cuda.synchronize()
        assert (st.status[:B] == 0).all()
        dq = st.dq[:B].cpu().numpy()
        # the CPU loop on the same posture
        fks = [pykin.forward(model, q_now[i]) for i in range(B)]
        pose_cpu = np.stack([np.concatenate([fk["frame_R"][f].reshape(9), fk["frame_p"][f]]) for fk in fks])
        w_cpu = spring_wrench(pose_cpu, wall_cpu, s["stiffness"], np)
        ref = fb.step(model_case(fmodel, B, cart_pose=[pose_cpu], cart_wrench=[w_cpu]), state_cpu)
        twist = ref["cart_twist_out"][0]
        cpu = dict(leaf)
        cpu["A"] = [np.stack([fk["J"][f] for fk in fks]), None]
        cpu["task"] = [[(pose_cpu, pose_ref, twist)], [(q_now, s["q_ref"], None)]]
        cpu["bound"] = [(q_now,) + tuple(leaf["bound"][0][1:]), leaf["bound"][1]]
        worst, dq_ref = accept(plan, cpu, dq, f"step {k}")
        dtw = np.abs(dev["task"][0][0][2].cpu().numpy() - twist).max()
        print(f"step {k}: max |dq - dq_cpu| = {worst:.3e}, max |twist - twist_cpu| = {dtw:.3e}, max |twist| = {np.abs(twist).max():.3e}, max |dq| = {np.abs(dq).max():.3e}")
        # the desired twist: the producers' round-off (1e-12 of a pose entry) through the spring (stiffness) and the compliance
        assert dtw <= 1e-12 * s["stiffness"] * np.abs(fmodel._m.cart_C[:6]).max() * 10 + 1e-15
        assert np.abs(twist).max() > 1e-6, "the admittance term does not move the task"
        q += st.dq[:B]
    dstate = np.abs(fbk.state.cpu().numpy() - state_cpu).max()
    print(f"filter state after {STEPS} steps: max |device - cpu| = {dstate:.3e}, max |state| = {np.abs(state_cpu).max():.3e}")
    assert dstate <= 1e-9 * max(1.0, np.abs(state_cpu).max())
    assert (state_cpu[:, 18:24] != 0.0).all()          # yd: the filter carried its history


@pytest.mark.parametrize("dense", [False, True], ids=["scalar", "dense"])
def test_joint_admittance_stack_closed_loop(dense, gpu_device):
    plan, leaf, model, fmodel = synth.make_joint_admittance_stack(SB, dense=dense)
    s, B, n = leaf["state"], SB, plan.n
    D = Dynamics(model, device=0)
    st = BatchedStack(plan, B, device=0, want_levels=False)
    fbk = Feedback(fmodel, B, device=0)
    dev, db, q, tau, h = synth.bind_joint_admittance(st, D, fbk, leaf)
    rng = np.random.default_rng(5)
    ext0, gain = rng.uniform(-5.0, 5.0, (B, n)), 40.0           # an external torque that depends on the posture reached
    ext0_t, q0_t = torch.as_tensor(ext0, **F64), torch.as_tensor(s["q0"], **F64)
    state_cpu = np.zeros((B, fbk.count))
    for k in range(STEPS):
        q_now = q.cpu().numpy().copy()
        D.forward(q, batch=db)
        tau.copy_(h - (ext0_t + gain * (q - q0_t)))
        fbk.launch()
        st.cycle(dev)
        torch.cuda.synchronize()
        assert (st.status[:B] == 0).all()
        dq = st.dq[:B].cpu().numpy()
        h_cpu = np.stack([dyn_ref.Ref(model, q_now[i]).tau() for i in range(B)])
        tau_cpu = h_cpu - (ext0 + gain * (q_now - s["q0"]))
        ref = fb.step(model_case(fmodel, B, joint_h=h_cpu, joint_tau=tau_cpu, joint_C=s["joint_C"]), state_cpu)
        cpu = dict(leaf)
        cpu["task"] = [[(q_now, s["q_ref"], ref["joint_qdot_out"])]]
        cpu["bound"] = [(q_now,) + tuple(leaf["bound"][0][1:]), leaf["bound"][1]]
        worst, _ = accept(plan, cpu, dq, f"step {k}")
        dqd = np.abs(dev["task"][0][0][2].cpu().numpy() - ref["joint_qdot_out"]).max()
        print(f"step {k}: max |dq - dq_cpu| = {worst:.3e}, max |qdot_des - cpu| = {dqd:.3e}, max |qdot_des| = {np.abs(ref['joint_qdot_out']).max():.3e}")
        assert (dev["task"][0][0][2][:, :6] == 0.0).all()
        assert np.abs(ref["joint_qdot_out"]).max() > 1e-7
        q += st.dq[:B]
    dstate = np.abs(fbk.state.cpu().numpy() - state_cpu).max()
    print(f"filter state after {STEPS} steps: max |device - cpu| = {dstate:.3e}, max |state| = {np.abs(state_cpu).max():.3e}")
    # u = h - tau: the difference of two torques of up to a few hundred N m computed two ways (dynamics producer / link Jacobians)
    assert dstate <= 1e-9 * max(1.0, np.abs(state_cpu).max())


def estimation_leaf_cpu(plan, leaf, model, q, qdot, omega):
    """the base-estimation leaf on the CPU: contacts from oracle/pykin.py through kin_rows_ref.rowset_rows, the IMU block from
    feedback_ref's restatement"""
    B, legs = leaf["B"], len(model.wheel_joints)
    A = np.zeros((B, 3 * legs + 6, 6))
    bs = [np.zeros((B, 3)) for _ in range(legs)]
    Jb, pose_b = np.zeros((B, 6, model.n)), np.zeros((B, 12))
    for i in range(B):
        fk = pykin.forward(model, q[i])
        for c in range(legs):
            A[i, 3 * c:3 * c + 3], bs[c][i], _ = kr.rowset_rows(model, model.rowsets[c], fk, qdot[i])
        Jb[i], pose_b[i] = fk["J"][0], np.concatenate([fk["frame_R"][0].reshape(9), fk["frame_p"][0]])
    case = dict(B=B, nv=model.n, floating_base=1, n_cart=0, joint=0, imu=1, contact=False, n_pairs=0, n=6,
                imu_fb_J=Jb, imu_pose=pose_b, imu_omega=omega)
    r = fb.step(case, None)
    A[:, 3 * legs:] = r["imu_A"]
    cpu = dict(leaf)
    cpu["A"] = [A]
    cpu["task"] = [[(b, None, None) for b in bs] + [(r["imu_b"], None, None)]]
    return cpu


def test_base_estimation_with_the_imu_recovers_the_planted_twist(gpu_device):
    """step 0: the six-variable least-squares solution is the planted base twist to the 1e-9 the stack without the IMU asks (the
    gyroscope reading is consistent with it); then the posture follows the measured velocity for four more cycles, against the CPU
    loop"""
    plan, leaf, model = synth.make_base_estimation_stack(SB, imu=True)
    s, B = leaf["state"], SB
    assert plan.n == 6 and plan.levels[0][-1].name == "imu" and plan.levels[0][-1].rows == 6
    K = kin.Kinematics(model, device=0)
    st = BatchedStack(plan, B, device=0, want_levels=False)
    dev, kb, q, qdot, fbks = synth.bind_base_estimation(st, K, leaf)
    assert len(fbks) == 1 and fbks[0].state is None
    for k in range(STEPS):
        q_now = q.cpu().numpy().copy()
        K.forward(q, batch=kb)
        fbks[0].launch()
        st.cycle(dev)
        torch.cuda.synchronize()
        assert (st.status[:B] == 0).all()
        dq = st.dq[:B].cpu().numpy()
        if k == 0:
            err = np.abs(dq - s["qdot"][:, :6]).max()
            print(f"max |dq - planted twist| = {err:.3e}")
            assert err <= 1e-9
            legs = len(model.wheel_joints)
            A = st.A[0][:B].cpu().numpy()
            assert (A[:, 3 * legs:3 * legs + 3] == 0.0).all() and np.abs(A[:, 3 * legs + 3:]).max() > 0.1
            assert np.abs(dev["task"][0][legs][0].cpu().numpy()[:, 3:]).max() > 0.1
        cpu = estimation_leaf_cpu(plan, leaf, model, q_now, s["qdot"], s["imu_omega"])
        worst, _ = accept(plan, cpu, dq, f"step {k}")
        dA = np.abs(st.A[0][:B].cpu().numpy() - cpu["A"][0]).max()
        print(f"step {k}: max |dq - dq_cpu| = {worst:.3e}, max |A - A_cpu| = {dA:.3e}")
        assert dA <= 1e-12
        q += 1.0e-3 * qdot


def test_base_estimation_contact_error_term(gpu_device):
    """contact_lambda != 0: every contact's leaf is the producer's b plus lambda [p_d - p; -e_o] (restated on the CPU from
    oracle/pykin.py's poses), and the cycle solves the stack the device assembled as the oracle does"""
    lam = 0.7
    plan, leaf, model = synth.make_base_estimation_stack(SB, imu=True, contact_lambda=lam)
    s, B, legs = leaf["state"], SB, 4
    rng = np.random.default_rng(2)
    for c in range(legs):
        s["contact_pose_ref"][:, c] = np.stack([fb.random_pose(rng) for _ in range(B)])
    K = kin.Kinematics(model, device=0)
    st = BatchedStack(plan, B, device=0, want_levels=False)
    dev, kb, q, qdot, fbks = synth.bind_base_estimation(st, K, leaf)
    assert len(fbks) == legs
    for rep in range(2):                                  # a repeated call gives the same leaves
        K.forward(q, batch=kb)
        for f in fbks:
            f.launch()
    st.cycle(dev)
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all()
    full = dict(leaf)
    full["A"] = [st.A[0][:B].cpu().numpy()]
    full["task"] = [[(t[0][:B].cpu().numpy(), None, None) for t in dev["task"][0]]]
    for c in range(legs):
        got = full["task"][0][c][0]
        for i in range(B):
            fk = pykin.forward(model, s["q0"][i])
            T = np.concatenate([fk["frame_R"][1 + c].reshape(9), fk["frame_p"][1 + c]])
            _, b_in, _ = kr.rowset_rows(model, model.rowsets[c], fk, s["qdot"][i])
            want = b_in + lam * fb.contact_error(T, s["contact_pose_ref"][i, c])
            assert np.abs(got[i] - want).max() <= 1e-11, (c, i)
    accept(plan, full, st.dq[:B].cpu().numpy(), "contact error")
