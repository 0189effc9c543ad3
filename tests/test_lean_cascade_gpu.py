"""The lean path of the 32-lane BOX kernels (osot_kernels.h: lean_plan) on the device: BASELINE configs 2 and 3 are full-width,
box-only plans, so osot_cascade_kernel<32, ., false, true>, osot_cycle_kernel<32, false, true> and osot_control_cycle_kernel<32, false,
true> run their lean body on them.  The general instantiation (osot_solver_set_specialisation(False)) has one body: the same bits are
asked of both, through every launch that can take the lean path."""
import numpy as np
import pytest
import torch

from opensot_amd import abi, synth
from opensot_amd import kinematics as kin
from opensot_amd.plan import Bound, StackPlan, Task, eps_abs_from_factor
from opensot_amd.solver import BatchedStack

pytestmark = pytest.mark.gpu

B = 192


@pytest.mark.parametrize("cfg", ["C3", "C2"])
def test_lean_launches_match_the_general_instantiation_gpu(gpu_device, cfg):
    plan, leaf = synth.make_velocity_stack(cfg, B, seed=6021)
    spec = BatchedStack(plan, B, device=0)
    gen = BatchedStack(plan, B, device=0)
    gen.set_specialisation(False)
    for st in (spec, gen):
        st.update(st.load_leaf(leaf)); st.solve(B)
    torch.cuda.synchronize()
    assert (spec.status[:B] == 0).all() and int(spec.iterations[:B].max()) > 0
    assert torch.equal(spec.dq[:B], gen.dq[:B])
    assert torch.equal(spec.status[:B], gen.status[:B]) and torch.equal(spec.iterations[:B], gen.iterations[:B])


@pytest.mark.parametrize("cfg", ["C3", "C2"])
def test_lean_cycle_matches_update_and_solve_gpu(gpu_device, cfg):
    plan, leaf = synth.make_velocity_stack(cfg, B, seed=6022)
    two = BatchedStack(plan, B, device=0)
    one = BatchedStack(plan, B, device=0)
    two.update(two.load_leaf(leaf)); two.solve(B)
    one.cycle(one.load_leaf(leaf))
    torch.cuda.synchronize()
    assert (one.status[:B] == 0).all()
    assert torch.equal(one.dq[:B], two.dq[:B])
    assert torch.equal(one.status[:B], two.status[:B]) and torch.equal(one.iterations[:B], two.iterations[:B])


def test_lean_control_cycle_matches_the_three_calls_gpu(gpu_device):
    """the 32-DoF humanoid, CoM / four Cartesian / Postural under the joint and velocity limit box: three closed-loop steps of
    osot_control_cycle against osot_kinematics + osot_cycle + the integration"""
    m = kin.humanoid32()
    n = m.n
    f64 = dict(dtype=torch.float64, device=torch.device("cuda", 0))
    rng = np.random.default_rng(23)
    q0 = np.zeros((B, n))
    q0[:, [m.names.index(s + "KneeSag") for s in "RL"]] = 0.5
    q0[:, [m.names.index(s + "HipSag") for s in "RL"]] = -0.25
    q0[:, [m.names.index(s + "AnkSag") for s in "RL"]] = -0.25
    q0[:, [m.names.index(s + "Elbj") for s in "RL"]] = -0.6
    q0 += rng.normal(0.0, 0.02, (B, n))
    levels = [[Task(abi.TASK_COM, 3, lam=0.1, name="com")],
              [Task(abi.TASK_CARTESIAN, 6, weight=0.1, lam=0.1, name="l_wrist"), Task(abi.TASK_CARTESIAN, 6, lam=0.1, name="r_wrist"),
               Task(abi.TASK_CARTESIAN, 6, lam=0.1, name="l_sole"), Task(abi.TASK_CARTESIAN, 6, lam=0.1, name="r_sole")],
              [Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural")]]
    bounds = [Bound(abi.BOUND_JOINT_LIMITS, scaling=1.0, name="jl"), Bound(abi.BOUND_VELOCITY_LIMITS, dT=0.01, name="vl")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=[], eps_abs=eps_abs_from_factor(1e6))
    K = kin.Kinematics(m, device=0)

    def make():
        st = BatchedStack(plan, B, device=0, want_levels=False)
        q = torch.as_tensor(q0, **f64).contiguous()
        pose = [torch.zeros((B, 12), **f64) for _ in range(4)]
        com = torch.zeros((B, 3), **f64)
        kw = dict(frame_pose={f: pose[f] for f in range(4)}, frame_J={f: (st.A[1], 6 * f) for f in range(4)}, com=com, com_J=(st.A[0], 0))
        K.forward(q, **kw)
        torch.cuda.synchronize()
        pose_d = [p.clone() for p in pose]
        pose_d[0][:, 9:] += torch.as_tensor([0.04, 0.03, 0.03], **f64)
        pose_d[1][:, 9:] += torch.as_tensor([0.04, -0.03, 0.03], **f64)
        com_d = com.clone(); com_d[:, 0] += 0.02
        qmin = torch.full((B, n), -2.5, **f64); qmax = torch.full((B, n), 2.5, **f64)
        qdot_max = torch.full((B, n), 2.0, **f64)
        leaf = {"B": B, "task": [[(com, com_d, None)], [(pose[f], pose_d[f], None) for f in range(4)], [(q, q.clone(), None)]],
                "bound": [(q, qmin, qmax), (qdot_max, None, None)], "rows": []}
        return st, q, kw, leaf

    sta, qa, kwa, leafa = make()
    stb, qb, kwb, leafb = make()
    kb = K.batch_args(qb, **kwb)
    for step in range(3):
        K.forward(qa, **kwa)
        sta.cycle(leafa)
        qa += sta.dq[:B]
        stb.control_cycle(K, kb, leafb, q_integrate=qb)
        torch.cuda.synchronize()
        assert (sta.status[:B] == 0).all() and (stb.status[:B] == 0).all()
        assert torch.equal(qa, qb), f"step {step}"
    assert torch.equal(sta.dq[:B], stb.dq[:B])
    assert float(sta.dq[:B].abs().max()) > 1e-5
