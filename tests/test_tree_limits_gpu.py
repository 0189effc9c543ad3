"""The tree producers at their declared limits ON THE DEVICE (the cases of tests/tree_cases.py; tests/test_tree_limits_host.py runs them
through the host emulation, which runs the lanes one after another and so cannot see a missing barrier, a leak between the halves of
the packed kernel or an LDS race):

  osot_kinematics   every size 1 .. 64, chain / random / interleaved trees, frame options on and off, every output bound, B = 1, 2, 3
                    and 5 with different robots in the two halves of a packed wavefront, with and without the pair stage -- against
                    oracle/pykin.py at the project's absolute 1e-12
  osot_dynamics     the same trees against the host build of the same source at test_dynamics_gpu.DEVICE_TOL, both instantiations
  osot_posture_gradient   a chain of 33 and a random tree of 64 against tests/gradient_ref.py at gradient_cases.PARITY_TOL
  the geometry rig  every closed-form collision case in one launch, judged by the certificate of tests/convex_ref.py
  osot_control_cycle   random trees of 20 joints (the 32-lane plan, twelve idle lanes) and 40 joints (the 40-lane plan) against the
                    three separate calls, bit for bit

The measured deviations are in profiles/tree_limits.txt."""
import time

import numpy as np
import pytest
import torch

from opensot_amd import abi
from opensot_amd import kinematics as kin
from opensot_amd.dynamics import Dynamics

import gradient_cases as gc
import gradient_ref as gref
import test_momentum_host as tmh
import tree_cases as tc
from test_dynamics_gpu import DEVICE_TOL
from test_dynamics_host import GRAVITY, rel
from test_posture_gradient_gpu import run_producer

pytestmark = pytest.mark.gpu
F64 = dict(dtype=torch.float64, device="cuda:0")
GPU_TOPOLOGIES = ("chain", "random", "interleaved")
BATCHES = (1, 2, 3, 5)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), **F64)


def run_kinematics(K, m, q, env_pose=None, pairs=True):
    """osot_kinematics with every output bound (pairs=False: without the pair outputs) -> numpy arrays in the layout of
    tree_cases.output_shapes, canaries included"""
    B, n = q.shape
    F, P = len(m.frames), len(m.pairs)
    t = {k: torch.full(s, tc.CANARY, **F64) for k, s in tc.output_shapes(m, B).items()}
    kw = dict(frame_pose={f: t["poses"][f] for f in range(F)}, frame_J={f: (t["A"], 6 * f) for f in range(F)}, com=t["com"],
              com_J=(t["A"], 6 * F))
    if m.points:
        kw["points"] = t["points"]
    if P and pairs:
        kw.update(pair_dist=t["pd"], pair_J=(t["pJ"], 0), pair_points=t["pp"])
        if env_pose is not None:
            kw["env_pose"] = dev(env_pose)
    K.forward(dev(q), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def kinematics_case(m, env_pose=None, label=""):
    """all batches of one model, with and without the pair stage; the reference is computed once for the largest batch"""
    K = kin.Kinematics(m, device=0)
    q = tc.draw_q(m, max(BATCHES))
    ref = tc.reference(m, q, env_pose=env_pose)
    worst = {}
    for B in BATCHES:
        for pairs in (True, False):
            if not pairs and not m.pairs and B != BATCHES[0]:
                continue
            got = run_kinematics(K, m, q[:B], env_pose=env_pose, pairs=pairs)
            w = tc.compare(got, m, ref[:B], tc.DEVICE_BOUND, pairs=pairs)
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    print(f"kinematics {label}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ---- osot_kinematics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [False, True])
@pytest.mark.parametrize("topology", GPU_TOPOLOGIES)
@pytest.mark.parametrize("n", tc.SIZES)
def test_kinematics_on_the_trees_gpu(n, topology, options, gpu_device):
    """n <= 32: osot_kin_kernel<., 32> (two robots per wavefront, the lanes beyond n idle but in every ballot, barrier and prefix
    sum); n >= 33: <., 64> (bit 63 of the masks, a frame, a pair and a point on lane 63, six rounds of pointer jumping at depth 64)"""
    t0 = time.perf_counter()
    m = tc.tree_case(n, topology)
    kinematics_case(tc.with_options(m) if options else m, label=f"n={n} {topology} options={int(options)}")
    print(f"wall {time.perf_counter() - t0:.3f} s")


def test_every_declared_maximum_at_once_gpu(gpu_device):
    """64 joints, 8 frames with relative bases, BODY and masks, 32 pairs (16 of them against 16 environment shapes), 16 points"""
    from test_tree_limits_host import full_model
    t0 = time.perf_counter()
    m = full_model()
    kinematics_case(m, env_pose=m.env_pose_array(), label="every maximum")
    print(f"wall {time.perf_counter() - t0:.3f} s")


# ---- osot_dynamics ---------------------------------------------------------------------------------------------------------------------------
def run_dynamics(dyn, m, q, qd, momentum):
    B, n, F = q.shape[0], m.n, len(m.frames)
    full = lambda *s: torch.full(s, tc.CANARY, **F64)
    out = dict(M=full(B, n * n), h=full(B, n), jdq=full(B, 6 * F), com_jdq=full(B, 3), cmm_lin=full(B, 3, n), cmm_ang=full(B, 3, n),
               momentum=full(B, 6))
    kw = dict(cmm_lin=out["cmm_lin"], cmm_ang=out["cmm_ang"], momentum=out["momentum"]) if momentum else {}
    dyn.forward(dev(q), None if qd is None else dev(qd), M=out["M"], h=out["h"], frame_jdotqdot={f: (out["jdq"], 6 * f) for f in range(F)},
                com_jdotqdot=out["com_jdq"], **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["M"], out["jdq"] = out["M"].reshape(B, n, n), out["jdq"].reshape(B, F, 6)
    return out


@pytest.mark.parametrize("topology", GPU_TOPOLOGIES)
@pytest.mark.parametrize("n", tc.SIZES)
def test_dynamics_on_the_trees_gpu(n, topology, gpu_device):
    """device build against host build of osot_dyn.h (its first stage is kin_instance<false, 64>): the plain instantiation and the
    one with the centroidal momentum outputs, B = 1 and 5, qdot given and NULL"""
    t0 = time.perf_counter()
    m = tc.tree_case(n, topology)
    dyn = Dynamics(m, 0, GRAVITY)
    q, qd = tc.draw_q(m, 5), tc.draw_qdot(m, 5)
    ref, ref0 = tmh.emu_momentum(m, q, qd), tmh.emu_momentum(m, q, None, want=())
    floor = 1e-3 * np.abs(ref["cmm_lin"]).max()         # (a lone prismatic joint has no angular momentum: tests/test_tree_limits_host.py)
    worst = 0.0
    for B in (1, 5):
        for momentum in (False, True):
            got = run_dynamics(dyn, m, q[:B], qd[:B], momentum)
            for k in ("M", "h", "jdq", "com_jdq") + (("cmm_lin", "cmm_ang", "momentum") if momentum else ()):
                d = np.abs(got[k] - ref[k][:B]).max() / max(np.abs(ref[k][:B]).max(), floor if k == "cmm_ang" else 1e-300)
                worst = max(worst, d)
                assert d <= DEVICE_TOL, (B, momentum, k, d)
            if not momentum:
                assert all((got[k] == tc.CANARY).all() for k in ("cmm_lin", "cmm_ang", "momentum"))
            for i in range(B):
                assert np.array_equal(got["M"][i], got["M"][i].T)
                np.linalg.cholesky(got["M"][i])
        g0 = run_dynamics(dyn, m, q[:B], None, False)               # qdot = NULL: only the gravity term remains
        assert rel(g0["h"], ref0["h"][:B]) <= DEVICE_TOL and np.all(g0["jdq"] == 0.0) and np.all(g0["com_jdq"] == 0.0)
        assert np.array_equal(g0["M"], got["M"])
    print(f"dynamics n={n} {topology}: device vs host rel {worst:.1e}  wall {time.perf_counter() - t0:.3f} s")


# ---- osot_posture_gradient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,topology", [(33, "chain"), (64, "random")])
def test_posture_gradient_on_the_trees_gpu(n, topology, gpu_device):
    """compared as tests/test_posture_gradient_gpu.py compares: the restatement's batched engine, gradient_cases.deviation and its bound"""
    t0 = time.perf_counter()
    m = tc.tree_case(n, topology)
    F, CM, EF = abi.GRAD_MANIPULABILITY_FRAME, abi.GRAD_MANIPULABILITY_COM, abi.GRAD_MIN_EFFORT
    terms = [gref.term(F, 0, W=np.linspace(0.5, 1.0, n)), gref.term(CM), gref.term(EF, W=np.full(n, 1e-2))]
    q, _ = gref.draw(m, terms, 2, seed=n, cap=gc.COND_CAP)
    b, value = run_producer(m, terms, q)
    ref = gref.gradients(m, q, terms, gc.GRAVITY, np.float64, "batched")
    d, vd = gc.deviation(b, ref), gc.value_deviation(value, ref)
    print(f"gradient n={n} {topology}: b {d} value {vd}  wall {time.perf_counter() - t0:.3f} s")
    assert (d <= gc.PARITY_TOL).all() and (vd <= gc.PARITY_TOL).all()


# ---- the closed-form geometry rig ----------------------------------------------------------------------------------------------------------
def test_rig_gpu(gpu_device):
    """every case of tree_cases.Rig as one launch (one instance per case, per-instance environment poses)"""
    from test_tree_limits_host import RIG_COINCIDENT
    t0 = time.perf_counter()
    rig = tc.rig()
    assert int(rig.coincident.sum()) == RIG_COINCIDENT
    K = kin.Kinematics(rig.model, device=0)
    got = run_kinematics(K, rig.model, rig.q, env_pose=rig.env)
    w = rig.check(got["pd"][:rig.B], got["pJ"][:rig.B, :6], got["pp"][:rig.B])
    assert (got["pJ"][:, 6] == tc.CANARY).all() and (got["pd"][rig.B] == tc.CANARY).all() and (got["pp"][rig.B] == tc.CANARY).all()
    print("rig on the device: " + " ".join(f"{k} {v:.1e}" for k, v in w.items()) + f"  wall {time.perf_counter() - t0:.3f} s")


# ---- osot_control_cycle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20, 40])
def test_control_cycle_on_a_random_tree_gpu(n, gpu_device):
    """the fused cycle on a random tree with prismatic joints in mid-chain: n = 20 runs kin_instance<., 32> with twelve idle lanes in
    the 32-lane plan, n = 40 kin_instance<., 64> in the 40-lane plan.  A box plan (CoM / four Cartesian tasks / Postural), held to
    the criterion of test_kinematics.test_control_cycle_in_one_launch_matches_the_three_calls: every array bit-identical"""
    from test_kinematics import control_cycle_matches_the_three_calls
    t0 = time.perf_counter()
    m = tc.tree_case(n, "random")
    assert any(m.jtype[j] == abi.JOINT_PRISMATIC and m.parent[j] >= 0 for j in range(n))
    rng = np.random.default_rng(n)
    control_cycle_matches_the_three_calls(m, "box", tc.draw_q(m, 5) * 0.5 + rng.normal(0.0, 0.02, (5, n)), rng)
    print(f"control cycle n={n}: wall {time.perf_counter() - t0:.3f} s")
