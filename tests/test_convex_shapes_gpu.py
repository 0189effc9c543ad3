"""Convex collision shapes on the device: the CONVEX instantiation of the kinematics producer (opensot_amd/csrc/osot_kin.h, stage 5,
with the per-lane GJK of osot_convex.h) on the 32-DoF humanoid (two robots per wavefront) and on the 35-coordinate COMAN (one),
checked by the certificate of tests/convex_ref.py, against osot_shape_distance on the host, against the numpy kinematics and
against central differences of the device's own distances."""
import ctypes as C
import os

import numpy as np
import pytest

import convex_ref as cr
from opensot_amd import abi, kinematics as kin
from opensot_amd.plan import Bound, Rows, StackPlan, Task, eps_abs_from_factor, subtask
from oracle import pykin
from test_convex_shapes_host import GAP, MEMBER, _segment_pose, distance

pytestmark = pytest.mark.gpu

INTERSECTING = 7      # index of the pair whose cores always overlap
CLOSED_FORM = (0, 1)
ENV_PAIR = 8


def _model(which):
    """nine pairs on either robot (the joint names are common to both): capsule-capsule and capsule-box (closed form), box-box
    link-link, cylinder-box, cylinder-cylinder, hull-hull (16 vertices), hull-capsule, a pair of boxes around the elbow joint (their
    cores always intersect), and box-box against an environment box with a run-time pose"""
    if which == "humanoid32":
        m = kin.humanoid32()
    else:
        m = kin.from_json(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coman_tree.json"))[0]
    nm = m.names.index
    rng = np.random.default_rng(12)
    Rz = lambda a: np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    Rx = lambda a: np.array([[1.0, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    hull = lambda s: rng.uniform(-1.0, 1.0, (16, 3)) * np.array([0.03, 0.03, 0.07]) * s
    S = m.link_shapes
    S["Lfore_cap"] = (nm("LElbj"), (0, 0, -0.02), (0, 0, -0.12), 0.03)
    S["Rfore_cap"] = (nm("RElbj"), (0, 0, -0.02), (0, 0, -0.12), 0.03)
    S["Rfore_box"] = dict(joint="RElbj", kind="box", half=(0.03, 0.025, 0.06), R=Rz(0.2), p=(0, 0, -0.07), r=0.005)
    S["torso_box"] = dict(joint="WaistYaw", kind="box", half=(0.06, 0.09, 0.08), R=Rx(0.1), p=(0, 0, 0.10))
    S["Lthigh_cyl"] = dict(joint="LHipYaw", kind="cylinder", size=(0.035, 0.0, 0.05), R=Rx(0.15), p=(0, 0, -0.06))
    S["Rthigh_cyl"] = dict(joint="RHipYaw", kind="cylinder", size=(0.03, 0.0, 0.05), R=Rx(-0.1), p=(0, 0, -0.06), r=0.004)
    S["Lshin_hull"] = dict(joint="LKneeSag", kind="hull", verts=hull(1.0), p=(0, 0, -0.10))
    S["Rshin_hull"] = dict(joint="RKneeSag", kind="hull", verts=hull(0.9), p=(0, 0, -0.10), r=0.003)
    S["Lupper_box"] = dict(joint="LShYaw", kind="box", half=(0.04, 0.04, 0.04), p=m.p0[nm("LElbj")], r=0.01)
    S["Lelbow_box"] = dict(joint="LElbj", kind="box", half=(0.03, 0.05, 0.04), R=Rz(0.4), r=0.02)
    names = [("Lfore_cap", "Rfore_cap"), ("Lfore_cap", "torso_box"), ("Rfore_box", "torso_box"), ("Lthigh_cyl", "torso_box"),
             ("Lthigh_cyl", "Rthigh_cyl"), ("Lshin_hull", "Rshin_hull"), ("Rshin_hull", "Lfore_cap"), ("Lupper_box", "Lelbow_box")]
    m.pairs = [m.link_pair(a, b) for a, b in names]
    m.self_pairs = list(m.pairs)
    m.pair_names = list(names)
    assert m.add_collision_shape("table", "world", ("box", (0.30, 0.50, 0.04)), (Rz(0.3) @ Rx(0.1), (0.45, -0.2, -0.05)))
    m.set_links_vs_environment(["Rfore_box"])
    assert len(m.pairs) == 9 and m.pair_names[ENV_PAIR] == ("Rfore_box", "table")
    return m


_KIND_NAME = {abi.SHAPE_BOX: "box", abi.SHAPE_CYLINDER: "cylinder", abi.SHAPE_HULL: "hull"}


def _sides(m, pr, fk, env):
    """the two shapes of a pair tuple in the form of tests/convex_ref.py with their world poses from the numpy kinematics"""
    ja, a0, a1, ra, jb, b0, b1, rb, ex = pr if len(pr) > 8 else tuple(pr) + ({},)
    Rw, pw = fk["Rw"], fk["pw"]
    Rc, pc = pykin._carrier(m, fk, jb, ex, env)
    out = []
    for side, (Rl, pl, e0, e1, r) in enumerate(((Rw[ja], pw[ja], a0, a1, ra), (Rc, pc, b0, b1, rb))):
        kind = ex.get("kind_a" if side == 0 else "kind", abi.SHAPE_CAPSULE)
        if kind == abi.SHAPE_CAPSULE:
            pose, hl = _segment_pose(Rl @ np.asarray(e0, float) + pl, Rl @ np.asarray(e1, float) + pl)
            out += [dict(kind="capsule", size=np.array([0.0, 0.0, hl]), radius=r), pose]
            continue
        R, p = (ex["R_a"], ex["p_a"]) if side == 0 else (ex["R"], ex["p"])
        size = ex["size_a"] if side == 0 else ex["half"]
        verts = ex.get("hull_a" if side == 0 else "hull")
        sh = dict(kind=_KIND_NAME[kind], size=np.asarray(size, float), radius=r)
        if verts is not None:
            sh["verts"] = np.asarray(verts, float)
        out += [sh, (Rl @ np.asarray(R, float).reshape(3, 3), pl + Rl @ np.asarray(p, float))]
    return out


def _point_velocity(m, fk, anc, j, joint, c):
    """column j of the Jacobian of the point c carried by `joint` (-1: the world)"""
    if joint < 0 or j not in anc[joint]:
        return np.zeros(3)
    z = fk["Rw"][j] @ m.axis[j]
    return np.cross(z, c - fk["pw"][j]) if m.jtype[j] == 0 else z


class _Run:
    """the producer's pair outputs for a batch of configurations"""

    def __init__(self, m, K, q, torch):
        dev = torch.device("cuda", 0)
        B, P, n = q.shape[0], len(m.pairs), m.n
        self.tq = torch.as_tensor(q, device=dev).contiguous()
        self.J = torch.full((B, P + 1, n), 7.0, dtype=torch.float64, device=dev)
        self.d = torch.full((B, P), 7.0, dtype=torch.float64, device=dev)
        self.pts = torch.full((B, P, 6), 7.0, dtype=torch.float64, device=dev)
        K.forward(self.tq, pair_dist=self.d, pair_J=(self.J, 0), pair_points=self.pts)
        torch.cuda.synchronize()
        self.dist, self.rows, self.points = self.d.cpu().numpy(), self.J.cpu().numpy(), self.pts.cpu().numpy()


@pytest.mark.parametrize("which,B", [("humanoid32", 5), ("coman35", 3)])
def test_convex_pairs_on_the_device(which, B, gpu_device):
    """humanoid32: JMAX = 32, two robots per wavefront, B = 5 leaves the last wavefront's second half idle; COMAN: JMAX = 64.
    For every pair of every instance: the certificate on the device's witness points (gap <= 1e-10 m), the distance against
    osot_shape_distance on the host (1e-10), the intersecting pair at -r_a - r_b with a zero row, each row against
    n . (J_a(ca) - J_b(cb)) from the numpy kinematics (1e-10) and against central differences of the device's own distance (h = 1e-6,
    2e-7 as for the environment pairs of tests/test_kinematics.py); the closed-form pairs bit-identical to the same model without the
    convex pairs; moving the environment box changes only its pair."""
    import torch
    lib = abi.lib()
    m = _model(which)
    n, P = m.n, len(m.pairs)
    K = kin.Kinematics(m, device=0)
    rng = np.random.default_rng(77)
    q = rng.uniform(-0.35, 0.35, (B, n))
    run = _Run(m, K, q, torch)
    assert (run.rows[:, P] == 7.0).all()                    # the row behind the block is not touched
    rad = np.array([p[3] + p[7] for p in m.pairs])
    env = m.env_pose_array()
    anc = []
    for j in range(n):
        anc.append({j} | (anc[m.parent[j]] if m.parent[j] >= 0 else set()))
    separated = 0
    worst = dict(gap=0.0, host=0.0, row=0.0)
    for i in range(B):
        fk = pykin.forward(m, q[i])
        for k, pr in enumerate(m.pairs):
            A, pA, Bs, pB = _sides(m, pr, fk, env)
            ca, cb = run.points[i, k, :3], run.points[i, k, 3:]
            rc, dh, cah, cbh, it = distance(lib, A, pA, Bs, pB)
            assert rc == abi.OK
            if k in CLOSED_FORM:
                assert abs(dh - run.dist[i, k]) <= 1e-10
            assert abs(np.linalg.norm(ca - cb) - rad[k] - run.dist[i, k]) <= 1e-15
            if k == INTERSECTING or dh == -rad[k]:
                assert dh == -rad[k] and (run.rows[i, k] == 0.0).all(), (which, i, k, run.dist[i, k], dh)
                if k not in CLOSED_FORM:      # (GJK reports one common point; the closed forms two points within 1e-12)
                    assert run.dist[i, k] == -rad[k] and np.array_equal(ca, cb)
                continue
            separated += 1
            cert = cr.certify(A, pA, Bs, pB, ca, cb)
            worst["gap"] = max(worst["gap"], cert["gap"]); worst["host"] = max(worst["host"], abs(dh - run.dist[i, k]))
            assert cert["in_a"] <= MEMBER and cert["in_b"] <= MEMBER and -1e-12 <= cert["gap"] <= GAP, (which, i, k, cert)
            assert abs(dh - run.dist[i, k]) <= 1e-10, (which, i, k, dh, run.dist[i, k])
            nn = (ca - cb) / np.linalg.norm(ca - cb)
            ja, jb = pr[0], pr[4]
            row = np.array([nn @ (_point_velocity(m, fk, anc, j, ja, ca) - _point_velocity(m, fk, anc, j, jb, cb)) for j in range(n)])
            worst["row"] = max(worst["row"], np.abs(row - run.rows[i, k]).max())
            assert np.abs(row - run.rows[i, k]).max() <= 1e-10, (which, i, k)
    assert separated >= (P - 1) * B - 3, separated
    print(f"{which}: {separated} separated pairs, max certificate gap {worst['gap']:.3e} m, max |device - host| {worst['host']:.3e} m, "
          f"max row error {worst['row']:.3e}")
    # central differences of the device's own distances: one launch over q +- h e_j
    h = 1e-6
    qq = np.repeat(q, 2 * n, axis=0).reshape(B, n, 2, n)
    for j in range(n):
        qq[:, j, 0, j] += h; qq[:, j, 1, j] -= h
    fd = _Run(m, K, qq.reshape(B * 2 * n, n), torch).dist.reshape(B, n, 2, P)
    Jfd = ((fd[:, :, 0] - fd[:, :, 1]) / (2 * h)).transpose(0, 2, 1)          # [B][P][n]
    ok = run.dist + rad > 1e-3                                               # (intersecting cores have no normal: zero row)
    assert ok.sum() >= (P - 1) * B - 3 and np.abs(run.rows[:, :P] - Jfd)[ok].max() < 2e-7
    # the closed-form pairs: the same bits as from the model without the convex pairs (the non-CONVEX instantiation)
    m0 = _model(which)
    m0.env_shapes = []; m0.env_links = []
    m0.pairs = [m.pairs[k] for k in CLOSED_FORM]; m0.self_pairs = list(m0.pairs); m0.pair_names = [m.pair_names[k] for k in CLOSED_FORM]
    run0 = _Run(m0, kin.Kinematics(m0, device=0), q, torch)
    for k0, k in enumerate(CLOSED_FORM):
        assert np.array_equal(run0.dist[:, k0], run.dist[:, k]) and np.array_equal(run0.rows[:, k0], run.rows[:, k])
        assert np.array_equal(run0.points[:, k0], run.points[:, k])
    # moveCollisionShape: only the environment pair changes
    assert m.move_collision_shape("table", (np.eye(3), (0.5, 0.1, 0.3)))
    moved = _Run(m, K, q, torch)
    same = [k for k in range(P) if k != ENV_PAIR]
    assert np.array_equal(moved.dist[:, same], run.dist[:, same]) and np.array_equal(moved.rows[:, same], run.rows[:, same])
    assert np.abs(moved.dist[:, ENV_PAIR] - run.dist[:, ENV_PAIR]).min() > 1e-3
    fk = pykin.forward(m, q[1])
    A, pA, Bs, pB = _sides(m, m.pairs[ENV_PAIR], fk, m.env_pose_array())
    cert = cr.certify(A, pA, Bs, pB, moved.points[1, ENV_PAIR, :3], moved.points[1, ENV_PAIR, 3:])
    assert cert["in_a"] <= MEMBER and cert["in_b"] <= MEMBER and -1e-12 <= cert["gap"] <= GAP


def _wall_scenario(torch, B):
    """the scenario of test_closed_loop_hand_stops_at_a_world_box (tests/test_kinematics.py) with the forearm declared as a BOX"""
    from opensot_amd.solver import BatchedStack
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    d_min = 0.02
    rng = np.random.default_rng(3)
    m = kin.humanoid32_pairs(kin.humanoid32())
    m.self_pairs = []; m.pairs = []; m.pair_names = []
    m.link_shapes["Rforearm"] = dict(joint="RElbj", kind="box", half=(0.03, 0.03, 0.065), p=(0, 0, -0.085))
    n = m.n
    q0 = np.zeros((B, n))
    q0[:, [m.names.index(s + "Elbj") for s in "RL"]] = -0.9
    q0 += rng.normal(0.0, 0.01, (B, n))
    hand = pykin.forward(m, q0[0])["frame_p"][m.frame_index("r_wrist")]
    assert m.add_collision_shape("wall", "world", ("box", (0.10, 0.60, 0.60)), (np.eye(3), hand + np.array([0.12 + 0.05, 0.0, 0.0])))
    m.set_links_vs_environment(["Rhand", "Rforearm"])
    P = len(m.pairs)
    assert P == 2 and m.desc().pair_kind_a[1] == abi.SHAPE_BOX
    wrist = subtask(Task(abi.TASK_CARTESIAN, 6, lam=0.1, name="r_wrist"), [0, 1, 2])
    levels = [[Task(abi.TASK_CARTESIAN, 6, lam=0.1, name="l_sole"), Task(abi.TASK_CARTESIAN, 6, lam=0.1, name="r_sole")],
              [wrist], [Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural")]]
    rows = [Rows(abi.ROWS_COLLISION, P, d_threshold=d_min, detection_threshold=0.0, bound_scaling=0.2, name="env")]
    plan = StackPlan(n=n, levels=levels, bounds=[Bound(abi.BOUND_VELOCITY_LIMITS, dT=0.01, name="vl")], rowblocks=rows,
                     eps_abs=eps_abs_from_factor(1e6))
    st = BatchedStack(plan, B, device=0, want_levels=False)
    K = kin.Kinematics(m, device=0)
    q = torch.as_tensor(q0, **f64).contiguous()
    pose = [torch.zeros((B, 12), **f64) for _ in range(4)]
    Jd = torch.zeros((B, P, n), **f64); dist = torch.zeros((B, P), **f64); pts = torch.zeros((B, P, 6), **f64)
    Jw = torch.zeros((B, 6, n), **f64)
    fr = m.frame_index
    kw = dict(frame_pose={f: pose[f] for f in range(4)}, frame_J={fr("l_sole"): (st.A[0], 0), fr("r_sole"): (st.A[0], 6), fr("r_wrist"): (Jw, 0)})

    def fk():
        K.forward(q, pair_dist=dist, pair_J=(Jd, 0), pair_points=pts, **kw)
        st.A[1][:B, 0:3].copy_(Jw[:, 0:3])
    fk(); torch.cuda.synchronize()
    pose_d = [p.clone() for p in pose]
    pose_d[fr("r_wrist")][:, 9] += 0.22          # 10 cm behind the wall's near face
    leaf = {"B": B, "task": [[(pose[fr("l_sole")], pose_d[fr("l_sole")], None), (pose[fr("r_sole")], pose_d[fr("r_sole")], None)],
                             [(pose[fr("r_wrist")], pose_d[fr("r_wrist")], None)], [(q, q.clone(), None)]],
            "bound": [(torch.full((B, n), 2.0, **f64), None, None)], "rows": [(Jd, dist, None)]}
    return dict(m=m, st=st, K=K, q=q, fk=fk, leaf=leaf, dist=dist, pts=pts, Jd=Jd, kw=kw, d_min=d_min, P=P, B=B)


def test_closed_loop_forearm_box_stops_at_a_world_box(gpu_device):
    """30 steps of osot_kinematics + osot_cycle with a box-box pair feeding the CollisionAvoidance rows: every step is solved and the
    CERTIFIED distance (the separating slab along the device's witnesses, minus the radii) never drops below the safety distance by
    more than 1e-9"""
    import torch
    s = _wall_scenario(torch, B=6)
    m, st, q, B, P = s["m"], s["st"], s["q"], s["B"], s["P"]
    rad = np.array([p[3] + p[7] for p in m.pairs])
    env = m.env_pose_array()
    lowest, first = np.inf, None
    for step in range(30):
        s["fk"]()
        st.cycle(s["leaf"])
        torch.cuda.synchronize()
        assert (st.status[:B] == 0).all(), step
        qh, pts, dist = q.cpu().numpy(), s["pts"].cpu().numpy(), s["dist"].cpu().numpy()
        for i in range(B):
            fk = pykin.forward(m, qh[i])
            for k, pr in enumerate(m.pairs):
                A, pA, Bs, pB = _sides(m, pr, fk, env)
                cert = cr.certify(A, pA, Bs, pB, pts[i, k, :3], pts[i, k, 3:])
                assert cert["in_a"] <= MEMBER and cert["in_b"] <= MEMBER and -1e-12 <= cert["gap"] <= GAP, (step, i, k, cert)
                assert abs(cert["len"] - rad[k] - dist[i, k]) <= 1e-12
                lowest = min(lowest, cert["slab"] - rad[k])
        first = dist.copy() if first is None else first
        q += st.dq[:B]
    assert lowest >= s["d_min"] - 1e-9, lowest
    assert (dist < first - 0.03).all(axis=0).any()          # the arm did move towards the wall
    print(f"closed loop: lowest certified distance {lowest:.6f} m (safety distance {s['d_min']})")


def test_control_cycle_refuses_convex_pairs(gpu_device):
    """the fused control cycle has no instantiation with GJK: with pair outputs bound it answers OSOT_ERR_UNSUPPORTED and says what
    to call; without pair outputs it runs, with the results of osot_kinematics + osot_cycle"""
    import torch
    s = _wall_scenario(torch, B=6)
    st, K, q, B = s["st"], s["K"], s["q"], s["B"]
    lb, out = st._update_args(s["leaf"], True)
    qb = st._qp_batch(B)
    stream = C.c_void_p(torch.cuda.current_stream(st.device).cuda_stream)
    for outputs in (dict(pair_dist=s["dist"]), dict(pair_J=(s["Jd"], 0)), dict(pair_points=s["pts"])):
        kb = K.batch_args(q, **outputs, **s["kw"])
        rc = st._lib.osot_control_cycle(st._h, K._h, C.byref(kb), C.byref(lb), C.byref(out), C.byref(qb), None, stream)
        assert rc == abi.ERR_UNSUPPORTED and b"convex collision pairs: use osot_kinematics + osot_cycle" in st._lib.osot_last_error()
        rc = st._lib.osot_control_rollout(st._h, K._h, C.byref(kb), C.byref(lb), C.byref(out), C.byref(qb), C.c_void_p(q.data_ptr()), 2,
                                          None, None, stream)
        assert rc == abi.ERR_UNSUPPORTED and b"convex collision pairs" in st._lib.osot_last_error()
    # without pair outputs: the rows keep the distances of the last osot_kinematics call
    s["fk"]()
    st.cycle(s["leaf"])
    torch.cuda.synchronize()
    dq = st.dq[:B].clone()
    st.dq.zero_()
    st.control_cycle(K, K.batch_args(q, **s["kw"]), s["leaf"], q_integrate=None)
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all() and torch.equal(st.dq[:B], dq)
