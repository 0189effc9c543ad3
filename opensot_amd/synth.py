"""Seeded synthetic humanoid stacks for the BASELINE.json configurations.

Produces (StackPlan, leaf) where `leaf` holds the per-instance inputs that the reference obtains from
XBot::ModelInterface (Jacobians, poses, CoM, q) plus references and limits, as numpy fp64 arrays.
No solving happens here.  There is no robot model on this path (xbot2_interface is un-vendored):
Jacobians are N(0, 0.3^2) with kinematic-chain sparsity, poses are random rigid transforms.

leaf layout (all instance-major):
  leaf["A"][k]            : [B][ma_k][n]   stacked task Jacobians of level k (Postural rows implicit)
  leaf["task"][k][j]      : (p0, p1, p2)   per osot_leaf_ptrs in include/osot_mi355x.h
  leaf["bound"][j]        : (p0, p1, p2)
  leaf["rows"][j]         : (p0, p1, p2)
"""
import numpy as np

from . import abi
from .plan import Bound, Rows, StackPlan, Task, eps_abs_from_factor

# 32-DoF humanoid column map: 6 floating-base + 7 + 7 (arms) + 6 + 6 (legs)
_BASE = list(range(0, 6))
_LIMBS = {
    "l_arm": list(range(6, 13)),
    "r_arm": list(range(13, 20)),
    "l_leg": list(range(20, 26)),
    "r_leg": list(range(26, 32)),
}


def _rot_exp(w):
    """Rodrigues: exp([w]x) for w [..., 3] -> [..., 3, 3]."""
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    th = np.where(th < 1e-12, 1e-12, th)
    k = w / th
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -k[..., 2], k[..., 1]
    K[..., 1, 0], K[..., 1, 2] = k[..., 2], -k[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -k[..., 1], k[..., 0]
    s, c = np.sin(th)[..., None], np.cos(th)[..., None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def _pose(R, p):
    return np.concatenate([R.reshape(R.shape[0], 9), p], axis=1)


def _limb_jacobian(rng, B, rows, n, cols):
    J = np.zeros((B, rows, n))
    J[:, :, cols] = rng.normal(0.0, 0.3, size=(B, rows, len(cols)))
    return J


def _cartesian_leaf(rng, B):
    R = _rot_exp(rng.normal(0.0, 0.2, size=(B, 3)))
    p = rng.uniform(-1.0, 1.0, size=(B, 3))
    dth = rng.normal(size=(B, 3))
    dth *= (rng.uniform(0.0, 0.1, size=(B, 1)) / np.linalg.norm(dth, axis=1, keepdims=True))
    dp = rng.normal(size=(B, 3))
    dp *= (rng.uniform(0.0, 0.05, size=(B, 1)) / np.linalg.norm(dp, axis=1, keepdims=True))
    Rd = R @ _rot_exp(dth)
    pd = p + dp
    return _pose(R, p), _pose(Rd, pd), None


def _box_leaf(rng, B, n, jl=True, vl=True):
    bounds, leaf = [], []
    if jl:
        half = rng.uniform(0.5, 2.5, size=(B, n))
        qmin, qmax = -half, half
        q = rng.uniform(qmin, qmax)
        # some joints sit close to a limit so that the joint-limit side of the box binds
        near = rng.random((B, n)) < 0.1
        q = np.where(near, qmax - rng.uniform(0.0, 0.01, size=(B, n)), q)
        bounds.append(Bound(abi.BOUND_JOINT_LIMITS, scaling=1.0, name="joint_limits"))
        leaf.append((q, qmin, qmax))
    if vl:
        bounds.append(Bound(abi.BOUND_VELOCITY_LIMITS, dT=0.01, name="velocity_limits"))
        leaf.append((np.full((B, n), 2.0), None, None))
    return bounds, leaf


def make_velocity_stack(config, B, seed=None, n=32, eps_factor=1e6, P=16):
    """config in {"C2", "C3", "C4"}; returns (plan, leaf)."""
    assert n == 32, "the synthetic humanoid column map is 32-DoF"
    cfg_id = {"C2": 2, "C3": 3, "C4": 4}[config]
    rng = np.random.default_rng(1000 * cfg_id if seed is None else seed)

    def cart(name, limb, weight=1.0, lam=0.1):
        t = Task(abi.TASK_CARTESIAN, 6, weight=weight, lam=lam, name=name)
        J = _limb_jacobian(rng, B, 6, n, _BASE + _LIMBS[limb])
        return t, J, _cartesian_leaf(rng, B)

    def com(lam=0.1):
        t = Task(abi.TASK_COM, 3, lam=lam, name="com")
        J = rng.normal(0.0, 0.3, size=(B, 3, n))
        p = rng.uniform(-0.2, 0.2, size=(B, 3))
        pd = p + rng.uniform(-0.05, 0.05, size=(B, 3))
        return t, J, (p, pd, None)

    def postural(weight=1.0, lam=0.01, q=None):
        t = Task(abi.TASK_POSTURAL, n, weight=weight, lam=lam, name="postural")
        qq = rng.uniform(-1.0, 1.0, size=(B, n)) if q is None else q
        qd = qq + rng.normal(0.0, 0.1, size=(B, n))
        return t, None, (qq, qd, None)

    if config == "C2":
        # one level, soft priorities (cf. coman_ik.cpp:429): r_wrist + 1e-4*postural, joint-limit box
        bounds, bleaf = _box_leaf(rng, B, n, jl=True, vl=False)
        blocks = [[cart("r_wrist", "r_arm", lam=1.0), postural(weight=1e-4, lam=1.0, q=bleaf[0][0])]]
        rowblocks, rleaf = [], []
    else:
        bounds, bleaf = _box_leaf(rng, B, n, jl=True, vl=True)
        blocks = [
            [com()],
            [cart("l_wrist", "l_arm", weight=0.1), cart("r_wrist", "r_arm"),
             cart("l_sole", "l_leg"), cart("r_sole", "r_leg")],
            [postural(q=bleaf[0][0])],
        ]
        rowblocks, rleaf = [], []
        if config == "C4":
            # self-collision rows (CollisionAvoidance.cpp:96-152): P candidate pairs sorted by distance,
            # about 30 % beyond the detection threshold (-> unused zero rows)
            Jd = np.zeros((B, P, n))
            for r in range(P):
                cols = rng.choice(np.arange(6, n), size=14, replace=False)
                Jd[:, r, cols] = rng.normal(0.0, 0.3, size=(B, 14))
            d = np.sort(rng.uniform(0.0, 0.072, size=(B, P)), axis=1)
            rowblocks.append(Rows(abi.ROWS_COLLISION, P, d_threshold=0.0, detection_threshold=0.05,
                                  bound_scaling=1.0, name="self_collision"))
            rleaf.append((Jd, d, None))

    levels, A, tleaf = [], [], []
    for lev in blocks:
        levels.append([t for (t, _, _) in lev])
        Js = [J for (_, J, _) in lev if J is not None]
        A.append(np.ascontiguousarray(np.concatenate(Js, axis=1)) if Js else None)
        tleaf.append([lf for (_, _, lf) in lev])
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=rowblocks,
                     eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": A, "task": tleaf, "bound": bleaf, "rows": rleaf}
    return plan, leaf


def perturb(leaf, rng, scale=0.01):
    """temporally coherent next cycle: every float input moves by ~1 % (MPC-rollout-like)."""
    def j(a):
        return None if a is None else a * (1.0 + scale * rng.standard_normal(a.shape))
    out = {"B": leaf["B"], "A": [j(a) for a in leaf["A"]],
           "task": [[tuple(j(x) for x in t) for t in lev] for lev in leaf["task"]],
           "bound": [tuple(j(x) for x in t) for t in leaf["bound"]],
           "rows": [tuple(j(x) for x in t) for t in leaf["rows"]]}
    if leaf.get("C") is not None:      # producer-written constraint rows (config 5: [B_u, -J_f'], [B, -Jc'])
        out["C"] = [j(a) for a in leaf["C"]]
    if leaf.get("W") is not None:      # dense task weights stay as they are (symmetric positive definite)
        out["W"] = leaf["W"]
    if "reg" in leaf:
        out["reg"] = tuple(j(x) for x in leaf["reg"])
    if "reg_A" in leaf:
        out["reg_A"] = j(leaf["reg_A"])
    return out


def add_regularisation(plan, leaf, kind=abi.TASK_GENERIC, rows=None, weight=1e-3, lam=0.1, seed=0, dense=False):
    """attach a user regularisation task (AutoStack::setRegularisationTask) to a synthetic stack: the reference's own
    use (tests/solvers/TestiHQP.cpp:112-120) is a minimum-velocity GenericTask(I, -qdot/dt); a Postural works alike.
    dense=True: a task with a STORED Jacobian (iHQP.cpp:265-278 takes any task): GENERIC (random A_r, b), CARTESIAN
    (6 rows: a link Jacobian and poses) or COM (3 rows); leaf["reg_A"] is A_r [B][rows][n]."""
    rng = np.random.default_rng(seed + 977)
    n, B = plan.n, leaf["B"]
    rows = n if rows is None else rows
    if dense:
        rows = {abi.TASK_CARTESIAN: 6, abi.TASK_COM: 3}.get(kind, rows)
        plan.regularisation = Task(kind, rows, weight=weight, lam=lam, name="regularisation")
        plan.regularisation_dense = True
        leaf["reg_A"] = rng.normal(0.0, 0.3, size=(B, rows, n))
        if kind == abi.TASK_CARTESIAN:
            leaf["reg"] = _cartesian_leaf(rng, B)
        elif kind == abi.TASK_COM:
            p = rng.uniform(-0.2, 0.2, size=(B, 3))
            leaf["reg"] = (p, p + rng.uniform(-0.05, 0.05, size=(B, 3)), None)
        else:
            leaf["reg"] = (rng.normal(0.0, 0.1, size=(B, rows)), None, None)
        return plan, leaf
    plan.regularisation = Task(kind, rows, weight=weight, lam=lam, lam2=2.0 * np.sqrt(lam), name="regularisation")
    if kind == abi.TASK_GENERIC:
        leaf["reg"] = (rng.normal(0.0, 0.1, size=(B, rows)), None, None)
    elif kind == abi.TASK_POSTURAL:
        q = rng.uniform(-1, 1, size=(B, rows))
        leaf["reg"] = (q, q + rng.normal(0, 0.1, size=(B, rows)), None)
    else:   # ACC_POSTURAL: [q_ref - q ; qdot_ref - qdot], qddot_ref
        leaf["reg"] = (rng.normal(0, 0.1, size=(B, 2 * rows)), None, rng.normal(0, 0.1, size=(B, rows)))
    return plan, leaf


def make_id_stack(B, seed=None, nv=38, n_contacts=4, eps_factor=1e6, torque_limits=True):
    """BASELINE config 5: floating-base inverse dynamics in torque mode, x = [qddot (nv); F (3 per point contact)]
    (src/utils/InverseDynamics.cpp:12-28; bindings/python/examples/LittleDog_id.py:60-106).

    levels : 0 = acceleration::CoM (3) + two acceleration::Cartesian (6 each)      [J 0] written by the producer
             1 = acceleration::Postural on qddot ([I_nv 0], implicit)
    rows   : DynamicFeasibility (6 eq) [B_u, -J_f'], FrictionCone (5 per contact), TorqueLimits (nv) [B, -Jc'],
             acceleration::JointLimits (nv unit rows), acceleration::VelocityLimits (nv unit rows)
    Model quantities (B, h, J, Jdot*qdot) are synthetic: B = L L' + I, h ~ N(0, 5^2), J ~ N(0, 0.3^2).
    (make_coman_id_stack is the stack whose model quantities come from the device producers.)
    The stack is feasible by construction around qddot = 0 with supporting contact forces.
    """
    rng = np.random.default_rng(5000 if seed is None else seed)
    nf = 3 * n_contacts
    n = nv + nf
    assert n <= abi.MAX_VARS
    # dynamics
    Lm = rng.normal(0.0, 0.3, size=(B, nv, nv))
    Bm = Lm @ np.transpose(Lm, (0, 2, 1)) + np.eye(nv)
    Jc = np.zeros((B, n_contacts, 3, nv))                      # point-contact linear Jacobians
    Jc[:, :, :, :6] = rng.normal(0.0, 0.5, size=(B, n_contacts, 3, 6))
    for ct in range(n_contacts):
        cols = 6 + ct * 6 + np.arange(6)
        Jc[:, ct][:, :, cols] = rng.normal(0.0, 0.3, size=(B, 3, 6))
    # contact frames and a nominal force inside every cone; h chosen so that (qddot = 0, F = F0) is dynamically
    # consistent on the floating base and well inside the torque limits
    wRl = _rot_exp(rng.normal(0.0, 0.15, size=(B, n_contacts, 3)))
    F0_local = np.concatenate([rng.uniform(-3, 3, size=(B, n_contacts, 2)), rng.uniform(40, 80, size=(B, n_contacts, 1))], axis=2)
    F0 = np.einsum("bcij,bcj->bci", wRl, F0_local)                # world frame
    JcT_F0 = np.einsum("bcij,bci->bj", Jc, F0)                    # sum_c Jc' F0
    h = JcT_F0 + np.concatenate([np.zeros((B, 6)), rng.normal(0.0, 5.0, size=(B, nv - 6))], axis=1)
    tau_max = np.full((B, nv), 30.0)                              # tight enough that some torque limits bind
    tau_max[:, :6] = 1.0e3                                        # floating-base rows: loose (equality handles them)
    # tasks
    Jcom = rng.normal(0.0, 0.3, size=(B, 3, nv))
    Jh = [_limb_jacobian(rng, B, 6, nv, list(range(0, 6)) + list(range(30 + 4 * k, 34 + 4 * k))) for k in range(2)]
    A0 = np.zeros((B, 15, n))
    A0[:, 0:3, :nv] = Jcom
    A0[:, 3:9, :nv] = Jh[0]
    A0[:, 9:15, :nv] = Jh[1]

    def acc_leaf(rows):
        pe = rng.normal(0.0, 0.02, size=(B, rows)); ve = rng.normal(0.0, 0.05, size=(B, rows))
        return np.concatenate([pe, ve], axis=1), rng.normal(0.0, 0.1, size=(B, rows)), None
    q = rng.uniform(-1.0, 1.0, size=(B, nv)); qd = rng.normal(0.0, 0.2, size=(B, nv))
    half = rng.uniform(1.5, 2.5, size=(B, nv))
    levels = [[Task(abi.TASK_ACC_COM, 3, lam=10.0, lam2=5.0, name="com"),
               Task(abi.TASK_ACC_CARTESIAN, 6, lam=10.0, lam2=5.0, name="l_hand"),
               Task(abi.TASK_ACC_CARTESIAN, 6, lam=10.0, lam2=5.0, name="r_hand")],
              [Task(abi.TASK_ACC_POSTURAL, nv, lam=10.0, lam2=5.0, name="postural")]]
    tleaf = [[acc_leaf(3), acc_leaf(6), acc_leaf(6)],
             [(np.concatenate([rng.normal(0.0, 0.1, size=(B, nv)), -qd], axis=1), None, None)]]
    # constraint rows written by the producer (zero-copy into C): dynamic feasibility and torque limits
    Cdyn = np.zeros((B, 6, n)); Ctau = np.zeros((B, nv, n))
    Cdyn[:, :, :nv] = Bm[:, :6, :]
    Ctau[:, :, :nv] = Bm
    for ct in range(n_contacts):
        # DynamicFeasibility.cpp:38-41: -(J[0:k, 0:6])' ; TorqueLimits.cpp:39-40: -(J[0:k, :])'
        Cdyn[:, :, nv + 3 * ct: nv + 3 * ct + 3] = -np.transpose(Jc[:, ct][:, :, :6], (0, 2, 1))
        Ctau[:, :, nv + 3 * ct: nv + 3 * ct + 3] = -np.transpose(Jc[:, ct], (0, 2, 1))
    rowblocks = [Rows(abi.ROWS_DYN_FEASIBILITY, 6, name="dynamic_feasibility"),
                 Rows(abi.ROWS_FRICTION_CONE, 5 * n_contacts, first_col=nv, mu=0.8, name="friction_cones")]
    rleaf = [(h[:, :6].copy(), None, None), (wRl.reshape(B, n_contacts, 9), None, None)]
    Cleaf = [Cdyn, None]
    if torque_limits:
        rowblocks.append(Rows(abi.ROWS_TORQUE_LIMITS, nv, name="torque_limits"))
        rleaf.append((h, tau_max, None)); Cleaf.append(Ctau)
    rowblocks.append(Rows(abi.ROWS_ACC_JOINT_LIMITS, nv, first_col=0, dT=0.001, p=20.0, name="joint_limits"))
    rleaf.append((np.concatenate([q, qd], axis=1), np.concatenate([-half, half], axis=1), np.full((B, nv), 500.0)))
    Cleaf.append(None)
    # four row blocks at most (OSOT_MAX_ROWBLOCKS): velocity limits only when torque limits are left out
    if not torque_limits:
        rowblocks.append(Rows(abi.ROWS_ACC_VELOCITY_LIMITS, nv, first_col=0, dT=0.001, p=20.0, name="velocity_limits"))
        rleaf.append((qd, np.full((B, nv), 20.0), None)); Cleaf.append(None)
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [A0, None], "task": tleaf, "bound": [], "rows": rleaf, "C": Cleaf,
            "model": {"B": Bm, "h": h, "Jc": Jc, "nv": nv}}
    return plan, leaf


def wrench_rows(kind, wRl, lims, mu):
    """the rows of one surface contact over its wrench [f; tau] (numpy, [B][rows][6]): A * blockdiag(wRl', wRl') with A the
    mu/sqrt(2) pyramid on f (force::FrictionCone, FrictionCone.cpp:35-56), Ai (force::CoP, CoP.cpp:24-69) or A0 * Ad2
    (force::NormalTorque, NormalTorque.cpp:5-69).  wRl [B][3][3], lims [B][4] = (x_l, x_u, y_l, y_u)."""
    B = wRl.shape[0]
    if kind == abi.ROWS_WRENCH_FRICTION_CONE:
        m = mu / np.sqrt(2.0)
        A = np.zeros((B, 5, 6))
        A[:, :, :3] = [[1, 0, -m], [-1, 0, -m], [0, 1, -m], [0, -1, -m], [0, 0, -1]]
    else:
        xl, xu, yl, yu = (lims[:, i] for i in range(4))
        if kind == abi.ROWS_COP:
            A = np.zeros((B, 4, 6))
            A[:, 0, 2], A[:, 0, 4] = xl, 1.0
            A[:, 1, 2], A[:, 1, 4] = -xu, -1.0
            A[:, 2, 2], A[:, 2, 3] = yl, -1.0
            A[:, 3, 2], A[:, 3, 3] = -yu, 1.0
        else:
            X = (np.abs(xl) + np.abs(xu)) / 2.0
            Y = (np.abs(yl) + np.abs(yu)) / 2.0
            K = -mu * (X + Y)
            sgn = np.array([[-1, -1, -1, -1, 1], [-1, 1, -1, 1, 1], [1, -1, 1, -1, 1], [1, 1, 1, 1, 1],
                            [1, 1, -1, -1, -1], [1, -1, -1, 1, -1], [-1, 1, 1, -1, -1], [-1, -1, 1, 1, -1]], dtype=float)
            A = np.zeros((B, 8, 6))
            A[:, :, 0] = sgn[None, :, 0] * Y[:, None]
            A[:, :, 1] = sgn[None, :, 1] * X[:, None]
            A[:, :, 2] = K[:, None]
            A[:, :, 3] = sgn[None, :, 2] * mu
            A[:, :, 4] = sgn[None, :, 3] * mu
            A[:, :, 5] = sgn[None, :, 4]
            Ad2 = np.broadcast_to(np.eye(6), (B, 6, 6)).copy()
            px, py = (xu + xl) / 2.0, (yu + yl) / 2.0
            Ad2[:, 3, 2], Ad2[:, 4, 2], Ad2[:, 5, 0], Ad2[:, 5, 1] = py, -px, -py, px
            A = A @ Ad2
    Ad = np.zeros((B, 6, 6))
    Rt = np.transpose(wRl, (0, 2, 1))
    Ad[:, :3, :3] = Rt
    Ad[:, 3:, 3:] = Rt
    return A @ Ad


def make_surface_id_stack(B, seed=None, nv=44, n_contacts=4, eps_factor=1e6):
    """floating-base inverse dynamics with SURFACE contacts: x = [qddot (nv); 6-D wrench [f; tau] per contact] (contact_dim = 6,
    src/utils/InverseDynamics.cpp:16-27): the feet and hands of a humanoid that stands and holds.  n = nv + 6 contacts; up to 64
    the wavefront route, 65 .. 128 the wide route (BatchedStack(route="auto")).

    levels : 0 = acceleration::CoM (3) + two acceleration::Cartesian (6 each)      [J 0] written by the producer
             1 = acceleration::Postural on qddot ([I_nv 0], implicit)
    rows   : DynamicFeasibility (6 eq) [B_u, -J_f'], force::FrictionCone on the wrenches (5 per contact), force::CoP (4 per
             contact), force::NormalTorque (8 per contact), TorqueLimits (nv) [B, -Jc'], acceleration::JointLimits (nv unit
             rows), force::WrenchLimits as unit rows on the wrench columns (6 per contact) -- seven blocks
    Feasible by construction: the nominal (qddot = 0, W0) is dynamically consistent on the floating base and W0 lies strictly
    inside every friction, CoP and normal-torque row (asserted); torque limits are tight enough that some bind."""
    rng = np.random.default_rng(7000 if seed is None else seed)
    nf = 6 * n_contacts
    n = nv + nf
    assert n <= abi.MAX_QP_VARS and nf <= abi.ID_MAX_FORCE_VARS and nv >= 16
    mu = 0.8
    # dynamics: B = L L' + I; each contact's 6 x nv Jacobian acts on the floating base and on a limb of 6 joints
    Lm = rng.normal(0.0, 0.3, size=(B, nv, nv))
    Bm = Lm @ np.transpose(Lm, (0, 2, 1)) + np.eye(nv)
    Jc = np.zeros((B, n_contacts, 6, nv))
    Jc[:, :, :, :6] = rng.normal(0.0, 0.5, size=(B, n_contacts, 6, 6))
    for ct in range(n_contacts):
        cols = 6 + (6 * ct + np.arange(6)) % (nv - 6)
        Jc[:, ct][:, :, cols] = rng.normal(0.0, 0.3, size=(B, 6, 6))
    # contact frames, foot rectangles and a nominal wrench inside every row: the CoP near the rectangle's middle, small
    # tangential forces and normal torque
    wRl = _rot_exp(rng.normal(0.0, 0.15, size=(B, n_contacts, 3)))
    lims = np.stack([rng.uniform(-0.12, -0.08, size=(B, n_contacts)), rng.uniform(0.10, 0.15, size=(B, n_contacts)),
                     rng.uniform(-0.07, -0.05, size=(B, n_contacts)), rng.uniform(0.05, 0.07, size=(B, n_contacts))], axis=2)
    fz = rng.uniform(40.0, 80.0, size=(B, n_contacts))
    f_loc = np.stack([rng.uniform(-3, 3, size=(B, n_contacts)), rng.uniform(-3, 3, size=(B, n_contacts)), fz], axis=2)
    cx = (lims[..., 0] + lims[..., 1]) / 2 + rng.uniform(-0.01, 0.01, size=(B, n_contacts))
    cy = (lims[..., 2] + lims[..., 3]) / 2 + rng.uniform(-0.01, 0.01, size=(B, n_contacts))
    t_loc = np.stack([cy * fz, -cx * fz, rng.uniform(-0.3, 0.3, size=(B, n_contacts))], axis=2)
    W0 = np.concatenate([np.einsum("bcij,bcj->bci", wRl, f_loc), np.einsum("bcij,bcj->bci", wRl, t_loc)], axis=2)
    for kind in (abi.ROWS_WRENCH_FRICTION_CONE, abi.ROWS_COP, abi.ROWS_NORMAL_TORQUE):
        for ct in range(n_contacts):
            v = np.einsum("brj,bj->br", wrench_rows(kind, wRl[:, ct], lims[:, ct], mu), W0[:, ct])
            assert v.max() < -1e-3, (kind, ct, v.max())
    h = np.einsum("bcij,bci->bj", Jc, W0) + np.concatenate([np.zeros((B, 6)), rng.normal(0.0, 5.0, size=(B, nv - 6))], axis=1)
    tau_max = np.full((B, nv), 30.0)
    tau_max[:, :6] = 1.0e3
    # tasks: CoM and the two hands on qddot
    Jcom = rng.normal(0.0, 0.3, size=(B, 3, nv))
    Jh = [_limb_jacobian(rng, B, 6, nv, list(range(0, 6)) + list(range(nv - 8 + 4 * k, nv - 4 + 4 * k))) for k in range(2)]
    A0 = np.zeros((B, 15, n))
    A0[:, 0:3, :nv] = Jcom
    A0[:, 3:9, :nv] = Jh[0]
    A0[:, 9:15, :nv] = Jh[1]

    def acc_leaf(rows):
        pe = rng.normal(0.0, 0.02, size=(B, rows)); ve = rng.normal(0.0, 0.05, size=(B, rows))
        return np.concatenate([pe, ve], axis=1), rng.normal(0.0, 0.1, size=(B, rows)), None
    q = rng.uniform(-1.0, 1.0, size=(B, nv)); qd = rng.normal(0.0, 0.2, size=(B, nv))
    half = rng.uniform(1.5, 2.5, size=(B, nv))
    levels = [[Task(abi.TASK_ACC_COM, 3, lam=10.0, lam2=5.0, name="com"),
               Task(abi.TASK_ACC_CARTESIAN, 6, lam=10.0, lam2=5.0, name="l_hand"),
               Task(abi.TASK_ACC_CARTESIAN, 6, lam=10.0, lam2=5.0, name="r_hand")],
              [Task(abi.TASK_ACC_POSTURAL, nv, lam=10.0, lam2=5.0, name="postural")]]
    tleaf = [[acc_leaf(3), acc_leaf(6), acc_leaf(6)],
             [(np.concatenate([rng.normal(0.0, 0.1, size=(B, nv)), -qd], axis=1), None, None)]]
    Cdyn = np.zeros((B, 6, n)); Ctau = np.zeros((B, nv, n))
    Cdyn[:, :, :nv] = Bm[:, :6, :]
    Ctau[:, :, :nv] = Bm
    for ct in range(n_contacts):
        Cdyn[:, :, nv + 6 * ct: nv + 6 * ct + 6] = -np.transpose(Jc[:, ct][:, :, :6], (0, 2, 1))
        Ctau[:, :, nv + 6 * ct: nv + 6 * ct + 6] = -np.transpose(Jc[:, ct], (0, 2, 1))
    R9, L4 = np.ascontiguousarray(wRl.reshape(B, n_contacts, 9)), np.ascontiguousarray(lims)
    wl = np.tile(np.array([-1.0e3, -1.0e3, -1.0e3, -200.0, -200.0, -200.0]), (B, n_contacts))   # WrenchLimits
    rowblocks = [Rows(abi.ROWS_DYN_FEASIBILITY, 6, name="dynamic_feasibility"),
                 Rows(abi.ROWS_WRENCH_FRICTION_CONE, 5 * n_contacts, first_col=nv, mu=mu, name="friction_cones"),
                 Rows(abi.ROWS_COP, 4 * n_contacts, first_col=nv, name="cop"),
                 Rows(abi.ROWS_NORMAL_TORQUE, 8 * n_contacts, first_col=nv, mu=mu, name="normal_torque"),
                 Rows(abi.ROWS_TORQUE_LIMITS, nv, name="torque_limits"),
                 Rows(abi.ROWS_ACC_JOINT_LIMITS, nv, first_col=0, dT=0.001, p=20.0, name="joint_limits"),
                 Rows(abi.ROWS_UNIT_GENERIC, nf, first_col=nv, name="wrench_limits")]
    rleaf = [(h[:, :6].copy(), None, None), (R9, None, None), (R9, L4, None), (R9, L4, None), (h, tau_max, None),
             (np.concatenate([q, qd], axis=1), np.concatenate([-half, half], axis=1), np.full((B, nv), 500.0)), (wl, -wl, None)]
    Cleaf = [Cdyn, None, None, None, Ctau, None, None]
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [A0, None], "task": tleaf, "bound": [], "rows": rleaf, "C": Cleaf,
            "model": {"B": Bm, "h": h, "Jc": Jc, "nv": nv}, "nominal": np.concatenate([np.zeros((B, nv)), W0.reshape(B, nf)], axis=1)}
    return plan, leaf


def computed_torque(leaf, x):
    """InverseDynamics::computedTorque (src/utils/InverseDynamics.cpp:57-96): tau = B qddot + h - sum_c Jc' F_c;
    the six floating-base rows must vanish.  The contact dimension (3: point contacts, 6: surface contacts) is Jc's."""
    md = leaf["model"]; nv = md["nv"]
    qdd = x[:, :nv]; F = x[:, nv:].reshape(x.shape[0], -1, md["Jc"].shape[2])
    return np.einsum("bij,bj->bi", md["B"], qdd) + md["h"] - np.einsum("bcij,bci->bj", md["Jc"], F)


def make_generic_stack(B, n, level_rows, n_eq=0, n_ineq=0, seed=0, box=0.5, duplicate_eq_in_level=None,
                       postural_last=True, eps_factor=1e6, n_local=0, local_level=0, unit_box=None, local_equality=False):
    """small generic stacks (tasks::GenericTask blocks, GenericConstraint rows, generic box) for robot-free tests:
    e.g. a Panda-like 7-variable 2-level stack, or stacks whose optimality rows duplicate global equality rows
    (the `<< (l_sole + r_sole)` situation of examples/cpp/coman_ik.cpp:442 where 39 equality rows meet 35
    variables).  duplicate_eq_in_level = k copies the global equality rows into level k's task (consistent b)."""
    rng = np.random.default_rng(seed)
    levels, A, tleaf = [], [], []
    Ceq = rng.normal(0.0, 0.5, size=(B, n_eq, n)) if n_eq else None
    beq = rng.uniform(-0.02, 0.02, size=(B, n_eq)) if n_eq else None
    for k, m in enumerate(level_rows):
        Ak = rng.normal(0.0, 0.4, size=(B, m, n))
        bk = rng.normal(0.0, 0.05, size=(B, m))
        if duplicate_eq_in_level == k and n_eq:
            Ak = np.concatenate([Ceq, Ak], axis=1); bk = np.concatenate([beq, bk], axis=1)
        levels.append([Task(abi.TASK_GENERIC, Ak.shape[1], name=f"generic{k}")])
        A.append(np.ascontiguousarray(Ak)); tleaf.append([(bk, None, None)])
    if postural_last:
        q = rng.uniform(-1, 1, size=(B, n))
        levels.append([Task(abi.TASK_POSTURAL, n, lam=0.1, name="postural")])
        A.append(None); tleaf.append([(q, q + rng.normal(0, 0.1, size=(B, n)), None)])
    rowblocks, rleaf = [], []
    if n_eq:
        rowblocks.append(Rows(abi.ROWS_GENERIC, n_eq, name="equalities")); rleaf.append((Ceq, beq, beq.copy()))
    if n_ineq:
        Ci = rng.normal(0.0, 0.5, size=(B, n_ineq, n))
        rowblocks.append(Rows(abi.ROWS_GENERIC, n_ineq, name="inequalities"))
        rleaf.append((Ci, -rng.uniform(0.01, 0.2, size=(B, n_ineq)), rng.uniform(0.01, 0.2, size=(B, n_ineq))))
    if n_local:   # task-local rows (`task << constraint`): tight enough to bind at their level
        Cl = rng.normal(0.0, 0.5, size=(B, n_local, n))
        rowblocks.append(Rows(abi.ROWS_GENERIC, n_local, name="task_local", level=local_level))
        lol, upl = -rng.uniform(0.001, 0.02, size=(B, n_local)), rng.uniform(0.001, 0.02, size=(B, n_local))
        if local_equality:   # `task << equality`: a row the solution of the level above does NOT satisfy
            upl = lol.copy()
        rleaf.append((Cl, lol, upl))
    if unit_box is not None:   # (level or None, half width): a box as unit rows; with a level: a task-local bound
        lvl, hw = unit_box
        rowblocks.append(Rows(abi.ROWS_UNIT_GENERIC, n, name="unit_box", first_col=0, level=lvl))
        rleaf.append((np.full((B, n), -hw), np.full((B, n), hw), None))
    bounds, bleaf = [], []
    if box:
        bounds.append(Bound(abi.BOUND_GENERIC, name="box")); bleaf.append((np.full((B, n), -box), np.full((B, n), box), None))
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    return plan, {"B": B, "A": A, "task": tleaf, "bound": bleaf, "rows": rleaf}


def make_lowrank_stack(B, n, m=3, seed=0, weight=0.3, postural_weight=None, dependent=False, zero_row=False,
                       second_level_rows=5, box=0.4, eps_factor=1e6):
    """a level with only a few stored rows (the closed-form low-rank path of the cascade kernel): m <= 4 generic
    rows with a non-unit weight, optionally sharing the level with a weighted Postural block (soft priority, as in
    coman_ik.cpp:429), optionally with a linearly dependent or an all-zero row; a second generic level and a box."""
    rng = np.random.default_rng(seed)
    A0 = rng.normal(0.0, 0.4, size=(B, m, n))
    b0 = rng.normal(0.0, 0.05, size=(B, m))
    if dependent and m >= 2:
        A0[:, m - 1] = 2.0 * A0[:, 0]          # dependent direction (inconsistent right-hand side: least squares)
    if zero_row:
        A0[:, min(1, m - 1)] = 0.0
    lev0 = [Task(abi.TASK_GENERIC, m, weight=weight, name="few_rows")]
    leaf0 = [(b0, None, None)]
    if postural_weight is not None:
        q = rng.uniform(-1, 1, size=(B, n))
        lev0.append(Task(abi.TASK_POSTURAL, n, weight=postural_weight, lam=0.1, name="postural_soft"))
        leaf0.append((q, q + rng.normal(0, 0.1, size=(B, n)), None))
    levels, A, tleaf = [lev0], [np.ascontiguousarray(A0)], [leaf0]
    if second_level_rows:
        A1 = rng.normal(0.0, 0.4, size=(B, second_level_rows, n))
        levels.append([Task(abi.TASK_GENERIC, second_level_rows, name="second")])
        A.append(A1); tleaf.append([(rng.normal(0.0, 0.05, size=(B, second_level_rows)), None, None)])
    bounds = [Bound(abi.BOUND_GENERIC, name="box")]
    bleaf = [(np.full((B, n), -box), np.full((B, n), box), None)]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=[], eps_abs=eps_abs_from_factor(eps_factor))
    return plan, {"B": B, "A": A, "task": tleaf, "bound": bleaf, "rows": []}


def make_subtask_stack(B, seed=0, n=32, eps_factor=1e6):
    """config-3-like stack built from SubTasks (`task % {rows}`, src/tasks/SubTask.cpp): CoM restricted to x, y with
    its own lambda; position-only wrists (rows 0..2 of the Cartesian tasks, one with a sub-task lambda of 0.5), full
    feet; a Postural sub-task on the actuated joints 6..n-1 (its unit rows are stored, not implicit)."""
    from .plan import subtask
    rng = np.random.default_rng(seed)
    com = Task(abi.TASK_COM, 3, lam=0.1, name="com")
    carts = {nm: Task(abi.TASK_CARTESIAN, 6, weight=(0.1 if nm == "l_wrist" else 1.0), lam=0.1, name=nm)
             for nm in ("l_wrist", "r_wrist", "l_sole", "r_sole")}
    post = Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural")
    lev0 = [subtask(com, [0, 1], lam=0.7)]
    lev1 = [subtask(carts["l_wrist"], [0, 1, 2], lam=0.5), subtask(carts["r_wrist"], [0, 1, 2]), carts["l_sole"], carts["r_sole"]]
    act = list(range(6, n))
    lev2 = [subtask(post, act, n=n)]
    bounds, bleaf = _box_leaf(rng, B, n, jl=True, vl=True)
    q = bleaf[0][0]
    A0 = rng.normal(0.0, 0.3, size=(B, 3, n))[:, [0, 1]]
    limb = {"l_wrist": "l_arm", "r_wrist": "r_arm", "l_sole": "l_leg", "r_sole": "r_leg"}
    J = {nm: _limb_jacobian(rng, B, 6, n, _BASE + _LIMBS[limb[nm]]) for nm in carts}
    A1 = np.concatenate([J["l_wrist"][:, :3], J["r_wrist"][:, :3], J["l_sole"], J["r_sole"]], axis=1)
    A2 = np.zeros((B, len(act), n))
    for r, jn in enumerate(act):
        A2[:, r, jn] = 1.0
    p = rng.uniform(-0.2, 0.2, size=(B, 3))
    tleaf = [[(p, p + rng.uniform(-0.05, 0.05, size=(B, 3)), None)],
             [_cartesian_leaf(rng, B) for _ in range(4)],
             [(q, q + rng.normal(0.0, 0.1, size=(B, n)), None)]]
    plan = StackPlan(n=n, levels=[lev0, lev1, lev2], bounds=bounds, rowblocks=[], eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [np.ascontiguousarray(A0), np.ascontiguousarray(A1), A2], "task": tleaf, "bound": bleaf, "rows": []}
    return plan, leaf


def make_feature_stack(B, seed=0, n=32, eps_factor=1e6, body_frame=True, dense=True, bands=True, candidates=24, many_blocks=True):
    """a velocity stack that exercises the options beyond the benchmark configurations (all of them parts of the reference's
    surface): a Cartesian task with a BODY Jacobian (Cartesian.cpp:93-100), a task with a full weight matrix
    (Task.h:273-300) next to scalar-weighted ones, TaskToConstraint rows with per-row error bands
    (TaskToConstraint.cpp:34-68), a collision block that picks its rows among more candidate pairs than rows
    (CollisionAvoidance.cpp:120-131), and more than four row blocks.  Returns (plan, leaf); leaf["W"] holds the weight
    matrices."""
    rng = np.random.default_rng(seed)
    bounds, bleaf = _box_leaf(rng, B, n, jl=True, vl=True)

    def cart(name, limb, weight=1.0, lam=0.1, **kw):
        return (Task(abi.TASK_CARTESIAN, 6, weight=weight, lam=lam, name=name, **kw),
                _limb_jacobian(rng, B, 6, n, _BASE + _LIMBS[limb]), _cartesian_leaf(rng, B))

    def spd(rows):
        M = rng.normal(0.0, 0.4, size=(B, rows, rows))
        return M @ np.transpose(M, (0, 2, 1)) + 0.5 * np.eye(rows)

    l0 = [cart("l_sole", "l_leg", body_frame=body_frame), cart("r_sole", "r_leg")]
    # (two tasks on the SAME limb: they conflict, so the weights -- and the off-diagonal entries of W -- shape the answer)
    l1 = [cart("l_wrist", "l_arm", weight=0.3, dense_weight=dense), cart("l_elbow", "l_arm", lam=0.2)]
    q = bleaf[0][0]
    l2 = [(Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural"), None, (q, q + rng.normal(0.0, 0.1, size=(B, n)), None))]
    levels, A, tleaf, Wl = [], [], [], []
    for lev in (l0, l1, l2):
        levels.append([t for (t, _, _) in lev])
        Js = [J for (_, J, _) in lev if J is not None]
        A.append(np.ascontiguousarray(np.concatenate(Js, axis=1)) if Js else None)
        tleaf.append([lf for (_, _, lf) in lev])
        Wl.append([spd(t.rows) if t.dense_weight else None for (t, _, _) in lev])
    rowblocks, rleaf, Cleaf = [], [], []
    # CoM as a constraint with a per-row band (TaskToConstraint with err_lb / err_ub vectors)
    p = rng.uniform(-0.2, 0.2, size=(B, 3))
    elb = [-0.02, -0.01, -0.03] if bands else 0.0
    eub = [0.01, 0.02, 0.0] if bands else 0.0
    rowblocks.append(Rows(abi.ROWS_TASK_COM, 3, lam=0.1, err_lb=elb, err_ub=eub, name="com_band"))
    rleaf.append((p, p + rng.uniform(-0.01, 0.01, size=(B, 3)), None)); Cleaf.append(rng.normal(0.0, 0.3, size=(B, 3, n)))
    # self-collision: `candidates` pairs supplied in arbitrary order, the 8 closest become rows
    P = 8
    Jd = np.zeros((B, candidates, n))
    for r in range(candidates):
        cols = rng.choice(np.arange(6, n), size=14, replace=False)
        Jd[:, r, cols] = rng.normal(0.0, 0.3, size=(B, 14))
    d = rng.uniform(0.0, 0.09, size=(B, candidates))
    rowblocks.append(Rows(abi.ROWS_COLLISION, P, d_threshold=0.0, detection_threshold=0.05, bound_scaling=1.0,
                          n_candidates=(candidates if candidates != P else 0), name="self_collision"))
    rleaf.append((Jd, d, None)); Cleaf.append(None)
    if many_blocks:   # four more (small) generic blocks: six row blocks in all
        for i in range(4):
            Ci = rng.normal(0.0, 0.5, size=(B, 2, n))
            rowblocks.append(Rows(abi.ROWS_GENERIC, 2, name=f"generic{i}"))
            rleaf.append((Ci, -rng.uniform(0.05, 0.3, size=(B, 2)), rng.uniform(0.05, 0.3, size=(B, 2)))); Cleaf.append(None)
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": A, "task": tleaf, "bound": bleaf, "rows": rleaf, "C": Cleaf, "W": Wl}
    return plan, leaf


def wide_id_levels(rng, nv=56, ncon=5, tau_max=60.0):
    """two levels of a floating-base inverse-dynamics stack WIDER than 64 variables as explicit QPs in BackEnd convention (the shape of
    src/utils/InverseDynamics.cpp:12-28): x = [qddot (nv); F (3 per point contact)]; rows: dynamic feasibility (6 equalities), friction
    pyramids (5 rows per contact), torque limits (nv - 6 bilateral rows); box: acceleration limits and force limits.  Level 0: 15 task
    rows on qddot (a CoM and two Cartesian tasks), level 1: a Postural task on qddot under level 0's optimality rows.
    Returns (n, level) with level(k, xs) -> (H, g, A, lA, uA, l, u), xs = the solutions of the levels above."""
    nf = 3 * ncon
    n = nv + nf
    Q = rng.normal(size=(nv, nv)) * 0.3
    M = Q.T @ Q + np.eye(nv) * 2.0
    Jc = rng.normal(size=(nf, nv)) * 0.5
    h = rng.normal(size=nv) * 2.0
    h[2] += 9.81 * 5.0
    dyn = np.hstack([M, -Jc.T])
    rows, lo, up = [], [], []
    for r in range(6):
        rows.append(dyn[r]); lo.append(-h[r]); up.append(-h[r])
    mu = 0.7
    for c in range(ncon):
        fx, fy, fz = nv + 3 * c, nv + 3 * c + 1, nv + 3 * c + 2
        for (a, sgn) in ((fx, 1), (fx, -1), (fy, 1), (fy, -1)):
            row = np.zeros(n); row[a] = sgn; row[fz] = -mu
            rows.append(row); lo.append(-np.inf); up.append(0.0)
        row = np.zeros(n); row[fz] = 1.0
        rows.append(row); lo.append(0.0); up.append(1.0e3)
    for r in range(6, nv):
        rows.append(dyn[r]); lo.append(-tau_max - h[r]); up.append(tau_max - h[r])
    Cm, lo, up = np.array(rows), np.array(lo), np.array(up)
    l = np.concatenate([-np.full(nv, 80.0), np.full(nf, -1.0e3)])
    u = np.concatenate([np.full(nv, 80.0), np.full(nf, 1.0e3)])
    m0 = 15
    A0 = np.hstack([rng.normal(size=(m0, nv)) * 0.6, np.zeros((m0, nf))])
    b0 = rng.normal(size=m0) * 3.0
    qref = rng.normal(size=nv) * 0.5

    def level(k, xs):
        if k == 0:
            return A0.T @ A0, -A0.T @ b0, Cm, lo, up, l, u
        H = np.zeros((n, n)); H[:nv, :nv] = np.eye(nv)
        g = np.zeros(n); g[:nv] = -qref
        t = A0 @ xs[0]
        return H, g, np.vstack([Cm, A0]), np.concatenate([lo, t]), np.concatenate([up, t]), l, u
    return n, level


def make_wide_robot_stack(B, n=96, levels=3, seed=0, eps_factor=1e6, n_ineq=16, n_local=8):
    """a robot-like velocity stack WIDER than a wavefront (n = 65 .. 128: a 45-DoF humanoid with a floating base and hands): CoM and
    the feet first, the hands and the head next, an implicit Postural block last (levels = 3; levels = 2 folds the first two), joint
    and velocity limits, generic inequality rows on every level and task-local rows of the middle level (`task << constraint`).
    Columns: the 6 floating-base coordinates, then five limbs of (n - 6) / 5 joints each.  Returns (plan, leaf) as
    make_velocity_stack; the workgroup route (BatchedStack(route="wide")) and tools/bench_wide_plan.py run it."""
    assert 7 <= n <= abi.MAX_QP_VARS and levels in (2, 3)
    rng = np.random.default_rng(seed)
    limb = (n - 6) // 5
    limbs = {nm: list(range(6 + i * limb, 6 + (i + 1) * limb)) for i, nm in enumerate(("l_leg", "r_leg", "l_arm", "r_arm", "head"))}
    limbs["head"] = list(range(6 + 4 * limb, n))      # (the remainder of the columns)

    def cart(name, cols, weight=1.0, lam=0.1):
        return Task(abi.TASK_CARTESIAN, 6, weight=weight, lam=lam, name=name), _limb_jacobian(rng, B, 6, n, _BASE + cols), _cartesian_leaf(rng, B)

    def com(lam=0.1):
        p = rng.uniform(-0.2, 0.2, size=(B, 3))
        return (Task(abi.TASK_COM, 3, lam=lam, name="com"), rng.normal(0.0, 0.3, size=(B, 3, n)) / np.sqrt(n / 32.0),
                (p, p + rng.uniform(-0.05, 0.05, size=(B, 3)), None))

    bounds, bleaf = _box_leaf(rng, B, n, jl=True, vl=True)
    first = [com(), cart("l_sole", limbs["l_leg"]), cart("r_sole", limbs["r_leg"])]
    second = [cart("l_wrist", limbs["l_arm"], weight=0.1), cart("r_wrist", limbs["r_arm"]), cart("gaze", limbs["head"], weight=0.5)]
    q = bleaf[0][0]
    post = (Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural"), None, (q, q + rng.normal(0.0, 0.1, size=(B, n)), None))
    blocks = [first, second, [post]] if levels == 3 else [first + second, [post]]
    plan_levels, A, tleaf = [], [], []
    for lev in blocks:
        plan_levels.append([t for (t, _, _) in lev])
        Js = [J for (_, J, _) in lev if J is not None]
        A.append(np.ascontiguousarray(np.concatenate(Js, axis=1)) if Js else None)
        tleaf.append([lf for (_, _, lf) in lev])
    rowblocks, rleaf = [], []
    if n_ineq:
        Ci = rng.normal(0.0, 0.3, size=(B, n_ineq, n)) / np.sqrt(n / 32.0)
        rowblocks.append(Rows(abi.ROWS_GENERIC, n_ineq, name="inequalities"))
        rleaf.append((Ci, -rng.uniform(0.01, 0.1, size=(B, n_ineq)), rng.uniform(0.01, 0.1, size=(B, n_ineq))))
    if n_local:
        Cl = rng.normal(0.0, 0.3, size=(B, n_local, n)) / np.sqrt(n / 32.0)
        rowblocks.append(Rows(abi.ROWS_GENERIC, n_local, name="task_local", level=len(blocks) - 2))
        rleaf.append((Cl, -rng.uniform(0.002, 0.02, size=(B, n_local)), rng.uniform(0.002, 0.02, size=(B, n_local))))
    plan = StackPlan(n=n, levels=plan_levels, bounds=bounds, rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    return plan, {"B": B, "A": A, "task": tleaf, "bound": bleaf, "rows": rleaf}


def make_coman_id_stack(B, seed=None, tree=None, inertia=None, eps_factor=1e6):
    """Floating-base inverse dynamics of the reference's COMAN (35 coordinates) standing on both soles as SURFACE contacts:
    x = [qddot (35); wrench l_sole (6); wrench r_sole (6)], n = 47 (wavefront route).  The MODEL QUANTITIES ARE LEFT FOR THE PRODUCERS
    (opensot_amd.dynamics.IdStep: osot_kinematics + osot_dynamics every step); the leaf carries references, limits and the state.

    levels : 0 = acceleration::Contact on l_sole and r_sole (6 rows each: J qddot = -Jdot qdot) + acceleration::CoM (3)
             1 = acceleration::Postural on the 35 coordinates
    rows   : DynamicFeasibility (6), force::FrictionCone on the two wrenches (10), force::CoP (8), TorqueLimits (35)
    The posture is a standing one, knees bent, soles flat, at rest; the postural reference moves the arms and the waist by a few
    hundredths of a radian, so the robot moves while the wrenches stay well inside the cones and the CoP rectangles (the contact
    frame of cones and CoP is the ground: identity).  Returns (plan, leaf, model); leaf["state"] = q0, qdot0, q_ref."""
    import os
    from . import kinematics as kin
    here = os.path.dirname(os.path.abspath(__file__))
    gold = os.path.join(os.path.dirname(here), "tests", "golden")
    model, lo, up = kin.from_json(tree or os.path.join(gold, "coman_tree.json"), inertia or os.path.join(gold, "coman_inertia.json"))
    rng = np.random.default_rng(9000 if seed is None else seed)
    nv, nf = model.n, 12
    n = nv + nf
    ix = model.names.index
    q0 = np.zeros((B, nv))
    for s_ in "LR":
        q0[:, ix(s_ + "HipSag")] = -0.3; q0[:, ix(s_ + "KneeSag")] = 0.6; q0[:, ix(s_ + "AnkSag")] = -0.3
        q0[:, ix(s_ + "Elbj")] = -0.8; q0[:, ix(s_ + "ShSag")] = 0.2
    q0[:, ix("LShLat")] = 0.3; q0[:, ix("RShLat")] = -0.3
    upper = list(range(ix("WaistLat"), ix("RHipSag")))          # waist and arms
    q0[:, upper] += rng.normal(0.0, 0.02, (B, len(upper)))
    q0 = np.clip(q0, np.maximum(lo, -10.0) + 1e-3, np.minimum(up, 10.0) - 1e-3)
    q_ref = q0.copy()
    q_ref[:, upper] += rng.uniform(-0.05, 0.05, (B, len(upper)))
    z = lambda *sh: np.zeros(sh)
    levels = [[Task(abi.TASK_ACC_CARTESIAN, 6, lam=0.0, lam2=0.0, name="l_sole_contact"),
               Task(abi.TASK_ACC_CARTESIAN, 6, lam=0.0, lam2=0.0, name="r_sole_contact"),
               Task(abi.TASK_ACC_COM, 3, lam=25.0, lam2=10.0, name="com")],
              [Task(abi.TASK_ACC_POSTURAL, nv, lam=25.0, lam2=10.0, name="postural")]]
    tleaf = [[(z(B, 12), z(B, 6), None), (z(B, 12), z(B, 6), None), (z(B, 6), z(B, 3), None)],
             [(np.concatenate([q_ref - q0, z(B, nv)], axis=1), None, None)]]
    R9 = np.tile(np.eye(3).reshape(9), (B, 2, 1))
    lims = np.tile(np.array([-0.06, 0.12, -0.045, 0.045]), (B, 2, 1))       # the sole rectangle around the sole frame's origin
    tau_max = np.full((B, nv), 60.0)
    tau_max[:, :6] = 1.0e3                                      # floating-base rows: the equality handles them
    mu = 0.8
    rowblocks = [Rows(abi.ROWS_DYN_FEASIBILITY, 6, name="dynamic_feasibility"),
                 Rows(abi.ROWS_WRENCH_FRICTION_CONE, 10, first_col=nv, mu=mu, name="friction_cones"),
                 Rows(abi.ROWS_COP, 8, first_col=nv, name="cop"),
                 Rows(abi.ROWS_TORQUE_LIMITS, nv, name="torque_limits")]
    rleaf = [(z(B, 6), None, None), (R9, None, None), (R9, lims, None), (z(B, nv), tau_max, None)]
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [z(B, 15, n), None], "task": tleaf, "bound": [], "rows": rleaf, "C": [None] * 4,
            "state": {"q0": q0, "qdot0": z(B, nv), "q_ref": q_ref}, "contacts": ("l_sole", "r_sole"), "nv": nv}
    return plan, leaf, model


def make_coman_id_tracking_stack(B, gain_type=abi.ACC_GAIN_ACCELERATION, seed=None, tree=None, inertia=None, hand="l_wrist", eps_factor=1e6):
    """make_coman_id_stack with TRACKING tasks whose leaves osot_acc_tasks writes (opensot_amd.dynamics.IdTrackingStep), n = 47:

    levels : 0 = acceleration::Contact on l_sole and r_sole (6 rows each) + acceleration::CoM (3), as in make_coman_id_stack
             1 = acceleration::Cartesian on `hand` (6 rows) with Kp, Kd MATRICES, following a reference pose that moves with a
                 reference twist; with gain_type = abi.ACC_GAIN_FORCE the gains are Mi Kp, Mi Kd (GainType::Force) and a virtual
                 force enters as a_ref + Mi f
             2 = acceleration::Postural with matrix gains (Force variant: M^-1 in front of them): the producer's qddot_d is the
                 block's p2, the plan's lambda = lambda2 = 0 on it
    rows   : as make_coman_id_stack
    leaf["state"]["tracking"]: hand (frame name), gain_type, Kp, Kd (6 x 6), orientation_gain, offset [B][3] (the reference starts that
    far from the hand's first pose), vel_ref [B][6] (towards the hand: the reference and the hand meet), f_virtual [B][6] or None,
    post_Kp / post_Kd (nv x nv), post_lam / post_lam2.  Returns (plan, leaf, model)."""
    plan0, leaf, model = make_coman_id_stack(B, seed=seed, tree=tree, inertia=inertia, eps_factor=eps_factor)
    rng = np.random.default_rng(9100 if seed is None else seed + 100)
    nv, n = model.n, plan0.n
    force = gain_type == abi.ACC_GAIN_FORCE
    z = lambda *sh: np.zeros(sh)
    S = rng.uniform(-1.0, 1.0, (6, 6))
    # Acceleration type: Kp in 1 / s^2.  Force type: a stiffness in N / m in front of Mi, which at the wrist is the inverse of a few
    # hundredths of a kilogram (Mi Kp comes to about 200 / s^2: the explicit 1 ms integration of IdStep stays far from its limit)
    Kp = (10.0 if force else 100.0) * (np.eye(6) + 0.05 * (S + S.T))
    Kd = (1.0 if force else 20.0) * np.eye(6)
    offset = rng.uniform(0.01, 0.02, (B, 3)) * rng.choice([-1.0, 1.0], (B, 3))
    vel_ref = np.concatenate([-0.5 * offset, z(B, 3)], axis=1)
    d = rng.uniform(0.8, 1.2, nv)
    post_Kp, post_Kd = (0.2 if force else 25.0) * np.diag(d), (0.04 if force else 10.0) * np.diag(d)
    levels = [plan0.levels[0],
              [Task(abi.TASK_ACC_CARTESIAN, 6, lam=1.0, lam2=1.0, orientation_gain=1.0, name=hand, acc_gain_matrices=True)],
              [Task(abi.TASK_ACC_POSTURAL, nv, lam=0.0, lam2=0.0, name="postural")]]
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=plan0.rowblocks, eps_abs=plan0.eps_abs)
    leaf = dict(leaf)
    leaf["A"] = [leaf["A"][0], z(B, 6, n), None]
    leaf["task"] = [leaf["task"][0], [(z(B, 84), z(B, 6), z(B, 6))], [(z(B, 2 * nv), None, z(B, nv))]]
    leaf["state"] = dict(leaf["state"], tracking=dict(
        hand=hand, gain_type=int(gain_type), Kp=Kp, Kd=Kd, orientation_gain=1.0, offset=offset, vel_ref=vel_ref,
        f_virtual=np.tile(np.array([0.0, 0.0, 0.1, 0.0, 0.0, 0.0]), (B, 1)) if force else None,
        post_Kp=post_Kp, post_Kd=post_Kd, post_lam=1.0, post_lam2=1.0))
    return plan, leaf, model


# the sole rectangle around a sole frame's origin (x_l, x_u, y_l, y_u): the CoP limits of make_coman_id_stack, and the corners of the
# support polygon of make_coman_balance_stack
SOLE_RECTANGLE = (-0.06, 0.12, -0.045, 0.045)


def make_balance_stack(B, seed=None, n=32, P=8, margin=0.002, eps_factor=1e6):
    """A velocity stack with the balance constraint of the reference's walking / whole-body IK stacks,
    `(com / postural) << joint_limits << velocity_limits << convex_hull` (constraints::velocity::ConvexHull, ConvexHull.cpp:41-134):

    levels : 0 = velocity::CoM (3 rows; its Jacobian is the hull block's leaf p0: one [B][3][n] array), 1 = velocity::Postural
    box    : joint limits, velocity limits
    rows   : OSOT_ROWS_CONVEX_HULL on P contact points, safety margin `margin`

    Model quantities are synthetic: com_J ~ N(0, 0.3^2), the contact points a polygon around the CoM (in shuffled order, a quarter of
    them inside it), so dq = 0 is feasible; the CoM reference lies 0.1 .. 0.3 m away, beyond the polygon, so hull rows become active."""
    rng = np.random.default_rng(11000 if seed is None else seed)
    assert 3 <= P <= abi.KIN_MAX_POINTS
    bounds, bleaf = _box_leaf(rng, B, n, jl=True, vl=True)
    Jcom = rng.normal(0.0, 0.3, size=(B, 3, n))
    com = rng.uniform(-0.2, 0.2, size=(B, 3))
    ang = rng.uniform(0.0, 2.0 * np.pi, size=(B, 1))
    pd = com + np.concatenate([np.cos(ang), np.sin(ang), np.zeros((B, 1))], axis=1) * rng.uniform(0.1, 0.3, size=(B, 1))
    nh = max(3, P - P // 4)                                     # points on the polygon; the rest lie inside
    th = 2.0 * np.pi * (np.arange(nh)[None, :] + rng.uniform(-0.15, 0.15, size=(B, nh))) / nh + rng.uniform(0.0, 2.0 * np.pi, size=(B, 1))
    rad = rng.uniform(0.03, 0.06, size=(B, nh))
    rad = np.concatenate([rad, rad[:, :P - nh] * rng.uniform(0.1, 0.4, size=(B, P - nh))], axis=1)
    th = np.concatenate([th, rng.uniform(0.0, 2.0 * np.pi, size=(B, P - nh))], axis=1)
    pts = np.stack([com[:, :1] + rad * np.cos(th), com[:, 1:2] + rad * np.sin(th), rng.uniform(-0.9, -0.8, size=(B, P))], axis=2)
    pts = np.ascontiguousarray(np.take_along_axis(pts, np.argsort(rng.random((B, P)), axis=1)[:, :, None], axis=1))
    q = bleaf[0][0]
    levels = [[Task(abi.TASK_COM, 3, lam=1.0, name="com")], [Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural")]]
    tleaf = [[(com, pd, None)], [(q, q + rng.normal(0.0, 0.1, size=(B, n)), None)]]
    rowblocks = [Rows(abi.ROWS_CONVEX_HULL, P, bound_scaling=margin, name="convex_hull")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [Jcom, None], "task": tleaf, "bound": bleaf, "rows": [(Jcom, com, pts)], "C": [None]}
    return plan, leaf


def make_coman_balance_stack(B, seed=None, tree=None, margin=0.02, eps_factor=1e6):
    """The same stack on the reference's COMAN (35 coordinates) with every model quantity LEFT FOR THE KINEMATICS PRODUCER: the CoM, its
    Jacobian (written into A_0, which is also the hull block's leaf p0) and the eight contact points -- the four corners of each sole
    (SOLE_RECTANGLE around the l_sole / r_sole frames) on the two feet's links (KinModel.add_point).  A closed loop through
    osot_control_cycle / osot_control_rollout never leaves the device: the polygon follows the posture.
    The posture is a standing one, knees bent; the CoM reference lies `push` = 0.3 m ahead and to the side, beyond the polygon.
    Returns (plan, leaf, model); leaf["state"] = q0, q_ref, push.  bind_balance() wires the device tensors."""
    import os
    from . import kinematics as kin
    here = os.path.dirname(os.path.abspath(__file__))
    model, lo, up = kin.from_json(tree or os.path.join(os.path.dirname(here), "tests", "golden", "coman_tree.json"))
    rng = np.random.default_rng(12000 if seed is None else seed)
    n = model.n
    ix = model.names.index
    xl, xu, yl, yu = SOLE_RECTANGLE
    for name in ("l_sole", "r_sole"):
        _, jf, Rf, pf = model.frames[model.frame_index(name)]
        for cx, cy in ((xl, yl), (xu, yl), (xu, yu), (xl, yu)):
            model.add_point(jf, np.asarray(pf, dtype=float) + np.asarray(Rf, dtype=float) @ np.array([cx, cy, 0.0]))
    q0 = np.zeros((B, n))
    for s_ in "LR":
        q0[:, ix(s_ + "HipSag")] = -0.3; q0[:, ix(s_ + "KneeSag")] = 0.6; q0[:, ix(s_ + "AnkSag")] = -0.3
        q0[:, ix(s_ + "Elbj")] = -0.8; q0[:, ix(s_ + "ShSag")] = 0.2
    q0[:, ix("LShLat")] = 0.3; q0[:, ix("RShLat")] = -0.3
    q0[:, 6:] += rng.normal(0.0, 0.02, (B, n - 6))
    qmin, qmax = np.maximum(lo, -10.0), np.minimum(up, 10.0)
    q0 = np.clip(q0, qmin + 1e-3, qmax - 1e-3)
    q_ref = q0 + rng.uniform(-0.05, 0.05, (B, n))
    ang = rng.uniform(0.0, 2.0 * np.pi, size=(B, 1))
    push = 0.3 * np.concatenate([np.cos(ang), np.sin(ang), np.zeros((B, 1))], axis=1)
    z = lambda *sh: np.zeros(sh)
    levels = [[Task(abi.TASK_COM, 3, lam=1.0, name="com")], [Task(abi.TASK_POSTURAL, n, lam=0.1, name="postural")]]
    bounds = [Bound(abi.BOUND_JOINT_LIMITS, scaling=1.0, name="joint_limits"), Bound(abi.BOUND_VELOCITY_LIMITS, dT=0.05, name="velocity_limits")]
    rowblocks = [Rows(abi.ROWS_CONVEX_HULL, len(model.points), bound_scaling=margin, name="convex_hull")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [z(B, 3, n), None], "task": [[(z(B, 3), z(B, 3), None)], [(q0.copy(), q_ref, None)]],
            "bound": [(q0.copy(), np.tile(qmin, (B, 1)), np.tile(qmax, (B, 1))), (np.full((B, n), 2.0), None, None)],
            "rows": [(z(B, 3, n), z(B, 3), z(B, len(model.points), 3))], "C": [None],
            "state": {"q0": q0, "q_ref": q_ref, "push": push}}
    return plan, leaf, model


def bind_balance(stack, kin, leaf):
    """wire make_coman_balance_stack to the device: one q tensor is the producer's input, the Postural task's and the joint limits' q
    (and what q_integrate advances); the producer writes the CoM into the CoM task's and the hull block's leaf, its Jacobian into
    stack.A[0] (= the hull block's p0) and the contact points into the hull block's p2.  The CoM reference is the first posture's CoM
    plus leaf["state"]["push"].  -> (dev_leaf, kin_batch, q)"""
    import torch
    B = leaf["B"]
    dev = stack.load_leaf(leaf)
    f64 = dict(dtype=torch.float64, device=stack.device)
    q = torch.as_tensor(leaf["state"]["q0"], **f64).contiguous()
    com = torch.zeros((B, 3), **f64)
    pts = torch.zeros((B, len(kin.model.points), 3), **f64)
    kw = dict(com=com, com_J=(stack.A[0], 0), points=pts)
    kin.forward(q, **kw)
    com_ref = com.clone() + torch.as_tensor(leaf["state"]["push"], **f64)
    dev["task"][0][0] = (com, com_ref, None)
    dev["task"][1][0] = (q, dev["task"][1][0][1], None)
    dev["bound"][0] = (q,) + tuple(dev["bound"][0][1:])
    dev["rows"][0] = (stack.A[0], com, pts)
    return dev, kin.batch_args(q, **kw), q


# ---- the recursively feasible joint limits, the Cartesian position constraint, CartesianVelocity ----------------------------------
def near_limit_states(rng, B, n, qmin, qmax, amax):
    """i.i.d. states that exercise the joint-limit kinds where a closed loop does not go (the swap branch of ECBF): q within
    10^U(-4, -1) of a limit (upper or lower with equal odds), qdot ~ N(0, 1) sqrt(2 amax gap) -- velocities of the size that just
    stops inside the gap.  -> q, qdot [B][n]"""
    gap = 10.0 ** rng.uniform(-4.0, -1.0, size=(B, n))
    upper = rng.random((B, n)) < 0.5
    q = np.where(upper, qmax - gap, qmin + gap)
    qdot = rng.normal(size=(B, n)) * np.sqrt(2.0 * amax * gap)
    return q, qdot


def make_viability_stack(B, n, kind=abi.ROWS_ACC_JOINT_LIMITS_VIABILITY, seed=None, dT=0.01, p=1.0, qdot_max=2.0, qddot_max=12.0,
                         alpha=15.0, lam=400.0, first_col=0, rows=None, eps_factor=1e6):
    """`postural << joint_limits` of the reference's closed-loop joint-limit tests (tests/constraints/acceleration/
    TestJointLimitsViability.cpp, TestJointLimitsECBF.cpp) without a robot: one level, acceleration::Postural (lambda, lambda2 =
    2 sqrt(lambda)) on all n coordinates, under ONE block of `kind` (ROWS_ACC_JOINT_LIMITS_VIABILITY with the step-ahead predictor p,
    or ROWS_ACC_JOINT_LIMITS_ECBF with a1 = a2 = a3 = alpha) on the coordinates first_col .. first_col + rows - 1 (default: all).
    Limits +-U(0.5, 2.5); the start is the middle of the range, at rest.  The leaf's q is q - q_neutral with a zero neutral
    posture (see OSOT_ROWS_ACC_JOINT_LIMITS_VIABILITY in the header for the convention).
    leaf["state"]: q, qdot [B][n], qmin, qmax [B][rows]; set_viability_state() writes a state into the leaf in place."""
    assert kind in (abi.ROWS_ACC_JOINT_LIMITS_VIABILITY, abi.ROWS_ACC_JOINT_LIMITS_ECBF)
    rng = np.random.default_rng(13000 if seed is None else seed)
    rows = n - first_col if rows is None else rows
    half = rng.uniform(0.5, 2.5, size=(B, rows))
    qmin, qmax = -half, half
    q, qdot = np.zeros((B, n)), np.zeros((B, n))
    q[:, first_col:first_col + rows] = 0.5 * (qmin + qmax)
    lim = [np.full((B, rows), qdot_max), np.full((B, rows), qddot_max)]
    if kind == abi.ROWS_ACC_JOINT_LIMITS_ECBF:
        lim += [np.full((B, rows), float(alpha))] * 3
    levels = [[Task(abi.TASK_ACC_POSTURAL, n, lam=lam, lam2=2.0 * np.sqrt(lam), name="postural")]]
    rowblocks = [Rows(kind, rows, first_col=first_col, dT=dT, p=p, name="joint_limits")]
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [None], "task": [[(np.zeros((B, 2 * n)), None, None)]], "bound": [],
            "rows": [(np.zeros((B, 2 * rows)), np.concatenate([qmin, qmax], axis=1), np.concatenate(lim, axis=1))], "C": [None],
            "state": {"q": q, "qdot": qdot, "qmin": qmin, "qmax": qmax}}
    set_viability_state(plan, leaf, q, qdot, q)
    return plan, leaf


def set_viability_state(plan, leaf, q, qdot, q_ref):
    """write the state (q, qdot [B][n]) and the posture reference q_ref [B][n] into the leaf arrays of make_viability_stack, in place:
    the Postural task's [q_ref - q ; -qdot] and the limit block's [q ; qdot] on its columns"""
    n, rb = plan.n, plan.rowblocks[0]
    c0, r = rb.first_col, rb.rows
    t0 = leaf["task"][0][0][0]
    t0[:, :n] = q_ref - q
    t0[:, n:] = -qdot
    r0 = leaf["rows"][0][0]
    r0[:, :r] = q[:, c0:c0 + r]
    r0[:, r:] = qdot[:, c0:c0 + r]


def make_invariance_stack(B, n, seed=None, dt=1e-3, p=0.9, qdot_max=2.0, qddot_max=20.0, lam=0.1, eps_factor=1e6):
    """`postural << velocity_limits << joint_limits_invariance` of the reference's tests/constraints/velocity/
    TestJointLimitsInvariance.cpp without a robot: velocity::Postural (lambda) under BOUND_VELOCITY_LIMITS (qdot_max, dT = dt) and
    BOUND_JOINT_LIMITS_INVARIANCE (qddot_max, dt, the step-ahead predictor p).  Limits +-U(0.5, 2.5); the start is the middle of the
    range, at rest.  Per cycle the caller integrates q += dq and writes qdot_prev = dq / dt into the bound's leaf p2.
    leaf["state"]: q, qmin, qmax [B][n]."""
    rng = np.random.default_rng(14000 if seed is None else seed)
    half = rng.uniform(0.5, 2.5, size=(B, n))
    qmin, qmax = -half, half
    q = 0.5 * (qmin + qmax)
    levels = [[Task(abi.TASK_POSTURAL, n, lam=lam, name="postural")]]
    bounds = [Bound(abi.BOUND_VELOCITY_LIMITS, dT=dt, name="velocity_limits"),
              Bound(abi.BOUND_JOINT_LIMITS_INVARIANCE, scaling=p, dT=dt, name="joint_limits_invariance")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=[], eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [None], "task": [[(q.copy(), q.copy(), None)]],
            "bound": [(np.full((B, n), qdot_max), None, None),
                      (q.copy(), np.concatenate([qmin, qmax, np.full((B, n), qddot_max)], axis=1), np.zeros((B, n)))],
            "rows": [], "C": [], "state": {"q": q, "qmin": qmin, "qmax": qmax}}
    return plan, leaf


def make_position_stack(B, n, R, seed=None, kind=abi.ROWS_POSITION_CARTESIAN, bound_scaling=1.0, eps_factor=1e6):
    """A velocity stack under the reference's workspace constraint, `(task / postural) << joint_limits << velocity_limits <<
    position_constraint` (constraints::velocity::CartesianPositionConstraint, CartesianPositionConstraint.cpp:81-108):

    levels : 0 = velocity::Cartesian on a link (ROWS_POSITION_CARTESIAN) or velocity::CoM (ROWS_POSITION_COM); its Jacobian A_0 is
             the position block's leaf p0 (one [B][6][n] / [B][3][n] array), its actual pose / CoM the block's p1;  1 = Postural
    box    : joint limits, velocity limits
    rows   : R half-spaces A_c x <= b_c on the link's / the CoM's position

    Model quantities are synthetic (J ~ N(0, 0.3^2), a random pose).  Half-space 0 has the direction of the task's position error as its
    normal; in every second instance it lies 30 % of the way to where the task's gain would take the position in one step, so the
    unconstrained optimum violates it; elsewhere it lies beyond the reference.  The others are random planes 0.05 .. 0.2 m away."""
    assert kind in (abi.ROWS_POSITION_CARTESIAN, abi.ROWS_POSITION_COM) and 1 <= R <= abi.MAX_POSITION_ROWS
    rng = np.random.default_rng(15000 if seed is None else seed)
    cart = kind == abi.ROWS_POSITION_CARTESIAN
    lam = 0.1
    bounds, bleaf = _box_leaf(rng, B, n, jl=True, vl=True)
    mt = 6 if cart else 3
    J = rng.normal(0.0, 0.3, size=(B, mt, n))
    if cart:
        Ta, Td, _ = _cartesian_leaf(rng, B)
        x, xd = Ta[:, 9:], Td[:, 9:]
        task, tl = Task(abi.TASK_CARTESIAN, 6, lam=lam, name="link"), (Ta, Td, None)
    else:
        x = rng.uniform(-0.2, 0.2, size=(B, 3))
        dp = rng.normal(size=(B, 3))
        xd = x + dp * (rng.uniform(0.02, 0.05, size=(B, 1)) / np.linalg.norm(dp, axis=1, keepdims=True))
        task, tl = Task(abi.TASK_COM, 3, lam=lam, name="com"), (x, xd, None)
    Ac = rng.normal(size=(B, R, 3))
    Ac /= np.linalg.norm(Ac, axis=2, keepdims=True)
    bc = np.einsum("brk,bk->br", Ac, x) + rng.uniform(0.05, 0.2, size=(B, R))
    e = xd - x
    dist = np.linalg.norm(e, axis=1)
    Ac[:, 0] = e / dist[:, None]
    frac = np.where(np.arange(B) % 2 == 0, 0.3, 20.0)
    bc[:, 0] = np.einsum("bk,bk->b", Ac[:, 0], x) + frac * lam * dist / bound_scaling
    q = bleaf[0][0]
    levels = [[task], [Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural")]]
    tleaf = [[tl], [(q, q + rng.normal(0.0, 0.1, size=(B, n)), None)]]
    rowblocks = [Rows(kind, R, bound_scaling=bound_scaling, name="position_constraint")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    p2 = np.concatenate([Ac.reshape(B, 3 * R), bc], axis=1)
    leaf = {"B": B, "A": [J, None], "task": tleaf, "bound": bleaf, "rows": [(J, tl[0], p2)], "C": [None]}
    return plan, leaf


def make_coman_position_stack(B, seed=None, tree=None, frame="l_wrist", plane=0.1, beyond=0.3, bound_scaling=0.5, eps_factor=1e6):
    """`(l_wrist / postural) << joint_limits << velocity_limits << position_constraint` on the reference's COMAN (35 coordinates) with the
    hand's pose and Jacobian LEFT FOR THE KINEMATICS PRODUCER: the Jacobian goes into A_0, which is also the position block's leaf p0
    (level 0 holds the hand's task alone, so A_0 is the dense [B][6][n] array the block reads), the pose into the task's p0, which is
    also the block's p1.  A frame whose task SHARES its level with other tasks has its Jacobian rows inside a wider A_k (row stride
    ma_k n): the block cannot read those, so such a frame is declared a second time in the model (osot_kin_desc), its second frame_J
    pointing at a dense [B][6][n] leaf buffer of its own.
    One half-space: a plane `plane` metres ahead of the hand, normal to a per-instance horizontal direction; the hand's reference lies
    `beyond` metres past it.  Returns (plan, leaf, model); leaf["state"] = q0, q_ref, normal [B][3].  bind_position() wires the device
    tensors."""
    import os
    from . import kinematics as kin
    here = os.path.dirname(os.path.abspath(__file__))
    model, lo, up = kin.from_json(tree or os.path.join(os.path.dirname(here), "tests", "golden", "coman_tree.json"))
    rng = np.random.default_rng(16000 if seed is None else seed)
    n = model.n
    ix = model.names.index
    q0 = np.zeros((B, n))
    for s_ in "LR":
        q0[:, ix(s_ + "HipSag")] = -0.3; q0[:, ix(s_ + "KneeSag")] = 0.6; q0[:, ix(s_ + "AnkSag")] = -0.3
        q0[:, ix(s_ + "Elbj")] = -0.8; q0[:, ix(s_ + "ShSag")] = 0.2
    q0[:, ix("LShLat")] = 0.3; q0[:, ix("RShLat")] = -0.3
    q0[:, 6:] += rng.normal(0.0, 0.02, (B, n - 6))
    qmin, qmax = np.maximum(lo, -10.0), np.minimum(up, 10.0)
    q0 = np.clip(q0, qmin + 1e-3, qmax - 1e-3)
    q_ref = q0.copy()
    ang = rng.uniform(-0.5, 0.5, size=(B, 1))                     # ahead of the robot, up to half a radian to either side
    normal = np.concatenate([np.cos(ang), np.sin(ang), np.zeros((B, 1))], axis=1)
    z = lambda *sh: np.zeros(sh)
    levels = [[Task(abi.TASK_CARTESIAN, 6, lam=0.1, name=frame)], [Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural")]]
    bounds = [Bound(abi.BOUND_JOINT_LIMITS, scaling=1.0, name="joint_limits"), Bound(abi.BOUND_VELOCITY_LIMITS, dT=0.05, name="velocity_limits")]
    rowblocks = [Rows(abi.ROWS_POSITION_CARTESIAN, 1, bound_scaling=bound_scaling, name="position_constraint")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [z(B, 6, n), None], "task": [[(z(B, 12), z(B, 12), None)], [(q0.copy(), q_ref, None)]],
            "bound": [(q0.copy(), np.tile(qmin, (B, 1)), np.tile(qmax, (B, 1))), (np.full((B, n), 2.0), None, None)],
            "rows": [(z(B, 6, n), z(B, 12), np.concatenate([normal, z(B, 1)], axis=1))], "C": [None],
            "state": {"q0": q0, "q_ref": q_ref, "normal": normal, "frame": frame, "plane": plane, "beyond": beyond}}
    return plan, leaf, model


def bind_position(stack, kin, leaf):
    """wire make_coman_position_stack to the device: one q tensor is the producer's input, the Postural task's and the joint limits' q
    (and what q_integrate advances); the producer writes the hand's pose into the Cartesian task's p0 (= the position block's p1) and its
    Jacobian into stack.A[0] (= the block's p0).  The plane lies leaf["state"]["plane"] metres ahead of the first posture's hand along
    the instance's normal, the hand's reference "beyond" metres past it, with the first posture's orientation.
    -> (dev_leaf, kin_batch, q)"""
    import torch
    B, s = leaf["B"], leaf["state"]
    dev = stack.load_leaf(leaf)
    f64 = dict(dtype=torch.float64, device=stack.device)
    q = torch.as_tensor(s["q0"], **f64).contiguous()
    f = kin.model.frame_index(s["frame"])
    pose = torch.zeros((B, 12), **f64)
    kw = dict(frame_pose={f: pose}, frame_J={f: (stack.A[0], 0)})
    kin.forward(q, **kw)
    nrm = torch.as_tensor(s["normal"], **f64)
    ref = pose.clone()
    ref[:, 9:] += (s["plane"] + s["beyond"]) * nrm
    p2 = torch.cat([nrm, (nrm * pose[:, 9:]).sum(dim=1, keepdim=True) + s["plane"]], dim=1).contiguous()
    dev["task"][0][0] = (pose, ref, None)
    dev["task"][1][0] = (q, dev["task"][1][0][1], None)
    dev["bound"][0] = (q,) + tuple(dev["bound"][0][1:])
    dev["rows"][0] = (stack.A[0], pose, p2)
    return dev, kin.batch_args(q, **kw), q


def cartesian_velocity_rows(task_kind, v_lim, dT, name="cartesian_velocity"):
    """constraints::velocity::CartesianVelocity (src/constraints/velocity/CartesianVelocity.cpp:77-96; `comVelocity` of the reference's
    DefaultHumanoidStack): -v_lim dT <= J dq <= v_lim dT on the linear velocity of the CoM or of a link.  It needs no kind of its own: it
    is the task used as a constraint (constraints::TaskToConstraint) with lambda = 0 -- so b = 0 whatever the pose error -- and the
    error band +-v_lim dT.  task_kind: ROWS_TASK_COM (3 rows; v_lim a scalar or 3 values) or ROWS_TASK_CARTESIAN (6 rows; v_lim a
    scalar or 6 values: the reference bounds the three linear rows only, so pass a large value for the angular ones).  The leaf is the
    task's own (actual and desired pose / CoM; the desired one is not felt at lambda = 0, p2 = NULL); the producer writes J into C."""
    assert task_kind in (abi.ROWS_TASK_COM, abi.ROWS_TASK_CARTESIAN)
    rows = 3 if task_kind == abi.ROWS_TASK_COM else 6
    band = np.broadcast_to(np.asarray(v_lim, dtype=float), (rows,)) * float(dT)
    assert (band >= 0.0).all()
    return Rows(task_kind, rows, lam=0.0, orientation_gain=1.0, err_lb=(-band).tolist(), err_ub=band.tolist(), name=name)


# ---- velocity::MinimumEffort and velocity::Manipulability: the b comes from the posture-gradient producer ---------------------------
def _coman_bent(rng, B, tree=None):
    """the reference's COMAN from the tree fixture in a standing posture, knees and elbows bent: (model, q0 [B][n], q_min, q_max)"""
    import os
    from . import kinematics as kin
    here = os.path.dirname(os.path.abspath(__file__))
    model, lo, up = kin.from_json(tree or os.path.join(os.path.dirname(here), "tests", "golden", "coman_tree.json"))
    n, ix = model.n, model.names.index
    q0 = np.zeros((B, n))
    for s_ in "LR":
        q0[:, ix(s_ + "HipSag")] = -0.3; q0[:, ix(s_ + "KneeSag")] = 0.6; q0[:, ix(s_ + "AnkSag")] = -0.3
        q0[:, ix(s_ + "Elbj")] = -0.8; q0[:, ix(s_ + "ShSag")] = 0.2
    q0[:, ix("LShLat")] = 0.3; q0[:, ix("RShLat")] = -0.3
    q0[:, 6:] += rng.normal(0.0, 0.02, (B, n - 6))
    qmin, qmax = np.maximum(lo, -10.0), np.minimum(up, 10.0)
    return model, np.clip(q0, qmin + 1e-3, qmax - 1e-3), qmin, qmax


def make_min_effort_stack(B, seed=None, tree=None, w_scale=1e-5, lam=1.0, step=1e-3, eps_factor=1e6):
    """tasks::velocity::MinimumEffort alone in a stack, as tests/tasks/velocity/TestMinimumEffort.cpp:80-104 builds it on COMAN: one level,
    A = I, W = I, b = -lambda grad(tau_g' W_effort tau_g) with W_effort = w_scale I (the test sets 1e-5 I).  The task is an implicit
    OSOT_TASK_POSTURAL block whose actual and reference posture are the SAME array (lambda (q - q) = 0) and whose feed-forward leaf p2
    is the producer's output.  Returns (plan, leaf, model, terms): terms is the list for gradient.PostureGradient;
    bind_posture_gradient() wires the device tensors."""
    from .gradient import posture_term
    rng = np.random.default_rng(17000 if seed is None else seed)
    model, q0, _, _ = _coman_bent(rng, B, tree)
    n = model.n
    plan = StackPlan(n=n, levels=[[Task(abi.TASK_POSTURAL, n, lam=1.0, name="min_effort")]], eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [None], "task": [[(q0.copy(), q0.copy(), np.zeros((B, n)))]], "bound": [], "rows": [], "C": [],
            "state": {"q0": q0, "gradient": [(0, 0, 0)]}}
    terms = [posture_term(abi.GRAD_MIN_EFFORT, step=step, lam=lam, W=np.full(n, w_scale))]
    return plan, leaf, model, terms


def make_coman_manipulability_stack(B, seed=None, tree=None, lam=1.0, step=1e-3, postural_lam=0.1, dT=0.01, eps_factor=1e6):
    """`((l_wrist + r_wrist) / (manipulability_l + manipulability_r + postural)) << joint_limits << velocity_limits` on the reference's
    COMAN, after tests/tasks/velocity/TestManipulability.cpp:55-100: the two wrists are Cartesian tasks RELATIVE to the waist (a frame
    "Waist" on the pelvis link is added to the model), the bottom level aggregates the two velocity::Manipulability tasks of those
    Cartesian tasks with velocity::Postural.  The manipulability tasks (A = I) are OSOT_TASK_GENERIC blocks with stored unit rows --
    the level also holds the implicit Postural block, which must be its last one -- and their b is the producer's output, written
    straight into the blocks' leaf p0.  Poses and Jacobians of the wrists are left for the kinematics producer.
    Returns (plan, leaf, model, terms); leaf["state"] = q0, q_ref; bind_posture_gradient() wires the device tensors."""
    from .gradient import posture_term
    rng = np.random.default_rng(18000 if seed is None else seed)
    model, q0, qmin, qmax = _coman_bent(rng, B, tree)
    n = model.n
    model.frames = list(model.frames) + [("Waist", model.names.index("VIRTUALJOINT_6"), np.eye(3), (0.0, 0.0, 0.0))]
    fl, fr, fw = model.frame_index("l_wrist"), model.frame_index("r_wrist"), model.frame_index("Waist")
    model.frame_base = {fl: fw, fr: fw}
    z = lambda *sh: np.zeros(sh)
    levels = [[Task(abi.TASK_CARTESIAN, 6, lam=1.0, name="l_wrist"), Task(abi.TASK_CARTESIAN, 6, lam=1.0, name="r_wrist")],
              [Task(abi.TASK_GENERIC, n, name="manipulability::l_wrist"), Task(abi.TASK_GENERIC, n, name="manipulability::r_wrist"),
               Task(abi.TASK_POSTURAL, n, lam=postural_lam, name="postural")]]
    bounds = [Bound(abi.BOUND_JOINT_LIMITS, scaling=0.2, name="joint_limits"), Bound(abi.BOUND_VELOCITY_LIMITS, dT=dT, name="velocity_limits")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, eps_abs=eps_abs_from_factor(eps_factor))
    unit = np.tile(np.concatenate([np.eye(n), np.eye(n)], axis=0), (B, 1, 1))
    leaf = {"B": B, "A": [z(B, 12, n), unit],
            "task": [[(z(B, 12), z(B, 12), None), (z(B, 12), z(B, 12), None)], [(z(B, n), None, None), (z(B, n), None, None), (q0.copy(), q0.copy(), None)]],
            "bound": [(q0.copy(), np.tile(qmin, (B, 1)), np.tile(qmax, (B, 1))), (np.full((B, n), np.pi / 2.0), None, None)],
            "rows": [], "C": [],
            "state": {"q0": q0, "q_ref": q0.copy(), "frames": (fl, fr), "gradient": [(1, 0, 0), (1, 1, 1)]}}
    terms = [posture_term(abi.GRAD_MANIPULABILITY_FRAME, frame=fl, step=step, lam=lam),
             posture_term(abi.GRAD_MANIPULABILITY_FRAME, frame=fr, step=step, lam=lam)]
    return plan, leaf, model, terms


def bind_posture_gradient(stack, grad, leaf, kin=None):
    """wire make_min_effort_stack / make_coman_manipulability_stack to the device: ONE q tensor is the gradient producer's input, the
    Postural block's actual posture, the joint limits' q and (with `kin`, a kinematics.Kinematics of the same model) the kinematics
    producer's input; leaf["state"]["gradient"] lists (level, block, term): the producer writes term's b into that block's leaf --
    p2, the feed-forward, of an implicit Postural block whose reference is then q itself, p0 of a Generic block.  With `kin` the wrists'
    relative poses go into the Cartesian tasks' p0 and their Jacobians into stack.A[0]; the Cartesian references are the first
    posture's poses.  -> (dev_leaf, grad_batch, kin_batch or None, q)"""
    import torch
    B, s = leaf["B"], leaf["state"]
    dev = stack.load_leaf(leaf)
    f64 = dict(dtype=torch.float64, device=stack.device)
    q = torch.as_tensor(s["q0"], **f64).contiguous()
    out = {}
    for (k, j, term) in s["gradient"]:
        p0, p1, p2 = dev["task"][k][j]
        if stack.plan.levels[k][j].kind == abi.TASK_POSTURAL:
            dev["task"][k][j] = (q, q, p2)
            out[term] = p2
        else:
            out[term] = p0
    kb = None
    if kin is not None:
        frames = s["frames"]
        poses = [dev["task"][0][i][0] for i in range(len(frames))]
        kw = dict(frame_pose={f: poses[i] for i, f in enumerate(frames)}, frame_J={f: (stack.A[0], 6 * i) for i, f in enumerate(frames)})
        kin.forward(q, **kw)
        for i in range(len(frames)):
            dev["task"][0][i] = (poses[i], poses[i].clone(), None)
        last = len(dev["task"][1]) - 1
        dev["task"][1][last] = (q, torch.as_tensor(s["q_ref"], **f64).contiguous(), None)
        dev["bound"][0] = (q,) + tuple(dev["bound"][0][1:])
        kb = kin.batch_args(q, **kw)
    return dev, grad.batch_args(q, b=out), kb, q


# ---- the momentum tasks: their rows come from the dynamics producer's centroidal momentum matrix ----------------------------------------
def make_coman_momentum_stack(B, seed=None, tree=None, inertia=None, momentum=True, linear_momentum=False, swing=0.3, postural_lam=0.1,
                              dT=0.01, eps_factor=1e6):
    """`((l_sole + r_sole + com) / angular_momentum / postural) << joint_limits << velocity_limits` on the reference's COMAN with its
    inertia fixture: the soles and the CoM hold their first poses, tasks::velocity::AngularMomentum (AngularMomentum.cpp:44-51: A = the
    angular rows of the centroidal momentum matrix, b = the desired momentum, here zero) sits above a Postural task whose reference
    swings the arms and the waist by up to `swing` radians -- so the bottom level asks for angular momentum and the level above it
    refuses.  The momentum task is an OSOT_TASK_GENERIC block of 3 stored rows that the DYNAMICS producer writes (osot_dyn_batch.cmm_ang)
    and whose b is the leaf p0; poses, Jacobians and the CoM are left for the kinematics producer.
    momentum=False drops that level and changes nothing else.  linear_momentum=True replaces the CoM task by the 3-row
    tasks::velocity::LinearMomentum block (LinearMomentum.cpp:43-48: A = the linear rows, b = 0) in the same rows of A_0.
    Returns (plan, leaf, model); leaf["state"] = q0, q_ref, momentum = (level, first row) or None, linear_momentum = (0, 12) or None.
    bind_momentum() wires the device tensors."""
    import json
    import os
    rng = np.random.default_rng(19000 if seed is None else seed)
    here = os.path.dirname(os.path.abspath(__file__))
    model, q0, qmin, qmax = _coman_bent(rng, B, tree)
    model.inertia = np.array(json.load(open(inertia or os.path.join(os.path.dirname(here), "tests", "golden", "coman_inertia.json")))["inertia"],
                             dtype=float).reshape(model.n, 6)
    n, ix = model.n, model.names.index
    upper = list(range(ix("WaistLat"), ix("RHipSag")))          # waist and arms
    q_ref = q0.copy()
    q_ref[:, upper] += rng.uniform(-swing, swing, (B, len(upper)))
    q_ref = np.clip(q_ref, qmin + 1e-3, qmax - 1e-3)
    z = lambda *sh: np.zeros(sh)
    third = Task(abi.TASK_GENERIC, 3, name="linear_momentum") if linear_momentum else Task(abi.TASK_COM, 3, lam=1.0, name="com")
    levels = [[Task(abi.TASK_CARTESIAN, 6, lam=1.0, name="l_sole"), Task(abi.TASK_CARTESIAN, 6, lam=1.0, name="r_sole"), third]]
    A = [z(B, 15, n)]
    tleaf = [[(z(B, 12), z(B, 12), None), (z(B, 12), z(B, 12), None), (z(B, 3), None, None) if linear_momentum else (z(B, 3), z(B, 3), None)]]
    if momentum:
        levels.append([Task(abi.TASK_GENERIC, 3, name="angular_momentum")])
        A.append(z(B, 3, n))
        tleaf.append([(z(B, 3), None, None)])
    levels.append([Task(abi.TASK_POSTURAL, n, lam=postural_lam, name="postural")])
    A.append(None)
    tleaf.append([(q0.copy(), q_ref, None)])
    bounds = [Bound(abi.BOUND_JOINT_LIMITS, scaling=0.2, name="joint_limits"), Bound(abi.BOUND_VELOCITY_LIMITS, dT=dT, name="velocity_limits")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": A, "task": tleaf,
            "bound": [(q0.copy(), np.tile(qmin, (B, 1)), np.tile(qmax, (B, 1))), (np.full((B, n), np.pi / 2.0), None, None)],
            "rows": [], "C": [],
            "state": {"q0": q0, "q_ref": q_ref, "frames": (model.frame_index("l_sole"), model.frame_index("r_sole")),
                      "momentum": (1, 0) if momentum else None, "linear_momentum": (0, 12) if linear_momentum else None}}
    return plan, leaf, model


def bind_momentum(stack, kin, dyn, leaf):
    """wire make_coman_momentum_stack to the device: ONE q tensor is the input of both producers, the Postural block's actual posture and
    the joint limits' q.  The kinematics producer writes the soles' poses into the Cartesian tasks' p0, their Jacobians and the CoM's
    into stack.A[0]; the dynamics producer writes the angular rows of the momentum matrix into stack.A[level] at the momentum block's
    rows (and the linear rows into stack.A[0] where the stack has the LinearMomentum block).  The references of the soles and of the CoM
    are the first posture's; the b of the momentum blocks are their leaf p0 (zero; the caller owns them).
    -> (dev_leaf, kin_batch, dyn_batch or None, q)"""
    import torch
    B, s = leaf["B"], leaf["state"]
    dev = stack.load_leaf(leaf)
    f64 = dict(dtype=torch.float64, device=stack.device)
    q = torch.as_tensor(s["q0"], **f64).contiguous()
    frames = s["frames"]
    poses = [dev["task"][0][i][0] for i in range(2)]
    kw = dict(frame_pose={f: poses[i] for i, f in enumerate(frames)}, frame_J={f: (stack.A[0], 6 * i) for i, f in enumerate(frames)})
    if s["linear_momentum"] is None:
        kw.update(com=dev["task"][0][2][0], com_J=(stack.A[0], 12))
    kin.forward(q, **kw)
    for i in range(2):
        dev["task"][0][i] = (poses[i], poses[i].clone(), None)
    if s["linear_momentum"] is None:
        dev["task"][0][2] = (kw["com"], kw["com"].clone(), None)
    last = len(dev["task"]) - 1
    dev["task"][last][0] = (q, dev["task"][last][0][1], None)
    dev["bound"][0] = (q,) + tuple(dev["bound"][0][1:])
    dk = {}
    if s["momentum"] is not None:
        dk["cmm_ang"] = (stack.A[s["momentum"][0]], s["momentum"][1])
    if s["linear_momentum"] is not None:
        dk["cmm_lin"] = (stack.A[s["linear_momentum"][0]], s["linear_momentum"][1])
    db = None
    if dk:
        dyn.forward(q, **dk)
        db = dyn.batch_args(q, **dk)
    return dev, kin.batch_args(q, **kw), db, q


def make_coman_id_momentum_stack(B, seed=None, tree=None, inertia=None, eps_factor=1e6):
    """make_coman_id_stack with tasks::acceleration::AngularMomentum (AngularMomentum.cpp:31-60) between the contact / CoM level and the
    Postural one: an OSOT_TASK_GENERIC block of 3 rows [A_ang 0] of row length n = 47 that the dynamics producer writes into the
    zero-initialised A_1 (osot_dyn_batch.cmm_ang with ld = n), its b = Ldot_d + lambda K (L_d - L) formed by the same launch into the
    block's leaf p0 (osot_dyn_batch.ang_mom_b) with lambda = 1, K = I, L_d = 0, Ldot_d = 0.
    Returns (plan, leaf, model) for dynamics.IdMomentumStep; leaf["state"]["momentum"] = dict(level, row, lam, K)."""
    plan0, leaf, model = make_coman_id_stack(B, seed=seed, tree=tree, inertia=inertia, eps_factor=eps_factor)
    n = plan0.n
    levels = [plan0.levels[0], [Task(abi.TASK_GENERIC, 3, name="angular_momentum")], plan0.levels[1]]
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=plan0.rowblocks, eps_abs=plan0.eps_abs)
    leaf["A"] = [leaf["A"][0], np.zeros((B, 3, n)), None]
    leaf["task"] = [leaf["task"][0], [(np.zeros((B, 3)), None, None)], leaf["task"][1]]
    leaf["state"]["momentum"] = dict(level=1, row=0, lam=1.0, K=np.eye(3))
    return plan, leaf, model


# ---- wheeled-legged robots: PureRolling / Contact / OmniWheels4X rows from the kinematics producer --------------------------------
WHEEL_RADIUS = 0.08


def make_wheeled_tree(legs=4, leg_joints=2):
    """A wheeled-legged tree: a floating base of 3 prismatic + 3 revolute coordinates (x, y, z, roll, pitch, yaw), then per leg
    `leg_joints` revolute joints (a hip yaw about z, pitch joints about y) and a wheel joint spinning about its LOCAL z, which lies
    along the base's y at q = 0 (the convention of PureRolling: _wheel_axis = (0, 0, 1), PureRolling.cpp:10).  Legs in the order
    front-left, front-right, hind-left, hind-right (OmniWheels4X's order).  Frames: "base" on the last base joint, "wheel_<i>" at the
    centre of wheel i.  n = 6 + legs * (leg_joints + 1) <= 64."""
    from . import kinematics as kin
    P, R = abi.JOINT_PRISMATIC, abi.JOINT_REVOLUTE
    X, Y, Z = [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]
    I = np.eye(3)
    Rw = np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])        # the wheel joint's frame: its z is the parent's y
    rows = [("base_x", -1, P, X, (0, 0, 0), I, 0.0), ("base_y", 0, P, Y, (0, 0, 0), I, 0.0), ("base_z", 1, P, Z, (0, 0, 0), I, 0.0),
            ("base_roll", 2, R, X, (0, 0, 0), I, 0.0), ("base_pitch", 3, R, Y, (0, 0, 0), I, 0.0), ("base_yaw", 4, R, Z, (0, 0, 0), I, 20.0)]
    assert legs >= 1 and leg_joints >= 1 and 6 + legs * (leg_joints + 1) <= abi.KIN_MAX_JOINTS
    wheels = []
    for leg in range(legs):
        sx, sy = (1.0 if (leg // 2) % 2 == 0 else -1.0), (1.0 if leg % 2 == 0 else -1.0)
        parent = 5
        for k in range(leg_joints):
            xyz = (sx * 0.3, sy * 0.2, -0.05) if k == 0 else (0.05 * sx if k == 1 else 0.0, 0.0, -0.25)
            rows.append((f"leg{leg}_j{k}", parent, R, Z if k == 0 else Y, xyz, I, 1.5))
            parent = len(rows) - 1
        rows.append((f"wheel_{leg}_joint", parent, R, Z, (0.0, sy * 0.05, -0.25), Rw, 1.0))
        wheels.append(len(rows) - 1)
    n = len(rows)
    m = kin.KinModel(parent=[r[1] for r in rows], jtype=[r[2] for r in rows], axis=np.array([r[3] for r in rows], dtype=float),
                     R0=np.array([r[5] for r in rows], dtype=float), p0=np.array([r[4] for r in rows], dtype=float),
                     mass=np.array([r[6] for r in rows], dtype=float), com=np.zeros((n, 3)), names=[r[0] for r in rows])
    m.frames = [("base", 5, I, (0.0, 0.0, 0.0))] + [(f"wheel_{i}", w, I, (0.0, 0.0, 0.0)) for i, w in enumerate(wheels)]
    m.wheel_joints = wheels
    return m


def wheeled_posture(model, B, seed=0):
    """B standing postures of make_wheeled_tree: the base within 0.2 m / 0.15 rad of the origin, legs bent by 0.2 .. 0.6 rad, wheels
    anywhere; the wheel axes stay well away from the vertical"""
    rng = np.random.default_rng(31000 + seed)
    n = model.n
    q = np.zeros((B, n))
    q[:, :3] = rng.uniform(-0.2, 0.2, (B, 3)); q[:, 2] += 0.2 * ((n - 6) // len(model.wheel_joints))
    q[:, 3:6] = rng.uniform(-0.15, 0.15, (B, 3))
    for j in range(6, n):
        if j in model.wheel_joints:
            q[:, j] = rng.uniform(-3.0, 3.0, B)
        elif model.axis[j][2] == 1.0:
            q[:, j] = rng.uniform(-0.3, 0.3, B)
        else:
            q[:, j] = rng.uniform(0.2, 0.6, B) * (1.0 if (j % 2) else -1.0)
    return q


def make_wheeled_stack(B, seed=None, legs=4, leg_joints=4, omni=False, eps_factor=1e6):
    """The velocity stack of a wheeled-legged robot with every model quantity LEFT FOR THE KINEMATICS PRODUCER:

    levels : 0 = one tasks::velocity::PureRolling per wheel (4 rows each, b = 0: OSOT_TASK_GENERIC blocks whose rows the producer writes
             into A_0), 1 = velocity::Cartesian on the base (the producer writes its Jacobian into A_1 and its pose into the leaf),
             2 = velocity::Postural
    box    : joint limits, velocity limits
    rows   : omni=True: constraints::velocity::OmniWheels4X as a global equality block (OSOT_ROWS_GENERIC, lo = up = 0, rows written
             into C by the producer)

    leg_joints = 4 (26 coordinates): the 16 rolling rows and the base's 6 leave the posture 4 directions; with fewer joints the last
    level's equalities outnumber the variables.
    Returns (plan, leaf, model); leaf["state"] = q0, q_ref, base_step.  bind_wheeled() wires the device tensors."""
    rng = np.random.default_rng(32000 if seed is None else seed)
    model = make_wheeled_tree(legs, leg_joints)
    n = model.n
    for i in range(legs):
        model.add_pure_rolling(f"wheel_{i}", WHEEL_RADIUS)
    if omni:
        assert legs == 4
        model.add_omni_wheels_4x("base", 0.3, 0.2, WHEEL_RADIUS, model.wheel_joints)
    q0 = wheeled_posture(model, B, seed=0 if seed is None else seed)
    q_ref = q0 + rng.uniform(-0.05, 0.05, (B, n))
    # the base's reference pose: a small step ahead of where it stands (filled in from the producer's pose by the binder)
    base_step = np.concatenate([rng.uniform(-0.01, 0.01, (B, 2)), rng.uniform(-0.003, 0.003, (B, 1))], axis=1)
    z = lambda *sh: np.zeros(sh)
    levels = [[Task(abi.TASK_GENERIC, 4, name=f"pure_rolling_{i}") for i in range(legs)],
              [Task(abi.TASK_CARTESIAN, 6, lam=0.5, name="base")], [Task(abi.TASK_POSTURAL, n, lam=0.1, name="postural")]]
    bounds = [Bound(abi.BOUND_JOINT_LIMITS, scaling=1.0, name="joint_limits"), Bound(abi.BOUND_VELOCITY_LIMITS, dT=0.05, name="velocity_limits")]
    rowblocks = [Rows(abi.ROWS_GENERIC, 3, name="omni_wheels_4x")] if omni else []
    plan = StackPlan(n=n, levels=levels, bounds=bounds, rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    qmin, qmax = np.full(n, -10.0), np.full(n, 10.0)
    ident = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (B, 1))
    leaf = {"B": B, "A": [z(B, 4 * legs, n), z(B, 6, n), None],
            "task": [[(z(B, 4), None, None) for _ in range(legs)], [(ident.copy(), ident.copy(), None)], [(q0.copy(), q_ref, None)]],
            "bound": [(q0.copy(), np.tile(qmin, (B, 1)), np.tile(qmax, (B, 1))), (np.full((B, n), 2.0), None, None)],
            "rows": [(z(B, 3, n), z(B, 3), z(B, 3))] if omni else [], "C": [None] if omni else [],
            "state": {"q0": q0, "q_ref": q_ref, "base_step": base_step}}
    return plan, leaf, model


def wheeled_outputs(model, omni):
    """where the producer writes for make_wheeled_stack: (frame_pose, frame_J, rowset_A) as {index: ("A", level, first row) /
    ("task", level, task) / ("C", block, first row)}"""
    legs = len(model.wheel_joints)
    rs = {i: ("A", 0, 4 * i) for i in range(legs)}
    if omni:
        rs[legs] = ("C", 0, 0)
    return {0: ("task", 1, 0)}, {0: ("A", 1, 0)}, rs


def bind_wheeled(stack, kin, leaf):
    """wire make_wheeled_stack to the device: one q tensor is the producer's input, the Postural task's and the joint limits' q; the
    producer writes the PureRolling rows into stack.A[0], the base's Jacobian into stack.A[1], its pose into the Cartesian task's leaf
    and, for the omni variant, the OmniWheels4X rows into the row block's p0.  The base's reference is the first posture's pose moved
    by leaf["state"]["base_step"].  -> (dev_leaf, kin_batch, q)"""
    import torch
    B = leaf["B"]
    dev = stack.load_leaf(leaf)
    f64 = dict(dtype=torch.float64, device=stack.device)
    q = torch.as_tensor(leaf["state"]["q0"], **f64).contiguous()
    pose = torch.zeros((B, 12), **f64)
    legs = len(kin.model.wheel_joints)
    rs = {i: (stack.A[0], 4 * i) for i in range(legs)}
    omni = len(kin.model.rowsets) > legs
    if omni:
        Crows = dev["rows"][0][0]
        rs[legs] = (Crows, 0)
    kw = dict(frame_pose={0: pose}, frame_J={0: (stack.A[1], 0)}, rowset_A=rs)
    kin.forward(q, **kw)
    ref = pose.clone()
    ref[:, 9:] += torch.as_tensor(leaf["state"]["base_step"], **f64)
    dev["task"][1][0] = (pose, ref, None)
    dev["task"][2][0] = (q, dev["task"][2][0][1], None)
    dev["bound"][0] = (q,) + tuple(dev["bound"][0][1:])
    return dev, kin.batch_args(q, **kw), q


def _frame_lin_jacobian(model, q, f):
    """numpy: world position p and linear Jacobian [3][n] of frame f's origin at q[n] (the recurrence of KinModel.points_world)"""
    n = model.n
    Rw, pw = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for j in range(n):
        if model.jtype[j] == abi.JOINT_REVOLUTE:
            x, y, z = model.axis[j]
            c, s = np.cos(q[j]), np.sin(q[j])
            K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
            Rl, pl = model.R0[j] @ (np.eye(3) + s * K + (1.0 - c) * (K @ K)), model.p0[j]
        else:
            Rl, pl = model.R0[j], model.p0[j] + model.R0[j] @ model.axis[j] * q[j]
        a = model.parent[j]
        Rw[j], pw[j] = (Rl, pl) if a < 0 else (Rw[a] @ Rl, Rw[a] @ pl + pw[a])
    _, jf, _, pf = model.frames[f]
    p = pw[jf] + Rw[jf] @ np.asarray(pf, dtype=float)
    J = np.zeros((3, n))
    j = jf
    while j >= 0:
        zj = Rw[j] @ model.axis[j]
        J[:, j] = np.cross(zj, p - pw[j]) if model.jtype[j] == abi.JOINT_REVOLUTE else zj
        j = model.parent[j]
    return p, J


def _frame_ang_jacobian(model, q, f):
    """numpy: world rotation R and angular Jacobian [3][n] of frame f at q[n] (the recurrence of _frame_lin_jacobian)"""
    n = model.n
    Rw = np.zeros((n, 3, 3))
    for j in range(n):
        Rl = model.R0[j]
        if model.jtype[j] == abi.JOINT_REVOLUTE:
            x, y, z = model.axis[j]
            c, s = np.cos(q[j]), np.sin(q[j])
            K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
            Rl = model.R0[j] @ (np.eye(3) + s * K + (1.0 - c) * (K @ K))
        a = model.parent[j]
        Rw[j] = Rl if a < 0 else Rw[a] @ Rl
    _, jf, Rf, _ = model.frames[f]
    J = np.zeros((3, n))
    j = jf
    while j >= 0:
        if model.jtype[j] == abi.JOINT_REVOLUTE:
            J[:, j] = Rw[j] @ model.axis[j]
        j = model.parent[j]
    return Rw[jf] @ np.asarray(Rf, dtype=float), J


def make_base_estimation_stack(B, seed=None, legs=4, leg_joints=2, eps_factor=2e2, imu=False, contact_lambda=0.0):
    """Floating-base estimation after examples/cpp/qp_estimation.cpp: a 6-variable plan whose one level holds a
    tasks::floating_base::Contact per wheel, here a point contact (K = [I 0]: the 3 linear rows) on a frame "contact_<i>" fixed on
    the rim of wheel i; A = (K Ad(R_f') J_f)[:, 0:6] and b = -(K Ad(R_f') J_f)[:, 6:] qdot[6:] are both written by the producer
    (split contact row sets: A into A_0, b into the OSOT_TASK_GENERIC leaves).  The joint velocities qdot[6:] are made consistent with
    a base twist planted in qdot[0:6] -- each leg's three joints carry its contact frame's velocity to zero -- so the least-squares
    residual is zero and the solution is the planted twist.  eps_factor: iHQP's default regularisation (the answer is asked to 1e-9).
    imu=True: a tasks::floating_base::IMU block (6 rows over the six variables: zeros, then the angular rows of the base link's Jacobian;
    b = [0; R_imu omega], IMU.cpp:33-42) joins the level behind the contacts, as in the example; its rows and b are osot_feedback's.
    The IMU sits on the base link (frame "base"); the gyroscope reading leaf["state"]["imu_omega"] is the planted twist's angular
    velocity in the IMU's frame, so the solution stays the planted twist.
    contact_lambda != 0: the lambda * err term of floating_base::Contact (Contact.cpp:55-66).  err has six entries, so the contacts
    become full ones (K = I: 6 rows each, as the reference's constructor needs for that term); the producer's b goes to a buffer
    and osot_feedback adds lambda [p_d - p; -e_o] against leaf["state"]["contact_pose_ref"] [B][legs][12] (all zero: the first
    posture's poses).  The angular rows are not consistent with the planted twist (the wheels spin): the answer is a least-squares one.
    Returns (plan, leaf, model); leaf["state"] = q0, qdot (+ contact_rows, imu, imu_omega, contact_lambda, contact_pose_ref, feedback:
    the feedback.FeedbackModel, where either option is on); bind_base_estimation() wires the device tensors."""
    rng = np.random.default_rng(33000 if seed is None else seed)
    model = make_wheeled_tree(legs, leg_joints)
    n = model.n
    K = np.eye(6) if contact_lambda != 0.0 else np.eye(6)[:3]
    rows = K.shape[0]
    model.frames = model.frames[:1]                       # the base; the wheel centres make room for the contact frames
    for i, w in enumerate(model.wheel_joints):
        model.frames.append((f"contact_{i}", w, np.eye(3), (WHEEL_RADIUS, 0.0, 0.0)))
        model.add_contact_rows(f"contact_{i}", K, split=True)
    q0 = wheeled_posture(model, B, seed=0 if seed is None else seed)
    qdot = np.zeros((B, n))
    qdot[:, :6] = rng.uniform(-0.5, 0.5, (B, 6))
    per = leg_joints + 1
    for i in range(B):
        for k in range(legs):
            _, J = _frame_lin_jacobian(model, q0[i], model.frame_index(f"contact_{k}"))
            cols = list(range(6 + k * per, 6 + (k + 1) * per))
            sol, *_ = np.linalg.lstsq(J[:, cols], -J[:, :6] @ qdot[i, :6], rcond=None)
            qdot[i, cols] = sol
            assert np.abs(J @ qdot[i]).max() < 1e-12, "a leg cannot hold its contact still: pick another posture"
    z = lambda *sh: np.zeros(sh)
    tasks = [Task(abi.TASK_GENERIC, rows, name=f"contact_{i}") for i in range(legs)] + ([Task(abi.TASK_GENERIC, 6, name="imu")] if imu else [])
    plan = StackPlan(n=6, levels=[tasks], eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [z(B, rows * legs + (6 if imu else 0), 6)],
            "task": [[(z(B, rows), None, None) for _ in range(legs)] + ([(z(B, 6), None, None)] if imu else [])],
            "bound": [], "rows": [], "C": [], "state": {"q0": q0, "qdot": qdot}}
    if imu or contact_lambda != 0.0:
        from .feedback import FeedbackModel
        omega = np.zeros((B, 3))
        for i in range(B):
            R, Jw = _frame_ang_jacobian(model, q0[i], 0)
            omega[i] = R.T @ (Jw @ qdot[i])
        leaf["state"].update(contact_rows=rows, imu=bool(imu), imu_omega=omega, contact_lambda=float(contact_lambda),
                             contact_pose_ref=z(B, legs, 12), feedback=FeedbackModel(n, floating_base=True, imu=imu, contact_lambda=contact_lambda))
    return plan, leaf, model


# ---- the force-space tasks: wrench distribution over surface contacts (rows from osot_force_rows) --------------------------------------
def _force_rowblocks(B, C_, mu, R9, lims, wrench_max=(1.0e3, 1.0e3, 1.0e3, 200.0, 200.0, 200.0)):
    """force::FrictionCone, force::CoP on the C wrenches at columns 0 .. 6 C - 1 and force::WrenchLimits as unit rows"""
    wl = np.tile(np.asarray(wrench_max, dtype=float), (B, C_))
    blocks = [Rows(abi.ROWS_WRENCH_FRICTION_CONE, 5 * C_, first_col=0, mu=mu, name="friction_cones"),
              Rows(abi.ROWS_COP, 4 * C_, first_col=0, name="cop"),
              Rows(abi.ROWS_UNIT_GENERIC, 6 * C_, first_col=0, name="wrench_limits")]
    return blocks, [(R9, None, None), (R9, lims, None), (-wl, wl, None)]


def make_coman_force_stack(B, form="com", seed=None, tree=None, inertia=None, com_acc=0.2, eps_factor=1e6):
    """The reference's wrench-distribution stack on its COMAN standing on both soles (surface contacts l_sole, r_sole; the posture of
    make_coman_id_stack, at rest), x = [w_l_sole (6); w_r_sole (6) | tau (29)]:

      form "com"    (n = 12): level 0 = force::CoM (6 rows [I 0; P_c I] per contact, b from the CoM references), level 1 = force::Wrenches
                    (the selection I_12, b = the reference wrenches: half the weight on each sole); global rows: force::FrictionCone,
                    force::CoP, force::WrenchLimits
      form "static" (n = 41): the torques join x; level 0 = force::FloatingBase ((Jc_c[:, 0:6])' per contact, b = the floating-base
                    part of the gravity term) in place of force::CoM, level 1 as above; the StaticConstraint's 29 equality rows
                    [(Jc_c[:, 6:35])' I] x = g[6:35] come first among the global rows
    Every force block is OSOT_TASK_GENERIC / OSOT_ROWS_GENERIC and arrives zeroed: opensot_amd.dynamics.ForceStep has osot_kinematics,
    osot_dynamics and osot_force_rows write them every cycle.  The CoM reference asks for up to com_acc m/s^2 of acceleration from
    the first CoM.  Returns (plan, leaf, model); leaf["force"] names the blocks for ForceStep, leaf["state"] = q0, qdot0."""
    assert form in ("com", "static")
    _, idleaf, model = make_coman_id_stack(B, seed=seed, tree=tree, inertia=inertia)
    rng = np.random.default_rng(41000 if seed is None else seed)
    nv, C_ = model.n, 2
    na = nv - 6
    n = 12 + (na if form == "static" else 0)
    mass = float(np.sum(model.mass))
    z = lambda *sh: np.zeros(sh)
    w_ref = np.tile(np.array([0.0, 0.0, 0.5 * mass * 9.81, 0.0, 0.0, 0.0]), (B, C_))
    levels = [[Task(abi.TASK_GENERIC, 6, name="force_com" if form == "com" else "floating_base")],
              [Task(abi.TASK_GENERIC, 12, name="wrenches")]]
    Asel = np.zeros((12, n)); Asel[:, :12] = np.eye(12)
    R9 = np.tile(np.eye(3).reshape(9), (B, C_, 1))
    lims = np.tile(np.array(SOLE_RECTANGLE), (B, C_, 1))
    rowblocks, rleaf = _force_rowblocks(B, C_, 0.8, R9, lims)
    Cl = [None] * 3
    static_block = None
    if form == "static":
        rowblocks.insert(0, Rows(abi.ROWS_GENERIC, na, name="static_constraint"))
        rleaf.insert(0, (z(B, na, n), z(B, na), z(B, na)))
        Cl.insert(0, None)
        static_block = 0
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [z(B, 6, n), np.tile(Asel, (B, 1, 1))], "task": [[(z(B, 6), None, None)], [(w_ref, None, None)]],
            "bound": [], "rows": rleaf, "C": Cl,
            "state": {"q0": idleaf["state"]["q0"], "qdot0": z(B, nv)},
            "force": {"form": form, "nv": nv, "wrench_col": [0, 6], "torque_col": 12 if form == "static" else -1, "contacts": ("l_sole", "r_sole"),
                      "mass": mass, "com_gains": (25.0, 10.0, 1.0), "task": (0, 0), "task_index": 0, "static_block": static_block,
                      "com_acc_ref": rng.uniform(-com_acc, com_acc, (B, 3))}}
    return plan, leaf, model


def make_wide_force_stack(B, seed=None, nv=64, n_contacts=8, eps_factor=1e6):
    """The "static" form of make_coman_force_stack at the producer's limits, on synthetic model quantities: nv = 64 coordinates, eight
    surface contacts, x = [8 wrenches (48); tau (58)], n = 106 -- the wide route (osot_solver_create_wide).  No tree: leaf["force"]
    ["quantities"] holds pose, Jc, com, momentum, h_gravity (what the producers would write), made so that a nominal wrench set W0
    strictly inside every cone and CoP rectangle balances the gravity term (asserted): h_gravity = sum_c Jc_c' W0_c + [0; tau0].
    level 0 = force::FloatingBase, level 1 = force::Wrenches with references near W0; rows: StaticConstraint (58 equalities),
    force::FrictionCone, force::CoP, force::WrenchLimits.  Returns (plan, leaf, None) for dynamics.ForceStep(kin_model=None)."""
    rng = np.random.default_rng(43000 if seed is None else seed)
    C_, na = n_contacts, nv - 6
    nf = 6 * C_
    n = nf + na
    assert n <= abi.MAX_QP_VARS and C_ <= abi.FORCE_MAX_CONTACTS
    mu = 0.8
    Jc = np.zeros((B, C_, 6, nv))
    Jc[:, :, :, :6] = rng.normal(0.0, 0.5, size=(B, C_, 6, 6))
    for ct in range(C_):
        cols = 6 + (7 * ct + np.arange(7)) % na
        Jc[:, ct][:, :, cols] = rng.normal(0.0, 0.3, size=(B, 6, 7))
    wRl = _rot_exp(rng.normal(0.0, 0.15, size=(B, C_, 3)))
    lims = np.stack([rng.uniform(-0.12, -0.08, size=(B, C_)), rng.uniform(0.10, 0.15, size=(B, C_)),
                     rng.uniform(-0.07, -0.05, size=(B, C_)), rng.uniform(0.05, 0.07, size=(B, C_))], axis=2)
    fz = rng.uniform(40.0, 80.0, size=(B, C_))
    f_loc = np.stack([rng.uniform(-3, 3, size=(B, C_)), rng.uniform(-3, 3, size=(B, C_)), fz], axis=2)
    cx = (lims[..., 0] + lims[..., 1]) / 2 + rng.uniform(-0.01, 0.01, size=(B, C_))
    cy = (lims[..., 2] + lims[..., 3]) / 2 + rng.uniform(-0.01, 0.01, size=(B, C_))
    t_loc = np.stack([cy * fz, -cx * fz, rng.uniform(-0.3, 0.3, size=(B, C_))], axis=2)
    W0 = np.concatenate([np.einsum("bcij,bcj->bci", wRl, f_loc), np.einsum("bcij,bcj->bci", wRl, t_loc)], axis=2)
    for kind in (abi.ROWS_WRENCH_FRICTION_CONE, abi.ROWS_COP):
        for ct in range(C_):
            v = np.einsum("brj,bj->br", wrench_rows(kind, wRl[:, ct], lims[:, ct], mu), W0[:, ct])
            assert v.max() < -1e-3, (kind, ct, v.max())
    h = np.einsum("bcij,bci->bj", Jc, W0) + np.concatenate([np.zeros((B, 6)), rng.normal(0.0, 5.0, size=(B, na))], axis=1)
    pose = [np.concatenate([wRl[:, ct].reshape(B, 9), rng.uniform(-0.5, 0.5, (B, 3))], axis=1) for ct in range(C_)]
    z = lambda *sh: np.zeros(sh)
    levels = [[Task(abi.TASK_GENERIC, 6, name="floating_base")], [Task(abi.TASK_GENERIC, nf, name="wrenches")]]
    Asel = np.zeros((nf, n)); Asel[:, :nf] = np.eye(nf)
    w_ref = W0.reshape(B, nf) + rng.normal(0.0, 1.0, size=(B, nf))
    rowblocks, rleaf = _force_rowblocks(B, C_, mu, np.ascontiguousarray(wRl.reshape(B, C_, 9)), np.ascontiguousarray(lims))
    rowblocks.insert(0, Rows(abi.ROWS_GENERIC, na, name="static_constraint"))
    rleaf.insert(0, (z(B, na, n), z(B, na), z(B, na)))
    plan = StackPlan(n=n, levels=levels, bounds=[], rowblocks=rowblocks, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [z(B, 6, n), np.tile(Asel, (B, 1, 1))], "task": [[(z(B, 6), None, None)], [(w_ref, None, None)]],
            "bound": [], "rows": rleaf, "C": [None] * 4,
            "force": {"form": "static", "nv": nv, "wrench_col": [6 * c for c in range(C_)], "torque_col": nf, "contacts": None,
                      "mass": 60.0, "com_gains": (25.0, 10.0, 1.0), "task": (0, 0), "task_index": 0, "static_block": 0,
                      "quantities": {"pose": pose, "Jc": Jc, "com": rng.uniform(-0.2, 0.2, (B, 3)), "momentum": z(B, 6), "h_gravity": h},
                      "nominal": W0.reshape(B, nf)}}
    return plan, leaf, None


# ---- the tasks driven by measurements: references and rows from osot_feedback (opensot_amd/feedback.py) -------------------------------
def min_joint_vel_task(n, dT, eps=1.0, name="MinJointVel"):
    """tasks::acceleration::MinJointVel (src/tasks/acceleration/MinJointVel.cpp:6-34) needs no kind of its own: it is an
    acceleration::Postural with lambda = 0, lambda2 = 1 / dT and zero references, b = -qdot / dT, weighted eps I (setEps).  The leaf is
    the OSOT_TASK_ACC_POSTURAL one with p0 = [0 ; -qdot], p2 = NULL."""
    if eps < 0.0:
        raise ValueError("eps should be positive!")
    return Task(abi.TASK_ACC_POSTURAL, n, weight=float(eps), lam=0.0, lam2=1.0 / float(dT), name=name)


def collision_task_rows(stack, dev, level, block, pair_J, pair_dist):
    """tasks::velocity::CollisionAvoidance (the task built on the constraint's rows): the `ca` group of feedback.Feedback.bind that writes
    A = -J and b = err of the violated pairs into block `block` of level `level`, an OSOT_TASK_GENERIC block with one row per pair.
    pair_J ([B][n_pairs][n], or (tensor, first row)) and pair_dist [B][n_pairs] are what osot_kinematics wrote."""
    tasks = stack.plan.levels[level]
    assert tasks[block].kind == abi.TASK_GENERIC
    return dict(J=pair_J, dist=pair_dist, A=(stack.A[level], sum(t.rows for t in tasks[:block])), b=dev["task"][level][block][0])


def make_cartesian_admittance_stack(B, seed=None, tree=None, frame="l_wrist", K=(500.0, 500.0, 500.0, 50.0, 50.0, 50.0), lam=0.01, dt=0.002,
                                    wall=0.03, stiffness=2000.0, eps_factor=1e6):
    """`(CartesianAdmittance(l_wrist) / postural) << joint_limits << velocity_limits` on the reference's COMAN: the wrist's pose and
    Jacobian are left for the kinematics producer, the task's desired twist (leaf p2) for osot_feedback.  The admittance is the
    constructor's with setImpedanceParams(K, 1.1 K dt / lambda, lambda, dt); the task's lambda is that lambda.  The measured wrench is
    the caller's: leaf["state"]["wall"] [B][3] is a point `wall` metres from the first posture's wrist for the virtual spring
    f = stiffness (x_wall - x) the tests and tools drive it with.  Returns (plan, leaf, model, fmodel); bind_cartesian_admittance()
    wires the device tensors."""
    from .feedback import FeedbackModel
    rng = np.random.default_rng(34000 if seed is None else seed)
    model, q0, qmin, qmax = _coman_bent(rng, B, tree)
    n = model.n
    fmodel = FeedbackModel(n, floating_base=True)
    t = fmodel.add_cartesian_admittance(**FeedbackModel.cartesian_admittance_defaults())
    K = np.asarray(K, dtype=float)
    fmodel.set_impedance_params(t, K, 1.1 * K * dt / lam, lam, dt)
    d = rng.normal(size=(B, 3))
    z = lambda *sh: np.zeros(sh)
    levels = [[Task(abi.TASK_CARTESIAN, 6, lam=lam, name="admittance::" + frame)], [Task(abi.TASK_POSTURAL, n, lam=0.01, name="postural")]]
    bounds = [Bound(abi.BOUND_JOINT_LIMITS, scaling=1.0, name="joint_limits"), Bound(abi.BOUND_VELOCITY_LIMITS, dT=0.05, name="velocity_limits")]
    plan = StackPlan(n=n, levels=levels, bounds=bounds, eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [z(B, 6, n), None], "task": [[(z(B, 12), z(B, 12), z(B, 6))], [(q0.copy(), q0.copy(), None)]],
            "bound": [(q0.copy(), np.tile(qmin, (B, 1)), np.tile(qmax, (B, 1))), (np.full((B, n), 2.0), None, None)],
            "rows": [], "C": [],
            "state": {"q0": q0, "q_ref": q0.copy(), "frame": frame, "wall": wall * d / np.linalg.norm(d, axis=1, keepdims=True),
                      "stiffness": stiffness}}
    return plan, leaf, model, fmodel


def bind_cartesian_admittance(stack, kin, fbk, leaf):
    """wire make_cartesian_admittance_stack to the device: one q tensor is the kinematics producer's input, the Postural task's and the
    joint limits' q; the producer writes the wrist's pose into the Cartesian task's p0 (= osot_feedback's cart_pose) and its Jacobian
    into stack.A[0]; osot_feedback (fbk: a feedback.Feedback of the stack's model) writes the task's p2 from `wrench` [B][6], the
    caller's measurement.  The task's reference pose is the first posture's.  -> (dev_leaf, kin_batch, q, wrench)"""
    import torch
    B, s = leaf["B"], leaf["state"]
    dev = stack.load_leaf(leaf)
    f64 = dict(dtype=torch.float64, device=stack.device)
    q = torch.as_tensor(s["q0"], **f64).contiguous()
    f = kin.model.frame_index(s["frame"])
    pose, twist, wrench = torch.zeros((B, 12), **f64), torch.zeros((B, 6), **f64), torch.zeros((B, 6), **f64)
    kw = dict(frame_pose={f: pose}, frame_J={f: (stack.A[0], 0)})
    kin.forward(q, **kw)
    dev["task"][0][0] = (pose, pose.clone(), twist)
    dev["task"][1][0] = (q, dev["task"][1][0][1], None)
    dev["bound"][0] = (q,) + tuple(dev["bound"][0][1:])
    fbk.bind(cart=[dict(pose=pose, wrench=wrench, twist_out=twist)])
    return dev, kin.batch_args(q, **kw), q, wrench


def make_joint_admittance_stack(B, seed=None, tree=None, inertia=None, dense=False, eps_factor=1e6):
    """`JointAdmittance << joint_limits << velocity_limits` on the reference's COMAN: one Postural level (lambda = 0.005, the
    constructor's) whose desired velocity (leaf p2) is osot_feedback's C filter(h - tau), h from osot_dynamics, tau the caller's
    measurement.  dense: a symmetric positive definite compliance matrix around the constructor's 0.00015 I instead of the scalar.
    Returns (plan, leaf, model, fmodel); leaf["state"] = q0, q_ref, joint_C ([n][n] or None); bind_joint_admittance() wires the tensors."""
    import os
    from . import kinematics as kin
    from .feedback import FeedbackModel
    here = os.path.dirname(os.path.abspath(__file__))
    gold = os.path.join(os.path.dirname(here), "tests", "golden")
    rng = np.random.default_rng(35000 if seed is None else seed)
    _, q0, qmin, qmax = _coman_bent(rng, B, tree)
    model, _, _ = kin.from_json(tree or os.path.join(gold, "coman_tree.json"), inertia or os.path.join(gold, "coman_inertia.json"))
    n = model.n
    defaults = FeedbackModel.joint_admittance_defaults()
    fmodel = FeedbackModel(n, floating_base=True)
    fmodel.set_joint_admittance(**defaults)
    Cm = None
    if dense:
        G = rng.normal(0.0, 0.1, (n, n))
        Cm = defaults["C"] * (np.eye(n) + 0.5 * (G + G.T) / n)
    q_ref = q0.copy()
    q_ref[:, 6:] += rng.uniform(-0.05, 0.05, (B, n - 6))
    plan = StackPlan(n=n, levels=[[Task(abi.TASK_POSTURAL, n, lam=defaults["lam"], name="joint_admittance")]],
                     bounds=[Bound(abi.BOUND_JOINT_LIMITS, scaling=1.0, name="joint_limits"), Bound(abi.BOUND_VELOCITY_LIMITS, dT=0.05, name="velocity_limits")],
                     eps_abs=eps_abs_from_factor(eps_factor))
    leaf = {"B": B, "A": [None], "task": [[(q0.copy(), q_ref, np.zeros((B, n)))]],
            "bound": [(q0.copy(), np.tile(qmin, (B, 1)), np.tile(qmax, (B, 1))), (np.full((B, n), 2.0), None, None)],
            "rows": [], "C": [], "state": {"q0": q0, "q_ref": q_ref, "joint_C": Cm}}
    return plan, leaf, model, fmodel


def bind_joint_admittance(stack, dyn, fbk, leaf):
    """wire make_joint_admittance_stack to the device: one q tensor is the dynamics producer's input, the Postural task's and the joint
    limits' q; osot_dynamics (dyn: a dynamics.Dynamics of the model, at rest) writes h, osot_feedback the task's p2 from h and `tau`
    [B][n], the caller's measurement.  -> (dev_leaf, dyn_batch, q, tau, h)"""
    import torch
    B, s = leaf["B"], leaf["state"]
    n = stack.plan.n
    dev = stack.load_leaf(leaf)
    f64 = dict(dtype=torch.float64, device=stack.device)
    q = torch.as_tensor(s["q0"], **f64).contiguous()
    h, tau, qd = torch.zeros((B, n), **f64), torch.zeros((B, n), **f64), torch.zeros((B, n), **f64)
    dev["task"][0][0] = (q, dev["task"][0][0][1], qd)
    dev["bound"][0] = (q,) + tuple(dev["bound"][0][1:])
    joint = dict(tau=tau, h=h, qdot_out=qd)
    if s["joint_C"] is not None:
        joint["C"] = torch.as_tensor(s["joint_C"], **f64).contiguous()
    fbk.bind(joint=joint)
    return dev, dyn.batch_args(q, None, h=h), q, tau, h


def bind_base_estimation(stack, kin, leaf, fbk=None):
    """wire make_base_estimation_stack to the device: the producer writes the contacts' A into stack.A[0] and their b into the blocks'
    leaves -- with contact_lambda != 0 into a buffer of its own, from which osot_feedback (one call per contact: fbks, a list of
    feedback.Feedback) forms the leaf's b = b_in + lambda err against leaf["state"]["contact_pose_ref"] (zeros: the first posture's
    contact poses are taken).  With imu=True the base link's Jacobian and pose go to buffers osot_feedback reads, the gyroscope
    reading is leaf["state"]["imu_omega"], and the IMU block's rows land behind the contacts' in stack.A[0], its b in its leaf.
    fbk: a feedback.Feedback of leaf["state"]["feedback"], or None to make them here.
    -> (dev_leaf, kin_batch, q, qdot, fbks): launch every entry of fbks between osot_kinematics and osot_cycle"""
    import torch
    from .feedback import Feedback
    B, s = leaf["B"], leaf["state"]
    legs, n, rows = len(kin.model.wheel_joints), kin.model.n, s.get("contact_rows", 3)
    dev = stack.load_leaf(leaf)
    f64 = dict(dtype=torch.float64, device=stack.device)
    q, qdot = torch.as_tensor(s["q0"], **f64).contiguous(), torch.as_tensor(s["qdot"], **f64).contiguous()
    lam, imu = s.get("contact_lambda", 0.0), s.get("imu", False)
    b_in = torch.zeros((B, 6 * legs), **f64) if lam != 0.0 else None
    kw = dict(rowset_A={i: (stack.A[0], rows * i) for i in range(legs)}, qdot=qdot,
              rowset_b={i: ((b_in, 6 * i) if lam != 0.0 else (dev["task"][0][i][0], 0)) for i in range(legs)})
    fbks = []
    if lam != 0.0:
        poses = [torch.zeros((B, 12), **f64) for _ in range(legs)]
        kw["frame_pose"] = {1 + i: poses[i] for i in range(legs)}
    if imu:
        base_pose, base_J = torch.zeros((B, 12), **f64), torch.zeros((B, 6, n), **f64)
        kw.setdefault("frame_pose", {})[0] = base_pose
        kw["frame_J"] = {0: (base_J, 0)}
    kin.forward(q, **kw)
    if lam != 0.0:
        ref = torch.as_tensor(s["contact_pose_ref"], **f64).contiguous()
        for i in range(legs):
            if not np.any(s["contact_pose_ref"][:, i]):
                ref[:, i] = poses[i]
    for i in range(legs if lam != 0.0 else 0):
        f = Feedback(s["feedback"], B, stack.device) if (fbk is None or i > 0) else fbk
        f.bind(contact=dict(pose=poses[i], pose_ref=ref[:, i].contiguous(), b_in=(b_in, 6 * i), b_out=dev["task"][0][i][0]),
               imu=dict(fb_J=base_J, pose=base_pose, omega=torch.as_tensor(s["imu_omega"], **f64).contiguous(),
                        A=(stack.A[0], rows * legs), b=dev["task"][0][legs][0]) if (imu and i == 0) else None)
        fbks.append(f)
    if imu and lam == 0.0:
        f = Feedback(s["feedback"], B, stack.device) if fbk is None else fbk
        f.bind(imu=dict(fb_J=base_J, pose=base_pose, omega=torch.as_tensor(s["imu_omega"], **f64).contiguous(),
                        A=(stack.A[0], rows * legs), b=dev["task"][0][legs][0]))
        fbks.append(f)
    return dev, kin.batch_args(q, **kw), q, qdot, fbks
