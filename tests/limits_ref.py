"""The recursively feasible joint limits and the Cartesian position constraint restated in numpy (test infrastructure): the update()s of
acceleration::JointLimitsViability (src/constraints/acceleration/JointLimitsViability.cpp:79-190), acceleration::JointLimitsECBF
(JointLimitsECBF.cpp:36-71), velocity::JointLimitsInvariance (src/constraints/velocity/JointLimitsInvariance.cpp:47-206) and
velocity::CartesianPositionConstraint (CartesianPositionConstraint.cpp:81-108, both constructors), vectorised over [B][rows], in the
reference's order of operations and IN THE DTYPE OF THEIR INPUTS (float64, or np.longdouble to measure the formulas' own rounding
sensitivity).

smin / smax are std::min / std::max as the reference's compiler spells them, `(b < a) ? b : a` and `(a < b) ? b : a`: a NaN second
argument is ignored.  Viability's M2 = -qdot^2 / (2 (q_max - q)) is -0/0 for a joint exactly on its limit at rest, and
std::min(M1, NaN) is M1; np.minimum / np.maximum would hand the NaN on.

The leaf carries ONE q - q_neutral (the product's convention, that of OSOT_ROWS_ACC_JOINT_LIMITS); the reference takes the raw q in
M2 / m2 and difference(q, neutral) elsewhere, the same thing for a zero neutral posture.

The oracle knows nothing of these kinds, so every comparison with it goes through the GENERIC TWIN of a plan: the same stack with each
new block replaced by OSOT_ROWS_UNIT_GENERIC / OSOT_ROWS_GENERIC / OSOT_BOUND_GENERIC carrying the numbers written out here."""
import ctypes as C

import numpy as np

from opensot_amd import abi
from opensot_amd.plan import Bound, Rows, StackPlan

LO = -1.0e20
LIMIT_KINDS = (abi.ROWS_ACC_JOINT_LIMITS_VIABILITY, abi.ROWS_ACC_JOINT_LIMITS_ECBF)
POSITION_KINDS = (abi.ROWS_POSITION_CARTESIAN, abi.ROWS_POSITION_COM)

# rounding sensitivity of the reference's formulas on the tests' inputs, max |fp64 - longdouble| (measured on x86-64, 80-bit long double;
# DESIGN.md): used where np.longdouble is no wider than float64
RECORDED_SENSITIVITY = {("viability", 1e-3): 1.1e-10, ("viability", 1e-2): 2.6e-12, "ecbf": 1.3e-14, "invariance": 3e-19}


def smin(a, b):
    """std::min(a, b) = (b < a) ? b : a, elementwise"""
    with np.errstate(invalid="ignore"):
        return np.where(b < a, b, a)


def smax(a, b):
    """std::max(a, b) = (a < b) ? b : a, elementwise"""
    with np.errstate(invalid="ignore"):
        return np.where(a < b, b, a)


def _swap_clamp(lb, ub, amax):
    """computeJointAccBounds' tail: swap where ub < lb, then clamp both into [-amax, amax] -> lb, ub, swapped"""
    swapped = ub < lb
    lb, ub = np.where(swapped, ub, lb), np.where(swapped, lb, ub)
    lb = np.where(lb < -amax, -amax, lb)
    ub = np.where(ub > amax, amax, ub)
    return lb, ub, swapped


def viability_bounds(q, qdot, qmin, qmax, vmax, amax, dT, p):
    """JointLimitsViability::update -> (lb, ub, swapped)"""
    T = q.dtype.type
    two, four = T(2.0), T(4.0)
    dt = T(p) * T(dT)
    a = dt * dt
    with np.errstate(divide="ignore", invalid="ignore"):
        # accBoundsFromPosLimits
        M1 = -qdot / dt
        M2 = -(qdot * qdot) / (two * (qmax - q))
        M3 = two * (qmax - q - dt * qdot) / a
        m2 = (qdot * qdot) / (two * (q - qmin))
        m3 = two * (qmin - q - dt * qdot) / a
        pos = qdot >= 0
        ub_pos = np.where(pos, np.where(M3 > M1, M3, smin(M1, M2)), M3)
        lb_pos = np.where(pos, m3, np.where(m3 < M1, m3, smax(M1, m2)))
        # accBoundsFromViability
        b1 = dt * (two * qdot + amax * dt)
        c1 = qdot * qdot - two * amax * (qmax - q - dt * qdot)
        d1 = b1 * b1 - four * a * c1
        ub_via = np.where(d1 >= 0, smax(M1, (-b1 + np.sqrt(np.where(d1 >= 0, d1, 0))) / (two * a)), M1)
        b2 = dt * (two * qdot - amax * dt)
        c2 = qdot * qdot - two * amax * (q + dt * qdot - qmin)
        d2 = b2 * b2 - four * a * c2
        lb_via = np.where(d2 >= 0, smin(M1, (-b2 - np.sqrt(np.where(d2 >= 0, d2, 0))) / (two * a)), M1)
        # computeJointAccBounds
        ub_vel = (vmax - qdot) / dt
        lb_vel = (-vmax - qdot) / dt
        ub = smin(smin(smin(ub_pos, ub_vel), ub_via), amax)
        lb = smax(smax(smax(lb_pos, lb_vel), lb_via), -amax)
    return _swap_clamp(lb, ub, amax)


def ecbf_bounds(q, qdot, qmin, qmax, vmax, amax, a1, a2, a3):
    """JointLimitsECBF::update -> (lb, ub, swapped)"""
    lower = -(a1 + a2) * qdot + (a1 * a2) * (qmin - q)
    upper = -(a1 + a2) * qdot + (a1 * a2) * (qmax - q)
    ub = smin(smin(upper, a3 * (vmax - qdot)), amax)
    lb = smax(smax(lower, a3 * (-vmax - qdot)), -amax)
    return _swap_clamp(lb, ub, amax)


def invariance_bounds(q, qdot_prev, qmin, qmax, amax, dt, p):
    """JointLimitsInvariance::update -> (lb, ub, swapped)"""
    T = q.dtype.type
    dt, p, two = T(dt), T(p), T(2.0)
    sup, inf = qmax - q, qmin - q
    with np.errstate(invalid="ignore"):
        acc = dt * dt * amax + dt * qdot_prev
        d = two * amax * dt * dt * p * sup
        via = np.where(d < 0, -np.sqrt(np.abs(d)), np.sqrt(np.abs(d)))
        ub = np.where(qdot_prev <= 0, np.where(sup < acc, sup, acc), np.where(via < acc, via, acc))
        acc = -dt * dt * amax + dt * qdot_prev
        d = two * -amax * dt * dt * p * inf
        via = np.where(d < 0, np.sqrt(np.abs(d)), -np.sqrt(np.abs(d)))
        lb = np.where(qdot_prev >= 0, np.where(inf > acc, inf, acc), np.where(via > acc, via, acc))
    swapped = lb > ub
    return np.where(swapped, ub, lb), np.where(swapped, lb, ub), swapped


def position_rows(J, x, Ac, bc, scaling):
    """CartesianPositionConstraint::update -> (C [B][R][n], lo [B][R], up [B][R]); J [B][>= 3][n] (rows 0 .. 2 are used), x [B][3],
    Ac [B][R][3], bc [B][R]"""
    Cw = np.einsum("brk,bkn->brn", Ac, J[:, :3])
    up = (bc - np.einsum("brk,bk->br", Ac, x)) * scaling
    return Cw, np.full(up.shape, LO), up


# ---- the blocks of a plan from their leaf inputs -----------------------------------------------------------------------------------
def split(a, k):
    """[B][k * r] -> k arrays [B][r]"""
    a = np.asarray(a)
    r = a.shape[1] // k
    return [a[:, i * r:(i + 1) * r] for i in range(k)]


def limit_block(rb, p0, p1, p2, dtype=np.float64):
    """(lb, ub, swapped) of a Viability / ECBF row block rb (plan.Rows) from its leaf inputs, evaluated in dtype"""
    cv = lambda a: np.asarray(a, dtype=dtype)
    q, qd = split(cv(p0), 2)
    qmin, qmax = split(cv(p1), 2)
    if rb.kind == abi.ROWS_ACC_JOINT_LIMITS_VIABILITY:
        vmax, amax = split(cv(p2), 2)
        return viability_bounds(q, qd, qmin, qmax, vmax, amax, rb.dT, rb.p)
    vmax, amax, a1, a2, a3 = split(cv(p2), 5)
    return ecbf_bounds(q, qd, qmin, qmax, vmax, amax, a1, a2, a3)


def invariance_block(bd, p0, p1, p2, dtype=np.float64):
    cv = lambda a: np.asarray(a, dtype=dtype)
    qmin, qmax, amax = split(cv(p1), 3)
    return invariance_bounds(cv(p0), cv(p2), qmin, qmax, amax, bd.dT, bd.scaling)


def position_block(rb, p0, p1, p2, n):
    p0, p1, p2 = (np.asarray(a, dtype=float) for a in (p0, p1, p2))
    B, R = p0.shape[0], rb.rows
    cart = rb.kind == abi.ROWS_POSITION_CARTESIAN
    J = p0.reshape(B, 6 if cart else 3, n)
    x = p1.reshape(B, -1)[:, 9:12] if cart else p1.reshape(B, 3)
    return position_rows(J, x, p2[:, :3 * R].reshape(B, R, 3), p2[:, 3 * R:], rb.bound_scaling)


def tolerance(f64, wide, recorded, value):
    """the allowance of check 2: max(10 x max|fp64 - longdouble|, 1e-13 max(1, |value|)), elementwise in value; where np.longdouble is
    no wider than float64 the recorded sensitivity stands in (and the caller says so)"""
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        sens = float(np.abs(f64.astype(np.longdouble) - wide).max())
    else:
        sens = recorded
    return np.maximum(10.0 * sens, 1e-13 * np.maximum(1.0, np.abs(value))), sens


def generic_twin(plan, leaf):
    """the same stack with every Viability / ECBF block as OSOT_ROWS_UNIT_GENERIC (lo, up), every position block as OSOT_ROWS_GENERIC
    (C, lo, up) and the invariance bound as OSOT_BOUND_GENERIC (l, u) -> (plan, leaf)"""
    blocks, rows, Cl = [], [], []
    Cin = leaf.get("C") or [None] * len(plan.rowblocks)
    for j, rb in enumerate(plan.rowblocks):
        if rb.kind in LIMIT_KINDS:
            lb, ub, _ = limit_block(rb, *leaf["rows"][j])
            blocks.append(Rows(abi.ROWS_UNIT_GENERIC, rb.rows, first_col=rb.first_col, name=rb.name + "_generic", level=rb.level))
            rows.append((lb, ub, None)); Cl.append(None)
        elif rb.kind in POSITION_KINDS:
            blocks.append(Rows(abi.ROWS_GENERIC, rb.rows, name=rb.name + "_generic", level=rb.level))
            rows.append(position_block(rb, *leaf["rows"][j], plan.n)); Cl.append(None)
        else:
            blocks.append(rb); rows.append(leaf["rows"][j]); Cl.append(Cin[j])
    bounds, bleaf = [], []
    for j, bd in enumerate(plan.bounds):
        if bd.kind == abi.BOUND_JOINT_LIMITS_INVARIANCE:
            lb, ub, _ = invariance_block(bd, *leaf["bound"][j])
            bounds.append(Bound(abi.BOUND_GENERIC, name=bd.name + "_generic")); bleaf.append((lb, ub, None))
        else:
            bounds.append(bd); bleaf.append(leaf["bound"][j])
    twin = StackPlan(n=plan.n, levels=plan.levels, bounds=bounds, rowblocks=blocks, eps_abs=plan.eps_abs, max_iter=plan.max_iter)
    tleaf = dict(leaf)
    tleaf["rows"], tleaf["C"], tleaf["bound"] = rows, Cl, bleaf
    return twin, tleaf


# ---- the closed loops of the reference's tests, in numpy (the restatement driving itself) ----------------------------------------------
def acc_closed_loop(kind, qmin, qmax, dT, vmax, amax, p=1.0, alpha=15.0, lam=400.0, steps=(300, 300), keep_every=25, q0=None):
    """testBoundsWithTrajectory without a robot and without a solver: the one-level Postural QP under unit-row bounds is x = clip(b, lb,
    ub).  `steps[0]` cycles towards q_max + 1, then `steps[1]` towards q_min - 1; q += qdot dT + x dT^2 / 2, qdot += x dT.
    -> dict: kept states q, qdot [K][B][n] (every keep_every-th), max violation of q / qdot / x, fraction of active bounds"""
    B, n = qmin.shape
    q = 0.5 * (qmin + qmax) if q0 is None else q0.copy()                 # the middle of the range
    qd = np.zeros((B, n))
    V, A = np.full((B, n), vmax), np.full((B, n), amax)
    al = np.full((B, n), float(alpha))
    lam2 = 2.0 * np.sqrt(lam)
    kept_q, kept_qd = [], []
    viol, active, total, t = 0.0, 0, 0, 0
    for target, ns in ((qmax + 1.0, steps[0]), (qmin - 1.0, steps[1])):
        for _ in range(ns):
            if t % keep_every == 0:
                kept_q.append(q.copy()); kept_qd.append(qd.copy())
            t += 1
            if kind == abi.ROWS_ACC_JOINT_LIMITS_VIABILITY:
                lb, ub, _ = viability_bounds(q, qd, qmin, qmax, V, A, dT, p)
            else:
                lb, ub, _ = ecbf_bounds(q, qd, qmin, qmax, V, A, al, al, al)
            b = lam2 * (-qd) + lam * (target - q)
            x = np.clip(b, lb, ub)
            active += int((x != b).sum()); total += x.size
            q = q + qd * dT + 0.5 * x * dT * dT
            qd = qd + x * dT
            viol = max(viol, (q - qmax).max(), (qmin - q).max(), (np.abs(qd) - V).max(), (np.abs(x) - A).max())
    return {"q": np.stack(kept_q), "qdot": np.stack(kept_qd), "violation": viol, "active": active / total}


def invariance_closed_loop(qmin, qmax, dt, vmax, amax, p, lam=0.1, steps=(2500, 2500), keep_every=25):
    """TestJointLimitsInvariance's loop without a robot: dq = clip(lam (target - q), max(lb, -vmax dt), min(ub, vmax dt)), q += dq,
    qdot_prev = dq / dt -> dict: kept states q, qdot_prev [K][B][n], max limit violation, max (|delta qdot| / dt - amax)"""
    B, n = qmin.shape
    q = 0.5 * (qmin + qmax)
    v = np.zeros((B, n))
    A = np.full((B, n), amax)
    kept_q, kept_v = [], []
    viol, acc, t = 0.0, -np.inf, 0
    for target, ns in ((qmax + 1.0, steps[0]), (qmin - 1.0, steps[1])):
        for _ in range(ns):
            if t % keep_every == 0:
                kept_q.append(q.copy()); kept_v.append(v.copy())
            t += 1
            lb, ub, _ = invariance_bounds(q, v, qmin, qmax, A, dt, p)
            dq = np.clip(lam * (target - q), np.maximum(lb, -vmax * dt), np.minimum(ub, vmax * dt))
            q = q + dq
            vn = dq / dt
            acc = max(acc, (np.abs(vn - v) / dt - amax).max())
            v = vn
            viol = max(viol, (q - qmax).max(), (qmin - q).max())
    return {"q": np.stack(kept_q), "qdot": np.stack(kept_v), "violation": viol, "acc_excess": acc}


# ---- the update kernel's host builds (tests/emu), bounds included --------------------------------------------------------------------
def host_update(fn, plan, leaf, *extra):
    """AutoStack::update through an emulated update entry fn(plan, leaf, out, *extra) on host arrays (stacks without dense weights or
    regularisation) -> (rc, {"b", "C" (stored rows, pre-filled with 7), "lo", "up", "l", "u"})"""
    B, n, L = leaf["B"], plan.n, plan.L
    keep = []

    def p(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data
    lb = abi.LeafBatch(); lb.B = B
    for k, lev in enumerate(leaf["task"]):
        for j, (p0, p1, p2) in enumerate(lev):
            lb.task[k][j].p0, lb.task[k][j].p1, lb.task[k][j].p2 = p(p0), p(p1), p(p2)
    for j, (p0, p1, p2) in enumerate(leaf["bound"]):
        lb.bound[j].p0, lb.bound[j].p1, lb.bound[j].p2 = p(p0), p(p1), p(p2)
    for j, (p0, p1, p2) in enumerate(leaf["rows"]):
        lb.rows[j].p0, lb.rows[j].p1, lb.rows[j].p2 = p(p0), p(p1), p(p2)
    out = abi.AssembledOut()
    res = {"b": [np.zeros((B, plan.m(k))) for k in range(L)], "w": [np.ones((B, plan.m(k))) for k in range(L)],
           "C": np.full((B, plan.nc_stored, n), 7.0), "lo": np.zeros((B, plan.nc)), "up": np.zeros((B, plan.nc)),
           "l": np.zeros((B, n)), "u": np.zeros((B, n))}
    for k in range(L):
        out.b[k], out.w[k] = res["b"][k].ctypes.data, res["w"][k].ctypes.data
    for j, Cj in enumerate(leaf.get("C", [])):
        if Cj is not None:
            o = plan.rows_stored_offset(j)
            res["C"][:, o:o + Cj.shape[1]] = Cj
    out.C, out.lo, out.up = res["C"].ctypes.data, res["lo"].ctypes.data, res["up"].ctypes.data
    if plan.bounds:
        out.l, out.u = res["l"].ctypes.data, res["u"].ctypes.data
    pd = plan.to_c()
    rc = fn(C.byref(pd), C.byref(lb), C.byref(out), *extra)
    return rc, res
