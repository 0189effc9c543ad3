"""tests/momentum_ref.py -- TEST INFRASTRUCTURE ONLY: numpy restatement of the centroidal momentum outputs of the dynamics
producer (opensot_amd/csrc/osot_dyn.h, stage 5a) by a DIFFERENT algorithm.

The kernel shifts F_j = Ic_j S_j, the composite-inertia product it forms for the inertia matrix, from the world origin to the
centre of mass.  Here everything comes from the dense LINK JACOBIANS of tests/dyn_ref.py (no recursion over the tree, no
composite inertia), with Jv_l at the link's centre of mass c_l and c_G the centre of mass of the whole tree:
    A_lin = sum_l  m_l Jv_l
    A_ang = sum_l  Ibar_l Jw_l + m_l [c_l - c_G]x Jv_l
    h_G   = A qdot
and, as a second value that uses no Jacobian of a sum, from the link velocities themselves:
    h_G   = [sum_l m_l v_cl;  sum_l Ibar_l w_l + m_l (c_l - c_G) x v_cl]
Rows are [linear (3); angular (3)], world axes, about the centre of mass."""
import numpy as np

import dyn_ref


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def one(model, q, qdot=None):
    """dict(cmm [6][n], momentum [6], momentum_links [6], com [3], total_mass) at one posture"""
    r = dyn_ref.Ref(model, q, qdot)
    n, mass = model.n, np.asarray(model.mass, dtype=float)
    mt = mass.sum()
    cG = (mass[:, None] * r.cw).sum(axis=0) / mt
    A = np.zeros((6, n))
    hl = np.zeros(6)
    for l in range(n):
        J = r.jac(l, r.cw[l])
        A[:3] += mass[l] * J[:3]
        A[3:] += r.Ibar[l] @ J[3:] + mass[l] * skew(r.cw[l] - cG) @ J[:3]
        # the link's own velocities: angular velocity, and the joint origin's velocity carried to the centre of mass
        w = r.w[l]
        vc = r.vo[l] + np.cross(w, r.cw[l] - r.pw[l])
        hl[:3] += mass[l] * vc
        hl[3:] += r.Ibar[l] @ w + mass[l] * np.cross(r.cw[l] - cG, vc)
    return dict(cmm=A, momentum=A @ r.qd, momentum_links=hl, com=cG, total_mass=mt)


def batch(model, q, qdot=None):
    """q [B][n] (qdot likewise or None) -> dict(cmm [B][6][n], momentum [B][6], momentum_links [B][6], com [B][3])"""
    parts = [one(model, q[i], None if qdot is None else qdot[i]) for i in range(len(q))]
    return {k: np.array([p[k] for p in parts]) for k in ("cmm", "momentum", "momentum_links", "com")}
