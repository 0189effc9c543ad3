"""tests/dyn_ref.py -- TEST INFRASTRUCTURE ONLY: numpy restatement of the rigid-body dynamics producer by a DIFFERENT algorithm.

The kernel (opensot_amd/csrc/osot_dyn.h) works with spatial vectors about the world origin, ancestor sums and subtree
aggregates.  Here everything comes from dense LINK JACOBIANS on top of oracle.pykin's forward kinematics (projected
Newton-Euler / Kane's form, no recursion over the tree):
    M   = sum_l  m_l Jv_l' Jv_l + Jw_l' (R_l I_l R_l') Jw_l
    h   = sum_l  Jv_l' m_l (Jvdot_l qdot - g) + Jw_l' (Ibar_l Jwdot_l qdot + w_l x Ibar_l w_l)
    tau = the same sums with  Jv_l qddot + Jvdot_l qdot  and  Jw_l qddot + Jwdot_l qdot  (= M qddot + h)
with Jv_l at the link's centre of mass and Jdot the ANALYTIC time derivative of the Jacobian columns
(d/dt z_j = w_j x z_j, d/dt (p - p_j) = v_p - v_pj).  Jdot qdot of a frame / of the CoM are the same derivative applied to qdot."""
import numpy as np

from oracle import pykin


def inertia_of(model):
    I6 = np.zeros((model.n, 6)) if getattr(model, "inertia", None) is None else np.asarray(model.inertia, dtype=float).reshape(model.n, 6)
    I = np.zeros((model.n, 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        I[:, a, b] = I6[:, k]; I[:, b, a] = I6[:, k]
    return I


class Ref:
    """everything at one (q, qdot)"""

    def __init__(self, model, q, qdot=None, gravity=(0.0, 0.0, -9.81)):
        self.m, self.n = model, model.n
        n = self.n
        self.q = np.asarray(q, dtype=float)
        self.qd = np.zeros(n) if qdot is None else np.asarray(qdot, dtype=float)
        self.g = np.asarray(gravity, dtype=float)
        self.fk = pykin.forward(model, self.q)
        self.Rw, self.pw = self.fk["Rw"], self.fk["pw"]
        self.z = np.einsum("jab,jb->ja", self.Rw, model.axis)
        self.cw = np.einsum("jab,jb->ja", self.Rw, model.com) + self.pw
        self.anc = []
        for j in range(n):
            self.anc.append([j] + (self.anc[model.parent[j]] if model.parent[j] >= 0 else []))
        self.Ibar = np.einsum("jab,jbc,jdc->jad", self.Rw, inertia_of(model), self.Rw)
        # angular velocity of every link and linear velocity of every joint origin
        self.w = np.array([self.jac(j, self.pw[j])[3:] @ self.qd for j in range(n)])
        self.vo = np.array([self.jac(j, self.pw[j])[:3] @ self.qd for j in range(n)])

    def jac(self, l, p):
        """6 x n [linear; angular] Jacobian of the point p (world) fixed to link l"""
        J = np.zeros((6, self.n))
        for j in self.anc[l]:
            if self.m.jtype[j] == 0:
                J[:3, j] = np.cross(self.z[j], p - self.pw[j]); J[3:, j] = self.z[j]
            else:
                J[:3, j] = self.z[j]
        return J

    def jac_dot(self, l, p):
        """its analytic time derivative along qdot"""
        Jd = np.zeros((6, self.n))
        vp = self.jac(l, p)[:3] @ self.qd
        for j in self.anc[l]:
            zd = np.cross(self.w[j], self.z[j])
            if self.m.jtype[j] == 0:
                Jd[:3, j] = np.cross(zd, p - self.pw[j]) + np.cross(self.z[j], vp - self.vo[j]); Jd[3:, j] = zd
            else:
                Jd[:3, j] = zd
        return Jd

    def inertia_matrix(self):
        M = np.zeros((self.n, self.n))
        for l in range(self.n):
            J = self.jac(l, self.cw[l])
            M += self.m.mass[l] * J[:3].T @ J[:3] + J[3:].T @ self.Ibar[l] @ J[3:]
        return M

    def tau(self, qddot=None):
        """generalised forces for qddot (None: zero, i.e. the non-linear term h)"""
        qdd = np.zeros(self.n) if qddot is None else np.asarray(qddot, dtype=float)
        t = np.zeros(self.n)
        for l in range(self.n):
            J, Jd = self.jac(l, self.cw[l]), self.jac_dot(l, self.cw[l])
            a = J @ qdd + Jd @ self.qd
            w = J[3:] @ self.qd
            t += J[:3].T @ (self.m.mass[l] * (a[:3] - self.g)) + J[3:].T @ (self.Ibar[l] @ a[3:] + np.cross(w, self.Ibar[l] @ w))
        return t

    def frame_jdot_qdot(self, f):
        _, jf, _, pf = self.m.frames[f]
        p = self.pw[jf] + self.Rw[jf] @ np.asarray(pf, dtype=float)
        return self.jac_dot(jf, p) @ self.qd

    def frame_jacobian(self, f):
        _, jf, _, pf = self.m.frames[f]
        return self.jac(jf, self.pw[jf] + self.Rw[jf] @ np.asarray(pf, dtype=float))

    def com_jdot_qdot(self):
        s = np.zeros(3)
        for l in range(self.n):
            s += self.m.mass[l] * (self.jac_dot(l, self.cw[l])[:3] @ self.qd)
        return s / self.m.mass.sum()


def batch(model, q, qdot=None, gravity=(0.0, 0.0, -9.81)):
    """q [B][n] (qdot likewise or None) -> dict(M [B][n][n], h [B][n], jdq [B][F][6], com_jdq [B][3])"""
    B, n = q.shape
    F = len(model.frames)
    out = dict(M=np.zeros((B, n, n)), h=np.zeros((B, n)), jdq=np.zeros((B, F, 6)), com_jdq=np.zeros((B, 3)))
    for i in range(B):
        r = Ref(model, q[i], None if qdot is None else qdot[i], gravity)
        out["M"][i] = r.inertia_matrix(); out["h"][i] = r.tau()
        for f in range(F):
            out["jdq"][i, f] = r.frame_jdot_qdot(f)
        out["com_jdq"][i] = r.com_jdot_qdot()
    return out
