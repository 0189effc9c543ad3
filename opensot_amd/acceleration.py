"""The acceleration task leaves on the device (include/osot_mi355x.h: osot_acc_tasks; csrc/osot_acc.h): pose, velocity and joint
errors of acceleration::Cartesian / CoM / Postural, their gain matrices, GainType::Force (Mi = J M^-1 J' and M^-1 v from one
Cholesky factor of the inertia matrix per instance) and computeInertiaInverse, from the tensors osot_kinematics and osot_dynamics
fill.  Plumbing only: the arithmetic is in csrc/osot_acc.h."""
import ctypes as C

import numpy as np
import torch

from . import abi

ACCELERATION, FORCE = abi.ACC_GAIN_ACCELERATION, abi.ACC_GAIN_FORCE


class AccModel:
    """osot_acc_model: the settings of the tasks, with the reference's defaults (Kp = Kd = I, orientation gain 1, GainType
    Acceleration, lambda = lambda2 = 1).

        cart      one dict per acceleration::Cartesian term: gain_type=, gain_matrices=, Kp=, Kd= (6 x 6, host), orientation_gain=
        com       None, or a dict: gain_matrices=, Kp=, Kd= (3 x 3, host)
        postural  None, or a dict: gain_type=, gain_matrices=, lam=, lam2=, Kp=, Kd= (nv x nv, host or device; None = the identity)
    """

    def __init__(self, nv, cart=(), com=None, postural=None, device=0):
        self.nv, self.n_cart, self.device = int(nv), len(cart), torch.device("cuda", device)
        assert self.n_cart <= abi.ACC_MAX_CART
        m = abi.AccModel()
        m.nv, m.n_cart = self.nv, self.n_cart
        self.cart_gains = []
        for t, term in enumerate(cart):
            m.cart_gain_type[t] = int(term.get("gain_type", ACCELERATION))
            m.cart_gain_matrices[t] = 1 if term.get("gain_matrices", False) else 0
            m.cart_orientation_gain[t] = float(term.get("orientation_gain", 1.0))
            Kp = np.asarray(term.get("Kp", np.eye(6)), dtype=float).reshape(36)
            Kd = np.asarray(term.get("Kd", np.eye(6)), dtype=float).reshape(36)
            for i in range(36):
                m.cart_Kp[36 * t + i], m.cart_Kd[36 * t + i] = float(Kp[i]), float(Kd[i])
            self.cart_gains.append(m.cart_gain_matrices[t] == 1 or m.cart_gain_type[t] == FORCE)
        self.has_com = com is not None
        if com is not None:
            m.has_com, m.com_gain_matrices = 1, 1 if com.get("gain_matrices", False) else 0
            Kp = np.asarray(com.get("Kp", np.eye(3)), dtype=float).reshape(9)
            Kd = np.asarray(com.get("Kd", np.eye(3)), dtype=float).reshape(9)
            for i in range(9):
                m.com_Kp[i], m.com_Kd[i] = float(Kp[i]), float(Kd[i])
        self.com_gains = bool(m.com_gain_matrices)
        self.has_postural = postural is not None
        self._keep = []
        if postural is not None:
            m.has_postural = 1
            m.post_gain_type = int(postural.get("gain_type", ACCELERATION))
            m.post_gain_matrices = 1 if postural.get("gain_matrices", False) else 0
            m.post_lambda, m.post_lambda2 = float(postural.get("lam", 1.0)), float(postural.get("lam2", 1.0))
            for key, field in (("Kp", "post_Kp"), ("Kd", "post_Kd")):
                K = postural.get(key)
                assert K is None or m.post_gain_matrices, "postural Kp / Kd need gain_matrices=True (osot_acc_tasks refuses them otherwise)"
                if K is not None:
                    K = K if isinstance(K, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(K, dtype=np.float64))
                    K = K.to(device=self.device, dtype=torch.float64).contiguous()
                    assert tuple(K.shape) == (self.nv, self.nv)
                    self._keep.append(K)
                    setattr(m, field, K.data_ptr())
        self._m = m


class AccTasks:
    """An AccModel bound to tensors: batch_args() builds the osot_acc_batch (the tensors must outlive its use), forward() launches
    osot_acc_tasks on torch's current stream.  Nothing allocates in forward(): it can be captured into a graph."""

    def __init__(self, model):
        self.model = model
        self._lib = abi.lib()

    def batch_args(self, B, q=None, qdot=None, M=None, cart=(), com=None, postural=None, Minv=None, ok=None):
        """cart: one dict per term: J= (tensor [B][rows][ld], first row) like frame_J of kinematics.Kinematics (a bare tensor: row 0)
        -- six rows of stack.A[k] or of IdModel.Jc --, pose=, pose_ref= [B][12], vel_ref=, f_virtual=, a_ref_in= [B][6] or None,
        p0= tensor [B][>= 12 or 84] or (tensor, first column) or None -- the leaf p0 of the task --, a_ref_out= [B][6], Mi= [B][36].
        com: dict(J= (tensor, first row), com=, com_ref=, vel_ref= [B][3], p0= tensor [B][>= 6 or 24]).
        postural: dict(q_ref=, qdot_ref=, qddot_ref= [B][nv], p0= [B][2 nv], qddot_out= [B][nv]).
        M: as Dynamics.batch_args takes it (IdModel.Bm); Minv: likewise; ok: int32 [B]."""
        mo, nv = self.model, self.model.nv
        b = abi.AccBatch()
        b.B = B

        def inp(t, shape, dtype=torch.float64):
            assert t.is_contiguous() and t.dtype == dtype and t.shape[0] >= B and tuple(t.shape[1:]) == shape, (tuple(t.shape), shape)
            return t.data_ptr()

        def rows(t, nrows):
            t, row = t if isinstance(t, tuple) else (t, 0)
            assert t.is_contiguous() and t.dim() == 3 and t.dtype == torch.float64 and t.shape[0] >= B
            assert row >= 0 and row + nrows <= t.shape[1] and t.shape[2] >= nv
            return t.data_ptr() + 8 * row * t.shape[2], t.shape[1] * t.shape[2], t.shape[2]

        def place(t, width):
            t, col = t if isinstance(t, tuple) else (t, 0)
            assert t.is_contiguous() and t.dim() == 2 and t.dtype == torch.float64 and t.shape[0] >= B and col + width <= t.shape[1]
            return t.data_ptr() + 8 * col, t.shape[1]

        def square(t):
            assert t.is_contiguous() and t.dtype == torch.float64 and t.shape[0] >= B and t[0].numel() >= nv * nv
            return t.data_ptr(), t[0].numel()
        if q is not None:
            b.q = inp(q, (nv,))
        if qdot is not None:
            b.qdot = inp(qdot, (nv,))
        if M is not None:
            b.M, b.M_stride = square(M)
        assert len(cart) == mo.n_cart
        for t, term in enumerate(cart):
            b.cart_J[t], b.cart_J_stride[t], b.cart_J_ld[t] = rows(term["J"], 6)
            b.cart_pose[t], b.cart_pose_ref[t] = inp(term["pose"], (12,)), inp(term["pose_ref"], (12,))
            for key in ("vel_ref", "f_virtual", "a_ref_in", "a_ref_out"):
                if term.get(key) is not None:
                    getattr(b, "cart_" + key)[t] = inp(term[key], (6,))
            if term.get("Mi") is not None:
                b.cart_Mi[t] = inp(term["Mi"], (36,))
            if term.get("p0") is not None:
                b.cart_p0[t], b.cart_p0_stride[t] = place(term["p0"], 84 if mo.cart_gains[t] else 12)
        if com is not None:
            b.com_J, b.com_J_stride, b.com_J_ld = rows(com["J"], 3)
            b.com, b.com_ref = inp(com["com"], (3,)), inp(com["com_ref"], (3,))
            if com.get("vel_ref") is not None:
                b.com_vel_ref = inp(com["vel_ref"], (3,))
            if com.get("p0") is not None:
                b.com_p0, b.com_p0_stride = place(com["p0"], 24 if mo.com_gains else 6)
        if postural is not None:
            b.post_q_ref = inp(postural["q_ref"], (nv,))
            for key in ("qdot_ref", "qddot_ref", "qddot_out"):
                if postural.get(key) is not None:
                    setattr(b, "post_" + key, inp(postural[key], (nv,)))
            if postural.get("p0") is not None:
                b.post_p0 = inp(postural["p0"], (2 * nv,))
        if Minv is not None:
            b.Minv, b.Minv_stride = square(Minv)
        if ok is not None:
            b.ok = inp(ok, (), torch.int32)
        return b

    def forward(self, batch):
        """osot_acc_tasks with a batch_args() result, stream-ordered on torch's current stream"""
        st = C.c_void_p(torch.cuda.current_stream(self.model.device).cuda_stream)
        abi.check(self._lib.osot_acc_tasks(C.byref(self.model._m), C.byref(batch), st), "osot_acc_tasks")
