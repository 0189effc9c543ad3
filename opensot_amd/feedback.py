"""The tasks driven by measurements on the device (include/osot_mi355x.h: osot_feedback; csrc/osot_feedback.h): the desired twist of
velocity::CartesianAdmittance, the desired velocity of velocity::JointAdmittance, the rows of floating_base::IMU, the lambda * err
term of floating_base::Contact and the rows of tasks::velocity::CollisionAvoidance, written into the leaves of existing kinds.

    model = FeedbackModel(nv, floating_base=True)
    model.add_cartesian_admittance(**FeedbackModel.cartesian_admittance_defaults())     # -> term index
    model.set_joint_admittance(**FeedbackModel.joint_admittance_defaults())
    fbk = Feedback(model, B, device=0)          # owns the filter state [B][count]
    fbk.step(cart=[dict(pose=, wrench=, twist_out=)], joint=dict(tau=, h=, qdot_out=), ...)     # one launch on torch's stream

Plumbing only: the arithmetic is in csrc/osot_feedback.h."""
import ctypes as C
import math

import numpy as np
import torch

from . import abi


def admittance_params(K, D, lam, dt):
    """osot_admittance_params: CartesianAdmittance::computeParameters -> (C, M, w); raises where D[i] <= K[i] dt / lambda"""
    K, D = np.ascontiguousarray(K, dtype=np.float64).reshape(6), np.ascontiguousarray(D, dtype=np.float64).reshape(6)
    Cc, M, w = np.zeros(6), np.zeros(6), np.zeros(6)
    p = lambda a: a.ctypes.data_as(abi.dp)
    abi.check(abi.lib().osot_admittance_params(p(K), p(D), float(lam), float(dt), p(Cc), p(M), p(w)), "osot_admittance_params")
    return Cc, M, w


class FeedbackModel:
    """osot_feedback_model: sizes, the constants of every admittance term, the contact gain, the collision threshold."""

    def __init__(self, nv, floating_base=True, imu=False, contact_lambda=0.0, n_pairs=0, n=None, ca_threshold=0.0):
        m = abi.FeedbackModel()
        m.nv, m.floating_base, m.imu, m.n_pairs, m.n = int(nv), int(bool(floating_base)), int(bool(imu)), int(n_pairs), int(nv if n is None else n)
        m.contact_lambda, m.ca_threshold = float(contact_lambda), float(ca_threshold)
        self._m = m
        self.cart = []          # per term: dict(K, D, lam, dt) as the reference's getters would report them

    nv = property(lambda self: self._m.nv)
    n_cart = property(lambda self: self._m.n_cart)
    n_pairs = property(lambda self: self._m.n_pairs)
    n = property(lambda self: self._m.n)

    # -- the reference's defaults ------------------------------------------------------------------------------------------------
    @classmethod
    def cartesian_admittance_defaults(cls):
        """the constructor of CartesianAdmittance (CartesianAdmittance.cpp:30-44): dt = 0.002, lambda = 0.01, K = (1e4 x 3, 1e5 x 3),
        D = 1.1 K dt / lambda, C from computeParameters, filter damping 1 -- and the filter KEEPS ITS OWN omega = 1 and ts = 0.01
        (SecondOrderFilter's constructor): the constructor computes w but never hands it to the filter.  set_impedance_params /
        set_raw_params do, as setImpedanceParams / setRawParams."""
        dt, lam = 0.002, 0.01
        K = np.array([1e4, 1e4, 1e4, 1e5, 1e5, 1e5])
        D = 1.1 * K * dt / lam
        Cc, M, w = admittance_params(K, D, lam, dt)
        return dict(C=Cc, omega=np.ones(6), damping=np.ones(6), ts=0.01, deadzone=np.zeros(6), lam=lam)

    @classmethod
    def joint_admittance_defaults(cls):
        """the constructor of JointAdmittance (JointAdmittance.cpp:5-26); lam is the Postural task's lambda"""
        return dict(C=0.00015, ts=0.002, damping=1.0, omega=2.0 * math.pi * 8.0, lam=0.005)

    # -- terms -------------------------------------------------------------------------------------------------------------------
    def add_cartesian_admittance(self, C, omega, damping, ts, deadzone=None, lam=None):
        """-> the index of the new term; lam (the Cartesian task's lambda) is kept for the caller, the kernel does not read it"""
        t = self._m.n_cart
        assert t < abi.FEEDBACK_MAX_CART
        self._m.n_cart = t + 1
        self.cart.append(dict(lam=lam))
        self._fill(t, C=C, omega=omega, damping=damping, deadzone=np.zeros(6) if deadzone is None else deadzone)
        self._m.cart_ts[t] = float(ts)
        return t

    def _fill(self, t, **kw):
        for name, v in kw.items():
            v = np.broadcast_to(np.asarray(v, dtype=np.float64), (6,))
            for c in range(6):
                getattr(self._m, "cart_" + name)[6 * t + c] = float(v[c])

    def set_impedance_params(self, t, K, D, lam, dt):
        """setImpedanceParams (CartesianAdmittance.cpp:203-244): C and the filters' omega from computeParameters.  The filters' time
        step stays what it was, as in the reference (only setRawParams hands dt to the filter).  -> lam, the task's lambda"""
        K, D = np.asarray(K, dtype=np.float64), np.asarray(D, dtype=np.float64)
        if (D <= 0.0).any() or (K <= 0.0).any() or dt <= 0.0:
            raise ValueError("K, D and dt must be positive")
        Cc, M, w = admittance_params(K, D, lam, dt)
        self._fill(t, C=Cc, omega=w)
        self.cart[t].update(lam=lam, K=K, D=D, M=M, dt=dt)
        return lam

    def set_raw_params(self, t, C, omega, lam, dt):
        """setRawParams (CartesianAdmittance.cpp:246-295): C, the filters' omega and time step; lam must be 0, as there"""
        if lam != 0:
            raise ValueError("TBD lambda > 0")
        C, omega = np.asarray(C, dtype=np.float64), np.asarray(omega, dtype=np.float64)
        if (C < 0.0).any() or (omega < 0.0).any() or dt < 0.0:
            return False
        self._fill(t, C=C, omega=omega)
        self._m.cart_ts[t] = float(dt)
        self.cart[t].update(lam=lam, dt=dt)
        return True

    def set_dead_zone(self, t, amplitude):
        if (np.asarray(amplitude) < 0.0).any():
            return False
        self._fill(t, deadzone=amplitude)
        return True

    def set_joint_admittance(self, C=0.00015, ts=0.002, damping=1.0, omega=2.0 * math.pi * 8.0, lam=None):
        """the joint filter and the scalar compliance (a dense matrix is bound per call: Feedback.step(joint=dict(C=...)))"""
        m = self._m
        m.joint, m.joint_C_scalar, m.joint_ts, m.joint_damping, m.joint_omega = 1, float(C), float(ts), float(damping), float(omega)

    def state_doubles(self):
        n = C.c_int()
        abi.check(abi.lib().osot_feedback_state_doubles(C.byref(self._m), C.byref(n)), "osot_feedback_state_doubles")
        return n.value


class Feedback:
    """A FeedbackModel for B instances on a device: owns the filter state, binds tensors, launches osot_feedback on torch's current
    stream.  Nothing allocates after bind(), so launch() can be captured into a graph."""

    def __init__(self, model, B, device=0):
        self.model, self.B = model, int(B)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.count = model.state_doubles()
        self.state = torch.zeros((self.B, self.count), dtype=torch.float64, device=self.device) if self.count else None
        self._batch = None
        self._keep = None

    def reset(self, value=None):
        """zero the state (a fresh filter), or u = ud = y = yd = value: the reference's reset(initial_state).  value: a scalar, or
        per channel [6 n_cart (+ nv)] or [B][6 n_cart (+ nv)], the Cartesian terms first"""
        if self.state is None:
            return
        if value is None:
            self.state.zero_()
            return
        m = self.model
        ch = self.count // 4
        v = torch.as_tensor(value, dtype=torch.float64, device=self.device).expand(self.B, ch) if np.ndim(value) else \
            torch.full((self.B, ch), float(value), dtype=torch.float64, device=self.device)
        for t in range(m.n_cart):
            self.state[:, 24 * t:24 * t + 24] = v[:, 6 * t:6 * t + 6].repeat(1, 4)
        if m._m.joint:
            self.state[:, 24 * m.n_cart:] = v[:, 6 * m.n_cart:].repeat(1, 4)

    def bind(self, cart=None, joint=None, imu=None, contact=None, ca=None):
        """the osot_feedback_batch of the calls to come (the tensors are kept alive here).
        cart: a list, entry t = None or dict(pose= [B][12], wrench= [B][6], twist_out= [B][6], wrench_ref= [B][6], twist_in= [B][6]);
        joint: dict(tau= [B][nv], h= [B][nv], qdot_out= [B][nv], C= [nv][nv] or absent);
        imu: dict(fb_J= tensor [B][rows][nv] or (tensor, first row), pose= [B][12], omega= [B][3], A= tensor [B][rows][ld] or (tensor,
              first row), b= tensor [B][>= 6] or (tensor, first column));
        contact: dict(pose=, pose_ref= [B][12], b_in=, b_out= tensor [B][>= 6] or (tensor, first column));
        ca: dict(J= tensor [B][rows][n] or (tensor, first row), dist= [B][n_pairs], A= like J with ld >= n, b= like imu's b)."""
        m, B = self.model, self.B
        nv, P, n = m.nv, m.n_pairs, m.n
        b = abi.FeedbackBatch()
        b.B = B
        if self.state is not None:
            b.state = self.state.data_ptr()

        def inp(t, shape):
            assert t.is_contiguous() and t.dtype == torch.float64 and t.shape[0] >= B and tuple(t.shape[1:]) == shape, (tuple(t.shape), shape)
            return t.data_ptr()

        def rows(t, nrows, width):
            t, row = t if isinstance(t, tuple) else (t, 0)
            assert t.is_contiguous() and t.dim() == 3 and t.dtype == torch.float64 and t.shape[0] >= B
            assert row >= 0 and row + nrows <= t.shape[1] and t.shape[2] >= width
            return t.data_ptr() + 8 * row * t.shape[2], t.shape[1] * t.shape[2], t.shape[2]

        def place(t, width):
            t, col = t if isinstance(t, tuple) else (t, 0)
            assert t.is_contiguous() and t.dim() == 2 and t.dtype == torch.float64 and t.shape[0] >= B and col + width <= t.shape[1]
            return t.data_ptr() + 8 * col, t.shape[1]
        for t, term in enumerate(cart or ()):
            if term is None:
                continue
            b.cart_pose[t], b.cart_wrench[t], b.cart_twist_out[t] = inp(term["pose"], (12,)), inp(term["wrench"], (6,)), inp(term["twist_out"], (6,))
            if term.get("wrench_ref") is not None:
                b.cart_wrench_ref[t] = inp(term["wrench_ref"], (6,))
            if term.get("twist_in") is not None:
                b.cart_twist_in[t] = inp(term["twist_in"], (6,))
        if joint is not None:
            b.joint_tau, b.joint_h, b.joint_qdot_out = inp(joint["tau"], (nv,)), inp(joint["h"], (nv,)), inp(joint["qdot_out"], (nv,))
            if joint.get("C") is not None:
                Cm = joint["C"]
                assert Cm.is_contiguous() and Cm.dtype == torch.float64 and tuple(Cm.shape) == (nv, nv)
                b.joint_C = Cm.data_ptr()
        if imu is not None:
            if imu.get("A") is not None:
                b.imu_fb_J, b.imu_fb_J_stride, ldj = rows(imu["fb_J"], 6, nv)
                assert ldj == nv, "the rows of fb_J have length nv"
                b.imu_A, b.imu_A_stride, b.imu_A_ld = rows(imu["A"], 6, 6)
            if imu.get("b") is not None:
                b.imu_pose, b.imu_omega = inp(imu["pose"], (12,)), inp(imu["omega"], (3,))
                b.imu_b, b.imu_b_stride = place(imu["b"], 6)
        if contact is not None:
            b.contact_pose, b.contact_pose_ref = inp(contact["pose"], (12,)), inp(contact["pose_ref"], (12,))
            b.contact_b_in, b.contact_b_in_stride = place(contact["b_in"], 6)
            b.contact_b_out, b.contact_b_out_stride = place(contact["b_out"], 6)
        if ca is not None:
            b.ca_dist = inp(ca["dist"], (P,))
            if ca.get("A") is not None:
                b.ca_J, b.ca_J_stride, ldj = rows(ca["J"], P, n)
                assert ldj == n, "the rows of J have length n"
                b.ca_A, b.ca_A_stride, b.ca_A_ld = rows(ca["A"], P, n)
            if ca.get("b") is not None:
                b.ca_b, b.ca_b_stride = place(ca["b"], P)
        self._batch, self._keep = b, (cart, joint, imu, contact, ca)
        return b

    def launch(self, batch=None):
        """osot_feedback with the bound batch, stream-ordered on torch's current stream"""
        batch = self._batch if batch is None else batch
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        abi.check(abi.lib().osot_feedback(C.byref(self.model._m), C.byref(batch), st), "osot_feedback")

    def step(self, **groups):
        """bind (where groups are given) and launch"""
        if groups or self._batch is None:
            self.bind(**groups)
        self.launch()
