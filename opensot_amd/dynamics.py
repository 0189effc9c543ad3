"""Host side of the inverse-dynamics producers (include/osot_mi355x.h: osot_id_rows, osot_computed_torque): the model
quantities the reference asks XBot::ModelInterface for (inertia matrix, non-linear term, contact Jacobians;
DynamicFeasibility.cpp:24-36, TorqueLimits.cpp:27-40, InverseDynamics.cpp:67-77) as device tensors, and the ctypes plumbing
that points the producer at the row ranges of a BatchedStack's A_k / C buffers.  Plumbing only: the arithmetic is in
csrc/osot_id.h."""
import ctypes as C

import numpy as np
import torch

from . import abi


def _t(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(device)


class Dynamics:
    """osot_dyn handle (include/osot_mi355x.h: osot_dyn_create / osot_dynamics): inertia matrix, non-linear term, Jdot qdot of the
    model's frames and of the centre of mass for a batch of postures, written in place into device tensors.  Mirrors
    kinematics.Kinematics; the arithmetic is in csrc/osot_dyn.h."""

    def __init__(self, model, device=0, gravity=(0.0, 0.0, -9.81)):
        self.model = model
        self._lib = abi.lib()
        self._h = C.c_void_p()
        kd, dd = model.desc(), abi.DynDesc()
        I = np.zeros((model.n, 6)) if getattr(model, "inertia", None) is None else np.asarray(model.inertia, dtype=float).reshape(model.n, 6)
        for j in range(model.n):
            for i in range(6):
                dd.inertia[j][i] = float(I[j, i])
        for i in range(3):
            dd.gravity[i] = float(gravity[i])
        abi.check(self._lib.osot_dyn_create(C.byref(kd), C.byref(dd), int(device), C.byref(self._h)), "osot_dyn_create")
        self.device = torch.device("cuda", device)

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self._lib.osot_dyn_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def batch_args(self, q, qdot=None, M=None, h=None, frame_jdotqdot=None, com_jdotqdot=None, cmm_lin=None, cmm_ang=None,
                   momentum=None, ang_mom_b=None):
        """the osot_dyn_batch of a call (pointers and strides; the tensors must outlive its use).  q, qdot [B][n] (device, qdot
        may be None); M: a tensor whose leading dimension is the batch and whose instances start with the n x n matrix (IdModel.Bm,
        or anything wider: the stride is its row length); h [B][n]; frame_jdotqdot: {frame index: tensor [B][6]} or
        {frame index: (tensor [B][w], first column)} -- e.g. a task's leaf array p1; com_jdotqdot: tensor [B][>= 3] or (tensor, column).
        Centroidal momentum: cmm_lin / cmm_ang: (tensor [B][rows][ld], first row) like frame_J of kinematics.Kinematics (a bare
        tensor: row 0) -- the 3 linear / angular rows of the momentum matrix, n doubles of each row, e.g. a Generic block's rows of
        stack.A[k]; momentum: tensor [B][>= 6] or (tensor, column), [linear; angular]; ang_mom_b: dict(out= tensor [B][>= 3] or
        (tensor, column), ref= L_d [B][3] or None, rate_ref= Ldot_d [B][3] or None, K= 3 x 3 (host) or None for the identity,
        lam=) -- the b of acceleration::AngularMomentum, Ldot_d + lam K (L_d - L)"""
        B, n = q.shape
        assert n == self.model.n and q.is_contiguous() and q.dtype == torch.float64
        b = abi.DynBatch()
        b.B, b.q = B, q.data_ptr()
        if qdot is not None:
            assert qdot.shape == q.shape and qdot.is_contiguous() and qdot.dtype == torch.float64
            b.qdot = qdot.data_ptr()
        if M is not None:
            assert M.is_contiguous() and M.shape[0] >= B and M[0].numel() >= n * n
            b.M, b.M_stride = M.data_ptr(), M[0].numel()
        if h is not None:
            assert h.is_contiguous() and h.shape[0] >= B and h.shape[1] == n
            b.h = h.data_ptr()

        def place(t, width):
            t, col = t if isinstance(t, tuple) else (t, 0)
            assert t.is_contiguous() and t.dim() == 2 and t.shape[0] >= B and col + width <= t.shape[1]
            return t.data_ptr() + 8 * col, t.shape[1]
        for f, t in (frame_jdotqdot or {}).items():
            b.frame_Jdot_qdot[f], b.frame_Jdot_qdot_stride[f] = place(t, 6)
        if com_jdotqdot is not None:
            b.com_Jdot_qdot, b.com_Jdot_qdot_stride = place(com_jdotqdot, 3)

        def rows(t):
            t, row = t if isinstance(t, tuple) else (t, 0)
            assert t.is_contiguous() and t.dim() == 3 and t.dtype == torch.float64 and t.shape[0] >= B
            assert row >= 0 and row + 3 <= t.shape[1] and t.shape[2] >= n
            return t.data_ptr() + 8 * row * t.shape[2], t.shape[1] * t.shape[2], t.shape[2]
        if cmm_lin is not None:
            b.cmm_lin, b.cmm_lin_stride, b.cmm_lin_ld = rows(cmm_lin)
        if cmm_ang is not None:
            b.cmm_ang, b.cmm_ang_stride, b.cmm_ang_ld = rows(cmm_ang)
        if momentum is not None:
            b.momentum, b.momentum_stride = place(momentum, 6)
        if ang_mom_b is not None:
            b.ang_mom_b, b.ang_mom_b_stride = place(ang_mom_b["out"], 3)
            for key, field in (("ref", "ang_mom_ref"), ("rate_ref", "ang_mom_rate_ref")):
                r = ang_mom_b.get(key)
                if r is not None:
                    assert r.is_contiguous() and r.dtype == torch.float64 and r.shape == (B, 3)
                    setattr(b, field, r.data_ptr())
            K = ang_mom_b.get("K")
            if K is not None:
                K = np.asarray(K, dtype=float).reshape(9)
                for i in range(9):
                    b.ang_mom_gain[i] = float(K[i])
            b.ang_mom_lambda = float(ang_mom_b.get("lam", 1.0))
        return b

    def forward(self, q, qdot=None, M=None, h=None, frame_jdotqdot=None, com_jdotqdot=None, cmm_lin=None, cmm_ang=None,
                momentum=None, ang_mom_b=None, batch=None):
        """osot_dynamics, stream-ordered on torch's current stream (batch: a batch_args() result to reuse)"""
        b = batch if batch is not None else self.batch_args(q, qdot, M, h, frame_jdotqdot, com_jdotqdot, cmm_lin, cmm_ang, momentum, ang_mom_b)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        abi.check(self._lib.osot_dynamics(self._h, C.byref(b), stream), "osot_dynamics")


class IdModel:
    """B [B][nv][nv], h [B][nv], Jc [B][contacts][3 or 6][nv]; x = [qddot; forces] (InverseDynamics.cpp:12-28)"""

    @classmethod
    def empty(cls, B, nv, n_contacts, contact_dim=6, device=0, floating_base=True):
        """a model on zeroed device tensors that the producers fill IN PLACE every cycle: Bm and h by Dynamics.forward(M=model.Bm,
        h=model.h), Jc by Kinematics.forward(frame_J={frame: model.contact_rows(c)}) -- IdModel keeps the tensors it is given when
        they already are float64 on its device, so write_rows / computed_torque read what the producers wrote"""
        dev = torch.device("cuda", device)
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        return cls(z(B, nv, nv), z(B, nv), z(B, n_contacts, contact_dim, nv), device=device, floating_base=floating_base)

    def contact_rows(self, c):
        """(tensor [B][n_contacts * contact_dim][nv], first row) of contact c: the frame_J binding of kinematics.Kinematics"""
        assert self.cdim == 6, "the kinematics producer writes the six rows of a frame's Jacobian"
        return self.Jc.view(self.B, self.n_contacts * self.cdim, self.nv), c * self.cdim

    def __init__(self, Bm, h, Jc, device=0, floating_base=True):
        self.device = torch.device("cuda", device)
        self.Bm, self.h, self.Jc = _t(Bm, self.device), _t(h, self.device), _t(Jc, self.device)
        self.B, self.nv = self.Bm.shape[0], self.Bm.shape[1]
        self.n_contacts, self.cdim = self.Jc.shape[1], self.Jc.shape[2]
        self.n = self.nv + self.n_contacts * self.cdim
        self.floating_base = floating_base
        self._lib = abi.lib()

    def _c(self):
        m = abi.IdModel()
        m.B, m.nv, m.n_contacts, m.contact_dim = self.B, self.nv, self.n_contacts, self.cdim
        m.Bm, m.h, m.Jc = self.Bm.data_ptr(), self.h.data_ptr(), self.Jc.data_ptr()
        m.floating_base = 1 if self.floating_base else 0
        return m

    def write_rows(self, stack, dyn_block=None, tau_block=None, tasks=()):
        """dyn_block / tau_block: indices of the plan's DYN_FEASIBILITY / TORQUE_LIMITS row blocks; tasks: (level, first row,
        J [B][rows][nv]) -- the [J 0] task matrices.  Everything lands in stack.C / stack.A[level] in place."""
        plan, n = stack.plan, stack.plan.n
        assert n == self.n
        cs = plan.nc_stored * n
        pd = lambda j: None if j is None else C.c_void_p(stack.C.data_ptr() + 8 * plan.rows_stored_offset(j) * n)
        nt = len(tasks)
        vp = C.c_void_p
        Jp = (vp * max(nt, 1))(); Jr = (C.c_int * max(nt, 1))(); Ad = (vp * max(nt, 1))(); As = (C.c_longlong * max(nt, 1))()
        keep = []
        for i, (k, row0, J) in enumerate(tasks):
            J = _t(J, self.device); keep.append(J)
            Jp[i], Jr[i] = J.data_ptr(), J.shape[1]
            Ad[i] = stack.A[k].data_ptr() + 8 * row0 * n
            As[i] = plan.ma(k) * n
        m = self._c()
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        abi.check(self._lib.osot_id_rows(C.byref(m), pd(dyn_block), cs, pd(tau_block), cs, nt, Jp, Jr, Ad, As, st), "osot_id_rows")

    def computed_torque(self, x, fb_tol=10e-3):
        """InverseDynamics::computedTorque: (tau [B][nv], ok [B]) for the solved x [B][n]; ok = 0 where a floating-base row
        of tau exceeds fb_tol (the reference's 10e-3, InverseDynamics.cpp:87)"""
        B = x.shape[0]
        x = x.contiguous()
        tau = torch.empty((B, self.nv), dtype=torch.float64, device=self.device)
        ok = torch.empty((B,), dtype=torch.int32, device=self.device)
        m = self._c(); m.B = B
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        abi.check(self._lib.osot_computed_torque(C.byref(m), C.c_void_p(x.data_ptr()), C.c_void_p(tau.data_ptr()),
                                                 C.c_void_p(ok.data_ptr()), fb_tol, st), "osot_computed_torque")
        return tau, ok


class IdStep:
    """One device-resident inverse-dynamics control step of a stack made by synth.make_coman_id_stack:
        q, qdot -> osot_kinematics + osot_dynamics -> leaf errors -> osot_id_rows -> osot_cycle -> osot_computed_torque -> integrate
    produce() runs the two producer launches; consume() everything behind them, reading ONLY the tensors the producers fill
    (model.Bm / h / Jc, Jcom, com, jdq, com_jdq) -- so a caller may fill those from another source instead (the tests upload
    host-computed quantities).  Every launch goes to torch's current stream; nothing allocates after the constructor, so step()
    can be captured into a graph."""

    def __init__(self, plan, leaf, kin_model, device=0, dt=1.0e-3, gravity=(0.0, 0.0, -9.81)):
        from .kinematics import Kinematics
        from .solver import BatchedStack
        B, nv = leaf["B"], leaf["nv"]
        self.B, self.nv, self.dt, self.plan = B, nv, dt, plan
        self.st = BatchedStack(plan, B, device=device)
        self.dev = self.st.load_leaf(leaf)
        d = self.st.device
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(d)
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=d)
        self.q, self.qdot, self.q_ref = t(leaf["state"]["q0"]), t(leaf["state"]["qdot0"]), t(leaf["state"]["q_ref"])
        self.kin, self.dyn = Kinematics(kin_model, device), Dynamics(kin_model, device, gravity)
        self.frames = [kin_model.frame_index(c) for c in leaf["contacts"]]
        self.model = IdModel.empty(B, nv, len(self.frames), 6, device=device)
        self.Jcom, self.com, self.com_ref = z(B, 3, nv), z(B, 3), None
        # the leaves the producers write straight into: Jdot qdot of the contact tasks and of the CoM task (p1), h of the torque limits (p0)
        (self.p0_l, self.jdq_l, _), (self.p0_r, self.jdq_r, _), (self.p0_com, self.jdq_com, _) = self.dev["task"][0]
        self.p0_post = self.dev["task"][-1][0][0]                 # (the Postural block is the last level's)
        self.h_u = self.dev["rows"][0][0]
        self.dev["rows"][3] = (self.model.h, self.dev["rows"][3][1], None)
        self.J12 = self.model.Jc.view(B, 12, nv)
        self.tau, self.ok = z(B, nv), torch.zeros((B,), dtype=torch.int32, device=d)
        self._mc = self.model._c()
        self._lib = abi.lib()

    def produce(self):
        self.kin.forward(self.q, frame_J={f: self.model.contact_rows(c) for c, f in enumerate(self.frames)}, com=self.com,
                         com_J=(self.Jcom, 0))
        self.dyn.forward(self.q, self.qdot, M=self.model.Bm, h=self.model.h,
                         frame_jdotqdot={self.frames[0]: self.jdq_l, self.frames[1]: self.jdq_r}, com_jdotqdot=self.jdq_com)

    def consume(self):
        nv, dt = self.nv, self.dt
        if self.com_ref is None:
            self.com_ref = self.com.clone()
        # leaf errors (what the tasks' _update() computes): CoM and postural; the contact tasks ask for zero acceleration
        self.p0_com[:, :3] = self.com_ref - self.com
        self.p0_com[:, 3:] = -(self.Jcom * self.qdot[:, None, :]).sum(dim=2)
        self.p0_post[:, :nv] = self.q_ref - self.q
        self.p0_post[:, nv:] = -self.qdot
        self.h_u.copy_(self.model.h[:, :6])
        self.model.write_rows(self.st, dyn_block=0, tau_block=3, tasks=[(0, 0, self.J12), (0, 12, self.Jcom)])
        self.st.cycle(self.dev)
        x = self.st.dq[:self.B]
        stream = C.c_void_p(torch.cuda.current_stream(self.st.device).cuda_stream)
        abi.check(self._lib.osot_computed_torque(C.byref(self._mc), C.c_void_p(x.data_ptr()), C.c_void_p(self.tau.data_ptr()),
                                                 C.c_void_p(self.ok.data_ptr()), 10e-3, stream), "osot_computed_torque")

    def integrate(self):
        qdd = self.st.dq[:self.B, :self.nv]
        self.q.add_(self.qdot, alpha=self.dt).add_(qdd, alpha=0.5 * self.dt * self.dt)
        self.qdot.add_(qdd, alpha=self.dt)

    def step(self, producers=True):
        if producers:
            self.produce()
        self.consume()
        self.integrate()


class IdMomentumStep(IdStep):
    """IdStep for a stack made by synth.make_coman_id_momentum_stack: the same osot_dynamics launch also writes the rows [A_ang 0] of
    the acceleration::AngularMomentum block straight into stack.A[level] (row length n = the plan's, the force columns stay zero) and its
    b = Ldot_d + lambda K (L_d - L) into the block's leaf p0; consume() neither computes nor copies them.  The centroidal momentum of
    every step lands in self.momentum [B][6].  L_ref / Ldot_ref [B][3] are the caller's (zero here; the reference's task zeroes its own
    after every update).  On a leaf without state["momentum"] (synth.make_coman_id_stack) only self.momentum is added."""

    def __init__(self, plan, leaf, kin_model, device=0, dt=1.0e-3, gravity=(0.0, 0.0, -9.81)):
        super().__init__(plan, leaf, kin_model, device, dt, gravity)
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.st.device)
        self.momentum, self.L_ref, self.Ldot_ref = z(self.B, 6), z(self.B, 3), z(self.B, 3)
        self._extra = dict(momentum=self.momentum)
        m = leaf["state"].get("momentum")
        if m is not None:
            self._extra.update(cmm_ang=(self.st.A[m["level"]], m["row"]),
                               ang_mom_b=dict(out=self.dev["task"][m["level"]][0][0], ref=self.L_ref, rate_ref=self.Ldot_ref, K=m["K"], lam=m["lam"]))

    def produce(self):
        self.kin.forward(self.q, frame_J={f: self.model.contact_rows(c) for c, f in enumerate(self.frames)}, com=self.com,
                         com_J=(self.Jcom, 0))
        self.dyn.forward(self.q, self.qdot, M=self.model.Bm, h=self.model.h,
                         frame_jdotqdot={self.frames[0]: self.jdq_l, self.frames[1]: self.jdq_r}, com_jdotqdot=self.jdq_com, **self._extra)


class IdTrackingStep(IdStep):
    """IdStep for a stack made by synth.make_coman_id_tracking_stack:
        q, qdot -> osot_kinematics + osot_dynamics -> osot_acc_tasks -> osot_id_rows -> osot_cycle -> osot_computed_torque -> integrate
    consume() calls osot_acc_tasks (acceleration.AccTasks) in place of IdStep's torch expressions: the CoM errors, the hand's pose and
    velocity errors with their gain matrices (GainType::Force: Mi Kp, Mi Kd and a_ref + Mi f from a Cholesky factor of model.Bm; no
    inverse inertia matrix is asked of the host), the postural errors and qddot_d.  The hand's reference pose starts at
    `offset` from its first pose and moves with vel_ref (hand_ref, hand_vel_ref: the caller's to rewrite)."""

    def __init__(self, plan, leaf, kin_model, device=0, dt=1.0e-3, gravity=(0.0, 0.0, -9.81)):
        from .acceleration import AccModel, AccTasks
        super().__init__(plan, leaf, kin_model, device, dt, gravity)
        B, nv, d = self.B, self.nv, self.st.device
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(d)
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=d)
        tr = leaf["state"]["tracking"]
        self.hand = kin_model.frame_index(tr["hand"])
        self.p0_hand, self.jdq_hand, self.a_ref_hand = self.dev["task"][1][0]
        self.qddot_d = self.dev["task"][2][0][2]
        self.Jhand, self.hand_pose, self.hand_ref, self.hand_vel_ref = z(B, 6, nv), z(B, 12), z(B, 12), t(tr["vel_ref"])
        self._offset = t(tr["offset"])
        self.f_virtual = t(tr["f_virtual"]) if tr["f_virtual"] is not None else None
        self.com_ref = z(B, 3)
        self._refs_set = False
        self.acc_ok = torch.zeros((B,), dtype=torch.int32, device=d)
        am = AccModel(nv, cart=[dict(gain_type=tr["gain_type"], gain_matrices=True, Kp=tr["Kp"], Kd=tr["Kd"], orientation_gain=tr["orientation_gain"])],
                      com=dict(gain_matrices=False),
                      postural=dict(gain_type=tr["gain_type"], gain_matrices=True, lam=tr["post_lam"], lam2=tr["post_lam2"], Kp=tr["post_Kp"], Kd=tr["post_Kd"]),
                      device=device)
        self.acc = AccTasks(am)
        # what the step binds (acc_args: for a caller who wants the same batch with more outputs, e.g. Minv=)
        self.acc_args = dict(
            q=self.q, qdot=self.qdot, M=self.model.Bm,
            cart=[dict(J=self.Jhand, pose=self.hand_pose, pose_ref=self.hand_ref, vel_ref=self.hand_vel_ref, f_virtual=self.f_virtual,
                       p0=self.p0_hand, a_ref_out=self.a_ref_hand)],
            com=dict(J=self.Jcom, com=self.com, com_ref=self.com_ref, p0=self.p0_com),
            postural=dict(q_ref=self.q_ref, p0=self.p0_post, qddot_out=self.qddot_d), ok=self.acc_ok)
        self._ab = self.acc.batch_args(B, **self.acc_args)

    def produce(self):
        frames = {f: self.model.contact_rows(c) for c, f in enumerate(self.frames)}
        frames[self.hand] = (self.Jhand, 0)
        self.kin.forward(self.q, frame_pose={self.hand: self.hand_pose}, frame_J=frames, com=self.com, com_J=(self.Jcom, 0))
        self.dyn.forward(self.q, self.qdot, M=self.model.Bm, h=self.model.h,
                         frame_jdotqdot={self.frames[0]: self.jdq_l, self.frames[1]: self.jdq_r, self.hand: self.jdq_hand},
                         com_jdotqdot=self.jdq_com)

    def consume(self):
        if not self._refs_set:                          # the first CoM and the hand's first pose (host-side flag: set before a capture)
            self.com_ref.copy_(self.com)
            self.hand_ref.copy_(self.hand_pose)
            self.hand_ref[:, 9:12].add_(self._offset)
            self._refs_set = True
        self.acc.forward(self._ab)
        self.solve()

    def solve(self):
        """everything behind the leaves: reads only what the producers and osot_acc_tasks wrote (a caller may fill the leaves
        p0_com, p0_hand, a_ref_hand, p0_post, qddot_d from another source instead).  Apart from the hand's rows in write_rows this
        is the tail of IdStep.consume, restated here because IdStep keeps its consume() in one piece: a change to either goes
        to both."""
        self.h_u.copy_(self.model.h[:, :6])
        self.model.write_rows(self.st, dyn_block=0, tau_block=3, tasks=[(0, 0, self.J12), (0, 12, self.Jcom), (1, 0, self.Jhand)])
        self.st.cycle(self.dev)
        x = self.st.dq[:self.B]
        stream = C.c_void_p(torch.cuda.current_stream(self.st.device).cuda_stream)
        abi.check(self._lib.osot_computed_torque(C.byref(self._mc), C.c_void_p(x.data_ptr()), C.c_void_p(self.tau.data_ptr()),
                                                 C.c_void_p(self.ok.data_ptr()), 10e-3, stream), "osot_computed_torque")

    def integrate(self):
        super().integrate()
        self.hand_ref[:, 9:12].add_(self.hand_vel_ref[:, :3], alpha=self.dt)     # the reference moves with its twist


def force_gains(J, Bi, Kp, Kd, p0, rows, f_virtual=None, a_ref=None):
    """GainType::Force of acceleration::Cartesian (src/tasks/acceleration/Cartesian.cpp:161-169): Mi = J Bi J' per instance
    (compute_cartesian_inertia_inverse, :517-524), Gp = Mi Kp and Gd = Mi Kd written into the task's leaf array
    p0 [B][2 rows + 2 rows^2] behind the errors (Task.acc_gain_matrices), a_ref [B][rows] += Mi f_virtual.
    J [B][rows][nv], Bi [B][nv][nv] device tensors; Kp, Kd rows x rows (host)."""
    B, r, nv = J.shape
    assert r == rows and p0.shape == (B, 2 * rows + 2 * rows * rows) and p0.is_contiguous() and J.is_contiguous() and Bi.is_contiguous()
    Kp = np.ascontiguousarray(Kp, dtype=np.float64).reshape(rows * rows)
    Kd = np.ascontiguousarray(Kd, dtype=np.float64).reshape(rows * rows)
    vp = C.c_void_p
    st = vp(torch.cuda.current_stream(J.device).cuda_stream)
    abi.check(abi.lib().osot_id_force_gains(B, nv, rows, vp(J.data_ptr()), vp(Bi.data_ptr()), Kp.ctypes.data_as(abi.dp),
                                            Kd.ctypes.data_as(abi.dp), vp(f_virtual.data_ptr()) if f_virtual is not None else None,
                                            vp(p0.data_ptr() + 8 * 2 * rows), 2 * rows + 2 * rows * rows,
                                            vp(a_ref.data_ptr()) if a_ref is not None else None, st), "osot_id_force_gains")


class ForceModel:
    """osot_force_model (include/osot_mi355x.h: osot_force_rows): the layout of x = [w_0 .. w_{C-1} (6 each) | optionally tau (nv - 6)]
    and the settings of the force tasks.  wrench_col: first column of every wrench (default 0, 6, ...); torque_col: first of the
    nv - 6 torque columns or -1; com_gains = (lambda, lambda2, lambda_ang) of force::CoM; cart_contact, Kp, Kd (6 x 6, host) of
    force::Cartesian.  Plumbing only: the arithmetic is in csrc/osot_force.h."""

    def __init__(self, n_contacts, nv, n, wrench_col=None, torque_col=-1, mass=1.0, gravity=(0.0, 0.0, -9.81), com_gains=(1.0, 1.0, 1.0),
                 cart_contact=0, Kp=None, Kd=None):
        self.n_contacts, self.nv, self.n, self.torque_col = int(n_contacts), int(nv), int(n), int(torque_col)
        self.wrench_col = [6 * c for c in range(self.n_contacts)] if wrench_col is None else [int(w) for w in wrench_col]
        assert len(self.wrench_col) == self.n_contacts <= abi.FORCE_MAX_CONTACTS
        m = abi.ForceModel()
        m.n_contacts, m.nv, m.n, m.torque_col, m.cart_contact, m.mass = self.n_contacts, self.nv, self.n, self.torque_col, int(cart_contact), float(mass)
        for c, w in enumerate(self.wrench_col):
            m.wrench_col[c] = w
        for i in range(3):
            m.gravity[i] = float(gravity[i])
        m.com_lambda, m.com_lambda2, m.com_lambda_ang = (float(g) for g in com_gains)
        Kp = np.eye(6) if Kp is None else np.asarray(Kp, dtype=float).reshape(6, 6)
        Kd = np.eye(6) if Kd is None else np.asarray(Kd, dtype=float).reshape(6, 6)
        for i in range(36):
            m.cart_Kp[i], m.cart_Kd[i] = float(Kp.reshape(36)[i]), float(Kd.reshape(36)[i])
        self._m = m
        self._lib = abi.lib()

    def batch_args(self, B, Jc=None, pose=None, com=None, momentum=None, h_gravity=None, qdot=None, enabled=None,
                   com_A=None, com_b=None, com_refs=None, fb_A=None, static_A=None, static_lo=None, static_up=None, static_q_tau=None,
                   cart_b=None, cart_refs=None):
        """the osot_force_batch of a call (pointers and strides; the tensors must outlive its use).  Inputs: Jc [B][C][6][nv], pose: a
        list of C tensors [B][12], com [B][3], momentum [B][6], h_gravity [B][nv], qdot [B][nv], enabled int32 [B][C].
        com_A / fb_A / static_A: (tensor [B][rows][ld], first row) like cmm_ang of Dynamics.batch_args (a bare tensor: row 0) -- a Generic
        block's rows of stack.A[k], or the leaf p0 of an OSOT_ROWS_GENERIC block.  com_b / cart_b / static_lo / static_up: tensor
        [B][>= width] or (tensor, first column), e.g. the leaf p0 of an OSOT_TASK_GENERIC block, p1 / p2 of an OSOT_ROWS_GENERIC block.
        com_refs: dict(pos=, vel=, acc=, ang_mom=, ang_mom_rate=) of [B][3] tensors; cart_refs: dict(pose= [B][12], vel= [B][6],
        f_des= [B][6], pose_error= [B][6])."""
        C_, nv, n, na = self.n_contacts, self.nv, self.n, self.nv - 6
        b = abi.ForceBatch()
        b.B = B

        def inp(t, shape, dtype=torch.float64):
            assert t.is_contiguous() and t.dtype == dtype and t.shape[0] >= B and tuple(t.shape[1:]) == shape, (tuple(t.shape), shape)
            return t.data_ptr()

        def rows(t, nrows):
            t, row = t if isinstance(t, tuple) else (t, 0)
            assert t.is_contiguous() and t.dim() == 3 and t.dtype == torch.float64 and t.shape[0] >= B
            assert row >= 0 and row + nrows <= t.shape[1] and t.shape[2] >= n
            return t.data_ptr() + 8 * row * t.shape[2], t.shape[1] * t.shape[2], t.shape[2]

        def place(t, width):
            t, col = t if isinstance(t, tuple) else (t, 0)
            assert t.is_contiguous() and t.dim() == 2 and t.dtype == torch.float64 and t.shape[0] >= B and col + width <= t.shape[1]
            return t.data_ptr() + 8 * col, t.shape[1]
        for c, p in enumerate(pose or ()):
            b.pose[c] = inp(p, (12,))
        for name, t, shape in (("Jc", Jc, (C_, 6, nv)), ("com", com, (3,)), ("momentum", momentum, (6,)), ("h_gravity", h_gravity, (nv,)),
                               ("qdot", qdot, (nv,)), ("static_q_tau", static_q_tau, (na,))):
            if t is not None:
                setattr(b, name, inp(t, shape))
        if enabled is not None:
            b.enabled = inp(enabled, (C_,), torch.int32)
        if com_A is not None:
            b.com_A, b.com_A_stride, b.com_A_ld = rows(com_A, 6)
        if fb_A is not None:
            b.fb_A, b.fb_A_stride, b.fb_A_ld = rows(fb_A, 6)
        if static_A is not None:
            b.static_A, b.static_A_stride, b.static_A_ld = rows(static_A, na)
        if static_lo is not None:
            (b.static_lo, b.static_b_stride), (b.static_up, s2) = place(static_lo, na), place(static_up, na)
            assert s2 == b.static_b_stride
        if com_b is not None:
            b.com_b, b.com_b_stride = place(com_b, 6)
        for key, field in (("pos", "com_pos_ref"), ("vel", "com_vel_ref"), ("acc", "com_acc_ref"), ("ang_mom", "ang_mom_ref"),
                           ("ang_mom_rate", "ang_mom_rate_ref")):
            if (com_refs or {}).get(key) is not None:
                setattr(b, field, inp(com_refs[key], (3,)))
        if cart_b is not None:
            b.cart_b, b.cart_b_stride = place(cart_b, 6)
        for key, field, w in (("pose", "cart_pose_ref", 12), ("vel", "cart_vel_ref", 6), ("f_des", "cart_f_des", 6), ("pose_error", "cart_pose_error", 6)):
            if (cart_refs or {}).get(key) is not None:
                setattr(b, field, inp(cart_refs[key], (w,)))
        return b

    def write_rows(self, batch, device=None):
        """osot_force_rows, stream-ordered on torch's current stream"""
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        abi.check(self._lib.osot_force_rows(C.byref(self._m), C.byref(batch), st), "osot_force_rows")


def wrench_selection(n, wrench_cols):
    """the constant A of force::Wrench / Wrenches and of force::Cartesian (Force.cpp:5-26, 51-87): the selection of the listed
    wrenches' six columns, [6 len(wrench_cols)][n] -- written once into an OSOT_TASK_GENERIC block, its b is the reference"""
    A = np.zeros((6 * len(wrench_cols), n))
    for i, w in enumerate(wrench_cols):
        A[6 * i:6 * i + 6, w:w + 6] = np.eye(6)
    return A


class ForceStep:
    """One device-resident wrench-distribution cycle of a stack made by synth.make_coman_force_stack / make_wide_force_stack:
        q, qdot -> osot_kinematics + osot_dynamics (momentum) + osot_dynamics (qdot = NULL: the gravity term) -> osot_force_rows -> osot_cycle
    produce() runs the three producer launches; consume() everything behind them, reading ONLY the tensors the producers fill
    (pose, Jc, com, momentum, h_gravity) -- so a caller may fill those from another source instead (kin_model=None: the stack
    carries no tree; leaf["force"]["quantities"] is uploaded once).  The rows land in the OSOT_TASK_GENERIC / OSOT_ROWS_GENERIC blocks
    leaf["force"] names: force::CoM or force::FloatingBase at level 0 of stack.A, the StaticConstraint rows in its block's leaf
    (C, lo, up).  force::FloatingBase's b, the caller's floating_base_torque, is the floating-base part of the gravity term.
    enabled [B][C] int32 and com_refs (zero tensors: p_d = the first CoM after the first produce()) are the caller's to rewrite.
    Every launch goes to torch's current stream; nothing allocates after the constructor, so step() can be captured into a graph."""

    def __init__(self, plan, leaf, kin_model=None, device=0, gravity=(0.0, 0.0, -9.81)):
        from .solver import BatchedStack
        f = leaf["force"]
        B, nv, C_ = leaf["B"], f["nv"], len(f["wrench_col"])
        self.B, self.nv, self.plan, self.form = B, nv, plan, f["form"]
        self.st = BatchedStack(plan, B, device=device)
        self.dev = self.st.load_leaf(leaf)
        d = self.st.device
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(d)
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=d)
        self.pose = [z(B, 12) for _ in range(C_)]
        self.Jc, self.com, self.momentum, self.h_gravity = z(B, C_, 6, nv), z(B, 3), z(B, 6), z(B, nv)
        self.enabled = torch.ones((B, C_), dtype=torch.int32, device=d)
        self.kin = self.dyn = None
        if kin_model is not None:
            from .kinematics import Kinematics
            self.q, self.qdot = t(leaf["state"]["q0"]), t(leaf["state"]["qdot0"])
            self.kin, self.dyn = Kinematics(kin_model, device), Dynamics(kin_model, device, gravity)
            frames = [kin_model.frame_index(c) for c in f["contacts"]]
            J = self.Jc.view(B, 6 * C_, nv)
            self._kb = self.kin.batch_args(self.q, frame_pose={fr: self.pose[c] for c, fr in enumerate(frames)},
                                           frame_J={fr: (J, 6 * c) for c, fr in enumerate(frames)}, com=self.com)
            self._db_mom = self.dyn.batch_args(self.q, self.qdot, momentum=self.momentum)
            self._db_grav = self.dyn.batch_args(self.q, None, h=self.h_gravity)
        else:
            Q = f["quantities"]
            for c in range(C_):
                self.pose[c].copy_(t(Q["pose"][c]))
            self.Jc.copy_(t(Q["Jc"])); self.com.copy_(t(Q["com"])); self.momentum.copy_(t(Q["momentum"])); self.h_gravity.copy_(t(Q["h_gravity"]))
        self.model = ForceModel(C_, nv, plan.n, f["wrench_col"], f["torque_col"], mass=f["mass"], gravity=gravity, com_gains=f["com_gains"])
        self.com_refs = dict(pos=z(B, 3), vel=z(B, 3), acc=t(f["com_acc_ref"]) if f.get("com_acc_ref") is not None else z(B, 3),
                             ang_mom=z(B, 3), ang_mom_rate=z(B, 3))
        self._com_ref_set = False
        kw = dict(Jc=self.Jc, pose=self.pose, com=self.com, momentum=self.momentum, h_gravity=self.h_gravity, enabled=self.enabled)
        lvl, row = f["task"]
        self.b0 = self.dev["task"][lvl][f["task_index"]][0]            # leaf p0 of the level's force block: its b
        if self.form == "com":
            kw.update(com_A=(self.st.A[lvl], row), com_b=self.b0, com_refs=self.com_refs)
        else:
            kw.update(fb_A=(self.st.A[lvl], row))
        if f.get("static_block") is not None:
            Cs, lo, up = self.dev["rows"][f["static_block"]]
            kw.update(static_A=Cs, static_lo=lo, static_up=up)
        self._fb = self.model.batch_args(B, **kw)

    def produce(self):
        self.kin.forward(self.q, batch=self._kb)
        self.dyn.forward(self.q, batch=self._db_mom)
        self.dyn.forward(self.q, batch=self._db_grav)

    def consume(self):
        if not self._com_ref_set:                       # p_d: the first CoM (host-side flag: set before a capture)
            self.com_refs["pos"].copy_(self.com)
            self._com_ref_set = True
        if self.form != "com":
            self.b0.copy_(self.h_gravity[:, :6])        # floating_base_torque: a plain leaf
        self.model.write_rows(self._fb, self.st.device)
        self.st.cycle(self.dev)

    def step(self, producers=True):
        if producers and self.kin is not None:
            self.produce()
        self.consume()
