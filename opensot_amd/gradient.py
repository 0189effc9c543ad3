"""Host side of the posture-gradient producer (include/osot_mi355x.h: osot_grad_create / osot_posture_gradient): the b of
tasks::velocity::Manipulability and tasks::velocity::MinimumEffort (Manipulability.cpp:58-84, MinimumEffort.cpp:51-77) for a batch
of postures, written in place into device tensors -- usually straight into the leaf array of the block that carries the task.
Plumbing only: the arithmetic is in csrc/osot_grad.h."""
import ctypes as C

import numpy as np
import torch

from . import abi


def posture_term(kind, frame=0, step=1e-3, lam=1.0, W=None, active=None):
    """one term of a PostureGradient.  kind: abi.GRAD_MANIPULABILITY_FRAME (frame = index of a frame of the model; its frame_base is
    honoured), abi.GRAD_MANIPULABILITY_COM or abi.GRAD_MIN_EFFORT.  step: the finite-difference step (the reference's default 1e-3);
    lam: Task::setLambda; W: the DIAGONAL of the worker's constant weight (setW), one entry per coordinate, default ones -- a dense W
    is not offered; active: the active joints (Task::setActiveJointsMask), default all: the gradient entry of any other joint is 0"""
    return dict(kind=int(kind), frame=int(frame), step=float(step), lam=float(lam), W=W, active=active)


def grad_desc(model, terms, gravity=(0.0, 0.0, -9.81)):
    """the osot_grad_desc of a list of posture_term()s for a KinModel"""
    d = abi.GradDesc()
    d.n_terms = len(terms)
    for k, t in enumerate(terms[:abi.GRAD_MAX_TERMS]):
        d.kind[k], d.frame[k], d.step[k], d.lambda_[k] = int(t["kind"]), int(t["frame"]), float(t["step"]), float(t["lam"])
        d.joint_mask[k] = 0 if t["active"] is None else sum(1 << int(j) for j in set(t["active"]))
        W = np.ones(model.n) if t["W"] is None else np.asarray(t["W"], dtype=float).reshape(model.n)
        for j in range(model.n):
            d.W_diag[k][j] = float(W[j])
    for i in range(3):
        d.gravity[i] = float(gravity[i])
    return d


class PostureGradient:
    """osot_grad handle + the binding of its outputs to device buffers.  Mirrors kinematics.Kinematics."""

    def __init__(self, model, terms, device=0, gravity=(0.0, 0.0, -9.81)):
        self.model, self.terms = model, list(terms)
        self._lib = abi.lib()
        self._h = C.c_void_p()
        kd, gd = model.desc(), grad_desc(model, self.terms, gravity)
        abi.check(self._lib.osot_grad_create(C.byref(kd), C.byref(gd), int(device), C.byref(self._h)), "osot_grad_create")
        self.device = torch.device("cuda", device)

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self._lib.osot_grad_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def batch_args(self, q, b=None, value=None):
        """the osot_grad_batch of a call (pointers and strides; the tensors must outlive its use).  q [B][n] (device);
        b: {term index: tensor [B][>= n]} or {term index: (tensor [B][w], first column)} -- e.g. the leaf array p2 of a Postural
        block or p0 of a Generic block; value: {term index: tensor [B]}, the index / the effort at q"""
        B, n = q.shape
        assert n == self.model.n and q.is_contiguous() and q.dtype == torch.float64
        gb = abi.GradBatch()
        gb.B, gb.q = B, q.data_ptr()
        for t, dst in (b or {}).items():
            dst, col = dst if isinstance(dst, tuple) else (dst, 0)
            assert 0 <= t < len(self.terms) and dst.is_contiguous() and dst.dtype == torch.float64 and dst.dim() == 2
            assert dst.shape[0] >= B and col >= 0 and col + n <= dst.shape[1]
            gb.b[t], gb.b_stride[t] = dst.data_ptr() + 8 * col, dst.shape[1]
        for t, v in (value or {}).items():
            assert 0 <= t < len(self.terms) and v.is_contiguous() and v.dtype == torch.float64 and v.numel() >= B
            gb.value[t] = v.data_ptr()
        return gb

    def forward(self, q, b=None, value=None, batch=None):
        """osot_posture_gradient, stream-ordered on torch's current stream (batch: a batch_args() result to reuse)"""
        gb = self.batch_args(q, b, value) if batch is None else batch
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        abi.check(self._lib.osot_posture_gradient(self._h, C.byref(gb), stream), "osot_posture_gradient")
