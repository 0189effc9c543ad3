"""torch.Tensor in / out entry points: what `pyopensot` gives a Python planner in the reference
(bindings/python/solver.hpp:26-31: `solve(solver) -> VectorXd`; :67-91: iHQP(stack, eps_regularisation, be_solver), solve,
getNumberOfTasks, setActiveStack, activateAllStacks, getBackEndName, setEpsRegularisation; :93-...: nHQP), for B instances
at once on CUDA/HIP tensors: the device pointers of the caller's tensors go STRAIGHT to the C-ABI (include/osot_mi355x.h),
results come back as tensors on the same device and stream -- no host copies, no staging.

    qp_solve(H, g, A, lA, uA, l, u, ...)   B generic QPs in BackEnd convention through either back-end
    qp_multipliers(..., x)                 their multipliers and active sets (QPOasesBackEnd::getDualSolution / getActiveBounds)
    qp_layer(H, g, A, lA, uA, l, u)        the active-set solve as a differentiable layer (n <= 64; up to 128 with
                                           workspace = qp_sens_workspace(B, n, nc), as qp_multipliers)
    ihqp_layer(stack, b, w, lo, up, ...)   the cascade of a BatchedStack as a differentiable layer over its assembled inputs (n <= 64)
    iHQP / nHQP                            the cascade front-ends on a BatchedStack, `solve()` returning dq as a tensor;
                                           iHQP.getObjective(i) / getDualSolution(i) / getActiveSet(i) / getSensitivityFlag(i) / getLevelQP(i) after a solve
"""
import ctypes as C
import enum

import torch

from . import abi
from .plan import StackPlan, eps_abs_from_factor
from .solver import BatchedStack


class solver_back_ends(enum.Enum):
    """OpenSoT::solvers::solver_back_ends (bindings/python/solver.hpp:34-43): the two this build implements"""
    qpOASES = 0     # -> the wavefront dual active-set kernel (qpOASES conventions: eps = 1e3 * 2.221e-16 * factor)
    OSQP = 1        # -> the OSQP-convention ADMM kernel (eps = 2.22e-13 * factor)


def _chk(t, name, shape=None, dtype=torch.float64):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a tensor on the GPU")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (its device pointer is handed to the kernel as it is)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return C.c_void_p(t.data_ptr())


def admm_state(B, n, nc, box=True, device=0):
    """the warm-start state of the OSQP-convention back-end for B instances (what OSQPBackEnd's osqp workspace carries from
    one control cycle to the next, OSQPBackEnd.cpp:120-143): x, y, rho; rho = 0 means "no state yet" """
    dev = torch.device("cuda", device) if isinstance(device, int) else device
    return {"x": torch.zeros((B, n), dtype=torch.float64, device=dev),
            "y": torch.zeros((B, nc + (n if box else 0)), dtype=torch.float64, device=dev),
            "rho": torch.zeros((B,), dtype=torch.float64, device=dev)}


def qp_hot_state(B, n, device=0):
    """the hot-start state of the active-set back-end for B QPs of n variables (osot_qp_solve_batch_hot): int32 [B][ints], every
    entry -1 = "nothing recorded" (a cold start).  Row i is instance i's inequality working set as its last solve left it, in codes
    that belong to this library and to ONE shape (n, nc): take a fresh state (or fill_(-1)) when the shape changes."""
    ints = C.c_int(0)
    abi.check(abi.lib().osot_qp_hot_state_ints(int(n), C.byref(ints)), "osot_qp_hot_state_ints")
    dev = torch.device("cuda", device) if isinstance(device, int) else device
    return torch.full((B, ints.value), -1, dtype=torch.int32, device=dev)


def qp_solve(H, g, A=None, lA=None, uA=None, l=None, u=None, eps_regularisation=2e2, be_solver=solver_back_ends.qpOASES,
             max_iter=0, warm=None, scaling=0, hot=None):
    """B QPs  min 1/2 x'Hx + g'x  s.t.  lA <= A x <= uA,  l <= x <= u  (BackEnd.h:125-150).
    H [B][n][n], g [B][n], A [B][nc][n], lA / uA [B][nc], l / u [B][n] (A.. and l, u optional), float64, on one GPU.
    eps_regularisation is the back-end factory's FACTOR (BackEndFactory.cpp:4-17).
    OSQP back-end only: warm = admm_state(...) carried from call to call (warm start), scaling = Ruiz passes (0 = osqp's 10,
    negative = none).
    Active-set back-end only: hot = qp_hot_state(B, n) carried from call to call (hot start: every solve begins from the working set
    the instance's previous solve ended with, as QPOasesBackEnd::solve does; the answer is the cold one up to round-off).
    Returns (x [B][n], status [B] int32 OSOT_STATUS_*, iterations [B] int32), stream-ordered on the current stream."""
    lib = abi.lib()
    if H.dim() != 3 or H.shape[1] != H.shape[2]:
        raise ValueError("H must be [B][n][n]")
    B, n = H.shape[0], H.shape[1]
    nc = 0 if A is None else A.shape[1]
    dev = H.device
    pH, pg = _chk(H, "H"), _chk(g, "g", (B, n))
    pA, plA, puA = _chk(A, "A", (B, nc, n)), _chk(lA, "lA", (B, nc)), _chk(uA, "uA", (B, nc))
    pl, pu = _chk(l, "l", (B, n)), _chk(u, "u", (B, n))
    x = torch.empty((B, n), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    iters = torch.empty((B,), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if be_solver == solver_back_ends.OSQP:
            if hot is not None:
                raise ValueError("hot is the active-set back-end's state; the OSQP back-end's warm start is warm = admm_state(...)")
            opt = abi.AdmmOptions()
            opt.max_iter = max_iter
            opt.scaling = scaling
            m = nc + (n if l is not None else 0)
            wx = wy = wr = None
            if warm is not None:
                wx, wy, wr = _chk(warm["x"], "warm x", (B, n)), _chk(warm["y"], "warm y", (B, m)), _chk(warm["rho"], "warm rho", (B,))
            abi.check(lib.osot_qp_solve_batch_admm_warm(B, n, nc, pH, pg, pA, plA, puA, pl, pu, 2.22e-13 * eps_regularisation,
                                                        C.byref(opt), wx, wy, wr,
                                                        C.c_void_p(x.data_ptr()), C.c_void_p(status.data_ptr()),
                                                        C.c_void_p(iters.data_ptr()), stream), "osot_qp_solve_batch_admm_warm")
        else:
            if warm is not None:
                raise ValueError("warm is the OSQP back-end's state; the active-set back-end's hot start is hot = qp_hot_state(...)")
            if hot is not None:
                if not isinstance(hot, torch.Tensor) or hot.device != dev:
                    raise TypeError(f"hot must be a tensor on {dev}, where the problem is")
                ints = C.c_int(0)
                abi.check(lib.osot_qp_hot_state_ints(n, C.byref(ints)), "osot_qp_hot_state_ints")
                ph = _chk(hot, "hot", (B, ints.value), dtype=torch.int32)
                abi.check(lib.osot_qp_solve_batch_hot(B, n, nc, pH, pg, pA, plA, puA, pl, pu, eps_abs_from_factor(eps_regularisation),
                                                      max_iter, C.c_void_p(x.data_ptr()), C.c_void_p(status.data_ptr()),
                                                      C.c_void_p(iters.data_ptr()), ph, stream), "osot_qp_solve_batch_hot")
                return x, status, iters
            abi.check(lib.osot_qp_solve_batch(B, n, nc, pH, pg, pA, plA, puA, pl, pu, eps_abs_from_factor(eps_regularisation), max_iter,
                                              C.c_void_p(x.data_ptr()), C.c_void_p(status.data_ptr()),
                                              C.c_void_p(iters.data_ptr()), stream), "osot_qp_solve_batch")
    return x, status, iters


def _sens_batch(H, g, A, lA, uA, l, u, x, status, eps_regularisation):
    """abi.QpSensBatch with the inputs bound (outputs are the caller's to bind) -> (batch, B, n, nc)"""
    if H.dim() != 3 or H.shape[1] != H.shape[2]:
        raise ValueError("H must be [B][n][n]")
    B, n = H.shape[0], H.shape[1]
    nc = 0 if A is None else A.shape[1]
    b = abi.QpSensBatch()
    b.B, b.n, b.nc, b.eps_abs = B, n, nc, eps_abs_from_factor(eps_regularisation)
    b.H, b.g = _chk(H, "H"), _chk(g, "g", (B, n))
    if nc:
        b.A, b.lA, b.uA = _chk(A, "A", (B, nc, n)), _chk(lA, "lA", (B, nc)), _chk(uA, "uA", (B, nc))
    b.l, b.u = _chk(l, "l", (B, n)), _chk(u, "u", (B, n))
    b.x = _chk(x, "x", (B, n))
    b.status = _chk(status, "status", (B,), dtype=torch.int32)
    return b, B, n, nc


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _sens_options(options):
    if options is None:
        return None
    o = abi.QpSensOptions()
    o.active_tol, o.dual_tol, o.rank_tol = (float(options.get(k, 0.0)) for k in ("active_tol", "dual_tol", "rank_tol"))
    return C.byref(o)


def qp_sens_workspace(B, n, nc, device=None):
    """the workspace qp_multipliers(..., workspace=) and qp_layer(..., workspace=) need for B QPs of n variables and nc rows
    (osot_qp_sens_workspace_bytes): a uint8 tensor on the GPU, empty for n <= 64.  It is sized by the workgroups in flight, not by
    B, and serves one call at a time."""
    nbytes = C.c_size_t(0)
    abi.check(abi.lib().osot_qp_sens_workspace_bytes(int(B), int(n), int(nc), C.byref(nbytes)), "osot_qp_sens_workspace_bytes")
    if device is None:
        device = torch.cuda.current_device()
    dev = torch.device("cuda", device) if isinstance(device, int) else device
    return torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)


def _sens_call(b, options, workspace, dev):
    """osot_qp_sensitivity_batch, or with a workspace osot_qp_sensitivity_batch_ws, on the current stream of dev"""
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if workspace is None:
            try:
                abi.check(abi.lib().osot_qp_sensitivity_batch(C.byref(b), options, stream), "osot_qp_sensitivity_batch")
            except RuntimeError as e:
                if 64 < b.n <= 128:
                    raise RuntimeError(f"{e}; with workspace=qp_sens_workspace(B, n, nc) the call takes up to 128 variables") from None
                raise
            return
        if not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise TypeError(f"workspace must be a contiguous uint8 tensor on {dev} (qp_sens_workspace(B, n, nc) makes it)")
        abi.check(abi.lib().osot_qp_sensitivity_batch_ws(C.byref(b), options, _ptr(workspace), workspace.numel(), stream),
                  "osot_qp_sensitivity_batch_ws")


def qp_multipliers(H, g, A, lA, uA, l, u, x, status=None, eps_regularisation=2e2, options=None, workspace=None):
    """The multipliers and the active set of B QPs at their solutions x [B][n] (qp_solve's, or anybody's): what QPOasesBackEnd keeps as
    getDualSolution (nV + nC entries, the bounds first; QPOasesBackEnd.cpp:153-158) and getActiveBounds / getActiveConstraints.
    status [B] int32 (qp_solve's) or None = all solved.  options: dict with active_tol, dual_tol, rank_tol (0 or absent = 1e-8, 1e-9,
    1e-11).  n <= 64; with workspace = qp_sens_workspace(B, n, nc) n goes up to 128 (without it 65 .. 128 variables are refused:
    RuntimeError).
    Returns (y [B][n + nc] float64 in qpOASES' convention: H~ x + g = y_b + A' y_c, y > 0 on a lower side, y < 0 on an upper side;
    active [B][n + nc] int32: 0, -1 lower, +1 upper, 2 equality; flag [B] int32 OSOT_SENS_*: 0 unique, 1 degenerate (a valid one-sided
    answer), 2 skipped (not solved, x not finite or H + eps I not positive definite: zeros)), stream-ordered on the current stream."""
    b, B, n, nc = _sens_batch(H, g, A, lA, uA, l, u, x, status, eps_regularisation)
    dev = H.device
    y = torch.empty((B, n + nc), dtype=torch.float64, device=dev)
    active = torch.empty((B, n + nc), dtype=torch.int32, device=dev)
    flag = torch.empty((B,), dtype=torch.int32, device=dev)
    b.y, b.active, b.flag = _ptr(y), _ptr(active), _ptr(flag)
    _sens_call(b, _sens_options(options), workspace, dev)
    return y, active, flag


class _QpLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, g, A, lA, uA, l, u, eps_regularisation, max_iter, hot, last, workspace):
        x, status, iters = qp_solve(H, g, A, lA, uA, l, u, eps_regularisation=eps_regularisation, max_iter=max_iter, hot=hot)
        last.status, last.iterations = status, iters
        last.flag = torch.full((H.shape[0],), -1, dtype=torch.int32, device=H.device)      # filled by the backward pass
        ctx.save_for_backward(*[t for t in (H, g, A, lA, uA, l, u, x, status) if t is not None])
        ctx.present = [t is not None for t in (H, g, A, lA, uA, l, u)]
        ctx.eps, ctx.last, ctx.workspace = eps_regularisation, last, workspace
        return x

    @staticmethod
    def backward(ctx, grad_x):
        saved = list(ctx.saved_tensors)
        H, g, A, lA, uA, l, u = (saved.pop(0) if p else None for p in ctx.present)
        x, status = saved
        b, B, n, nc = _sens_batch(H, g, A, lA, uA, l, u, x, status, ctx.eps)
        gx = grad_x.contiguous()
        b.grad_x, b.flag = _ptr(gx), _ptr(ctx.last.flag)
        grads = []
        for k, (name, t) in enumerate(zip(("grad_H", "grad_g", "grad_A", "grad_lA", "grad_uA", "grad_l", "grad_u"), (H, g, A, lA, uA, l, u))):
            out = None
            if t is not None and ctx.needs_input_grad[k]:      # NULL for every input that does not need a gradient
                out = torch.empty_like(t)
                setattr(b, name, _ptr(out))
            grads.append(out)
        ctx.last.bound = [name for name, o in zip(("H", "g", "A", "lA", "uA", "l", "u"), grads) if o is not None]
        _sens_call(b, None, ctx.workspace, H.device)
        return (*grads, None, None, None, None, None)


class _QpLayerLast:
    """what the last qp_layer call left: status, iterations [B] int32 of the solve; flag [B] int32 OSOT_SENS_* of the backward pass (-1 until
    it has run); bound: the inputs whose gradient outputs the backward pass handed to the kernel"""
    status = iterations = flag = None
    bound = ()


def qp_layer(H, g, A=None, lA=None, uA=None, l=None, u=None, eps_regularisation=2e2, max_iter=0, hot=None, workspace=None):
    """qp_solve through the active-set back-end as a differentiable layer: x [B][n] carries autograd's graph to H, g, A, lA, uA, l, u
    (those that require a gradient).  The backward pass is one launch of osot_qp_sensitivity_batch: the active set at x, its
    multipliers and one more solve of the same KKT system with the upstream gradient on the right-hand side; grad_H is symmetric
    (the derivative with respect to a symmetric H), an equality's gradient goes to its lower bound.  An instance that was not solved
    (status != 0) or that the backward pass skipped contributes a zero gradient; at a degenerate solution (flag 1) the gradient is a
    valid one-sided one.  `qp_layer.last` holds status, iterations and flag of the most recent call.
    n <= 64 without a workspace (ValueError above; the solve alone goes to 128 through qp_solve); with workspace =
    qp_sens_workspace(B, n, nc), which the backward pass hands to osot_qp_sensitivity_batch_ws, n goes up to 128.  The
    OSQP-convention back-end is not offered as a layer: its solutions stop at 1e-5, too far from a vertex to read the active set from."""
    if H.dim() == 3 and H.shape[1] > 64 and workspace is None:
        raise ValueError("qp_layer: more than 64 variables (without a workspace the backward pass is built for n <= 64; pass "
                         "workspace=qp_sens_workspace(B, n, nc) for up to 128; qp_solve alone takes up to 128)")
    last = _QpLayerLast()
    qp_layer.last = last
    return _QpLayer.apply(H, g, A, lA, uA, l, u, eps_regularisation, max_iter, hot, last, workspace)


qp_layer.last = _QpLayerLast()


class _IhqpLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stack, last, where, *tensors):
        B = tensors[0].shape[0]
        for (name, k), t in zip(where, tensors):
            dst = getattr(stack, name)
            (dst if k is None else dst[k])[:B].copy_(t)
        stack.solve(B)
        last.status = stack.status[:B].clone()
        last.flag = None                                   # filled by the backward pass
        ctx.stack, ctx.last, ctx.where, ctx.B = stack, last, where, B
        return stack.dq[:B].clone()

    @staticmethod
    def backward(ctx, grad_dq):
        need = ctx.needs_input_grad[3:]
        want_A = any(n and name in ("A", "C") for n, (name, _) in zip(need, ctx.where))
        g = ctx.stack.backward(ctx.B, grad_dq.contiguous(), want_A=want_A)
        ctx.last.flag = g["flag"]
        grads = [((g[name] if k is None else g[name][k]) if n else None) for n, (name, k) in zip(need, ctx.where)]
        return (None, None, None, *grads)


class _IhqpLayerLast:
    """what the last ihqp_layer call left: status [B] int32 of the solve; flag: list of [B] int32 OSOT_SENS_* per level of the
    backward pass (None until it has run)"""
    status = flag = None


def ihqp_layer(stack, b, w=None, lo=None, up=None, l=None, u=None, A=None, C=None):
    """The cascade of a BatchedStack (the wavefront route, or the wide route with 65 .. 128 variables) as a differentiable layer over its ASSEMBLED inputs: b, w, A are lists with one
    tensor per level ([B][m_k], [B][m_k], [B][ma_k][n]; an entry, or the whole argument, may be None: the stack's buffer is used as it
    is), lo, up [B][nc], l, u [B][n], C [B][nc_stored][n].  The tensors are copied into the stack's buffers, the stack is solved, and dq
    [B][n] comes back carrying autograd's graph to those of them that require a gradient.  The backward pass is
    BatchedStack.backward on the stack's buffers and x_levels AS THEY ARE THEN: run it before the stack is solved again.  An instance
    that was not solved contributes a zero gradient; at a degenerate level the gradient is a valid one-sided one.  `ihqp_layer.last`
    holds status and the levels' flags of the most recent call.  Raises before solving on a wide stack with n <= 64 (such a plan
    belongs on the wavefront route) and on a plan with a dense-weight level or a regularisation task (the backward pass is not built
    for them)."""
    plan = stack.plan
    if stack.route != "wavefront" and plan.n <= abi.MAX_VARS:
        raise ValueError("ihqp_layer: the backward pass is built for the wavefront route (n <= 64), not for a wide stack")
    if plan.regularisation is not None or any(plan.dense_level(k) for k in range(plan.L)):
        raise ValueError("ihqp_layer: the backward pass is not built for plans with a dense-weight level or a regularisation task")
    where, tensors = [], []
    for name, v in (("b", b), ("w", w), ("A", A)):
        for k, t in enumerate(v or []):
            if t is not None:
                where.append((name, k)); tensors.append(t)
    for name, t in (("lo", lo), ("up", up), ("l", l), ("u", u), ("C", C)):
        if t is not None:
            where.append((name, None)); tensors.append(t)
    if not tensors:
        raise ValueError("ihqp_layer: no input tensor")
    B = tensors[0].shape[0]
    for (name, k), t in zip(where, tensors):
        dst = getattr(stack, name)
        dst = dst if k is None else dst[k]
        if dst is None:
            raise ValueError(f"ihqp_layer: the stack has no buffer {name}" + ("" if k is None else f"[{k}]"))
        _chk(t, name, (B,) + tuple(dst.shape[1:]))
    last = _IhqpLayerLast()
    ihqp_layer.last = last
    return _IhqpLayer.apply(stack, last, tuple(where), *tensors)


ihqp_layer.last = _IhqpLayerLast()


class iHQP:
    """pyopensot.iHQP for B instances of one stack (bindings/python/solver.hpp:67-91).  The stack's per-cycle inputs are the
    BatchedStack's device tensors (`self.stack.A[k]`, leaf dictionaries of tensors: the caller's producers write into them);
    `solve()` runs update + cascade in one launch and returns dq [B][n] on the device."""

    def __init__(self, plan: StackPlan, max_batch: int, eps_regularisation: float = 2e2,
                 be_solver: solver_back_ends = solver_back_ends.qpOASES, device: int = 0):
        if be_solver != solver_back_ends.qpOASES:
            raise RuntimeError("Back-end is not available!")     # BackEndFactory.cpp:87 (the cascade kernel embeds the active-set solver)
        plan.eps_abs = eps_abs_from_factor(eps_regularisation)
        self.stack = BatchedStack(plan, max_batch, device=device)
        self._active = [True] * plan.L

    def solve(self, dev_leaf=None, B=None):
        """dev_leaf: the cycle's leaf tensors (BatchedStack.load_leaf layout): update + solve.  None: solve the assembled
        arrays as they are.  Returns dq [B][n] (a view of the solver's output tensor)."""
        self.stack.level_active = None if all(self._active) else list(self._active)
        if dev_leaf is not None:
            B = self.stack.cycle(dev_leaf)
        else:
            B = self.stack.max_batch if B is None else B
            self.stack.solve(B)
        self._solved, self._sens = B, None
        return self.stack.dq[:B]

    def status(self, B=None):
        return self.stack.status[:(self.stack.max_batch if B is None else B)]

    def _level_results(self, i):
        """multipliers, working sets and objectives of every level of the last solve(): computed on the first question after it"""
        if getattr(self, "_solved", None) is None:
            raise RuntimeError("no solve() yet")
        if not 0 <= i < self.stack.plan.L:
            raise IndexError(f"level {i} of {self.stack.plan.L}")
        if self._sens is None:
            self._sens = self.stack.multipliers(self._solved)
        return self._sens

    def getObjective(self, i):
        """iHQP::getObjective(i, val) (iHQP.cpp:381-389) of the last solve(): [B] tensor, the back-end's getObjVal() of level i"""
        return self._level_results(i)["objective"][:, i]

    def getDualSolution(self, i):
        """the dual solution of level i's back-end (QPOasesBackEnd::getDualSolution): y [B][n + rows_i], qpOASES' sign, the bounds first"""
        return self._level_results(i)["y"][i]

    def getSensitivityFlag(self, i):
        """[B] int32 OSOT_SENS_* of level i: 0 = the multipliers are unique, 1 = degenerate (a valid answer), 2 = skipped (zeros).  No
        counterpart in the reference, whose back-end reports whatever its working set holds"""
        return self._level_results(i)["flag"][i]

    def getActiveSet(self, i):
        """the working set of level i's back-end (getActiveBounds / getActiveConstraints): [B][n + rows_i] int32, the bounds first"""
        return self._level_results(i)["active"][i]

    def getLevelQP(self, i):
        """iHQP::getBackEnd(i)'s problem data: dict H (without eps), g, A, lA, uA, l, u of the last solve()"""
        if getattr(self, "_solved", None) is None:
            raise RuntimeError("no solve() yet")
        return self.stack.level_qp(i, self._solved)

    def getNumberOfTasks(self):
        return self.stack.plan.L

    def setActiveStack(self, stack_index, flag):
        self._active[stack_index] = bool(flag)

    def activateAllStacks(self):
        self._active = [True] * self.stack.plan.L

    def getBackEndName(self):
        return "MI355X dual active set (qpOASES conventions)"

    def setEpsRegularisation(self, eps, stack_index=None):
        raise RuntimeError("eps is part of the static plan of a BatchedStack: construct the solver with it")


class nHQP(iHQP):
    """pyopensot.nHQP (bindings/python/solver.hpp: nHQP(stack, bounds, eps, be_solver), setMinSingularValueRatio,
    setPerformAbRegularization, setPerformSelectiveNullSpaceRegularization)"""

    def __init__(self, plan, max_batch, eps_regularisation=2e2, be_solver=solver_back_ends.qpOASES, device=0, free_vars=None):
        super().__init__(plan, max_batch, eps_regularisation, be_solver, device)
        self._opts = dict(free_vars=free_vars, min_sv_ratio=0.05, ab_regularization=True, selective_ns_regularization=True)

    def setMinSingularValueRatio(self, sv_min):
        if not 0.0 <= sv_min <= 1.0:
            raise ValueError("[nHQP::TaskData::set_min_sv_ratio] Minimum singular value threshold should respect 0 < s < 1")
        self._opts["min_sv_ratio"] = float(sv_min)

    def setPerformAbRegularization(self, flag):
        self._opts["ab_regularization"] = bool(flag)

    def setPerformSelectiveNullSpaceRegularization(self, flag):
        self._opts["selective_ns_regularization"] = bool(flag)

    def solve(self, dev_leaf=None, B=None):
        if dev_leaf is not None:
            B = self.stack.update(dev_leaf)
        else:
            B = self.stack.max_batch if B is None else B
        self.stack.solve_nhqp(B, **self._opts)
        return self.stack.dq[:B]


class eHQP(iHQP):
    """pyopensot.eHQP (bindings/python/solver.hpp:56-61: eHQP(stack), getSigmaMin, setSigmaMin): the equality-only front-end,
    damped pseudo-inverses and projectors (src/solvers/eHQP.cpp); the stack's constraints and bounds are not used"""

    def __init__(self, plan, max_batch, device=0):
        super().__init__(plan, max_batch, device=device)
        self._sigma_min = 1e-12          # eHQP.cpp:56

    def getSigmaMin(self):
        return self._sigma_min

    def setSigmaMin(self, sigma_min):
        if sigma_min > 0:                # eHQP.cpp:156-166: non-positive values are ignored
            self._sigma_min = float(sigma_min)

    def solve(self, dev_leaf=None, B=None):
        if dev_leaf is not None:
            B = self.stack.update(dev_leaf)
        else:
            B = self.stack.max_batch if B is None else B
        self.stack.solve_ehqp(B, self._sigma_min)
        return self.stack.dq[:B]

