"""tests/gradient_cases.py -- TEST INFRASTRUCTURE ONLY: the shapes, terms, inputs and cached references that the posture-gradient
tests share (tests/test_posture_gradient_host.py without a GPU, tests/test_posture_gradient_gpu.py on one), and the call of the
kernel source through the host lock-step emulation (tests/emu/grad_host.cpp)."""
import ctypes as C
import functools
import os

import numpy as np

from opensot_amd import abi
from opensot_amd import kinematics as kin
from opensot_amd.gradient import grad_desc

import gradient_ref as gref
import native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAVITY = (0.0, 0.0, -9.81)
COND_CAP = 1e4
# 10 x the larger of the two worst deviations from the long-double arbiter, in units of the cancellation scale max(|f+|, |f-|) / (2 step)
# (measured on the committed seeds: tests/test_posture_gradient_host.py, module docstring); the issue caps it at 1e-10
PARITY_TOL = 1.7e-12
assert PARITY_TOL <= 1e-10


# ---- the four shapes ------------------------------------------------------------------------------------------------------------
def chain_model(n, link, seed):
    """a fixed-base serial chain of n revolute joints: axes cycle through skewed directions, links of length `link`, one tip frame"""
    rng = np.random.default_rng(seed)
    base = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.6, 0.0, 0.8], [0.0, 0.8, 0.6]])
    ax = np.array([base[j % len(base)] for j in range(n)])
    p0 = np.array([[link * (0.4 if j % 2 else 0.1), link * (0.1 if j % 3 else -0.3), link] for j in range(n)])
    p0[0] = 0.0
    m = kin.KinModel(parent=[j - 1 for j in range(n)], jtype=[abi.JOINT_REVOLUTE] * n, axis=ax,
                     R0=np.array([kin._rpy(*rng.uniform(-0.4, 0.4, 3)) for _ in range(n)]), p0=p0,
                     mass=rng.uniform(0.3, 1.5, n), com=rng.uniform(-0.05, 0.05, (n, 3)), names=[f"j{j}" for j in range(n)])
    m.frames = [("tip", n - 1, kin._rpy(0.1, -0.2, 0.3), (0.02, 0.0, link))]
    return m


def floating_weights(n, fill=1.0):
    """W_diag = 0 on the six floating-base coordinates"""
    W = np.full(n, fill)
    W[:6] = 0.0
    return W


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, terms, q [B][n]) of a named shape; q is reject-sampled so that cond(J W J') <= COND_CAP for every manipulability term"""
    F, CM, EF = abi.GRAD_MANIPULABILITY_FRAME, abi.GRAD_MANIPULABILITY_COM, abi.GRAD_MIN_EFFORT
    if name == "chain7":
        m = chain_model(7, 0.3, 3)
        terms = [gref.term(F, 0, W=np.linspace(1.0, 2.0, 7)), gref.term(CM, lam=0.5), gref.term(EF, W=np.full(7, 1e-2), lam=2.0)]
        B, seed = 3, 21
    elif name in ("humanoid32", "humanoid32_b257"):
        m = kin.humanoid32()
        m.frame_base = {1: 2}                         # r_wrist relative to l_sole
        n = m.n
        W = floating_weights(n) * np.linspace(0.5, 1.5, n)             # non-uniform
        holes = [j for j in range(n) if j % 5 != 2]                    # a joint mask with holes
        terms = [gref.term(F, 0, W=W, active=holes), gref.term(F, 1, W=floating_weights(n), lam=0.7),
                 gref.term(CM, W=np.linspace(1.0, 2.0, n), step=2e-3), gref.term(EF, W=np.linspace(1e-3, 3e-3, n), active=holes)]
        B, seed = (5, 22) if name == "humanoid32" else (257, 25)
    elif name == "coman35":
        m, _, _ = kin.from_json(os.path.join(ROOT, "tests", "golden", "coman_tree.json"))
        n = m.n
        terms = [gref.term(F, m.frame_index("l_wrist"), W=floating_weights(n)), gref.term(F, m.frame_index("r_wrist"), W=floating_weights(n)),
                 gref.term(CM), gref.term(EF, W=np.full(n, 1e-3))]
        B, seed = 4, 23
    elif name == "chain64":
        m = chain_model(64, 0.05, 4)
        terms = [gref.term(F, 0, W=np.linspace(0.5, 1.0, 64)), gref.term(CM), gref.term(EF, W=np.full(64, 1e-2))]
        B, seed = 2, 24
    else:
        raise KeyError(name)
    q, tries = gref.draw(m, terms, B, seed, COND_CAP)
    return m, terms, q


SHAPES = ("chain7", "humanoid32", "coman35", "chain64")


@functools.lru_cache(maxsize=None)
def reference(name, engine="pykin"):
    """the float64 restatement of a named shape, computed once per process and shared (callers must not write into it)"""
    m, terms, q = case(name)
    ref = gref.gradients(m, q, terms, GRAVITY, np.float64, engine)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def deviation(got_b, ref):
    """worst |got - ref| of b per term, in units of |lambda| x the cancellation scale max(|f+|, |f-|) / (2 step) of its instance: [T]"""
    return np.array([(np.abs(got_b[t] - ref["b"][t]).max(axis=1) / (abs(ref["lam"][t]) * ref["scale"][t])).max() for t in range(len(got_b))])


def value_deviation(got_value, ref):
    """worst |got - ref| of f(q) per term, relative to |f(q)|: the same unit (a relative error of the cost)"""
    return np.array([(np.abs(got_value[t] - ref["value"][t]) / np.abs(ref["value"][t])).max() for t in range(len(got_value))])


# ---- the kernel source on the host ------------------------------------------------------------------------------------------------
_lib = None


def grad_lib():
    """tests/emu/libosot_grad_host.so (tests/native_build.py)"""
    global _lib
    if _lib is None:
        L = native_build.load("grad_host")
        L.grad_host_gradient.argtypes = [C.POINTER(abi.KinDesc), C.POINTER(abi.GradDesc), C.POINTER(abi.GradBatch)]
        _lib = L
    return _lib


def emu_gradient(model, terms, q, gravity=GRAVITY):
    """the gradient kernel body on host arrays: q [B][n] -> dict(b [T][B][n], value [T][B])"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    B, n = q.shape
    T = len(terms)
    kd, gd, b = model.desc(), grad_desc(model, terms, gravity), abi.GradBatch()
    out = dict(b=np.full((T, B, n), 7.0), value=np.full((T, B), 7.0))
    b.B, b.q = B, q.ctypes.data
    for t in range(T):
        b.b[t], b.b_stride[t], b.value[t] = out["b"][t].ctypes.data, n, out["value"][t].ctypes.data
    rc = grad_lib().grad_host_gradient(C.byref(kd), C.byref(gd), C.byref(b))
    assert rc == abi.OK, rc
    return out
