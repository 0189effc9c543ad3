"""The rigid-body dynamics producer (osot_dyn_create / osot_dynamics, opensot_amd/csrc/osot_dyn.h), CPU side: the kernel source
through the host lock-step emulation (tests/emu/dyn_host.cpp) against the numpy restatement by another algorithm
(tests/dyn_ref.py), identities against the kinematics producer and finite differences, the refusals of osot_dyn_create (they
need no GPU) and the ctypes mirrors.

Measured on the committed seeds (host build against the restatement, relative to the largest entry of the compared array):
worst 1.6e-15 (com_Jdot_qdot on humanoid32; M 5.0e-16, h 3.6e-16, frame Jdot qdot 4.1e-16).  PARITY_TOL is 10x the worst."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from opensot_amd import abi
from opensot_amd import kinematics as kin

import dyn_ref
import native_build
from helpers import emu_kinematics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAVITY = (0.0, 0.0, -9.81)
PARITY_TOL = 1.6e-14     # 10 x the worst measured deviation (module docstring); the issue caps it at 1e-10
FD_EPS, FD_TOL = 1e-6, 1e-6
assert PARITY_TOL <= 1e-10

_lib = None


def dyn_lib():
    """tests/emu/libosot_dyn_host.so (tests/native_build.py)"""
    global _lib
    if _lib is None:
        L = native_build.load("dyn_host")
        L.dyn_host_dynamics.argtypes = [C.POINTER(abi.KinDesc), C.POINTER(abi.DynDesc), C.POINTER(abi.DynBatch)]
        _lib = L
    return _lib


def dyn_desc(model, gravity=GRAVITY):
    d = abi.DynDesc()
    I = np.zeros((model.n, 6)) if model.inertia is None else np.asarray(model.inertia, dtype=float).reshape(model.n, 6)
    for j in range(model.n):
        for i in range(6):
            d.inertia[j][i] = float(I[j, i])
    for i in range(3):
        d.gravity[i] = float(gravity[i])
    return d


def emu_dynamics(model, q, qdot=None, gravity=GRAVITY, want=("M", "h", "jdq", "com"), rc_only=False):
    """the dynamics kernel body on host arrays: q [B][n] -> dict(M [B][n][n], h [B][n], jdq [B][F][6], com_jdq [B][3])"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    B, n = q.shape
    F = len(model.frames)
    kd, dd, b = model.desc(), dyn_desc(model, gravity), abi.DynBatch()
    b.B, b.q = B, q.ctypes.data
    if qdot is not None:
        qdot = np.ascontiguousarray(qdot, dtype=np.float64)
        b.qdot = qdot.ctypes.data
    out = dict(M=np.full((B, n, n), 7.0), h=np.full((B, n), 7.0), jdq=np.full((B, F, 6), 7.0), com_jdq=np.full((B, 3), 7.0))
    if "M" in want:
        b.M, b.M_stride = out["M"].ctypes.data, n * n
    if "h" in want:
        b.h = out["h"].ctypes.data
    if "jdq" in want:
        for f in range(F):
            b.frame_Jdot_qdot[f] = out["jdq"].ctypes.data + 8 * 6 * f
            b.frame_Jdot_qdot_stride[f] = 6 * F
    if "com" in want:
        b.com_Jdot_qdot, b.com_Jdot_qdot_stride = out["com_jdq"].ctypes.data, 3
    rc = dyn_lib().dyn_host_dynamics(C.byref(kd), C.byref(dd), C.byref(b))
    if rc_only:
        return rc
    assert rc == abi.OK, rc
    return out


# ---- the three models -------------------------------------------------------------------------------------------------------
def random_inertia(n, rng, scale=2e-2):
    """tensors of actual mass distributions: I = Q diag(b + c, a + c, a + b) Q' with second moments a, b, c > 0"""
    out = np.zeros((n, 6))
    for j in range(n):
        a = rng.uniform(0.1, 1.0, 3) * scale
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        I = Q @ np.diag([a[1] + a[2], a[0] + a[2], a[0] + a[1]]) @ Q.T
        out[j] = [I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]]
    return out


def humanoid_model():
    m = kin.humanoid32()
    m.inertia = random_inertia(m.n, np.random.default_rng(11))
    m.inertia[:5] = 0.0          # the virtual links carry nothing
    return m, -np.ones(m.n), np.ones(m.n)


def coman_model():
    m, lo, up = kin.from_json(os.path.join(ROOT, "tests", "golden", "coman_tree.json"), os.path.join(ROOT, "tests", "golden", "coman_inertia.json"))
    lo, up = np.where(np.isfinite(lo), lo, -0.5), np.where(np.isfinite(up), up, 0.5)
    return m, lo, up


def chain3_model():
    """revolute - prismatic - revolute, skewed axes and offsets, one frame on the last link and one on the slider"""
    ax = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])
    m = kin.KinModel(parent=[-1, 0, 1], jtype=[abi.JOINT_REVOLUTE, abi.JOINT_PRISMATIC, abi.JOINT_REVOLUTE], axis=ax,
                     R0=np.array([kin._rpy(0.1, -0.2, 0.3), kin._rpy(0.4, 0.2, -0.1), kin._rpy(-0.3, 0.5, 0.2)]),
                     p0=np.array([[0.0, 0.0, 0.1], [0.2, 0.05, 0.0], [0.0, -0.1, 0.3]]), mass=np.array([1.5, 0.7, 2.0]),
                     com=np.array([[0.05, 0.0, 0.1], [0.0, 0.02, 0.15], [0.1, -0.05, 0.0]]), names=["j0", "slide", "j2"])
    m.frames = [("tip", 2, kin._rpy(0.2, 0.1, 0.0), (0.05, 0.0, 0.25)), ("slider", 1, np.eye(3), (0.0, 0.1, 0.0))]
    m.inertia = random_inertia(3, np.random.default_rng(5))
    return m, np.array([-2.0, -0.3, -2.0]), np.array([2.0, 0.5, 2.0])


MODELS = {"humanoid32": (humanoid_model, 6, 101), "coman35": (coman_model, 6, 102), "chain3": (chain3_model, 8, 103)}


def sample(name):
    make, B, seed = MODELS[name]
    m, lo, up = make()
    rng = np.random.default_rng(seed)
    return m, rng.uniform(lo, up, (B, m.n)), rng.uniform(-2.0, 2.0, (B, m.n)), rng


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_host_build_against_restatement(name):
    m, q, qd, _ = sample(name)
    got, ref = emu_dynamics(m, q, qd), dyn_ref.batch(m, q, qd, GRAVITY)
    for k in ("M", "h", "jdq", "com_jdq"):
        d = rel(got[k], ref[k])
        print(f"{name} {k}: rel {d:.3e}")
        assert d <= PARITY_TOL, (name, k, d)
    g0 = emu_dynamics(m, q, None)                       # qdot = NULL: the gravity term, no bias acceleration
    ref0 = dyn_ref.batch(m, q, None, GRAVITY)
    assert rel(g0["h"], ref0["h"]) <= PARITY_TOL and np.all(g0["jdq"] == 0.0) and np.all(g0["com_jdq"] == 0.0)
    assert np.array_equal(g0["M"], got["M"])


# ---- 2. identities against the kinematics producer ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_inertia_matrix_symmetric_positive_definite(name):
    m, q, qd, _ = sample(name)
    M = emu_dynamics(m, q, qd)["M"]
    for i in range(len(q)):
        assert np.array_equal(M[i], M[i].T)             # bit for bit
        np.linalg.cholesky(M[i])


@pytest.mark.parametrize("name", ["humanoid32", "coman35"])
def test_floating_base_rows_are_the_centre_of_mass(name):
    m, q, _, _ = sample(name)
    _, J, _ = emu_kinematics(m, q)
    Jcom = J[:, 6 * len(m.frames):, :]
    got = emu_dynamics(m, q, None)
    mt = m.mass.sum()
    assert rel(got["M"][:, :3, :], mt * Jcom) <= PARITY_TOL
    assert rel(got["h"], -mt * np.einsum("bin,i->bn", Jcom, np.array(GRAVITY))) <= PARITY_TOL


@pytest.mark.parametrize("name", sorted(MODELS))
def test_coriolis_power(name):
    """qdot' (h(q, qdot) - h(q, 0)) = 0.5 qdot' Mdot qdot, Mdot by central differences of the producer's own M"""
    m, q, qd, _ = sample(name)
    hc = emu_dynamics(m, q, qd)["h"] - emu_dynamics(m, q, None)["h"]
    Mp, Mm = emu_dynamics(m, q + FD_EPS * qd, None)["M"], emu_dynamics(m, q - FD_EPS * qd, None)["M"]
    Md = (Mp - Mm) / (2 * FD_EPS)
    lhs = np.einsum("bi,bi->b", qd, hc)
    rhs = 0.5 * np.einsum("bi,bij,bj->b", qd, Md, qd)
    scale = np.abs(np.einsum("bi,bij,bj->b", np.abs(qd), np.abs(Md), np.abs(qd))).max()
    print(f"{name}: coriolis power {np.abs(lhs - rhs).max() / scale:.3e}")
    assert np.abs(lhs - rhs).max() <= FD_TOL * scale


@pytest.mark.parametrize("name", sorted(MODELS))
def test_jdot_qdot_against_differences_of_the_kinematics_producer(name):
    """d/dt (J qdot) at qddot = 0: central differences of osot_kinematics' J(q +- eps qdot) qdot"""
    m, q, qd, _ = sample(name)
    F = len(m.frames)
    got = emu_dynamics(m, q, qd)
    _, Jp, _ = emu_kinematics(m, q + FD_EPS * qd)
    _, Jm, _ = emu_kinematics(m, q - FD_EPS * qd)
    fd = np.einsum("brn,bn->br", Jp - Jm, qd) / (2 * FD_EPS)
    for f in range(F):
        assert rel(got["jdq"][:, f], fd[:, 6 * f:6 * f + 6]) <= FD_TOL, (name, f)
    assert rel(got["com_jdq"], fd[:, 6 * F:]) <= FD_TOL


@pytest.mark.parametrize("name", sorted(MODELS))
def test_equation_of_motion(name):
    """M qddot + h of the producer against the restatement's tau(q, qdot, qddot) for random qddot (measured: 4.8e-16 at worst)"""
    m, q, qd, rng = sample(name)
    qdd = rng.uniform(-5.0, 5.0, q.shape)
    got = emu_dynamics(m, q, qd)
    lhs = np.einsum("bij,bj->bi", got["M"], qdd) + got["h"]
    ref = np.array([dyn_ref.Ref(m, q[i], qd[i], GRAVITY).tau(qdd[i]) for i in range(len(q))])
    assert rel(lhs, ref) <= PARITY_TOL


def test_strided_outputs_leave_the_gaps():
    m, q, qd, _ = sample("chain3")
    B, n = q.shape
    q, qd = np.ascontiguousarray(q), np.ascontiguousarray(qd)
    M = np.full((B, n * n + 5), 7.0); p1 = np.full((B, 11), 7.0); cj = np.full((B, 4), 7.0)
    b = abi.DynBatch()
    b.B, b.q, b.qdot, b.M, b.M_stride = B, q.ctypes.data, qd.ctypes.data, M.ctypes.data, n * n + 5
    b.frame_Jdot_qdot[1], b.frame_Jdot_qdot_stride[1] = p1.ctypes.data + 8 * 2, 11
    b.com_Jdot_qdot, b.com_Jdot_qdot_stride = cj.ctypes.data, 4
    kd, dd = m.desc(), dyn_desc(m)
    assert dyn_lib().dyn_host_dynamics(C.byref(kd), C.byref(dd), C.byref(b)) == abi.OK
    ref = emu_dynamics(m, q, qd)
    assert np.array_equal(M[:, :n * n].reshape(B, n, n), ref["M"]) and np.all(M[:, n * n:] == 7.0)
    assert np.array_equal(p1[:, 2:8], ref["jdq"][:, 1]) and np.all(p1[:, :2] == 7.0) and np.all(p1[:, 8:] == 7.0)
    assert np.array_equal(cj[:, :3], ref["com_jdq"]) and np.all(cj[:, 3] == 7.0)


# ---- 3. refusals (no GPU is touched before them) and the ABI ------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return abi.lib()


def _create(lib, kd, dd):
    h = C.c_void_p()
    rc = lib.osot_dyn_create(C.byref(kd), C.byref(dd), 0, C.byref(h))
    assert not h.value
    return rc, lib.osot_last_error()


def test_create_refusals(lib):
    m, _, _ = chain3_model()
    good_k, good_d = m.desc, lambda: dyn_desc(m)
    assert lib.osot_dyn_create(None, None, 0, None) == abi.ERR_INVALID
    cases = []
    kd, dd = good_k(), good_d(); kd.parent[1] = 1; cases.append((kd, dd, b"tree order"))
    kd, dd = good_k(), good_d(); kd.n = abi.KIN_MAX_JOINTS + 1; cases.append((kd, dd, b"joint count"))
    kd, dd = good_k(), good_d(); kd.n = 0; cases.append((kd, dd, b"joint count"))
    kd, dd = good_k(), good_d(); kd.type[0] = 2; cases.append((kd, dd, b"joint type"))
    kd, dd = good_k(), good_d(); kd.axis[1][0] = 0.7; cases.append((kd, dd, b"unit vectors"))
    kd, dd = good_k(), good_d(); kd.p0[2][1] = float("nan"); cases.append((kd, dd, b"NaN"))
    kd, dd = good_k(), good_d(); dd.inertia[0][3] = float("nan"); cases.append((kd, dd, b"NaN"))
    kd, dd = good_k(), good_d(); dd.gravity[2] = float("inf"); cases.append((kd, dd, b"NaN"))
    kd, dd = good_k(), good_d(); kd.mass[0] = -1.0; cases.append((kd, dd, b"negative link mass"))
    kd, dd = good_k(), good_d(); kd.frame_joint[0] = 3; cases.append((kd, dd, b"frame attached"))
    kd, dd = good_k(), good_d()
    for i, v in enumerate((1.0, 0.0, 0.0, -0.5, 0.0, 1.0)): dd.inertia[1][i] = v       # a negative principal moment
    cases.append((kd, dd, b"positive semi-definite"))
    kd, dd = good_k(), good_d()
    for i, v in enumerate((1.0, 2.0, 0.0, 1.0, 0.0, 5.0)): dd.inertia[1][i] = v        # indefinite through the off-diagonal
    cases.append((kd, dd, b"positive semi-definite"))
    kd, dd = good_k(), good_d()
    for i, v in enumerate((1.0, 0.0, 0.0, 1.0, 0.0, 2.5)): dd.inertia[2][i] = v        # 1 + 1 < 2.5
    cases.append((kd, dd, b"triangle"))
    for kd, dd, text in cases:
        rc, msg = _create(lib, kd, dd)
        assert rc == abi.ERR_INVALID and text in msg, (text, rc, msg)


def test_batch_refusals_on_the_host_build():
    """osot_dynamics' checks (dyn_check_batch, shared with the library): relative / BODY frames, strides, frames out of range"""
    m, q, qd, _ = sample("chain3")
    assert emu_dynamics(m, q, qd, rc_only=True) == abi.OK
    m.frame_body = {0: True}
    assert emu_dynamics(m, q, qd, rc_only=True) == abi.ERR_UNSUPPORTED
    assert emu_dynamics(m, q, qd, want=("M", "h", "com"), rc_only=True) == abi.OK      # only the frame's Jdot qdot is refused
    m.frame_body = {}
    m.frame_base = {1: 0}
    assert emu_dynamics(m, q, qd, rc_only=True) == abi.ERR_UNSUPPORTED
    m.frame_base = {}
    b = abi.DynBatch(); b.B = 1; b.q = q.ctypes.data
    M = np.zeros(9); b.M, b.M_stride = M.ctypes.data, 8
    kd, dd = m.desc(), dyn_desc(m)
    assert dyn_lib().dyn_host_dynamics(C.byref(kd), C.byref(dd), C.byref(b)) == abi.ERR_INVALID
    b.M = None; b.frame_Jdot_qdot[2] = M.ctypes.data; b.frame_Jdot_qdot_stride[2] = 6
    assert dyn_lib().dyn_host_dynamics(C.byref(kd), C.byref(dd), C.byref(b)) == abi.ERR_INVALID
    b.frame_Jdot_qdot[2] = None; b.q = None
    assert dyn_lib().dyn_host_dynamics(C.byref(kd), C.byref(dd), C.byref(b)) == abi.ERR_INVALID


def test_dynamics_null_arguments(lib):
    assert lib.osot_dynamics(None, None, None) == abi.ERR_INVALID and b"null" in lib.osot_last_error()
    assert lib.osot_dyn_destroy(None) == abi.OK


def test_struct_layouts(lib):
    lib.osot_abi_layout.argtypes = [C.c_char_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]
    for name, cls in (("osot_dyn_desc", abi.DynDesc), ("osot_dyn_batch", abi.DynBatch)):
        size, nf = C.c_ulonglong(), C.c_int()
        offs = (C.c_ulonglong * 64)()
        assert lib.osot_abi_layout(name.encode(), C.byref(size), offs, 64, C.byref(nf)) == abi.OK, name
        assert size.value == C.sizeof(cls)
        mine = [getattr(cls, f[0]).offset for f in cls._fields_]
        assert nf.value == len(mine) and list(offs[:nf.value]) == mine
    for s in ("osot_dyn_create", "osot_dyn_destroy", "osot_dynamics"):
        assert s in abi.SYMBOLS and hasattr(lib, s)


def test_coman_inertia_fixture():
    """the committed tensors are physical and belong to the committed tree"""
    m, _, _ = coman_model()
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "coman_inertia.json")))
    assert doc["n"] == m.n == 35 and doc["names"] == m.names
    for j in range(m.n):
        I = dyn_ref.inertia_of(m)[j]
        w = np.linalg.eigvalsh(I)
        assert w[0] >= 0.0 and w[0] + w[1] >= w[2] * (1 - 1e-12)
        assert (m.mass[j] > 0) == (w[2] > 0)


# ---- 4. the COMAN inverse-dynamics stack on the producers, host side ------------------------------------------------------------
def coman_quantities(model, q, qd, source="emu", frames=(2, 3)):
    """the model quantities of one control step, from the host build of the two producers ("emu") or from the restatement ("ref")"""
    B, n = q.shape
    if source == "emu":
        d = emu_dynamics(model, q, qd)
        _, J, com = emu_kinematics(model, q)
        F = len(model.frames)
        Jc = np.stack([J[:, 6 * f:6 * f + 6] for f in frames], axis=1)
        return dict(M=d["M"], h=d["h"], Jc=Jc, jdq=d["jdq"][:, list(frames)], com_jdq=d["com_jdq"], Jcom=J[:, 6 * F:], com=com)
    out = dict(M=np.zeros((B, n, n)), h=np.zeros((B, n)), Jc=np.zeros((B, 2, 6, n)), jdq=np.zeros((B, 2, 6)), com_jdq=np.zeros((B, 3)),
               Jcom=np.zeros((B, 3, n)), com=np.zeros((B, 3)))
    for i in range(B):
        r = dyn_ref.Ref(model, q[i], qd[i], GRAVITY)
        out["M"][i], out["h"][i] = r.inertia_matrix(), r.tau()
        for c, f in enumerate(frames):
            out["Jc"][i, c], out["jdq"][i, c] = r.frame_jacobian(f), r.frame_jdot_qdot(f)
        out["com_jdq"][i], out["Jcom"][i], out["com"][i] = r.com_jdot_qdot(), r.fk["Jcom"], r.fk["com"]
    return out


def _ref_quantities_one(args):
    model, q, qd = args
    return coman_quantities(model, q[None], qd[None], "ref")


def coman_quantities_parallel(pool, model, q, qd):
    """the restatement for a batch, one instance per task of a process pool (it is a python loop over links and joints)"""
    parts = list(pool.map(_ref_quantities_one, [(model, q[i], qd[i]) for i in range(len(q))]))
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}


def coman_fill_leaf(leaf, Q, q, qd, com_ref):
    """the leaf of synth.make_coman_id_stack for this step (numpy): A_0, the producer-written rows of C, errors, h"""
    B, nv = q.shape
    n = nv + 12
    A0 = np.zeros((B, 15, n))
    A0[:, :12, :nv] = Q["Jc"].reshape(B, 12, nv); A0[:, 12:, :nv] = Q["Jcom"]
    Cdyn, Ctau = np.zeros((B, 6, n)), np.zeros((B, nv, n))
    Cdyn[:, :, :nv] = Q["M"][:, :6]; Ctau[:, :, :nv] = Q["M"]
    for c in range(2):
        Cdyn[:, :, nv + 6 * c:nv + 6 * c + 6] = -np.transpose(Q["Jc"][:, c][:, :, :6], (0, 2, 1))
        Ctau[:, :, nv + 6 * c:nv + 6 * c + 6] = -np.transpose(Q["Jc"][:, c], (0, 2, 1))
    z = np.zeros
    out = dict(leaf)
    out["A"] = [A0, None]
    out["C"] = [Cdyn, None, None, Ctau]
    pcom = np.concatenate([com_ref - Q["com"], -np.einsum("bij,bj->bi", Q["Jcom"], qd)], axis=1)
    out["task"] = [[(z((B, 12)), Q["jdq"][:, 0], None), (z((B, 12)), Q["jdq"][:, 1], None), (pcom, Q["com_jdq"], None)],
                   [(np.concatenate([leaf["state"]["q_ref"] - q, -qd], axis=1), None, None)]]
    rows = list(leaf["rows"])
    rows[0] = (Q["h"][:, :6].copy(), None, None)
    rows[3] = (Q["h"], rows[3][1], None)
    out["rows"] = rows
    return out


def coman_host_loop(B, steps, seed, source="emu", perturb=0.0, dt=1e-3):
    """the closed loop on the host: producers' host build (or the restatement) -> emulated update + cascade -> explicit integration.
    perturb: every model quantity is multiplied by (1 + perturb * u), u uniform in [-1, 1], before it is used"""
    from helpers import emu_cascade, emu_update
    from opensot_amd import synth
    plan, leaf, model = synth.make_coman_id_stack(B, seed=seed)
    q, qd = leaf["state"]["q0"].copy(), leaf["state"]["qdot0"].copy()
    rng = np.random.default_rng(1)
    com_ref, traj, worst = None, [], 0.0
    for _ in range(steps):
        Q = coman_quantities(model, q, qd, source)
        if perturb:
            Q = {k: v * (1.0 + perturb * rng.uniform(-1, 1, v.shape)) for k, v in Q.items()}
        com_ref = Q["com"].copy() if com_ref is None else com_ref
        lf = coman_fill_leaf(leaf, Q, q, qd, com_ref)
        res = emu_update(plan, lf)
        asm = dict(B=B, n=plan.n, L=plan.L, A=lf["A"], b=res["b"], w=res["w"], C=res["C"], lo=res["lo"], up=res["up"], l=None, u=None)
        x, _, st, _ = emu_cascade(plan, asm)
        assert (st == 0).all(), st
        qdd, W = x[:, :model.n], x[:, model.n:].reshape(B, 2, 6)
        tau = np.einsum("bij,bj->bi", Q["M"], qdd) + Q["h"] - np.einsum("bcij,bci->bj", Q["Jc"], W)
        worst = max(worst, np.abs(tau[:, :6]).max())
        assert np.abs(tau[:, 6:]).max() <= 60.0 + 1e-8
        q = q + dt * qd + 0.5 * dt * dt * qdd
        qd = qd + dt * qdd
        traj.append(q.copy())
    return np.array(traj), worst


def test_coman_id_stack_host_loop_is_stable_under_input_round_off():
    """The pre-check of the seeds the GPU closed loop uses (tests/test_dynamics_gpu.py): through the host builds of the producers
    and of the cascade the stack solves every step with the floating-base rows of the torque at round-off, and the same run with
    every model quantity perturbed by 1e-13 relative stays within the 1e-6 cap of the trajectory comparison.  (Here B = 4 and
    8 steps: the emulated cascade runs a 47-variable instance in about a second.)"""
    a, worst = coman_host_loop(4, 8, seed=31)
    b, _ = coman_host_loop(4, 8, seed=31, perturb=1e-13)
    print(f"floating-base torque residual {worst:.3e}, |q - q_perturbed| {np.abs(a - b).max():.3e}")
    assert worst <= 1e-8
    assert np.abs(a - b).max() <= 1e-6
