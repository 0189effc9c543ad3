"""The centroidal momentum outputs of the dynamics producer (osot_dyn_batch.cmm_lin / cmm_ang / momentum / ang_mom_b,
opensot_amd/csrc/osot_dyn.h stage 5a), CPU side: the kernel source through the host lock-step emulation (tests/emu/dyn_host.cpp)
against the numpy restatement by another algorithm (tests/momentum_ref.py), identities against the kinematics producer and the
inertia matrix, the analytic single link, the layout of the strided outputs and the refusals of dyn_check_batch.

Measured on the committed seeds (host build against the restatement, relative to the largest entry of the compared array), worst
over the six models: cmm_lin 6.3e-16 (chain64), cmm_ang 6.5e-15 (humanoid32; coman35 6.0e-15 -- the shift n_j - c_G x f_j cancels
where the base is far from the origin), momentum 8.4e-16 (chain64), momentum against the link-velocity form 6.1e-16 (coman35);
cmm_lin against total_mass * com_J 4.4e-16 (humanoid32), against M[:3] 0 (the same values); cmm qdot against momentum 5.6e-16
(chain64).  Worst of all: 6.5e-15; PARITY_TOL is 10x that."""
import ctypes as C

import numpy as np
import pytest

from opensot_amd import abi
from opensot_amd import kinematics as kin

import momentum_ref
import test_dynamics_host as tdh
from helpers import emu_kinematics
from test_dynamics_host import rel

PARITY_TOL = 6.5e-14     # 10 x the worst measured deviation (module docstring); capped at the 1e-10 of test_dynamics_host.py
assert PARITY_TOL <= 1e-10


# ---- the six models ---------------------------------------------------------------------------------------------------------
def _random_tree(parent, jtype, seed):
    rng = np.random.default_rng(seed)
    n = len(parent)
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    m = kin.KinModel(parent=list(parent), jtype=list(jtype), axis=ax,
                     R0=np.array([kin._rpy(*rng.uniform(-0.6, 0.6, 3)) for _ in range(n)]), p0=rng.uniform(-0.15, 0.15, (n, 3)),
                     mass=rng.uniform(0.3, 2.0, n), com=rng.uniform(-0.08, 0.08, (n, 3)), names=[f"j{j}" for j in range(n)])
    m.inertia = tdh.random_inertia(n, rng)
    lim = np.where(np.array(jtype) == abi.JOINT_REVOLUTE, 1.5, 0.3)
    return m, -lim, lim


def single_model():
    """n = 1: one revolute link"""
    return _random_tree([-1], [abi.JOINT_REVOLUTE], 21)


def tree7_model():
    """siblings interleave, so the depth-first order differs from the index order; joints 2 and 5 are prismatic"""
    R, P = abi.JOINT_REVOLUTE, abi.JOINT_PRISMATIC
    return _random_tree([-1, 0, 0, 1, 2, 1, 2], [R, R, P, R, R, P, R], 22)


def chain64_model():
    """a serial chain of 64 joints: every lane, and the deepest pointer jumping"""
    R, P = abi.JOINT_REVOLUTE, abi.JOINT_PRISMATIC
    return _random_tree(list(range(-1, 63)), [P if j % 9 == 4 else R for j in range(64)], 23)


MODELS = dict(tdh.MODELS)                 # chain3 (B = 8), humanoid32 (6), coman35 (6): read-only
MODELS.update({"single": (single_model, 1, 104), "tree7": (tree7_model, 5, 105), "chain64": (chain64_model, 3, 106)})
FLOATING = ("humanoid32", "coman35")


def sample(name, B=None):
    make, B0, seed = MODELS[name]
    B = B0 if B is None else B
    m, lo, up = make()
    rng = np.random.default_rng(seed)
    return m, rng.uniform(lo, up, (B, m.n)), rng.uniform(-2.0, 2.0, (B, m.n)), rng


def momentum_batch(model, q, qdot, out, pad=0, slack=0, wide=0, ang=None, base=("M", "h", "jdq", "com"),
                   want=("cmm_lin", "cmm_ang", "momentum")):
    """the osot_dyn_batch of a call on host arrays, and the arrays (filled with 7.0) in `out`.  pad: ld = n + pad; slack: doubles
    between the instances of the matrix rows; wide: extra doubles per instance of momentum / ang_mom_b;
    ang: dict(ref=, rate_ref=, K=, lam=) binds ang_mom_b"""
    B, n = q.shape
    F = len(model.frames)
    b = abi.DynBatch()
    b.B, b.q = B, q.ctypes.data
    if qdot is not None:
        b.qdot = qdot.ctypes.data
    out.update(M=np.full((B, n, n), 7.0), h=np.full((B, n), 7.0), jdq=np.full((B, max(F, 1), 6), 7.0), com_jdq=np.full((B, 3), 7.0))
    if "M" in base:
        b.M, b.M_stride = out["M"].ctypes.data, n * n
    if "h" in base:
        b.h = out["h"].ctypes.data
    if "jdq" in base:
        for f in range(F):
            b.frame_Jdot_qdot[f] = out["jdq"].ctypes.data + 8 * 6 * f
            b.frame_Jdot_qdot_stride[f] = 6 * F
    if "com" in base:
        b.com_Jdot_qdot, b.com_Jdot_qdot_stride = out["com_jdq"].ctypes.data, 3
    ld = n + pad
    for k in ("cmm_lin", "cmm_ang"):
        out[k + "_raw"] = np.full((B, 3 * ld + slack), 7.0)
        if k in want:
            setattr(b, k, out[k + "_raw"].ctypes.data); setattr(b, k + "_stride", 3 * ld + slack); setattr(b, k + "_ld", ld if pad else 0)
    out["momentum_raw"], out["ang_mom_b_raw"] = np.full((B, 6 + wide), 7.0), np.full((B, 3 + wide), 7.0)
    if "momentum" in want:
        b.momentum, b.momentum_stride = out["momentum_raw"].ctypes.data, 6 + wide
    if ang is not None:
        b.ang_mom_b, b.ang_mom_b_stride = out["ang_mom_b_raw"].ctypes.data, 3 + wide
        for key, field in (("ref", "ang_mom_ref"), ("rate_ref", "ang_mom_rate_ref")):
            if ang.get(key) is not None:
                out["_" + key] = np.ascontiguousarray(ang[key], dtype=np.float64)
                setattr(b, field, out["_" + key].ctypes.data)
        if ang.get("K") is not None:
            for i, v in enumerate(np.asarray(ang["K"], dtype=float).reshape(9)):
                b.ang_mom_gain[i] = float(v)
        b.ang_mom_lambda = float(ang.get("lam", 1.0))
    return b


def views(out, n, pad=0):
    ld = n + pad
    for k in ("cmm_lin", "cmm_ang"):
        out[k] = out[k + "_raw"][:, :3 * ld].reshape(-1, 3, ld)[:, :, :n]
    out["momentum"], out["ang_mom_b"] = out["momentum_raw"][:, :6], out["ang_mom_b_raw"][:, :3]
    return out


def emu_momentum(model, q, qdot=None, **kw):
    """the dynamics kernel body with the momentum outputs on host arrays: dict(cmm_lin [B][3][n], cmm_ang [B][3][n],
    momentum [B][6], ang_mom_b [B][3], M, h, jdq, com_jdq and the *_raw arrays with their gaps)"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    qdot = None if qdot is None else np.ascontiguousarray(qdot, dtype=np.float64)
    out = {}
    b = momentum_batch(model, q, qdot, out, **kw)
    kd, dd = model.desc(), tdh.dyn_desc(model)
    rc = tdh.dyn_lib().dyn_host_dynamics(C.byref(kd), C.byref(dd), C.byref(b))
    assert rc == abi.OK, rc
    return views(out, model.n, kw.get("pad", 0))


_cache = {}


def case(name):
    """(model, q, qdot, host build, restatement) of a model, computed once and shared (nobody writes to them)"""
    if name not in _cache:
        m, q, qd, _ = sample(name)
        _cache[name] = (m, q, qd, emu_momentum(m, q, qd), momentum_ref.batch(m, q, qd))
    return _cache[name]


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_host_build_against_restatement(name):
    m, q, qd, got, ref = case(name)
    for k, a, r in (("cmm_lin", got["cmm_lin"], ref["cmm"][:, :3]), ("cmm_ang", got["cmm_ang"], ref["cmm"][:, 3:]),
                    ("momentum", got["momentum"], ref["momentum"]), ("momentum (links)", got["momentum"], ref["momentum_links"])):
        d = rel(a, r)
        print(f"{name} {k}: rel {d:.3e}")
        assert d <= PARITY_TOL, (name, k, d)


# ---- 2. identities against the kinematics producer and the inertia matrix -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_linear_rows_are_the_centre_of_mass_jacobian(name):
    m, q, qd, got, _ = case(name)
    _, J, _ = emu_kinematics(m, q)
    d = rel(got["cmm_lin"], m.mass.sum() * J[:, 6 * len(m.frames):, :])
    print(f"{name} cmm_lin against total_mass * com_J: rel {d:.3e}")
    assert d <= PARITY_TOL
    if name in FLOATING:
        d = rel(got["cmm_lin"], got["M"][:, :3, :])
        print(f"{name} cmm_lin against M[:3]: rel {d:.3e}")
        assert d <= PARITY_TOL


# ---- 3. momentum = matrix * qdot ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_momentum_is_the_matrix_times_qdot(name):
    m, q, qd, got, _ = case(name)
    cmm = np.concatenate([got["cmm_lin"], got["cmm_ang"]], axis=1)
    d = rel(np.einsum("brn,bn->br", cmm, qd), got["momentum"])
    print(f"{name} cmm qdot against momentum: rel {d:.3e}")
    assert d <= PARITY_TOL
    g0 = emu_momentum(m, q, None)
    assert np.all(g0["momentum"] == 0.0)
    assert np.array_equal(g0["cmm_lin"], got["cmm_lin"]) and np.array_equal(g0["cmm_ang"], got["cmm_ang"])


# ---- 4. the single link, analytic ---------------------------------------------------------------------------------------------
def test_single_link_analytic():
    m, q, qd, got, _ = case("single")
    a = m.axis[0]
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    I = np.zeros((3, 3))
    for k, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        I[r, c] = I[c, r] = m.inertia[0][k]
    for i in range(len(q)):
        R = m.R0[0] @ (np.eye(3) + np.sin(q[i, 0]) * Kx + (1.0 - np.cos(q[i, 0])) * Kx @ Kx)     # Rodrigues
        z, p = R @ a, m.p0[0]
        c = p + R @ m.com[0]
        assert rel(got["cmm_ang"][i, :, 0], R @ I @ R.T @ z) <= PARITY_TOL
        assert rel(got["cmm_lin"][i, :, 0], m.mass[0] * np.cross(z, c - p)) <= PARITY_TOL


# ---- 5. the existing outputs do not move -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_existing_outputs_are_bit_identical(name):
    m, q, qd, got, _ = case(name)
    plain = tdh.emu_dynamics(m, q, qd)
    for k in ("M", "h", "com_jdq"):
        assert np.array_equal(got[k], plain[k]), (name, k)
    F = len(m.frames)
    assert np.array_equal(got["jdq"][:, :F], plain["jdq"])
    only = emu_momentum(m, q, qd, base=())                  # nothing but the new outputs: stages 4 and 5 are forced
    for k in ("cmm_lin", "cmm_ang", "momentum"):
        assert np.array_equal(only[k], got[k]), (name, k)
    assert np.all(only["M"] == 7.0) and np.all(only["h"] == 7.0) and np.all(only["com_jdq"] == 7.0)


# ---- 6. layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain3", "tree7", "chain64"])
def test_strided_outputs_leave_the_gaps(name):
    m, q, qd, got, _ = case(name)
    B, n = q.shape
    ang = dict(ref=np.zeros((B, 3)), lam=1.0)
    w = emu_momentum(m, q, qd, pad=5, slack=4, wide=3, ang=ang)
    dense = emu_momentum(m, q, qd, ang=ang)
    for k in ("cmm_lin", "cmm_ang"):
        assert np.array_equal(w[k], got[k])
        raw = w[k + "_raw"]
        rows = raw[:, :3 * (n + 5)].reshape(B, 3, n + 5)
        assert np.all(rows[:, :, n:] == 7.0) and np.all(raw[:, 3 * (n + 5):] == 7.0)
    assert np.array_equal(w["momentum"], got["momentum"]) and np.all(w["momentum_raw"][:, 6:] == 7.0)
    assert np.array_equal(w["ang_mom_b"], dense["ang_mom_b"]) and np.all(w["ang_mom_b_raw"][:, 3:] == 7.0)
    assert np.all(w["ang_mom_b"] != 7.0)


# ---- 7. the b of acceleration::AngularMomentum ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_ang_mom_b(name):
    m, q, qd, _, _ = case(name)
    B = len(q)
    rng = np.random.default_rng(7)
    Ld, Ldd, K, lam = rng.uniform(-1, 1, (B, 3)), rng.uniform(-3, 3, (B, 3)), rng.uniform(-2, 2, (3, 3)), 0.7
    got = emu_momentum(m, q, qd, ang=dict(ref=Ld, rate_ref=Ldd, K=K, lam=lam))
    e = Ld - got["momentum"][:, 3:]
    want = Ldd + lam * np.einsum("ij,bj->bi", K, e)
    largest = np.maximum(np.abs(Ldd), lam * np.abs(K[None] * e[:, None, :]).max(axis=2))
    assert np.all(np.abs(got["ang_mom_b"] - want) <= 4 * np.spacing(largest)), np.abs(got["ang_mom_b"] - want).max()
    # no reference: L_d = L, b = Ldot_d
    assert np.array_equal(emu_momentum(m, q, qd, ang=dict(rate_ref=Ldd, K=K, lam=lam))["ang_mom_b"], Ldd)
    # no rate reference: that term is absent
    nr = emu_momentum(m, q, qd, ang=dict(ref=Ld, K=K, lam=lam))["ang_mom_b"]
    w2 = lam * np.einsum("ij,bj->bi", K, e)
    assert np.all(np.abs(nr - w2) <= 4 * np.spacing(lam * np.abs(K[None] * e[:, None, :]).max(axis=2)))
    assert np.all(emu_momentum(m, q, qd, ang=dict(lam=lam))["ang_mom_b"] == 0.0)
    # an all-zero K is the identity
    z = emu_momentum(m, q, qd, ang=dict(ref=Ld, rate_ref=Ldd, K=np.zeros((3, 3)), lam=lam))["ang_mom_b"]
    i3 = emu_momentum(m, q, qd, ang=dict(ref=Ld, rate_ref=Ldd, K=np.eye(3), lam=lam))["ang_mom_b"]
    assert np.array_equal(z, i3)
    assert np.all(np.abs(z - (Ldd + lam * e)) <= 4 * np.spacing(np.maximum(np.abs(Ldd), lam * np.abs(e))))


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_batch_refusals():
    m, q, qd, _ = sample("chain3", B=2)
    q, qd = np.ascontiguousarray(q), np.ascontiguousarray(qd)
    n = m.n
    kd, dd = m.desc(), tdh.dyn_desc(m)
    ang = dict(ref=np.zeros((2, 3)), rate_ref=np.zeros((2, 3)), lam=1.0)

    def refused(change):
        out = {}
        b = momentum_batch(m, q, qd, out, pad=2, ang=ang)
        change(b)
        rc = tdh.dyn_lib().dyn_host_dynamics(C.byref(kd), C.byref(dd), C.byref(b))
        untouched = all(np.all(out[k] == 7.0) for k in ("M", "h", "jdq", "com_jdq", "cmm_lin_raw", "cmm_ang_raw", "momentum_raw", "ang_mom_b_raw"))
        return rc == abi.ERR_INVALID and untouched

    assert not refused(lambda b: None)                      # the batch itself is fine
    assert refused(lambda b: setattr(b, "cmm_lin_ld", n - 1))
    assert refused(lambda b: setattr(b, "cmm_ang_ld", n - 1))
    assert refused(lambda b: setattr(b, "cmm_ang_ld", -1))
    assert refused(lambda b: setattr(b, "cmm_lin_stride", 3 * (n + 2) - 1))
    assert refused(lambda b: setattr(b, "cmm_ang_stride", 3 * (n + 2) - 1))
    assert refused(lambda b: setattr(b, "cmm_ang_stride", 0))

    def dense_short(b):                                     # ld = 0 means n: the stride is measured against 3 n
        b.cmm_lin_ld, b.cmm_lin_stride = 0, 3 * n - 1
    assert refused(dense_short)
    assert refused(lambda b: setattr(b, "momentum_stride", 5))
    assert refused(lambda b: setattr(b, "ang_mom_b_stride", 2))

    def ref_without_b(b):
        b.ang_mom_b, b.ang_mom_rate_ref = None, None
    assert refused(ref_without_b)

    def rate_without_b(b):
        b.ang_mom_b, b.ang_mom_ref = None, None
    assert refused(rate_without_b)

    def bad_gain(b):
        b.ang_mom_gain[4] = float("nan")
    assert refused(bad_gain)
    assert refused(lambda b: setattr(b, "ang_mom_lambda", float("inf")))


def test_struct_mirror_has_the_fields_at_the_end():
    """the new fields follow com_Jdot_qdot_stride, so positional initialisers of the older fields stay valid"""
    names = [f[0] for f in abi.DynBatch._fields_]
    assert names[:10] == ["B", "q", "qdot", "M", "M_stride", "h", "frame_Jdot_qdot", "frame_Jdot_qdot_stride", "com_Jdot_qdot",
                          "com_Jdot_qdot_stride"]
    assert names[10:] == ["cmm_lin", "cmm_lin_stride", "cmm_lin_ld", "cmm_ang", "cmm_ang_stride", "cmm_ang_ld", "momentum",
                          "momentum_stride", "ang_mom_b", "ang_mom_b_stride", "ang_mom_ref", "ang_mom_rate_ref", "ang_mom_gain",
                          "ang_mom_lambda"]


# ---- 9. the momentum stacks, driven on the CPU ---------------------------------------------------------------------------------
def test_momentum_stacks_on_the_cpu():
    """synth.make_coman_momentum_stack with and without the momentum level: a short closed loop through the restatements and the oracle
    solver (tests/momentum_cases.py; the GPU tests run 40 cycles of it on the device).  momentum=False drops the level and nothing else"""
    import momentum_cases as mc
    from opensot_amd import synth
    pa, la, _ = synth.make_coman_momentum_stack(2, seed=5)
    pb, lb, _ = synth.make_coman_momentum_stack(2, seed=5, momentum=False)
    assert [t.name for lev in pa.levels for t in lev] == ["l_sole", "r_sole", "com", "angular_momentum", "postural"]
    assert [t.name for lev in pb.levels for t in lev] == ["l_sole", "r_sole", "com", "postural"]
    assert np.array_equal(la["state"]["q_ref"], lb["state"]["q_ref"]) and np.array_equal(la["state"]["q0"], lb["state"]["q0"])
    pl, ll, _ = synth.make_coman_momentum_stack(2, seed=5, linear_momentum=True)
    assert pl.levels[0][2].kind == abi.TASK_GENERIC and pl.levels[0][2].rows == 3 and ll["state"]["linear_momentum"] == (0, 12)
    a, ma = mc.velocity_loop(synth.make_coman_momentum_stack, 2, 3, seed=5, momentum=True)
    b, mb = mc.velocity_loop(synth.make_coman_momentum_stack, 2, 3, seed=5, momentum=False)
    print(f"max|A_ang dq|: with the task {a.max():.3e}, without {b.min():.3e}")
    assert (a < b).all() and ma <= 1e-3 and mb <= 1e-3
    pi, li, mi = synth.make_coman_id_momentum_stack(2, seed=31)
    assert pi.n == 47 and pi.L == 3 and pi.ma(1) == 3 and li["A"][1].shape == (2, 3, 47) and li["state"]["momentum"]["lam"] == 1.0
