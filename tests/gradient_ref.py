"""tests/gradient_ref.py -- TEST INFRASTRUCTURE ONLY: the reference's posture gradients by brute force.

What tasks::velocity::Manipulability::_update (Manipulability.cpp:58-84) and MinimumEffort::_update (MinimumEffort.cpp:51-77) do:
for every active joint i the WHOLE model is evaluated at q + step e_i and at q - step e_i, the worker's cost is computed from the
Jacobian (sqrt(fabs(det(J W J'))), Manipulability.h:145-150) or from the gravity compensation (tau' W tau, MinimumEffort.h:89-96),
and grad[i] = (f+ - f-) / (2 step);  b = lambda grad  /  b = -1.0 lambda grad.  This is deliberately NOT the kernel's route (one
forward kinematics and a rigid motion per perturbed joint, opensot_amd/csrc/osot_grad.h).

Two engines evaluate the model:
  "pykin"   -- 2 n calls of oracle.pykin.forward per instance, numpy.linalg.det: float64 only (pykin stores float64)
  "batched" -- the same forward kinematics written once for a whole array of configurations and for any dtype: all 2 n B perturbed
               postures in one pass.  It is what runs in numpy.longdouble as the arbiter, and in float64 where 2 n B calls of
               pykin.forward would take minutes (B = 257).  tests/test_posture_gradient_host.py checks it against pykin.forward.
A term is a dict: kind (abi.GRAD_*), frame (index, MANIPULABILITY_FRAME), step, lam, W (n weights), active (list of joints or None)."""
import numpy as np

from opensot_amd import abi
from oracle import pykin


def term(kind, frame=0, step=1e-3, lam=1.0, W=None, active=None):
    return dict(kind=kind, frame=frame, step=step, lam=lam, W=W, active=active)


def _ancestors(model):
    anc = []
    for j in range(model.n):
        anc.append({j} | (anc[model.parent[j]] if model.parent[j] >= 0 else set()))
    return anc


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def forward_batched(model, Q, dtype=np.float64):
    """oracle.pykin.forward for an array of configurations Q [N][n], in `dtype`: dict(frame_R [F][N][3][3], frame_p [F][N][3],
    J [F][N][6][n] (world), Jcom [N][3][n])"""
    Q = np.asarray(Q, dtype=dtype)
    N, n = Q.shape
    one = dtype(1.0)
    ax, R0, p0 = np.asarray(model.axis, dtype=dtype), np.asarray(model.R0, dtype=dtype), np.asarray(model.p0, dtype=dtype)
    mass, com = np.asarray(model.mass, dtype=dtype), np.asarray(model.com, dtype=dtype)
    Rw, pw = np.zeros((N, n, 3, 3), dtype=dtype), np.zeros((N, n, 3), dtype=dtype)
    for j in range(n):
        if model.jtype[j] == 0:
            x, y, z = ax[j]
            c, s = np.cos(Q[:, j]), np.sin(Q[:, j])
            v = one - c
            Rq = np.stack([np.stack([c + x * x * v, x * y * v - z * s, x * z * v + y * s], -1),
                           np.stack([y * x * v + z * s, c + y * y * v, y * z * v - x * s], -1),
                           np.stack([z * x * v - y * s, z * y * v + x * s, c + z * z * v], -1)], -2)
            Rl = np.einsum("ab,Nbc->Nac", R0[j], Rq)
            pl = np.broadcast_to(p0[j], (N, 3))
        else:
            Rl = np.broadcast_to(R0[j], (N, 3, 3))
            pl = p0[j] + (R0[j] @ ax[j]) * Q[:, j, None]
        a = model.parent[j]
        if a < 0:
            Rw[:, j], pw[:, j] = Rl, pl
        else:
            Rw[:, j] = np.einsum("Nab,Nbc->Nac", Rw[:, a], Rl)
            pw[:, j] = np.einsum("Nab,Nb->Na", Rw[:, a], pl) + pw[:, a]
    z = np.einsum("Njab,jb->Nja", Rw, ax)
    cw = np.einsum("Njab,jb->Nja", Rw, com) + pw
    anc = _ancestors(model)
    out = dict(frame_R=[], frame_p=[], J=[])
    for (_, jf, Rf, pf) in model.frames:
        R = np.einsum("Nab,bc->Nac", Rw[:, jf], np.asarray(Rf, dtype=dtype))
        p = pw[:, jf] + np.einsum("Nab,b->Na", Rw[:, jf], np.asarray(pf, dtype=dtype))
        J = np.zeros((N, 6, n), dtype=dtype)
        for j in anc[jf]:
            if model.jtype[j] == 0:
                J[:, :3, j] = _cross(z[:, j], p - pw[:, j]); J[:, 3:, j] = z[:, j]
            else:
                J[:, :3, j] = z[:, j]
        out["frame_R"].append(R); out["frame_p"].append(p); out["J"].append(J)
    Jc = np.zeros((N, 3, n), dtype=dtype)
    for l in range(n):
        if mass[l] == 0:
            continue
        for j in anc[l]:
            if model.jtype[j] == 0:
                Jc[:, :, j] += mass[l] * _cross(z[:, j], cw[:, l] - pw[:, j])
            else:
                Jc[:, :, j] += mass[l] * z[:, j]
    out["Jcom"] = Jc / mass.sum()
    return out


def _relative_batched(fk, f, g):
    """oracle.pykin.relative for the batched dict: the Jacobian of frame f relative to frame g, in g's coordinates"""
    Jd, Jb = fk["J"][f], fk["J"][g]
    d = fk["frame_p"][f] - fk["frame_p"][g]
    # skew(p_d - p_b) J_b,angular, column by column
    lin = Jd[:, :3] - Jb[:, :3] + np.swapaxes(_cross(d[:, None, :], np.swapaxes(Jb[:, 3:], 1, 2)), 1, 2)
    ang = Jd[:, 3:] - Jb[:, 3:]
    Rb = fk["frame_R"][g]
    return np.concatenate([np.einsum("Nba,Nbj->Naj", Rb, lin), np.einsum("Nba,Nbj->Naj", Rb, ang)], axis=1)


def det_any(A):
    """determinant of one square matrix in its own dtype (numpy.linalg.det computes in float64): elimination with partial pivoting"""
    A = np.array(A)
    if A.dtype == np.float64:
        return np.linalg.det(A)
    m = A.shape[0]
    det = A.dtype.type(1.0)
    for k in range(m):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if A[p, k] == 0:
            return A.dtype.type(0.0)
        if p != k:
            A[[k, p]] = A[[p, k]]
            det = -det
        det = det * A[k, k]
        A[k + 1:, k:] -= np.outer(A[k + 1:, k] / A[k, k], A[k, k:])
    return det


def frame_base_of(model, f):
    g = model.frame_base.get(f)
    if g is None:
        return None
    return model.frame_index(g) if isinstance(g, str) else int(g)


def jacobian_of(model, fk, t, batched):
    """the worker's Cartesian / CoM task matrix for term t from a forward-kinematics result (one configuration, or the batched dict)"""
    if t["kind"] == abi.GRAD_MANIPULABILITY_COM:
        return fk["Jcom"]
    f, g = t["frame"], frame_base_of(model, t["frame"])
    if g is None:
        return fk["J"][f]
    return _relative_batched(fk, f, g) if batched else pykin.relative(fk, f, g)[2]


def gram(J, W):
    """J W J' (diagonal W), the last two axes"""
    return np.einsum("...aj,j,...bj->...ab", J, W, J)


def _cost_from(model, fk, t, gravity, dtype, batched):
    """the worker's cost at every configuration of fk: array [N] (batched) or a scalar"""
    W = np.ones(model.n, dtype=dtype) if t["W"] is None else np.asarray(t["W"], dtype=dtype)
    if t["kind"] == abi.GRAD_MIN_EFFORT:
        tau = -np.asarray(model.mass, dtype=dtype).sum() * np.einsum("...aj,a->...j", fk["Jcom"], np.asarray(gravity, dtype=dtype))
        return np.einsum("...j,j,...j->...", tau, W, tau)
    G = gram(jacobian_of(model, fk, t, batched), W)
    if batched:
        if dtype == np.float64:
            return np.sqrt(np.abs(np.linalg.det(G)))
        return np.sqrt(np.abs(np.array([det_any(g) for g in G], dtype=dtype)))
    return np.sqrt(np.abs(det_any(G)))


def costs(model, Q, terms, gravity, dtype=np.float64, engine="batched"):
    """f of every term at every configuration of Q [N][n]: [T][N]"""
    Q = np.asarray(Q, dtype=dtype)
    if engine == "batched":
        fk = forward_batched(model, Q, dtype)
        return np.stack([_cost_from(model, fk, t, gravity, dtype, True) for t in terms])
    assert dtype == np.float64, "oracle.pykin.forward computes in float64"
    out = np.zeros((len(terms), len(Q)))
    for k, q in enumerate(Q):
        fk = pykin.forward(model, q)
        for ti, t in enumerate(terms):
            out[ti, k] = _cost_from(model, fk, t, gravity, dtype, False)
    return out


def gradients(model, q, terms, gravity=(0.0, 0.0, -9.81), dtype=np.float64, engine="pykin"):
    """the reference's loop for a batch q [B][n]: dict(b [T][B][n], value [T][B], fp, fm [T][B][n] (the two costs of every joint),
    scale [T][B] = max(|f+|, |f-|) / (2 step): the cancellation scale the tolerances are stated in, lam [T])"""
    q = np.asarray(q, dtype=dtype)
    B, n = q.shape
    T = len(terms)
    steps = sorted({t["step"] for t in terms})
    fp, fm = np.zeros((T, B, n), dtype=dtype), np.zeros((T, B, n), dtype=dtype)
    for st in steps:
        sel = [i for i, t in enumerate(terms) if t["step"] == st]
        d = dtype(st) * np.eye(n, dtype=dtype)
        Qp = (q[:, None, :] + d[None]).reshape(B * n, n)          # model.sum(q, deltas): plain addition
        Qm = (q[:, None, :] - d[None]).reshape(B * n, n)
        cp = costs(model, Qp, [terms[i] for i in sel], gravity, dtype, engine)
        cm = costs(model, Qm, [terms[i] for i in sel], gravity, dtype, engine)
        for k, i in enumerate(sel):
            fp[i], fm[i] = cp[k].reshape(B, n), cm[k].reshape(B, n)
    value = costs(model, q, terms, gravity, dtype, engine)
    b = np.zeros((T, B, n), dtype=dtype)
    scale = np.zeros((T, B), dtype=dtype)
    for i, t in enumerate(terms):
        two_step = dtype(2.0) * dtype(t["step"])
        grad = (fp[i] - fm[i]) / two_step
        if t["active"] is not None:
            off = np.ones(n, dtype=bool); off[list(t["active"])] = False
            grad[:, off] = 0
        lam = dtype(t["lam"])
        b[i] = -dtype(1.0) * lam * grad if t["kind"] == abi.GRAD_MIN_EFFORT else lam * grad
        scale[i] = np.maximum(np.abs(fp[i]), np.abs(fm[i])).max(axis=1) / two_step
    return dict(b=b, value=value, fp=fp, fm=fm, scale=scale, lam=np.array([t["lam"] for t in terms], dtype=np.float64))


def cond_ok(model, q, terms, cap=1e4):
    """True where cond(J W J') <= cap at q for every manipulability term (the draw is kept)"""
    fk = pykin.forward(model, q)
    for t in terms:
        if t["kind"] == abi.GRAD_MIN_EFFORT:
            continue
        W = np.ones(model.n) if t["W"] is None else np.asarray(t["W"], dtype=float)
        if not np.linalg.cond(gram(jacobian_of(model, fk, t, False), W)) <= cap:
            return False
    return True


def draw(model, terms, B, seed, cap=1e4, lo=-0.8, hi=0.8):
    """B configurations from U(lo, hi), reject-sampled on the CPU until every one meets the condition cap: (q [B][n], draws made)"""
    rng = np.random.default_rng(seed)
    out, tries = [], 0
    while len(out) < B:
        q = rng.uniform(lo, hi, model.n)
        tries += 1
        assert tries <= 50 * B, "the geometry cannot meet the condition cap: change the geometry, not the cap"
        if cond_ok(model, q, terms, cap):
            out.append(q)
    return np.array(out), tries
