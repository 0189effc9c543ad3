"""tests/convex_ref.py -- TEST INFRASTRUCTURE ONLY (numpy): what the convex collision shapes are checked against.

A CERTIFICATE, not a second solver.  For every core kind: the support function h(n) = max over the core of n . x, a membership
test, and certify(A, B, ca, cb):
  1. ca is a point of A and cb a point of B (to 1e-12): |ca - cb| bounds the distance FROM ABOVE;
  2. with n = (ca - cb) / |ca - cb| the slab -(h_A(-n) + h_B(n)) = min_A n.x - max_B n.x separates the cores: it bounds the distance
     FROM BELOW.
Both within `gap` of each other prove the distance to `gap`, whatever produced the witnesses.  The certificate itself is checked
(tests/test_convex_shapes_host.py) against brute_force_distance: the minimum over the surface triangles of two polytopes of the
closed-form vertex / triangle and edge / edge distances.

A shape is a dict: kind ("capsule" | "box" | "cylinder" | "hull"), size[3] (capsule: (-, -, half length); box: half extents;
cylinder: (radius, -, half length)), radius (rounding), verts [nv][3]; a pose is (R[3][3], p[3]) = world_T_shape."""
import numpy as np


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def support(shape, pose, n):
    """h(n): the largest n . x over the CORE (the rounding radius is not part of it)"""
    R, p = pose
    l = R.T @ n
    k, s = shape["kind"], np.asarray(shape.get("size", np.zeros(3)), float)
    if k == "capsule":
        return float(n @ p + s[2] * abs(l[2]))
    if k == "box":
        return float(n @ p + s @ np.abs(l))
    if k == "cylinder":
        return float(n @ p + s[2] * abs(l[2]) + s[0] * np.hypot(l[0], l[1]))
    return float(n @ p + (np.asarray(shape["verts"], float) @ l).max())


def _hull_violation(V, x):
    """how far x is from the convex hull of the rows of V (0 = a member)"""
    from scipy.optimize import nnls
    from scipy.spatial import ConvexHull, QhullError
    V = np.unique(np.asarray(V, float).reshape(-1, 3), axis=0)
    if len(V) >= 4:
        try:
            eq = ConvexHull(V).equations          # unit normals: rows [a | b], a . x + b <= 0 inside
            return float(max(0.0, (eq[:, :3] @ x + eq[:, 3]).max()))
        except QhullError:
            pass
    # a flat hull (a point, a segment, a polygon): least squares over the simplex lambda >= 0, sum lambda = 1
    A = np.vstack([V.T, np.ones((1, len(V)))])
    lam, res = nnls(A, np.concatenate([x, [1.0]]))
    return float(res)


def violation(shape, pose, x):
    """0 for a point of the core, else (about) its distance to it"""
    R, p = pose
    l = R.T @ (np.asarray(x, float) - p)
    k, s = shape["kind"], np.asarray(shape.get("size", np.zeros(3)), float)
    if k == "capsule":
        return float(max(abs(l[0]), abs(l[1]), abs(l[2]) - s[2], 0.0))
    if k == "box":
        return float(max((np.abs(l) - s).max(), 0.0))
    if k == "cylinder":
        return float(max(np.hypot(l[0], l[1]) - s[0], abs(l[2]) - s[2], 0.0))
    return _hull_violation(shape["verts"], l)


def certify(A, poseA, B, poseB, ca, cb):
    """-> dict(len = |ca - cb|, slab = the separating slab along ca - cb, gap = len - slab, in_a, in_b = membership violations)"""
    ca, cb = np.asarray(ca, float), np.asarray(cb, float)
    ln = float(np.linalg.norm(ca - cb))
    n = (ca - cb) / ln
    slab = -(support(A, poseA, -n) + support(B, poseB, n))
    return dict(len=ln, slab=slab, gap=ln - slab, in_a=violation(A, poseA, ca), in_b=violation(B, poseB, cb))


# ---- brute force for polytopes -----------------------------------------------------------------------------------------------
def world_vertices(shape, pose):
    R, p = pose
    k, s = shape["kind"], np.asarray(shape.get("size", np.zeros(3)), float)
    if k == "capsule":
        L = np.array([[0, 0, -s[2]], [0, 0, s[2]]])
    elif k == "box":
        L = np.array([[sx * s[0], sy * s[1], sz * s[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    elif k == "hull":
        L = np.asarray(shape["verts"], float).reshape(-1, 3)
    else:
        raise ValueError("a cylinder is not a polytope")
    return L @ R.T + p


def _triangles(V):
    from scipy.spatial import ConvexHull
    if len(V) == 2:
        return V[[0, 1, 1]][None]               # a segment: one degenerate triangle
    return V[ConvexHull(V).simplices]           # [m][3][3]


def _point_segment(P, A, B):
    """[n][m] distances of the points P[n] to the segments A[m] B[m]"""
    d = B - A
    dd = np.einsum("mi,mi->m", d, d)
    t = np.einsum("nmi,mi->nm", P[:, None] - A[None], d) / np.where(dd > 0, dd, 1.0)
    t = np.clip(np.where(dd > 0, t, 0.0), 0.0, 1.0)
    return np.linalg.norm(P[:, None] - (A[None] + t[..., None] * d[None]), axis=2)


def _point_triangle(P, T):
    """[n][m] distances of the points P[n] to the triangles T[m][3][3]: the foot of the perpendicular where it falls inside, else
    the nearest edge"""
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    out = np.minimum(np.minimum(_point_segment(P, a, b), _point_segment(P, b, c)), _point_segment(P, c, a))
    e1, e2 = b - a, c - a
    nrm = np.cross(e1, e2)
    nn = np.einsum("mi,mi->m", nrm, nrm)
    ok = nn > 1e-30
    w = P[:, None] - a[None]
    g11, g12, g22 = np.einsum("mi,mi->m", e1, e1), np.einsum("mi,mi->m", e1, e2), np.einsum("mi,mi->m", e2, e2)
    r1, r2 = np.einsum("nmi,mi->nm", w, e1), np.einsum("nmi,mi->nm", w, e2)
    det = np.where(ok, g11 * g22 - g12 * g12, 1.0)
    u, v = (r1 * g22 - r2 * g12) / det, (g11 * r2 - g12 * r1) / det
    inside = ok[None] & (u >= 0) & (v >= 0) & (u + v <= 1)
    plane = np.abs(np.einsum("nmi,mi->nm", w, nrm)) / np.sqrt(np.where(ok, nn, 1.0))
    return np.where(inside, plane, out)


def _segment_segment(A0, A1, B0, B1):
    """[n][m] distances of the segments A[n] and B[m]: an end point against the other segment, or the common perpendicular where
    its feet lie inside both"""
    out = np.minimum(np.minimum(_point_segment(A0, B0, B1), _point_segment(A1, B0, B1)),
                     np.minimum(_point_segment(B0, A0, A1), _point_segment(B1, A0, A1)).T)
    d1, d2 = (A1 - A0)[:, None], (B1 - B0)[None]
    r = A0[:, None] - B0[None]
    a, e, b = (d1 * d1).sum(2), (d2 * d2).sum(2), (d1 * d2).sum(2)
    c, f = (d1 * r).sum(2), (d2 * r).sum(2)
    den = a * e - b * b
    ok = den > 1e-14 * a * e
    den = np.where(ok, den, 1.0)
    s, t = (b * f - c * e) / den, (a * f - b * c) / den
    inside = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    perp = np.linalg.norm(r + s[..., None] * d1 - t[..., None] * d2, axis=2)
    return np.where(inside, perp, out)


def brute_force_distance(A, poseA, B, poseB):
    """distance of two SEPARATED polytope cores (segment, box, hull): min over the pairs of surface triangles"""
    VA, VB = world_vertices(A, poseA), world_vertices(B, poseB)
    TA, TB = _triangles(VA), _triangles(VB)
    best = min(_point_triangle(VA, TB).min(), _point_triangle(VB, TA).min())
    edges = lambda T: (np.concatenate([T[:, 0], T[:, 1], T[:, 2]]), np.concatenate([T[:, 1], T[:, 2], T[:, 0]]))
    (a0, a1), (b0, b1) = edges(TA), edges(TB)
    return float(min(best, _segment_segment(a0, a1, b0, b1).min()))


# ---- random cases ------------------------------------------------------------------------------------------------------------
KINDS = ("sphere", "capsule", "box", "rounded_box", "cylinder", "hull4", "hull16", "hull32")


def random_shape(name, rng, lo=0.03, hi=0.3):
    """one of KINDS with sizes in [lo, hi] metres"""
    u = lambda: float(rng.uniform(lo, hi))
    if name == "sphere":
        return dict(kind="capsule", size=np.zeros(3), radius=u())
    if name == "capsule":
        return dict(kind="capsule", size=np.array([0.0, 0.0, u()]), radius=0.5 * u())
    if name == "box":
        return dict(kind="box", size=np.array([u(), u(), u()]), radius=0.0)
    if name == "rounded_box":
        return dict(kind="box", size=np.array([u(), u(), u()]), radius=0.3 * u())
    if name == "cylinder":
        return dict(kind="cylinder", size=np.array([u(), 0.0, u()]), radius=0.0)
    nv = int(name[4:])
    return dict(kind="hull", size=np.zeros(3), radius=0.0, verts=rng.uniform(-1.0, 1.0, (nv, 3)) * np.array([u(), u(), u()]))


def bounding_radius(shape):
    k, s = shape["kind"], np.asarray(shape.get("size", np.zeros(3)), float)
    if k == "capsule":
        return s[2]
    if k == "box":
        return float(np.linalg.norm(s))
    if k == "cylinder":
        return float(np.hypot(s[0], s[2]))
    return float(np.linalg.norm(shape["verts"], axis=1).max())


def random_separated_pair(ka, kb, rng, min_sep=0.01):
    """two shapes and poses whose CORES are at least min_sep apart: the second one is pushed away along a random direction until a
    separating slab of that width exists"""
    A, B = random_shape(ka, rng), random_shape(kb, rng)
    poseA = (random_rotation(rng), rng.uniform(-0.5, 0.5, 3))
    RB = random_rotation(rng)
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    side = rng.normal(size=3) * 0.1
    # along n: h_A(n) + want + h_B(-n) puts B's core exactly `want` behind A's in that direction
    want = min_sep + float(rng.uniform(0.0, 0.3))
    pB = np.zeros(3)
    off = support(A, poseA, n) + want + support(B, (RB, pB), -n)
    base = poseA[1] + side                       # ... and beside A's centre by a few centimetres
    pB = n * off + (base - n * (base @ n))
    return A, poseA, B, (RB, pB)
