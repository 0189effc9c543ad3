"""velocity::ConvexHull restated in numpy (test infrastructure): the support polygon's rows as the reference builds them
(src/constraints/velocity/ConvexHull.cpp:41-134, src/utils/convex_hull_utils.cpp:142-174), one instance at a time, in the reference's
order of operations -- getSupportPolygonPoints in the "COM" frame, the projection on z = 0, getLineCoefficients, getConstraints.

The reference's hull itself comes from PCL / qhull on pcl::PointXYZ (float32 points); PCL is no dependency of this project and the product
works in fp64, so the hull here is a monotone chain in fp64 with the product's predicate: the sign of cross(u, v) = u.x v.y - u.y v.x, exact,
no epsilon.  It is a DIFFERENT algorithm from the kernel's (which looks for every point's counter-clockwise successor): the two agree
where the predicate is unambiguous -- points in general position, and coordinates whose products are exact (dyadic fixtures).

Row order (the product's, OSOT_ROWS_CONVEX_HULL): row r is the edge from the r-th hull vertex in order of POINT INDEX to its
counter-clockwise successor; rows at or beyond the vertex count are the reference's A.setZero() / b = 1e10; fewer than three vertices
leave all rows that way (the reference keeps its previous hull; the update is stateless).

The oracle knows nothing of this row kind, so every comparison with it goes through the GENERIC TWIN of a plan: the same stack with
the hull block replaced by an OSOT_ROWS_GENERIC block carrying the rows written out here."""
import numpy as np

from opensot_amd import abi
from opensot_amd.plan import Rows, StackPlan

INACTIVE_UP, LO = 1.0e10, -1.0e20


def support_polygon_points(points_world, com):
    """convex_hull::getSupportPolygonPoints(..., "COM"): CoM_T_point = world_T_CoM^-1 * world_T_point with world_T_CoM = [I | com]"""
    return np.asarray(points_world, dtype=float) - np.asarray(com, dtype=float)


def project(points):
    """projectPCL2Plane on the plane (0 0 1 0): x and y stay, z = 0"""
    return np.asarray(points, dtype=float)[:, :2].copy()


def cross(u, v):
    return u[0] * v[1] - u[1] * v[0]


def hull_successors(xy):
    """{vertex index: index of its counter-clockwise successor} of the convex hull of xy [P][2]: Andrew's monotone chain on the distinct
    points (a duplicate is represented by its lowest index), popping on cross <= 0 (a point on a segment between two others is no
    vertex).  Empty when fewer than three vertices remain."""
    first = {}
    for i, p in enumerate(xy):
        first.setdefault((float(p[0]), float(p[1])), i)
    pts = sorted(first)                       # lexicographic: x, then y
    if len(pts) < 3:
        return {}

    def turn(o, a, b):
        return cross((a[0] - o[0], a[1] - o[1]), (b[0] - o[0], b[1] - o[1]))

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and turn(h[-2], h[-1], p) <= 0.0:
                h.pop()
            h.append(p)
        return h
    lower, upper = half(pts), half(pts[::-1])
    ring = lower[:-1] + upper[:-1]            # counter-clockwise
    if len(ring) < 3:
        return {}
    idx = [first[p] for p in ring]
    return {idx[k]: idx[(k + 1) % len(idx)] for k in range(len(idx))}


def get_line_coefficients(p0, p1):
    x1, x2, y1, y2 = p0[0], p1[0], p0[1], p1[1]
    a = y1 - y2
    b = x2 - x1
    c = -b * y1 - a * x1
    return a, b, c


def get_constraints(xy, P, margin):
    """ConvexHull::getConstraints over the hull of xy in the product's row order -> (A [P][2], b [P], active rows)"""
    A = np.zeros((P, 2))
    b = np.full(P, INACTIVE_UP)
    succ = hull_successors(xy)
    z = 0
    for i in sorted(succ):
        a_, b_, c_ = get_line_coefficients(xy[i], xy[succ[i]])
        if c_ <= 0.0:
            A[z, 0], A[z, 1], b[z] = +a_, +b_, -c_
        else:
            A[z, 0], A[z, 1], b[z] = -a_, -b_, +c_
        b[z] -= margin * np.sqrt(a_ * a_ + b_ * b_)
        z += 1
    return A, b, z


def hull_rows(J, com, points, margin):
    """one instance: (C [P][n], lo [P], up [P], active rows, xy [P][2]) from the CoM Jacobian J [3][n] (rows 0 and 1 are used: _Aineq =
    _C * _JCoM.block(0, 0, 2, n)), the CoM [3] and the contact points' world positions [P][3]"""
    P = points.shape[0]
    xy = project(support_polygon_points(points, com))
    A, b, z = get_constraints(xy, P, margin)
    return A @ J[:2], np.full(P, LO), b, z, xy


def hull_block(rb, p0, p1, p2, n):
    """(C [B][P][n], lo [B][P], up [B][P], active [B]) of a hull row block rb (plan.Rows) from its leaf inputs"""
    B, P = p0.shape[0], rb.rows
    Cb, lo, up, act = np.zeros((B, P, n)), np.zeros((B, P)), np.zeros((B, P)), np.zeros(B, dtype=int)
    for i in range(B):
        Cb[i], lo[i], up[i], act[i], _ = hull_rows(np.asarray(p0[i], dtype=float).reshape(3, n), p1[i], np.asarray(p2[i], dtype=float).reshape(P, 3),
                                                   rb.bound_scaling)
    return Cb, lo, up, act


def generic_twin(plan, leaf):
    """the same stack with every hull block as OSOT_ROWS_GENERIC rows (C, lo, up) -> (plan, leaf)"""
    blocks, rows, Cl = [], [], []
    Cin = leaf.get("C") or [None] * len(plan.rowblocks)
    for j, rb in enumerate(plan.rowblocks):
        if rb.kind == abi.ROWS_CONVEX_HULL:
            p0, p1, p2 = leaf["rows"][j]
            blocks.append(Rows(abi.ROWS_GENERIC, rb.rows, name=rb.name + "_generic", level=rb.level))
            rows.append(hull_block(rb, p0, p1, p2, plan.n)[:3])
            Cl.append(None)
        else:
            blocks.append(rb)
            rows.append(leaf["rows"][j])
            Cl.append(Cin[j])
    twin = StackPlan(n=plan.n, levels=plan.levels, bounds=plan.bounds, rowblocks=blocks, eps_abs=plan.eps_abs, max_iter=plan.max_iter)
    tleaf = dict(leaf)
    tleaf["rows"], tleaf["C"] = rows, Cl
    return twin, tleaf


def dyadic_cases():
    """degenerate inputs on coordinates that are multiples of 2^-6 (the CoM too), so every product of the predicate and of the line
    coefficients is exact and a contracted multiply-add cannot flip a sign: name -> (points [P][3], com [3], margin, expected number
    of active rows, vertex indices in row order or None)"""
    u = 2.0 ** -6
    z = lambda pts: np.array([[x * u, y * u, 0.25 * (k % 3)] for k, (x, y) in enumerate(pts)])
    com0 = np.array([3 * u, -2 * u, 0.5])
    sq = [(-8, -8), (8, -8), (8, 8), (-8, 8)]
    cases = {
        # duplicated points: the copies of a lower-indexed point are no vertices
        "duplicates": (z([sq[0], sq[1], sq[0], sq[2], sq[3], sq[1], sq[2], sq[3]]), com0, 0.0, 4, [0, 1, 3, 4]),
        # three collinear points on an edge: the middle one (index 1) is no vertex
        "collinear_on_edge": (z([(-8, -8), (0, -8), (8, -8), (8, 8), (-8, 8)]), com0, 0.0, 4, [0, 2, 3, 4]),
        # an interior point and points out of angular order
        "shuffled": (z([(8, 8), (1, 1), (-8, -8), (-8, 8), (8, -8), (0, 3)]), com0, 0.0, 4, [0, 2, 3, 4]),
        "all_collinear": (z([(-8, -4), (0, 0), (8, 4), (4, 2), (-4, -2)]), com0, 0.0, 0, None),
        "all_coincident": (z([(5, 5)] * 4), com0, 0.0, 0, None),
        # the CoM exactly on the bottom edge: c == 0 there, the `<=` branch keeps (a, b)
        "com_on_edge": (z(sq), np.array([2 * u, -8 * u, 0.5]), 0.0, 4, [0, 1, 2, 3]),
        # the CoM outside the polygon (beyond the right edge): that row comes out flipped, as the reference produces it
        "com_outside": (z(sq), np.array([12 * u, 1 * u, 0.5]), 0.0, 4, [0, 1, 2, 3]),
        # a margin larger than the distance to an edge: a negative upper bound
        "margin_beyond_edge": (z(sq), np.array([6 * u, 0.0, 0.5]), 4 * u, 4, [0, 1, 2, 3]),
    }
    return cases


def dyadic_batch(P=8):
    """the dyadic cases as ONE batch of P points per instance (short cases are filled with copies of their first point: duplicates of a
    lower index are dropped) -> names, points [B][P][3], com [B][3], active rows [B]; margin 0 except where a case sets one, so the
    batch is returned per margin"""
    out = {}
    for name, (pts, com, margin, nact, _) in dyadic_cases().items():
        fill = np.repeat(pts[:1], P - len(pts), axis=0)
        out.setdefault(margin, []).append((name, np.concatenate([pts, fill]), com, nact))
    return out
