// osot_convex.h -- closest points of two convex cores by GJK, per lane: no cross-lane operation, no LDS, no barrier.
// Plain C++ (no HIP): the kinematics producer's CONVEX instantiation (osot_kin.h, stage 5) calls it from a lane, the host calls
// it from osot_shape_distance and tools/convex_fuzz.cpp.  What the reference's collision module (FCL behind xbot2) computes for
// the shapes a URDF declares (src/constraints/velocity/CollisionAvoidance.cpp:96-200).
//
// A CORE is a convex set in its own frame (R, p: world_T_shape); the shape is the core grown by a rounding radius r >= 0, which
// GJK never sees:  distance = |ca - cb| - r_a - r_b  with the witnesses ca, cb ON THE CORES (the convention of the closed forms).
//   segment   mid point p, half vector s (world): capsule (r > 0) and sphere (s = 0)
//   box       half extents s, sharp (r = 0) or rounded
//   cylinder  axis = z of the shape frame, s = (radius, -, half length): axis term + rim term
//   hull      convex hull of nv = 1 .. 32 vertices (shape frame): arg-max over the vertices
//
// GJK on the Minkowski difference A - B in double precision.  Every simplex vertex keeps BOTH its witnesses, so ca and cb are the
// same barycentric combination as v.  The distance step is the brute-force form of Johnson's sub-algorithm: the origin is
// projected onto the affine hull of every sub-simplex (1 + .. = 15 at most), a projection with barycentric coordinates >= 0 is a
// point of the simplex, and the shortest of those IS the closest point -- no sign tests on a recursion of determinants, a
// degenerate (flat) sub-simplex is skipped and its faces answer for it.
//
// STOPPING RULE (DESIGN.md "Convex collision shapes"): with v the closest point so far and w = s_A(-v) - s_B(v),
//   1. |v|^2 - v.w <= kGjkRelGap |v|^2          (v.w / |v| is a separating slab: a lower bound of the distance)
//   2. w is already a vertex of the simplex, or does not enter the closest sub-simplex (it would come back next round)
//   3. the simplex encloses the origin, or |v| <= kGjkTouch: the cores intersect -- no normal, witnesses coincide
//   4. kGjkMaxIter support evaluations
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define OSOT_CVX_FN __host__ __device__ inline
#else
#define OSOT_CVX_FN inline
#endif

namespace osot {

constexpr double kGjkRelGap = 1.0e-13;   // relative duality gap of rule 1
constexpr int kGjkMaxIter = 96;          // rule 4 (host run, DESIGN.md: at most 9 for polytopes, a few dozen with a cylinder's rim)
constexpr double kGjkTouch = 1.0e-12;    // |ca - cb| at or below this: the cores touch or intersect (stage 5's "no direction" threshold)
constexpr int kGjkMaxHull = 32;          // vertices of one hull

enum { CVX_SEGMENT = 0, CVX_BOX = 1, CVX_CYLINDER = 2, CVX_HULL = 3 };   // = OSOT_SHAPE_* (a capsule's core is a segment)

struct ConvexCore {
    int kind;
    double R[9], p[3];       // world_T_shape, R row-major (a segment: R unused, p = mid point)
    double s[3];             // segment: half vector in the WORLD; box: half extents; cylinder: (radius, -, half length)
    const double* v;         // hull: nv vertices [nv][3] in the shape frame
    int nv;
};

struct GjkResult {
    double ca[3], cb[3];     // witnesses on the cores (world); equal when the cores intersect
    double len;              // |ca - cb|; 0 when the cores intersect
    int iterations;          // support evaluations
    int intersect;           // rule 3
    int capped;              // rule 4 ended the run
};

// a segment core from its end points in the world
OSOT_CVX_FN void convex_segment(ConvexCore& c, const double* e0, const double* e1) {
    c.kind = CVX_SEGMENT; c.v = nullptr; c.nv = 0;
    for (int i = 0; i < 9; ++i) c.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) { c.p[i] = 0.5 * (e0[i] + e1[i]); c.s[i] = 0.5 * (e1[i] - e0[i]); }
}

// support point of a core in the world direction d (any length, may be zero): the point of the core furthest along d
OSOT_CVX_FN void convex_support(const ConvexCore& c, const double* d, double* out) {
    if (c.kind == CVX_SEGMENT) {
        const double sg = (d[0] * c.s[0] + d[1] * c.s[1] + d[2] * c.s[2]) >= 0.0 ? 1.0 : -1.0;
        for (int i = 0; i < 3; ++i) out[i] = c.p[i] + sg * c.s[i];
        return;
    }
    double l[3], q[3];       // R' d, the support point in the shape frame
    for (int i = 0; i < 3; ++i) l[i] = c.R[i] * d[0] + c.R[3 + i] * d[1] + c.R[6 + i] * d[2];
    if (c.kind == CVX_BOX) {
        for (int i = 0; i < 3; ++i) q[i] = l[i] >= 0.0 ? c.s[i] : -c.s[i];
    } else if (c.kind == CVX_CYLINDER) {
        const double rho = sqrt(l[0] * l[0] + l[1] * l[1]);
        const double k = rho > 0.0 ? c.s[0] / rho : 0.0;      // (a direction along the axis: any rim point, the centre is one)
        q[0] = k * l[0]; q[1] = k * l[1]; q[2] = l[2] >= 0.0 ? c.s[2] : -c.s[2];
    } else {
        int best = 0;
        double hb = c.v[0] * l[0] + c.v[1] * l[1] + c.v[2] * l[2];
        for (int k = 1; k < c.nv; ++k) {
            const double h = c.v[3 * k] * l[0] + c.v[3 * k + 1] * l[1] + c.v[3 * k + 2] * l[2];
            if (h > hb) { hb = h; best = k; }
        }
        for (int i = 0; i < 3; ++i) q[i] = c.v[3 * best + i];
    }
    for (int i = 0; i < 3; ++i) out[i] = c.R[3 * i] * q[0] + c.R[3 * i + 1] * q[1] + c.R[3 * i + 2] * q[2] + c.p[i];
}

OSOT_CVX_FN double cvx_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// One candidate of the distance step: the barycentric coordinates l[0 .. m-1] of the projection of the origin onto the affine
// hull of y_0 .. y_{m-1} (m = 1 .. 4).  False: the sub-simplex is flat (its faces are candidates of their own) or the
// projection lies outside it.
OSOT_CVX_FN bool cvx_project(const int m, const double* y0, const double* y1, const double* y2, const double* y3, double* l) {
    const double flat = 1.0e-28;      // squared sine / volume ratio below which a sub-simplex counts as flat (double: 1e-32 is noise)
    if (m == 1) { l[0] = 1.0; return true; }
    double e1[3], e2[3], e3[3];
    for (int i = 0; i < 3; ++i) { e1[i] = y1[i] - y0[i]; e2[i] = (m > 2) ? y2[i] - y0[i] : 0.0; e3[i] = (m > 3) ? y3[i] - y0[i] : 0.0; }
    const double g11 = cvx_dot(e1, e1), b1 = -cvx_dot(y0, e1);
    if (m == 2) {
        if (!(g11 > 0.0)) return false;
        const double t = b1 / g11;
        l[0] = 1.0 - t; l[1] = t;
        return t >= 0.0 && t <= 1.0;
    }
    if (m == 3) {
        // The 2 x 2 normal equations from the vertex OPPOSITE THE LONGEST EDGE.  Near the end of a run against a cylinder's rim
        // the triangles are needles (two support points 1e-6 apart): from the far vertex the two edges are parallel to 1e-5, the
        // determinant cancels to 1e-10 of its terms and the projection is off by 1e-7 -- the run then stalls at a gap of 1e-9.
        // From an end of the short edge the angle is the triangle's largest and the system is as well conditioned as it gets.
        double e0[3];
        for (int i = 0; i < 3; ++i) e0[i] = y2[i] - y1[i];
        const double n0 = cvx_dot(e0, e0), n1 = cvx_dot(e2, e2), n2 = g11;      // squared edge opposite y0, y1, y2
        const int base = (n0 >= n1 && n0 >= n2) ? 0 : (n1 >= n2 ? 1 : 2);
        double q0[3], f1[3], f2[3];
        for (int i = 0; i < 3; ++i) {
            q0[i] = base == 0 ? y0[i] : (base == 1 ? y1[i] : y2[i]);
            f1[i] = (base == 0 ? y1[i] : (base == 1 ? y2[i] : y0[i])) - q0[i];
            f2[i] = (base == 0 ? y2[i] : (base == 1 ? y0[i] : y1[i])) - q0[i];
        }
        const double h11 = cvx_dot(f1, f1), h12 = cvx_dot(f1, f2), h22 = cvx_dot(f2, f2), c1 = -cvx_dot(q0, f1), c2 = -cvx_dot(q0, f2);
        const double det = h11 * h22 - h12 * h12;
        if (!(det > flat * h11 * h22)) return false;
        const double u = (c1 * h22 - c2 * h12) / det, w = (h11 * c2 - h12 * c1) / det, t = 1.0 - u - w;
        l[0] = base == 0 ? t : (base == 1 ? w : u);
        l[1] = base == 0 ? u : (base == 1 ? t : w);
        l[2] = base == 0 ? w : (base == 1 ? u : t);
        return t >= 0.0 && u >= 0.0 && w >= 0.0;
    }
    const double g22 = cvx_dot(e2, e2);
    // m == 4: [e1 e2 e3] x = -y0 by Cramer's rule
    const double g33 = cvx_dot(e3, e3);
    const double c23[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
    const double c31[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
    const double c12[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double det = cvx_dot(e1, c23);
    if (!(det * det > flat * g11 * g22 * g33)) return false;
    const double x1 = -cvx_dot(y0, c23) / det, x2 = -cvx_dot(y0, c31) / det, x3 = -cvx_dot(y0, c12) / det;
    l[0] = 1.0 - x1 - x2 - x3; l[1] = x1; l[2] = x2; l[3] = x3;
    return l[0] >= 0.0 && x1 >= 0.0 && x2 >= 0.0 && x3 >= 0.0;
}

// closest points of two cores.  The simplex lives in four fixed slots with a bit mask of the ones in use; every loop over the
// slots and over the sub-simplices has constant bounds, so on the device the slots are registers, not indexed memory.
OSOT_CVX_FN void gjk_closest(const ConvexCore& A, const ConvexCore& B, GjkResult& out) {
    double Y[4][3], WA[4][3], WB[4][3], lam[4] = {1.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < 4; ++s)
        for (int i = 0; i < 3; ++i) { Y[s][i] = 0.0; WA[s][i] = 0.0; WB[s][i] = 0.0; }
    double v[3];
    {
        double d[3] = {A.p[0] - B.p[0], A.p[1] - B.p[1], A.p[2] - B.p[2]}, nd[3];
        if (!(cvx_dot(d, d) > 0.0)) { d[0] = 1.0; d[1] = 0.0; d[2] = 0.0; }
        for (int i = 0; i < 3; ++i) nd[i] = -d[i];
        convex_support(A, nd, WA[0]);
        convex_support(B, d, WB[0]);
        for (int i = 0; i < 3; ++i) { Y[0][i] = WA[0][i] - WB[0][i]; v[i] = Y[0][i]; }
    }
    unsigned act = 1u;
    int it = 0, hit = 0, capped = 0;
    for (;;) {
        const double vv = cvx_dot(v, v);
        if (!(vv > kGjkTouch * kGjkTouch)) { hit = 1; break; }                 // rule 3 (touching)
        if (it >= kGjkMaxIter) { capped = 1; break; }                          // rule 4
        ++it;
        double wa[3], wb[3], w[3];
        const double nv_[3] = {-v[0], -v[1], -v[2]};
        convex_support(A, nv_, wa);
        convex_support(B, v, wb);
        for (int i = 0; i < 3; ++i) w[i] = wa[i] - wb[i];
        if (vv - cvx_dot(v, w) <= kGjkRelGap * vv) break;                      // rule 1
        bool seen = false;
        int slot = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int s = 3; s >= 0; --s) {
            const bool used = ((act >> s) & 1u) != 0u;
            seen = seen || (used && w[0] == Y[s][0] && w[1] == Y[s][1] && w[2] == Y[s][2]);
            slot = used ? slot : s;
        }
        if (seen) break;                                                       // rule 2
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int s = 0; s < 4; ++s)
            if (s == slot)
                for (int i = 0; i < 3; ++i) { Y[s][i] = w[i]; WA[s][i] = wa[i]; WB[s][i] = wb[i]; }
        const unsigned all = act | (1u << slot);
        // distance step: every sub-simplex of the slots in use
        double best = INFINITY, bl[4] = {0.0, 0.0, 0.0, 0.0};
        unsigned bmask = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (unsigned mk = 1u; mk < 16u; ++mk) {
            if ((mk & ~all) != 0u) continue;
            const double* y[4] = {Y[0], Y[0], Y[0], Y[0]};
            int idx[4] = {0, 0, 0, 0}, m = 0;
            for (int s = 0; s < 4; ++s)
                if ((mk >> s) & 1u) { y[m] = Y[s]; idx[m] = s; ++m; }
            double l[4] = {0.0, 0.0, 0.0, 0.0};
            if (!cvx_project(m, y[0], y[1], y[2], y[3], l)) continue;
            double c[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < 4; ++k)
                if (k < m)
                    for (int i = 0; i < 3; ++i) c[i] += l[k] * y[k][i];
            // (|c|^2 of the point the coordinates really give, also for a tetrahedron around the origin: an ill-conditioned solve
            //  can then only lose to a face, never claim a distance the simplex does not have)
            const double cc = cvx_dot(c, c);
            if (cc < best) {
                best = cc; bmask = mk;
                for (int s = 0; s < 4; ++s) bl[s] = 0.0;
                for (int k = 0; k < 4; ++k)
                    if (k < m)
                        for (int s = 0; s < 4; ++s) bl[s] = (s == idx[k]) ? l[k] : bl[s];
            }
        }
        if (bmask == 0u) break;                    // (cannot happen: a vertex always projects) keep the last closest point
        if (!((bmask >> slot) & 1u)) break;        // rule 2: w does not enter the closest sub-simplex; the last v stands
        act = bmask;
        for (int s = 0; s < 4; ++s) lam[s] = bl[s];
        for (int i = 0; i < 3; ++i) v[i] = lam[0] * Y[0][i] + lam[1] * Y[1][i] + lam[2] * Y[2][i] + lam[3] * Y[3][i];
        if (bmask == 15u) { hit = 1; break; }                                  // rule 3 (enclosed)
    }
    for (int i = 0; i < 3; ++i) {
        out.ca[i] = lam[0] * WA[0][i] + lam[1] * WA[1][i] + lam[2] * WA[2][i] + lam[3] * WA[3][i];
        out.cb[i] = lam[0] * WB[0][i] + lam[1] * WB[1][i] + lam[2] * WB[2][i] + lam[3] * WB[3][i];
    }
    if (hit) {
        // intersecting cores have no normal: one common point, distance -r_a - r_b (the closed forms' "segment inside the box")
        for (int i = 0; i < 3; ++i) { out.ca[i] = 0.5 * (out.ca[i] + out.cb[i]); out.cb[i] = out.ca[i]; }
        out.len = 0.0;
    } else {
        const double dv[3] = {out.ca[0] - out.cb[0], out.ca[1] - out.cb[1], out.ca[2] - out.cb[2]};
        out.len = sqrt(cvx_dot(dv, dv));
    }
    out.iterations = it;
    out.intersect = hit;
    out.capped = capped;
}

// what osot_kin_create and osot_shape_distance ask of a shape's numbers; nullptr = fine
OSOT_CVX_FN const char* convex_check_size(const int kind, const double* size, const double radius) {
    if (!(radius >= 0.0) || !(radius <= 1.0e300)) return "collision shape: the rounding radius must be finite and not negative";
    if (kind == CVX_HULL) return nullptr;
    for (int i = 0; i < 3; ++i)
        if (!(size[i] >= 0.0) || !(size[i] <= 1.0e300)) return "collision shape: sizes must be finite and not negative";
    return nullptr;
}
OSOT_CVX_FN const char* convex_check_rotation(const double* R) {
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            const double g = R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b];
            if (!(fabs(g - (a == b ? 1.0 : 0.0)) <= 1.0e-9)) return "collision shape: the rotation is not orthonormal (to 1e-9)";
        }
    return nullptr;
}

}  // namespace osot
