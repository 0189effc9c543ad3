// opensot_amd/csrc/osot_kin.h -- batched kinematics producer.
//
// One wavefront per instance, LANE = JOINT (n <= 64).  Per instance:
//   1. lane j: local transform T_j(q_j) = [R0_j Rot(axis_j, q_j) | p0_j] (revolute) or [R0_j | p0_j + R0_j axis_j q_j]
//      (prismatic) -> LDS
//   2. lane j: world transform of its joint frame by pointer jumping over the ancestor chain (log2(depth) rounds)
//      -> LDS, with the world axis z_j and origin p_j
//   3. frames: pose out; column j of the frame Jacobian = [z_j x (p_f - p_j); z_j] (revolute) / [z_j; 0] (prismatic)
//      if joint j is an ancestor of the frame's link, else 0.  Row r of the 6 x n block is written by all lanes at
//      once: one coalesced 8 n-byte store per row, straight into the stacked A_k.
//   4. centre of mass: c = sum m_l c_l / M (wave reduction); column j of its Jacobian from the subtree aggregates
//      (mass and first moment of the links joint j moves): z_j x (Sc_j - Sm_j p_j) / M  (prismatic: (Sm_j / M) z_j)
//   3b. contact points (lane = point): world position of a point fixed in a link -> the convex-hull rows' leaf
//   5. self-collision pairs (capsule / sphere pairs): lane p = pair for the closest points of the two axis segments
//      (world frame) -> distance d = |c_a - c_b| - r_a - r_b and unit normal n -> LDS; then one coalesced row per
//      pair, lane j = joint: J_d[j] = n . (v_j(c_a) [j moves a] - v_j(c_b) [j moves b]),  v_j(c) = z_j x (c - p_j)
//      (revolute) or z_j (prismatic).  (A point of the capsule SURFACE, c - r n, has the same velocity along n.)
//      CONVEX instantiation: a pair that is not capsule / capsule or capsule / box (box, cylinder or hull on either side) gets its
//      closest points from the lane's own GJK run (osot_convex.h); the table and the row loop behind it are the same.
// HBM-bound by construction: reads 8 n bytes of q, writes (6 F + 3) n 8 + 96 F + 24 bytes per instance.
#pragma once
#include <osot_team.h>
#include <osot_mi355x.h>
#include <osot_convex.h>
#include <cmath>

namespace osot {

struct DevKin {            // osot_kin_desc + ancestor masks, in device memory
    osot_kin_desc d;
    unsigned long long anc[OSOT_KIN_MAX_JOINTS];   // bit a set: joint a is an ancestor of (or is) joint j
    unsigned long long sub[OSOT_KIN_MAX_JOINTS];   // bit l set: link l is moved by joint j (j itself included)
    double total_mass;
    // depth-first (pre-order) position of every joint: the links a joint moves are the positions dfs_pos[j] .. sub_end[j] - 1, so a
    // subtree aggregate is a DIFFERENCE OF PREFIX SUMS over that order (the centre-of-mass Jacobian, stage 4)
    int dfs_pos[OSOT_KIN_MAX_JOINTS];
    int sub_end[OSOT_KIN_MAX_JOINTS];
    unsigned rowset_frames;    // bit f set: a row set hangs on frame f (the ROWS instantiation computes its column without a frame_J)
};

// the tables derived from the tree (h.d set, parent[j] < j checked by the caller): shared by osot_kin_create and the emulator's driver
inline void kin_build_tables(DevKin& h) {
    const int n = h.d.n;
    h.total_mass = 0.0;
    for (int j = 0; j < OSOT_KIN_MAX_JOINTS; ++j) { h.anc[j] = 0ull; h.sub[j] = 0ull; h.dfs_pos[j] = j; h.sub_end[j] = j + 1; }
    for (int j = 0; j < n; ++j) {
        h.anc[j] = (1ull << j) | (h.d.parent[j] >= 0 ? h.anc[h.d.parent[j]] : 0ull);
        for (int a = 0; a <= j; ++a) if ((h.anc[j] >> a) & 1ull) h.sub[a] |= (1ull << j);
        h.total_mass += h.d.mass[j];
    }
    if (!(h.total_mass > 0.0)) h.total_mass = 1.0;
    h.rowset_frames = 0u;
    for (int s = 0; s < h.d.n_rowsets && s < OSOT_KIN_MAX_ROWSETS; ++s)
        if (h.d.rowset_frame[s] >= 0 && h.d.rowset_frame[s] < OSOT_KIN_MAX_FRAMES) h.rowset_frames |= 1u << h.d.rowset_frame[s];
    int next_child[OSOT_KIN_MAX_JOINTS], root_off = 0;      // parents come before their children: one pass
    for (int j = 0; j < n; ++j) {
        const int size = __builtin_popcountll(h.sub[j]), pa = h.d.parent[j];
        if (pa < 0) { h.dfs_pos[j] = root_off; root_off += size; }
        else { h.dfs_pos[j] = next_child[pa]; next_child[pa] += size; }
        next_child[j] = h.dfs_pos[j] + 1;
        h.sub_end[j] = h.dfs_pos[j] + size;
    }
}

// osot_kin_create's checks of the frames (shared with osot_dyn_create, osot_dyn.h): the joint a frame is attached to, its
// relative base link (Cartesian.cpp:40-51: a base link that is not the distal link)
inline int kin_check_frames(const osot_kin_desc* d, const char** why) {
    for (int f = 0; f < d->n_frames; ++f)
        if (d->frame_joint[f] < 0 || d->frame_joint[f] >= d->n) { *why = "frame attached to a joint out of range"; return OSOT_ERR_INVALID; }
    for (int f = 0; f < d->n_frames; ++f)
        if (d->frame_base[f] < 0 || d->frame_base[f] > d->n_frames || d->frame_base[f] == f + 1) {
            *why = "frame_base must be 0 (world) or 1 + the index of another frame";
            return OSOT_ERR_INVALID;
        }
    return OSOT_OK;
}

// ... and of the contact points (osot_kin_desc.point_*)
inline int kin_check_points(const osot_kin_desc* d, const char** why) {
    if (d->n_points < 0 || d->n_points > OSOT_KIN_MAX_POINTS) { *why = "contact point count out of range (0..16)"; return OSOT_ERR_INVALID; }
    for (int i = 0; i < d->n_points; ++i)
        if (d->point_joint[i] < 0 || d->point_joint[i] >= d->n) { *why = "contact point attached to a joint out of range"; return OSOT_ERR_INVALID; }
    return OSOT_OK;
}

// ... and of the row sets and gaze references (osot_kin_desc.rowset_*, gaze_*); kin_check_frames has passed
__host__ __device__ inline int kin_rowset_rows(int kind) { return kind == OSOT_ROWSET_CONTACT ? 6 : (kind == OSOT_ROWSET_PURE_ROLLING ? 4 : 3); }
inline int kin_check_rowsets(const osot_kin_desc* d, const char** why) {
    if (d->n_rowsets < 0 || d->n_rowsets > OSOT_KIN_MAX_ROWSETS) { *why = "row set count out of range (0..8)"; return OSOT_ERR_INVALID; }
    if (d->n_gaze < 0 || d->n_gaze > OSOT_KIN_MAX_FRAMES) { *why = "gaze count out of range (0..8)"; return OSOT_ERR_INVALID; }
    for (int s = 0; s < d->n_rowsets; ++s) {
        const int kind = d->rowset_kind[s], f = d->rowset_frame[s];
        if (kind != OSOT_ROWSET_CONTACT && kind != OSOT_ROWSET_PURE_ROLLING && kind != OSOT_ROWSET_OMNI4X) { *why = "unknown row set kind"; return OSOT_ERR_INVALID; }
        if (f < 0 || f >= d->n_frames) { *why = "row set on a frame out of range"; return OSOT_ERR_INVALID; }
        if (d->frame_base[f] != 0) { *why = "a row set uses the world pose and Jacobian of its frame: frame_base must be 0"; return OSOT_ERR_INVALID; }
        if (d->rowset_row_mask[s] == 0) { *why = "row set with an empty row_mask"; return OSOT_ERR_INVALID; }
        if (d->rowset_row_mask[s] < 0 || (d->rowset_row_mask[s] >> kin_rowset_rows(kind)) != 0) { *why = "row_mask names a row the kind does not have"; return OSOT_ERR_INVALID; }
        if (d->rowset_split[s] != 0 && kind != OSOT_ROWSET_CONTACT) { *why = "only a contact row set can be split"; return OSOT_ERR_INVALID; }
        if (d->rowset_split[s] != 0 && d->n <= 6) { *why = "a split contact needs more than 6 coordinates"; return OSOT_ERR_INVALID; }
        if (kind == OSOT_ROWSET_OMNI4X)
            for (int w = 0; w < 4; ++w)
                if (d->rowset_wheel[s][w] < 6 || d->rowset_wheel[s][w] >= d->n) { *why = "wheel coordinate out of range (6 .. n - 1)"; return OSOT_ERR_INVALID; }
    }
    for (int g = 0; g < d->n_gaze; ++g)
        if (d->gaze_frame[g] < 0 || d->gaze_frame[g] >= d->n_frames) { *why = "gaze on a frame out of range"; return OSOT_ERR_INVALID; }
    return OSOT_OK;
}
// PureRolling::setOutwardNormal (PureRolling.cpp:19-47) as written: osot_pure_rolling_s33 (include/osot_mi355x.h)
inline int kin_pure_rolling_s33(const double* nrm, double* s33, double* unit) {
    if (!nrm || !s33) return OSOT_ERR_INVALID;
    const double len = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
    if (!(len > 0.0) || !(len <= 1.0e300)) return OSOT_ERR_INVALID;
    const double uz[3] = {nrm[0] / len, nrm[1] / len, nrm[2] / len};
    int x = 0;                                              // ux = e1
    if (std::fabs(uz[1]) < std::fabs(uz[x])) x = 1;         // e2 against e1
    if (std::fabs(uz[2]) < std::fabs(uz[x])) x = 2;         // e3 against the ux chosen so far
    double ux[3] = {0.0, 0.0, 0.0};
    ux[x] = 1.0;
    const double uy[3] = {uz[1] * ux[2] - uz[2] * ux[1], uz[2] * ux[0] - uz[0] * ux[2], uz[0] * ux[1] - uz[1] * ux[0]};
    for (int i = 0; i < 3; ++i) { s33[3 * i] = ux[i]; s33[3 * i + 1] = uy[i]; s33[3 * i + 2] = uz[i]; }   // columns ux, uy, uz
    if (unit) for (int i = 0; i < 3; ++i) unit[i] = uz[i];
    return OSOT_OK;
}

__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void mat3_vec(const double* A, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double clamp01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }
// closest points of the segments [p1, q1] and [p2, q2] (either may have zero length): parameters s, t in [0, 1]
__device__ inline void closest_segment_points(const double* p1, const double* q1, const double* p2, const double* q2,
                                              double* c1, double* c2) {
    const double tiny = 1.0e-18;
    double d1[3], d2[3], r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { d1[i] = q1[i] - p1[i]; d2[i] = q2[i] - p2[i]; r[i] = p1[i] - p2[i]; }
    const double a = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
    const double e = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
    const double f = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2];
    const double c = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2];
    double s = 0.0, t = 0.0;
    if (a <= tiny && e <= tiny) {
    } else if (a <= tiny) {
        t = clamp01(f / e);
    } else if (e <= tiny) {
        s = clamp01(-c / a);
    } else {
        const double b = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
        const double den = a * e - b * b;            // >= 0; 0 for parallel axes: any s, take 0
        s = (den > tiny * a * e) ? clamp01((b * f - c * e) / den) : 0.0;
        t = (b * s + f) / e;
        if (t < 0.0) { t = 0.0; s = clamp01(-c / a); }
        else if (t > 1.0) { t = 1.0; s = clamp01((b - c) / a); }
        // Near-parallel axes (under 1e-5 rad): below about 3e-7 rad den is the round-off of a e - b^2 and s is chance; where t then
        // stays inside (0, 1) the pair above can be the wrong end of the overlap, too long by the angle times the overlap.  A
        // minimiser of two such segments has an end point of one of them, so the four end-point projections are tried as well.
        // One is taken only where it is shorter beyond round-off: parallel axes keep the pair they had, bit for bit.
        if (!(den > 1.0e-10 * a * e)) {
            double w[3] = {r[0] + s * d1[0] - t * d2[0], r[1] + s * d1[1] - t * d2[1], r[2] + s * d1[2] - t * d2[2]};
            double best = (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * (1.0 - 1.0e-14);
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const double fix = (k & 1) ? 1.0 : 0.0;
                const double sk = (k < 2) ? fix : clamp01((b * fix - c) / a);
                const double tk = (k < 2) ? clamp01((b * fix + f) / e) : fix;
#pragma unroll
                for (int i = 0; i < 3; ++i) w[i] = r[i] + sk * d1[i] - tk * d2[i];
                const double dk = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
                if (dk < best) { best = dk; s = sk; t = tk; }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { c1[i] = p1[i] + s * d1[i]; c2[i] = p2[i] + t * d2[i]; }
}

// closest points of the segment [p0, p1] and the axis-aligned box [-h, h] (all in the BOX frame): ca on the segment, cb on
// the box.  dist^2(t) = sum_i max(|P_i(t)| - h_i, 0)^2 along P(t) = p0 + t (p1 - p0) is convex and piecewise quadratic with
// at most six breakpoints (where a coordinate crosses one of its two faces): on every piece the minimiser of the quadratic
// is clamped to the piece and the best piece wins -- exact, no iteration (FCL, which the reference's collision module
// wraps, runs GJK on the same convex problem).
__device__ inline void closest_segment_box(const double* p0, const double* p1, const double* h, double* ca, double* cb) {
    double v[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    double bp[8];
    bp[0] = 0.0; bp[7] = 1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const bool mv = fabs(v[i]) > 1.0e-300;
        const double ta = mv ? (-h[i] - p0[i]) / v[i] : 0.0, tb = mv ? (h[i] - p0[i]) / v[i] : 0.0;
        bp[1 + 2 * i] = clamp01(ta);
        bp[2 + 2 * i] = clamp01(tb);
    }
    // sort the eight values (a fixed odd-even network: no data-dependent indexing, the array stays in registers)
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
#pragma unroll
        for (int i = (pass & 1); i + 1 < 8; i += 2) {
            const double lo = fmin(bp[i], bp[i + 1]), hi = fmax(bp[i], bp[i + 1]);
            bp[i] = lo; bp[i + 1] = hi;
        }
    }
    double best = INFINITY, tbest = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double t0 = bp[k], t1 = bp[k + 1], tm = 0.5 * (t0 + t1);
        double qa = 0.0, qb = 0.0;          // f(t) = qa t^2 + 2 qb t + qc on this piece; minimiser -qb / qa
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double pm = p0[i] + tm * v[i];
            const double side = pm > h[i] ? 1.0 : (pm < -h[i] ? -1.0 : 0.0);
            const double off = p0[i] - side * h[i];      // excess_i(t) = off + t v_i where the coordinate is outside
            qa += (side != 0.0) ? v[i] * v[i] : 0.0;
            qb += (side != 0.0) ? off * v[i] : 0.0;
        }
        double t = (qa > 0.0) ? -qb / qa : t0;
        t = t < t0 ? t0 : (t > t1 ? t1 : t);
        double f = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double pt = p0[i] + t * v[i];
            const double ex = pt > h[i] ? pt - h[i] : (pt < -h[i] ? pt + h[i] : 0.0);
            f += ex * ex;
        }
        if (f < best) { best = f; tbest = t; }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ca[i] = p0[i] + tbest * v[i];
        cb[i] = ca[i] > h[i] ? h[i] : (ca[i] < -h[i] ? -h[i] : ca[i]);
    }
}

#ifndef OSOT_KIN_TS
#define OSOT_KIN_TS 12
#endif
// contact points, lane = point: R_w p + p_w of the point's joint from the world transforms Tw in LDS -> points [B][n_points][3], the
// OSOT_ROWS_CONVEX_HULL leaf p2 (convex_hull::getSupportPolygonPoints: getPose(link).translation()).  Not inlined: the producer's
// kernels keep their register allocation (profiles/convex_hull_kernel_resources.txt).
__device__ inline __attribute__((noinline)) void kin_points(const DevKin* __restrict__ K, double* points, const long long inst, const int j, const double* Tw) {
    constexpr int TS = OSOT_KIN_TS;
    const int np = K->d.n_points;
    if (j >= np) return;
    const int jp = K->d.point_joint[j];
    const double lp[3] = {K->d.point_p[j][0], K->d.point_p[j][1], K->d.point_p[j][2]};
    double wp[3];
    mat3_vec(Tw + jp * TS, lp, wp);
#pragma unroll
    for (int i = 0; i < 3; ++i) points[(inst * np + j) * 3 + i] = wp[i] + Tw[jp * TS + 9 + i];
}
// the witness points of a pair, ca then cb (lane = pair), from the pair table in LDS -> pair_points [B][n_pairs][6].  Not inlined, like
// kin_points: the instantiations keep their register allocation.
__device__ inline __attribute__((noinline)) void kin_pair_points(double* out, const long long row, const double* pw) {
#pragma unroll
    for (int i = 0; i < 6; ++i) out[row * 6 + i] = pw[3 + i];
}
// Closest points of a CONVEX pair (lane = pair): the two cores from the model and the carrier frames (side a: its link; side b: link,
// world or environment pose), GJK, the witnesses.  e: the world end points of the two capsule segments (a side that is a capsule).
// Not inlined: one body for both sizes of the producer, and the closed-form pairs beside it keep their code.
__device__ inline __attribute__((noinline)) void kin_convex_pair(const DevKin* __restrict__ K, const int p, const double* Ra, const double* pa,
                                                                 const double* Rc, const double* pc, const double* e, double* ca, double* cb) {
    ConvexCore C[2];
#pragma unroll
    for (int sd = 0; sd < 2; ++sd) {
        const int kind = sd == 0 ? K->d.pair_kind_a[p] : K->d.pair_kind[p];
        if (kind == OSOT_SHAPE_CAPSULE) { convex_segment(C[sd], e + 6 * sd, e + 6 * sd + 3); continue; }
        const double* Rl = sd == 0 ? Ra : Rc;
        const double* pl = sd == 0 ? pa : pc;
        const double* SR = sd == 0 ? K->d.pair_shape_R_a[p] : K->d.pair_shape_R[p];
        const double* Sp = sd == 0 ? K->d.pair_shape_p_a[p] : K->d.pair_shape_p[p];
        const double* sz = sd == 0 ? K->d.pair_size_a[p] : K->d.pair_box[p];
        double t[3];
        mat3_mul(Rl, SR, C[sd].R);
        mat3_vec(Rl, Sp, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) { C[sd].p[i] = pl[i] + t[i]; C[sd].s[i] = sz[i]; }
        C[sd].kind = kind;
        C[sd].v = &K->d.hull_vertex[K->d.pair_hull[p][sd][0]][0];
        C[sd].nv = K->d.pair_hull[p][sd][1];
    }
    GjkResult r;
    gjk_closest(C[0], C[1], r);
#pragma unroll
    for (int i = 0; i < 3; ++i) { ca[i] = r.ca[i]; cb[i] = r.cb[i]; }
}
// cross3 for the functions below that are written without contraction (the pragma is lexical: an inlined cross3 keeps its own setting)
__device__ __forceinline__ void cross3_as_written(const double* a, const double* b, double* o) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// ---- row sets (osot_kin_desc.rowset_*): the rows of ONE set, lane = joint.  colw: the lane's column of the frame's WORLD Jacobian
// [linear; angular] (zero for a lane without a joint), Rf: the frame's world rotation; M(pose) is uniform over the lanes, the product
// is lane-local; A / b / qd already point at the instance (A, b may be null).  The one cross-lane step is the split contact's
// b = -sum_{j >= 6} A_j qdot_j (colsum: every lane calls it).  Written without contraction (the bits of the expressions as written,
// in every instantiation and in the host build) and not inlined (one body per JMAX beside the producer's stages).
template <int JMAX>
__device__ inline __attribute__((noinline)) void kin_rowset(const DevKin* __restrict__ K, const int s, double* A, double* b, const double* qd,
                                                            const bool live, const bool valid, const int j, const int n, const double* colw,
                                                            const double* Rf) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const int kind = K->d.rowset_kind[s], mask = K->d.rowset_row_mask[s];
    const bool split = K->d.rowset_split[s] != 0;
    const double* P = K->d.rowset_param[s];
    double row[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (kind == OSOT_ROWSET_CONTACT) {
        // A = K Ad(R_f') J_f (velocity/Contact.cpp:19-33)
        double v[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v[i] = Rf[i] * colw[0] + Rf[3 + i] * colw[1] + Rf[6 + i] * colw[2];
            v[3 + i] = Rf[i] * colw[3] + Rf[3 + i] * colw[4] + Rf[6 + i] * colw[5];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r)
            row[r] = P[6 * r] * v[0] + P[6 * r + 1] * v[1] + P[6 * r + 2] * v[2] + P[6 * r + 3] * v[3] + P[6 * r + 4] * v[4] + P[6 * r + 5] * v[5];
    } else if (kind == OSOT_ROWSET_PURE_ROLLING) {
        // A = S [J_lin + J_ang x d; J_ang], d = -r n, S = [S33 0; 0 0 0 a'], a = (R_f e_z) x n normalised (PureRolling.cpp:50-77)
        const double d[3] = {-1.0 * P[0] * P[1], -1.0 * P[0] * P[2], -1.0 * P[0] * P[3]};
        double cx[3], a[3];
        cross3_as_written(colw + 3, d, cx);
        const double jc[3] = {colw[0] + cx[0], colw[1] + cx[1], colw[2] + cx[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) row[i] = P[4 + 3 * i] * jc[0] + P[4 + 3 * i + 1] * jc[1] + P[4 + 3 * i + 2] * jc[2];
        const double ez[3] = {Rf[2], Rf[5], Rf[8]};
        cross3_as_written(ez, P + 1, a);
        const double an = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);      // (0 for a wheel axis along n: no guard, as the reference)
        a[0] /= an; a[1] /= an; a[2] /= an;
        row[3] = a[0] * colw[3] + a[1] * colw[4] + a[2] * colw[5];
    } else {
        // OmniWheels4X.cpp:22-74: the constant selection in columns 0 .. 5, R_base (r / 4) v_j behind them
        if (j < 6) {
            row[0] = (j == 0) ? 1.0 : 0.0; row[1] = (j == 1) ? 1.0 : 0.0; row[2] = (j == 5) ? 1.0 : 0.0;
        } else {
            const double il = 1.0 / (P[0] + P[1]), q4 = P[2] / 4.0;
            double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (K->d.rowset_wheel[s][w] != j) continue;
                v[0] -= 1.0;
                v[1] -= (w == 0 || w == 3) ? -1.0 : 1.0;
                v[2] -= (w == 0 || w == 2) ? -il : il;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) v[i] *= q4;
#pragma unroll
            for (int i = 0; i < 3; ++i) row[i] = Rf[3 * i] * v[0] + Rf[3 * i + 1] * v[1] + Rf[3 * i + 2] * v[2];
        }
    }
    const int nrows = kin_rowset_rows(kind);
    const double qj = (split && b && qd) ? qd[j < n ? j : 0] : 0.0;
    int o = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        if (r >= nrows || !((mask >> r) & 1)) continue;
        if (split) {
            if (A && valid && live && j < 6) A[o * 6 + j] = row[r];
            if (b) {
                const double sum = colsum<JMAX>((valid && j >= 6) ? row[r] * qj : 0.0);
                if (j == 0 && live) b[o] = -sum;
            }
        } else if (A && valid && live) {
            A[o * n + j] = row[r];
        }
        ++o;
    }
}
// ---- gaze reference of ONE gaze (Gaze.cpp:52-74, cartesian_utils.cpp:27-35), one lane: T = [R | p] the pose its frame publishes,
// gp the point, ref the 12 doubles of the Cartesian leaf's reference pose -- overwritten where |t| >= 0.2, untouched below.
__device__ inline __attribute__((noinline)) void kin_gaze_ref(const double* T, const double* gp, double* ref) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double dg[3] = {gp[0] - T[9], gp[1] - T[10], gp[2] - T[11]};
    double t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = T[i] * dg[0] + T[3 + i] * dg[1] + T[6 + i] * dg[2];      // R'(g - p)
    const double nt = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    if (!(nt >= 0.2)) return;                                                                 // GAZE_THRESHOLD
    // pan = atan2(t_y, t_x), tilt = atan2(t_z, rho) with rho = sqrt(t_y^2 + t_x^2): their cosines and sines are ratios of t, rho and
    // |t| -- formed directly, without the round trip through the angles (square roots and divisions are correctly rounded on the host
    // and on the device alike; atan2 / sincos are not, and cost a few hundred instructions).  rho = 0: pan = atan2(0, 0) = 0.
    const double rho = sqrt(t[1] * t[1] + t[0] * t[0]);
    const bool has_pan = rho > 0.0;
    const double cp = has_pan ? t[0] / rho : 1.0, sp = has_pan ? t[1] / rho : 0.0;
    const double cs = rho / nt, sn = -(t[2] / nt);                                            // cos(-tilt), sin(-tilt)
    // Identity, DoRotZ(pan), DoRotY(-tilt): [[cp cs, -sp, cp sn], [sp cs, cp, sp sn], [-sn, 0, cs]]
    ref[0] = cs * cp; ref[1] = -sp; ref[2] = sn * cp;
    ref[3] = cs * sp; ref[4] = cp;  ref[5] = sn * sp;
    ref[6] = -sn;     ref[7] = 0.0; ref[8] = cs;
    ref[9] = 0.0; ref[10] = 0.0; ref[11] = 0.0;
}
// LDS one instance of kin_instance needs, in doubles (the int / 64-bit tables included): transforms, axes, centres of mass, parents,
// ancestor masks -- and the pair table of the PAIRS instantiation
template <int JMAX> constexpr int kin_lds_doubles(bool pairs) {
    return JMAX * OSOT_KIN_TS + JMAX * 3 + JMAX * 4 + (JMAX + 1) / 2 + JMAX + OSOT_KIN_MAX_FRAMES * (14 + 1) + (pairs ? OSOT_KIN_MAX_PAIRS * 9 : 0);
}
// The kinematics of ONE instance by the JMAX lanes j = 0 .. JMAX - 1 that call it together (lane = joint; the reductions are
// colsum<JMAX>).  `lds` = kin_lds_doubles<JMAX>(PAIRS) doubles of this instance's own.  The kernel below calls it for one instance
// per wavefront (JMAX = 64) or two (JMAX = 32: the halves); osot_control_cycle_kernel calls it in front of the instance's update.
// PAIRS: the instantiation with the self-collision stage (step 5); the other one keeps the leaner register / LDS budget
// CONVEX (with PAIRS): the stage also serves pairs of convex shapes (kin_convex_pair); launched only for a model that has one
// ROWS: the instantiation with the row sets and gaze references (kin_rowset, kin_gaze_ref); launched only for a call that binds one.
// Off, every line of it is behind `if constexpr`: the other instantiations are the code they were
// developer knob (tools/build_variant.sh NAME -DOSOT_KIN_PHASES): instance 0 prints the clock count of every stage
#ifdef OSOT_KIN_PHASES
#define KIN_PHASE(tag) do { const long long t_ = (long long)clock64(); if (inst == 0 && j == 0) printf("KIN " tag " %lld\n", t_ - kph_); kph_ = (long long)clock64(); } while (0)
#else
#define KIN_PHASE(tag) do { } while (0)
#endif
template <bool PAIRS, int JMAX, bool CONVEX = false, bool ROWS = false>
__device__ __forceinline__ void kin_instance(const DevKin* __restrict__ K, const osot_kin_batch& Bt, const long long inst, const bool live,
                                             const int j, double* lds) {
    constexpr int TS = OSOT_KIN_TS;
    double* Tb = lds;                                     // ONE transform buffer [R | p] per joint (round 3; it was a ping-pong
    //                                              pair: a round of the pointer jumping reads, synchronises, writes, synchronises
    //                                              either way, so the second buffer bought nothing and cost 3 KB per instance:
    //                                              10.4 KB per wavefront instead of 16.5 -> 15 wavefronts per CU instead of 9)
    double* Tl = Tb;
    double* Zw = Tb + JMAX * TS;                          // world joint axes
    double* Cw = Zw + JMAX * 3;                           // world link centres of mass, mass
    unsigned long long* Anc = reinterpret_cast<unsigned long long*>(Cw + JMAX * 4);   // ancestor masks
    int* Par = reinterpret_cast<int*>(Anc + JMAX);        // parent indices (the chain walk must not chase pointers through HBM)
    double* Fw = reinterpret_cast<double*>(Par + 2 * ((JMAX + 1) / 2));               // per frame: world [R | p], its joint, body flag
    unsigned long long* Fq = reinterpret_cast<unsigned long long*>(Fw + OSOT_KIN_MAX_FRAMES * 14);   // ... column mask
    double* Pw = reinterpret_cast<double*>(Fq + OSOT_KIN_MAX_FRAMES);                 // per pair: normal n, axis points c_a, c_b (world)
    (void)Pw;
#ifdef OSOT_KIN_PHASES
    long long kph_ = (long long)clock64();
#endif
    const int n = K->d.n;
    const bool valid = j < n && live;
    Par[j] = valid ? K->d.parent[j] : -1;
    Anc[j] = valid ? K->anc[j] : 0ull;
    // ---- 1. local transforms.  Everything the lane needs from the model (23 loads) and its q are fetched in ONE batch, in front of the
    // sincos (computed whatever the joint type: its ~1.5 k clocks then run under the loads instead of behind the type's round trip)
    const int jc = (j < n) ? j : 0;
    const double qj = Bt.q[(live ? inst : 0) * n + jc];
    const int type_j = K->d.type[jc];
    const int dfs_j = K->dfs_pos[jc], end_j = K->sub_end[jc];
    double R0[9], ax[3], p0j[3], comj[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R0[i] = K->d.R0[jc][i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { ax[i] = K->d.axis[jc][i]; p0j[i] = K->d.p0[jc][i]; comj[i] = K->d.com[jc][i]; }
    const double mass_j = K->d.mass[jc];
    {
        double sn, cs;
        sincos(qj, &sn, &cs);
        double R[9], p[3];
        if (type_j == OSOT_JOINT_REVOLUTE) {
            const double v = 1.0 - cs, x = ax[0], y = ax[1], z = ax[2];
            const double Rq[9] = {cs + x * x * v,     x * y * v - z * sn, x * z * v + y * sn,
                                  y * x * v + z * sn, cs + y * y * v,     y * z * v - x * sn,
                                  z * x * v - y * sn, z * y * v + x * sn, cs + z * z * v};   // Rodrigues
            mat3_mul(R0, Rq, R);
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = p0j[i];
        } else {
            double t[3];
            mat3_vec(R0, ax, t);
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = R0[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = p0j[i] + qj * t[i];
        }
        if (valid) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Tl[j * TS + i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) Tl[j * TS + 9 + i] = p[i];
        }
    }
    wave_sync();
    KIN_PHASE("local");
    // ---- 2. world transforms by POINTER JUMPING: every lane keeps T(jp -> j), the transform from the frame of its
    // jump pointer jp to its own frame, and in each round composes it with T(jp(jp) -> jp) read from LDS and jumps:
    // ceil(log2(depth + 1)) rounds (4 for a humanoid) instead of a walk of `depth` steps up the chain.
    double Rw[9], pw[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rw[i] = valid ? Tl[j * TS + i] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) pw[i] = valid ? Tl[j * TS + 9 + i] : 0.0;
    {
        int jp = Par[j];
        while (wave_ballot(jp >= 0) != 0ull) {
            int njp = jp;
            if (jp >= 0) {
                double Ra[9], pa[3], Rn[9], pn[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) Ra[i] = Tb[jp * TS + i];
#pragma unroll
                for (int i = 0; i < 3; ++i) pa[i] = Tb[jp * TS + 9 + i];
                mat3_mul(Ra, Rw, Rn);
                mat3_vec(Ra, pw, pn);
#pragma unroll
                for (int i = 0; i < 9; ++i) Rw[i] = Rn[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) pw[i] = pn[i] + pa[i];
                njp = Par[jp];
            }
            wave_sync();            // everybody has read Par and the transforms of this round
#pragma unroll
            for (int i = 0; i < 9; ++i) Tb[j * TS + i] = Rw[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) Tb[j * TS + 9 + i] = pw[i];
            Par[j] = njp;
            jp = njp;
            wave_sync();
        }
    }
    KIN_PHASE("jump");
    double* Tw = Tb;               // final world transforms (re-written below, after the last round's barrier: a joint without a parent never entered the loop's writes)
    double zj[3];
    {
        double z[3], cl[3];
        mat3_vec(Rw, ax, z);
        mat3_vec(Rw, comj, cl);
        if (valid) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Tw[j * TS + i] = Rw[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) Tw[j * TS + 9 + i] = pw[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { Zw[j * 3 + i] = valid ? z[i] : 0.0; zj[i] = valid ? z[i] : 0.0; }
        // m_j [c_j, 1] at the joint's depth-first position (joints beyond n: zeros at their own index, which no joint below n has)
        const int pos = valid ? dfs_j : j;
#pragma unroll
        for (int i = 0; i < 3; ++i) Cw[pos * 4 + i] = valid ? mass_j * (cl[i] + pw[i]) : 0.0;
        Cw[pos * 4 + 3] = valid ? mass_j : 0.0;
    }
    const bool revolute = valid && type_j == OSOT_JOINT_REVOLUTE;
    // ---- 3a. world frames, lane = frame: the frame's joint, offset and options in one batch of loads per lane, [R | p] and the joint
    // into LDS for the Jacobian columns below; the pose goes out from here
    const int nfr = K->d.n_frames;
    {
        const int f = (j < nfr) ? j : 0;
        const int jf = K->d.frame_joint[f];
        double FR[9], Fp[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) FR[i] = K->d.frame_R[f][i];
#pragma unroll
        for (int i = 0; i < 3; ++i) Fp[i] = K->d.frame_p[f][i];
        const int body_f = K->d.frame_body[f];
        const int base_f = K->d.frame_base[f];                    // 0: the world; g + 1: frame g is the base link frame (Cartesian.cpp:73-81)
        const unsigned long long cm_f = K->d.frame_col_mask[f];   // Task::applyActiveJointsMask (Task.h:129-139)
        double* pose_out = nullptr;        // (a select chain: a lane-indexed read of the argument struct would be served from a scratch copy)
#pragma unroll
        for (int ff = 0; ff < OSOT_KIN_MAX_FRAMES; ++ff) pose_out = (f == ff) ? Bt.frame_pose[ff] : pose_out;
        wave_sync();               // the world transforms are in LDS
        double Rj[9], pj[3], Rf[9], t[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rj[i] = Tw[jf * TS + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) pj[i] = Tw[jf * TS + 9 + i];
        mat3_mul(Rj, FR, Rf);
        mat3_vec(Rj, Fp, t);
        if (j < nfr) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Fw[j * 14 + i] = Rf[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) Fw[j * 14 + 9 + i] = pj[i] + t[i];
            Fw[j * 14 + 12] = (double)jf;
            Fw[j * 14 + 13] = (double)((body_f ? 1 : 0) + 2 * base_f);   // options: bit 0 = BODY Jacobian, the rest = base frame + 1
            Fq[j] = cm_f;
            if (pose_out && live && base_f <= 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) pose_out[inst * 12 + i] = Rf[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) pose_out[inst * 12 + 9 + i] = pj[i] + t[i];
            }
        }
        wave_sync();
        if (j < nfr && pose_out && live && base_f > 0) {
            // relative pose base_T_distal = [R_b'R_d | R_b'(p_d - p_b)] (ModelInterface::getPose(distal, base, T), Cartesian.cpp:80-81);
            // the base frame's world pose was published by its own lane above
            const double* Bw = Fw + (base_f - 1) * 14;
            double Rb[9], dp[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) Rb[i] = Bw[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) dp[i] = (pj[i] + t[i]) - Bw[9 + i];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
                    pose_out[inst * 12 + 3 * r + cc] = Rb[r] * Rf[cc] + Rb[3 + r] * Rf[3 + cc] + Rb[6 + r] * Rf[6 + cc];
                pose_out[inst * 12 + 9 + r] = Rb[r] * dp[0] + Rb[3 + r] * dp[1] + Rb[6 + r] * dp[2];
            }
        }
        if constexpr (ROWS) {
            // gaze references, lane = frame: the pose the frame publishes (the expressions above), whether or not it is bound
            const int ng = K->d.n_gaze;
            if (ng > 0 && j < nfr && live) {
                double T[12];
                if (base_f <= 0) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) T[i] = Rf[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) T[9 + i] = pj[i] + t[i];
                } else {
                    const double* Bw = Fw + (base_f - 1) * 14;
                    double Rb[9], dp[3];
#pragma unroll
                    for (int i = 0; i < 9; ++i) Rb[i] = Bw[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) dp[i] = (pj[i] + t[i]) - Bw[9 + i];
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int cc = 0; cc < 3; ++cc) T[3 * r + cc] = Rb[r] * Rf[cc] + Rb[3 + r] * Rf[3 + cc] + Rb[6 + r] * Rf[6 + cc];
                        T[9 + r] = Rb[r] * dp[0] + Rb[3 + r] * dp[1] + Rb[6 + r] * dp[2];
                    }
                }
                for (int g = 0; g < ng; ++g) {
                    const double* gp = Bt.gaze_point[g];
                    double* gr = Bt.gaze_ref[g];
                    if (gp && gr && K->d.gaze_frame[g] == j) kin_gaze_ref(T, gp + inst * 3, gr + inst * 12);
                }
            }
        }
    }
    // ---- 3b. contact points (the world transforms in LDS are unchanged since the barrier of 3a)
    if (Bt.points && K->d.n_points > 0 && live) kin_points(K, Bt.points, inst, j, Tw);
    KIN_PHASE("world");
    // ---- 3. frames: the Jacobian columns, lane = joint
    // (a frame's transform and options come from the LDS table in one batch of reads -- fetched from the model here, every frame started
    //  behind a round trip of scalar loads; the row address stays a scalar load of the argument struct: through LDS it became a
    //  per-lane address and the six stores paid for it, 2.9 k -> 3.4 k clocks)
    for (int f = 0; f < nfr; ++f) {
        double Rf[9], pf[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rf[i] = Fw[f * 14 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) pf[i] = Fw[f * 14 + 9 + i];
        const int jf = (int)Fw[f * 14 + 12];
        const int opt = (int)Fw[f * 14 + 13];
        const bool body = (opt & 1) != 0;
        const int bf = (opt >> 1) - 1;                   // base frame of a relative Cartesian task, -1: the world
        const int jb = (bf >= 0) ? (int)Fw[bf * 14 + 12] : 0;
        const unsigned long long cm = Fq[f];
        double* Jf = Bt.frame_J[f];                      // (the argument struct: scalar loads, a uniform base address for the stores)
        if constexpr (!ROWS) { if (!Jf) continue; }
        else { if (!Jf && !((K->rowset_frames >> f) & 1u)) continue; }
        const long long jstride = Bt.frame_J_stride[f];
        [[maybe_unused]] double colw[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // ROWS: the world column, in front of the frame's options
        if (valid) {
            double col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            // joint j moves the distal link (+1), the base link (-1: the base body's point at the distal origin moves the same way,
            // so the joints both chains share cancel), both or neither (0).  World base: the ancestor test as before
            const bool in_d = ((Anc[jf] >> j) & 1ull) != 0ull;
            const bool in_b = bf >= 0 && ((Anc[jb] >> j) & 1ull) != 0ull;
            if (in_d != in_b) {
                if (revolute) {
                    const double dlt[3] = {pf[0] - pw[0], pf[1] - pw[1], pf[2] - pw[2]};
                    cross3(zj, dlt, col);
                    col[3] = zj[0]; col[4] = zj[1]; col[5] = zj[2];
                } else {
                    col[0] = zj[0]; col[1] = zj[1]; col[2] = zj[2];
                }
                if (in_b) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) col[i] = -col[i];
                }
            }
            if constexpr (ROWS) {
#pragma unroll
                for (int i = 0; i < 6; ++i) colw[i] = col[i];
            }
            if (body || bf >= 0) {
                // BODY Jacobian Ad(R_f') J (Cartesian.cpp:93-100): both halves rotated by R_f'; a relative Jacobian is expressed in
                // its base frame: R_b' (getRelativeJacobian, Cartesian.cpp:75-76) -- and BODY on top of that is Ad((R_b'R_d)') R_b' = R_d'
                double Rr[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) Rr[i] = body ? Rf[i] : Fw[(bf >= 0 ? bf : 0) * 14 + i];
                double rl[3], ra[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    rl[i] = Rr[i] * col[0] + Rr[3 + i] * col[1] + Rr[6 + i] * col[2];
                    ra[i] = Rr[i] * col[3] + Rr[3 + i] * col[4] + Rr[6 + i] * col[5];
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) { col[i] = rl[i]; col[3 + i] = ra[i]; }
            }
            const bool masked = cm != 0ull && !((cm >> j) & 1ull);
            if (!ROWS || Jf) {
                double* J = Jf + inst * jstride;
#pragma unroll
                for (int r = 0; r < 6; ++r) J[r * n + j] = masked ? 0.0 : col[r];
            }
        }
        if constexpr (ROWS) {
            // the row sets on this frame (a frame with one has the world as its base: colw is its world column)
            if ((K->rowset_frames >> f) & 1u) {
                const int ns = K->d.n_rowsets;
                for (int s = 0; s < ns; ++s) {
                    if (K->d.rowset_frame[s] != f) continue;
                    double* As = Bt.rowset_A[s];
                    double* bs = Bt.rowset_b[s];
                    if (!As && !bs) continue;
                    const long long io = live ? inst : 0;
                    kin_rowset<JMAX>(K, s, As ? As + io * Bt.rowset_A_stride[s] : nullptr, bs ? bs + io * Bt.rowset_b_stride[s] : nullptr,
                                     Bt.rowset_qdot ? Bt.rowset_qdot + io * n : nullptr, live, valid, j, n, colw, Rf);
                }
            }
        }
    }
    KIN_PHASE("frames");
    // ---- 4. centre of mass and its Jacobian
    if (Bt.com || Bt.com_J) {
        const double iM = fast_rcp(K->total_mass);       // (one reciprocal instead of six fp64 divisions)
        // Inclusive prefix sums of m_l [c_l, 1] over the depth-first order (written there by the world stage), lane = position:
        // log2(JMAX) rounds of "read the entry d positions back, add, write".  The links joint j moves are a contiguous range of that
        // order, so S_j = P[sub_end_j - 1] - P[dfs_j - 1]; the total is the last entry (positions beyond n hold zeros).
        // (the 0/1 matrix-vector product this replaces read all 4 JMAX entries per lane: 4.4 k of the producer's 15.9 k clocks)
        double a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = Cw[j * 4 + i];
#pragma unroll
        for (int d = 1; d < JMAX; d <<= 1) {
            double t[4];
            const int src = (j >= d) ? j - d : 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) t[i] = Cw[src * 4 + i];
            wave_sync();
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] += (j >= d) ? t[i] : 0.0; Cw[j * 4 + i] = a[i]; }
            wave_sync();
        }
        if (Bt.com) {
            const int i3 = (j < 3) ? j : 0;
            const double tot = Cw[(JMAX - 1) * 4 + i3];
            if (j < 3 && live) Bt.com[inst * 3 + j] = tot * iM;
        }
        if (Bt.com_J) {
            // column j = z_j x (Sc_j - Sm_j p_j) / M  (revolute)   or   (Sm_j / M) z_j  (prismatic)
            const int hi = valid ? end_j - 1 : 0, lo = (valid && dfs_j > 0) ? dfs_j - 1 : 0;
            double sc[3], sm;
            {
                double ph[4], pl[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { ph[i] = Cw[hi * 4 + i]; pl[i] = Cw[lo * 4 + i]; }
                const bool from0 = !(valid && dfs_j > 0);
#pragma unroll
                for (int i = 0; i < 3; ++i) sc[i] = ph[i] - (from0 ? 0.0 : pl[i]);
                sm = ph[3] - (from0 ? 0.0 : pl[3]);
            }
            double acc[3];
            if (revolute) {
                const double dlt[3] = {sc[0] - sm * pw[0], sc[1] - sm * pw[1], sc[2] - sm * pw[2]};
                cross3(zj, dlt, acc);
            } else {
                acc[0] = sm * zj[0]; acc[1] = sm * zj[1]; acc[2] = sm * zj[2];
            }
            if (valid) {
                const unsigned long long cm = K->d.com_col_mask;
                const bool masked = cm != 0ull && !((cm >> j) & 1ull);
                double* J = Bt.com_J + inst * Bt.com_J_stride;
#pragma unroll
                for (int r = 0; r < 3; ++r) J[r * n + j] = masked ? 0.0 : acc[r] * iM;
            }
        }
    }
    KIN_PHASE("com");
    // ---- 5. self-collision pairs
    if constexpr (PAIRS) {
    const int np = K->d.n_pairs;
    if (np > 0 && (Bt.pair_dist || Bt.pair_J || Bt.pair_points)) {
        if (j < np && live) {
            double e[2][6];
            double Rc[9], pc[3];      // carrier frame of side b (link, world, or the runtime pose of an environment shape)
            double Ra[9], pa[3];      // CONVEX: ... and of side a (its link)
            (void)Ra; (void)pa;
#pragma unroll
            for (int sd = 0; sd < 2; ++sd) {
                const int js = K->d.pair_joint[j][sd];
                double Rj[9], pj[3];
                const int env = (sd == 1) ? K->d.pair_env[j] - 1 : -1;
                if (js >= 0) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) Rj[i] = Tw[js * TS + i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) pj[i] = Tw[js * TS + 9 + i];
                } else if (env >= 0 && Bt.env_pose) {
                    const double* E = Bt.env_pose + inst * Bt.env_pose_stride + env * 12;
#pragma unroll
                    for (int i = 0; i < 9; ++i) Rj[i] = E[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) pj[i] = E[9 + i];
                } else {
#pragma unroll
                    for (int i = 0; i < 9; ++i) Rj[i] = (i % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
                    for (int i = 0; i < 3; ++i) pj[i] = 0.0;
                }
                double t0[3], t1[3];
                mat3_vec(Rj, &K->d.pair_seg[j][sd][0], t0);
                mat3_vec(Rj, &K->d.pair_seg[j][sd][3], t1);
#pragma unroll
                for (int i = 0; i < 3; ++i) { e[sd][i] = t0[i] + pj[i]; e[sd][3 + i] = t1[i] + pj[i]; }
                if (sd == 1) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) Rc[i] = Rj[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) pc[i] = pj[i];
                }
                if constexpr (CONVEX) {
                    if (sd == 0) {
#pragma unroll
                        for (int i = 0; i < 9; ++i) Ra[i] = Rj[i];
#pragma unroll
                        for (int i = 0; i < 3; ++i) pa[i] = pj[i];
                    }
                }
            }
            double ca[3], cb[3];
            bool closed_form = true;      // capsule / capsule and capsule / box: the same code, the same bits, in every instantiation
            if constexpr (CONVEX) {
                const int ka = K->d.pair_kind_a[j], kb = K->d.pair_kind[j];
                closed_form = ka == OSOT_SHAPE_CAPSULE && (kb == OSOT_SHAPE_CAPSULE || kb == OSOT_SHAPE_BOX);
                if (!closed_form) kin_convex_pair(K, j, Ra, pa, Rc, pc, &e[0][0], ca, cb);
            }
            if (!closed_form) {      // (ca, cb are there)
            } else if (K->d.pair_kind[j] == OSOT_SHAPE_BOX) {
                // box frame in the world: (Rc, pc) o (shape_R, shape_p); side a's segment goes into it, the closest points
                // come back out
                double Rb[9], tb[3], pb[3];
                mat3_mul(Rc, K->d.pair_shape_R[j], Rb);
                mat3_vec(Rc, K->d.pair_shape_p[j], tb);
#pragma unroll
                for (int i = 0; i < 3; ++i) pb[i] = pc[i] + tb[i];
                double s0[3], s1[3], la[3], lb[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {   // R_b' (x - p_b)
                    s0[i] = Rb[i] * (e[0][0] - pb[0]) + Rb[3 + i] * (e[0][1] - pb[1]) + Rb[6 + i] * (e[0][2] - pb[2]);
                    s1[i] = Rb[i] * (e[0][3] - pb[0]) + Rb[3 + i] * (e[0][4] - pb[1]) + Rb[6 + i] * (e[0][5] - pb[2]);
                }
                closest_segment_box(s0, s1, K->d.pair_box[j], la, lb);
                double wa[3], wb[3];
                mat3_vec(Rb, la, wa);
                mat3_vec(Rb, lb, wb);
#pragma unroll
                for (int i = 0; i < 3; ++i) { ca[i] = wa[i] + pb[i]; cb[i] = wb[i] + pb[i]; }
            } else {
                closest_segment_points(&e[0][0], &e[0][3], &e[1][0], &e[1][3], ca, cb);
            }
            const double dv[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
            const double len = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
            const bool deg = !(len > 1.0e-12);      // coincident axis points: no direction; the row is zero
            const double il = deg ? 0.0 : 1.0 / len;
#pragma unroll
            for (int i = 0; i < 3; ++i) { Pw[j * 9 + i] = dv[i] * il; Pw[j * 9 + 3 + i] = ca[i]; Pw[j * 9 + 6 + i] = cb[i]; }
            if (Bt.pair_dist) Bt.pair_dist[inst * np + j] = len - K->d.pair_radius[j][0] - K->d.pair_radius[j][1];
            if (Bt.pair_points) kin_pair_points(Bt.pair_points, inst * np + j, Pw + j * 9);
        }
        wave_sync();
        if (Bt.pair_J) {
            double* J = Bt.pair_J + inst * Bt.pair_J_stride;
            for (int p = 0; p < np; ++p) {
                const int ja = K->d.pair_joint[p][0], jb = K->d.pair_joint[p][1];
                const double sa = ((Anc[ja] >> j) & 1ull) ? 1.0 : 0.0;
                const double sb = (jb >= 0 && ((Anc[jb < 0 ? 0 : jb] >> j) & 1ull)) ? 1.0 : 0.0;   // (a world shape: no joint moves it)
                const double nn[3] = {Pw[p * 9], Pw[p * 9 + 1], Pw[p * 9 + 2]};
                double val;
                if (revolute) {
                    // n . (z x (c_a - p_j)) sa - n . (z x (c_b - p_j)) sb = n . (z x (sa (c_a - p_j) - sb (c_b - p_j)))
                    const double dl[3] = {sa * (Pw[p * 9 + 3] - pw[0]) - sb * (Pw[p * 9 + 6] - pw[0]),
                                          sa * (Pw[p * 9 + 4] - pw[1]) - sb * (Pw[p * 9 + 7] - pw[1]),
                                          sa * (Pw[p * 9 + 5] - pw[2]) - sb * (Pw[p * 9 + 8] - pw[2])};
                    double cr[3];
                    cross3(zj, dl, cr);
                    val = nn[0] * cr[0] + nn[1] * cr[1] + nn[2] * cr[2];
                } else {
                    val = (sa - sb) * (nn[0] * zj[0] + nn[1] * zj[1] + nn[2] * zj[2]);
                }
                if (valid) J[p * n + j] = val;
            }
        }
    }
    }
}

// JMAX = 32: TWO instances per wavefront (lanes 0..31 and 32..63 each run a robot of <= 32 joints: every instruction, every
// 64-lane store carries two instances);  JMAX = 64: one instance per wavefront.
template <bool PAIRS, int JMAX, bool CONVEX = false, bool ROWS = false>
__global__ void __launch_bounds__(64) osot_kin_kernel(const DevKin* __restrict__ K, const osot_kin_batch Bt) {
    constexpr int PACK = 64 / JMAX;
    constexpr int SLICE = kin_lds_doubles<JMAX>(PAIRS);
    OSOT_STATIC_LDS(double, kin_lds, PACK * SLICE);
    const int sub = (PACK == 2) ? (int)(threadIdx.x >> 5) : 0;
    const int j = (PACK == 2) ? (int)(threadIdx.x & 31u) : (int)threadIdx.x;
    const long long inst = (long long)blockIdx.x * PACK + sub;
    const bool live = inst < Bt.B;            // (an odd batch leaves the last wavefront's second half idle)
    kin_instance<PAIRS, JMAX, CONVEX, ROWS>(K, Bt, inst, live, j, kin_lds + sub * SLICE);
}

}  // namespace osot
