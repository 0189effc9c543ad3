// opensot_amd/csrc/osot_dyn.h -- batched rigid-body dynamics producer: inertia matrix M(q), non-linear term h(q, qdot),
// Jdot qdot of frames and of the centre of mass (what the inverse-dynamics leaves ask XBot::ModelInterface for:
// computeInertiaMatrix, computeNonlinearTerm, getJdotTimesV, getCOMJdotTimesV).
//
// One wavefront per instance, LANE = JOINT (n <= 64), on top of the transform stages of the kinematics producer (kin_instance with no
// output bound: local transforms, world transforms by pointer jumping, world frames -- all left in LDS).
// Every spatial quantity is expressed in the WORLD frame about the WORLD ORIGIN, coordinates [angular; linear], so quantities of
// different links add without transforms and both tree passes are log-depth:
//   1. motion subspace S_j = [z_j; p_j x z_j] (revolute) / [0; z_j] (prismatic); link inertia about the world origin:
//      mass m, first moment m c, rotational inertia R I_cm R' + m (c.c E - c c')
//   2. link velocity v_j = sum over the ancestor chain of S_a qdot_a, then the bias acceleration a_j = sum over the chain of
//      (v_a x S_a) qdot_a -- two sums by POINTER JUMPING (ceil(log2(depth + 1)) rounds each)
//   3. frames, lane = frame: Jdot qdot = [a_o + alpha x p + omega x (v_o + omega x p); alpha]; CoM: the mass-weighted classical
//      accelerations of the link centres of mass (wave reduction)
//   4. link wrench f_j = I_j (a_j - a_gravity) + v_j x* (I_j v_j); composite inertias Ic_j and subtree wrenches by DIFFERENCES OF
//      PREFIX SUMS over the depth-first order (16 values per link, log2(64) rounds): the links a joint moves are contiguous there
//   5. h_j = S_j . f_subtree(j);  F_j = Ic_j S_j;  M[i][j] = S_i . F_j where i is an ancestor of j (or j itself), mirrored, zero
//      elsewhere.  Row r is written by all lanes at once (one coalesced 8 n-byte store); both M[r][c] and M[c][r] evaluate the SAME
//      fma chain on the same operands, so M is symmetric bit for bit.
//  5a. (only in the instantiation with the centroidal momentum outputs) F_j = [n_j; f_j] is the spatial momentum of the subtree joint j
//      moves per unit qdot_j about the world origin; about the centre of mass c_G it is column j of the centroidal momentum matrix,
//      rows [linear; angular] = [f_j; n_j - c_G x f_j], world axes (computeCentroidalMomentumMatrix: the reference reads block(0,0,3,n)
//      as linear, block(3,0,3,n) as angular).  c_G = the last prefix sum of stage 4 / total mass.  momentum = sum_j column_j qdot_j
//      (wave reduction; computeCentroidalMomentum), ang_mom_b = Ldot_d + lambda K (L_d - L_angular) (acceleration::AngularMomentum with
//      CMMdot * v = 0 as in the reference).  The cancellation is in n_j - c_G x f_j: both grow with the distance of c_G from the origin.
// Algorithmic bytes per instance: reads 8 n (q) + 8 n (qdot), writes 8 n^2 (M) + 8 n (h) + 48 F (frames) + 24 (CoM)
// (+ 48 n (momentum matrix) + 48 (momentum) + 24 (ang_mom_b) when bound).
#pragma once
#include <cmath>
#include <cstring>
#include "osot_kin.h"

namespace osot {

struct DevDyn {            // the tree with its tables, the rotational inertias and gravity, in device memory
    DevKin k;
    double inertia[OSOT_KIN_MAX_JOINTS][6];
    double gravity[3];
};

// symmetric 3 x 3 [xx xy xz yy yz zz] positive semi-definite up to tol: every principal minor >= -tol^(order)
inline bool dyn_psd3(const double* s, double tol) {
    const double xx = s[0], xy = s[1], xz = s[2], yy = s[3], yz = s[4], zz = s[5];
    if (!(xx >= -tol) || !(yy >= -tol) || !(zz >= -tol)) return false;
    if (!(xx * yy - xy * xy >= -tol * tol) || !(xx * zz - xz * xz >= -tol * tol) || !(yy * zz - yz * yz >= -tol * tol)) return false;
    const double det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz);
    return det >= -tol * tol * tol;
}

// osot_dyn_create's checks and the device image (no device is touched): shared with the host build of the kernel (tests/emu/dyn_host.cpp)
inline int dyn_build(const osot_kin_desc* t, const osot_dyn_desc* in, DevDyn& h, const char** why) {
    if (!t || !in) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (t->n < 1 || t->n > OSOT_KIN_MAX_JOINTS) { *why = "joint count out of range"; return OSOT_ERR_INVALID; }
    if (t->n_frames < 0 || t->n_frames > OSOT_KIN_MAX_FRAMES) { *why = "frame count out of range"; return OSOT_ERR_INVALID; }
    for (int j = 0; j < t->n; ++j) {
        if (t->parent[j] >= j || t->parent[j] < -1) { *why = "joints must be in tree order (parent[j] < j)"; return OSOT_ERR_INVALID; }
        if (t->type[j] != OSOT_JOINT_REVOLUTE && t->type[j] != OSOT_JOINT_PRISMATIC) { *why = "unknown joint type"; return OSOT_ERR_INVALID; }
        double a2 = 0.0;
        bool finite = std::isfinite(t->mass[j]);
        for (int i = 0; i < 3; ++i) { a2 += t->axis[j][i] * t->axis[j][i]; finite = finite && std::isfinite(t->p0[j][i]) && std::isfinite(t->com[j][i]); }
        for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(t->R0[j][i]);
        for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(in->inertia[j][i]);
        if (!finite || !std::isfinite(a2)) { *why = "the model holds a NaN or an infinity"; return OSOT_ERR_INVALID; }
        if (!(std::fabs(a2 - 1.0) <= 1.0e-9)) { *why = "joint axes must be unit vectors"; return OSOT_ERR_INVALID; }
        if (!(t->mass[j] >= 0.0)) { *why = "negative link mass"; return OSOT_ERR_INVALID; }
        const double* I = in->inertia[j];
        const double tr = I[0] + I[3] + I[5];
        const double tol = 1.0e-12 * (std::fabs(tr) > 1.0e-300 ? std::fabs(tr) : 1.0e-300);
        if (!dyn_psd3(I, tol)) { *why = "an inertia tensor is not positive semi-definite"; return OSOT_ERR_INVALID; }
        // principal moments I1 + I2 >= I3 for every ordering  <=>  tr(I) / 2 E - I is positive semi-definite
        const double T[6] = {0.5 * tr - I[0], -I[1], -I[2], 0.5 * tr - I[3], -I[4], 0.5 * tr - I[5]};
        if (!dyn_psd3(T, tol)) { *why = "an inertia tensor violates the triangle inequalities of its principal moments"; return OSOT_ERR_INVALID; }
    }
    for (int i = 0; i < 3; ++i) if (!std::isfinite(in->gravity[i])) { *why = "the model holds a NaN or an infinity"; return OSOT_ERR_INVALID; }
    {
        const int rc = kin_check_frames(t, why);
        if (rc != OSOT_OK) return rc;
    }
    for (int f = 0; f < t->n_frames; ++f) {
        bool finite = true;
        for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(t->frame_R[f][i]);
        for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(t->frame_p[f][i]);
        if (!finite) { *why = "the model holds a NaN or an infinity"; return OSOT_ERR_INVALID; }
    }
    double mt = 0.0;
    for (int j = 0; j < t->n; ++j) mt += t->mass[j];
    if (!(mt > 0.0)) { *why = "the model has no mass"; return OSOT_ERR_INVALID; }
    std::memset(&h, 0, sizeof(h));
    h.k.d = *t;
    h.k.d.n_pairs = 0;
    kin_build_tables(h.k);
    for (int j = 0; j < t->n; ++j) for (int i = 0; i < 6; ++i) h.inertia[j][i] = in->inertia[j][i];
    for (int i = 0; i < 3; ++i) h.gravity[i] = in->gravity[i];
    return OSOT_OK;
}

// osot_dynamics' checks of a batch against the tree
inline int dyn_check_batch(const osot_kin_desc& t, const osot_dyn_batch* b, const char** why) {
    if (!b) { *why = "null argument"; return OSOT_ERR_INVALID; }
    if (b->B < 0) { *why = "negative batch"; return OSOT_ERR_INVALID; }
    if (b->B == 0) return OSOT_OK;
    if (!b->q) { *why = "q is null"; return OSOT_ERR_INVALID; }
    if (b->M && b->M_stride < (long long)t.n * t.n) { *why = "M_stride is below n * n"; return OSOT_ERR_INVALID; }
    for (int f = 0; f < OSOT_KIN_MAX_FRAMES; ++f) {
        if (!b->frame_Jdot_qdot[f]) continue;
        if (f >= t.n_frames) { *why = "Jdot qdot asked for a frame the model does not have"; return OSOT_ERR_INVALID; }
        if (t.frame_base[f] != 0 || t.frame_body[f] != 0) {
            *why = "Jdot qdot of a frame with a relative base link or a BODY Jacobian is not offered (world frames only)";
            return OSOT_ERR_UNSUPPORTED;
        }
        if (b->frame_Jdot_qdot_stride[f] < 6) { *why = "frame_Jdot_qdot_stride is below 6"; return OSOT_ERR_INVALID; }
    }
    if (b->com_Jdot_qdot && b->com_Jdot_qdot_stride < 3) { *why = "com_Jdot_qdot_stride is below 3"; return OSOT_ERR_INVALID; }
    const struct { const double* p; long long stride; int ld; } rows[2] = {{b->cmm_lin, b->cmm_lin_stride, b->cmm_lin_ld},
                                                                           {b->cmm_ang, b->cmm_ang_stride, b->cmm_ang_ld}};
    for (int i = 0; i < 2; ++i) {
        if (!rows[i].p) continue;
        const long long ld = rows[i].ld ? rows[i].ld : t.n;
        if (ld < t.n) { *why = "a momentum matrix row length (ld) is below n"; return OSOT_ERR_INVALID; }
        if (rows[i].stride < 3 * ld) { *why = "a momentum matrix stride is below 3 * ld"; return OSOT_ERR_INVALID; }
    }
    if (b->momentum && b->momentum_stride < 6) { *why = "momentum_stride is below 6"; return OSOT_ERR_INVALID; }
    if (b->ang_mom_b && b->ang_mom_b_stride < 3) { *why = "ang_mom_b_stride is below 3"; return OSOT_ERR_INVALID; }
    if (!b->ang_mom_b && (b->ang_mom_ref || b->ang_mom_rate_ref)) { *why = "ang_mom_ref / ang_mom_rate_ref without ang_mom_b"; return OSOT_ERR_INVALID; }
    bool finite = std::isfinite(b->ang_mom_lambda);
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(b->ang_mom_gain[i]);
    if (!finite) { *why = "ang_mom_gain or ang_mom_lambda is not finite"; return OSOT_ERR_INVALID; }
    return OSOT_OK;
}

// which instantiation of osot_dyn_kernel a batch runs: DYN_PLAIN has no stage 5a and keeps the early returns of stages 4 and 5 (a
// batch that binds no centroidal momentum output pays nothing for them), DYN_MOMENTUM forces those stages and adds 5a; DYN_ANY
// decides per launch (the host build of the tests, which launches osot_dyn_kernel<64>)
enum { DYN_PLAIN = 0, DYN_MOMENTUM = 1, DYN_ANY = 2 };
__host__ __device__ inline bool dyn_wants_momentum(const osot_dyn_batch& b) { return b.cmm_lin || b.cmm_ang || b.momentum || b.ang_mom_b; }

// the kinematics batch the kernel hands to kin_instance: same B and q, no output
inline osot_kin_batch dyn_kin_batch(const osot_dyn_batch& b) {
    osot_kin_batch kb;
    std::memset(&kb, 0, sizeof(kb));
    kb.B = b.B;
    kb.q = b.q;
    return kb;
}

// one fma chain, the same at every call site (M[r][c] and M[c][r] must agree bit for bit)
__device__ __forceinline__ double dot6(const double* a, const double* b) {
    return fma(a[5], b[5], fma(a[4], b[4], fma(a[3], b[3], fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0])))));
}

// a[] = this joint's term on entry, the sum of the terms over its ancestor chain (itself included) on return; buf [W][JMAX] then
// holds every joint's sum.  Pointer jumping: the lane keeps the sum from itself up to (excluding) its jump pointer, adds the
// pointer's sum and jumps twice as far every round.
template <int JMAX, int W>
__device__ __forceinline__ void ancestor_sum(double* buf, int* Par, const int j, const int par_j, double (&a)[W]) {
#pragma unroll
    for (int i = 0; i < W; ++i) buf[i * JMAX + j] = a[i];
    Par[j] = par_j;
    wave_sync();
    int jp = par_j;
    while (wave_ballot(jp >= 0) != 0ull) {
        const int src = jp >= 0 ? jp : j;
        double t[W];
#pragma unroll
        for (int i = 0; i < W; ++i) t[i] = buf[i * JMAX + src];
        const int njp = jp >= 0 ? Par[src] : -1;
        wave_sync();                // everybody has read this round's sums and pointers
#pragma unroll
        for (int i = 0; i < W; ++i) { a[i] += jp >= 0 ? t[i] : 0.0; buf[i * JMAX + j] = a[i]; }
        Par[j] = njp;
        jp = njp;
        wave_sync();
    }
}

// LDS of one instance, in doubles: the kinematics stages' slice, the motion subspaces [6][JMAX] and a [16][JMAX] buffer that
// holds the velocities and bias accelerations, then the prefix sums, then F_j = Ic_j S_j
template <int JMAX> constexpr int dyn_lds_doubles() { return kin_lds_doubles<JMAX>(false) + JMAX * (6 + 16); }

template <int JMAX, bool MOMENTUM>
__device__ __forceinline__ void dyn_instance(const DevDyn* __restrict__ D, const osot_dyn_batch& Bt, const osot_kin_batch& Kb,
                                             const long long inst, const bool live, const int j, double* lds) {
    constexpr int TS = OSOT_KIN_TS;
    const DevKin* __restrict__ K = &D->k;
    const int n = K->d.n;
    const int jc = (j < n) ? j : 0;
    // the lane's own model entries and qdot (their latency runs under the kinematics stages)
    double Icm[6], ax[3], comj[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) Icm[i] = D->inertia[jc][i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { ax[i] = K->d.axis[jc][i]; comj[i] = K->d.com[jc][i]; }
    const int par_model = K->d.parent[jc], type_j = K->d.type[jc], dfs_j = K->dfs_pos[jc], end_j = K->sub_end[jc];
    const double mass_j = K->d.mass[jc];
    const double grav[3] = {D->gravity[0], D->gravity[1], D->gravity[2]};
    const double qd_in = Bt.qdot ? Bt.qdot[(live ? inst : 0) * n + jc] : 0.0;
    // ---- the kinematics producer's own stages with no output bound: local transforms, world transforms by pointer jumping, world
    // frames.  They leave the world [R | p] of every joint and of every frame in LDS (kin_instance's layout).
    // (Kb: a kinematics batch of the same B and q with every output NULL, made by the host -- dyn_kin_batch -- so that it sits in
    //  the kernel arguments like the kinematics kernel's own: a copy built here would be indexed by frame from scratch)
    kin_instance<false, JMAX>(K, Kb, inst, live, j, lds);
    // kin_instance's LDS layout, restated: [R | p] per joint (TS doubles), world axes (3), m [c, 1] (4), ancestor masks, parents, then
    // 14 doubles per frame ([R | p], joint, options) and a mask per frame.  The sum is tied to kin_lds_doubles so that a change of
    // that layout does not go unnoticed here.
    static_assert(kin_lds_doubles<JMAX>(false) == JMAX * TS + JMAX * 3 + JMAX * 4 + JMAX + (JMAX + 1) / 2 + OSOT_KIN_MAX_FRAMES * (14 + 1),
                  "osot_dyn.h restates the LDS layout of kin_instance (osot_kin.h): update both");
    const double* Tw = lds;
    unsigned long long* Anc = reinterpret_cast<unsigned long long*>(lds + JMAX * TS + JMAX * 3 + JMAX * 4);
    int* Par = reinterpret_cast<int*>(Anc + JMAX);
    const double* Fw = reinterpret_cast<const double*>(Par + 2 * ((JMAX + 1) / 2));
    double* Sd = lds + kin_lds_doubles<JMAX>(false);
    double* X = Sd + JMAX * 6;
    const bool valid = j < n && live;
    const bool revolute = valid && type_j == OSOT_JOINT_REVOLUTE;
    const int par_j = valid ? par_model : -1;
    const double qd = valid ? qd_in : 0.0;
    struct { double Rw[9], pw[3], zj[3], comj[3], mass_j; int dfs_j, end_j; } L;     // (joints beyond n wrote nothing: zeros)
#pragma unroll
    for (int i = 0; i < 9; ++i) L.Rw[i] = valid ? Tw[j * TS + i] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) L.pw[i] = valid ? Tw[j * TS + 9 + i] : 0.0;
    mat3_vec(L.Rw, ax, L.zj);
#pragma unroll
    for (int i = 0; i < 3; ++i) L.comj[i] = comj[i];
    L.mass_j = mass_j; L.dfs_j = dfs_j; L.end_j = end_j;
    // ---- 1. motion subspace and link inertia about the world origin
    double S[6];
    {
        double pz[3];
        cross3(L.pw, L.zj, pz);
#pragma unroll
        for (int i = 0; i < 3; ++i) { S[i] = revolute ? L.zj[i] : 0.0; S[3 + i] = revolute ? pz[i] : L.zj[i]; }   // (zj = 0 beyond n)
#pragma unroll
        for (int i = 0; i < 6; ++i) Sd[i * JMAX + j] = S[i];
    }
    const double m = valid ? L.mass_j : 0.0;
    double c[3], hm[3], Io[6];
    {
        double cl[3];
        mat3_vec(L.Rw, L.comj, cl);
#pragma unroll
        for (int i = 0; i < 3; ++i) { c[i] = cl[i] + L.pw[i]; hm[i] = m * c[i]; }
        const double Is[9] = {Icm[0], Icm[1], Icm[2], Icm[1], Icm[3], Icm[4], Icm[2], Icm[4], Icm[5]};
        double RI[9];
        mat3_mul(L.Rw, Is, RI);
        const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
        // R I R' (upper triangle) + m (c.c E - c c')
        const int ra[6] = {0, 0, 0, 1, 1, 2}, rb[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int a = ra[k], b = rb[k];
            const double rir = RI[3 * a] * L.Rw[3 * b] + RI[3 * a + 1] * L.Rw[3 * b + 1] + RI[3 * a + 2] * L.Rw[3 * b + 2];
            Io[k] = valid ? rir + m * ((a == b ? cc : 0.0) - c[a] * c[b]) : 0.0;
        }
    }
    // ---- 2. link velocities and bias accelerations: sums over the ancestor chains
    double v[6], ab[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = S[i] * qd;
    ancestor_sum<JMAX, 6>(X, Par, j, par_j, v);
    {
        double w1[3], w2[3], w3[3];
        cross3(v, S, w1);              // omega x s_w
        cross3(v, S + 3, w2);          // omega x s_v
        cross3(v + 3, S, w3);          // v_o x s_w
#pragma unroll
        for (int i = 0; i < 3; ++i) { ab[i] = w1[i] * qd; ab[3 + i] = (w2[i] + w3[i]) * qd; }
    }
    ancestor_sum<JMAX, 6>(X + 6 * JMAX, Par, j, par_j, ab);
    // ---- 3. Jdot qdot of the frames (lane = frame) and of the centre of mass
    const int nfr = K->d.n_frames;
    {
        const int f = (j < nfr) ? j : 0;
        const int jf = K->d.frame_joint[f];
        double* out = nullptr;             // (a select chain: a lane-indexed read of the argument struct would go through scratch)
        long long ostride = 0;
#pragma unroll
        for (int ff = 0; ff < OSOT_KIN_MAX_FRAMES; ++ff) {
            out = (f == ff) ? Bt.frame_Jdot_qdot[ff] : out;
            ostride = (f == ff) ? Bt.frame_Jdot_qdot_stride[ff] : ostride;
        }
        double p[3], vf[6], af[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = Fw[f * 14 + 9 + i];      // the frame's world origin (kin_instance, stage 3a)
#pragma unroll
        for (int i = 0; i < 6; ++i) { vf[i] = X[i * JMAX + jf]; af[i] = X[(6 + i) * JMAX + jf]; }
        double wp[3], vp[3], ap[3], wv[3];
        cross3(vf, p, wp);
#pragma unroll
        for (int i = 0; i < 3; ++i) vp[i] = vf[3 + i] + wp[i];
        cross3(af, p, ap);
        cross3(vf, vp, wv);
        if (j < nfr && out && live) {
            double* o = out + inst * ostride;
#pragma unroll
            for (int i = 0; i < 3; ++i) { o[i] = af[3 + i] + ap[i] + wv[i]; o[3 + i] = af[i]; }
        }
    }
    if (Bt.com_Jdot_qdot) {
        double wc[3], vc[3], ac[3], wv[3];
        cross3(v, c, wc);
#pragma unroll
        for (int i = 0; i < 3; ++i) vc[i] = v[3 + i] + wc[i];
        cross3(ab, c, ac);
        cross3(v, vc, wv);
        const double iM = fast_rcp(K->total_mass);
        double s[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = colsum<JMAX>(m * (ab[3 + i] + ac[i] + wv[i])) * iM;
        if (j == 0 && live) {
            double* o = Bt.com_Jdot_qdot + inst * Bt.com_Jdot_qdot_stride;
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = s[i];
        }
    }
    if (!MOMENTUM && !Bt.M && !Bt.h) return;          // (the momentum outputs need the subtree aggregates and F_j)
    // ---- 4. link wrench; subtree aggregates of [m, m c, Io, wrench] as differences of prefix sums over the depth-first order
    double agg[16];
    {
        const double ag[3] = {ab[3] - grav[0], ab[4] - grav[1], ab[5] - grav[2]};     // (gravity as an acceleration of the base)
        double Ivn[3], Ivf[3], t1[3], t2[3];
        // I v = [Io omega + h x v_o; m v_o - h x omega],  I a likewise
        const double Iw[3] = {Io[0] * v[0] + Io[1] * v[1] + Io[2] * v[2], Io[1] * v[0] + Io[3] * v[1] + Io[4] * v[2],
                              Io[2] * v[0] + Io[4] * v[1] + Io[5] * v[2]};
        const double Ia[3] = {Io[0] * ab[0] + Io[1] * ab[1] + Io[2] * ab[2], Io[1] * ab[0] + Io[3] * ab[1] + Io[4] * ab[2],
                              Io[2] * ab[0] + Io[4] * ab[1] + Io[5] * ab[2]};
        cross3(hm, v + 3, t1);
        cross3(hm, v, t2);
#pragma unroll
        for (int i = 0; i < 3; ++i) { Ivn[i] = Iw[i] + t1[i]; Ivf[i] = m * v[3 + i] - t2[i]; }
        double a1[3], a2[3], c1[3], c2[3], c3[3];
        cross3(hm, ag, a1);
        cross3(hm, ab, a2);
        cross3(v, Ivn, c1);            // omega x n
        cross3(v + 3, Ivf, c2);        // v_o x f
        cross3(v, Ivf, c3);            // omega x f
        agg[0] = m;
#pragma unroll
        for (int i = 0; i < 3; ++i) agg[1 + i] = hm[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) agg[4 + i] = Io[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            agg[10 + i] = valid ? (Ia[i] + a1[i]) + (c1[i] + c2[i]) : 0.0;
            agg[13 + i] = valid ? (m * ag[i] - a2[i]) + c3[i] : 0.0;
        }
    }
    wave_sync();                       // the frames have read the velocities and accelerations this buffer held
    {
        const int pos = valid ? L.dfs_j : j;      // (joints beyond n: zeros at their own index, which no joint below n has)
#pragma unroll
        for (int i = 0; i < 16; ++i) X[i * JMAX + pos] = agg[i];
    }
    wave_sync();
#pragma unroll
    for (int i = 0; i < 16; ++i) agg[i] = X[i * JMAX + j];
#pragma unroll
    for (int d = 1; d < JMAX; d <<= 1) {
        double t[16];
        const int src = (j >= d) ? j - d : 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = X[i * JMAX + src];
        wave_sync();
#pragma unroll
        for (int i = 0; i < 16; ++i) { agg[i] += (j >= d) ? t[i] : 0.0; X[i * JMAX + j] = agg[i]; }
        wave_sync();
    }
    {
        const int hi = valid ? L.end_j - 1 : 0, lo = (valid && L.dfs_j > 0) ? L.dfs_j - 1 : 0;
        const bool from0 = !(valid && L.dfs_j > 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const double ph = X[i * JMAX + hi], pl = X[i * JMAX + lo];
            agg[i] = ph - (from0 ? 0.0 : pl);
        }
    }
    // ---- 5. h_j = S_j . f_subtree(j);  F_j = Ic_j S_j;  the rows of M
    if (Bt.h && valid) Bt.h[inst * n + j] = dot6(S, agg + 10);
    if (!MOMENTUM && !Bt.M) return;
    double F[6];
    {
        const double* hc = agg + 1;
        const double* Ic = agg + 4;
        double t1[3], t2[3];
        cross3(hc, S + 3, t1);
        cross3(hc, S, t2);
        F[0] = Ic[0] * S[0] + Ic[1] * S[1] + Ic[2] * S[2] + t1[0];
        F[1] = Ic[1] * S[0] + Ic[3] * S[1] + Ic[4] * S[2] + t1[1];
        F[2] = Ic[2] * S[0] + Ic[4] * S[1] + Ic[5] * S[2] + t1[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) F[3 + i] = agg[0] * S[3 + i] - t2[i];
    }
    // ---- 5a. centroidal momentum: F_j is the spatial momentum of the subtree joint j moves per unit qdot_j, about the world
    // origin; moved to the centre of mass c_G it is column j of the momentum matrix, [linear f_j; angular n_j - c_G x f_j].
    // The last prefix sum is the whole tree's [m, m c].
    if (MOMENTUM) {
        const double iM = fast_rcp(K->total_mass);
        double cG[3], cf[3], col[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) cG[i] = X[(1 + i) * JMAX + (n - 1)] * iM;
        cross3(cG, F + 3, cf);
#pragma unroll
        for (int i = 0; i < 3; ++i) { col[i] = valid ? F[3 + i] : 0.0; col[3 + i] = valid ? F[i] - cf[i] : 0.0; }
        if (Bt.cmm_lin && valid) {
            const long long ld = Bt.cmm_lin_ld ? Bt.cmm_lin_ld : n;
            double* o = Bt.cmm_lin + inst * Bt.cmm_lin_stride + j;
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i * ld] = col[i];
        }
        if (Bt.cmm_ang && valid) {
            const long long ld = Bt.cmm_ang_ld ? Bt.cmm_ang_ld : n;
            double* o = Bt.cmm_ang + inst * Bt.cmm_ang_stride + j;
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i * ld] = col[3 + i];
        }
        if (Bt.momentum || Bt.ang_mom_b) {
            double hG[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) hG[i] = colsum<JMAX>(col[i] * qd);
            if (Bt.momentum && j == 0 && live) {
                double* o = Bt.momentum + inst * Bt.momentum_stride;
#pragma unroll
                for (int i = 0; i < 6; ++i) o[i] = hG[i];
            }
            if (Bt.ang_mom_b && j == 0 && live) {
                // acceleration::AngularMomentum: b = Ldot_d + lambda K (L_d - L); no reference = the task's _is_init == false
                // branch (L_d = L)
                const double* Kg = Bt.ang_mom_gain;
                bool unit = true;
#pragma unroll
                for (int i = 0; i < 9; ++i) unit = unit && Kg[i] == 0.0;
                double e[3], rate[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    e[i] = Bt.ang_mom_ref ? Bt.ang_mom_ref[inst * 3 + i] - hG[3 + i] : 0.0;
                    rate[i] = Bt.ang_mom_rate_ref ? Bt.ang_mom_rate_ref[inst * 3 + i] : 0.0;
                }
                double* o = Bt.ang_mom_b + inst * Bt.ang_mom_b_stride;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double Ke = unit ? e[i] : Kg[3 * i] * e[0] + Kg[3 * i + 1] * e[1] + Kg[3 * i + 2] * e[2];
                    o[i] = Bt.ang_mom_ref ? rate[i] + Bt.ang_mom_lambda * Ke : rate[i];
                }
            }
        }
        if (!Bt.M) return;
    }
    wave_sync();                       // everybody has read its prefix sums
#pragma unroll
    for (int i = 0; i < 6; ++i) X[i * JMAX + j] = F[i];
    wave_sync();
    const unsigned long long anc_j = Anc[j];
    double* Mi = Bt.M + (live ? inst : 0) * Bt.M_stride;
    for (int r = 0; r < n; ++r) {
        double Sr[6], Fr[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) { Sr[i] = Sd[i * JMAX + r]; Fr[i] = X[i * JMAX + r]; }
        const bool r_moves_j = ((anc_j >> r) & 1ull) != 0ull;       // r is an ancestor of j, or j itself
        const bool j_moves_r = ((Anc[r] >> j) & 1ull) != 0ull;
        double a[6], b[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) { a[i] = r_moves_j ? Sr[i] : S[i]; b[i] = r_moves_j ? F[i] : Fr[i]; }
        const double val = dot6(a, b);                               // S_ancestor . F_descendant either way
        if (valid) Mi[(long long)r * n + j] = (r_moves_j || j_moves_r) ? val : 0.0;
    }
}

template <int JMAX, int MODE = DYN_ANY>
__global__ void __launch_bounds__(64) osot_dyn_kernel(const DevDyn* __restrict__ D, const osot_dyn_batch Bt, const osot_kin_batch Kb) {
    OSOT_STATIC_LDS(double, dyn_lds, dyn_lds_doubles<JMAX>());
    const int j = (int)threadIdx.x;
    const long long inst = (long long)blockIdx.x;
    if (MODE == DYN_MOMENTUM || (MODE == DYN_ANY && dyn_wants_momentum(Bt))) dyn_instance<JMAX, true>(D, Bt, Kb, inst, inst < Bt.B, j, dyn_lds);
    else dyn_instance<JMAX, false>(D, Bt, Kb, inst, inst < Bt.B, j, dyn_lds);
}

}  // namespace osot
