// tests/emu/acc_tasks_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The acceleration-leaf producer (opensot_amd/csrc/osot_acc.h) through the host lock-step emulation of
// tests/emu/hip/hip_runtime.h, with the checks of osot_acc_tasks (acc_check).  Built by tests/acc_ref.py; used by
// tests/test_acc_tasks_host.py (no GPU needed) and as the reference of tests/test_acc_tasks_gpu.py.  libosot_mi355x.so launches
// the same kernel body.
// With -DOSOT_ACC_TASKS_MAIN it is a stand-alone program (for -fsanitize=address,undefined): the largest shape (nv = 64, eight
// Force-type Cartesian terms, CoM, a Force-type postural term, Minv) and the smallest (nv = 1, postural only), every array of
// its exact size on the heap, one instance of the large batch with a singular M.
#include <osot_team.h>
#include "osot_acc.h"

using namespace osot;

#define ACC_API extern "C" __attribute__((visibility("default")))

// osot_acc_tasks' answer to its arguments alone -> code, *why = the reason
ACC_API int acc_host_check(const osot_acc_model* m, const osot_acc_batch* b, const char** why) {
    static const char* none = "";
    *why = none;
    return acc_check(m, b, why);
}

ACC_API int acc_host_tasks(const osot_acc_model* m, const osot_acc_batch* b) {
    const char* why = "";
    const int rc = acc_check(m, b, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "acc host: %s\n", why); return rc; }
    if (b->B == 0) return OSOT_OK;
    AccArgs A;
    A.M = *m; A.Bt = *b;
    emu::launch(osot_acc_tasks_kernel, (unsigned)b->B, (size_t)acc_lds_bytes(m, b), 64, A);
    return OSOT_OK;
}

ACC_API int acc_host_lds_bytes(const osot_acc_model* m, const osot_acc_batch* b) { return acc_lds_bytes(m, b); }
ACC_API double acc_host_pivot_rel(int nv) { return acc_pivot_rel(nv); }

#ifdef OSOT_ACC_TASKS_MAIN
#include <memory>

namespace {
const double kSentinel = -7.25e300;
unsigned long long g_seed = 0x9E3779B97F4A7C15ull;
double rnd() {   // xorshift64*, uniform in (-1, 1)
    g_seed ^= g_seed >> 12; g_seed ^= g_seed << 25; g_seed ^= g_seed >> 27;
    return (double)((g_seed * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}
std::unique_ptr<double[]> filled(size_t count, bool random) {
    std::unique_ptr<double[]> p(new double[count]);
    for (size_t i = 0; i < count; ++i) p[i] = random ? rnd() : kSentinel;
    return p;
}
int count_bad(const double* p, size_t n, bool want_zero) {
    int bad = 0;
    for (size_t i = 0; i < n; ++i) bad += want_zero ? (p[i] != 0.0) : !std::isfinite(p[i]) || p[i] == kSentinel;
    return bad;
}

// one shape, every output bound; instance `singular` (or none: -1) gets a zero row and column in M
int run_shape(int B, int nv, int nc, bool com, bool post, int singular) {
    osot_acc_model M;
    memset(&M, 0, sizeof(M));
    M.nv = nv; M.n_cart = nc; M.has_com = com; M.com_gain_matrices = com; M.has_postural = post;
    M.post_gain_type = OSOT_ACC_GAIN_FORCE; M.post_gain_matrices = 1; M.post_lambda = 10.0; M.post_lambda2 = 2.0;
    for (int t = 0; t < nc; ++t) { M.cart_gain_type[t] = OSOT_ACC_GAIN_FORCE; M.cart_gain_matrices[t] = 1; M.cart_orientation_gain[t] = 0.5; }
    for (int i = 0; i < 36 * nc; ++i) { M.cart_Kp[i] = rnd(); M.cart_Kd[i] = rnd(); }
    for (int i = 0; i < 9; ++i) { M.com_Kp[i] = rnd(); M.com_Kd[i] = rnd(); }
    auto Kp = filled((size_t)nv * nv, true), Kd = filled((size_t)nv * nv, true);
    if (post) { M.post_Kp = Kp.get(); M.post_Kd = Kd.get(); }
    osot_acc_batch Bt;
    memset(&Bt, 0, sizeof(Bt));
    Bt.B = B;
    auto q = filled((size_t)B * nv, true), qd = filled((size_t)B * nv, true), Mm = filled((size_t)B * nv * nv, false);
    for (int i = 0; i < B; ++i) {   // M = A A' + nv I, lower triangle only (the upper stays a sentinel: it is not read)
        auto Am = filled((size_t)nv * nv, true);
        for (int r = 0; r < nv; ++r)
            for (int c = 0; c <= r; ++c) {
                double s = (r == c) ? (double)nv : 0.0;
                for (int k = 0; k < nv; ++k) s += Am[r * nv + k] * Am[c * nv + k];
                Mm[((size_t)i * nv + r) * nv + c] = s;
            }
        if (i == singular) {
            const int z = nv / 2;
            for (int r = z; r < nv; ++r) Mm[((size_t)i * nv + r) * nv + z] = 0.0;
            for (int c = 0; c <= z; ++c) Mm[((size_t)i * nv + z) * nv + c] = 0.0;
        }
    }
    Bt.q = q.get(); Bt.qdot = qd.get(); Bt.M = Mm.get(); Bt.M_stride = (long long)nv * nv;
    std::unique_ptr<double[]> J[8], pose[8], pref[8], vref[8], fv[8], ain[8], p0[8], aout[8], Mi[8];
    for (int t = 0; t < nc; ++t) {
        J[t] = filled((size_t)B * 6 * nv, true); vref[t] = filled((size_t)B * 6, true); fv[t] = filled((size_t)B * 6, true);
        ain[t] = filled((size_t)B * 6, true); p0[t] = filled((size_t)B * 84, false); aout[t] = filled((size_t)B * 6, false);
        Mi[t] = filled((size_t)B * 36, false); pose[t] = filled((size_t)B * 12, true); pref[t] = filled((size_t)B * 12, true);
        for (int i = 0; i < B; ++i)
            for (int w = 0; w < 2; ++w) {   // proper rotations: about z by a random angle
                double* T = (w ? pref[t] : pose[t]).get() + i * 12;
                const double a = 3.0 * rnd();
                const double R[9] = {cos(a), -sin(a), 0, sin(a), cos(a), 0, 0, 0, 1};
                memcpy(T, R, sizeof(R));
            }
        Bt.cart_J[t] = J[t].get(); Bt.cart_J_stride[t] = 6 * nv; Bt.cart_J_ld[t] = nv;
        Bt.cart_pose[t] = pose[t].get(); Bt.cart_pose_ref[t] = pref[t].get(); Bt.cart_vel_ref[t] = vref[t].get();
        Bt.cart_f_virtual[t] = fv[t].get(); Bt.cart_a_ref_in[t] = ain[t].get();
        Bt.cart_p0[t] = p0[t].get(); Bt.cart_p0_stride[t] = 84; Bt.cart_a_ref_out[t] = aout[t].get(); Bt.cart_Mi[t] = Mi[t].get();
    }
    auto Jc = filled((size_t)B * 3 * nv, true), c3 = filled((size_t)B * 3, true), cp0 = filled((size_t)B * 24, false);
    if (com) {
        Bt.com_J = Jc.get(); Bt.com_J_stride = 3 * nv; Bt.com_J_ld = nv; Bt.com = c3.get(); Bt.com_ref = q.get(); Bt.com_vel_ref = c3.get();
        Bt.com_p0 = cp0.get(); Bt.com_p0_stride = 24;
    }
    auto qr = filled((size_t)B * nv, true), pp0 = filled((size_t)B * 2 * nv, false), qdd = filled((size_t)B * nv, false);
    if (post) { Bt.post_q_ref = qr.get(); Bt.post_qdot_ref = qr.get(); Bt.post_qddot_ref = qr.get(); Bt.post_p0 = pp0.get(); Bt.post_qddot_out = qdd.get(); }
    auto Minv = filled((size_t)B * nv * nv, false);
    Bt.Minv = Minv.get(); Bt.Minv_stride = (long long)nv * nv;
    std::unique_ptr<int[]> ok(new int[B]);
    for (int i = 0; i < B; ++i) ok[i] = -1;
    Bt.ok = ok.get();
    if (acc_host_tasks(&M, &Bt) != OSOT_OK) return 1;
    int bad = 0;
    for (int i = 0; i < B; ++i) {
        const bool sing = (i == singular);
        bad += (ok[i] != (sing ? 0 : 1));
        bad += count_bad(Minv.get() + (size_t)i * nv * nv, (size_t)nv * nv, sing);
        for (int t = 0; t < nc; ++t) {
            bad += count_bad(p0[t].get() + (size_t)i * 84, 12, false);
            bad += count_bad(p0[t].get() + (size_t)i * 84 + 12, 72, sing);
            bad += count_bad(Mi[t].get() + (size_t)i * 36, 36, sing);
            for (int d = 0; d < 6; ++d) bad += sing ? (aout[t][i * 6 + d] != ain[t][i * 6 + d]) : !std::isfinite(aout[t][i * 6 + d]);
        }
        if (com) bad += count_bad(cp0.get() + (size_t)i * 24, 24, false);
        if (post) {
            bad += count_bad(pp0.get() + (size_t)i * 2 * nv, 2 * (size_t)nv, false);
            for (int k = 0; k < nv; ++k) bad += sing ? (qdd[i * nv + k] != qr[i * nv + k]) : !std::isfinite(qdd[i * nv + k]);
        }
    }
    printf("acc_tasks: B = %d nv = %d n_cart = %d com = %d postural = %d: %d failed expectations\n", B, nv, nc, (int)com, (int)post, bad);
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    bad += run_shape(3, 64, 8, true, true, 1);     // the most right-hand sides, the second pass full
    bad += run_shape(2, 1, 0, false, true, -1);    // the smallest
    bad += run_shape(5, 35, 3, true, true, -1);
    if (bad) { printf("acc_tasks: FAILED\n"); return 1; }
    printf("acc_tasks: ok\n");
    return 0;
}
#endif
