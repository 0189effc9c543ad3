// tests/emu/feedback_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The measurement-driven producer (opensot_amd/csrc/osot_feedback.h) through the host lock-step emulation of
// tests/emu/hip/hip_runtime.h, with the checks of osot_feedback (feedback_check) and its two host helpers.  Built by
// tests/feedback_ref.py; used by tests/test_feedback_host.py (no GPU needed) and as the reference of tests/test_feedback_gpu.py.
// libosot_mi355x.so launches the same kernel body.
// With -DOSOT_FEEDBACK_MAIN it is a stand-alone program (for -fsanitize=address,undefined): three shapes, three calls each, into
// destinations fenced by sentinels, every input array of its exact size on the heap.
#include <osot_team.h>
#include "osot_feedback.h"

using namespace osot;

#define FEEDBACK_API extern "C" __attribute__((visibility("default")))

// osot_feedback's answer to its arguments alone -> code, *why = the reason
FEEDBACK_API int feedback_host_check(const osot_feedback_model* m, const osot_feedback_batch* b, const char** why) {
    static const char* none = "";
    *why = none;
    return feedback_check(m, b, why);
}

FEEDBACK_API int feedback_host_run(const osot_feedback_model* m, const osot_feedback_batch* b) {
    const char* why = "";
    const int rc = feedback_check(m, b, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "feedback host: %s\n", why); return rc; }
    if (b->B == 0) return OSOT_OK;
    FeedbackCoeffs k;
    feedback_coeffs(m, &k);
    emu::launch(osot_feedback_kernel, (unsigned)b->B, (size_t)feedback_lds_bytes(m, b), 64, *m, *b, k);
    return OSOT_OK;
}

// out = {a0, a1, a2, 1 / a0} as osot_feedback computes them
FEEDBACK_API void feedback_host_coeff(double omega, double eps, double ts, double* out) {
    double c[3], a0;
    feedback_filter_coeff(omega, eps, ts, c, &a0);
    out[0] = a0; out[1] = c[1]; out[2] = c[2]; out[3] = c[0];
}

FEEDBACK_API int feedback_host_state_doubles(const osot_feedback_model* m) { return feedback_state_count(m); }

FEEDBACK_API int feedback_host_admittance_params(const double* K, const double* D, double lambda, double dt, double* C, double* M, double* w,
                                                 const char** why) {
    static const char* none = "";
    *why = none;
    return feedback_admittance_params(K, D, lambda, dt, C, M, w, why);
}

#ifdef OSOT_FEEDBACK_MAIN
#include <memory>

namespace {
const double kSentinel = -7.25e300;
unsigned long long g_seed = 0x9E3779B97F4A7C15ull;
double rnd() {   // xorshift64*, uniform in (-1, 1)
    g_seed ^= g_seed >> 12; g_seed ^= g_seed << 25; g_seed ^= g_seed >> 27;
    return (double)((g_seed * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}
std::unique_ptr<double[]> filled(size_t count, int how) {   // how: 0 = sentinel, 1 = random, 2 = zero
    std::unique_ptr<double[]> p(new double[count]);
    for (size_t i = 0; i < count; ++i) p[i] = how == 1 ? rnd() : how == 2 ? 0.0 : kSentinel;
    return p;
}
void rotations(double* T, int B) {   // proper rotations about z in front of the random origins
    for (int i = 0; i < B; ++i) {
        const double a = 3.0 * rnd();
        const double R[9] = {cos(a), -sin(a), 0, sin(a), cos(a), 0, 0, 0, 1};
        memcpy(T + 12 * i, R, sizeof(R));
    }
}

// one shape: every group bound, ld = n + pad, three calls; returns the number of failed expectations
int run_shape(int B, int nv, int n_cart, int n_pairs, int n, int pad, bool dense) {
    const int ld = n + pad, ild = 6 + pad;
    osot_feedback_model M;
    memset(&M, 0, sizeof(M));
    M.nv = nv; M.floating_base = 1; M.n_cart = n_cart; M.joint = 1; M.imu = nv >= 6; M.n_pairs = n_pairs; M.n = n;
    for (int c = 0; c < 6 * n_cart; ++c) { M.cart_C[c] = 1e-3 * (2.0 + rnd()); M.cart_deadzone[c] = 0.25 * (1.0 + rnd()); M.cart_omega[c] = 20.0 + 10.0 * rnd(); M.cart_damping[c] = 1.0 + 0.5 * rnd(); }
    for (int t = 0; t < n_cart; ++t) M.cart_ts[t] = 0.002 * (t + 1);
    M.joint_omega = 50.0; M.joint_damping = 1.0; M.joint_ts = 0.002; M.joint_C_scalar = 0.00015; M.contact_lambda = 0.3; M.ca_threshold = 0.01;
    osot_feedback_batch Bt;
    memset(&Bt, 0, sizeof(Bt));
    Bt.B = B;
    const int count = feedback_state_count(&M);
    auto state = filled((size_t)B * count, 2);
    Bt.state = state.get();
    std::unique_ptr<double[]> pose[OSOT_FEEDBACK_MAX_CART], wrench[OSOT_FEEDBACK_MAX_CART], wref[OSOT_FEEDBACK_MAX_CART], tin[OSOT_FEEDBACK_MAX_CART], tout[OSOT_FEEDBACK_MAX_CART];
    for (int t = 0; t < n_cart; ++t) {
        pose[t] = filled((size_t)B * 12, 1); rotations(pose[t].get(), B);
        wrench[t] = filled((size_t)B * 6, 1); wref[t] = filled((size_t)B * 6, 1); tin[t] = filled((size_t)B * 6, 1); tout[t] = filled((size_t)B * 6, 0);
        Bt.cart_pose[t] = pose[t].get(); Bt.cart_wrench[t] = wrench[t].get(); Bt.cart_wrench_ref[t] = wref[t].get();
        Bt.cart_twist_in[t] = tin[t].get(); Bt.cart_twist_out[t] = tout[t].get();
    }
    auto tau = filled((size_t)B * nv, 1), h = filled((size_t)B * nv, 1), Cd = filled((size_t)nv * nv, 1), qd = filled((size_t)B * nv, 0);
    Bt.joint_tau = tau.get(); Bt.joint_h = h.get(); Bt.joint_C = dense ? Cd.get() : nullptr; Bt.joint_qdot_out = qd.get();
    auto fbJ = filled((size_t)B * 6 * nv, 1), ipose = filled((size_t)B * 12, 1), iom = filled((size_t)B * 3, 1);
    auto iA = filled((size_t)B * 6 * ild, 0), ib = filled((size_t)B * 6, 0);
    rotations(ipose.get(), B);
    if (M.imu) {
        Bt.imu_fb_J = fbJ.get(); Bt.imu_fb_J_stride = 6 * nv; Bt.imu_pose = ipose.get(); Bt.imu_omega = iom.get();
        Bt.imu_A = iA.get(); Bt.imu_A_stride = 6 * ild; Bt.imu_A_ld = ild; Bt.imu_b = ib.get(); Bt.imu_b_stride = 6;
    }
    auto cp = filled((size_t)B * 12, 1), cr = filled((size_t)B * 12, 1), cin = filled((size_t)B * 6, 1), cout = filled((size_t)B * 6, 0);
    rotations(cp.get(), B); rotations(cr.get(), B);
    Bt.contact_pose = cp.get(); Bt.contact_pose_ref = cr.get(); Bt.contact_b_in = cin.get(); Bt.contact_b_in_stride = 6;
    Bt.contact_b_out = cout.get(); Bt.contact_b_out_stride = 6;
    auto J = filled((size_t)B * n_pairs * n, 1), dist = filled((size_t)B * n_pairs, 1), A = filled((size_t)B * n_pairs * ld, 0), cb = filled((size_t)B * n_pairs, 0);
    for (int i = 0; i < B * n_pairs; ++i) dist[i] = (i % 3 == 0) ? M.ca_threshold : 0.05 * dist[i];
    Bt.ca_J = J.get(); Bt.ca_J_stride = (long long)n_pairs * n; Bt.ca_dist = dist.get();
    Bt.ca_A = A.get(); Bt.ca_A_stride = (long long)n_pairs * ld; Bt.ca_A_ld = ld; Bt.ca_b = cb.get(); Bt.ca_b_stride = n_pairs;
    for (int call = 0; call < 3; ++call)
        if (feedback_host_run(&M, &Bt) != OSOT_OK) return 1;
    // expectations: copies and negations are exact, the untouched columns keep the sentinel, everything else is finite
    int bad = 0;
    for (int i = 0; i < B; ++i) {
        for (int p = 0; p < n_pairs; ++p) {
            const bool violated = !(dist[i * n_pairs + p] - M.ca_threshold > 0.0);
            bad += (cb[i * n_pairs + p] != (violated ? dist[i * n_pairs + p] - M.ca_threshold : 0.0));
            for (int c = 0; c < ld; ++c) {
                const double a = A[((size_t)i * n_pairs + p) * ld + c];
                bad += (c >= n) ? (a != kSentinel) : (a != (violated ? -J[((size_t)i * n_pairs + p) * n + c] : 0.0));
            }
        }
        if (M.imu)
            for (int r = 0; r < 6; ++r) {
                for (int c = 0; c < ild; ++c) {
                    const double a = iA[((size_t)i * 6 + r) * ild + c];
                    bad += (c >= 6) ? (a != kSentinel) : (a != (r < 3 ? 0.0 : fbJ[((size_t)i * 6 + r) * nv + c]));
                }
                bad += (r < 3) ? (ib[i * 6 + r] != 0.0) : !std::isfinite(ib[i * 6 + r]);
            }
        for (int c = 0; c < 6; ++c) bad += !std::isfinite(cout[i * 6 + c]);
        for (int j = 0; j < nv; ++j) bad += (j < 6) ? (qd[i * nv + j] != 0.0) : !std::isfinite(qd[i * nv + j]);
        for (int t = 0; t < n_cart; ++t) for (int c = 0; c < 6; ++c) bad += !std::isfinite(tout[t][i * 6 + c]);
        for (int k = 0; k < count; ++k) bad += !std::isfinite(state[(size_t)i * count + k]);
    }
    printf("feedback: B = %d nv = %d n_cart = %d n_pairs = %d n = %d ld = %d %s: %d failed expectations\n", B, nv, n_cart, n_pairs, n, ld,
           dense ? "dense" : "scalar", bad);
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    bad += run_shape(3, 7, 1, 1, 7, 0, false);       // one actuated coordinate, one pair
    bad += run_shape(2, 64, 8, 32, 106, 3, true);    // every lane busy, both column halves, the staging array full
    bad += run_shape(65, 35, 2, 16, 35, 5, true);    // more instances than lanes, ld > n
    if (bad) { printf("feedback: FAILED\n"); return 1; }
    printf("feedback: ok\n");
    return 0;
}
#endif
