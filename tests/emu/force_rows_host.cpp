// tests/emu/force_rows_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The force-space row producer (opensot_amd/csrc/osot_force.h) through the host lock-step emulation of
// tests/emu/hip/hip_runtime.h, with the checks of osot_force_rows (force_check).  Built by tests/force_ref.py; used by
// tests/test_force_rows_host.py (no GPU needed) and as the reference of tests/test_force_rows_gpu.py.  libosot_mi355x.so launches
// the same kernel body.
// With -DOSOT_FORCE_ROWS_MAIN it is a stand-alone program (for -fsanitize=address,undefined): the three shapes of the tests into
// destinations fenced by sentinels, every input array of its exact size on the heap.
#include <osot_team.h>
#include "osot_force.h"

using namespace osot;

#define FORCE_API extern "C" __attribute__((visibility("default")))

// osot_force_rows' answer to its arguments alone -> code, *why = the reason
FORCE_API int force_host_check(const osot_force_model* m, const osot_force_batch* b, const char** why) {
    static const char* none = "";
    *why = none;
    return force_check(m, b, why);
}

FORCE_API int force_host_rows(const osot_force_model* m, const osot_force_batch* b) {
    const char* why = "";
    const int rc = force_check(m, b, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "force host: %s\n", why); return rc; }
    if (b->B == 0) return OSOT_OK;
    emu::launch(osot_force_rows_kernel, (unsigned)b->B, (size_t)force_lds_bytes(m->n_contacts), 64, *m, *b);
    return OSOT_OK;
}

#ifdef OSOT_FORCE_ROWS_MAIN
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

// one shape: every output bound, ld = n + pad; returns the number of failed expectations
int run_shape(int B, int C, int nv, const int* wrench_col, int torque_col, int n, int pad) {
    const int na = nv - 6, ld = n + pad;
    osot_force_model M;
    memset(&M, 0, sizeof(M));
    M.n_contacts = C; M.nv = nv; M.n = n; M.torque_col = torque_col; M.cart_contact = C - 1;
    for (int c = 0; c < C; ++c) M.wrench_col[c] = wrench_col[c];
    M.mass = 31.5; M.gravity[2] = -9.81; M.com_lambda = 10.0; M.com_lambda2 = 2.0; M.com_lambda_ang = 0.5;
    for (int i = 0; i < 36; ++i) { M.cart_Kp[i] = rnd(); M.cart_Kd[i] = rnd(); }
    osot_force_batch Bt;
    memset(&Bt, 0, sizeof(Bt));
    Bt.B = B;
    std::unique_ptr<double[]> pose[OSOT_FORCE_MAX_CONTACTS];
    for (int c = 0; c < C; ++c) {
        pose[c] = filled((size_t)B * 12, true);
        for (int i = 0; i < B; ++i) {   // a proper rotation: about z by a random angle
            double* T = pose[c].get() + i * 12;
            const double a = 3.0 * rnd();
            const double R[9] = {cos(a), -sin(a), 0, sin(a), cos(a), 0, 0, 0, 1};
            memcpy(T, R, sizeof(R));
        }
        Bt.pose[c] = pose[c].get();
    }
    auto Jc = filled((size_t)B * C * 6 * nv, true), com = filled((size_t)B * 3, true), mom = filled((size_t)B * 6, true);
    auto hg = filled((size_t)B * nv, true), qd = filled((size_t)B * nv, true), ref3 = filled((size_t)B * 3, true);
    auto ref6 = filled((size_t)B * 6, true), qtau = filled((size_t)B * (na > 0 ? na : 1), true);
    std::unique_ptr<int[]> en(new int[(size_t)B * C]);
    for (int i = 0; i < B * C; ++i) en[i] = (i % 5 != 3);
    Bt.Jc = Jc.get(); Bt.com = com.get(); Bt.momentum = mom.get(); Bt.h_gravity = hg.get(); Bt.qdot = qd.get(); Bt.enabled = en.get();
    auto comA = filled((size_t)B * 6 * ld, false), fbA = filled((size_t)B * 6 * ld, false);
    auto stA = filled((size_t)B * (na > 0 ? na : 1) * ld, false), lo = filled((size_t)B * (na > 0 ? na : 1), false);
    auto up = filled((size_t)B * (na > 0 ? na : 1), false), comb = filled((size_t)B * 6, false), cartb = filled((size_t)B * 6, false);
    Bt.com_A = comA.get(); Bt.com_A_stride = 6 * ld; Bt.com_A_ld = ld;
    Bt.fb_A = fbA.get(); Bt.fb_A_stride = 6 * ld; Bt.fb_A_ld = ld;
    Bt.com_b = comb.get(); Bt.com_b_stride = 6;
    Bt.com_pos_ref = ref3.get(); Bt.com_vel_ref = ref3.get(); Bt.com_acc_ref = ref3.get(); Bt.ang_mom_ref = ref3.get(); Bt.ang_mom_rate_ref = ref3.get();
    if (na > 0) {
        Bt.static_A = stA.get(); Bt.static_A_stride = (long long)na * ld; Bt.static_A_ld = ld;
        Bt.static_lo = lo.get(); Bt.static_up = up.get(); Bt.static_b_stride = na; Bt.static_q_tau = qtau.get();
    }
    Bt.cart_b = cartb.get(); Bt.cart_b_stride = 6; Bt.cart_pose_ref = pose[0].get(); Bt.cart_vel_ref = ref6.get(); Bt.cart_f_des = ref6.get();
    if (force_host_rows(&M, &Bt) != OSOT_OK) return 1;
    // expectations: a column is written exactly when it belongs to a wrench (static rows: or to the torques); transposes are copies
    int bad = 0;
    for (int i = 0; i < B; ++i)
        for (int col = 0; col < ld; ++col) {
            int ct = -1, d = 0;
            for (int c = 0; c < C; ++c) if (col >= wrench_col[c] && col < wrench_col[c] + 6) { ct = c; d = col - wrench_col[c]; }
            const bool tq = torque_col >= 0 && col >= torque_col && col < torque_col + na;
            const bool on = ct >= 0 && en[i * C + ct];
            for (int r = 0; r < 6; ++r) {
                const double a = comA[((size_t)i * 6 + r) * ld + col], f = fbA[((size_t)i * 6 + r) * ld + col];
                if (ct < 0) { bad += (a != kSentinel) + (f != kSentinel); continue; }
                bad += (f != (on ? Jc[(((size_t)i * C + ct) * 6 + d) * nv + r] : 0.0));
                if (!on) bad += (a != 0.0);
                else if (r < 3 || d >= 3) bad += (a != ((d == r) ? 1.0 : 0.0));
            }
            for (int r = 0; r < na; ++r) {
                const double s = stA[((size_t)i * na + r) * ld + col];
                if (ct >= 0) bad += (s != (on ? Jc[(((size_t)i * C + ct) * 6 + d) * nv + 6 + r] : 0.0));
                else if (tq) bad += (s != ((col - torque_col == r) ? 1.0 : 0.0));
                else bad += (s != kSentinel);
            }
        }
    for (int i = 0; i < B * na; ++i) bad += (lo[i] != hg[(i / na) * nv + 6 + i % na] - qtau[i]) + (up[i] != lo[i]);
    for (int i = 0; i < B * 6; ++i) bad += !std::isfinite(comb[i]) + !std::isfinite(cartb[i]);
    printf("force_rows: B = %d C = %d nv = %d n = %d ld = %d: %d failed expectations\n", B, C, nv, n, ld, bad);
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    const int w1[1] = {0};
    bad += run_shape(3, 1, 7, w1, 6, 7, 0);                      // one static row
    const int w8[8] = {0, 6, 12, 18, 24, 30, 36, 42};
    bad += run_shape(2, 8, 64, w8, 48, 106, 0);                  // both column halves, the staging array full
    const int w3[3] = {40, 3, 21};
    bad += run_shape(65, 3, 35, w3, 47, 80, 5);                  // non-contiguous wrenches, ld > n
    if (bad) { printf("force_rows: FAILED\n"); return 1; }
    printf("force_rows: ok\n");
    return 0;
}
#endif
