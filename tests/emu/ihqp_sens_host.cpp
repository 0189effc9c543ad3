// tests/emu/ihqp_sens_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The level-QP kernel, the multiplier kernel, the objective kernel and the pull-back kernel of osot_ihqp_sensitivity (opensot_amd/csrc/osot_ihqp_sens.h,
// osot_qp_sens.h) through the host lock-step emulation of tests/emu/hip/hip_runtime.h, with the checks of osot_ihqp_level_qp and
// osot_ihqp_sensitivity.  A solver handle is a plan, a route, max_batch and the task switches here: the checks take exactly those.
// Built by tests/ihqp_sens_ref.py; used by tests/test_ihqp_sens_host.py (no GPU needed) and as the reference of
// tests/test_ihqp_sens_gpu.py.  libosot_mi355x.so launches the same kernel bodies from the same loop (ihqp_sens_levels).
// With -DOSOT_IHQP_SENS_MAIN it is a stand-alone program (for -fsanitize=address,undefined) over the smallest case of the tests:
// n = 7, two levels of 3 and 4 rows, one stored row block, a box, B = 8; every array of its exact size on the heap, sentinels around
// the outputs and the workspace; x_levels from a dense KKT solve of the two levels (no bound and no row of the block is active); the
// backward pass with every gradient output bound.
#include <osot_team.h>
#include "osot_ihqp_sens.h"

using namespace osot;

#define IHQP_API extern "C" __attribute__((visibility("default")))

namespace {
struct EmuLaunch {
    const osot_qp_sens_options* opt;
    void level_qp(const LevelQpArgs& Q) {
        if (Q.P.n <= 32) emu::launch(osot_ihqp_level_qp_kernel<32>, (unsigned)Q.D.B, (size_t)level_qp_lds_bytes(Q.P.n), 64, Q);
        else emu::launch(osot_ihqp_level_qp_kernel<64>, (unsigned)Q.D.B, (size_t)level_qp_lds_bytes(Q.P.n), 64, Q);
    }
    int sens(const osot_qp_sens_batch& b) {
        SensArgs S;
        S.b = b;
        sens_options(opt, &S.active_tol, &S.dual_tol, &S.rank_tol);
        if (b.n <= 32) emu::launch(osot_qp_sens_kernel<32>, (unsigned)b.B, (size_t)sens_lds_bytes(b.n), 64, S);
        else emu::launch(osot_qp_sens_kernel<64>, (unsigned)b.B, (size_t)sens_lds_bytes(b.n), 64, S);
        return OSOT_OK;
    }
    void objective(const ObjectiveArgs& O) { emu::launch(osot_ihqp_objective_kernel, (unsigned)O.B, (size_t)O.n * sizeof(double), 64, O); }
    void pullback(const PullbackArgs& R) { emu::launch(osot_ihqp_pullback_kernel, (unsigned)R.D.B, (size_t)pullback_lds_bytes(R.P.n), 64, R); }
    void zero(void* p, size_t bytes) { memset(p, 0, bytes); }
    void copy(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); }
};
const char* kNone = "";
}  // namespace

IHQP_API int ihqp_host_level_rows(const osot_plan_desc* plan, int level, int* rows) {
    if (!plan || !rows || level < 0 || level >= plan->n_levels) return OSOT_ERR_INVALID;
    LevelPlan P;
    make_plan_shape(*plan, nullptr, nullptr, P);
    *rows = level_qp_rows(P, level);
    return OSOT_OK;
}

IHQP_API int ihqp_host_workspace_bytes(const osot_plan_desc* plan, int B, int want_backward, int want_grad_A, unsigned long long* bytes) {
    if (!plan || !bytes || B < 0) return OSOT_ERR_INVALID;
    LevelPlan P;
    make_plan_shape(*plan, nullptr, nullptr, P);
    *bytes = (unsigned long long)ihqp_sens_workspace(P, B, want_backward != 0, want_grad_A != 0).total * sizeof(double);
    return OSOT_OK;
}

// osot_ihqp_level_qp: run = 0 answers the arguments alone
IHQP_API int ihqp_host_level_qp(const osot_plan_desc* plan, int wide, int max_batch, const unsigned char* task_active, const osot_qp_batch* b,
                                int level, const osot_level_qp* out, int run, const char** why) {
    *why = kNone;
    LevelQpArgs Q;
    const int rc = level_qp_check(*plan, wide, max_batch, task_active, b, level, out, Q, why);
    if (rc != OSOT_OK || !run || b->B == 0) return rc;
    EmuLaunch{nullptr}.level_qp(Q);
    return OSOT_OK;
}

// osot_ihqp_sensitivity: run = 0 answers the arguments alone
IHQP_API int ihqp_host_sensitivity(const osot_plan_desc* plan, int wide, int max_batch, const unsigned char* task_active,
                                   const osot_ihqp_sens_batch* b, const osot_qp_sens_options* opt, int run, const char** why) {
    *why = kNone;
    LevelQpArgs Q;
    const int rc = ihqp_sens_check(*plan, wide, max_batch, task_active, b, opt, Q, why);
    if (rc != OSOT_OK || !run || b->qp.B == 0) return rc;
    return ihqp_sens_levels(Q, b, EmuLaunch{opt});
}

#ifdef OSOT_IHQP_SENS_MAIN
#include <vector>

namespace {
const double kSentinel = -7.25e300;
const int kPad = 3;
unsigned long long g_seed = 0x9E3779B97F4A7C15ull;
double rnd() {   // xorshift64*, uniform in (-1, 1)
    g_seed ^= g_seed >> 12; g_seed ^= g_seed << 25; g_seed ^= g_seed >> 27;
    return (double)((g_seed * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}
struct Fenced {
    std::vector<double> v;
    size_t count;
    explicit Fenced(size_t c) : v(c + 2 * kPad, kSentinel), count(c) {}
    double* p() { return v.data() + kPad; }
    bool intact() const { for (int i = 0; i < kPad; ++i) if (v[i] != kSentinel || v[v.size() - 1 - i] != kSentinel) return false; return true; }
    int not_finite() const { int b = 0; for (size_t i = 0; i < count; ++i) b += !std::isfinite(v[kPad + i]) || v[kPad + i] == kSentinel; return b; }
};
// K z = rhs, Gaussian elimination with partial pivoting
std::vector<double> ge_solve(std::vector<double> K, std::vector<double> z, int m) {
    for (int c = 0; c < m; ++c) {
        int p = c;
        for (int r = c + 1; r < m; ++r) if (fabs(K[r * m + c]) > fabs(K[p * m + c])) p = r;
        for (int q = 0; q < m; ++q) std::swap(K[c * m + q], K[p * m + q]);
        std::swap(z[c], z[p]);
        for (int r = c + 1; r < m; ++r) {
            const double f = K[r * m + c] / K[c * m + c];
            for (int q = c; q < m; ++q) K[r * m + q] -= f * K[c * m + q];
            z[r] -= f * z[c];
        }
    }
    for (int c = m - 1; c >= 0; --c) {
        for (int q = c + 1; q < m; ++q) z[c] -= K[c * m + q] * z[q];
        z[c] /= K[c * m + c];
    }
    return z;
}
}  // namespace

int main() {
    const int B = 8, n = 7, L = 2, m[2] = {3, 4}, nc = 2;
    const double eps = 2.221e-7;
    osot_plan_desc plan;
    memset(&plan, 0, sizeof(plan));
    plan.n = n; plan.n_levels = L; plan.eps_abs = eps;
    for (int k = 0; k < L; ++k) {
        plan.level[k].n_tasks = 1;
        plan.level[k].task[0].kind = OSOT_TASK_GENERIC; plan.level[k].task[0].rows = m[k]; plan.level[k].task[0].weight = 1.0;
    }
    plan.n_bounds = 1; plan.bound[0].kind = OSOT_BOUND_GENERIC;
    plan.n_rowblocks = 1; plan.rowblock[0].kind = OSOT_ROWS_GENERIC; plan.rowblock[0].rows = nc;
    std::vector<double> A[2], b[2], w[2], C((size_t)B * nc * n), lo((size_t)B * nc, -10.0), up((size_t)B * nc, 10.0), l((size_t)B * n, -10.0),
        u((size_t)B * n, 10.0), dq((size_t)B * n), xl((size_t)B * L * n);
    std::vector<int> status(B, OSOT_STATUS_SOLVED);
    for (int k = 0; k < L; ++k) { A[k].resize((size_t)B * m[k] * n); b[k].resize((size_t)B * m[k]); w[k].resize((size_t)B * m[k]); }
    for (int i = 0; i < B; ++i) {
        for (int k = 0; k < L; ++k) {
            for (int e = 0; e < m[k] * n; ++e) A[k][(size_t)i * m[k] * n + e] = rnd();
            for (int r = 0; r < m[k]; ++r) { b[k][(size_t)i * m[k] + r] = 0.2 * rnd(); w[k][(size_t)i * m[k] + r] = 1.0 + 0.5 * rnd(); }
        }
        for (int e = 0; e < nc * n; ++e) C[(size_t)i * nc * n + e] = 0.1 * rnd();
        // level 0: (H + eps I) x = -g; level 1: the same under A_0 x = A_0 x_0
        std::vector<double> x0;
        for (int k = 0; k < L; ++k) {
            const int ne = k == 0 ? 0 : m[0], dim = n + ne;
            std::vector<double> K((size_t)dim * dim, 0.0), rhs(dim, 0.0);
            const double *Ak = &A[k][(size_t)i * m[k] * n], *bk = &b[k][(size_t)i * m[k]], *wk = &w[k][(size_t)i * m[k]];
            for (int r = 0; r < m[k]; ++r)
                for (int p = 0; p < n; ++p) {
                    rhs[p] += Ak[r * n + p] * wk[r] * bk[r];
                    for (int q = 0; q < n; ++q) K[p * dim + q] += Ak[r * n + p] * wk[r] * Ak[r * n + q];
                }
            for (int p = 0; p < n; ++p) K[p * dim + p] += eps;
            for (int r = 0; r < ne; ++r) {
                const double* a = &A[0][(size_t)i * m[0] * n + r * n];
                for (int p = 0; p < n; ++p) { K[p * dim + n + r] = a[p]; K[(n + r) * dim + p] = a[p]; rhs[n + r] += a[p] * x0[p]; }
            }
            const std::vector<double> z = ge_solve(K, rhs, dim);
            for (int p = 0; p < n; ++p) xl[((size_t)i * L + k) * n + p] = z[p];
            if (k == 0) x0.assign(z.begin(), z.begin() + n);
        }
        for (int p = 0; p < n; ++p) dq[(size_t)i * n + p] = xl[((size_t)i * L + L - 1) * n + p];
    }
    status[5] = OSOT_STATUS_MAX_ITER;        // one failed instance: skipped with zeros at both levels
    int rows[2];
    unsigned long long bytes = 0;
    for (int k = 0; k < L; ++k) if (ihqp_host_level_rows(&plan, k, &rows[k]) != OSOT_OK) return 1;
    if (ihqp_host_workspace_bytes(&plan, B, 1, 1, &bytes) != OSOT_OK || bytes % 8) return 1;
    Fenced ws(bytes / 8), y0((size_t)B * (n + rows[0])), y1((size_t)B * (n + rows[1])), obj((size_t)B * L);
    std::vector<int> act0((size_t)B * (n + rows[0]) + 2, -9), act1((size_t)B * (n + rows[1]) + 2, -9), flag0(B + 2, -9), flag1(B + 2, -9);
    osot_ihqp_sens_batch S;
    memset(&S, 0, sizeof(S));
    S.qp.B = B;
    for (int k = 0; k < L; ++k) { S.qp.A[k] = A[k].data(); S.qp.b[k] = b[k].data(); S.qp.w[k] = w[k].data(); }
    S.qp.C = C.data(); S.qp.lo = lo.data(); S.qp.up = up.data(); S.qp.l = l.data(); S.qp.u = u.data();
    S.qp.dq = dq.data(); S.qp.x_levels = xl.data(); S.qp.status = status.data();
    S.y[0] = y0.p(); S.y[1] = y1.p(); S.active[0] = act0.data() + 1; S.active[1] = act1.data() + 1;
    S.flag[0] = flag0.data() + 1; S.flag[1] = flag1.data() + 1; S.objective = obj.p();
    S.workspace = ws.p(); S.workspace_bytes = bytes;
    // the backward pass with every gradient output bound
    std::vector<double> gdq((size_t)B * n);
    for (double& v : gdq) v = rnd();
    Fenced gb0((size_t)B * m[0]), gb1((size_t)B * m[1]), gw0((size_t)B * m[0]), gw1((size_t)B * m[1]), gc0((size_t)B * n), gc1((size_t)B * n),
        gA0((size_t)B * m[0] * n), gA1((size_t)B * m[1] * n), gC((size_t)B * nc * n), glo((size_t)B * nc), gup((size_t)B * nc), gl((size_t)B * n),
        gu((size_t)B * n);
    S.grad_dq = gdq.data();
    S.grad_b[0] = gb0.p(); S.grad_b[1] = gb1.p(); S.grad_w[0] = gw0.p(); S.grad_w[1] = gw1.p(); S.grad_c[0] = gc0.p(); S.grad_c[1] = gc1.p();
    S.grad_A[0] = gA0.p(); S.grad_A[1] = gA1.p(); S.grad_C = gC.p(); S.grad_lo = glo.p(); S.grad_up = gup.p(); S.grad_l = gl.p(); S.grad_u = gu.p();
    Fenced* grads[13] = {&gb0, &gb1, &gw0, &gw1, &gc0, &gc1, &gA0, &gA1, &gC, &glo, &gup, &gl, &gu};
    const char* why = "";
    const int rc = ihqp_host_sensitivity(&plan, 0, B, nullptr, &S, nullptr, 1, &why);
    if (rc != OSOT_OK) { printf("ihqp_sens: refused: %s\n", why); return 1; }
    int bad = 0;
    bad += !ws.intact() + !y0.intact() + !y1.intact() + !obj.intact();
    bad += y0.not_finite() + y1.not_finite() + obj.not_finite();
    for (Fenced* f : grads) bad += !f->intact() + f->not_finite();
    double gsum = 0.0;
    for (size_t e = 0; e < gc1.count; ++e) gsum += fabs(gc1.p()[e]);
    bad += !(gsum > 0.0);                    // (grad_c of the last level is dx: not all zero)
    bad += act0.front() != -9 || act0.back() != -9 || act1.front() != -9 || act1.back() != -9;
    bad += flag0.front() != -9 || flag0.back() != -9 || flag1.front() != -9 || flag1.back() != -9;
    for (int i = 0; i < B; ++i) {
        const int want = i == 5 ? OSOT_SENS_SKIPPED : OSOT_SENS_OK;
        if (flag0[1 + i] != want || flag1[1 + i] != want) { printf("  instance %d: flags %d %d, expected %d\n", i, flag0[1 + i], flag1[1 + i], want); ++bad; }
        int n_active = 0;
        for (int e = 0; e < n + rows[1]; ++e) n_active += act1[1 + (size_t)i * (n + rows[1]) + e] != 0;
        if (n_active != (i == 5 ? 0 : m[0])) { printf("  instance %d: %d active at level 1, expected the %d optimality rows\n", i, n_active, m[0]); ++bad; }
        for (int k = 0; k < L; ++k) {      // the objective against a plain evaluation of 1/2 |A x - b|^2_W - 1/2 b'Wb + eps/2 |x|^2
            double f = 0.0;
            const double* x = &xl[((size_t)i * L + k) * n];
            for (int r = 0; r < m[k]; ++r) {
                double ax = 0.0;
                for (int p = 0; p < n; ++p) ax += A[k][(size_t)i * m[k] * n + r * n + p] * x[p];
                const double bb = b[k][(size_t)i * m[k] + r], ww = w[k][(size_t)i * m[k] + r];
                f += 0.5 * ww * (ax - bb) * (ax - bb) - 0.5 * ww * bb * bb;
            }
            for (int p = 0; p < n; ++p) f += 0.5 * eps * x[p] * x[p];
            const double got = obj.p()[(size_t)i * L + k];
            if (i == 5 ? got != 0.0 : fabs(got - f) > 1e-12 * (1.0 + fabs(f))) { printf("  instance %d level %d: objective %.17g, expected %.17g\n", i, k, got, f); ++bad; }
        }
    }
    printf("ihqp_sens: B = %d n = %d levels (%d, %d) nc = %d: %d failed expectations\n", B, n, m[0], m[1], nc, bad);
    if (bad) { printf("ihqp_sens: FAILED\n"); return 1; }
    printf("ihqp_sens: ok\n");
    return 0;
}
#endif
