// tests/emu/ihqp_sens_wide_host.cpp -- TEST INFRASTRUCTURE ONLY.
// osot_ihqp_level_qp and osot_ihqp_sensitivity on a handle of osot_solver_create_wide (65 .. 128 variables) compiled for the host: the
// level-QP, objective and pull-back functions of opensot_amd/csrc/osot_ihqp_sens_wide.h and sensbig::run of osot_qp_sens_big.h, from
// the schedule the product runs (ihqp_sens_levels), with the checks of the two entries (level_qp_check, ihqp_sens_check).  A solver
// handle is a plan, a route, max_batch and the task switches here: the checks take exactly those.  Built by
// tests/ihqp_sens_wide_ref.py; used by tests/test_ihqp_sens_wide_host.py (no GPU needed) and as the emulation of
// tests/test_ihqp_sens_wide_gpu.py.  libosot_mi355x.so runs the same source as 256-thread workgroups.
//
// Two teams, as in qp_sens_big_host.cpp: a team of one thread (every parallel section a plain loop), and a team of nthreads POSIX
// threads whose sections run one thread at a time in a FIXED order (a barrier passes the turn to the next thread of the order).
// Order 0 lets thread 0 finish each section before the others start, order 1 lets it start last: a value that one thread writes in
// a section where the others still read it -- a missing barrier -- comes out differently under the two orders, and the results
// differ from the team of one.  Every launch works on an LDS block of exactly its size, and the multiplier launches on the slices of
// the caller's workspace, as on the device.
//
// With -DOSOT_IHQP_SENS_WIDE_MAIN it is a stand-alone program (for -fsanitize=address,undefined) over the shape of the tests' case p:
// n = 65, two levels of 3 and 4 rows, one stored row block of 2, a box, B = 4; every array of its exact size on the heap, sentinels
// around the outputs and the workspace; x_levels from a dense KKT solve of the two levels (no bound and no row of the block is
// active); the backward pass with every gradient output bound, as a team of one and as a team of 7.
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <osot_team.h>
#include "osot_ihqp_sens_wide.h"

using namespace osot;

#define IHQP_API extern "C" __attribute__((visibility("default")))

namespace {
struct TeamOne {
    int tid = 0, nt = 1;
    static constexpr int kOwners = ihqpwide::kOwners;
    void sync() const {}
};
struct Turns {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> order;   // thread ids in the order they run each section
    int pos = 0;              // whose turn: order[pos]
    void wait_turn(int tid) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return order[pos] == tid; }); }
    void pass() { { std::lock_guard<std::mutex> lk(mu); pos = (pos + 1) % (int)order.size(); } cv.notify_all(); }
};
struct TeamTurns {
    int tid, nt;
    Turns* T;
    static constexpr int kOwners = ihqpwide::kOwners;
    void sync() const { T->pass(); T->wait_turn(tid); }
};

// one workgroup: body(team member) by a team of one, or by nthreads threads taking turns
template <class Body>
void workgroup(int nthreads, int t0_last, Body&& body) {
    if (nthreads == 1) { body(TeamOne{}); return; }
    Turns T;
    for (int i = 0; i < nthreads; ++i) T.order.push_back(t0_last ? (i + 1) % nthreads : i);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t] {
            const TeamTurns tm{t, nthreads, &T};
            T.wait_turn(t);
            body(tm);
            T.pass();                 // (every member leaves after the same final barrier)
        });
    for (auto& t : th) t.join();
}

struct HostLaunch {
    const osot_qp_sens_options* opt;
    double* slices;          // the Y slices: the workspace behind ihqp_wide_front_bytes
    int grid, nthreads, t0_last;
    void level_qp(const LevelQpArgs& Q) {
        for (long long inst = 0; inst < Q.D.B; ++inst) {
            std::unique_ptr<char[]> lds(new char[ihqpwide::level_lds_bytes(Q.P.n)]);
            workgroup(nthreads, t0_last, [&](const auto& tm) { ihqpwide::level_qp(tm, Q, inst, lds.get()); });
        }
    }
    int sens(const osot_qp_sens_batch& b) {
        SensArgs S;
        S.b = b;
        sens_options(opt, &S.active_tol, &S.dual_tol, &S.rank_tol);
        for (int w = 0; w < grid; ++w) {      // workgroup w walks the batch with stride grid on slice w
            std::unique_ptr<char[]> lds(new char[sensbig::lds_bytes(b.n, b.nc)]);
            double* slice = slices + (size_t)w * (sensbig::slice_bytes(b.n) / sizeof(double));
            workgroup(nthreads, t0_last, [&](const auto& tm) {
                for (long long inst = w; inst < b.B; inst += grid) sensbig::run(tm, S, inst, lds.get(), slice);
            });
        }
        return OSOT_OK;
    }
    void objective(const ObjectiveArgs& O) {
        for (long long inst = 0; inst < O.B; ++inst) {
            std::unique_ptr<char[]> lds(new char[ihqpwide::objective_lds_bytes(O.n)]);
            workgroup(nthreads, t0_last, [&](const auto& tm) { ihqpwide::objective(tm, O, inst, lds.get()); });
        }
    }
    void pullback(const PullbackArgs& R) {
        for (long long inst = 0; inst < R.D.B; ++inst) {
            std::unique_ptr<char[]> lds(new char[ihqpwide::pullback_lds_bytes(R.P.n)]);
            workgroup(nthreads, t0_last, [&](const auto& tm) { ihqpwide::pullback(tm, R, inst, lds.get()); });
        }
    }
    void zero(void* p, size_t bytes) { memset(p, 0, bytes); }
    void copy(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); }
};
const char* kNone = "";
}  // namespace

IHQP_API int ihqp_wide_host_level_lds_bytes(int n) { return ihqpwide::level_lds_bytes(n); }
IHQP_API int ihqp_wide_host_pullback_lds_bytes(int n) { return ihqpwide::pullback_lds_bytes(n); }

// osot_ihqp_sens_workspace_bytes on a wide handle, and the part in front of the Y slices
IHQP_API int ihqp_wide_host_workspace_bytes(const osot_plan_desc* plan, int B, int want_backward, int want_grad_A, unsigned long long* bytes,
                                            unsigned long long* front) {
    if (!plan || !bytes || B < 0) return OSOT_ERR_INVALID;
    LevelPlan P;
    make_plan_shape(*plan, nullptr, nullptr, P);
    *bytes = ihqp_wide_workspace_bytes(P, B, want_backward != 0, want_grad_A != 0);
    if (front) *front = ihqp_wide_front_bytes(P, B, want_backward != 0, want_grad_A != 0);
    return OSOT_OK;
}

// osot_ihqp_level_qp: run = 0 answers the arguments alone
IHQP_API int ihqp_wide_host_level_qp(const osot_plan_desc* plan, int wide, int max_batch, const unsigned char* task_active, const osot_qp_batch* b,
                                     int level, const osot_level_qp* out, int run, int nthreads, int t0_last, const char** why) {
    *why = kNone;
    if (nthreads < 1 || nthreads > 64) return OSOT_ERR_INVALID;
    LevelQpArgs Q;
    const int rc = level_qp_check(*plan, wide, max_batch, task_active, b, level, out, Q, why);
    if (rc != OSOT_OK || !run || b->B == 0) return rc;
    if (!ihqpwide::serves(*plan, wide)) { *why = "not a plan of the wide kernels"; return OSOT_ERR_UNSUPPORTED; }
    HostLaunch{nullptr, nullptr, 0, nthreads, t0_last}.level_qp(Q);
    return OSOT_OK;
}

// osot_ihqp_sensitivity: run = 0 answers the arguments alone
IHQP_API int ihqp_wide_host_sensitivity(const osot_plan_desc* plan, int wide, int max_batch, const unsigned char* task_active,
                                        const osot_ihqp_sens_batch* b, const osot_qp_sens_options* opt, int run, int nthreads, int t0_last,
                                        const char** why) {
    *why = kNone;
    if (nthreads < 1 || nthreads > 64) return OSOT_ERR_INVALID;
    LevelQpArgs Q;
    const int rc = ihqp_sens_check(*plan, wide, max_batch, task_active, b, opt, Q, why);
    if (rc != OSOT_OK || !run || b->qp.B == 0) return rc;
    if (!ihqpwide::serves(*plan, wide)) { *why = "not a plan of the wide kernels"; return OSOT_ERR_UNSUPPORTED; }
    char* slices = static_cast<char*>(b->workspace) + ihqp_wide_front_bytes(Q.P, b->qp.B, b->grad_dq != nullptr, ihqp_wants_grad_A(*b, Q.P.L));
    return ihqp_sens_levels(Q, b, HostLaunch{opt, reinterpret_cast<double*>(slices), ihqp_wide_sens_grid(Q.P, b->qp.B), nthreads, t0_last});
}

#ifdef OSOT_IHQP_SENS_WIDE_MAIN
namespace {
const double kSentinel = -7.25e300;
const int kPad = 4;          // (an even count: the fenced workspace keeps the alignment of its block)
unsigned long long g_seed = 0x9E3779B97F4A7C15ull;
double rnd() {   // xorshift64*, uniform in (-1, 1)
    g_seed ^= g_seed >> 12; g_seed ^= g_seed << 25; g_seed ^= g_seed >> 27;
    return (double)((g_seed * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}
struct Fenced {
    std::unique_ptr<double[]> v;      // (operator new[]: 16-byte aligned)
    size_t count;
    explicit Fenced(size_t c) : v(new double[c + 2 * kPad]), count(c) { for (size_t i = 0; i < c + 2 * kPad; ++i) v[i] = kSentinel; }
    double* p() { return v.get() + kPad; }
    void clear() { for (size_t i = 0; i < count + 2 * kPad; ++i) v[i] = kSentinel; }
    bool intact() const { for (int i = 0; i < kPad; ++i) if (v[i] != kSentinel || v[count + 2 * kPad - 1 - i] != kSentinel) return false; return true; }
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
    const int B = 4, n = 65, L = 2, m[2] = {3, 4}, nc = 2, rows[2] = {nc, nc + m[0]};
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
    status[2] = OSOT_STATUS_MAX_ITER;        // one failed instance: skipped with zeros at both levels
    unsigned long long bytes = 0, front = 0;
    if (ihqp_wide_host_workspace_bytes(&plan, B, 1, 1, &bytes, &front) != OSOT_OK || bytes % 16 || front % 16 || front >= bytes) return 1;
    Fenced ws(bytes / 8), y0((size_t)B * (n + rows[0])), y1((size_t)B * (n + rows[1])), obj((size_t)B * L);
    if (reinterpret_cast<uintptr_t>(ws.p()) % 16) { printf("ihqp_sens_wide: the workspace block is not 16-byte aligned\n"); return 1; }
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
    std::vector<double> gdq((size_t)B * n);
    for (double& v : gdq) v = rnd();
    Fenced gb0((size_t)B * m[0]), gb1((size_t)B * m[1]), gw0((size_t)B * m[0]), gw1((size_t)B * m[1]), gc0((size_t)B * n), gc1((size_t)B * n),
        gA0((size_t)B * m[0] * n), gA1((size_t)B * m[1] * n), gC((size_t)B * nc * n), glo((size_t)B * nc), gup((size_t)B * nc), gl((size_t)B * n),
        gu((size_t)B * n);
    S.grad_dq = gdq.data();
    S.grad_b[0] = gb0.p(); S.grad_b[1] = gb1.p(); S.grad_w[0] = gw0.p(); S.grad_w[1] = gw1.p(); S.grad_c[0] = gc0.p(); S.grad_c[1] = gc1.p();
    S.grad_A[0] = gA0.p(); S.grad_A[1] = gA1.p(); S.grad_C = gC.p(); S.grad_lo = glo.p(); S.grad_up = gup.p(); S.grad_l = gl.p(); S.grad_u = gu.p();
    Fenced* grads[13] = {&gb0, &gb1, &gw0, &gw1, &gc0, &gc1, &gA0, &gA1, &gC, &glo, &gup, &gl, &gu};
    int bad = 0;
    std::vector<double> first;               // grad_A of level 0 of the team of one
    for (int nthreads : {1, 7}) {
        ws.clear(); y0.clear(); y1.clear(); obj.clear();
        for (Fenced* f : grads) f->clear();
        const char* why = "";
        const int rc = ihqp_wide_host_sensitivity(&plan, 1, B, nullptr, &S, nullptr, 1, nthreads, 0, &why);
        if (rc != OSOT_OK) { printf("ihqp_sens_wide: refused: %s\n", why); return 1; }
        bad += !ws.intact() + !y0.intact() + !y1.intact() + !obj.intact();
        bad += y0.not_finite() + y1.not_finite() + obj.not_finite();
        for (Fenced* f : grads) bad += !f->intact() + f->not_finite();
        double gsum = 0.0;
        for (size_t e = 0; e < gc1.count; ++e) gsum += fabs(gc1.p()[e]);
        bad += !(gsum > 0.0);                // (grad_c of the last level is dx: not all zero)
        if (nthreads == 1) first.assign(gA0.p(), gA0.p() + gA0.count);
        else bad += memcmp(first.data(), gA0.p(), gA0.count * sizeof(double)) != 0;      // the bits do not depend on the team
        bad += act0.front() != -9 || act0.back() != -9 || act1.front() != -9 || act1.back() != -9;
        bad += flag0.front() != -9 || flag0.back() != -9 || flag1.front() != -9 || flag1.back() != -9;
        for (int i = 0; i < B; ++i) {
            const int want = i == 2 ? OSOT_SENS_SKIPPED : OSOT_SENS_OK;
            if (flag0[1 + i] != want || flag1[1 + i] != want) { printf("  instance %d: flags %d %d, expected %d\n", i, flag0[1 + i], flag1[1 + i], want); ++bad; }
            int n_active = 0;
            for (int e = 0; e < n + rows[1]; ++e) n_active += act1[1 + (size_t)i * (n + rows[1]) + e] != 0;
            if (n_active != (i == 2 ? 0 : m[0])) { printf("  instance %d: %d active at level 1, expected the %d optimality rows\n", i, n_active, m[0]); ++bad; }
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
                if (i == 2 ? got != 0.0 : fabs(got - f) > 1e-12 * (1.0 + fabs(f))) { printf("  instance %d level %d: objective %.17g, expected %.17g\n", i, k, got, f); ++bad; }
            }
        }
        printf("ihqp_sens_wide: team of %d: B = %d n = %d levels (%d, %d) nc = %d: %d failed expectations so far\n", nthreads, B, n, m[0], m[1], nc, bad);
    }
    if (bad) { printf("ihqp_sens_wide: FAILED\n"); return 1; }
    printf("ihqp_sens_wide: ok\n");
    return 0;
}
#endif
