// tests/emu/qp_sens_big_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The multiplier / sensitivity route for 65 .. 128 variables (opensot_amd/csrc/osot_qp_sens_big.h, sensbig::run) compiled for the
// host, with the checks of osot_qp_sensitivity_batch_ws (sens_ws_check).  Built by tests/qp_sens_big_ref.py; used by
// tests/test_qp_sens_big_host.py (no GPU needed) and as the emulation of tests/test_qp_sens_big_gpu.py.  libosot_mi355x.so runs
// the same source as a 256-thread workgroup (osot_qp_sens_big_kernel).  A batch of n <= 64 goes to osot_qp_sens_kernel through
// the lock-step emulation, as the product's entry sends it there.
//
// Two teams, as in big_hot_host.cpp: a team of one thread (every parallel section a plain loop), and a team of nthreads POSIX
// threads whose sections run one thread at a time in a FIXED order (a barrier passes the turn to the next thread of the order).
// Order 0 lets thread 0 finish each section before the others start, order 1 lets it start last: a value that one thread writes
// in a section where the others still read it -- a missing barrier -- comes out differently under the two orders, and the results
// differ from the team of one.
//
// With -DOSOT_QP_SENS_BIG_MAIN it is a stand-alone program (for -fsanitize=address,undefined): QPs whose solution and multipliers
// are known by construction (x and y are drawn, g = -H~x + y_b + A'y_c), every array of its exact size on the heap with sentinels
// around the outputs, over the edges of tests/test_qp_sens_big_host.py.
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <osot_team.h>
#include "osot_qp_sens_big.h"

using namespace osot;

#define SENS_API extern "C" __attribute__((visibility("default")))

namespace {
struct TeamOne { int tid = 0, nt = 1; void sync() const {} };

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
    void sync() const { T->pass(); T->wait_turn(tid); }
};

// one workgroup: the instances first, first + stride, ... on one LDS block and one slice, both of their exact sizes
void workgroup(const SensArgs& S, int first, int stride, int nthreads, int t0_last) {
    const int n = S.b.n, nc = S.b.nc;
    std::unique_ptr<char[]> lds(new char[sensbig::lds_bytes(n, nc)]);
    std::unique_ptr<double[]> slice(new double[sensbig::slice_bytes(n) / sizeof(double)]);
    if (nthreads == 1) {
        for (long long inst = first; inst < S.b.B; inst += stride) sensbig::run(TeamOne{}, S, inst, lds.get(), slice.get());
        return;
    }
    Turns T;
    for (int i = 0; i < nthreads; ++i) T.order.push_back(t0_last ? (i + 1) % nthreads : i);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t] {
            const TeamTurns tm{t, nthreads, &T};
            T.wait_turn(t);
            for (long long inst = first; inst < S.b.B; inst += stride) sensbig::run(tm, S, inst, lds.get(), slice.get());
            T.pass();                 // (every member leaves after the same final barrier)
        });
    for (auto& t : th) t.join();
}
}  // namespace

// osot_qp_sensitivity_batch_ws's answer to its arguments alone -> code, *why = the reason
SENS_API int sens_big_host_check(const osot_qp_sens_batch* b, const osot_qp_sens_options* o, const void* workspace, size_t workspace_bytes,
                                 const char** why) {
    static const char* none = "";
    *why = none;
    return sens_ws_check(b, o, workspace, workspace_bytes, why);
}

// osot_qp_sens_workspace_bytes
SENS_API int sens_big_host_workspace_bytes(int B, int n, int nc, size_t* bytes, const char** why) {
    static const char* none = "";
    *why = none;
    const int rc = sens_ws_bytes_check(B, n, nc, bytes, why);
    if (rc == OSOT_OK) *bytes = sensbig::workspace_bytes(B, n, nc);
    return rc;
}

SENS_API size_t sens_big_host_lds_bytes(int n, int nc) { return sensbig::lds_bytes(n, nc); }
SENS_API int sens_big_host_slots(int n, int nc) { return sensbig::slots(n, nc); }
SENS_API size_t sens_big_host_slice_bytes(int n) { return sensbig::slice_bytes(n); }

// the batch through the route the product's entry takes.  groups: the number of workgroups that walk the batch (the product's
// min(B, slots)); nthreads = 1: the team of one, > 1: the turn-taking team with thread 0 first (t0_last = 0) or last (1)
SENS_API int sens_big_host_run(const osot_qp_sens_batch* b, const osot_qp_sens_options* o, int groups, int nthreads, int t0_last) {
    if (groups < 1 || nthreads < 1 || nthreads > 64) return OSOT_ERR_INVALID;
    const char* why = "";
    // a workspace of the size the entry asks for goes through the check; the host's workgroups then work on slices of their own,
    // each a heap block of exactly its size
    const size_t wbytes = b && b->n >= 1 && b->n <= sensbig::kMaxVars && b->nc >= 0 ? sensbig::workspace_bytes(b->B, b->n, b->nc) : 0;
    std::vector<max_align_t> workspace(wbytes / sizeof(max_align_t) + 1);
    const int rc = sens_ws_check(b, o, workspace.data(), wbytes, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "qp_sens_big host: %s\n", why); return rc; }
    if (b->B == 0) return OSOT_OK;
    SensArgs S;
    S.b = *b;
    sens_options(o, &S.active_tol, &S.dual_tol, &S.rank_tol);
    if (b->n <= 32) emu::launch(osot_qp_sens_kernel<32>, (unsigned)b->B, (size_t)sens_lds_bytes(b->n), 64, S);
    else if (b->n <= OSOT_MAX_VARS) emu::launch(osot_qp_sens_kernel<64>, (unsigned)b->B, (size_t)sens_lds_bytes(b->n), 64, S);
    else {
        const int G = b->B < groups ? b->B : groups;
        for (int w = 0; w < G; ++w) workgroup(S, w, G, nthreads, t0_last);
    }
    return OSOT_OK;
}

#ifdef OSOT_QP_SENS_BIG_MAIN
#include <functional>

namespace {
const double kSentinel = -7.25e300;
const int kPad = 3;
unsigned long long g_seed = 0x9E3779B97F4A7C15ull;
double rnd() {   // xorshift64*, uniform in (-1, 1)
    g_seed ^= g_seed >> 12; g_seed ^= g_seed << 25; g_seed ^= g_seed >> 27;
    return (double)((g_seed * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

// one instance under construction: sides (0, -1, +1, 2) of the bounds and rows, then the arrays
struct Inst {
    int n, nc;
    std::vector<double> H, A, x, l, u, lA, uA, yb, yc, g;
    std::vector<int> bside, rside;
};

// exact-size heap arrays; outputs carry kPad sentinels on both sides
struct Fenced {
    std::vector<double> v;
    size_t count;
    explicit Fenced(size_t c) : v(c + 2 * kPad, kSentinel), count(c) {}
    double* p() { return v.data() + kPad; }
    bool intact() const { for (int i = 0; i < kPad; ++i) if (v[i] != kSentinel || v[v.size() - 1 - i] != kSentinel) return false; return true; }
    int not_finite() const { int b = 0; for (size_t i = 0; i < count; ++i) b += !std::isfinite(v[kPad + i]) || v[kPad + i] == kSentinel; return b; }
};

struct Expect { int flag; bool check_y; };

// B instances of (n, nc); shape(inst, i) marks the active sides and may edit the arrays after they are drawn (post)
int run_case(const char* name, int B, int n, int nc, bool box, const std::function<void(Inst&, int)>& shape,
             const std::function<void(Inst&, int)>& post, const std::function<Expect(int)>& expect, int fail_instance = -1) {
    const double eps = 4.442e-11;
    std::vector<double> H((size_t)B * n * n), g((size_t)B * n), A((size_t)B * nc * n), lA((size_t)B * nc), uA((size_t)B * nc), l((size_t)B * n),
        u((size_t)B * n), x((size_t)B * n), gx((size_t)B * n), yref((size_t)B * (n + nc));
    std::vector<int> status(B, 0);
    for (int i = 0; i < B; ++i) {
        Inst q;
        q.n = n; q.nc = nc;
        q.H.assign((size_t)n * n, 0.0); q.A.resize((size_t)nc * n); q.x.resize(n); q.l.resize(n); q.u.resize(n); q.lA.resize(nc); q.uA.resize(nc);
        q.yb.assign(n, 0.0); q.yc.assign(nc, 0.0); q.g.resize(n); q.bside.assign(n, 0); q.rside.assign(nc, 0);
        std::vector<double> M((size_t)(n + 3) * n);
        for (double& v : M) v = rnd();
        for (int r = 0; r < n; ++r)
            for (int c = 0; c <= r; ++c) { double s = 0.0; for (int k = 0; k < n + 3; ++k) s += M[k * n + r] * M[k * n + c]; q.H[r * n + c] = q.H[c * n + r] = s; }
        for (double& v : q.A) v = rnd();
        for (double& v : q.x) v = 0.3 * rnd();
        shape(q, i);
        for (int k = 0; k < n; ++k) {
            const int s = q.bside[k];
            q.l[k] = q.x[k] - (s == -1 || s == 2 ? 0.0 : 0.5); q.u[k] = q.x[k] + (s == 1 || s == 2 ? 0.0 : 0.5);
            q.yb[k] = s == 0 ? 0.0 : (s == 1 ? -1.0 : 1.0) * (0.5 + fabs(rnd()));
        }
        for (int r = 0; r < nc; ++r) {
            double ax = 0.0;
            for (int k = 0; k < n; ++k) ax = fma(q.A[r * n + k], q.x[k], ax);      // (the kernel's own chain: an active row sits on its bound)
            const int s = q.rside[r];
            q.lA[r] = s == -1 || s == 2 ? ax : ax - 0.5; q.uA[r] = s == 1 || s == 2 ? ax : ax + 0.5;
            if (s == 2) q.uA[r] = q.lA[r];
            q.yc[r] = s == 0 ? 0.0 : (s == 1 ? -1.0 : 1.0) * (0.5 + fabs(rnd()));
        }
        post(q, i);
        for (int k = 0; k < n; ++k) {      // g = -H~x + y_b + A'y_c
            double s = -eps * q.x[k];
            for (int c = 0; c < n; ++c) s -= q.H[k * n + c] * q.x[c];
            s += q.yb[k];
            for (int r = 0; r < nc; ++r) s += q.A[r * n + k] * q.yc[r];
            q.g[k] = s;
        }
        std::copy(q.H.begin(), q.H.end(), H.begin() + (size_t)i * n * n);
        std::copy(q.A.begin(), q.A.end(), A.begin() + (size_t)i * nc * n);
        std::copy(q.g.begin(), q.g.end(), g.begin() + (size_t)i * n);
        std::copy(q.x.begin(), q.x.end(), x.begin() + (size_t)i * n);
        std::copy(q.l.begin(), q.l.end(), l.begin() + (size_t)i * n);
        std::copy(q.u.begin(), q.u.end(), u.begin() + (size_t)i * n);
        std::copy(q.lA.begin(), q.lA.end(), lA.begin() + (size_t)i * nc);
        std::copy(q.uA.begin(), q.uA.end(), uA.begin() + (size_t)i * nc);
        std::copy(q.yb.begin(), q.yb.end(), yref.begin() + (size_t)i * (n + nc));
        std::copy(q.yc.begin(), q.yc.end(), yref.begin() + (size_t)i * (n + nc) + n);
        for (int k = 0; k < n; ++k) gx[(size_t)i * n + k] = rnd();
    }
    if (fail_instance >= 0) {
        status[fail_instance] = OSOT_STATUS_MAX_ITER;
        for (int k = 0; k < n; ++k) x[(size_t)fail_instance * n + k] = NAN;
    }
    Fenced y((size_t)B * (n + nc)), gH((size_t)B * n * n), gg((size_t)B * n), gA((size_t)B * nc * n), glA((size_t)B * nc), guA((size_t)B * nc),
        gl((size_t)B * n), gu((size_t)B * n);
    std::vector<int> active((size_t)B * (n + nc) + 2, -9), flag(B + 2, -9);
    osot_qp_sens_batch b;
    memset(&b, 0, sizeof(b));
    b.B = B; b.n = n; b.nc = nc; b.H = H.data(); b.g = g.data(); b.eps_abs = eps; b.x = x.data(); b.status = status.data(); b.grad_x = gx.data();
    if (nc) { b.A = A.data(); b.lA = lA.data(); b.uA = uA.data(); b.grad_A = gA.p(); b.grad_lA = glA.p(); b.grad_uA = guA.p(); }
    if (box) { b.l = l.data(); b.u = u.data(); b.grad_l = gl.p(); b.grad_u = gu.p(); }
    b.y = y.p(); b.active = active.data() + 1; b.grad_H = gH.p(); b.grad_g = gg.p(); b.flag = flag.data() + 1;
    if (sens_big_host_run(&b, nullptr, 2, 1, 0) != OSOT_OK) return 1;      // two workgroups: with B = 3 the first one walks two instances
    int bad = 0;
    Fenced* outs[8] = {&y, &gH, &gg, &gA, &glA, &guA, &gl, &gu};
    for (Fenced* f : outs) {
        const bool bound = (f == &y || f == &gH || f == &gg) || ((f == &gA || f == &glA || f == &guA) && nc) || ((f == &gl || f == &gu) && box);
        bad += !f->intact();
        if (bound) bad += f->not_finite();
        else for (double v : f->v) bad += v != kSentinel;
    }
    bad += active.front() != -9 || active.back() != -9 || flag.front() != -9 || flag.back() != -9;
    for (int i = 0; i < B; ++i) {
        const Expect e = expect(i);
        if (flag[1 + i] != e.flag) { printf("  %s: instance %d has flag %d, expected %d\n", name, i, flag[1 + i], e.flag); ++bad; }
        for (int k = 0; k < n + nc; ++k) {
            const double got = y.p()[(size_t)i * (n + nc) + k];
            if (e.flag == OSOT_SENS_SKIPPED) bad += got != 0.0 || active[1 + (size_t)i * (n + nc) + k] != 0;
            else if (e.check_y && fabs(got - yref[(size_t)i * (n + nc) + k]) > 1e-6) { printf("  %s: instance %d y[%d] = %.17g, expected %.17g\n", name, i, k, got, yref[(size_t)i * (n + nc) + k]); ++bad; }
        }
    }
    printf("qp_sens_big: %-22s B = %d n = %d nc = %d: %d failed expectations\n", name, B, n, nc, bad);
    return bad;
}

const std::function<void(Inst&, int)> kNothing = [](Inst&, int) {};
const std::function<Expect(int)> kAllOk = [](int) { return Expect{OSOT_SENS_OK, true}; };
const std::function<Expect(int)> kAllDegenerate = [](int) { return Expect{OSOT_SENS_DEGENERATE, false}; };
}  // namespace

int main() {
    int bad = 0;
    const auto mixed = [](Inst& q, int i) {     // a few lower and upper bounds, rows of every kind
        for (int k = 0; k < q.n; k += 3) q.bside[k] = (k + i) % 2 ? 1 : -1;
        for (int r = 0; r < q.nc && r < q.n / 2; r += 2) q.rside[r] = r % 4 ? 1 : (r % 3 ? -1 : 2);
    };
    bad += run_case("no_candidate", 3, 65, 5, true, kNothing, kNothing, kAllOk);
    bad += run_case("all_bounds", 3, 65, 4, true, [](Inst& q, int i) { for (int k = 0; k < q.n; ++k) q.bside[k] = (k + i) % 2 ? 1 : -1; }, kNothing, kAllOk);
    bad += run_case("no_A_no_box", 3, 66, 0, false, kNothing, kNothing, kAllOk);
    bad += run_case("rows_past_256", 3, 65, 300, true, [](Inst& q, int i) { q.rside[3] = 1; q.rside[255] = -1; q.rside[256 + i] = 1; q.rside[299] = 2; q.bside[64] = -1; },
                    kNothing, kAllOk);
    bad += run_case("full_capacity", 2, 128, 128, true, [](Inst& q, int i) { for (int k = 0; k < 128; ++k) { q.bside[k] = (k + i) % 2 ? 1 : -1; q.rside[k] = k % 2 ? 1 : -1; } },
                    kNothing, kAllDegenerate);
    bad += run_case("2n_plus_some", 3, 65, 70, true, [](Inst& q, int) { for (int k = 0; k < q.n; ++k) q.bside[k] = -1; for (int r = 0; r < 68; ++r) q.rside[r] = 1; },
                    kNothing, kAllDegenerate);
    bad += run_case("one_sided_row", 3, 65, 9, true, [](Inst& q, int) { q.rside[8] = 1; q.rside[2] = -1; },
                    [](Inst& q, int) { q.lA[8] = -INFINITY; q.uA[2] = INFINITY; }, kAllOk);
    bad += run_case("l_equals_u", 3, 65, 3, true, [](Inst& q, int i) { q.bside[i] = 2; q.bside[64] = 2; q.rside[1] = 2; }, kNothing, kAllOk);
    bad += run_case("failed_instance", 3, 65, 9, true, mixed, kNothing,
                    [](int i) { return Expect{i == 1 ? OSOT_SENS_SKIPPED : OSOT_SENS_OK, true}; }, 1);
    bad += run_case("row_repeats_bound", 3, 65, 4, true, [](Inst& q, int) { q.bside[2] = -1; q.rside[1] = -1; },
                    [](Inst& q, int) { for (int k = 0; k < q.n; ++k) q.A[1 * q.n + k] = k == 2 ? 1.0 : 0.0; q.lA[1] = q.x[2]; q.uA[1] = q.x[2] + 0.5; },
                    kAllDegenerate);
    bad += run_case("n100", 2, 100, 40, true, mixed, kNothing, kAllOk);
    bad += run_case("n128", 2, 128, 24, true, mixed, kNothing, kAllOk);
    bad += run_case("n64", 2, 64, 24, true, mixed, kNothing, kAllOk);      // the entry's other route
    if (bad) { printf("qp_sens_big: FAILED\n"); return 1; }
    printf("qp_sens_big: ok\n");
    return 0;
}
#endif
