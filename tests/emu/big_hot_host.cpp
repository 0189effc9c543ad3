// tests/emu/big_hot_host.cpp -- TEST INFRASTRUCTURE: the HOT instantiation of the wide-QP solver (opensot_amd/csrc/osot_qp_big.h,
// big::solve<true>) compiled for the host, so that the hot start of the 65 .. 128-variable route is checked where no GPU is present.
// Not part of the product: libosot_mi355x.so runs the same source as a 256-thread workgroup (osot_qp_big_hot_kernel).
//
// Two teams, as in cascade_wide_host.cpp: a team of one thread (every parallel section a plain loop), and a team of nthreads POSIX
// threads whose sections run one thread at a time in a FIXED order (a barrier passes the turn to the next thread of the order).
// Order 0 lets thread 0 finish each section before the others start, order 1 lets it start last: a value that thread 0 writes in a
// section where the others still read it -- a missing barrier -- gives the others a different value under the two orders, and the
// results differ from the team of one.
//
// With -DOSOT_BIG_HOT_MAIN the file is a stand-alone program (for a sanitizer build): it reads one problem and a number of hot lists
// from a binary file, solves the problem once per list and prints what came out.  Every array lives in a heap block of exactly its
// size, so an access out of range is an error the sanitizer sees.
#define OSOT_BIG_HOST 1
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include "osot_qp_big.h"

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
}  // namespace

// the three hot-start constants as the solver's own code sees them (by unqualified name from inside namespace big), and the list length
namespace osot { namespace big {
static void hot_constants_seen(double* out) { out[0] = kHotBatch; out[1] = kHotAbandon; out[2] = kHotDropTol; out[3] = kHotLen; }
} }
extern "C" __attribute__((visibility("default")))
void osot_big_hot_constants(double* out) { osot::big::hot_constants_seen(out); }

// hot_in / hot_out: [128] each (they may be the same array).  nthreads = 1: the team of one; > 1: the turn-taking team with
// thread 0 first (t0_last = 0) or last (t0_last = 1).
extern "C" __attribute__((visibility("default")))
int osot_big_hot_host_solve(int n, int nc, const double* H, const double* g, const double* A, const double* lA, const double* uA,
                            const double* l, const double* u, double eps_abs, int max_iter, double* x, int* status, int* iters,
                            const int* hot_in, int* hot_out, int nthreads, int t0_last) {
    using namespace osot::big;
    if (n < 1 || n > kMaxVars || nc < 0 || nc > kMaxRows || nthreads < 1 || nthreads > 64 || !hot_in || !hot_out) return -1;
    std::vector<double> work(2 * (size_t)n * n);
    std::vector<double> sh((shared_bytes(n, nc) + 7) / 8);
    Args a;
    a.n = n; a.nc = nc; a.max_iter = max_iter > 0 ? max_iter : 20 * (n + nc) + 100; a.eps = eps_abs;
    a.H = H; a.g = g; a.A = A; a.lA = lA; a.uA = uA; a.l = l; a.u = u;
    a.x = x; a.status = status; a.iters = iters;
    a.Lw = work.data(); a.J = work.data() + (size_t)n * n;
    a.hot_in = hot_in; a.hot_out = hot_out;
    const Shared s = carve(sh.data(), n, nc);
    if (nthreads == 1) {
        solve<true>(TeamOne{}, a, s);
        return 0;
    }
    Turns T;
    for (int i = 0; i < nthreads; ++i) T.order.push_back(t0_last ? (i + 1) % nthreads : i);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t] {
            const TeamTurns tm{t, nthreads, &T};
            T.wait_turn(t);
            solve<true>(tm, a, s);
            T.pass();                 // (every member leaves after the same final barrier)
        });
    for (auto& t : th) t.join();
    return 0;
}

#ifdef OSOT_BIG_HOT_MAIN
// file: int32 n, nc, has_box, n_lists, max_iter; float64 eps; float64 H[n n], g[n], A[nc n], lA[nc], uA[nc], (l[n], u[n]);
// int32 lists[n_lists][128].  Per list one line: status iterations, then x (17 digits), then the recorded list.
namespace {
template <class T> bool rd(std::FILE* f, std::vector<T>& v, size_t count) { v.resize(count); return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count; }
}
int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s problem.bin\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<int> hd;
    std::vector<double> eps, H, g, A, lA, uA, l, u;
    bool ok = rd(f, hd, 5) && rd(f, eps, 1);
    if (!ok || hd[0] < 1 || hd[0] > osot::big::kMaxVars || hd[1] < 0 || hd[1] > osot::big::kMaxRows || hd[3] < 0 || hd[3] > 64) { std::fprintf(stderr, "bad header\n"); return 2; }
    const int n = hd[0], nc = hd[1], has_box = hd[2], n_lists = hd[3], max_iter = hd[4];
    ok = rd(f, H, (size_t)n * n) && rd(f, g, n) && rd(f, A, (size_t)nc * n) && rd(f, lA, nc) && rd(f, uA, nc);
    if (has_box) ok = ok && rd(f, l, n) && rd(f, u, n);
    for (int k = 0; ok && k < n_lists; ++k) {
        std::vector<int> in, out(osot::big::kHotLen, 12345);
        ok = rd(f, in, osot::big::kHotLen);
        if (!ok) break;
        std::vector<double> x(n, 0.0);
        std::vector<int> st(1, -1), it(1, 0);
        const int rc = osot_big_hot_host_solve(n, nc, H.data(), g.data(), nc ? A.data() : nullptr, nc ? lA.data() : nullptr,
                                               nc ? uA.data() : nullptr, has_box ? l.data() : nullptr, has_box ? u.data() : nullptr,
                                               eps[0], max_iter, x.data(), st.data(), it.data(), in.data(), out.data(), 1, 0);
        if (rc != 0) { std::fprintf(stderr, "refused\n"); return 2; }
        std::printf("%d %d", st[0], it[0]);
        for (int i = 0; i < n; ++i) std::printf(" %.17g", x[i]);
        for (int q = 0; q < osot::big::kHotLen; ++q) std::printf(" %d", out[q]);
        std::printf("\n");
    }
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short file\n"); return 2; }
    return 0;
}
#endif
