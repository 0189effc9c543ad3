// tests/emu/cascade_wide_hot_host.cpp -- TEST INFRASTRUCTURE: the HOT instantiation of the wide iHQP cascade
// (opensot_amd/csrc/osot_cascade_wide.h, cascade_instance<true>: every level's working set carried from call to call in a state the
// caller owns) compiled for the host, so that osot_ihqp_solve_hot's algorithm is checked where no GPU is present.  Not part of the
// product: libosot_mi355x.so runs the same source as one 256-thread workgroup per instance (osot_cascade_wide_hot_kernel).
//
// Two teams, as in cascade_wide_host.cpp: a team of one thread (every parallel section a plain loop), and a team of nthreads POSIX
// threads whose sections run one thread at a time in a FIXED order (a barrier passes the turn to the next thread of the order).
// Order 0 lets thread 0 finish each section before the others start, order 1 lets it start last: a value that thread 0 writes in a
// section where the others still read it -- a missing barrier -- gives the others a different value under the two orders, and the
// results differ from the team of one.
//
// With -DOSOT_WIDE_HOT_MAIN the file is a stand-alone program (for a sanitizer build): it builds two plans of its own, solves them
// cold and then from foreign lists of every kind (see main), and exits 0 when every hot answer is the cold one.  Every array lives
// in a heap block of exactly its size, so an access out of range is an error the sanitizer sees.
#define OSOT_BIG_HOST 1
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include "osot_cascade_wide.h"

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

// qb: host pointers, as osot_ihqp_solve_hot takes device pointers.  task_active: [OSOT_MAX_LEVELS * OSOT_MAX_TASKS] or null.
// hot: [B][n_levels][128] (osot_solver_hot_state_ints), or null for the cold instantiation (what wide_host_ihqp runs).
// nthreads = 1: the team of one; > 1: the turn-taking team with thread 0 first (t0_last = 0) or last (t0_last = 1).
extern "C" __attribute__((visibility("default")))
int wide_host_ihqp_hot(const osot_plan_desc* pd, const osot_qp_batch* qb, const unsigned char* task_active, int nthreads, int t0_last, int* hot) {
    using namespace osot;
    if (!pd || !qb || pd->n < 1 || pd->n > OSOT_MAX_QP_VARS || nthreads < 1 || nthreads > 64) return -1;
    wide::Plan P;
    wide::make_plan(*pd, qb->level_active, task_active, P);
    wide::Batch D;
    std::memset(&D, 0, sizeof(D));
    const char* why = "";
    const int rc = fill_batch_ptrs(*pd, P, *qb, D, &why);   // (the product's checks and null-out rules: wide_launch)
    if (rc != OSOT_OK) return rc;
    const int n = P.n;
    std::vector<double> slot(2 * (size_t)n * n);
    std::vector<double> smem((wide::shared_bytes(n, P.nrows) + 7) / 8 + 2);
    char* sm = reinterpret_cast<char*>(smem.data());
    auto instance = [&](const auto& tm, long long inst) {
        if (hot) wide::cascade_instance<true>(tm, P, D, inst, sm, slot.data(), hot);
        else wide::cascade_instance(tm, P, D, inst, sm, slot.data());
    };
    for (long long inst = 0; inst < D.B; ++inst) {
        if (nthreads == 1) {
            instance(TeamOne{}, inst);
            continue;
        }
        Turns T;
        for (int i = 0; i < nthreads; ++i) T.order.push_back(t0_last ? (i + 1) % nthreads : i);
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; ++t)
            th.emplace_back([&, t] {
                const TeamTurns tm{t, nthreads, &T};
                T.wait_turn(t);
                instance(tm, inst);
                T.pass();                 // (every member leaves after the same final barrier)
            });
        for (auto& x : th) x.join();
    }
    return 0;
}

#ifdef OSOT_WIDE_HOT_MAIN
// Two plans built here: two GENERIC levels, the second closed by an implicit Postural block over all variables (a full-rank cost:
// the answer is well defined beyond the eps of the regularisation), a block of GENERIC rows (the first n_eq of them equalities, every third of the others
// one-sided), a block of task-local unit rows at the second level, a GENERIC box.  wide: 70 variables (the whole list is staged in
// LDS); small: 20 variables with 2 (n + nc) < 128 (thread 0 reads the tail of the list where it is).
namespace {
struct Rng {
    unsigned long long s;
    double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    double sym(double a) { return a * (2.0 * uni() - 1.0); }
    int below(int m) { return (int)(uni() * m) % m; }
};
struct Problem {
    osot_plan_desc pd;
    int B, n, L, nc, nrows_gen, nloc;
    std::vector<double> A[2], b[2], C, lo, up, l, u;
    std::vector<int> m;
};
void make_problem(Problem& p, int B, int n, int m0, int m1, int n_eq, int n_ineq, int nloc, unsigned long long seed) {
    std::memset(&p.pd, 0, sizeof(p.pd));
    p.B = B; p.n = n; p.L = 2; p.nrows_gen = n_eq + n_ineq; p.nloc = nloc; p.nc = p.nrows_gen + nloc;
    p.m = {m0, m1};
    p.pd.n = n; p.pd.n_levels = 2; p.pd.eps_abs = 4.442e-11;   // (iHQP's default eps_regularisation: 1e3 * 2.221e-16 * 2e2); max_iter 0 = the default
    for (int k = 0; k < 2; ++k) {
        p.pd.level[k].n_tasks = 1;
        p.pd.level[k].task[0].kind = OSOT_TASK_GENERIC; p.pd.level[k].task[0].rows = p.m[k]; p.pd.level[k].task[0].weight = 1.0;
        p.pd.level[k].task[0].lambda = 1.0; p.pd.level[k].task[0].sub_lambda = 1.0;
    }
    p.pd.level[1].n_tasks = 2;
    p.pd.level[1].task[1] = p.pd.level[1].task[0];
    p.pd.level[1].task[1].kind = OSOT_TASK_POSTURAL; p.pd.level[1].task[1].rows = n;
    p.pd.n_bounds = 1; p.pd.bound[0].kind = OSOT_BOUND_GENERIC; p.pd.bound[0].scaling = 1.0;
    p.pd.n_rowblocks = 2;
    p.pd.rowblock[0].kind = OSOT_ROWS_GENERIC; p.pd.rowblock[0].rows = p.nrows_gen;
    p.pd.rowblock[1].kind = OSOT_ROWS_UNIT_GENERIC; p.pd.rowblock[1].rows = nloc; p.pd.rowblock[1].first_col = 2; p.pd.rowblock[1].only_level = 2;
    Rng r{seed};
    for (int k = 0; k < 2; ++k) {
        p.A[k].resize((size_t)B * p.m[k] * n); p.b[k].resize((size_t)B * (p.m[k] + (k == 1 ? n : 0)));   // (b of the Postural block behind the task's)
        for (auto& v : p.A[k]) v = r.sym(0.5);
        for (auto& v : p.b[k]) v = r.sym(0.3);
    }
    p.C.resize((size_t)B * p.nrows_gen * n); p.lo.resize((size_t)B * p.nc); p.up.resize((size_t)B * p.nc);
    p.l.resize((size_t)B * n); p.u.resize((size_t)B * n);
    for (auto& v : p.C) v = r.sym(0.5);
    // the variables of the task-local rows stay out of the first level and of the global rows: whatever the first level's solution,
    // the second level finds them inside their local bounds, so the stack is feasible at every level
    for (int i = 0; i < B; ++i)
        for (int c = 2; c < 2 + nloc; ++c) {
            for (int q = 0; q < m0; ++q) p.A[0][((size_t)i * m0 + q) * n + c] = 0.0;
            for (int q = 0; q < p.nrows_gen; ++q) p.C[((size_t)i * p.nrows_gen + q) * n + c] = 0.0;
        }
    for (int i = 0; i < B; ++i) {
        std::vector<double> x0(n);
        for (auto& v : x0) v = r.sym(0.02);
        for (int c = 0; c < n; ++c) { p.l[(size_t)i * n + c] = -0.05; p.u[(size_t)i * n + c] = 0.05; }
        for (int q = 0; q < p.nrows_gen; ++q) {
            double cx = 0.0;
            for (int c = 0; c < n; ++c) cx += p.C[((size_t)i * p.nrows_gen + q) * n + c] * x0[c];
            double lo = cx - 0.02 * r.uni(), up = cx + 0.02 * r.uni();
            if (q < n_eq) lo = up = cx;
            else if (q % 3 == 0) lo = -1.0e20;
            else if (q % 3 == 1) up = 1.0e20;
            p.lo[(size_t)i * p.nc + q] = lo; p.up[(size_t)i * p.nc + q] = up;
        }
        for (int q = 0; q < nloc; ++q) { p.lo[(size_t)i * p.nc + p.nrows_gen + q] = -0.03; p.up[(size_t)i * p.nc + p.nrows_gen + q] = 0.03; }
    }
}
struct Result { std::vector<double> dq; std::vector<int> status, iters; };
int run(const Problem& p, int* hot, Result& out) {
    osot_qp_batch qb;
    std::memset(&qb, 0, sizeof(qb));
    qb.B = p.B;
    for (int k = 0; k < 2; ++k) { qb.A[k] = p.A[k].data(); qb.b[k] = p.b[k].data(); }
    qb.C = p.C.data(); qb.lo = p.lo.data(); qb.up = p.up.data(); qb.l = p.l.data(); qb.u = p.u.data();
    out.dq.assign((size_t)p.B * p.n, 0.0); out.status.assign(p.B, -1); out.iters.assign(p.B, 0);
    qb.dq = out.dq.data(); qb.status = out.status.data(); qb.iterations = out.iters.data();
    return wide_host_ihqp_hot(&p.pd, &qb, nullptr, 1, 0, hot);
}
}  // namespace

int main() {
    Problem wide, small;
    make_problem(wide, 2, 70, 12, 16, 4, 26, 6, 11);
    make_problem(small, 2, 20, 4, 6, 2, 4, 2, 5);
    std::vector<int> recorded_small;
    int bad = 0;
    for (Problem* pp : {&small, &wide}) {
        const Problem& p = *pp;
        const int per = p.L * osot::big::kHotLen, N = p.B * per, n = p.n, nc = p.nc;
        Result cold;
        if (run(p, nullptr, cold) != 0) { std::fprintf(stderr, "refused\n"); return 2; }
        for (int i = 0; i < p.B; ++i) if (cold.status[i] != 0) { std::fprintf(stderr, "n = %d: cold status %d\n", n, cold.status[i]); return 2; }
        std::vector<std::vector<int>> lists;
        std::vector<const char*> names;
        auto add = [&](const char* nm, std::vector<int> v) { names.push_back(nm); lists.push_back(std::move(v)); };
        add("none", std::vector<int>(N, -1));
        Rng r{17};
        { std::vector<int> v(N); for (auto& e : v) e = r.below(4 * (n + nc)) - (n + nc) / 2; add("random, negative and out of range", v); }
        { std::vector<int> v(N); for (auto& e : v) e = (r.uni() < 0.5) ? 0x7fffffff - r.below(3) : (int)0x80000000 + r.below(3); add("extreme", v); }
        { std::vector<int> v(N); for (int q = 0; q < N; ++q) v[q] = 2 * (n + (q / 7) % nc) + 1; add("duplicates", v); }
        { std::vector<int> v(N); for (int q = 0; q < N; ++q) v[q] = 2 * (q % osot::big::kHotLen); add("every lower bound", v); }
        { std::vector<int> v(N); for (int q = 0; q < N; ++q) v[q] = 2 * (n + q % 4) + (q & 1); add("equality rows", v); }
        { std::vector<int> v(N); for (int q = 0; q < N; ++q) { const int row = 4 + q % (p.nrows_gen - 4); v[q] = 2 * (n + row) + ((row % 3 == 0) ? 0 : 1); } add("infinite sides", v); }
        if (!recorded_small.empty()) { std::vector<int> v(N, -1); for (int q = 0; q < N && q < (int)recorded_small.size(); ++q) v[q] = recorded_small[q]; add("another plan's state", v); }
        for (size_t c = 0; c < lists.size(); ++c) {
            std::vector<int> state = lists[c];
            for (int cycle = 0; cycle < 2; ++cycle) {        // the foreign list, then what that solve recorded
                Result hot;
                if (run(p, state.data(), hot) != 0) { std::fprintf(stderr, "refused\n"); return 2; }
                double worst = 0.0, scale = 1.0;
                for (size_t e = 0; e < cold.dq.size(); ++e) { scale = std::fmax(scale, std::fabs(cold.dq[e])); worst = std::fmax(worst, std::fabs(hot.dq[e] - cold.dq[e])); }
                int st = 0, it = 0, itc = 0;
                for (int i = 0; i < p.B; ++i) { st |= hot.status[i]; it += hot.iters[i]; itc += cold.iters[i]; }
                for (int e : state) if (e < -1 || (e >> 1) >= n + nc + p.m[0]) { std::fprintf(stderr, "n = %d, %s: recorded entry %d\n", n, names[c], e); ++bad; break; }
                std::printf("n = %d  %-36s cycle %d: status %d  iterations %d (cold %d)  |dq - cold| %.3g\n", n, names[c], cycle, st, it, itc, worst / scale);
                if (st != 0 || !(worst <= 1.0e-8 * scale)) ++bad;
            }
            if (pp == &small && c == 0) recorded_small = state;
        }
    }
    if (bad) { std::fprintf(stderr, "%d case(s) differ from the cold answer\n", bad); return 1; }
    return 0;
}
#endif
