// tests/emu/cascade_wide_host.cpp -- TEST INFRASTRUCTURE: the wide iHQP cascade of opensot_amd/csrc/osot_cascade_wide.h compiled for
// the host, so that its algorithm is checked against the oracle where no GPU is present.  Not part of the product:
// libosot_mi355x.so runs the same source as one 256-thread workgroup per instance.
//
// Two teams: a team of one thread (every parallel section a plain loop), and a team of nthreads POSIX threads whose sections run
// one thread at a time in a FIXED order (a barrier passes the turn to the next thread of the order; after the last one the next
// section starts).  Order 0 lets thread 0 finish each section before the others start, order 1 lets it start last: a value that
// thread 0 writes in a section where the others still read it -- a missing barrier -- gives the others a different value under the
// two orders, and the results differ from the team of one.
#define OSOT_BIG_HOST 1
#include <condition_variable>
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

// The active-set tolerances the wide route was compiled with, by unqualified name from inside namespace big -- what the solver's own code
// sees: a private copy re-introduced in osot_qp_big.h would shadow the shared header's (osot_qp_tol.h) here exactly as it would there.
namespace osot { namespace big {
static void tolerances_seen(double* out) {
    out[0] = kViolTol; out[1] = kEqTol; out[2] = kDepTol2; out[3] = kDepFloor2; out[4] = kRatioTol; out[5] = kSlackTol;
    out[6] = kSlackCap; out[7] = kSpanAccept; out[8] = kRefineFloor; out[9] = (double)kRefineMax; out[10] = kInfty;
}
} }
// out[11]: violation, equality, dependence, dependence floor, ratio, slack (relative), slack cap, span accept, refine floor, refinements, infinity
extern "C" __attribute__((visibility("default")))
void wide_host_tolerances(double* out) { osot::big::tolerances_seen(out); }

// qb: host pointers, as osot_ihqp_solve takes device pointers.  task_active: [OSOT_MAX_LEVELS * OSOT_MAX_TASKS] or null.
// nthreads = 1: the team of one; > 1: the turn-taking team with thread 0 first (t0_last = 0) or last (t0_last = 1).
extern "C" __attribute__((visibility("default")))
int wide_host_ihqp(const osot_plan_desc* pd, const osot_qp_batch* qb, const unsigned char* task_active, int nthreads, int t0_last) {
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
    for (long long inst = 0; inst < D.B; ++inst) {
        if (nthreads == 1) {
            wide::cascade_instance(TeamOne{}, P, D, inst, sm, slot.data());
            continue;
        }
        Turns T;
        for (int i = 0; i < nthreads; ++i) T.order.push_back(t0_last ? (i + 1) % nthreads : i);
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; ++t)
            th.emplace_back([&, t] {
                const TeamTurns tm{t, nthreads, &T};
                T.wait_turn(t);
                wide::cascade_instance(tm, P, D, inst, sm, slot.data());
                T.pass();                 // (every member leaves after the same final barrier)
            });
        for (auto& x : th) x.join();
    }
    return 0;
}
