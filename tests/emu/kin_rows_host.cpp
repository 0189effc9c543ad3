// tests/emu/kin_rows_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The kinematics producer (opensot_amd/csrc/osot_kin.h) with its ROWS flag on -- the row sets and gaze references -- through the host
// lock-step emulation of tests/emu/hip/hip_runtime.h, both JMAX, with and without the closed-form pair stage, and with the checks of
// osot_kin_create (the tree order, kin_check_frames, kin_check_rowsets).  Built by tests/kin_rows_ref.py; used by
// tests/test_kin_rows_host.py (no GPU needed) and tests/test_kin_rows_gpu.py.  libosot_mi355x.so launches the same kernel body.
#include <osot_team.h>
#include "osot_kin.h"

using namespace osot;

namespace {
int build(const osot_kin_desc* d, DevKin& h, const char** why) {
    if (!d || d->n < 1 || d->n > OSOT_KIN_MAX_JOINTS) { *why = "joint count out of range"; return OSOT_ERR_INVALID; }
    if (d->n_frames < 0 || d->n_frames > OSOT_KIN_MAX_FRAMES) { *why = "frame count out of range"; return OSOT_ERR_INVALID; }
    for (int j = 0; j < d->n; ++j)
        if (d->parent[j] >= j || d->parent[j] < -1) { *why = "joints must be in tree order (parent[j] < j)"; return OSOT_ERR_INVALID; }
    std::memset(&h, 0, sizeof(h));
    h.d = *d;
    kin_build_tables(h);
    int rc = kin_check_frames(d, why);
    if (rc == OSOT_OK) rc = kin_check_rowsets(d, why);
    return rc;
}

// The row-set and gaze stage ALONE, on a pose and a world Jacobian that are GIVEN (the device's own outputs): what the stage computes
// from its inputs, apart from the stages in front of it.  pose [F][B][12], J [F][B][6][n] (world frames, no options).
template <int JMAX>
void stage_kernel(const DevKin* K, const osot_kin_batch Bt, const double* pose, const double* J) {
    constexpr int PACK = 64 / JMAX;
    const int sub = (PACK == 2) ? (int)(threadIdx.x >> 5) : 0;
    const int j = (PACK == 2) ? (int)(threadIdx.x & 31u) : (int)threadIdx.x;
    const long long inst = (long long)blockIdx.x * PACK + sub;
    const bool live = inst < Bt.B;
    const int n = K->d.n;
    const bool valid = j < n && live;
    const long long io = live ? inst : 0;
    for (int s = 0; s < K->d.n_rowsets; ++s) {
        double* As = Bt.rowset_A[s];
        double* bs = Bt.rowset_b[s];
        if (!As && !bs) continue;
        const int f = K->d.rowset_frame[s];
        const double* T = pose + ((long long)f * Bt.B + io) * 12;
        double colw[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Rf[9];
        for (int i = 0; i < 9; ++i) Rf[i] = T[i];
        if (valid) for (int r = 0; r < 6; ++r) colw[r] = J[(((long long)f * Bt.B + io) * 6 + r) * n + j];
        kin_rowset<JMAX>(K, s, As ? As + io * Bt.rowset_A_stride[s] : nullptr, bs ? bs + io * Bt.rowset_b_stride[s] : nullptr,
                         Bt.rowset_qdot ? Bt.rowset_qdot + io * n : nullptr, live, valid, j, n, colw, Rf);
    }
    if (j < K->d.n_gaze && live && Bt.gaze_point[j] && Bt.gaze_ref[j])
        kin_gaze_ref(pose + ((long long)K->d.gaze_frame[j] * Bt.B + inst) * 12, Bt.gaze_point[j] + inst * 3, Bt.gaze_ref[j] + inst * 12);
}
}  // namespace

// osot_kin_create's answer to a description, without a device: the code and the reason
extern "C" __attribute__((visibility("default"))) int kin_rows_host_check(const osot_kin_desc* d, const char** why) {
    static DevKin h;
    *why = "";
    return build(d, h, why);
}

extern "C" __attribute__((visibility("default"))) int kin_rows_host_kinematics(const osot_kin_desc* d, const osot_kin_batch* b) {
    static DevKin h;
    const char* why = "";
    const int rc = build(d, h, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "kin rows host: %s\n", why); return rc; }
    if (!b || b->B < 0 || !b->q) return OSOT_ERR_INVALID;
    for (int s = 0; s < d->n_rowsets; ++s)
        if (b->rowset_b[s] && !b->rowset_qdot) return OSOT_ERR_INVALID;
    if (b->B == 0) return OSOT_OK;
    const bool pairs = d->n_pairs > 0 && (b->pair_dist || b->pair_J || b->pair_points);
    if (d->n <= 32) {
        if (pairs) emu::launch(osot_kin_kernel<true, 32, false, true>, (unsigned)((b->B + 1) / 2), 0, 64, (const DevKin*)&h, *b);
        else emu::launch(osot_kin_kernel<false, 32, false, true>, (unsigned)((b->B + 1) / 2), 0, 64, (const DevKin*)&h, *b);
    } else {
        if (pairs) emu::launch(osot_kin_kernel<true, 64, false, true>, (unsigned)b->B, 0, 64, (const DevKin*)&h, *b);
        else emu::launch(osot_kin_kernel<false, 64, false, true>, (unsigned)b->B, 0, 64, (const DevKin*)&h, *b);
    }
    return OSOT_OK;
}

extern "C" __attribute__((visibility("default"))) int kin_rows_host_stage(const osot_kin_desc* d, const osot_kin_batch* b, const double* pose,
                                                                          const double* J) {
    static DevKin h;
    const char* why = "";
    const int rc = build(d, h, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "kin rows host: %s\n", why); return rc; }
    if (!b || b->B < 1 || !pose || !J) return OSOT_ERR_INVALID;
    if (d->n <= 32) emu::launch(stage_kernel<32>, (unsigned)((b->B + 1) / 2), 0, 64, (const DevKin*)&h, *b, pose, J);
    else emu::launch(stage_kernel<64>, (unsigned)b->B, 0, 64, (const DevKin*)&h, *b, pose, J);
    return OSOT_OK;
}

extern "C" __attribute__((visibility("default"))) int kin_rows_host_s33(const double* normal, double* s33, double* unit) {
    return kin_pure_rolling_s33(normal, s33, unit);
}
