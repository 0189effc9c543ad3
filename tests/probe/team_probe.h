// tests/probe/team_probe.h -- TEST INFRASTRUCTURE ONLY.
// One probe kernel written only in terms of the osot_team.h interface and compiled twice from this text: for gfx950 against
// opensot_amd/csrc/osot_team.h (tests/probe/team_probe.hip -> libosot_team_probe.so) and for the host against the twin
// tests/emu/osot_team.h (tests/emu/emu_driver.cpp -> emu_team_probe).  tests/test_team_primitives.py compares the two with
// each other and with an independent numpy statement of every primitive.
//
// One wavefront per block, one case per block.  Case k reads
//     op[k], np[k], sarg[k]            the primitive, its NP template argument (32, 40, 56, 64; ignored where there is none)
//                                      and one wave-uniform integer argument (source lane, half selector, ...)
//     din [k][PROBE_ND][64]  double    per-lane inputs, slot-major: lane l's value of slot j is din[(k * PROBE_ND + j) * 64 + l]
//     iin [k][PROBE_NI][64]  int       (bit patterns of unsigned values; byte addresses for permute_f64)
//     fin [k][PROBE_NF][64]  float
// and writes every lane's outputs to dout [k][PROBE_ND][64], iout [k][PROBE_NI][64], fout [k][PROBE_NF][64] (slots a case does
// not write keep what the caller put there).  Every primitive is called by all 64 lanes outside any lane-dependent branch:
// the switch below is on wave-uniform values.
#pragma once
#include <osot_team.h>

enum : int {
    PROBE_ND = 8, PROBE_NI = 4, PROBE_NF = 2,
    // data movement
    OP_BCAST = 0, OP_BCAST_I, OP_BCAST_F32, OP_BCAST_U32, OP_UNIFORM_I, OP_UNIFORM_D, OP_UNIFORM_B, OP_UNIFORM_U32,
    OP_PERMUTE_F64, OP_ROWGROUP_GATHER4, OP_SHIFT_DOWN, OP_SHIFT_DOWN_I, OP_FROM_HALF,
    // masks
    OP_BALLOT_BELOW, OP_FIRST_LANE_EQUAL, OP_FIRST_LANE_EQUAL_F32,
    // reductions
    OP_QUAD_SUM, OP_ROW16_SUM, OP_ROWGROUP_SUM, OP_COLSUM, OP_COLSUM2, OP_HALFSUM, OP_COLMAX, OP_COLMIN, OP_COLMAX_F32,
    OP_ROW16_MAX_U32, OP_COLARGMIN,
    // matrix core
    OP_MFMA_F64,
    // scalar numerics (every slot is one argument)
    OP_FAST_RCP, OP_FAST_RCP1, OP_FAST_DIV, OP_FAST_SQRT_RSQRT, OP_FREXP_EXPONENT, OP_SCALE_POW2,
    OP_COUNT
};

namespace osot_probe {
using namespace osot;

struct Lane {
    const double* d; const int* i; const float* f;      // this lane's slot 0 (slot j is [64 * j])
    double* od; int* oi; float* of;
    int s;                                              // the wave-uniform argument
};

// the primitives templated on NP
template <int NP>
__device__ __forceinline__ void probe_np(int op, const Lane& L) {
    switch (op) {
    case OP_SHIFT_DOWN: L.od[0] = shift_down<NP>(L.d[0]); break;
    case OP_SHIFT_DOWN_I: L.oi[0] = shift_down_i<NP>(L.i[0]); break;
    case OP_FROM_HALF: L.od[0] = from_half<NP>(L.d[0], L.s); break;
    case OP_COLSUM: L.od[0] = colsum<NP>(L.d[0]); break;
    case OP_COLSUM2: { double ra, rb; colsum2<NP>(L.d[0], L.d[64], ra, rb); L.od[0] = ra; L.od[64] = rb; break; }
    case OP_HALFSUM: L.od[0] = halfsum<NP>(L.d[0]); break;
    case OP_COLMAX: L.od[0] = colmax<NP>(L.d[0]); break;
    case OP_COLMIN: L.od[0] = colmin<NP>(L.d[0]); break;
    case OP_COLMAX_F32: L.of[0] = colmax_f32<NP>(L.f[0]); break;
    case OP_COLARGMIN: { double v = L.d[0]; int p = L.i[0]; colargmin<NP>(v, p); L.od[0] = v; L.oi[0] = p; break; }
    default: break;
    }
}

__device__ __forceinline__ void probe_plain(int op, const Lane& L) {
    switch (op) {
    case OP_BCAST: L.od[0] = bcast(L.d[0], L.s); break;
    case OP_BCAST_I: L.oi[0] = bcast_i(L.i[0], L.s); break;
    case OP_BCAST_F32: L.of[0] = bcast_f32(L.f[0], L.s); break;
    case OP_BCAST_U32: L.oi[0] = (int)bcast_u32((unsigned)L.i[0], L.s); break;
    case OP_UNIFORM_I: L.oi[0] = uniform_i(L.i[0]); break;
    case OP_UNIFORM_D: L.od[0] = uniform_d(L.d[0]); break;
    case OP_UNIFORM_B: L.oi[0] = uniform_b(L.i[0] != 0) ? 1 : 0; break;
    case OP_UNIFORM_U32: L.oi[0] = (int)uniform_u32((unsigned)L.i[0]); break;
    case OP_PERMUTE_F64: L.od[0] = permute_f64(L.d[0], L.i[0]); break;
    case OP_ROWGROUP_GATHER4: {
        const Quad g = rowgroup_gather4(L.d[0]);
        L.od[0] = g.a; L.od[64] = g.b; L.od[128] = g.c; L.od[192] = g.d;
        break;
    }
    case OP_BALLOT_BELOW: {
        const unsigned long long m = wave_ballot(L.i[0] != 0);
        L.oi[0] = (int)(unsigned)m; L.oi[64] = (int)(unsigned)(m >> 32); L.oi[128] = lanes_below(m);
        break;
    }
    case OP_FIRST_LANE_EQUAL: L.oi[0] = first_lane_equal(L.d[0], L.d[64]); break;
    case OP_FIRST_LANE_EQUAL_F32: L.oi[0] = first_lane_equal_f32(L.f[0], L.f[64]); break;
    case OP_QUAD_SUM: L.od[0] = quad_sum(L.d[0]); break;
#ifndef OSOT_EMULATION
    case OP_ROW16_SUM: L.od[0] = row16_sum(L.d[0]); break;      // (the twin has none: no kernel body calls it directly)
#endif
    case OP_ROWGROUP_SUM: L.od[0] = rowgroup_sum(L.d[0]); break;
    case OP_ROW16_MAX_U32: L.oi[0] = (int)row16_max_u32((unsigned)L.i[0]); break;
    case OP_MFMA_F64: {
        v4f64 c;
        for (int r = 0; r < 4; ++r) c[r] = L.d[64 * (2 + r)];
        const v4f64 d = mfma_f64_16x16x4(L.d[0], L.d[64], c);
        for (int r = 0; r < 4; ++r) L.od[64 * r] = d[r];
        break;
    }
    case OP_FAST_RCP: for (int j = 0; j < PROBE_ND; ++j) L.od[64 * j] = fast_rcp(L.d[64 * j]); break;
    case OP_FAST_RCP1: for (int j = 0; j < PROBE_ND; ++j) L.od[64 * j] = fast_rcp1(L.d[64 * j]); break;
    case OP_FAST_DIV: for (int j = 0; j < PROBE_ND / 2; ++j) L.od[64 * j] = fast_div(L.d[64 * j], L.d[64 * (j + PROBE_ND / 2)]); break;
    case OP_FAST_SQRT_RSQRT:
        for (int j = 0; j < PROBE_ND / 2; ++j) {
            double s, rs;
            fast_sqrt_rsqrt(L.d[64 * j], s, rs);
            L.od[64 * j] = s; L.od[64 * (j + PROBE_ND / 2)] = rs;
        }
        break;
    case OP_FREXP_EXPONENT: for (int j = 0; j < PROBE_NI; ++j) L.oi[64 * j] = frexp_exponent(L.d[64 * j]); break;
    case OP_SCALE_POW2: for (int j = 0; j < PROBE_NI; ++j) L.od[64 * j] = scale_pow2(L.d[64 * j], L.i[64 * j]); break;
    default: break;
    }
}

static __global__ void __launch_bounds__(64) team_probe_kernel(const int* op, const int* np, const int* sarg, const double* din,
                                                               const int* iin, const float* fin, double* dout, int* iout, float* fout) {
    const long long k = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int o = uniform_i(op[k]), n = uniform_i(np[k]);
    Lane L;
    L.d = din + k * PROBE_ND * 64 + lane; L.od = dout + k * PROBE_ND * 64 + lane;
    L.i = iin + k * PROBE_NI * 64 + lane; L.oi = iout + k * PROBE_NI * 64 + lane;
    L.f = fin + k * PROBE_NF * 64 + lane; L.of = fout + k * PROBE_NF * 64 + lane;
    L.s = uniform_i(sarg[k]);
    if (o == OP_SHIFT_DOWN || o == OP_SHIFT_DOWN_I || o == OP_FROM_HALF || o == OP_COLSUM || o == OP_COLSUM2 || o == OP_HALFSUM ||
        o == OP_COLMAX || o == OP_COLMIN || o == OP_COLMAX_F32 || o == OP_COLARGMIN) {
        if (n == 32) probe_np<32>(o, L);
        else if (n == 40) probe_np<40>(o, L);
        else if (n == 56) probe_np<56>(o, L);
        else if (n == 64) probe_np<64>(o, L);
    } else {
        probe_plain(o, L);
    }
}

// the arguments a caller hands over are checked once, on the host, in both builds: 0 = fine
inline int probe_check(int ncase, const int* op, const int* np, const int* sarg) {
    if (ncase <= 0 || ncase > 4096) return -1;
    for (int k = 0; k < ncase; ++k) {
        if (op[k] < 0 || op[k] >= OP_COUNT) return -2;
        if (np[k] != 32 && np[k] != 40 && np[k] != 56 && np[k] != 64) return -3;
        if (sarg[k] < 0 || sarg[k] > 63) return -4;          // (a v_readlane index)
        if (op[k] == OP_FROM_HALF && sarg[k] > 1) return -4;
    }
    return 0;
}
}  // namespace osot_probe
