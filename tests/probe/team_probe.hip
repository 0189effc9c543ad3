// tests/probe/team_probe.hip -- TEST INFRASTRUCTURE ONLY: the device build of tests/probe/team_probe.h against the product's
// opensot_amd/csrc/osot_team.h (tests/native_build.py team_probe -> libosot_team_probe.so; loaded by tests/helpers.py:team_probe_lib).
#include "team_probe.h"

#define PROBE_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = (int)e_; goto done; } } while (0)

// allocates, copies in, launches one wavefront per case, synchronises, copies back; returns the HIP error code (0 = fine)
// or a negative number for arguments the kernel must not be handed (osot_probe::probe_check)
extern "C" __attribute__((visibility("default"))) int osot_team_probe(int ncase, const int* op, const int* np, const int* sarg,
                                                                      const double* din, const int* iin, const float* fin,
                                                                      double* dout, int* iout, float* fout) {
    int rc = osot_probe::probe_check(ncase, op, np, sarg);
    if (rc) return rc;
    const size_t nk = (size_t)ncase * sizeof(int), nd = (size_t)ncase * PROBE_ND * 64 * sizeof(double),
                 ni = (size_t)ncase * PROBE_NI * 64 * sizeof(int), nf = (size_t)ncase * PROBE_NF * 64 * sizeof(float);
    int *d_op = nullptr, *d_np = nullptr, *d_sarg = nullptr, *d_iin = nullptr, *d_iout = nullptr;
    double *d_din = nullptr, *d_dout = nullptr;
    float *d_fin = nullptr, *d_fout = nullptr;
    PROBE_HIP(hipMalloc(&d_op, nk)); PROBE_HIP(hipMalloc(&d_np, nk)); PROBE_HIP(hipMalloc(&d_sarg, nk));
    PROBE_HIP(hipMalloc(&d_din, nd)); PROBE_HIP(hipMalloc(&d_dout, nd));
    PROBE_HIP(hipMalloc(&d_iin, ni)); PROBE_HIP(hipMalloc(&d_iout, ni));
    PROBE_HIP(hipMalloc(&d_fin, nf)); PROBE_HIP(hipMalloc(&d_fout, nf));
    PROBE_HIP(hipMemcpy(d_op, op, nk, hipMemcpyHostToDevice)); PROBE_HIP(hipMemcpy(d_np, np, nk, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_sarg, sarg, nk, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_din, din, nd, hipMemcpyHostToDevice)); PROBE_HIP(hipMemcpy(d_dout, dout, nd, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_iin, iin, ni, hipMemcpyHostToDevice)); PROBE_HIP(hipMemcpy(d_iout, iout, ni, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_fin, fin, nf, hipMemcpyHostToDevice)); PROBE_HIP(hipMemcpy(d_fout, fout, nf, hipMemcpyHostToDevice));
    osot_probe::team_probe_kernel<<<dim3((unsigned)ncase), dim3(64), 0, 0>>>(d_op, d_np, d_sarg, d_din, d_iin, d_fin, d_dout, d_iout, d_fout);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(dout, d_dout, nd, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(iout, d_iout, ni, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(fout, d_fout, nf, hipMemcpyDeviceToHost));
done:
    for (void* p : {(void*)d_op, (void*)d_np, (void*)d_sarg, (void*)d_din, (void*)d_dout, (void*)d_iin, (void*)d_iout, (void*)d_fin, (void*)d_fout}) (void)hipFree(p);
    return rc;
}
