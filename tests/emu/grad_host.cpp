// tests/emu/grad_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The posture-gradient producer (opensot_amd/csrc/osot_grad.h) through the host lock-step emulation of
// tests/emu/hip/hip_runtime.h, with the checks of osot_grad_create / osot_posture_gradient (grad_build, grad_check_batch).  Built by
// tests/emu/build_grad.sh; used by tests/test_posture_gradient_host.py (no GPU needed).  libosot_mi355x.so launches the same kernel body.
// With -DOSOT_GRAD_STANDALONE it is a program of its own (one small case, for a sanitizer build).
#include <osot_team.h>
#include "osot_grad.h"

using namespace osot;

extern "C" __attribute__((visibility("default"))) int grad_host_gradient(const osot_kin_desc* tree, const osot_grad_desc* desc,
                                                                        const osot_grad_batch* b) {
    static DevGrad h;
    const char* why = "";
    int rc = grad_build(tree, desc, h, &why);
    if (rc == OSOT_OK) rc = grad_check_batch(h.k.d.n, h.n_terms, b, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "grad host: %s\n", why); return rc; }
    if (b->B == 0) return OSOT_OK;
    emu::launch(osot_grad_kernel<64>, (unsigned)b->B, 0, 64, (const DevGrad*)&h, *b, grad_kin_batch(*b));
    return OSOT_OK;
}

#ifdef OSOT_GRAD_STANDALONE
// a 5-joint arm on a slider (prismatic, then four revolute joints with skewed axes), one frame at the tip: every kind, B = 2
int main() {
    static osot_kin_desc t;
    static osot_grad_desc d;
    std::memset(&t, 0, sizeof(t));
    std::memset(&d, 0, sizeof(d));
    t.n = 5;
    const double ax[5][3] = {{1, 0, 0}, {0, 0, 1}, {0, 1, 0}, {0.6, 0, 0.8}, {0, 1, 0}};
    for (int j = 0; j < t.n; ++j) {
        t.parent[j] = j - 1;
        t.type[j] = j == 0 ? OSOT_JOINT_PRISMATIC : OSOT_JOINT_REVOLUTE;
        for (int i = 0; i < 3; ++i) { t.axis[j][i] = ax[j][i]; t.p0[j][i] = 0.05 * (i + 1) + 0.03 * j; t.com[j][i] = 0.02 * (j + i); }
        for (int i = 0; i < 9; ++i) t.R0[j][i] = (i % 4 == 0) ? 1.0 : 0.0;
        t.mass[j] = 1.0 + 0.5 * j;
    }
    t.n_frames = 1;
    t.frame_joint[0] = 4;
    for (int i = 0; i < 9; ++i) t.frame_R[0][i] = (i % 4 == 0) ? 1.0 : 0.0;
    t.frame_p[0][2] = 0.1;
    d.n_terms = 3;
    for (int k = 0; k < 3; ++k) {
        d.kind[k] = k; d.step[k] = 1.0e-3; d.lambda[k] = 1.0;
        for (int j = 0; j < t.n; ++j) d.W_diag[k][j] = 1.0 + 0.1 * j;
    }
    d.gravity[2] = -9.81;
    const int B = 2;
    std::vector<double> q(B * t.n), out(3 * B * t.n, 7.0), val(3 * B, 7.0);
    for (int i = 0; i < B * t.n; ++i) q[i] = 0.3 * std::sin(1.0 + i);
    osot_grad_batch b;
    std::memset(&b, 0, sizeof(b));
    b.B = B; b.q = q.data();
    for (int k = 0; k < 3; ++k) { b.b[k] = out.data() + k * B * t.n; b.b_stride[k] = t.n; b.value[k] = val.data() + k * B; }
    const int rc = grad_host_gradient(&t, &d, &b);
    if (rc != OSOT_OK) return 1;
    for (double v : out) if (!std::isfinite(v) || v == 7.0) { printf("bad output %g\n", v); return 2; }
    for (double v : val) if (!std::isfinite(v) || v == 7.0) { printf("bad value %g\n", v); return 2; }
    printf("grad standalone ok: effort %.17g index %.17g\n", val[2 * B], val[B]);
    return 0;
}
#endif
