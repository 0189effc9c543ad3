// tests/emu/surface_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The update kernel and the inverse-dynamics producers (opensot_amd/csrc/osot_kernels.h, osot_id.h) through the host lock-step
// emulation of tests/emu/hip/hip_runtime.h, beyond the wavefront route: plans checked by the workgroup route's validator
// (n <= OSOT_MAX_QP_VARS) and ID models of nv + forces <= 128.  Built by tests/emu/build_surface.sh; used by
// tests/test_surface_contact_host.py (no GPU needed).  libosot_mi355x.so launches the same kernel bodies.
#include <osot_team.h>
#include "osot_host_plan.h"
#include "osot_id.h"

using namespace osot;

#define SURF_API extern "C" __attribute__((visibility("default")))

// osot_stack_update of either route: wide = 0 validates as osot_plan_validate, 1 as osot_plan_validate_wide
SURF_API int surf_stack_update(const osot_plan_desc* plan, const osot_leaf_batch* leaf, const osot_assembled_out* out, int wide) {
    const char* why;
    int rc = plan_validate(plan, &why, wide);
    if (rc != OSOT_OK) { fprintf(stderr, "surface host: %s\n", why); return rc; }
    static DevUpdatePlan PL;
    make_update_plan(*plan, PL);
    DevUpdate U;
    rc = make_update_args(*plan, PL, leaf, out, &PL, U, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "surface host: %s\n", why); return rc; }
    emu::launch(osot_update_kernel, (unsigned)leaf->B, 0, 64, U);
    return OSOT_OK;
}

// the producers with the size checks of osot_id_rows / osot_computed_torque (opensot_amd/csrc/osot_mi355x.hip: id_model_check)
static int surf_model_n(const osot_id_model* m) {
    const int nf = m->n_contacts * m->contact_dim;
    if (m->contact_dim != 3 && m->contact_dim != 6) return -1;
    if (nf > OSOT_ID_MAX_FORCE_VARS || m->nv + nf > OSOT_MAX_QP_VARS) return -1;
    return m->nv + nf;
}

SURF_API int surf_id_rows(const osot_id_model* m, double* C_dyn, long long dyn_stride, double* C_tau, long long tau_stride,
                          int n_tasks, const double* const* J, const int* J_rows, double* const* A_dst, const long long* A_stride) {
    const int n = surf_model_n(m);
    if (n < 0 || n_tasks < 0 || n_tasks > OSOT_MAX_TASKS) return OSOT_ERR_UNSUPPORTED;
    DevIdRows R;
    memset(&R, 0, sizeof(R));
    R.B = m->B; R.nv = m->nv; R.n_contacts = m->n_contacts; R.cdim = m->contact_dim; R.n = n;
    R.Bm = m->Bm; R.Jc = m->Jc; R.C_dyn = C_dyn; R.dyn_stride = dyn_stride; R.C_tau = C_tau; R.tau_stride = tau_stride;
    R.n_tasks = n_tasks;
    for (int i = 0; i < n_tasks; ++i) { R.J[i] = J[i]; R.J_rows[i] = J_rows[i]; R.A_dst[i] = A_dst[i]; R.A_stride[i] = A_stride[i]; }
    emu::launch(osot_id_rows_kernel, (unsigned)m->B, 0, 64, R);
    return OSOT_OK;
}

SURF_API int surf_computed_torque(const osot_id_model* m, const double* x, double* tau, int* ok, double fb_tol) {
    const int n = surf_model_n(m);
    if (n < 0) return OSOT_ERR_UNSUPPORTED;
    DevTorque T;
    memset(&T, 0, sizeof(T));
    T.B = m->B; T.nv = m->nv; T.n_contacts = m->n_contacts; T.cdim = m->contact_dim; T.n = n;
    T.floating_base = m->floating_base; T.Bm = m->Bm; T.h = m->h; T.Jc = m->Jc; T.x = x; T.tau = tau; T.ok = ok; T.fb_tol = fb_tol;
    emu::launch(osot_torque_kernel, (unsigned)m->B, 0, 64, T);
    return OSOT_OK;
}

SURF_API int surf_force_gains(int B, int nv, int rows, const double* J, const double* Bi, const double* Kp, const double* Kd,
                              const double* f, double* G, long long G_stride, double* a_ref) {
    if (nv < 1 || nv > OSOT_MAX_QP_VARS || rows < 1 || rows > 6) return OSOT_ERR_INVALID;
    DevForceGains F;
    memset(&F, 0, sizeof(F));
    F.B = B; F.nv = nv; F.rows = rows; F.J = J; F.Bi = Bi; F.f = f; F.G = G; F.G_stride = G_stride; F.a_ref = a_ref;
    for (int i = 0; i < rows * rows; ++i) { F.Kp[i] = Kp[i]; F.Kd[i] = Kd[i]; }
    if (nv <= 64) emu::launch(osot_force_gains_kernel<64>, (unsigned)B, 0, 64, F);
    else emu::launch(osot_force_gains_kernel<OSOT_MAX_QP_VARS>, (unsigned)B, 0, 64, F);
    return OSOT_OK;
}
