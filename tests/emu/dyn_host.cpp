// tests/emu/dyn_host.cpp -- TEST INFRASTRUCTURE ONLY.
// The rigid-body dynamics producer (opensot_amd/csrc/osot_dyn.h) through the host lock-step emulation of
// tests/emu/hip/hip_runtime.h, with the checks of osot_dyn_create / osot_dynamics (dyn_build, dyn_check_batch).  Built by
// tests/emu/build_dyn.sh; used by tests/test_dynamics_host.py (no GPU needed).  libosot_mi355x.so launches the same kernel body.
#include <osot_team.h>
#include "osot_dyn.h"

using namespace osot;

extern "C" __attribute__((visibility("default"))) int dyn_host_dynamics(const osot_kin_desc* tree, const osot_dyn_desc* inertia,
                                                                       const osot_dyn_batch* b) {
    static DevDyn h;
    const char* why = "";
    int rc = dyn_build(tree, inertia, h, &why);
    if (rc == OSOT_OK) rc = dyn_check_batch(h.k.d, b, &why);
    if (rc != OSOT_OK) { fprintf(stderr, "dyn host: %s\n", why); return rc; }
    if (b->B == 0) return OSOT_OK;
    emu::launch(osot_dyn_kernel<64>, (unsigned)b->B, 0, 64, (const DevDyn*)&h, *b, dyn_kin_batch(*b));
    return OSOT_OK;
}
