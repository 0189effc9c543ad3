#!/bin/sh
# builds the device probe of the wavefront primitives (test infrastructure only): tests/probe/team_probe.h against the
# product's opensot_amd/csrc/osot_team.h for gfx950 (cross-compiles without a GPU)
set -e
cd "$(dirname "$0")"
"${HIPCC:-/opt/rocm/bin/hipcc}" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -fvisibility=hidden \
    -I. -I../../opensot_amd/csrc team_probe.hip -o libosot_team_probe.so
