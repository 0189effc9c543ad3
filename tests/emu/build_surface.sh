#!/bin/sh
# builds the host lock-step emulation of the update kernel and the inverse-dynamics producers beyond 64 variables
# (tests/emu/surface_host.cpp; test infrastructure only)
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -DOSOT_EMULATION -fPIC -shared -fvisibility=hidden -Wl,-Bsymbolic -I. -I../../opensot_amd/csrc -I../../include \
    -Wno-unused-parameter surface_host.cpp -o libosot_surface_host.so
