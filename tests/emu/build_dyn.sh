#!/bin/sh
# builds the host lock-step emulation of the rigid-body dynamics producer (tests/emu/dyn_host.cpp; test infrastructure only)
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -DOSOT_EMULATION -fPIC -shared -fvisibility=hidden -Wl,-Bsymbolic -I. -I../../opensot_amd/csrc -I../../include \
    -Wno-unused-parameter dyn_host.cpp -o libosot_dyn_host.so
