#!/bin/sh
# builds the host lock-step emulation of the posture-gradient producer (tests/emu/grad_host.cpp; test infrastructure only)
set -e
cd "$(dirname "$0")"
g++ -O1 -g -std=c++17 -DOSOT_EMULATION -fPIC -shared -fvisibility=hidden -Wl,-Bsymbolic -I. -I../../opensot_amd/csrc -I../../include \
    -Wno-unused-parameter grad_host.cpp -o libosot_grad_host.so
