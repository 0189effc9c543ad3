#!/bin/sh
# builds the host version of the wide iHQP cascade (opensot_amd/csrc/osot_cascade_wide.h; test infrastructure only)
set -e
cd "$(dirname "$0")"
g++ -O2 -g -std=c++17 -fPIC -shared -fvisibility=hidden -pthread -I../../opensot_amd/csrc -I../../include cascade_wide_host.cpp \
    -o libosot_wide_host.so
