#!/bin/sh
# builds the host version of the wide-QP solver's HOT instantiation (opensot_amd/csrc/osot_qp_big.h, big::solve<true>; test
# infrastructure only).  "lib": the library the tests load.  "asan": the same file as a stand-alone program under AddressSanitizer and
# UndefinedBehaviorSanitizer, their runtimes linked statically (a program of its own: no sanitizer is loaded into the interpreter,
# and the program starts in whatever environment it is given).  No argument: both.
set -e
cd "$(dirname "$0")"
what="${1:-both}"
if [ "$what" = lib ] || [ "$what" = both ]; then
    g++ -O2 -g -std=c++17 -fPIC -shared -fvisibility=hidden -pthread -I../../opensot_amd/csrc -I../../include big_hot_host.cpp \
        -o libosot_big_hot_host.so
fi
if [ "$what" = asan ] || [ "$what" = both ]; then
    g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -static-libasan -static-libubsan \
        -pthread -DOSOT_BIG_HOT_MAIN -I../../opensot_amd/csrc -I../../include big_hot_host.cpp -o big_hot_asan
fi
