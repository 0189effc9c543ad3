"""opensot_amd/csrc/osot_convex.h under AddressSanitizer and UndefinedBehaviorSanitizer: tools/convex_fuzz.cpp is a program of its own
(its own main, the sanitizer runtimes linked into it), built with the host compiler and run as a child process over 1e5 random and
degenerate pairs of cores.  Nothing is loaded into the interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_convex_fuzz_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "convex_fuzz")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",      # (static runtimes: the program
                           # starts in whatever environment it is given, like tests/native_build.py's big_hot_asan)
                           "-I" + os.path.join(ROOT, "opensot_amd", "csrc"), os.path.join(ROOT, "tools", "convex_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe, "100000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "100000 pairs" in r.stdout and " 0 failures" in r.stdout
