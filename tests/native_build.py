"""tests/native_build.py -- TEST INFRASTRUCTURE ONLY: the one recipe and the one staleness rule of every native piece the suite
compiles for itself (the host builds of the kernel headers under tests/emu, the stand-alone sanitizer program, the device probe).

    ensure(name) -> path        build the artifact if it is stale
    load(name)   -> ctypes.CDLL ensure(), then one handle per name per process
    python tests/native_build.py [NAME ...]     ensure() the named artifacts (all of them without a name), printing each command

What an artifact depends on is what the compiler says it read (-MMD), never a list kept by hand; "the recipe changed" is this file
being newer than the output.  The flags are the ones the emulated results were recorded with: bit-identical results depend on them,
so they differ between entries on purpose (-O1 / -O2, -pthread, the statically linked sanitizer runtimes)."""
import collections
import ctypes
import os
import re
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = os.path.abspath(__file__)

INCLUDES = ["-I../../opensot_amd/csrc", "-I../../include"]
# the lock-step emulation: the kernel headers against tests/emu/hip/hip_runtime.h and the twin tests/emu/osot_team.h (-I.)
LOCKSTEP = ["g++", "-O1", "-g", "-std=c++17", "-DOSOT_EMULATION", "-fPIC", "-shared", "-fvisibility=hidden", "-Wl,-Bsymbolic", "-I."] \
    + INCLUDES + ["-Wno-unused-parameter"]
# a team of one thread: the same source the product runs as a 256-thread workgroup (-pthread where the file also has the
# turn-taking team of several threads)
TEAM_OF_ONE = ["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden"]

Artifact = collections.namedtuple("Artifact", "dir source output command")   # command: compiler and flags, run in `dir`


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


ARTIFACTS = {
    # the host lock-step emulation of the product kernels
    "emu": Artifact("tests/emu", "emu_driver.cpp", "libosot_emu.so", LOCKSTEP),
    # the update kernel and the inverse-dynamics producers beyond 64 variables
    "surface_host": Artifact("tests/emu", "surface_host.cpp", "libosot_surface_host.so", LOCKSTEP),
    # the rigid-body dynamics producer
    "dyn_host": Artifact("tests/emu", "dyn_host.cpp", "libosot_dyn_host.so", LOCKSTEP),
    # the posture-gradient producer
    "grad_host": Artifact("tests/emu", "grad_host.cpp", "libosot_grad_host.so", LOCKSTEP),
    # the wide-QP solver (opensot_amd/csrc/osot_qp_big.h)
    "big_host": Artifact("tests/emu", "big_host.cpp", "libosot_big_host.so", TEAM_OF_ONE + INCLUDES),
    # its HOT instantiation (big::solve<true>): the library the tests load ...
    "big_hot_host": Artifact("tests/emu", "big_hot_host.cpp", "libosot_big_hot_host.so", TEAM_OF_ONE + ["-pthread"] + INCLUDES),
    # ... and the same file as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, their runtimes linked
    # statically (a program of its own: no sanitizer is loaded into the interpreter, and the program starts in whatever
    # environment it is given)
    "big_hot_asan": Artifact("tests/emu", "big_hot_host.cpp", "big_hot_asan",
                             ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                              "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-pthread", "-DOSOT_BIG_HOT_MAIN"] + INCLUDES),
    # the wide iHQP cascade (opensot_amd/csrc/osot_cascade_wide.h)
    "wide_host": Artifact("tests/emu", "cascade_wide_host.cpp", "libosot_wide_host.so", TEAM_OF_ONE + ["-pthread"] + INCLUDES),
    # the device probe of the wavefront primitives: tests/probe/team_probe.h against the product's opensot_amd/csrc/osot_team.h
    # for gfx950 (cross-compiles without a GPU)
    "team_probe": Artifact("tests/probe", "team_probe.hip", "libosot_team_probe.so",
                           [_hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden",
                            "-I.", "-I../../opensot_amd/csrc"]),
}


def output_path(name):
    a = ARTIFACTS[name]
    return os.path.join(ROOT, a.dir, a.output)


def parse_depfile(text):
    """the prerequisites of every rule of a make-style depfile, in order (backslash-continued lines joined, "\\ " a space in a
    name); ValueError where the text holds no rule"""
    deps, rules = [], 0
    for line in text.replace("\\\n", " ").split("\n"):
        if not line.strip():
            continue
        m = re.match(r"^(.*?):(?:\s|$)(.*)$", line)
        if not m:
            raise ValueError(f"not a rule: {line[:80]!r}")
        rules += 1
        deps += [d.replace("\\ ", " ") for d in re.split(r"(?<!\\)\s+", m.group(2).strip()) if d]
    if not rules or not deps:
        raise ValueError("no rule with prerequisites")
    return deps


def dependencies(depfile, build_dir):
    """the files a depfile names, paths relative to the build directory resolved against it"""
    with open(depfile) as f:
        return [os.path.normpath(os.path.join(build_dir, d)) for d in parse_depfile(f.read())]


def is_stale(output, depfile, build_dir, recipe=RECIPE):
    """the one staleness rule, a function of paths and modification times alone: the output or its depfile is missing, the depfile
    cannot be read as one, a file it names is missing or newer than the output, or the recipe is newer than the output"""
    try:
        built = os.path.getmtime(output)
        return any(os.path.getmtime(f) > built for f in dependencies(depfile, build_dir) + [recipe])
    except (OSError, ValueError):
        return True


def command_line(name, output):
    """the compiler command of an artifact, writing `output` (a name in the build directory) and the depfile of the artifact"""
    a = ARTIFACTS[name]
    return [w() if callable(w) else w for w in a.command] + [a.source, "-MMD", "-MF", a.output + ".d", "-o", output]


def build(name):
    """compile to a temporary name beside the output, then move it there: another process never loads a half-written library"""
    a = ARTIFACTS[name]
    cwd = os.path.join(ROOT, a.dir)
    tmp = f"{a.output}.tmp.{os.getpid()}"
    cmd = command_line(name, tmp)
    print(shlex.join(cmd), flush=True)
    try:
        subprocess.check_call(cmd, cwd=cwd)
        os.replace(os.path.join(cwd, tmp), os.path.join(cwd, a.output))
    finally:
        if os.path.exists(os.path.join(cwd, tmp)):
            os.remove(os.path.join(cwd, tmp))
    return os.path.join(cwd, a.output)


def ensure(name):
    out = output_path(name)
    if is_stale(out, out + ".d", os.path.dirname(out)):
        build(name)
    return out


_loaded = {}


def load(name):
    if name not in _loaded:
        _loaded[name] = ctypes.CDLL(ensure(name))
    return _loaded[name]


if __name__ == "__main__":
    for name in sys.argv[1:] or ARTIFACTS:
        ensure(name)
