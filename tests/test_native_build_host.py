"""tests/native_build.py: the staleness rule on files with set modification times (no compiler), the table, and -- for every
artifact the suite builds anyway -- that the compiler's depfile names what the hand-kept lists of the loaders named before it, and
the three inputs those lists had missed.  No GPU."""
import os

import pytest

import native_build as nb

CSRC, INC, EMU, PROBE = "opensot_amd/csrc/", "include/", "tests/emu/", "tests/probe/"

# the regression record: what each loader's own "is it stale?" list named before the lists went (its build script aside: the recipe
# is tests/native_build.py now, and is_stale() watches it for every artifact).  The emulator's loader had no list but a glob over
# opensot_amd/csrc/*.h, include/*.h and every file under tests/emu, the other libraries' sources included; what is recorded for it
# is the part of that glob its translation unit includes.
HAND_LISTS = {
    "emu": [CSRC + h for h in ("osot_admm.h", "osot_ehqp.h", "osot_host_plan.h", "osot_id.h", "osot_kernels.h", "osot_kin.h", "osot_nhqp.h",
                               "osot_nhqp_host.h", "osot_plan_shape.h", "osot_qp_core.h", "osot_qp_tol.h")]
           + [INC + "osot_mi355x.h", EMU + "emu_driver.cpp", EMU + "osot_team.h", EMU + "hip/hip_runtime.h"],
    "big_host": [CSRC + "osot_qp_big.h", CSRC + "osot_qp_tol.h", EMU + "big_host.cpp"],
    "big_hot_host": [CSRC + "osot_qp_big.h", CSRC + "osot_qp_tol.h", EMU + "big_hot_host.cpp"],
    "big_hot_asan": [CSRC + "osot_qp_big.h", CSRC + "osot_qp_tol.h", EMU + "big_hot_host.cpp"],
    "surface_host": [CSRC + "osot_kernels.h", CSRC + "osot_id.h", CSRC + "osot_host_plan.h", INC + "osot_mi355x.h", EMU + "surface_host.cpp"],
    "dyn_host": [CSRC + "osot_dyn.h", CSRC + "osot_kin.h", INC + "osot_mi355x.h", EMU + "dyn_host.cpp", EMU + "osot_team.h"],
    "grad_host": [CSRC + "osot_grad.h", CSRC + "osot_kin.h", INC + "osot_mi355x.h", EMU + "grad_host.cpp", EMU + "osot_team.h",
                  EMU + "hip/hip_runtime.h"],
    "wide_host": [CSRC + "osot_cascade_wide.h", CSRC + "osot_qp_big.h", CSRC + "osot_qp_tol.h", CSRC + "osot_plan_shape.h",
                  EMU + "cascade_wide_host.cpp"],
    "team_probe": [CSRC + "osot_team.h", PROBE + "team_probe.h", PROBE + "team_probe.hip"],
}
# what the hand lists had missed
GAPS = {"surface_host": CSRC + "osot_qp_core.h", "dyn_host": EMU + "hip/hip_runtime.h", "wide_host": INC + "osot_mi355x.h"}


# ---- the staleness rule ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def tree(tmp_path):
    """a build directory `b` with a source, an output and its depfile, a header outside it and a recipe: everything older (t = 100)
    than the output (t = 200).  -> (output, depfile, build_dir, recipe, {name: path}), and touch(path, t)"""
    b = tmp_path / "b"
    (tmp_path / "inc").mkdir()
    b.mkdir()
    files = {"src": b / "a.cpp", "hdr": tmp_path / "inc" / "a.h", "out": b / "liba.so", "dep": b / "liba.so.d", "recipe": tmp_path / "recipe.py"}
    for f in files.values():
        f.write_text("")
    files["dep"].write_text("liba.so.tmp.1: a.cpp \\\n ../inc/a.h\n")
    for name, f in files.items():
        os.utime(f, (100, 100))
    os.utime(files["out"], (200, 200))
    return files


def stale(files):
    return nb.is_stale(str(files["out"]), str(files["dep"]), str(files["out"].parent), str(files["recipe"]))


def test_fresh_output_is_not_stale(tree):
    assert not stale(tree)
    os.utime(tree["hdr"], (200, 200))        # as old as the output is not newer than it
    assert not stale(tree)


def test_missing_output_is_stale(tree):
    tree["out"].unlink()
    assert stale(tree)


def test_missing_depfile_is_stale(tree):
    tree["dep"].unlink()
    assert stale(tree)


@pytest.mark.parametrize("text", ["", "\n\n", "no rule here\n", "liba.so:\n", "\x00\x01\x02"])
def test_unparsable_depfile_is_stale(tree, text):
    tree["dep"].write_text(text)
    os.utime(tree["dep"], (100, 100))
    assert stale(tree)


@pytest.mark.parametrize("which", ["src", "hdr"])
def test_newer_dependency_is_stale(tree, which):
    os.utime(tree[which], (201, 201))
    assert stale(tree)


@pytest.mark.parametrize("which", ["src", "hdr"])
def test_missing_dependency_is_stale(tree, which):
    tree[which].unlink()
    assert stale(tree)


def test_newer_recipe_is_stale(tree):
    os.utime(tree["recipe"], (201, 201))
    assert stale(tree)


def test_depfile_continuations_and_relative_paths(tree, tmp_path):
    """backslash-continued lines, several rules, a name with an escaped space, an absolute path: relative names resolve against the
    build directory, wherever the process stands"""
    text = "liba.so.tmp.1: a.cpp \\\n ../inc/a.h \\\n  ../inc/../inc/b\\ c.h\nother.o: /abs/d.h\n"
    assert nb.parse_depfile(text) == ["a.cpp", "../inc/a.h", "../inc/../inc/b c.h", "/abs/d.h"]
    tree["dep"].write_text(text)
    got = nb.dependencies(str(tree["dep"]), str(tmp_path / "b"))
    assert got == [str(tmp_path / "b" / "a.cpp"), str(tmp_path / "inc" / "a.h"), str(tmp_path / "inc" / "b c.h"), "/abs/d.h"]


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def test_table_sources_exist_and_outputs_are_distinct():
    assert set(nb.ARTIFACTS) == set(HAND_LISTS)
    for name, a in nb.ARTIFACTS.items():
        assert os.path.isfile(os.path.join(nb.ROOT, a.dir, a.source)), name
    outputs = [nb.output_path(name) for name in nb.ARTIFACTS]
    assert len(set(outputs)) == len(outputs)


def test_command_adds_only_the_depfile_and_the_output_name():
    cmd = nb.command_line("dyn_host", "X")
    assert cmd[-6:] == ["dyn_host.cpp", "-MMD", "-MF", "libosot_dyn_host.so.d", "-o", "X"] and cmd[:-6] == nb.LOCKSTEP


# ---- the depfiles of the real artifacts ----------------------------------------------------------------------------------------------
def deps_of(name):
    out = nb.ensure(name)
    assert os.path.isfile(out) and not nb.is_stale(out, out + ".d", os.path.dirname(out))
    return {os.path.relpath(f, nb.ROOT) for f in nb.dependencies(out + ".d", os.path.dirname(out))}


@pytest.mark.parametrize("name", sorted(HAND_LISTS))
def test_depfile_covers_the_hand_list(name):
    deps = deps_of(name)
    assert not [f for f in HAND_LISTS[name] if f not in deps]
    assert name not in GAPS or GAPS[name] in deps
