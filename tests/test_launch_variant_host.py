"""Which kernel an iHQP launch of the wavefront route runs: the host decision (opensot_amd/csrc/osot_host_plan.h:
choose_kernel_variant) over every combination of its inputs against a restatement of its rules written here, and the set of
variants osot_solver_create prepares (kernel_variants) against what the decision can return.  CPU only."""
import ctypes as C
import itertools

import pytest

from opensot_amd import abi
from helpers import emu_lib

CASCADE, CYCLE, CONTROL = 0, 1, 2
LAYOUTS = (32, 40, 56, 64)
BOOLS = ("fused", "control", "roll", "pairs_out", "prof", "plan_extra", "hotstart", "force_extra", "specialise", "rows_all_equalities")
PROF_REFUSAL = "phase profiling is not available for plans with dense weights or inactive tasks"
CONTROL_REFUSAL = "the fused control cycle carries no profiling code (use osot_kinematics + osot_cycle)"


def expected(T, nc, fused, control, roll, pairs_out, prof, plan_extra, hotstart, force_extra, specialise, rows_all_equalities):
    """the rules, in their order -> (code, message, (family, prof, extra, box, roll) or None)"""
    hot_on = hotstart and not prof                                                          # 1
    if prof and not fused and plan_extra:                                                   # 2
        return abi.ERR_UNSUPPORTED, PROF_REFUSAL, None
    extra = plan_extra or hot_on                                                            # 3
    if force_extra and not prof:
        extra = True
    box = specialise and not extra and (T == 32 if nc == 0 else (fused and rows_all_equalities))   # 4
    if pairs_out:                                                                           # 5
        box = False
    if control and (prof or not fused):                                                     # 6
        return abi.ERR_UNSUPPORTED, CONTROL_REFUSAL, None
    if control:                                                                             # 7
        v = (CONTROL, False, False, True, roll) if box else (CONTROL, False, True, False, roll) if extra else (CONTROL, False, False, False, roll)
    elif box and T == 32:
        v = (CYCLE, False, False, True, False) if fused else (CASCADE, prof, False, True, False)
    elif box and not prof:
        v = (CYCLE, False, False, True, False) if fused else (CASCADE, False, False, True, False)
    elif fused:
        v = (CYCLE, False, extra, False, False)
    elif prof:
        v = (CASCADE, True, False, False, False)
    elif extra:
        v = (CASCADE, False, True, False, False)
    else:
        v = (CASCADE, False, False, False, False)
    return abi.OK, "", v


def decide(T, nc, *flags):
    facts = (C.c_int * 12)(T, nc, *[int(f) for f in flags])
    out = (C.c_int * 5)()
    why = C.c_char_p()
    rc = emu_lib().emu_choose_kernel_variant(facts, out, C.byref(why))
    v = (out[0], bool(out[1]), bool(out[2]), bool(out[3]), bool(out[4]))
    return rc, why.value.decode(), (v if rc == abi.OK else None)


@pytest.fixture(scope="module")
def decisions():
    """{(T, nc, flags...): (code, message, variant)} over every combination of the inputs"""
    return {(T, nc) + flags: decide(T, nc, *flags)
            for T in LAYOUTS for nc in (0, 3) for flags in itertools.product((False, True), repeat=len(BOOLS))}


def test_every_input_gives_the_variant_the_rules_give(decisions):
    assert len(decisions) == 4 * 2 * 2 ** len(BOOLS)
    for key, got in decisions.items():
        assert got == expected(*key), dict(zip(("T", "nc") + BOOLS, key))
        if got[2] is not None:
            family, prof, extra, box, roll = got[2]
            assert not (box and extra)
            assert not (family == CASCADE and prof and extra)
            assert not (family == CONTROL and prof)
            assert family == CONTROL or not roll        # only the control cycle has a rollout instantiation
            assert family == CASCADE or not prof        # ... and only the cascade an instrumented one


def test_creation_prepares_what_a_launch_can_select(decisions):
    # prepared today, never selected: BOX without the update half needs a plan without constraint rows at T = 32 (rule 4), so the solve-only
    # BOX cascade of the wider layouts is reached by no launch (the host emulation runs it: tests/test_emulated_kernels.py)
    never_selected = {T: {(CASCADE, False, False, True, False)} if T != 32 else set() for T in LAYOUTS}
    for T in LAYOUTS:
        buf = (C.c_int * (5 * 14))()
        n = emu_lib().emu_kernel_variants(T, buf)
        prepared = [(buf[5 * i], bool(buf[5 * i + 1]), bool(buf[5 * i + 2]), bool(buf[5 * i + 3]), bool(buf[5 * i + 4])) for i in range(n)]
        assert n == (14 if T == 32 else 13) and len(set(prepared)) == n
        selected = {v for key, (rc, _, v) in decisions.items() if key[0] == T and rc == abi.OK}
        assert not (selected & never_selected[T])
        assert set(prepared) == selected | never_selected[T]
