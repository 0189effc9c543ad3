"""Hot start of the working sets on the wide route, CPU side: cascade_instance<true> of opensot_amd/csrc/osot_cascade_wide.h (what
osot_ihqp_solve_hot / osot_cycle_hot run) compiled for the host (tests/emu/cascade_wide_hot_host.cpp, tests/wide_hot_ref.py) against
the cold build of the same source, against the oracle, under foreign lists, level / task switches and a failing level, with a team
of four threads against the team of one, and as a stand-alone program under ASan + UBSan."""
import functools

import numpy as np
import pytest

from opensot_amd import synth
from oracle import pyoracle

import test_surface_contact_host as surf
from test_wide_plan_host import close, generic_wide, oracle_solve, wide_host
from wide_hot_ref import HOT_LEN, drifted, new_state, run_sanitizer_program, scaled_diff, tight_stack, wide_host_hot

# Worst scaled |dq_hot - dq_cold| over every fixture, cycle and list content of this file (test_hot_against_cold_* print theirs), host
# build, g++ -O2: 2.0e-11, the 68-variable surface stack from a list of random codes (every other foreign list and fixture at most
# 3.3e-13; the chains of a repeat and three drifted cycles at most 9.4e-14, the tight 72-variable stack; the level / task switches 2.8e-17).
HOT_VS_COLD_MEASURED = 2.0e-11
HOT_VS_COLD = min(100 * HOT_VS_COLD_MEASURED, 1e-8)
# Worst residual |a'x - bound| / max(1, |bound|) of a recorded constraint at its level's solution (test_cold_lists_...): 2.0e-13
# (the 68-variable surface stack; the generic stacks 3.7e-15 and below)
ACTIVE_RESIDUAL_MEASURED = 2.0e-13
ACTIVE_RESIDUAL = min(100 * ACTIVE_RESIDUAL_MEASURED, 1e-8)

FIXTURES = ["surface68", "surface86", "tight72", "generic65", "generic80", "generic128", "robot80", "generic20"]
FEWER = ("surface68", "surface86", "tight72")     # strictly fewer iterations on every instance of an exact repeat


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(plan, asm) of a fixture, assembled once"""
    if name.startswith("surface"):
        n = int(name[7:])
        plan, leaf = surf.stack(6, n, n + 1)
        return plan, surf._assembled(plan, leaf)
    if name == "tight72":
        plan, leaf = tight_stack(4)
    elif name == "robot80":
        plan, leaf = synth.make_wide_robot_stack(8, 80, seed=1)
    elif name == "generic20":      # 2 (n + nc) < 128: the list-staging branch where thread 0 reads global memory
        plan, leaf = generic_wide(8, 20, seed=3, level_rows=[4, 6], n_eq=2, n_ineq=6, n_local=2)
        assert 2 * (plan.n + plan.nc) < HOT_LEN
    else:
        n = int(name[7:])
        plan, leaf = generic_wide(8, n, seed=n)
    return plan, pyoracle.assemble(plan, leaf)


@functools.lru_cache(maxsize=None)
def cold(name, cycle=0):
    plan, asm = fixture(name)
    return wide_host(plan, drifted(asm, cycle))


@functools.lru_cache(maxsize=None)
def chain(name):
    """the fixture solved hot five times on one state: from empty lists, an exact repeat, three cycles under 1 % drift
    -> [(result, state after it)]"""
    plan, asm = fixture(name)
    state = new_state(asm["B"], asm["L"])
    out = []
    for cycle in (0, 0, 1, 2, 3):
        res = wide_host_hot(plan, drifted(asm, cycle), state)
        out.append((res, state.copy()))
    return out


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def row_level(plan):
    """per constraint row: the level it belongs to (task-local rows), or -1 (global rows)"""
    lev = []
    for rb in plan.rowblocks:
        lev += [-1 if rb.level is None else rb.level] * rb.rows
    return np.array(lev, dtype=int)


# ---- 1. empty lists: the cold result, bit for bit; what is recorded is a valid working set ------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_cold_lists_give_the_cold_bits_and_record_active_inequalities(name):
    plan, asm = fixture(name)
    (res, state), c = chain(name)[0], cold(name)
    assert same_bits(res, c)                     # dq, x_levels, status, iterations, accepted_slack
    n, nc, L, B = plan.n, plan.nc, plan.L, asm["B"]
    lev = row_level(plan)
    worst, count = 0.0, 0
    for i in range(B):
        for k in range(L):
            lst = state[i, k * HOT_LEN:(k + 1) * HOT_LEN]
            cnt = int((lst >= 0).sum())
            assert (lst[:cnt] >= 0).all() and (lst[cnt:] == -1).all()            # compacted to the front
            assert len(set(lst[:cnt].tolist())) == cnt
            x = res[1][i, k]
            for enc in lst[:cnt]:
                code, upper = int(enc) >> 1, int(enc) & 1
                assert code < n + nc + sum(plan.m(j) for j in range(k))
                if code < n:
                    lo, up, ax = asm["l"][i, code], asm["u"][i, code], x[code]
                else:
                    r = code - n
                    assert r < nc, "an optimality row is an equality: never recorded"
                    assert lev[r] in (-1, k), "a task-local row of another level has no bounds at this one"
                    lo, up, ax = asm["lo"][i, r], asm["up"][i, r], asm["C"][i, r] @ x
                assert lo != up
                bound = up if upper else lo
                assert abs(bound) < 1e20
                worst = max(worst, abs(ax - bound) / max(1.0, abs(bound)))
                count += 1
    print(f"{name}: {count} recorded constraints, worst residual {worst:.3g}")
    assert worst <= ACTIVE_RESIDUAL
    if name != "robot80":
        assert count > 0


# ---- 2. exact repeat ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_exact_repeat_never_takes_more_iterations(name):
    (res, _), c = chain(name)[1], cold(name)
    print(f"{name}: cold {c[3].tolist()} hot {res[3].tolist()}")
    assert (res[2] == 0).all() and (res[4] == c[4]).all()
    assert (res[3] <= c[3]).all()
    if name in FEWER:
        assert (res[3] < c[3]).all()


# ---- 3. against the oracle: the repeat and three chained cycles under drift ---------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_hot_answers_pass_the_cold_tests_checks(name):
    plan, asm = fixture(name)
    for step, cycle in ((1, 0), (2, 1), (3, 2), (4, 3)):
        (dq, xl, st, it, slack), _ = chain(name)[step]
        a = drifted(asm, cycle)
        assert (st == 0).all()
        if name.startswith("surface"):
            surf._judge(a, dq, st)
            assert (slack <= 1e-7).all()
        elif name == "tight72":        # (the eiQuadProg restatement stops on this stack; the reference's qpOASES solves it)
            if pyoracle.ref_available():
                rq = pyoracle.ihqp_solve_batch(a, pyoracle.BE_QPOASES_REF, nthreads=1)
                assert (rq["status"] == 1).all() and close(dq, rq["dq"], 1e-9)
            else:
                print(f"{name}: the reference's qpOASES build is absent -- this stack's hot answers are judged against cold alone")
        else:
            ref = oracle_solve(a)
            assert (ref["status"] == 1).all()
            assert close(dq, ref["dq"]) and close(xl, ref["x_levels"])


# ---- 4. hot against cold on the same inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_hot_against_cold_over_the_chain(name):
    worst = 0.0
    its = []
    for step, cycle in ((1, 0), (2, 1), (3, 2), (4, 3)):
        (res, _), c = chain(name)[step], cold(name, cycle)
        assert np.array_equal(res[2], c[2]) and (res[2] == 0).all()
        worst = max(worst, scaled_diff(res[0], c[0]), scaled_diff(res[1], c[1]))
        its.append((int(c[3].max()), int(res[3].max())))
    print(f"{name}: worst scaled |hot - cold| {worst:.3g}; (cold max, hot max) iterations per cycle {its}")
    assert worst <= HOT_VS_COLD


# ---- 5. foreign lists -----------------------------------------------------------------------------------------------------------------
def foreign_lists(name):
    plan, asm = fixture(name)
    n, nc, L, B = plan.n, plan.nc, plan.L, asm["B"]
    rng = np.random.default_rng(5)
    shape = (B, L * HOT_LEN)
    lists = {"random": rng.integers(-(n + nc), 4 * (n + nc), size=shape),
             "extreme": rng.choice(np.array([-2 ** 31, -2 ** 31 + 1, 2 ** 31 - 1, 2 ** 31 - 2, -2, 2 * (n + nc), 2 * (n + nc) + 1]), size=shape),
             "every lower bound": np.tile(2 * np.arange(HOT_LEN), (B, L))}
    other = chain("generic128" if name != "generic128" else "surface68")[1][1]
    lists["another plan's state"] = np.resize(other, shape)
    lo, up = asm["lo"], asm["up"]
    dup, eq, inf = np.full(shape, -1), np.full(shape, -1), np.full(shape, -1)
    for i in range(B):
        ineq = np.nonzero((lo[i] != up[i]) & (up[i] < 1e20))[0]
        if len(ineq):
            dup[i] = 2 * (n + ineq[i % len(ineq)]) + 1
        # equalities: the rows with lo == up, then the optimality rows of the levels above (positions behind the constraint rows)
        e = [2 * (n + r) + s for r in np.nonzero(lo[i] == up[i])[0] for s in (0, 1)] + [2 * (n + nc + q) for q in range(plan.m(0))]
        eq[i] = np.resize(np.array(e), shape[1])
        f = [2 * (n + r) for r in np.nonzero(lo[i] <= -1e20)[0]] + [2 * (n + r) + 1 for r in np.nonzero(up[i] >= 1e20)[0]]
        if asm["l"] is not None:
            f += [2 * c for c in np.nonzero(asm["l"][i] <= -1e20)[0]] + [2 * c + 1 for c in np.nonzero(asm["u"][i] >= 1e20)[0]]
        if f:
            inf[i] = np.resize(np.array(f), shape[1])
    lists["duplicates"], lists["equality rows"], lists["infinite sides"] = dup, eq, inf
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in lists.items()}


@pytest.mark.parametrize("name", FIXTURES)
def test_foreign_lists_give_the_cold_answer(name):
    plan, asm = fixture(name)
    c = cold(name)
    worst = 0.0
    for what, state in foreign_lists(name).items():
        res = wide_host_hot(plan, asm, state)
        assert (res[2] == 0).all(), what
        d = max(scaled_diff(res[0], c[0]), scaled_diff(res[1], c[1]))
        worst = max(worst, d)
        assert d <= HOT_VS_COLD, (what, d)
        assert ((state >= -1) & ((state >> 1) < plan.n + plan.nc)).all(), what      # what was recorded over the garbage is a list
    print(f"{name}: worst scaled |hot - cold| over foreign lists {worst:.3g}")


def test_foreign_lists_in_the_sanitizer_program():
    """the same kinds of lists on two plans the program builds itself (70 variables; 20 variables with the unstaged tail), under
    AddressSanitizer and UndefinedBehaviorSanitizer, as a child process: exit status 0 = no report and every answer the cold one"""
    r = run_sanitizer_program()
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "another plan's state" in r.stdout and "n = 20" in r.stdout and "n = 70" in r.stdout


# ---- 6. switches between cycles -------------------------------------------------------------------------------------------------------
def test_level_and_task_switches_between_cycles():
    B, n = 3, 80
    plan, leaf = synth.make_generic_stack(B, n, [10, 8, 14], n_ineq=20, unit_box=(None, 0.6), seed=3 * n)
    from opensot_amd import abi
    plan.levels[1].append(synth.Task(abi.TASK_GENERIC, 5, name="extra"))
    leaf["A"][1] = np.concatenate([leaf["A"][1], np.random.default_rng(1).normal(0, 0.4, size=(B, 5, n))], axis=1)
    leaf["task"][1].append((np.random.default_rng(2).normal(0, 0.05, size=(B, 5)), None, None))
    off = {(1, 1): False}
    asm_on, asm_off = pyoracle.assemble(plan, leaf), pyoracle.assemble(plan, leaf, task_active=off)
    all_on, no1 = [True] * 4, [True, False, True, True]
    state = new_state(B, plan.L)
    worst = 0.0
    lvl1 = slice(HOT_LEN, 2 * HOT_LEN)
    for asm, act, ta in ((asm_on, all_on, None), (asm_off, no1, off), (asm_off, all_on, off), (asm_on, all_on, None)):
        before = state.copy()
        res = wide_host_hot(plan, asm, state, active=act, task_active=ta)
        c = wide_host(plan, asm, active=act, task_active=ta)
        assert (res[2] == 0).all() and (c[2] == 0).all()
        worst = max(worst, scaled_diff(res[0], c[0]))
        for k in range(4):
            if act[k]:
                worst = max(worst, scaled_diff(res[1][:, k], c[1][:, k]))
        if not act[1]:
            assert (before[:, lvl1] >= 0).any()                                 # (there is something to lose)
            assert before[:, lvl1].tobytes() == state[:, lvl1].tobytes()
    print(f"switches: worst scaled |hot - cold| {worst:.3g}")
    assert worst <= HOT_VS_COLD


# ---- 7. a failing instance ------------------------------------------------------------------------------------------------------------
def test_failing_level_clears_its_list_and_leaves_the_lower_ones():
    plan, asm = fixture("generic80")
    B, L = asm["B"], asm["L"]
    state = new_state(B, L)
    wide_host_hot(plan, asm, state)
    recorded = state.copy()
    assert all((recorded[:, k * HOT_LEN:(k + 1) * HOT_LEN] >= 0).any() for k in range(L))
    # level 0 infeasible: two copies of one row, asked to be +1 and -1
    lo, up = asm["lo"], asm["up"]
    r0, r1 = [int(r) for r in np.nonzero((lo[0] != up[0]) & (row_level(plan) == -1))[0][:2]]
    bad = dict(asm)
    bad["C"], bad["lo"], bad["up"] = asm["C"].copy(), lo.copy(), up.copy()
    bad["C"][:, r1] = bad["C"][:, r0]
    bad["lo"][:, r0] = bad["up"][:, r0] = 1.0
    bad["lo"][:, r1] = bad["up"][:, r1] = -1.0
    res = wide_host_hot(plan, bad, state)
    c = wide_host(plan, bad)
    assert (c[2] == 1).all() and np.array_equal(res[2], c[2])                   # INFEASIBLE: level 0's status
    assert (res[0] == 0).all()
    assert (state[:, :HOT_LEN] == -1).all()
    assert state[:, HOT_LEN:].tobytes() == recorded[:, HOT_LEN:].tobytes()
    # the next cycle, feasible again
    res = wide_host_hot(plan, asm, state)
    c = cold("generic80")
    assert (res[2] == 0).all()
    assert max(scaled_diff(res[0], c[0]), scaled_diff(res[1], c[1])) <= HOT_VS_COLD


# ---- 8. a team of four threads against the team of one --------------------------------------------------------------------------------
@pytest.mark.parametrize("t0_last", [False, True])
def test_hot_team_of_four_equals_team_of_one_state_included(t0_last):
    plan, leaf = tight_stack(2)
    asm = pyoracle.assemble(plan, leaf)
    one_state, four_state = new_state(2, plan.L), new_state(2, plan.L)
    for cycle in (0, 1):
        a = drifted(asm, cycle)
        one = wide_host_hot(plan, a, one_state)
        four = wide_host_hot(plan, a, four_state, nthreads=4, t0_last=t0_last)
        assert (one[2] == 0).all()
        assert same_bits(one, four)
        assert one_state.tobytes() == four_state.tobytes()
    c = wide_host(plan, drifted(asm, 1))
    assert (one[3] < c[3]).all()            # (the hot phase did something: it added, and under drift it removed)
