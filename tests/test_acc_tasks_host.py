"""The acceleration-leaf producer (opensot_amd/csrc/osot_acc.h: osot_acc_tasks) through the host lock-step emulation: no GPU needed.

What is bit-exact (single float64 operations, copies, the orientation error with contraction off) is compared bit for bit with the
numpy restatement of tests/acc_ref.py; fma chains against the forward-error bound of their sum; everything that comes out of the
Cholesky factor against the numpy.longdouble arbiter in units of cond2(M) max|X*| (acc_ref.CHOLESKY_TOL)."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from opensot_amd import abi
import acc_ref as ar
from acc_ref import ACC, FORCE, SENTINEL

WITH_M = [n for n in ar.CASES if ar.CASES[n]["M"] is not None]


@functools.lru_cache(maxsize=None)
def solved(name):
    """(case, emulated Outputs, float64 restatement, longdouble arbiter) of a named case: computed once, never modified"""
    case = ar.named_case(name)
    return case, ar.run_host(case), ar.restate(case), ar.restate(case, np.longdouble)


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


# ---- 1. bit-exact ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ar.CASES))
def test_differences_orientation_error_and_copies_are_bit_exact(name):
    case, out, ref, _ = solved(name)
    B, nv = case["B"], case["nv"]
    for t, term in enumerate(case["cart"]):
        p0 = out.p0(t)
        assert np.array_equal(p0[:, 0:6], ref["cart"][t]["pose_err"]), (name, t)
        if term["gain_type"] == ACC and term["gain_matrices"]:
            assert np.array_equal(p0[:, 12:48], np.broadcast_to(term["Kp"].reshape(36), (B, 36)))
            assert np.array_equal(p0[:, 48:84], np.broadcast_to(term["Kd"].reshape(36), (B, 36)))
        if term["gain_type"] == ACC or term["f_virtual"] is None:
            assert np.array_equal(out.a_ref_out(t), np.zeros((B, 6)) if term["a_ref_in"] is None else term["a_ref_in"])
    if case["com"] is not None:
        assert np.array_equal(out.com()[:, 0:3], ref["com"]["err"])
        if case["com"]["gain_matrices"]:
            assert np.array_equal(out.com()[:, 6:15], np.broadcast_to(case["com"]["Kp"].reshape(9), (B, 9)))
            assert np.array_equal(out.com()[:, 15:24], np.broadcast_to(case["com"]["Kd"].reshape(9), (B, 9)))
    if case["post"] is not None:
        assert np.array_equal(out.post(nv)[:, :nv], ref["post"]["pe"])
        assert np.array_equal(out.post(nv)[:, nv:], ref["post"]["ve"])
    assert np.all(out.ok[1:-1] == 1)


# ---- 2. fma chains within the forward-error bound of their sum -------------------------------------------------------------------------
def _vel_err_terms(J, qdot, vel_ref):
    """vel_ref - J qdot: the terms of row r, each [B][rows]"""
    terms = [] if vel_ref is None else [_ld(vel_ref)]
    return terms + [-_ld(J[:, :, k]) * _ld(qdot[:, k])[:, None] for k in range(qdot.shape[1])]


@pytest.mark.parametrize("name", list(ar.CASES))
def test_velocity_errors_and_postural_gain_products_within_the_bound_of_the_sum(name):
    case, out, _, _ = solved(name)
    nv = case["nv"]
    for t, term in enumerate(case["cart"]):
        want, bound = ar.value_and_bound(_vel_err_terms(term["J"][:, 1:7, :nv], case["qdot"], term["vel_ref"]))
        assert np.all(np.abs(_ld(out.p0(t)[:, 6:12]) - want) <= bound), (name, t)
    if case["com"] is not None:
        k = case["com"]
        want, bound = ar.value_and_bound(_vel_err_terms(k["J"][:, 1:4, :nv], case["qdot"], k["vel_ref"]))
        assert np.all(np.abs(_ld(out.com()[:, 3:6]) - want) <= bound), name
    p = case["post"]
    if p is not None and p["gain_type"] == ACC:
        # qddot_out = qddot_ref + lambda2 Kd vel_err + lambda Kp pos_err, the errors as the kernel wrote them
        pe, ve = _ld(out.post(nv)[:, :nv]), _ld(out.post(nv)[:, nv:])
        Kp = np.eye(nv) if p["Kp"] is None else p["Kp"]
        Kd = np.eye(nv) if p["Kd"] is None else p["Kd"]
        terms = [np.longdouble(p["lam"]) * _ld(Kp[:, j])[None, :] * pe[:, j:j + 1] for j in range(nv)]
        terms += [np.longdouble(p["lam2"]) * _ld(Kd[:, j])[None, :] * ve[:, j:j + 1] for j in range(nv)]
        if p["qddot_ref"] is not None:
            terms.append(_ld(p["qddot_ref"]))
        want, bound = ar.value_and_bound(terms)
        assert np.all(np.abs(_ld(out.qddot(nv)) - want) <= bound), name


# ---- 3. everything out of the Cholesky factor against the arbiter ------------------------------------------------------------------------
def test_the_tolerance_is_ten_times_the_restatements_own_worst_figure():
    worst = max(ar.worst_deviation(solved(n)[0], solved(n)[2], solved(n)[3]) for n in WITH_M)
    print("restatement, worst of the cases:", worst)
    assert worst[0] <= ar.RESTATEMENT_WORST <= 1e3 * 2.2e-16
    assert ar.CHOLESKY_TOL == 10.0 * ar.RESTATEMENT_WORST


@pytest.mark.parametrize("name", WITH_M)
def test_cholesky_outputs_against_the_longdouble_arbiter(name):
    case, out, _, arb = solved(name)
    nv = case["nv"]
    worst = ar.worst_deviation(case, out, arb)
    print(name, "emulated kernel:", worst)
    assert worst[0] <= ar.CHOLESKY_TOL, worst
    assert worst[0] <= ar.EMULATED_WORST, "acc_ref.EMULATED_WORST is out of date"
    for t, term in enumerate(case["cart"]):
        if term["gain_type"] == FORCE:
            assert np.array_equal(out.Mi(t), np.transpose(out.Mi(t), (0, 2, 1)))
    if case["minv"]:
        Mi = out.minv(nv)
        assert np.array_equal(Mi, np.transpose(Mi, (0, 2, 1)))
        for i in range(case["B"]):
            res = np.max(np.abs(_ld(case["M"][i]) @ _ld(Mi[i]) - np.eye(nv))) / np.linalg.cond(case["M"][i])
            print(name, i, "max|M Minv - I| / cond2(M) =", float(res))
            assert res <= ar.CHOLESKY_TOL, (name, i, float(res))


# ---- 4. identities that do not depend on the restatement -------------------------------------------------------------------------------
def test_force_type_Mi_equals_the_force_gains_entry_fed_the_numpy_inverse():
    import surface_ref
    case, out, _, _ = solved("nv35")
    B, nv = case["B"], case["nv"]
    t = next(i for i, term in enumerate(case["cart"]) if term["gain_type"] == FORCE)
    J = np.ascontiguousarray(case["cart"][t]["J"][:, 1:7, :nv])
    Bi = np.ascontiguousarray(np.linalg.inv(case["M"]))
    eye, G = np.eye(6), np.zeros((B, 72))
    assert surface_ref.surface_lib().surf_force_gains(B, nv, 6, J.ctypes.data, Bi.ctypes.data, eye.ctypes.data, eye.ctypes.data, None,
                                              G.ctypes.data, 72, None) == abi.OK
    for i in range(B):
        dev = np.max(np.abs(out.Mi(t)[i] - G[i, :36].reshape(6, 6))) / (np.linalg.cond(case["M"][i]) * np.max(np.abs(G[i, :36])))
        assert dev <= ar.CHOLESKY_TOL, (i, dev)


def test_acceleration_type_Gp_of_identity_gains_is_exactly_the_identity():
    case = ar.make_case(3, 7, cart=[(ACC, 1)])
    case["cart"][0]["Kp"], case["cart"][0]["Kd"] = np.eye(6), np.eye(6)
    out = ar.run_host(case)
    assert np.array_equal(out.p0(0)[:, 12:48], np.broadcast_to(np.eye(6).reshape(36), (3, 36)))
    assert np.array_equal(out.p0(0)[:, 48:84], np.broadcast_to(np.eye(6).reshape(36), (3, 36)))


# ---- 5. nothing else is written --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ar.CASES))
def test_sentinels_around_every_output_survive_and_nothing_unread_is_read(name):
    case, out, _, _ = solved(name)
    assert out.fences_intact()
    # (NaN sits in columns nv .. ld-1 of every Jacobian row and above the diagonal of M: nothing that was written may hold one)
    for a in out.arrays():
        assert not np.any(np.isnan(a.astype(float)))
    nv = case["nv"]
    for t, term in enumerate(case["cart"]):
        assert not np.any(out.p0(t) == SENTINEL)
        assert np.all(out.cart_Mi[t] == SENTINEL) == (term["gain_type"] != FORCE)
    if case["post"] is not None:
        assert not np.any(out.post(nv) == SENTINEL) and not np.any(out.qddot(nv) == SENTINEL)
    assert np.all(out.Minv == SENTINEL) == (not case["minv"])


@pytest.mark.parametrize("left_out", [w for w in ar.Outputs.ALL if w != "cart_p0"])
def test_an_output_left_null_is_not_touched_and_the_others_do_not_change(left_out):
    case, full, _, _ = solved("nv35")
    want = tuple(w for w in ar.Outputs.ALL if w != left_out)
    if left_out == "cart_a_ref_out":
        case = dict(case, cart=[dict(t, f_virtual=None, a_ref_in=None) for t in case["cart"]])   # its inputs go with it
    out = ar.run_host(case, want)
    names = ["com_p0", "post_p0", "post_qddot_out", "Minv", "ok"] + ["cart_p0"] * 3 + ["cart_a_ref_out"] * 3 + ["cart_Mi"] * 3
    for a, b, name in zip(out.arrays(), full.arrays(), names):
        if name == left_out:
            assert np.all(a == (SENTINEL if name != "ok" else -7)), name
        else:
            assert np.array_equal(a, b), (left_out, name)


def test_p0_left_null():
    case, full, _, _ = solved("nv35")
    out = ar.run_host(case, tuple(w for w in ar.Outputs.ALL if w != "cart_p0"))
    assert all(np.all(a == SENTINEL) for a in out.cart_p0)
    assert all(np.array_equal(a, b) for a, b in zip(out.cart_Mi + out.cart_a_ref_out + [out.Minv], full.cart_Mi + full.cart_a_ref_out + [full.Minv]))


# ---- 6. a failed pivot -------------------------------------------------------------------------------------------------------------------
def test_a_failed_pivot_zeroes_the_force_outputs_of_its_instance_only():
    case = ar.singular_case(solved("nv35")[0])
    ar.check_failed_pivot(ar.run_host(case), solved("nv35")[1], case)


def test_pivot_threshold_is_the_headers():
    for nv in (1, 7, 64):
        assert ar.lib().acc_host_pivot_rel(nv) == ar.pivot_rel(nv) == (nv + 1) * 2.0 ** -52


# ---- 7. every refusal ----------------------------------------------------------------------------------------------------------------------
def _structs(case, want=ar.Outputs.ALL):
    out, keep = ar.Outputs(case, want), []
    m, b = ar.structs(case, out, lambda a: a.ctypes.data, keep)
    return m, b, (out, keep)


def _set(obj, field, value, index=None):
    if index is None:
        setattr(obj, field, value)
    else:
        getattr(obj, field)[index] = value


NAN = float("nan")
REFUSALS = [
    # (struct, field, index, value, the words the reason must hold)
    ("m", "nv", None, 0, "nv"), ("m", "n_cart", None, 9, "n_cart"), ("m", "n_cart", None, -1, "n_cart"), ("b", "B", None, -1, "B"),
    ("m", "cart_gain_type", 1, 2, "cart_gain_type"), ("m", "post_gain_type", None, 7, "post_gain_type"),
    ("m", "cart_gain_matrices", 0, 3, "cart_gain_matrices"), ("m", "has_com", None, 2, "has_com"),
    ("m", "cart_Kp", 40, NAN, "cart_Kp"), ("m", "cart_Kd", 3, float("inf"), "cart_Kd"), ("m", "cart_orientation_gain", 2, NAN, "cart_orientation_gain"),
    ("m", "com_Kp", 4, NAN, "com_Kp"), ("m", "com_Kd", 0, NAN, "com_Kd"), ("m", "post_lambda", None, NAN, "post_lambda"),
    ("m", "post_lambda2", None, float("-inf"), "post_lambda2"),
    ("b", "M", None, None, "M is null"), ("b", "M_stride", None, 35 * 35 - 1, "M_stride"),
    ("b", "qdot", None, None, "qdot"), ("b", "q", None, None, "q is null"),
    ("b", "cart_J", 1, None, "cart_J"), ("b", "cart_pose", 0, None, "cart_pose"), ("b", "cart_pose_ref", 2, None, "cart_pose_ref"),
    ("b", "cart_J_ld", 1, 34, "cart_J_ld"), ("b", "cart_J_stride", 2, 6 * 48 - 1, "cart_J_stride"),
    ("b", "cart_p0_stride", 0, 11, "cart_p0_stride"), ("b", "cart_p0_stride", 1, 83, "cart_p0_stride"),
    ("b", "com_J", None, None, "com_J"), ("b", "com_J_ld", None, 34, "com_J_ld"), ("b", "com_J_stride", None, 3 * 48 - 1, "com_J_stride"),
    ("b", "com_p0_stride", None, 23, "com_p0_stride"), ("b", "post_q_ref", None, None, "post_q_ref"),
    ("b", "Minv_stride", None, 35 * 35 - 1, "Minv_stride"),
]


@pytest.mark.parametrize("which,field,index,value,words", REFUSALS)
def test_refusals_name_the_field(which, field, index, value, words):
    m, b, keep = _structs(solved("nv35")[0])
    assert ar.host_check(m, b) == (abi.OK, "")
    _set(m if which == "m" else b, field, value, index)
    rc, why = ar.host_check(m, b)
    assert rc == abi.ERR_INVALID and words in why, (rc, why)


def test_refusals_of_aliases_and_of_pointers_without_their_term():
    case = solved("nv35")[0]
    get = lambda b, field, index: getattr(b, field) if index is None else getattr(b, field)[index]
    # (output or unowned slot, its index, the pointer it is given: field, index, the words of the reason)
    alias = [("cart_a_ref_out", 1, "cart_a_ref_in", 1, "aliases"), ("cart_p0", 0, "cart_pose", 0, "aliases"), ("cart_Mi", 1, "cart_J", 1, "aliases"),
             ("com_p0", None, "com", None, "com_p0 aliases"), ("post_p0", None, "q", None, "aliases"),
             ("post_qddot_out", None, "post_qddot_ref", None, "aliases"), ("Minv", None, "M", None, "Minv aliases M"),
             ("cart_pose", 3, "cart_pose", 0, "beyond n_cart"), ("cart_p0", 7, "cart_p0", 0, "beyond n_cart"),
             ("cart_Mi", 0, "cart_Mi", 1, "not OSOT_ACC_GAIN_FORCE"), ("cart_f_virtual", 2, "cart_f_virtual", 1, "not OSOT_ACC_GAIN_FORCE")]
    for field, index, src, src_index, words in alias:
        m, b, keep = _structs(case)
        _set(b, field, get(b, src, src_index), index)
        rc, why = ar.host_check(m, b)
        assert rc == abi.ERR_INVALID and words in why, (field, rc, why)
    # references without their output
    m, b, keep = _structs(case)
    b.cart_a_ref_out[1] = None
    rc, why = ar.host_check(m, b)
    assert rc == abi.ERR_INVALID and "without cart_a_ref_out" in why
    # postural gain matrices without the flag that makes the kernel read them
    m, b, keep = _structs(case)
    m.post_gain_matrices = 0
    rc, why = ar.host_check(m, b)
    assert rc == abi.ERR_INVALID and "post_gain_matrices is 0" in why, (rc, why)
    # groups the model lacks
    for flag, words in (("has_com", "has_com"), ("has_postural", "has_postural")):
        m, b, keep = _structs(case)
        setattr(m, flag, 0)
        if flag == "has_postural":
            m.post_gain_type = ACC       # (otherwise M would still be asked for: not the point here)
        rc, why = ar.host_check(m, b)
        assert rc == abi.ERR_INVALID and words in why, (rc, why)


def test_more_than_64_coordinates_are_unsupported_and_point_at_the_other_entry():
    m, b, keep = _structs(solved("nv35")[0])
    m.nv = 65
    rc, why = ar.host_check(m, b)
    assert rc == abi.ERR_UNSUPPORTED and "osot_id_force_gains" in why and "inverse" in why


def test_an_empty_batch_is_a_no_op():
    m, b, (out, keep) = _structs(solved("nv35")[0])
    b.B = 0
    assert ar.lib().acc_host_tasks(C.byref(m), C.byref(b)) == abi.OK
    assert all(np.all(a == (SENTINEL if a.dtype != np.int32 else -7)) for a in out.arrays())


# ---- 8. the stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer -----------------------------------------------------
def test_sanitized_standalone_program_runs_clean():
    """its own main, statically linked runtimes, a child process: nothing is loaded into the interpreter"""
    r = subprocess.run([ar.ensure_sanitized()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nv = 64 n_cart = 8" in r.stdout and "acc_tasks: ok" in r.stdout


# ---- 9. the tracking stack through the emulated update ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain_type", [ACC, FORCE])
def test_tracking_stack_validates_and_its_assembled_b_is_the_reference_formulas(gain_type):
    from helpers import emu_update
    from opensot_amd import synth
    B = 2
    plan, leaf, model = synth.make_coman_id_tracking_stack(B, gain_type=gain_type, seed=31)
    assert abi.lib().osot_plan_validate(C.byref(plan.to_c())) == abi.OK
    q = leaf["state"]["q0"]
    qd = np.random.default_rng(4).uniform(-0.2, 0.2, q.shape)
    Q = ar.tracking_quantities(model, leaf, q, qd)
    hand_ref = Q["hand_pose"].copy()
    hand_ref[:, 9:12] += leaf["state"]["tracking"]["offset"]
    com_ref = Q["com"] + 0.01
    case = ar.tracking_case(leaf, Q, q, qd, com_ref, hand_ref)
    out, nv = ar.run_host(case, ("cart_p0", "cart_a_ref_out", "com_p0", "post_p0", "post_qddot_out", "ok")), model.n
    assert np.all(out.ok[1:-1] == 1)
    res = emu_update(plan, ar.tracking_leaf(leaf, Q, out.p0(0), out.a_ref_out(0), out.com(), out.post(nv), out.qddot(nv)))
    b_hand, b_com, b_post, scale = ar.tracking_b(plan, Q, ar.restate(case, np.longdouble))
    cond = np.array([np.linalg.cond(M) for M in case["M"]])
    # hand: every Cholesky-based factor is within CHOLESKY_TOL cond2(M) of its size; the sums add (k + 2) u of theirs (k = 14 terms)
    tol = ((ar.CHOLESKY_TOL * cond if gain_type == FORCE else 0.0) + 16 * ar.U) * scale
    err = np.abs(_ld(res["b"][1]) - b_hand).max(axis=1)
    print("hand b: worst error / bound", float((err / tol).max()))
    assert np.all(err <= tol)
    # CoM: lambda2 vel_err + lambda pose_err - Jdot qdot, vel_err an fma chain of nv terms
    com_scale = 10.0 * (np.abs(Q["Jcom"]).sum(axis=2) * np.abs(qd).max()).max(axis=1) + 25.0 * 0.01 + np.abs(Q["com_jdq"]).max(axis=1)
    assert np.all(np.abs(_ld(res["b"][0][:, 12:15]) - b_com).max(axis=1) <= (nv + 5) * ar.U * com_scale)
    assert np.all(res["b"][0][:, :12] == -np.concatenate([Q["jdq"][:, 0], Q["jdq"][:, 1]], axis=1))     # the contacts: -Jdot qdot
    # postural: b = p2 = qddot_d (lambda = lambda2 = 0 on the block)
    assert np.array_equal(res["b"][2], out.qddot(nv))
    dev = np.abs(_ld(res["b"][2]) - b_post).max(axis=1) / np.abs(b_post).max(axis=1)
    print("postural b: worst deviation / cond2(M)", float((dev / cond).max()))
    assert np.all(dev <= (ar.CHOLESKY_TOL * cond if gain_type == FORCE else (2 * nv + 3) * ar.U * 40.0))
