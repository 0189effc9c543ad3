"""The measurement-driven producer (opensot_amd/csrc/osot_feedback.h) on the host: the kernel through the lock-step emulation against
the numpy restatement of tests/feedback_ref.py, the host helpers, the refusals of osot_feedback, and the stand-alone sanitizer
program.  No GPU needed."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from opensot_amd import abi
import feedback_ref as fb

LD = np.longdouble


# ---- the filter ------------------------------------------------------------------------------------------------------------------------
def _filter_case(B=5, seed=3):
    """two Cartesian terms and the joint filter, nothing else bound"""
    return fb.make_case(B, 9, n_cart=2, seed=seed, imu=False, contact=False)


@pytest.mark.parametrize("start", ["zero", "reset"])
@pytest.mark.parametrize("steps", [1, 3, 40])
def test_filter_emulation_equals_the_restatement(steps, start):
    """1, 3 (the first step at which udd / ydd carry signal) and 40 steps with a new input every step, from zero state and from
    reset(value): outputs and state of the emulated kernel are the float64 restatement's bits; and every single step, taken from the
    state the step started in, is within (k + 2) 2^-53 sum |terms| / |a0| of its longdouble value, k = 5 terms"""
    case = _filter_case()
    rng = np.random.default_rng(steps)
    n = fb.state_count(case)
    state = np.zeros((case["B"], n)) if start == "zero" else np.full((case["B"], n), 0.37)
    ref_state = state.copy()
    cj = fb.host_coeff(case["joint_omega"], case["joint_damping"], case["joint_ts"])
    worst = 0.0
    for k in range(steps):
        for t in range(2):
            case["cart_wrench"][t] = rng.uniform(-2.0, 2.0, (case["B"], 6))
        case["joint_tau"] = rng.uniform(-30.0, 30.0, (case["B"], case["nv"]))
        before = state.copy()
        out = fb.run_host(case, state)
        ref = fb.step(case, ref_state)
        assert np.array_equal(state, ref_state), k
        fb.check_outputs(out, ref, case, what=("cart", "joint"))
        # the single step against longdouble, from the float64 state and the float64 coefficients of the host
        terms, a0 = fb.filter_terms(fb.joint_views(case, before), case["joint_h"] - case["joint_tau"], cj[0], cj[1], cj[2])
        val, bound = sum(terms) / a0, 7 * fb.U * sum(np.abs(v) for v in terms) / abs(a0)
        err = np.abs(fb.joint_views(case, state)[2].astype(LD) - val)
        assert (err <= bound).all(), k
        worst = max(worst, float((err / np.maximum(bound, LD(1e-300))).max()))
        for t in range(2):
            e = fb.deadzone(fb.rotate_wrench(case["cart_pose"][t], case["cart_wrench"][t]), case["cart_deadzone"][t][None, :]) - case["cart_wrench_ref"][t]
            c = np.stack([fb.host_coeff(case["cart_omega"][t][ch], case["cart_damping"][t][ch], case["cart_ts"][t]) for ch in range(6)])
            terms, a0 = fb.filter_terms(fb.cart_views(case, before)[t], e, c[None, :, 0], c[None, :, 1], c[None, :, 2])
            val, bound = sum(terms) / a0, 7 * fb.U * sum(np.abs(v) for v in terms) / np.abs(a0)
            err = np.abs(fb.cart_views(case, state)[t][2].astype(LD) - val)
            assert (err <= bound).all(), (k, t)
    print(f"{steps} steps from {start}: worst single-step err / bound (joint) = {worst:.3f}")
    if start == "zero" and steps == 1:
        u, ud, y, yd = fb.joint_views(case, state)
        assert (ud == 0.0).all() and (yd == 0.0).all() and (u != 0.0).all() and (y != 0.0).all()


def test_reset_value_is_a_fixed_point_of_a_constant_input():
    """reset(v) then the input v: the filter has unit DC gain, so y stays at v to rounding (a0 + a1 + a2 = 4 exactly in the reals)"""
    case = fb.make_case(2, 7, seed=1, imu=False, contact=False)
    v = 1.25
    case["joint_h"], case["joint_tau"] = np.full((2, 7), v), np.zeros((2, 7))
    state = np.full((2, fb.state_count(case)), v)
    fb.run_host(case, state)
    a0, a1, a2, _ = fb.host_coeff(case["joint_omega"], case["joint_damping"], case["joint_ts"])
    # 7 roundings of the step and 4 * 2^-53 relative on each coefficient, all on terms of size |a_k| v / a0
    assert np.abs(fb.joint_views(case, state)[2] - v).max() <= (7 + 4) * fb.U * v * (4.0 + abs(a1) + abs(a2) + a0) / a0


def test_filter_coefficients():
    """a0, a1, a2 of the host within 4 * 2^-53 relative of the longdouble ones (the same expression from the same doubles)"""
    rng = np.random.default_rng(0)
    sets = [(1.0, 1.0, 0.01), (2.0 * math.pi * 8.0, 1.0, 0.002), (1.0, 0.8, 0.01)] + \
           [(float(rng.uniform(1.0, 100.0)), float(rng.uniform(0.0, 2.0)), float(rng.uniform(1e-3, 1e-2))) for _ in range(40)]
    for omega, eps, ts in sets:
        got = fb.host_coeff(omega, eps, ts)
        ref = fb.filter_coeff(omega, eps, ts, dtype=LD)
        for name, g, r in zip(("a0", "a1", "a2"), got[:3], ref):
            assert abs(LD(g) - r) <= 4 * fb.U * abs(r), (name, omega, eps, ts, float(g), float(r))
        assert got[3] == 1.0 / got[0]
        assert tuple(got[:3]) == tuple(float(v) for v in fb.filter_coeff(omega, eps, ts))     # the float64 restatement: the same bits


# ---- the dead zone ---------------------------------------------------------------------------------------------------------------------
def test_dead_zone():
    """exactly at +-dz (inside: 0), inside, outside, and dz = 0 (every value passes, a zero stays zero)"""
    B = 8
    case = fb.make_case(B, 6, n_cart=2, seed=2, joint=False, imu=False, contact=False, refs=False)
    dz = 0.25
    case["cart_deadzone"] = np.array([[dz] * 6, [0.0] * 6])
    case["cart_C"] = np.ones((2, 6))
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    vals = np.array([dz, -dz, 0.1, -0.1, 0.75, -0.75, 0.0, np.nextafter(dz, 1.0)])
    for t in range(2):
        case["cart_pose"][t] = np.tile(eye, (B, 1))
        case["cart_wrench"][t] = np.tile(vals[:, None], (1, 6))
    state = np.zeros((B, fb.state_count(case)))
    fb.run_host(case, state)
    u0, u1 = fb.cart_views(case, state)[0][0], fb.cart_views(case, state)[1][0]      # u: what entered the filter
    expect = np.array([0.0, 0.0, 0.0, 0.0, 0.75 - dz, -0.75 + dz, 0.0, np.nextafter(dz, 1.0) - dz])
    assert np.array_equal(u0, np.tile(expect[:, None], (1, 6)))
    assert np.array_equal(u1, np.tile(vals[:, None], (1, 6)))
    assert np.array_equal(fb.deadzone(np.tile(vals[:, None], (1, 6)), dz), u0)


# ---- osot_admittance_params ------------------------------------------------------------------------------------------------------------
def test_admittance_params_closed_forms_and_refusal():
    K = np.array([1e4, 1e4, 1e4, 1e5, 1e5, 1e5])
    lam, dt = 0.01, 0.002
    D = 1.1 * K * dt / lam                                   # the constructor's, CartesianAdmittance.cpp:30-36
    rc, why, Cc, M, w = fb.host_admittance_params(K, D, lam, dt)
    assert rc == abi.OK
    assert np.array_equal(Cc, lam * (1.0 / K))
    assert np.array_equal(M, (dt / lam) * D - ((dt * dt) / lam) * (1.0 / Cc))
    assert np.array_equal(w, dt * (1.0 / (Cc * M)))
    # C = lambda / K, M = dt (D - K dt / lambda) / lambda, w = dt / (C M), in longdouble
    Kl, Dl = K.astype(LD), D.astype(LD)
    Cl = LD(lam) / Kl
    Ml = LD(dt) * (Dl - Kl * LD(dt) / LD(lam)) / LD(lam)
    assert (np.abs(Cc - Cl) <= 4 * fb.U * np.abs(Cl)).all()
    # M is a difference of two nearly equal numbers (D = 1.1 K dt / lambda): bounded by the roundings of the two
    assert (np.abs(M - Ml) <= 8 * fb.U * (LD(dt) / LD(lam)) * Dl).all()
    assert (M > 0.0).all() and (w > 0.0).all()
    for i in range(6):
        Dbad = D.copy()
        Dbad[i] = K[i] * dt / lam                            # D[i] <= K[i] dt / lambda: equality is refused
        rc, why, Cc, M, w = fb.host_admittance_params(K, Dbad, lam, dt)
        assert rc == abi.ERR_INVALID and "D[i] <= K[i] * dt / lambda" in why
        assert (Cc == fb.SENTINEL).all() and (M == fb.SENTINEL).all() and (w == fb.SENTINEL).all()


# ---- joint admittance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [6, 7, 35, 64])
def test_dense_compliance_within_its_bound(nv):
    """row i of C y is an fma chain over j: within nv 2^-53 sum_j |C_ij y_j| of the longdouble sum"""
    case = fb.make_case(3, nv, dense=True, floating_base=0, seed=nv, imu=False, contact=False)
    state = np.zeros((3, fb.state_count(case)))
    out = fb.run_host(case, state)
    y = fb.joint_views(case, state)[2]
    terms = fb.joint_terms(case, y)
    err = np.abs(out.joint_qdot_out.astype(LD) - sum(terms))
    assert (err <= nv * fb.U * sum(np.abs(t) for t in terms)).all()
    assert (out.joint_qdot_out != 0.0).all()


@pytest.mark.parametrize("nv,floating_base", [(6, 1), (7, 1), (7, 0), (35, 1)])
@pytest.mark.parametrize("dense", [False, True], ids=["scalar", "dense"])
def test_scalar_path_and_the_zero_head(nv, floating_base, dense):
    case = fb.make_case(3, nv, dense=dense, floating_base=floating_base, seed=10 + nv, imu=False, contact=False)
    state = np.zeros((3, fb.state_count(case)))
    ref_state = state.copy()
    out = fb.run_host(case, state, calls=2)
    fb.step(case, ref_state)
    ref = fb.step(case, ref_state)
    assert np.array_equal(state, ref_state)
    q = out.joint_qdot_out
    if floating_base:
        assert (q[:, :6] == 0.0).all()
        if nv == 6:
            assert (q == 0.0).all()
        assert (q[:, 6:] != 0.0).all()
    else:
        assert (q != 0.0).all()
    if not dense:
        assert np.array_equal(q, ref["joint_qdot_out"])
        assert np.array_equal(q[:, 6 * floating_base:], (case["joint_C_scalar"] * ref["joint_y"])[:, 6 * floating_base:])


# ---- IMU, collision rows, contact error ------------------------------------------------------------------------------------------------
ROW_SHAPES = [(6, 1, 7, 0), (7, 1, 7, 3), (35, 32, 64, 0), (64, 32, 106, 5), (35, 16, 35, 2)]


@pytest.mark.parametrize("nv,n_pairs,n,pad", ROW_SHAPES)
def test_imu_and_collision_rows_are_bit_exact_and_nothing_else_is_written(nv, n_pairs, n, pad):
    case = fb.make_case(3, nv, n_cart=1, n_pairs=n_pairs, n=n, seed=nv + n)
    state = np.zeros((3, fb.state_count(case)))
    ref_state = state.copy()
    out = fb.run_host(case, state, pad=pad)
    fb.check_outputs(out, fb.step(case, ref_state), case)
    assert np.array_equal(state, ref_state)


def test_collision_rows_at_zero_above_and_below():
    """err == 0 counts as violated (the reference `continue`s only on err > 0)"""
    case = fb.make_case(1, 7, n_pairs=3, n=7, seed=0, joint=False, imu=False, contact=False)
    thr = case["ca_threshold"]
    case["ca_dist"] = np.array([[thr, np.nextafter(thr, 1.0), np.nextafter(thr, -1.0)]])
    out = fb.run_host(case, None)
    J = case["ca_J"][0]
    assert np.array_equal(out.ca_A[0, 1], -J[0]) and out.ca_b[0, 1] == 0.0
    assert (out.ca_A[0, 2] == 0.0).all() and out.ca_b[0, 2] == 0.0
    assert np.array_equal(out.ca_A[0, 3], -J[2]) and out.ca_b[0, 3] == np.nextafter(thr, -1.0) - thr < 0.0


def test_contact_error():
    """within 5e-15 absolute of the longdouble restatement for |p| <= 2 (about twenty roundings on quantities below 2), and the
    float64 restatement's bits"""
    case = fb.make_case(40, 7, seed=4, joint=False, imu=False)
    assert np.abs(case["contact_pose"][:, 9:]).max() <= 2.0 and np.abs(case["contact_pose_ref"][:, 9:]).max() <= 2.0
    out = fb.run_host(case, None)
    got = out.contact_b_out[:, 1:7]
    lam = LD(case["contact_lambda"])
    ref = np.stack([case["contact_b_in"][i].astype(LD) + lam * fb.contact_error_ld(case["contact_pose"][i], case["contact_pose_ref"][i])
                    for i in range(40)])
    err = np.abs(got.astype(LD) - ref)
    print(f"contact error: max |err| = {float(err.max()):.3e}")
    assert err.max() <= 5e-15
    fb.check_outputs(out, fb.step(case, None), case, what=("contact",))
    # idempotent: b_in is not b_out
    again = fb.run_host(case, None)
    assert np.array_equal(again.contact_b_out, out.contact_b_out)


def test_contact_error_on_each_side_of_the_sign_flip():
    """a pose pair on each side of q . q_d = 0 (a relative rotation just below and just above pi): the short-path rule flips q, the
    error stays continuous in magnitude and both sides are within the bound"""
    axis = np.array([0.0, 0.6, 0.8])
    case = fb.make_case(2, 7, seed=6, joint=False, imu=False)
    Ta = fb.random_pose(np.random.default_rng(1))
    sides = []
    for i, ang in enumerate((math.pi - 1e-3, math.pi + 1e-3)):
        Tr = np.concatenate([(fb.force_ref.rotation(axis, ang) @ Ta[:9].reshape(3, 3)).reshape(9), Ta[9:]])
        case["contact_pose"][i], case["contact_pose_ref"][i] = Ta, Tr
        q, qd = fb.rot_to_quat(Ta[:9]), fb.rot_to_quat(Tr[:9])
        sides.append(sum(a * b for a, b in zip(q, qd)))
    assert sides[0] * sides[1] < 0.0, sides
    case["contact_b_in"][:] = 0.0
    case["contact_lambda"] = 1.0
    out = fb.run_host(case, None)
    got = out.contact_b_out[:, 1:7]
    ref = np.stack([fb.contact_error_ld(case["contact_pose"][i], case["contact_pose_ref"][i]) for i in range(2)])
    assert np.abs(got.astype(LD) - ref).max() <= 5e-15
    # |e_o| = sin(theta / 2) on the short path on both sides, the direction flips
    assert abs(np.linalg.norm(got[0, 3:]) - math.sin((math.pi - 1e-3) / 2)) <= 1e-12
    assert abs(np.linalg.norm(got[1, 3:]) - math.sin((math.pi - 1e-3) / 2)) <= 1e-12
    assert got[0, 3:] @ got[1, 3:] < 0.0


def test_null_references_and_unbound_terms():
    """NULL wrench_ref / twist_in are zeros; a term without cart_twist_out keeps its state"""
    case = fb.make_case(3, 7, n_cart=2, seed=5, refs=False, imu=False, contact=False)
    state = np.zeros((3, fb.state_count(case)))
    ref_state = state.copy()
    out = fb.run_host(case, state)
    fb.check_outputs(out, fb.step(case, ref_state), case)
    assert np.array_equal(state, ref_state)
    out2 = fb.Outputs(case)
    m, b = fb.structs(case, out2, state, lambda a: a.ctypes.data)
    b.cart_pose[1] = b.cart_wrench[1] = b.cart_twist_out[1] = None
    before = state.copy()
    assert fb.lib().feedback_host_run(C.byref(m), C.byref(b)) == abi.OK
    assert np.array_equal(state[:, 24:48], before[:, 24:48]) and not np.array_equal(state[:, :24], before[:, :24])
    assert (out2.cart_twist_out[1] == fb.SENTINEL).all()


def test_state_doubles():
    for nv, nc, joint in ((7, 0, 0), (7, 3, 0), (35, 2, 1), (64, 8, 1), (6, 0, 1)):
        m = abi.FeedbackModel()
        m.nv, m.n_cart, m.joint = nv, nc, joint
        assert fb.lib().feedback_host_state_doubles(C.byref(m)) == 4 * (6 * nc + nv * joint)


def test_B65_more_instances_than_lanes():
    case = fb.make_case(65, 35, n_cart=2, n_pairs=16, n=35, dense=True, seed=9)
    state = np.zeros((65, fb.state_count(case)))
    ref_state = state.copy()
    out = fb.run_host(case, state, pad=1, calls=3)
    for _ in range(2):
        fb.step(case, ref_state)
    fb.check_outputs(out, fb.step(case, ref_state), case)
    assert np.array_equal(state, ref_state)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def _good():
    case = fb.make_case(2, 35, n_cart=2, n_pairs=4, n=35, dense=True, seed=0)
    out = fb.Outputs(case, pad=2)
    state = np.zeros((2, fb.state_count(case)))
    m, b = fb.structs(case, out, state, lambda a: a.ctypes.data)
    return case, out, state, m, b


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def _item(arr, i, v):
    arr[i] = v


REFUSALS = [
    ("nv_low", lambda m, b: _set(m, nv=0), "nv is outside 1 .. 64"),
    ("nv_high", lambda m, b: _set(m, nv=65), "nv is outside 1 .. 64"),
    ("floating_base", lambda m, b: _set(m, floating_base=2), "floating_base is not 0 or 1"),
    ("n_cart_low", lambda m, b: _set(m, n_cart=-1), "n_cart is outside 0 .. 8"),
    ("n_cart_high", lambda m, b: _set(m, n_cart=9), "n_cart is outside 0 .. 8"),
    ("joint_flag", lambda m, b: _set(m, joint=2), "joint is not 0 or 1"),
    ("imu_flag", lambda m, b: _set(m, imu=-1), "imu is not 0 or 1"),
    ("n_pairs_high", lambda m, b: _set(m, n_pairs=33), "n_pairs is outside 0 .. 32"),
    ("n_low", lambda m, b: _set(m, n=0), "n is outside 1 .. 128"),
    ("n_high", lambda m, b: _set(m, n=129), "n is outside 1 .. 128"),
    ("B_negative", lambda m, b: _set(b, B=-1), "B is negative"),
    ("cart_ts", lambda m, b: _item(m.cart_ts, 1, 0.0), "a cart_ts is not positive and finite"),
    ("cart_C_nan", lambda m, b: _item(m.cart_C, 7, float("nan")), "a cart_C is not finite"),
    ("deadzone_negative", lambda m, b: _item(m.cart_deadzone, 0, -1e-9), "a cart_deadzone is negative or not finite"),
    ("cart_omega_zero", lambda m, b: _item(m.cart_omega, 11, 0.0), "a cart_omega is not positive and finite"),
    ("cart_damping_inf", lambda m, b: _item(m.cart_damping, 3, float("inf")), "a cart_damping is negative or not finite"),
    ("joint_ts", lambda m, b: _set(m, joint_ts=-0.002), "joint_ts is not positive and finite"),
    ("joint_omega", lambda m, b: _set(m, joint_omega=float("nan")), "joint_omega is not positive and finite"),
    ("joint_damping", lambda m, b: _set(m, joint_damping=-1.0), "joint_damping is negative or not finite"),
    ("joint_C_scalar", lambda m, b: _set(m, joint_C_scalar=float("inf")), "joint_C_scalar is not finite"),
    ("contact_lambda", lambda m, b: _set(m, contact_lambda=float("nan")), "contact_lambda is not finite"),
    ("ca_threshold", lambda m, b: _set(m, ca_threshold=float("inf")), "ca_threshold is not finite"),
    ("state_null", lambda m, b: _set(b, state=None), "state is null"),
    ("cart_beyond", lambda m, b: _item(b.cart_wrench_ref, 2, b.cart_wrench_ref[0]), "bound to a term beyond n_cart"),
    ("cart_input_orphan", lambda m, b: _item(b.cart_twist_out, 1, None), "without cart_twist_out"),
    ("cart_pose_null", lambda m, b: _item(b.cart_pose, 0, None), "cart_pose / cart_wrench is null"),
    ("cart_alias", lambda m, b: _item(b.cart_twist_out, 1, b.cart_twist_in[1]), "cart_twist_out aliases cart_twist_in"),
    ("joint_off", lambda m, b: _set(m, joint=0), "joint_qdot_out with joint == 0"),
    ("joint_tau_null", lambda m, b: _set(b, joint_tau=None), "joint_tau / joint_h is null"),
    ("joint_orphan", lambda m, b: _set(b, joint_qdot_out=None), "without joint_qdot_out"),
    ("imu_off", lambda m, b: _set(m, imu=0), "imu_A / imu_b with imu == 0"),
    ("imu_nv", lambda m, b: _set(m, nv=5), "imu rows asked with nv below 6"),
    ("imu_J_null", lambda m, b: _set(b, imu_fb_J=None), "imu_fb_J is null"),
    ("imu_J_stride", lambda m, b: _set(b, imu_fb_J_stride=6 * 35 - 1), "imu_fb_J_stride is below 6 * nv"),
    ("imu_ld", lambda m, b: _set(b, imu_A_ld=5), "imu_A_ld is below 6"),
    ("imu_A_stride", lambda m, b: _set(b, imu_A_stride=6 * 8 - 1), "imu_A_stride is below 6 * ld"),
    ("imu_J_orphan", lambda m, b: _set(b, imu_A=None), "imu_fb_J without imu_A"),
    ("imu_pose_null", lambda m, b: _set(b, imu_omega=None), "imu_pose / imu_omega is null"),
    ("imu_b_stride", lambda m, b: _set(b, imu_b_stride=5), "imu_b_stride is below 6"),
    ("imu_pose_orphan", lambda m, b: _set(b, imu_b=None), "imu_pose / imu_omega without imu_b"),
    ("contact_ref_null", lambda m, b: _set(b, contact_pose_ref=None), "contact_pose / contact_pose_ref / contact_b_in is null"),
    ("contact_in_stride", lambda m, b: _set(b, contact_b_in_stride=5), "contact_b_in_stride is below 6"),
    ("contact_out_stride", lambda m, b: _set(b, contact_b_out_stride=0), "contact_b_out_stride is below 6"),
    ("contact_alias", lambda m, b: _set(b, contact_b_out=b.contact_b_in, contact_b_out_stride=6), "contact_b_out aliases contact_b_in"),
    ("contact_orphan", lambda m, b: _set(b, contact_b_out=None), "without contact_b_out"),
    ("ca_no_pairs", lambda m, b: _set(m, n_pairs=0), "ca_A / ca_b with n_pairs == 0"),
    ("ca_dist_null", lambda m, b: _set(b, ca_dist=None), "ca_dist is null"),
    ("ca_orphan", lambda m, b: _set(b, ca_A=None, ca_b=None), "ca_dist / ca_J without ca_A / ca_b"),
    ("ca_J_null", lambda m, b: _set(b, ca_J=None), "ca_J is null"),
    ("ca_alias", lambda m, b: _set(b, ca_A=b.ca_J), "ca_A aliases ca_J"),
    ("ca_J_stride", lambda m, b: _set(b, ca_J_stride=4 * 35 - 1), "ca_J_stride is below n_pairs * n"),
    ("ca_ld", lambda m, b: _set(b, ca_A_ld=34), "ca_A_ld is below n"),
    ("ca_A_stride", lambda m, b: _set(b, ca_A_stride=4 * 37 - 1), "ca_A_stride is below n_pairs * ld"),
    ("ca_J_orphan", lambda m, b: _set(b, ca_A=None), "ca_J without ca_A"),
    ("ca_b_stride", lambda m, b: _set(b, ca_b_stride=3), "ca_b_stride is below n_pairs"),
]


def test_the_good_arguments_pass():
    _, _, _, m, b = _good()
    assert fb.host_check(m, b) == (abi.OK, "")
    b.B = 0
    assert fb.host_check(m, b) == (abi.OK, "")


def test_interleaved_contact_b_is_not_an_alias():
    """b_in and b_out six doubles apart in one buffer with one stride: disjoint entries"""
    case, out, state, m, b = _good()
    buf = np.zeros((2, 12))
    b.contact_b_in, b.contact_b_in_stride, b.contact_b_out, b.contact_b_out_stride = buf.ctypes.data, 12, buf.ctypes.data + 48, 12
    assert fb.host_check(m, b) == (abi.OK, "")
    b.contact_b_out = buf.ctypes.data + 40
    assert fb.host_check(m, b)[0] == abi.ERR_INVALID


@pytest.mark.parametrize("name,spoil,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(name, spoil, reason):
    _, _, _, m, b = _good()
    spoil(m, b)
    rc, why = fb.host_check(m, b)
    assert rc == abi.ERR_INVALID and reason in why, (rc, why)


def test_refused_before_anything_is_written():
    case, out, state, m, b = _good()
    m.n_pairs = 33
    assert fb.lib().feedback_host_run(C.byref(m), C.byref(b)) == abi.ERR_INVALID
    assert all((a == fb.SENTINEL).all() for a in out.arrays().values()) and (state == 0.0).all()


# ---- the stand-alone sanitizer program -------------------------------------------------------------------------------------------------
def test_sanitized_program():
    """tests/emu/feedback_host.cpp with its own main under ASan + UBSan (statically linked runtimes): three shapes, three calls each,
    every input array of its exact size on the heap, every destination checked entry by entry"""
    exe = fb.ensure_sanitized()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "feedback: ok" in r.stdout
