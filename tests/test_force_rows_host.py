"""The force-space row producer (opensot_amd/csrc/osot_force.h) on the host: the kernel through the lock-step emulation against the
numpy restatement of tests/force_ref.py, the refusals of osot_force_rows, and the stand-alone sanitizer program.  No GPU needed."""
import math
import subprocess

import numpy as np
import pytest

from opensot_amd import abi
import force_ref as fr

SHAPE_B = [("C1_nv7", 3), ("C8_nv64", 2), ("C3_nv35", 3)]


@pytest.fixture(scope="module", params=SHAPE_B, ids=[s for s, _ in SHAPE_B])
def ran(request):
    name, B = request.param
    case, ld = fr.shape_case(name, B, seed=11)
    return case, ld, fr.run_host(case, ld)


def block(a, rows):
    return a[:, 1:1 + rows, :]


def test_matrix_blocks_are_bit_exact(ran):
    """(1), (2), (3): copies, transposes, negations and one subtraction per entry"""
    case, ld, out = ran
    n, na = case["n"], case["nv"] - 6
    for name, ref, rows, static in (("com_A", fr.com_A(case), 6, False), ("fb_A", fr.fb_A(case), 6, False),
                                    ("static_A", fr.static_A(case), na, True)):
        cols = fr.written_columns(case, static)
        got = block(getattr(out, name), rows)
        assert np.array_equal(got[:, :, cols], ref[:, :, cols]), name
    assert np.array_equal(out.static_lo[:, 1:1 + na], fr.static_b(case))
    assert np.array_equal(out.static_up[:, 1:1 + na], fr.static_b(case))


def test_nothing_else_is_written(ran):
    """every entry outside the written columns and rows still holds the sentinel"""
    case, ld, out = ran
    na = case["nv"] - 6
    for name, rows, static in (("com_A", 6, False), ("fb_A", 6, False), ("static_A", na, True)):
        a = getattr(out, name).copy()
        a[:, 1:1 + rows, fr.written_columns(case, static)] = fr.SENTINEL
        assert (a == fr.SENTINEL).all(), name
        assert (getattr(out, name)[:, 1:1 + rows, fr.written_columns(case, static)] != fr.SENTINEL).all(), name
    for name, w in (("com_b", 6), ("cart_b", 6), ("static_lo", na), ("static_up", na)):
        a = getattr(out, name).copy()
        assert (a[:, 1:1 + w] != fr.SENTINEL).all(), name
        a[:, 1:1 + w] = fr.SENTINEL
        assert (a == fr.SENTINEL).all(), name


def check_b(got, terms, what):
    val, bound = fr.value_and_bound(terms)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - val)
    print(f"{what}: max |err| = {float(err.max()):.3e}, min bound = {float(bound.min()):.3e}, max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), what


def test_com_b_within_its_forward_error_bound(ran):
    case, ld, out = ran
    lin, ang = fr.com_b_terms(case)
    check_b(out.com_b[:, 1:4], lin, "com_b linear")
    check_b(out.com_b[:, 4:7], ang, "com_b angular")


def test_cart_b_within_its_forward_error_bound(ran):
    case, ld, out = ran
    check_b(out.cart_b[:, 1:7], fr.cart_b_terms(case), "cart_b")


def test_orientation_error_is_the_restated_sequence():
    """with Kp = I, Kd = 0, no f_des, cart_b IS e (each fma adds 0 or multiplies by 1): the kernel's quaternion error equals the
    restatement's bit for bit -- both are the same IEEE operations in the same order"""
    case, ld = fr.shape_case("C3_nv35", 40, seed=5)
    case["cart_Kp"], case["cart_Kd"], case["cart_f_des"] = np.eye(6), np.zeros((6, 6)), None
    out = fr.run_host(case, ld, want=("cart_b",))
    assert np.array_equal(out.cart_b[:, 1:7], fr.pose_error(case))


@pytest.mark.parametrize("theta", [1.0e-1, 1.0e-2, 1.0e-3])
def test_orientation_error_small_angle(theta):
    """e_o = 2 sin(theta / 2) axis against the rotation vector theta axis of R_ref R': they differ by the cubic term theta^3 / 24
    (an alternating series, so the term bounds the difference); 2^-48 covers the roundings of the O(1) rotation entries"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        Ta = fr.random_pose(rng)
        Tr = np.concatenate([(fr.rotation(axis, theta) @ Ta[:9].reshape(3, 3)).reshape(9), Ta[9:]])
        eo = fr.orientation_error(Ta, Tr)
        assert np.abs(eo - theta * axis).max() <= theta ** 3 / 24.0 + 2.0 ** -48
        assert eo @ axis > 0.0        # from the actual to the reference orientation
    # and through the kernel
    case, ld = fr.shape_case("C1_nv7", 4, seed=1)
    case["cart_Kp"], case["cart_Kd"], case["cart_f_des"] = np.eye(6), np.zeros((6, 6)), None
    axis = np.array([0.6, 0.0, 0.8])
    Ta = case["pose"][0]
    case["cart_pose_ref"] = np.stack([np.concatenate([(fr.rotation(axis, theta) @ Ta[i, :9].reshape(3, 3)).reshape(9), Ta[i, 9:]]) for i in range(4)])
    out = fr.run_host(case, ld, want=("cart_b",))
    assert np.abs(out.cart_b[:, 4:7] - theta * axis).max() <= theta ** 3 / 24.0 + 2.0 ** -48


def test_pose_error_input_replaces_e():
    case, ld = fr.shape_case("C3_nv35", 3, seed=8, pose_error=True)
    out = fr.run_host(case, ld, want=("cart_b",))
    check_b(out.cart_b[:, 1:7], fr.cart_b_terms(case), "cart_b with pose_error")
    other = dict(case, cart_pose_ref=case["cart_pose_ref"][::-1].copy())     # not read
    assert np.array_equal(fr.run_host(other, ld, want=("cart_b",)).cart_b, out.cart_b)


def test_null_references():
    """NULL references: p_d = the CoM, L_d = the momentum, everything else zero"""
    case, ld = fr.shape_case("C3_nv35", 3, seed=9, refs=False, qdot=False)
    out = fr.run_host(case, ld)
    lin, ang = fr.com_b_terms(case)
    check_b(out.com_b[:, 1:4], lin, "com_b linear")
    assert (out.com_b[:, 4:7] == 0.0).all()
    check_b(out.cart_b[:, 1:7], fr.cart_b_terms(case), "cart_b")
    assert np.array_equal(out.static_lo[:, 1:-1], case["h_gravity"][:, 6:])


def test_enabled_mask():
    """a disabled contact's block is exactly zero; all-enabled equals no mask, bit for bit"""
    case, ld = fr.shape_case("C3_nv35", 4, seed=2, enabled=[[1, 0, 1], [0, 0, 0], [1, 1, 1], [0, 1, 0]])
    out = fr.run_host(case, ld)
    na = case["nv"] - 6
    for i in range(4):
        for c, w in enumerate(case["wrench_col"]):
            for name, rows in (("com_A", 6), ("fb_A", 6), ("static_A", na)):
                blk = getattr(out, name)[i, 1:1 + rows, w:w + 6]
                if case["enabled"][i, c]:
                    assert np.abs(blk).sum() > 0.0
                else:
                    assert (blk == 0.0).all(), (name, i, c)
    assert np.array_equal(out.static_A[:, 1:1 + na, case["torque_col"]:case["torque_col"] + na], np.broadcast_to(np.eye(na), (4, na, na)))
    ones, none = fr.run_host(dict(case, enabled=np.ones((4, 3), dtype=np.int32)), ld), fr.run_host(dict(case, enabled=None), ld)
    for name, a in ones.arrays().items():
        assert np.array_equal(a, none.arrays()[name]), name


def test_strides_larger_than_one_instance_and_B65():
    """more instances than lanes; the instance stride is the one given"""
    case, ld = fr.shape_case("C3_nv35", 65, seed=4)
    out = fr.run_host(case, ld)
    cols = fr.written_columns(case, True)
    assert np.array_equal(out.static_A[:, 1:-1, :][:, :, cols], fr.static_A(case)[:, :, cols])
    assert np.array_equal(out.fb_A[:, 1:7, :][:, :, fr.written_columns(case, False)], fr.fb_A(case)[:, :, fr.written_columns(case, False)])


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def _good():
    case, ld = fr.shape_case("C3_nv35", 2, seed=0)
    out = fr.Outputs(case, ld)
    m, b = fr.structs(case, out, lambda a: a.ctypes.data)
    return case, out, m, b


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


REFUSALS = [
    ("C_low", lambda m, b: _set(m, n_contacts=0), "n_contacts is outside 1 .. 8"),
    ("C_high", lambda m, b: _set(m, n_contacts=9), "n_contacts is outside 1 .. 8"),
    ("nv_low", lambda m, b: _set(m, nv=5), "nv is below 6"),
    ("nv_high", lambda m, b: _set(m, nv=65), "nv is above 64"),
    ("static_nv6", lambda m, b: _set(m, nv=6, torque_col=-1), "static rows asked with nv == 6"),
    ("wrench_leaves", lambda m, b: m.wrench_col.__setitem__(0, 75), "a wrench_col range leaves 0 .. n-1"),
    ("wrench_negative", lambda m, b: m.wrench_col.__setitem__(1, -1), "a wrench_col range leaves 0 .. n-1"),
    ("torque_leaves", lambda m, b: _set(m, torque_col=52), "the torque_col range leaves 0 .. n-1"),
    ("wrench_overlap", lambda m, b: m.wrench_col.__setitem__(2, 7), "two wrench_col ranges overlap"),
    ("torque_overlap", lambda m, b: _set(m, torque_col=44), "the torque_col range overlaps a wrench_col range"),
    ("com_ld", lambda m, b: _set(b, com_A_ld=79), "com_A_ld is below n"),
    ("fb_ld", lambda m, b: _set(b, fb_A_ld=79), "fb_A_ld is below n"),
    ("static_ld", lambda m, b: _set(b, static_A_ld=1), "static_A_ld is below n"),
    ("com_stride", lambda m, b: _set(b, com_A_stride=6 * 85 - 1), "com_A_stride is below 6 * ld"),
    ("fb_stride", lambda m, b: _set(b, fb_A_stride=0), "fb_A_stride is below 6 * ld"),
    ("static_stride", lambda m, b: _set(b, static_A_stride=29 * 85 - 1), "static_A_stride is below (nv - 6) * ld"),
    ("com_b_stride", lambda m, b: _set(b, com_b_stride=5), "com_b_stride is below 6"),
    ("cart_b_stride", lambda m, b: _set(b, cart_b_stride=5), "cart_b_stride is below 6"),
    ("static_b_stride", lambda m, b: _set(b, static_b_stride=28), "static_b_stride is below nv - 6"),
    ("lo_without_up", lambda m, b: _set(b, static_up=None), "static_lo and static_up go together"),
    ("com_refs_orphan", lambda m, b: _set(b, com_b=None), "ang_mom_rate_ref without com_b"),
    ("q_tau_orphan", lambda m, b: _set(b, static_lo=None, static_up=None), "static_q_tau without static_lo / static_up"),
    ("cart_refs_orphan", lambda m, b: _set(b, cart_b=None), "cart_pose_error without cart_b"),
    ("mass_nan", lambda m, b: _set(m, mass=float("nan")), "mass is not finite"),
    ("mass_inf", lambda m, b: _set(m, mass=float("inf")), "mass is not finite"),
    ("lambda_inf", lambda m, b: _set(m, com_lambda2=float("inf")), "com_lambda2 / com_lambda_ang is not finite"),
    ("Kp_nan", lambda m, b: m.cart_Kp.__setitem__(35, float("nan")), "cart_Kp / cart_Kd is not finite"),
    ("Kd_inf", lambda m, b: m.cart_Kd.__setitem__(0, float("-inf")), "cart_Kp / cart_Kd is not finite"),
    ("Jc_null", lambda m, b: _set(b, Jc=None), "Jc is null"),
    ("com_null", lambda m, b: _set(b, com=None), "com is null"),
    ("cart_contact", lambda m, b: _set(m, cart_contact=3), "cart_contact is not a contact"),
    ("B_negative", lambda m, b: _set(b, B=-1), "B is negative"),
]


def test_the_good_arguments_pass():
    _, _, m, b = _good()
    assert fr.host_check(m, b) == (abi.OK, "")


@pytest.mark.parametrize("name,spoil,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(name, spoil, reason):
    _, _, m, b = _good()
    spoil(m, b)
    rc, why = fr.host_check(m, b)
    assert rc == abi.ERR_INVALID and reason in why, (rc, why)


def test_refused_before_anything_is_written():
    case, out, m, b = _good()
    m.wrench_col[0] = 75
    import ctypes as C
    assert fr.lib().force_host_rows(C.byref(m), C.byref(b)) == abi.ERR_INVALID
    assert all((a == fr.SENTINEL).all() for a in out.arrays().values())


# ---- the stand-alone sanitizer program -------------------------------------------------------------------------------------------------
def test_sanitized_program():
    """tests/emu/force_rows_host.cpp with its own main under ASan + UBSan (statically linked runtimes): the three shapes, every
    input array of its exact size on the heap, every destination checked entry by entry"""
    exe = fr.ensure_sanitized()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "force_rows: ok" in r.stdout
