"""The tree producers at the limits their header declares (opensot_amd/csrc/osot_kin.h: any tree of 1 .. 64 joints, revolute or
prismatic, 8 frames, 32 pairs, 16 points, 16 environment shapes), CPU side -- the trees and the geometry rig of tests/tree_cases.py:

  1. the REFERENCE first: oracle/pykin.py against central differences on trees with prismatic joints in mid-chain;
  2. the kinematics kernel body through the host emulator against it: every size, topology, with and without the frame options;
  3. the host build of the dynamics kernel against tests/dyn_ref.py and tests/momentum_ref.py on the same trees;
  4. the descriptor check of osot_kin_create at every declared maximum and one beyond;
  5. the closed-form collision pairs at parallel axes, abutting ends, faces, edges and corners, judged by the certificate of
     tests/convex_ref.py.
tests/test_tree_limits_gpu.py runs the same cases on the device, where the lanes really run together.

Measured here (worst over all cases): emulated kinematics against pykin 7.5e-15 (frame Jacobian, chain of 63), positions 2.7e-15;
dynamics 6.4e-15 relative (star of 64), momentum 2.2e-14 (star of 63); the rig: certificate gap 4.6e-15 m (the restatement's own witnesses:
3.9e-14), against pykin 8.9e-16 (distance), 5.6e-14 (rows, where the witnesses are the same: 21 of the 4170 pairs, all flat by
construction, hold two different certified minimisers).  The closed form as it was before its end-point projections fails 17 of the
rig's in-plane cases, by up to 5.0e-9 m"""
import ctypes as C

import numpy as np
import pytest

from opensot_amd import abi
from oracle import pykin

import dyn_ref
import momentum_ref
import test_dynamics_host as tdh
import test_momentum_host as tmh
import tree_cases as tc
from test_dynamics_host import lib      # noqa: F401  (the fixture: the product library, built where it is missing)


# ---- 1. the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,topology", [(33, "random"), (64, "chain")])
def test_restatement_matches_finite_differences_on_the_trees(n, topology):
    """pykin.forward, pykin.pair_distances and pykin.relative against central differences (h = 1e-6) at the bounds of
    tests/test_kinematics.py: 1e-8 for the frames and the centre of mass, 5e-8 for the pairs and the relative frames.  A pair's row is
    compared where its axis points are more than 1e-3 m apart (closer, the unit normal amplifies the differences' round-off)."""
    m = tc.tree_case(n, topology)
    assert any(m.jtype[j] == abi.JOINT_PRISMATIC and m.parent[j] >= 0 for j in range(n))
    q = tc.draw_q(m, 1)[0]
    h = 1e-6
    o = pykin.forward(m, q)
    step = [(pykin.forward(m, q + h * e), pykin.forward(m, q - h * e)) for e in np.eye(n)]      # shared by all three comparisons
    Jc = np.array([(a["com"] - b["com"]) / (2 * h) for a, b in step]).T
    assert np.abs(Jc - o["Jcom"]).max() < 1e-8
    for f in range(len(m.frames)):                # as test_kinematics._fd_jacobians: d p, and d R R' = [w]x
        Jf = np.zeros((6, n))
        for j, (a, b) in enumerate(step):
            Jf[:3, j] = (a["frame_p"][f] - b["frame_p"][f]) / (2 * h)
            S = (a["frame_R"][f] - b["frame_R"][f]) / (2 * h) @ o["frame_R"][f].T
            Jf[3:, j] = [S[2, 1], S[0, 2], S[1, 0]]
        assert np.abs(Jf - o["J"][f]).max() < 1e-8
    # the pairs
    d, J = pykin.pair_distances(m, q, fk=o)
    Jfd = np.array([(pykin.pair_distances(m, q + h * e, fk=a)[0] - pykin.pair_distances(m, q - h * e, fk=b)[0]) / (2 * h)
                    for e, (a, b) in zip(np.eye(n), step)]).T
    apart = d + np.array([pr[3] + pr[7] for pr in m.pairs]) > 1e-3
    assert apart.sum() >= 0.75 * len(m.pairs)
    assert np.abs(J - Jfd)[apart].max() < 5e-8
    # the relative frames of with_options: frame f relative to g
    mo = tc.with_options(m)
    for f, g in mo.frame_base.items():
        R, p, Jr = pykin.relative(o, f, g)
        Jfd = np.zeros((6, n))
        for j, (a, b) in enumerate(step):
            Ra, pa, _ = pykin.relative(a, f, g)
            Rb, pb, _ = pykin.relative(b, f, g)
            Jfd[:3, j] = (pa - pb) / (2 * h)
            S = (Ra - Rb) / (2 * h) @ R.T
            Jfd[3:, j] = [S[2, 1], S[0, 2], S[1, 0]]
        assert np.abs(Jr - Jfd).max() < 5e-8, (f, g)


# ---- 2. the emulated kinematics kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", tc.TOPOLOGIES)
@pytest.mark.parametrize("n", tc.SIZES)
def test_emulated_kinematics_on_the_trees(n, topology):
    """every output of the kernel body (poses, frame Jacobians, CoM and its Jacobian, contact points, pair distances, rows and
    witness points) against the restatement, with and without the frame options, with and without the pair stage; B = 3: the
    packed kernel (n <= 32) runs two different robots in one wavefront and leaves the last half idle"""
    base = tc.tree_case(n, topology)
    q = tc.draw_q(base, 3)
    for m in (base, tc.with_options(base)):
        ref = tc.reference(m, q)
        bound = tc.HOST_BOUND if m is base else tc.HOST_BOUND_OPTIONS
        w = tc.compare(tc.emu_kin(m, q), m, ref, bound)
        tc.compare(tc.emu_kin(m, q, pairs=False), m, ref, bound, pairs=False)
        print(f"n={n} {topology} options={m is not base}: " + " ".join(f"{k} {v:.1e}" for k, v in w.items()))
    # what the options must do where a wrong lane would show: frame 0 keeps the column of joint n - 1 alone
    if n > 1:
        A = tc.emu_kin(tc.with_options(base), q)["A"]
        assert np.abs(A[:3, 0:6, :n - 1]).max() == 0.0 and np.abs(A[:3, 0:6, n - 1]).max() > 0.0


def test_tree_cases_are_what_they_say():
    for n in tc.SIZES:
        for t in tc.TOPOLOGIES:
            m = tc.tree_case(n, t)
            assert m.n == n and m.frames[0][1] == n - 1 and len(m.points) == abi.KIN_MAX_POINTS and m.points[0][0] == n - 1
            assert len(m.frames) == min(abi.KIN_MAX_FRAMES, 2 * n + 2)
            assert len(m.pairs) == (abi.KIN_MAX_PAIRS if n >= 2 else 0) and (n < 2 or m.pairs[0][0] == n - 1)
            assert np.abs(np.linalg.norm(m.axis, axis=1) - 1.0).max() < 1e-15
            if n > 3:
                assert any(m.jtype[j] == abi.JOINT_PRISMATIC and m.parent[j] >= 0 for j in range(n))
    depth = lambda m: max(bin(a).count("1") for a in _anc(m))
    assert depth(tc.tree_case(64, "chain")) == 64 and depth(tc.tree_case(64, "star")) == 2
    m = tc.tree_case(64, "interleaved")
    assert m.parent[:4] == [-1, -1, 0, 1] and depth(m) == 32
    assert tc.tree_case(33, "forest").parent[:3] == [-1, -1, -1]
    d = tc.with_options(tc.tree_case(64, "random")).desc()
    assert d.frame_col_mask[0] == 1 << 63 and d.frame_col_mask[1] == (1 << 64) - 1 and (d.com_col_mask >> 63) & 1
    assert [d.frame_base[f] for f in range(8)] == [0, 0, 2, 1, 8, 7, 0, 0] and [d.frame_body[f] for f in range(4)] == [1, 0, 1, 1]


def _anc(m):
    anc = []
    for j in range(m.n):
        anc.append((1 << j) | (anc[m.parent[j]] if m.parent[j] >= 0 else 0))
    return anc


# ---- 3. the host build of the dynamics kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", tc.TOPOLOGIES)
@pytest.mark.parametrize("n", tc.SIZES)
def test_host_dynamics_on_the_trees(n, topology):
    """both instantiations (without and with the centroidal momentum outputs) against the restatements, at the constants of
    tests/test_dynamics_host.py and tests/test_momentum_host.py"""
    m = tc.tree_case(n, topology)
    B = 2
    q, qd = tc.draw_q(m, B), tc.draw_qdot(m, B)
    ref, mref = dyn_ref.batch(m, q, qd, tdh.GRAVITY), momentum_ref.batch(m, q, qd)
    plain, mom = tdh.emu_dynamics(m, q, qd), tmh.emu_momentum(m, q, qd)
    worst = 0.0
    for got in (plain, mom):
        for k in ("M", "h", "jdq", "com_jdq"):
            d = tdh.rel(got[k], ref[k])
            worst = max(worst, d)
            assert d <= tdh.PARITY_TOL, (k, d)
        for i in range(B):
            assert np.array_equal(got["M"][i], got["M"][i].T)
            np.linalg.cholesky(got["M"][i])
    for k in ("M", "h", "jdq", "com_jdq"):
        assert np.array_equal(plain[k], mom[k]), k                # the existing outputs do not see the new ones
    wm = 0.0
    # (the angular rows of a lone prismatic joint are zero -- round-off against round-off: their scale is at least a millimetre of
    #  lever arm on the linear rows)
    floor = 1e-3 * np.abs(mref["cmm"][:, :3]).max()
    for k, want in (("cmm_lin", mref["cmm"][:, :3]), ("cmm_ang", mref["cmm"][:, 3:]), ("momentum", mref["momentum"])):
        d = np.abs(mom[k] - want).max() / max(np.abs(want).max(), floor)
        wm = max(wm, d)
        assert d <= tmh.PARITY_TOL, (k, d)
    assert tdh.rel(mom["momentum"], mref["momentum_links"]) <= tmh.PARITY_TOL
    g0 = tdh.emu_dynamics(m, q, None)                             # qdot = NULL: the gravity term alone
    assert tdh.rel(g0["h"], dyn_ref.batch(m, q, None, tdh.GRAVITY)["h"]) <= tdh.PARITY_TOL and np.all(g0["jdq"] == 0.0)
    print(f"n={n} {topology}: dynamics {worst:.1e} momentum {wm:.1e}")


# ---- 4. the declared limits ------------------------------------------------------------------------------------------------------------------
def full_model():
    """every declared maximum at once: 64 joints, 8 frames with options, 16 points, 16 environment shapes, 32 pairs (16 of them
    link / environment pairs, one per environment shape)"""
    from opensot_amd import kinematics as kin
    m = tc.with_options(tc.tree_case(64, "random"))
    m.pairs = list(m.pairs[:16]); m.self_pairs = list(m.pairs)
    m.link_shapes = {"last": (63, (0.0, 0.0, -0.05), (0.0, 0.0, 0.05), 0.02)}
    rng = np.random.default_rng(2)
    for e in range(abi.KIN_MAX_ENV):
        shape = ("box", (0.1, 0.2, 0.3)) if e % 2 else ("capsule", 0.2, 0.03)
        assert m.add_collision_shape(f"e{e}", "world", shape, (tc.cr.random_rotation(rng), rng.uniform(-2.0, 2.0, 3)))
    m.set_links_vs_environment(["last"])
    return m


def test_kin_create_accepts_the_maxima_and_refuses_one_more(lib):
    m = full_model()
    d = m.desc()
    assert (d.n, d.n_frames, d.n_pairs, d.n_points, d.n_env) == (64, 8, 32, 16, 16)
    h = C.c_void_p()
    rc = lib.osot_kin_create(C.byref(d), 0, C.byref(h))
    # the descriptor passes every check; without a device the call ends at the device (tests/test_tree_limits_gpu.py runs this model)
    assert rc in (abi.OK, abi.ERR_HIP), (rc, lib.osot_last_error())
    if rc == abi.OK:
        assert lib.osot_kin_destroy(h) == abi.OK
    for field, value, text in (("n", 65, b"joint count"), ("n", 0, b"joint count"), ("n_frames", 9, b"frame count"),
                               ("n_pairs", 33, b"pair count"), ("n_points", 17, b"contact point count"), ("n_env", 17, b"environment shape count")):
        d = m.desc()
        setattr(d, field, value)
        h = C.c_void_p()
        assert lib.osot_kin_create(C.byref(d), 0, C.byref(h)) == abi.ERR_INVALID, field
        msg = lib.osot_last_error()
        assert msg and text in msg and not h.value, (field, msg)
    # the emulated kernel on the full model, every output bound
    q = tc.draw_q(m, 2)
    env = m.env_pose_array()
    w = tc.compare(tc.emu_kin(m, q, env_pose=env), m, tc.reference(m, q, env_pose=env), tc.HOST_BOUND_OPTIONS)
    print("full model: " + " ".join(f"{k} {v:.1e}" for k, v in w.items()))


# ---- 5. the closed-form geometry rig ----------------------------------------------------------------------------------------------------------
def test_rig_reference_passes_its_own_certificate():
    """the restatement's two closed forms (pykin.closest_segment_points, pykin.segment_box_closest) on the rig's cases, judged by the
    same certificate: what the kernel is compared with is right where the kernel is asked to be"""
    from test_convex_shapes_host import GAP, MEMBER
    import convex_ref as cr
    rig = tc.rig()
    worst = 0.0
    for i in range(rig.B):
        for k in range(6):
            A, pA, Bs, pB = rig.pair_geometry(i, k)
            ca, cb = rig.reference_witnesses(i, k)
            if rig.coincident[i, k]:
                assert np.linalg.norm(ca - cb) <= 1e-12
                continue
            cert = cr.certify(A, pA, Bs, pB, ca, cb)
            worst = max(worst, cert["gap"])
            assert cert["in_a"] <= MEMBER and cert["in_b"] <= MEMBER and -1e-12 <= cert["gap"] <= GAP, (rig.names[i], k, cert)
    print(f"restatement on the rig: largest certificate gap {worst:.1e} m")


def test_emulated_rig():
    """the kernel body on every case of the rig, one batch instance each: certificate, pair_dist against the witnesses, distance and
    row against the restatement, and the coincident witnesses exactly where the cases put them"""
    rig = tc.rig()
    assert rig.B == rig.n_capsule + 14 + 300 and rig.n_capsule == 3 * rig.n_capsule_base == 3 * 127
    assert int(rig.coincident.sum()) == RIG_COINCIDENT
    got = tc.emu_kin(rig.model, rig.q, env_pose=rig.env)
    w = rig.check(got["pd"][:rig.B], got["pJ"][:rig.B, :6], got["pp"][:rig.B])
    assert (got["pJ"][:, 6] == tc.CANARY).all() and (got["pd"][rig.B] == tc.CANARY).all()
    print("emulated rig: " + " ".join(f"{k} {v:.1e}" for k, v in w.items()))


# the (instance, pair) entries of the rig whose witnesses coincide by construction: 3 crossing axes, the segment along an edge, 2
# segments through the box, and the 6 moved copies of the crossing axes (every capsule case is moved twice).  The only exclusion of
# the certificate, pinned here.
RIG_COINCIDENT = 12
