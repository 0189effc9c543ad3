"""Convex collision shapes without a GPU: opensot_amd/csrc/osot_convex.h through osot_shape_distance (the code the producer's lanes
run, on the host), checked by the CERTIFICATE of tests/convex_ref.py -- a feasible pair of witnesses bounds the distance from above,
the separating slab along them from below -- and the certificate itself against a brute force over surface triangles."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import convex_ref as cr
from opensot_amd import abi, kinematics as kin
from oracle import pykin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-10          # the certificate's bound (metres): four orders inside the project's 1e-6 parity rule on dq
MEMBER = 1e-12       # ca in A, cb in B


def _constant(name):
    src = open(os.path.join(ROOT, "opensot_amd", "csrc", "osot_convex.h")).read()
    return float(re.search(r"constexpr \w+ " + name + r" = ([0-9.eE+-]+);", src).group(1))


MAX_ITER = int(_constant("kGjkMaxIter"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return abi.lib()


_CODE = {"capsule": abi.SHAPE_CAPSULE, "box": abi.SHAPE_BOX, "cylinder": abi.SHAPE_CYLINDER, "hull": abi.SHAPE_HULL}


def c_shape(s):
    """(abi.Shape, the array its vertex pointer needs alive)"""
    o = abi.Shape()
    o.kind = _CODE.get(s["kind"], s["kind"]) if isinstance(s["kind"], str) else int(s["kind"])
    for i in range(3):
        o.size[i] = float(np.asarray(s.get("size", np.zeros(3)), float)[i])
    o.radius = float(s.get("radius", 0.0))
    V = np.ascontiguousarray(np.asarray(s.get("verts", np.zeros((0, 3))), float).reshape(-1, 3))
    o.n_vertices = int(s.get("n_vertices", len(V)))
    o.vertices = V.ctypes.data_as(abi.dp) if len(V) else None
    return o, V


def c_pose(pose):
    return np.concatenate([np.asarray(pose[0], float).reshape(9), np.asarray(pose[1], float).reshape(3)])


def distance(lib, A, poseA, B, poseB):
    """-> (rc, dist, ca, cb, iterations)"""
    a, keep_a = c_shape(A)
    b, keep_b = c_shape(B)
    Ta, Tb = c_pose(poseA), c_pose(poseB)
    d, it = C.c_double(np.nan), C.c_int(-1)
    ca, cb = np.full(3, np.nan), np.full(3, np.nan)
    rc = lib.osot_shape_distance(C.byref(a), Ta.ctypes.data_as(abi.dp), C.byref(b), Tb.ctypes.data_as(abi.dp), C.byref(d),
                                 ca.ctypes.data_as(abi.dp), cb.ctypes.data_as(abi.dp), C.byref(it))
    return rc, d.value, ca, cb, it.value


I3, O3 = np.eye(3), np.zeros(3)


def test_certificate_against_brute_force_on_polytopes(lib):
    """the certificate is not trusted unseen: on polytope pairs (segment, box, hull) the certified distance equals the minimum
    over the pairs of surface triangles (closed-form vertex / triangle and edge / edge distances) to 1e-12"""
    rng = np.random.default_rng(101)
    kinds = ("capsule", "box", "hull4", "hull16", "hull32")
    worst = 0.0
    for t in range(40):
        ka, kb = kinds[t % 5], kinds[(t // 5 + t) % 5]
        A, pA, B, pB = cr.random_separated_pair(ka, kb, rng)
        rc, d, ca, cb, it = distance(lib, A, pA, B, pB)
        assert rc == abi.OK and it < MAX_ITER
        cert = cr.certify(A, pA, B, pB, ca, cb)
        bf = cr.brute_force_distance(A, pA, B, pB)
        worst = max(worst, abs(cert["len"] - bf), abs(cert["slab"] - bf))
        assert abs(cert["len"] - bf) <= 1e-12 and abs(cert["slab"] - bf) <= GAP and cert["slab"] <= bf + 1e-12, (ka, kb, cert, bf)
        assert cert["in_a"] <= MEMBER and cert["in_b"] <= MEMBER
    print(f"polytopes: max |certified - brute force| = {worst:.3e}")


def test_certificate_set(lib):
    """every unordered pair of kinds from {sphere, capsule, box, rounded box, cylinder, hull of 4 / 16 / 32 vertices}, 40 random poses
    each (sizes 0.03 - 0.3 m, core separation >= 1 cm): the witnesses are members to 1e-12 and the separating slab along them is within
    1e-10 m of their distance; no case reaches kGjkMaxIter (no case is excluded).
    Measured over the set (host, gcc): largest gap 3.6e-14 m; at most 9 iterations without a cylinder, at most 45 with one."""
    rng = np.random.default_rng(7)
    worst, iters = 0.0, {}
    for ka, kb in itertools.combinations_with_replacement(cr.KINDS, 2):
        for _ in range(40):
            A, pA, B, pB = cr.random_separated_pair(ka, kb, rng)
            rc, d, ca, cb, it = distance(lib, A, pA, B, pB)
            assert rc == abi.OK
            assert 0 <= it < MAX_ITER, (ka, kb, it)
            cert = cr.certify(A, pA, B, pB, ca, cb)
            worst = max(worst, cert["gap"])
            curved = "cylinder" in (ka, kb)
            iters[curved] = max(iters.get(curved, 0), it)
            assert cert["in_a"] <= MEMBER and cert["in_b"] <= MEMBER, (ka, kb, cert)
            assert -1e-12 <= cert["gap"] <= GAP, (ka, kb, cert)
            assert cert["slab"] >= 0.01 - 1e-12
            assert abs(d - (cert["len"] - A["radius"] - B["radius"])) <= 1e-15
    print(f"certificate set: max gap {worst:.3e} m, iterations <= {iters.get(False)} (polytopes / segments), <= {iters.get(True)} (with a cylinder)")


def test_known_answers(lib):
    # two axis-aligned unit boxes 0.5 apart: parallel faces -- the distance is exact, the witnesses (not unique) are members and
    # their difference is the gap vector
    box = dict(kind="box", size=np.full(3, 0.5), radius=0.0)
    rc, d, ca, cb, it = distance(lib, box, (I3, O3), box, (I3, np.array([1.5, 0.0, 0.0])))
    assert rc == abi.OK and d == 0.5 and it < MAX_ITER
    assert cr.violation(box, (I3, O3), ca) == 0.0 and cr.violation(box, (I3, np.array([1.5, 0, 0])), cb) == 0.0
    assert np.abs((ca - cb) - np.array([-0.5, 0.0, 0.0])).max() <= 1e-15
    # a cylinder above a large box face, its axis tilted by theta: distance = plane offset - (h |cos theta| + r sin theta)
    slab = dict(kind="box", size=np.array([5.0, 5.0, 0.5]), radius=0.0)
    r, h, z0 = 0.07, 0.2, 1.1
    cyl = dict(kind="cylinder", size=np.array([r, 0.0, h]), radius=0.0)
    for th in (0.0, 0.3, 1.0, 0.5 * np.pi, 2.0):
        Rx = np.array([[1.0, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])
        rc, d, ca, cb, it = distance(lib, cyl, (Rx, np.array([0.3, -0.2, z0])), slab, (I3, O3))
        want = (z0 - 0.5) - (h * abs(np.cos(th)) + r * np.sin(th))
        assert rc == abi.OK and it < MAX_ITER and abs(d - want) <= 1e-12, (th, d, want)
        assert abs(cb[2] - 0.5) <= 1e-12
    # the rounding radii are subtracted, the witnesses stay on the cores
    rb = dict(kind="box", size=np.full(3, 0.5), radius=0.1)
    sph = dict(kind="capsule", size=O3, radius=0.2)
    rc, d, ca, cb, it = distance(lib, rb, (I3, O3), sph, (I3, np.array([0.0, 2.0, 0.0])))
    assert abs(d - (1.5 - 0.1 - 0.2)) <= 1e-15 and np.abs(ca - [0, 0.5, 0]).max() <= 1e-15 and np.abs(cb - [0, 2.0, 0]).max() <= 1e-15


def _emu_pairs(m, q, with_points=True):
    """the producer's non-CONVEX instantiation through the emulator -> pair_dist [B][P], pair_J [B][P][n], pair_points [B][P][6]"""
    from helpers import emu_lib
    L = emu_lib()
    L.emu_kinematics.argtypes = [C.POINTER(abi.KinDesc), C.POINTER(abi.KinBatch)]
    q = np.ascontiguousarray(q, dtype=np.float64)
    B, n = q.shape
    P = len(m.pairs)
    d = m.desc()
    kb = abi.KinBatch()
    kb.B = B
    kb.q = q.ctypes.data
    pd, pJ, pp = np.zeros((B, P)), np.zeros((B, P, n)), np.full((B, P, 6), np.nan)
    kb.pair_dist = pd.ctypes.data; kb.pair_J = pJ.ctypes.data; kb.pair_J_stride = P * n
    if with_points:
        kb.pair_points = pp.ctypes.data
    env = np.ascontiguousarray(m.env_pose_array())
    if env.size:
        kb.env_pose = env.ctypes.data
    assert L.emu_kinematics(C.byref(d), C.byref(kb)) == 0
    return pd, pJ, pp


def _old_style_model():
    m = kin.humanoid32_pairs(kin.humanoid32())
    m.self_pairs = m.pairs[:4]; m.pairs = m.pairs[:4]; m.pair_names = m.pair_names[:4]
    Rz = lambda a: np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    assert m.add_collision_shape("table", "world", ("box", (0.30, 0.80, 0.04)), (Rz(0.3), (0.33, 0.05, 0.10)))
    assert m.add_collision_shape("ball", "world", ("sphere", 0.08), (np.eye(3), (0.25, -0.30, 0.30)))
    assert m.add_collision_shape("chest_plate", "WaistYaw", ("box", (0.06, 0.20, 0.16)), (Rz(0.1), (0.11, 0.0, 0.14)))
    m.set_links_vs_environment(["Lhand", "Rhand", "Lforearm", "Rforearm"])
    return m


def _segment_pose(e0, e1):
    """world_T_shape of a capsule (axis z, centred) whose axis runs from e0 to e1 -> (pose, half length)"""
    z = e1 - e0
    L = np.linalg.norm(z)
    z = z / L if L > 0 else np.array([0.0, 0.0, 1.0])
    x = np.cross(z, [1.0, 0, 0] if abs(z[0]) < 0.9 else [0, 1.0, 0])
    x /= np.linalg.norm(x)
    return (np.stack([x, np.cross(z, x), z], axis=1), 0.5 * (e0 + e1)), 0.5 * L


def test_emulated_old_style_model_and_capsule_box_both_ways(lib):
    """emu_kinematics runs the non-CONVEX instantiation: an old-style model still matches the restatement, pair_points is filled with
    ca - cb consistent with pair_dist, and binding pair_points changes no other output.  Every capsule / box pair is then run the
    other way as well -- GJK with the capsule declared as a segment core -- and agrees with the closed form to 1e-12."""
    m = _old_style_model()
    rng = np.random.default_rng(31)
    B, P = 5, len(m.pairs)
    q = rng.uniform(-0.8, 0.8, (B, m.n))
    pd, pJ, pp = _emu_pairs(m, q)
    pd0, pJ0, _ = _emu_pairs(m, q, with_points=False)
    assert np.array_equal(pd, pd0) and np.array_equal(pJ, pJ0)
    rad = np.array([p[3] + p[7] for p in m.pairs])
    boxes = 0
    for i in range(B):
        d, Jd = pykin.pair_distances(m, q[i])
        assert np.abs(pd[i] - d).max() < 1e-12 and np.abs(pJ[i] - Jd).max() < 1e-12
        ln = np.linalg.norm(pp[i, :, :3] - pp[i, :, 3:], axis=1)
        assert np.abs(ln - rad - pd[i]).max() <= 1e-15
        fk = pykin.forward(m, q[i])
        env = m.env_pose_array()
        for k, pr in enumerate(m.pairs):
            ex = pr[8] if len(pr) > 8 else {}
            if ex.get("kind", 0) != abi.SHAPE_BOX:
                continue
            ja, a0, a1, ra, jb = pr[:5]
            Rw, pw = fk["Rw"], fk["pw"]
            poseA, hl = _segment_pose(Rw[ja] @ np.asarray(a0, float) + pw[ja], Rw[ja] @ np.asarray(a1, float) + pw[ja])
            Rc, pc = pykin._carrier(m, fk, jb, ex, env)
            poseB = (Rc @ np.asarray(ex["R"], float).reshape(3, 3), pc + Rc @ np.asarray(ex["p"], float))
            cap = dict(kind="capsule", size=np.array([0.0, 0.0, hl]), radius=ra)
            box = dict(kind="box", size=np.asarray(ex["half"], float), radius=pr[7])
            rc, dg, ca, cb, it = distance(lib, cap, poseA, box, poseB)
            assert rc == abi.OK and it < MAX_ITER
            if pd[i, k] + rad[k] > 1e-9:          # (a segment inside the box: both say -r_a - r_b)
                assert abs(dg - pd[i, k]) <= 1e-12, (i, k, dg, pd[i, k])
                boxes += 1
            else:
                assert dg == -rad[k]
    assert boxes >= 20


def test_degenerate_inputs(lib):
    """coincident centres, touching cores and one core inside the other give -r_a - r_b; zero sizes, repeated vertices and a hull of
    one point give finite results under the iteration cap"""
    box = lambda h, r=0.0: dict(kind="box", size=np.full(3, float(h)), radius=r)
    sph = lambda r: dict(kind="capsule", size=O3, radius=r)
    rng = np.random.default_rng(5)
    R = cr.random_rotation(rng)
    V = rng.uniform(-0.2, 0.2, (8, 3))
    hull = dict(kind="hull", verts=V, radius=0.01)
    at = lambda *p: (I3, np.array(p, float))
    overlapping = [
        (box(0.5, 0.1), (R, O3), box(0.3, 0.02), (I3, O3)),                         # coincident centres
        (box(0.5), at(0, 0, 0), box(0.5, 0.05), at(1.0, 0, 0)),                      # touching faces
        (box(0.5), at(0, 0, 0), sph(0.03), at(0.1, -0.2, 0.3)),                      # a point core inside a box
        (dict(kind="cylinder", size=np.array([0.3, 0, 0.3]), radius=0.0), (R, O3), hull, (R.T, np.array([0.01, 0.0, 0.02]))),
        (hull, (R, O3), hull, (R, O3)),
        (sph(0.1), at(1, 2, 3), sph(0.2), at(1, 2, 3)),
    ]
    for A, pA, B, pB in overlapping:
        rc, d, ca, cb, it = distance(lib, A, pA, B, pB)
        assert rc == abi.OK and it < MAX_ITER
        assert d == -A["radius"] - B["radius"], (d, A, B)
        assert np.isfinite(ca).all() and np.array_equal(ca, cb)
    one = dict(kind="hull", verts=np.array([[0.1, 0.2, 0.3]]), radius=0.0)
    dup = dict(kind="hull", verts=np.repeat(V[:3], 4, axis=0), radius=0.0)
    disc = dict(kind="cylinder", size=np.array([0.2, 0.0, 0.0]), radius=0.0)
    needle = dict(kind="cylinder", size=np.array([0.0, 0.0, 0.2]), radius=0.0)
    point = box(0.0)
    far = (R, np.array([0.9, -0.7, 0.8]))
    for A in (one, dup, disc, needle, point):
        for B in (one, dup, disc, needle, point, box(0.2), hull):
            rc, d, ca, cb, it = distance(lib, A, (R.T, O3), B, far)
            assert rc == abi.OK and 0 <= it < MAX_ITER
            assert np.isfinite(d) and np.isfinite(ca).all() and np.isfinite(cb).all()
            cert = cr.certify(A, (R.T, O3), B, far, ca, cb)
            assert cert["in_a"] <= MEMBER and cert["in_b"] <= MEMBER and -1e-12 <= cert["gap"] <= GAP, (A["kind"], B["kind"], cert)
    # known: a point against a point, a point against a box face
    rc, d, ca, cb, it = distance(lib, one, (I3, O3), one, at(1.0, 0, 0))
    assert abs(d - 1.0) <= 1e-15
    rc, d, ca, cb, it = distance(lib, point, at(0, 0, 2.0), box(0.5), at(0, 0, 0))
    assert abs(d - 1.5) <= 1e-15


def test_shape_distance_argument_checks(lib):
    box = dict(kind="box", size=np.full(3, 0.5), radius=0.0)
    ok = (I3, O3)
    away = (I3, np.array([3.0, 0, 0]))

    def refused(A, pA, code, text):
        rc = distance(lib, A, pA, box, away)[0]
        assert rc == code and text in lib.osot_last_error().decode(), (rc, lib.osot_last_error())
        rc = distance(lib, box, away, A, pA)[0]
        assert rc == code and text in lib.osot_last_error().decode()
    refused(dict(box, kind=4), ok, abi.ERR_UNSUPPORTED, "unknown collision shape kind")
    refused(dict(box, kind=-1), ok, abi.ERR_UNSUPPORTED, "unknown collision shape kind")
    refused(dict(box, size=np.array([0.5, -0.1, 0.5])), ok, abi.ERR_INVALID, "sizes must be finite and not negative")
    refused(dict(box, size=np.array([0.5, np.nan, 0.5])), ok, abi.ERR_INVALID, "sizes must be finite and not negative")
    refused(dict(box, size=np.array([np.inf, 0.1, 0.5])), ok, abi.ERR_INVALID, "sizes must be finite and not negative")
    refused(dict(box, radius=-0.01), ok, abi.ERR_INVALID, "rounding radius")
    refused(box, (1.001 * I3, O3), abi.ERR_INVALID, "not orthonormal")
    refused(box, (I3, np.array([0.0, np.nan, 0.0])), abi.ERR_INVALID, "pose must be finite")
    hull = dict(kind="hull", verts=np.zeros((33, 3)), radius=0.0)
    refused(hull, ok, abi.ERR_INVALID, "1 .. 32 vertices")
    refused(dict(kind="hull", verts=np.zeros((0, 3)), radius=0.0), ok, abi.ERR_INVALID, "1 .. 32 vertices")
    refused(dict(kind="hull", verts=np.array([[0.0, np.inf, 0.0]]), radius=0.0), ok, abi.ERR_INVALID, "vertices must be finite")
    assert lib.osot_shape_distance(None, None, None, None, None, None, None, None) == abi.ERR_INVALID
    # every output is optional
    a, _ = c_shape(box)
    T0, T1 = c_pose(ok), c_pose(away)
    assert lib.osot_shape_distance(C.byref(a), T0.ctypes.data_as(abi.dp), C.byref(a), T1.ctypes.data_as(abi.dp), None, None, None, None) == abi.OK


def _convex_model():
    m = kin.humanoid32_pairs(kin.humanoid32())
    m.self_pairs = m.pairs[:2]; m.pairs = m.pairs[:2]; m.pair_names = m.pair_names[:2]
    nm = m.names.index
    rng = np.random.default_rng(3)
    m.link_shapes["Rforearm_box"] = dict(joint=nm("RElbj"), kind="box", half=(0.03, 0.03, 0.08), p=(0, 0, -0.08))
    m.link_shapes["torso_hull"] = dict(joint="WaistYaw", kind="hull", verts=rng.uniform(-0.1, 0.1, (16, 3)), p=(0, 0, 0.14), r=0.01)
    assert m.add_collision_shape("wheel", "world", ("cylinder", 0.10, 0.15), (np.eye(3), (0.4, 0.0, 0.2)))
    assert m.add_collision_shape("rock", "world", ("convex", rng.uniform(-0.1, 0.1, (8, 3))), (np.eye(3), (0.4, 0.3, 0.2)))
    m.self_pairs.append(m.link_pair("Rforearm_box", "torso_hull"))
    m.pair_names.append(("Rforearm_box", "torso_hull"))
    m.set_links_vs_environment(["Rforearm_box", "Lhand"])
    return m


def test_python_model_and_descriptor_checks(lib):
    """KinModel takes cylinders and convex vertex sets, pairs any link shape with any other shape and fills the appended descriptor
    fields; osot_kin_create refuses a bad descriptor with its reason before it touches a device"""
    m = kin.humanoid32()
    with pytest.raises(ValueError):
        m.add_collision_shape("m", "world", ("mesh", "file.stl"))
    with pytest.raises(ValueError):
        m.add_collision_shape("m", "world", ("convex", np.zeros((33, 3))))
    m = _convex_model()
    d = m.desc()
    assert d.n_pairs == 2 + 1 + 4 and d.n_hull_vertices == 16 + 8
    k = 2      # box (link) against hull (link)
    assert (d.pair_kind_a[k], d.pair_kind[k]) == (abi.SHAPE_BOX, abi.SHAPE_HULL) and list(d.pair_hull[k][1]) == [0, 16]
    assert list(d.pair_size_a[k]) == [0.03, 0.03, 0.08] and d.pair_radius[k][1] == 0.01 and d.pair_joint[k][1] == m.names.index("WaistYaw")
    assert [(d.pair_kind_a[p], d.pair_kind[p], d.pair_env[p]) for p in range(3, 7)] == \
        [(abi.SHAPE_BOX, abi.SHAPE_CYLINDER, 1), (abi.SHAPE_BOX, abi.SHAPE_HULL, 2), (abi.SHAPE_CAPSULE, abi.SHAPE_CYLINDER, 1),
         (abi.SHAPE_CAPSULE, abi.SHAPE_HULL, 2)]
    assert list(d.pair_box[3]) == [0.15, 0.0, 0.05] and list(d.pair_hull[4][1]) == [16, 8] and list(d.pair_hull[6][1]) == [16, 8]
    assert all(d.pair_kind_a[p] == 0 and d.pair_kind[p] == 0 for p in range(2))
    h = C.c_void_p()

    def refused(change, code, text):
        d = m.desc()
        change(d)
        rc = lib.osot_kin_create(C.byref(d), 0, C.byref(h))
        assert rc == code and text in lib.osot_last_error().decode(), (rc, lib.osot_last_error())

    def setv(arr, idx, val):
        def f(d):
            a = getattr(d, arr)
            for i in idx[:-1]:
                a = a[i]
            a[idx[-1]] = val
        return f
    refused(setv("pair_kind", (3,), 4), abi.ERR_UNSUPPORTED, "unknown collision shape kind")
    refused(setv("pair_kind_a", (3,), 7), abi.ERR_UNSUPPORTED, "unknown collision shape kind")
    refused(setv("pair_kind_a", (0,), -1), abi.ERR_UNSUPPORTED, "unknown collision shape kind")
    refused(setv("pair_hull", (4, 1, 0), 17), abi.ERR_INVALID, "hull vertex range outside n_hull_vertices")
    refused(setv("pair_hull", (4, 1, 0), -1), abi.ERR_INVALID, "hull vertex range outside n_hull_vertices")
    refused(setv("pair_hull", (2, 1, 1), 33), abi.ERR_INVALID, "1 .. 32 vertices")
    refused(setv("pair_hull", (2, 1, 1), 0), abi.ERR_INVALID, "1 .. 32 vertices")
    refused(lambda d: setattr(d, "n_hull_vertices", 257), abi.ERR_INVALID, "hull vertex count out of range")
    refused(setv("pair_size_a", (3, 1), -0.03), abi.ERR_INVALID, "sizes must be finite and not negative")
    refused(setv("pair_size_a", (2, 2), float("nan")), abi.ERR_INVALID, "sizes must be finite and not negative")
    refused(setv("pair_box", (3, 0), float("inf")), abi.ERR_INVALID, "sizes must be finite and not negative")
    refused(setv("pair_shape_R_a", (3, 0), 1.0001), abi.ERR_INVALID, "not orthonormal")
    refused(setv("pair_shape_R", (5, 4), 0.5), abi.ERR_INVALID, "not orthonormal")
    refused(setv("hull_vertex", (3, 1), float("nan")), abi.ERR_INVALID, "hull vertices must be finite")
