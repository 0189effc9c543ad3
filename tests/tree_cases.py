"""tests/tree_cases.py -- TEST INFRASTRUCTURE ONLY (numpy): the trees and the geometry rig that put the tree producers
(opensot_amd/csrc/osot_kin.h: kin_instance, the body of osot_kin_kernel and the first stage of the dynamics, posture-gradient and
fused control-cycle kernels) at the limits their header promises, shared by tests/test_tree_limits_host.py (the host emulation) and
tests/test_tree_limits_gpu.py (the device).

  tree_case(n, topology, seed)   a random tree of 1 .. 64 joints: chain (depth n), star, random, interleaved (index order is not the
                                 depth-first order, two roots), forest (three roots); about 30 % prismatic joints in mid-chain, unit
                                 axes in random directions under random R0, frames / pairs / points up to the declared maxima with
                                 frame 0, one pair and one point on joint n - 1 (the last busy lane)
  with_options(m)                BODY frames, active-joint masks (only joint n - 1; every joint: bit 63 at n = 64; every third joint
                                 removed), a CoM mask, relative base frames
  reference(m, q)                oracle/pykin.py (with test_kinematics._expected_relative for the options) for every output
  output_shapes / emu_kin / compare   one layout of every output of the producer with a 7.0 canary row behind every block and a canary
                                 instance behind the batch, the emulator's run into it, and the comparison with the reference
  Rig                            the closed-form collision pairs (capsule / capsule, capsule / sphere, capsule / box) at the poses
                                 where such code goes wrong, one batch instance per case, judged by the certificate of
                                 tests/convex_ref.py

Positions stay within a few metres (p0 ~ N(0, 0.1 m) per coordinate: a chain of 64 wanders about 1.4 m, at worst 11 m), so the
project's absolute bounds keep their meaning."""
import ctypes as C

import numpy as np

from opensot_amd import abi, kinematics as kin
from oracle import pykin

import convex_ref as cr

SIZES = (1, 2, 3, 31, 32, 33, 63, 64)
TOPOLOGIES = ("chain", "star", "random", "interleaved", "forest")
CANARY = 7.0


# ---- 1. the trees ---------------------------------------------------------------------------------------------------------------------
def parents(n, topology, rng):
    if topology == "chain":
        return [j - 1 for j in range(n)]
    if topology == "star":
        return [-1] + [0] * (n - 1)
    if topology == "random":
        return [-1] + [int(rng.integers(max(0, j - 5), j)) for j in range(1, n)]
    if topology == "interleaved":            # two chains, even and odd joints: siblings and cousins alternate in index order
        return [j - 2 if j >= 2 else -1 for j in range(n)]
    if topology == "forest":                 # three roots, the rest on any of the five joints before them
        return [-1 if j < 3 else int(rng.integers(max(0, j - 5), j)) for j in range(n)]
    raise KeyError(topology)


def tree_case(n, topology, seed=0):
    """the KinModel of a random tree (module docstring); the same arguments give the same model"""
    rng = np.random.default_rng([n, TOPOLOGIES.index(topology), seed])
    R, P = abi.JOINT_REVOLUTE, abi.JOINT_PRISMATIC
    parent = parents(n, topology, rng)
    jtype = [P if rng.uniform() < 0.3 else R for _ in range(n)]
    inner = [j for j in range(n) if parent[j] >= 0]
    if inner and not any(jtype[j] == P for j in inner):        # never only the roots: a prismatic joint under a rotated parent
        jtype[inner[len(inner) // 2]] = P
    if n >= 2 and all(t == P for t in jtype):
        jtype[0] = R
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    m = kin.KinModel(parent=parent, jtype=jtype, axis=ax, R0=np.array([cr.random_rotation(rng) for _ in range(n)]),
                     p0=rng.normal(0.0, 0.1, (n, 3)), mass=rng.uniform(0.1, 2.0, n), com=rng.normal(0.0, 0.05, (n, 3)),
                     names=[f"j{j}" for j in range(n)])
    from test_dynamics_host import random_inertia
    m.inertia = random_inertia(n, rng)
    F = min(abi.KIN_MAX_FRAMES, 2 * n + 2)
    where = [n - 1] + [int(rng.integers(0, n)) for _ in range(F - 1)]
    m.frames = [(f"f{f}", where[f], cr.random_rotation(rng), tuple(rng.normal(0.0, 0.1, 3))) for f in range(F)]
    if n >= 2:
        for k in range(abi.KIN_MAX_PAIRS):
            ja = n - 1 if k == 0 else int(rng.integers(0, n))
            jb = int(rng.integers(0, n - 1))
            jb += jb >= ja                                   # another joint
            ends = rng.normal(0.0, 0.08, (2, 2, 3))
            for sd in range(2):
                if rng.uniform() < 0.25:
                    ends[sd, 1] = ends[sd, 0]                # a sphere
            ra, rb = rng.uniform(0.01, 0.05, 2)
            m.pairs.append((ja, tuple(ends[0, 0]), tuple(ends[0, 1]), float(ra), jb, tuple(ends[1, 0]), tuple(ends[1, 1]), float(rb)))
    for i in range(abi.KIN_MAX_POINTS):
        m.add_point(n - 1 if i == 0 else int(rng.integers(0, n)), rng.normal(0.0, 0.1, 3))
    return m


def with_options(m):
    """the same tree with every frame option at once (a new model; the frames, pairs and points are shared, read-only)"""
    import copy
    o = copy.copy(m)
    n, F = m.n, len(m.frames)
    o.frame_body = {0: True, 2: True, 3: True}
    o.frame_active_joints = {0: [n - 1], 1: list(range(n)), 3: [j for j in range(n) if j % 3 != 2]}
    o.com_active_joints = sorted({j for j in range(n) if j % 2 == 0} | {n - 1})
    # a base frame has no base of its own (test_kinematics._relative_model): 1 and 0 serve, with outputs and options of their own,
    # and in the larger models F - 1 and 6
    o.frame_base = {2: 1, 3: 0}
    if F >= 6:
        o.frame_base[4] = F - 1
    if F == abi.KIN_MAX_FRAMES:
        o.frame_base[5] = 6
    return o


def draw_q(m, B, seed=0):
    """B postures from clearly different ranges (revolute: 0.8 rad wide around -1.0, 0.9, -0.3, 1.4, 0.2, ...; prismatic +-0.3 m
    around a tenth of that): two robots that share a packed wavefront are not alike"""
    rng = np.random.default_rng([m.n, seed, 77])
    centre = np.array([-1.0, 0.9, -0.3, 1.4, 0.2, -1.6, 0.6, 1.1])[np.arange(B) % 8]
    rev = np.array(m.jtype) == abi.JOINT_REVOLUTE
    q = np.where(rev[None], centre[:, None] + rng.uniform(-0.4, 0.4, (B, m.n)), 0.1 * centre[:, None] + rng.uniform(-0.3, 0.3, (B, m.n)))
    return np.ascontiguousarray(q)


def draw_qdot(m, B, seed=0):
    return np.ascontiguousarray(np.random.default_rng([m.n, seed, 78]).uniform(-2.0, 2.0, (B, m.n)))


# ---- 2. reference, output layout, comparison ---------------------------------------------------------------------------------------------
def reference(m, q, env_pose=None):
    """per instance: dict(R [F][3][3], p [F][3], J [F][6][n], com, Jcom, points, d [P], Jd [P][n]) from oracle/pykin.py"""
    from test_kinematics import _expected_relative
    out = []
    for i in range(len(q)):
        o = pykin.forward(m, q[i])
        r = dict(R=[], p=[], J=[], com=o["com"], points=m.points_world(q[i]))
        for f in range(len(m.frames)):
            R, p, J = _expected_relative(m, o, f)
            r["R"].append(R); r["p"].append(p); r["J"].append(J)
        Jc = o["Jcom"].copy()
        if m.com_active_joints is not None:
            keep = np.zeros(m.n, dtype=bool); keep[m.com_active_joints] = True
            Jc[:, ~keep] = 0.0
        r["Jcom"] = Jc
        if m.pairs:
            E = None if env_pose is None else (env_pose[i] if np.ndim(env_pose) == 3 else env_pose)
            r["d"], r["Jd"] = pykin.pair_distances(m, q[i], fk=o, env_pose=E)
        out.append(r)
    return out


def output_shapes(m, B):
    """name -> shape of every output array: one canary instance behind the batch, one canary row behind every block of rows"""
    n, F, P, NP = m.n, len(m.frames), len(m.pairs), len(m.points)
    s = dict(poses=(F, B + 1, 12), A=(B + 1, 6 * F + 3 + 1, n), com=(B + 1, 3), points=(B + 1, max(NP, 1), 3))
    if P:
        s.update(pd=(B + 1, P), pJ=(B + 1, P + 1, n), pp=(B + 1, P, 6))
    return s


def emu_kin(m, q, env_pose=None, pairs=True):
    """the kinematics kernel body through the host emulator with EVERY output bound (pairs=False: without the pair outputs, the
    instantiation without stage 5) -> dict of arrays in the layout of output_shapes"""
    from helpers import emu_lib
    L = emu_lib()
    L.emu_kinematics.argtypes = [C.POINTER(abi.KinDesc), C.POINTER(abi.KinBatch)]
    q = np.ascontiguousarray(q, dtype=np.float64)
    B, n = q.shape
    F, P = len(m.frames), len(m.pairs)
    out = {k: np.full(s, CANARY) for k, s in output_shapes(m, B).items()}
    d, kb = m.desc(), abi.KinBatch()
    kb.B, kb.q = B, q.ctypes.data
    rows = out["A"].shape[1]
    for f in range(F):
        kb.frame_pose[f] = out["poses"][f].ctypes.data
        kb.frame_J[f] = out["A"].ctypes.data + 8 * 6 * f * n
        kb.frame_J_stride[f] = rows * n
    kb.com = out["com"].ctypes.data
    kb.com_J, kb.com_J_stride = out["A"].ctypes.data + 8 * 6 * F * n, rows * n
    if m.points:
        kb.points = out["points"].ctypes.data
    if P and pairs:
        kb.pair_dist, kb.pair_points = out["pd"].ctypes.data, out["pp"].ctypes.data
        kb.pair_J, kb.pair_J_stride = out["pJ"].ctypes.data, (P + 1) * n
        if env_pose is not None:
            env_pose = np.ascontiguousarray(env_pose, dtype=np.float64)
            kb.env_pose = env_pose.ctypes.data
            kb.env_pose_stride = env_pose.shape[-2] * 12 if env_pose.ndim == 3 else 0
    assert L.emu_kinematics(C.byref(d), C.byref(kb)) == abi.OK
    return out


# the project's absolute bound on the device (tests/test_kinematics.py: the relative frames, the environment pairs)
DEVICE_BOUND = dict(R=1e-12, p=1e-12, J=1e-12, com=1e-12, Jcom=1e-12, points=1e-12, d=1e-12, Jd=1e-12)
# the emulated tests' own bounds (tests/test_kinematics.py): test_emulated_kernel_matches_restatement and
# test_emulated_pair_distances_match_restatement for world frames, test_emulated_relative_base_frames for a model with relative bases
HOST_BOUND = dict(R=1e-14, p=1e-14, J=1e-13, com=1e-14, Jcom=1e-14, points=1e-14, d=1e-14, Jd=1e-13)
HOST_BOUND_OPTIONS = dict(HOST_BOUND, R=1e-13, p=1e-13, J=1e-12)


def compare(got, m, ref, bound, pairs=True):
    """every output of a run (layout of output_shapes) against reference(): asserts the bound per quantity and the canaries; returns
    the worst absolute deviation per quantity"""
    B, n, F, P, NP = len(ref), m.n, len(m.frames), len(m.pairs), len(m.points)
    w = dict.fromkeys(bound, 0.0)
    up = lambda k, a, b: w.__setitem__(k, max(w[k], float(np.abs(np.asarray(a) - np.asarray(b)).max()) if np.size(b) else 0.0))
    for i, r in enumerate(ref):
        for f in range(F):
            up("R", got["poses"][f][i][:9].reshape(3, 3), r["R"][f])
            up("p", got["poses"][f][i][9:], r["p"][f])
            up("J", got["A"][i, 6 * f:6 * f + 6], r["J"][f])
        up("com", got["com"][i], r["com"])
        up("Jcom", got["A"][i, 6 * F:6 * F + 3], r["Jcom"])
        if NP:
            up("points", got["points"][i, :NP], r["points"])
        if P and pairs:
            up("d", got["pd"][i], r["d"])
            up("Jd", got["pJ"][i, :P], r["Jd"])
            ln = np.linalg.norm(got["pp"][i, :, :3] - got["pp"][i, :, 3:], axis=1)
            rad = np.array([pr[3] + pr[7] for pr in m.pairs])
            assert np.abs(ln - rad - got["pd"][i]).max() <= 1e-15, "pair_points and pair_dist disagree"
    for k in w:
        assert w[k] <= bound[k], (k, w[k], bound[k])
    assert np.isfinite(got["A"]).all()
    # canaries: the row behind the blocks, the instance behind the batch -- and the pair outputs that were not bound
    assert (got["A"][:, 6 * F + 3] == CANARY).all() and (got["A"][B] == CANARY).all()
    assert (got["poses"][:, B] == CANARY).all() and (got["com"][B] == CANARY).all() and (got["points"][B] == CANARY).all()
    if not NP:
        assert (got["points"] == CANARY).all()
    if P:
        if pairs:
            assert (got["pJ"][:, P] == CANARY).all() and (got["pJ"][B] == CANARY).all()
            assert (got["pd"][B] == CANARY).all() and (got["pp"][B] == CANARY).all()
        else:
            assert all((got[k] == CANARY).all() for k in ("pd", "pJ", "pp"))
    return w


# ---- 3. the closed-form geometry rig ---------------------------------------------------------------------------------------------------
def _rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _frame_with_z(d):
    """a rotation whose third column is exactly d (a unit vector)"""
    d = np.asarray(d, float)
    x = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(d, x), d], axis=1)


def _clips_box(s0, s1, half):
    """does the segment meet the box [-half, half]?  Slab clipping: the parameter interval inside every pair of faces"""
    t0, t1 = 0.0, 1.0
    for i in range(3):
        v = s1[i] - s0[i]
        if v == 0.0:
            if abs(s0[i]) > half[i]:
                return False
            continue
        a, b = (-half[i] - s0[i]) / v, (half[i] - s0[i]) / v
        t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return t0 <= t1


class Rig:
    """One model: a six-joint floating base (x, y, z, roll, pitch, yaw) carrying a 1 m capsule on its z axis, and a second root
    (a skew slider and a hinge) carrying a sphere; both paired with a world capsule (0.5 m), a world sphere and a world box through
    add_collision_shape / set_links_vs_environment: six pairs per instance, in the order
        0 capsule / world capsule   1 capsule / world sphere   2 capsule / world box
        3 sphere / world capsule    4 sphere / world sphere    5 sphere / world box.
    Every case is one batch instance: q places the link shapes (q = 0: the link frames are the identity, exactly) and the
    per-instance env_pose [B][3][12] places the world shapes RELATIVE to the link shape of the case's target pair; the world shapes
    the case does not speak of are parked about 2 m away at generic poses.  coincident [B][6]: the (instance, pair) entries whose
    witnesses coincide BY CONSTRUCTION (crossing axes, a segment along an edge, a segment through the box).

    Near-parallel axes (angle th), two families.  OUT of the plane of the two axes, about a pivot half a metre in front of the second
    axis' start, so the minimiser is an end point -- an interior minimiser of axes at th is determined only to 1.1e-16 / th^2 along
    the axes (1e-4 m at 1e-6 rad), which no comparison of rows at 1e-12 could survive, whatever the implementation.  IN the plane,
    towards the link capsule and away from it: the distance changes along the overlap by th per metre, the minimiser is one end of
    the overlap, and an implementation whose parameter is the round-off of a e - b^2 returns the other end, too long by th x the
    overlap (5e-9 m at 1e-8 rad: the closed form before its end-point projections).  Every capsule case is run twice more under a
    random rigid motion of the whole scene, where that round-off appears.

    Rows.  Where the minimiser is NOT UNIQUE (parallel axes with overlapping spans, a segment parallel to the face it is closest to)
    the distance is only one-sidedly differentiable and every minimiser gives another valid row: the kernel and the restatement
    pick different ones (and, at axes within 1e-9 rad of parallel in a moved scene, a e - b^2 is round-off and the pick is chance).
    So the row of EVERY pair is held to 1e-12 against the restatement's row formula at the kernel's own witnesses -- which the
    certificate has just proved to be minimisers -- and against pykin's row as well wherever pykin's witnesses are the same (to
    1e-9 m).  Witnesses that differ are both certified, which proves the minimiser is not unique, and that is accepted only for the
    target pair of a case that is flat BY CONSTRUCTION (`flat`: out-of-plane axes within 1e-9 rad of parallel whose spans meet, a
    segment with a direction component exactly zero, i.e. parallel to a pair of faces): a witness that drifts on any other pair
    fails the comparison with pykin."""
    CAP_HALF, WCAP_HALF = 0.5, 0.25
    R_CAP, R_SPH, R_WCAP, R_WSPH = 0.05, 0.04, 0.03, 0.06
    BOX_HALF = np.array([0.2, 0.3, 0.15])
    SPH_AT = np.array([0.1, 0.2, -0.1])              # the sphere's centre in the hinge's frame
    # (about 2 m from the link shapes, which stay within 0.9 m of the origin and of (1.1, 0.6, 0.1): no witness pair of the rig is 4 m
    #  apart, so one unit in the last place of a length is at most 4.4e-16 and `pair_dist = len - r_a - r_b to 1e-15` can be asked)
    PARK = {"wcap": (np.array([0.3, 1.8, 0.9]), 11), "wsph": (np.array([0.2, -1.8, 0.9]), 12), "wbox": (np.array([0.0, 0.5, -2.0]), 13)}
    ENV = ("wcap", "wsph", "wbox")

    def __init__(self, seed=5):
        P, R = abi.JOINT_PRISMATIC, abi.JOINT_REVOLUTE
        I = np.eye(3)
        ax = np.array([I[0], I[1], I[2], I[0], I[1], I[2], [0.6, 0.0, 0.8], [0.0, 0.8, 0.6]])
        p0 = np.zeros((8, 3)); p0[6] = [1.0, 0.4, 0.2]
        names = ["x", "y", "z", "roll", "pitch", "yaw", "slide", "hinge"]
        m = kin.KinModel(parent=[-1, 0, 1, 2, 3, 4, -1, 6], jtype=[P, P, P, R, R, R, P, R], axis=ax, R0=np.array([I] * 8), p0=p0,
                         mass=np.ones(8), com=np.zeros((8, 3)), names=names)
        m.link_shapes = {"cap": (5, (0.0, 0.0, -self.CAP_HALF), (0.0, 0.0, self.CAP_HALF), self.R_CAP),
                         "sph": (7, tuple(self.SPH_AT), tuple(self.SPH_AT), self.R_SPH)}
        assert m.add_collision_shape("wcap", "world", ("capsule", 2 * self.WCAP_HALF, self.R_WCAP))
        assert m.add_collision_shape("wsph", "world", ("sphere", self.R_WSPH))
        assert m.add_collision_shape("wbox", "world", ("box", tuple(2 * self.BOX_HALF)))
        m.set_links_vs_environment(["cap", "sph"])
        assert len(m.pairs) == 6
        self.model = m
        self.shapes = {"cap": dict(kind="capsule", size=np.array([0.0, 0.0, self.CAP_HALF]), radius=self.R_CAP),
                       "sph": dict(kind="capsule", size=np.zeros(3), radius=self.R_SPH),
                       "wcap": dict(kind="capsule", size=np.array([0.0, 0.0, self.WCAP_HALF]), radius=self.R_WCAP),
                       "wsph": dict(kind="capsule", size=np.zeros(3), radius=self.R_WSPH),
                       "wbox": dict(kind="box", size=self.BOX_HALF, radius=0.0)}
        self.rng = np.random.default_rng(seed)
        self.q, self.env, self.names, self.coincident, self.target, self.poses = [], [], [], [], [], []
        self.flat, self.target_pair = [], []      # flat: the target pair's minimiser may not be unique, by construction
        self._capsule_cases()
        self.n_capsule_base = len(self.q)
        self._moved_cases(2 * self.n_capsule_base)
        self.n_capsule = len(self.q)
        self._box_cases()
        self.q, self.env = np.ascontiguousarray(self.q), np.ascontiguousarray(self.env)
        self.coincident = np.array(self.coincident, dtype=bool)
        self.B = len(self.q)

    # -- poses of the link shapes (numpy forward kinematics, oracle/pykin.py) and of the world shapes of an instance
    def link_poses(self, q):
        fk = pykin.forward(self.model, q)
        return {"cap": (fk["Rw"][5], fk["pw"][5]), "sph": (fk["Rw"][7], fk["Rw"][7] @ self.SPH_AT + fk["pw"][7])}

    def pair_geometry(self, i, k):
        """(shape a, pose a, shape b, pose b) of pair k of instance i, for the certificate"""
        a, b = ("cap", "sph")[k // 3], self.ENV[k % 3]
        E = self.env[i, k % 3]
        return self.shapes[a], self.poses[i][a], self.shapes[b], (E[:9].reshape(3, 3), E[9:])

    # -- adding one instance: the target link shape, the world shapes the case places (in that link shape's frame), the rest parked
    def _add(self, name, link, placed, q=None, coincident=(), flat=False):
        q = np.zeros(8) if q is None else np.asarray(q, float)
        poses = self.link_poses(q)
        Rl, pl = poses[link]
        E = np.zeros((3, 12))
        for s, nm in enumerate(self.ENV):
            if nm in placed:
                R, p = placed[nm]
                Rw, pw = Rl @ np.asarray(R, float), Rl @ np.asarray(p, float) + pl
            else:
                at, sd = self.PARK[nm]
                Rw, pw = cr.random_rotation(np.random.default_rng(sd)), at
            E[s, :9], E[s, 9:] = Rw.reshape(9), pw
        grp = 0 if link == "cap" else 1
        self.q.append(q); self.env.append(E); self.names.append(name); self.poses.append(poses)
        self.coincident.append([(k // 3 == grp) and self.ENV[k % 3] in coincident for k in range(6)])
        self.target.append((link, dict(placed), tuple(coincident), flat))
        self.flat.append(flat)
        self.target_pair.append((0 if link == "cap" else 3) + self.ENV.index(next(iter(placed))))

    def _capsule_cases(self):
        h, w = self.CAP_HALF, self.WCAP_HALF
        # near-parallel axes: the world capsule beside the link capsule (0.3 m along x), its start at the longitudinal offset `off`
        # from the link capsule's start, tilted by th about x around the pivot 0.5 m in front of its start; both orientations
        for th in (0.0, 1e-12, 1e-9, 1e-6, 1e-3):
            for off in (-2.0, -0.5, 0.3, 0.9, 1.5):
                for flip in (False, True):
                    u = _rx(th) @ np.array([0.0, 0.0, 1.0])
                    pivot = np.array([0.3, 0.0, -h + off - 0.5])
                    centre = pivot + (0.5 + w) * u
                    R = _rx(th) @ (np.diag([1.0, -1.0, -1.0]) if flip else np.eye(3))
                    # (out of the plane the distance changes by (s th)^2 / 0.6 along the overlap: under 1e-15 m at th <= 1e-9 -- flat)
                    self._add(f"parallel th={th:g} off={off:g} flip={int(flip)}", "cap", {"wcap": (R, centre)},
                              flat=th <= 1e-9 and off in (-0.5, 0.3, 0.9))
        # ... and tilted IN the plane of the two axes, towards the link capsule and away from it: the distance falls or rises along the
        # overlap by th per metre, so the minimiser is one END of the overlap -- and a parameter that is the round-off of a e - b^2
        # (under 3e-7 rad, once the scene is moved) would pick the other, too long by th x the overlap
        ry_ = lambda a: np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        for th in (1e-12, 1e-9, 1e-8, 1e-6, 1e-3):
            for off in (-0.5, 0.3, 0.9):
                for sign in (1.0, -1.0):
                    for flip in (False, True):
                        u = ry_(sign * th) @ np.array([0.0, 0.0, 1.0])
                        start = np.array([0.3, 0.0, -h + off])
                        R = ry_(sign * th) @ (np.diag([1.0, -1.0, -1.0]) if flip else np.eye(3))
                        self._add(f"in-plane th={sign * th:g} off={off:g} flip={int(flip)}", "cap", {"wcap": (R, start + w * u)})
        # crossing axes: the witnesses coincide, the distance is minus the radii
        ry = lambda a: np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        self._add("crossing, perpendicular", "cap", {"wcap": (ry(0.5 * np.pi), (0.0, 0.0, 0.2))}, coincident=("wcap",))
        self._add("crossing, oblique", "cap", {"wcap": (ry(0.7), (0.0, 0.0, -0.3))}, coincident=("wcap",))
        self._add("crossing, off centre", "cap", {"wcap": (_rx(1.1), tuple(0.1 * (_rx(1.1) @ np.array([0.0, 0.0, 1.0]))))}, coincident=("wcap",))
        # ends that abut: collinear with a gap, both orientations; side by side with the end planes level
        self._add("collinear, gap 0.2", "cap", {"wcap": (np.eye(3), (0.0, 0.0, h + 0.2 + w))})
        self._add("collinear, gap 0.2, flipped", "cap", {"wcap": (np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, -h - 0.2 - w))})
        self._add("end planes level", "cap", {"wcap": (np.eye(3), (0.0, 0.25, h + w))})
        self._add("skew, end to end", "cap", {"wcap": (ry(0.5 * np.pi), (w + 0.1, 0.0, h + 0.1))})
        # a point against a segment (both ways), a point against a point
        for nm, p in (("beside", (0.2, -0.1, 0.1)), ("beyond the end", (0.1, 0.1, h + 0.3)), ("on the extension", (0.0, 0.0, -h - 0.2)),
                      ("level with the end", (0.3, 0.0, h))):
            self._add(f"world sphere {nm}", "cap", {"wsph": (np.eye(3), p)})
        for nm, p in (("beside", (0.15, 0.1, 0.05)), ("beyond the end", (0.1, -0.1, w + 0.2)), ("on the extension", (0.0, 0.0, w + 0.15)),
                      ("level with the end", (0.0, 0.2, -w))):
            self._add(f"link sphere {nm}", "sph", {"wcap": (cr.random_rotation(self.rng), p)}, q=self._q_sphere())
        self._add("point / point", "sph", {"wsph": (np.eye(3), (0.1, 0.2, -0.2))})
        self._add("point / point, moved", "sph", {"wsph": (np.eye(3), (-0.3, 0.0, 0.1))}, q=self._q_sphere())

    def _q_sphere(self):
        q = np.zeros(8)
        q[6:] = self.rng.uniform(-0.3, 0.3), self.rng.uniform(-1.5, 1.5)
        return q

    def _moved_cases(self, count):
        """`count` of the capsule cases (round and round) again under a random rigid motion of the whole scene: the floating base (or the second root)
        moves the link shape, and the world shapes are placed relative to it as before"""
        base, names = list(self.target[:self.n_capsule_base]), list(self.names[:self.n_capsule_base])
        for c in range(count):
            k = c % len(base)
            link, placed, coincident, flat = base[k]
            q = np.zeros(8)
            if link == "cap":
                q[:3], q[3:6] = self.rng.uniform(-0.2, 0.2, 3), self.rng.uniform(-3.0, 3.0, 3)
            else:
                q = self._q_sphere()
            self._add("moved: " + names[k], link, placed, q=q, coincident=coincident, flat=flat)

    def _box_segment(self, name, mid, d, coincident=False):
        """the link capsule's axis as the segment mid -+ 0.5 d of the BOX frame: the box is posed so (the link frame is the identity)"""
        flat = bool((np.asarray(d) == 0.0).any())          # parallel to a pair of faces: a stretch of the segment may be equally close
        M = _frame_with_z(d)                         # box frame <- link frame: M e_z = d
        Rb = M.T
        self._add(name, "cap", {"wbox": (Rb, -Rb @ np.asarray(mid, float))}, coincident=("wbox",) if coincident else (), flat=flat)

    def _box_point(self, name, pt):
        """the link sphere's centre as the point pt of the BOX frame, the box turned at random"""
        R = cr.random_rotation(self.rng)
        self._add(name, "sph", {"wbox": (R, -R @ np.asarray(pt, float))}, q=self._q_sphere())

    def _box_cases(self):
        hx, hy, hz = self.BOX_HALF
        X, Y, Z = np.eye(3)
        self._box_segment("parallel to a face, above it", (0.05, 0.02, hz + 0.1), X)
        self._box_segment("parallel to a face, above an edge", (hx, 0.05, hz + 0.1), Y)
        self._box_segment("parallel to a face, outside an edge", (hx + 0.15, 0.05, hz + 0.1), Y)
        self._box_segment("over a corner", (hx + 0.05, hy - 0.05, hz + 0.1), np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0))
        self._box_segment("over a corner, inclined", (hx + 0.1, hy + 0.1, hz + 0.2), np.array([1.0, -1.0, 0.5]) / 1.5)
        self._box_segment("along an edge", (hx, 0.1, hz), Y, coincident=True)
        self._box_segment("through the box", (0.01, 0.02, 0.03), np.array([2.0, -1.0, 2.0]) / 3.0, coincident=True)
        self._box_segment("through the box along an axis", (0.05, -0.1, 0.0), Z, coincident=True)
        self._box_segment("perpendicular to a face, both ends beside it", (hx + 0.1, 0.05, 0.0), Z)
        # ("just outside": 1 mm.  The unit normal is (ca - cb) / len, and ca - cb carries the round-off of coordinates of 0.3 m,
        #  5.5e-17: rows can agree to 1e-12 between two implementations only where len >= 6e-5 m)
        self._box_segment("parallel to an axis just outside a face", (0.0, hy + 1e-3, 0.05), X)
        self._box_segment("parallel to an axis just outside an edge", (0.0, hy + 1e-3, hz + 1e-3), X)
        for nm, p in (("a face", (0.05, -0.1, hz + 0.2)), ("an edge", (hx + 0.1, 0.0, hz + 0.1)), ("a corner", (hx + 0.1, hy + 0.2, -hz - 0.1))):
            self._box_point(f"a point off {nm}", p)
        # random segments with one to three direction components exactly zero (three: the point), one in five with an end coordinate
        # exactly on a face plane; a draw that meets the box inflated by 1 mm is drawn again (slab clipping: no code under test)
        made = 0
        while made < 300:
            zeros = 1 + made % 3
            c = self.rng.uniform(-1.0, 1.0, 3) * (self.BOX_HALF + 0.25)      # (the box stays clear of the link sphere)
            if zeros == 3:
                if (np.abs(c) <= self.BOX_HALF + 1e-3).all():
                    continue
                self._box_point("random point", c)
                made += 1
                continue
            d = self.rng.standard_normal(3)
            d[self.rng.permutation(3)[:zeros]] = 0.0
            d /= np.linalg.norm(d)
            s0 = c - 0.5 * d
            if made % 5 == 0:
                i = int(self.rng.integers(0, 3))
                s0[i] = self.BOX_HALF[i] * (1.0 if self.rng.uniform() < 0.5 else -1.0)      # an end on a face plane
            if _clips_box(s0, s0 + d, self.BOX_HALF + 1e-3):
                continue
            self._box_segment(f"random segment, {zeros} zero components", s0 + 0.5 * d, d)
            made += 1

    def reference_witnesses(self, i, k):
        """the witnesses of the restatement's closed forms (pykin.closest_segment_points, pykin.segment_box_closest)"""
        A, pA, Bs, pB = self.pair_geometry(i, k)
        ends = lambda s, pose: (pose[0] @ np.array([0.0, 0.0, -s["size"][2]]) + pose[1], pose[0] @ np.array([0.0, 0.0, s["size"][2]]) + pose[1])
        a0, a1 = ends(A, pA)
        if Bs["kind"] == "box":
            la, lb = pykin.segment_box_closest(pB[0].T @ (a0 - pB[1]), pB[0].T @ (a1 - pB[1]), Bs["size"])
            return pB[0] @ la + pB[1], pB[0] @ lb + pB[1]
        return pykin.closest_segment_points(a0, a1, *ends(Bs, pB))

    def row_at(self, fk, k, ca, cb):
        """the restatement's row of pair k (oracle/pykin.pair_distances) at GIVEN witnesses; the world shapes move with no joint"""
        m = self.model
        row, dv = np.zeros(m.n), ca - cb
        j = m.pairs[k][0]
        while j >= 0:
            z = fk["Rw"][j] @ m.axis[j]
            v = np.cross(z, ca - fk["pw"][j]) if m.jtype[j] == abi.JOINT_REVOLUTE else z
            row[j] = (dv / np.linalg.norm(dv)) @ v
            j = m.parent[j]
        return row

    # -- the checks, on whatever ran the model (the emulator, the device): pd [B][6], pJ [B][6][8], pp [B][6][6]
    def check(self, pd, pJ, pp):
        """asserts every check of the rig; returns dict(gap = the largest certificate gap, member, d, Jd = worst deviations from pykin)"""
        from test_convex_shapes_host import GAP, MEMBER
        m = self.model
        rad = np.array([pr[3] + pr[7] for pr in m.pairs])
        w = dict(gap=0.0, member=0.0, d=0.0, Jd=0.0, Jd_at_witnesses=0.0, len=0.0, not_unique=0)
        assert np.isfinite(pd).all() and np.isfinite(pJ).all() and np.isfinite(pp).all()
        ln = np.linalg.norm(pp[:, :, :3] - pp[:, :, 3:], axis=2)
        assert ln.max() < 4.0                            # (the recomputed length is the kernel's to one unit in the last place)
        ra, rb = np.array([pr[3] for pr in m.pairs]), np.array([pr[7] for pr in m.pairs])
        w["len"] = float(np.abs((ln - ra[None]) - rb[None] - pd).max())
        assert w["len"] <= 1e-15, w["len"]
        # the coincident witnesses are the named ones, no more and no fewer
        assert np.array_equal(ln <= 1e-12, self.coincident), [(self.names[i], k) for i, k in np.argwhere((ln <= 1e-12) != self.coincident)]
        for i in range(self.B):
            fk = pykin.forward(m, self.q[i])
            d, Jd = pykin.pair_distances(m, self.q[i], fk=fk, env_pose=self.env[i])
            w["d"] = max(w["d"], float(np.abs(pd[i] - d).max()))
            assert np.abs(pd[i] - d).max() <= 1e-12, (self.names[i], pd[i] - d)
            for k in range(6):
                A, pA, Bs, pB = self.pair_geometry(i, k)
                ca, cb = pp[i, k, :3], pp[i, k, 3:]
                if self.coincident[i, k]:
                    ia, ib = cr.violation(A, pA, ca), cr.violation(Bs, pB, cb)
                    assert abs(pd[i, k] + rad[k]) <= 1e-12 and (pJ[i, k] == 0.0).all(), (self.names[i], k)
                else:
                    cert = cr.certify(A, pA, Bs, pB, ca, cb)
                    ia, ib = cert["in_a"], cert["in_b"]
                    w["gap"] = max(w["gap"], cert["gap"])
                    assert -1e-12 <= cert["gap"] <= GAP, (self.names[i], k, cert)
                    dev = float(np.abs(pJ[i, k] - self.row_at(fk, k, ca, cb)).max())
                    w["Jd_at_witnesses"] = max(w["Jd_at_witnesses"], dev)
                    assert dev <= 1e-12, (self.names[i], k, dev)
                    ra_, rb_ = self.reference_witnesses(i, k)
                    if max(np.abs(ca - ra_).max(), np.abs(cb - rb_).max()) <= 1e-9:
                        dev = float(np.abs(pJ[i, k] - Jd[k]).max())
                        w["Jd"] = max(w["Jd"], dev)
                        assert dev <= 1e-12, (self.names[i], k, dev)
                    else:          # two different minimisers: the restatement's must carry the certificate as well
                        rc = cr.certify(A, pA, Bs, pB, ra_, rb_)
                        assert rc["in_a"] <= MEMBER and rc["in_b"] <= MEMBER and -1e-12 <= rc["gap"] <= GAP, (self.names[i], k, rc)
                        # ... and the pair must be one whose minimiser is not unique BY CONSTRUCTION: the target pair of a case with
                        # (all but) parallel axes, or of a segment with a direction component exactly zero (parallel to a face)
                        assert k == self.target_pair[i] and self.flat[i], (self.names[i], k)
                        w["not_unique"] += 1
                w["member"] = max(w["member"], ia, ib)
                assert ia <= MEMBER and ib <= MEMBER, (self.names[i], k, ia, ib)
        return w


_rig = None


def rig():
    """the one Rig of a process (read-only)"""
    global _rig
    if _rig is None:
        _rig = Rig()
    return _rig
