"""tests/kin_rows_ref.py -- TEST INFRASTRUCTURE ONLY: what the row-set and gaze tests share.

  * a numpy restatement of the four formulas (velocity::Contact / floating_base::Contact, velocity::PureRolling,
    constraints::velocity::OmniWheels4X, velocity::Gaze's reference), in the reference's order of operations, on the pose and the world
    Jacobian of oracle/pykin.py;
  * the recipe of the host build tests/emu/kin_rows_host.cpp (the kinematics kernel with its ROWS flag on through the lock-step
    emulation, both JMAX), built with native_build's flags, staleness rule and write-then-rename rule;
  * the four trees of the tests with their row sets, one canaried output layout, the emulated run into it.
"""
import copy
import ctypes as C
import os
import shlex
import subprocess

import numpy as np

from opensot_amd import abi, synth
from oracle import pykin
import native_build
import tree_cases as tc

EMU = os.path.join(native_build.ROOT, "tests", "emu")
SOURCE = "kin_rows_host.cpp"
LIBRARY = "libosot_kin_rows_host.so"
COMMAND = native_build.LOCKSTEP
CANARY = tc.CANARY
GAZE_THRESHOLD = 0.2


# ---- 1. the host build ---------------------------------------------------------------------------------------------------------------
def ensure():
    """build tests/emu/libosot_kin_rows_host.so if it is stale (native_build.is_stale), to a temporary name first"""
    out = os.path.join(EMU, LIBRARY)
    if native_build.is_stale(out, out + ".d", EMU, recipe=os.path.abspath(__file__)) or \
            os.path.getmtime(native_build.RECIPE) > os.path.getmtime(out):
        tmp = f"{LIBRARY}.tmp.{os.getpid()}"
        cmd = COMMAND + [SOURCE, "-MMD", "-MF", LIBRARY + ".d", "-o", tmp]
        print(shlex.join(cmd), flush=True)
        try:
            subprocess.check_call(cmd, cwd=EMU)
            os.replace(os.path.join(EMU, tmp), out)
        finally:
            if os.path.exists(os.path.join(EMU, tmp)):
                os.remove(os.path.join(EMU, tmp))
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(ensure())
        dp = C.POINTER(C.c_double)
        _lib.kin_rows_host_check.argtypes = [C.POINTER(abi.KinDesc), C.POINTER(C.c_char_p)]
        _lib.kin_rows_host_kinematics.argtypes = [C.POINTER(abi.KinDesc), C.POINTER(abi.KinBatch)]
        _lib.kin_rows_host_stage.argtypes = [C.POINTER(abi.KinDesc), C.POINTER(abi.KinBatch), C.c_void_p, C.c_void_p]
        _lib.kin_rows_host_s33.argtypes = [dp, dp, dp]
    return _lib


def host_check(desc):
    """osot_kin_create's answer to a description, from the host build -> (code, reason)"""
    why = C.c_char_p()
    rc = lib().kin_rows_host_check(C.byref(desc), C.byref(why))
    return rc, (why.value or b"").decode()


def host_s33(normal):
    nrm = (C.c_double * 3)(*[float(v) for v in normal])
    s33, unit = (C.c_double * 9)(), (C.c_double * 3)()
    assert lib().kin_rows_host_s33(nrm, s33, unit) == abi.OK
    return np.array(s33[:]).reshape(3, 3), np.array(unit[:])


# ---- 2. the restatement --------------------------------------------------------------------------------------------------------------
def s33_literal(n):
    """PureRolling::setOutwardNormal (PureRolling.cpp:19-47), line by line -> (the block _update() puts into _S, the unit normal)"""
    n = np.asarray(n, dtype=float)
    world_contact_plane_normal = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])      # normalize(): squaredNorm in index order
    e1, e2, e3 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
    uz = world_contact_plane_normal
    ux = e1
    if abs(uz @ e2) < abs(uz @ ux):
        ux = e2
    if abs(uz @ e3) < abs(uz @ ux):
        ux = e3
    uy = np.cross(uz, ux)
    local_R_world = np.stack([ux, uy, uz], axis=1)       # `<< ux, uy, uz`: three columns
    local_R_world = local_R_world.T.copy()               # transposeInPlace
    return local_R_world.T.copy(), uz                    # _S.block<3,3>(0,0) = _local_R_world.transpose()


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rowset_matrix(rs, R):
    """M with rows = M J_f for a CONTACT / PURE_ROLLING set at the frame rotation R (all rows of the kind), None for OMNI4X"""
    P = rs["param"]
    if rs["kind"] == abi.ROWSET_CONTACT:
        Ad = np.zeros((6, 6)); Ad[:3, :3] = R.T; Ad[3:, 3:] = R.T
        return P.reshape(6, 6) @ Ad
    if rs["kind"] == abi.ROWSET_PURE_ROLLING:
        r, nrm, S33 = P[0], P[1:4], P[4:13].reshape(3, 3)
        d = -1.0 * r * nrm
        a = np.cross(R @ np.array([0.0, 0.0, 1.0]), nrm)
        a = a / np.linalg.norm(a)
        S = np.zeros((4, 6)); S[:3, :3] = S33; S[3, 3:] = a
        T = np.eye(6); T[:3, 3:] = -_skew(d)               # [J_lin + J_ang x d; J_ang]
        return S @ T
    return None


def rowset_rows(model, rs, fk, qdot=None):
    """the rows of one set at one posture (fk = pykin.forward) -> (A [rows][n] or [rows][6], b or None, |M|_inf)"""
    n, f = model.n, rs["frame"]
    R, J = fk["frame_R"][f], fk["J"][f]
    kind, P = rs["kind"], rs["param"]
    if kind == abi.ROWSET_CONTACT:
        # Contact.cpp:19-33: rotate both blocks by R', then K
        Jr = np.concatenate([R.T @ J[:3], R.T @ J[3:]], axis=0)
        A = P.reshape(6, 6) @ Jr
        norm = np.abs(rowset_matrix(rs, R)).sum(axis=1).max()
    elif kind == abi.ROWSET_PURE_ROLLING:
        r, nrm, S33 = P[0], P[1:4], P[4:13].reshape(3, 3)
        d = -1.0 * r * nrm
        Jc = np.concatenate([J[:3] + np.cross(J[3:].T, d).T, J[3:]], axis=0)
        a = np.cross(R @ np.array([0.0, 0.0, 1.0]), nrm)
        a = a / np.sqrt(a @ a)
        S = np.zeros((4, 6)); S[:3, :3] = S33; S[3, 3:] = a
        A = S @ Jc
        norm = np.abs(rowset_matrix(rs, R)).sum(axis=1).max()
    else:
        l1, l2, r = P[0], P[1], P[2]
        Jw = np.zeros((3, n))
        Jw[0, 0] = 1.0; Jw[1, 1] = 1.0; Jw[2, 5] = 1.0
        fl, fr, hl, hr = rs["wheels"]
        Jw[0, fl] -= 1.0; Jw[1, fl] -= -1.0; Jw[2, fl] -= -1.0 / (l1 + l2)
        Jw[0, fr] -= 1.0; Jw[1, fr] -= 1.0; Jw[2, fr] -= 1.0 / (l1 + l2)
        Jw[0, hl] -= 1.0; Jw[1, hl] -= 1.0; Jw[2, hl] -= -1.0 / (l1 + l2)
        Jw[0, hr] -= 1.0; Jw[1, hr] -= -1.0; Jw[2, hr] -= 1.0 / (l1 + l2)
        Jw[:, 6:] *= r / 4.0
        A = Jw.copy()
        A[:, 6:] = R @ Jw[:, 6:]
        norm = 1.0
    kept = [i for i in range(A.shape[0]) if (rs["mask"] >> i) & 1]
    A = A[kept]
    b = None
    if rs["split"]:
        b = -(A[:, 6:] @ qdot[6:]) if qdot is not None else None
        A = A[:, :6]
    return A, b, float(norm)


def gaze_rotation(R, p, g, real=np.float64):
    """Gaze::setGaze + computePanTiltMatrix (Gaze.cpp:52-74, cartesian_utils.cpp:27-35) for the pose [R | p] and the point g ->
    (|t|, the 12 doubles of the new reference or None below the threshold, t); real: the arithmetic (np.longdouble for the error)"""
    R, p, g = (np.asarray(x, dtype=real) for x in (R, p, g))
    t = R.T @ (g - p)
    nt = np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    if not nt >= real(GAZE_THRESHOLD):
        return nt, None, t
    pan = np.arctan2(t[1], t[0])
    tilt = np.arctan2(t[2], np.sqrt(t[1] * t[1] + t[0] * t[0]))
    cp, sp, cs, sn = np.cos(pan), np.sin(pan), np.cos(-tilt), np.sin(-tilt)
    z = real(0.0)
    M = np.array([cs * cp, -sp, sn * cp, cs * sp, cp, sn * sp, -sn, z, cs, z, z, z], dtype=real)
    return nt, M, t


# ---- 3. the trees ----------------------------------------------------------------------------------------------------------------------
def _random_K(rng, rows=6):
    return rng.uniform(-2.0, 2.0, (rows, 6))


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def chain7():
    """a 7-joint chain: JMAX = 32, and B = 3 leaves the last wavefront half empty"""
    m = copy.copy(tc.tree_case(7, "chain", seed=3))
    m.rowsets, m.gazes = [], []
    rng = np.random.default_rng(707)
    m.add_contact_rows(0, _random_K(rng))
    m.add_pure_rolling(1, 0.07, normal=_unit(rng))
    m.add_omni_wheels_4x(2, 0.3, 0.2, 0.05, (6, 6, 6, 6))
    m.add_contact_rows(3, _random_K(rng, 4), split=True)
    m.add_gaze(0); m.add_gaze(4)
    return m


def tree33():
    m = copy.copy(tc.tree_case(33, "random", seed=1))
    m.rowsets, m.gazes = [], []
    rng = np.random.default_rng(3333)
    m.add_pure_rolling(0, 0.1, normal=(0, 0, 1))
    m.add_pure_rolling(5, 0.05, normal=_unit(rng), rows=(0, 1))
    m.add_contact_rows(2, np.eye(6))
    m.add_contact_rows(0, _random_K(rng, 5), split=True)
    m.add_omni_wheels_4x(7, 0.25, 0.15, 0.06, (6, 17, 32, 9))
    m.add_gaze(1); m.add_gaze(7)
    return m


def tree64():
    """64 joints, 8 row sets of mixed kinds and masks, 8 gaze frames at once; frames 2 and 5 are RELATIVE (gaze only), frame 4 carries
    a BODY Jacobian and a column mask that the row sets on it must not see"""
    m = copy.copy(tc.tree_case(64, "random", seed=2))
    m.rowsets, m.gazes = [], []
    m.frame_base = {2: 1, 5: 6}
    m.frame_body = {4: True}
    m.frame_active_joints = {4: [j for j in range(64) if j % 3 != 1]}
    rng = np.random.default_rng(6464)
    m.add_contact_rows(0, _random_K(rng))                                                   # all six rows
    m._add_rowset(abi.ROWSET_CONTACT, 4, 0b101010, _random_K(rng).reshape(36))               # rows 1, 3, 5
    m.add_contact_rows(1, _random_K(rng), split=True)                                        # split, six rows
    m._add_rowset(abi.ROWSET_CONTACT, 6, 0b100001, _random_K(rng).reshape(36), split=True)   # split, rows 0 and 5
    m.add_pure_rolling(0, 0.09, normal=_unit(rng))                                           # PureRolling
    m.add_pure_rolling(3, 0.04, normal=_unit(rng), rows=(0, 1, 2))                           # PureRollingPosition, control_z
    m.add_pure_rolling(7, 0.12, normal=(1, 0, 0), rows=(3,))                                 # PureRollingOrientation
    m._add_rowset(abi.ROWSET_OMNI4X, 4, 0b101, [0.2, 0.3, 0.07], wheels=(63, 6, 40, 41))     # rows 0 and 2
    for f in range(8):
        m.add_gaze(f)
    return m


def wheeled():
    plan, leaf, m = synth.make_wheeled_stack(3, omni=True)
    m.add_gaze("base")
    m.q0 = leaf["state"]["q0"]
    return m


CASES = {"chain7": (chain7, 3), "tree33": (tree33, 2), "tree64": (tree64, 2), "wheeled": (wheeled, 3)}


def postures(m, B, seed=0):
    if hasattr(m, "wheel_joints"):
        return synth.wheeled_posture(m, B, seed=seed)
    return tc.draw_q(m, B, seed=seed)


def gaze_points(m, q, seed=0):
    """per gaze and instance a point at a drawn distance from the frame, alternating around the threshold: 0.1 (kept), 0.3, 1.5
    (overwritten), in a direction with sqrt(t_x^2 + t_y^2) >= 0.05 |t| / 0.1 -> points [G][B][3], distances [G][B]"""
    rng = np.random.default_rng([m.n, seed, 99])
    B, G = len(q), len(m.gazes)
    pts, dist = np.zeros((G, B, 3)), np.zeros((G, B))
    ref = tc.reference(m, q)
    for g, f in enumerate(m.gazes):
        for i in range(B):
            R, p = ref[i]["R"][f], ref[i]["p"][f]
            while True:
                t = _unit(rng)
                if np.hypot(t[0], t[1]) >= 0.5:
                    break
            dist[g, i] = (0.1, 0.3, 1.5)[(g + i) % 3]
            pts[g, i] = p + R @ (dist[g, i] * t)
    return pts, dist


# ---- 4. one output layout, the emulated run ------------------------------------------------------------------------------------------------
def layout(m, B):
    """first row of every set inside the padded arrays (one canary row in front of and behind every set, one canary instance)"""
    off, o = {}, 1
    for s in range(len(m.rowsets)):
        off[s] = o
        o += m.rowset_rows(s) + 1
    return off, o


def outputs(m, B, gaze_prev=None, pairs=False):
    """pairs: the pair outputs as well (pd, pJ, pp in the layout of tree_cases.output_shapes): the instantiations with the pair stage"""
    F, G, n = len(m.frames), len(m.gazes), m.n
    off, rows = layout(m, B)
    out = dict(poses=np.full((F, B + 1, 12), CANARY), J=np.full((F, B + 1, 6, n), CANARY), RA=np.full((B + 1, rows, n), CANARY),
               RS=np.full((B + 1, rows, 6), CANARY), rb=np.full((B + 1, rows), CANARY),
               gaze=np.full((max(G, 1), B + 1, 12), np.nan) if gaze_prev is None else np.array(gaze_prev, dtype=float))
    if pairs:
        P = len(m.pairs)
        out.update(pd=np.full((B + 1, P), CANARY), pJ=np.full((B + 1, P + 1, n), CANARY), pp=np.full((B + 1, P, 6), CANARY))
    return out, off


def batch(m, q, out, off, qdot=None, points=None, frames=True):
    q = np.ascontiguousarray(q, dtype=np.float64)
    B, n = q.shape
    kb = abi.KinBatch()
    kb.B, kb.q = B, q.ctypes.data
    keep = [q]
    if frames:
        for f in range(len(m.frames)):
            kb.frame_pose[f] = out["poses"][f].ctypes.data
            kb.frame_J[f] = out["J"][f].ctypes.data
            kb.frame_J_stride[f] = 6 * n
    if "pd" in out:
        kb.pair_dist, kb.pair_points = out["pd"].ctypes.data, out["pp"].ctypes.data
        kb.pair_J, kb.pair_J_stride = out["pJ"].ctypes.data, (len(m.pairs) + 1) * n
    rows = out["RA"].shape[1]
    for s, rs in enumerate(m.rowsets):
        if rs["split"]:
            kb.rowset_A[s] = out["RS"].ctypes.data + 8 * off[s] * 6
            kb.rowset_A_stride[s] = rows * 6
            if qdot is not None:
                kb.rowset_b[s] = out["rb"].ctypes.data + 8 * off[s]
                kb.rowset_b_stride[s] = rows
        else:
            kb.rowset_A[s] = out["RA"].ctypes.data + 8 * off[s] * n
            kb.rowset_A_stride[s] = rows * n
    if qdot is not None:
        qdot = np.ascontiguousarray(qdot, dtype=np.float64)
        keep.append(qdot)
        kb.rowset_qdot = qdot.ctypes.data
    if points is not None:
        points = np.ascontiguousarray(points, dtype=np.float64)
        keep.append(points)
        for g in range(len(m.gazes)):
            kb.gaze_point[g] = points[g].ctypes.data
            kb.gaze_ref[g] = out["gaze"][g].ctypes.data
    return kb, keep


def emu_rows(m, q, qdot=None, points=None, gaze_prev=None, pairs=False):
    """the kernel (ROWS instantiation) through the host emulation with every frame output, every row set and every gaze bound;
    pairs: the pair outputs too (osot_kin_kernel<true, ., false, true>)"""
    out, off = outputs(m, len(q), gaze_prev, pairs)
    kb, keep = batch(m, q, out, off, qdot, points)
    d = m.desc()
    assert lib().kin_rows_host_kinematics(C.byref(d), C.byref(kb)) == abi.OK
    out["off"] = off
    return out


def stage_rows(m, q, pose, J, qdot=None, points=None, gaze_prev=None):
    """the row-set and gaze stage ALONE through the host emulation, on a GIVEN pose [F][B][12] and world Jacobian [F][B][6][n]"""
    B = len(q)
    out, off = outputs(m, B, gaze_prev)
    kb, keep = batch(m, q, out, off, qdot, points, frames=False)
    pose = np.ascontiguousarray(pose, dtype=np.float64); J = np.ascontiguousarray(J, dtype=np.float64)
    assert pose.shape == (len(m.frames), B, 12) and J.shape == (len(m.frames), B, 6, m.n)
    d = m.desc()
    assert lib().kin_rows_host_stage(C.byref(d), C.byref(kb), pose.ctypes.data, J.ctypes.data) == abi.OK
    out["off"] = off
    return out


def got_rows(m, out, s, i):
    """what a run wrote for set s of instance i -> (A, b or None)"""
    o, r = out["off"][s], m.rowset_rows(s)
    if m.rowsets[s]["split"]:
        return out["RS"][i, o:o + r], out["rb"][i, o:o + r]
    return out["RA"][i, o:o + r], None


def canaries_intact(m, out, B, with_b=True):
    """everything outside the sets' own rows is still the canary: the rows between the sets, the columns of the other layout, the
    instance behind the batch"""
    mask = {k: np.ones(out[k].shape, dtype=bool) for k in ("RA", "RS", "rb")}
    for s, rs in enumerate(m.rowsets):
        o, r = out["off"][s], m.rowset_rows(s)
        if rs["split"]:
            mask["RS"][:B, o:o + r] = False
            if with_b:
                mask["rb"][:B, o:o + r] = False
        else:
            mask["RA"][:B, o:o + r] = False
    return all((out[k][mask[k]] == CANARY).all() for k in mask) and not any((out[k][~mask[k]] == CANARY).any() for k in mask)


def compare_rows(m, q, out, bound_J, qdot=None):
    """every set of every instance against the restatement at bound_J x max(1, |M|_inf) (b: x the 1-norm of qdot[6:] as well)
    -> the worst ratio error / bound"""
    worst = 0.0
    for i in range(len(q)):
        fk = pykin.forward(m, q[i])
        for s, rs in enumerate(m.rowsets):
            A, b, norm = rowset_rows(m, rs, fk, None if qdot is None else qdot[i])
            gA, gb = got_rows(m, out, s, i)
            bound = bound_J * max(1.0, norm)
            err = float(np.abs(gA - A).max())
            assert err <= bound, (s, i, err, bound)
            worst = max(worst, err / bound)
            if b is not None:
                bb = bound * max(1.0, float(np.abs(qdot[i, 6:]).sum()))
                eb = float(np.abs(gb - b).max())
                assert eb <= bb, (s, i, eb, bb)
                worst = max(worst, eb / bb)
    return worst


# ---- 5. the wheeled stacks on the host -------------------------------------------------------------------------------------------------
def fill_wheeled_leaf(plan, leaf, model, source):
    """the leaf of synth.make_wheeled_stack with the producer's share filled in on the host -> a new leaf.
    source "emu": what the emulated kernel writes (rows into A_0 / the row block's C, the base's Jacobian into A_1, its pose into the
    Cartesian leaf); "ref": the GENERIC TWIN -- the same rows from the restatement, handed in as plain OSOT_TASK_GENERIC /
    OSOT_ROWS_GENERIC data, with pose and Jacobian of oracle/pykin.py"""
    q = leaf["state"]["q0"]
    B, legs = leaf["B"], len(model.wheel_joints)
    new = dict(leaf)
    new["A"] = [a.copy() if a is not None else None for a in leaf["A"]]
    pose = np.zeros((B, 12))
    Crows = np.zeros((B, 3, model.n))
    if source == "emu":
        out = emu_rows(model, q)
        for s in range(legs):
            for i in range(B):
                new["A"][0][i, 4 * s:4 * s + 4] = got_rows(model, out, s, i)[0]
        new["A"][1][:] = out["J"][0][:B]
        pose[:] = out["poses"][0][:B]
        if len(model.rowsets) > legs:
            for i in range(B):
                Crows[i] = got_rows(model, out, legs, i)[0]
    else:
        for i in range(B):
            fk = pykin.forward(model, q[i])
            for s in range(legs):
                new["A"][0][i, 4 * s:4 * s + 4] = rowset_rows(model, model.rowsets[s], fk)[0]
            new["A"][1][i] = fk["J"][0]
            pose[i, :9] = fk["frame_R"][0].reshape(9); pose[i, 9:] = fk["frame_p"][0]
            if len(model.rowsets) > legs:
                Crows[i] = rowset_rows(model, model.rowsets[legs], fk)[0]
    ref = pose.copy()
    ref[:, 9:] += leaf["state"]["base_step"]
    new["task"] = [list(lev) for lev in leaf["task"]]
    new["task"][1][0] = (pose, ref, None)
    if plan.rowblocks:
        new["rows"] = [(Crows, np.zeros((B, 3)), np.zeros((B, 3)))]
    return new


def fill_estimation_leaf(plan, leaf, model):
    """the leaf of synth.make_base_estimation_stack with A and b from the emulated kernel (split contact row sets) -> a new leaf"""
    q, qdot = leaf["state"]["q0"], leaf["state"]["qdot"]
    B, legs = leaf["B"], len(model.wheel_joints)
    out = emu_rows(model, q, qdot=qdot)
    new = dict(leaf)
    new["A"] = [np.zeros((B, 3 * legs, 6))]
    task = []
    for s in range(legs):
        b = np.zeros((B, 3))
        for i in range(B):
            A, bi = got_rows(model, out, s, i)
            new["A"][0][i, 3 * s:3 * s + 3] = A
            b[i] = bi
        task.append((b, None, None))
    new["task"] = [task]
    return new


def emulated_wheeled_solve(plan, leaf, model):
    """make_wheeled_stack on the host: the emulated producer's rows through the emulated update and cascade -> dq, status, asm"""
    import helpers
    from oracle import pyoracle
    pyoracle.build()
    mine = fill_wheeled_leaf(plan, leaf, model, "emu")
    asm = pyoracle.assemble(plan, mine)           # (the layout emu_cascade takes; A and the rows' C are the producer's)
    upd = helpers.emu_update(plan, mine)
    for k in range(plan.L):
        asm["b"][k] = upd["b"][k]
    asm["l"], asm["u"] = upd["l"], upd["u"]
    if plan.rowblocks:
        asm["C"], asm["lo"], asm["up"] = upd["C"], upd["lo"], upd["up"]
    dq, xl, st, it = helpers.emu_cascade(plan, asm)
    return dq, st, asm
