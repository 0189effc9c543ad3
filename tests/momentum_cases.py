"""tests/momentum_cases.py -- TEST INFRASTRUCTURE ONLY: the stacks of synth.make_coman_momentum_stack / make_coman_id_momentum_stack
filled on the CPU -- oracle.pykin for poses, Jacobians and the CoM, tests/momentum_ref.py for the momentum matrix -- and their closed
loops driven by the oracle solver.  The GPU tests compare against these; the loops are the pre-check of the GPU closed loops."""
import numpy as np

from oracle import pykin, pyoracle

import momentum_ref


def velocity_fill(plan, leaf, model, q, refs=None):
    """the numpy leaf of make_coman_momentum_stack at the postures q [B][n]: -> (leaf, refs, A_ang [B][3][n]); refs (the soles' first
    poses and the first CoM) are made from q where None"""
    B, n = q.shape
    s = leaf["state"]
    fl, fr = s["frames"]
    A0, Aang, poses, com = np.zeros((B, 15, n)), np.zeros((B, 3, n)), [np.zeros((B, 12)), np.zeros((B, 12))], np.zeros((B, 3))
    for i in range(B):
        fk = pykin.forward(model, q[i])
        for k, f in enumerate((fl, fr)):
            poses[k][i] = np.concatenate([fk["frame_R"][f].reshape(9), fk["frame_p"][f]])
            A0[i, 6 * k:6 * k + 6] = fk["J"][f]
        cmm = momentum_ref.one(model, q[i])["cmm"]
        Aang[i] = cmm[3:]
        com[i] = fk["com"]
        A0[i, 12:] = cmm[:3] if s["linear_momentum"] is not None else fk["Jcom"]
    refs = refs or dict(poses=[p.copy() for p in poses], com=com.copy())
    out = dict(leaf)
    out["A"] = [A0] + ([Aang] if s["momentum"] is not None else []) + [None]
    third = (np.zeros((B, 3)), None, None) if s["linear_momentum"] is not None else (com, refs["com"], None)
    out["task"] = [[(poses[0], refs["poses"][0], None), (poses[1], refs["poses"][1], None), third]] \
        + ([[(np.zeros((B, 3)), None, None)]] if s["momentum"] is not None else []) + [[(q.copy(), s["q_ref"], None)]]
    out["bound"] = [(q.copy(),) + tuple(leaf["bound"][0][1:]), leaf["bound"][1]]
    return out, refs, Aang


def velocity_loop(make, B, cycles, seed, **kw):
    """kinematics -> momentum matrix -> oracle solve -> q += dq on the CPU: (max|A_ang dq| [cycles][B], how far the soles moved)"""
    plan, leaf, model = make(B, seed=seed, **kw)
    q, refs, norms = leaf["state"]["q0"].copy(), None, []
    for _ in range(cycles):
        lf, refs, Aang = velocity_fill(plan, leaf, model, q, refs)
        res = pyoracle.ihqp_solve_batch(pyoracle.assemble(plan, lf), pyoracle.BE_EIQP_EQ, nthreads=4)
        assert (res["status"] == 1).all(), res["status"]
        norms.append(np.abs(np.einsum("brn,bn->br", Aang, res["dq"])).max(axis=1))
        q = q + res["dq"]
    lf, _, _ = velocity_fill(plan, leaf, model, q, refs)
    moved = max(np.abs(lf["task"][0][k][0] - refs["poses"][k]).max() for k in range(2))
    return np.array(norms), moved


def id_fill(plan, leaf, model, q, qd, com_ref):
    """the numpy leaf of make_coman_id_momentum_stack (or of make_coman_id_stack) at the state (q, qd), from the restatements:
    -> (leaf, momentum [B][6])"""
    from test_dynamics_host import coman_fill_leaf, coman_quantities
    B, nv = q.shape
    Q = coman_quantities(model, q, qd, "ref")
    lf = coman_fill_leaf(leaf, Q, q, qd, Q["com"] if com_ref is None else com_ref)
    mom = momentum_ref.batch(model, q, qd)
    m = leaf["state"].get("momentum")
    if m is not None:
        A1 = np.zeros((B, 3, plan.n))
        A1[:, :, :nv] = mom["cmm"][:, 3:]
        b = m["lam"] * np.einsum("ij,bj->bi", np.asarray(m["K"]), -mom["momentum"][:, 3:])       # L_d = 0, Ldot_d = 0
        lf["A"] = [lf["A"][0], A1, None]
        lf["task"] = [lf["task"][0], [(b, None, None)], lf["task"][1]]
    return lf, mom["momentum"], Q["com"]


def id_assemble(plan, lf):
    """the oracle's assembled problem of a filled inverse-dynamics leaf (the wrench rows through their generic twin, tests/surface_ref.py)"""
    from surface_ref import generic_twin
    return pyoracle.assemble(*generic_twin(plan, lf))


def id_loop(make, B, steps, seed, dt=1e-3):
    """the inverse-dynamics closed loop on the CPU, restatements -> oracle solve -> explicit integration: max|angular momentum| [steps][B]"""
    plan, leaf, model = make(B, seed=seed)
    q, qd, com_ref, out = leaf["state"]["q0"].copy(), leaf["state"]["qdot0"].copy(), None, []
    for _ in range(steps):
        lf, mom, com = id_fill(plan, leaf, model, q, qd, com_ref)
        com_ref = com if com_ref is None else com_ref
        res = pyoracle.ihqp_solve_batch(id_assemble(plan, lf), pyoracle.BE_EIQP_EQ, nthreads=4)
        assert (res["status"] == 1).all(), res["status"]
        out.append(np.abs(mom[:, 3:]).max(axis=1))
        qdd = res["dq"][:, :model.n]
        q = q + dt * qd + 0.5 * dt * dt * qdd
        qd = qd + dt * qdd
    return np.array(out)
