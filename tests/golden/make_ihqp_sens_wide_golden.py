"""tests/golden/make_ihqp_sens_wide_golden.py -- writes tests/golden/ihqp_sens_wide.npz: the fixture of the per-level multiplier tests
of the wide route (65 .. 128 variables).  It follows make_ihqp_sens_golden.py.

For the cases (p) .. (t) of ihqp_sens_wide_ref.cases(): inputs from ihqp_sens_ref.draw, and per instance the reference's cascade --
every active level's QP (the float64 restatement ihqp_sens_ref.restate_level_qp, with the optimality bounds from the reference's own
x of the levels above) solved by the reference's qpOASES (oracle.pyref.RefBackEnd: needs oracle/_ref, which build() makes where the
reference is present): x_levels, y = getDual() and getObjective() per level, and a seeded grad_dq.  Data only.

An instance is kept only if, by the reference's numbers alone, every multiplier of an active inequality and every gap of an inactive
side is at least 1e-6 at EVERY level (qp_sens_ref.margins_ok per level).  At most one instance in four may be dropped per case:
asserted here; a case that cannot meet it needs another generator (a looser box, fewer rows), not another cap.

    python tests/golden/make_ihqp_sens_wide_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from oracle import pyref          # noqa: E402
import ihqp_sens_wide_ref as W    # noqa: E402
import qp_sens_ref                # noqa: E402


def reference_chain(case, inp, i):
    """-> (ok, x_levels [L][n], [y_k], objective [L]) of instance i by the reference's qpOASES, level by level"""
    p, n = case.plan, case.plan.n
    xl, ys, obj = np.zeros((p.L, n)), [], np.zeros(p.L)
    for k in range(p.L):
        rows = case.rows(k)
        if not case.active(k):
            ys.append(np.zeros(n + rows))
            continue
        q = W.restate_level_qp(case, inp, i, k, xl)
        be = pyref.RefBackEnd(n, rows, pyref.HST_SEMIDEF, W.EPS_FACTOR)
        assert be.eps_abs == W.EPS_ABS
        if not be.initProblem(q["H"], q["g"], q["A"] if rows else None, q["lA"] if rows else None, q["uA"] if rows else None, q["l"], q["u"]):
            return False, xl, ys, obj
        xl[k], y = be.getSolution(), be.getDual()
        obj[k] = be.getObjective()
        ys.append(y)
        if not qp_sens_ref.margins_ok(q["A"] if rows else None, q["lA"], q["uA"], q["l"], q["u"], xl[k], y):
            return False, xl, ys, obj
    return True, xl, ys, obj


def main():
    assert pyref.available(), "oracle/_ref is missing: run build() where the reference is present"
    out = {"eps_abs": np.float64(W.EPS_ABS)}
    for name, case in W.cases().items():
        p = case.plan
        rng = np.random.default_rng([ord(name), p.n, p.L, case.B, 2024])
        kept, dropped = [], 0
        while len(kept) < case.B:
            inp = W.draw(case, rng, 1)
            ok, xl, ys, obj = reference_chain(case, inp, 0)
            if not ok:
                dropped += 1
                assert 3 * dropped <= case.B, f"case {name}: more than one instance in four is dropped"
                continue
            kept.append((inp, xl, ys, obj))
        cat = lambda f: np.concatenate([f(kp[0]) for kp in kept])
        for k in range(p.L):
            if p.ma(k):
                out[f"{name}_A{k}"] = cat(lambda q: q["A"][k])
            out[f"{name}_b{k}"] = cat(lambda q: q["b"][k])
            out[f"{name}_w{k}"] = cat(lambda q: q["w"][k])
            out[f"{name}_y{k}"] = np.stack([kp[2][k] for kp in kept])
        for key in ("C", "lo", "up", "l", "u"):
            if kept[0][0][key] is not None:
                out[f"{name}_{key}"] = cat(lambda q: q[key])
        out[f"{name}_x_levels"] = np.stack([kp[1] for kp in kept])
        out[f"{name}_objective"] = np.stack([kp[3] for kp in kept])
        out[f"{name}_grad_dq"] = rng.normal(size=(case.B, p.n))
        print(f"case {name}: {dropped} of {len(kept) + dropped} instances dropped, non-zero multipliers per instance and level (bounds, rows) "
              f"{[[(int(np.count_nonzero(y[:p.n])), int(np.count_nonzero(y[p.n:]))) for y in kp[2]] for kp in kept]}")
    path = os.path.join(HERE, "ihqp_sens_wide.npz")
    np.savez(path, **out)
    print(f"{os.path.relpath(path, os.path.dirname(os.path.dirname(HERE)))}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
