"""tests/golden/make_qp_sens_golden.py -- writes tests/golden/qp_sens.npz: the fixture of the multiplier / sensitivity tests.

Inputs from helpers.random_qp at the shapes of qp_sens_ref.SHAPES; for each instance x and y of the reference's own qpOASES
(oracle.pyref.RefBackEnd.getSolution / getDual: needs oracle/_ref, which build() makes where the reference is present) and a seeded
grad_x.  With the reference alone it asserts that every instance is non-degenerate -- every active inequality has |y| >= 1e-6,
every inactive finite side a gap >= 1e-6 -- and draws an instance again otherwise.

    python tests/golden/make_qp_sens_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from oracle import pyref          # noqa: E402
import helpers                    # noqa: E402
import qp_sens_ref                # noqa: E402

EPS_FACTOR = 2e2


def solve_reference(H, g, A, lA, uA, l, u):
    n, nc = len(g), 0 if A is None else A.shape[0]
    be = pyref.RefBackEnd(n, nc, pyref.HST_SEMIDEF, EPS_FACTOR)
    inf = lambda a: None if a is None else np.clip(a, -1e20, 1e20)
    ok = be.initProblem(H, g, A, inf(lA), inf(uA), l, u)
    return ok, be.getSolution(), be.getDual(), be.eps_abs


def main():
    assert pyref.available(), "oracle/_ref is missing: run build() where the reference is present"
    out = {}
    for s, (n, nc, n_eq, B) in enumerate(qp_sens_ref.SHAPES):
        rng = np.random.default_rng([n, nc, n_eq, B, 2024])
        keys = ("H", "g", "A", "lA", "uA", "l", "u")
        rows = {k: [] for k in keys + ("x", "y")}
        redrawn = 0
        while len(rows["x"]) < B:
            q = dict(zip(keys, helpers.random_qp(rng, 1, n, nc, n_eq=n_eq, box=True)))
            one = {k: (None if v is None else v[0]) for k, v in q.items()}
            ok, x, y, eps_abs = solve_reference(*[one[k] for k in keys])
            if not ok or not qp_sens_ref.margins_ok(one["A"], one["lA"], one["uA"], one["l"], one["u"], x, y):
                redrawn += 1
                assert redrawn < 4 * B, "too many degenerate draws"
                continue
            for k in keys:
                rows[k].append(one[k])
            rows["x"].append(x); rows["y"].append(y)
        for k in keys + ("x", "y"):
            if rows[k][0] is not None:
                out[f"s{s}_{k}"] = np.stack(rows[k])
        out[f"s{s}_grad_x"] = rng.normal(size=(B, n))
        out["eps_abs"] = np.float64(eps_abs)
        print(f"shape {(n, nc, n_eq, B)}: {redrawn} instances drawn again, active per instance {[int(np.count_nonzero(y)) for y in rows['y']]}")
    path = os.path.join(HERE, "qp_sens.npz")
    np.savez(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
