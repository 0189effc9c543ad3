"""tests/golden/make_qp_sens_big_golden.py -- writes tests/golden/qp_sens_big.npz: the fixture of the multiplier / sensitivity tests
for 65 .. 128 variables (osot_qp_sensitivity_batch_ws).

As make_qp_sens_golden.py: inputs from helpers.random_qp at the shapes of qp_sens_big_ref.SHAPES; for each instance x and y of the
reference's own qpOASES (oracle.pyref.RefBackEnd.getSolution / getDual: needs oracle/_ref, which build() makes where the reference
is present) and a seeded grad_x.  With the reference alone it asserts that every instance is non-degenerate -- every active
inequality has |y| >= 1e-6, every inactive finite side a gap >= 1e-6 -- and draws an instance again otherwise.  Only data goes
into the file.

    python tests/golden/make_qp_sens_big_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from oracle import pyref          # noqa: E402
import helpers                    # noqa: E402
import qp_sens_ref                # noqa: E402
import qp_sens_big_ref            # noqa: E402
from make_qp_sens_golden import solve_reference   # noqa: E402


def main():
    assert pyref.available(), "oracle/_ref is missing: run build() where the reference is present"
    out = {}
    for s, (n, nc, n_eq, B) in enumerate(qp_sens_big_ref.SHAPES):
        rng = np.random.default_rng([n, nc, n_eq, B, 2026])
        keys = ("H", "g", "A", "lA", "uA", "l", "u")
        rows = {k: [] for k in keys + ("x", "y")}
        redrawn = 0
        while len(rows["x"]) < B:
            q = dict(zip(keys, helpers.random_qp(rng, 1, n, nc, n_eq=n_eq, box=True)))
            one = {k: (None if v is None else v[0]) for k, v in q.items()}
            ok, x, y, eps_abs = solve_reference(*[one[k] for k in keys])
            if not ok or not qp_sens_ref.margins_ok(one["A"], one["lA"], one["uA"], one["l"], one["u"], x, y):
                redrawn += 1
                assert redrawn < 4 * B + 4, "too many degenerate draws"
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
    path = os.path.join(HERE, "qp_sens_big.npz")
    np.savez(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
