"""tools/bench_kin_rows.py -- what the row sets cost osot_kinematics: the wheeled tree of synth.make_wheeled_stack (26 coordinates, the four
PureRolling sets and the OmniWheels4X set) at B = 4096, the SAME model and the same other outputs (the base's pose and Jacobian) with
and without the row-set outputs bound.  The yardstick is the launch without them; the cost is reported as a ratio.

    python tools/bench_kin_rows.py [--batch 4096] [--steps 2000] [--warmup 20] [--repeats 5] [--out profiles/kin_rows_bench.txt]

The two variants ALTERNATE, `repeats` runs each; per run the time of `steps` back-to-back launches between two device events.  Median
and spread (min .. max) of each, and the ratio of the medians; --out writes the summary lines and the JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from opensot_amd import kinematics as kin, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.batch
    plan, leaf, model = synth.make_wheeled_stack(B, seed=0, omni=True)
    n, legs = model.n, len(model.wheel_joints)
    K = kin.Kinematics(model, device=0)
    f64 = dict(dtype=torch.float64, device=torch.device("cuda", 0))
    q = torch.as_tensor(leaf["state"]["q0"], **f64).contiguous()
    pose, A1 = torch.zeros((B, 12), **f64), torch.zeros((B, 6, n), **f64)
    A0, Crows = torch.zeros((B, 4 * legs, n), **f64), torch.zeros((B, 3, n), **f64)
    base = dict(frame_pose={0: pose}, frame_J={0: (A1, 0)})
    rows = dict(base, rowset_A={**{i: (A0, 4 * i) for i in range(legs)}, legs: (Crows, 0)})
    batches = {"without": K.batch_args(q, **base), "with": K.batch_args(q, **rows)}

    def run(kb):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            K.forward(q, batch=kb)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.steps          # microseconds per launch

    for kb in batches.values():
        for _ in range(a.warmup):
            K.forward(q, batch=kb)
    torch.cuda.synchronize()
    times = {k: [] for k in batches}
    for _ in range(a.repeats):
        for k, kb in batches.items():
            times[k].append(run(kb))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"bench": "kin_rows", "batch": B, "n": n, "steps": a.steps, "repeats": a.repeats, "row_sets": legs + 1, "rows": 4 * legs + 3,
           "us_per_launch": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in times.items()},
           "ratio_with_over_without": med["with"] / med["without"],
           "bytes_written_per_instance": {"without": 8 * (12 + 6 * n), "with": 8 * (12 + 6 * n + (4 * legs + 3) * n)}}
    line = json.dumps(res)
    text = summary(res) + "the JSON line:\n" + line + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def summary(r):
    """the lines of profiles/kin_rows_bench.txt in front of the JSON line"""
    w, wo = r["us_per_launch"]["with"], r["us_per_launch"]["without"]
    bw, bwo = r["bytes_written_per_instance"]["with"], r["bytes_written_per_instance"]["without"]
    B = r["batch"]
    return (f"tools/bench_kin_rows.py: osot_kinematics on the wheeled tree of synth.make_wheeled_stack ({r['n']} coordinates), B = {B}, the same\n"
            f"model and the same other outputs (the base's pose and Jacobian) WITHOUT and WITH its {r['row_sets']} row sets bound ({r['rows']} rows of\n"
            f"{r['n']} doubles per instance).  The two alternate, {r['repeats']} runs each of {r['steps']} back-to-back launches between two device events.\n\n"
            f"  without row sets: median {wo['median']:.3f} us per launch (min {wo['min']:.3f}, max {wo['max']:.3f}); {bwo} bytes written per instance\n"
            f"  with row sets:    median {w['median']:.3f} us per launch (min {w['min']:.3f}, max {w['max']:.3f}); {bw} bytes written per instance\n"
            f"  ratio with / without: {r['ratio_with_over_without']:.3f} in time, {bw / bwo:.3f} in bytes written\n"
            f"  bytes written over time: {B * bwo / wo['median'] * 1e-6:.3f} TB/s without, {B * bw / w['median'] * 1e-6:.3f} TB/s with\n"
            "  (the yardstick is the launch without the sets; no threshold was set in advance)\n\n")


if __name__ == "__main__":
    main()
