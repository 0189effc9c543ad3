"""Throughput of the inverse-dynamics control step with SURFACE contacts (6-D wrenches: force::FrictionCone, force::CoP,
force::NormalTorque rows; synth.make_surface_id_stack) on both routes:
    osot_id_rows  ->  osot_cycle (update + cascade)  ->  osot_computed_torque
n = 56 (nv 32, 4 contacts: wavefront route), 68 (nv 44, 4), 86 (nv 56, 5) and 128 (nv 80, 8) (wide route).  The timed steps are
ONE captured HIP graph of --steps control steps, replayed over a window of at least --window seconds.  One JSON line per size.

Per-kernel times come from a separate profiler run of a few replays of one size (--replays R --window 0), e.g.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o surf -- python tools/bench_surface_id.py --sizes 68 --replays 3
and  --kernel-stats CSV --sizes 68  turns the stats file into one JSON line: average time of each kernel, and for the ID producers
the bytes they move (from the shapes) over their time, against the 8 TB/s HBM spec and the ~6.3 TB/s a copy achieves.
    python tools/bench_surface_id.py [--sizes 56,68,86,128] [--B 4096] [--steps 10] [--window 0.5]"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from opensot_amd import synth

SIZES = {56: (32, 4), 68: (44, 4), 86: (56, 5), 128: (80, 8)}
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.3


def producer_bytes(n):
    """bytes one instance moves through the ID producers (read + write, from the shapes): osot_id_rows_kernel reads B (nv x nv),
    the contact Jacobians (6 contacts x nv) and the task Jacobians (15 x nv) and writes 6 + nv rows of C and 15 rows of A_0;
    osot_torque_kernel reads B, the contact Jacobians, h and x and writes tau"""
    nv, nc = SIZES[n]
    nf = 6 * nc
    rows = 8 * (nv * nv + nf * nv + 15 * nv + (6 + nv + 15) * n)
    tau = 8 * (nv * nv + nf * nv + nv + n + nv) + 4
    return {"osot_id_rows_kernel": rows, "osot_torque_kernel": tau}


def setup(n, B):
    import torch
    from opensot_amd.dynamics import IdModel
    from opensot_amd.solver import BatchedStack
    nv, nc = SIZES[n]
    plan, leaf = synth.make_surface_id_stack(B, seed=n, nv=nv, n_contacts=nc)
    st = BatchedStack(plan, B, device=0, want_levels=False)
    bare = dict(leaf); bare["A"] = [np.zeros_like(leaf["A"][0]), None]; bare["C"] = [None] * len(plan.rowblocks)
    dev = st.load_leaf(bare)
    md = IdModel(leaf["model"]["B"], leaf["model"]["h"], leaf["model"]["Jc"], device=0)
    J = [torch.as_tensor(np.ascontiguousarray(leaf["A"][0][:, o:o + r, :nv])).to(st.device) for o, r in ((0, 3), (3, 6), (9, 6))]
    tasks = [(0, 0, J[0]), (0, 3, J[1]), (0, 9, J[2])]
    out = {}

    def step():
        md.write_rows(st, dyn_block=0, tau_block=4, tasks=tasks)
        st.cycle(dev, cached=True)
        out["tau"], out["ok"] = md.computed_torque(st.dq[:B])
    return plan, st, step, out


def run(n, B, steps, window, replays):
    import torch
    plan, st, step, out = setup(n, B)
    s = torch.cuda.Stream()
    st.stream = s
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(steps):
            step()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    reps, el = max(replays, 1), 0.0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        el = e0.elapsed_time(e1) * 1e-3
        if replays or el >= window:
            break
        reps = max(reps + 1, int(reps * 1.5 * window / max(el, 1e-6)))
    t_step = el / (reps * steps)
    solved = int((st.status[:B] == 0).sum().item())
    ok = int(out["ok"].sum().item())
    nv, nc = SIZES[n]
    return {"tool": "bench_surface_id", "n": n, "nv": nv, "contacts": nc, "B": B, "route": st.route,
            "rows": {"levels": [plan.m(k) for k in range(plan.L)], "nc": plan.nc, "nc_stored": plan.nc_stored},
            "solves_per_s": B / t_step, "step_ms": 1e3 * t_step, "steps_per_graph": steps, "replays": reps,
            "solved": solved, "torque_ok": ok, "iterations_mean": float(st.iterations[:B].double().mean().item())}


def kernel_stats(path, n, B):
    rows = list(csv.DictReader(open(path)))
    line = {"tool": "bench_surface_id", "kernel_stats": os.path.basename(path), "n": n, "B": B, "kernels": {}}
    by = producer_bytes(n)
    for r in rows:
        name = r["Name"]
        avg_us = float(r["AverageNs"]) / 1e3
        short = name.split("(")[0].replace("void ", "").replace("osot::", "")
        short = short.split("<")[0] + ("<" + short.split("<", 1)[1] if "<" in short else "")
        e = {"calls": int(r["Calls"]), "average_us": avg_us, "percentage": float(r["Percentage"])}
        base = short.split("<")[0]
        if base in by:
            tbs = B * by[base] / (avg_us * 1e-6) / 1e12
            e.update(bytes_per_instance=by[base], tb_per_s=tbs, frac_of_spec=tbs / HBM_SPEC_TBS, frac_of_copy=tbs / HBM_COPY_TBS)
        line["kernels"][short] = e
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="56,68,86,128")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--replays", type=int, default=0, help="a fixed number of graph replays (profiler runs); 0 = time a window")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of one size: print its summary and exit")
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    if a.kernel_stats:
        print(json.dumps(kernel_stats(a.kernel_stats, sizes[0], a.B)), flush=True)
        return
    for n in sizes:
        print(json.dumps(run(n, a.B, a.steps, a.window, a.replays)), flush=True)


if __name__ == "__main__":
    main()
