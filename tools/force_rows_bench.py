"""Throughput of the force-space row producer (osot_force_rows) and of the whole wrench-distribution cycle (dynamics.ForceStep.step():
osot_kinematics, osot_dynamics twice, osot_force_rows, osot_cycle) on the COMAN force stacks of synth.make_coman_force_stack:
form "com" (n = 12) and form "static" (n = 41).  One JSON line per form:
    rows_per_s ......... instances per second through osot_force_rows alone
    algorithmic_bytes .. what one instance must move (read + write, from the shapes) and the bytes per second that makes; the HBM can
                         move no more than its 8 TB/s, so traffic / algorithmic bytes <= 8 TB/s / achieved
    steps_per_s ........ ForceStep.step() per second (B instances each)
Timing: warm-up, then ONE captured graph of --launches launches replayed between two events on one stream, the best of --repeats.
    python tools/force_rows_bench.py [--B 4096] [--launches 50] [--repeats 7] [--out profiles/force_rows.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opensot_amd import synth

HBM_SPEC_TBS = 8.0


def algorithmic_bytes(form, nv=35, C=2):
    """bytes one instance moves through osot_force_rows (read + write, from the shapes)"""
    na = nv - 6
    if form == "com":      # reads the poses' origins, the CoM, the momentum, the references, the mask; writes 6 rows of 6 C columns and b
        return 8 * (3 * C + 3 + 6 + 5 * 3 + 6 * 6 * C + 6) + 4 * C
    # reads the contact Jacobians, the gravity term, the mask; writes 6 + na rows of 6 C columns, the identity block, lo and up
    return 8 * (6 * C * nv + nv + 6 * 6 * C + na * (6 * C + na) + 2 * na) + 4 * C


def timed(fn, stream, launches, repeats):
    import torch
    with torch.cuda.stream(stream):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for _ in range(launches):
            fn()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3 / launches)
    return min(times), sorted(times)[len(times) // 2]


def run(form, B, launches, repeats):
    import torch
    from opensot_amd.dynamics import ForceStep
    plan, leaf, model = synth.make_coman_force_stack(B, form)
    step = ForceStep(plan, leaf, model, device=0)
    s = torch.cuda.Stream()
    step.st.stream = s
    with torch.cuda.stream(s):
        step.step()
    torch.cuda.synchronize()
    t_rows, t_rows_med = timed(lambda: step.model.write_rows(step._fb, step.st.device), s, launches, repeats)
    t_step, t_step_med = timed(step.step, s, max(launches // 5, 1), repeats)
    by = algorithmic_bytes(form)
    tbs = B * by / t_rows / 1e12
    return {"tool": "force_rows_bench", "form": form, "n": plan.n, "B": B, "launches_per_timing": launches, "repeats": repeats,
            "rows_us": 1e6 * t_rows, "rows_us_median": 1e6 * t_rows_med, "rows_per_s": B / t_rows,
            "algorithmic_bytes": by, "algorithmic_tb_per_s": tbs, "traffic_over_algorithmic_at_most": HBM_SPEC_TBS / tbs,
            "step_us": 1e6 * t_step, "step_us_median": 1e6 * t_step_med, "steps_per_s": 1.0 / t_step, "instances_per_s": B / t_step,
            "solved": int((step.st.status[:B] == 0).sum().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the lines, the commit and the device name to this file")
    a = ap.parse_args()
    import torch
    lines = [json.dumps(run(form, a.B, a.launches, a.repeats)) for form in ("com", "static")]
    for l in lines:
        print(l, flush=True)
    if a.out:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = "unknown"
        with open(a.out, "w") as f:
            f.write(f"tools/force_rows_bench.py --B {a.B} --launches {a.launches} --repeats {a.repeats}\n")
            f.write(f"commit (parent of the measured tree): {commit}\ndevice: {torch.cuda.get_device_name(0)}\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
