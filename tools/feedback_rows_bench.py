"""Launch time of the measurement-driven producer (osot_feedback) on the COMAN shape: nv = 35, two Cartesian admittance terms, the
joint filter with a dense compliance, the IMU rows, the contact error and 16 collision pair rows of n = 35 columns, every group bound.
One JSON line with the dense compliance, one with the scalar one:
    us ................. microseconds per launch
    algorithmic_bytes .. what one instance must move (read + write, from the shapes) and the bytes per second that makes; the HBM can
                         move no more than its 8 TB/s, so traffic / algorithmic bytes <= 8 TB/s / achieved
Timing: warm-up, then ONE captured graph of --launches launches replayed between two events on one stream, the best of --repeats.
    python tools/feedback_rows_bench.py [--B 4096] [--launches 50] [--repeats 7] [--out profiles/feedback_rows.txt]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC_TBS = 8.0


def algorithmic_bytes(nv=35, n_cart=2, n_pairs=16, n=35):
    """bytes one instance moves through osot_feedback (read + write, from the shapes); the dense compliance is one matrix for the
    batch and is not counted"""
    count = 4 * (6 * n_cart + nv)
    doubles = 2 * count                                # the filter state, read and rewritten
    doubles += n_cart * (12 + 6 + 6)                   # pose, wrench, twist_out of every term
    doubles += 3 * nv                                  # tau, h, qdot_out
    doubles += 18 + 12 + 3 + 18 + 6                    # IMU: rows 3 .. 5 of fb_J's six columns, pose, omega; 18 + 18 of A, b
    doubles += 12 + 12 + 6 + 6                         # contact: two poses, b_in, b_out
    doubles += n_pairs * (2 * n + 2)                   # J and A rows, dist and b
    return 8 * doubles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the line, the commit and the device name to this file")
    a = ap.parse_args()
    import torch
    lines = [run(a, dense) for dense in (True, False)]
    if a.out:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = "unknown"
        with open(a.out, "w") as fh:
            fh.write(f"tools/feedback_rows_bench.py --B {a.B} --launches {a.launches} --repeats {a.repeats}\n")
            fh.write(f"commit (parent of the measured tree): {commit}\ndevice: {torch.cuda.get_device_name(0)}\n")
            fh.write("\n".join(lines) + "\n")


def run(a, dense):
    """one JSON line: the COMAN shape with the dense compliance, or with the scalar one (no staging through LDS)"""
    import torch
    from opensot_amd.feedback import Feedback, FeedbackModel
    B, nv, P, n = a.B, 35, 16, 35
    rng = np.random.default_rng(0)
    model = FeedbackModel(nv, floating_base=True, imu=True, contact_lambda=0.5, n_pairs=P, n=n, ca_threshold=0.01)
    for _ in range(2):
        t = model.add_cartesian_admittance(**FeedbackModel.cartesian_admittance_defaults())
        model.set_raw_params(t, np.full(6, 1e-4), np.full(6, 50.0), 0, 0.002)
    model.set_joint_admittance(**FeedbackModel.joint_admittance_defaults())
    f = Feedback(model, B, device=0)
    tn = lambda *s: torch.as_tensor(rng.uniform(-1.0, 1.0, s), dtype=torch.float64, device="cuda:0").contiguous()
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    eye = torch.cat([torch.eye(3, dtype=torch.float64, device="cuda:0").reshape(9), z(3)])
    pose = lambda: (tn(B, 12) * 0.0 + eye).contiguous()
    f.bind(cart=[dict(pose=pose(), wrench=tn(B, 6), twist_out=z(B, 6)) for _ in range(2)],
           joint=dict(tau=tn(B, nv), h=tn(B, nv), qdot_out=z(B, nv), C=tn(nv, nv) * 1e-3 if dense else None),
           imu=dict(fb_J=tn(B, 6, nv), pose=pose(), omega=tn(B, 3), A=z(B, 6, 6), b=z(B, 6)),
           contact=dict(pose=pose(), pose_ref=pose(), b_in=tn(B, 6), b_out=z(B, 6)),
           ca=dict(J=tn(B, P, n), dist=tn(B, P) * 0.05, A=z(B, P, n), b=z(B, P)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(5):
            f.launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(a.launches):
            f.launch()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3 / a.launches)
    best, med = min(times), sorted(times)[len(times) // 2]
    by = algorithmic_bytes(nv, 2, P, n)
    tbs = B * by / best / 1e12
    line = json.dumps({"tool": "feedback_rows_bench", "B": B, "nv": nv, "n_cart": 2, "n_pairs": P, "n": n, "dense_C": dense,
                       "state_doubles": f.count, "launches_per_timing": a.launches, "repeats": a.repeats, "us": 1e6 * best,
                       "us_median": 1e6 * med, "instances_per_s": B / best, "algorithmic_bytes": by, "algorithmic_tb_per_s": tbs,
                       "traffic_over_algorithmic_at_most": HBM_SPEC_TBS / tbs, "finite": bool(torch.isfinite(f.state).all().item())})
    print(line, flush=True)
    return line


if __name__ == "__main__":
    main()
