"""Throughput of the rigid-body dynamics producer alone (osot_dynamics: M, h, Jdot qdot of every frame and of the CoM) next to the
kinematics producer on the same model and batch (osot_kinematics: every frame Jacobian, CoM and its Jacobian), with the time the
producer's algorithmic bytes would take at an ASSUMED memory bandwidth (--hbm-gbs; at B = 4096 the outputs fit in the last-level
cache, so only the large batch is a comparison with HBM), and the captured inverse-dynamics control step on the COMAN stack with and
without the two producer launches.  The times are CALL times (event-bracketed launches, host argument building included); kernel
times come from a rocprofv3 --kernel-trace --stats run of this tool.  One JSON line per measurement.

    python tools/bench_dynamics.py [--out profiles/dynamics_bench.jsonl] [--hbm-gbs 4000]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opensot_amd import kinematics as kin          # noqa: E402
from opensot_amd.dynamics import Dynamics          # noqa: E402


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def bench_step(reps, B=4096):
    """the captured inverse-dynamics control step on the COMAN stack (kinematics + dynamics + leaf errors + id_rows + cycle +
    computed torque + integration) with and without the two producer launches, per graph replay"""
    from opensot_amd import synth
    from opensot_amd.dynamics import IdStep
    out = []
    for producers in (True, False):
        plan, leaf, model = synth.make_coman_id_stack(B, seed=31)
        loop = IdStep(plan, leaf, model, device=0)
        loop.step(); torch.cuda.synchronize()
        q0, qd0 = loop.q.clone(), loop.qdot.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            loop.step(producers)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            loop.step(producers)

        def run():
            loop.q.copy_(q0); loop.qdot.copy_(qd0)      # every replay from the same state (two small copies inside the bracket)
            g.replay()
        t = timed(run, reps)
        torch.cuda.synchronize()
        ok = int((loop.st.status[:B] == 0).sum())
        out.append(dict(bench="coman_id_step_graph", B=B, n=plan.n, producers=producers, step_s=t, steps_per_s=B / t, solved=f"{ok}/{B}"))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="achievable HBM write bandwidth to compare against, GB/s")
    args = ap.parse_args()
    models = {"humanoid32": kin.humanoid32()}
    coman, _, _ = kin.from_json(os.path.join(ROOT, "tests", "golden", "coman_tree.json"), os.path.join(ROOT, "tests", "golden", "coman_inertia.json"))
    models["coman35"] = coman
    lines = []
    for name, m in models.items():
        n, F = m.n, len(m.frames)
        dyn, kn = Dynamics(m, 0), kin.Kinematics(m, 0)
        for B in (4096, 32768):
            g = torch.Generator(device="cuda").manual_seed(1)
            q = (torch.rand((B, n), dtype=torch.float64, device="cuda", generator=g) - 0.5)
            qd = (torch.rand((B, n), dtype=torch.float64, device="cuda", generator=g) - 0.5) * 2
            M = torch.empty((B, n, n), dtype=torch.float64, device="cuda"); h = torch.empty((B, n), dtype=torch.float64, device="cuda")
            jd = torch.empty((B, 6 * F), dtype=torch.float64, device="cuda"); cj = torch.empty((B, 3), dtype=torch.float64, device="cuda")
            A = torch.empty((B, 6 * F + 3, n), dtype=torch.float64, device="cuda"); com = torch.empty((B, 3), dtype=torch.float64, device="cuda")
            t_dyn = timed(lambda: dyn.forward(q, qd, M=M, h=h, frame_jdotqdot={f: (jd, 6 * f) for f in range(F)}, com_jdotqdot=cj), args.reps)
            t_kin = timed(lambda: kn.forward(q, frame_J={f: (A, 6 * f) for f in range(F)}, com=com, com_J=(A, 6 * F)), args.reps)
            by_dyn = 16 * n + 8 * n * n + 8 * n + 48 * F + 24
            by_kin = 8 * n + (6 * F + 3) * n * 8 + 24
            lines.append(dict(bench="dynamics_producer", model=name, n=n, frames=F, B=B,
                              dynamics_s=t_dyn, dynamics_instances_per_s=B / t_dyn, dynamics_bytes_per_instance=by_dyn,
                              dynamics_bytes_at_assumed_bw_s=B * by_dyn / (args.hbm_gbs * 1e9),
                              kinematics_s=t_kin, kinematics_instances_per_s=B / t_kin, kinematics_bytes_per_instance=by_kin,
                              hbm_gbs_assumed=args.hbm_gbs))
            print(json.dumps(lines[-1]), flush=True)
    lines += bench_step(args.reps)
    if args.out:
        with open(args.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
