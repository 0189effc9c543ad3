"""osot_acc_tasks on the COMAN shape (nv = 35) against the torch expressions of dynamics.IdStep.consume it replaces.

    python tools/acc_tasks_bench.py [--B 4096] [--launches 200] [--repeats 7]

Every timing: warm-up, then one captured graph of N repetitions replayed between two events on one stream; best and median of the
repeats.  Three subjects, on the tensors one produce() of the step left on the device:
    torch      the four element-wise / reduction statements of IdStep.consume (CoM and postural errors: scalar gains, no matrices)
    acc        osot_acc_tasks of synth.make_coman_id_tracking_stack, gain_type Acceleration (the same errors, plus the hand's pose
               and velocity errors, its gain matrices and the postural qddot_d with matrix gains: no factorisation)
    force      the same with GainType::Force (Cholesky of M, 6 + 1 right-hand sides)
    force+Minv the same with computeInertiaInverse bound
One JSON line per subject."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opensot_amd import abi, synth  # noqa: E402
from opensot_amd.dynamics import IdStep, IdTrackingStep  # noqa: E402


def timed(fn, launches, repeats):
    """microseconds per call of fn: (best, median) over `repeats` replays of a graph of `launches` calls"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(launches):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / launches)
    return min(out), statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "acc_tasks_bench needs a GPU"
    B = a.B
    plan, leaf, model = synth.make_coman_id_stack(B, seed=31)
    base = IdStep(plan, leaf, model, device=0)
    base.produce()
    base.com_ref = base.com.clone()
    nv = base.nv

    def torch_leaves():
        base.p0_com[:, :3] = base.com_ref - base.com
        base.p0_com[:, 3:] = -(base.Jcom * base.qdot[:, None, :]).sum(dim=2)
        base.p0_post[:, :nv] = base.q_ref - base.q
        base.p0_post[:, nv:] = -base.qdot
    subjects = [("torch", torch_leaves, None)]
    keep = []
    for name, gt, minv in (("acc", abi.ACC_GAIN_ACCELERATION, False), ("force", abi.ACC_GAIN_FORCE, False), ("force+Minv", abi.ACC_GAIN_FORCE, True)):
        p, lf, m = synth.make_coman_id_tracking_stack(B, gain_type=gt, seed=31)
        st = IdTrackingStep(p, lf, m, device=0)
        st.produce()
        st.consume()
        torch.cuda.synchronize()
        assert (st.acc_ok == 1).all()
        extra = {}
        if minv:
            extra["Minv"] = torch.zeros((B, nv, nv), dtype=torch.float64, device=st.st.device)
        batch = st.acc.batch_args(B, **st.acc_args, **extra)        # the step's own bindings, in a batch of this tool's
        keep.append(extra)
        keep.append(st)
        subjects.append((name, (lambda s=st, b=batch: s.acc.forward(b)), st))
    for name, fn, st in subjects:
        best, med = timed(fn, a.launches, a.repeats)
        print(json.dumps({"tool": "acc_tasks_bench", "subject": name, "B": B, "nv": nv, "launches_per_timing": a.launches, "repeats": a.repeats,
                          "us": best, "us_median": med, "instances_per_s": B / (best * 1e-6)}), flush=True)


if __name__ == "__main__":
    main()
