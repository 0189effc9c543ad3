"""Throughput of the posture-gradient producer (osot_posture_gradient, opensot_amd/csrc/osot_grad.h) on the reference's COMAN with one
wrist manipulability term plus the minimum-effort term, against the only device route there was before it: the reference's own loop,
2 n osot_kinematics launches on perturbed postures with the wrist's and the CoM's Jacobians left on the device (the determinants and
quadratic forms that would still follow are NOT counted, in the brute-force route's favour).  Also the producer's share of one control
step (producer + osot_control_cycle of synth.make_coman_manipulability_stack).  One JSON line.
Timing: warm-up, device events around a window of at least --window seconds.
    python tools/bench_posture_gradient.py [--batch 4096] [--window 0.5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opensot_amd import abi, synth
from opensot_amd import kinematics as kin
from opensot_amd.gradient import PostureGradient, posture_term
from opensot_amd.solver import BatchedStack


def timed(fn, window):
    """device-event time (s) per call of fn over a window of at least `window` seconds, after a warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        el = e0.elapsed_time(e1) * 1e-3
        if el >= window:
            return el / reps, reps
        reps = max(reps + 1, int(reps * 1.5 * window / max(el, 1e-6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    B = a.batch
    f64 = dict(dtype=torch.float64, device="cuda:0")
    model, _, _ = kin.from_json(os.path.join(ROOT, "tests", "golden", "coman_tree.json"))
    n = model.n
    W = np.ones(n); W[:6] = 0.0
    fw = model.frame_index("l_wrist")
    terms = [posture_term(abi.GRAD_MANIPULABILITY_FRAME, frame=fw, W=W), posture_term(abi.GRAD_MIN_EFFORT, W=np.full(n, 1e-5))]
    rng = np.random.default_rng(1)
    q = torch.as_tensor(rng.uniform(-0.8, 0.8, (B, n)), **f64).contiguous()
    g = PostureGradient(model, terms, device=0)
    outs = [torch.zeros((B, n), **f64) for _ in terms]
    gb = g.batch_args(q, b=dict(enumerate(outs)))
    t_grad, reps = timed(lambda: g.forward(q, batch=gb), a.window)

    # the brute-force route: 2 n launches of the kinematics producer, each on its own perturbed copy of q, Jacobians kept on the device
    K = kin.Kinematics(model, device=0)
    step = 1e-3
    qs = q[None, :, :].repeat(2 * n, 1, 1)
    for i in range(n):
        qs[2 * i, :, i] += step
        qs[2 * i + 1, :, i] -= step
    Jf = torch.zeros((2 * n, B, 6, n), **f64)
    Jc = torch.zeros((2 * n, B, 3, n), **f64)
    kbs = [K.batch_args(qs[k], frame_J={fw: (Jf[k], 0)}, com_J=(Jc[k], 0)) for k in range(2 * n)]
    lib, stream = abi.lib(), torch.cuda.current_stream().cuda_stream
    import ctypes as C

    def brute():
        for kb in kbs:
            abi.check(lib.osot_kinematics(K._h, C.byref(kb), C.c_void_p(stream)), "osot_kinematics")
    t_brute, _ = timed(brute, a.window)

    # share of one control step: producer + fused control cycle of the manipulability stack
    plan, leaf, m2, t2 = synth.make_coman_manipulability_stack(B, seed=4)
    st = BatchedStack(plan, B, device=0, want_levels=False)
    K2, g2 = kin.Kinematics(m2, device=0), PostureGradient(m2, t2, device=0)
    dev, gb2, kb2, q2 = synth.bind_posture_gradient(st, g2, leaf, kin=K2)
    t_g2, _ = timed(lambda: g2.forward(q2, batch=gb2), a.window)
    t_cycle, _ = timed(lambda: st.control_cycle(K2, kb2, dev), a.window)
    print(json.dumps({"bench": "posture_gradient", "B": B, "n": n, "terms": "l_wrist manipulability + minimum effort",
                      "producer_ms": 1e3 * t_grad, "producer_instances_per_s": B / t_grad, "producer_reps": reps,
                      "brute_force_ms": 1e3 * t_brute, "brute_force_instances_per_s": B / t_brute, "brute_force_launches": 2 * n,
                      "ratio_producer_over_brute_force": t_brute / t_grad,
                      "control_step": {"stack": "make_coman_manipulability_stack", "producer_two_wrists_ms": 1e3 * t_g2,
                                       "control_cycle_ms": 1e3 * t_cycle, "producer_share": t_g2 / (t_g2 + t_cycle)}}))


if __name__ == "__main__":
    main()
