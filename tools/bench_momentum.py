"""What the centroidal momentum outputs of osot_dynamics cost: the dynamics producer on COMAN (35 coordinates) at B = 4096,
    (a) the existing outputs only (M, h, Jdot qdot of every frame and of the CoM)
    (b) the same call with every momentum output added (cmm_lin, cmm_ang, momentum, ang_mom_b)
and, with --parent-lib, (a) through a second build of the library (the parent commit's), in the SAME process and alternating with this
build's, so that the two see the same machine.  A sample is the event-bracketed time of --reps back-to-back calls of one prebuilt batch
(GPU-bound: a call returns before its kernel ends) divided by --reps; --rounds samples per variant, taken round-robin.  Reported: the
median and the spread (min .. max) of every variant's samples, and the ratios of the medians.  The outputs of (a) are compared bit for
bit between the variants first.

    python tools/bench_momentum.py [--parent-lib PATH] [--out profiles/momentum_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opensot_amd import abi                         # noqa: E402
from opensot_amd import kinematics as kin           # noqa: E402
from opensot_amd.dynamics import Dynamics           # noqa: E402


class Handle:
    """an osot_dyn handle of a library given by path (the parent build): the same two entry points, no other state"""

    def __init__(self, path, model, gravity=(0.0, 0.0, -9.81)):
        self.lib = C.CDLL(path)
        self.h = C.c_void_p()
        kd, dd = model.desc(), abi.DynDesc()
        for j in range(model.n):
            for i in range(6):
                dd.inertia[j][i] = float(model.inertia[j][i])
        for i in range(3):
            dd.gravity[i] = float(gravity[i])
        assert self.lib.osot_dyn_create(C.byref(kd), C.byref(dd), 0, C.byref(self.h)) == 0

    def call(self, batch, stream):
        assert self.lib.osot_dynamics(self.h, C.byref(batch), stream) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a build of libosot_mi355x.so from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU"
    gold = os.path.join(ROOT, "tests", "golden")
    m, _, _ = kin.from_json(os.path.join(gold, "coman_tree.json"), os.path.join(gold, "coman_inertia.json"))
    B, n, F = args.B, m.n, len(m.frames)
    f64 = dict(dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.rand((B, n), generator=g, **f64) - 0.5
    qd = (torch.rand((B, n), generator=g, **f64) - 0.5) * 2
    e = lambda *s: torch.empty(s, **f64)

    def outputs():
        return dict(M=e(B, n, n), h=e(B, n), jd=e(B, 6 * F), cj=e(B, 3))
    dyn = Dynamics(m, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def batch(o, new):
        kw = {}
        if new:
            o.update(lin=e(B, 3, n), ang=e(B, 3, n), mom=e(B, 6), b=e(B, 3), ref=torch.zeros((B, 3), **f64))
            kw = dict(cmm_lin=o["lin"], cmm_ang=o["ang"], momentum=o["mom"], ang_mom_b=dict(out=o["b"], ref=o["ref"], lam=1.0))
        return dyn.batch_args(q, qd, M=o["M"], h=o["h"], frame_jdotqdot={f: (o["jd"], 6 * f) for f in range(F)}, com_jdotqdot=o["cj"], **kw)
    this = lambda b: abi.check(dyn._lib.osot_dynamics(dyn._h, C.byref(b), stream), "osot_dynamics")
    variants = {}
    if args.parent_lib:
        parent = Handle(args.parent_lib, m)
        o = outputs()
        variants["(a) existing outputs, parent build"] = (o, batch(o, False), lambda b: parent.call(b, stream))
    o = outputs()
    variants["(a) existing outputs, this build"] = (o, batch(o, False), this)
    o = outputs()
    variants["(b) with the momentum outputs, this build"] = (o, batch(o, True), this)
    for o, b, call in variants.values():            # warm up, then: the existing outputs are the same bits everywhere
        call(b)
    torch.cuda.synchronize()
    first = next(iter(variants.values()))[0]
    for name, (o, _, _) in variants.items():
        for k in ("M", "h", "jd", "cj"):
            assert torch.equal(o[k], first[k]), (name, k)
    samples = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, (o, b, call) in variants.items():
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                call(b)
            z.record(); torch.cuda.synchronize()
            samples[name].append(a.elapsed_time(z) / args.reps * 1e3)
    lines = [f"osot_dynamics, coman35 (n = {n}, {F} frames), B = {B}: microseconds per call; {args.rounds} samples of {args.reps} calls each, round-robin",
             "M, h, frame Jdot qdot and com Jdot qdot are bit-identical between the variants"]
    med = {}
    for name, s in samples.items():
        med[name] = statistics.median(s)
        lines.append(f"{name:45s} median {med[name]:8.2f}  min {min(s):8.2f}  max {max(s):8.2f}")
    names = list(variants)
    if args.parent_lib:
        lines.append(f"(a) this build / parent build: {med[names[1]] / med[names[0]]:.4f}")
    lines.append(f"(b) / (a), this build: {med[names[-1]] / med[names[-2]]:.4f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
