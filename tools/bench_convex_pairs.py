"""tools/bench_convex_pairs.py -- kinematics instances per second of the 32-DoF humanoid with 16 CONVEX pairs (the producer's
CONVEX instantiation: per-lane GJK) next to the same model with its 16 capsule pairs (closed forms).  One JSON line.

    python tools/bench_convex_pairs.py [--batch 4096] [--steps 50] [--warmup 10]

Both models bind pair_dist and pair_J; times are device events around `steps` back-to-back launches."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def convex_model(kin):
    """the 16 pairs of humanoid32_pairs with boxes, cylinders and hulls in place of the capsules"""
    m = kin.humanoid32_pairs(kin.humanoid32())
    rng = np.random.default_rng(1)
    names = list(m.pair_names)
    S = m.link_shapes
    for k, (name, s) in enumerate(list(S.items())):
        j, a0, a1, r = s
        a0, a1 = np.asarray(a0, float), np.asarray(a1, float)
        c, hl = 0.5 * (a0 + a1), 0.5 * np.linalg.norm(a1 - a0)
        if k % 3 == 0:
            S[name] = dict(joint=j, kind="box", half=(r, r, hl + r), p=c)
        elif k % 3 == 1:
            S[name] = dict(joint=j, kind="cylinder", size=(r, 0.0, hl + r), p=c)
        else:
            S[name] = dict(joint=j, kind="hull", verts=rng.uniform(-1.0, 1.0, (16, 3)) * np.array([r, r, hl + r]), p=c)
    m.pairs = [m.link_pair(a, b) for a, b in names]
    m.self_pairs = list(m.pairs)
    return m


def rate(kin, torch, m, B, steps, warmup):
    K = kin.Kinematics(m, device=0)
    dev = torch.device("cuda", 0)
    P, n = len(m.pairs), m.n
    q = torch.as_tensor(np.random.default_rng(2).uniform(-0.4, 0.4, (B, n)), device=dev).contiguous()
    d = torch.zeros((B, P), dtype=torch.float64, device=dev)
    J = torch.zeros((B, P, n), dtype=torch.float64, device=dev)
    kb = K.batch_args(q, pair_dist=d, pair_J=(J, 0))
    for _ in range(warmup):
        K.forward(q, batch=kb)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        K.forward(q, batch=kb)
    t1.record()
    torch.cuda.synchronize()
    return B * steps / (t0.elapsed_time(t1) * 1e-3)


def main():
    import torch
    from opensot_amd import kinematics as kin
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    capsule = rate(kin, torch, kin.humanoid32_pairs(kin.humanoid32()), a.batch, a.steps, a.warmup)
    convex = rate(kin, torch, convex_model(kin), a.batch, a.steps, a.warmup)
    print(json.dumps({"bench": "convex_pairs", "batch": a.batch, "steps": a.steps, "pairs": 16,
                      "capsule_instances_per_s": capsule, "convex_instances_per_s": convex}))


if __name__ == "__main__":
    main()
