"""developer helper (GPU box): hot against cold start of the batched explicit QP beyond 64 variables (osot_qp_solve_batch_hot against
osot_qp_solve_batch, the same commit) over drifting control cycles: the two levels of the floating-base inverse-dynamics stacks of 70
and 88 variables (synth.wide_id_levels, B = 1024) and the random (128, 80) shape (B = 512).  Per configuration ten cycles with 1 %
noise on g and on the bounds; cycle 0 fills the state and is not counted; which of the two launches of a cycle goes first alternates.  One JSON line per configuration and mode:
QPs/s over the counted cycles, mean and max iterations per instance (a launch is as long as its slowest instance: the max matters).
--cold-only --lib PATH runs the cold entry of ANOTHER build of the library (a parent commit's, which has no hot entry) on the same
configurations, for an A/B of the cold kernel.
usage: python tools/bench_qp_hot.py [--cycles 10] [--out profiles/qp_hot_bench.jsonl] [--cold-only [--lib PATH] [--tag NAME]]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from opensot_amd import abi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--cycles", type=int, default=10)
ap.add_argument("--out", default="")
ap.add_argument("--cold-only", action="store_true", help="the cold entry alone (what a parent commit also has)")
ap.add_argument("--lib", default="", help="with --cold-only: another build of libosot_mi355x.so")
ap.add_argument("--tag", default="", help="copied into every output line")
opt = ap.parse_args()
assert not opt.lib or opt.cold_only, "--lib is for --cold-only"
_other = None


def the_lib():
    global _other
    if not opt.lib:
        return abi.lib()
    if _other is None:
        vp = C.c_void_p
        _other = C.CDLL(opt.lib)
        _other.osot_last_error.restype = C.c_char_p
        _other.osot_qp_solve_batch.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_double, C.c_int, vp, vp, vp, vp]
    return _other
dev = torch.device("cuda", 0)
EPS = 2.221e-7        # tools/bench_wide_qp.py's


def id_levels(nv, ncon, B):
    """the two levels of B stacks; level 1 under the optimality rows of level 0's solution (taken from the oracle-free cold solve)"""
    gens = []
    for b in range(B):
        n, level = synth.wide_id_levels(np.random.default_rng(1000 + b), nv, ncon)
        gens.append(level)
    q0 = [lv(0, []) for lv in gens]
    yield n, 0, [np.stack([q[j] for q in q0]) for j in range(7)]
    x0 = solve(*to_dev([np.stack([q[j] for q in q0]) for j in range(7)]), None)[0].cpu().numpy()
    q1 = [lv(1, [x0[i]]) for i, lv in enumerate(gens)]
    yield n, 1, [np.stack([q[j] for q in q1]) for j in range(7)]


def to_dev(arrs):
    return [torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev) for a in arrs]


def solve(H, g, A, lA, uA, l, u, hot):
    B, n, nc = H.shape[0], H.shape[1], A.shape[1]
    x = torch.empty((B, n), dtype=torch.float64, device=dev)
    st = torch.empty((B,), dtype=torch.int32, device=dev); it = torch.empty((B,), dtype=torch.int32, device=dev)
    p = lambda a: C.c_void_p(a.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = the_lib()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if hot is None:
        rc = L.osot_qp_solve_batch(B, n, nc, p(H), p(g), p(A), p(lA), p(uA), p(l), p(u), EPS, 0, p(x), p(st), p(it), stream)
    else:
        rc = L.osot_qp_solve_batch_hot(B, n, nc, p(H), p(g), p(A), p(lA), p(uA), p(l), p(u), EPS, 0, p(x), p(st), p(it), p(hot), stream)
    e1.record()
    assert rc == abi.OK, L.osot_last_error()
    torch.cuda.synchronize()
    return x, st, it, e0.elapsed_time(e1)


def run(name, arrs):
    H, g, A, lA, uA, l, u = to_dev(arrs)
    B, n, nc = H.shape[0], H.shape[1], A.shape[1]
    gen = torch.Generator(device="cpu").manual_seed(17)
    noise = lambda shape: (1.0 + 0.01 * torch.randn(shape, generator=gen, dtype=torch.float64)).to(dev)
    hot = None
    if not opt.cold_only:
        from opensot_amd import torch_api
        hot = torch_api.qp_hot_state(B, n)
    solve(H, g, A, lA, uA, l, u, None)          # (first launch: module load, LDS attribute)
    acc = {m: {"ms": 0.0, "it_sum": 0, "it_max": 0, "solved": 0} for m in ("cold", "hot")}
    worst = 0.0
    for cycle in range(opt.cycles):
        if cycle:
            g = g * noise(g.shape)
            fr = noise(lA.shape); lA = lA * fr; uA = uA * fr      # (one factor per row: an equality row stays one)
            fb = noise(l.shape); l = l * fb; u = u * fb
        # (the order alternates from cycle to cycle: the second launch of a pair finds H and A in the last-level cache)
        res = {}
        for m in (("cold", "hot") if cycle % 2 == 0 else ("hot", "cold")):
            if m == "cold" or hot is not None:
                res[m] = solve(H, g, A, lA, uA, l, u, hot if m == "hot" else None)
        xc, stc, itc, msc = res["cold"]
        if hot is not None:
            both = (stc == 0) & (res["hot"][1] == 0)
            d = ((res["hot"][0] - xc).abs().amax(dim=1) / xc.abs().amax(dim=1).clamp(min=1.0))[both]
            worst = max(worst, float(d.max()) if d.numel() else 0.0)
        if cycle == 0:
            continue
        for m, (x, st, it, ms) in res.items():
            a = acc[m]
            a["ms"] += ms; a["it_sum"] += int(it.sum()); a["it_max"] = max(a["it_max"], int(it.max())); a["solved"] += int((st == 0).sum())
    lines = []
    for m in sorted(res):
        a = acc[m]; k = opt.cycles - 1
        lines.append({"tag": opt.tag, "config": name, "n": n, "nc": nc, "B": B, "mode": m, "cycles": k, "kqps": round(B * k / a["ms"], 2),
                      "ms_per_launch": round(a["ms"] / k, 3), "mean_iterations": round(a["it_sum"] / (B * k), 2),
                      "max_iterations": a["it_max"], "solved": a["solved"], "of": B * k,
                      "max_scaled_diff_hot_cold": worst if m == "hot" else None})
    for ln in lines:
        print(json.dumps(ln), flush=True)
        if opt.out:
            with open(os.path.join(ROOT, opt.out) if not os.path.isabs(opt.out) else opt.out, "a") as f:
                f.write(json.dumps(ln) + "\n")


for nv, ncon in ((55, 5), (61, 9)):
    for n, k, arrs in id_levels(nv, ncon, 1024):
        run(f"wide_id_levels n={n} level {k}", arrs)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import random_qp
run("random_qp (128, 80, 40 equalities)", list(random_qp(np.random.default_rng(208), 512, 128, 80, 40)))
