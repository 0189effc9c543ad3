"""developer helper (GPU box): hot against cold start of the batched iHQP cascade on the wide route (osot_ihqp_solve_hot against
osot_ihqp_solve on one handle, the same commit) over drifting control cycles: the surface-contact inverse-dynamics stacks of 68 and 86
variables (synth.make_surface_id_stack) at B = 1024 and 4096, and the 96-variable robot stack (synth.make_wide_robot_stack, B = 1024)
whose working sets are nearly empty -- what the hot start costs where it has nothing to gain.  The stack is assembled once on the
device (osot_stack_update); per cycle every level's b, the rows' bounds and the box are scaled in place by one factor per instance
within 1 % (both sides of a row by the same factor: an equality stays one), then the cold and the hot call solve the same arrays,
which of the two goes first alternating from cycle to cycle.  Cycle 0 fills the state and is not counted.  Three runs per
configuration, each from the undrifted arrays and an empty state; one JSON line per configuration and mode: solves/s as min - max over
the runs (device events around the call), mean and max iterations per instance over the counted cycles (a launch is as long as its
slowest instance: the max matters), the worst scaled |dq_hot - dq_cold|.
usage: python tools/bench_wide_hot.py [--cycles 9] [--runs 3] [--out profiles/wide_hot_bench.jsonl] [--quick]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from opensot_amd import synth
from opensot_amd.solver import BatchedStack

ap = argparse.ArgumentParser()
ap.add_argument("--cycles", type=int, default=9, help="counted cycles per run")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default="")
ap.add_argument("--quick", action="store_true", help="B = 64 everywhere: a rehearsal of the script, not a measurement")
opt = ap.parse_args()
assert torch.cuda.is_available(), "bench_wide_hot.py measures on the GPU; there is none"
dev = torch.device("cuda", 0)

SURFACE = {68: (44, 4), 86: (56, 5)}     # n -> (nv, surface contacts)


def drift_targets(st):
    """(tensors scaled by one factor per instance) per group: each level's b; lo and up; l and u"""
    groups = [[b] for b in st.b]
    if st.lo is not None:
        groups.append([st.lo, st.up])
    if st.l is not None:
        groups.append([st.l, st.u])
    return groups


def timed(st, B, hot):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    st.solve(B, hot=hot)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), st.dq[:B].clone(), st.status[:B].clone(), st.iterations[:B].clone()


def run(name, plan, leaf, B):
    st = BatchedStack(plan, B, device=0)
    assert st.route == "wide"
    st.update(st.load_leaf(leaf))
    torch.cuda.synchronize()
    groups = drift_targets(st)
    keep = [[t.clone() for t in g] for g in groups]
    state = st.hot_state()
    timed(st, B, None); timed(st, B, state)          # (first launches: module load, LDS attribute)
    per_run = {"cold": [], "hot": []}
    acc = {m: {"it_sum": 0, "it_max": 0, "solved": 0} for m in ("cold", "hot")}
    worst = 0.0
    for r in range(opt.runs):
        for g, k in zip(groups, keep):
            for t, c in zip(g, k):
                t.copy_(c)
        state.fill_(-1)
        gen = torch.Generator(device="cpu").manual_seed(17 + r)
        ms = {"cold": 0.0, "hot": 0.0}
        for cycle in range(opt.cycles + 1):
            if cycle:
                for g in groups:
                    f = (1.0 + 0.01 * (2.0 * torch.rand((st.max_batch, 1), generator=gen, dtype=torch.float64) - 1.0)).to(dev)
                    for t in g:
                        t.copy_(torch.where(t.abs() >= 1e20, t, t * f))
            res = {}
            for m in (("cold", "hot") if (cycle + r) % 2 == 0 else ("hot", "cold")):
                res[m] = timed(st, B, state if m == "hot" else None)
            both = (res["cold"][2] == 0) & (res["hot"][2] == 0)
            d = ((res["hot"][1] - res["cold"][1]).abs().amax(dim=1) / res["cold"][1].abs().amax(dim=1).clamp(min=1.0))[both]
            worst = max(worst, float(d.max()) if d.numel() else 0.0)
            if cycle == 0:
                continue
            for m, (t_ms, _, status, it) in res.items():
                ms[m] += t_ms
                a = acc[m]
                a["it_sum"] += int(it.sum()); a["it_max"] = max(a["it_max"], int(it.max())); a["solved"] += int((status == 0).sum())
        for m in ms:
            per_run[m].append(B * opt.cycles / ms[m])          # thousand solves per second
    total = B * opt.cycles * opt.runs
    for m in ("cold", "hot"):
        a = acc[m]
        ln = {"config": name, "n": plan.n, "levels": plan.L, "B": B, "mode": m, "cycles": opt.cycles, "runs": opt.runs,
              "ksolves_per_s_min": round(min(per_run[m]), 2), "ksolves_per_s_max": round(max(per_run[m]), 2),
              "mean_iterations": round(a["it_sum"] / total, 2), "max_iterations": a["it_max"], "solved": a["solved"], "of": total,
              "resident_workgroups": st.resident_waves(), "max_scaled_diff_hot_cold": worst if m == "hot" else None}
        print(json.dumps(ln), flush=True)
        if opt.out:
            with open(opt.out if os.path.isabs(opt.out) else os.path.join(ROOT, opt.out), "a") as f:
                f.write(json.dumps(ln) + "\n")


for n, (nv, contacts) in SURFACE.items():
    for B in ((64,) if opt.quick else (1024, 4096)):
        plan, leaf = synth.make_surface_id_stack(B, seed=n + 1, nv=nv, n_contacts=contacts)
        run(f"surface_id_stack n={n}", plan, leaf, B)
B = 64 if opt.quick else 1024
plan, leaf = synth.make_wide_robot_stack(B, 96, levels=3, seed=9)
run("wide_robot_stack n=96", plan, leaf, B)
