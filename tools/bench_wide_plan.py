"""Throughput of batched iHQP plans wider than a wavefront (65 .. 128 variables) on the workgroup route (osot_solver_create_wide +
osot_cycle: one 256-thread workgroup per instance, opensot_amd/csrc/osot_cascade_wide.h), against
  - the same plans solved LEVEL BY LEVEL through osot_qp_solve_batch with the optimality rows assembled in torch (the only GPU way
    before the wide route), and
  - the reference's qpOASES per host thread (oracle.ihqp_solve_batch(..., BE_QPOASES_REF)) where oracle/_ref exists.
One JSON line per configuration.  Timing: warm-up, device events around a window of at least --window seconds.
    python tools/bench_wide_plan.py [--window 0.3] [--batches 1024,4096] [--sizes 70,96,128]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opensot_amd import abi, synth
from opensot_amd.solver import BatchedStack
from oracle import pyoracle

FP64_SPEC_TFLOPS = 78.6   # (bench.py: MI355X FP64 peak; the measured roof of profiles/r06_fp64_peak.json when present)


def fp64_roof():
    p = os.path.join(ROOT, "profiles", "r06_fp64_peak.json")
    try:
        with open(p) as f:
            d = json.load(f)
        for k in ("v_fma_f64_tflops", "tflops"):   # (the kernel builds H with v_fma_f64)
            if k in d:
                return float(d[k]), os.path.relpath(p, ROOT)
    except (OSError, ValueError):
        pass
    return FP64_SPEC_TFLOPS, "spec"


def timed(fn, window):
    """device-event time (s) per call of fn over a window of at least `window` seconds, after a warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps, el = 1, 0.0
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


def level_by_level(st, plan, B):
    """the plan's cascade as explicit QPs, one osot_qp_solve_batch per level: H, g and the optimality rows assembled in torch from
    the update's arrays (levels: GENERIC / Cartesian / CoM blocks + an implicit Postural block; GENERIC row blocks)"""
    n, L = plan.n, plan.L
    lib = abi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    f64 = dict(dtype=torch.float64, device=st.device)
    x = torch.zeros((B, n), **f64)
    status = torch.zeros((B,), dtype=torch.int32, device=st.device)
    iters = torch.zeros((B,), dtype=torch.int32, device=st.device)
    eye = torch.eye(n, **f64)
    opt_A, opt_b = [], []
    offs = [plan.rows_offset(j) for j in range(len(plan.rowblocks))]
    for k in range(L):
        m, ma = plan.m(k), plan.ma(k)
        H = torch.zeros((B, n, n), **f64)
        g = torch.zeros((B, n), **f64)
        w, b = st.w[k][:B], st.b[k][:B]
        if ma:
            A = st.A[k][:B]
            WA = A * w[:, :ma, None]
            H += torch.bmm(A.transpose(1, 2), WA)
            g -= torch.bmm(WA.transpose(1, 2), b[:, :ma, None])[..., 0]
        npost = m - ma
        if npost:
            H[:, range(npost), range(npost)] += w[:, ma:]
            g[:, :npost] -= w[:, ma:] * b[:, ma:]
        rows_A, rows_lo, rows_up = [], [], []
        for j, rb in enumerate(plan.rowblocks):
            if rb.level is not None and rb.level != k:
                continue
            o, so = offs[j], plan.rows_stored_offset(j)
            rows_A.append(st.C[:B, so:so + rb.rows]); rows_lo.append(st.lo[:B, o:o + rb.rows]); rows_up.append(st.up[:B, o:o + rb.rows])
        for Aj, bj in zip(opt_A, opt_b):
            rows_A.append(Aj); rows_lo.append(bj); rows_up.append(bj)
        Ac = torch.cat(rows_A, 1).contiguous() if rows_A else None
        lA = torch.cat(rows_lo, 1).contiguous() if rows_A else None
        uA = torch.cat(rows_up, 1).contiguous() if rows_A else None
        nc = 0 if Ac is None else Ac.shape[1]
        rc = lib.osot_qp_solve_batch(B, n, nc, p(H), p(g), p(Ac), p(lA), p(uA), p(st.l[:B]), p(st.u[:B]),
                                     plan.eps_abs, 0, p(x), p(status), p(iters), stream)
        assert rc == abi.OK
        if k + 1 < L:   # optimality rows A_k x = A_k x_k
            Ak = torch.cat(([st.A[k][:B]] if ma else []) + ([eye[:npost].expand(B, npost, n)] if npost else []), 1).contiguous()
            opt_A.append(Ak)
            opt_b.append(torch.bmm(Ak, x[..., None])[..., 0].contiguous())
    return x, status


def algorithmic(plan, iters_mean):
    """flops and bytes of one solve: per level the H build (2 ma n (n + 1) / 2 multiply-adds over the lower triangle), the Cholesky and
    J = L^-T (n^3 / 3 + n^3 / 3 multiply-adds), the active-set iterations (about three passes over J: d = J'n, z = J2 d2, the update
    of J: 3 x 2 n^2 flops each); bytes: the stored rows of the levels and of C read once per level, J and L written and read once"""
    n, L = plan.n, plan.L
    fl, by = 0.0, 0.0
    for k in range(L):
        fl += plan.ma(k) * n * (n + 1) + 2 * (2 * n ** 3 / 3)
        by += 8 * (plan.ma(k) * n + plan.nc_stored * n + 2 * 2 * n * n)
    fl += iters_mean * 3 * 2 * n * n
    return fl, by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--batches", default="1024,4096")
    ap.add_argument("--sizes", default="70,96,128")
    ap.add_argument("--ref-sample", type=int, default=32)
    a = ap.parse_args()
    roof, roof_src = fp64_roof()
    for n in [int(v) for v in a.sizes.split(",")]:
        levels = 2 if n == 70 else 3
        for B in [int(v) for v in a.batches.split(",")]:
            plan, leaf = synth.make_wide_robot_stack(B, n, levels=levels, seed=n)
            st = BatchedStack(plan, B, device=0)
            dev = st.load_leaf(leaf)
            t_cycle, reps = timed(lambda: st.cycle(dev), a.window)
            ok = int((st.status[:B] == 0).sum().item())
            it_mean = float(st.iterations[:B].double().mean().item())
            st.set_timing(1)
            st.cycle(dev); torch.cuda.synchronize(); st.kernel_time_ms(reset=True)
            for _ in range(5):
                st.cycle(dev)
            kern_ms = st.kernel_time_ms(reset=True)[0]
            st.set_timing(0)
            st.update(dev)
            t_lvl, _ = timed(lambda: level_by_level(st, plan, B), a.window)
            x_lvl, s_lvl = level_by_level(st, plan, B)
            torch.cuda.synchronize()
            both = (s_lvl == 0) & (st.status[:B] == 0)
            agree = float((x_lvl - st.dq[:B])[both].abs().max().item()) if bool(both.any()) else None
            fl, by = algorithmic(plan, it_mean)
            line = {"tool": "bench_wide_plan", "n": n, "levels": levels, "B": B, "route": "wide",
                    "rows": {"levels": [plan.m(k) for k in range(plan.L)], "nc": plan.nc},
                    "fused_solves_per_s": B / t_cycle, "fused_cycle_ms": 1e3 * t_cycle, "cascade_kernel_ms": kern_ms,
                    "solved": ok, "iterations_mean": it_mean, "window_reps": reps,
                    "level_by_level_solves_per_s": B / t_lvl, "level_by_level_ms": 1e3 * t_lvl,
                    "fused_over_level_by_level": t_lvl / t_cycle, "max_abs_diff_vs_level_by_level": agree,
                    "algorithmic_flops_per_solve": fl, "algorithmic_bytes_per_solve": by,
                    "fp64_tflops_achieved": B * fl / t_cycle / 1e12, "fp64_roof_tflops": roof, "fp64_roof_source": roof_src,
                    "fp64_roof_frac": B * fl / t_cycle / 1e12 / roof}
            if pyoracle.ref_available() and a.ref_sample > 0:   # (a sample of the same plan: the reference's loop on one host thread)
                k = min(a.ref_sample, B)
                plan_s, leaf_s = synth.make_wide_robot_stack(k, n, levels=levels, seed=n)
                rq = pyoracle.ihqp_solve_batch(pyoracle.assemble(plan_s, leaf_s), pyoracle.BE_QPOASES_REF, nthreads=1)
                line["qpoases_ref_solves_per_s_per_thread"] = k / rq["seconds"]
            print(json.dumps(line), flush=True)
            del st


if __name__ == "__main__":
    main()
