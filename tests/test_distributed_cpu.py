"""N>1 path on CPU: world_size-2 gloo processes run THE SAME objects bench.py runs with RCCL -- `ShardGather` (ONE
all_gather_into_tensor per step: dq rows and status words in one block, sized for the largest shard; the solver's outputs
bound straight into that block as bench.py does, or copied in) and `ShardedCycle` + `timed_steps` (the per-rank step loop
and its barrier bracket) -- with the solve stubbed at the BatchedStack boundary."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from opensot_amd.parallel import ShardedCycle, ShardGather, all_gather_dq, shard_range, timed_steps


def test_shard_range_partitions():
    for total in (0, 1, 7, 4096, 32768, 10):
        for world in (1, 2, 3, 8):
            spans = [shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            for a, b in zip(spans, spans[1:]):
                assert a[1] == b[0]
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_range(10, 2, 2)


class _StubStack:
    """stands in for opensot_amd.solver.BatchedStack on CPU tensors: `solve` writes a dq that depends only on the GLOBAL
    instance index and on the cycle's inputs, `update` consumes the cycle's leaf"""

    def __init__(self, lo, hi, n):
        self.lo, self.n = lo, n
        B = hi - lo
        self.dq = torch.zeros((B, n), dtype=torch.float64)
        self.status = torch.full((B,), -1, dtype=torch.int32)
        self.A = None
        self.cycle_value = None
        self.calls = []

    def update(self, dev_leaf):
        self.cycle_value = float(dev_leaf["bias"])
        self.calls.append("update")

    def solve(self, B):
        idx = torch.arange(self.lo, self.lo + B, dtype=torch.float64)
        self.dq[:B] = idx[:, None] * 10.0 + torch.arange(self.n, dtype=torch.float64)[None, :] + self.cycle_value + self.A
        self.status[:B] = (idx % 3 == 0).to(torch.int32)      # a few "unsolved" instances: the status must travel too
        self.calls.append("solve")


class _StubFusedStack(_StubStack):
    """a stack with BatchedStack.cycle(): ShardedCycle then BINDS its dq / status to the collective's send block before
    every step (the zero-copy route bench.py takes): whatever tensors `dq` / `status` point at when cycle() runs get written"""

    def cycle(self, dev_leaf):
        self.update(dev_leaf)
        self.solve(self.dq.shape[0] if self.B is None else self.B)

    B = None


def _worker(rank, world, port, total, n, q, fused=False):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = shard_range(total, rank, world)
    stack = _StubFusedStack(lo, hi, n) if fused else _StubStack(lo, hi, n)
    if fused:
        stack.B = hi - lo                       # (the bound views hold the LARGEST shard's rows: solve only this rank's)
    gather = ShardGather(total, n, torch.device("cpu"), torch.float64)
    K = 3
    cyc = ShardedCycle(stack, [{"bias": 100.0 * k} for k in range(K)], [1000.0 * k for k in range(K)], hi - lo, gather)
    steps, warmup = 4, 2
    elapsed = timed_steps(cyc.step, steps, warmup, sync=lambda: None, dist=dist, device=torch.device("cpu"))
    last = (steps + warmup - 1) % K           # the cycle the last step ran
    one_shot = all_gather_dq(stack.dq[:hi - lo], total)  # the convenience form must agree with the resident buffers
    q.put((rank, gather.dq.numpy().copy(), gather.status.numpy().copy(), one_shot.numpy().copy(), last, elapsed,
           stack.calls == ["update", "solve"] * (steps + warmup)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("total,fused", [(8, False), (7, False), (1, False), (8, True), (7, True)])
def test_two_rank_step_loop_and_gather(total, fused):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    n = 5
    procs = [ctx.Process(target=_worker, args=(r, 2, port, total, n, q, fused)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    idx = np.arange(total)
    for rank, dq, status, one_shot, last, elapsed, order_ok in res:
        want = idx[:, None] * 10.0 + np.arange(n)[None, :] + 100.0 * last + 1000.0 * last
        np.testing.assert_array_equal(dq, want)              # global instance order, uneven shards included
        np.testing.assert_array_equal(one_shot, want)
        np.testing.assert_array_equal(status, (idx % 3 == 0).astype(np.int32))
        assert order_ok and elapsed > 0.0
    assert res[0][5] == res[1][5]                            # the elapsed time is the MAX over ranks on every rank


def _lane_worker(rank, world, port, per_rank, S, n, q):
    """a rank's shard as S lanes (PipelinedCycle), each lane with its OWN process group and gather -- bench.py's layout"""
    from opensot_amd.parallel import PipelinedCycle, lane_ranges
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo = rank * per_rank
    K = 2
    lanes, gathers = [], []
    spans = lane_ranges(per_rank, S)
    for a, b in spans:
        grp = dist.new_group(list(range(world)))
        stack = _StubFusedStack(lo + a, lo + b, n)
        stack.B = b - a
        g = ShardGather((b - a) * world, n, torch.device("cpu"), torch.float64, group=grp, sizes=[b - a] * world)
        lanes.append(ShardedCycle(stack, [{"bias": 100.0 * k} for k in range(K)], [1000.0 * k for k in range(K)], b - a, g))
        gathers.append(g)
    pipe = PipelinedCycle(lanes, None)
    steps, warmup = 3, 1
    elapsed = timed_steps(pipe.step, steps, warmup, sync=lambda: None, dist=dist, device=torch.device("cpu"))
    last = (steps + warmup - 1) % K
    q.put((rank, [g.dq.numpy().copy() for g in gathers], [g.status.numpy().copy() for g in gathers], last, elapsed))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_pipelined_lanes():
    """world of two, two lanes per rank with uneven sub-batches (5 = 3 + 2): lane j's gather holds lane j of rank 0, then
    lane j of rank 1, each with the values its global instance index dictates"""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    per_rank, S, n = 5, 2, 4
    procs = [ctx.Process(target=_lane_worker, args=(r, 2, port, per_rank, S, n, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from opensot_amd.parallel import lane_ranges
    spans = lane_ranges(per_rank, S)
    for rank, dqs, sts, last, elapsed in res:
        for j, (a, b) in enumerate(spans):
            idx = np.concatenate([np.arange(r * per_rank + a, r * per_rank + b) for r in range(2)])
            want = idx[:, None] * 10.0 + np.arange(n)[None, :] + 100.0 * last + 1000.0 * last
            np.testing.assert_array_equal(dqs[j], want)
            np.testing.assert_array_equal(sts[j], (idx % 3 == 0).astype(np.int32))
        assert elapsed > 0.0


def test_bench_self_launches_two_ranks_on_the_stub_backend():
    """`python bench.py --gpus 2` with no launcher around it: bench.py re-executes itself under
    torch.distributed.run with two ranks; here on the stub back-end (CPU tensors, gloo), which runs the script's own
    sharding, lanes, per-lane gathers and timing bracket end to end.  rc 0 and ONE JSON line with n_gpus 2."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "stub", "--steps", "3",
                        "--warmup", "1", "--batch-per-gpu", "48", "--lanes", "2"], capture_output=True, text=True, timeout=600,
                       env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    # the driver's capture is finite (round 4: a 31 KB line came back unparsed): the line is compact, strict JSON, and the last
    # thing on stdout
    assert len(lines[0]) < 12288 and r.stdout.rstrip().endswith(lines[0])
    out = json.loads(lines[0], parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["config"]["global_batch"] == 96
    assert len(out["config"]["workload"]) <= 300
    assert out["solved_ok_all_ranks"] == "96/96" and "STUB" in out["data"]


def test_bench_dump_outputs_on_the_stub_backend(tmp_path):
    """`bench.py --dump-outputs DIR`: the last timed step's dq and status of every instance, in global instance order, as float64
    .npy files; the same arguments give the same files, and a world of two hands back rank 0's rows where a world of one has
    them.  The result line's ms_per_step is the time of one of the --steps timed steps."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)

    def run(gpus, name):
        d = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(gpus), "--backend", "stub", "--steps", "3",
                            "--warmup", "1", "--batch-per-gpu", "48", "--lanes", "2", "--dump-outputs", str(d),
                            "--details", str(tmp_path / (name + ".json"))], capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0.0
        assert abs(out["value"] * out["ms_per_step"] - 1e3 * 48 * gpus) <= 1e-5 * out["value"] * out["ms_per_step"]
        dq, status = np.load(d / "dq.npy"), np.load(d / "status.npy")
        assert dq.dtype == np.float64 and status.dtype == np.float64
        assert dq.shape == (48 * gpus, 32) and status.shape == (48 * gpus,)
        assert np.isfinite(dq).all() and (status == 0).all()
        return dq
    one = run(1, "one")
    np.testing.assert_array_equal(run(1, "again"), one)
    two = run(2, "two")
    np.testing.assert_array_equal(two[:48], one)
    assert not np.array_equal(two[48:], one)
