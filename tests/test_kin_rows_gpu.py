"""The row sets and gaze references of the kinematics producer on the device: osot_kinematics against the host emulation and the
restatement of tests/kin_rows_ref.py, the wheeled stack in a cycle and in a captured graph, the refusals.

Bit-identity.  The row-set stage is compiled without multiply-add contraction, so on the SAME inputs the device and the host build
agree bit for bit: test_stage_is_bit_identical_to_the_host_build feeds the host build of the stage the pose and the world Jacobian
the device itself published and asks for equal bits of every row and every gaze reference.  The stages in front of it (sincos, the
transforms, the Jacobian columns) are contracted on the device and differ from the host emulation in the last bits, as they always
have (tree_cases.DEVICE_BOUND): the whole kernel against the whole emulation is therefore reported (profiles/kin_rows.txt) and held
to the device bound per set, DEVICE_BOUND["J"] x max(1, |M|_inf).  The split contact's b is a wave reduction: a DPP tree on the device, a sequence in the emulation's twin
(tests/emu/osot_team.h says so), so b is held to the rounding of a 64-term sum instead."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from opensot_amd import abi, kinematics as kin, synth
from opensot_amd.solver import BatchedStack
from oracle import pykin
import kin_rows_ref as kr
import tree_cases as tc

pytestmark = pytest.mark.gpu
F64 = dict(dtype=torch.float64, device="cuda")
EPS = 2.0 ** -52


def device_rows(K, m, q, qd=None, pts=None, frames=True, pairs=False):
    """osot_kinematics into the layout of kr.outputs -> the same dict of numpy arrays as kr.emu_rows"""
    B = len(q)
    host, off = kr.outputs(m, B, pairs=pairs)
    dev = {k: torch.as_tensor(v, **F64).contiguous() for k, v in host.items()}
    kw = dict(rowset_A={s: ((dev["RS"] if rs["split"] else dev["RA"]), off[s]) for s, rs in enumerate(m.rowsets)})
    if frames:
        kw.update(frame_pose={f: dev["poses"][f] for f in range(len(m.frames))}, frame_J={f: (dev["J"][f], 0) for f in range(len(m.frames))})
    if qd is not None:
        kw.update(rowset_b={s: (dev["rb"], off[s]) for s, rs in enumerate(m.rowsets) if rs["split"]}, qdot=torch.as_tensor(qd, **F64).contiguous())
    if pts is not None:
        P = torch.as_tensor(pts, **F64).contiguous()
        kw.update(gaze_point={g: P[g] for g in range(len(m.gazes))}, gaze_ref={g: dev["gaze"][g] for g in range(len(m.gazes))})
    if pairs:
        kw.update(pair_dist=dev["pd"], pair_J=(dev["pJ"], 0), pair_points=dev["pp"])
    K.forward(torch.as_tensor(q, **F64).contiguous(), **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    out["off"] = off
    return out


@pytest.fixture(scope="module")
def models(gpu_device):
    return {name: (make(), B) for name, (make, B) in kr.CASES.items()}


def world_frames(m, q, got):
    """pose and WORLD Jacobian of every frame as the device computes them, the stage's inputs: what the run published -- for a model
    with BODY Jacobians or column masks, what the same instantiation publishes for the same model without those options (the row
    sets take the column from in front of the options; poses do not depend on them)"""
    B = len(q)
    if not m.frame_body and not m.frame_active_joints:
        return got["poses"][:, :B], got["J"][:, :B]
    plain = copy.copy(m)
    plain.frame_body, plain.frame_active_joints = {}, {}
    ref = device_rows(kin.Kinematics(plain, device=0), plain, q)
    assert np.array_equal(ref["poses"], got["poses"])
    return ref["poses"][:, :B], ref["J"][:, :B]


def _check(m, q, qd, pts, got, whole=None):
    """the device's run against (1) the host build of the stage on the device's own pose and world Jacobian, bit for bit (b: the
    rounding of a 64-term sum), (2) the restatement at DEVICE_BOUND["J"] x max(1, |M|_inf), (3) the whole emulated kernel, when
    given, at the same bound per set (b: x max(1, |qdot[6:]|_1); gaze references: the device bound on R and p, 1e-12 each, carried
    through t = R'(g - p) and the normalisation, 3 (|g - p| + 1) 1e-12 / |t|) -> worst |device - emulation|"""
    B = len(q)
    assert kr.canaries_intact(m, got, B)
    pose, J = world_frames(m, q, got)
    stage = kr.stage_rows(m, q, pose, J, qd, pts)
    assert got["gaze"].tobytes() == stage["gaze"].tobytes()
    worst = 0.0
    for i in range(B):
        fk = pykin.forward(m, q[i])
        for s, rs in enumerate(m.rowsets):
            (A, b), (As, bs) = kr.got_rows(m, got, s, i), kr.got_rows(m, stage, s, i)
            assert np.array_equal(A, As), (s, i)
            full, _, norm = kr.rowset_rows(m, dict(rs, split=False), fk)
            bound = tc.DEVICE_BOUND["J"] * max(1.0, norm)
            if rs["split"]:
                assert np.abs(b - bs).max() <= 64 * EPS * max(float((np.abs(full[:, 6:]) @ np.abs(qd[i, 6:])).max()), 1.0), (s, i)
            if whole is not None:
                Aw, bw = kr.got_rows(m, whole, s, i)
                assert np.abs(A - Aw).max() <= bound, (s, i)
                worst = max(worst, float(np.abs(A - Aw).max()))
                if rs["split"]:
                    assert np.abs(b - bw).max() <= bound * max(1.0, float(np.abs(qd[i, 6:]).sum())), (s, i)
                    worst = max(worst, float(np.abs(b - bw).max()))
    kr.compare_rows(m, q, got, tc.DEVICE_BOUND["J"], qd)
    if whole is not None:
        assert np.array_equal(np.isnan(whole["gaze"]), np.isnan(got["gaze"]))
        for g, f in enumerate(m.gazes):
            for i in range(B):
                if np.isnan(got["gaze"][g, i]).any():
                    continue
                T = got["poses"][f][i]
                d = pts[g, i] - T[9:]
                t = T[:9].reshape(3, 3).T @ d
                err = float(np.abs(got["gaze"][g, i] - whole["gaze"][g, i]).max())
                assert err <= 3.0 * (np.linalg.norm(d) + 1.0) * tc.DEVICE_BOUND["R"] / np.linalg.norm(t), (g, i, err)
                worst = max(worst, err)
    return worst


@pytest.mark.parametrize("name", list(kr.CASES))
def test_stage_is_bit_identical_to_the_host_build(name, models):
    """the four trees: every row set and gaze reference (module docstring), sets on frames with a BODY Jacobian or a column mask
    included; the whole kernel against the whole emulation within the device bound per set, and reported"""
    m, B = models[name]
    K = kin.Kinematics(m, device=0)
    q, qd = kr.postures(m, B), tc.draw_qdot(m, B)
    pts, dist = kr.gaze_points(m, q)
    got = device_rows(K, m, q, qd, pts)
    worst = _check(m, q, qd, pts, got, whole=kr.emu_rows(m, q, qd, pts))
    print(f"{name}: max |device - host emulation| over rows, b and gaze references = {worst:.3e}")


@pytest.mark.parametrize("name", ["chain7", "tree64"])
def test_rows_beside_the_pair_stage(name, models):
    """osot_kin_kernel<true, JMAX, false, true>, JMAX = 32 and 64: the tree's 32 capsule pairs bound together with the row sets.  The
    rows pass every check of the run without them, and are its bits; the pair outputs are the bits of the producer without the
    ROWS flag (a call that binds the pair outputs alone)"""
    m, B = models[name]
    assert len(m.pairs) == abi.KIN_MAX_PAIRS
    K = kin.Kinematics(m, device=0)
    q, qd = kr.postures(m, B), tc.draw_qdot(m, B)
    pts, dist = kr.gaze_points(m, q)
    got = device_rows(K, m, q, qd, pts, pairs=True)
    _check(m, q, qd, pts, got)
    alone = device_rows(K, m, q, qd, pts)
    for k in ("RA", "RS", "rb", "poses", "J"):
        assert np.array_equal(got[k], alone[k]), k
    assert got["gaze"].tobytes() == alone["gaze"].tobytes()
    P, n = len(m.pairs), m.n
    pd, pJ, pp = (torch.full(sh, kr.CANARY, **F64) for sh in ((B + 1, P), (B + 1, P + 1, n), (B + 1, P, 6)))
    K.forward(torch.as_tensor(q, **F64).contiguous(), pair_dist=pd, pair_J=(pJ, 0), pair_points=pp)
    torch.cuda.synchronize()
    for k, t in (("pd", pd), ("pJ", pJ), ("pp", pp)):
        assert np.array_equal(got[k], t.cpu().numpy()), k
    assert not (got["pd"][:B] == kr.CANARY).any() and (got["pJ"][:, P] == kr.CANARY).all() and (got["pd"][B] == kr.CANARY).all()


@pytest.mark.parametrize("name,B", [("chain7", 1), ("chain7", 130), ("tree64", 1), ("tree64", 130), ("wheeled", 130)])
def test_batch_sizes(name, B, models):
    """B = 1 and 130: a half-empty wavefront at JMAX = 32, more than one workgroup wave, an instance behind the batch untouched"""
    m, _ = models[name]
    K = kin.Kinematics(m, device=0)
    q, qd = kr.postures(m, B, seed=B), tc.draw_qdot(m, B, seed=B)
    pts, dist = kr.gaze_points(m, q[:4], seed=B)
    pts = np.ascontiguousarray(np.tile(pts, (1, (B + 3) // 4, 1))[:, :B])      # (the points of the first four postures, reused)
    got = device_rows(K, m, q, qd, pts)
    _check(m, q, qd, pts, got)


def test_rows_without_frame_outputs_are_the_same_bits(models):
    m, B = models["tree33"]
    K = kin.Kinematics(m, device=0)
    q = kr.postures(m, B)
    a, b = device_rows(K, m, q), device_rows(K, m, q, frames=False)
    assert np.array_equal(a["RA"], b["RA"]) and np.array_equal(a["RS"], b["RS"]) and (b["J"] == kr.CANARY).all()


def wheeled(B, omni=False):
    plan, leaf, model = synth.make_wheeled_stack(B, seed=0, omni=omni)
    K = kin.Kinematics(model, device=0)
    st = BatchedStack(plan, B, device=0, want_levels=False)
    dev, kb, q = synth.bind_wheeled(st, K, leaf)
    return plan, leaf, model, K, st, dev, kb, q


@pytest.mark.parametrize("omni", [False, True])
def test_wheeled_stack_cycle_matches_the_emulated_solve(omni, gpu_device):
    B = 8
    plan, leaf, model, K, st, dev, kb, q = wheeled(B, omni)
    K.forward(q, batch=kb)
    st.cycle(dev)
    torch.cuda.synchronize()
    assert (st.status[:B] == 0).all()
    dq, status, asm = kr.emulated_wheeled_solve(plan, leaf, model)
    assert (status == abi.STATUS_SOLVED).all()
    got = st.dq[:B].cpu().numpy()
    print(f"omni={omni}: max |dq - dq_emulated| = {np.abs(got - dq).max():.3e}, max |dq| = {np.abs(dq).max():.3e}")
    assert np.abs(got - dq).max() <= 1e-6
    assert np.abs(st.A[0][:B].cpu().numpy() - asm["A"][0]).max() <= tc.DEVICE_BOUND["J"]


def test_graph_capture_of_producer_and_cycle(gpu_device):
    """one torch.cuda.graph of osot_kinematics + osot_cycle replays the same bits (the process keeps its default hardware queues)"""
    B = 8
    plan, leaf, model, K, st, dev, kb, q = wheeled(B, omni=True)
    K.forward(q, batch=kb)
    st.cycle(dev)
    torch.cuda.synchronize()
    want = [st.dq[:B].clone(), st.A[0][:B].clone(), st.A[1][:B].clone(), st.status[:B].clone()]
    s = torch.cuda.Stream()
    st.stream = s
    with torch.cuda.stream(s):                          # one stream, captured once, replayed (Kinematics.forward: torch's current one)
        K.forward(q, batch=kb)
        st.cycle(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        K.forward(q, batch=kb)
        st.cycle(dev)
    st.dq.fill_(-3.0); st.A[0].fill_(-3.0); st.A[1].fill_(-3.0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(want, [st.dq[:B], st.A[0][:B], st.A[1][:B], st.status[:B]]):
        assert torch.equal(a, b)


def test_refusals(gpu_device):
    """osot_control_cycle on a model with row sets: OSOT_ERR_UNSUPPORTED naming osot_kinematics + osot_cycle; a bound rowset_b without
    qdot: OSOT_ERR_INVALID at call time"""
    B = 2
    plan, leaf, model, K, st, dev, kb, q = wheeled(B)
    with pytest.raises(RuntimeError) as e:
        st.control_cycle(K, kb, dev)
    assert f"code {abi.ERR_UNSUPPORTED}" in str(e.value) and "row sets / gaze references: use osot_kinematics + osot_cycle" in str(e.value)
    # row sets together with the pair outputs of a model that has a convex (GJK) pair: refused, two calls serve it
    mc = kr.chain7()
    mc.pairs = [(6, (0, 0, 0), (0, 0, 0), 0.0, 2, (0, 0, 0), (0, 0, 0), 0.0,
                 dict(kind=abi.SHAPE_BOX, half=(0.05, 0.04, 0.03), kind_a=abi.SHAPE_BOX, size_a=(0.03, 0.03, 0.06)))]
    Kc = kin.Kinematics(mc, device=0)
    qc = torch.as_tensor(kr.postures(mc, B), **F64).contiguous()
    dist, RA = torch.zeros((B, 1), **F64), torch.zeros((B, 8, mc.n), **F64)
    with pytest.raises(RuntimeError) as e:
        Kc.forward(qc, pair_dist=dist, rowset_A={0: (RA, 0)})
    assert f"code {abi.ERR_UNSUPPORTED}" in str(e.value) and "row sets / gaze references with convex collision pairs" in str(e.value)
    Kc.forward(qc, pair_dist=dist)
    Kc.forward(qc, rowset_A={0: (RA, 0)})
    torch.cuda.synchronize()
    assert float(RA.abs().max()) > 0.0 and float(dist.abs().max()) > 0.0
    m = kr.tree33()
    K2 = kin.Kinematics(m, device=0)
    s = [k for k, rs in enumerate(m.rowsets) if rs["split"]][0]
    qq = torch.as_tensor(kr.postures(m, B), **F64).contiguous()
    bt = torch.zeros((B, 8), **F64)
    with pytest.raises(RuntimeError) as e:
        K2.forward(qq, rowset_b={s: (bt, 0)})
    assert f"code {abi.ERR_INVALID}" in str(e.value) and "rowset_qdot is null" in str(e.value)
