"""lean_rows (osot_qp_core.h) on the device: the specialised launch (the lean body of osot_cascade_kernel<32, ., false, true>, implicit row
addresses by one loop over the levels) against the general instantiation (row table), bit for bit, with one, two and three levels
above the eliminating level; and the same through the fused osot_cycle."""
import pytest
import torch

from opensot_amd import synth
from opensot_amd.solver import BatchedStack
from test_lean_rows_host import STACKS

pytestmark = pytest.mark.gpu

B = 70     # more than one wavefront's worth of workgroups per CU is not needed; an odd count beyond 64


@pytest.mark.parametrize("name", list(STACKS))
def test_lean_rows_match_the_general_instantiation_gpu(gpu_device, name):
    rows = STACKS[name]
    plan, leaf = synth.make_generic_stack(B, 32, rows, seed=61 + len(rows))
    spec = BatchedStack(plan, B, device=0)
    gen = BatchedStack(plan, B, device=0)
    gen.set_specialisation(False)
    fused = BatchedStack(plan, B, device=0)
    for st in (spec, gen):
        st.update(st.load_leaf(leaf)); st.solve(B)
    fused.cycle(fused.load_leaf(leaf))
    torch.cuda.synchronize()
    assert (spec.status[:B] == 0).all() and bool((spec.iterations[:B] >= sum(rows)).all())
    for other in (gen, fused):
        assert torch.equal(spec.dq[:B].view(torch.int64), other.dq[:B].view(torch.int64))
        assert torch.equal(spec.x_levels[:B].view(torch.int64), other.x_levels[:B].view(torch.int64))
        assert torch.equal(spec.status[:B], other.status[:B]) and torch.equal(spec.iterations[:B], other.iterations[:B])
