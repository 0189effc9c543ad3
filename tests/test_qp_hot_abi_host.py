"""The hot-start entries of the explicit-QP surface where they need no GPU: the size of the state, the argument checks (those of
osot_qp_solve_batch, made before anything touches the device), the empty batch."""
import ctypes as C

import pytest

from opensot_amd import abi


@pytest.mark.parametrize("n,ints", [(1, 32), (32, 32), (33, 64), (64, 64), (65, 128), (128, 128)])
def test_hot_state_ints(n, ints):
    out = C.c_int(-5)
    assert abi.lib().osot_qp_hot_state_ints(n, C.byref(out)) == abi.OK
    assert out.value == ints


def test_hot_state_ints_refusals():
    L = abi.lib()
    out = C.c_int(-5)
    for n in (0, 129, -1):
        assert L.osot_qp_hot_state_ints(n, C.byref(out)) == abi.ERR_INVALID
        assert out.value == -5
    assert L.osot_qp_hot_state_ints(72, None) == abi.ERR_INVALID


def test_solve_batch_hot_argument_refusals():
    L = abi.lib()
    z = C.c_void_p(0)
    p = C.c_void_p(64)     # (a non-null value: the refusals below come before any pointer is used)
    hot = lambda B, n, nc, H=z, g=z, A=z, lA=z, uA=z, l=z, u=z, x=z, st=z, h=p: \
        L.osot_qp_solve_batch_hot(B, n, nc, H, g, A, lA, uA, l, u, 1e-9, 0, x, st, z, h, z)
    assert hot(1, 0, 0) == abi.ERR_INVALID
    assert hot(1, 129, 0) == abi.ERR_INVALID
    assert hot(-1, 72, 0) == abi.ERR_INVALID
    assert hot(1, 72, -1) == abi.ERR_INVALID
    assert hot(1, 72, 0) == abi.ERR_INVALID                                  # null H / g / x / status
    assert hot(1, 72, 0, H=p, g=p, x=p) == abi.ERR_INVALID                   # null status
    assert hot(1, 72, 3, H=p, g=p, x=p, st=p) == abi.ERR_INVALID             # rows without A / lA / uA
    assert hot(1, 72, 0, H=p, g=p, x=p, st=p, l=p) == abi.ERR_INVALID        # l without u
    assert hot(1, 24, 0, H=p, g=p, x=p, st=p, u=p) == abi.ERR_INVALID
    for n in (4, 40, 72, 128):                                               # an empty batch passes whatever its pointers
        assert hot(0, n, 0) == abi.OK
        assert hot(0, n, 0, h=z) == abi.OK
