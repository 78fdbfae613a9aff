"""The staged GEMM epilogue requests every second operand of a whole tile (the saved act' tensor of a dgrad, the
residual, the second residual) in one batch before its store loop instead of one load per 16-byte chunk inside it
(gemm_epilogue, vy_gemm.hip).  The arithmetic per element is the same, so the two paths -- switched in one process by
vy_debug_set_epilogue_prefetch -- must agree bit for bit, on whole tiles, on ragged ones (which keep the loop) and on
launches that hold both; each case is also held against the fp64 reference of the dgrad / linear tests, at their tolerance."""
import ctypes as C
import math

import pytest
import torch

from tests.test_kernels_gpu import check, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _both(fn):
    """fn() with the prefetch on, then off -> (on, off); the switch is left on."""
    from vyomai_amd import _lib
    lib = _lib.load()
    lib.vy_debug_set_epilogue_prefetch.argtypes = [C.c_int]
    try:
        lib.vy_debug_set_epilogue_prefetch(1)
        on = fn()
        lib.vy_debug_set_epilogue_prefetch(0)
        off = fn()
    finally:
        lib.vy_debug_set_epilogue_prefetch(1)
    torch.cuda.synchronize()
    return on, off


# 256 x 256 tiles (output width 3072): 2560 rows are 10 whole row tiles, 2600 add a ragged 11th -- both paths in one launch
@pytest.mark.parametrize("M", [2560, 2600])
def test_dgrad_saved_derivative_256x256(M):
    from vyomai_amd import _lib, ops
    N, K = 3072, 128                                   # output columns, contraction
    dy = rnd(M, K, seed=1).to(BF)
    wt = (rnd(N, K, seed=2) / math.sqrt(K)).to(BF)     # W^T as vy_linear_dgrad takes it: [output columns, contraction]
    p = rnd(M, N, seed=3).double().requires_grad_(True)
    torch.nn.functional.gelu(p).sum().backward()
    deriv = p.grad.to(BF)                              # what FFN1 saves with ACT_SAVE_DERIV: act'(pre), rounded
    want = (dy.double() @ wt.double().t()) * deriv.double()
    dyd, wtd, dd = dy.to(DEV), wt.to(DEV), deriv.to(DEV)
    on, off = _both(lambda: ops.linear_dgrad(dyd, wtd, dd, _lib.ACT_GELU_ERF | _lib.ACT_SAVE_DERIV))
    assert torch.equal(on, off)
    check(on, want, 4e-2, 1e-2, "dgrad with saved derivative")


# 256 x 192 tiles: 10240 x 768 is the smallest launch on the large-M branch at this width (40 x 4 tiles); 760 columns
# leave the last column tile ragged
@pytest.mark.parametrize("N", [768, 760])
def test_dgrad_two_residual_gradients_256x192(N):
    from vyomai_amd import ops
    M, K = 10240, 64
    dy = rnd(M, K, seed=1).to(BF)
    wt = (rnd(N, K, seed=2) / math.sqrt(K)).to(BF)
    a1, a2 = rnd(M, N, seed=4).to(BF), rnd(M, N, seed=5).to(BF)
    want = dy.double() @ wt.double().t() + a1.double() + a2.double()
    dyd, wtd, a1d, a2d = dy.to(DEV), wt.to(DEV), a1.to(DEV), a2.to(DEV)
    on, off = _both(lambda: ops.linear_dgrad(dyd, wtd, None, 0, a1d, None, a2d))
    assert torch.equal(on, off)
    check(on, want, 4e-2, 1e-2, "dgrad + add_to + add_to2")
    # one addend: the operand the 256 x 192 tile already requests before the staging
    on, off = _both(lambda: ops.linear_dgrad(dyd, wtd, None, 0, a1d))
    assert torch.equal(on, off)
    check(on, dy.double() @ wt.double().t() + a1.double(), 4e-2, 1e-2, "dgrad + add_to")


# 512 rows: 128 x 128 mid-M tiles; 264 rows: the all-rows tile (320 rows: ragged, keeps the loop)
@pytest.mark.parametrize("M", [512, 264])
def test_forward_residual_mid_m(M):
    from vyomai_amd import ops
    N, K = 768, 64
    x = rnd(M, K, seed=1).to(BF)
    w = rnd(N, K, seed=2, scale=1 / math.sqrt(K)).to(BF)
    b = rnd(N, seed=3, scale=0.1).to(BF)
    r = rnd(M, N, seed=4).to(BF)
    want = x.double() @ w.double().t() + b.double() + r.double()
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    on, off = _both(lambda: ops.linear(xd, wd, bd, residual=rd))
    assert torch.equal(on, off)
    check(on, want, 3e-2, 1e-2, "linear + residual")


def test_forward_tanh_gelu_residual_256x192_keeps_its_path():
    """The tanh GELU (and the run-time activations) stay on the path they had -- the 256 x 192 tile's request before the
    staging, the loop otherwise: held against the reference so that the shared chunk code cannot drift under them."""
    from vyomai_amd import _lib, ops
    M, N, K = 10240, 768, 64
    x = rnd(M, K, seed=1).to(BF)
    w = rnd(N, K, seed=2, scale=1 / math.sqrt(K)).to(BF)
    b = rnd(N, seed=3, scale=0.1).to(BF)
    r = rnd(M, N, seed=4).to(BF)
    pre = x.double() @ w.double().t() + b.double()
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    for act, fn in ((_lib.ACT_GELU_TANH, lambda t: torch.nn.functional.gelu(t, approximate="tanh")),
                    (_lib.ACT_SILU, torch.nn.functional.silu)):
        on, off = _both(lambda: ops.linear(xd, wd, bd, act=act, residual=rd))
        assert torch.equal(on, off)
        check(on, fn(pre) + r.double(), 3e-2, 1e-2, f"linear + act {act} + residual")
