"""Every caller of the ordered column sum (vyomai_amd/csrc/vy_colsum.h) against tests/colsum_rule.py, bit for bit: the
workgroups riding in the grouped weight-gradient launch and the stand-alone launches on crafted slabs, and the
stand-alone launches behind the RMSNorm, LayerNorm and QK-norm backward kernels on the slabs those kernels leave.  The
data makes nearly every add round (colsum_rule.slab_data), so another order of the same adds is another result: what
each planted mutation moves is measured in test_colsum_rule_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests import colsum_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(F32, id="fp32")]
ACC = [pytest.param(False, id="overwrite"), pytest.param(True, id="accumulate")]
EPS = 1e-6
START = 3.0


def _st():
    return torch.cuda.current_stream().cuda_stream


def start(N):
    return torch.full((N,), START, device=DEV)


def base(N, acc):
    return np.full(N, START, R.F32) if acc else None


def same_bits(got, want, what):
    got = got.detach().cpu()
    want = torch.tensor(np.asarray(want))
    assert torch.equal(got, want), f"{what}: {int((got.view(torch.int32) != want.view(torch.int32)).sum())} of {got.numel()} columns differ"


@functools.lru_cache(maxsize=None)
def crafted(W, N):
    """-> the two slabs [2, W, N] and their ordered column sums [2, N] without a base (one computation per shape)."""
    slabs = np.stack([R.slab_data(W, N, R.case_seed(W, N)), R.slab_data(W, N, R.case_seed(W, N) + 1)])
    sums = np.stack([R.ordered_colsum(s, R.slices_rule(W)) for s in slabs])
    slabs.setflags(write=False)
    sums.setflags(write=False)
    return slabs, sums


@pytest.mark.parametrize("acc", ACC)
@pytest.mark.parametrize("dtype", [pytest.param(BF, id="rider"), pytest.param(F32, id="standalone")])
@pytest.mark.parametrize("W,N", R.SLABS)
def test_crafted_slabs(W, N, dtype, acc):
    """A ColSum entry and nothing else: bf16 sums it in riding workgroups of the grouped launch, fp32 in the stand-alone
    launches (which overwrite slab rows when there are several slices: they get a copy)."""
    from vyomai_amd import ops
    slabs, sums = crafted(W, N)
    ws = torch.tensor(slabs).reshape(-1).to(DEV)
    dg, db = start(N), start(N)
    ops.linear_wgrad_grouped([ops.ColSum(ws.clone(), dg, db, acc, dtype)])
    torch.cuda.synchronize()
    for s, (out, name) in enumerate(((dg, "out0"), (db, "out1"))):
        same_bits(out, base(N, acc) + sums[s] if acc else sums[s], f"{name} of {W} x {N}")   # (base + total: the rule's last add)


def rms_launch(M, N, dtype, acc):
    """vy_rmsnorm_bwd with the test's own slab -> (dw, slab [WB, N], the guard floats behind it)."""
    from vyomai_amd import _lib
    WB = _lib.load().vy_layernorm_bwd_ws_rows(M)
    g = torch.Generator().manual_seed(M + N)
    dy = torch.randn(M, N, generator=g).to(dtype).to(DEV)
    x = torch.randn(M, N, generator=g).to(dtype).to(DEV)
    w = (1 + 0.1 * torch.randn(N, generator=g)).to(dtype).to(DEV)
    dx = torch.empty_like(x)
    dw = start(N)
    ws = torch.full((WB * N + 64,), -7.5, device=DEV)
    _lib.call("vy_rmsnorm_bwd", dy.data_ptr(), N, x.data_ptr(), N, w.data_ptr(), None, 0, dx.data_ptr(), N, dw.data_ptr(),
              1.0 if acc else 0.0, ws.data_ptr(), M, N, EPS, 0.0, _lib.dtype_code(dtype), _st())
    torch.cuda.synchronize()
    return dw, ws[:WB * N].view(WB, N).cpu().numpy(), ws[WB * N:].cpu()


@pytest.mark.parametrize("acc", ACC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [200, 252])
def test_rmsnorm_one_slice(M, dtype, acc):
    """50 and 63 slab rows: one slice, nothing of the slab is overwritten, dw is its ordered column sum."""
    N = 136
    dw, slab, guard = rms_launch(M, N, dtype, acc)
    assert slab.shape[0] == (M + 3) // 4 and bool((guard == -7.5).all())
    same_bits(dw, R.ordered_colsum(slab, 1, base(N, acc)), f"dw of {M} x {N}")


@pytest.mark.parametrize("acc", ACC)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_fourteen_slices(dtype, acc):
    """70 slab rows: the first row of each of the 14 slices holds the slice's sum afterwards, and dw is those rows added
    from 0.f in slice order.  (The slice sums themselves are held by test_crafted_slabs and test_layernorm.)"""
    M, N = 280, 136
    dw, slab, guard = rms_launch(M, N, dtype, acc)
    assert slab.shape[0] == 70 and R.slices_rule(70) == 16 and bool((guard == -7.5).all())
    firsts = [slab[w0] for w0 in range(0, 70, 5)]
    assert len(firsts) == 14
    same_bits(dw, R.add_slices(firsts, base(N, acc)), "dw of 280 x 136")


@pytest.mark.parametrize("acc", ACC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [280, 2048])
def test_layernorm(M, dtype, acc):
    """70 and 512 slab rows: dgamma / dbeta of layernorm_bwd are the ordered column sums of the slab pair that
    layernorm_bwd_partial leaves on the same inputs."""
    from vyomai_amd import ops
    N = 136
    g = torch.Generator().manual_seed(M)
    dy = torch.randn(M, N, generator=g).to(dtype).to(DEV)
    x = (2 * torch.randn(M, N, generator=g) + 0.3).to(dtype).to(DEV)
    gamma = (1 + 0.1 * torch.randn(N, generator=g)).to(dtype).to(DEV)
    mean = x.float().mean(-1)
    rstd = torch.rsqrt(x.float().var(-1, unbiased=False) + EPS)
    _, ws = ops.layernorm_bwd_partial(dy, x, gamma, mean, rstd)
    torch.cuda.synchronize()
    WB = ws.numel() // (2 * N)
    assert WB == min(512, M // 4)
    slabs = ws.view(2, WB, N).cpu().numpy()
    dg, db = start(N), start(N)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db, accumulate=acc)
    torch.cuda.synchronize()
    same_bits(dg, R.ordered_colsum(slabs[0], R.slices_rule(WB), base(N, acc)), f"dgamma of {M} x {N}")
    same_bits(db, R.ordered_colsum(slabs[1], R.slices_rule(WB), base(N, acc)), f"dbeta of {M} x {N}")


@pytest.mark.parametrize("acc", ACC)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,h,hk,dh", R.QK_CASES)
def test_qknorm(T, h, hk, dh, dtype, acc):
    """vy_qknorm_bwd with the test's own slab, which is never overwritten: columns [0, dh) sum to dq_scale, [dh, 2 dh) to
    dk_scale, in ONE slice at any row count."""
    from vyomai_amd import _lib
    floats = _lib.load().vy_qknorm_bwd_ws_floats(T, h, hk, dh)
    rows = R.qk_slab_rows(T, h, hk, dh)
    assert floats == rows * 2 * dh
    Wd = (h + 2 * hk) * dh
    g = torch.Generator().manual_seed(T + dh)
    qkv = torch.randn(T, Wd, generator=g).to(dtype).to(DEV)
    dqkv = torch.randn(T, Wd, generator=g).to(dtype).to(DEV)
    qs = (1 + 0.1 * torch.randn(dh, generator=g)).to(DEV)
    ks = (1 + 0.1 * torch.randn(dh, generator=g)).to(DEV)
    dq, dk = start(dh), start(dh)
    ws = torch.full((floats + 64,), -7.5, device=DEV)
    _lib.call("vy_qknorm_bwd", dqkv.data_ptr(), Wd, qkv.data_ptr(), Wd, qs.data_ptr(), ks.data_ptr(), EPS, dq.data_ptr(),
              dk.data_ptr(), 1.0 if acc else 0.0, ws.data_ptr(), T, h, hk, dh, _lib.dtype_code(dtype), _st())
    torch.cuda.synchronize()
    assert bool((ws[floats:] == -7.5).all())
    slab = ws[:floats].view(rows, 2 * dh).cpu().numpy()
    same_bits(dq, R.ordered_colsum(slab[:, :dh], 1, base(dh, acc)), f"dq_scale of {rows} rows")
    same_bits(dk, R.ordered_colsum(slab[:, dh:], 1, base(dh, acc)), f"dk_scale of {rows} rows")
