"""vy_qknorm_rope_fwd and vy_qknorm_bwd (vy_qknorm.hip) against float64 torch on the same rounded inputs, in fp32 and
bf16.  The head widths take a lane group of 1 (dh 8), 8, 16 and 32 (256) lanes, and the 12-of-16 (96) and 28-of-32 (224)
groups with idle lanes."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
UNIT = {torch.float32: 2.0 ** -24, BF: 2.0 ** -8}      # unit roundoff of the storage type
SHAPES = [(4, 2, 64), (2, 1, 224), (8, 2, 128), (1, 1, 8), (3, 1, 256), (2, 2, 96)]
EPS = 1e-6
SENTINEL = 7.5


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def scales(g, dh):
    return ((1.0 + 0.1 * (2 * torch.rand(dh, generator=g) - 1)).float(), (1.0 + 0.1 * (2 * torch.rand(dh, generator=g) - 1)).float())


def packed_rows(g, T, h, hk, dh, dtype, zero_tok):
    """(T, W + 8) rows in `dtype`: randn heads, the last q head and the first k head of token zero_tok all zero, the
    8 pad columns a sentinel -> (rows, W)."""
    H3 = h + 2 * hk
    x = torch.randn(T, H3, dh, generator=g)
    x[zero_tok, h - 1] = 0.0
    x[zero_tok, h] = 0.0
    W = H3 * dh
    rows = torch.full((T, W + 8), SENTINEL)
    rows[:, :W] = x.view(T, W)
    return rows.to(dtype), W


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pos0", [0, 91])
@pytest.mark.parametrize("h,hk,dh", SHAPES)
def test_qknorm_rope_fwd_vs_fp64(h, hk, dh, pos0, dtype):
    """B x L = 3 x 50 rows with ld = W + 8, q and k written into strided views of larger sentinel-filled buffers.

    Bound: the derived one of test_qknorm_rope_write_vs_fp64 (tests/test_qwen3_gpu.py) -- the arithmetic is the same
    function (vy_qknorm.h) -- (dh/2 + 12) 2^-24 (|a'| + |b'|) relative to the fp64 normalised pair a', b', plus ONE
    rounding at the store, u_store |want|.  The input rows, their pads and everything outside the two views keep their
    bits; an all-zero head comes out as zeros."""
    from vyomai_amd import ops
    g = torch.Generator().manual_seed(dh + h + pos0)
    B, L, table_rows = 3, 50, 160
    T, zero_tok = B * L, 77
    rows, W = packed_rows(g, T, h, hk, dh, dtype, zero_tok)
    qs, ks = scales(g, dh)
    inv = 1.0 / (1e6 ** (torch.arange(0, dh, 2).float() / dh))
    ang = torch.outer(torch.arange(table_rows).float(), inv)
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    qkv = rows.to(DEV).view(B, L, W + 8)
    qbuf = torch.full((B, h, L + 3, dh + 8), SENTINEL, dtype=dtype, device=DEV)
    kbuf = torch.full((B + 1, hk, L + 2, dh + 16), SENTINEL, dtype=dtype, device=DEV)
    q, k = qbuf[:, :, 1:L + 1, :dh], kbuf[1:, :, 2:, :dh]
    ops.qknorm_rope(qkv, h, hk, dh, qs.to(DEV), ks.to(DEV), EPS, cos.to(DEV), sin.to(DEV), pos0, q, k)
    torch.cuda.synchronize()
    assert torch.equal(bits(qkv.cpu().view(T, W + 8)), bits(rows)), "the saved activation was modified"
    qc, kc = qbuf.cpu(), kbuf.cpu()
    got = torch.cat([qc[:, :, 1:L + 1, :dh], kc[1:, :, 2:, :dh]], dim=1).permute(0, 2, 1, 3).reshape(T, h + hk, dh)
    assert torch.isfinite(got.float()).all()
    x = rows[:, :W].double().view(T, h + 2 * hk, dh)[:, :h + hk]
    scale = torch.cat([qs.double().expand(h, dh), ks.double().expand(hk, dh)])
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * scale
    pos = (pos0 + torch.arange(L)).repeat(B)
    c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    a, b = n[..., :dh // 2], n[..., dh // 2:]
    want = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    mag = (a.abs() + b.abs()).repeat(1, 1, 2)
    err = (got.double() - want).abs()
    bound = UNIT[dtype] * want.abs() + (dh / 2 + 12) * 2.0 ** -24 * mag
    live = bound > 0
    print(f"qknorm + rope forward max err / bound {float((err[live] / bound[live]).max()):.3f}")
    assert (err <= bound).all()
    zero = got[zero_tok, h - 1:h + 1].float()
    assert (zero == 0).all(), "an all-zero head must give zeros"
    # everything outside the two views keeps the sentinel
    qc[:, :, 1:L + 1, :dh] = SENTINEL
    kc[1:, :, 2:, :dh] = SENTINEL
    assert (qc.float() == SENTINEL).all() and (kc.float() == SENTINEL).all()


def _bwd_case(h, hk, dh, T, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    rows, W = packed_rows(g, T, h, hk, dh, dtype, T // 2)
    drows, _ = packed_rows(g, T, h, hk, dh, dtype, 0)
    drows[0, (h - 1) * dh:(h + 1) * dh] = torch.randn(2 * dh, generator=g).to(dtype)    # (no zero heads in dy)
    qs, ks = scales(g, dh)
    start = torch.randn(2, dh, generator=g)
    return rows, drows, W, qs, ks, start


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h,hk,dh,T", [s + (150,) for s in SHAPES] + [(1, 1, 8, 2100), (8, 2, 128, 2100), (8, 2, 128, 3300)])
def test_qknorm_bwd_vs_fp64(h, hk, dh, T, dtype):
    """T = 150 is 2 to 29 workgroups' worth of partials; T = 2100 is 17 workgroups at dh = 8 (256 units each, the last
    partly filled) and 657 at (8, 2, 128) (two slices of 16 units each, the last slice half filled: the load-ahead path),
    so the fixed-order sum over the slab runs over many rows per row group; T = 3300 there (a case of this file's own)
    makes it three slices each.

    dx against fp64 autograd of x * rsqrt(mean x^2 + eps) * g within 1e-5 (1 + |want|) + rtol |want|, rtol 0 (fp32) or
    2^-7 (bf16: the one store rounding): the floor scales with |want| because the all-zero heads have r = 1000.  The scale
    gradients within 1e-5 sqrt(units) (the bar of test_rmsnorm_bwd_vs_fp64 for fp32 sums), with beta = 1 onto a random
    start.  The dv columns, both pads and the saved rows keep their bits; a second run gives the same bits."""
    from vyomai_amd import ops
    rows, drows, W, qs, ks, start = _bwd_case(h, hk, dh, T, dtype, 7 * dh + h + T)
    H2 = h + hk

    def run():
        d = drows.to(DEV)
        dq, dk = start[0].to(DEV).clone(), start[1].to(DEV).clone()
        x = rows.to(DEV)
        ops.qknorm_bwd_(d[:, :W], x[:, :W], h, hk, dh, qs.to(DEV), ks.to(DEV), EPS, dq, dk, True)
        torch.cuda.synchronize()
        return d.cpu(), dq.cpu(), dk.cpu(), x.cpu()

    got, dq, dk, x_after = run()
    assert torch.equal(bits(x_after), bits(rows)), "the saved activation was modified"
    assert torch.equal(bits(got[:, H2 * dh:]), bits(drows[:, H2 * dh:])), "dv columns or the pad changed"
    x = rows[:, :H2 * dh].double().view(T, H2, dh).requires_grad_(True)
    gq, gk = qs.double().requires_grad_(True), ks.double().requires_grad_(True)
    scale = torch.cat([gq.expand(h, dh), gk.expand(hk, dh)])
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * scale
    (n * drows[:, :H2 * dh].double().view(T, H2, dh)).sum().backward()
    want = x.grad.view(T, H2 * dh)
    err = (got[:, :H2 * dh].double() - want).abs()
    rtol = 0.0 if dtype == torch.float32 else 2.0 ** -7
    bound = 1e-5 * (1 + want.abs()) + rtol * want.abs()
    print(f"qknorm backward dx max err / bound {float((err / bound).max()):.3f}, largest |dx| {float(want.abs().max()):.1f}")
    assert torch.isfinite(got.float()).all() and (err <= bound).all()
    for name, g_got, g_want, s0, units in (("dq_scale", dq, gq.grad, start[0], T * h), ("dk_scale", dk, gk.grad, start[1], T * hk)):
        e = float((g_got.double() - (s0.double() + g_want)).abs().max())
        print(f"{name} max err {e:.3e}, bar {1e-5 * units ** 0.5:.3e}")
        assert e <= 1e-5 * units ** 0.5, name
    again = run()
    assert torch.equal(bits(again[0]), bits(got)) and torch.equal(again[1], dq) and torch.equal(again[2], dk)


def test_qknorm_bwd_overwrites_with_beta_zero():
    from vyomai_amd import ops
    h, hk, dh, T = 4, 2, 64, 150
    rows, drows, W, qs, ks, start = _bwd_case(h, hk, dh, T, BF, 3)
    outs = []
    for fill in (0.0, float("nan")):
        d, x = drows.to(DEV), rows.to(DEV)
        dq, dk = torch.full((dh,), fill, device=DEV), torch.full((dh,), fill, device=DEV)
        ops.qknorm_bwd_(d[:, :W], x[:, :W], h, hk, dh, qs.to(DEV), ks.to(DEV), EPS, dq, dk, False)
        outs.append((dq.cpu(), dk.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[1][0]).all() and float(outs[1][0].abs().max()) > 0
