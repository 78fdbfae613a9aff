"""Kernel-level parity: every C-ABI entry point vs the CPU oracle / a plain fp32-fp64 torch
restatement of the same op, on the same seeded inputs.  Runs on the MI355X box (-m gpu).

Tolerances: f32 kernels 1e-5 (north_star); bf16 kernels are compared with the oracle evaluated on
the bf16-rounded inputs, bar = a few bf16 ulps of the output scale.
"""
import math

import numpy as np
import pytest
import torch

from oracle import vyom_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from vyomai_amd import ops, _lib
    return ops, _lib


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def check(got, want, atol, rtol=0.0, what=""):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    bad = err > bound
    if bad.any():
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.numel()} off; max err {err.max():.3e} (atol {atol}); "
            f"first at {idx}: got {got[tuple(idx)]:.6f} want {want[tuple(idx)]:.6f}")


ACTS = {0: lambda x: x, 1: O.gelu_erf, 2: O.gelu_tanh}


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 768), (51, 1003, 768), (300, 768, 72),
                                   (16, 768, 768), (1, 256, 3072), (1024, 3072, 768), (640, 768, 3072),
                                   (32, 3072, 768), (32, 1003, 768), (7, 768, 3072), (32, 64, 40),
                                   # <= 4 rows: the matrix-vector kernel (one wave per output column)
                                   (1, 2048, 16384), (2, 1003, 768), (3, 770, 264), (4, 768, 3072), (1, 5, 8),
                                   # > 1024 rows: the 256 x 192 tile kernel (M / N / K tails)
                                   (2000, 768, 768), (4096, 1003, 768), (1500, 384, 72), (3072, 3072, 768),
                                   # mid-size M with few tiles: K split over workgroups (fp32 partial tiles + finish launch):
                                   # PaliGemma-shape prefill (264 rows; Gemma out-projection, SigLIP fc1 / fc2 with a K tail) and
                                   # the 2112 rows of the captioning decoder (configs[3])
                                   (264, 2048, 2048), (264, 2048, 16384), (256, 4304, 1152), (256, 1152, 4304), (2112, 768, 3072),
                                   (2112, 768, 768)])
@pytest.mark.parametrize("act", [0, 1])
def test_linear_bf16(M, N, K, act):
    ops, _ = _ops()
    x = rnd(M, K, seed=1).bfloat16()
    w = rnd(N, K, seed=2, scale=1 / math.sqrt(K)).bfloat16()
    b = rnd(N, seed=3, scale=0.1).bfloat16()
    r = rnd(M, N, seed=4).bfloat16()
    pre_ref = x.double() @ w.double().t() + b.double()
    want = ACTS[act](pre_ref) + r.double()
    ldy = (N + 7) // 8 * 8
    pre = torch.zeros(M, ldy, dtype=torch.bfloat16, device=DEV)
    y = ops.linear(x.to(DEV), w.to(DEV), b.to(DEV), act=act, residual=r.to(DEV), pre_out=pre[:, :N])
    torch.cuda.synchronize()
    check(y, want, 3e-2, 1e-2, f"linear bf16 {M}x{N}x{K} act{act}")
    check(pre[:, :N], pre_ref, 3e-2, 1e-2, "pre_out")
    # no bias / no residual / no pre path
    y2 = ops.linear(x.to(DEV), w.to(DEV))
    check(y2, x.double() @ w.double().t(), 3e-2, 1e-2, "linear bf16 plain")


def test_linear_bf16_wide_mid_m_and_split_k_equals_unsplit():
    """(264, 32768, 2048): Gemma's gate/up projection at prefill (768 tiles: not split).  And the split launches against
    the same GEMM without a workspace (one workgroup per tile walks all of K): equal up to the fp32 summation order."""
    ops, lib = _ops()
    M, N, K = 264, 32768, 2048
    x = rnd(M, K, seed=1).bfloat16().to(DEV)
    w = rnd(N, K, seed=2, scale=1 / math.sqrt(K)).bfloat16().to(DEV)
    y = ops.linear(x, w)
    cols = torch.arange(0, N, 37, device=DEV)
    check(y[:, cols], x.double() @ w[cols].double().t(), 3e-2, 1e-2, "gate/up shape")
    from vyomai_amd._lib import call
    for (M, N, K) in [(264, 2048, 16384), (256, 1152, 4304), (2112, 768, 3072)]:
        x = rnd(M, K, seed=3).bfloat16().to(DEV)
        w = rnd(N, K, seed=4, scale=1 / math.sqrt(K)).bfloat16().to(DEV)
        b = rnd(N, seed=5, scale=0.1).bfloat16().to(DEV)
        r = rnd(M, N, seed=6).bfloat16().to(DEV)
        split = ops.linear(x, w, b, act=1, residual=r)
        st = torch.cuda.current_stream()
        call("vy_workspace_set", st.cuda_stream, None, 0)            # no workspace: the one-launch kernel
        ops._WS.pop((st.device_index, st.cuda_stream), None)
        try:
            import vyomai_amd.ops as O_
            saved, O_._mid_ws = O_._mid_ws, lambda rows: None
            whole = ops.linear(x, w, b, act=1, residual=r)
        finally:
            O_._mid_ws = saved
        d = (split.float() - whole.float()).abs().max().item()
        assert d <= 2 ** -6 * max(1.0, whole.float().abs().max().item()), (M, N, K, d)   # a bf16 rounding step at most
        # the same two launches on integer data: every partial sum is exact, so the split is invisible
        xi, wi = ints(M, K, seed=3).bfloat16().to(DEV), thin_ternary(N, K, K, seed=4).bfloat16().to(DEV)
        bi, ri = ints(N, seed=5, lo=-2, hi=2).bfloat16().to(DEV), ints(M, N, seed=6, lo=-2, hi=2).bfloat16().to(DEV)
        want = xi.float().cpu() @ wi.float().cpu().t() + bi.float().cpu() + ri.float().cpu()
        assert_bf16_exact(want, f"split-K {M}x{N}x{K}")
        for act in (0, 1):
            split = ops.linear(xi, wi, bi, act=act, residual=ri)
            call("vy_workspace_set", st.cuda_stream, None, 0)
            ops._WS.pop((st.device_index, st.cuda_stream), None)
            try:
                saved, O_._mid_ws = O_._mid_ws, lambda rows: None
                whole = ops.linear(xi, wi, bi, act=act, residual=ri)
            finally:
                O_._mid_ws = saved
            check_exact(split, whole, f"split-K against one launch, integer data, act {act}, {M}x{N}x{K} (m, n)")
            if act == 0:
                check_exact(whole, want, f"one launch, integer data {M}x{N}x{K} (m, n)")


# ---- exact-integer GEMMs: small-integer inputs are exact in bf16, every partial sum is an integer far below 2^24, so
# fp32 accumulation is exact IN ANY ORDER (split-K included) and the bar is zero.  These cover indexing, tails, tiling and
# the epilogue order; the Gaussian tests above cover GELU and the bars on real-valued data.
def ints(*shape, seed=0, lo=-1, hi=1):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def thin_ternary(N, K, red, seed=0):
    """Weight in {-1, 0, 1}, each entry kept with probability min(1, 1024 / red) (red: the reduction length).  The WEIGHT
    is thinned, not the activation, so that every k of every activation row meets a non-zero weight in some column."""
    g = torch.Generator().manual_seed(seed + 77 * N + K)
    keep = torch.rand(N, K, generator=g) < min(1.0, 1024.0 / red)
    return ints(N, K, seed=seed) * keep


def assert_bf16_exact(want, what):
    """bf16 holds every integer of magnitude <= 256: the expected values must all be there (100 % of the elements)."""
    big = float(want.abs().max())
    assert big <= 256, f"{what}: expected magnitude {big} is not exact in bf16; the test data is wrong"


def check_exact(got, want, what):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = ~(got == want)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} not bit-exact; first at {idx}: "
                             f"got {got[tuple(idx)]} want {want[tuple(idx)]}")


LINEAR_SHAPES = [(128, 128, 64), (256, 384, 768), (51, 1003, 768), (300, 768, 72),
                 (16, 768, 768), (1, 256, 3072), (1024, 3072, 768), (640, 768, 3072),
                 (32, 3072, 768), (32, 1003, 768), (7, 768, 3072), (32, 64, 40),
                 (1, 2048, 16384), (2, 1003, 768), (3, 770, 264), (4, 768, 3072), (1, 5, 8),
                 (2000, 768, 768), (4096, 1003, 768), (1500, 384, 72), (3072, 3072, 768),
                 (264, 2048, 2048), (264, 2048, 16384), (256, 4304, 1152), (256, 1152, 4304), (2112, 768, 3072),
                 (2112, 768, 768)]       # test_linear_bf16's list
LINEAR_EDGES = [
    # gemv (<= 4 rows) / skinny
    (5, 768, 3072), (5, 1003, 768),
    # skinny (<= 32 rows) / mid
    (33, 3072, 768), (33, 1003, 768),
    # the all-rows tiles: 128 x 128 up to 128 rows, 256 x 128 up to 256, 320 x 128 up to 320, then 128 x 128 again
    (128, 768, 768), (129, 768, 768), (256, 768, 768), (257, 768, 768), (320, 768, 768), (321, 768, 768),
    (129, 1003, 264), (257, 1003, 264), (321, 1003, 264),
    # mid / large: 1025 rows leave the mid-size tiles once the 256 x 192 grid has 160 tiles (N >= 5953)
    (1024, 768, 768), (1025, 768, 768), (1024, 6144, 264), (1025, 6144, 264),
    # 256 x 192 tiles with the three-deep ring (N < 3072) / 256 x 256 tiles; at 2048 rows the 3071 / 3072 grids have 128
    # tiles and stay on the mid-size kernel, at 4096 rows they are the two large kernels
    (2048, 3071, 768), (2048, 3072, 768), (4096, 3071, 768), (4096, 3072, 264),
    # skinny width limit (N <= 8192), then the 32 x 128 fallback
    (32, 8192, 768), (32, 8200, 768),
    # K = 16: not a multiple of 32 (the 32-column skinny kernel); K = 8: the 32 x 128 fallback
    (32, 768, 16), (32, 768, 8)]
assert not set(LINEAR_SHAPES) & set(LINEAR_EDGES)


@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES + LINEAR_EDGES)
def test_linear_bf16_exact(M, N, K):
    ops, _ = _ops()
    x = ints(M, K, seed=1)
    w = thin_ternary(N, K, K, seed=2)
    b = ints(N, seed=3, lo=-2, hi=2)
    r = ints(M, N, seed=4, lo=-2, hi=2)
    plain = x @ w.t()                   # fp32 on the CPU: integers below 2^24, exact
    pre_ref = plain + b
    want = pre_ref + r
    for t, what in ((plain, "x w^T"), (pre_ref, "pre"), (want, "y")):
        assert_bf16_exact(t, f"{M}x{N}x{K} {what}")
    xd, wd = x.bfloat16().to(DEV), w.bfloat16().to(DEV)
    ldy = (N + 7) // 8 * 8
    pre = torch.zeros(M, ldy, dtype=torch.bfloat16, device=DEV)
    y = ops.linear(xd, wd, b.bfloat16().to(DEV), act=0, residual=r.bfloat16().to(DEV), pre_out=pre[:, :N])
    torch.cuda.synchronize()
    check_exact(y, want, f"linear bf16 exact {M}x{N}x{K} (m, n)")
    check_exact(pre[:, :N], pre_ref, "pre_out (m, n)")
    if ldy > N:
        assert float(pre[:, N:].abs().max()) == 0, "pre_out: padding columns written"
    check_exact(ops.linear(xd, wd), plain, f"linear bf16 exact plain {M}x{N}x{K} (m, n)")
    if N % 8:
        # rows that are not 16-byte aligned: the scalar epilogue
        out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        ops.linear(xd, wd, out=out)
        check_exact(out, plain, f"linear bf16 exact, unpadded rows {M}x{N}x{K} (m, n)")


@pytest.mark.parametrize("M,N,K", [(51, 1003, 768), (130, 64, 16), (64, 64, 4), (257, 192, 260)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_f32(M, N, K, act):
    ops, _ = _ops()
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    b, r = rnd(N, seed=3, scale=0.1), rnd(M, N, seed=4)
    want = ACTS[act](x.double() @ w.double().t() + b.double()) + r.double()
    y = ops.linear(x.to(DEV), w.to(DEV), b.to(DEV), act=act, residual=r.to(DEV))
    check(y, want, 1e-5, 1e-5, f"linear f32 {M}x{N}x{K}")


def _qkv_ref(x, w, b, h, hk, dh, pos0, rope, dtype):
    """oracle: three projections -> split heads -> apply_rotary in `dtype` like the reference."""
    B, L, _ = x.shape
    y = (x.double() @ w.double().t() + b.double()).to(dtype)
    q, k, v = y.split([h * dh, hk * dh, hk * dh], dim=-1)
    q, k, v = O.split_heads(q, dh), O.split_heads(k, dh), O.split_heads(v, dh)
    if rope:
        fr = O.rotary_angles(dh, pos0 + L + 1)[:, pos0:pos0 + L]
        q, k = O.apply_rotary(q, k, fr)
    return q, k, v


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,L,K,h,hk,dh,rope", [(2, 96, 768, 12, 4, 64, True), (2, 17, 64, 4, 2, 16, True),
                                               (3, 50, 768, 12, 12, 64, False), (2, 1, 768, 12, 4, 64, True),
                                               (1, 40, 256, 2, 1, 128, True), (4, 300, 768, 12, 4, 64, True),
                                               (32, 1, 768, 12, 12, 64, True), (5, 1, 768, 12, 4, 64, False),
                                               (3, 700, 768, 12, 12, 64, True),
                                               # <= 4 rows without the fused rotary epilogue: the matrix-vector kernel
                                               (1, 1, 2048, 8, 1, 256, True), (3, 1, 256, 2, 1, 128, False),
                                               (4, 1, 768, 12, 4, 64, False), (2, 2, 1152, 16, 16, 72, False)])
def test_qkv_rope(dtype, B, L, K, h, hk, dh, rope):
    ops, _ = _ops()
    pos0 = 5
    N = (h + 2 * hk) * dh
    x = rnd(B, L, K, seed=1).to(dtype)
    w = rnd(N, K, seed=2, scale=1 / math.sqrt(K)).to(dtype)
    b = rnd(N, seed=3, scale=0.1).to(dtype)
    qr, kr, vr = _qkv_ref(x, w, b, h, hk, dh, pos0, rope, dtype)
    cos = sin = None
    if rope:
        cos, sin = ops.rope_tables(dh, 64 + L, DEV)
    q = torch.zeros(B, h, L, dh, dtype=dtype, device=DEV)
    # k/v written straight into a (B, hk, maxlen, dh) static cache at pos0
    kc = torch.zeros(B, hk, pos0 + L + 3, dh, dtype=dtype, device=DEV)
    vc = torch.zeros_like(kc)
    ops.qkv_rope(x.to(DEV), w.to(DEV), b.to(DEV), h, hk, dh, cos, sin, pos0, q,
                 kc[:, :, pos0:pos0 + L], vc[:, :, pos0:pos0 + L])
    tol = 4e-2 if dtype == torch.bfloat16 else 1e-5
    check(q, qr, tol, tol, "q")
    check(kc[:, :, pos0:pos0 + L], kr, tol, tol, "k (cache slice)")
    check(vc[:, :, pos0:pos0 + L], vr, tol, tol, "v (cache slice)")
    assert float(kc[:, :, :pos0].abs().max()) == 0 and float(kc[:, :, pos0 + L:].abs().max()) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,L,K,h,hk,dh", [(3, 50, 768, 12, 12, 64), (5, 1, 768, 12, 4, 64), (3, 1, 256, 2, 1, 128),
                                          (4, 1, 768, 12, 4, 64), (2, 2, 1152, 16, 16, 72)])
def test_qkv_no_rope_exact(dtype, B, L, K, h, hk, dh):
    """The rows of test_qkv_rope without rotary, on integer data: q and the K / V cache slices bit-exact, the cache rows
    outside [pos0, pos0 + L) still zero."""
    ops, _ = _ops()
    pos0 = 5
    N = (h + 2 * hk) * dh
    x = ints(B, L, K, seed=1)
    w = thin_ternary(N, K, K, seed=2)
    b = ints(N, seed=3, lo=-2, hi=2)
    y = x @ w.t() + b
    assert_bf16_exact(y, "qkv")
    qr, kr, vr = (O.split_heads(t, dh) for t in y.split([h * dh, hk * dh, hk * dh], dim=-1))
    q = torch.zeros(B, h, L, dh, dtype=dtype, device=DEV)
    kc = torch.zeros(B, hk, pos0 + L + 3, dh, dtype=dtype, device=DEV)
    vc = torch.zeros_like(kc)
    ops.qkv_rope(x.to(dtype).to(DEV), w.to(dtype).to(DEV), b.to(dtype).to(DEV), h, hk, dh, None, None, pos0, q,
                 kc[:, :, pos0:pos0 + L], vc[:, :, pos0:pos0 + L])
    check_exact(q, qr, "q (b, head, l, c)")
    check_exact(kc[:, :, pos0:pos0 + L], kr, "k (cache slice)")
    check_exact(vc[:, :, pos0:pos0 + L], vr, "v (cache slice)")
    for c in (kc, vc):
        assert float(c[:, :, :pos0].abs().max()) == 0 and float(c[:, :, pos0 + L:].abs().max()) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,N", [(51, 768), (4, 64), (1000, 2048), (33, 1152)])
def test_layernorm(dtype, M, N):
    ops, _ = _ops()
    x = (rnd(M, N, seed=1) * 2 + 0.5).to(dtype)
    g = (1 + 0.1 * rnd(N, seed=2)).to(dtype)
    b = (0.1 * rnd(N, seed=3)).to(dtype)
    want = torch.nn.functional.layer_norm(x.double(), (N,), g.double(), b.double(), 1e-5)
    y, mean, rstd = ops.layernorm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5, save_stats=True)
    tol = 3e-2 if dtype == torch.bfloat16 else 2e-6
    check(y, want, tol, tol, "layernorm")
    check(mean, x.double().mean(-1), 1e-5, 1e-5, "mean")
    check(rstd, (x.double().var(-1, unbiased=False) + 1e-5).rsqrt(), 1e-5, 1e-5, "rstd")


def _dense_mask(B, L, S, causal, start_pos, keypad, addmask):
    m = torch.zeros(B, 1, L, S)
    fmin = torch.finfo(torch.float32).min
    if causal:
        i = torch.arange(L)[:, None]
        j = torch.arange(S)[None, :]
        m = m + torch.where(j <= i + start_pos, 0.0, fmin)[None, None]
    if keypad is not None:
        m = m + (1.0 - keypad[:, None, None, :].float()) * fmin
    m = m.clamp_min(fmin)  # (1-c*k)*min in the reference is one factor: never -inf
    if addmask is not None:
        m = m + addmask
    return m


ATTN_CASES = [
    # B, h, hk, L, S, dh, causal, start, keypad, additive
    (2, 4, 2, 200, 200, 64, True, 0, False, False),
    (2, 4, 4, 128, 128, 64, False, 0, False, False),
    (2, 4, 2, 130, 130, 64, True, 0, True, False),
    (2, 12, 4, 40, 100, 64, True, 60, True, False),
    (1, 2, 2, 70, 70, 64, False, 0, True, False),
    (2, 2, 1, 65, 65, 64, False, 0, False, True),
    (2, 3, 3, 512, 512, 64, True, 0, False, False),
    (1, 2, 1, 150, 150, 128, True, 0, False, False),
    (2, 2, 2, 64, 64, 128, False, 0, True, False),
    (2, 4, 2, 17, 17, 16, True, 0, True, False),   # row-wise kernel (dh 16)
    (3, 12, 12, 197, 197, 64, False, 0, False, False),  # ViT shape
    # other head widths: the general MFMA kernel (bf16) / the row-wise kernel (fp32)
    (1, 16, 16, 256, 256, 72, False, 0, False, False),   # SigLIP-So400m (Examples/paligemma.ipynb cell 9)
    (2, 8, 1, 264, 264, 256, True, 0, False, False),     # Gemma-2B prefill, MQA (cell 12)
    (2, 8, 1, 70, 110, 256, True, 40, True, False),      # chunked prefill with padding (left padding: dead rows)
    (2, 3, 3, 100, 100, 96, False, 0, True, False),
    (1, 2, 2, 130, 130, 160, True, 0, False, False),
    (2, 4, 2, 33, 33, 72, True, 0, True, False),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_fwd(dtype, case):
    ops, _ = _ops()
    B, h, hk, L, S, dh, causal, start, use_kp, use_add = case
    q = rnd(B, h, L, dh, seed=1).to(dtype)
    k = rnd(B, hk, S, dh, seed=2).to(dtype)
    v = rnd(B, hk, S, dh, seed=3).to(dtype)
    keypad = None
    if use_kp:
        keypad = torch.ones(B, S, dtype=torch.uint8)
        keypad[0, S - S // 3:] = 0            # right padding
        if B > 1:
            keypad[1, : min(5, S - 1)] = 0    # LEFT padding: with a causal mask rows 0..4 are fully masked
    addmask = None
    if use_add:
        addmask = rnd(B, 1, L, S, seed=5)
        addmask[:, :, :, ::7] = torch.finfo(torch.float32).min
    mask = _dense_mask(B, L, S, causal, start, keypad, addmask)
    want = O.merge_heads(O.sdpa(q.float(), O.repeat_kv(k.float(), h // hk), O.repeat_kv(v.float(), h // hk), mask))
    lse = torch.zeros(B, h, L, dtype=torch.float32, device=DEV)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, start_pos=start,
                        keypad=keypad.to(DEV) if keypad is not None else None,
                        addmask=addmask.to(DEV) if addmask is not None else None, lse=lse)
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    check(got, want, tol, tol, f"attention {case}")
    s = (q.float() @ O.repeat_kv(k.float(), h // hk).transpose(-1, -2)) / math.sqrt(dh) + mask
    live = (mask > torch.finfo(torch.float32).min / 2).any(-1).expand(B, h, L)  # skip fully masked rows
    ref_lse = torch.logsumexp(s.double(), -1)
    check(torch.where(live, lse.cpu().double(), 0.0), torch.where(live, ref_lse, 0.0),
          2e-2 if dtype == torch.bfloat16 else 1e-4, 1e-4, "lse")


# ---- the tuned kernels' stage writer and mask words, byte for byte ----------------------------------------------------
# B = 1, h = 2, hk = 1, L = 200, K / V with 256 random rows.  200 keys are four key tiles for the three-deep ring (a slot
# is reused) and end in a ragged tile of 8 keys.
def attn_tile_case(dh, seed=20):
    q = rnd(1, 2, 200, dh, seed=seed).to(torch.bfloat16).to(DEV)
    k = rnd(1, 1, 256, dh, seed=seed + 1).to(torch.bfloat16).to(DEV)
    v = rnd(1, 1, 256, dh, seed=seed + 2).to(torch.bfloat16).to(DEV)
    hide = torch.ones(1, 256, dtype=torch.uint8, device=DEV)
    hide[:, 200:] = 0
    return q, k, v, hide


def attn_tile_fwd(ops, q, k, v, S, causal, keypad):
    lse = torch.zeros(1, 2, 200, dtype=torch.float32, device=DEV)
    out = ops.attention(q, k[:, :, :S], v[:, :, :S], causal=causal, keypad=keypad, lse=lse)
    return out, lse


def same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    n = a.element_size()
    diff = (a.view(torch.uint8).view(-1, n) != b.view(torch.uint8).view(-1, n)).any(-1)
    assert not diff.any(), f"{what}: {int(diff.sum())}/{diff.numel()} elements differ, first at flat index {int(diff.nonzero()[0])}"


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dh", [64, 128])
def test_attention_fwd_keypad_of_ones_equals_no_keypad(dh, causal):
    ops, _ = _ops()
    q, k, v, _hide = attn_tile_case(dh)
    ones = torch.ones(1, 200, dtype=torch.uint8, device=DEV)
    a = attn_tile_fwd(ops, q, k, v, 200, causal, None)
    b = attn_tile_fwd(ops, q, k, v, 200, causal, ones)
    same_bytes(a[0], b[0], "out")
    same_bytes(a[1], b[1], "lse")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dh", [64, 128])
def test_attention_fwd_short_s_equals_padded_s(dh, causal):
    """S = 200 without a mask (the last tile takes the clamped-row writer path) == S = 256 with keys 200..255 hidden by a
    key-padding mask (the same tile takes the whole-tile path, the mask word hides the keys)."""
    ops, _ = _ops()
    q, k, v, hide = attn_tile_case(dh)
    a = attn_tile_fwd(ops, q, k, v, 200, causal, None)
    b = attn_tile_fwd(ops, q, k, v, 256, causal, hide)
    same_bytes(a[0], b[0], "out")
    same_bytes(a[1], b[1], "lse")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,h,hk,S,dh", [(3, 12, 12, 37, 64), (32, 12, 4, 640, 64), (2, 8, 1, 300, 256), (1, 4, 2, 1, 16)])
def test_attention_decode(dtype, B, h, hk, S, dh):
    ops, _ = _ops()
    q = rnd(B, h, 1, dh, seed=1).to(dtype)
    kc = rnd(B, hk, S + 9, dh, seed=2).to(dtype)
    vc = rnd(B, hk, S + 9, dh, seed=3).to(dtype)
    want = O.merge_heads(O.sdpa(q.float(), O.repeat_kv(kc[:, :, :S].float(), h // hk),
                                O.repeat_kv(vc[:, :, :S].float(), h // hk), None))
    got = ops.attention_decode(q.to(DEV), kc.to(DEV), vc.to(DEV), S)
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    check(got, want, tol, tol, "decode")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rope_standalone_and_inverse(dtype):
    ops, _ = _ops()
    B, H, L, dh, pos0 = 2, 3, 19, 64, 7
    x = rnd(B, H, L, dh, seed=1).to(dtype)
    cos, sin = ops.rope_tables(dh, 64, DEV)
    fr = O.rotary_angles(dh, 64)[:, pos0:pos0 + L]
    want, _ = O.apply_rotary(x, x, fr)
    y = ops.rope_(x.to(DEV).clone(), cos, sin, pos0)
    # the standalone kernel mirrors the reference's per-op rounding
    check(y, want, 1e-6 if dtype == torch.float32 else 1e-2, 0, "rope")
    back = ops.rope_(y.clone(), cos, sin, pos0, inverse=True)
    # two roundings per direction in bf16: allow 3 ulps
    check(back, x, 1e-2 if dtype == torch.bfloat16 else 1e-6, 1.2e-2 if dtype == torch.bfloat16 else 0,
          "rope inverse round trip")


# ---- results do not depend on the environment --------------------------------------------------------------------------
# The variables that once selected a lost kernel variant or switched a timing experiment on inside a shipped kernel
# (no stores, no tile loop, no atomic epilogue: wrong results on purpose).  Nothing reads them any more.
STALE_ENV = {"VY_SKINNY_DBG": "16", "VY_ATTN_DIAG": "2", "VY_WGRAD_DIAG": "1", "VY_GEMM_VARIANT": "8", "VY_GEMM_M16": "0",
             "VY_GEMM_MID16": "0", "VY_GEMM_ROT": "1", "VY_WGRAD_M16": "0", "VY_DECODE_ROW_FINISH": "0"}


def _child_main():
    """Existing exact checks at the smallest shape that takes each launcher the variables of STALE_ENV used to reach, run as
    `python -m tests.test_kernels_gpu` in a fresh process by test_results_do_not_depend_on_the_environment (such variables
    are read once per process)."""
    from tests.test_bwd_kernels_gpu import test_wgrad_exact
    for M, N, K in ((16, 768, 768),                             # the 16-column skinny kernel
                    (128, 128, 64),                             # mid-size M
                    (4096, 3072, 264), (4096, 3071, 768)):      # the two large-M kernels
        test_linear_bf16_exact(M, N, K)
    test_attention_fwd(torch.bfloat16, ATTN_CASES[1])           # dh = 64, L = 128: the tuned MFMA forward
    test_wgrad_exact(torch.bfloat16, 256, 128, 128)
    print("child ok")


def test_results_do_not_depend_on_the_environment():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(STALE_ENV)
    r = subprocess.run([sys.executable, "-m", "tests.test_kernels_gpu"], cwd=root, env=e, timeout=300,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    _child_main()
