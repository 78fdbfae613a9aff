"""vy_lora_expand_epi and vy_cls_head_fwd / vy_cls_head_bwd on the MI355X.

vy_lora_expand_epi against the fp64 restatement of tests/lora_epi_rule.py from the same storage-dtype inputs, the bar
derived there from the rounding budget (printed by every case): T = 51 (a ragged last tile) and 16, N = 64 and 192 with
boundaries (64, 128), r_pad 32 and 64, every activation code, p in {0, 0.1, 0.5}, aliased and separate outputs, bf16 and
fp32, and the multiply mode the backward uses.  The dropped set is the mask vy_dropout exports, element for element.
The classification head against F.cross_entropy in fp64."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import lora_epi_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SHAPES = [(64, ()), (192, (64, 128))]
SEED, OFFSET = 4242, 7


def tiles_of(T):
    from vyomai_amd.lora_train import identity_tiles
    t = identity_tiles(T)
    return t.to(DEV), t.shape[0]


def mask_of(T, N, p):
    from vyomai_amd import ops
    if p == 0:
        return torch.ones(T, N, dtype=torch.bool)
    return ops.dropout(torch.ones(T, N, dtype=torch.float32, device=DEV), p, SEED, OFFSET).cpu() != 0


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("r_pad", [32, 64])
@pytest.mark.parametrize("N,bounds", SHAPES, ids=["N64", "N192"])
@pytest.mark.parametrize("T", [51, 16])
def test_expand_epi_against_the_fp64_rule(T, N, bounds, r_pad, dtype):
    from vyomai_amd import ops
    print(R.derivation(r_pad, dtype))
    alpha = 1.5
    z, u, B, other = R.make_inputs(T, N, bounds, r_pad, dtype)
    tiles, n = tiles_of(T)
    al = torch.tensor([alpha], dtype=torch.float32, device=DEV)
    zd, ud, Bd, od = z.to(DEV), u.to(DEV), B.to(DEV).unsqueeze(0).contiguous(), other.to(DEV)
    what = f"T{T} N{N} r{r_pad} {dtype}"
    worst = 0.0
    for code in R.ACT_NAMES:
        for alias in (True, False):
            zz = zd.clone()
            out = zz if alias else torch.full_like(zz, float("nan"))
            pre = torch.full_like(zz, float("nan"))
            ret = ops.lora_expand_epi_(zz, ud, Bd, al, tiles, n, bounds, act=code, pre=pre, out=None if alias else out)
            assert ret.data_ptr() == out.data_ptr()
            if not alias:
                assert torch.equal(zz, zd), "a separate output leaves z alone"
            worst = max(worst, R.check_act(code, out.cpu(), pre.cpu(), z, u, B, alpha, bounds, r_pad, dtype, what))
    for p in (0.0, 0.1, 0.5):
        keep = mask_of(T, N, p)
        if p > 0:
            assert 0 < int((~keep).sum()) < keep.numel()
        for alias in (True, False):
            zz = zd.clone()
            out = zz if alias else torch.full_like(zz, float("nan"))
            ops.lora_expand_epi_(zz, ud, Bd, al, tiles, n, bounds, residual=od, dropout=(p, SEED, OFFSET) if p else None,
                                 out=None if alias else out)
            # the dropped set is vy_dropout's, element for element: where the exported mask drops, the output is the
            # residual bit for bit; where it keeps, the output is within the budget of v * scale + res (an element the
            # kernel dropped instead would miss it by |v * scale|)
            worst = max(worst, R.check_drop_res(out.cpu(), keep, p, z, u, B, alpha, bounds, r_pad, other, dtype, what))
    print(f"{what}: worst (|got - want| - half ulp) / budget = {worst:.3f}")


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("T,N,R_", [(51, 256, 32), (16, 64, 192)])
def test_expand_epi_multiply_mode(T, N, R_, dtype):
    """The backward's twin: out = (z + alpha u @ B^T) * mul with B the transposed stacked A, r_pad := R up to 192."""
    from vyomai_amd import ops
    z, u, B, mul = R.make_inputs(T, N, (), R_, dtype, seed=3)
    tiles, n = tiles_of(T)
    al = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    zz = z.to(DEV)
    ops.lora_expand_epi_(zz, u.to(DEV), B.to(DEV).unsqueeze(0).contiguous(), al, tiles, n, mul=mul.to(DEV))
    worst = R.check_mul(zz.cpu(), z, u, B, 0.5, (), R_, mul, dtype, f"T{T} N{N} R{R_} {dtype}")
    print(f"worst ratio {worst:.3f}")


def test_expand_epi_refuses_bad_arguments():
    from vyomai_amd import ops
    z, u, B, other = (t.to(DEV) for t in R.make_inputs(16, 64, (), 32, BF))
    B = B.unsqueeze(0).contiguous()
    tiles, n = tiles_of(16)
    al = torch.ones(1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="exactly one of"):
        ops.lora_expand_epi_(z, u, B, al, tiles, n)
    with pytest.raises(ValueError, match="exactly one of"):
        ops.lora_expand_epi_(z, u, B, al, tiles, n, act=1, pre=other, residual=other)
    with pytest.raises(ValueError, match="other than ACT_NONE"):
        ops.lora_expand_epi_(z, u, B, al, tiles, n, act=0, pre=other)
    with pytest.raises(ValueError, match="writes act"):
        ops.lora_expand_epi_(z, u, B, al, tiles, n, act=1)
    with pytest.raises(ValueError, match="must not be the output"):
        ops.lora_expand_epi_(z, u, B, al, tiles, n, residual=z)
    with pytest.raises(ValueError, match=r"dropout p = 1.0"):
        ops.lora_expand_epi_(z, u, B, al, tiles, n, residual=other, dropout=(1.0, 1, 1))
    with pytest.raises(ValueError, match="share float32 or bfloat16"):
        ops.lora_expand_epi_(z, u, B, al, tiles, n, residual=other.float())
    with pytest.raises(ValueError, match="u must be"):
        ops.lora_expand_epi_(z, u[:, :16], B, al, tiles, n, residual=other)


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("code", [1, 3, 6])
def test_saved_derivative_feeds_the_existing_dgrad(code, dtype):
    """ACT mode's pre handed to linear_dgrad(pre=, act | ACT_SAVE_DERIV) is the gradient of act(z + delta):
    dX = (dY W2) * act'(v) within the rule's budget for pre, carried through the product, plus the dgrad's own fp32
    accumulation over its Nout terms, its bf16 staging of dY W in front of the factor, and one output rounding."""
    from vyomai_amd import _lib, ops
    T, N, r_pad, Nout, alpha = 51, 64, 32, 48, 1.5
    z, u, B, _ = R.make_inputs(T, N, (), r_pad, dtype, seed=5)
    g = torch.Generator().manual_seed(11)
    dy = torch.randn(T, Nout, generator=g).to(dtype)
    w2 = (torch.randn(Nout, N, generator=g) / math.sqrt(Nout)).to(dtype)
    tiles, n = tiles_of(T)
    zz, pre = z.to(DEV), torch.empty(T, N, dtype=dtype, device=DEV)
    ops.lora_expand_epi_(zz, u.to(DEV), B.to(DEV).unsqueeze(0).contiguous(),
                         torch.tensor([alpha], dtype=torch.float32, device=DEV), tiles, n, act=code, pre=pre)
    dx = ops.linear_dgrad(dy.to(DEV), w2.t().contiguous().to(DEV), pre=pre, act=code | _lib.ACT_SAVE_DERIV).cpu()
    v, dv = R.pre_sum(z, u, B, alpha, (), r_pad)
    gw = dy.double() @ w2.double()
    d_gw = (Nout + 1) * R.EPS32 * (dy.double().abs() @ w2.double().abs())
    deriv = R.act_grad64(code, v)
    lip2 = R.LIP[code][1]
    if lip2 is None:        # relu6: the stored derivative is exact on either side; compare against the stored one
        deriv = pre.cpu().double()
        d_pre = torch.zeros_like(v)
    else:
        d_pre = lip2 * dv + 32 * R.EPS32 * v.abs().clamp_min(1.0) + R.half_ulp(deriv, dtype)
    want = gw * deriv
    # vy_linear_dgrad's bf16 kernels stage the GEMM result in the storage dtype BEFORE the epilogue's factor
    # (vy_gemm.hip, gemm_epilogue: "the staged tile holds the pre-activation (bf16)"): half an ulp of dY W, times act'
    d_stage = R.half_ulp(gw, dtype) * deriv.abs() if dtype == BF else torch.zeros_like(gw)
    d = deriv.abs() * d_gw + gw.abs() * d_pre + d_stage + R.EPS32 * want.abs()
    worst = R.holds(dx, want, d, dtype, f"dgrad through saved act' ({R.ACT_NAMES[code]}, {dtype})")
    print(f"worst ratio {worst:.3f}")


# ---- the classification head -----------------------------------------------------------------------------------
def head_inputs(C, d, dtype, B=3, L=17):
    g = torch.Generator().manual_seed(100 * C + d)
    hidden = torch.randn(B, L, d, generator=g).to(dtype)
    w = (torch.randn(C, d, generator=g) / math.sqrt(d)).to(dtype)
    b = (0.1 * torch.randn(C, generator=g)).to(dtype)
    labels = torch.tensor([(7 * i + 3) % C for i in range(B)])
    return hidden, w, b, labels


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [64, 768])
@pytest.mark.parametrize("C", [1, 5, 151])
def test_cls_head_against_fp64_cross_entropy(C, d, dtype):
    from vyomai_amd import ops
    hidden, w, b, labels = head_inputs(C, d, dtype)
    B, L, _ = hidden.shape
    hd, wd, bd, ld = hidden.to(DEV), w.to(DEV), b.to(DEV), labels.to(DEV)
    h0 = hidden[:, 0, :].double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    logits64 = h0 @ w64.t() + b64
    loss64 = F.cross_entropy(logits64, labels)
    loss64.backward()
    # fp32 dot products over d terms: (d + 1) eps sum |h w|, then the softmax's few fp32 operations
    tol = (d + 2) * 2.0 ** -24 * float((h0.detach().abs() @ w64.detach().abs().t()).max()) + 1e-6
    logits = ops.cls_head_fwd(hd, wd, bd)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (B, C)
    assert float((logits.cpu().double() - logits64.detach()).abs().max()) <= tol
    runs = []
    for _ in range(2):
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        dlogits, lse, loss = ops.cls_head_fwd(hd, wd, bd, ld, err)
        dw = torch.full((C, d), float("nan"), dtype=torch.float32, device=DEV)
        db = torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)
        dh = ops.cls_head_bwd(hd, wd, dlogits, None, dw, db, False)
        assert int(err.item()) == 0
        runs.append((dlogits.cpu(), lse.cpu(), loss.cpu(), dw.cpu(), db.cpu(), dh.cpu()))
    for a, c in zip(*runs):
        assert torch.equal(a, c), "two calls give identical bits"
    dlogits, lse, loss, dw, db, dh = runs[0]
    print(f"C={C} d={d} {dtype}: loss {float(loss):.7f} fp64 {float(loss64.detach()):.7f} (logit tolerance {tol:.2e})")
    assert abs(float(loss) - float(loss64)) <= 2 * tol
    assert float((lse.double() - torch.logsumexp(logits64.detach(), dim=1)).abs().max()) <= 2 * tol
    # gradients: dlogits carries the logits' error through the softmax (|d softmax| <= |d logit|), then sums of B terms
    gtol = 4 * tol / B
    assert float((dw.double() - w64.grad).abs().max()) <= gtol * float(h0.detach().abs().max()) * B + 1e-7
    assert float((db.double() - b64.grad).abs().max()) <= gtol * B + 1e-7
    half = 2.0 ** -8 if dtype == BF else 2.0 ** -24      # the unit roundoff of the storage dtype
    want = h0.grad
    assert float((dh[:, 0, :].double() - want).abs().max()) <= gtol * float(w64.detach().abs().sum(0).max()) + half * float(want.abs().max()) + 1e-9
    assert torch.count_nonzero(dh[:, 1:, :]) == 0, "rows 1 .. L - 1 of the hidden gradient are exactly zero"
    # accumulate = 1 adds to what is there; gscale scales all three
    gs = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    dw2, db2 = dw.to(DEV).clone(), db.to(DEV).clone()
    dh2 = ops.cls_head_bwd(hd, wd, dlogits.to(DEV), gs, dw2, db2, True)
    assert torch.allclose(dw2.cpu(), 1.5 * dw, rtol=1e-6, atol=1e-9) and torch.allclose(db2.cpu(), 1.5 * db, rtol=1e-6, atol=1e-9)
    assert torch.allclose(dh2.cpu().float(), 0.5 * dh.float(), rtol=2.0 ** -7 if dtype == BF else 1e-6, atol=1e-9)


def test_cls_head_out_of_range_label_raises():
    import vyomai_amd as V
    from tests.golden import cases_encoder_lora as E
    from vyomai_amd import ops
    hidden, w, b, labels = head_inputs(5, 64, torch.float32)
    for bad_value in (5, -1, -100):
        bad = labels.clone()
        bad[1] = bad_value
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        dlogits, _, loss = ops.cls_head_fwd(hidden.to(DEV), w.to(DEV), b.to(DEV), bad.to(DEV), err)
        assert int(err.item()) == 1
        assert torch.count_nonzero(dlogits[1]) == 0 and torch.count_nonzero(dlogits[0]) > 0
        keep = torch.tensor([0, 2])     # the row is ignored, not clamped: the mean of the other two
        want = F.cross_entropy(hidden[keep, 0, :].double() @ w.double().t() + b.double(), labels[keep])
        assert abs(float(loss) - float(want)) < 1e-5
    m = V.EncoderForSequenceClassification(E.cfg("abs"), E.NUM_LABELS).to(DEV).eval()
    ids, mask, lab = (torch.from_numpy(a).to(DEV) for a in E.batch())
    m.classification_loss(ids, mask, lab, check_labels=True)
    lab[2] = E.NUM_LABELS
    with pytest.raises(ValueError, match="outside"):
        m.classification_loss(ids, mask, lab, check_labels=True)
    m.classification_loss(ids, mask, lab)                  # without the check: the flag waits
    with pytest.raises(ValueError, match="outside"):
        m.raise_on_label_error()
    m.raise_on_label_error()                               # raised once, then clean
