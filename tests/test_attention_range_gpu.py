"""vy_attn_fwd and vy_attn_bwd on scores that move the running maximum (the staircase of tests/attn_range.py), and the
bf16 backward's contract for query rows without a visible key.  Every reference is fp64 on the cast inputs; every bar is
the project's own or derived from the case's data in fp64 (never from what the kernels return); each case prints its
worst error next to the bar."""
import math

import pytest
import torch

from tests import attn_range as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = R.BF, R.F32


def _ops():
    from vyomai_amd import ops
    return ops


def _dev(t):
    return t.to(DEV) if t is not None else None


def within(got, want, bar, what, where=None):
    """|got - want| <= bar elementwise (where `where`), finite; -> the worst error / bar ratio."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - want).abs()
    bar = bar if torch.is_tensor(bar) else torch.full_like(want, bar)
    if where is not None:
        err = torch.where(where, err, torch.zeros_like(err))
    ratio = err / bar
    worst = float(ratio.max())
    print(f"  {what}: max err {float(err.max()):.3e}, worst err / bar {worst:.3f}")
    if worst > 1.0:
        idx = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())}/{ratio.numel()} outside the bar, worst err / bar {worst:.2f} at "
                             f"{idx}: got {got[idx]:.6f} want {want[idx]:.6f} bar {bar[idx]:.3e}")
    return worst


# ---- 2. forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.FWD_CASES, ids=R.case_id)
def test_attention_fwd_range(c):
    ops = _ops()
    q, k, v, keypad, addmask, mask = R.fwd_inputs(c)
    want_out, want_lse, live = R.reference_fwd(q, k, v, mask)
    out_bar, lse_bar = R.fwd_bars(c, q, k, v, addmask, want_out, want_lse)
    lse = torch.zeros(c.B, c.h, c.L, dtype=torch.float32, device=DEV)
    got = ops.attention(_dev(q), _dev(k), _dev(v), causal=c.causal, start_pos=c.start, keypad=_dev(keypad),
                        addmask=_dev(addmask), lse=lse)
    torch.cuda.synchronize()
    print(R.case_id(c))
    within(got, want_out, out_bar, "out")
    within(lse, want_lse, lse_bar, "lse (live rows)", where=live)
    if c.kp == "head" and c.causal:      # rows that see padded keys only: the column mean of V over every key
        assert not live[0, 0, :70].any() and not live[1, 0, :5].any() and live[0, 0, 70:].all()


# ---- 3. backward ---------------------------------------------------------------------------------------------------------
# B, h, hk, L, S, dh, causal, start, kp, dtype
BWD_CASES = [
    ("tuned64", 1, 2, 1, 200, 200, 64, True, 0, None, BF),
    ("tuned64", 1, 2, 2, 131, 131, 64, False, 0, None, BF),
    ("tuned64", 2, 4, 2, 40, 196, 64, True, 156, None, BF),
    ("tuned64", 2, 2, 1, 192, 192, 64, False, 0, "tail", BF),
    ("general", 1, 4, 1, 130, 130, 128, True, 0, None, BF),
    ("general", 1, 2, 1, 97, 97, 256, False, 0, None, BF),
    ("general", 1, 2, 2, 130, 130, 72, True, 0, None, BF),
    ("fp32", 1, 2, 1, 130, 130, 64, True, 0, None, F32),
    ("fp32", 1, 2, 2, 67, 67, 72, False, 0, None, F32),
]


def _bwd_id(c):
    return R.case_id(R.FwdCase(*c, 64, "stair"))


def reference_bwd(q, k, v, do, mask):
    """fp64 autograd through the reference formulation (scores + additive mask, softmax, @ v), as test_attention_bwd
    builds it.  do: (B, L, h * dh).  -> out (B, L, h * dh), dq, dk, dv, and P (B, h, L, S)."""
    h, hk, dh = q.shape[1], k.shape[1], q.shape[3]
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    s = qd @ R.rep(kd, h // hk).transpose(-1, -2) / math.sqrt(dh) + mask.double()
    p = torch.softmax(s, -1)
    o = p @ R.rep(vd, h // hk)
    out = o.permute(0, 2, 1, 3).reshape(do.shape)
    (out * do.double()).sum().backward()
    return out.detach(), qd.grad, kd.grad, vd.grad, p.detach()


def bwd_budgets(q, k, v, do, out_ref, p, grads, u):
    """The forward-error budget of dq, dk, dv in fp64, one unit roundoff u per rounding that the operands of each sum
    undergo in the kernels.  dS = P (dP - delta), delta = rowsum(dO O), A = |dS| + P sum_d |dO| |O|:
        budget(dq) = u (scale A |k| + |dq|)      dS is rounded once (bf16(P dP'), P itself stays fp32 there), O -- in delta --
                                                 is the forward's rounded output, the result is rounded once
        budget(dk) = u (scale A^T |q| + |dk|)    the same dS and delta, summed over the query heads of the KV group
        budget(dv) = u (P^T |dO| + |dv|)         P is rounded once for the dV MFMA, the result once
    Read in vy_bwd.hip: attn_bwd_dq_kernel / attn_bwd_dkdv_kernel (dh = 64) and attn_bwd_gen_dq_kernel /
    attn_bwd_gen_dkdv_kernel round exactly these (ds / dsf / sf, pf, the stores); scores, dP, lse, delta and the
    accumulators are fp32, q / k / v / dO are exact inputs.  Nothing to add to the list."""
    B, h, L, dh = q.shape
    hk, S = k.shape[1], k.shape[2]
    n = h // hk
    scale = 1.0 / math.sqrt(dh)
    dq, dk, dv = grads
    dod = do.double().view(B, L, h, dh).permute(0, 2, 1, 3)
    od = out_ref.view(B, L, h, dh).permute(0, 2, 1, 3)
    kr, vr = R.rep(k.double(), n), R.rep(v.double(), n)
    dP = dod @ vr.transpose(-1, -2)
    delta = (dod * od).sum(-1, keepdim=True)
    dS = p * (dP - delta)
    A = dS.abs() + p * (dod.abs() * od.abs()).sum(-1, keepdim=True)
    group = lambda t: t.view(B, hk, n, S, dh).sum(2)
    b_dq = u * (scale * A @ kr.abs() + dq.abs())
    b_dk = u * (scale * group(A.transpose(-1, -2) @ q.double().abs()) + dk.abs())
    b_dv = u * (group(p.transpose(-1, -2) @ dod.abs()) + dv.abs())
    return b_dq, b_dk, b_dv


def packed_grads(B, h, hk, L, S, dh, dtype):
    """dq / dk / dv as views of one packed (B, max(L, S), (h + 2 hk) dh) buffer, the layout the QKV dgrad consumes."""
    packed = torch.zeros(B, max(L, S), (h + 2 * hk) * dh, dtype=dtype, device=DEV)
    dq = packed[:, :L, : h * dh].view(B, L, h, dh).permute(0, 2, 1, 3)
    dk = packed[:, :S, h * dh:(h + hk) * dh].view(B, S, hk, dh).permute(0, 2, 1, 3)
    dv = packed[:, :S, (h + hk) * dh:].view(B, S, hk, dh).permute(0, 2, 1, 3)
    return dq, dk, dv


@pytest.mark.parametrize("case", BWD_CASES, ids=_bwd_id)
def test_attention_bwd_range(case):
    """The unit-normal bars do not transfer: k[..., 0] reaches about 18 and sum_j dS_ij = 0, so dq is a cancelling sum of
    large terms and an ideal bf16 backward sits at 0.9 - 1.2 of 4e-2 + 3e-2 |want|.  The bar per element is the larger
    of the project's bar and twice the forward-error budget above (the factor 2: fp32 accumulation order and exp2).
    Against a vacuous test: for at least 90 % of the elements of each tensor twice the budget stays below 5 % of the
    tensor's largest expected magnitude."""
    ops = _ops()
    family, B, h, hk, L, S, dh, causal, start, kp, dtype = case
    q, k, v = R.staircase(B, h, hk, L, S, dh, 64, start_pos=start, seed=23, dtype=dtype)
    do = torch.randn(B, L, h * dh, generator=torch.Generator().manual_seed(29)).to(dtype)
    keypad = R.keypad_of(kp, B, S)
    mask = R.dense_mask(B, L, S, causal, start, keypad, None)
    out_ref, *grads, p = reference_bwd(q, k, v, do, mask)
    if dtype == BF:
        u, project = 2.0 ** -8, (4e-2, 3e-2)
    else:
        u, project = 2.0 ** -24 * (dh + 2), (3e-5, 1e-4)
    budgets = bwd_budgets(q, k, v, do, out_ref, p, grads, u)
    qg, kg, vg = _dev(q), _dev(k), _dev(v)
    lse = torch.zeros(B, h, L, dtype=torch.float32, device=DEV)
    out = ops.attention(qg, kg, vg, causal=causal, start_pos=start, keypad=_dev(keypad), lse=lse)
    got = packed_grads(B, h, hk, L, S, dh, dtype)
    ops.attention_bwd(qg, kg, vg, out, _dev(do), lse, *got, causal=causal, start_pos=start, keypad=_dev(keypad))
    torch.cuda.synchronize()
    print(_bwd_id(case))
    for name, g, want, budget in zip(("dq", "dk", "dv"), got, grads, budgets):
        small = float((2 * budget < 0.05 * want.abs().max()).double().mean())
        print(f"  {name}: 2 x budget below 5 % of max|want| = {float(want.abs().max()):.3f} in {100 * small:.1f} % of the elements")
        assert small >= 0.9, f"{name}: the budget is vacuous ({100 * small:.1f} % of the elements below 5 % of the largest)"
        bar = torch.maximum(project[0] + project[1] * want.abs(), 2 * budget)
        within(g, want, bar, name)


# ---- 4. bf16 backward: rows without a visible key --------------------------------------------------------------------------
# B, h, hk, L, dh, causal, keypad of sequence 0 ("quarter": the first L // 4 keys hidden; "all"), fused rotary inverse
DEAD_CASES = [
    ("tuned64", 2, 4, 2, 100, 64, True, "quarter", False),
    ("tuned64", 2, 3, 1, 70, 64, False, "all", False),
    ("general", 2, 4, 2, 100, 128, True, "quarter", False),
    ("general", 2, 3, 1, 70, 128, False, "all", False),
    ("general", 1, 2, 2, 50, 72, False, "all", False),
    ("tuned64-rope", 2, 4, 2, 100, 64, True, "quarter", True),
]


def rope_inverse(x, cos, sin, pos0):
    """The transposed rotation of a gradient (B, heads, L, dh) in fp64: lo' = lo c + hi s, hi' = hi c - lo s."""
    L, half = x.shape[2], x.shape[3] // 2
    c, s = cos[pos0:pos0 + L].double(), sin[pos0:pos0 + L].double()
    lo, hi = x[..., :half], x[..., half:]
    return torch.cat([lo * c + hi * s, hi * c - lo * s], -1)


@pytest.mark.parametrize("case", DEAD_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}x{c[4]}x{c[5]}-{'causal' if c[6] else 'full'}-{c[7]}")
def test_attention_bwd_bf16_rows_without_a_visible_key(case):
    """The "left" construction of BWD_F32_CASES in bf16, dO non-zero everywhere.  The documented contract of the bf16
    kernels: a row without a visible key takes no part in the backward -- its dq is exactly zero and dk / dv are what
    fp64 autograd gives with dO zeroed at those rows; live rows are untouched; the forward still writes the column mean
    of V there.  (The fp32 kernels differentiate the uniform softmax instead: test_attention_bwd_fp32.)"""
    ops = _ops()
    family, B, h, hk, L, dh, causal, hide, rope = case
    S = L
    q, k, v = R.normal(B, h, hk, L, S, dh, seed=31, dtype=BF)
    do = torch.randn(B, L, h * dh, generator=torch.Generator().manual_seed(37)).to(BF)
    assert (do != 0).all()
    keypad = torch.ones(B, S, dtype=torch.uint8)
    keypad[0, : S // 4] = 0
    if hide == "all":
        keypad[0, :] = 0
    mask = R.dense_mask(B, L, S, causal, 0, keypad, None)
    live = (mask > R.FMIN / 2).any(-1).expand(B, h, L)                  # (B, h, L)
    dead = ~live
    assert dead.any() and (hide == "all" or live[0].any())
    do_live = torch.where(live.permute(0, 2, 1)[..., None], do.view(B, L, h, dh), torch.zeros((), dtype=BF)).reshape(B, L, h * dh)
    out_ref, dq_ref, dk_ref, dv_ref, _ = reference_bwd(q, k, v, do_live, mask)
    qg, kg, vg, kpg = _dev(q), _dev(k), _dev(v), _dev(keypad)
    lse = torch.zeros(B, h, L, dtype=torch.float32, device=DEV)
    out = ops.attention(qg, kg, vg, causal=causal, keypad=kpg, lse=lse)
    dq, dk, dv = packed_grads(B, h, hk, L, S, dh, BF)
    kw = {}
    if rope:
        cos, sin = ops.rope_tables(dh, 128, DEV)
        kw = dict(cos=cos, sin=sin, rope_pos0=3)
        dq_ref, dk_ref = rope_inverse(dq_ref, cos.cpu(), sin.cpu(), 3), rope_inverse(dk_ref, cos.cpu(), sin.cpu(), 3)
    ops.attention_bwd(qg, kg, vg, out, _dev(do), lse, dq, dk, dv, causal=causal, keypad=kpg, **kw)
    torch.cuda.synchronize()
    print(case)
    # the forward: the column mean of V at dead rows (the reference's uniform softmax), the usual bars everywhere
    within(out, out_ref, 2e-2 + 2e-2 * out_ref.abs(), "fwd out")
    vmean = R.rep(v.double(), h // hk).mean(2, keepdim=True).expand(B, h, L, dh).permute(0, 2, 1, 3).reshape(B, L, h * dh)
    dead_o = dead.permute(0, 2, 1)[..., None].expand(B, L, h, dh).reshape(B, L, h * dh)
    within(out, vmean, 2e-2 + 2e-2 * vmean.abs(), "fwd out at dead rows vs the column mean of V", where=dead_o)
    dqc = dq.float().cpu()
    assert torch.isfinite(dqc).all()
    nz = (dqc != 0) & dead[..., None]
    assert not nz.any(), f"dq of a row without a visible key: {int(nz.sum())} non-zero elements, first at {nz.nonzero()[0].tolist()}"
    bar = lambda want: 4e-2 + 3e-2 * want.abs()
    within(dq, dq_ref, bar(dq_ref), "dq (live rows: the plain reference; dead rows: 0)")
    within(dk, dk_ref, bar(dk_ref), "dk vs autograd with dO zeroed at the dead rows")
    within(dv, dv_ref, bar(dv_ref), "dv vs autograd with dO zeroed at the dead rows")
