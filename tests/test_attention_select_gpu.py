"""vy_attn_fwd and vy_attn_bwd on selector inputs (tests/attn_select.py): every row one-hot at its last or first visible
key, or two-hot at chosen keys, next to unit-normal data; every bar derived in fp64 from the case's data and the roundings
the kernels perform, never from what they return.  Each case prints its worst err / bar per tensor.  The guard that these
inputs and bars catch a mask edge, a key, a KV head, a V block or a dk / dv row that is one off is
tests/test_attention_select_cpu.py."""
import pytest
import torch

from tests import attn_select as A

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vyomai_amd import ops
    return ops


def _dev(t):
    return t.to(DEV) if t is not None else None


def within(got, want, bar, what, where=None):
    """|got - want| <= bar elementwise (where `where`), finite; -> the worst err / bar."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    ratio = A.ratios(got, want, bar, where)
    worst = float(ratio.max())
    print(f"  {what}: max err {float((got - want).abs().max()):.3e}, worst err / bar {worst:.3f}")
    if worst > 1.0:
        idx = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())}/{ratio.numel()} outside the bar, worst err / bar {worst:.2f} at "
                             f"{idx}: got {got[idx]:.6f} want {want[idx]:.6f} bar {bar[idx]:.3e}")
    return worst


def forward(ops, f):
    c = f.c
    lse = torch.zeros(c.B, c.h, c.L, dtype=torch.float32, device=DEV)
    out = ops.attention(_dev(f.q), _dev(f.k), _dev(f.v), causal=c.causal, start_pos=c.start, keypad=_dev(f.keypad), lse=lse)
    return out, lse


@pytest.mark.parametrize("cr", A.case_regimes(A.FWD_CASES), ids=A.cr_id)
def test_attention_fwd_select(cr):
    c, regime = cr
    f = A.forward_problem(c, regime)
    out, lse = forward(_ops(), f)
    torch.cuda.synchronize()
    print(A.cr_id(cr))
    within(out, f.want_out, f.out_bar, "out")
    within(lse, f.want_lse, f.lse_bar, "lse (live rows)", where=f.live)


def packed_grads(c, fill=A.SENTINEL):
    """dq / dk / dv as views of one packed (B, max(L, S), (h + 2 hk) dh) buffer, the layout the QKV dgrad consumes, filled
    with a sentinel; `outside`: what belongs to none of the three views."""
    packed = torch.full((c.B, max(c.L, c.S), (c.h + 2 * c.hk) * c.dh), fill, dtype=c.dtype, device=DEV)
    outside = torch.ones(packed.shape, dtype=torch.bool, device=DEV)
    outside[:, :c.L, : c.h * c.dh] = False
    outside[:, :c.S, c.h * c.dh:] = False
    dq = packed[:, :c.L, : c.h * c.dh].view(c.B, c.L, c.h, c.dh).permute(0, 2, 1, 3)
    dk = packed[:, :c.S, c.h * c.dh:(c.h + c.hk) * c.dh].view(c.B, c.S, c.hk, c.dh).permute(0, 2, 1, 3)
    dv = packed[:, :c.S, (c.h + c.hk) * c.dh:].view(c.B, c.S, c.hk, c.dh).permute(0, 2, 1, 3)
    return packed, outside, dq, dk, dv


def backward(ops, f, **rope):
    c = f.c
    out, lse = forward(ops, f)
    packed, outside, dq, dk, dv = packed_grads(c)
    ops.attention_bwd(_dev(f.q), _dev(f.k), _dev(f.v), out, _dev(f.do), lse, dq, dk, dv, causal=c.causal, start_pos=c.start,
                      keypad=_dev(f.keypad), **rope)
    torch.cuda.synchronize()
    touched = outside & (packed != A.SENTINEL)
    assert not touched.any(), (f"{int(touched.sum())} elements outside dq / dk / dv were written, first at "
                               f"{touched.nonzero()[0].tolist()} of the packed {tuple(packed.shape)} buffer")
    if c.L < c.S:
        assert outside[:, c.L:, : c.h * c.dh].all()      # rows >= L of the dq columns belong to nobody
    return dq, dk, dv


@pytest.mark.parametrize("cr", A.case_regimes(A.BWD_CASES), ids=A.cr_id)
def test_attention_bwd_select(cr):
    """The gradients go into the packed buffer, pre-filled with a sentinel: everything outside the three views, the rows
    >= L of the dq columns included, still holds it afterwards.  bf16: dO is non-zero at rows without a visible key too
    and the reference has it zeroed there (the kernels' contract, tests/test_attention_range_gpu.py)."""
    c, regime = cr
    f = A.backward_problem(c, regime)
    got = backward(_ops(), f)
    print(A.cr_id(cr))
    for name, g, want, bar in zip(("dq", "dk", "dv"), got, f.grads, f.bars):
        if name in A.SHARP[regime]:
            share = A.sharp_share(bar, want)
            print(f"  {name}: bar below 5 % of max|want| = {float(want.abs().max()):.3f} in {100 * share:.1f} % of the elements")
            assert share >= 0.9, f"{name}: the bar is vacuous ({100 * share:.1f} % of the elements below 5 % of the largest)"
        within(g, want, bar, name)


@pytest.mark.parametrize("c", A.ROPE_CASES, ids=A.case_id)
def test_attention_bwd_select_rope_inverse(c):
    """The `pair` regime with the rotary inverse inside vy_attn_bwd, against rope_inverse of the fp64 gradients."""
    ops = _ops()
    f = A.backward_problem(c, "pair")
    cos, sin = ops.rope_tables(c.dh, 192, DEV)
    dq, dk, dv = backward(ops, f, cos=cos, sin=sin, rope_pos0=3)
    cos, sin = cos.cpu(), sin.cpu()
    wants = [A.rope_inverse(w, cos, sin, 3) for w in f.grads[:2]]
    bars = A.rope_bars(c, f.bars[:2], f.grads[:2], wants, cos, sin, 3)
    print(A.case_id(c) + "-pair-rope")
    within(dq, wants[0], bars[0], "dq")
    within(dk, wants[1], bars[1], "dk")
    within(dv, f.grads[2], f.bars[2], "dv")
