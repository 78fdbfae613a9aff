"""Guard of the staircase generator (tests/attn_range.py): a torch emulation of a tile-wise online softmax -- `period`-key
steps, the lazy threshold of attn_fwd_mfma_kernel, one `any` per 32 query rows, bf16 P, fp32 elsewhere -- with three
faults that can be switched in.  On the staircase the faithful emulation meets the bars of the GPU test and every fault
breaks them; on unit-normal data the faults go unnoticed, which is why the regime exists.  No kernel runs here."""
import math

import pytest
import torch

from tests import attn_range as R
from tests.test_kernels_gpu import ATTN_CASES, rnd

LN2 = math.log(2.0)
FAULTS = ("no_rescale", "alpha_zero", "o_not_l")


def emulate(q, k, v, mask, period, lazy=8.0, group=32, p_dtype=R.BF, fault=None):
    """Online softmax over steps of `period` keys.  lazy: the running maximum moves only where some row of a group of
    `group` consecutive query rows has a step maximum above m + lazy (log2 units), as vy_attn.hip does; None: every row
    follows its own maximum at every step (AttnGen::step, the row-wise kernel).  fault, applied from the second step on
    wherever a rescale happens: "no_rescale" (m moves, O and l keep their old scale), "alpha_zero" (alpha = 0),
    "o_not_l" (O rescaled, l not).
    -> out (B, L, h * dh), lse (B, h, L), the number of steps after the first in which a row with l > 0 was rescaled,
    per (batch, head)."""
    B, h, L, dh = q.shape
    S, n = k.shape[2], h // k.shape[1]
    qf, kf, vf = q.float(), R.rep(k.float(), n), R.rep(v.float(), n)
    vis = (mask > R.FMIN / 2).expand(B, 1, L, S)
    add = torch.where(vis, mask.expand(B, 1, L, S), torch.zeros(()))
    m = torch.full((B, h, L), R.FMIN)
    l = torch.zeros(B, h, L)
    o = torch.zeros(B, h, L, dh)
    rescales = torch.zeros(B, h, dtype=torch.long)
    ninf = torch.tensor(float("-inf"))
    for t, k0 in enumerate(range(0, S, period)):
        k1 = min(S, k0 + period)
        s = (qf @ kf[:, :, k0:k1].transpose(-1, -2)) * (1.0 / math.sqrt(dh)) + add[..., k0:k1]
        s = torch.where(vis[..., k0:k1], s, ninf)
        tmax = s.max(-1).values
        if lazy is None:
            fire = tmax > m
        else:
            over = tmax > m + lazy * LN2
            Lp = (L + group - 1) // group * group
            over = torch.nn.functional.pad(over, (0, Lp - L))
            fire = over.view(B, h, Lp // group, group).any(-1, keepdim=True).expand(B, h, Lp // group, group)
            fire = fire.reshape(B, h, Lp)[..., :L]
        m_new = torch.where(fire, torch.maximum(m, tmax), m)
        alpha = torch.exp(m - m_new)
        a_o, a_l = alpha, alpha
        if t > 0:
            rescales += (fire & (l > 0) & (m_new > m)).any(-1).long()
            one = torch.ones(())
            if fault == "no_rescale":
                a_o = a_l = torch.where(fire, one, alpha)
            elif fault == "alpha_zero":
                a_o = a_l = torch.where(fire, torch.zeros(()), alpha)
            elif fault == "o_not_l":
                a_l = torch.where(fire, one, alpha)
        m = m_new
        p = torch.exp(s - m[..., None])
        l = l * a_l + p.sum(-1)
        pv = p if p_dtype is None else p.to(p_dtype).float()
        o = o * a_o[..., None] + pv @ vf[:, :, k0:k1]
    dead = l == 0
    o = torch.where(dead[..., None], vf.sum(2, keepdim=True).expand_as(o), o)
    l = torch.where(dead, torch.full_like(l, float(S)), l)
    out = (o / l[..., None]).permute(0, 2, 1, 3).reshape(B, L, h * dh)
    return out, m + torch.log(l), rescales


def emu_args(c):
    if c.dtype == R.F32 or c.family == "rowwise":
        return dict(lazy=None, p_dtype=None)
    if c.dh in (64, 128):
        return dict(lazy=8.0, group=32, p_dtype=R.BF)
    return dict(lazy=None, p_dtype=R.BF)


def outside(out, lse, want_out, want_lse, live, bars):
    """-> fraction of out elements outside the bar, whether lse (live rows) is inside, max |out error|."""
    err = (out.double() - want_out).abs()
    lerr = torch.where(live, (lse.double() - want_lse).abs(), torch.zeros((), dtype=torch.float64))
    lse_ok = bool((lerr <= torch.where(live, bars[1], torch.ones((), dtype=torch.float64))).all())
    return float((err > bars[0]).double().mean()), lse_ok, float(err.max())


@pytest.mark.parametrize("c", R.FWD_CASES, ids=R.case_id)
def test_emulation_on_the_forward_cases(c):
    q, k, v, keypad, addmask, mask = R.fwd_inputs(c)
    want_out, want_lse, live = R.reference_fwd(q, k, v, mask)
    bars = R.fwd_bars(c, q, k, v, addmask, want_out, want_lse)
    kw = emu_args(c)
    out, lse, rescales = emulate(q, k, v, mask, c.period, **kw)
    frac, lse_ok, worst = outside(out, lse, want_out, want_lse, live, bars)
    print(f"{R.case_id(c)}: faithful max err {worst:.3e}, rescales after step 0 per (b, h): {rescales.flatten().tolist()}")
    assert frac == 0.0 and lse_ok, f"the faithful emulation misses the bars: {frac:.4f} of out outside, max err {worst:.3e}"
    if c.data != "stair":
        return      # descending / unit-normal / additive: the faithful emulation only
    assert (rescales >= 1).all(), f"no rescale after the first step in some (batch, head): {rescales.tolist()}"
    for fault in FAULTS:
        out, lse, _ = emulate(q, k, v, mask, c.period, fault=fault, **kw)
        frac, _, worst = outside(out, lse, want_out, want_lse, live, bars)
        print(f"  {fault}: {100 * frac:.1f} % of out outside the bars, max err {worst:.3e}")
        assert frac >= 0.01, f"{fault} goes unnoticed: only {100 * frac:.2f} % of out outside the bars"


def test_faults_pass_on_unit_normal_data():
    """ATTN_CASES[0] of tests/test_kernels_gpu.py with its own data: the lazy rescale runs on the first step only, so the
    three faults change nothing and the existing bars hold."""
    B, h, hk, L, S, dh, causal, start, _, _ = ATTN_CASES[0]
    q, k, v = (rnd(B, n, T, dh, seed=sd).to(R.BF) for n, T, sd in ((h, L, 1), (hk, S, 2), (hk, S, 3)))
    mask = R.dense_mask(B, L, S, causal, start, None, None)
    want_out, want_lse, live = R.reference_fwd(q, k, v, mask)
    bars = (2e-2 + 2e-2 * want_out.abs(), 2e-2 + 1e-4 * want_lse.abs())
    for fault in (None,) + FAULTS:
        out, lse, rescales = emulate(q, k, v, mask, 64, fault=fault)
        frac, lse_ok, worst = outside(out, lse, want_out, want_lse, live, bars)
        print(f"{fault}: max err {worst:.3e}, rescales after step 0: {int(rescales.sum())}")
        assert frac == 0.0 and lse_ok, fault
        assert int(rescales.sum()) == 0
