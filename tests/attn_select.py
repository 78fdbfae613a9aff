"""Attention inputs on which every key position matters ("selector" inputs), the case tables of the dense kernels and
bars derived from the rounding budget.

Unit-normal softmax is close to an average over the keys: an index that is off by one among 200 keys, a V block permuted
against its K block, a dk / dv row stored one row off or a mask edge that is one key too generous all hide under
2e-2 + 2e-2 |want| (forward) and 4e-2 + 3e-2 |want| (backward).  Two remedies, used together:

  regimes  "ramp" / "ramp_desc": every row is one-hot at its last / first visible key, so a key that is wrongly visible
           takes the row over and a key that is wrongly hidden hands it to its neighbour (out, lse, dv);
           "pair": every row is two-hot at chosen keys, so dS is non-zero at known places (dq, dk);
           "normal": unit-normal data, for the bars.
  bars     per element, in fp64 from the case's data: one unit roundoff per rounding that the kernels perform on the
           operands of each sum, times 2 (fp32 accumulation order, exp2) -- never from what a kernel returns.

Shared by tests/test_attention_select_cpu.py (the guard: torch emulations with faults switched in, no kernel) and
tests/test_attention_select_gpu.py.  No GPU at import.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from tests import attn_range as R
from tests.test_attention_range_gpu import bwd_budgets, reference_bwd, rope_inverse   # noqa: F401  (no GPU at import)

BF, F32, FMIN = R.BF, R.F32, R.FMIN
U_BF16 = 2.0 ** -8
F32_EPS = 2.0 ** -24
SENTINEL = -1984.0          # -31 * 64: exact in bf16, far from every expected gradient

Case = namedtuple("Case", "family B h hk L S dh causal start kp dtype")


def _c(family, B, h, hk, L, S, dh, causal, start=0, kp=None, dtype=BF):
    return Case(family, B, h, hk, L, S, dh, causal, start, kp, dtype)


# the smallest sizes that reach every path: ragged last tiles, more than one 64-key tile and 128-row query block, GQA and
# MQA, start_pos, every key-padding kind, every head width with a kernel of its own
FWD_CASES = [
    _c("tuned64", 2, 4, 2, 200, 200, 64, True),
    _c("tuned64", 2, 4, 2, 40, 100, 64, True, 60, "tail"),
    _c("tuned64", 1, 2, 2, 131, 131, 64, False, 0, "hole"),
    _c("tuned64", 1, 2, 1, 257, 257, 64, True),
    _c("tuned128", 1, 4, 2, 150, 150, 128, True),
    _c("tuned128", 2, 2, 2, 70, 70, 128, False, 0, "head"),
    _c("general", 2, 4, 2, 130, 130, 72, True, 0, "tail"),
    _c("general", 2, 3, 3, 100, 100, 96, False, 0, "hole"),
    _c("general", 1, 2, 2, 130, 130, 160, True),
    _c("general", 1, 8, 1, 264, 264, 256, True),
    _c("general", 2, 8, 1, 70, 110, 256, True, 40, "head"),
    _c("general", 1, 2, 2, 64, 64, 40, False),
    _c("rowwise", 2, 4, 2, 17, 17, 16, True, 0, "tail"),
    _c("rowwise", 2, 4, 2, 17, 17, 16, True, 0, "tail", F32),
    _c("rowwise", 1, 2, 1, 130, 130, 64, True, 0, None, F32),
    _c("rowwise", 1, 2, 2, 67, 67, 72, False, 0, "hole", F32),
]

# what vy_attn_bwd serves of the table: the tuned dh = 64 kernels, the general bf16 kernels (dh = 128 included) and the
# plain fp32 kernels
BWD_CASES = [c for c in FWD_CASES if c.family == "tuned64"] + [
    c._replace(family="general") for c in FWD_CASES
    if c.dtype == BF and c.dh in (128, 72, 96, 256, 40)] + [
    c._replace(family="fp32") for c in FWD_CASES if c.dtype == F32 and c.dh != 16]

ROPE_CASES = [FWD_CASES[1], FWD_CASES[4]._replace(family="general")]     # fused into the dh = 64 epilogues / launched after


def case_id(c):
    return (f"{c.family}-{c.B}x{c.h}x{c.hk}x{c.L}x{c.S}x{c.dh}-{'causal' if c.causal else 'full'}"
            f"{'-start%d' % c.start if c.start else ''}{'-' + c.kp if c.kp else ''}-{'bf16' if c.dtype == BF else 'fp32'}")


def regimes_of(c):
    """ramp_desc (one-hot at the FIRST visible key) where leading keys are hidden."""
    return ("normal", "pair", "ramp") + (("ramp_desc",) if c.kp == "head" else ())


def case_regimes(cases):
    return [(c, r) for c in cases for r in regimes_of(c)]


def cr_id(cr):
    return f"{case_id(cr[0])}-{cr[1]}"


# the tensors that a regime is meant to test: there 2 x budget must be a sharp bar (the range test's condition)
SHARP = {"normal": ("dq", "dk", "dv"), "pair": ("dq", "dk", "dv"), "ramp": ("dv",), "ramp_desc": ("dv",)}


def sharp_share(bar, want):
    """The share of the elements whose bar is below 5 % of the tensor's largest expected magnitude."""
    return float((bar < 0.05 * want.abs().max()).double().mean())


# ---- masks -----------------------------------------------------------------------------------------------------------------
def keypad_of(kind, B, S):
    """"tail" / "head": those of attn_range.keypad_of (written for S = 192 and S = 150), scaled to S.  "hole": three
    interior keys hidden, one of them the last key of the first 64-key tile."""
    if kind is None:
        return None
    kp = torch.ones(B, S, dtype=torch.uint8)
    for b in range(B):
        if kind == "tail":
            kp[b, ((130, 66)[b % 2] * S) // 192:] = 0
        elif kind == "head":
            kp[b, : max(1, ((70, 5)[b % 2] * S) // 150)] = 0
        elif kind == "hole":
            kp[b, [63, S // 3 + b, 2 * S // 3 + 1 + 2 * b]] = 0
        else:
            raise ValueError(kind)
    return kp


def visible(c, keypad, diag=0, drop_last=False):
    """(B, L, S) bool.  diag: the causal edge moved by that many keys; drop_last: key S - 1 hidden (the guard's faults)."""
    vis = torch.ones(c.B, c.L, c.S, dtype=torch.bool)
    if c.causal:
        vis &= (torch.arange(c.S)[None, :] <= torch.arange(c.L)[:, None] + c.start + diag)[None]
    if keypad is not None:
        vis &= keypad.bool()[:, None, :]
    if drop_last:
        vis[..., c.S - 1] = False
    return vis


# ---- the regimes -----------------------------------------------------------------------------------------------------------
RAMP_G = 128.0


def ramp(c, seed, descending=False):
    """q, k unit-normal but for two components: k[..., 0] = j // 16, k[..., 1] = j % 16, q[..., 0] = 16 g, q[..., 1] = g.
    Every value is exact in bf16 and the raw score gains exactly g j: at least 8 nat a key at dh = 256."""
    q, k, v = R.normal(c.B, c.h, c.hk, c.L, c.S, c.dh, seed=seed)
    j = torch.arange(c.S)
    if descending:
        j = c.S - 1 - j
    k[..., 0] = (j // 16).float()
    k[..., 1] = (j % 16).float()
    q[..., 0] = 16 * RAMP_G
    q[..., 1] = RAMP_G
    return q, k, v


def pair_width(c):
    return 4 if c.dh < 40 else 13       # 13 keeps partners from aligning with the 16- and 64-key blocks


def pair_amp(dh):
    return 2.0 ** math.ceil(math.log2(12 * math.sqrt(dh)))


def pair_targets(c, vis, seed):
    """-> a, b (B, h, L) long, -1: none.  Even heads: a = the last visible key of the row; odd heads: a seeded random
    visible key.  b: a seeded random visible key with b % W == a % W, b != a."""
    W = pair_width(c)
    rng = np.random.RandomState(seed)
    a = torch.full((c.B, c.h, c.L), -1, dtype=torch.long)
    b = a.clone()
    visn = vis.numpy()
    for bi in range(c.B):
        for i in range(c.L):
            cand = np.flatnonzero(visn[bi, i])
            if cand.size == 0:
                continue
            for hd in range(c.h):
                aa = cand[-1] if hd % 2 == 0 else cand[rng.randint(cand.size)]
                mates = cand[(cand % W == aa % W) & (cand != aa)]
                a[bi, hd, i] = int(aa)
                if mates.size:
                    b[bi, hd, i] = int(mates[rng.randint(mates.size)])
    return a, b


def pair(c, vis, seed):
    """Key j carries a product code: a one in component j // W and a one in component nh + j % W.  The query adds amp at
    the code components of its targets a and b (which share j % W): both score exactly 3 amp -- sums of small integers,
    whatever the order -- and every other key at most 2 amp, at least 12 nat lower.  The spare components: k unit-normal
    and q zero in the first half, q unit-normal and k zero in the second, so every column of dq and of dk carries
    something and no score moves."""
    W = pair_width(c)
    nh = -(-c.S // W)
    c0 = nh + W
    assert c0 <= c.dh - 2, (c, c0)
    half = c0 + (c.dh - c0) // 2
    amp = pair_amp(c.dh)
    qn, kn, v = R.normal(c.B, c.h, c.hk, c.L, c.S, c.dh, seed=seed)
    q, k = torch.zeros_like(qn), torch.zeros_like(kn)
    k[..., c0:half] = kn[..., c0:half]
    q[..., half:] = qn[..., half:]
    j = torch.arange(c.S)
    k[:, :, j, j // W] = 1.0
    k[:, :, j, nh + j % W] = 1.0
    a, b = pair_targets(c, vis, seed + 1)
    code = torch.zeros(c.B, c.h, c.L, c0)
    for t in (a, b):
        on = (t >= 0).float()
        tc = t.clamp_min(0)
        code.scatter_add_(-1, (tc // W)[..., None], (amp * on)[..., None])
        code.scatter_add_(-1, (nh + tc % W)[..., None], (amp * on)[..., None])
    q[..., :c0] = code
    return q, k, v, a, b


SEEDS = {"normal": 41, "pair": 43, "ramp": 47, "ramp_desc": 53}


def inputs(c, regime):
    """-> q (B, h, L, dh), k, v (B, hk, S, dh), dO (B, L, h dh), all cast to the storage type; keypad or None; targets."""
    keypad = keypad_of(c.kp, c.B, c.S)
    seed = SEEDS[regime]
    targets = None
    if regime == "normal":
        q, k, v = R.normal(c.B, c.h, c.hk, c.L, c.S, c.dh, seed=seed)
    elif regime == "pair":
        q, k, v, *targets = pair(c, visible(c, keypad), seed)
    else:
        q, k, v = ramp(c, seed, descending=regime == "ramp_desc")
    do = torch.randn(c.B, c.L, c.h * c.dh, generator=torch.Generator().manual_seed(seed + 100)).to(c.dtype)
    assert (do != 0).all()
    exact = {"normal": 0, "pair": -(-c.S // pair_width(c)) + pair_width(c)}.get(regime, 2)
    for t in (q, k):                # the selecting components survive the cast to the storage type unchanged
        assert torch.equal(t.to(c.dtype)[..., :exact].float(), t[..., :exact])
    return q.to(c.dtype), k.to(c.dtype), v.to(c.dtype), do, keypad, targets


# ---- bars ------------------------------------------------------------------------------------------------------------------
def merge(x):
    """(B, h, L, dh) -> (B, L, h dh)"""
    B, h, L, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, L, h * dh)


def score_delta(c, q, k):
    """(B, h, L, S): what an fp32 dot product of dh exact products, the scale and the mask select can be off by, per
    score: (dh + 2) 2^-24 scale sum_d |q_id k_jd| (attn_range.fwd_bars uses its maximum)."""
    absdot = q.double().abs() @ R.rep(k.double().abs(), c.h // c.hk).transpose(-1, -2)
    return (c.dh + 2) * F32_EPS / math.sqrt(c.dh) * absdot


def fwd_bars(c, q, k, v, p, want_out, want_lse):
    """-> the bar on out (B, L, h dh) and on lse (B, h, L, live rows).
    bf16 out: 2 u (sum_j P_ij |v_j| + |out|), u = 2^-8 -- P is rounded once for the PV MFMA and the result once; scores,
    maximum, sum and accumulators are fp32 (vy_attn.hip:197-233, AttnGen::step; the lazy rescale keeps p <= 2^8, still a
    relative rounding) -- plus the fp32 score term of attn_range.fwd_bars, delta 2 sum_j P_ij |v_j|.
    fp32 out: attn_range.fwd_bars.  lse (fp32 in both): 1e-4 + 1e-4 |want| + delta."""
    delta = float(score_delta(c, q, k).max())
    lse_bar = 1e-4 + 1e-4 * want_lse.abs() + delta
    if c.dtype != BF:
        out_bar, lse_bar32 = R.fwd_bars(c, q, k, v, None, want_out, want_lse)
        assert torch.allclose(lse_bar, lse_bar32, rtol=1e-12, atol=0)
        return out_bar, lse_bar
    pv = merge(p @ R.rep(v.double().abs(), c.h // c.hk))
    return 2 * U_BF16 * (pv + want_out.abs()) + delta * 2 * pv, lse_bar


def bwd_bars(c, q, k, v, do, out_ref, p, want_lse, grads, mask, live):
    """-> the bars on dq, dk, dv.  bf16: 2 x bwd_budgets with u = 2^-8, no project floor under it.  fp32: the larger of
    the project's 3e-5 + 1e-4 |want| and 2 x (bwd_budgets with u = 2^-24 (dh + 2), plus a score term).  Both: plus
    underflow_terms.
    The score term, fp32 only: bwd_budgets charges one relative u per operand, which covers scores of a few nat; the
    ramp's reach 2000, and the error of a score enters P = exp(scale s - lse) absolutely.  The backward recomputes s
    (attn_bwd_f32_dq_kernel / attn_bwd_f32_dkdv_kernel, vy_bwd.hip:1634-1644: dh fmaf in fp32) and subtracts the
    forward's lse (attn_rowwise_kernel of vy_attn.hip: its own fp32 dot products in another order, m + log l stored as
    fp32).  To first order P is off by the factor 1 + eps_ij,
        eps_ij = delta_ij + sum_j P_ij delta_ij + 2 2^-24 |lse_i|      (delta_ij: score_delta)
    and so is dS = P (dP - delta):  budget(dv) += (P eps)^T |dO|,  budget(dq) += scale (eps |dS|) |k|,
    budget(dk) += scale (eps |dS|)^T |q|.  Without the term the guard's fp32 emulation, whose forward and
    backward even share one score matrix, sits at 0.66 of the dk bar on the ramp of (1, 2, 2, 67, 67, 72), and the
    kernels, whose forward and backward do not, err by 3.0e-3 on dv on the ramp of (1, 2, 1, 130, 130, 64) where the bar
    is at most 3e-5 + 1e-4 * 6.1.  With it the emulation and the kernels sit at 0.06 or less and every fault of the guard
    still lands at 700 or more in some regime: on the ramp fp32 pins positions, not digits."""
    vis = (mask > FMIN / 2).expand(c.B, 1, c.L, c.S) & live[..., None]
    flush = underflow_terms(c, q, k, v, do, out_ref, vis)
    if c.dtype == BF:
        return tuple(2 * (b + f) for b, f in zip(bwd_budgets(q, k, v, do, out_ref, p, grads, U_BF16), flush))
    budgets = bwd_budgets(q, k, v, do, out_ref, p, grads, F32_EPS * (c.dh + 2))
    B, h, L, dh = q.shape
    hk, S = k.shape[1], k.shape[2]
    n = h // hk
    scale = 1.0 / math.sqrt(dh)
    d = score_delta(c, q, k)
    eps = d + (p * d).sum(-1, keepdim=True) + 2 * F32_EPS * want_lse.abs()[..., None]
    dod, od = merge_inv(do.double(), h), merge_inv(out_ref, h)
    dP = dod @ R.rep(v.double(), n).transpose(-1, -2)
    E = eps * (p * (dP - (dod * od).sum(-1, keepdim=True))).abs()
    group = lambda t: t.view(B, hk, n, S, dh).sum(2)
    extra = (scale * E @ R.rep(k.double().abs(), n),
             scale * group(E.transpose(-1, -2) @ q.double().abs()),
             group((p * eps).transpose(-1, -2) @ dod.abs()))
    return tuple(torch.maximum(3e-5 + 1e-4 * w.abs(), 2 * (b + e + f)) for w, b, e, f in zip(grads, budgets, extra, flush))


def underflow_terms(c, q, k, v, do, out_ref, vis):
    """Absolute terms that a relative budget lacks: where a row is one-hot the other keys' P = exp2(c s - lse log2 e) lie
    below fp32's smallest normal number eta = 2^-126, and the raw exp2 instruction returns 0 for them
    (__builtin_amdgcn_exp2f, vy_bwd.hip:1310,1424; no fp32 or bf16 store keeps a denormal either): every P and every
    dS = P (dP - delta) of a visible (i, j) is off by up to eta more, every stored result by up to eta.  1e-38 against
    gradients of order 1: the terms only keep 0 from being the one value inside the bar.  Hidden keys and rows without
    a visible key add nothing: their P is an exact 0 by select."""
    eta = 2.0 ** -126
    B, h, L, dh = q.shape
    hk, S = k.shape[1], k.shape[2]
    n = h // hk
    scale = 1.0 / math.sqrt(dh)
    dod, od = merge_inv(do.double(), h), merge_inv(out_ref, h)
    visd = vis.expand(B, h, L, S).double()
    D = visd * ((dod @ R.rep(v.double(), n).transpose(-1, -2) - (dod * od).sum(-1, keepdim=True)).abs() + 1)
    group = lambda t: t.view(B, hk, n, S, dh).sum(2)
    any_q = visd.amax(-1, keepdim=True)                                    # (B, h, L, 1)
    any_k = group(visd.amax(-2)[..., None].expand(B, h, S, dh)).clamp_max(1)  # (B, hk, S, dh)
    return (eta * (scale * D @ R.rep(k.double().abs(), n) + any_q),
            eta * (scale * group(D.transpose(-1, -2) @ q.double().abs()) + any_k),
            eta * (group(visd.transpose(-1, -2) @ dod.abs()) + any_k))


def merge_inv(x, h):
    """(B, L, h dh) -> (B, h, L, dh)"""
    B, L, hd = x.shape
    return x.view(B, L, h, hd // h).permute(0, 2, 1, 3)


def rope_bars(c, bars, wants, wants_rot, cos, sin, pos0):
    """The bars on dq, dk after the rotary inverse lo' = lo c + hi s, hi' = hi c - lo s (fp32 tables, fp32 arithmetic).
    dh = 64: the rotation is fused into the epilogues (attn_store_scaled_rope, vy_attn_tile.h:202-216), it acts on the
    fp32 accumulators and the result is rounded once -- the budget before the store rounding, u |want|, rotated, plus
    u |rotated|.  Otherwise vy_rope_fwd runs after the kernels (vy_bwd.hip:1730-1734) on the stored bf16 gradients and
    rounds once more -- the whole budget rotated, plus u |rotated|.  (The bars are 2 x budget.)"""
    out = []
    for bar, want, rot in zip(bars, wants, wants_rot):
        if c.dh == 64:
            bar = (bar - 2 * U_BF16 * want.abs()).clamp_min(0)
        L, half = bar.shape[2], bar.shape[3] // 2
        cc, ss = cos[pos0:pos0 + L].double().abs(), sin[pos0:pos0 + L].double().abs()
        lo, hi = bar[..., :half], bar[..., half:]
        out.append(torch.cat([lo * cc + hi * ss, hi * cc + lo * ss], -1) + 2 * U_BF16 * rot.abs())
    return out


# ---- one problem per (case, regime), computed once and shared --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_problem(c, regime):
    q, k, v, do, keypad, targets = inputs(c, regime)
    mask = R.dense_mask(c.B, c.L, c.S, c.causal, c.start, keypad, None)
    want_out, want_lse, live = R.reference_fwd(q, k, v, mask)
    s = q.double() @ R.rep(k.double(), c.h // c.hk).transpose(-1, -2) / math.sqrt(c.dh) + mask.double()
    p = torch.softmax(s, -1)
    out_bar, lse_bar = fwd_bars(c, q, k, v, p, want_out, want_lse)
    assert bool((visible(c, keypad).any(-1)[:, None] == live).all())
    return SimpleNamespace(c=c, regime=regime, q=q, k=k, v=v, do=do, keypad=keypad, mask=mask, targets=targets, p=p,
                           want_out=want_out, want_lse=want_lse, live=live, out_bar=out_bar, lse_bar=lse_bar)


@functools.lru_cache(maxsize=None)
def backward_problem(c, regime):
    """The forward problem plus the fp64 gradients and their bars.  bf16: a row without a visible key takes no part in
    the backward (the kernels' documented contract, tests/test_attention_range_gpu.py) -- the reference is autograd with
    dO zeroed at those rows.  The fp32 cases have no such row."""
    f = forward_problem(c, regime)
    do = f.do
    if c.dtype == BF:
        do = torch.where(f.live.permute(0, 2, 1)[..., None], f.do.view(c.B, c.L, c.h, c.dh),
                         torch.zeros((), dtype=BF)).reshape(c.B, c.L, c.h * c.dh)
    else:
        assert f.live.all()
    out_ref, dq, dk, dv, p = reference_bwd(f.q, f.k, f.v, do, f.mask)
    grads = (dq, dk, dv)
    bars = bwd_bars(c, f.q, f.k, f.v, do, out_ref, p, f.want_lse, grads, f.mask, f.live)
    return SimpleNamespace(**vars(f), do_live=do, grads=grads, bars=bars)


def ratio(got, want, bar, where=None):
    """-> worst |got - want| / bar (where `where`), max |got - want|.  Where the bar is 0 -- dk / dv of a hidden key, dq
    of a row without a visible key, dq columns whose k column is all zeros: sums of exact zeros -- only 0 passes."""
    return float(ratios(got, want, bar, where).max()), float((got.detach().double().cpu() - want).abs().max())


def ratios(got, want, bar, where=None):
    err = (got.detach().double().cpu() - want).abs()
    if where is not None:
        err = torch.where(where, err, torch.zeros_like(err))
    return torch.where(err == 0, torch.zeros_like(err), err / bar)
