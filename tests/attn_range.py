"""Attention inputs whose scores move the running maximum, the fp64 references that go with them and the derived bars.

Unit-normal q and k give scaled scores of about N(0, 1): the first key tile sets the running maximum of an online
softmax and no later tile raises it by much, so the rescale of the accumulators (O and l times exp(m_old - m_new))
is never exercised -- and in attn_fwd_mfma_kernel, which rescales lazily (only when some row of the wave would see
p > 2^8), the branch runs once, on zeros.  The staircase puts a score ramp into component 0: every `period` keys
(one online-softmax step of the kernel under test) the score of row i rises by gain_i * height, with three gains
that make the rows of one wave disagree about whether the maximum has to move.

Shared by tests/test_attention_range_cpu.py (the generator's guard: a CPU emulation with faults switched in) and
tests/test_attention_range_gpu.py, and by the "staircase" regime of the paged-attention harnesses.
"""
import math
from collections import namedtuple

import torch

from tests.test_kernels_gpu import _dense_mask as dense_mask   # the reference's additive finfo.min mask (no GPU at import)

BF = torch.bfloat16
FMIN = torch.finfo(torch.float32).min

# kernel -> keys that one online-softmax step covers -> where that was read
PERIODS = {
    "attn_fwd_mfma_kernel<64|128>": (64, "vyomai_amd/csrc/vy_attn.hip:76,116 (k_tile = 64 rows; compute(): k0 = tile * 64)"),
    "AttnGen::step (attn_fwd_gen_kernel, paged_prefill_kernel bf16)": (
        64, "vyomai_amd/csrc/vy_attn_gen.h:73-93 (four 16-key blocks); vy_attn.hip:380 and vy_paged.hip:681 (k0 = t * 64)"),
    "attn_rowwise_kernel": ("NWV * (64 / CPR) * U = 16 * 64 / CPR", "vyomai_amd/csrc/vy_attn.hip:458,495-496 (KPP, U = 4, STRIDE)"),
    "paged_dec_kernel (decode; fp32 paged prefill)": (
        "PD_NW * U * (64 / LPK), U = 4 (8 for fp8 pages)", "vyomai_amd/csrc/vy_paged.hip:18-20,66,120 (NW * CK per trip)"),
    "vy_dec_attn (vy_decode.hip)": (None, "vyomai_amd/csrc/vy_decode.hip:386-388,456-463 (two passes over resident scores: no rescale)"),
    "attn_bwd_*": (None, "vyomai_amd/csrc/vy_bwd.hip:546,1135 (P = exp2(c s - lse log2 e): no running maximum; data period 64)"),
}


def rowwise_period(dh, dtype):
    """Keys one trip of attn_rowwise_kernel's workgroup covers (NWV = 4 waves, U = 4 key groups per trip)."""
    vec = 8 if dtype == BF else 4
    cpr = 1
    while cpr * vec < dh:
        cpr *= 2
    return 4 * (64 // cpr) * 4


def paged_decode_period(dh, dtype, fp8=False):
    """Keys one trip of paged_dec_kernel's workgroup covers (pd_lpk: the head's 16-byte chunks, a power of two >= 8)."""
    nch = dh // (8 if dtype == BF else 4)
    lpk = 8
    while lpk < nch:
        lpk *= 2
    return 4 * (8 if fp8 else 4) * (64 // lpk)


GAINS = (2.0 / 3.0, 1.0, 2.0)     # x height 6: 4 nat a step (below the lazy threshold of 8 log2 = 5.55 nat), 6 and 12


def stair_levels(S, period, height=6.0, descending=False):
    lv = height * (torch.arange(S) // period).float()
    return -lv if descending else lv


def row_gains(L, gains=GAINS, start_pos=0):
    return torch.tensor(gains, dtype=torch.float32)[(torch.arange(L) + start_pos) % len(gains)]


def staircase(B, h, hk, L, S, dh, period, height=6.0, gains=GAINS, start_pos=0, seed=0, dtype=torch.float32,
              descending=False):
    """q (B, h, L, dh), k and v (B, hk, S, dh), cast to dtype.  Without a mask the scaled score of (i, j) is
    gain_i * height * (j // period) plus noise of sigma about 0.5.  Every reference is computed from the cast tensors."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, h, L, dh, generator=g)
    k = 0.5 * torch.randn(B, hk, S, dh, generator=g)
    v = torch.randn(B, hk, S, dh, generator=g)
    q[..., 0] = math.sqrt(dh) * row_gains(L, gains, start_pos)
    k[..., 0] = stair_levels(S, period, height, descending)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def normal(B, h, hk, L, S, dh, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, h, L, dh, generator=g)
    k = torch.randn(B, hk, S, dh, generator=g)
    v = torch.randn(B, hk, S, dh, generator=g)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def rep(x, n):
    return x if n == 1 else x.repeat_interleave(n, 1)


def reference_fwd(q, k, v, mask):
    """fp64 on the cast tensors, the formulation of O.sdpa (scores + additive mask, softmax, @ v; O.sdpa itself works in
    fp32).  -> out (B, L, h * dh), lse (B, h, L), live (B, h, L): rows with a visible key."""
    B, h, L, dh = q.shape
    n = h // k.shape[1]
    s = q.double() @ rep(k.double(), n).transpose(-1, -2) / math.sqrt(dh) + mask.double()
    out = torch.softmax(s, -1) @ rep(v.double(), n)
    live = (mask > FMIN / 2).any(-1).expand(B, h, L)
    return out.permute(0, 2, 1, 3).reshape(B, L, h * dh), torch.logsumexp(s, -1), live


# ---- forward cases (section by section of the kernel families) -----------------------------------------------------------
# kp: None | "tail" (keys >= 130 of sequence 0 and >= 66 of sequence 1 hidden) | "head" (keys < 70 of sequence 0 -- a whole
# first tile -- and < 5 of sequence 1 hidden).  data: "stair" | "desc" | "normal" | "add" (unit-normal q / k / v, the
# staircase in the additive mask) | "add1" (the same with one broadcast mask row, am_sl = 0)
FwdCase = namedtuple("FwdCase", "family B h hk L S dh causal start kp dtype period data")


def _c(family, B, h, hk, L, S, dh, causal, start=0, kp=None, dtype=BF, period=64, data="stair"):
    return FwdCase(family, B, h, hk, L, S, dh, causal, start, kp, dtype, period, data)


F32 = torch.float32
FWD_CASES = [
    _c("tuned64", 1, 2, 1, 200, 200, 64, True),
    _c("tuned64", 1, 2, 2, 130, 130, 64, False),
    _c("tuned64", 2, 4, 2, 40, 196, 64, True, start=156),
    _c("tuned64", 1, 2, 1, 257, 257, 64, True),
    _c("tuned64", 2, 2, 1, 192, 192, 64, False, kp="tail"),
    _c("tuned128", 1, 2, 1, 131, 131, 128, False),
    _c("tuned128", 1, 4, 2, 150, 150, 128, True),
] + [_c("general", 1, 2, 1, 130, 130, dh, causal) for dh in (72, 96, 256) for causal in (True, False)] + [
    _c("rowwise", 1, 2, 1, 130, 130, 64, True, dtype=F32, period=rowwise_period(64, F32)),
    _c("rowwise", 1, 2, 2, 67, 67, 72, False, dtype=F32, period=rowwise_period(72, F32)),
    _c("rowwise", 2, 4, 2, 17, 17, 16, True, dtype=F32, period=8),
    _c("rowwise", 2, 4, 2, 17, 17, 16, True, dtype=BF, period=8),
    _c("additive", 2, 2, 1, 65, 130, 64, False, dtype=BF, data="add"),
    _c("additive", 2, 2, 1, 65, 130, 64, False, dtype=F32, data="add"),
    _c("additive", 2, 2, 1, 65, 130, 64, False, dtype=BF, data="add1"),
] + [_c("hidden-tile", 2, 2, 1, 150, 150, dh, causal, kp="head", data=data)
     for dh in (64, 128) for causal in (False, True) for data in ("normal", "stair")] + [
    _c("descending", 1, 2, 1, 200, 200, 64, True, data="desc"),
    _c("descending", 1, 2, 1, 130, 130, 72, False, data="desc"),
]


def case_id(c):
    return (f"{c.family}-{c.data}-{c.B}x{c.h}x{c.hk}x{c.L}x{c.S}x{c.dh}-{'causal' if c.causal else 'full'}"
            f"{'-start%d' % c.start if c.start else ''}{'-' + c.kp if c.kp else ''}-{'bf16' if c.dtype == BF else 'fp32'}")


def keypad_of(kind, B, S):
    if kind is None:
        return None
    kp = torch.ones(B, S, dtype=torch.uint8)
    if kind == "tail":
        kp[0, 130:] = 0
        kp[1, 66:] = 0
    elif kind == "head":
        kp[0, :70] = 0
        kp[1, :5] = 0
    else:
        raise ValueError(kind)
    return kp


def fwd_inputs(c, seed=11):
    """-> q, k, v (cast), keypad or None, addmask or None, the dense additive mask (B, 1, L, S)."""
    addmask = None
    if c.data in ("stair", "desc"):
        q, k, v = staircase(c.B, c.h, c.hk, c.L, c.S, c.dh, c.period, start_pos=c.start, seed=seed, dtype=c.dtype,
                            descending=c.data == "desc")
    else:
        q, k, v = normal(c.B, c.h, c.hk, c.L, c.S, c.dh, seed=seed, dtype=c.dtype)
    if c.data == "add":
        addmask = (row_gains(c.L)[:, None] * stair_levels(c.S, 64)[None, :]).expand(c.B, 1, c.L, c.S).contiguous()
    elif c.data == "add1":
        addmask = stair_levels(c.S, 64).expand(c.B, 1, 1, c.S).contiguous()
    if addmask is not None:
        addmask[..., ::7] = FMIN
    keypad = keypad_of(c.kp, c.B, c.S)
    return q, k, v, keypad, addmask, dense_mask(c.B, c.L, c.S, c.causal, c.start, keypad, addmask)


def fwd_bars(c, q, k, v, addmask, want_out, want_lse):
    """-> the bar on out (B, L, h * dh) and on lse (B, h, L).
    bf16: the bars of test_attention_fwd.  fp32: scores reach about 40 here, so an fp32 dot product carries more absolute
    error than on unit-normal data: a score is off by at most delta = (dh + 2) 2^-24 scale max_ij sum_d |q_id k_jd| (dh
    products and sums, the scale, the mask add), which changes a softmax weight by about delta relatively, hence out by
    at most 2 max|v| delta and lse by delta.  With an additive mask the sum x + mask is rounded once more: + 2^-24 times
    the largest finite |mask| + |score|."""
    if c.dtype == BF:
        return 2e-2 + 2e-2 * want_out.abs(), 2e-2 + 1e-4 * want_lse.abs()
    n = c.h // c.hk
    absdot = q.double().abs() @ rep(k.double().abs(), n).transpose(-1, -2)
    scale = 1.0 / math.sqrt(c.dh)
    delta = (c.dh + 2) * 2.0 ** -24 * scale * float(absdot.max())
    if addmask is not None:
        fin = addmask[addmask > FMIN / 2]
        delta += 2.0 ** -24 * (float(fin.abs().max()) + scale * float(absdot.max()))
    out_bar = torch.maximum(1e-5 + 1e-5 * want_out.abs(), torch.full_like(want_out, 2 * float(v.double().abs().max()) * delta))
    return out_bar, 1e-4 + 1e-4 * want_lse.abs() + delta
