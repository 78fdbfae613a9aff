"""Shape tables, inputs, fp64 references and bars for the training path's streaming kernels (vyomai_amd/csrc/vy_misc.hip):
LayerNorm forward and backward with the slab column sums, token embedding, the two transposes, the fp32/bf16 cast, AdamW
and vy_sumsq.

Every width table holds both sides of each boundary of the dispatcher it is written for, and dispatch_chunks() restates
that dispatcher so that the coverage assertions can name the instantiation a width reaches.  Every reference is fp64 on
the cast inputs.  A bar is the project's own (elementwise_bars, the 1e-5 parity bar of the statistics, the reduction bars
of test_rmsnorm_bwd_vs_fp64) or derived here from the fp64 reference; none comes from what a kernel returns.

Shared by tests/test_stream_kernels_cpu.py (the guard of the generators: fp32 restatements with faults switched in, no
kernel) and tests/test_stream_kernels_gpu.py.  Nothing here touches the GPU.
"""
import math

import torch

from tests.test_causal_lm_gpu import elementwise_bars   # the bars only (no GPU at import)
from tests.test_kernels_gpu import ints, rnd

BF, F32 = torch.bfloat16, torch.float32
DTYPES = (BF, F32)
VEC = {BF: 8, F32: 4}          # elements of a 16-byte chunk
EPS = 1e-5
SENTINEL = 7.0                 # exact in bf16; what every padded output buffer is filled with before a launch
STAT_BAR = (1e-5, 1e-5)        # mean / rstd: the project's fp32 parity bar, atol + rtol |want|


def tname(dtype):
    return "bf16" if dtype == BF else "fp32"


def worst_ratio(got, want, bar):
    """max |got - want| / bar over the elements; got must be finite.  bar: a number or a tensor like want."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    bar = bar.double() if torch.is_tensor(bar) else torch.full_like(want, float(bar))
    return float(((got - want).abs() / bar).max())


def linear_bar(want, atol, rtol):
    return atol + rtol * want.double().abs()


def dispatch_chunks(N, dtype, most):
    """Chunks per lane CH of the instantiation ln_fwd_dispatch (most = 16) / ln_bwd_dispatch (most = 4) launches for rows
    of N elements: the first CH of 1, 2, 4, 8, 16 with N / VEC <= 64 CH.  None: refused ("too wide")."""
    nch = N // VEC[dtype]
    for ch in (1, 2, 4, 8, 16):
        if ch <= most and nch <= 64 * ch:
            return ch
    return None


# ---- 1. LayerNorm forward ---------------------------------------------------------------------------------------------
LN_FWD_WIDTHS = {BF: (8, 64, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192),
                 F32: (4, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096)}
LN_FWD_ROWS = (5, 7)                       # a workgroup holds four rows (one per wave): a ragged last workgroup both times
LN_FWD_TOO_WIDE = {BF: 8200, F32: 4100}
LN_FWD_STRIDED = {BF: 1032, F32: 516}      # the width that also runs with ldx = N + VEC, ldy = N + 2 VEC
LN_FWD_PADS = (1, 2)                       # a different pad per operand: a stride read from the wrong one shows
LN_FWD_NO_STATS = {BF: 520, F32: 260}      # the width that also runs without mean / rstd pointers
# the offset, small and constant regimes: N = 768 and the widest row of every CH
LN_FWD_OFFSET_WIDTHS = {BF: (768, 512, 1024, 2048, 4096, 8192), F32: (768, 256, 512, 1024, 2048, 4096)}
REGIMES = ("plain", "offset", "small", "constant")


def ln_fwd_cases(dtype):
    """(regime, M, N) of every forward case of a type."""
    out = [("plain", M, N) for N in LN_FWD_WIDTHS[dtype] for M in LN_FWD_ROWS]
    return out + [(regime, M, N) for regime in REGIMES[1:] for N in LN_FWD_OFFSET_WIDTHS[dtype] for M in LN_FWD_ROWS]


def ln_fwd_inputs(dtype, regime, M, N):
    """x (M, N), gamma, beta (N), cast to dtype.  plain: the data of test_layernorm (mean 0.5, sigma 2).  offset: rows of
    64 + 2 randn -- E[x^2] is a thousand times the variance, so a variance taken in one pass (E[x^2] - mean^2) loses three
    digits in fp32 and a two-pass one loses none.  small: 2^-9 randn, a variance of 3.8e-6 beside eps = 1e-5, so a
    dropped eps nearly doubles rstd (on plain and offset data it moves rstd by 1.25e-6).  constant: each row one
    bf16-exact value: the variance is 0, rstd = eps^-1/2, y = beta, and without eps 0 * inf."""
    base = rnd(M, N, seed=1)
    if regime == "constant":
        x = (4.0 * rnd(M, seed=7)).to(BF).float()[:, None].expand(M, N).clone()
    else:
        x = {"plain": base * 2 + 0.5, "offset": 64.0 + 2.0 * base, "small": base * 2.0 ** -9}[regime]
    return x.to(dtype), (1 + 0.1 * rnd(N, seed=2)).to(dtype), (0.1 * rnd(N, seed=3)).to(dtype)


def ln_fwd_reference(x, gamma, beta, eps=EPS):
    """fp64 on the cast inputs -> y (M, N), mean (M), rstd (M)."""
    xd = x.double()
    mean = xd.mean(-1)
    rstd = (xd.var(-1, unbiased=False) + eps).rsqrt()
    y = (xd - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    return y, mean, rstd


def ln_fwd_y_bar(dtype, regime, gamma, y, mean, rstd):
    """elementwise_bars(dtype) of y.  In the offset regime the mean may be off by delta <= 1e-5 (1 + |mean|), its own bar,
    and that moves y by |gamma| rstd delta: the term is added, computed from the fp64 reference."""
    atol, rtol = elementwise_bars(dtype)
    bar = linear_bar(y, atol, rtol)
    if regime == "offset":
        delta = STAT_BAR[0] + STAT_BAR[1] * mean.abs()
        bar = bar + gamma.double().abs()[None, :] * (rstd * delta)[:, None]
    return bar


# ---- 2. LayerNorm backward --------------------------------------------------------------------------------------------
LN_BWD_WIDTHS = {BF: (8, 512, 520, 768, 1024, 1032, 2048), F32: (4, 256, 260, 512, 516, 768, 1024)}
LN_BWD_TOO_WIDE = {BF: 2056, F32: 1028}
# 1, 3: waves without a row.  5: a second, ragged workgroup.  252, 253: 63 and 64 slab rows (one slice / sixteen slices of
# vy_ln_colsum_slices).  257: 65 slab rows, sixteen slices of 5, three of them empty.  2049: the slab is capped at 512 rows
# = 2048 waves, wave 0 takes a second row through the pipeline.  4100: waves 0..3 take three rows, the others two.
LN_BWD_ROWS = (1, 3, 5, 252, 253, 257, 2049, 4100)
LN_BWD_STRIDED = (257, 768)                # (M, N) that also runs with a different pad per operand, per type
LN_BWD_PADS = (1, 2, 3)                    # lddy, ldx, lddx = N + 1, 2, 3 VEC
LN_BWD_COLSUM_ROWS = (3, 253, 257, 2049)   # partial + ColSum against vy_layernorm_bwd, at N = 768


def ln_bwd_ws_rows(M):
    """vy_layernorm_bwd_ws_rows: workgroups = slab rows, four waves each."""
    return min(512, max(1, (M + 3) // 4))


def ln_colsum_slices(WB):
    """vy_ln_colsum_slices (vy_common.h)."""
    return 16 if WB >= 64 else 1


def ln_bwd_cases(dtype):
    """(M, N): every N at M = 5 and 257, every M at N = 768 and at the narrowest and the widest N."""
    Ns = LN_BWD_WIDTHS[dtype]
    cases = {(M, N) for N in Ns for M in (5, 257)} | {(M, N) for M in LN_BWD_ROWS for N in (768, min(Ns), max(Ns))}
    return sorted(cases)


def ln_bwd_inputs(dtype, M, N):
    """dy, x (M, N), gamma (N) cast to dtype (the data of test_layernorm_bwd), and mean, rstd (M) in fp32: the fp64
    statistics of the cast x, rounded once -- they do not come from the forward kernel."""
    x = (rnd(M, N, seed=1) * 2 + 0.3).to(dtype)
    gamma = (1 + 0.1 * rnd(N, seed=2)).to(dtype)
    dy = rnd(M, N, seed=4).to(dtype)
    xd = x.double()
    mean = xd.mean(-1).float()
    rstd = (xd.var(-1, unbiased=False) + EPS).rsqrt().float()
    return dy, x, gamma, mean, rstd


def ln_bwd_reference(dy, x, gamma, mean, rstd):
    """fp64 of what the kernel is given (the fp32 statistics included) -> dx (M, N), dgamma, dbeta (N)."""
    dyd, mu, rs = dy.double(), mean.double()[:, None], rstd.double()[:, None]
    xh = (x.double() - mu) * rs
    gy = dyd * gamma.double()
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    return rs * (gy - s1 - xh * s2), (dyd * xh).sum(0), dyd.sum(0)


def colsum_bars(dtype, M):
    """(atol, rtol) of dgamma / dbeta: the bars test_rmsnorm_bwd_vs_fp64 holds dw to."""
    return (2e-3 * math.sqrt(M), 1e-3) if dtype == BF else (1e-5 * max(1.0, math.sqrt(M)), 0.0)


def ln_twin_inputs(dtype, M, N):
    """The exact twin of the column sums: x, dy integers in -2..2, mean[row] in {-1, 0, 1}, rstd[row] in {1/2, 1/4},
    gamma = 1.  xhat = (x - mean) rstd is a multiple of 1/8 with |xhat| <= 1.5, so every term of dgamma is a multiple of
    1/8 below 4 and every term of dbeta an integer of magnitude <= 2: sums over M <= 4100 rows stay far below 2^24 eighths
    and are exact in fp32 in any order."""
    x = ints(M, N, seed=1, lo=-2, hi=2).to(dtype)
    dy = ints(M, N, seed=4, lo=-2, hi=2).to(dtype)
    mean = ints(M, seed=5, lo=-1, hi=1)
    r = torch.arange(M)
    rstd = 0.25 * (1.0 + ((r + r // 2048) % 2).float())     # neighbours differ, and so do rows r and r + 2048 (one walk)
    return dy, x, torch.ones(N).to(dtype), mean, rstd


def ln_twin_expected(dy, x, mean, rstd, dtype=torch.float64):
    """dgamma, dbeta of the twin, summed in `dtype`: fp64 and fp32 must agree to the bit (test_stream_kernels_cpu.py)."""
    dyd = dy.to(dtype)
    xh = (x.to(dtype) - mean.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    return (dyd * xh).sum(0), dyd.sum(0)


# ---- 4. embedding -----------------------------------------------------------------------------------------------------
EMB_WIDTHS = {BF: (8, 72, 768, 776), F32: (4, 72, 768, 776)}
EMB_VOCABS = (1, 1031)
EMB_ROWS = (1, 5, 500)
EMB_PADDING = 3


def emb_ids(M, V, seed=0):
    """M random ids in [0, V) that hold 0 and V - 1 (as far as M allows)."""
    g = torch.Generator().manual_seed(seed + 31 * M + V)
    ids = torch.randint(0, V, (M,), generator=g)
    ids[0] = 0
    ids[-1] = V - 1
    return ids


def emb_bwd_ids(pattern, M, V):
    """"dups": ids from 40 rows of the table, so every one of them collides.  "same": all M rows the same id, the worst
    collision of the atomics.  "mixed": random ids with the padding row, -1, V and V + 5 among them."""
    g = torch.Generator().manual_seed(17 + M)
    if pattern == "dups":
        ids = torch.randint(0, 40, (M,), generator=g) * (V // 40)
        ids[0], ids[-1] = 0, V - 1
    elif pattern == "same":
        ids = torch.full((M,), V - 2, dtype=torch.long)
    else:
        ids = torch.randint(0, V, (M,), generator=g)
        ids[::7] = EMB_PADDING
        ids[1::50] = -1
        ids[2::50] = V
        ids[3::50] = V + 5
    return ids


def emb_bwd_reference(dout, ids, V, padding_idx, fill=3.0):
    """fill + index_add_ in fp64 over the ids the kernel keeps (in range and not the padding row)."""
    keep = (ids >= 0) & (ids < V)
    if padding_idx is not None:
        keep &= ids != padding_idx
    want = torch.full((V, dout.shape[1]), fill, dtype=torch.float64)
    want.index_add_(0, ids[keep], dout.double()[keep])
    return want, keep


# ---- 5. transposes ----------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = ((1, 7), (31, 1), (33, 65), (100, 257), (768, 3072))
TRANSPOSE_BATCH_SHAPES = ((768, 768), (2304, 768), (1031, 768), (70, 200), (3, 5))     # test_transpose_batched's


# ---- 6. cast ----------------------------------------------------------------------------------------------------------
CAST_SIZES = (1, 3, 5, 1023, 4096 * 1024 + 7)      # the last is past the grid cap of 4096 workgroups x 1024 elements


def cast_halfway():
    """fp32 values exactly halfway between two bf16 neighbours: every normal bf16 pattern of 64 exponents (both parities of
    the last kept bit, both signs) with 0x8000 below it.  Round-to-nearest-even goes down from an even neighbour and up
    from an odd one; truncation and round-half-up each get half of them wrong."""
    exps = torch.arange(1, 255, 4)
    upper = (exps[:, None] << 7 | torch.arange(128)[None, :]).reshape(-1)
    upper = torch.cat([upper, upper | 0x8000])
    words = (upper << 16) | 0x8000                                       # int64: 32-bit patterns, sign bit included
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).view(F32)


def cast_specials():
    """+-0, +-inf, the largest finite fp32 of both signs (they round to inf), NaN."""
    return torch.tensor([0.0, -0.0, float("inf"), float("-inf"), torch.finfo(F32).max, -torch.finfo(F32).max,
                         float("nan")], dtype=F32)


def cast_source(n):
    """n fp32 values: the specials and the halfway values first (as far as n allows), unit-normal data behind them.  No
    fp32 denormals: whether a kernel flushes them is not pinned here."""
    head = torch.cat([cast_specials(), cast_halfway()])
    if n <= head.numel():
        return head[:n].clone()
    return torch.cat([head, rnd(n - head.numel(), seed=6)])


def all_bf16_patterns():
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF)


# ---- 7. AdamW and sumsq -----------------------------------------------------------------------------------------------
ADAMW_SIZES = (1, 3, 4, 5, 1023, 100003)
ADAMW_STRIDE_N = 8192 * 1024 + 5       # past the grid cap of 8192 workgroups x 1024 elements
ADAMW_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAMW_BAR = (1e-6, 1e-5)
SUMSQ_SIZES = (1, 5, 8192 * 1024 + 13)  # the last wants 1025 partials: past the cap of 1024, a second walk of the range


def adamw_paths(n):
    """The paths of adamw_kernel that n elements reach: a thread owns elements 4 t .. 4 t + 3, whole quads take the vector
    path (i + 3 < n), the last n % 4 elements the scalar tail."""
    return ({"vector"} if n >= 4 else set()) | ({"tail"} if n % 4 else set())


def f32(v):
    return float(torch.tensor(v, dtype=F32))


def adamw_reference(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, scale):
    """One step of adamw_kernel's formula in fp64: decoupled decay, then the moments, then the bias-corrected step.  The
    hyper-parameters reach the kernel as fp32 and are rounded to fp32 here first (1 - fl(0.999) and 1 - 0.999 differ by
    1.3e-5 relative, more than the bar).  p, g, m, v: fp64 tensors -> p, m, v."""
    lr, b1, b2, eps, wd, scale = (f32(t) for t in (lr, beta1, beta2, eps, weight_decay, scale))
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    gg = g * scale
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * gg
    v = b2 * v + (1.0 - b2) * gg * gg
    return p - (lr / bc1) * (m / (v.sqrt() / bc2s + eps)), m, v
