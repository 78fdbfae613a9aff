"""The QKV projection + rotary epilogue (vy_qkv_rope_fwd; vy_gemm.hip: gemm_epilogue<..., EPI = 1>, epi_qkv_pair, the
skinny kernels' rotary branches, gemm_splitk_finish_kernel<..., EPI = 1>, vy_rope_qk after the GEMM where the rotation
is not fused) held bit for bit on every GEMM route.  Shared by test_qkv_rope_rule_cpu.py (the routes, the helper's
convention against the oracle, the planted mutations) and test_qkv_rope_exact_gpu.py (the kernels).  Pure CPU.

The entry point takes the cos / sin tables as arguments, so two rules need no tolerance:

  Q  quarter turns: cos = [1, 0, -1, 0][t], sin = [0, 1, 0, -1][t] from a seeded t = randint(0, 4) per (row, d).  Every
     rotation is a signed permutation of a pair; with the integer operands of the exact GEMM tests (x and bias in -2..2,
     thin ternary weights, assert_bf16_exact on the projection) every output is an integer that bf16 and fp32 hold:
     equal on every route, in both dtypes.  (A value comparison: -0 == 0.)
  R  real angles (ops.rope_tables), bf16: the projection is still exact, so the rotary stage has ONE right answer, the
     reference's q * cos + rotate_half(q) * sin evaluated in bf16 with cos / sin cast to bf16 first and every product
     and the sum rounded -- on the CPU (y_bf * c_bf) + (rotate_half(y_bf) * s_bf) in torch bf16 arithmetic.

route() restates launch_bf16's choice of kernel for EPI = 1.  It cannot observe which kernel ran: it is kept honest by
test_qkv_rope_rule_cpu.py (every case's declared route equals it, every route is reached) and by the comment that ties
it to the launcher -- it has to move with launch_bf16, launch_mid, splitk_slices (vy_gemm.hip) and ops._mid_ws."""
import functools

import numpy as np
import torch

from tests.test_kernels_gpu import assert_bf16_exact, ints, thin_ternary

BF = torch.bfloat16
GUARD = 3                  # cache rows behind the written slice
WS_BYTES = 64 << 20        # ops._WS_BYTES

MUTATIONS = ("unrotated", "pos_plus_1", "pos_minus_1", "sin_sign", "partner_xor1", "kv_boundary_one_far",
             "kv_boundary_one_short", "batch_stuck_in_block", "table_row_mod_256", "kv_at_l")


# ---------------------------------------------------------------------------------------------------------------
# the route.  MUST MOVE WITH launch_bf16 / launch_mid / splitk_slices / qkv_impl (vy_gemm.hip) and ops._mid_ws.
# ---------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def splitk_slices(tiles, KT, target):
    """splitk_slices of vy_gemm.hip with one launch chain (g_chains == 1)."""
    if tiles * 3 >= target * 2:
        return 1
    S = min((target + tiles // 2) // tiles, KT // 2, 16)
    if S < 2:
        return 1
    p2 = 2
    while p2 * 2 <= S:
        p2 *= 2
    per = cdiv(KT, p2)
    return cdiv(KT, per)


def fused(dh, rope, dtype=BF):
    """qkv_impl: the rotation rides the GEMM's epilogue for bf16 and 64-wide heads only."""
    return bool(rope) and dtype == BF and dh == 64


def rotation(dh, rope, dtype=BF):
    return "none" if not rope else ("fused" if fused(dh, rope, dtype) else "rope_qk")


def route(M, N, K, dh, rope, has_workspace, dtype=BF):
    """The kernel vy_qkv_rope_fwd launches for M rows (operands 16-byte aligned, K % 8 == 0, which the entry point
    requires).  rope: tables given.  has_workspace: the stream has a split-K workspace of ops._WS_BYTES, which
    ops._mid_ws registers for 32 < M <= 4096."""
    if dtype != BF:
        return "f32"
    f = fused(dh, rope, dtype)
    if M <= 4 and not f:
        return "gemv"
    if M <= 32 and K % 32 == 0 and N % 16 == 0 and N // 32 < 200 and (not f or (N % 64 == 0 and dh == 64)):
        return "skinny16"
    if M <= 32 and K % 16 == 0 and (not f or N % 64 == 0) and N <= 8192:
        return "skinny32"
    if M <= 32:
        return "tile32x128"
    if M <= 1024 or cdiv(M, 256) * cdiv(N, 192) < 160:
        if 128 < M <= 256:
            name, BM, target = "all256", 256, 256
        elif 128 < M <= 320:
            name, BM, target = "all320", 320, 256
        else:
            name, BM, target = "mid128", 128, 448
        tiles = cdiv(M, BM) * cdiv(N, 128)
        S = splitk_slices(tiles, cdiv(K, 64), target)
        ws = has_workspace and 32 < M <= 4096 and S * tiles * BM * 128 * 4 <= WS_BYTES
        return name + ("+splitk" if S > 1 and ws else "")
    return "m16_256" if N >= 3072 else "x3m16_192"


ROUTES = ("gemv", "skinny16", "skinny32", "tile32x128", "mid128", "all256", "all320", "mid128+splitk", "all256+splitk",
          "all320+splitk", "x3m16_192", "m16_256", "f32")
FUSED_ROUTES = tuple(r for r in ROUTES if r not in ("gemv", "f32"))     # gemv and fp32 never fuse the rotation


# ---------------------------------------------------------------------------------------------------------------
# the case table: (B, L, K, h, hk, dh) -> the route it is meant to reach with the rotation on
# ---------------------------------------------------------------------------------------------------------------
def _case(route_, B, L, K, h, hk, dh, dtype=BF, pos0=5, ws=True, store="vec"):
    c = dict(route=route_, B=B, L=L, K=K, h=h, hk=hk, dh=dh, dtype=dtype, pos0=pos0, ws=ws, store=store,
             M=B * L, N=(h + 2 * hk) * dh)
    c["id"] = "%s-%dx%dx%d-h%dx%dx%d-%s%s%s%s" % (route_, B, L, K, h, hk, dh, "bf16" if dtype == BF else "f32",
                                                 "" if pos0 == 5 else f"-pos{pos0}", "" if ws else "-nows",
                                                 "" if store == "vec" else "-" + store)
    return c


def cases():
    out = []
    a = lambda *args, **kw: out.append(_case(*args, **kw))
    # 16-column skinny kernel, rotation fused
    a("skinny16", 32, 1, 768, 12, 12, 64)
    a("skinny16", 7, 1, 64, 4, 2, 64)
    # 32-column skinny kernel: K no multiple of 32
    a("skinny32", 32, 1, 48, 12, 4, 64)
    # 32 x 128 fallback: K no multiple of 16
    a("tile32x128", 17, 1, 40, 4, 2, 64)
    a("tile32x128", 2, 9, 40, 4, 2, 64)
    # 128 x 128 mid tile: 100 rows, 900 rows, 1500 rows (past 1024, 6 x 7 = 42 tiles of 256 x 192: under 160)
    a("mid128", 2, 50, 136, 12, 4, 64)
    a("mid128", 3, 300, 136, 12, 4, 64)
    a("mid128", 5, 300, 136, 12, 4, 64)
    a("mid128", 2, 50, 136, 12, 4, 64, pos0=1000)
    # all-rows tiles
    a("all256", 3, 67, 136, 12, 4, 64)
    a("all320", 4, 75, 136, 12, 4, 64)
    a("all320", 1, 300, 136, 12, 12, 64)
    # split-K + finish: the 100-, 201-, 300- and 900-row cases at K = 520, with the workspace and without it
    for ws in (True, False):
        s = "+splitk" if ws else ""
        a("mid128" + s, 2, 50, 520, 12, 4, 64, ws=ws)
        a("all256" + s, 3, 67, 520, 12, 4, 64, ws=ws)
        a("all320" + s, 4, 75, 520, 12, 4, 64, ws=ws)
        a("all320" + s, 1, 300, 520, 12, 12, 64, ws=ws)
        a("mid128" + s, 3, 300, 520, 12, 4, 64, ws=ws)
    # 256 x 192, three-deep ring: 15 x 12 tiles; 23 x 7 tiles with the k | v boundary (column 1024) inside a tile
    a("x3m16_192", 12, 300, 136, 12, 12, 64)
    a("x3m16_192", 19, 300, 136, 12, 4, 64)
    # 256 x 256, no rotary table in LDS: N = 3072
    a("m16_256", 9, 300, 72, 32, 8, 64)
    # rotation not fused (vy_rope_qk after the GEMM).  1800 x 1024 is 8 x 6 = 48 tiles of 256 x 192, so launch_bf16 keeps
    # it on the mid-size tile; 3600 x 2304 with 128-wide heads is the large kernel without the fused rotation
    a("mid128+splitk", 1, 40, 264, 2, 1, 128)       # 4 tiles, 5 k-stages: two slices
    a("mid128", 2, 17, 64, 4, 2, 16)
    a("gemv", 2, 2, 1152, 16, 16, 72)
    a("mid128", 6, 300, 72, 4, 2, 128)
    a("x3m16_192", 12, 300, 72, 12, 3, 128)
    # fp32 (Rule Q only)
    a("f32", 2, 17, 64, 4, 2, 16, dtype=torch.float32)
    a("f32", 3, 50, 72, 12, 4, 64, dtype=torch.float32)
    a("f32", 2, 67, 260, 16, 16, 72, dtype=torch.float32)
    # store forms, one case per kernel family: q with a sequence stride of dh + 4 (vec8 = 0: the scalar stores), K / V
    # slices of a cache whose head stride is a multiple of 4 and no multiple of 8
    for store in ("qpad", "kvpad"):
        a("skinny16", 7, 1, 64, 4, 2, 64, store=store)
        a("skinny32", 32, 1, 48, 12, 4, 64, store=store)
        a("tile32x128", 2, 9, 40, 4, 2, 64, store=store)
        a("all256", 3, 67, 136, 12, 4, 64, store=store)
        a("all256+splitk", 3, 67, 520, 12, 4, 64, store=store)
        a("x3m16_192", 19, 300, 136, 12, 4, 64, store=store)
        a("m16_256", 9, 300, 72, 32, 8, 64, store=store)
        a("gemv", 2, 2, 1152, 16, 16, 72, store=store)
        a("f32", 3, 50, 72, 12, 4, 64, dtype=torch.float32, store=store)
    assert len({c["id"] for c in out}) == len(out)
    return out


def route_of(c, rope):
    return route(c["M"], c["N"], c["K"], c["dh"], rope, c["ws"], c["dtype"])


# ---------------------------------------------------------------------------------------------------------------
# operands and tables
# ---------------------------------------------------------------------------------------------------------------
def quarter_tables(rows, dh, seed=0):
    """fp32 cos / sin (rows, dh / 2): every angle a multiple of a quarter turn."""
    g = torch.Generator().manual_seed(4241 + 31 * rows + dh + seed)
    t = torch.randint(0, 4, (rows, dh // 2), generator=g)
    return (torch.tensor([1.0, 0.0, -1.0, 0.0])[t].contiguous(), torch.tensor([0.0, 1.0, 0.0, -1.0])[t].contiguous())


def real_tables(rows, dh):
    """fp32 cos / sin (rows, dh / 2), evaluated on the host as vyomai_amd.ops.rope_tables does."""
    inv_freq = 1.0 / (10000 ** (torch.arange(0, dh, 2).float() / dh))
    ang = torch.einsum("i,j->ij", torch.arange(rows).type_as(inv_freq), inv_freq)
    return ang.cos().contiguous(), ang.sin().contiguous()


def table_rows(c):
    return c["pos0"] + c["L"] + 1       # one row past the last position: pos_plus_1 stays inside the table


@functools.lru_cache(maxsize=None)
def _operands(B, L, K, h, hk, dh):
    N = (h + 2 * hk) * dh
    x = ints(B, L, K, seed=1, lo=-2, hi=2)
    w = thin_ternary(N, K, K, seed=2)
    b = ints(N, seed=3, lo=-2, hi=2)
    y = x.view(B * L, K) @ w.t() + b         # fp32 on the CPU: integers far below 2^24, exact
    assert_bf16_exact(y, f"qkv projection {B}x{L}x{K} -> {N}")
    return x, w, b, y


def operands(c):
    """-> x (B, L, K), w (N, K), bias (N), y = x w^T + bias (M, N): fp32 tensors of small integers.  Computed once per
    shape and shared: leave them unchanged."""
    return _operands(c["B"], c["L"], c["K"], c["h"], c["hk"], c["dh"])


# ---------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------
def rotate_half(t):
    half = t.shape[-1] // 2
    return torch.cat((-t[..., half:], t[..., :half]), dim=-1)


def rotate(t, cos, sin, pos, dtype=torch.float64, inverse=False, partner_xor1=False):
    """t (..., L, dh) rotated at the table rows pos (L,): t * cos + rotate_half(t) * sin in `dtype`, cos / sin cast to
    `dtype` first, every operation rounded to it (the reference's apply_rotary_pos_emb).  inverse: the transposed
    rotation (sin negated)."""
    c = torch.cat((cos[pos], cos[pos]), dim=-1).to(dtype)
    s = torch.cat((sin[pos], sin[pos]), dim=-1).to(dtype)
    if inverse:
        s = -s
    t = t.to(dtype)
    if partner_xor1:
        d = torch.arange(t.shape[-1])
        other = t[..., d ^ 1] * torch.where(d < t.shape[-1] // 2, -1.0, 1.0).to(dtype)
    else:
        other = rotate_half(t)
    return t * c + other * s


def expect(c, cos, sin, rule="Q", mut=None):
    """-> q (B, h, L, dh), k, v (B, hk, L, dh) in fp64 for the case's operands.  cos / sin None: no rotation.
    rule Q: fp64 arithmetic (exact for quarter turns); rule R: bf16 arithmetic.  mut: one of MUTATIONS planted."""
    B, L, h, hk, dh, pos0 = c["B"], c["L"], c["h"], c["hk"], c["dh"], c["pos0"]
    M = B * L
    y = operands(c)[3]
    heads = y.view(M, h + 2 * hk, dh).permute(1, 0, 2)                # (head, row, dh)
    if cos is not None and mut != "unrotated":
        l = torch.arange(M) % L
        if mut == "table_row_mod_256":
            l = l % 256
        pos = pos0 + l + {"pos_plus_1": 1, "pos_minus_1": -1}.get(mut, 0)
        s = -sin if mut == "sin_sign" else sin
        nrot = h + hk + {"kv_boundary_one_far": 1, "kv_boundary_one_short": -1}.get(mut, 0)
        dt = torch.float64 if rule == "Q" else BF
        src = heads if rule == "Q" else heads.to(BF)
        rot = rotate(src[:nrot], cos, s, pos, dt, partner_xor1=mut == "partner_xor1").double()
        heads = torch.cat((rot, heads[nrot:].double()), dim=0)
    heads = heads.double()
    # row m of the projection lands at (batch, position) = (m / L, m % L)
    m = np.arange(M)
    b = m // L
    if mut == "batch_stuck_in_block":
        b = (m // 256 * 256) // L
    src = np.full(M, -1)
    src[b * L + m % L] = m                  # (numpy: of repeated indices the last one is assigned)
    placed = torch.zeros(h + 2 * hk, M, dh, dtype=torch.float64)
    hit = torch.from_numpy(src >= 0)
    placed[:, hit] = heads[:, torch.from_numpy(src[src >= 0])]
    out = placed.view(h + 2 * hk, B, L, dh).permute(1, 0, 2, 3)
    return out[:, :h], out[:, h:h + hk], out[:, h + hk:]


def in_cache(t, c, mut=None):
    """k or v (B, hk, L, dh) -> the (B, hk, pos0 + L + GUARD, dh) cache it is written into, zero elsewhere."""
    B, hk, L, dh = t.shape
    cache = torch.zeros(B, hk, c["pos0"] + L + GUARD, dh, dtype=t.dtype)
    at = 0 if mut == "kv_at_l" else c["pos0"]
    cache[:, :, at:at + L] = t
    return cache


def band(c, mut):
    """-> {"q" | "k" | "v": boolean mask over q (B, h, L, dh) or the k / v caches} of the elements the mutation is
    meant to move, or None where the mutation does not apply to the case (it would leave the expectation as it is)."""
    B, L, h, hk, dh, pos0 = c["B"], c["L"], c["h"], c["hk"], c["dh"], c["pos0"]
    cap = pos0 + L + GUARD
    q = torch.zeros(B, h, L, dh, dtype=torch.bool)
    k, v = torch.zeros(B, hk, cap, dh, dtype=torch.bool), torch.zeros(B, hk, cap, dh, dtype=torch.bool)
    kw = k[:, :, pos0:pos0 + L]
    vw = v[:, :, pos0:pos0 + L]
    if mut in ("unrotated", "pos_plus_1", "pos_minus_1", "sin_sign", "partner_xor1"):
        q[:], kw[:] = True, True
        return {"q": q, "k": k}
    if mut == "kv_boundary_one_far":
        vw[:, 0] = True
        return {"v": v}
    if mut == "kv_boundary_one_short":
        kw[:, hk - 1] = True
        return {"k": k}
    if mut == "table_row_mod_256":
        if L <= 256:
            return None
        q[:, :, 256:], kw[:, :, 256:] = True, True
        return {"q": q, "k": k}
    if mut == "batch_stuck_in_block":
        m = torch.arange(B * L)
        moved = ((m // 256 * 256) // L != m // L).view(B, 1, L, 1)      # the rows behind a boundary inside their block
        if not bool(moved.any()):
            return None
        q[:], kw[:], vw[:] = moved, moved, moved
        return {"q": q, "k": k, "v": v}
    if mut == "kv_at_l":
        for t in (k, v):
            t[:, :, :L], t[:, :, pos0:pos0 + L] = True, True
        return {"k": k, "v": v}
    raise ValueError(mut)
