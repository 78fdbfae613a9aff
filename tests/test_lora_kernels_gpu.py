"""vy_lora_shrink + vy_lora_expand (ops.lora_delta_) on the MI355X: exact integer data bit for bit, random data against
fp64 on the same inputs at the bars test_kernels_gpu.py holds vy_linear_fwd to (fp32: 1e-5 + 1e-5 |want|; bf16: 3e-2 +
1e-2 |want| with the oracle on the bf16-rounded inputs, u rounded to bf16 as include/vyom_hip.h says), and everything
that must stay as it was: rows outside the tiles, the padding columns of y's rows, rows behind T, skipped tiles.

One layout of rows for every case: tiles of 1, 15 and 16 rows, a 17-row segment (16 + 1), three slots in one launch,
gaps without an adapter between them; the tiles are listed out of row order."""
import math

import pytest
import torch

from tests.test_kernels_gpu import check, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SLOTS = 3
# (row0, nrows, slot): rows 0-1, 3, 50-52 and 70-71 belong to no tile
TILES = [(53, 16, 0), (2, 1, 0), (4, 15, 1), (69, 1, 0), (19, 16, 2), (35, 15, 2)]
T, CANARY, PAD = 72, 4, 8
ALPHA = (1.0, -1.5, 0.5)
# (K, N, boundaries, r_pad)
SHAPES = [(64, 48, (16, 32), 32), (512, 1024, (), 64), (512, 48, (16, 32), 64), (64, 1024, (), 32)]


def in_tile():
    m = torch.zeros(T, dtype=torch.bool)
    slot = torch.full((T,), -1)
    for r0, n, s in TILES:
        assert not m[r0:r0 + n].any()
        m[r0:r0 + n], slot[r0:r0 + n] = True, s
    return m, slot


def restate(y, x, A, B, alpha, bounds, r_pad, round_u):
    """fp64 on the same inputs -> (T, N); round_u: u takes the dtype's rounding between the two products."""
    live, slot = in_tile()
    N = y.shape[1]
    part = torch.zeros(N, dtype=torch.long)
    for b in bounds:
        part += torch.arange(N) >= b
    want = y.double().clone()
    for t in range(T):
        if live[t]:
            s = int(slot[t])
            u = round_u(x[t].double() @ A[s].double().t())
            cols = part[:, None] * r_pad + torch.arange(r_pad)[None]                    # (N, r_pad)
            want[t] += alpha[s] * (u[cols] * B[s].double()).sum(-1)
    return want


def launch(y, x, A, B, alpha, bounds, tiles=TILES):
    """y (T, N) values -> (the buffer (T + CANARY, N + PAD) before, after), y a view of its first T rows / N columns."""
    from vyomai_amd import ops
    N = y.shape[1]
    buf = torch.full((T + CANARY, N + PAD), 7.0, dtype=y.dtype)
    buf[:T, :N] = y
    before = buf.clone()
    dbuf = buf.to(DEV)
    tl = torch.tensor(tiles, dtype=torch.int32, device=DEV).view(-1, 3)
    out = ops.lora_delta_(dbuf[:T, :N], x.to(DEV), A.to(DEV), B.to(DEV), torch.tensor(alpha, device=DEV), tl, len(tiles),
                          bounds, name="test")
    torch.cuda.synchronize()
    assert out.data_ptr() == dbuf.data_ptr()
    return before, dbuf.cpu()


def untouched(before, after, N):
    live, _ = in_tile()
    assert torch.equal(after[:T][~live], before[:T][~live]), "a row outside every tile changed"
    assert torch.equal(after[:, N:], before[:, N:]), "the padding columns of y's rows were written"
    assert torch.equal(after[T:], before[T:]), "rows behind T were written"


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,N,bounds,r_pad", SHAPES)
def test_exact_integer_data(K, N, bounds, r_pad, dtype):
    """Asymmetric A and B with two non-zeros per row, integer x, y and alpha: |u| <= 8 and |y| <= 136, every
    intermediate exact in bf16, so the result is required bit for bit.  A swapped row / column, a wrong part or slot or
    a k the two operands disagree about all show."""
    g = torch.Generator().manual_seed(K + N)
    parts = 1 + len(bounds)
    R = parts * r_pad
    x = torch.randint(-2, 3, (T, K), generator=g).float()
    y = torch.randint(-40, 41, (T, N), generator=g).float()
    A = torch.zeros(SLOTS, R, K)
    B = torch.zeros(SLOTS, N, r_pad)
    for s in range(SLOTS):
        for r in range(R):
            A[s, r, (7 * r + 3 * s + 1) % K] += 1 + r % 2
            A[s, r, (13 * r + 5 * s + 2) % K] -= 2
        for n in range(N):
            B[s, n, (3 * n + s) % r_pad] += 1 + n % 3
            B[s, n, (5 * n + 7 * s + 1) % r_pad] -= 1 + s
    alpha = (1.0, 2.0, -1.0)
    want = restate(y, x, A, B, alpha, bounds, r_pad, lambda u: u)
    assert float(want.abs().max()) <= 256 and bool((want != y.double()).any())
    before, after = launch(y.to(dtype), x.to(dtype), A.to(dtype), B.to(dtype), alpha, bounds)
    untouched(before, after, N)
    assert torch.equal(after[:T, :N].double(), want), f"{int((after[:T, :N].double() != want).sum())} elements differ"


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,N,bounds,r_pad", SHAPES)
def test_random_data_against_fp64(K, N, bounds, r_pad, dtype):
    parts = 1 + len(bounds)
    x, y = rnd(T, K, seed=1).to(dtype), rnd(T, N, seed=2).to(dtype)
    A = rnd(SLOTS, parts * r_pad, K, seed=3, scale=1 / math.sqrt(K)).to(dtype)
    B = rnd(SLOTS, N, r_pad, seed=4, scale=1 / math.sqrt(r_pad)).to(dtype)
    want = restate(y, x, A, B, ALPHA, bounds, r_pad, lambda u: u.to(dtype).double())
    before, after = launch(y, x, A, B, ALPHA, bounds)
    untouched(before, after, N)
    live, _ = in_tile()
    got = after[:T, :N]
    print(f"{dtype} K {K} N {N} r_pad {r_pad}: max |got - fp64| {float((got.double() - want).abs().max()):.3e}")
    assert bool((got[live] != before[:T, :N][live]).any())
    if dtype == BF:
        check(got, want, 3e-2, 1e-2, "lora delta bf16")
    else:
        check(got, want, 1e-5, 1e-5, "lora delta fp32")


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_skipped_tiles_change_nothing(dtype):
    """slot -1, slot == slots, rows that leave [0, T) at either end, more than 16 rows, no rows: skipped unread, in a
    launch of their own and beside live tiles."""
    K, N, bounds, r_pad = SHAPES[0]
    x, y = rnd(T, K, seed=1).to(dtype), rnd(T, N, seed=2).to(dtype)
    A = rnd(SLOTS, 3 * r_pad, K, seed=3, scale=1 / math.sqrt(K)).to(dtype)
    B = rnd(SLOTS, N, r_pad, seed=4, scale=1 / math.sqrt(r_pad)).to(dtype)
    dead = [(0, 2, -1), (50, 3, SLOTS), (70, 5, 0), (-1, 2, 1), (T, 1, 0), (50, 17, 2), (3, 0, 1), (0, 1, 1 << 20)]
    before, after = launch(y, x, A, B, ALPHA, bounds, tiles=dead)
    assert torch.equal(before, after)
    _, alone = launch(y, x, A, B, ALPHA, bounds)
    _, mixed = launch(y, x, A, B, ALPHA, bounds, tiles=dead[:4] + TILES + dead[4:])
    assert torch.equal(alone, mixed)


def test_no_tiles_launches_nothing_and_host_checks(monkeypatch):
    from vyomai_amd import ops
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a: calls.append(name))
    y = torch.zeros(4, 48, device=DEV)
    x = torch.zeros(4, 64, device=DEV)
    A, B = torch.zeros(2, 32, 64, device=DEV), torch.zeros(2, 48, 32, device=DEV)
    al, tl = torch.ones(2, device=DEV), torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    assert ops.lora_delta_(y, x, A, B, al, tl[:0], 0) is y and calls == []
    ops.lora_delta_(y, x, A, B, al, tl, 1)
    assert calls == ["vy_lora_shrink", "vy_lora_expand"]
    for bad, match in (((y, x[:, :48].contiguous(), A[:, :, :48].contiguous(), B, al, tl, 1), r"\(qkv\): K = 48"),
                       ((y[:, :40], x, A, B[:, :40].contiguous(), al, tl, 1), r"\(qkv\): .*N = 40"),
                       ((y, x, A, B, al, tl, 1, (8,)), "boundaries"),
                       ((y, x, A, B, al, tl, 1, (16,)), "A must be a contiguous"),
                       ((y, x.bfloat16(), A, B, al, tl, 1), "must share"),
                       ((y, x, A, B, al.double(), tl, 1), "alpha must be"),
                       ((y, x, A, B, al, tl.long(), 1), "tiles must be"),
                       ((y, x, A, B, al, tl, 2), "tiles must be")):
        with pytest.raises(ValueError, match=match):
            ops.lora_delta_(*bad, name="qkv")
