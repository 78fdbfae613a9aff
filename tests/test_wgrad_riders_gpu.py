"""vy_linear_wgrad_riders: zero and transposing riders behind the tiles of the 256 x 256 weight gradient.  Nothing here
rounds, so every demand is torch.equal: dw / db against the same launch without riders, the cleared ranges against
zeros with their neighbours untouched, every W^T against src.t().

Every shape keeps at most TWO M-splits: a sum of two float atomics on zero does not depend on their order, three do."""
import pytest
import torch

from vyomai_amd import ops
from vyomai_amd._lib import VyomHipError

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
M, N = 4096, 8200
# K -> (tiles, M-splits, what the riders find): 33 x 3 = 99 tiles x 2 splits, less than one round; 33 x 9 = 297 tiles,
# 1.16 rounds; 33 x 8 = 264 tiles, 8 workgroups in the last round and 248 CUs idle
SHAPES = (520, 2056, 2048)
SENTINEL = 7.0
CHUNK = 1 << 16   # floats a zero rider clears


def _operands(n, k):
    g = torch.Generator(device=DEV).manual_seed(1000 * n + k)
    ld = (n + 63) // 64 * 64
    dybuf = torch.zeros(M * ld, dtype=BF, device=DEV)
    dy = dybuf.view(M, ld)[:, :n]
    dy.copy_((torch.randn(M, n, device=DEV, generator=g) * 0.05).to(BF))
    x = torch.randn(M, k, device=DEV, generator=g).to(BF)
    alpha = torch.full((1,), 0.75, device=DEV)
    return dybuf, dy, x, alpha


def _plain(dy, x, alpha):
    n, k = dy.shape[1], x.shape[1]
    dw = torch.full((n, k), SENTINEL, device=DEV)
    db = torch.full((n,), SENTINEL, device=DEV)
    ops.linear_wgrad(dy, x, dw, db, False, alpha)
    return dw, db


@pytest.fixture(scope="module")
def plain():
    """(operands, dw, db) of the rider-less launch per K, computed once."""
    cache = {}

    def get(n, k):
        if (n, k) not in cache:
            dybuf, dy, x, alpha = _operands(n, k)
            cache[(n, k)] = (dybuf, dy, x, alpha, *_plain(dy, x, alpha))
        return cache[(n, k)]
    return get


class Riders:
    """Zero ranges inside one sentinel-filled buffer (16-byte aligned but otherwise odd starts, lengths that are no
    multiple of the chunk) and a transpose batch: ragged 64 x 64 tiles, a padded destination stride, one single tile."""

    def __init__(self):
        lens = (2 * CHUNK + 12345, 1001, CHUNK, 70003)
        self.buf = torch.full((sum(lens) + 4096,), SENTINEL, device=DEV)
        self.want = self.buf.clone()
        self.zero, o = [], 0
        for i, n in enumerate(lens):
            o = (o + 40 + 8 * i) // 8 * 8 + 4      # 4 mod 8 floats: 16-byte aligned and no more
            self.zero.append(self.buf[o:o + n])
            self.want[o:o + n] = 0.0
            o += n + 3                              # sentinels stay between the ranges
        g = torch.Generator(device=DEV).manual_seed(7)
        self.pairs, self.full = [], []
        for r, c, pad in ((70, 130, 0), (768, 776, 24), (64, 64, 0), (1031, 768, 1)):
            src = torch.randn(r, c, device=DEV, generator=g).to(BF)
            full = torch.full((c, r + pad), 3.0, dtype=BF, device=DEV)
            self.pairs.append((src, full[:, :r]))
            self.full.append((full, r))
        self.batch = ops.TransposeBatch(self.pairs)

    def check_done(self):
        assert torch.equal(self.buf, self.want)     # the ranges are zero, every float outside them is the sentinel
        for (src, dst), (full, r) in zip(self.pairs, self.full):
            assert torch.equal(dst, src.t())
            assert bool((full[:, r:] == 3.0).all())  # pad columns stay as they were

    def check_untouched(self):
        assert bool((self.buf == SENTINEL).all())
        for full, _ in self.full:
            assert bool((full == 3.0).all())


@pytest.mark.parametrize("k", SHAPES)
def test_riders_change_nothing_and_do_their_work(plain, k):
    _, dy, x, alpha, dw0, db0 = plain(N, k)
    dw1, db1 = _plain(dy, x, alpha)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1), "two rider-less launches differ: the shape is not order-free"
    rd = Riders()
    dw = torch.full((N, k), SENTINEL, device=DEV)
    db = torch.full((N,), SENTINEL, device=DEV)
    zero_taken, tiles = ops.linear_wgrad_riders(dy, x, dw, db, False, alpha, zero=rd.zero, transposes=rd.batch)
    # a few MB against a budget of tens: everything rides
    assert zero_taken == [z.numel() for z in rd.zero] and tiles == rd.batch.total
    assert torch.equal(dw, dw0) and torch.equal(db, db0)
    rd.check_done()


def test_offset_form_of_the_batched_transpose():
    """What the riders do not take, TransposeBatch.run(first) does: tiles 8 .. of the table -- the 6 tiles of the first
    matrix and the first 2 (of 13 per tile row) of the second stay as they were."""
    rd = Riders()
    rd.batch.run(first=8)
    assert bool((rd.full[0][0] == 3.0).all())
    src, dst = rd.pairs[1]
    want = src.t().clone()
    want[:128, :64] = 3.0                     # tiles 0 and 1 of this matrix: output rows 0..127, columns 0..63
    assert torch.equal(dst, want)
    for (src, dst) in rd.pairs[2:]:
        assert torch.equal(dst, src.t())
    rd.batch.run(first=rd.batch.total)        # nothing left: no launch
    assert bool((rd.buf == SENTINEL).all())


def test_full_last_round_carries_nothing(plain):
    """N = 8192, K = 2048: 32 x 8 = 256 tiles, items % 256 == 0, no CU is idle: 0 taken, the targets untouched."""
    _, dy, x, alpha, dw0, db0 = plain(8192, 2048)
    rd = Riders()
    dw = torch.full((8192, 2048), SENTINEL, device=DEV)
    db = torch.full((8192,), SENTINEL, device=DEV)
    zero_taken, tiles = ops.linear_wgrad_riders(dy, x, dw, db, False, alpha, zero=rd.zero, transposes=rd.batch)
    assert zero_taken == [0] * len(rd.zero) and tiles == 0
    assert torch.equal(dw, dw0) and torch.equal(db, db0)
    rd.check_untouched()


def test_small_tile_launch_carries_nothing():
    """A launch that does not take the 256 x 256 branch (M < 4096) reports 0 and computes what linear_wgrad does."""
    g = torch.Generator(device=DEV).manual_seed(3)
    dy = torch.randn(512, 256, device=DEV, generator=g).to(BF)
    x = torch.randn(512, 128, device=DEV, generator=g).to(BF)
    rd = Riders()
    dw, db = torch.empty(256, 128, device=DEV), torch.empty(256, device=DEV)
    zero_taken, tiles = ops.linear_wgrad_riders(dy, x, dw, db, False, None, zero=rd.zero, transposes=rd.batch)
    assert zero_taken == [0] * len(rd.zero) and tiles == 0
    dw0, db0 = torch.empty_like(dw), torch.empty_like(db)
    ops.linear_wgrad(dy, x, dw0, db0, False, None)
    assert torch.equal(dw, dw0) and torch.equal(db, db0)   # 4 tiles x 2 M-splits
    rd.check_untouched()


def test_zero_ranges_that_meet_the_launch_are_refused(plain):
    dybuf, dy, x, alpha, dw0, db0 = plain(N, 520)
    dw, db = dw0.clone(), db0.clone()
    for bad in (dw.view(-1)[1024:2048], db[4:1004], dybuf.view(torch.float32)[4096:8192], x.view(-1).view(torch.float32)[:64]):
        with pytest.raises(VyomHipError, match="intersects"):
            ops.linear_wgrad_riders(dy, x, dw, db, True, alpha, zero=[bad])
    with pytest.raises(VyomHipError, match="aligned"):
        ops.linear_wgrad_riders(dy, x, dw, db, True, alpha, zero=[torch.ones(64, device=DEV)[1:33]])
    assert torch.equal(dw, dw0) and torch.equal(db, db0)   # a refused call launches nothing
