"""vy_lora_wgrad (ops.lora_wgrad) and the adapter's two data-gradient products (ops.lora_dgrad_) on the MI355X.

vy_lora_wgrad: exact integer data bit for bit (sparse asymmetric operands: a swapped part, row or k shows), random data
against fp64 on the same inputs at the bars test_bwd_kernels_gpu.py holds vy_linear_wgrad to -- the arithmetic is the
same, exact products and fp32 sums over M -- bf16: 2e-3 sqrt(M) + 1e-3 |want|; fp32: 8e-6 sqrt(M) + 1e-5 |want|.  Every
case: the padded columns of u / t (and a part without an adapter) are NaN and must not reach an output; every output
sits between guard elements; accumulate adds onto 3.0; two runs are bitwise equal.

M_SPLIT: the launcher cuts M into chunks of max(128, ...) rows (vy_lora_wgrad_chunk_rows: about 1024 workgroups over
the column tiles, at least 128 rows a chunk), so for both shapes here 257 = 2 * 128 + 1 is the smallest M with three
chunks, the last one ragged (one row).

ops.lora_dgrad_: t = dY @ B per part and dX += alpha * t @ A against fp64 at the `lora delta` bars of
test_lora_kernels_gpu.py, M = 17 and M = 33 (the second crosses a 16-row tile twice), what dX held is kept."""
import math

import pytest
import torch

from tests.test_kernels_gpu import check, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
M_SPLIT = 257
MS = (1, 17, 300, M_SPLIT)
GUARD = 64
# (K, N, boundaries), (r_pad, rank per part; None: a part without an adapter)
SHAPES = [(64, 48, (16, 32)), (512, 1024, ())]
RANKS = [(32, (32, 32, 32)), (32, (8, 8, 8)), (32, (32, None, 8)), (64, (33, 64, None))]
NAN = float("nan")


def cases():
    seen, out = set(), []
    for K, N, bounds in SHAPES:
        for r_pad, ranks in RANKS:
            ranks = ranks[: 1 + len(bounds)]
            if (K, N, r_pad, ranks) not in seen:
                seen.add((K, N, r_pad, ranks))
                out.append((K, N, bounds, r_pad, ranks))
    return out


def poison(mat, r_pad, ranks):
    """NaN into the columns no output may depend on: j >= rank of each part, every column of a part without adapter."""
    mat = mat.clone()
    for p, r in enumerate(ranks):
        mat[:, p * r_pad + (r or 0):(p + 1) * r_pad] = NAN
    return mat


def guarded(shape, fill):
    """A contiguous fp32 tensor of `shape` on the device between GUARD elements of 7.0 -> (flat buffer, the view)."""
    n = shape[0] * shape[1]
    flat = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device=DEV)
    view = flat[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return flat, view


def run(dy, u, x, t, bounds, r_pad, ranks, alpha, onto=None):
    """-> ([dA_p], [dB_p]) on the host (None for a part without an adapter); guards checked."""
    from vyomai_amd import ops
    N, K = dy.shape[1], x.shape[1]
    cols = [0, *bounds, N]
    bufs, dA, dB = [], [], []
    for p, r in enumerate(ranks):
        if r is None:
            dA.append(None)
            dB.append(None)
            continue
        fa, va = guarded((r, K), NAN if onto is None else onto)
        fb, vb = guarded((cols[p + 1] - cols[p], r), NAN if onto is None else onto)
        bufs += [fa, fb]
        dA.append(va)
        dB.append(vb)
    ops.lora_wgrad(dy.to(DEV), u.to(DEV), x.to(DEV), t.to(DEV), dA, dB, bounds, r_pad, alpha, accumulate=onto is not None,
                   name="test")
    torch.cuda.synchronize()
    for f in bufs:
        assert bool((f[:GUARD] == 7.0).all()) and bool((f[-GUARD:] == 7.0).all()), "a guard element was written"
    return [None if a is None else a.cpu() for a in dA], [None if b is None else b.cpu() for b in dB]


def restate(dy, u, x, t, bounds, r_pad, ranks, alpha, onto=0.0):
    N = dy.shape[1]
    cols = [0, *bounds, N]
    dA, dB = [], []
    for p, r in enumerate(ranks):
        if r is None:
            dA.append(None)
            dB.append(None)
            continue
        j0 = p * r_pad
        dB.append(onto + alpha * dy[:, cols[p]:cols[p + 1]].double().t() @ u[:, j0:j0 + r].double())
        dA.append(onto + alpha * t[:, j0:j0 + r].double().t() @ x.double())
    return dA, dB


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_exact_integer_data(dtype):
    """Integer dY and x in [-2, 2]; u and t with two non-zeros per row whose columns and values depend on the row and
    differ between u and t; alpha = 2: every product and every sum (|sum| <= 2 * 300 * 2 * 3) is exact, so the outputs
    are required bit for bit, overwriting and accumulating onto 3.0."""
    for K, N, bounds, r_pad, ranks in cases():
        R = len(ranks) * r_pad
        for M in MS:
            g = torch.Generator().manual_seed(K + N + M)
            dy = torch.randint(-2, 3, (M, N), generator=g).float()
            x = torch.randint(-2, 3, (M, K), generator=g).float()
            u, t = torch.zeros(M, R), torch.zeros(M, R)
            for m in range(M):
                u[m, (5 * m + 1) % R] += 1 + m % 3
                u[m, (11 * m + 4) % R] -= 2
                t[m, (7 * m + 2) % R] -= 1 + m % 2
                t[m, (3 * m + 5) % R] += 3
            u, t = poison(u, r_pad, ranks), poison(t, r_pad, ranks)
            args = (dy.to(dtype), u.to(dtype), x.to(dtype), t.to(dtype), bounds, r_pad, ranks, 2.0)
            for onto in (None, 3.0):
                got = run(*args, onto=onto)
                want = restate(*args, onto=onto or 0.0)
                for name, gs, ws in (("dA", got[0], want[0]), ("dB", got[1], want[1])):
                    for p, (a, w) in enumerate(zip(gs, ws)):
                        if w is None:
                            assert a is None
                            continue
                        assert M < 300 or bool((w != (onto or 0.0)).any()), "the case must produce something"
                        assert torch.equal(a.double(), w), (f"{name}[{p}] K {K} N {N} M {M} ranks {ranks} onto {onto}: "
                                                            f"{int((a.double() != w).sum())} elements differ")


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_random_data_against_fp64(dtype):
    atol, rtol = (2e-3, 1e-3) if dtype == BF else (8e-6, 1e-5)
    for K, N, bounds, r_pad, ranks in cases():
        R = len(ranks) * r_pad
        for M in MS:
            dy, x = rnd(M, N, seed=1).to(dtype), rnd(M, K, seed=2).to(dtype)
            u = poison(rnd(M, R, seed=3), r_pad, ranks).to(dtype)
            t = poison(rnd(M, R, seed=4), r_pad, ranks).to(dtype)
            args = (dy, u, x, t, bounds, r_pad, ranks, -0.75)
            for onto in (None, 3.0):
                got = run(*args, onto=onto)
                want = restate(*args, onto=onto or 0.0)
                for name, gs, ws in (("dA", got[0], want[0]), ("dB", got[1], want[1])):
                    for p, (a, w) in enumerate(zip(gs, ws)):
                        if w is not None:
                            check(a, w, atol * math.sqrt(M), rtol, f"{name}[{p}] K {K} N {N} M {M} ranks {ranks} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_two_runs_are_bitwise_equal_at_the_split(dtype):
    """Three chunks of M, the last one ragged: the partials are added in chunk order by the finish launch."""
    from vyomai_amd import ops
    for K, N, bounds, r_pad, ranks in cases()[:1] + cases()[-1:]:
        assert ops.lora_wgrad_chunk_rows(M_SPLIT, N, K) == 128 and ops.lora_wgrad_chunk_rows(M_SPLIT - 1, N, K) == 128
        R = len(ranks) * r_pad
        M = M_SPLIT
        dy, x = rnd(M, N, seed=5).to(dtype), rnd(M, K, seed=6).to(dtype)
        u, t = poison(rnd(M, R, seed=7), r_pad, ranks).to(dtype), poison(rnd(M, R, seed=8), r_pad, ranks).to(dtype)
        first = run(dy, u, x, t, bounds, r_pad, ranks, 0.75)
        second = run(dy, u, x, t, bounds, r_pad, ranks, 0.75)
        for a, b in zip(first[0] + first[1], second[0] + second[1]):
            assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M", [17, 33])
def test_data_gradient_products(M, dtype):
    """t = dY @ B per part through the block-diagonal transposed shadow, dX += alpha * t @ A through the transposed
    stacked A; a part without an adapter is all zero in both shadows."""
    from vyomai_amd import ops
    from vyomai_amd.lora_train import identity_tiles
    alpha = 1.5
    for K, N, bounds, r_pad, ranks in ((64, 64, (16, 32), 32, (32, None, 8)), (512, 1024, (), 64, (40,))):
        cols = [0, *bounds, N]
        R = len(ranks) * r_pad
        Bt, At = torch.zeros(R, N), torch.zeros(K, R)
        for p, r in enumerate(ranks):
            if r is None:
                continue
            b = rnd(cols[p + 1] - cols[p], r, seed=10 + p, scale=1 / math.sqrt(r))         # lora_b (out, rank)
            a = rnd(r, K, seed=20 + p, scale=1 / math.sqrt(K))                              # lora_a (rank, in)
            Bt[p * r_pad:p * r_pad + r, cols[p]:cols[p + 1]] = b.t()
            At[:, p * r_pad:p * r_pad + r] = a.t()
        Bt, At = Bt.to(dtype), At.to(dtype)
        dy, dx0 = rnd(M, N, seed=1).to(dtype), rnd(M, K, seed=2).to(dtype)
        tiles = identity_tiles(M)
        dx = dx0.to(DEV)
        t = ops.lora_dgrad_(dx, dy.to(DEV), Bt.to(DEV), At.to(DEV), torch.tensor([alpha], device=DEV), tiles.to(DEV),
                            tiles.shape[0], name="test")
        want_t = dy.double() @ Bt.double().t()
        want_dx = dx0.double() + alpha * want_t.to(dtype).double() @ At.double().t()
        bars = (3e-2, 1e-2) if dtype == BF else (1e-5, 1e-5)
        check(t, want_t, *bars, f"t M {M} K {K} N {N} {dtype}")
        check(dx, want_dx, *bars, f"dX M {M} K {K} N {N} {dtype}")
        assert bool((dx.cpu() != dx0).any())
        only_t = ops.lora_dgrad_(None, dy.to(DEV), Bt.to(DEV), At.to(DEV), torch.tensor([alpha], device=DEV),
                                 tiles.to(DEV), tiles.shape[0], name="test")
        assert torch.equal(only_t, t)
