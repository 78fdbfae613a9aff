"""The training path's streaming kernels (vy_misc.hip) at every instantiation, against the fp64 references and bars of
tests/stream_cases.py: LayerNorm forward and backward with the slab column sums, token embedding, the two transposes, the
fp32/bf16 cast, AdamW and vy_sumsq.  Entry points whose ops.* wrapper allocates a contiguous output are called through
_lib.call with padded buffers; every padded output is filled with a sentinel first, and the pad columns and the rows past
M must still hold it afterwards.  Each case prints its worst error next to its bar.  The same tables run through fp32
restatements with faults switched in on the CPU (tests/test_stream_kernels_cpu.py)."""
import pytest
import torch

from tests import stream_cases as S
from tests.test_kernels_gpu import check, check_exact, ints, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = S.BF, S.F32
IDS = [S.tname(t) for t in S.DTYPES]


def _lib():
    from vyomai_amd import _lib
    return _lib


def _ops():
    from vyomai_amd import ops
    return ops


def _st():
    return torch.cuda.current_stream().cuda_stream


def held(got, want, atol, rtol, what):
    """Prints the worst error against the bar atol + rtol |want|, then check()."""
    err = float((got.detach().double().cpu() - want.double()).abs().max())
    print(f"  {what}: max err {err:.3e}, worst err / bar {S.worst_ratio(got, want, S.linear_bar(want, atol, rtol)):.3f} "
          f"(bar {atol:g} + {rtol:g} |want|)")
    check(got, want, atol, rtol, what)


def held_to(got, want, bar, what):
    """The same for a bar given per element."""
    worst = S.worst_ratio(got, want, bar)
    print(f"  {what}: max err {float((got.detach().double().cpu() - want.double()).abs().max()):.3e}, "
          f"worst err / bar {worst:.3f}")
    assert worst <= 1.0, f"{what}: worst err / bar {worst:.3f}"


def in_pad(t, pad):
    """t (M, N) on the CPU -> a device view [:, :N] of an (M, N + pad) buffer (the pad holds the sentinel)."""
    M, N = t.shape
    buf = torch.full((M, N + pad), S.SENTINEL, dtype=t.dtype, device=DEV)
    buf[:, :N] = t.to(DEV)
    return buf[:, :N]


def out_pad(M, N, pad, dtype):
    """-> an (M + 1, N + pad) device buffer of sentinels: the output view is [:M, :N]."""
    return torch.full((M + 1, N + pad), S.SENTINEL, dtype=dtype, device=DEV)


def sentinel_intact(buf, M, N, what):
    assert bool((buf[:M, N:] == S.SENTINEL).all()), f"{what}: pad columns written"
    assert bool((buf[M:] == S.SENTINEL).all()), f"{what}: rows past M written"


def bits16(t):
    return t.contiguous().view(torch.int16)


# ---- 1. LayerNorm forward ---------------------------------------------------------------------------------------------
def ln_fwd_launch(x, gamma, beta, pads=(0, 0), stats=True):
    """vy_layernorm_fwd on buffers padded by pads = (of x, of y) elements -> y (M, N), mean, rstd (M) (None without
    stats); the sentinels are checked."""
    L = _lib()
    M, N = x.shape
    xv, yb = in_pad(x, pads[0]), out_pad(M, N, pads[1], x.dtype)
    g, b = gamma.to(DEV), beta.to(DEV)
    mean = torch.full((M + 1,), S.SENTINEL, device=DEV)
    rstd = torch.full((M + 1,), S.SENTINEL, device=DEV)
    L.call("vy_layernorm_fwd", xv.data_ptr(), N + pads[0], g.data_ptr(), b.data_ptr(), yb.data_ptr(), N + pads[1],
           mean.data_ptr() if stats else None, rstd.data_ptr() if stats else None, M, N, S.EPS, L.dtype_code(x.dtype), _st())
    torch.cuda.synchronize()
    sentinel_intact(yb, M, N, "y")
    tail = slice(M, None) if stats else slice(None)
    assert bool((mean[tail] == S.SENTINEL).all()) and bool((rstd[tail] == S.SENTINEL).all()), "mean / rstd past M written"
    return yb[:M, :N], (mean[:M] if stats else None), (rstd[:M] if stats else None)


def ln_fwd_params():
    out = []
    for dtype in S.DTYPES:
        for regime in S.REGIMES:
            for N in (S.LN_FWD_WIDTHS if regime == "plain" else S.LN_FWD_OFFSET_WIDTHS)[dtype]:
                out.append(pytest.param(dtype, regime, N, id=f"{S.tname(dtype)}-{regime}-{N}"))
    return out


@pytest.mark.parametrize("dtype,regime,N", ln_fwd_params())
def test_layernorm_fwd(dtype, regime, N):
    """layernorm_fwd_kernel<T, CH> at both sides of every CH boundary, 5 and 7 rows; y, mean and rstd against fp64.  The
    strided width also runs with ldx = N + VEC and ldy = N + 2 VEC, another one without the statistics pointers.  The
    small and constant regimes are the ones a dropped eps shows in; a constant row gives y = beta."""
    print(f"{S.tname(dtype)} {regime} N={N}: layernorm_fwd_kernel<{S.tname(dtype)}, {S.dispatch_chunks(N, dtype, 16)}>")
    for M in S.LN_FWD_ROWS:
        x, g, b = S.ln_fwd_inputs(dtype, regime, M, N)
        want_y, want_mean, want_rstd = S.ln_fwd_reference(x, g, b)
        y_bar = S.ln_fwd_y_bar(dtype, regime, g, want_y, want_mean, want_rstd)
        runs = [((0, 0), True)]
        if regime == "plain" and N == S.LN_FWD_STRIDED[dtype]:
            runs.append((tuple(p * S.VEC[dtype] for p in S.LN_FWD_PADS), True))
        if regime == "plain" and N == S.LN_FWD_NO_STATS[dtype]:
            runs.append(((0, 0), False))
        for pads, stats in runs:
            y, mean, rstd = ln_fwd_launch(x, g, b, pads, stats)
            what = f"M={M} pads={pads}"
            held_to(y, want_y, y_bar, "y " + what)
            if stats:
                held(mean, want_mean, *S.STAT_BAR, "mean " + what)
                held(rstd, want_rstd, *S.STAT_BAR, "rstd " + what)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_layernorm_fwd_refusals(dtype):
    """One chunk past the widest instantiation: "too wide".  A width that is no multiple of the 16-byte chunk: "multiples
    of".  Both before any launch: the output keeps the sentinel."""
    L = _lib()
    for N, msg in ((S.LN_FWD_TOO_WIDE[dtype], "too wide"), (S.VEC[dtype] + S.VEC[dtype] // 2, "multiples of")):
        x = torch.ones(5, N, dtype=dtype, device=DEV)
        w = torch.ones(N, dtype=dtype, device=DEV)
        y = torch.full((5, N), S.SENTINEL, dtype=dtype, device=DEV)
        with pytest.raises(L.VyomHipError, match=msg):
            L.call("vy_layernorm_fwd", x.data_ptr(), N, w.data_ptr(), w.data_ptr(), y.data_ptr(), N, None, None, 5, N, S.EPS,
                   L.dtype_code(dtype), _st())
        torch.cuda.synchronize()
        assert bool((y == S.SENTINEL).all())


# ---- 2. LayerNorm backward --------------------------------------------------------------------------------------------
def ln_bwd_launch(case, dgamma, dbeta, accumulate, pads=(0, 0, 0)):
    """vy_layernorm_bwd on buffers padded by pads = (of dy, of x, of dx) elements -> dx (M, N); dgamma / dbeta are written
    in place; the sentinels are checked and the inputs must keep their bits."""
    L = _lib()
    dy, x, gamma, mean, rstd = case
    M, N = x.shape
    WB = L.load().vy_layernorm_bwd_ws_rows(M)
    assert WB == S.ln_bwd_ws_rows(M)
    dv, xv, dxb = in_pad(dy, pads[0]), in_pad(x, pads[1]), out_pad(M, N, pads[2], x.dtype)
    g, mu, rs = gamma.to(DEV), mean.to(DEV), rstd.to(DEV)
    ws = torch.empty(2 * WB * N, dtype=F32, device=DEV)
    L.call("vy_layernorm_bwd", dv.data_ptr(), N + pads[0], xv.data_ptr(), N + pads[1], g.data_ptr(), mu.data_ptr(), rs.data_ptr(),
           dxb.data_ptr(), N + pads[2], dgamma.data_ptr(), dbeta.data_ptr(), 1.0 if accumulate else 0.0, ws.data_ptr(), M, N,
           L.dtype_code(x.dtype), _st())
    torch.cuda.synchronize()
    sentinel_intact(dxb, M, N, "dx")
    assert torch.equal(dv.cpu(), dy) and torch.equal(xv.cpu(), x), "an input was written"
    return dxb[:M, :N]


def ln_bwd_params():
    return [pytest.param(dtype, M, N, id=f"{S.tname(dtype)}-{M}x{N}") for dtype in S.DTYPES for M, N in S.ln_bwd_cases(dtype)]


def bwd_pads(dtype, M, N):
    """The pads (of dy, of x, of dx) a case runs with: none, and on the strided case a different one per operand."""
    strided = (tuple(p * S.VEC[dtype] for p in S.LN_BWD_PADS),) if (M, N) == S.LN_BWD_STRIDED else ()
    return ((0, 0, 0),) + strided


@pytest.mark.parametrize("dtype,M,N", ln_bwd_params())
def test_layernorm_bwd_vs_fp64(dtype, M, N):
    """layernorm_bwd_kernel<T, CH> + vy_colsum with statistics computed in fp64 (not by the forward kernel): dx, dgamma
    and dbeta against fp64; a second run gives the same bits; accumulate adds onto them."""
    case = S.ln_bwd_inputs(dtype, M, N)
    want_dx, want_dg, want_db = S.ln_bwd_reference(*case)
    print(f"{S.tname(dtype)} {M}x{N}: layernorm_bwd_kernel<{S.tname(dtype)}, {S.dispatch_chunks(N, dtype, 4)}>, "
          f"{S.ln_bwd_ws_rows(M)} slab rows in {S.ln_colsum_slices(S.ln_bwd_ws_rows(M))} slice(s)")
    for pad in bwd_pads(dtype, M, N):
        dg = torch.full((N,), S.SENTINEL, device=DEV)
        db = torch.full((N,), S.SENTINEL, device=DEV)
        dx = ln_bwd_launch(case, dg, db, False, pad)
        held(dx, want_dx, *S.elementwise_bars(dtype), f"dx pad={pad}")
        held(dg, want_dg, *S.colsum_bars(dtype, M), f"dgamma pad={pad}")
        held(db, want_db, *S.colsum_bars(dtype, M), f"dbeta pad={pad}")
        dg2, db2 = torch.zeros_like(dg), torch.zeros_like(db)
        dx2 = ln_bwd_launch(case, dg2, db2, False, pad)
        assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db), "a second run gave other bits"
        ln_bwd_launch(case, dg2, db2, True, pad)
        assert torch.equal(dg2, dg + dg) and torch.equal(db2, db + db), "accumulate did not add onto the sums"


@pytest.mark.parametrize("dtype,M,N", ln_bwd_params())
def test_layernorm_bwd_column_sums_exact_twin(dtype, M, N):
    """Integer x and dy, chosen statistics, gamma = 1: every term of dgamma is a multiple of 1/8 and every term of dbeta
    an integer, so the sums are exact in fp32 in any order.  A row dropped, duplicated or read with another row's
    statistics in the wave walk, the four-wave sum, the slices or the finish launch is a non-zero difference."""
    case = S.ln_twin_inputs(dtype, M, N)
    dy, x, _, mean, rstd = case
    want_dg, want_db = S.ln_twin_expected(dy, x, mean, rstd)
    for pad in bwd_pads(dtype, M, N):
        dg = torch.full((N,), S.SENTINEL, device=DEV)
        db = torch.full((N,), S.SENTINEL, device=DEV)
        ln_bwd_launch(case, dg, db, False, pad)
        check_exact(dg, want_dg, f"dgamma {M}x{N} pad={pad}")
        check_exact(db, want_db, f"dbeta {M}x{N} pad={pad}")
        dg.fill_(3.0)
        db.fill_(3.0)
        ln_bwd_launch(case, dg, db, True, pad)
        check_exact(dg, want_dg + 3.0, f"dgamma accumulated onto 3.0, {M}x{N} pad={pad}")
        check_exact(db, want_db + 3.0, f"dbeta accumulated onto 3.0, {M}x{N} pad={pad}")


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_layernorm_bwd_refusals(dtype):
    L = _lib()
    for N, msg in ((S.LN_BWD_TOO_WIDE[dtype], "too wide"), (S.VEC[dtype] + S.VEC[dtype] // 2, "multiples of")):
        t = torch.ones(5, N, dtype=dtype, device=DEV)
        dx = torch.full((5, N), S.SENTINEL, dtype=dtype, device=DEV)
        row = torch.ones(N, dtype=dtype, device=DEV)
        stat = torch.ones(5, device=DEV)
        dg = torch.full((N,), S.SENTINEL, device=DEV)
        ws = torch.empty(2 * S.ln_bwd_ws_rows(5) * N, device=DEV)
        with pytest.raises(L.VyomHipError, match=msg):
            L.call("vy_layernorm_bwd", t.data_ptr(), N, t.data_ptr(), N, row.data_ptr(), stat.data_ptr(), stat.data_ptr(),
                   dx.data_ptr(), N, dg.data_ptr(), dg.data_ptr(), 0.0, ws.data_ptr(), 5, N, L.dtype_code(dtype), _st())
        torch.cuda.synchronize()
        assert bool((dx == S.SENTINEL).all()) and bool((dg == S.SENTINEL).all())


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("M", S.LN_BWD_COLSUM_ROWS)
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_partial_plus_grouped_column_sums_give_the_bits_of_layernorm_bwd(dtype, M, acc):
    """vy_layernorm_bwd_partial followed by a ColSum entry of linear_wgrad_grouped == vy_layernorm_bwd, bit for bit, at 1,
    64, 65 and 512 slab rows."""
    ops = _ops()
    N = 768
    case = tuple(t.to(DEV) for t in S.ln_bwd_inputs(dtype, M, N))
    dg_ref = torch.full((N,), 3.0, device=DEV)
    db_ref = torch.full((N,), 3.0, device=DEV)
    dx_ref = ops.layernorm_bwd(*case, dg_ref, db_ref, accumulate=acc)
    dx, ws = ops.layernorm_bwd_partial(*case)
    assert ws.numel() == 2 * S.ln_bwd_ws_rows(M) * N
    dg = torch.full((N,), 3.0, device=DEV)
    db = torch.full((N,), 3.0, device=DEV)
    ops.linear_wgrad_grouped([ops.ColSum(ws, dg, db, acc, dtype)])
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref)
    assert torch.equal(dg, dg_ref), (dg - dg_ref).abs().max().item()
    assert torch.equal(db, db_ref), (db - db_ref).abs().max().item()


# ---- 4. embedding -----------------------------------------------------------------------------------------------------
def emb_fwd_launch(table, ids, err):
    """vy_embedding_fwd with a table row stride and an output row stride of d + VEC -> out (M, d)."""
    L = _lib()
    V, d = table.shape
    M, pad = ids.numel(), S.VEC[table.dtype]
    tv, ob = in_pad(table, pad), out_pad(M, d, pad, table.dtype)
    idd = ids.to(DEV)
    L.call("vy_embedding_fwd", tv.data_ptr(), d + pad, idd.data_ptr(), ob.data_ptr(), d + pad, M, d, V,
           None if err is None else err.data_ptr(), L.dtype_code(table.dtype), _st())
    torch.cuda.synchronize()
    sentinel_intact(ob, M, d, "embedding out")
    return ob[:M, :d].cpu()


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_embedding_fwd(dtype):
    for d in S.EMB_WIDTHS[dtype]:
        for V in S.EMB_VOCABS:
            table = rnd(V, d, seed=8).to(dtype)
            for M in S.EMB_ROWS:
                ids = S.emb_ids(M, V)
                err = torch.zeros(1, dtype=torch.int32, device=DEV)
                out = emb_fwd_launch(table, ids, err)
                assert torch.equal(out, table[ids]), (d, V, M)
                assert int(err.item()) == 0, (d, V, M)
                assert torch.equal(emb_fwd_launch(table, ids, None), table[ids]), (d, V, M)    # no flag pointer
                if M >= 5:                       # ids just outside the table: flagged, written as zeros, nothing else moves
                    bad = ids.clone()
                    bad[1], bad[3] = -1, V
                    out = emb_fwd_launch(table, bad, err)
                    assert int(err.item()) == 1, (d, V, M)
                    good = (bad >= 0) & (bad < V)
                    assert torch.equal(out[good], table[bad[good]]), (d, V, M)
                    assert bool((out[~good] == 0).all()) and int((~good).sum()) == 2, (d, V, M)


@pytest.mark.parametrize("padding_idx", [None, S.EMB_PADDING])
@pytest.mark.parametrize("pattern", ["dups", "same", "mixed"])
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_embedding_bwd_exact(dtype, pattern, padding_idx):
    """Integer gradients: the atomic sums are exact in any order.  dw starts at 3.0 with a row stride of d + 4; the
    padding row, the rows of skipped ids and the pad columns keep the 3.0."""
    ops = _ops()
    M, V = 500, 1031
    ids = S.emb_bwd_ids(pattern, M, V)
    for d in S.EMB_WIDTHS[dtype]:
        dout = ints(M, d, seed=9, lo=-2, hi=2).to(dtype)
        want, keep = S.emb_bwd_reference(dout, ids, V, padding_idx)
        assert float(want.abs().max()) < 2 ** 24
        dwb = torch.full((V, d + 4), 3.0, device=DEV)
        ops.embedding_bwd_(in_pad(dout, S.VEC[dtype]), ids.to(DEV), dwb[:, :d], padding_idx)
        torch.cuda.synchronize()
        check_exact(dwb[:, :d], want, f"dw {pattern} d={d} padding_idx={padding_idx} (row, column)")
        assert bool((dwb[:, d:] == 3.0).all()), "dw: pad columns written"
        untouched = torch.ones(V, dtype=torch.bool)
        untouched[ids[keep]] = False
        assert bool((dwb[untouched.to(DEV)] == 3.0).all())
        if padding_idx is not None:
            assert bool(untouched[padding_idx])
        if pattern == "same":
            assert int((~untouched).sum()) == 1 and float((want[V - 2] - 3.0).abs().max()) > 2      # 500 rows onto one


# ---- 5. transposes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", S.TRANSPOSE_SHAPES)
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_transpose_ragged_and_strided(dtype, R, C):
    """vy_transpose (the 32 x 33 LDS tile) on shapes that are no multiples of 32: the input a slice of a wider buffer, the
    output with a row stride of R + 3."""
    ops = _ops()
    wide = rnd(R, C + 5, seed=10).to(dtype).to(DEV)
    src = wide[:, 2:2 + C]
    ob = torch.full((C + 1, R + 3), S.SENTINEL, dtype=dtype, device=DEV)
    ret = ops.transpose(src, out=ob[:C, :R])
    torch.cuda.synchronize()
    assert torch.equal(ret, src.t()), (R, C)
    sentinel_intact(ob, C, R, "transpose out")
    assert torch.equal(ops.transpose(src), src.t())          # the wrapper's own contiguous output


def _batch_pair(R, C, dtype, seed, offset_base=False):
    """(src, dst, dst buffer): dst is [:, :R] of a (C, R rounded up to 8) buffer of 7.0.  offset_base: the source starts one
    element into its buffer with a row stride of C: an aligned stride on a base that is not, the scalar path."""
    t = rnd(R, C, seed=seed).to(dtype)
    if offset_base:
        buf = torch.zeros(R * C + 8, dtype=dtype, device=DEV)
        src = buf[1:1 + R * C].view(R, C)
        src.copy_(t.to(DEV))
        assert src.data_ptr() % 16 != 0 and C % S.VEC[dtype] == 0
    else:
        src = t.to(DEV)
    ld = (R + 7) // 8 * 8
    dbuf = torch.full((C, ld), S.SENTINEL, dtype=dtype, device=DEV)
    return src, dbuf[:, :R], dbuf


BATCHES = {
    "five": [(R, C, False) for R, C in S.TRANSPOSE_BATCH_SHAPES],
    "offset_base": [(70, 200, True), (768, 768, False), (1031, 768, True)],
    "one": [(100, 257, False)],
    "forty_small": [(1 + (7 * i) % 90, 1 + (11 * i) % 130, False) for i in range(40)],     # 1..6 tiles each: the bisection
}


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_transpose_batched_cases(dtype, batch):
    ops = _ops()
    trio = [_batch_pair(R, C, dtype, seed=20 + i, offset_base=off) for i, (R, C, off) in enumerate(BATCHES[batch])]
    tb = ops.TransposeBatch([(src, dst) for src, dst, _ in trio])
    assert tb.n == len(trio) and tb.total == sum(-(-s.shape[0] // 64) * -(-s.shape[1] // 64) for s, _, _ in trio)
    tb.run()
    torch.cuda.synchronize()
    for src, dst, dbuf in trio:
        R, C = src.shape
        assert torch.equal(dst, src.t()), (batch, R, C)
        assert bool((dbuf[:, R:] == S.SENTINEL).all()), ("pad columns written", batch, R, C)


# ---- 6. cast ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,offset", [(n, 0) for n in S.CAST_SIZES] + [(1023, 1), (S.CAST_SIZES[-1], 1)])
def test_cast_fp32_to_bf16_bit_for_bit(n, offset):
    """vy_cast fp32 -> bf16 == torch's cast (round to nearest even), bit for bit: unit-normal data, the values halfway
    between two bf16 neighbours (both parities, both signs), +-0, +-inf, the largest finite fp32.  NaN is compared with
    isnan.  fp32 denormals are left out: whether they are flushed is not pinned here.  offset 1: the source view starts
    one element into its buffer."""
    ops = _ops()
    src = S.cast_source(n)
    buf = torch.zeros(n + 1, dtype=F32, device=DEV)
    sv = buf[offset:offset + n]
    sv.copy_(src.to(DEV))
    db = torch.full((n + 8,), S.SENTINEL, dtype=BF, device=DEV)
    ops.cast(sv, db[:n])
    torch.cuda.synchronize()
    got, want = db[:n].cpu(), src.to(BF)
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(bits16(got)[~nan], bits16(want)[~nan]), int((bits16(got) != bits16(want))[~nan].sum())
    assert bool((db[n:] == S.SENTINEL).all()), "written past n"


def test_cast_bf16_to_fp32_every_pattern():
    ops = _ops()
    src = S.all_bf16_patterns()
    db = torch.full((65536 + 8,), S.SENTINEL, dtype=F32, device=DEV)
    ops.cast(src.to(DEV), db[:65536])
    torch.cuda.synchronize()
    got, want = db[:65536].cpu(), src.float()
    nan = torch.isnan(want)
    assert int(nan.sum()) == 2 * 127 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])
    assert bool((db[65536:] == S.SENTINEL).all())


def test_cast_refuses_an_unsupported_pair():
    ops = _ops()
    a = torch.ones(8, device=DEV)
    b = torch.full((8,), S.SENTINEL, device=DEV)
    with pytest.raises(_lib().VyomHipError, match="unsupported"):
        ops.cast(a, b)
    torch.cuda.synchronize()
    assert bool((b == S.SENTINEL).all())


# ---- 7. AdamW and sumsq -----------------------------------------------------------------------------------------------
def adamw_state(n, seed=0):
    """p, g, m, v (fp32, CPU); m and v as after earlier steps (v >= 0)."""
    return rnd(n, seed=seed + 1), rnd(n, seed=seed + 2), 0.1 * rnd(n, seed=seed + 3), 0.01 * rnd(n, seed=seed + 4).pow(2)


def guarded(t, dtype=None):
    """t (n) -> a device view [:n] of an (n + 4) buffer whose tail holds the sentinel."""
    buf = torch.full((t.numel() + 4,), S.SENTINEL, dtype=dtype or t.dtype, device=DEV)
    buf[:t.numel()] = t.to(DEV)
    return buf[:t.numel()], buf


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32 if a.dtype == F32 else torch.int16),
                       b.contiguous().view(torch.int32 if b.dtype == F32 else torch.int16))


@pytest.mark.parametrize("n", S.ADAMW_SIZES)
def test_adamw_three_steps_vs_fp64(n):
    """adamw_kernel against an fp64 restatement of its formula over three consecutive steps, with and without decay, from
    step 1 and from step 1000, the gradient scale on the host and on the device; the bf16 shadow is torch's cast of the
    returned p, bit for bit."""
    ops = _ops()
    print(f"n={n}: paths {sorted(S.adamw_paths(n))}")
    p0, g0, m0, v0 = adamw_state(n)
    for wd in (0.0, 0.01):
        for step0 in (1, 1000):
            for on_device in (False, True):
                (p, pbuf), (m, mbuf), (v, vbuf) = guarded(p0), guarded(m0), guarded(v0)
                pb, pbbuf = guarded(torch.zeros(n), BF)
                rp, rm, rv = p0.double(), m0.double(), v0.double()
                sd = torch.tensor([0.37], dtype=F32, device=DEV) if on_device else None
                for k in range(3):
                    g = g0 * (k + 1)
                    ops.adamw_step(p, g.to(DEV), m, v, pb, S.ADAMW_HP["lr"], S.ADAMW_HP["beta1"], S.ADAMW_HP["beta2"],
                                   S.ADAMW_HP["eps"], wd, step0 + k, 1.0 if on_device else 0.37, scale_dev=sd)
                    rp, rm, rv = S.adamw_reference(rp, g.double(), rm, rv, weight_decay=wd, step=step0 + k, scale=0.37,
                                                   **S.ADAMW_HP)
                    assert torch.equal(bits16(pb), bits16(p.to(BF))), "the shadow is not the cast of p"
                what = f"wd={wd} step0={step0} scale on the {'device' if on_device else 'host'}"
                for name, got, want in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
                    held(got, want, *S.ADAMW_BAR, f"{name} {what}")
                for b in (pbuf, mbuf, vbuf, pbbuf):
                    assert bool((b[n:] == S.SENTINEL).all()), "written past n"


@pytest.mark.parametrize("n", [5, 1023, 100003])
def test_adamw_gate(n):
    """gate = 0: p, m, v and the shadow keep their bits.  gate = 1: the bits of the ungated launch."""
    ops = _ops()
    p0, g0, m0, v0 = adamw_state(n, seed=10)
    hp = (S.ADAMW_HP["lr"], S.ADAMW_HP["beta1"], S.ADAMW_HP["beta2"], S.ADAMW_HP["eps"], 0.01, 3)
    shadow0 = torch.full((n,), 5.0, dtype=BF)
    runs = {}
    for name, gate in (("plain", None), ("open", 1.0), ("shut", 0.0)):
        p, m, v, pb = (t.clone().to(DEV) for t in (p0, m0, v0, shadow0))
        gt = None if gate is None else torch.tensor([gate], dtype=F32, device=DEV)
        ops.adamw_step(p, g0.to(DEV), m, v, pb, *hp, gate=gt)
        torch.cuda.synchronize()
        runs[name] = (p.cpu(), m.cpu(), v.cpu(), pb.cpu())
    for got, before in zip(runs["shut"], (p0, m0, v0, shadow0)):
        assert same_bits(got, before), "gate = 0 changed something"
    for got, want in zip(runs["open"], runs["plain"]):
        assert same_bits(got, want), "gate = 1 differs from the ungated launch"
    assert not same_bits(runs["plain"][0], p0)


def test_adamw_grid_stride_loop():
    """n = 8192 * 1024 + 5: more elements than the capped grid covers in one pass.  A slice at the front, a slice across
    8192 * 1024 and the tail against fp64; the shadow against torch's cast over the whole array."""
    ops = _ops()
    n, cut = S.ADAMW_STRIDE_N, 8192 * 1024
    p0, g0, m0, v0 = adamw_state(n, seed=20)
    p, m, v, pb = p0.clone().to(DEV), m0.clone().to(DEV), v0.clone().to(DEV), torch.zeros(n, dtype=BF, device=DEV)
    ops.adamw_step(p, g0.to(DEV), m, v, pb, S.ADAMW_HP["lr"], S.ADAMW_HP["beta1"], S.ADAMW_HP["beta2"], S.ADAMW_HP["eps"],
                   0.01, 2)
    torch.cuda.synchronize()
    assert torch.equal(bits16(pb), bits16(p.to(BF)))
    for name, sl in (("front", slice(0, 4096)), ("across the cap", slice(cut - 2048, cut + 2048)), ("tail", slice(n - 64, n))):
        want = S.adamw_reference(p0[sl].double(), g0[sl].double(), m0[sl].double(), v0[sl].double(), weight_decay=0.01,
                                 step=2, scale=1.0, **S.ADAMW_HP)
        for what, got, w in zip("pmv", (p, m, v), want):
            held(got[sl], w, *S.ADAMW_BAR, f"{what} {name}")


@pytest.mark.parametrize("n", S.SUMSQ_SIZES)
def test_sumsq_exact_on_integers(n):
    ops = _ops()
    x = ints(n, seed=11)
    want = float(x.double().pow(2).sum())
    assert want < 2 ** 24
    assert float(ops.sumsq(x.to(DEV))) == want, n


def test_sumsq_same_bits_twice_and_refuses_an_unaligned_view():
    ops = _ops()
    x = rnd(S.SUMSQ_SIZES[-1], seed=12).to(DEV)
    a, b = ops.sumsq(x).clone(), ops.sumsq(x).clone()
    assert same_bits(a.reshape(1), b.reshape(1))
    want = float(x.double().pow(2).sum())
    assert abs(float(a) - want) <= 2e-6 * want          # test_sumsq_and_device_scaled_adamw's bar
    with pytest.raises(_lib().VyomHipError, match="16-byte aligned"):
        ops.sumsq(x[1:])
