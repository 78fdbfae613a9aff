"""Guard of tests/stream_cases.py: fp32 torch restatements of the LayerNorm kernels of vy_misc.hip, with the faults the
special regimes were built for switched in.  No kernel runs here.

Forward: the two-pass form of layernorm_fwd_kernel (per-lane partial sums over the lane's chunks, a butterfly over the 64
lanes, the variance about the mean) and a one-pass variant (E[x^2] - mean^2).  Backward: layernorm_bwd_kernel's wave walk
(wave w takes rows w, w + W, ...), the four-wave sum of a workgroup, the slab and the sliced column sums of
vy_colsum, with two faults: the last row of a walk of more than one row is skipped; row r uses the statistics of row
r + W.  Asserted: the faithful restatements sit at no more than half of every bar on every case of the tables, the
one-pass variant breaks the rstd bar on every offset case and none on the others, a dropped eps breaks the small and the
constant regime and passes on plain and offset data, each backward fault breaks the exact twin wherever a wave walks more
than one row, x read with dy's row stride shows only when every operand has a different pad, and the twin's expected values
are the same in fp64 and fp32."""
import pytest
import torch

from tests import stream_cases as S

BF, F32 = S.BF, S.F32
IDS = [S.tname(t) for t in S.DTYPES]


# ---- restatements -------------------------------------------------------------------------------------------------------
def lane_sums(t, dtype):
    """t (M, N) fp32 -> (M, 64): lane l adds the elements of its chunks l, l + 64, ... in the kernels' order."""
    M, N = t.shape
    vec = S.VEC[dtype]
    ch = -(-N // (64 * vec))
    pad = torch.zeros(M, ch * 64 * vec)
    pad[:, :N] = t                                  # a missing chunk adds 0.0: exact
    v = pad.view(M, ch, 64, vec)
    s = torch.zeros(M, 64)
    for c in range(ch):
        for e in range(vec):
            s = s + v[:, c, :, e]
    return s


def wave_sum(s):
    """vy_wave_sum: xor butterfly over the 64 lanes -> (M,)."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def ln_fwd_restated(x, gamma, beta, dtype, one_pass=False, no_eps=False):
    v, N = x.float(), x.shape[1]
    mean = wave_sum(lane_sums(v, dtype)) / N
    if one_pass:
        var = (wave_sum(lane_sums(v * v, dtype)) / N - mean * mean).clamp_min(0.0)
    else:
        d = v - mean[:, None]
        var = wave_sum(lane_sums(d * d, dtype)) / N
    rstd = 1.0 / torch.sqrt(var if no_eps else var + S.EPS)
    y = ((v - mean[:, None]) * rstd[:, None] * gamma.float() + beta.float()).to(dtype)
    return y, mean, rstd


BWD_FAULTS = ("skip_last", "stats_ahead")


def read_with_stride(t, ld, read_ld):
    """t (M, N) laid out with a row stride of ld in a sentinel-filled buffer, read back with a row stride of read_ld."""
    M, N = t.shape
    buf = torch.full((M, ld), S.SENTINEL, dtype=t.dtype)
    buf[:, :N] = t
    return torch.as_strided(buf.reshape(-1), (M, N), (read_ld, 1))


def colsum_restated(slab, out, acc):
    """vy_colsum on a [WB, N] slab: slices of rows, four row groups a slice summed in row order, ((p0 + p1) + p2) + p3,
    the slices in slice order."""
    WB, N = slab.shape
    slices = S.ln_colsum_slices(WB)
    rps = -(-WB // slices)
    parts = []
    for w0 in range(0, WB, rps):
        w1 = min(WB, w0 + rps)
        p = []
        for g in range(4):
            a = torch.zeros(N)
            for w in range(w0 + g, w1, 4):
                a = a + slab[w]
            p.append(a)
        parts.append(((p[0] + p[1]) + p[2]) + p[3])
    base = out if acc else torch.zeros(N)
    if slices == 1:
        return base + parts[0]
    a = torch.zeros(N)
    for part in parts:
        a = a + part
    return base + a


def ln_bwd_restated(dy, x, gamma, mean, rstd, dtype, fault=None, dgamma=None, dbeta=None, pads=None):
    """-> dx (cast to dtype), dgamma, dbeta; dgamma / dbeta given: accumulated onto.  pads (of dy, of x, of dx, in chunks):
    the operands sit in buffers with those row strides; the fault swapped_stride reads x with dy's."""
    M, N = x.shape
    if pads is not None:
        lddy, ldx = N + pads[0] * S.VEC[dtype], N + pads[1] * S.VEC[dtype]
        dy, x = read_with_stride(dy, lddy, lddy), read_with_stride(x, ldx, lddy if fault == "swapped_stride" else ldx)
    WB = S.ln_bwd_ws_rows(M)
    W = 4 * WB
    xv, dv, g = x.float(), dy.float(), gamma.float()
    dg, db, dx = torch.zeros(W, N), torch.zeros(W, N), torch.zeros(M, N)
    for r0 in range(0, M, W):
        rows = torch.arange(r0, min(M, r0 + W))
        n = rows.numel()
        srow = torch.where(rows + W < M, rows + W, rows) if fault == "stats_ahead" else rows
        mu, rs = mean[srow][:, None], rstd[srow][:, None]
        xh = (xv[rows] - mu) * rs
        gy = dv[rows] * g
        s1 = (wave_sum(lane_sums(gy, dtype)) / N)[:, None]
        s2 = (wave_sum(lane_sums(gy * xh, dtype)) / N)[:, None]
        o = rs * (gy - s1 - xh * s2)
        live = torch.ones(n, dtype=torch.bool)
        if fault == "skip_last" and r0 > 0:
            live = rows + W < M
        keep = live[:, None].float()
        dx[rows] = o * keep
        dg[:n] = dg[:n] + dv[rows] * xh * keep
        db[:n] = db[:n] + dv[rows] * keep
    slab_g, slab_b = dg.view(WB, 4, N), db.view(WB, 4, N)
    slab_g = ((slab_g[:, 0] + slab_g[:, 1]) + slab_g[:, 2]) + slab_g[:, 3]
    slab_b = ((slab_b[:, 0] + slab_b[:, 1]) + slab_b[:, 2]) + slab_b[:, 3]
    acc = dgamma is not None
    return dx.to(dtype), colsum_restated(slab_g, dgamma, acc), colsum_restated(slab_b, dbeta, acc)


# ---- the tables reach what they were written for ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_tables_cover_every_instantiation(dtype):
    vec = S.VEC[dtype]
    fwd = [S.dispatch_chunks(N, dtype, 16) for N in S.LN_FWD_WIDTHS[dtype]]
    assert set(fwd) == {1, 2, 4, 8, 16}, fwd
    for ch in (1, 2, 4, 8):              # both sides of every boundary
        assert 64 * ch * vec in S.LN_FWD_WIDTHS[dtype] and 64 * ch * vec + vec in S.LN_FWD_WIDTHS[dtype], ch
    assert S.dispatch_chunks(64 * 16 * vec, dtype, 16) == 16 and 64 * 16 * vec in S.LN_FWD_WIDTHS[dtype]
    assert S.LN_FWD_TOO_WIDE[dtype] == 64 * 16 * vec + vec and S.dispatch_chunks(S.LN_FWD_TOO_WIDE[dtype], dtype, 16) is None
    assert {S.dispatch_chunks(N, dtype, 16) for N in S.LN_FWD_OFFSET_WIDTHS[dtype]} == {1, 2, 4, 8, 16}
    assert 768 in S.LN_FWD_OFFSET_WIDTHS[dtype]
    bwd = [S.dispatch_chunks(N, dtype, 4) for N in S.LN_BWD_WIDTHS[dtype]]
    assert set(bwd) == {1, 2, 4}, bwd
    for ch in (1, 2):
        assert 64 * ch * vec in S.LN_BWD_WIDTHS[dtype] and 64 * ch * vec + vec in S.LN_BWD_WIDTHS[dtype], ch
    assert max(S.LN_BWD_WIDTHS[dtype]) == 64 * 4 * vec and S.LN_BWD_TOO_WIDE[dtype] == 64 * 4 * vec + vec
    assert S.dispatch_chunks(S.LN_BWD_TOO_WIDE[dtype], dtype, 4) is None
    cases = S.ln_bwd_cases(dtype)
    Ns = S.LN_BWD_WIDTHS[dtype]
    assert all((M, N) in cases for N in Ns for M in (5, 257))
    assert all((M, N) in cases for M in S.LN_BWD_ROWS for N in (768, min(Ns), max(Ns)))
    assert S.LN_BWD_STRIDED in cases
    assert len(set(S.LN_BWD_PADS)) == 3 and len(set(S.LN_FWD_PADS)) == 2 and 0 not in S.LN_BWD_PADS + S.LN_FWD_PADS
    assert {S.dispatch_chunks(N, dtype, 16) for N in S.LN_FWD_OFFSET_WIDTHS[dtype]} == {1, 2, 4, 8, 16}      # every regime
    assert all((g, M, N) in S.ln_fwd_cases(dtype) for g in S.REGIMES[1:] for N in S.LN_FWD_OFFSET_WIDTHS[dtype] for M in S.LN_FWD_ROWS)


def test_row_counts_cover_the_wave_walk_and_the_column_sum_slices():
    rows = {M: S.ln_bwd_ws_rows(M) for M in S.LN_BWD_ROWS}
    assert rows[1] == 1 and rows[3] == 1 and rows[5] == 2            # waves without a row; a ragged second workgroup
    assert (rows[252], rows[253], rows[257]) == (63, 64, 65)         # both sides of vy_ln_colsum_slices' threshold
    assert {S.ln_colsum_slices(wb) for wb in rows.values()} == {1, 16}
    assert S.ln_colsum_slices(63) == 1 and S.ln_colsum_slices(64) == 16
    rps = -(-65 // 16)
    assert rps == 5 and len(range(0, 65, rps)) == 13                 # 65 slab rows: three of the sixteen slices are empty
    assert rows[2049] == 512 and rows[4100] == 512                   # the cap: 2048 waves
    assert 2049 - 4 * 512 == 1 and -(-4100 // 2048) == 3             # wave 0 alone walks on; waves 0..3 take three rows
    for M in S.LN_BWD_COLSUM_ROWS:
        assert M in S.LN_BWD_ROWS


def test_adamw_sizes_reach_the_vector_path_and_the_tail():
    paths = {n: S.adamw_paths(n) for n in S.ADAMW_SIZES}
    assert {"tail"} in paths.values() and {"vector"} in paths.values() and {"vector", "tail"} in paths.values(), paths
    assert S.adamw_paths(S.ADAMW_STRIDE_N) == {"vector", "tail"} and S.ADAMW_STRIDE_N > 8192 * 1024
    assert S.CAST_SIZES[-1] > 4096 * 1024 and -(-S.SUMSQ_SIZES[-1] // 8192) > 1024


# ---- LayerNorm forward ------------------------------------------------------------------------------------------------
def fwd_ratios(dtype, regime, M, N, one_pass, no_eps=False):
    x, g, b = S.ln_fwd_inputs(dtype, regime, M, N)
    y, mean, rstd = S.ln_fwd_reference(x, g, b)
    gy, gm, gr = ln_fwd_restated(x, g, b, dtype, one_pass, no_eps)
    if not (torch.isfinite(gy.float()).all() and torch.isfinite(gr).all()):
        return (float("inf"),) * 3
    return (S.worst_ratio(gy, y, S.ln_fwd_y_bar(dtype, regime, g, y, mean, rstd)),
            S.worst_ratio(gm, mean, S.linear_bar(mean, *S.STAT_BAR)),
            S.worst_ratio(gr, rstd, S.linear_bar(rstd, *S.STAT_BAR)))


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_two_pass_forward_sits_at_half_of_every_bar(dtype):
    for regime, M, N in S.ln_fwd_cases(dtype):
        ry, rm, rr = fwd_ratios(dtype, regime, M, N, one_pass=False)
        print(f"{regime} {M}x{N} {S.tname(dtype)}: err / bar y {ry:.3f} mean {rm:.3f} rstd {rr:.4f}")
        assert max(ry, rm, rr) <= 0.5, (regime, M, N, ry, rm, rr)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_one_pass_variance_breaks_the_offset_regime_only(dtype):
    for regime, M, N in S.ln_fwd_cases(dtype):
        ry, rm, rr = fwd_ratios(dtype, regime, M, N, one_pass=True)
        print(f"{regime} {M}x{N} {S.tname(dtype)} one pass: err / bar y {ry:.3f} mean {rm:.3f} rstd {rr:.3f}")
        if regime == "offset":
            assert rr > 1.0, (M, N, rr)
        else:
            assert max(ry, rm, rr) <= 1.0, (M, N, ry, rm, rr)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_dropped_eps_breaks_the_small_and_constant_regimes_only(dtype):
    """Without eps rstd nearly doubles on small data and is 1 / 0 on a constant row (y = 0 * inf); on plain and offset
    data, a variance of 4 beside eps = 1e-5, it passes every bar at every width of 256 and more: why the two regimes are
    there."""
    for regime, M, N in S.ln_fwd_cases(dtype):
        ry, rm, rr = fwd_ratios(dtype, regime, M, N, one_pass=False, no_eps=True)
        if regime == "small":
            assert ry > 1.0 and rr > 1.0, (M, N, ry, rr)
        elif regime == "constant":
            assert ry == float("inf"), (M, N, ry)
        elif N >= 256:      # (a row of 4 or 8 elements can have a variance small enough on its own for eps to show)
            assert max(ry, rm, rr) <= 1.0, (regime, M, N, ry, rm, rr)


def test_a_constant_row_gives_beta():
    for dtype in S.DTYPES:
        x, g, b = S.ln_fwd_inputs(dtype, "constant", 5, 768)
        assert bool((x == x[:, :1]).all()) and torch.equal(x.float(), x.to(BF).float()) and len(set(x[:, 0].tolist())) == 5
        y, mean, rstd = S.ln_fwd_reference(x, g, b)
        assert torch.equal(y, b.double().expand(5, 768)) and torch.equal(mean, x[:, 0].double())
        assert torch.equal(ln_fwd_restated(x, g, b, dtype)[0], b.expand(5, 768))


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_restated_backward_sits_at_half_of_every_bar(dtype):
    for M, N in S.ln_bwd_cases(dtype):
        case = S.ln_bwd_inputs(dtype, M, N)
        dx, dg, db = S.ln_bwd_reference(*case)
        gx, gg, gb = ln_bwd_restated(*case, dtype)
        rx = S.worst_ratio(gx, dx, S.linear_bar(dx, *S.elementwise_bars(dtype)))
        rg = S.worst_ratio(gg, dg, S.linear_bar(dg, *S.colsum_bars(dtype, M)))
        rb = S.worst_ratio(gb, db, S.linear_bar(db, *S.colsum_bars(dtype, M)))
        print(f"{M}x{N} {S.tname(dtype)}: err / bar dx {rx:.3f} dgamma {rg:.4f} dbeta {rb:.4f}")
        assert max(rx, rg, rb) <= 0.5, (M, N, rx, rg, rb)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_exact_twin_is_exact_and_catches_both_faults(dtype):
    reachable = 0
    for M, N in S.ln_bwd_cases(dtype):
        dy, x, gamma, mean, rstd = S.ln_twin_inputs(dtype, M, N)
        want = S.ln_twin_expected(dy, x, mean, rstd, torch.float64)
        want32 = S.ln_twin_expected(dy, x, mean, rstd, torch.float32)
        for w64, w32 in zip(want, want32):
            assert torch.equal(w64, w32.double()), (M, N)            # the exactness claim, proven
            assert torch.equal(w64 * 8, (w64 * 8).round()) and float(w64.abs().max()) * 8 < 2 ** 24
        _, dg, db = ln_bwd_restated(dy, x, gamma, mean, rstd, dtype)
        assert torch.equal(dg.double(), want[0]) and torch.equal(db.double(), want[1]), (M, N)
        three = torch.full((N,), 3.0)
        _, dg, db = ln_bwd_restated(dy, x, gamma, mean, rstd, dtype, dgamma=three, dbeta=three)
        assert torch.equal(dg.double(), want[0] + 3.0) and torch.equal(db.double(), want[1] + 3.0), (M, N)
        walks_on = M > 4 * S.ln_bwd_ws_rows(M)                        # some wave takes a second row
        reachable += walks_on
        for fault in BWD_FAULTS:
            _, dg, db = ln_bwd_restated(dy, x, gamma, mean, rstd, dtype, fault=fault)
            same = torch.equal(dg.double(), want[0]) and torch.equal(db.double(), want[1])
            assert same != walks_on, (fault, M, N)                    # caught wherever it can happen, and only there
            if fault == "stats_ahead" and walks_on:
                assert not torch.equal(dg.double(), want[0])          # wrong statistics show in dgamma (dbeta has none)
    assert reachable >= 6                                             # 2049 and 4100 rows at three widths


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_swapped_stride_shows_only_with_a_different_pad_per_operand(dtype):
    """x read with dy's row stride: invisible without pads and with the same pad on every operand (what the strided case
    first ran with), a broken dx bar with LN_BWD_PADS."""
    M, N = S.LN_BWD_STRIDED
    case = S.ln_bwd_inputs(dtype, M, N)
    dx, dg, db = S.ln_bwd_reference(*case)
    for pads, caught in ((None, False), ((1, 1, 1), False), (S.LN_BWD_PADS, True)):
        for fault in (None, "swapped_stride"):
            gx, gg, gb = ln_bwd_restated(*case, dtype, fault=fault, pads=pads)
            rx = S.worst_ratio(gx, dx, S.linear_bar(dx, *S.elementwise_bars(dtype)))
            rg = S.worst_ratio(gg, dg, S.linear_bar(dg, *S.colsum_bars(dtype, M)))
            assert (rx > 1.0) == (caught and fault is not None), (pads, fault, rx)
            assert fault is not None or rg <= 0.5, (pads, rg)


# ---- the cast's halfway values ----------------------------------------------------------------------------------------
def test_halfway_values_tell_rounding_modes_apart():
    h = S.cast_halfway()
    word = h.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert bool(((word & 0xFFFF) == 0x8000).all()) and torch.isfinite(h).all()
    assert bool((h.abs() >= torch.finfo(F32).tiny).all())                      # no denormals
    odd = ((word >> 16) & 1).bool()
    neg = (word >> 31).bool()
    for a in (odd, ~odd):
        for b in (neg, ~neg):
            assert int((a & b).sum()) >= 1000
    rne = h.to(BF).view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(rne, (word >> 16) + odd.long())                         # torch rounds to nearest even
    assert int((rne != (word >> 16)).sum()) == int(odd.sum())                  # truncation: wrong on the odd half
    assert int((rne != (word >> 16) + 1).sum()) == int((~odd).sum())           # round-half-up: wrong on the even half
    assert torch.isinf(S.cast_specials()[4:6].to(BF)).all()
