"""Guard of tests/prenorm_cases.py: fp32 torch restatements of rmsnorm_fwd_kernel, gated_act_kernel (vy_misc.hip),
rmsnorm_bwd_kernel and gated_act_bwd_kernel (vy_prenorm.hip), with the faults the regimes and the strided and
grid-stride cases were built for switched in.  No kernel runs here.

The restatements keep the kernels' order: per-lane chunk sums, the xor butterfly (lane_sums and wave_sum of the stream
guard), the wave walk w, w + W, ..., the four-wave sum ((dw0 + r0) + r1) + r2 and the slab summed by
tests/colsum_rule.py.  Asserted: the tables reach every instantiation of both dispatchers and both sides of every
boundary; the faithful restatements stay inside every bar on every case (the worst ratio per kernel and output is
printed); the dw bar is never looser than the fp32 bar of test_rmsnorm_bwd_vs_fp64 on unit data; every fault breaks a
bar where the table of faults says so and passes where it says so -- the passing half is the evidence that the regime
or case is needed.  (The launchers' refusals are exercised on the host in tests/test_causal_lm_cpu.py.)"""
import pytest
import torch

from tests import colsum_rule
from tests import prenorm_cases as P
from tests import stream_cases as S
from tests.test_stream_kernels_cpu import lane_sums, wave_sum

BF, F32 = P.BF, P.F32
IDS = [P.tname(t) for t in P.DTYPES]
INF = float("inf")


def ratio(got, want, bar):
    """worst_ratio, or inf for a non-finite result (a fault may divide by zero)."""
    if not bool(torch.isfinite(got.float()).all()):
        return INF
    return P.worst_ratio(got, want, bar)


# ---- restatements -------------------------------------------------------------------------------------------------------
def rms_r(x32, dtype, N, fault, chunks):
    """r (M,) of rows x32 (M, N) in fp32: lane sums of squares, the butterfly, the mean, eps, the inverse root."""
    div = 64 * chunks * P.VEC[dtype] if fault == "mean_over_lanes" else N
    ms = wave_sum(lane_sums(x32 * x32, dtype)) / div
    if fault == "no_eps":
        return 1.0 / torch.sqrt(ms)
    if fault == "eps_outside":
        return 1.0 / (torch.sqrt(ms) + P.EPS)
    return 1.0 / torch.sqrt(ms + P.EPS)


def rms_fwd_restated(x, w, w_offset, dtype, fault=None):
    v, N = x.float(), x.shape[1]
    r = rms_r(v, dtype, N, fault, P.rms_fwd_chunks(N, dtype))
    off = 0.0 if fault == "offset_dropped" else w_offset
    return (v * r[:, None] * (off + w.float())).to(dtype)


def strided_rows(t, ld, read_ld=None):
    """t (M, N) laid out with a row stride of ld in a sentinel-filled buffer and read back with a row stride of read_ld
    (ld unless a fault reads it with another operand's)."""
    M, N = t.shape
    flat = P.padded(t, ld).reshape(-1)
    return torch.as_strided(flat, (M, N), (read_ld or ld, 1))


def rms_bwd_restated(dy, x, w, add, w_offset, dtype, fault=None, dw0=None, pads=None):
    """-> dx (cast to dtype), dw (fp32; dw0 given: accumulated onto).  pads: the operands sit in buffers with row strides
    N + pads[i] VEC (lddy, ldx, ldadd, lddx); the fault swapped_stride reads add_to with ldx."""
    M, N = x.shape
    vec = P.VEC[dtype]
    WB = S.ln_bwd_ws_rows(M)
    W = 4 * WB
    lddy, ldx, ldadd, _ = (N + p * vec for p in (pads or (0, 0, 0, 0)))
    xv, dv = strided_rows(x, ldx).float(), strided_rows(dy, lddy).float()
    av = strided_rows(add, ldadd, ldx if fault == "swapped_stride" else None).float() if add is not None else None
    g = (0.0 if fault == "offset_dropped" else w_offset) + w.float()
    ch, _ = P.rms_bwd_instantiation(N, dtype)
    div = 64 * ch * vec if fault == "mean_over_lanes" else N
    part, dx = torch.zeros(W, N), torch.zeros(M, N)
    for r0 in range(0, M, W):
        rows = torch.arange(r0, min(M, r0 + W))
        n = rows.numel()
        src = torch.where(rows + W < M, rows + W, rows) if fault == "row_ahead" else rows
        xr, dr = xv[src], dv[src]
        r = rms_r(xr, dtype, N, fault, ch)[:, None]
        cf = r * r * r * (wave_sum(lane_sums(xr * g * dr, dtype)) / div)[:, None]
        o = r * g * dr - xr * cf
        if av is not None:
            o = o + av[rows]
        keep = torch.ones(n, 1)
        if fault == "skip_last" and r0 > 0:
            keep = (rows + W < M).float()[:, None]
        dx[rows] = o * keep
        part[:n] = part[:n] + dr * xr * r * keep
    slab = part.view(WB, 4, N)
    slab = ((slab[:, 0] + slab[:, 1]) + slab[:, 2]) + slab[:, 3]
    dw = colsum_rule.ordered_colsum(slab.numpy(), S.ln_colsum_slices(WB), base=None if dw0 is None else dw0.numpy())
    return dx.to(dtype), torch.from_numpy(dw)


def act32(code, a):
    return P.act_fp64(code, a)          # torch's own functions, in the precision of a


def gated_views(gu, I, dtype, pad, fault):
    """gate, up (M, I) in fp32, read from a buffer with ldg = 2 I + pad VEC as the kernels address it."""
    M = gu.shape[0]
    ldg = 2 * I + pad * P.VEC[dtype]
    flat = P.padded(gu, ldg).float().reshape(-1)
    gate = torch.as_strided(flat, (M, I), (ldg, 1), 0)
    up = torch.as_strided(flat, (M, I), (ldg, 1), ldg // 2 if fault == "up_at_half_stride" else I)
    return (up, gate) if fault == "swap_halves" else (gate, up)


def one_walk_only(out, vec, row_chunks):
    """no_second_walk: the chunks past the capped grid's first pass keep what the buffer held.  out (M, k row_chunks vec):
    chunk i = m row_chunks + c of the kernel's loop owns columns c vec .. of every block of row_chunks vec columns."""
    M = out.shape[0]
    done = (torch.arange(M)[:, None] * row_chunks + torch.arange(row_chunks)[None, :]) < P.GATED_GRID_CAP
    done = done.repeat_interleave(vec, dim=1).repeat(1, out.shape[1] // (row_chunks * vec))
    return torch.where(done, out, torch.full_like(out, P.SENTINEL))


def gated_fwd_restated(gu, code, dtype, pad=0, fault=None):
    I = gu.shape[1] // 2
    gate, up = gated_views(gu, I, dtype, pad, fault)
    out = (act32(code, gate) * up).to(dtype)
    return one_walk_only(out, P.VEC[dtype], I // P.VEC[dtype]) if fault == "no_second_walk" else out


def gated_bwd_restated(d, gu, code, dtype, pad=0, fault=None):
    I = gu.shape[1] // 2
    gate, up = gated_views(gu, I, dtype, pad, fault)
    a = gate.clone().requires_grad_(True)
    f = act32(code, a)
    df, = torch.autograd.grad(f.sum(), a)
    f, dd = f.detach(), d.float()
    out = torch.cat([dd * up * df, dd * f], dim=1).to(dtype)
    return one_walk_only(out, P.VEC[dtype], I // P.VEC[dtype]) if fault == "no_second_walk" else out


# ---- the tables reach what they were written for ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_tables_cover_every_instantiation(dtype):
    vec, t = P.VEC[dtype], P.tname(dtype)
    fwd_chs = (1, 2, 4, 8, 16) + ((32,) if dtype == F32 else ())
    fwd = {f"rmsnorm_fwd_kernel<{t}, {P.rms_fwd_chunks(N, dtype)}>" for N in P.RMS_FWD_WIDTHS[dtype]}
    assert fwd == {f"rmsnorm_fwd_kernel<{t}, {ch}>" for ch in fwd_chs}, fwd
    bwd = {"rmsnorm_bwd_kernel<%s, %d, %s>" % ((t,) + P.rms_bwd_instantiation(N, dtype)) for N in P.RMS_BWD_WIDTHS[dtype]}
    assert bwd == {f"rmsnorm_bwd_kernel<{t}, {ch}, {ch <= 4}>" for ch in (1, 2, 4, 8, 16)}, bwd
    for widths, chs, chunks in ((P.RMS_FWD_WIDTHS[dtype], fwd_chs, lambda N: P.rms_fwd_chunks(N, dtype)),
                                (P.RMS_BWD_WIDTHS[dtype], (1, 2, 4, 8, 16), lambda N: P.rms_bwd_instantiation(N, dtype)[0])):
        for ch in chs[:-1]:                  # both sides of every boundary
            assert 64 * ch * vec in widths and 64 * ch * vec + vec in widths, ch
            assert chunks(64 * ch * vec) == ch and chunks(64 * ch * vec + vec) == 2 * ch
        assert max(widths) == 64 * chs[-1] * vec and 768 in widths and vec in widths
    # the refusal widths are one chunk above the widest
    assert P.RMS_FWD_TOO_WIDE[dtype] == max(P.RMS_FWD_WIDTHS[dtype]) + vec and P.rms_fwd_chunks(P.RMS_FWD_TOO_WIDE[dtype], dtype) is None
    assert P.RMS_BWD_TOO_WIDE[dtype] == max(P.RMS_BWD_WIDTHS[dtype]) + vec
    assert P.rms_bwd_instantiation(P.RMS_BWD_TOO_WIDE[dtype], dtype) is None
    assert (P.RMS_FWD_TOO_WIDE[dtype], P.RMS_BWD_TOO_WIDE[dtype]) == ((8200, 8200) if dtype == BF else (8196, 4100))
    # pipelined / not: the last pipelined width and the first that is not
    assert P.rms_bwd_instantiation(P.RMS_WIDEST_PIPELINED[dtype], dtype) == (4, True)
    assert P.rms_bwd_instantiation(P.RMS_FIRST_UNPIPELINED[dtype], dtype) == (8, False)
    assert P.RMS_FIRST_UNPIPELINED[dtype] == P.RMS_WIDEST_PIPELINED[dtype] + vec
    # the regimes run at 768 and the widest row of every CH
    assert {P.rms_fwd_chunks(N, dtype) for N in P.rms_fwd_regime_widths(dtype)} == set(fwd_chs)
    assert {P.rms_bwd_instantiation(N, dtype)[0] for N in P.rms_bwd_regime_widths(dtype)} == {1, 2, 4, 8, 16}
    assert 768 in P.rms_fwd_regime_widths(dtype) and 768 in P.rms_bwd_regime_widths(dtype)
    fc, bc = P.rms_fwd_cases(dtype), P.rms_bwd_cases(dtype)
    assert all(("unit", M, N) in fc for N in P.RMS_FWD_WIDTHS[dtype] for M in (5, 7))
    assert all((g, 5, N) in fc for g in P.REGIMES[1:] for N in P.rms_fwd_regime_widths(dtype))
    Ns = P.RMS_BWD_WIDTHS[dtype]
    assert all(("unit", M, N) in bc for N in Ns for M in (5, 257))
    for N in (768, min(Ns), P.RMS_WIDEST_PIPELINED[dtype], P.RMS_FIRST_UNPIPELINED[dtype]):
        assert all(("unit", M, N) in bc for M in P.RMS_BWD_ROWS), N
    assert ("unit", 2049, max(Ns)) in bc and P.rms_bwd_instantiation(max(Ns), dtype) == (16, False)
    assert all((g, 257, N) in bc for g in P.REGIMES[1:] for N in P.rms_bwd_regime_widths(dtype))
    # a second row through every instantiation: pipelined and not
    walked = {P.rms_bwd_instantiation(N, dtype) for g, M, N in bc if P.walks(M) > 1}
    assert {(1, True), (2, True), (4, True), (8, False), (16, False)} <= walked, walked
    assert P.walks(2049) == 2 and P.walks(4100) == 3 and all(P.walks(M) == 1 for M in P.RMS_BWD_ROWS if M < 2049)
    assert ("unit",) + P.RMS_FWD_STRIDED[dtype] in fc and ("unit",) + P.RMS_BWD_STRIDED[dtype] in bc
    assert len(set(P.RMS_FWD_PADS)) == 2 and len(set(P.RMS_BWD_PADS)) == 4 and 0 not in P.RMS_FWD_PADS + P.RMS_BWD_PADS


def test_gated_tables_cover_the_instantiations_the_strides_and_the_second_walk():
    assert {P.gated_instantiation(c) for c in P.ACTS.values()} == {"VY_ACT_GELU_ERF", "VY_ACT_GELU_TANH", "VY_ACT_RUNTIME"}
    assert len(P.ACTS) == 7 and P.gated_instantiation(P.SILU) == "VY_ACT_RUNTIME"
    assert P.GATED_STRIDED in P.GATED_SHAPES and len(set(P.GATED_BWD_PADS)) == 3 and len(set(P.GATED_FWD_PADS)) == 2
    assert 0 not in P.GATED_FWD_PADS + P.GATED_BWD_PADS
    for dtype in P.DTYPES:
        M, I = P.GATED_STRIDE_SHAPE[dtype]
        chunks = M * (I // P.VEC[dtype])
        assert I // P.VEC[dtype] == 1024 and chunks - P.GATED_GRID_CAP == 1024       # exactly the last row is the second walk
        assert -(-chunks // 256) > 8192 and M * 2 * I * (2 if dtype == BF else 4) < 68e6
        for Ms, Is in P.GATED_SHAPES:
            assert Ms * (Is // P.VEC[dtype]) <= P.GATED_GRID_CAP                        # the old shapes never walk on


# ---- RMSNorm forward --------------------------------------------------------------------------------------------------
def fwd_ratio(dtype, regime, M, N, w_offset, fault=None):
    x, _, _, w, _ = P.rms_inputs(dtype, regime, M, N)
    want = P.rms_fwd_reference(x, w, w_offset)
    return ratio(rms_fwd_restated(x, w, w_offset, dtype, fault), want, P.rms_y_bar(dtype, want))


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_faithful_forward_stays_inside_the_bar(dtype):
    worst = {}
    for regime, M, N in P.rms_fwd_cases(dtype):
        x, _, _, w, _ = P.rms_inputs(dtype, regime, M, N)
        for w_offset in P.W_OFFSETS:
            want = P.rms_fwd_reference(x, w, w_offset)
            got = rms_fwd_restated(x, w, w_offset, dtype)
            worst[regime] = max(worst.get(regime, 0.0), ratio(got, want, P.rms_y_bar(dtype, want)))
            if regime == "zero":
                assert bool((got[P.zero_rows(M)] == 0).all()) and bool((want[P.zero_rows(M)] == 0).all())
    for regime, r in worst.items():
        print(f"rmsnorm_fwd y {P.tname(dtype)} {regime}: worst err / bar {r:.3f}")
    assert set(worst) == set(P.REGIMES) and max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_forward_faults_fail_where_their_regime_is_and_pass_on_unit_data(dtype):
    for N in P.rms_fwd_regime_widths(dtype):
        for w_offset in P.W_OFFSETS:
            assert fwd_ratio(dtype, "small", 5, N, w_offset, "no_eps") > 1.0, N
            assert fwd_ratio(dtype, "zero", 5, N, w_offset, "no_eps") == INF, N          # 0 * inf
            assert fwd_ratio(dtype, "small", 5, N, w_offset, "eps_outside") > 1.0, N
            for fault in ("no_eps", "eps_outside"):
                assert fwd_ratio(dtype, "unit", 5, N, w_offset, fault) <= 1.0, (fault, N)   # why the regimes are needed
    for N in P.RMS_FWD_WIDTHS[dtype]:
        fills = N == 64 * P.rms_fwd_chunks(N, dtype) * P.VEC[dtype]
        for M in P.RMS_FWD_ROWS:
            assert (fwd_ratio(dtype, "unit", M, N, 1.0, "mean_over_lanes") > 1.0) != fills, (M, N)
            assert fwd_ratio(dtype, "unit", M, N, 1.0, "offset_dropped") > 1.0, (M, N)
            assert fwd_ratio(dtype, "unit", M, N, 0.0, "offset_dropped") <= 1.0, (M, N)
    assert sum(N == 64 * P.rms_fwd_chunks(N, dtype) * P.VEC[dtype] for N in P.RMS_FWD_WIDTHS[dtype]) == (5 if dtype == BF else 6)


# ---- RMSNorm backward -------------------------------------------------------------------------------------------------
def bwd_ratios(dtype, regime, M, N, w_offset, with_add, acc, fault=None, pads=None):
    """-> (worst dx err / bar, worst dw err / bar) of the restatement on one case."""
    x, dy, add, w, dw0 = P.rms_inputs(dtype, regime, M, N)
    add, dw0 = (add if with_add else None), (dw0 if acc else None)
    want_dx, want_dw, terms, abs_terms = P.rms_bwd_reference(dy, x, w, w_offset, add, dw0)
    dx, dw = rms_bwd_restated(dy, x, w, add, w_offset, dtype, fault, dw0, pads)
    return ratio(dx, want_dx, P.rms_dx_bar(dtype, want_dx, terms)), ratio(dw, want_dw, P.rms_dw_bar(abs_terms, dw0, M if regime == "unit" else None))


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_faithful_backward_stays_inside_both_bars(dtype):
    worst = {}
    for regime, M, N in P.rms_bwd_cases(dtype):
        for w_offset in P.W_OFFSETS:
            for with_add, acc in P.rms_bwd_runs(w_offset):
                rx, rw = bwd_ratios(dtype, regime, M, N, w_offset, with_add, acc)
                worst[regime] = tuple(max(a, b) for a, b in zip(worst.get(regime, (0.0, 0.0)), (rx, rw)))
                assert rx <= 1.0 and rw <= 1.0, (regime, M, N, w_offset, with_add, acc, rx, rw)
    for regime, (rx, rw) in worst.items():
        print(f"rmsnorm_bwd {P.tname(dtype)} {regime}: worst err / bar dx {rx:.3f} dw {rw:.3f}")
    assert set(worst) == set(P.REGIMES)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_dw_bar_is_no_looser_than_the_fp32_bar_on_unit_data(dtype):
    """On unit data the bar sits at or below colsum_bars(F32, M) in every column of every case, accumulating or not, and is
    the derived one (not the cap) up to 257 rows.  Printed: the derived bar and a faithful fp32 evaluation against
    colsum_bars(F32, M), per row count."""
    for M in P.RMS_BWD_ROWS:
        derived, evaluated, capped = 0.0, 0.0, False
        for N in (N for m, N in P.rms_bwd_unit_shapes(dtype) if m == M):
            x, dy, _, w, dw0 = P.rms_inputs(dtype, "unit", M, N)
            for start in (None, dw0):
                _, want_dw, _, abs_terms = P.rms_bwd_reference(dy, x, w, 1.0, None, start)
                old = S.linear_bar(want_dw, *S.colsum_bars(F32, M))
                bar = P.rms_dw_bar(abs_terms, start, M)
                assert bool((bar <= old).all()), (M, N)
                capped |= bool((bar < P.rms_dw_bar(abs_terms, start)).any())
                derived = max(derived, float((P.rms_dw_bar(abs_terms, start) / old).max()))
                _, dw = rms_bwd_restated(dy, x, w, None, 1.0, dtype, None, start)
                evaluated = max(evaluated, P.worst_ratio(dw, want_dw, old))
        print(f"dw {P.tname(dtype)} M={M}: derived bar / fp32 bar <= {derived:.3f}, fp32 evaluation / fp32 bar <= {evaluated:.3f}")
        assert capped == (derived > 1.0) and (capped == (M >= 2049)), (M, derived)
        assert evaluated <= 0.25, (M, evaluated)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_backward_eps_faults_fail_on_small_and_zero_rows_and_pass_on_unit_data(dtype):
    M = P.RMS_BWD_REGIME_ROWS
    for N in P.rms_bwd_regime_widths(dtype):
        rx, rw = bwd_ratios(dtype, "small", M, N, 1.0, False, False, "no_eps")
        assert rx > 1.0 and rw > 1.0, (N, rx, rw)
        assert bwd_ratios(dtype, "zero", M, N, 1.0, False, False, "no_eps") == (INF, INF), N
        rx, rw = bwd_ratios(dtype, "small", M, N, 1.0, False, False, "eps_outside")
        assert rx > 1.0 and rw > 1.0, (N, rx, rw)
        for fault in ("no_eps", "eps_outside"):
            assert max(bwd_ratios(dtype, "unit", M, N, 1.0, False, False, fault)) <= 1.0, (fault, N)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_backward_mean_and_offset_faults(dtype):
    for N in P.RMS_BWD_WIDTHS[dtype]:
        fills = N == 64 * P.rms_bwd_instantiation(N, dtype)[0] * P.VEC[dtype]
        rx, rw = bwd_ratios(dtype, "unit", 5, N, 1.0, False, False, "mean_over_lanes")
        assert (rx > 1.0) != fills and (rw > 1.0) != fills, (N, rx, rw)
        rx, rw = bwd_ratios(dtype, "unit", 5, N, 1.0, False, False, "offset_dropped")
        assert rx > 1.0 and rw <= 1.0, (N, rx, rw)          # dw holds no weight: dx alone sees the offset
        assert max(bwd_ratios(dtype, "unit", 5, N, 0.0, False, False, "offset_dropped")) <= 1.0, N


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_walk_faults_fail_exactly_where_a_wave_walks_a_second_row(dtype):
    reached = set()
    for M, N in P.rms_bwd_unit_shapes(dtype):
        if M == 257 and N not in (768, P.RMS_FIRST_UNPIPELINED[dtype]):
            continue                                        # one walk either way: 5 rows at every width say the same
        walks_on = P.walks(M) > 1
        for fault in ("skip_last", "row_ahead"):
            rx, rw = bwd_ratios(dtype, "unit", M, N, 1.0, False, False, fault)
            assert (rx > 1.0) == walks_on and (rw > 1.0) == walks_on, (fault, M, N, rx, rw)
        if walks_on:
            reached.add(P.rms_bwd_instantiation(N, dtype))
    assert reached == {(1, True), (2, True), (4, True), (8, False), (16, False)}, reached


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_swapped_stride_shows_only_with_a_different_pad_per_operand(dtype):
    M, N = P.RMS_BWD_STRIDED[dtype]
    same = tuple(P.RMS_BWD_PADS[:1] * 4)                    # every operand padded alike, as the first strided tests did
    for pads, caught in ((None, False), (same, False), (P.RMS_BWD_PADS, True)):
        assert max(bwd_ratios(dtype, "unit", M, N, 1.0, True, False, None, pads)) <= 1.0, pads
        rx, _ = bwd_ratios(dtype, "unit", M, N, 1.0, True, False, "swapped_stride", pads)
        assert (rx > 1.0) == caught, (pads, rx)


# ---- gated activations ------------------------------------------------------------------------------------------------
def gated_ratios(dtype, M, I, code, fwd_pad=0, bwd_pad=0, fault=None):
    gu, d = P.gated_inputs(dtype, M, I)
    want_out, want_dgu = P.gated_reference(gu, d, code)
    return (ratio(gated_fwd_restated(gu, code, dtype, fwd_pad, fault), want_out, P.gated_bar(dtype, want_out)),
            ratio(gated_bwd_restated(d, gu, code, dtype, bwd_pad, fault), want_dgu, P.gated_bar(dtype, want_dgu)))


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_gated_restatements_and_their_faults(dtype):
    worst = [0.0, 0.0]
    ldg_fwd, ldg_bwd = P.GATED_FWD_PADS[0], P.GATED_BWD_PADS[1]
    for M, I in P.GATED_SHAPES:
        for name, code in P.ACTS.items():
            rf, rb = gated_ratios(dtype, M, I, code)
            worst = [max(worst[0], rf), max(worst[1], rb)]
            assert min(gated_ratios(dtype, M, I, code, fault="swap_halves")) > 1.0, (name, M, I)
            assert max(gated_ratios(dtype, M, I, code, fault="up_at_half_stride")) <= 1.0, (name, M, I)   # ldg = 2 I hides it
            assert max(gated_ratios(dtype, M, I, code, fault="no_second_walk")) <= 1.0, (name, M, I)      # and one walk this
    M, I = P.GATED_STRIDED
    rf, rb = gated_ratios(dtype, M, I, P.SILU, ldg_fwd, ldg_bwd)
    worst = [max(worst[0], rf), max(worst[1], rb)]
    assert min(gated_ratios(dtype, M, I, P.SILU, ldg_fwd, ldg_bwd, "up_at_half_stride")) > 1.0
    assert min(gated_ratios(dtype, M, I, P.SILU, ldg_fwd, ldg_bwd, "swap_halves")) > 1.0
    print(f"gated_act {P.tname(dtype)}: worst err / bar fwd {worst[0]:.3f} bwd {worst[1]:.3f}")
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_no_second_walk_shows_in_the_last_row_of_the_grid_stride_case_only(dtype):
    gu, d, want_out, want_dgu = P.gated_stride_case(dtype)
    for got, bad, want in ((gated_fwd_restated(gu, P.SILU, dtype), gated_fwd_restated(gu, P.SILU, dtype, 0, "no_second_walk"), want_out),
                           (gated_bwd_restated(d, gu, P.SILU, dtype), gated_bwd_restated(d, gu, P.SILU, dtype, 0, "no_second_walk"),
                            want_dgu)):
        bar = P.gated_bar(dtype, want)
        assert ratio(got, want, bar) <= 1.0
        assert ratio(bad[:-1], want[:-1], bar[:-1]) <= 1.0 and ratio(bad[-1:], want[-1:], bar[-1:]) > 1.0
