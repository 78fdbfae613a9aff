"""The four streaming kernels of the pre-norm decoder blocks at every instantiation, against the fp64 references and bars
of tests/prenorm_cases.py: vy_rmsnorm_fwd and vy_gated_act_fwd (vy_misc.hip), vy_rmsnorm_bwd and vy_gated_act_bwd
(vy_prenorm.hip).  Every launch goes through _lib.call on sentinel-filled buffers: the pad columns and the rows past M
must still hold the sentinel afterwards and every input, pads included, must keep its bits.  The references are the fp64
formulas of prenorm_cases evaluated by torch on the device (the wide cases hold 17 M elements).  Each check prints its
worst error / bar; test_worst_ratios_report prints the worst per kernel, output and type, the figures DESIGN records.
The same tables run through fp32 restatements with faults switched in on the CPU (tests/test_prenorm_kernels_cpu.py)."""
import pytest
import torch

from tests import prenorm_cases as P
from tests import stream_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = P.BF, P.F32
IDS = [P.tname(t) for t in P.DTYPES]
WORST = {}


def _lib():
    from vyomai_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def held(kernel, output, dtype, got, want, bar, what):
    """Prints and records the worst |got - want| / bar (got and want on the device), then asserts it."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g = got.double()
    assert bool(torch.isfinite(g).all()), f"{kernel} {output} {what}: non-finite output"
    bar = bar if torch.is_tensor(bar) else torch.full_like(want, float(bar))
    worst = float(((g - want).abs() / bar).max())
    key = (kernel, output, P.tname(dtype))
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"  {kernel} {output} {what}: worst err / bar {worst:.3f}")
    assert worst <= 1.0, f"{kernel} {output} {what}: worst err / bar {worst:.3f}"


class Padded:
    """t (M, N) on the CPU in a device buffer of (M + extra, N + pad) sentinels; .view is [:M, :N], .ld the row stride."""

    def __init__(self, t, pad, extra=0):
        self.M, self.N = t.shape
        self.ld = self.N + pad
        self.buf = torch.full((self.M + extra, self.ld), P.SENTINEL, dtype=t.dtype, device=DEV)
        self.buf[:self.M, :self.N] = t.to(DEV)
        self.view = self.buf[:self.M, :self.N]
        self.before = bits(self.buf).clone()

    def ptr(self):
        return self.buf.data_ptr()

    def unchanged(self, what):
        assert torch.equal(bits(self.buf), self.before), f"{what}: an input was written"

    def sentinel_intact(self, what):
        assert bool((self.buf[:self.M, self.N:] == P.SENTINEL).all()), f"{what}: pad columns written"
        assert bool((self.buf[self.M:] == P.SENTINEL).all()), f"{what}: rows past M written"


def out_buffer(M, N, pad, dtype):
    """An output of (M + 1, N + pad) sentinels."""
    return Padded(torch.full((M, N), P.SENTINEL, dtype=dtype), pad, extra=1)


# ---- RMSNorm forward --------------------------------------------------------------------------------------------------
def rms_fwd_launch(x, w, w_offset, pads=(0, 0)):
    """vy_rmsnorm_fwd with ldx = N + pads[0], ldy = N + pads[1] -> y (M, N) on the device."""
    L = _lib()
    M, N = x.shape
    xb, yb, wd = Padded(x, pads[0]), out_buffer(M, N, pads[1], x.dtype), w.to(DEV)
    L.call("vy_rmsnorm_fwd", xb.ptr(), xb.ld, wd.data_ptr(), yb.ptr(), yb.ld, M, N, P.EPS, w_offset, L.dtype_code(x.dtype), _st())
    torch.cuda.synchronize()
    yb.sentinel_intact("y")
    xb.unchanged("x")
    assert torch.equal(bits(wd.cpu()), bits(w)), "w was written"
    return yb.view


def rms_fwd_params():
    out = []
    for dtype in P.DTYPES:
        seen = []
        for regime, _, N in P.rms_fwd_cases(dtype):
            if (regime, N) not in seen:
                seen.append((regime, N))
                out.append(pytest.param(dtype, regime, N, id=f"{P.tname(dtype)}-{regime}-{N}"))
    return out


@pytest.mark.parametrize("dtype,regime,N", rms_fwd_params())
def test_rmsnorm_fwd(dtype, regime, N):
    """rmsnorm_fwd_kernel<T, CH> at both sides of every CH boundary (5 and 7 rows: a ragged last workgroup), w_offset 0
    and 1, against fp64 within elementwise_bars.  The small, zero and outlier regimes run at 768 and the widest row of
    every CH; an all-zero row gives exact zeros.  The strided case runs with ldx = N + VEC, ldy = N + 2 VEC."""
    print(f"{P.tname(dtype)} {regime} N={N}: rmsnorm_fwd_kernel<{P.tname(dtype)}, {P.rms_fwd_chunks(N, dtype)}>")
    for M in [m for g, m, n in P.rms_fwd_cases(dtype) if (g, n) == (regime, N)]:
        x, _, _, w, _ = P.rms_inputs(dtype, regime, M, N)
        runs = [(0, 0)]
        if regime == "unit" and (M, N) == P.RMS_FWD_STRIDED[dtype]:
            runs.append(tuple(p * P.VEC[dtype] for p in P.RMS_FWD_PADS))
        for w_offset in P.W_OFFSETS:
            want = P.rms_fwd_reference(x.to(DEV), w.to(DEV), w_offset)
            for pads in runs:
                y = rms_fwd_launch(x, w, w_offset, pads)
                held("rmsnorm_fwd", "y", dtype, y, want, P.rms_y_bar(dtype, want), f"{regime} {M}x{N} w_offset={w_offset} pads={pads}")
                if regime == "zero":
                    assert bool((y[P.zero_rows(M).to(DEV)] == 0).all()), "an all-zero row must give exact zeros"
                    assert bool((want[P.zero_rows(M).to(DEV)] == 0).all())


# ---- RMSNorm backward -------------------------------------------------------------------------------------------------
def rms_bwd_launch(dy, x, w, add, w_offset, start, pads=(0, 0, 0, 0)):
    """vy_rmsnorm_bwd with lddy, ldx, ldadd, lddx = N + pads[i] -> dx (M, N), dw (N) on the device.  start (N) or None:
    dw is accumulated onto it (beta = 1) or overwrites a sentinel fill (beta = 0)."""
    L = _lib()
    M, N = x.shape
    WB = L.load().vy_layernorm_bwd_ws_rows(M)
    assert WB == S.ln_bwd_ws_rows(M)
    db, xb, dxb, wd = Padded(dy, pads[0]), Padded(x, pads[1]), out_buffer(M, N, pads[3], x.dtype), w.to(DEV)
    ab = Padded(add, pads[2]) if add is not None else None
    dw = start.to(DEV).clone() if start is not None else torch.full((N,), P.SENTINEL, device=DEV)
    ws = torch.empty(WB * N, dtype=F32, device=DEV)
    L.call("vy_rmsnorm_bwd", db.ptr(), db.ld, xb.ptr(), xb.ld, wd.data_ptr(), ab.ptr() if ab else None, ab.ld if ab else 0,
           dxb.ptr(), dxb.ld, dw.data_ptr(), 1.0 if start is not None else 0.0, ws.data_ptr(), M, N, P.EPS, w_offset,
           L.dtype_code(x.dtype), _st())
    torch.cuda.synchronize()
    dxb.sentinel_intact("dx")
    for b, name in ((db, "dy"), (xb, "x"), (ab, "add_to")):
        if b is not None:
            b.unchanged(name)
    assert torch.equal(bits(wd.cpu()), bits(w)), "w was written"
    return dxb.view, dw


def rms_bwd_params():
    return [pytest.param(dtype, regime, M, N, id=f"{P.tname(dtype)}-{regime}-{M}x{N}")
            for dtype in P.DTYPES for regime, M, N in P.rms_bwd_cases(dtype)]


@pytest.mark.parametrize("dtype,regime,M,N", rms_bwd_params())
def test_rmsnorm_bwd(dtype, regime, M, N):
    """rmsnorm_bwd_kernel<T, CH, PIPE> + the ordered column sum against fp64: w_offset 0 and 1, add_to on and off, dw
    overwritten and accumulated onto a random start (the four combinations spread over the two w_offsets).  dx within
    rms_dx_bar, dw within rms_dw_bar -- one bar for bf16 and fp32.  A second run gives the same bits.  The strided case
    runs with four different pads."""
    ch, pipe = P.rms_bwd_instantiation(N, dtype)
    print(f"{P.tname(dtype)} {regime} {M}x{N}: rmsnorm_bwd_kernel<{P.tname(dtype)}, {ch}, {str(pipe).lower()}>, "
          f"{S.ln_bwd_ws_rows(M)} slab rows, {P.walks(M)} row(s) a wave")
    x, dy, add, w, dw0 = P.rms_inputs(dtype, regime, M, N)
    xd, dyd, wd, addd, dw0d = (t.to(DEV) for t in (x, dy, w, add, dw0))
    unit_rows = M if regime == "unit" else None
    for w_offset in P.W_OFFSETS:
        base_dx, base_dw, terms, abs_terms = P.rms_bwd_reference(dyd, xd, wd, w_offset)
        runs = [(with_add, acc, (0, 0, 0, 0)) for with_add, acc in P.rms_bwd_runs(w_offset)]
        if regime == "unit" and (M, N) == P.RMS_BWD_STRIDED[dtype]:
            runs += [(True, acc, tuple(p * P.VEC[dtype] for p in P.RMS_BWD_PADS)) for acc in (False, True)]
        for with_add, acc, pads in runs:
            want_dx = base_dx + addd.double() if with_add else base_dx
            want_dw = base_dw + dw0d.double() if acc else base_dw
            dx, dw = rms_bwd_launch(dy, x, w, add if with_add else None, w_offset, dw0 if acc else None, pads)
            what = f"{regime} {M}x{N} w_offset={w_offset} add_to={with_add} accumulate={acc} pads={pads}"
            held("rmsnorm_bwd", "dx", dtype, dx, want_dx, P.rms_dx_bar(dtype, want_dx, terms), what)
            held("rmsnorm_bwd", "dw", dtype, dw, want_dw, P.rms_dw_bar(abs_terms, dw0d if acc else None, unit_rows), what)
            if regime == "zero" and not with_add:       # dx = eps^-1/2 (w_offset + w) dy on a zero row, r ~ 1000
                z = P.zero_rows(M).to(DEV)
                assert float(want_dx[z].abs().max()) > 500.0 and bool((terms[z] == want_dx[z].abs()).all())
        dx2, dw2 = rms_bwd_launch(dy, x, w, None, w_offset, None)
        dx3, dw3 = rms_bwd_launch(dy, x, w, None, w_offset, None)
        assert torch.equal(bits(dx2), bits(dx3)) and torch.equal(bits(dw2), bits(dw3)), "a second run gave other bits"


# ---- gated activations ------------------------------------------------------------------------------------------------
def gated_fwd_launch(gu, code, pads=(0, 0)):
    """vy_gated_act_fwd with ldg = 2 I + pads[0], ldo = I + pads[1] -> out (M, I) on the device."""
    L = _lib()
    M, I = gu.shape[0], gu.shape[1] // 2
    gb, ob = Padded(gu, pads[0]), out_buffer(M, I, pads[1], gu.dtype)
    L.call("vy_gated_act_fwd", gb.ptr(), gb.ld, ob.ptr(), ob.ld, M, I, code, L.dtype_code(gu.dtype), _st())
    torch.cuda.synchronize()
    ob.sentinel_intact("out")
    gb.unchanged("gate_up")
    return ob.view


def gated_bwd_launch(d, gu, code, pads=(0, 0, 0)):
    """vy_gated_act_bwd with lddo = I + pads[0], ldg = 2 I + pads[1], lddg = 2 I + pads[2] -> d_gate_up (M, 2 I)."""
    L = _lib()
    M, I = d.shape
    db, gb, ob = Padded(d, pads[0]), Padded(gu, pads[1]), out_buffer(M, 2 * I, pads[2], gu.dtype)
    L.call("vy_gated_act_bwd", db.ptr(), db.ld, gb.ptr(), gb.ld, ob.ptr(), ob.ld, M, I, code, L.dtype_code(gu.dtype), _st())
    torch.cuda.synchronize()
    ob.sentinel_intact("d_gate_up")
    db.unchanged("d_act")
    gb.unchanged("gate_up")
    return ob.view


@pytest.mark.parametrize("M,I", P.GATED_SHAPES)
@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_gated_act_every_code(dtype, M, I):
    """The seven codes, the kink values in the first row: gated_act_kernel<T, ACT> and gated_act_bwd_kernel<T, ACT> for
    the two compiled GELUs and the run-time-switched instantiation.  The strided shape also runs SiLU and the erf GELU
    with ldg > 2 I and a different pad on every operand."""
    gu, d = P.gated_inputs(dtype, M, I)
    for name, code in P.ACTS.items():
        want_out, want_dgu = P.gated_reference(gu.to(DEV), d.to(DEV), code)
        runs = [((0, 0), (0, 0, 0))]
        if (M, I) == P.GATED_STRIDED and name in ("silu", "gelu"):
            runs.append((tuple(p * P.VEC[dtype] for p in P.GATED_FWD_PADS), tuple(p * P.VEC[dtype] for p in P.GATED_BWD_PADS)))
        for fwd_pads, bwd_pads in runs:
            what = f"{name} ({P.gated_instantiation(code)}) {M}x{I}"
            held("gated_act_fwd", "out", dtype, gated_fwd_launch(gu, code, fwd_pads), want_out, P.gated_bar(dtype, want_out),
                 f"{what} pads={fwd_pads}")
            held("gated_act_bwd", "d_gate_up", dtype, gated_bwd_launch(d, gu, code, bwd_pads), want_dgu,
                 P.gated_bar(dtype, want_dgu), f"{what} pads={bwd_pads}")


_STRIDE_DEV = {}


def stride_case_on_device(dtype):
    """gate_up, d_act (CPU) and the fp64 out, d_gate_up (device) of the grid-stride case: computed once for both tests."""
    if dtype not in _STRIDE_DEV:
        gu, d = P.gated_inputs(dtype, *P.GATED_STRIDE_SHAPE[dtype])
        _STRIDE_DEV[dtype] = (gu, d) + P.silu_reference(gu.to(DEV), d.to(DEV))
    return _STRIDE_DEV[dtype]


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_gated_act_grid_stride_loop(dtype, direction):
    """2049 rows of 1024 chunks: 1024 chunks past the 8192 workgroups x 256 threads of the capped grid, so the last row
    is the threads' second walk.  fp64 over all rows; the last row asserted on its own."""
    gu, d, want_out, want_dgu = stride_case_on_device(dtype)
    if direction == "fwd":
        kernel, output, got, want = "gated_act_fwd", "out", gated_fwd_launch(gu, P.SILU), want_out
    else:
        kernel, output, got, want = "gated_act_bwd", "d_gate_up", gated_bwd_launch(d, gu, P.SILU), want_dgu
    bar = P.gated_bar(dtype, want)
    held(kernel, output, dtype, got[-1:], want[-1:], bar[-1:], "the last row: the second walk of the grid-stride loop")
    held(kernel, output, dtype, got, want, bar, f"all {gu.shape[0]} rows")


# ---- the figures -------------------------------------------------------------------------------------------------------
def test_worst_ratios_report():
    """Prints the worst error / bar per kernel, output and type over the cases above (figures for DESIGN, asserted case by
    case)."""
    for (kernel, output, t), worst in sorted(WORST.items()):
        print(f"worst {kernel} {output} {t}: {worst:.3f}")
        assert worst <= 1.0
