"""The fp8-weight matrix-vector decode kernels, one link at a time, against the rules of tests/gemv_w8_rule.py, and the row
quantiser against its restatement bit for bit.

Every case launches one kernel through its vy_debug_*_w8 wrapper (the internal launcher as it is) and names the
instantiation it runs in its parameter id: dec_gemv1_w8_kernel<EPI, CH, NB, NORM>, K = 2048 / 4096 / 8192 / 16384 are <2,1>,
<4,1>, <4,2>, <4,4>.  x carries NaN behind K, output buffers carry guard tails, the caches are NaN-filled with a head
stride larger than cap * dh; every bit outside the written row and columns must be unchanged.  The same case list runs
through an fp32 emulation on the CPU first (test_gemv_w8_rule_cpu.py).  Each case prints the worst
(|got - want| - 1/2 ulp) / delta it met."""
import ctypes as C

import pytest
import torch

from tests import gemv_w8_rule as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = W.cases()
VY_ERR_UNSUPPORTED = -2
WORST = {}

P, I32, I64, F32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "vy_debug_dec_gemv1_w8": [P, P, P, P, P, P, I32, I32, P],
    "vy_debug_dec_gemv1_gated_w8": [P, P, P, P, I32, I32, I32, F32, P],
    "vy_debug_dec_gemv1_qkv_w8": [P, P, P, P, P, P, P, I64, I32, I32, I32, P, P, I64, I32, I32, F32, P],
}


def lib():
    from vyomai_amd import _lib
    l = _lib.load()
    for name, sig in SIGNATURES.items():
        f = getattr(l, name)
        f.argtypes, f.restype = sig, C.c_int
    return l


def launch(c, inp):
    """Uploads the buffers of a case, launches its one kernel, -> the output buffers on the CPU."""
    l = lib()
    K, N, L = c["K"], c["N"], inp["L"]
    d = {k: v.to(DEV) for k, v in inp.items() if isinstance(v, torch.Tensor) and k != "wval"}
    ptr = lambda k: d[k].data_ptr() if k in d else None
    st = torch.cuda.current_stream().cuda_stream
    if c["kind"] == "plain":
        rc = l.vy_debug_dec_gemv1_w8(ptr("x"), ptr("codes"), ptr("scales"), ptr("bias"), ptr("res"), ptr("y"), N, K, st)
    elif c["kind"] == "gated":
        rc = l.vy_debug_dec_gemv1_gated_w8(ptr("x"), ptr("codes"), ptr("scales"), ptr("y"), N, K, c["norm"], W.EPS, st)
    else:
        h, hk, dh = c["heads"]
        row = c["pos"] * dh * 2                      # bytes: the cache row of this position, as the step driver passes it
        rc = l.vy_debug_dec_gemv1_qkv_w8(ptr("x"), ptr("codes"), ptr("scales"), ptr("bias"), ptr("q"), d["k"].data_ptr() + row,
                                         d["v"].data_ptr() + row, L["c_sh"], h, hk, dh, ptr("cos"), ptr("sin"), c["pos"], K,
                                         c["norm"], W.EPS, st)
    assert rc == 0, (c["id"], rc)
    torch.cuda.synchronize()
    return {k: d[k].cpu() for k in W.outputs_of(c)}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_link(case):
    """One launch of the instantiation the id names; the rule of the case's data kind per output, untouched bits elsewhere."""
    inp = W.make_inputs(case)
    worst = W.check(case, inp, launch(case, inp))
    fam = f"dec_gemv1_w8 {case['kind']} {case['data']}"
    WORST[fam] = max(WORST.get(fam, float("-inf")), worst)
    print(f"ratio {case['id']} {worst:.4f}")


def test_link_worst_ratios_report():
    """Prints the worst ratio per link and data kind over the cases above (a figure for DESIGN, asserted case by case)."""
    for fam, w in sorted(WORST.items()):
        print(f"worst {fam}: {w:.4f}")
        assert w <= 1.0


@pytest.mark.parametrize("what", ["K1024", "N6", "x_plus_8_bytes", "codes_plus_8_bytes", "no_scales"])
def test_w8_launchers_refuse_on_the_host(what):
    """K no kernel serves, N no multiple of 4, x or the codes off their 16-byte alignment, no scales: VY_ERR_UNSUPPORTED
    before any launch, through all three wrappers, and the outputs keep their bits."""
    l = lib()
    K, N = (1024 if what == "K1024" else 2048), (6 if what == "N6" else 8)
    x = torch.ones(K + 8, dtype=W.BF, device=DEV)
    w = torch.full((3 * N * K + 16,), 0x38, dtype=torch.uint8, device=DEV)
    s = torch.ones(3 * N, device=DEV)
    y = torch.full((64,), 3.0, dtype=W.BF, device=DEV)
    xp = x.data_ptr() + (8 if what == "x_plus_8_bytes" else 0)
    wp = w.data_ptr() + (8 if what == "codes_plus_8_bytes" else 0)
    sp = None if what == "no_scales" else s.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    assert l.vy_debug_dec_gemv1_w8(xp, wp, sp, None, None, y.data_ptr(), N, K, st) == VY_ERR_UNSUPPORTED
    assert l.vy_debug_dec_gemv1_gated_w8(xp, wp, sp, y.data_ptr(), N, K, 0, W.EPS, st) == VY_ERR_UNSUPPORTED
    dh = 2 if what == "N6" else 4
    assert l.vy_debug_dec_gemv1_qkv_w8(xp, wp, sp, None, y.data_ptr(), y.data_ptr() + 32, y.data_ptr() + 64, 8, 1, 1, dh,
                                       None, None, 0, K, 0, W.EPS, st) == VY_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())


# ---- the quantiser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,K", [(5, 2048), (1028, 4096), (4, 16384)])
def test_quant_rows_equals_the_rule_bit_for_bit(N, K, dtype):
    """Codes and scales of vy_quant_rows_fp8 against tests/gemv_w8_rule.quant_rows: rows spread over five decades, an
    all-zero row, a row of code values times 2^-3 with amax = 448 * 2^-3 (lossless), ldw = K + 24 with NaN in the padding,
    ldc = K + 8 with 0xA5 in the padding, a guard behind the scales."""
    from vyomai_amd import _lib
    g = torch.Generator().manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) * torch.logspace(-3, 2, N)[:, None]).to(dtype).float()
    w[1] = 0.0
    w[2] = W.decode_e4m3(torch.randint(0, 127, (K,), generator=g).to(torch.uint8)) * 0.125
    w[2, K - 1] = -56.0
    assert torch.equal(w.to(dtype).float(), w)
    ldw, ldc = K + 24, K + 8
    wp = torch.full((N, ldw), float("nan"), dtype=dtype)
    wp[:, :K] = w.to(dtype)
    wd = wp.to(DEV)
    codes = torch.full((N, ldc), 0xA5, dtype=torch.uint8, device=DEV)
    scales = torch.full((N + 3,), -7.0, device=DEV)
    _lib.call("vy_quant_rows_fp8", wd.data_ptr(), ldw, codes.data_ptr(), ldc, scales.data_ptr(), N, K, _lib.dtype_code(dtype),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want_c, want_s = W.quant_rows(w)
    got_c, got_s = codes.cpu(), scales.cpu()
    assert torch.equal(got_s[:N].view(torch.int32), want_s.view(torch.int32)) and bool((got_s[N:] == -7.0).all())
    assert torch.equal(got_c[:, :K], want_c), f"{int((got_c[:, :K] != want_c).sum())} codes differ"
    assert bool((got_c[:, K:] == 0xA5).all())
    assert float(want_s[1]) == 1.0 and int(want_c[1].max()) == 0
    assert float(want_s[2]) == 0.125 and torch.equal(W.decode_e4m3(got_c[2, :K]) * 0.125, w[2])
    assert bool(W.quant_error_ok(w, got_c[:, :K], got_s[:N]).all())


def test_quant_rows_refuses_bad_arguments():
    from vyomai_amd import _lib
    w = torch.ones(4, 2048, dtype=W.BF, device=DEV)
    c = torch.zeros(4, 2048, dtype=torch.uint8, device=DEV)
    s = torch.zeros(4, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_lib.VyomHipError, match="null operand"):
        _lib.call("vy_quant_rows_fp8", w.data_ptr(), 2048, None, 2048, s.data_ptr(), 4, 2048, _lib.dtype_code(W.BF), st)
    with pytest.raises(_lib.VyomHipError, match="4-byte"):
        _lib.call("vy_quant_rows_fp8", w.data_ptr(), 2048, c.data_ptr(), 2046, s.data_ptr(), 4, 2046, _lib.dtype_code(W.BF), st)
    with pytest.raises(_lib.VyomHipError, match="bad shape"):
        _lib.call("vy_quant_rows_fp8", w.data_ptr(), 1024, c.data_ptr(), 2048, s.data_ptr(), 4, 2048, _lib.dtype_code(W.BF), st)
    torch.cuda.synchronize()
    assert int(c.max()) == 0
