"""The single-sequence matrix-vector decode kernels, one link at a time, against the rules of tests/gemv_rule.py.

Every case launches one kernel through its vy_debug_* wrapper (the internal launcher as it is) and names the
instantiation it runs in its parameter id: dec_gemv1_kernel<EPI, CH, NB, NORM> for vy_dec_gemv1 / _gated / _qkv (B = 1;
K = 2048 / 4096 / 8192 / 16384 are <4,1>, <8,1>, <8,2>, <8,4>) and gemv_bf16_kernel<EPI, ACT, 4, PRESCALED, GATED> for
vy_gemv_norm / vy_gemv_qkv_norm / vy_gemv_gated (B <= 4, ldx > K).  Output buffers carry guard tails, the caches are
NaN-filled strided views with a head stride larger than cap * dh and a batch stride per row; every bit outside the
written row and columns must be unchanged.  The same case list runs through an fp32 emulation on the CPU first
(test_gemv_rule_cpu.py).  Each case prints the worst (|got - want| - 1/2 ulp) / delta it met: DESIGN records them."""
import ctypes as C

import pytest
import torch

from tests import gemv_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = R.cases()
VY_ERR_UNSUPPORTED, ACT_GELU_TANH = -2, 2
WORST = {}

P, I32, I64, F32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "vy_debug_dec_gemv1": [P, P, P, P, P, I32, I32, P],
    "vy_debug_dec_gemv1_gated": [P, P, P, I32, I32, I32, F32, P],
    "vy_debug_dec_gemv1_qkv": [P, P, P, P, P, P, I64, I32, I32, I32, P, P, I64, I32, I32, F32, P],
    "vy_debug_gemv_norm": [P, I64, P, I64, P, I32, F32, P, I64, P, I64, I64, I64, I64, P],
    "vy_debug_gemv_qkv_norm": [P, I64, P, I64, P, I32, F32, P, I64, I64, P, I64, I64, I64, P, I64, I64, I64, I64, I64, I32, I32,
                               I32, P, P, I64, P],
    "vy_debug_gemv_gated": [P, I64, P, I64, I32, F32, P, I64, I64, I64, I64, I32, P],
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
    K, M, N, L = c["K"], c["M"], c["N"], inp["L"]
    d = {k: v.to(DEV) for k, v in inp.items() if isinstance(v, torch.Tensor)}
    ptr = lambda k: d[k].data_ptr() if k in d else None
    st = torch.cuda.current_stream().cuda_stream
    lean, P_ = c["fam"] == "lean", c["norm"]
    if c["kind"] == "plain":
        if lean:
            rc = l.vy_debug_dec_gemv1(ptr("x"), ptr("w"), ptr("bias"), ptr("res"), ptr("y"), N, K, st)
        else:
            rc = l.vy_debug_gemv_norm(ptr("x"), L["ldx"], ptr("w"), K, ptr("bias"), P_, R.EPS, ptr("res"), L["ldy"], ptr("y"),
                                      L["ldy"], M, N, K, st)
    elif c["kind"] == "gated":
        if lean:
            rc = l.vy_debug_dec_gemv1_gated(ptr("x"), ptr("w"), ptr("y"), N, K, P_, R.EPS, st)
        else:
            rc = l.vy_debug_gemv_gated(ptr("x"), L["ldx"], ptr("w"), K, P_, R.EPS, ptr("y"), L["ldy"], M, N, K, ACT_GELU_TANH, st)
    else:
        h, hk, dh = c["heads"]
        row = c["pos"] * dh * 2                      # bytes: the cache row of this position, as the step driver passes it
        kp, vp = d["k"].data_ptr() + row, d["v"].data_ptr() + row
        if lean:
            rc = l.vy_debug_dec_gemv1_qkv(ptr("x"), ptr("w"), ptr("bias"), ptr("q"), kp, vp, L["c_sh"], h, hk, dh, ptr("cos"),
                                          ptr("sin"), c["pos"], K, P_, R.EPS, st)
        else:
            rc = l.vy_debug_gemv_qkv_norm(ptr("x"), L["ldx"], ptr("w"), K, ptr("bias"), P_, R.EPS, ptr("q"), L["q_sb"], dh, kp,
                                          L["c_sb"], L["c_sh"], dh, vp, L["c_sb"], L["c_sh"], dh, M, K, h, hk, dh, ptr("cos"),
                                          ptr("sin"), c["pos"], st)
    assert rc == 0, (c["id"], rc)
    torch.cuda.synchronize()
    return {k: d[k].cpu() for k in R.outputs_of(c)}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_link(case):
    """One launch of the instantiation the id names; exact / round / rotary rule per output, untouched bits elsewhere."""
    inp = R.make_inputs(case)
    worst = R.check(case, inp, launch(case, inp))
    fam = ("dec_gemv1 " if case["fam"] == "lean" else "gemv_bf16 ") + case["kind"] + (" gauss" if case["data"] == "gauss" else "")
    WORST[fam] = max(WORST.get(fam, float("-inf")), worst)
    print(f"ratio {case['id']} {worst:.4f}")


def test_link_worst_ratios_report():
    """Prints the worst ratio per kernel family over the cases above (a figure for DESIGN, asserted case by case)."""
    for fam, w in sorted(WORST.items()):
        print(f"worst {fam}: {w:.4f}")
        assert w <= 1.0


@pytest.mark.parametrize("N", [4096, 4100, 8192])
def test_rmsnorm_fp32_wide_rows(N):
    """vy_rmsnorm_fwd in fp32 past 4096 columns (rmsnorm_fwd_kernel<float, 32>: the fp32 Gemma step at d = 8192 is the
    yardstick of the step test) against fp64, 5 rows (a second workgroup, a partial one).  Bar: fp32 arithmetic, the sum
    of N squares in 64 lane sums and a wave reduction, three products per element: 1e-5 relative is 80 ulps."""
    from vyomai_amd import _lib
    g = torch.Generator().manual_seed(N)
    x, w = torch.randn(5, N, generator=g), 0.1 * torch.randn(N, generator=g)
    y = torch.full((5, N + 4), 7.0, device=DEV)
    xd, wd = x.to(DEV), w.to(DEV)
    _lib.call("vy_rmsnorm_fwd", xd.data_ptr(), N, wd.data_ptr(), y.data_ptr(), N + 4, 5, N, R.EPS, 1.0, _lib.dtype_code(torch.float32),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = x.double() * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + R.EPS) * (1.0 + w.double())
    got = y.cpu().double()
    assert bool(((got[:, :N] - want).abs() <= 1e-5 * want.abs() + 1e-7).all())
    assert bool((got[:, N:] == 7.0).all())


@pytest.mark.parametrize("what", ["K1024", "N6", "x_plus_8_bytes"])
def test_lean_launchers_refuse_on_the_host(what):
    """K no lean kernel serves, N no multiple of 4, x not 16-byte aligned: VY_ERR_UNSUPPORTED before any launch, through
    all three wrappers, and the outputs keep their bits."""
    l = lib()
    K, N = (1024 if what == "K1024" else 2048), (6 if what == "N6" else 8)
    x = torch.ones(K + 8, dtype=R.BF, device=DEV)
    w = torch.ones(3 * N, K, dtype=R.BF, device=DEV)
    y = torch.full((64,), 3.0, dtype=R.BF, device=DEV)
    xp = x.data_ptr() + (8 if what == "x_plus_8_bytes" else 0)
    st = torch.cuda.current_stream().cuda_stream
    assert l.vy_debug_dec_gemv1(xp, w.data_ptr(), None, None, y.data_ptr(), N, K, st) == VY_ERR_UNSUPPORTED
    assert l.vy_debug_dec_gemv1_gated(xp, w.data_ptr(), y.data_ptr(), N, K, 0, R.EPS, st) == VY_ERR_UNSUPPORTED
    # (h, hk, dh) = (1, 1, N / 3 ...): N = 3 dh; dh = 2 makes N = 6, dh = 4 makes N = 12 with the other two faults
    dh = 2 if what == "N6" else 4
    assert l.vy_debug_dec_gemv1_qkv(xp, w.data_ptr(), None, y.data_ptr(), y.data_ptr() + 32, y.data_ptr() + 64, 8, 1, 1, dh,
                                    None, None, 0, K, 0, R.EPS, st) == VY_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
