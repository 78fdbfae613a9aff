"""The reference's other hidden_act choices (silu / swish, tanh, sigmoid, relu6, leaky_relu; VyomAI/layers/ffn.py:7-15)
on the MI355X: the GEMM epilogues of every kernel family, the backward kernels, FeedForward / DecoderLayer / DecoderModel /
Vit against what the REAL reference produced (tests/golden/activations.npz), the lean decode step, and the error paths.

Kinked activations (relu6, leaky_relu).  Their derivative is a step, so ONE pre-activation that lands on the other side
of 0 or 6 moves a gradient by far more than any fp32 bar.  fp32 gradients are therefore compared only on inputs whose
reference pre-activations keep a margin from both kinks (asserted and stored by tests/golden/make_golden_acts.py), and
only after the kernel's own pre-activation has been shown to sit within margin / 8 of the reference's: a pass cannot rest
on a coincidence of flips.  In bf16 the pre-activations near a kink flip in ANY bf16 evaluation, the oracle's included;
there the bar is the project's bf16 rule: the HIP error against fp32 is at most 2x the gap the oracle
itself shows when it runs in bf16 on the CPU, plus 1e-2 of the tensor's scale.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vyom_oracle as O
from tests.golden import cases, cases_acts as CA
from tests.test_kernels_gpu import check, check_exact, ints, rnd, thin_ternary, assert_bf16_exact
from vyomai_amd import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# vy_act code -> the torch function the reference's table builds (nn.SiLU, nn.Tanh, nn.Sigmoid, nn.ReLU6, nn.LeakyReLU())
ACTS = {3: F.silu, 4: torch.tanh, 5: torch.sigmoid, 6: F.relu6, 7: F.leaky_relu}
NEW_CODES = sorted(ACTS)
SAVE_DERIV = 0x100


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _ops():
    from vyomai_amd import ops
    return ops


def act_grad(code, pre):
    """act'(pre) through torch autograd (its conventions at the kinks), in pre's dtype."""
    p = pre.detach().clone().requires_grad_(True)
    ACTS[code](p).sum().backward()
    return p.grad


def test_codes_match_the_library_constants():
    from vyomai_amd import _lib
    assert [_lib.ACT_SILU, _lib.ACT_TANH, _lib.ACT_SIGMOID, _lib.ACT_RELU6, _lib.ACT_LEAKY_RELU] == NEW_CODES
    assert _lib.ACT_SAVE_DERIV == SAVE_DERIV


# ---- kernel level -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(51, 1003, 768), (130, 64, 16), (257, 192, 260)])
@pytest.mark.parametrize("act", NEW_CODES)
def test_linear_f32(M, N, K, act):
    """test_kernels_gpu.test_linear_f32 for the new codes: fp64 reference, 1e-5 abs + 1e-5 rel."""
    ops = _ops()
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    b, r = rnd(N, seed=3, scale=0.1), rnd(M, N, seed=4)
    pre_ref = x.double() @ w.double().t() + b.double()
    want = ACTS[act](pre_ref) + r.double()
    pre = torch.zeros(M, (N + 7) // 8 * 8, device=DEV)
    y = ops.linear(x.to(DEV), w.to(DEV), b.to(DEV), act=act, residual=r.to(DEV), pre_out=pre[:, :N])
    check(y, want, 1e-5, 1e-5, f"linear f32 {M}x{N}x{K} act {act}")
    check(pre[:, :N], pre_ref, 1e-5, 1e-5, "pre_out")


def test_f32_tanh_and_sigmoid_saturate_without_nan():
    """|pre| of a few hundred: e^{2x} overflows fp32; the result must be the limit, not NaN."""
    ops = _ops()
    x = (rnd(64, 64, seed=5) * 40).to(DEV)
    w = (torch.eye(64) * 8).to(DEV)
    for dt in (torch.float32, BF):
        pre_ref = (x.to(dt).double().cpu() @ w.to(dt).double().cpu().t())
        assert pre_ref.abs().max() > 500
        for act in (3, 4, 5):
            for flag in (0, SAVE_DERIV):
                pre = torch.zeros(64, 64, dtype=dt, device=DEV)
                y = ops.linear(x.to(dt), w.to(dt), act=act | flag, pre_out=pre)
                assert torch.isfinite(y.float()).all() and torch.isfinite(pre.float()).all(), (dt, act, flag)
                tol = (1e-5, 1e-5) if dt == torch.float32 else (3e-2, 1e-2)
                check(y, ACTS[act](pre_ref), *tol, f"saturated act {act} {dt}")
                if flag:
                    check(pre, act_grad(act, pre_ref), *tol, f"saturated act' {act} {dt}")


# one shape per GEMM family of linear_impl, so that the run-time-code instantiation of each runs at least once
FAMILIES = [(1, 256, 3072, "gemv"), (7, 768, 3072, "skinny"), (32, 3072, 768, "skinny16"), (300, 768, 72, "generic"),
            (264, 2048, 2048, "split-K"), (1024, 3072, 768, "m16"), (4096, 1003, 768, "256x192")]


@pytest.mark.parametrize("M,N,K,family", FAMILIES)
def test_linear_bf16_every_family(M, N, K, family):
    """test_kernels_gpu.test_linear_bf16 for the new codes (3e-2 abs + 1e-2 rel), once with pre_out and once with
    VY_ACT_SAVE_DERIV, where the saved tensor is act'(bf16(pre)): the derivative of the kernel's OWN rounded
    pre-activation, so the 0 / 1 mask of the kinked activations is determined."""
    ops = _ops()
    x = rnd(M, K, seed=1).bfloat16()
    w = rnd(N, K, seed=2, scale=1 / math.sqrt(K)).bfloat16()
    b = rnd(N, seed=3, scale=0.1).bfloat16()
    r = rnd(M, N, seed=4).bfloat16()
    pre_ref = x.double() @ w.double().t() + b.double()
    ldy = (N + 7) // 8 * 8
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    for act in NEW_CODES:
        want = ACTS[act](pre_ref) + r.double()
        pre = torch.zeros(M, ldy, dtype=BF, device=DEV)
        y = ops.linear(xd, wd, bd, act=act, residual=rd, pre_out=pre[:, :N])
        check(y, want, 3e-2, 1e-2, f"{family} bf16 {M}x{N}x{K} act {act}")
        check(pre[:, :N], pre_ref, 3e-2, 1e-2, f"{family} pre_out act {act}")
        der = torch.zeros(M, ldy, dtype=BF, device=DEV)
        y2 = ops.linear(xd, wd, bd, act=act | SAVE_DERIV, residual=rd, pre_out=der[:, :N])
        check_exact(y2, y, f"{family} act {act}: the output does not depend on what is saved")
        want_d = act_grad(act, pre[:, :N].double().cpu())
        check(der[:, :N], want_d, 3e-2, 1e-2, f"{family} saved act' {act}")
        if act in (6, 7):
            # a step function of a value both sides hold exactly: bit-equal to torch on the same bf16 values
            check_exact(der[:, :N], act_grad(act, pre[:, :N].cpu()), f"{family} saved act' {act} (m, n)")
        if ldy > N:
            assert float(der[:, N:].abs().max()) == 0 and float(pre[:, N:].abs().max()) == 0, "padding columns written"


@pytest.mark.parametrize("M,N,K,family", FAMILIES)
def test_kinked_activations_exact_on_integers(M, N, K, family):
    """test_kernels_gpu's small-integer operands: the pre-activation is an exact integer (0 and 6 occur), so relu6 and
    leaky_relu outputs and their saved derivatives are bit-equal to torch on the same bf16 values."""
    ops = _ops()
    x, w, b = ints(M, K, seed=1), thin_ternary(N, K, K, seed=2), ints(N, seed=3, lo=-2, hi=2)
    pre_ref = x @ w.t() + b
    assert_bf16_exact(pre_ref, f"{M}x{N}x{K} pre")
    assert (pre_ref == 0).any() and (pre_ref == 6).any() and (pre_ref > 6).any() and (pre_ref < 0).any()
    pre_bf = pre_ref.to(BF)
    xd, wd, bd = x.to(BF).to(DEV), w.to(BF).to(DEV), b.to(BF).to(DEV)
    ldy = (N + 7) // 8 * 8
    for act in (6, 7):
        der = torch.zeros(M, ldy, dtype=BF, device=DEV)
        y = ops.linear(xd, wd, bd, act=act | SAVE_DERIV, pre_out=der[:, :N])
        check_exact(y, ACTS[act](pre_bf), f"{family} act {act} output (m, n)")
        check_exact(der[:, :N], act_grad(act, pre_bf), f"{family} act {act} saved derivative (m, n)")
        pre = torch.zeros(M, ldy, dtype=BF, device=DEV)
        y = ops.linear(xd, wd, bd, act=act, pre_out=pre[:, :N])
        check_exact(y, ACTS[act](pre_bf), f"{family} act {act} output with pre_out (m, n)")
        check_exact(pre[:, :N], pre_bf, f"{family} act {act} pre_out (m, n)")


@pytest.mark.parametrize("dt", [BF, torch.float32])
@pytest.mark.parametrize("act", NEW_CODES)
def test_backward_kernels(dt, act):
    """ops.act_bwd, and ops.linear_dgrad with the pre-activation and with the saved derivative.  The pre-activation is
    an input tensor, so the derivative mask is determined.  Bars: test_dgrad's in bf16, test_linear_f32's in fp32."""
    ops = _ops()
    tol = (4e-2, 1e-2) if dt == BF else (1e-5, 1e-5)
    for (M, N, K) in [(300, 768, 3072), (51, 3072, 768), (2112, 768, 3072)]:
        dy = rnd(M, N, seed=1).to(dt)
        w = (rnd(N, K, seed=2) / math.sqrt(N)).to(dt)
        pre = (rnd(M, K, seed=3) * 3).to(dt)      # |pre| reaches past 6
        add = rnd(M, K, seed=4).to(dt)
        dact = act_grad(act, pre.double())
        want = (dy.double() @ w.double()) * dact + add.double()
        wt = ops.transpose(w.to(DEV))
        got = ops.linear_dgrad(dy.to(DEV), wt, pre.to(DEV), act, add.to(DEV))
        check(got, want, *tol, f"dgrad {dt} act {act} {M}x{N}x{K}")
        saved = dact.to(dt)
        want_s = (dy.double() @ w.double()) * saved.double() + add.double()
        got = ops.linear_dgrad(dy.to(DEV), wt, saved.to(DEV), act | SAVE_DERIV, add.to(DEV))
        check(got, want_s, *tol, f"dgrad SAVE_DERIV {dt} act {act} {M}x{N}x{K}")
    dy, pre = rnd(520, 3072, seed=7).to(dt), (rnd(520, 3072, seed=8) * 3).to(dt)
    got = ops.act_bwd(dy.to(DEV), pre.to(DEV), act)
    check(got, dy.double() * act_grad(act, pre.double()), *tol, f"act_bwd {dt} act {act}")


# ---- error paths ------------------------------------------------------------------------------------------------------

def test_unknown_activation_is_an_error_everywhere():
    """An argument check, not a fault: every buffer handed over is valid."""
    from vyomai_amd import _lib
    ops = _ops()
    for dt in (BF, torch.float32):
        x, w = rnd(8, 64, seed=1).to(dt).to(DEV), rnd(64, 64, seed=2).to(dt).to(DEV)
        for code in (8, 99, 0x40, 99 | SAVE_DERIV):
            with pytest.raises(_lib.VyomHipError, match="unknown activation"):
                ops.linear(x, w, act=code)
            with pytest.raises(_lib.VyomHipError):
                ops.linear_dgrad(x, ops.transpose(w), x.clone(), code)
            with pytest.raises(_lib.VyomHipError):
                ops.act_bwd(x, x.clone(), code)
    # the decode entry points are C++ symbols of the library (not part of the C ABI): reached by their mangled names
    lib = _lib.load()
    B, N, K = 8, 64, 512
    x, w, b = rnd(B, K, seed=1).to(BF).to(DEV), rnd(N, K, seed=2).to(BF).to(DEV), rnd(N, seed=3).to(BF).to(DEV)
    g, be = torch.ones(K, dtype=BF, device=DEV), torch.zeros(K, dtype=BF, device=DEV)
    g2, be2 = torch.ones(N, dtype=BF, device=DEV), torch.zeros(N, dtype=BF, device=DEV)
    y = torch.full((B, N), 7.0, dtype=BF, device=DEV)
    part = torch.zeros(12 * 32 * N, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p, i, f = C.c_void_p, C.c_int, C.c_float
    dec_linear_ex = getattr(lib, "_Z16vy_dec_linear_exPKviS0_S0_S0_iS0_S0_fPviiiiiP12ihipStream_t")
    dec_linear_ex.argtypes, dec_linear_ex.restype = [p, i, p, p, p, i, p, p, f, p, i, i, i, i, i, p], i
    dec_res_ln = getattr(lib, "_Z20vy_dec_linear_res_lnPKviS0_S0_S0_iS0_S0_fPviPfiiiiP12ihipStream_t")
    dec_res_ln.argtypes, dec_res_ln.restype = [p, i, p, p, p, i, p, p, f, p, i, p, i, i, i, i, p], i
    VY_ERR_ARG = -1
    want = (x.double() @ w.double().t() + b.double()).cpu()
    for code, rc_want in ((0, 0), (3, 0), (99, VY_ERR_ARG), (8, VY_ERR_ARG)):
        y.fill_(7.0)
        # the plain projection: no residual, no LayerNorm operands
        rc = dec_linear_ex(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), None, 0, None, None, 0.0, y.data_ptr(), N, B, N, K, code, st)
        assert rc == rc_want, ("vy_dec_linear_ex plain", code, rc, lib.vy_last_error())
        torch.cuda.synchronize()
        if rc_want:
            assert float((y.float() - 7.0).abs().max()) == 0, "a refused call must not launch"
        else:
            check(y, want if code == 0 else F.silu(want), 3e-2, 1e-2, f"vy_dec_linear_ex plain act {code}")
        rc = dec_linear_ex(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), None, 0, g.data_ptr(), be.data_ptr(), 1e-5,
                           y.data_ptr(), N, B, N, K, code, st)
        assert rc == rc_want, ("vy_dec_linear_ex", code, rc, lib.vy_last_error())
        y.fill_(7.0)
        rc = dec_res_ln(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), None, 0, g2.data_ptr(), be2.data_ptr(), 1e-5,
                        y.data_ptr(), N, part.data_ptr(), B, N, K, code, st)
        assert rc == rc_want, ("vy_dec_linear_res_ln", code, rc, lib.vy_last_error())
        torch.cuda.synchronize()
        if rc_want:
            assert float((y.float() - 7.0).abs().max()) == 0, "a refused call must not launch"
        else:
            h = want if code == 0 else F.silu(want)
            check(y, F.layer_norm(h.to(BF).double(), (N,)), 4e-2, 1e-2, f"vy_dec_linear_res_ln act {code}")
    torch.cuda.synchronize()


# ---- module level, fp32, against the real reference (tests/golden/activations.npz) -----------------------------------------

def rel_err(got, want):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def abs_err(got, want):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max())


def _fill(mod, prefix, dtype=torch.float32):
    for n, t in mod.state_dict().items():
        t.copy_(T(recipe.param_value(prefix + n, tuple(t.shape))))
    return mod.to(DEV).to(dtype)


def _np(t):
    return t.detach().float().cpu().numpy()


def _check_pre_against_margin(g, key, pre_kernel):
    """The kernel's fp32 pre-activation sits within margin / 8 of the reference's: every derivative of relu6 and
    leaky_relu is then taken on the reference's side of the kinks, so a gradient comparison is meaningful."""
    margin = float(g[f"{key}.margin"][0])
    assert margin >= 8 * float(g[f"{key}.pre_err"][0])
    p = _np(pre_kernel).reshape(-1, pre_kernel.shape[-1])
    if f"{key}.pre" in g:
        e = abs_err(p, g[f"{key}.pre"])
        print(f"{key}: margin {margin:.3e}, kernel pre-activation off by {e:.3e}")
        assert e <= margin / 8, (key, e, margin)
        return
    # the wide case stores the elements within NEAR_BAND of a kink, and a sub-sampled grid
    idx = g[f"{key}.pre.near_idx"]
    e = abs_err(p.reshape(-1)[idx], g[f"{key}.pre.near_val"])
    e_sub = abs_err(CA.sub_grad(p), g[f"{key}.pre.sub"])
    print(f"{key}: margin {margin:.3e}, kernel pre-activation off by {e:.3e} near the kinks, {e_sub:.3e} on the grid")
    assert e <= margin / 8 and e_sub <= margin / 8, (key, e, e_sub, margin)
    far = np.ones(p.size, dtype=bool)
    far[idx] = False
    assert CA.kink_distance(p.reshape(-1)[far]).min() >= CA.NEAR_BAND / 2, "an element the fixture holds far from the kinks is near one"


@pytest.mark.parametrize("tag", ["micro", "wide"])
@pytest.mark.parametrize("name", CA.NAMES)
def test_feed_forward_fp32_vs_reference(golden, tag, name):
    from vyomai_amd.layers.ffn import FeedForward
    ops = _ops()
    g = golden("activations")
    cfg = CA.cfg_for(tag, name)
    cfg.hidden_dropout_prob = 0.0
    B, L = cases.MODULE_BL[tag]
    d = cfg.hidden_size
    # plain inputs: the forward at the existing `ffn` bar (test_modules_vs_golden), inference and training path
    ff = _fill(FeedForward(cfg), f"{tag}.ffn.")
    assert ff.act == CA.CODES[name]
    x, res = T(recipe.uniform(f"{tag}.x", (B, L, d))).to(DEV), T(recipe.uniform(f"{tag}.res", (B, L, d))).to(DEV)
    gout = T(recipe.uniform(f"{tag}.gout", (B, L, d))).to(DEV)
    with torch.no_grad():
        e = abs_err(CA.sub_act(_np(ff.eval()(x, res))), g[f"ffn.{tag}.{name}.y"])
    assert e <= 1e-5, e
    xg, rg = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    y = ff.train()(xg, rg)
    e = abs_err(CA.sub_act(_np(y)), g[f"ffn.{tag}.{name}.y"])
    assert e <= 1e-5, e
    if tag == "micro" and name in CA.SMOOTH:
        # smooth activations: the fp32 gradient bar of test_layer_gradients_fp32_vs_reference (1e-4 of the tensor's scale)
        (y * gout).sum().backward()
        assert rel_err(CA.sub_act(_np(xg.grad)), g[f"ffn.{tag}.{name}.dx"]) < 1e-4
        assert rel_err(CA.sub_act(_np(rg.grad)), g[f"ffn.{tag}.{name}.dres"]) < 1e-4
        for n, p in ff.named_parameters():
            e = rel_err(CA.sub_grad(_np(p.grad)), g[f"ffn.{tag}.{name}.d.{n}"])
            assert e < 1e-4, (n, e)
    if name == "swish":
        return
    # kink inputs: bar = 2x the reference's own fp32-vs-fp64 gap + 1e-5, after the pre-activation check
    kt = CA.KINK_TAGS[tag]
    k = f"kink.{tag}.{name}"
    ff = _fill(FeedForward(cfg), f"{kt}.ffn.").train()
    x = T(recipe.uniform(f"{kt}.x", (B, L, d), scale=CA.KINK_SCALE)).to(DEV)
    res, gout = T(recipe.uniform(f"{kt}.res", (B, L, d))).to(DEV), T(recipe.uniform(f"{kt}.gout", (B, L, d))).to(DEV)
    pre = torch.zeros(B * L, 4 * d, device=DEV)
    ops.linear(x.reshape(B * L, d), ff.intermediate.weight.detach(), ff.intermediate.bias.detach(), act=ff.act, pre_out=pre)
    _check_pre_against_margin(g, f"kink.{tag}", pre)
    xg, rg = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    y = ff(xg, rg)
    (y * gout).sum().backward()
    report, bad = [], []

    def held(what, got, key):
        e, bar = abs_err(got, g[f"{k}.{key}"]), 2 * float(g[f"{k}.gap.{key}"][0]) + 1e-5
        report.append(f"{what}: err {e:.3e} bar {bar:.3e}")
        if e > bar:
            bad.append(report[-1])
    held("y", CA.sub_act(_np(y)), "y")
    if tag == "micro" or name in CA.WIDE_GRAD_NAMES:
        held("dx", CA.sub_act(_np(xg.grad)), "dx")
        held("dres", CA.sub_act(_np(rg.grad)), "dres")
        for n, p in ff.named_parameters():
            held(n, CA.sub_grad(_np(p.grad)), f"d.{n}")
    print(f"{k}: " + "; ".join(report))
    assert not bad, bad


def _layer_setup(cfg, prefix, xtag, gtag, dtype=torch.float32):
    from vyomai_amd.layers.mask import AttnMask
    from vyomai_amd.layers.positional_embeddings import RopeSlice, RopeTable
    from vyomai_amd.models.decoder import DecoderLayer
    tag = "micro" if cfg.hidden_size == 64 else "wide"
    B, L = cases.MODULE_BL[tag]
    d = cfg.hidden_size
    dh = d // cfg.num_attention_heads
    cfg.hidden_dropout_prob = 0.0
    layer = _fill(DecoderLayer(cfg, 0, None), prefix).train()
    x = T(recipe.uniform(f"{xtag}.x", (B, L, d))).to(DEV).to(dtype).requires_grad_(True)
    gout = T(recipe.uniform(f"{gtag}.gout", (B, L, d))).to(DEV).to(dtype)
    mask = AttnMask.from_padding(T(cases.keypad(B, L)).to(DEV), causal=True, start_pos=0, query_len=L)
    freqs = RopeSlice(RopeTable(O.rotary_angles(dh, cfg.max_position_embeddings)), 0, L)
    return layer, x, gout, mask, freqs


@pytest.mark.parametrize("name", CA.GRAD_NAMES)
def test_decoder_layer_fp32_vs_reference(golden, name):
    """test_layer_gradients_fp32_vs_reference's setup and bars (2e-5 / 1e-4 / 1e-4) per activation: the wide forward for
    every name, wide gradients for silu, micro gradients for the rest -- relu6 and leaky_relu on the margin-checked
    input, after the kernel's pre-activation has been checked against the reference's."""
    ops = _ops()
    g = golden("activations")
    layer, x, gout, mask, freqs = _layer_setup(CA.cfg_for("wide", name), "wide.layer.None.", "wide", "wide")
    assert layer.feed_forward.act == CA.CODES[name]
    y, _ = layer(x, mask, freqs)
    assert y.dtype == torch.float32
    e = rel_err(CA.sub_act(_np(y)), g[f"layer.wide.{name}.y"])
    assert e < 2e-5, e
    if name == "silu":
        k = "layer.wide.silu"
    else:
        xtag = CA.LAYER_KINK_TAGS[int(g["layer.kink.tag"][0])] if name in CA.KINKED else "micro"
        layer, x, gout, mask, freqs = _layer_setup(CA.cfg_for("micro", name), "micro.layer.None.", xtag, "micro")
        if name in CA.KINKED:
            with torch.no_grad():
                a, _ = layer.attention(hidden_state=x.detach(), attention_mask=mask, freqs=freqs)
                ff = layer.feed_forward
                pre = torch.zeros(a.shape[0] * a.shape[1], ff.intermediate.weight.shape[0], device=DEV)
                ops.linear(a.reshape(pre.shape[0], -1), ff.intermediate.weight, ff.intermediate.bias, act=ff.act, pre_out=pre)
            _check_pre_against_margin(g, "layer.kink", pre)
        y, _ = layer(x, mask, freqs)
        k = f"layer.micro.{name}"
        e = rel_err(CA.sub_act(_np(y)), g[f"{k}.y"])
        assert e < 2e-5, e
    (y * gout).sum().backward()
    e = rel_err(CA.sub_act(_np(x.grad)), g[f"{k}.dx"])
    assert e < 1e-4, e
    for n, p in layer.named_parameters():
        e = rel_err(CA.sub_grad(_np(p.grad)), g[f"{k}.d.{n}"])
        assert e < 1e-4, (n, e)


# ---- model level, fp32 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pos", ["rope", "absolute"])
@pytest.mark.parametrize("name", CA.GRAD_NAMES)
def test_decoder_model_fp32(golden, name, pos):
    """test_models_gpu.test_decoder_fp32 per activation: hidden states at 1e-5, logits at 2e-5, generate ids bit-exact
    in the three cache modes."""
    import vyomai_amd as V
    g = golden("activations")
    m = V.DecoderModel(CA.model_cfg(name), pos, None)
    recipe.load_recipe_(m)
    m = m.to(DEV).eval()
    ids, am = cases.reference_test_inputs()
    k = f"model.{pos}.{name}"
    with torch.no_grad():
        o = m(T(ids).to(DEV), T(am).to(DEV))
    e = abs_err(CA.sub_act(_np(o.hidden_state)), g[f"{k}.hidden"])
    assert e <= 1e-5, e
    e = abs_err(_np(CA.sub_logits(o.logits)), g[f"{k}.logits"])
    assert e <= 2e-5, e
    p = torch.tensor([[9226, 16, 5, 1296]], dtype=torch.long, device=DEV)
    a = torch.ones(1, 4, dtype=torch.long, device=DEV)
    for mode, kw in (("nocache", dict(use_cache=False)), ("dynamic", dict(use_cache=True)),
                     ("static", dict(use_cache=True, use_static_cache=True))):
        t = m.generate(p, a, **kw).cpu().numpy()
        assert np.array_equal(t, g[f"{k}.gen.{mode}"]), (mode, t, g[f"{k}.gen.{mode}"])


def test_vit_silu_fp32(golden):
    """The wiring through FeedForward outside the decoder (test_models_gpu.test_vit_and_vlm's bar)."""
    import vyomai_amd as V
    g = golden("activations")
    vcfg = cases.vit_cfg()
    vcfg.hidden_act = "silu"
    vit = V.Vit(vcfg)
    recipe.load_recipe_(vit)
    vit = vit.to(DEV).eval()
    img = T(recipe.uniform("vit.img", (2, 3, 224, 224), 0.5, 0.5)).to(DEV)
    with torch.no_grad():
        y = vit(img.clone()).logits
    assert abs_err(_np(CA.sub_vit(y)), g["vit.silu.out"]) <= 2e-5
    assert abs_err(_np(y[:, 0, :]), g["vit.silu.cls"]) <= 2e-5


# ---- bf16 -------------------------------------------------------------------------------------------------------------

def _oracle_layer_grads(cfg, sd, x, gout, dtype):
    """Autograd through the CPU oracle's block in `dtype` (vanilla attention, rotary, causal + key padding)."""
    B, L, d = x.shape
    dh = d // cfg.num_attention_heads
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = x.detach().clone().to(dtype).requires_grad_(True)
    freqs = O.rotary_angles(dh, cfg.max_position_embeddings)[:, :L]
    mask = T(cases.causal_additive(B, L, 0, cases.keypad(B, L))).to(dtype)
    y = O.block(sd, "", O.Cfg.of(cfg), x, mask, freqs, False)
    (y * gout.to(dtype)).sum().backward()
    out = {"y": y.detach().float(), "dx": x.grad.float()}
    out.update({n: p.grad.float() for n, p in sd.items()})
    return out


@pytest.mark.parametrize("name", CA.GRAD_NAMES)
def test_decoder_layer_bf16(golden, name):
    """The wide layer in bf16, forward and backward, against fp32 autograd through the CPU oracle (pinned to the reference
    by tests/test_activations_cpu.py).  Smooth activations: the bars of test_layer_gradients_vs_reference
    (3e-2 / 5e-2 / 6e-2 of the tensor's scale).  Kinked activations: 34 rows of 0 / 1 derivatives, a handful of which
    flip in any bf16 evaluation (the oracle's own bf16-on-CPU run is 2.2e-1 off its fp32 on
    feed_forward.intermediate.weight.grad), so each gradient is held to 2x the oracle's bf16-on-CPU gap + 1e-2 of the
    tensor's scale; the forward keeps 3e-2."""
    g = golden("activations")
    cfg = CA.cfg_for("wide", name)
    layer, x, gout, mask, freqs = _layer_setup(cfg, "wide.layer.None.", "wide", "wide", dtype=BF)
    y, _ = layer(x, mask, freqs)
    (y.float() * gout.float()).sum().backward()
    sd = {n: T(recipe.param_value("wide.layer.None." + n, s)) for n, s in cases.layer_shapes(cfg, "vanilla").items()}
    x0, g0 = x.detach().cpu(), gout.cpu()        # the bf16-rounded inputs the kernels saw
    ref = _oracle_layer_grads(cfg, sd, x0.float(), g0.float(), torch.float32)
    assert rel_err(CA.sub_act(ref["y"].numpy()), g[f"layer.wide.{name}.y"]) < 1e-2        # same case as the fixture
    got = {"y": y, "dx": x.grad}
    got.update({n: p.grad for n, p in layer.named_parameters()})
    assert rel_err(got["y"], ref["y"].numpy()) < 3e-2, rel_err(got["y"], ref["y"].numpy())
    if name in CA.SMOOTH:
        assert rel_err(got["dx"], ref["dx"].numpy()) < 5e-2
        for n, _ in layer.named_parameters():
            e = rel_err(got[n], ref[n].numpy())
            assert e < 6e-2, (n, e)
        return
    orc = _oracle_layer_grads(cfg, {n: v.to(BF) for n, v in sd.items()}, x0, g0, BF)
    report, bad = [], []
    for n in ["dx"] + [n for n, _ in layer.named_parameters()]:
        scale = float(ref[n].abs().max())
        e = abs_err(got[n], ref[n].numpy()) / scale
        gap_ = float((orc[n] - ref[n]).abs().max()) / scale
        report.append(f"{n}: HIP {e:.2e} oracle-bf16 {gap_:.2e}")
        if e > 2 * gap_ + 1e-2:
            bad.append(report[-1])
    print(f"{name}: " + "; ".join(report))
    assert not bad, bad


def test_silu_decoder_layer_at_the_benchmark_size_vs_oracle():
    """test_training_gpu.test_decoder_layer_at_the_benchmark_size_vs_oracle with hidden_act = "silu": the large-tile FFN1
    kernel's run-time-code epilogue with VY_ACT_SAVE_DERIV at M = 16384 and the dgrad that multiplies by the saved act'."""
    from vyomai_amd.layers.mask import AttnMask
    from vyomai_amd.layers.positional_embeddings import RopeSlice, RopeTable
    from vyomai_amd.models.decoder import DecoderLayer
    import vyomai_amd as V
    cfg = V.EncoderConfig(num_hidden_layers=1, max_position_embeddings=1024, hidden_dropout_prob=0.0, hidden_act="silu")
    B, L, d = 32, 512, cfg.hidden_size
    dh = d // cfg.num_attention_heads
    layer = DecoderLayer(cfg, 0, None)
    assert layer.feed_forward.act == CA.CODES["silu"]
    for n, t in layer.state_dict().items():
        t.copy_(T(recipe.param_value("big.layer." + n, tuple(t.shape))))
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in layer.state_dict().items()}
    layer = layer.to(DEV).train()
    x0 = T(recipe.uniform("big.x", (B, L, d))).to(BF)
    g0 = T(recipe.uniform("big.gout", (B, L, d))).to(BF)
    x = x0.to(DEV).requires_grad_(True)
    tab = O.rotary_angles(dh, cfg.max_position_embeddings)
    mask = AttnMask.from_padding(None, causal=True, start_pos=0, query_len=L)
    y, _ = layer(x, mask, RopeSlice(RopeTable(tab), 0, L))
    (y.float() * g0.to(DEV).float()).sum().backward()
    torch.cuda.synchronize()
    xr = x0.float().requires_grad_(True)
    add = O.decoder_additive_mask(B, L, None, 0, torch.float32)
    yr = O.block(sd, "", O.Cfg.of(cfg), xr, add, tab[:, :L], False)
    (yr * g0.float()).sum().backward()

    def rel(a, b):
        return float((a.detach().float().cpu() - b.detach()).abs().max() / (b.detach().abs().max() + 1e-12))

    def rel_rms(a, b):
        a, b = a.detach().float().cpu(), b.detach()
        return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12))
    assert rel(y, yr) < 3e-2, rel(y, yr)
    assert rel_rms(y, yr) < 6e-3, rel_rms(y, yr)
    assert rel(x.grad, xr.grad) < 6e-2, rel(x.grad, xr.grad)
    assert rel_rms(x.grad, xr.grad) < 1.5e-2, rel_rms(x.grad, xr.grad)
    for n, p in layer.named_parameters():
        e = rel(p.grad, sd[n].grad)
        assert e < 6e-2, (n, e)


# ---- decode -----------------------------------------------------------------------------------------------------------

def _decode_model(name, dtype=BF):
    import vyomai_amd as V
    cfg = V.EncoderConfig(num_hidden_layers=2, max_position_embeddings=256, hidden_dropout_prob=0.0, hidden_act=name)
    m = V.DecoderModel(cfg, "rope", None)
    recipe.load_recipe_(m)
    return cfg, m.to(DEV).to(dtype).eval()


@pytest.mark.parametrize("B", [32, 7])
@pytest.mark.parametrize("name", CA.GRAD_NAMES)
def test_lean_decode_step_matches_general_and_fp32(name, B):
    """test_decode_lean_gpu.test_lean_step_matches_general_and_fp32, same bars, per activation.  The general step runs
    vy_linear_fwd, which refuses codes it does not know; a lean kernel that sent a new code to the identity (what
    the decode projection did before it knew them) is far outside these bars."""
    from tests.test_decode_lean_gpu import _plan, _step
    torch.manual_seed(1)
    cfg, m = _decode_model(name)
    x = (torch.randn(B, cfg.hidden_size) * 0.5).to(BF).to(DEV)
    pos = 37
    plan, cache = _plan(cfg, m, B, BF)
    assert plan.plan.act == CA.CODES[name]
    lg_lean, hd_lean, kv_lean = _step(plan, cache, x, pos, 1)
    plan2, cache2 = _plan(cfg, m, B, BF)
    lg_gen, hd_gen, kv_gen = _step(plan2, cache2, x, pos, 0)
    for (k1, v1), (k2, v2) in zip(kv_lean, kv_gen):
        assert (k1 - k2).abs().max() <= 4e-2 and (v1 - v2).abs().max() <= 4e-2
    assert (k1 - k2).abs().mean() <= 1e-3
    assert (hd_lean - hd_gen).abs().mean() <= 5e-3, (hd_lean - hd_gen).abs().mean()
    assert (lg_lean - lg_gen).abs().mean() <= 2e-2, (lg_lean - lg_gen).abs().mean()
    cfg32, m32 = _decode_model(name, dtype=torch.float32)
    plan32, cache32 = _plan(cfg32, m32, B, torch.float32)
    lg32, hd32, _ = _step(plan32, cache32, x.float(), pos, 1)
    e_lean = (hd_lean - hd32).abs().mean().item()
    e_gen = (hd_gen - hd32).abs().mean().item()
    assert e_lean <= 1.25 * e_gen + 1e-3, (e_lean, e_gen)
    el, eg = (lg_lean - lg32).abs().mean().item(), (lg_gen - lg32).abs().mean().item()
    assert el <= 1.25 * eg + 2e-3, (el, eg)
    # and the activation is really applied: the same plan with the identity's code is a different function
    plan3, cache3 = _plan(cfg, m, B, BF)
    plan3.plan.act = 0
    _, hd_id, _ = _step(plan3, cache3, x, pos, 1)
    assert (hd_id - hd_lean).abs().mean() > 10 * max((hd_lean - hd_gen).abs().mean().item(), 1e-3)


def test_silu_decode_graph_replay_matches_eager(monkeypatch):
    cfg, m = _decode_model("silu")
    ids = torch.from_numpy(recipe.token_ids("lean.ids", (5, 20), 3, cfg.vocab_size)).to(DEV)
    am = torch.ones_like(ids)
    monkeypatch.setenv("VY_DECODE_GRAPH", "1")
    t_graph = m.generate(ids, am, max_len=10, use_cache=True, use_static_cache=True)
    monkeypatch.setenv("VY_DECODE_GRAPH", "0")
    t_eager = m.generate(ids, am, max_len=10, use_cache=True, use_static_cache=True)
    t_dyn = m.generate(ids, am, max_len=10, use_cache=True, use_static_cache=False)
    assert torch.equal(t_graph, t_eager)
    assert torch.equal(t_graph, t_dyn)
