"""Single-sequence Gemma decode on fp8 weights (GemmaDecodePlan(weight_dtype="fp8"), vy_gemma_decoder_step_w8) on the MI355X.

Which chain ran is asserted before any number is compared: vy_debug_gemma_w8_last == (layers, 1) and the launches in
order.  Two kinds of weights:

  lossless   every projection row (and every row of the vocabulary matrix) is code * 2^k with one +-448 code in it, the
             norm weights are 0: the fp8 plan, the bf16 plans and the fp32 plan hold the same numbers (asserted on the
             plan's dequantised matrices), so the fp8 step is held to the bars test_paligemma_gpu.py sets for the lean
             bf16 chain: mean error against the fp32 step <= 1.3 e_general + 2e-3 scale, the K and V rows written at
             `pos` within 0.05 max(1, |.|) of the general chain's.
  recipe     recipe.param_value weights.  The reference is the fp32 plan on a model rebuilt from plan.dequantized()
             (projections split back out; norm weights 0 where the plan folded them into the codes), so that quantisation
             itself is outside the comparison.  Same bars; e_general is the general bf16 chain's error on the ORIGINAL
             weights against the fp32 step on them (the bf16 error level of the shape, no part of it from the code under
             test), and the K / V rows are held to the fp32 reference's, which has the fp8 plan's numbers.  The error
             against the original fp32 model -- what quantisation costs -- is printed, not asserted."""
import copy
import ctypes as C
import types

import pytest
import torch

from tests.golden import cases
from tests.test_paligemma_gpu import T, _one_layer
from vyomai_amd import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
POS = 40

SHAPES = [                                   # test_gemma_step_chains_one_layer's first four, then the two-layer stack
    (2048, 8, 1, 256, 16384, False),
    (4096, 16, 2, 256, 4096, True),
    (2048, 32, 4, 256, 8192, False),
    (8192, 8, 1, 256, 2048, False),
    "two_layer",
]


def _cfg(shape):
    if shape == "two_layer":
        return dict(cases.GEMMA, num_hidden_layers=2, vocab_size=4096), "pgl."
    d, h, hk, dh, ffn, bias = shape
    return _one_layer(d, h, hk, dh, ffn, bias), f"pg1.{d}.{h}.{ffn}."


def _dbg():
    from vyomai_amd import _lib
    lib = _lib.load()
    lib.vy_debug_set_gemma_lean.argtypes = [C.c_int]
    lib.vy_debug_gemma_w8_trace.argtypes, lib.vy_debug_gemma_w8_trace.restype = [C.POINTER(C.c_int), C.c_int], C.c_int
    return lib


def w8_last():
    lib, out, tr = _dbg(), (C.c_int * 2)(), (C.c_int * 64)()
    lib.vy_debug_gemma_w8_last(out)
    n = lib.vy_debug_gemma_w8_trace(tr, 64)
    return tuple(out), list(tr)[:n]


def _lossless_(w, g):
    """In place: every row code * 2^k with one +-448 in it; k puts a row product of unit-variance x near unit size (the
    root mean square of the 254 code values is ~99) and differs from row to row."""
    N, K = w.shape
    codes = torch.randint(0, 254, (N, K), generator=g)
    codes = (codes + (codes >= 127).long()).clamp(max=254).to(torch.uint8)        # skip 0x7F; 0xFF is never drawn
    val = codes.view(torch.float8_e4m3fn).float()
    val[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = 448.0 * (1 - 2 * (torch.arange(N) & 1)).float()
    k = -torch.round(torch.log2(torch.tensor(99.0 * K ** 0.5))) - (torch.arange(N) % 3)
    w.copy_(val * torch.exp2(k)[:, None])


def _models(shape, kind):
    from vyomai_amd.models import paligemma as P
    cfg, prefix = _cfg(shape)
    vis = P.SiglipVisionConfig(**dict(cases.SIGLIP, num_hidden_layers=1))
    txt = types.SimpleNamespace(**cfg)
    m32 = P.PaliGemmaForConditionalGeneration(P.PaliGemmaShape(vis, txt, txt.hidden_size))
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n, p in m32.named_parameters():
            if n.startswith("vision_tower.") or n.startswith("multi_modal_projector."):
                continue                                           # no part of a decode step
            streamed = n.startswith("layers.") and n.endswith("_proj.weight") or n == "embed_tokens.weight"
            if kind == "lossless" and streamed:
                _lossless_(p, g)
            elif kind == "lossless" and (n.endswith("layernorm.weight") or n == "norm.weight"):
                p.zero_()
            else:
                p.copy_(T(recipe.param_value(prefix + n, tuple(p.shape))))
                if kind == "lossless":
                    p.copy_(p.to(torch.bfloat16).float())          # biases: the same numbers in both precisions
    m16 = copy.deepcopy(m32).to(DEV).to(torch.bfloat16).eval()
    return m32.to(DEV).eval(), m16, txt


def _caches(txt, dt):
    g = torch.Generator().manual_seed(3)
    hk, dh = txt.num_key_value_heads, txt.head_dim
    return [(torch.randn(1, hk, 64, dh, generator=g).to(dt).to(DEV), torch.randn(1, hk, 64, dh, generator=g).to(dt).to(DEV))
            for _ in range(txt.num_hidden_layers)]


def _run(model, txt, x, **kw):
    """One step at POS on fresh caches -> (logits fp32, K rows, V rows, plan)."""
    from vyomai_amd.decode_plan import GemmaDecodePlan
    dt = model.embed_tokens.weight.dtype
    cs = _caches(txt, dt)
    plan = GemmaDecodePlan(model, cs, 1, **kw)
    out = plan.step(x.to(dt).to(DEV), POS).float().clone()
    torch.cuda.synchronize()
    return out, [c[0][:, :, POS].float().clone() for c in cs], [c[1][:, :, POS].float().clone() for c in cs], plan


def _rebuilt(m32, plan, txt, prescale):
    """The fp32 model that holds the fp8 plan's numbers: projections from plan.dequantized(), split back out."""
    m = copy.deepcopy(m32)
    deq = plan.dequantized()
    nq, nkv, ffn = txt.num_attention_heads * txt.head_dim, txt.num_key_value_heads * txt.head_dim, txt.intermediate_size
    with torch.no_grad():
        for i, layer in enumerate(m.layers):
            a, mlp = layer.self_attn, layer.mlp
            wqkv, wgu = deq[f"layers.{i}.wqkv"], deq[f"layers.{i}.wgu"]
            a.q_proj.weight.copy_(wqkv[:nq]); a.k_proj.weight.copy_(wqkv[nq:nq + nkv]); a.v_proj.weight.copy_(wqkv[nq + nkv:])
            a.o_proj.weight.copy_(deq[f"layers.{i}.wo"])
            mlp.gate_proj.weight.copy_(wgu[:ffn]); mlp.up_proj.weight.copy_(wgu[ffn:])
            mlp.down_proj.weight.copy_(deq[f"layers.{i}.wdown"])
            for norm in (layer.input_layernorm, layer.post_attention_layernorm):
                if prescale:                                   # the codes carry (1 + w) of both norms
                    norm.weight.zero_()
                else:                                          # the step reads bf16 norm weights
                    norm.weight.copy_(norm.weight.to(torch.bfloat16).float())
            for lin in (a.q_proj, a.k_proj, a.v_proj, a.o_proj):   # the step reads bf16 biases
                if lin.bias is not None:
                    lin.bias.copy_(lin.bias.to(torch.bfloat16).float())
        m.norm.weight.copy_(m.norm.weight.to(torch.bfloat16).float())
        m.embed_tokens.weight.copy_(deq["head"])
    return m


@pytest.mark.parametrize("kind", ["lossless", "recipe"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: str(v))
def test_w8_step_chain_and_bars(shape, kind):
    lib = _dbg()
    m32, m16, txt = _models(shape, kind)
    nl = txt.num_hidden_layers
    x = torch.randn(1, txt.hidden_size, generator=torch.Generator().manual_seed(4)) * 0.3
    try:
        lib.vy_debug_set_gemma_lean(0)
        gen, gen_k, gen_v, _ = _run(m16, txt, x, prescale=False)
    finally:
        lib.vy_debug_set_gemma_lean(1)
    ref, ref_k, ref_v, _ = _run(m32, txt, x)
    scale = ref.abs().mean().item()
    e_general = (gen - ref).abs().mean().item()
    assert e_general < 0.05 * scale + 1e-3, (e_general, scale)      # the bf16 error level of the general chain
    for prescale in (True, False):
        out, ks, vs, plan = _run(m16, txt, x, prescale=prescale, weight_dtype="fp8")
        last, trace = w8_last()
        per_layer = [2, 3, 4, 5, 4] if prescale else [1, 2, 3, 4, 1, 5, 4]
        assert last == (nl, 1) and trace == per_layer * nl + [1, 4], (last, trace)
        assert torch.isfinite(out).all()
        if kind == "lossless":
            deq = plan.dequantized()
            L0 = m16.layers[0]
            assert torch.equal(deq["layers.0.wo"], L0.self_attn.o_proj.weight.float())
            assert torch.equal(deq["layers.0.wgu"][: txt.intermediate_size], L0.mlp.gate_proj.weight.float())
            assert torch.equal(deq["head"], m32.embed_tokens.weight) and torch.equal(deq["head"], m16.embed_tokens.weight.float())
            want, want_k, want_v = ref, gen_k, gen_v
        else:
            want, want_k, want_v, _ = _run(_rebuilt(m32, plan, txt, prescale), txt, x)
            e_orig = (out - ref).abs().mean().item()
            print(f"quantisation {shape} prescale={prescale}: mean |logits - fp32 original| = {e_orig:.4e} "
                  f"({e_orig / scale:.4f} of mean |logits| {scale:.4e}; general bf16 chain: {e_general / scale:.4f})")
        e = (out - want).abs().mean().item()
        print(f"w8 step {shape} {kind} prescale={prescale}: e_fp8 {e:.4e} e_general {e_general:.4e} scale {scale:.4e}")
        assert e <= 1.3 * e_general + 2e-3 * scale, (e, e_general, scale)
        for a, b in zip(ks + vs, want_k + want_v):
            assert (a - b).abs().max().item() <= 0.05 * max(1.0, b.abs().max().item()), (prescale, "k / v rows")
        del plan


def test_plan_bytes_and_construction_errors():
    """weight_bytes of the fp8 plan is (K + 4) / (2 K) of the bf16 plan's, matrix by matrix; batch 2 and an fp32 model are
    ValueErrors at construction; a w8 plan has no bf16 head pointer for the bf16 step to read."""
    from vyomai_amd.decode_plan import GemmaDecodePlan
    m32, m16, txt = _models((2048, 8, 1, 256, 16384, False), "recipe")
    cs = _caches(txt, torch.bfloat16)
    p16 = GemmaDecodePlan(m16, cs, 1)
    p8 = GemmaDecodePlan(m16, cs, 1, weight_dtype="fp8")
    K = {"wqkv": 2048, "wo": 2048, "wgu": 2048, "wdown": 16384, "head": 2048}
    assert set(p16.weight_bytes) == set(p8.weight_bytes) == {"layers.0.wqkv", "layers.0.wo", "layers.0.wgu", "layers.0.wdown", "head"}
    for name, b8 in p8.weight_bytes.items():
        k = K[name.split(".")[-1]]
        assert b8 * 2 * k == p16.weight_bytes[name] * (k + 4), name
    assert p8.plan.head_w is None and p8.w8 is not None and p16.w8 is None
    with pytest.raises(ValueError, match="batch 1"):
        GemmaDecodePlan(m16, cs, 2, weight_dtype="fp8")
    with pytest.raises(ValueError, match="bf16 model"):
        GemmaDecodePlan(m32, _caches(txt, torch.float32), 1, weight_dtype="fp8")
    with pytest.raises(ValueError, match="dequantized"):
        p16.dequantized()


def test_generate_with_fp8_weights_runs_and_reuses_the_plan():
    """generate(..., weight_dtype="fp8") on the shape of test_paligemma_shape_generate_bf16_runs: tokens in range and of
    the right shape; a second call reuses the plan; the option is part of the generation-state key."""
    from vyomai_amd.models import paligemma as P
    vis = P.SiglipVisionConfig(**dict(cases.SIGLIP, num_hidden_layers=2))
    txt = types.SimpleNamespace(**dict(cases.GEMMA, num_hidden_layers=2, vocab_size=4096))
    m = P.PaliGemmaForConditionalGeneration(P.PaliGemmaShape(vis, txt, txt.hidden_size))
    for n, p in m.named_parameters():
        with torch.no_grad():
            p.copy_(T(recipe.param_value("pgm." + n, tuple(p.shape))))
    m = m.to(DEV).to(torch.bfloat16).eval()
    img = T(recipe.uniform("pgm.img", (1, 3, 224, 224), 0.5, 0.5)).to(DEV)
    ids = T(recipe.token_ids("pgm.ids", (1, 8), 3, 4096)).to(DEV)
    out = m.generate(img, ids, max_new_tokens=6, max_cache_len=384, weight_dtype="fp8")
    assert out.shape == (1, 6) and int(out.min()) >= 0 and int(out.max()) < 4096
    assert w8_last()[0] == (2, 1)
    plan = m._gen_state["plan"]
    assert plan.w8 is not None
    out2 = m.generate(img, ids, max_new_tokens=6, max_cache_len=384, weight_dtype="fp8")
    assert m._gen_state["plan"] is plan and torch.equal(out, out2)
    m.generate(img, ids, max_new_tokens=2, max_cache_len=384)
    assert m._gen_state["plan"] is not plan and m._gen_state["plan"].w8 is None
