"""Pin the CPU oracle against outputs of the real reference (tests/golden/*.npz).

No GPU.  fp32 bar: 2e-6 abs on O(1) activations (identical aten ops, different call
structure); token ids bit-exact.
"""
import numpy as np
import pytest
import torch

from oracle import vyom_oracle as O
from tests.golden import cases
from vyomai_amd import recipe

ATOL = 2e-6


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def sd_from(shapes, prefix=""):
    """name->tensor with recipe values; recipe key = prefix + name."""
    return {n: T(recipe.param_value(prefix + n, s)) for n, s in shapes.items()}


def close(got, want, atol=ATOL, what=""):
    got = got.detach().float().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol}"


@pytest.mark.parametrize("tag", ["micro", "wide"])
def test_modules(golden, tag):
    g = golden("modules")
    cfg = cases.micro_cfg() if tag == "micro" else cases.wide_cfg()
    c = O.Cfg.of(cfg)
    B, L = cases.MODULE_BL[tag]
    d, h = cfg.hidden_size, cfg.num_attention_heads
    dh = d // h
    x = T(recipe.uniform(f"{tag}.x", (B, L, d)))
    res = T(recipe.uniform(f"{tag}.res", (B, L, d)))
    keypad = cases.keypad(B, L)
    add_mask = O.padding_additive_mask(T(keypad).float(), torch.float32)
    full_freqs = O.rotary_angles(dh, cfg.max_position_embeddings)
    freqs = full_freqs[:, :L]
    close(freqs, g[f"{tag}.rope.angles"], 0, "angles")

    q = T(recipe.uniform(f"{tag}.q", (B, h, L, dh)))
    k = T(recipe.uniform(f"{tag}.k", (B, h, L, dh)))
    qe, ke = O.apply_rotary(q, k, freqs)
    close(qe, g[f"{tag}.rope.q"], 0, "rope.q")
    close(ke, g[f"{tag}.rope.k"], 0, "rope.k")

    sd = sd_from(cases.ffn_shapes(cfg), f"{tag}.ffn.")
    close(O.feed_forward(sd, "", c, x, res), g[f"{tag}.ffn"], what="ffn")
    sd = sd_from(cases.aso_shapes(cfg), f"{tag}.aso.")
    close(O.attention_self_output(sd, "", x, res, 1e-5), g[f"{tag}.aso"], what="aso")

    for name, kind in (("enc", "vanilla"), ("encgqa", "gqa"), ("vis", "vision")):
        sd = sd_from(cases.attn_shapes(cfg, kind), f"{tag}.{name}.")
        kw = dict(gqa=kind == "gqa", fused_qkv=kind == "vision")
        close(O.self_attention(sd, "", c, x, add_mask, None, **kw), g[f"{tag}.{name}.keypad"], what=name)
        close(O.self_attention(sd, "", c, x, None, None, **kw), g[f"{tag}.{name}.nomask"], what=name)
        close(O.self_attention(sd, "", c, x, add_mask, freqs, **kw), g[f"{tag}.{name}.keypad.rope"], what=name)

    for name, gqa in (("dec", False), ("decgqa", True)):
        sd = sd_from(cases.attn_shapes(cfg, "gqa" if gqa else "vanilla"), f"{tag}.{name}.")
        heads = cfg.num_key_value_heads if gqa else h
        for cname in ("static", "dynamic"):
            cache = (O.OracleStaticCache(1, B, heads, L + 3, dh) if cname == "static"
                     else O.OracleDynamicCache(1))
            causal = T(cases.causal_additive(B, L, 0, None))
            y = O.self_attention(sd, "", c, x, causal, freqs, gqa, cache=cache, start_pos=0)
            close(y, g[f"{tag}.{name}.{cname}.prefill"], what=f"{name}.{cname}.prefill")
            for s in range(3):
                xs = T(recipe.uniform(f"{tag}.xstep{s}", (B, 1, d)))
                y = O.self_attention(sd, "", c, xs, None, full_freqs[:, L + s:L + s + 1], gqa,
                                     cache=cache, start_pos=L + s)
                close(y, g[f"{tag}.{name}.{cname}.step{s}"], what=f"{name}.{cname}.step{s}")
            if cname == "static":
                close(cache.k[0], g[f"{tag}.{name}.static.kcache"], what="kcache")
                close(cache.v[0], g[f"{tag}.{name}.static.vcache"], what="vcache")
        cache = O.OracleDynamicCache(1)
        y0 = O.self_attention(sd, "", c, x[:, :L - 5], T(cases.causal_additive(B, L - 5, 0, keypad[:, :L - 5])),
                              full_freqs[:, :L - 5], gqa, cache=cache, start_pos=0)
        y1 = O.self_attention(sd, "", c, x[:, L - 5:], T(cases.causal_additive(B, 5, L - 5, keypad)),
                              full_freqs[:, L - 5:L], gqa, cache=cache, start_pos=L - 5)
        close(y0, g[f"{tag}.{name}.chunk0"], what="chunk0")
        close(y1, g[f"{tag}.{name}.chunk1"], what="chunk1")


@pytest.mark.parametrize("pos,at", [("absolute", None), ("rope", None), ("sinusoidal", "gqa"), ("rope", "gqa")])
def test_encoder_config1(golden, pos, at):
    """BASELINE.json configs[0]: EncoderModel(EncoderConfig default) B=4 seq=128 on CPU."""
    g = golden("encoder")
    cfg = cases.with_kv(cases.test_cfg(), at)
    sd = sd_from(cases.text_model_shapes(cfg, pos, at, head=False))
    ids = T(recipe.token_ids("enc.ids", (4, 128), 3, cfg.vocab_size))
    am = T(cases.keypad(4, 128)).float()
    c = O.Cfg.of(cfg)
    y = O.encoder_forward(sd, c, ids, am, pos, at)
    close(cases.sub(y), g[f"encoder.{pos}.{at}.pad"], what="enc.pad")
    s = g[f"encoder.{pos}.{at}.pad.sum"]
    assert abs(y.double().sum().item() - s[0]) < 1e-2 and abs(y.double().abs().sum().item() - s[1]) < 1e-1
    close(cases.sub(O.encoder_forward(sd, c, ids, None, pos, at)), g[f"encoder.{pos}.{at}.full_nopad"],
          what="enc.nopad")


@pytest.mark.parametrize("pos", ["absolute", "sinusoidal", "rope"])
@pytest.mark.parametrize("at", [None, "gqa"])
def test_decoder_models(golden, pos, at):
    g = golden("models_text")
    cfg = cases.with_kv(cases.test_cfg(), at)
    sd = sd_from(cases.text_model_shapes(cfg, pos, at, head=True))
    c = O.Cfg.of(cfg)
    ids, am = cases.reference_test_inputs()
    o = O.decoder_forward(sd, c, T(ids), T(am), pos, at)
    close(o.hidden_state, g[f"decoder.{pos}.{at}.hidden"], what="hidden")
    close(o.logits[:, :, ::97], g[f"decoder.{pos}.{at}.logits"], 5e-6, what="logits")
    p = torch.tensor([[9226, 16, 5, 1296]], dtype=torch.long)
    a = torch.ones(1, 4)
    for mode, kw in (("nocache", dict(use_cache=False)), ("dynamic", dict(use_cache=True)),
                     ("static", dict(use_cache=True, use_static_cache=True))):
        t = O.decoder_generate(sd, c, p, a, 5, pos, at, **kw)
        assert np.array_equal(t.numpy(), g[f"decoder.{pos}.{at}.gen.{mode}"]), mode
    pb = T(recipe.token_ids("dec.prompt3", (3, 9), 3, cfg.vocab_size))
    ab = torch.ones(3, 9)
    t = O.decoder_generate(sd, c, pb, ab, 6, pos, at, use_cache=True, use_static_cache=True)
    assert np.array_equal(t.numpy(), g[f"decoder.{pos}.{at}.gen3.static"])
    if pos == "rope" and at is None:
        t = O.generate(sd, c, p, 4, pos, at)
        assert np.array_equal(t.numpy(), g["decoder.rope.None.utilsgen"])
        t = O.decoder_generate(sd, c, pb, ab, 6, pos, at, use_cache=False)
        assert np.array_equal(t.numpy(), g[f"decoder.{pos}.{at}.gen3.nocache"])


def test_reference_cache_modes_agree(golden):
    """The strong form of the reference's (weak) cache-consistency asserts
    (tests/test_decoder.py:161-163): all three modes give identical ids in fp32."""
    g = golden("models_text")
    for pos in ("absolute", "sinusoidal", "rope"):
        for at in (None, "gqa"):
            a, b, c = (g[f"decoder.{pos}.{at}.gen.{m}"] for m in ("nocache", "dynamic", "static"))
            assert np.array_equal(a, b) and np.array_equal(a, c), (pos, at)


def test_vit_and_vlm(golden):
    g = golden("models_vision")
    vcfg = cases.vit_cfg()
    img = T(recipe.uniform("vit.img", (2, 3, 224, 224), 0.5, 0.5))
    vsd = sd_from(cases.vit_shapes(vcfg))
    y = O.vit_forward(vsd, vcfg, img)
    close(cases.sub(y), g["vit.out"], 5e-6, what="vit")
    close(y[:, 0, :], g["vit.cls"], 5e-6, what="vit.cls")
    ids, am = cases.reference_test_inputs()
    for pos, at in (("absolute", None), ("rope", "gqa"), ("rope", None)):
        cfg = cases.with_kv(cases.test_cfg(), at)
        c = O.Cfg.of(cfg)
        # VisionLanguageModel state_dict = encoder.* + decoder.*
        esd = sd_from(cases.vit_shapes(vcfg, "encoder."))
        esd = {k[len("encoder."):]: v for k, v in esd.items()}
        dsd = sd_from(cases.text_model_shapes(cfg, pos, at, head=True, p="decoder."))
        dsd = {k[len("decoder."):]: v for k, v in dsd.items()}
        enc = O.vit_forward(esd, vcfg, img)[:, 0, :]
        lg = O.vlm_decoder_forward(dsd, c, T(ids[:2]), T(am[:2]), enc, pos, at)
        close(lg[:, :, ::97], g[f"vlm.{pos}.{at}.logits"], 1e-5, what="vlm.logits")
        enc1 = O.vit_forward(esd, vcfg, img[:1])[:, 0, :]
        close(enc1, g[f"vlm.{pos}.{at}.enc"], 5e-6, what="vlm.enc")
        idx = torch.tensor([[0]])
        dh = cfg.hidden_size // cfg.num_attention_heads
        heads = cfg.num_key_value_heads if at == "gqa" else cfg.num_attention_heads
        t0 = O.generate_multimodel(dsd, c, enc1, idx, 8, pos, at)
        t1 = O.generate_multimodel(dsd, c, enc1, idx, 8, pos, at,
                                   cache=O.OracleStaticCache(cfg.num_hidden_layers, 1, heads,
                                                             cfg.max_position_embeddings, dh))
        t2 = O.generate_multimodel(dsd, c, enc1, idx, 8, pos, at,
                                   cache=O.OracleDynamicCache(cfg.num_hidden_layers))
        assert np.array_equal(t0.numpy(), g[f"vlm.{pos}.{at}.gen.nocache"])
        assert np.array_equal(t1.numpy(), g[f"vlm.{pos}.{at}.gen.static"])
        assert np.array_equal(t2.numpy(), g[f"vlm.{pos}.{at}.gen.dynamic"])


@pytest.mark.parametrize("tag", ["micro", "wide"])
@pytest.mark.parametrize("at", [None, "gqa"])
def test_gradients(golden, tag, at):
    """Autograd through the oracle == autograd through the reference (one decoder layer)."""
    g = golden("grads")
    cfg = cases.micro_cfg() if tag == "micro" else cases.wide_cfg()
    c = O.Cfg.of(cfg)
    B, L = cases.MODULE_BL[tag]
    d = cfg.hidden_size
    dh = d // cfg.num_attention_heads
    sd = sd_from(cases.layer_shapes(cfg, "gqa" if at == "gqa" else "vanilla"), f"{tag}.layer.{at}.")
    for v in sd.values():
        v.requires_grad_(True)
    x = T(recipe.uniform(f"{tag}.x", (B, L, d))).requires_grad_(True)
    gout = T(recipe.uniform(f"{tag}.gout", (B, L, d)))
    freqs = O.rotary_angles(dh, cfg.max_position_embeddings)[:, :L]
    mask = T(cases.causal_additive(B, L, 0, cases.keypad(B, L)))
    y = O.block(sd, "", c, x, mask, freqs, at == "gqa")
    (y * gout).sum().backward()
    close(y, g[f"{tag}.{at}.y"], what="y")
    close(x.grad, g[f"{tag}.{at}.dx"], 2e-5, what="dx")
    for n, p in sd.items():
        want = g[f"{tag}.{at}.d.{n}"]
        got = p.grad if p.grad.numel() <= 4096 else cases.sub2(p.grad)
        scale = max(1.0, float(np.abs(want).max()))
        close(got, want, 2e-5 * scale, what=n)


@pytest.mark.parametrize("pos,at", [("absolute", None), ("sinusoidal", None), ("rope", None), ("rope", "gqa")])
def test_seq2seq_models(golden, pos, at):
    """EncoderDecoderModel (self-attention -> cross-attention -> FFN): logits with and without masks,
    greedy generate_seq2seq token-exact in the no-cache / static / dynamic cache modes."""
    g = golden("seq2seq")
    cfg = cases.with_kv(cases.test_cfg(), at)
    sd = sd_from(cases.s2s_model_shapes(cfg, pos, at))
    c = O.Cfg.of(cfg)
    ids, am = cases.reference_test_inputs()
    ids, am = T(ids), T(am)
    logits, enc = O.encoder_decoder_forward(sd, c, c, ids, am, ids, am, enc_pos=pos, enc_attn=at, dec_pos=pos,
                                            dec_attn=at)
    close(enc[:, :, ::4], g[f"s2s.{pos}.{at}.enc"], what="enc")
    close(logits[:, :, ::97], g[f"s2s.{pos}.{at}.logits"], 5e-6, what="logits")
    l2, _ = O.encoder_decoder_forward(sd, c, c, ids, None, ids[:, :9], None, enc_pos=pos, enc_attn=at,
                                      dec_pos=pos, dec_attn=at)
    close(l2[:, :, ::97], g[f"s2s.{pos}.{at}.logits.nomask"], 5e-6, what="logits.nomask")
    enc_sd = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    e1 = O.encoder_forward(enc_sd, c, ids[:1], am[:1], pos, at)
    start = torch.tensor([[0]], dtype=torch.long)
    t = O.generate_seq2seq(sd, c, c, e1, am[:1], start, 7, pos, at, use_cache=False)
    assert np.array_equal(t.numpy(), g[f"s2s.{pos}.{at}.gen.nocache"])
    t = O.generate_seq2seq(sd, c, c, e1, am[:1], start, 7, pos, at, use_cache=True)
    assert np.array_equal(t.numpy(), g[f"s2s.{pos}.{at}.gen.static"])
    assert np.array_equal(t.numpy(), g[f"s2s.{pos}.{at}.gen.dynamic"])


@pytest.mark.parametrize("tag", ["micro", "wide"])
@pytest.mark.parametrize("at", [None, "gqa"])
def test_seq2seq_layer_gradients(golden, tag, at):
    """Autograd through the oracle == autograd through the reference (one Seq2SeqDecoderLayer,
    gradients w.r.t. the decoder state, the ENCODER output and every parameter)."""
    g = golden("seq2seq")
    cfg = cases.micro_cfg() if tag == "micro" else cases.wide_cfg()
    c = O.Cfg.of(cfg)
    B, L = cases.MODULE_BL[tag]
    S = L + 5
    d = cfg.hidden_size
    dh = d // cfg.num_attention_heads
    sd = sd_from(cases.s2s_layer_shapes(cfg, "gqa" if at == "gqa" else "vanilla"), f"{tag}.s2slayer.{at}.")
    for v in sd.values():
        v.requires_grad_(True)
    x = T(recipe.uniform(f"{tag}.s2s.x", (B, L, d))).requires_grad_(True)
    enc = T(recipe.uniform(f"{tag}.s2s.enc", (B, S, d))).requires_grad_(True)
    gout = T(recipe.uniform(f"{tag}.s2s.gout", (B, L, d)))
    freqs = O.rotary_angles(dh, cfg.max_position_embeddings)[:, :L]
    mask = T(cases.causal_additive(B, L, 0, cases.keypad(B, L)))
    emask = T((1.0 - cases.keypad(B, S)[:, None, None, :].astype(np.float32)) * cases.FMIN)
    a = O.self_attention(sd, "attention.", c, x, mask, freqs, at == "gqa")
    cr = O.cross_attention(sd, "cross_attention.", c, a, enc, emask, at == "gqa")
    y = O.feed_forward(sd, "feed_forward.", c, cr, x)
    (y * gout).sum().backward()
    close(y, g[f"grad.{tag}.{at}.y"], what="y")
    close(x.grad, g[f"grad.{tag}.{at}.dx"], 2e-5, what="dx")
    close(enc.grad, g[f"grad.{tag}.{at}.denc"], 2e-5, what="denc")
    for n, p in sd.items():
        want = g[f"grad.{tag}.{at}.d.{n}"]
        got = p.grad if p.grad.numel() <= 4096 else cases.sub2(p.grad)
        scale = max(1.0, float(np.abs(want).max()))
        close(got, want, 2e-5 * scale, what=n)


def test_paligemma_blocks(golden):
    """SigLIP and Gemma layers (true widths) vs the exec'd notebook cells."""
    g = golden("paligemma_blocks")
    S, G = cases.SIGLIP, cases.GEMMA
    sd = sd_from(cases.siglip_layer_shapes(), "pg.siglip.")
    x = T(recipe.uniform("pg.siglip.x", (2, 20, S["hidden_size"])))
    y = O.siglip_layer(sd, "", x, S["num_attention_heads"], S["layer_norm_eps"])
    close(cases.sub2(y.reshape(-1, y.shape[-1])), g["siglip.layer"], 1e-5, "siglip layer")
    sd = sd_from(cases.gemma_layer_shapes(), "pg.gemma.")
    xg = T(recipe.uniform("pg.gemma.x", (2, 12, G["hidden_size"])))
    args = (G["num_attention_heads"], G["num_key_value_heads"], G["head_dim"], G["rms_norm_eps"])
    causal = T(cases.causal_additive(2, 12, 0, None))
    for key, mask, pos0 in (("nomask", None, 0), ("causal", causal, 0), ("pos7", causal, 7)):
        y = O.gemma_layer(sd, "", xg, *args, mask, pos0)
        want = g[f"gemma.layer.{key}"]
        got = cases.sub2(y.reshape(-1, y.shape[-1]))
        scale = max(1.0, float(np.abs(want).max()))
        close(got, want, 2e-5 * scale, f"gemma layer {key}")
    w = T(recipe.param_value("pg.norm.weight", (G["hidden_size"],)))
    y = O.rms_norm_gemma(xg, w, G["rms_norm_eps"])
    close(cases.sub2(y.reshape(-1, y.shape[-1])), g["gemma.rmsnorm"], 2e-6, "rmsnorm")


# ---- sampling processors and speculative decoding --------------------------------

def _proc_args(cls, args):
    """(temperature, top_k, top_p) of a reference processor constructor call."""
    if cls in ("GreedyProcessor", "MultinomialProcessor"):
        return float(args[0]), 0, 0.0
    if cls == "TopKProcessor":
        return float(args[0]), int(args[1]), 0.0
    if cls == "NucleusProcessor":
        return float(args[0]), 0, float(args[1])
    return float(args[0]), int(args[1]), float(args[2])


@pytest.mark.parametrize("name", list(cases.PROCESSORS))
def test_sampling_processors(golden, name):
    g = golden("sampling")
    logits = T(cases.sampling_logits())
    t, k, p = _proc_args(*cases.PROCESSORS[name])
    assert np.array_equal(O.processor_masked_logits(logits, k, p).numpy(), g[f"proc.{name}.masked"])
    probs = O.processor_probs(logits, t, k, p)
    close(probs, g[f"proc.{name}.probs"], 1e-7, name)
    assert np.array_equal(torch.argmax(probs, -1).unsqueeze(-1).numpy(), g[f"proc.{name}.argmax"])


@pytest.mark.parametrize("name", list(cases.SPECULATIVE))
def test_speculative_decoding(golden, name):
    g = golden("sampling")
    c = cases.SPECULATIVE[name]
    tcfg, dcfg = cases.with_kv(cases.test_cfg(), None), cases.with_kv(cases.test_cfg(), None)
    tcfg.num_hidden_layers, dcfg.num_hidden_layers = c["target_layers"], c["drafter_layers"]
    tsd = sd_from(cases.text_model_shapes(tcfg, "rope", None, head=True), "spec.target.")
    dsd = sd_from(cases.text_model_shapes(dcfg, "rope", None, head=True), c["drafter_prefix"])
    tl = lambda ids: O.decoder_forward(tsd, O.Cfg.of(tcfg), ids, torch.ones_like(ids), "rope").logits
    dl = lambda ids: O.decoder_forward(dsd, O.Cfg.of(dcfg), ids, torch.ones_like(ids), "rope").logits
    draws, used = T(cases.speculative_draws()), [0]

    def rand_fn(n):
        used[0] += n
        return draws[used[0] - n:used[0]]

    prompt = T(recipe.token_ids("spec.prompt", (1, c["prompt_len"]), 3, tcfg.vocab_size))
    t, k, p = _proc_args(*c["processor"])
    ids, rate = O.speculative_generate(prompt, dl, tl, tcfg.vocab_size, tcfg.max_position_embeddings, rand_fn,
                                       gamma=c["gamma"], temperature=t, top_k=k, top_p=p, max_gen_len=c["max_gen_len"],
                                       eos_tokens_id=c["eos"], pad_token_id=2, skip_sample_adjustment=c["skip"],
                                       first_target=c["first_target"])
    assert ids == g[f"spec.{name}.ids"].tolist()
    assert abs(rate - float(g[f"spec.{name}.rate"][0])) < 1e-12
    assert used[0] == int(g[f"spec.{name}.draws_used"][0])
