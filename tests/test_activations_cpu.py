"""hidden_act on the host side (no GPU): FeedForward accepts every name of the reference's table
(VyomAI/layers/ffn.py:7-15), the activation codes of include/vyom_hip.h and vyomai_amd/_lib.py agree, and the CPU
oracle reproduces what the REAL reference computed for every name (tests/golden/activations.npz) at the bars of
tests/test_oracle_golden.py: 2e-6 abs on outputs, 2e-5 x the tensor's scale on gradients."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import vyom_oracle as O
from tests.golden import cases, cases_acts as CA
from tests.test_oracle_golden import ATOL, T, close, sd_from
from vyomai_amd import _lib, recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_NAMES = ("gelu", "leaky_relu", "relu6", "sigmoid", "silu", "swish", "tanh")
EXPECTED = {"gelu": _lib.ACT_GELU_ERF, "leaky_relu": _lib.ACT_LEAKY_RELU, "relu6": _lib.ACT_RELU6,
            "sigmoid": _lib.ACT_SIGMOID, "silu": _lib.ACT_SILU, "swish": _lib.ACT_SILU, "tanh": _lib.ACT_TANH}


@pytest.mark.parametrize("name", REFERENCE_NAMES)
def test_feed_forward_constructs_with_every_reference_name(name):
    from vyomai_amd.layers.ffn import FeedForward
    cfg = cases.micro_cfg()
    cfg.hidden_act = name
    assert FeedForward(cfg).act == EXPECTED[name]


def test_swish_is_silu_and_unknown_names_fall_back_to_gelu():
    from vyomai_amd.layers.ffn import FeedForward
    cfg = cases.micro_cfg()
    acts = {}
    for name in ("swish", "silu", "no_such_activation", None):
        cfg.hidden_act = name
        acts[name] = FeedForward(cfg).act
    assert acts["swish"] == acts["silu"] == _lib.ACT_SILU
    assert acts["no_such_activation"] == acts[None] == _lib.ACT_GELU_ERF      # reference :26-29
    assert CA.CODES == {n: EXPECTED[n] for n in CA.NAMES}


def test_every_model_family_constructs_with_silu():
    """No GPU is touched by construction: the families of the package all build their FFN from FeedForward."""
    import vyomai_amd as V
    cfg = cases.micro_cfg()
    cfg.hidden_act = "silu"
    vcfg = cases.vit_cfg()
    vcfg.hidden_act, vcfg.num_hidden_layers = "silu", 1
    tcfg = cases.TextCfg(num_hidden_layers=1, vocab_size=97, hidden_act="silu")       # the Vit's width
    models = [V.EncoderModel(cfg, "rope", None), V.DecoderModel(cfg, "rope", "gqa"), V.Vit(vcfg),
              V.VisionLanguageModel(tcfg, V.Vit(vcfg), "absolute", None),
              V.EncoderDecoderModel(cfg, cfg, None, "rope", None, "rope", None)]
    from vyomai_amd.layers.ffn import FeedForward
    for m in models:
        ffns = [x for x in m.modules() if isinstance(x, FeedForward)]
        assert ffns and all(f.act == _lib.ACT_SILU for f in ffns), type(m).__name__


def test_header_enum_equals_the_python_constants():
    text = open(os.path.join(ROOT, "include", "vyom_hip.h")).read()
    enum = re.search(r"typedef enum \{([^}]*)\} vy_act;", text).group(1)
    header = {k: int(v) for k, v in re.findall(r"VY_ACT_(\w+) = (\d+)", enum)}
    assert header == {"NONE": _lib.ACT_NONE, "GELU_ERF": _lib.ACT_GELU_ERF, "GELU_TANH": _lib.ACT_GELU_TANH,
                      "SILU": _lib.ACT_SILU, "TANH": _lib.ACT_TANH, "SIGMOID": _lib.ACT_SIGMOID,
                      "RELU6": _lib.ACT_RELU6, "LEAKY_RELU": _lib.ACT_LEAKY_RELU}
    assert (header["NONE"], header["GELU_ERF"], header["GELU_TANH"]) == (0, 1, 2)      # the old codes keep their values
    assert int(re.search(r"#define VY_ACT_SAVE_DERIV (0x[0-9a-fA-F]+)", text).group(1), 16) == _lib.ACT_SAVE_DERIV == 0x100
    assert len(set(header.values())) == len(header) and max(header.values()) < _lib.ACT_SAVE_DERIV


def test_fixture_holds_arrays_only_and_keeps_the_kink_margins(golden):
    path = os.path.join(ROOT, "tests", "golden", "activations.npz")
    assert os.path.getsize(path) <= 1 << 20
    with np.load(path, allow_pickle=False) as z:     # a pickled object would raise here
        for k in z.files:
            assert z[k].dtype.kind in "fiu", (k, z[k].dtype)
    g = golden("activations")
    for key, factor in (("kink.micro", 8), ("kink.wide", 8), ("layer.kink", CA.MARGIN_FACTOR)):
        margin, err = float(g[f"{key}.margin"][0]), float(g[f"{key}.pre_err"][0])
        assert margin >= factor * err, (key, margin, err)
    assert float(g["kink.micro.margin"][0]) >= CA.KINK_MIN_MARGIN and float(g["kink.wide.margin"][0]) >= CA.KINK_MIN_MARGIN
    # the scaled hidden state does cross both kinks of relu6
    pre = g["kink.micro.pre"]
    assert (pre > 6).mean() > 0.01 and (pre < 0).mean() > 0.3
    assert abs(float(CA.kink_distance(pre).min()) - float(g["kink.micro.margin"][0])) <= float(g["kink.micro.pre_err"][0])


def _ffn_grads(c, sd, x, res, gout):
    for v in sd.values():
        v.requires_grad_(True)
    x, res = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    y = O.feed_forward(sd, "", c, x, res)
    (y * gout).sum().backward()
    return y, x.grad, res.grad


def _close_grad(got, want, what):
    close(got, want, 2e-5 * max(1.0, float(np.abs(want).max())), what)


@pytest.mark.parametrize("tag", ["micro", "wide"])
@pytest.mark.parametrize("name", CA.NAMES)
def test_oracle_feed_forward(golden, tag, name):
    g = golden("activations")
    cfg = CA.cfg_for(tag, name)
    c = O.Cfg.of(cfg)
    B, L = cases.MODULE_BL[tag]
    d = cfg.hidden_size
    x, res = T(recipe.uniform(f"{tag}.x", (B, L, d))), T(recipe.uniform(f"{tag}.res", (B, L, d)))
    gout = T(recipe.uniform(f"{tag}.gout", (B, L, d)))
    sd = sd_from(cases.ffn_shapes(cfg), f"{tag}.ffn.")
    y, dx, dres = _ffn_grads(c, sd, x, res, gout)
    close(CA.sub_act(y.detach().numpy()), g[f"ffn.{tag}.{name}.y"], what="ffn y")
    if tag == "micro" and name in CA.SMOOTH:
        _close_grad(CA.sub_act(dx.numpy()), g[f"ffn.{tag}.{name}.dx"], "dx")
        _close_grad(CA.sub_act(dres.numpy()), g[f"ffn.{tag}.{name}.dres"], "dres")
        for n, p in sd.items():
            _close_grad(CA.sub_grad(p.grad.numpy()), g[f"ffn.{tag}.{name}.d.{n}"], n)
    if name == "swish":
        return
    # the kink inputs (the output is LayerNorm'ed, so it is O(1) here too)
    kt = CA.KINK_TAGS[tag]
    x = T(recipe.uniform(f"{kt}.x", (B, L, d), scale=CA.KINK_SCALE))
    res, gout = T(recipe.uniform(f"{kt}.res", (B, L, d))), T(recipe.uniform(f"{kt}.gout", (B, L, d)))
    sd = sd_from(cases.ffn_shapes(cfg), f"{kt}.ffn.")
    y, dx, dres = _ffn_grads(c, sd, x, res, gout)
    k = f"kink.{tag}.{name}"
    close(CA.sub_act(y.detach().numpy()), g[f"{k}.y"], what="kink y")
    if tag == "micro" or name in CA.WIDE_GRAD_NAMES:
        _close_grad(CA.sub_act(dx.numpy()), g[f"{k}.dx"], "kink dx")
        _close_grad(CA.sub_act(dres.numpy()), g[f"{k}.dres"], "kink dres")
        for n, p in sd.items():
            _close_grad(CA.sub_grad(p.grad.numpy()), g[f"{k}.d.{n}"], "kink " + n)


def _oracle_layer(cfg, prefix, x, gout):
    c = O.Cfg.of(cfg)
    B, L, d = x.shape
    dh = d // cfg.num_attention_heads
    sd = sd_from(cases.layer_shapes(cfg, "vanilla"), prefix)
    for v in sd.values():
        v.requires_grad_(True)
    x = x.clone().requires_grad_(True)
    freqs = O.rotary_angles(dh, cfg.max_position_embeddings)[:, :L]
    mask = T(cases.causal_additive(B, L, 0, cases.keypad(B, L)))
    y = O.block(sd, "", c, x, mask, freqs, False)
    (y * gout).sum().backward()
    return sd, y, x.grad


@pytest.mark.parametrize("name", CA.GRAD_NAMES)
def test_oracle_block(golden, name):
    g = golden("activations")
    tag = "wide"
    cfg = CA.cfg_for(tag, name)
    B, L = cases.MODULE_BL[tag]
    d = cfg.hidden_size
    x, gout = T(recipe.uniform(f"{tag}.x", (B, L, d))), T(recipe.uniform(f"{tag}.gout", (B, L, d)))
    sd, y, dx = _oracle_layer(cfg, f"{tag}.layer.None.", x, gout)
    close(CA.sub_act(y.detach().numpy()), g[f"layer.{tag}.{name}.y"], what="layer y")
    if name == "silu":
        _close_grad(CA.sub_act(dx.numpy()), g[f"layer.{tag}.{name}.dx"], "dx")
        for n, p in sd.items():
            _close_grad(CA.sub_grad(p.grad.numpy()), g[f"layer.{tag}.{name}.d.{n}"], n)
        return
    tag = "micro"
    cfg = CA.cfg_for(tag, name)
    B, L = cases.MODULE_BL[tag]
    d = cfg.hidden_size
    xtag = CA.LAYER_KINK_TAGS[int(g["layer.kink.tag"][0])] if name in CA.KINKED else tag
    x, gout = T(recipe.uniform(f"{xtag}.x", (B, L, d))), T(recipe.uniform(f"{tag}.gout", (B, L, d)))
    sd, y, dx = _oracle_layer(cfg, f"{tag}.layer.None.", x, gout)
    k = f"layer.{tag}.{name}"
    close(CA.sub_act(y.detach().numpy()), g[f"{k}.y"], what="micro layer y")
    _close_grad(CA.sub_act(dx.numpy()), g[f"{k}.dx"], "micro dx")
    for n, p in sd.items():
        _close_grad(CA.sub_grad(p.grad.numpy()), g[f"{k}.d.{n}"], "micro " + n)


@pytest.mark.parametrize("pos", ["rope", "absolute"])
@pytest.mark.parametrize("name", CA.GRAD_NAMES)
def test_oracle_decoder_model(golden, name, pos):
    g = golden("activations")
    cfg = CA.model_cfg(name)
    sd = sd_from(cases.text_model_shapes(cfg, pos, None, head=True))
    c = O.Cfg.of(cfg)
    ids, am = cases.reference_test_inputs()
    with torch.no_grad():
        o = O.decoder_forward(sd, c, T(ids), T(am), pos, None)
        k = f"model.{pos}.{name}"
        close(CA.sub_act(o.hidden_state.numpy()), g[f"{k}.hidden"], what="hidden")
        close(CA.sub_logits(o.logits), g[f"{k}.logits"], 5e-6, what="logits")
        p, a = torch.tensor([[9226, 16, 5, 1296]], dtype=torch.long), torch.ones(1, 4)
        for mode, kw in (("nocache", dict(use_cache=False)), ("dynamic", dict(use_cache=True)),
                         ("static", dict(use_cache=True, use_static_cache=True))):
            t = O.decoder_generate(sd, c, p, a, 5, pos, None, **kw)
            assert np.array_equal(t.numpy(), g[f"{k}.gen.{mode}"]), mode


def test_oracle_vit_silu(golden):
    g = golden("activations")
    vcfg = cases.vit_cfg()
    vcfg.hidden_act = "silu"
    img = T(recipe.uniform("vit.img", (2, 3, 224, 224), 0.5, 0.5))
    with torch.no_grad():
        y = O.vit_forward(sd_from(cases.vit_shapes(vcfg)), vcfg, img)
    close(CA.sub_vit(y), g["vit.silu.out"], 5e-6, what="vit")
    close(y[:, 0, :], g["vit.silu.cls"], 5e-6, what="vit.cls")
    assert np.abs(g["vit.silu.out"] - golden("models_vision")["vit.out"][..., ::4]).max() > 1e-2     # not the GELU model again
