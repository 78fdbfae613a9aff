"""Generate tests/golden/activations.npz by running the REAL reference (Ajax0564/VyomAI) on the CPU with every
``hidden_act`` of its table other than "gelu" (VyomAI/layers/ffn.py:7-15).  Same pattern as make_golden.py: the
reference is imported at run time, filled with the deterministic recipe, and only OUTPUTS are stored (fp32 arrays,
sub-sampled where large; case constants and sub-sampling rules in cases_acts.py).

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python tests/golden/make_golden_acts.py

Contents (key layout `<level>.<case>.<name>.<what>`):
  ffn.{micro,wide}.<name>.y            FeedForward on the plain inputs ({tag}.x, {tag}.res), all six names
  ffn.micro.<name>.{dx,dres,d.*}       ... gradients of (y * gout).sum(), smooth names (plain inputs are safe for them)
  kink.{micro,wide}.<name>.{y,dx,dres,d.*}   FeedForward on the scaled hidden state (cases_acts.KINK_TAGS); wide
                                       gradients for silu and relu6 only; `gap.*` = the reference's own fp32-vs-fp64 gap
  kink.{micro,wide}.{margin,pre_err,pre...}  distance of the nearest pre-activation to a kink, the reference's
                                       fp32-vs-fp64 pre-activation error, and the fp32 pre-activation itself
  layer.wide.<name>.y                  one DecoderLayer (setup of test_layer_gradients_fp32_vs_reference), forward
  layer.wide.silu.{dx,d.*}             ... and gradients
  layer.micro.<name>.{y,dx,d.*}        micro layer gradients: plain inputs for sigmoid / tanh; for relu6 / leaky_relu the
                                       first of cases_acts.LAYER_KINK_TAGS whose pre-activations keep the margin
  model.{rope,absolute}.<name>.*       2-layer DecoderModel: hidden, strided logits, generate ids in three cache modes
  vit.silu.*                           Vit (the wiring through FeedForward outside the decoder)
"""
from __future__ import annotations

import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"      # as make_golden.py / tests/conftest.py: MKL's vendor-neutral fp32 branch

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from VyomAI.layers import ffn as ref_ffn  # noqa: E402  (the reference)
from VyomAI.layers import positional_embeddings as ref_pos  # noqa: E402
from VyomAI.models import decoder as ref_dec  # noqa: E402
from VyomAI.models.vision_encoder import Vit  # noqa: E402

from vyomai_amd import recipe  # noqa: E402
from tests.golden import cases, cases_acts as CA  # noqa: E402

torch.manual_seed(0)


def T(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a))


def filled(module, prefix=""):
    with torch.no_grad():
        if not prefix:
            recipe.load_recipe_(module)
        else:
            for n, t in module.state_dict().items():
                if t.is_floating_point():
                    t.copy_(T(recipe.param_value(prefix + n, tuple(t.shape))))
    return module.eval()


def np32(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().numpy()


def gap(a32: torch.Tensor, a64: torch.Tensor) -> np.ndarray:
    """max |fp32 run - fp64 run| of one tensor, as a 1-element array."""
    return np.array([float((a32.detach().double() - a64.detach()).abs().max())], dtype=np.float64)


def run_ffn(cfg, prefix, x, res, gout, dtype):
    """Reference FeedForward forward + backward in `dtype`: (pre-activation, y, dx, dres, {name: grad})."""
    m = filled(ref_ffn.FeedForward(cfg), prefix).to(dtype)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    res = res.detach().clone().to(dtype).requires_grad_(True)
    pre = m.intermediate(x).detach()
    y = m(x, res)
    (y * gout.to(dtype)).sum().backward()
    return pre, y.detach(), x.grad, res.grad, {n: p.grad for n, p in m.named_parameters()}


def ffn_level(out):
    for tag in ("micro", "wide"):
        B, L = cases.MODULE_BL[tag]
        # ---- plain inputs ----
        for name in CA.NAMES:
            cfg = CA.cfg_for(tag, name)
            d = cfg.hidden_size
            x, res = T(recipe.uniform(f"{tag}.x", (B, L, d))), T(recipe.uniform(f"{tag}.res", (B, L, d)))
            gout = T(recipe.uniform(f"{tag}.gout", (B, L, d)))
            _, y, dx, dres, grads = run_ffn(cfg, f"{tag}.ffn.", x, res, gout, torch.float32)
            out[f"ffn.{tag}.{name}.y"] = CA.sub_act(np32(y))
            if tag == "micro" and name in CA.SMOOTH:
                out[f"ffn.{tag}.{name}.dx"], out[f"ffn.{tag}.{name}.dres"] = CA.sub_act(np32(dx)), CA.sub_act(np32(dres))
                for n, g in grads.items():
                    out[f"ffn.{tag}.{name}.d.{n}"] = CA.sub_grad(np32(g))
        # ---- kink inputs: the hidden state scaled so that both kinks of relu6 are crossed, margin asserted ----
        kt = CA.KINK_TAGS[tag]
        for name in CA.GRAD_NAMES:
            cfg = CA.cfg_for(tag, name)
            d = cfg.hidden_size
            x = T(recipe.uniform(f"{kt}.x", (B, L, d), scale=CA.KINK_SCALE))
            res, gout = T(recipe.uniform(f"{kt}.res", (B, L, d))), T(recipe.uniform(f"{kt}.gout", (B, L, d)))
            pre, y, dx, dres, grads = run_ffn(cfg, f"{kt}.ffn.", x, res, gout, torch.float32)
            pre64, y64, dx64, dres64, grads64 = run_ffn(cfg, f"{kt}.ffn.", x, res, gout, torch.float64)
            if f"kink.{tag}.margin" not in out:      # the pre-activation does not depend on the activation
                store_margin(out, f"kink.{tag}", pre, pre64, whole=(tag == "micro"))
            k = f"kink.{tag}.{name}"
            out[f"{k}.y"], out[f"{k}.gap.y"] = CA.sub_act(np32(y)), gap(y, y64)
            if tag == "micro" or name in CA.WIDE_GRAD_NAMES:
                out[f"{k}.dx"], out[f"{k}.gap.dx"] = CA.sub_act(np32(dx)), gap(dx, dx64)
                out[f"{k}.dres"], out[f"{k}.gap.dres"] = CA.sub_act(np32(dres)), gap(dres, dres64)
                for n, g in grads.items():
                    out[f"{k}.d.{n}"], out[f"{k}.gap.d.{n}"] = CA.sub_grad(np32(g)), gap(g, grads64[n])


def store_margin(out, key, pre, pre64, whole, searched=False):
    """Assert and store the kink margin of a set of reference pre-activations (see cases_acts.py): the two fixed
    FeedForward cases keep KINK_MIN_MARGIN, an input found by search keeps MARGIN_FACTOR x the reference's own error."""
    margin = float(CA.kink_distance(pre64.numpy()).min())
    err = float((pre.double() - pre64).abs().max())
    above, below = float((pre64 > 6).double().mean()), float((pre64 < 0).double().mean())
    print(f"{key}: margin {margin:.3e}  fp32-vs-fp64 pre-activation error {err:.3e}  >6: {above:.3%}  <0: {below:.3%}")
    assert margin >= (CA.MARGIN_FACTOR * err if searched else CA.KINK_MIN_MARGIN), (key, margin, err)
    assert margin >= 8 * err      # margin / 8, the bar of the GPU test's pre-activation check, is above the reference's own error
    # the fp32 pre-activations are on the same side of every kink as the fp64 ones
    assert float(CA.kink_distance(pre.numpy()).min()) >= margin - err
    out[f"{key}.margin"] = np.array([margin], dtype=np.float64)
    out[f"{key}.pre_err"] = np.array([err], dtype=np.float64)
    p = np32(pre).reshape(-1, pre.shape[-1])
    if whole:
        out[f"{key}.pre"] = p
    else:
        idx = CA.near_kinks(p)
        out[f"{key}.pre.near_idx"], out[f"{key}.pre.near_val"] = idx, p.reshape(-1)[idx]
        out[f"{key}.pre.sub"] = CA.sub_grad(p)


def run_layer(cfg, prefix, x, gout, dtype):
    """Reference DecoderLayer (vanilla attention, rotary, causal + key padding): setup of the layer-gradient tests."""
    B, L, d = x.shape
    layer = filled(ref_dec.DecoderLayer(cfg, 0, None), prefix).to(dtype)
    pres = []
    h = layer.feed_forward.intermediate.register_forward_hook(lambda m, i, o: pres.append(o.detach()))
    x = x.detach().clone().to(dtype).requires_grad_(True)
    freqs = ref_pos.RotaryEmbedding(cfg)(cfg.max_position_embeddings)[:, :L].to(dtype)
    mask = T(cases.causal_additive(B, L, 0, cases.keypad(B, L))).to(dtype)
    y, _ = layer(x, mask, freqs)
    (y * gout.to(dtype)).sum().backward()
    h.remove()
    return pres[0], y.detach(), x.grad, {n: p.grad for n, p in layer.named_parameters()}


def layer_level(out):
    # wide: forward for every name, gradients for silu
    tag = "wide"
    B, L = cases.MODULE_BL[tag]
    for name in CA.GRAD_NAMES:
        cfg = CA.cfg_for(tag, name)
        d = cfg.hidden_size
        x, gout = T(recipe.uniform(f"{tag}.x", (B, L, d))), T(recipe.uniform(f"{tag}.gout", (B, L, d)))
        _, y, dx, grads = run_layer(cfg, f"{tag}.layer.None.", x, gout, torch.float32)
        out[f"layer.{tag}.{name}.y"] = CA.sub_act(np32(y))
        if name == "silu":
            out[f"layer.{tag}.{name}.dx"] = CA.sub_act(np32(dx))
            for n, g in grads.items():
                out[f"layer.{tag}.{name}.d.{n}"] = CA.sub_grad(np32(g))
    # micro: gradients for the other names; the kinked ones on the first input tag whose pre-activations keep the margin
    tag = "micro"
    B, L = cases.MODULE_BL[tag]
    chosen = None
    for name in ("sigmoid", "tanh", "relu6", "leaky_relu"):
        cfg = CA.cfg_for(tag, name)
        d = cfg.hidden_size
        gout = T(recipe.uniform(f"{tag}.gout", (B, L, d)))
        if name in CA.SMOOTH:
            x = T(recipe.uniform(f"{tag}.x", (B, L, d)))
        else:
            if chosen is None:
                for kt in CA.LAYER_KINK_TAGS:
                    x = T(recipe.uniform(f"{kt}.x", (B, L, d)))
                    pre, *_ = run_layer(cfg, f"{tag}.layer.None.", x, gout, torch.float32)
                    pre64, *_ = run_layer(cfg, f"{tag}.layer.None.", x, gout, torch.float64)
                    margin = float(CA.kink_distance(pre64.numpy()).min())
                    err = float((pre.double() - pre64).abs().max())
                    print(f"layer {kt}: margin {margin:.3e} error {err:.3e}")
                    if margin >= CA.MARGIN_FACTOR * err:
                        chosen = kt
                        break
                assert chosen is not None, "no layer input tag keeps the kink margin"
                out["layer.kink.tag"] = np.array([CA.LAYER_KINK_TAGS.index(chosen)], dtype=np.int64)
            x = T(recipe.uniform(f"{chosen}.x", (B, L, d)))
        pre, y, dx, grads = run_layer(cfg, f"{tag}.layer.None.", x, gout, torch.float32)
        k = f"layer.{tag}.{name}"
        if name in CA.KINKED:
            pre64, y64, dx64, grads64 = run_layer(cfg, f"{tag}.layer.None.", x, gout, torch.float64)
            if "layer.kink.margin" not in out:
                store_margin(out, "layer.kink", pre, pre64, whole=True, searched=True)
            out[f"{k}.gap.y"], out[f"{k}.gap.dx"] = gap(y, y64), gap(dx, dx64)
            for n, g in grads.items():
                out[f"{k}.gap.d.{n}"] = gap(g, grads64[n])
        out[f"{k}.y"], out[f"{k}.dx"] = CA.sub_act(np32(y)), CA.sub_act(np32(dx))
        for n, g in grads.items():
            out[f"{k}.d.{n}"] = CA.sub_grad(np32(g))


@torch.no_grad()
def model_level(out):
    ids3, am3 = cases.reference_test_inputs()
    ids3, am3 = T(ids3), T(am3)
    for name in CA.GRAD_NAMES:
        for pos in ("rope", "absolute"):
            c = CA.model_cfg(name)
            m = filled(ref_dec.DecoderModel(c, pos, None))
            o = m(ids3, am3)
            k = f"model.{pos}.{name}"
            out[f"{k}.hidden"] = CA.sub_act(np32(o.hidden_state))
            out[f"{k}.logits"] = np32(CA.sub_logits(o.logits))
            p = torch.tensor([[9226, 16, 5, 1296]], dtype=torch.long)
            a = torch.ones(1, 4, dtype=torch.long)
            out[f"{k}.gen.nocache"] = m.generate(p, a, use_cache=False).numpy()
            out[f"{k}.gen.dynamic"] = m.generate(p, a, use_cache=True).numpy()
            out[f"{k}.gen.static"] = m.generate(p, a, use_cache=True, use_static_cache=True).numpy()
    vcfg = cases.vit_cfg()
    vcfg.hidden_act = "silu"
    img = T(recipe.uniform("vit.img", (2, 3, 224, 224), 0.5, 0.5))
    y = filled(Vit(vcfg))(img.clone()).logits
    out["vit.silu.out"], out["vit.silu.cls"] = np32(CA.sub_vit(y)), np32(y[:, 0, :])


if __name__ == "__main__":
    out = {}
    ffn_level(out)
    layer_level(out)
    model_level(out)
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    assert all(isinstance(v, np.ndarray) and v.dtype != object for v in out.values())
    path = os.path.join(HERE, "activations.npz")
    np.savez_compressed(path, **out)
    print(f"wrote activations.npz  {os.path.getsize(path) / 1024:.1f} KiB  keys={len(out)}")
