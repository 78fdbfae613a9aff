"""Encoder LoRA fine-tuning without a GPU: add_lora / lora_state_dict / merge_lora / disable_lora on an EncoderModel and
its holders against the reference's own keys and merged weights (tests/golden/encoder_lora.npz), the refusal messages,
the new entry points in the header and the binding, and tests/lora_epi_rule.py itself: an fp32 emulation of
vy_lora_expand_epi passes it, a delta added behind the epilogue fails it, and its restatement is the reference's
LoraLinear in front of the activation on the fixture's adapter."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vyomai_amd as V
from tests import lora_epi_rule as R
from tests.golden import cases_encoder_lora as E
from vyomai_amd import adapters, encoder_lora_train
from vyomai_amd._lib import VyomHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def classifier(model="abs"):
    pos, attn = E.MODELS[model]
    m = V.EncoderForSequenceClassification.from_config(E.cfg(model), E.NUM_LABELS, pos_embedding_type=pos,
                                                       attention_type=attn)
    E.load_weights_(m)
    return m


def reference_keys(base_keys, lora_keys):
    """The reference's state_dict keys after wrapping: <path>.linear.weight / .bias beside <path>.lora_a / .lora_b."""
    out = set(lora_keys)
    for k in base_keys:
        path, leaf = k.rsplit(".", 1)
        out.add(f"{path}.linear.{leaf}" if path + ".lora_a" in lora_keys else k)
    return out


@pytest.mark.parametrize("model", list(E.MODELS))
def test_add_lora_on_the_three_holders(golden, model):
    g = golden("encoder_lora")
    pos, attn = E.MODELS[model]
    for who, spec in E.ADAPTERS.items():
        fixture = [k for k in g[f"{model}.{who}.keys"].tolist() if not k.startswith("output.")]
        holders = {
            "": V.EncoderModel(E.cfg(model), pos, attn),
            "model.": classifier(model),
            "encoder.": V.EncoderForMaskedLM(E.cfg(model), pos, attn),
        }
        for prefix, m in holders.items():
            base_keys = set(m.state_dict())
            assert V.add_lora(m, rank=spec["rank"], alpha=spec["alpha"], targets=spec["on"]) is m
            lora_keys = {prefix + k[len("model."):] for k in fixture}
            assert set(V.lora_state_dict(m)) == lora_keys
            assert set(m.state_dict()) == reference_keys(base_keys, lora_keys)
            # everything that existed at wrapping time is frozen, the head of a holder included
            assert {n for n, p in m.named_parameters() if p.requires_grad} == lora_keys
            enc = m if prefix == "" else getattr(m, prefix[:-1])
            for layer in enc.all_layer:
                for path in adapters.ENCODER_TARGETS:
                    mod = layer
                    for part in path.split("."):
                        mod = getattr(mod, part)
                    assert isinstance(mod, V.LoraLinear) == (path in spec["on"]), path
                assert encoder_lora_train.layer_has_lora(layer)
            # the packed-QKV machinery still finds the base weights through the wrappers
            a = enc.all_layer[0].attention
            sh = E.shapes(model)
            assert [tuple(p.shape) for p in a._params()[:3]] == [sh[p] for p in E.QKV]
            assert tuple(a._packed()[0].shape) == (sum(sh[p][0] for p in E.QKV), 64)
    # the default is the notebook's five targets: key stays a plain nn.Linear
    m = V.add_lora(classifier(model).model, rank=8)
    assert type(m.all_layer[0].attention.key) is torch.nn.Linear
    assert all(isinstance(x, V.LoraLinear) for x in (m.all_layer[1].attention.query, m.all_layer[1].attention.value,
                                                    m.all_layer[1].attention.out.dense,
                                                    m.all_layer[1].feed_forward.intermediate,
                                                    m.all_layer[1].feed_forward.out))


def test_the_notebooks_order_keeps_the_head_trainable_and_loads_strictly(golden):
    g = golden("encoder_lora")
    for model in E.MODELS:
        for who, spec in E.ADAPTERS.items():
            m = classifier(model)
            base_keys = set(m.state_dict())
            V.add_lora(m.model, rank=spec["rank"], alpha=spec["alpha"], targets=spec["on"])
            keys = g[f"{model}.{who}.keys"].tolist()
            assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == keys == E.trained_keys(model, who)
            # a ClinicModel state dict under the reference's keys loads strictly
            lora_keys = {k for k in keys if not k.startswith("output.")}
            shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
            assert set(shapes) == reference_keys(base_keys, lora_keys)
            sd = {k: torch.full(s, 0.25) for k, s in shapes.items()}
            m.load_state_dict(sd, strict=True)
            assert float(m.model.all_layer[1].feed_forward.out.linear.bias[3]) == 0.25
            assert float(m.output.weight.detach()[4, 63]) == 0.25


def test_merge_lora_gives_the_fixtures_merged_weights(golden):
    g = golden("encoder_lora")
    for model in E.MODELS:
        for who, spec in E.ADAPTERS.items():
            tag = f"{model}.{who}"
            m = classifier(model)
            V.add_lora(m.model, rank=spec["rank"], alpha=spec["alpha"], targets=spec["on"])
            params = dict(m.named_parameters())
            with torch.no_grad():
                for k, v in E.adapter_state(model, who).items():
                    params[k].copy_(T(v))
            mods = [x for x in m.modules() if isinstance(x, V.LoraLinear)]
            with V.disable_lora(m):
                assert not any(x.enabled for x in mods) and not encoder_lora_train.layer_has_lora(m.model.all_layer[0])
            assert all(x.enabled for x in mods)
            biases = {n: p.detach().clone() for n, p in m.named_parameters() if n.endswith(".linear.bias")}
            assert V.merge_lora(m) is m
            assert not any(isinstance(x, V.LoraLinear) for x in m.modules())
            assert set(m.state_dict()) == set(classifier(model).state_dict())
            sd = m.state_dict()
            merged = [k for k in g if k.startswith(f"{tag}.merged.")]
            assert len(merged) == E.LAYERS * len(spec["on"])
            for k in merged:
                name = k[len(f"{tag}.merged."):]
                got = E.sub_g(sd[name].numpy())
                assert np.abs(got - g[k]).max() < 1e-6, k
            for n, b in biases.items():      # the bias-carrying linears come back whole
                assert torch.equal(sd[n.replace(".linear.bias", ".bias")], b)
            assert V.lora_state_dict(m) == {}


def test_refusals():
    cfg = E.cfg("abs")
    with pytest.raises(ValueError, match="lora_dropout 0.1.*use 0.0"):
        V.LoraLinear(torch.nn.Linear(64, 64), lora_dropout=0.1)
    for other in (V.DecoderModel(cfg, "rope", None), torch.nn.Linear(64, 64)):
        with pytest.raises(ValueError, match="prepares a ModelForCausalLM, not a .*EncoderModel.*fold a trained update"):
            V.add_lora(other)
    m = classifier()
    with pytest.raises(ValueError, match="targets .* must be a non-empty subset"):
        V.add_lora(m, targets=("attention.query", "self_attn.q_proj"))
    with pytest.raises(ValueError, match="targets .* must be a non-empty subset"):
        V.add_lora(m, targets=())
    with pytest.raises(ValueError, match="rank 65 must be"):
        V.add_lora(m, rank=65)
    assert all(p.requires_grad for p in m.parameters()), "a refused call changes nothing"
    V.add_lora(m.model, rank=8, targets=("feed_forward.out",))
    with pytest.raises(ValueError, match="already carries LoRA adapters"):
        V.add_lora(m, rank=8)
    # mixing LoRA and DoRA
    d = classifier()
    d.model.all_layer[0].attention.key = V.DoraLinear(d.model.all_layer[0].attention.key, rank=8)
    with pytest.raises(ValueError, match="carries DoRA adapters, and a layer runs one kind"):
        V.add_lora(d)
    with pytest.raises(ValueError, match="add_dora prepares a ModelForCausalLM, not a EncoderForSequenceClassification"):
        V.add_dora(classifier())
    # a wrapped sub-module called on its own, and a KV cache on a wrapped module
    layer = m.model.all_layer[0]
    x = torch.zeros(1, 4, 64)
    with pytest.raises(VyomHipError, match="applied by the EncoderLayer.*merge_lora"):
        layer.feed_forward(x, x)
    q = classifier()
    V.add_lora(q.model, rank=8, targets=("attention.query",))
    att = q.model.all_layer[0].attention
    with pytest.raises(VyomHipError, match="applied by the EncoderLayer"):
        att(x, None)
    with pytest.raises(VyomHipError, match="with a KV cache.*merge_lora"):
        att._attend(x, None, None, cache=object())
    with V.disable_lora(q):          # the base model: the guards let it through to the device check
        with pytest.raises(VyomHipError, match="CPU tensor"):
            att(x, None)
    with pytest.raises(VyomHipError, match="encoder layer got a CPU tensor"):
        q.model.all_layer[0](x, None)
    # cross-attention
    from vyomai_amd.layers.attention import EncoderDecoderAttention
    cross = EncoderDecoderAttention(cfg, 0)
    cross.value = V.LoraLinear(cross.value, rank=8)
    with pytest.raises(VyomHipError, match="no path through the encoder-decoder attention"):
        cross(x, x, None)
    with pytest.raises(ValueError, match="num_labels 0 must be"):
        V.EncoderForSequenceClassification(cfg, 0)


def test_new_entry_points_are_declared_and_exported():
    from vyomai_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vyom_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("vy_lora_expand_epi", 27), ("vy_cls_head_fwd", 14), ("vy_cls_head_bwd", 15)):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert proto is not None, name
        assert name in _lib.PROTOTYPES and name in _lib.ALL_SYMBOLS and hasattr(lib, name), name
        assert len(_lib.PROTOTYPES[name]) == proto.group(1).count(",") + 1 == n_args, name
    assert lib.vy_abi_version() == 5, "additive symbols: the ABI version stays"
    for mode, value in (("ACT", 0), ("DROP_RES", 1), ("MUL", 2)):
        assert re.search(r"VY_LORA_EPI_%s = %d\b" % (mode, value), hdr) and getattr(_lib, "LORA_EPI_" + mode) == value
    assert V.EncoderForSequenceClassification is V.models.encoder.EncoderForSequenceClassification


# ---- tests/lora_epi_rule.py itself ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_rule_accepts_the_kernels_arithmetic_and_rejects_a_delta_behind_the_epilogue(dtype):
    T_, N, bounds, r_pad, alpha = 51, 192, (64, 128), 32, 1.5
    z, u, B, other = R.make_inputs(T_, N, bounds, r_pad, dtype)
    print(R.derivation(r_pad, dtype))
    for code in R.ACT_NAMES:
        h, pre = R.emulate("act", z, u, B, alpha, bounds, r_pad, dtype, code=code)
        R.check_act(code, h, pre, z, u, B, alpha, bounds, r_pad, dtype)
        if code != 7:       # (leaky_relu is linear on each side: behind or in front only differs across the kink)
            with pytest.raises(AssertionError, match="outside the rule"):
                R.check_act(code, *R.emulate("act", z, u, B, alpha, bounds, r_pad, dtype, code=code, mutate=True), z, u, B,
                            alpha, bounds, r_pad, dtype)
    g = torch.Generator().manual_seed(5)
    for p in (0.0, 0.1, 0.5):
        keep = torch.rand(T_, N, generator=g) >= p
        s = R.emulate("drop_res", z, u, B, alpha, bounds, r_pad, dtype, res=other, keep=keep, p=p)
        R.check_drop_res(s, keep, p, z, u, B, alpha, bounds, r_pad, other, dtype)
        if p > 0:
            bad = R.emulate("drop_res", z, u, B, alpha, bounds, r_pad, dtype, res=other, keep=keep, p=p, mutate=True)
            with pytest.raises(AssertionError):
                R.check_drop_res(bad, keep, p, z, u, B, alpha, bounds, r_pad, other, dtype)
            flipped = keep.clone()
            flipped[7, 33] = ~flipped[7, 33]          # one element of the mask: the rule sees it
            with pytest.raises(AssertionError):
                R.check_drop_res(s, flipped, p, z, u, B, alpha, bounds, r_pad, other, dtype)
    out = R.emulate("mul", z, u, B, alpha, bounds, r_pad, dtype, mul=other)
    R.check_mul(out, z, u, B, alpha, bounds, r_pad, other, dtype)
    with pytest.raises(AssertionError, match="outside the rule"):
        R.check_mul((out.float() * 1.02).to(dtype), z, u, B, alpha, bounds, r_pad, other, dtype)


def test_rule_restates_the_references_lora_linear_on_the_fixtures_adapter():
    """act(linear(x) + alpha * F.linear(F.linear(x, lora_a), lora_b)) -- LoraLinear.forward, then FeedForward's act --
    and dropout-free LN input linear(x) + delta + residual, on layer 0 of the fixture's n5 / n6 adapters in fp64."""
    from vyomai_amd import recipe
    g = torch.Generator().manual_seed(3)
    for who, spec in E.ADAPTERS.items():
        state = E.adapter_state("abs", who)
        for path, code in (("feed_forward.intermediate", 1), ("attention.out.dense", None)):
            key = f"model.all_layer.0.{path}"
            A, Bm = T(state[key + ".lora_a"]).double(), T(state[key + ".lora_b"]).double()
            out_f, in_f = E.shapes("abs")[path]
            W = T(recipe.param_value(key + ".weight", (out_f, in_f))).double()
            b = T(recipe.param_value(key + ".bias", (out_f,))).double()
            x = torch.randn(51, in_f, generator=g, dtype=torch.float64)
            res = torch.randn(51, out_f, generator=g, dtype=torch.float64)
            r_pad = 32
            u = torch.zeros(51, r_pad, dtype=torch.float64)
            u[:, :spec["rank"]] = x @ A.t()
            Bp = torch.zeros(out_f, r_pad, dtype=torch.float64)
            Bp[:, :spec["rank"]] = Bm
            z = F.linear(x, W, b)
            lora = F.linear(x, W, b) + spec["alpha"] * F.linear(F.linear(x, A), Bm)      # LoraLinear.forward
            v, _ = R.pre_sum(z, u, Bp, spec["alpha"], (), r_pad)
            assert torch.allclose(v, lora, rtol=1e-12, atol=1e-12)
            if code is not None:
                assert torch.allclose(R.act64(code, v), F.gelu(lora), rtol=1e-12, atol=1e-12)
                vv = lora.clone().requires_grad_(True)
                F.gelu(vv).sum().backward()
                assert torch.allclose(R.act_grad64(code, v), vv.grad, rtol=1e-10, atol=1e-12)
            else:
                keep = torch.ones(51, out_f, dtype=torch.bool)
                R.check_drop_res(lora + res, keep, 0.0, z, u, Bp, spec["alpha"], (), r_pad, res, torch.float32)


def test_activation_restatements_match_torch_autograd():
    x = torch.linspace(-7, 7, 1401, dtype=torch.float64)
    fns = {1: F.gelu, 2: lambda t: F.gelu(t, approximate="tanh"), 3: F.silu, 4: torch.tanh, 5: torch.sigmoid,
           6: F.relu6, 7: F.leaky_relu}
    for code, fn in fns.items():
        xx = x.clone().requires_grad_(True)
        y = fn(xx)
        y.sum().backward()
        assert torch.allclose(R.act64(code, x), y.detach(), rtol=1e-12, atol=1e-13), code
        inner = (x != 0) & (x != 6)      # (torch's subgradient at a kink is its own choice)
        assert torch.allclose(R.act_grad64(code, x)[inner], xx.grad[inner], rtol=1e-9, atol=1e-12), code
        lip, lip2 = R.LIP[code]
        assert float(xx.grad.abs().max()) <= lip, (code, float(xx.grad.abs().max()))
        if lip2 is not None:             # sup |act''| by finite differences of the exact derivative
            d2 = (R.act_grad64(code, x[1:]) - R.act_grad64(code, x[:-1])) / (x[1] - x[0])
            assert float(d2.abs().max()) <= lip2, (code, float(d2.abs().max()))
