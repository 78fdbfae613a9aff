"""LoRA fine-tuning inside the fused post-LN block of the encoder (Examples/adapters.ipynb: a frozen BERT-style encoder
with LoraLinear around query / value / attention.output.dense / intermediate.dense / output.dense of every layer, and a
classification head on top): the forward of an EncoderLayer whose projections are wrapped in adapters.LoraLinear, and the
LoRA counterparts of autograd_train.SelfAttentionFn + LinearResidualLayerNormFn and FfnBlockFn.

The causal LM's recipe -- the plain fused GEMM, then the delta added behind it (lora_train.py) -- does not carry over:
three of this block's four GEMMs have a non-linear or stochastic epilogue, and the reference's wrapper sits in front of
it.  So an adapted group runs the plain GEMM with its bias and nothing else, vy_lora_shrink, and vy_lora_expand_epi,
the expand tile that carries the epilogue:

  qkv   plain GEMM + bias -> delta -> ops.rope_ (autograd_train._project_qkv(delta=)), then attention
  o     plain GEMM + bias -> shrink -> expand_epi(dropout + residual x)            -> LayerNorm
  ffn1  plain GEMM + bias -> shrink -> expand_epi(act; saves act')                 -> hmid, pre
  ffn2  plain GEMM + bias -> shrink -> expand_epi(dropout + residual layer input)  -> LayerNorm

A group without an adapter keeps the fused GEMM epilogue of the unwrapped layer.  The backward is the unwrapped
layer's LayerNorm, dropout, dgrad and attention launches and NO base weight gradient -- the base is frozen -- plus,
per adapted group, lora_train._adapter_backward (t = dY @ B, dX += alpha t A, both low-rank weight gradients).  Behind
an adapted ffn2 the adapter's dX term must be inside the product with act': the base dgrad runs without its act'
epilogue and vy_lora_expand_epi's multiply mode adds the term and multiplies in one pass."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional

import torch

from . import _lib, ops
from ._lib import VyomHipError
from .adapters import _ENCODER, ENCODER_GROUPS, LoraLinear
from .autograd import _drop_args
from .autograd_train import (WEIGHT_EPOCH, _attend, _attention_bwd, _attn_args, _defer_list, _ln_bwd, _project_qkv,
                             _require_bf16, _wt, _wt_packed)
from .layers.attention import _shadow
from .lora_train import (GroupOperands, _adapter_backward, _delta, _frozen_base, _param_grads, _rows, _save, _saved,
                         _tiles)

NO_CACHE = ("an encoder layer whose projections carry LoRA adapters (LoraLinear) cannot run {what}: that path would skip "
            "the adapter's term.  Fold the adapters into the weights with vyomai_amd.merge_lora(model) first")
CALL_THE_LAYER = ("{what} carries an enabled LoraLinear: its term is applied by the EncoderLayer that owns the module "
                  "(encoder_lora_train.py), inside the activation / dropout that follows the projection.  Call the layer "
                  "(or the model), or fold the adapters in with vyomai_amd.merge_lora(model)")


def _group_mods(layer, g: str):
    return [functools.reduce(getattr, path.split("."), layer) for path in _ENCODER[g]]


def _all_mods(layer):
    a, f = layer.attention, layer.feed_forward
    return (a.query, a.key, a.value, a.out.dense, f.intermediate, f.out)


def layer_has_lora(layer) -> bool:
    """Does any projection of this EncoderLayer carry an enabled LoraLinear?  (Every forward of every layer asks: six
    attribute reads.)"""
    for mod in _all_mods(layer):
        if type(mod) is LoraLinear and mod._off == 0:
            return True
    return False


def refuse_direct_call(what: str, *mods) -> None:
    """A sub-module of an EncoderLayer called on its own reads `weight` / `bias` through the wrapper and would compute
    the base alone: say so.  (A disabled wrapper -- disable_lora -- IS the base.)"""
    for m in mods:
        if type(m).__name__ in ("LoraLinear", "DoraLinear") and getattr(m, "enabled", True):
            raise VyomHipError(CALL_THE_LAYER.format(what=what))


def layer_operands(layer, dt, dev) -> Dict[str, Optional[GroupOperands]]:
    """group -> its packed operands (None: no enabled adapter on any of its parts), cached on the layer and rebuilt
    when a parameter version or autograd_train.WEIGHT_EPOCH changes."""
    cache = layer.__dict__.setdefault("_vy_lora_ops", {})
    out = {}
    for g in ENCODER_GROUPS:
        mods = _group_mods(layer, g)
        live = [m for m in mods if isinstance(m, LoraLinear) and m.enabled]
        if not live:
            out[g] = None
            continue
        key = (tuple((id(m), m.lora_a._version, m.lora_b._version, float(m.alpha), m.rank) for m in live),
               tuple(isinstance(m, LoraLinear) and m.enabled for m in mods), WEIGHT_EPOCH[0], dt, dev)
        hit = cache.get(g)
        if hit is None or hit[0] != key:
            hit = cache[g] = (key, GroupOperands(f"encoder layer {layer.layer_idx} {g}", mods, dt, dev))
        out[g] = hit[1]
    return out


def _at3(G: GroupOperands) -> torch.Tensor:
    """The transposed stacked A as vy_lora_expand_epi's B operand: (1, K, R)."""
    return G.At.unsqueeze(0)


def _expand_epi(G: GroupOperands, z, x, **epilogue):
    """z (.., N): the plain GEMM of x (.., K) with its bias -> (the epilogue's output in z's place, u)."""
    z2, x2 = _rows(z), _rows(x)
    tiles, n = _tiles(z2.shape[0], z2.device)
    u = ops.lora_shrink(x2, G.A, tiles, n, name=G.name)
    ops.lora_expand_epi_(z2, u, G.B, G.alpha, tiles, n, G.bounds, name=G.name, **epilogue)
    return z, u


def _out_projection(G: Optional[GroupOperands], x, w, b, residual, drop, us: dict, g: str):
    """dropout(x W^T + b [+ delta]) + residual -> s: `o` and `ffn2`."""
    dt = x.dtype
    if G is None:
        return ops.linear(x, _shadow(w, dt), _shadow(b, dt), residual=residual, dropout=drop)
    z = torch.empty((*x.shape[:-1], w.shape[0]), dtype=dt, device=x.device)
    ops.linear(x, _shadow(w, dt), _shadow(b, dt), out=z)
    s, us[g] = _expand_epi(G, z, x, residual=_rows(residual), dropout=drop)
    return s


def _attention_half(x, layer, am, G, drop, us: dict):
    """-> (y, (q, k, v, o, lse, s, mean, rstd)): LN(dropout(out(attn(x))) + x) with the adapters of qkv and o."""
    a = layer.attention
    aso = a.out
    dt = x.dtype
    delta = None
    if G["qkv"] is not None:
        def delta(g, y, n):
            us[g] = _delta(G[g], _rows(y), _rows(n))
    q, k, v, _ = _project_qkv(x, a, am, delta=delta)
    o, lse = _attend(q, k, v, am)
    s = _out_projection(G["o"], o, aso.dense.weight, aso.dense.bias, x, drop, us, "o")
    ln = aso.layernorm
    y, mean, rstd = ops.layernorm(s, _shadow(ln.weight, dt), _shadow(ln.bias, dt), ln.eps, save_stats=True)
    return y, (q, k, v, o, lse, s, mean, rstd)


def _ffn_half(x, residual, layer, G, drop, us: dict):
    """-> (y, (pre, hmid, s, mean, rstd)): LN(dropout(out(act(intermediate(x)))) + residual) with the adapters of ffn1
    and ffn2; pre holds act'."""
    ff = layer.feed_forward
    dt = x.dtype
    w1, b1 = ff.intermediate.weight, ff.intermediate.bias
    pre = torch.empty((*x.shape[:-1], w1.shape[0]), dtype=dt, device=x.device)
    hmid = torch.empty_like(pre)
    if G["ffn1"] is None:
        ops.linear(x, _shadow(w1, dt), _shadow(b1, dt), act=ff.act | _lib.ACT_SAVE_DERIV, pre_out=pre, out=hmid)
    else:
        ops.linear(x, _shadow(w1, dt), _shadow(b1, dt), out=hmid)
        _, us["ffn1"] = _expand_epi(G["ffn1"], hmid, x, act=ff.act, pre=_rows(pre))
    s = _out_projection(G["ffn2"], hmid, ff.out.weight, ff.out.bias, residual, drop, us, "ffn2")
    ln = ff.layernorm
    y, mean, rstd = ops.layernorm(s, _shadow(ln.weight, dt), _shadow(ln.bias, dt), ln.eps, save_stats=True)
    return y, (pre, hmid, s, mean, rstd)


def _ln_backward(dy, s, ln_w, ln_b, mean, rstd):
    """autograd_train._ln_bwd, except under a frozen LayerNorm (add_lora freezes what it finds): a trainer's arena gives
    frozen parameters gradient views too, and _ln_bwd would accumulate into them and report them ready -- the bucket
    reducer counts only trainable parameters and would step the bucket before its last gradients are written."""
    if ln_w.requires_grad != ln_b.requires_grad:
        raise VyomHipError("a LayerNorm inside a layer with LoRA adapters trains its weight and bias together or neither")
    if ln_w.requires_grad:
        return _ln_bwd(dy, s, ln_w, ln_b, mean, rstd)
    dg = torch.empty(ln_w.shape, dtype=torch.float32, device=s.device)
    db = torch.empty(ln_b.shape, dtype=torch.float32, device=s.device)
    return ops.layernorm_bwd(dy, s, _shadow(ln_w, s.dtype), mean, rstd, dg, db, accumulate=False), None, None


def _residual_grad(ctx, ds):
    """The residual path's gradient: deferred to the QKV dgrad epilogue of the layer when the layer opted in."""
    if ctx.defer is not None:
        ctx.defer.append(ds)
        return None
    return ds


class EncoderLoraAttentionFn(torch.autograd.Function):
    """SelfAttentionFn + LinearResidualLayerNormFn in one, with adapters on any of query / key / value / out.dense and
    a frozen base.  Inputs after `ln_b`: the lora_a / lora_b parameters of the qkv and o groups (autograd tracks them;
    the values are read from G)."""

    @staticmethod
    def forward(ctx, x, layer, mask, freqs, G, drop, ln_w, ln_b, *lora_params):
        _require_bf16(x)
        us = {}
        am = _attn_args(mask, freqs, x.shape[1], x.device)
        y, (q, k, v, o, lse, s, mean, rstd) = _attention_half(x, layer, am, G, drop, us)
        _save(ctx, (x, q, k, v, o, lse, s, mean, rstd), us)
        ctx.meta = (layer, G, am, drop, ln_w, ln_b, lora_params)
        ctx.defer = _defer_list(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x, q, k, v, o, lse, s, mean, rstd), us = _saved(ctx, 9)
        layer, G, am, drop, ln_w, ln_b, lora_params = ctx.meta
        a, grads = layer.attention, {}
        dt = x.dtype
        ds, dg, dbt = _ln_backward(dy.contiguous(), s, ln_w, ln_b, mean, rstd)
        dz = ops.dropout(ds, *drop) if drop is not None else ds        # the forward's mask; the residual's is ds itself
        do = ops.linear_dgrad(dz, _wt(a.out.dense.weight, dt))
        _adapter_backward(G["o"], _rows(dz), _rows(o), us.get("o"), _rows(do), grads)
        packed = _attention_bwd(q, k, v, o, do, lse, am)
        dx = None
        if ctx.needs_input_grad[0]:
            # this layer's residual gradients -- ds, and what the feed-forward deferred -- ride in the dgrad's epilogue
            adds = [ds] + (ctx.defer if ctx.defer is not None else [])
            a2 = adds[1] if len(adds) > 1 else None
            for t in adds[2:]:
                a2 = a2 + t
            dx = ops.linear_dgrad(packed, _wt_packed(a, a._packed()[0], dt), add_to=adds[0], add_to2=a2)
        if ctx.defer is not None:
            ctx.defer.clear()
        # (layer 0 over a frozen embedding: nobody reads dx, and the packed dgrad is skipped)
        _adapter_backward(G["qkv"], _rows(packed), _rows(x), us.get("qkv"), None if dx is None else _rows(dx), grads)
        return (dx, None, None, None, None, None, dg, dbt, *_param_grads(lora_params, grads))


class EncoderLoraFfnFn(torch.autograd.Function):
    """FfnBlockFn with adapters on any of intermediate / out and a frozen base."""

    @staticmethod
    def forward(ctx, x, residual, layer, G, drop, ln_w, ln_b, *lora_params):
        _require_bf16(x)
        us = {}
        y, (pre, hmid, s, mean, rstd) = _ffn_half(x, residual, layer, G, drop, us)
        _save(ctx, (x, pre, hmid, s, mean, rstd), us)
        ctx.meta = (layer, G, drop, ln_w, ln_b, lora_params)
        ctx.defer = _defer_list(residual) if residual is not x else None
        return y

    @staticmethod
    def backward(ctx, dy):
        (x, pre, hmid, s, mean, rstd), us = _saved(ctx, 6)
        layer, G, drop, ln_w, ln_b, lora_params = ctx.meta
        ff, grads = layer.feed_forward, {}
        dt = x.dtype
        ds, dg, dbt = _ln_backward(dy.contiguous(), s, ln_w, ln_b, mean, rstd)
        dz = ops.dropout(ds, *drop) if drop is not None else ds
        wt2 = _wt(ff.out.weight, dt)
        if G["ffn2"] is None:
            dpre = ops.linear_dgrad(dz, wt2, pre=pre, act=ff.act | _lib.ACT_SAVE_DERIV)   # (dz W2) * act', act' saved
        else:
            # (dz W2 + alpha (dz B) A) * act': the plain dgrad, then the adapter's term and the product in one pass
            g2 = G["ffn2"]
            dpre = ops.linear_dgrad(dz, wt2)
            t = _adapter_backward(g2, _rows(dz), _rows(hmid), us["ffn2"], None, grads)
            tiles, n = _tiles(t.shape[0], t.device)
            ops.lora_expand_epi_(_rows(dpre), t, _at3(g2), g2.alpha, tiles, n, mul=_rows(pre), name=g2.name)
        dx = ops.linear_dgrad(dpre, _wt(ff.intermediate.weight, dt))
        _adapter_backward(G["ffn1"], _rows(dpre), _rows(x), us.get("ffn1"), _rows(dx), grads)
        return (dx, _residual_grad(ctx, ds), None, None, None, dg, dbt, *_param_grads(lora_params, grads))


def _group_params(G, groups) -> List[torch.Tensor]:
    return [p for g in groups if G[g] is not None for p in G[g].params()]


def layer_lora_params(layer) -> List[torch.Tensor]:
    return [p for m in _all_mods(layer) if isinstance(m, LoraLinear) and m.enabled for p in (m.lora_a, m.lora_b)]


def encoder_layer_forward(layer, x, mask, freqs):
    """EncoderLayer.forward for a layer with enabled adapters: the training path when grad is enabled and the input, a
    LayerNorm parameter or a lora parameter requires grad, the same launches without a tape otherwise."""
    if not x.is_cuda:
        raise VyomHipError("vyomai_amd ops run on MI355X only: the encoder layer got a CPU tensor (no CPU fallback exists)")
    a, ff = layer.attention, layer.feed_forward
    for m in _all_mods(layer):
        if type(m).__name__ == "DoraLinear":
            raise VyomHipError(f"encoder layer {layer.layer_idx} mixes LoRA and DoRA wrappers, and a layer runs one kind "
                               "(DoRA on the encoder has no training path yet): merge_dora / merge_lora one of them first")
    _frozen_base(f"encoder layer {layer.layer_idx}", a.out.dense.weight, a.out.dense.bias, ff.intermediate.weight,
                 ff.intermediate.bias, ff.out.weight, ff.out.bias, *a._params())
    G = layer_operands(layer, x.dtype, x.device)
    ln1, ln2 = a.out.layernorm, ff.layernorm
    drop1 = _drop_args(a.out.dropout.p, a.out.training)
    drop2 = _drop_args(ff.dropout.p, ff.training)
    attn_p, ffn_p = _group_params(G, ("qkv", "o")), _group_params(G, ("ffn1", "ffn2"))
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in
                                                            (ln1.weight, ln1.bias, ln2.weight, ln2.bias, *attn_p, *ffn_p))):
        out = EncoderLoraAttentionFn.apply(x, layer, mask, freqs, G, drop1, ln1.weight, ln1.bias, *attn_p)
        return EncoderLoraFfnFn.apply(out, x, layer, G, drop2, ln2.weight, ln2.bias, *ffn_p)
    _require_bf16(x)
    am = _attn_args(mask, freqs, x.shape[1], x.device)
    out = _attention_half(x, layer, am, G, drop1, {})[0]
    return _ffn_half(out, x, layer, G, drop2, {})[0]
