"""LoRA fine-tuning inside the fused pre-norm blocks of ModelForCausalLM: the forward of a DecoderLayer whose
projections are wrapped in adapters.LoraLinear, and the LoRA counterparts of autograd_train.PreNormAttentionFn /
PreNormGatedMlpFn.  Both run the bodies those functions run (autograd_train.prenorm_attention_forward / _backward,
prenorm_gated_mlp_forward / _backward) and give them the two hooks defined here, so that

  * the adapter's delta lands behind each of the four GEMMs (vy_lora_shrink / vy_lora_expand over an identity tile
    table, one slot, the serving store's operand layout: a trained adapter is served with the arithmetic it was
    trained with, the storage-dtype rounding of u included) -- before RoPE, so the QKV GEMM is the plain one and
    ops.rope_ rotates the q and k head views of the packed buffer;
  * NO base weight gradient is launched: the base is frozen.  Per GEMM group with output gradient dY the backward adds
    t = dY @ B (one vy_lora_shrink over the block-diagonal transposed B), dX += alpha * t @ A (vy_lora_expand on the
    base dgrad's output) and both low-rank weight gradients in one vy_lora_wgrad.

The packed operands (A, B and their transposes) are rebuilt from lora_a / lora_b when a parameter version or
autograd_train.WEIGHT_EPOCH changes: at most once per optimizer step."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from ._lib import VyomHipError
from .adapters import _CAUSAL_LM, GROUPS, LoraLinear
from .autograd_train import (WEIGHT_EPOCH, _direct, _notify, _require_bf16, prenorm_attention_backward,
                             prenorm_attention_forward, prenorm_gated_mlp_backward, prenorm_gated_mlp_forward)
from .layers.attention import _shadow

NO_CACHE = ("a model whose projections carry LoRA adapters (LoraLinear) cannot run {what}: that path would skip the "
            "adapter's term.  Either fold the adapters into the weights with vyomai_amd.merge_lora(model), or serve the "
            "unwrapped base through ContinuousBatchEngine(..., adapters=store) with the adapter loaded from "
            "lora_state_dict(model)")


def identity_tiles(T: int) -> torch.Tensor:
    """The tile table of T consecutive rows that all carry slot 0 -> int32 (ceil(T / 16), 3) on the host: tile t is
    rows 16 t .. 16 t + 15, the last one ragged."""
    if int(T) != T or T < 1:
        raise ValueError(f"identity_tiles: T = {T} must be a positive integer")
    row0 = torch.arange(0, T, 16, dtype=torch.int32)
    return torch.stack([row0, torch.clamp(T - row0, max=16), torch.zeros_like(row0)], dim=1).contiguous()


_TILES: Dict[Tuple[int, torch.device], Tuple[torch.Tensor, int]] = {}


def _tiles(T: int, dev) -> Tuple[torch.Tensor, int]:
    hit = _TILES.get((T, dev))
    if hit is None:
        host = identity_tiles(T)
        hit = _TILES[(T, dev)] = (host.to(dev), host.shape[0])
    return hit


class GroupOperands:
    """One GEMM group's adapters in the store's layout: A (1, R, K) stacked, B (1, N, r_pad), rank padded to r_pad = 32
    or 64, a part without an adapter all zero; Bt (R, N) block-diagonal transposed B, At (K, R) transposed A."""

    def __init__(self, name: str, mods, dt, dev):
        self.name = name
        self.loras: List[Optional[LoraLinear]] = [m if isinstance(m, LoraLinear) and m.enabled else None for m in mods]
        live = [m for m in self.loras if m is not None]
        alphas = {float(m.alpha) for m in live}
        if len(alphas) != 1:
            raise ValueError(f"{name}: the parts of one packed projection share one alpha, got {sorted(alphas)}")
        self.alpha_f = alphas.pop()
        outs = [m.weight.shape[0] for m in mods]
        self.K, self.N = mods[0].weight.shape[1], sum(outs)
        self.cols = [sum(outs[:p]) for p in range(len(outs))]
        self.bounds = tuple(self.cols[1:])
        self.r_pad = 32 if max(m.rank for m in live) <= 32 else 64
        self.R = len(mods) * self.r_pad
        if self.K % 32 or self.N % 32 or any(o % 16 for o in outs):
            raise ValueError(f"{name}: in_features {self.K} and the packed width {self.N} must be multiples of 32, every "
                             f"out_features {outs} of 16 (vy_lora_shrink / vy_lora_expand)")
        self.A = torch.zeros((1, self.R, self.K), dtype=dt, device=dev)
        self.B = torch.zeros((1, self.N, self.r_pad), dtype=dt, device=dev)
        self.Bt = torch.zeros((self.R, self.N), dtype=dt, device=dev)
        self.alpha = torch.full((1,), self.alpha_f, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, m in enumerate(self.loras):
                if m is None:
                    continue
                a, b = _shadow(m.lora_a, dt).detach(), _shadow(m.lora_b, dt).detach()
                r0, c0 = p * self.r_pad, self.cols[p]
                self.A[0, r0:r0 + m.rank] = a
                self.B[0, c0:c0 + outs[p], :m.rank] = b
                self.Bt[r0:r0 + m.rank, c0:c0 + outs[p]] = b.t()
            self.At = self.A[0].t().contiguous()

    def params(self) -> List[torch.Tensor]:
        return [p for m in self.loras if m is not None for p in (m.lora_a, m.lora_b)]


def _group_mods(layer, g: str):
    out = []
    for path in _CAUSAL_LM[g]:
        owner, attr = path.split(".")
        out.append(getattr(getattr(layer, owner), attr))
    return out


def layer_has_lora(layer) -> bool:
    """Does any projection of this DecoderLayer carry an enabled LoraLinear?  (Every forward of every layer asks,
    decode steps included: seven attribute reads, nothing else.)"""
    a, m = layer.self_attn, layer.mlp
    for mod in (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj):
        if type(mod) is LoraLinear and mod._off == 0:
            return True
    return False


def layer_lora_params(layer) -> List[torch.Tensor]:
    return [p for g in GROUPS for m in _group_mods(layer, g) if isinstance(m, LoraLinear) and m.enabled
            for p in (m.lora_a, m.lora_b)]


def layer_operands(layer, dt, dev) -> Dict[str, Optional[GroupOperands]]:
    """group -> its packed operands (None: no enabled adapter on any of its parts), cached on the layer."""
    cache = layer.__dict__.setdefault("_vy_lora_ops", {})
    out = {}
    for g in GROUPS:
        mods = _group_mods(layer, g)
        live = [m for m in mods if isinstance(m, LoraLinear) and m.enabled]
        if not live:
            out[g] = None
            continue
        key = (tuple((id(m), m.lora_a._version, m.lora_b._version, float(m.alpha), m.rank) for m in live),
               tuple(isinstance(m, LoraLinear) and m.enabled for m in mods), WEIGHT_EPOCH[0], dt, dev)
        hit = cache.get(g)
        if hit is None or hit[0] != key:
            hit = cache[g] = (key, GroupOperands(f"layer {layer.self_attn.layer_idx} {g}", mods, dt, dev))
        out[g] = hit[1]
    return out


def _delta(G: Optional[GroupOperands], y2: torch.Tensor, x2: torch.Tensor) -> Optional[torch.Tensor]:
    """y2 += the group's delta over x2 in place -> u (None without adapters)."""
    if G is None:
        return None
    tiles, n = _tiles(y2.shape[0], y2.device)
    return ops.lora_delta_keep_u_(y2, x2, G.A, G.B, G.alpha, tiles, n, G.bounds, name=G.name)


def _frozen_base(what: str, *params) -> None:
    if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in params):
        raise VyomHipError(f"{what}: a layer with LoRA adapters trains lora_a / lora_b (and its norm weights) only and "
                           "launches no base weight or bias gradient; freeze the wrapped base (add_lora does: "
                           "requires_grad_(False))")


def lora_linear_forward(mod: LoraLinear, x: torch.Tensor) -> torch.Tensor:
    """A LoraLinear called on its own (inference)."""
    if not x.is_cuda:
        raise VyomHipError("vyomai_amd ops run on MI355X only: LoraLinear got a CPU tensor (no CPU fallback exists)")
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in mod.parameters())):
        raise VyomHipError("a LoraLinear trains inside its pre-norm block (DecoderLayer of ModelForCausalLM); call it "
                           "under torch.no_grad() on its own")
    dt = x.dtype
    y = ops.linear(x, _shadow(mod.linear.weight, dt), _shadow(mod.linear.bias, dt))
    if mod.enabled:
        G = GroupOperands("LoraLinear", [mod], dt, x.device)
        x2 = x.reshape(-1, x.shape[-1])
        y2 = torch.as_strided(y, (x2.shape[0], y.shape[-1]), (y.stride(-2) if y.dim() > 1 else y.shape[-1], 1),
                              y.storage_offset())
        _delta(G, y2, x2 if x2.is_contiguous() else x2.contiguous())
    return y


def _rows(t: torch.Tensor) -> torch.Tensor:
    return t.view(-1, t.shape[-1])


def _deltas(G, us: dict):
    """The forward hook of the shared block bodies, f(group, y, x) behind each of the four GEMMs (the serving hook's
    signature, adapters.layer_delta): adds the group's delta to y in place and leaves its u in us[group]."""
    def f(g, y, x):
        us[g] = _delta(G[g], _rows(y), _rows(x))
    return f


def _adapter_backwards(G, us: dict, grads: dict):
    """The backward hooks of the shared block bodies: group -> f(dy, x, dx), for the groups that carry adapters."""
    def hook(g):
        return lambda dy, x, dx: _adapter_backward(G[g], _rows(dy), _rows(x), us[g], None if dx is None else _rows(dx),
                                                   grads)
    return {g: hook(g) for g in G if G[g] is not None}


def _save(ctx, tensors, us: dict) -> None:
    """save_for_backward: the block's tensors, then the u of every group that has one."""
    ctx.groups = tuple(g for g, u in us.items() if u is not None)
    ctx.save_for_backward(*tensors, *(us[g] for g in ctx.groups))


def _saved(ctx, n: int):
    """-> (the block's n tensors, group -> u)."""
    ts = ctx.saved_tensors
    return ts[:n], dict(zip(ctx.groups, ts[n:]))


def _adapter_backward(G: Optional[GroupOperands], dy2, x2, u, dx2, grads: dict):
    """The adapter's part of one group's backward: t = dY @ B, dx2 += alpha * t @ A (dx2 None: nobody reads dX, or the
    caller adds the term itself from the t returned here) and both low-rank weight gradients, delivered as
    autograd_train._wgrad delivers them: accumulated into a trainer's arena gradient in place (and reported ready), or
    as fresh tensors in `grads` (id(parameter) -> gradient).  -> t (None without adapters)."""
    if G is None:
        return None
    tiles, n = _tiles(dy2.shape[0], dy2.device)
    t = ops.lora_dgrad_(dx2, dy2, G.Bt, G.At, G.alpha, tiles, n, name=G.name)
    live = [m for m in G.loras if m is not None and (m.lora_a.requires_grad or m.lora_b.requires_grad)]
    if not live:
        return t
    direct = all(_direct(m.lora_a) and _direct(m.lora_b) for m in live)
    dA: List[Optional[torch.Tensor]] = []
    dB: List[Optional[torch.Tensor]] = []
    for m in G.loras:
        if m is None or m not in live:
            dA.append(None)
            dB.append(None)
        elif direct:
            dA.append(m.lora_a.grad)
            dB.append(m.lora_b.grad)
        else:
            dA.append(torch.empty(m.lora_a.shape, dtype=torch.float32, device=dy2.device))
            dB.append(torch.empty(m.lora_b.shape, dtype=torch.float32, device=dy2.device))
    ops.lora_wgrad(dy2, u, x2, t, dA, dB, G.bounds, G.r_pad, G.alpha_f, accumulate=direct, name=G.name)
    for m, ga, gb in zip(G.loras, dA, dB):
        if ga is None:
            continue
        if direct:
            _notify(m.lora_a, m.lora_b)
        else:
            grads[id(m.lora_a)], grads[id(m.lora_b)] = ga.to(m.lora_a.dtype), gb.to(m.lora_b.dtype)
    return t


def _param_grads(params, grads: dict):
    return tuple(grads.get(id(p)) for p in params)


class LoraPreNormAttentionFn(torch.autograd.Function):
    """PreNormAttentionFn with adapters on any of q / k / v / o and a frozen base.  Inputs after `ln_w`: the lora_a /
    lora_b parameters of the layer's qkv and o groups (autograd tracks them; the values are read from G)."""

    @staticmethod
    def forward(ctx, x, layer, mask, freqs, G, ln_w, *lora_params):
        _require_bf16(x)
        a, us = layer.self_attn, {}
        y, (n, _, _, _, qkv, o, lse), am = prenorm_attention_forward(
            x, a, mask, freqs, ln_w, layer.input_layernorm.variance_epsilon, a.o_proj.weight, delta=_deltas(G, us))
        _save(ctx, (x, n, qkv, o, lse), us)
        ctx.meta = (layer, G, am, ln_w, lora_params)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x, n, qkv, o, lse), us = _saved(ctx, 5)
        layer, G, am, ln_w, lora_params = ctx.meta
        a, grads = layer.self_attn, {}
        # (layer 0 over a frozen embedding and a frozen norm: nobody reads dx)
        dx, dlnw, *_ = prenorm_attention_backward(
            dy, x, n, o, lse, am, a, ln_w, layer.input_layernorm.variance_epsilon, a.o_proj.weight, qkv=qkv,
            adapters=_adapter_backwards(G, us, grads), need_dx=ctx.needs_input_grad[0] or ln_w.requires_grad)
        return (dx, None, None, None, None, dlnw, *_param_grads(lora_params, grads))


class LoraPreNormGatedMlpFn(torch.autograd.Function):
    """PreNormGatedMlpFn with adapters on any of gate / up / down and a frozen base."""

    @staticmethod
    def forward(ctx, x, layer, G, ln_w, *lora_params):
        _require_bf16(x)
        mlp, us = layer.mlp, {}
        y, n, gu = prenorm_gated_mlp_forward(x, mlp, ln_w, layer.post_attention_layernorm.variance_epsilon, mlp.act,
                                             mlp.down_proj.weight, delta=_deltas(G, us))
        _save(ctx, (x, n, gu), us)
        ctx.meta = (layer, G, ln_w, lora_params)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x, n, gu), us = _saved(ctx, 3)
        layer, G, ln_w, lora_params = ctx.meta
        mlp, grads = layer.mlp, {}
        dx, dlnw, *_ = prenorm_gated_mlp_backward(
            dy, x, n, gu, mlp, ln_w, layer.post_attention_layernorm.variance_epsilon, mlp.act, mlp.gate_proj.weight,
            mlp.up_proj.weight, mlp.down_proj.weight, adapters=_adapter_backwards(G, us, grads))
        return (dx, None, None, dlnw, *_param_grads(lora_params, grads))


def decoder_layer_forward(layer, x, mask, freqs, past_key_value):
    """DecoderLayer.forward for a layer with enabled adapters: the training path when grad is enabled and the input or
    a lora parameter requires grad, the same launches without a tape otherwise."""
    if past_key_value is not None:
        raise VyomHipError(NO_CACHE.format(what="with a KV cache (generate(), past_key_values=)"))
    a, m = layer.self_attn, layer.mlp
    ln1, ln2 = layer.input_layernorm, layer.post_attention_layernorm
    _frozen_base(f"layer {a.layer_idx}", a.o_proj.weight, m.gate_proj.weight, m.up_proj.weight, m.down_proj.weight,
                 *a._params())
    G = layer_operands(layer, x.dtype, x.device)
    attn_p = [p for g in ("qkv", "o") if G[g] is not None for p in G[g].params()]
    mlp_p = [p for g in ("gate_up", "down") if G[g] is not None for p in G[g].params()]
    if torch.is_grad_enabled() and (x.requires_grad or ln1.weight.requires_grad or ln2.weight.requires_grad
                                    or any(p.requires_grad for p in attn_p + mlp_p)):
        x = LoraPreNormAttentionFn.apply(x, layer, mask, freqs, G, ln1.weight, *attn_p)
        return LoraPreNormGatedMlpFn.apply(x, layer, G, ln2.weight, *mlp_p)
    _require_bf16(x)
    delta = _deltas(G, {})
    x = prenorm_attention_forward(x, a, mask, freqs, ln1.weight, ln1.variance_epsilon, a.o_proj.weight, delta=delta)[0]
    return prenorm_gated_mlp_forward(x, m, ln2.weight, ln2.variance_epsilon, m.act, m.down_proj.weight, delta=delta)[0]
