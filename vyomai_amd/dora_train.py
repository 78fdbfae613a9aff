"""DoRA fine-tuning inside the fused pre-norm blocks of ModelForCausalLM: the forward and backward of a DecoderLayer
whose projections are wrapped in adapters.DoraLinear.  The reference's DoRA re-parameterises the weight,

    D = W + dora_a @ dora_b      c = ||D||_2 over dim 0      W' = dora_m * D / c

so every bit of adapter arithmetic is weight-sized.  A wrapped layer therefore runs the PLAIN block bodies
(autograd_train.prenorm_attention_forward / _backward, prenorm_gated_mlp_forward / _backward) launch for launch -- the
fused QKV + RoPE GEMM included -- on composed weights handed to them in place of the base shadows:

  * LayerWeights composes a layer's W' and c in ONE vy_dora_compose call, into the packed [q; k; v] and [gate; up]
    buffers the GEMMs read (a part without an adapter gets a copy of its plain shadow rows), and keeps them until a dora
    parameter's version or autograd_train.WEIGHT_EPOCH changes: at most once per optimizer step.  The transposed copies
    the dgrads read go through autograd_train._wt_cached with the composed matrix as source.
  * NO base weight gradient reaches a parameter: the base is frozen.  The backward produces G = dL/dW' for each group
    with a wrapped part through the existing weight-gradient launchers, into fp32 scratch that lives for one layer, and
    ONE vy_dora_bwd call per layer turns it into the gradients of dora_m, dora_a and dora_b -- at the end of the
    attention half's backward, the last of the layer to run, which is why that function owns all of the layer's dora
    parameters.  A group without a wrapped part launches no weight gradient at all."""
from __future__ import annotations

from typing import Dict, List

import torch

from . import autograd_train, ops
from ._lib import VyomHipError
from .adapters import _CAUSAL_LM, GROUPS, DoraLinear, LoraLinear
from .autograd_train import (WEIGHT_EPOCH, _direct, _notify, _require_bf16, _wt_cached, prenorm_attention_backward,
                             prenorm_attention_forward, prenorm_gated_mlp_backward, prenorm_gated_mlp_forward)
from .layers.attention import _shadow

NO_CACHE = ("a model whose projections carry DoRA adapters (DoraLinear) cannot run {what}: that path reads the base "
            "weights and would compute the base model.  Fold the adapters into the weights with "
            "vyomai_amd.merge_dora(model) first (DoRA renormalises the whole weight, so it is served merged)")


def _group_mods(layer, g: str):
    out = []
    for path in _CAUSAL_LM[g]:
        owner, attr = path.split(".")
        out.append(getattr(getattr(layer, owner), attr))
    return out


def _live(m) -> bool:
    return type(m) is DoraLinear and m._off == 0


def layer_has_dora(layer) -> bool:
    """Does any projection of this DecoderLayer carry an enabled DoraLinear?  (Every forward of every layer asks: seven
    attribute reads, nothing else.)"""
    a, m = layer.self_attn, layer.mlp
    for mod in (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj):
        if type(mod) is DoraLinear and mod._off == 0:
            return True
    return False


def _mod_params(m: DoraLinear) -> List[torch.Tensor]:
    return [m.dora_m, m.dora_a, m.dora_b]


def layer_dora_params(layer) -> List[torch.Tensor]:
    return [p for g in GROUPS for m in _group_mods(layer, g) if _live(m) for p in _mod_params(m)]


def _f32(p: torch.Tensor) -> torch.Tensor:
    """A dora parameter as the kernels read it: contiguous float32 (the parameter itself when it is)."""
    return _shadow(p, torch.float32).detach().contiguous()


class _Group:
    """One GEMM group's composed weight: w (N, K) in the compute dtype, the row offsets of its parts, and -- as the owner
    object autograd_train._wt_cached asks for -- its transposed copy, keyed on `stamp`."""

    def __init__(self, mods, dt, dev):
        self.mods = list(mods)
        self.outs = [m.weight.shape[0] for m in mods]
        self.rows = [sum(self.outs[:p]) for p in range(len(mods))]
        self.K = mods[0].weight.shape[1]
        self.w = torch.empty((sum(self.outs), self.K), dtype=dt, device=dev)
        self.c = {p: torch.empty((self.K,), dtype=torch.float32, device=dev) for p, m in enumerate(mods) if _live(m)}
        self.stamp = 0

    def part(self, p: int) -> torch.Tensor:
        return self.w[self.rows[p]:self.rows[p] + self.outs[p]]


class LayerWeights:
    """The composed weights of one layer in one compute dtype: w (group -> matrix, only the groups with an enabled
    DoraLinear), wt(group) and c; what the block bodies take as `weights`."""

    def __init__(self, layer, dt, dev):
        self.groups: Dict[str, _Group] = {}
        for g in GROUPS:
            mods = _group_mods(layer, g)
            if any(_live(m) for m in mods):
                self.groups[g] = _Group(mods, dt, dev)
        self.w = {g: G.w for g, G in self.groups.items()}
        self.dt = dt

    def compose(self) -> None:
        problems = []
        with torch.no_grad():
            for G in self.groups.values():
                for p, m in enumerate(G.mods):
                    if _live(m):
                        problems.append(ops.DoraProblem(w=m.linear.weight.detach(), a=_f32(m.dora_a), b=_f32(m.dora_b),
                                                        m=_f32(m.dora_m), c=G.c[p], wp=G.part(p)))
                    else:       # (no problem of the launch: its plain shadow rows)
                        G.part(p).copy_(_shadow(m.weight, self.dt).detach())
                G.stamp += 1
            ops.dora_compose(problems)

    def wt(self, g: str) -> torch.Tensor:
        dt = self.dt
        return _wt_cached(self.groups[g], lambda G: (G.stamp, dt), lambda G: G.w)

    def params(self) -> List[torch.Tensor]:
        return [p for G in self.groups.values() for m in G.mods if _live(m) for p in _mod_params(m)]


def layer_weights(layer, dt, dev) -> LayerWeights:
    """The layer's composed weights, cached on the layer; rebuilt -- one vy_dora_compose call -- when a dora parameter's
    or a wrapped base weight's version, the set of enabled wrappers or WEIGHT_EPOCH changed."""
    mods = [m for g in GROUPS for m in _group_mods(layer, g)]
    key = (tuple((id(m), _live(m), m.weight._version) + (tuple(p._version for p in _mod_params(m)) if _live(m) else ())
                 for m in mods), WEIGHT_EPOCH[0], dt, dev)
    shape = tuple(_live(m) for m in mods) + (dt, dev)
    hit = layer.__dict__.get("_vy_dora_w")
    if hit is None or hit[0] != shape:
        hit = [shape, None, LayerWeights(layer, dt, dev)]
        layer.__dict__["_vy_dora_w"] = hit
    if hit[1] != key:
        hit[2].compose()
        hit[1] = key
    return hit[2]


def _frozen_base(layer) -> None:
    a, m = layer.self_attn, layer.mlp
    base = [a.o_proj.weight, m.gate_proj.weight, m.up_proj.weight, m.down_proj.weight, *a._params()]
    if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in base):
        raise VyomHipError(f"layer {a.layer_idx}: a layer with DoRA adapters trains dora_m / dora_a / dora_b (and its norm "
                           "weights) only and delivers no base weight or bias gradient; freeze the base (add_dora does: "
                           "requires_grad_(False))")


def dora_linear_forward(mod: DoraLinear, x: torch.Tensor) -> torch.Tensor:
    """A DoraLinear called on its own (inference): compose + ops.linear."""
    if not x.is_cuda:
        raise VyomHipError("vyomai_amd ops run on MI355X only: DoraLinear got a CPU tensor (no CPU fallback exists)")
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in mod.parameters())):
        raise VyomHipError("a DoraLinear trains inside its pre-norm block (DecoderLayer of ModelForCausalLM); call it "
                           "under torch.no_grad() on its own")
    dt = x.dtype
    if not mod.enabled:
        return ops.linear(x, _shadow(mod.linear.weight, dt), _shadow(mod.linear.bias, dt))
    w = torch.empty(mod.linear.weight.shape, dtype=dt, device=x.device)
    c = torch.empty((mod.in_features,), dtype=torch.float32, device=x.device)
    ops.dora_compose([ops.DoraProblem(w=mod.linear.weight.detach(), a=_f32(mod.dora_a), b=_f32(mod.dora_b),
                                      m=_f32(mod.dora_m), c=c, wp=w)])
    return ops.linear(x, w, _shadow(mod.linear.bias, dt))


# ---- backward: G per group, then one vy_dora_bwd per layer ------------------------------------------------------------

_ITEMS = "grouped launch"     # key of `pend`: the (dy, x, G, None) items that wait for the layer's grouped launch


def _g_hooks(W: LayerWeights, names, pend: dict):
    """The `adapters` hooks of the shared block bodies, group -> f(dy, x, dx), for the groups of `names` that carry a
    wrapped part: G = dy^T x into fp32 scratch, left in pend[group] for _deliver.  A problem that the full-weight path
    would put into its grouped launch (autograd_train._wgrad_group.wants: enough rows, a tile count worth grouping)
    waits for the layer's ONE ops.linear_wgrad_grouped call in _deliver; the others launch here."""
    def hook(g):
        def f(dy, x, dx):
            G = W.groups[g]
            d2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
            if autograd_train._wgrad_group.wants(d2, G.w, None):
                buf = torch.zeros((G.w.shape[0], G.K), dtype=torch.float32, device=dy.device)   # (the launch accumulates)
                pend.setdefault(_ITEMS, []).append((d2, x2, buf, None))
            else:
                buf = torch.empty((G.w.shape[0], G.K), dtype=torch.float32, device=dy.device)
                ops.linear_wgrad(d2, x2, buf, None, accumulate=False)
            pend[g] = buf
        return f
    return {g: hook(g) for g in names if g in W.groups}


def _deliver(W: LayerWeights, pend: dict, grads: dict) -> None:
    """One vy_dora_bwd over every wrapped projection whose G is in `pend`, delivered as autograd_train._wgrad delivers a
    weight gradient: accumulated into a trainer's arena gradients in place (and reported ready), or as fresh tensors
    in `grads` (id(parameter) -> gradient)."""
    items = pend.pop(_ITEMS, None)
    if items:
        ops.linear_wgrad_grouped(items)
    todo = []
    for g, buf in pend.items():
        G = W.groups[g]
        for p, m in enumerate(G.mods):
            if _live(m) and any(q.requires_grad for q in _mod_params(m)):
                todo.append((G, p, m, buf[G.rows[p]:G.rows[p] + G.outs[p]]))
    pend.clear()
    if not todo:
        return
    direct = all(_direct(q) for *_, m, _ in todo for q in _mod_params(m) if q.requires_grad)
    problems, outs = [], []
    for G, p, m, g_rows in todo:
        dst = []
        for q in _mod_params(m):
            if direct and q.requires_grad:
                dst.append(q.grad)
            else:   # (returned to autograd below, or -- a parameter that does not train -- dropped)
                dst.append(torch.empty(q.shape, dtype=torch.float32, device=g_rows.device))
        problems.append(ops.DoraProblem(w=m.linear.weight.detach(), a=_f32(m.dora_a), b=_f32(m.dora_b), m=_f32(m.dora_m),
                                        c=G.c[p], g=g_rows, dm=dst[0], da=dst[1], db=dst[2]))
        outs.append((m, dst))
    ops.dora_bwd(problems, accumulate=direct)
    for m, dst in outs:
        live = [q for q in _mod_params(m) if q.requires_grad]
        if direct:
            _notify(*live)
        else:
            for q, t in zip(_mod_params(m), dst):
                if q.requires_grad:
                    grads[id(q)] = t.to(q.dtype)


class DoraPreNormAttentionFn(torch.autograd.Function):
    """PreNormAttentionFn on composed weights with a frozen base.  Inputs after `ln_w`: ALL of the layer's dora
    parameters, the MLP half's too -- this backward is the last of the layer to run and delivers them in one call."""

    @staticmethod
    def forward(ctx, x, layer, mask, freqs, W, pend, ln_w, *dora_params):
        _require_bf16(x)
        a = layer.self_attn
        y, (n, q, k, v, _, o, lse), am = prenorm_attention_forward(
            x, a, mask, freqs, ln_w, layer.input_layernorm.variance_epsilon, a.o_proj.weight, weights=W)
        ctx.save_for_backward(x, n, q, k, v, o, lse)
        ctx.meta = (layer, W, pend, am, ln_w, dora_params)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, n, q, k, v, o, lse = ctx.saved_tensors
        layer, W, pend, am, ln_w, dora_params = ctx.meta
        a, grads = layer.self_attn, {}
        # (layer 0 over a frozen embedding and a frozen norm: nobody reads dx)
        dx, dlnw, *_ = prenorm_attention_backward(
            dy, x, n, o, lse, am, a, ln_w, layer.input_layernorm.variance_epsilon, a.o_proj.weight, q=q, k=k, v=v,
            adapters=_g_hooks(W, ("qkv", "o"), pend), need_dx=ctx.needs_input_grad[0] or ln_w.requires_grad, weights=W)
        _deliver(W, pend, grads)
        return (dx, None, None, None, None, None, dlnw, *(grads.get(id(p)) for p in dora_params))


class DoraPreNormGatedMlpFn(torch.autograd.Function):
    """PreNormGatedMlpFn on composed weights with a frozen base; its G stay in `pend` for the attention half."""

    @staticmethod
    def forward(ctx, x, layer, W, pend, ln_w):
        _require_bf16(x)
        mlp = layer.mlp
        y, n, gu = prenorm_gated_mlp_forward(x, mlp, ln_w, layer.post_attention_layernorm.variance_epsilon, mlp.act,
                                             mlp.down_proj.weight, weights=W)
        ctx.save_for_backward(x, n, gu)
        ctx.meta = (layer, W, pend, ln_w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, n, gu = ctx.saved_tensors
        layer, W, pend, ln_w = ctx.meta
        mlp = layer.mlp
        dx, dlnw, *_ = prenorm_gated_mlp_backward(
            dy, x, n, gu, mlp, ln_w, layer.post_attention_layernorm.variance_epsilon, mlp.act, mlp.gate_proj.weight,
            mlp.up_proj.weight, mlp.down_proj.weight, adapters=_g_hooks(W, ("gate_up", "down"), pend), weights=W)
        return dx, None, None, None, dlnw


def decoder_layer_forward(layer, x, mask, freqs, past_key_value):
    """DecoderLayer.forward for a layer with enabled DoRA adapters: the training path when grad is enabled and the input
    or a dora parameter requires grad, the same launches without a tape otherwise."""
    if past_key_value is not None:
        raise VyomHipError(NO_CACHE.format(what="with a KV cache (generate(), past_key_values=)"))
    a, m = layer.self_attn, layer.mlp
    if any(isinstance(mod, LoraLinear) for g in GROUPS for mod in _group_mods(layer, g)):
        raise VyomHipError(f"layer {a.layer_idx} carries LoRA and DoRA adapters; a layer runs one kind (merge one first)")
    ln1, ln2 = layer.input_layernorm, layer.post_attention_layernorm
    _frozen_base(layer)
    W = layer_weights(layer, x.dtype, x.device)
    params = W.params()
    if torch.is_grad_enabled() and (x.requires_grad or ln1.weight.requires_grad or ln2.weight.requires_grad
                                    or any(p.requires_grad for p in params)):
        pend: Dict[str, torch.Tensor] = {}
        x = DoraPreNormAttentionFn.apply(x, layer, mask, freqs, W, pend, ln1.weight, *params)
        return DoraPreNormGatedMlpFn.apply(x, layer, W, pend, ln2.weight)
    _require_bf16(x)
    x = prenorm_attention_forward(x, a, mask, freqs, ln1.weight, ln1.variance_epsilon, a.o_proj.weight, weights=W)[0]
    return prenorm_gated_mlp_forward(x, m, ln2.weight, ln2.variance_epsilon, m.act, m.down_proj.weight, weights=W)[0]
