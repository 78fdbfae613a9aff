"""The model that the reference's Examples/simple_vllm.ipynb serves -- Qwen3Model and its parts (RMSNorm, FeedForward,
GroupedQueryAttention, TransformerBlock) under the notebook's class names, attribute names, cfg keys and parameter
dtypes, so state dicts interchange with strict loads in both directions -- behind the protocol of this package's
paged-KV engine (serving.ContinuousBatchEngine calls `forward_paged`; PagedKVManager reads `.config`).

cfg keys: vocab_size, context_length, emb_dim, n_heads, n_layers, hidden_dim, head_dim, qk_norm, n_kv_groups, rope_base,
dtype.  n_heads * head_dim need not equal emb_dim; out_head is a matrix of its own unless load_weights_into_qwen (or the
caller) ties it to tok_emb.  Linears and the embedding are in cfg["dtype"], every RMSNorm scale is fp32.

What differs from the notebook:

* qk_norm.  The per-head RMSNorm of q and k, the rotation and the page store are ONE launch
  (vy_paged_qknorm_rope_write): fp32 from the load of the projection to the one store.  The notebook's bf16 model rounds
  to bf16 after the norm and rotates in bf16 with its bf16 cos_buf / sin_buf.
* RoPE tables.  cos_buf / sin_buf are registered in cfg["dtype"] as the notebook registers them (they are part of its
  state dict) but no kernel reads them: the kernels read fp32 tables from the same formula, built on the host at
  construction and uploaded once per device.
* The block norms run through vy_rmsnorm_fwd, which takes the scale in the activations' dtype: in a bf16 model the fp32
  scale is rounded to bf16 once (a cached copy), where the notebook multiplies by the fp32 scale before its rounding.
* The notebook-signature forward(input_ids, k_caches, v_caches, metadata) is not reproduced (its mixed-step semantics
  are the engine's departure 1, serving.py).

Training (a model built with cfg["dtype"] = torch.float32: the parameters are the trainer's masters): forward_hidden,
clm_loss, sequence_logprobs and dpo_loss run each half of a block as ONE autograd function, as ModelForCausalLM does --
autograd_train.PreNormQkNormAttentionFn (vy_qknorm_rope_fwd / vy_qknorm_bwd around the plain packed QKV GEMM; a block
without qk_norm takes PreNormAttentionFn) and PreNormGatedMlpFn -- and the head through TiedLMHeadLossFn /
TiedLMHeadLogprobFn, tied or not.  GroupedQueryAttention and FeedForward carry the attribute names those functions ask
of a module as aliases over their own parameters.  LoRA on this model is not wired."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from .._lib import ACT_SILU, VyomHipError
from ..adapters import layer_delta
from ..autograd import gated_mlp
from ..layers.attention import _shadow
from ..layers.mask import AttnMask
from ..layers.paged import page_scales, paged_step_attention, paged_step_logits
from ..layers.positional_embeddings import RopeSlice, RopeTable
from .common import SequenceScoreMixin
from .custom_transformer import _need_gpu


def _packed_rows(owner: nn.Module, slot: str, linears, dtype: torch.dtype) -> torch.Tensor:
    """[W0; W1; ...] of bias-free linears in `dtype` for one packed GEMM.  A view when the copies sit back to back in one
    buffer (the trainer's arenas lay them out so); else a concatenation cached on `owner`, rebuilt when a member is
    written (its version counter), replaced (`lin.weight = ...`) or moved (its data pointer), or when the trainer's
    AdamW kernel has rewritten the arena copies (the weight epoch: it does not touch tensor versions)."""
    from ..autograd_train import WEIGHT_EPOCH
    ws = [lin.weight for lin in linears]
    cs = [_shadow(w, dtype).detach() for w in ws]
    c0, end = cs[0], cs[0].data_ptr()
    for c in cs:
        if not c.is_contiguous() or c.data_ptr() != end or \
                c.untyped_storage().data_ptr() != c0.untyped_storage().data_ptr():   # one buffer, not two neighbours
            break
        end += c.numel() * c.element_size()
    else:
        return torch.as_strided(c0, (sum(c.shape[0] for c in cs), c0.shape[1]), (c0.shape[1], 1))
    key = tuple((w._version, w.data_ptr()) for w in ws) + (WEIGHT_EPOCH[0], dtype)
    hit = getattr(owner, slot, None)
    if hit is None or hit[0] != key:
        hit = (key, torch.cat(cs, dim=0).contiguous())
        setattr(owner, slot, hit)
    return hit[1]


def _linear(cfg, n_in: int, n_out: int) -> nn.Linear:
    return nn.Linear(n_in, n_out, bias=False, dtype=cfg["dtype"])


class RMSNorm(nn.Module):
    """x * rsqrt(mean x^2 + eps) * scale (+ shift), statistics in fp32; scale (and shift) are fp32 parameters whatever
    the model's dtype.  `shift` exists for state-dict parity (bias=True); no kernel adds it and no model here uses it."""

    def __init__(self, emb_dim, eps=1e-6, bias=False):
        super().__init__()
        self.eps = float(eps)
        self.scale = nn.Parameter(torch.ones(emb_dim, dtype=torch.float32))
        self.register_parameter("shift", nn.Parameter(torch.zeros(emb_dim, dtype=torch.float32)) if bias else None)

    def forward(self, x):
        _need_gpu(x, "RMSNorm")
        if self.shift is not None:      # (no kernel adds it)
            raise VyomHipError("RMSNorm(bias=True): vy_rmsnorm_fwd has no shift operand")
        return ops.rmsnorm(x, _shadow(self.scale, x.dtype), self.eps, 0.0)

    def extra_repr(self):
        return f"{tuple(self.scale.shape)}, eps={self.eps}"


class FeedForward(nn.Module):
    """fc3(silu(fc1(x)) * fc2(x)): one packed [fc1; fc2] GEMM, vy_gated_act_fwd, fc3 with the residual in its epilogue."""

    def __init__(self, cfg):
        super().__init__()
        d, f = cfg["emb_dim"], cfg["hidden_dim"]
        self.fc1, self.fc2, self.fc3 = _linear(cfg, d, f), _linear(cfg, d, f), _linear(cfg, f, d)

    # what autograd_train.PreNormGatedMlpFn asks of a gated MLP, over the same three linears (no state_dict key)
    act = ACT_SILU
    gate_proj = property(lambda self: self.fc1)
    up_proj = property(lambda self: self.fc2)
    down_proj = property(lambda self: self.fc3)

    def _packed_gate_up(self, dtype: torch.dtype) -> torch.Tensor:
        return _packed_rows(self, "_vy_gu", (self.fc1, self.fc2), dtype)

    @torch.no_grad()
    def forward(self, x, residual: Optional[torch.Tensor] = None, delta=None):
        """delta (serving with adapters, adapters.layer_delta): f(group, y, x), called behind each of the two GEMMs."""
        _need_gpu(x, "FeedForward")
        return gated_mlp(x, self, ACT_SILU, _shadow(self.fc3.weight, x.dtype), residual, delta)[0]


class GroupedQueryAttention(nn.Module):
    """The projections and the optional q_norm / k_norm (RMSNorm(head_dim), one scale shared by all heads).  The
    computation lives in Qwen3Model.forward_paged: the norm in front and the residual behind share its launches."""

    def __init__(self, layer_idx, cfg):
        super().__init__()
        self.layer_idx, self.head_dim = layer_idx, cfg["head_dim"]
        self.num_heads, self.num_kv_groups = cfg["n_heads"], cfg["n_kv_groups"]
        if self.head_dim % 8 or self.head_dim > 256:
            raise ValueError(f"head_dim {self.head_dim} must be a multiple of 8 up to 256")
        if self.num_heads % self.num_kv_groups:
            raise ValueError(f"n_heads {self.num_heads} must be a multiple of n_kv_groups {self.num_kv_groups}")
        d, q_cols, kv_cols = cfg["emb_dim"], self.num_heads * self.head_dim, self.num_kv_groups * self.head_dim
        self.W_query, self.W_key, self.W_value = _linear(cfg, d, q_cols), _linear(cfg, d, kv_cols), _linear(cfg, d, kv_cols)
        self.out_proj = _linear(cfg, q_cols, d)
        qk_norm = bool(cfg.get("qk_norm"))
        self.q_norm = RMSNorm(self.head_dim) if qk_norm else None
        self.k_norm = RMSNorm(self.head_dim) if qk_norm else None

    def _packed_qkv(self, dtype: torch.dtype) -> torch.Tensor:
        return _packed_rows(self, "_vy_qkv", (self.W_query, self.W_key, self.W_value), dtype)

    # what autograd_train's packed-QKV functions (_packed_wgrad, _wt_packed, PreNorm*AttentionFn) ask of an attention
    # module, over the same three bias-free linears (no state_dict key, no second copy of a weight)
    _fused_qkv = False
    attention_bias = False
    num_attention_heads = property(lambda self: self.num_heads)
    num_key_value_heads = property(lambda self: self.num_kv_groups)

    def _params(self):
        return [self.W_query.weight, self.W_key.weight, self.W_value.weight]

    def _packed(self):
        return self._packed_qkv(self.W_query.weight.dtype), None

    def _packed_shadow(self, dtype: torch.dtype):
        return self._packed_qkv(dtype), None

    def forward(self, *args, **kwargs):
        raise VyomHipError("GroupedQueryAttention runs inside Qwen3Model.forward_paged")


class TransformerBlock(nn.Module):
    def __init__(self, cfg, layer_idx):
        super().__init__()
        self.att, self.ff = GroupedQueryAttention(layer_idx, cfg), FeedForward(cfg)
        self.norm1 = RMSNorm(cfg["emb_dim"])
        self.norm2 = RMSNorm(cfg["emb_dim"])

    def forward(self, *args, **kwargs):
        raise VyomHipError("TransformerBlock runs inside Qwen3Model.forward_paged")


class _ConfigView:
    """What PagedKVManager and ContinuousBatchEngine read from a model's config, derived from the cfg dict."""

    def __init__(self, cfg):
        self.vocab_size = cfg["vocab_size"]
        self.hidden_size = cfg["emb_dim"]
        self.intermediate_size = cfg["hidden_dim"]
        self.num_hidden_layers = cfg["n_layers"]
        self.num_attention_heads = cfg["n_heads"]
        self.num_key_value_heads = cfg["n_kv_groups"]
        self.head_dim = cfg["head_dim"]
        self.max_position_embeddings = cfg["context_length"]
        self.rope_theta = cfg["rope_base"]


class Qwen3Model(nn.Module, SequenceScoreMixin):
    """tok_emb, trf_blocks, final_norm, out_head and the cos_buf / sin_buf buffers of the notebook's model;
    `forward_paged` is the engine's protocol, `.config` the view PagedKVManager(model.config, ...) needs;
    forward_hidden / clm_loss / sequence_logprobs / dpo_loss are the training side (fp32 parameters)."""

    compute_dtype = None   # set by FlatTrainer (None = the parameters' dtype)

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.config = _ConfigView(cfg)
        d, vocab, dh = cfg["emb_dim"], cfg["vocab_size"], cfg["head_dim"]
        self.tok_emb = nn.Embedding(vocab, d, dtype=cfg["dtype"])
        self.trf_blocks = nn.ModuleList(TransformerBlock(cfg, i) for i in range(cfg["n_layers"]))
        self.final_norm = RMSNorm(d)
        self.out_head = _linear(cfg, d, vocab)
        inv_freq = 1.0 / (cfg["rope_base"] ** (torch.arange(0, dh, 2).float() / dh))
        freqs = torch.outer(torch.arange(cfg["context_length"]).float(), inv_freq)
        cos, sin = freqs.cos().contiguous(), freqs.sin().contiguous()
        self.register_buffer("cos_buf", cos.to(cfg["dtype"]))
        self.register_buffer("sin_buf", sin.to(cfg["dtype"]))
        # the tables the kernels read: fp32, evaluated on the host by the same two calls and uploaded once per device
        # (not buffers: they are neither saved nor cast by .to(dtype))
        self._rope = RopeTable(freqs)

    def tie_head(self) -> None:
        """out_head shares tok_emb's matrix from now on (state_dict() keeps both names)."""
        self.out_head.weight = self.tok_emb.weight

    def _rope_tables(self, dev: torch.device):
        return self._rope.on(dev)

    def forward(self, *args, **kwargs):
        raise VyomHipError("Qwen3Model is served through forward_paged(input_ids, positions, metadata, kv_mgr) "
                           "(serving.ContinuousBatchEngine); the notebook's forward(input_ids, k_caches, v_caches, "
                           "metadata) is not reproduced")

    # ---- training ---------------------------------------------------------------------------------
    def _table_pending(self, input_ids) -> bool:
        """Does this graph's backward also scatter embedding gradients into the head's table?  Only a tied head: an
        untied one is a table that embedded nothing."""
        w = self.tok_emb.weight
        return input_ids is not None and self.out_head.weight is w and torch.is_grad_enabled() and w.requires_grad

    def forward_hidden(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The trunk without the final norm over whole sequences: input_ids (B, L), positions 0 .. L-1 in every row;
        attention_mask: a 2-D padding mask (1 = token), which becomes the causal + key-padding descriptor.  With grad
        each half of a block is one autograd function; under torch.no_grad() the same launches run and nothing is
        kept."""
        from ..autograd_train import (EmbeddingFn, PreNormAttentionFn, PreNormGatedMlpFn, PreNormQkNormAttentionFn)
        _need_gpu(input_ids, "forward_hidden()")
        B, L = input_ids.shape
        if L > self.cfg["context_length"]:
            raise ValueError(f"sequence length {L} exceeds context_length {self.cfg['context_length']}")
        w = self.tok_emb.weight
        if torch.is_grad_enabled() and w.dtype != torch.float32 and any(p.requires_grad for p in self.parameters()):
            raise VyomHipError(f"Qwen3Model trains on fp32 parameters (the trainer's masters), these are {w.dtype}: build "
                               "the model with cfg['dtype'] = torch.float32 and load_state_dict() into it; bf16 compute "
                               "comes from FlatTrainer(model)")
        dt = self.compute_dtype or w.dtype
        if torch.is_grad_enabled() and w.requires_grad:
            x = EmbeddingFn.apply(input_ids, w, None, dt)
        else:
            x = ops.embedding(_shadow(w, dt), input_ids)
        if attention_mask is not None:
            if attention_mask.dim() != 2:
                raise VyomHipError("training needs a mask descriptor (pass the 2-D padding mask): dense additive masks "
                                   "have no backward kernel")
            mask = AttnMask.from_padding(attention_mask, causal=True, start_pos=0, query_len=L)
        else:
            mask = AttnMask(causal=True, start_pos=0, query_len=L, key_len=L) if L > 1 else None
        freqs = RopeSlice(self._rope, 0, L)
        for blk in self.trf_blocks:
            a, ff = blk.att, blk.ff
            if a.q_norm is not None:
                if a.q_norm.eps != a.k_norm.eps:
                    raise ValueError("q_norm and k_norm share one eps in vy_qknorm_rope_fwd")
                x = PreNormQkNormAttentionFn.apply(x, a, mask, freqs, blk.norm1.scale, blk.norm1.eps, a.out_proj.weight,
                                                   a.q_norm.scale, a.k_norm.scale, a.q_norm.eps, *a._params())
            else:
                x = PreNormAttentionFn.apply(x, a, mask, freqs, blk.norm1.scale, blk.norm1.eps, a.out_proj.weight,
                                             *a._params())
            x = PreNormGatedMlpFn.apply(x, ff, blk.norm2.scale, blk.norm2.eps, ff.act, ff.fc1.weight, ff.fc2.weight,
                                        ff.fc3.weight)
        return x

    def clm_loss(self, input_ids: torch.Tensor, labels: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                 ignore_index: int = -100) -> torch.Tensor:
        """Shifted next-token loss with the final RMSNorm, the vocabulary GEMM (out_head, tied or not) and the
        cross-entropy fused: the logits are reduced and overwritten by their gradient in place, never kept."""
        from ..autograd_train import TiedLMHeadLossFn
        hidden = self.forward_hidden(input_ids, attention_mask)
        return TiedLMHeadLossFn.apply(hidden, labels, ignore_index, self.final_norm.scale, self.final_norm.eps,
                                      self.out_head.weight, self._table_pending(input_ids),
                                      self._label_flag(hidden.device))

    # sequence_logprobs / dpo_loss: common.SequenceScoreMixin over these two
    def _score_trunk(self, input_ids, attention_mask, inputs_embeds=None):
        if inputs_embeds is not None:
            raise VyomHipError("Qwen3Model scores token ids (inputs_embeds is not wired)")
        return self.forward_hidden(input_ids, attention_mask)

    def _score_head(self):
        return self.final_norm.scale, self.final_norm.eps, self.out_head.weight

    # ---- serving ----------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_paged(self, input_ids: torch.Tensor, positions: torch.Tensor, metadata: dict, kv_mgr) -> torch.Tensor:
        """One step of serving.ContinuousBatchEngine -> logits (sequences, vocab) of the last row of each sequence whose
        rows reach its last token; arguments as ModelForCausalLM.forward_paged.

        Per layer: norm1 (vy_rmsnorm_fwd), the packed QKV GEMM, vy_paged_qknorm_rope_write (cfg["qk_norm"]; else
        vy_paged_rope_write), vy_attn_paged_decode for the rows with one query token, for the prefill rows ONE
        vy_attn_paged_prefill (varlen_prefill) or causal vy_attn_fwd per sequence (against its gathered pages when it
        starts from cached prefix blocks), out_proj with the residual, norm2, the packed fc1|fc2 GEMM,
        vy_gated_act_fwd (silu), fc3 with the residual.  final_norm and out_head see metadata["last_rows"] only."""
        _need_gpu(input_ids, "forward_paged()")
        if int(metadata["max_position"]) > self.cfg["context_length"]:
            raise ValueError(f"position {int(metadata['max_position'])} exceeds context_length {self.cfg['context_length']}")
        dev = input_ids.device
        x = ops.embedding(self.tok_emb.weight, input_ids.view(-1))
        dt = x.dtype
        cos, sin = self._rope_tables(dev)
        slots = metadata["slot_mapping"]
        for blk in self.trf_blocks:
            a = blk.att
            h, hk, dh = a.num_heads, a.num_kv_groups, a.head_dim
            kc, vc = kv_mgr.k_cache[a.layer_idx], kv_mgr.v_cache[a.layer_idx]
            delta = layer_delta(metadata, a.layer_idx)      # a step with adapted rows: the LoRA delta behind each GEMM
            n = blk.norm1(x)
            qkv = ops.linear(n, a._packed_qkv(dt))
            if delta is not None:
                delta("qkv", qkv, n)
            sc = page_scales(kv_mgr, a.layer_idx)      # fp8 pages: their scales; else nothing
            if a.q_norm is not None:
                if a.q_norm.eps != a.k_norm.eps:
                    raise ValueError("q_norm and k_norm share one eps in vy_paged_qknorm_rope_write")
                ops.paged_qknorm_rope_write_(qkv, positions, slots, cos, sin, _shadow(a.q_norm.scale, torch.float32),
                                             _shadow(a.k_norm.scale, torch.float32), a.q_norm.eps, h, kc, vc,
                                             k_page_scale=sc.get("k_scale"), v_page_scale=sc.get("v_scale"))
            else:
                ops.paged_rope_write_(qkv, positions, slots, cos, sin, h, kc, vc, **sc)
            o = paged_step_attention(qkv, kc, vc, metadata, h, hk, dh, **sc)
            x = ops.linear(o, _shadow(a.out_proj.weight, dt), None, residual=x)
            if delta is not None:
                delta("o", x, o)
            x = blk.ff(blk.norm2(x), residual=x, delta=delta)
        return paged_step_logits(x, metadata["last_rows"], self.final_norm, self.out_head.weight)


_HF_LAYER = (
    ("att.W_query.weight", "self_attn.q_proj.weight"),
    ("att.W_key.weight", "self_attn.k_proj.weight"),
    ("att.W_value.weight", "self_attn.v_proj.weight"),
    ("att.out_proj.weight", "self_attn.o_proj.weight"),
    ("att.q_norm.scale", "self_attn.q_norm.weight"),
    ("att.k_norm.scale", "self_attn.k_norm.weight"),
    ("norm1.scale", "input_layernorm.weight"),
    ("ff.fc1.weight", "mlp.gate_proj.weight"),
    ("ff.fc2.weight", "mlp.up_proj.weight"),
    ("ff.fc3.weight", "mlp.down_proj.weight"),
    ("norm2.scale", "post_attention_layernorm.weight"),
)


def load_weights_into_qwen(model: Qwen3Model, param_config, params) -> None:
    """A Hugging Face Qwen3 checkpoint, as a dict name -> tensor (e.g. safetensors.torch.load_file of a local file),
    into `model`, by the notebook's name mapping: model.embed_tokens / model.layers.<l>.{self_attn.{q,k,v,o}_proj,
    self_attn.{q,k}_norm, input_layernorm, mlp.{gate,up,down}_proj, post_attention_layernorm} / model.norm / lm_head.
    Values are copied into the model's own parameters (their dtype and device stay).  Without "lm_head.weight" the head
    is tied to tok_emb.  A missing tensor is a KeyError, a shape mismatch a ValueError; both name the tensor."""
    def assign(param, name):
        src = params[name]
        if tuple(param.shape) != tuple(src.shape):
            raise ValueError(f"Shape mismatch in tensor '{name}'. Left: {tuple(param.shape)}, Right: {tuple(src.shape)}")
        with torch.no_grad():
            param.copy_(torch.as_tensor(src).to(device=param.device, dtype=param.dtype))

    assign(model.tok_emb.weight, "model.embed_tokens.weight")
    for l, blk in enumerate(model.trf_blocks[:param_config["n_layers"]]):
        own = dict(blk.named_parameters())
        for mine, theirs in _HF_LAYER:
            if mine in own:                      # (q_norm / k_norm exist only with qk_norm)
                assign(own[mine], f"model.layers.{l}.{theirs}")
    assign(model.final_norm.scale, "model.norm.weight")
    if params.get("lm_head.weight") is None:
        model.tie_head()
        return
    if model.out_head.weight is model.tok_emb.weight:         # a head tied earlier gets a matrix of its own back
        model.out_head.weight = nn.Parameter(torch.empty_like(model.tok_emb.weight))
    assign(model.out_head.weight, "lm_head.weight")
