"""The reference's modern decoder (VyomAI/models/custom_transformer.py) on the HIP kernels: a Qwen2 / Llama-shaped
stack -- pre-norm RMSNorm, grouped-query attention with rotate-half RoPE (theta 1e6), biased q/k/v and a bias-free
o_proj, a bias-free gated MLP down(act(gate(x)) * up(x)), LM head tied to the embedding table.  Class names, constructor
signatures, attribute and parameter names are the reference's; `transformers` is not imported (Config is a plain
class, outputs are a small object, generation is this package's greedy loop).

Training: each half of a layer is ONE autograd function (autograd_train.PreNormAttentionFn / PreNormGatedMlpFn) whose
residual gradient rides in the RMSNorm backward's store; `clm_loss` fuses the final norm, the tied vocabulary GEMM and
the cross-entropy (TiedLMHeadLossFn) and never keeps the logits.  Inference: the static KV cache of layers/kv_cache.py,
single-token steps through vy_attn_decode."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from .._lib import VyomHipError
from ..adapters import DoraLinear, LoraLinear, layer_delta
from ..autograd import _mask_args, _wants_grad, gated_mlp
from ..layers.attention import _SelfAttentionBase, _shadow
from ..layers.ffn import _FUSED_ACT
from ..layers.kv_cache import DynamicCacheOne, StaticCacheOne
from ..layers.mask import AttnMask
from ..layers.paged import page_scales, paged_step_attention, paged_step_logits
from ..layers.positional_embeddings import RopeSlice, RopeTable, resolve_freqs
from .common import PositionMixin, SequenceScoreMixin


class Config:
    """The reference's Config (:17-73) without PretrainedConfig: same fields, same defaults."""

    keys_to_ignore_at_inference = ["past_key_values"]

    def __init__(self, vocab_size=32000, hidden_size=896, intermediate_size=4864, num_hidden_layers=4,
                 num_attention_heads=4, num_key_value_heads=2, hidden_act="silu", max_position_embeddings=32768,
                 initializer_range=0.02, rms_norm_eps=1e-6, use_cache=True, pad_token_id=0, eos_token_id=1,
                 bos_token_id=2, tie_word_embeddings=True, rope_theta=1000000.0, rope_scaling=None,
                 use_sliding_window=False, sliding_window=32768, max_window_layers=24, attention_dropout=0.0,
                 **kwargs):
        self.pad_token_id, self.bos_token_id, self.eos_token_id = pad_token_id, bos_token_id, eos_token_id
        self.tie_word_embeddings = tie_word_embeddings
        self.vocab_size = vocab_size
        self.max_position_embeddings = max_position_embeddings
        self.hidden_size = hidden_size
        self.intermediate_size = intermediate_size
        self.num_hidden_layers = num_hidden_layers
        self.num_attention_heads = num_attention_heads
        self.use_sliding_window = use_sliding_window
        self.sliding_window = sliding_window
        self.max_window_layers = max_window_layers
        if num_key_value_heads is None:
            num_key_value_heads = num_attention_heads
        self.num_key_value_heads = num_key_value_heads
        self.hidden_act = hidden_act
        self.initializer_range = initializer_range
        self.rms_norm_eps = rms_norm_eps
        self.use_cache = use_cache
        self.rope_theta = rope_theta
        self.rope_scaling = rope_scaling
        self.attention_dropout = attention_dropout
        for k, v in kwargs.items():
            setattr(self, k, v)


class CausalLMOutput:
    """What the reference returns as BaseModelOutputWithPast / CausalLMOutputWithPast."""

    def __init__(self, loss=None, logits=None, past_key_values=None, last_hidden_state=None):
        self.loss, self.logits = loss, logits
        self.past_key_values, self.last_hidden_state = past_key_values, last_hidden_state


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise VyomHipError(f"vyomai_amd ops run on MI355X only: {what} got a CPU tensor (no CPU fallback exists; move "
                           "the model and its inputs to 'cuda')")


class MLP(nn.Module):
    """down_proj(act_fn(gate_proj(x)) * up_proj(x)).  Reference :76-89."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.hidden_size = config.hidden_size
        self.intermediate_size = config.intermediate_size
        self.gate_proj = nn.Linear(self.hidden_size, self.intermediate_size, bias=False)
        self.up_proj = nn.Linear(self.hidden_size, self.intermediate_size, bias=False)
        self.down_proj = nn.Linear(self.intermediate_size, self.hidden_size, bias=False)
        if config.hidden_act not in _FUSED_ACT:
            raise ValueError(f"hidden_act {config.hidden_act!r} has no HIP kernel (known: {sorted(_FUSED_ACT)})")
        self.act = _FUSED_ACT[config.hidden_act]

    def _packed_gate_up(self, dtype: torch.dtype) -> torch.Tensor:
        """[Wgate; Wup] ([2 I, d]) in the compute dtype for the one packed GEMM: a view when the two copies sit back to
        back (the trainer's arenas lay them out so), else a concatenation cached per parameter version and weight epoch
        (the fused AdamW kernel rewrites the arena copies without touching tensor versions)."""
        from ..autograd_train import WEIGHT_EPOCH
        g = _shadow(self.gate_proj.weight, dtype).detach()
        u = _shadow(self.up_proj.weight, dtype).detach()
        I, d = g.shape
        if g.is_contiguous() and u.is_contiguous() and u.data_ptr() == g.data_ptr() + g.numel() * g.element_size() \
                and u.untyped_storage().data_ptr() == g.untyped_storage().data_ptr():   # one buffer, not two neighbours
            return torch.as_strided(g, (2 * I, d), (d, 1))
        key = (self.gate_proj.weight._version, self.up_proj.weight._version, WEIGHT_EPOCH[0], g.data_ptr(), u.data_ptr(),
               dtype)
        hit = getattr(self, "_gu", None)
        if hit is None or hit[0] != key:
            hit = self._gu = (key, torch.cat([g, u], dim=0).contiguous())
        return hit[1]

    def forward(self, x, residual: Optional[torch.Tensor] = None, delta=None):
        """delta (serving with adapters, adapters.layer_delta): f(group, y, x), called behind each of the two GEMMs."""
        _need_gpu(x, "MLP")
        if any(isinstance(p, LoraLinear) and p.enabled for p in (self.gate_proj, self.up_proj, self.down_proj)):
            raise VyomHipError("the gated MLP applies LoRA adapters (LoraLinear) inside its pre-norm block (DecoderLayer) "
                               "only; called on its own it would skip their term")
        if any(isinstance(p, DoraLinear) and p.enabled for p in (self.gate_proj, self.up_proj, self.down_proj)):
            raise VyomHipError("the gated MLP runs on DoRA's composed weights (DoraLinear) inside its pre-norm block "
                               "(DecoderLayer) only; called on its own it would compute the base model")
        if _wants_grad(x, self.gate_proj.weight, self.up_proj.weight, self.down_proj.weight):
            raise VyomHipError("the gated MLP trains inside its pre-norm block (DecoderLayer: RMSNorm, MLP and the "
                               "residual add are one autograd function); call it under torch.no_grad() on its own")
        return gated_mlp(x, self, self.act, _shadow(self.down_proj.weight, x.dtype), residual, delta)[0]


class Attention(_SelfAttentionBase):
    """q/k/v projections with bias, o_proj without (reference :164-223).  The forward lives in DecoderLayer: the
    RMSNorm in front and the residual add behind belong to the same fused group.  `query` / `key` / `value` alias the
    reference-named projections for the packed-QKV machinery shared with the other attention modules."""

    _lora_aware = True       # DecoderLayer adds a wrapped projection's low-rank term (lora_train.py)

    def __init__(self, config: Config, layer_idx: int):
        super().__init__()
        self.config = config
        self.layer_idx = layer_idx
        self.head_dim = getattr(config, "head_dim", config.hidden_size // config.num_attention_heads)
        if self.head_dim % 8 or self.head_dim > 256:
            raise ValueError(f"head_dim {self.head_dim} must be a multiple of 8 up to 256")
        self.num_attention_heads = config.num_attention_heads
        self.num_key_value_heads = config.num_key_value_heads
        if self.num_attention_heads % self.num_key_value_heads:
            raise ValueError(f"num_attention_heads {self.num_attention_heads} must be a multiple of "
                             f"num_key_value_heads {self.num_key_value_heads}")
        self.num_key_value_groups = config.num_attention_heads // config.num_key_value_heads
        self.scaling = self.head_dim ** -0.5
        self.attention_dropout = config.attention_dropout
        self.is_causal = True
        self.attention_bias = True
        self._fused_qkv = False
        self.q_proj = nn.Linear(config.hidden_size, config.num_attention_heads * self.head_dim, bias=True)
        self.k_proj = nn.Linear(config.hidden_size, config.num_key_value_heads * self.head_dim, bias=True)
        self.v_proj = nn.Linear(config.hidden_size, config.num_key_value_heads * self.head_dim, bias=True)
        self.o_proj = nn.Linear(config.num_attention_heads * self.head_dim, config.hidden_size, bias=False)

    query = property(lambda self: self.q_proj)
    key = property(lambda self: self.k_proj)
    value = property(lambda self: self.v_proj)


class RMSNorm(nn.Module):
    """weight * x * rsqrt(mean x^2 + eps), statistics in fp32.  Reference :227-244."""

    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, hidden_states):
        _need_gpu(hidden_states, "RMSNorm")
        if _wants_grad(hidden_states, self.weight):
            from ..autograd_train import RMSNormFn
            return RMSNormFn.apply(hidden_states, self.weight, self.variance_epsilon)
        return ops.rmsnorm(hidden_states, _shadow(self.weight, hidden_states.dtype), self.variance_epsilon, 0.0)

    def extra_repr(self):
        return f"{tuple(self.weight.shape)}, eps={self.variance_epsilon}"


class DecoderLayer(nn.Module):
    """x = x + o_proj(attn(RMSNorm(x))); x = x + mlp(RMSNorm(x)).  Reference :247-293.

    attention_mask: AttnMask descriptor, or the reference's 4-D additive tensor (inference only).
    position_embeddings: a RopeSlice (table + first position) instead of the reference's (cos, sin) pair.
    past_key_value: a whole-model cache of layers/kv_cache.py; cache_position: slot of the first token (int)."""

    def __init__(self, config: Config, layer_idx: int):
        super().__init__()
        self.hidden_size = config.hidden_size
        self.self_attn = Attention(config=config, layer_idx=layer_idx)
        self.mlp = MLP(config)
        self.input_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None,
                use_cache: Optional[bool] = False, cache_position=None, position_embeddings=None, **kwargs):
        _need_gpu(hidden_states, "DecoderLayer")
        a, m = self.self_attn, self.mlp
        x = hidden_states
        ln1, ln2 = self.input_layernorm, self.post_attention_layernorm
        from .. import lora_train
        if lora_train.layer_has_lora(self):
            # (training, and validation under no_grad: the adapter's delta behind each of the four GEMMs)
            return (lora_train.decoder_layer_forward(self, x, attention_mask, position_embeddings, past_key_value),)
        from .. import dora_train
        if dora_train.layer_has_dora(self):
            # (the plain block bodies on the composed weights; the adapter's own arithmetic is weight-sized)
            return (dora_train.decoder_layer_forward(self, x, attention_mask, position_embeddings, past_key_value),)
        if _wants_grad(x, a.o_proj.weight, m.down_proj.weight, ln1.weight):
            if past_key_value is not None:
                raise VyomHipError("KV caching is an inference feature; call under torch.no_grad()")
            from ..autograd_train import PreNormAttentionFn, PreNormGatedMlpFn
            x = PreNormAttentionFn.apply(x, a, attention_mask, position_embeddings, ln1.weight, ln1.variance_epsilon,
                                         a.o_proj.weight, *a._params())
            x = PreNormGatedMlpFn.apply(x, m, ln2.weight, ln2.variance_epsilon, m.act, m.gate_proj.weight,
                                        m.up_proj.weight, m.down_proj.weight)
            return (x,)
        B, L, _ = x.shape
        h, hk, dh = a.num_attention_heads, a.num_key_value_heads, a.head_dim
        dt, dev = x.dtype, x.device
        start = int(cache_position) if cache_position is not None else 0
        n = ln1(x)
        cos, sin, pos0 = resolve_freqs(position_embeddings, dev)
        q = torch.empty((B, h, L, dh), dtype=dt, device=dev)
        if past_key_value is not None:
            kw, vw = past_key_value.reserve(a.layer_idx, B, hk, L, dh, start, dt, dev)
        else:
            kw = torch.empty((B, hk, L, dh), dtype=dt, device=dev)
            vw = torch.empty_like(kw)
        sw, sb = a._packed_shadow(dt)
        ops.qkv_rope(n, sw, sb, h, hk, dh, cos, sin, pos0, q, kw, vw)
        k_all, v_all = past_key_value.commit(a.layer_idx) if past_key_value is not None else (kw, vw)
        S = k_all.shape[2]
        if L == 1 and attention_mask is None:
            o = ops.attention_decode(q, k_all, v_all, S)
        else:
            o = ops.attention(q, k_all, v_all, **_mask_args(attention_mask, B, L, S, dev))
        x = ops.linear(o, _shadow(a.o_proj.weight, dt), None, residual=x)
        return (m(ln2(x), residual=x),)


class BaseModel(nn.Module, PositionMixin):
    """Embedding, the layers and the final RMSNorm.  Reference :387-600 (the 4-D mask helpers are replaced by the mask
    descriptor: a 2-D padding mask becomes causal + key-padding AttnMask; a 4-D additive mask is passed through)."""

    def __init__(self, config: Config):
        super().__init__()
        self.padding_idx = getattr(config, "pad_token_id", 2)
        self.vocab_size = config.vocab_size
        self.config = config
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size, self.padding_idx)
        self.layers = nn.ModuleList([DecoderLayer(config, i) for i in range(config.num_hidden_layers)])
        self.norm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self._rope: Optional[RopeTable] = None
        self.apply(self._init_weights)

    def _init_weights(self, module):
        std = getattr(self.config, "initializer_range", 1e-6)
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=std)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(mean=0.0, std=std)
            if module.padding_idx is not None:
                module.weight.data[module.padding_idx].zero_()
        elif isinstance(module, RMSNorm):
            module.weight.data.fill_(1.0)

    def get_input_embeddings(self):
        return self.embed_tokens

    def set_input_embeddings(self, value):
        self.embed_tokens = value

    def _rope_slice(self, start: int, length: int) -> RopeSlice:
        """cos / sin for the positions in use (the reference's RotaryEmbedding, :337-363, evaluates its angles per
        forward): the table covers the next power of two, at least 256 positions, and grows on demand."""
        need = start + length
        if need > self.config.max_position_embeddings:
            raise ValueError(f"position {need} exceeds max_position_embeddings {self.config.max_position_embeddings}")
        if self._rope is None or self._rope.angles.shape[0] < need:
            n = 256
            while n < need:
                n *= 2
            n = min(n, self.config.max_position_embeddings)
            a = self.layers[0].self_attn
            inv = 1.0 / (self.config.rope_theta ** (torch.arange(0, a.head_dim, 2, dtype=torch.int64).float() / a.head_dim))
            self._rope = RopeTable(torch.outer(torch.arange(n).float(), inv))
        return RopeSlice(self._rope, start, length)

    def forward_hidden(self, input_ids=None, attention_mask=None, past_key_values=None, inputs_embeds=None,
                       use_cache=False, cache_position=None):
        """The trunk without the final norm -> (hidden, cache)."""
        if (input_ids is None) ^ (inputs_embeds is not None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        _need_gpu(input_ids if input_ids is not None else inputs_embeds, "BaseModel")
        x = self._embed(self.embed_tokens, input_ids) if inputs_embeds is None else self._cast(inputs_embeds)
        B, L, _ = x.shape
        train = _wants_grad(x, self.norm.weight, self.embed_tokens.weight)
        from .. import lora_train
        layers = self.layers[: self.config.num_hidden_layers]
        # (a cached step -- the decode loop -- does not ask: a wrapped layer refuses its past_key_value itself)
        from .. import dora_train
        lora = past_key_values is None and any(lora_train.layer_has_lora(layer) or dora_train.layer_has_dora(layer)
                                               for layer in layers)
        train = train or (lora and _wants_grad(*(p for layer in layers for p in lora_train.layer_lora_params(layer)
                                                 + dora_train.layer_dora_params(layer))))
        if train and past_key_values is not None:
            raise VyomHipError("KV caching is an inference feature; call under torch.no_grad()")
        cache = None
        if use_cache and not train and not lora:   # (adapters have no cached path: a wrapped model never starts a cache)
            cache = past_key_values if past_key_values is not None else DynamicCacheOne(self.config)
        if cache_position is not None:
            start = int(cache_position[0]) if torch.is_tensor(cache_position) else int(cache_position)
        else:
            start = int(getattr(cache, "_tokens_seen", 0)) if cache is not None else 0
        mask = None
        if attention_mask is not None and attention_mask.dim() == 4:
            if train:
                raise VyomHipError("training needs a mask descriptor (pass the 2-D padding mask): dense additive masks "
                                   "have no backward kernel")
            mask = attention_mask
        elif attention_mask is not None:
            mask = AttnMask.from_padding(attention_mask, causal=True, start_pos=start, query_len=L)
        elif L > 1:
            mask = AttnMask(causal=True, start_pos=start, query_len=L, key_len=start + L)
        freqs = self._rope_slice(start, L)
        for layer in self.layers[: self.config.num_hidden_layers]:
            x = layer(x, attention_mask=mask, past_key_value=cache, use_cache=cache is not None,
                      cache_position=start, position_embeddings=freqs)[0]
        if cache is not None:
            cache._tokens_seen = start + L
        return x, cache

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, use_cache=None, cache_position=None, **kwargs) -> CausalLMOutput:
        use_cache = use_cache if use_cache is not None else self.config.use_cache
        x, cache = self.forward_hidden(input_ids, attention_mask, past_key_values, inputs_embeds, use_cache,
                                       cache_position)
        return CausalLMOutput(last_hidden_state=self.norm(x), past_key_values=cache)


class ModelForCausalLM(nn.Module, SequenceScoreMixin):
    """BaseModel + the tied LM head.  Reference :606-747.

    The reference class inherits BaseModel and therefore also allocates a second trunk at the top level
    (embed_tokens.*, layers.*, norm.weight) that takes no part in forward.  It is not allocated here:
    state_dict() holds model.* and lm_head.weight, and load_state_dict() drops exactly the dead trunk's keys, so a
    reference checkpoint loads under strict=True."""

    compute_dtype = None   # set by FlatTrainer (None = the parameters' dtype)

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.model = BaseModel(config)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.lm_head.weight = self.model.embed_tokens.weight

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def set_input_embeddings(self, value):
        self.model.embed_tokens = value

    def get_output_embeddings(self):
        return self.lm_head

    def set_output_embeddings(self, new_embeddings):
        self.lm_head = new_embeddings

    def set_decoder(self, decoder):
        self.model = decoder

    def get_decoder(self):
        return self.model

    def dead_trunk_keys(self):
        """The state_dict keys of the reference's unused top-level trunk."""
        return {k[len("model."):] for k in self.state_dict() if k.startswith("model.")}

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        dead = self.dead_trunk_keys()
        kept = {k: v for k, v in state_dict.items() if k not in dead}
        return super().load_state_dict(kept, strict=strict, assign=assign)

    def _table_pending(self, input_ids) -> bool:
        """Does this graph's backward also scatter embedding gradients into the tied table?"""
        w = self.model.embed_tokens.weight
        return input_ids is not None and torch.is_grad_enabled() and w.requires_grad

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, labels=None, use_cache=None, cache_position=None, **kwargs) -> CausalLMOutput:
        out = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                         past_key_values=past_key_values, inputs_embeds=inputs_embeds, use_cache=use_cache,
                         cache_position=cache_position)
        hidden = out.last_hidden_state
        table = self.lm_head.weight
        if _wants_grad(hidden, table):
            from ..autograd_train import TiedLMHeadFn
            logits = TiedLMHeadFn.apply(hidden, table, self._table_pending(input_ids))
        else:
            logits = ops.linear(hidden, _shadow(table, hidden.dtype))
        loss = None
        if labels is not None:
            # (the logits are materialised, as in the reference; clm_loss is the path that never keeps them)
            from ..autograd_train import ShiftedXentFn
            loss = ShiftedXentFn.apply(logits, labels.to(logits.device), -100)
        return CausalLMOutput(loss=loss, logits=logits, past_key_values=out.past_key_values, last_hidden_state=hidden)

    def clm_loss(self, input_ids: torch.Tensor, labels: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                 ignore_index: int = -100) -> torch.Tensor:
        """Shifted next-token loss with the final RMSNorm, the tied vocabulary GEMM and the cross-entropy fused: the
        logits are reduced and overwritten by their gradient in place, never copied or up-cast."""
        from ..autograd_train import TiedLMHeadLossFn
        hidden, _ = self.model.forward_hidden(input_ids, attention_mask)
        norm = self.model.norm
        return TiedLMHeadLossFn.apply(hidden, labels, ignore_index, norm.weight, norm.variance_epsilon,
                                      self.lm_head.weight, self._table_pending(input_ids), self._label_flag(hidden.device))

    # sequence_logprobs / dpo_loss / _label_flag: common.SequenceScoreMixin over these two
    def _score_trunk(self, input_ids, attention_mask, inputs_embeds=None):
        if inputs_embeds is None:
            return self.model.forward_hidden(input_ids, attention_mask)[0]
        return self.model.forward_hidden(None, attention_mask, inputs_embeds=inputs_embeds)[0]

    def _score_head(self):
        return self.model.norm.weight, self.model.norm.variance_epsilon, self.lm_head.weight

    @torch.no_grad()
    def forward_paged(self, input_ids: torch.Tensor, positions: torch.Tensor, metadata: dict, kv_mgr) -> torch.Tensor:
        """One step of the continuous-batching engine (serving.ContinuousBatchEngine) -> logits (sequences, vocab) of
        the LAST row of each sequence.  input_ids (T,) are the step's packed tokens -- every unseen prompt token of a
        prefilling sequence, one token of a decoding one -- positions (T,) int32 their positions, `metadata` what
        ContinuousBatchEngine._plan_step built, kv_mgr the PagedKVManager whose pages are read and written.

        Per layer: input_layernorm, the packed QKV projection, vy_paged_rope_write (per-token RoPE in place + the K/V
        rows into their slots), attention -- vy_attn_paged_decode for the rows with one query token, causal vy_attn_fwd
        per prefilling sequence (straight on its slice of the packed buffer, or with start_pos = prefix_len against its
        gathered pages when it starts from cached prefix blocks), or, when the engine runs with varlen_prefill
        (metadata["prefill_varlen"]), ONE vy_attn_paged_prefill launch for every prefill row of the step, read through
        the block tables: no gather, no loop, and a segment may be a chunk in the middle of its prompt -- o_proj with the
        residual, post_attention_layernorm and the MLP as in DecoderLayer.forward.  Every token attends to its
        sequence's whole cached context, also in a step that mixes the two phases.  The final norm and the tied head
        see one row per sequence (the notebook of Examples/simple_vllm.ipynb projects all T rows and then indexes)."""
        base = self.model
        from .. import lora_train
        if any(lora_train.layer_has_lora(layer) for layer in base.layers[: self.config.num_hidden_layers]):
            raise VyomHipError(lora_train.NO_CACHE.format(what="forward_paged() (the serving engine)"))
        from .. import dora_train
        if any(dora_train.layer_has_dora(layer) for layer in base.layers[: self.config.num_hidden_layers]):
            raise VyomHipError(dora_train.NO_CACHE.format(what="forward_paged() (the serving engine)"))
        _need_gpu(input_ids, "forward_paged()")
        dev = input_ids.device
        x = base._embed(base.embed_tokens, input_ids.view(1, -1))[0]
        dt = x.dtype
        cos, sin = base._rope_slice(0, int(metadata["max_position"])).table.on(dev)
        slots = metadata["slot_mapping"]
        for layer in base.layers[: self.config.num_hidden_layers]:
            a = layer.self_attn
            h, hk, dh = a.num_attention_heads, a.num_key_value_heads, a.head_dim
            kc, vc = kv_mgr.k_cache[a.layer_idx], kv_mgr.v_cache[a.layer_idx]
            sw, sb = a._packed_shadow(dt)
            delta = layer_delta(metadata, a.layer_idx)      # a step with adapted rows: the LoRA delta behind each GEMM
            n = layer.input_layernorm(x)
            qkv = ops.linear(n, sw, sb)
            if delta is not None:
                delta("qkv", qkv, n)
            sc = page_scales(kv_mgr, a.layer_idx)      # fp8 pages: their scales; else nothing
            ops.paged_rope_write_(qkv, positions, slots, cos, sin, h, kc, vc, **sc)
            o = paged_step_attention(qkv, kc, vc, metadata, h, hk, dh, **sc)
            x = ops.linear(o, _shadow(a.o_proj.weight, dt), None, residual=x)
            if delta is not None:
                delta("o", x, o)
            x = layer.mlp(layer.post_attention_layernorm(x), residual=x, delta=delta)
        return paged_step_logits(x, metadata["last_rows"], base.norm, self.lm_head.weight)

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                 max_new_tokens: int = 20, eos_token_id=None) -> torch.Tensor:
        """Greedy decoding -> (B, prompt + max_new_tokens) ids.  The prompt (left-padded when attention_mask says so) is
        prefilled into a static KV cache, every further token is one single-token pass (vy_attn_decode when nothing is
        padded) and one vy_greedy_step.  Rows that have produced eos_token_id continue with pad_token_id.  (The
        reference inherits transformers' GenerationMixin; sampling, beams and stopping criteria are not reproduced.)"""
        from .. import lora_train
        if any(lora_train.layer_has_lora(layer) for layer in self.model.layers[: self.config.num_hidden_layers]):
            raise VyomHipError(lora_train.NO_CACHE.format(what="generate() (it decodes through a KV cache)"))
        from .. import dora_train
        if any(dora_train.layer_has_dora(layer) for layer in self.model.layers[: self.config.num_hidden_layers]):
            raise VyomHipError(dora_train.NO_CACHE.format(what="generate() (it decodes through a KV cache)"))
        _need_gpu(input_ids, "generate()")
        dev = input_ids.device
        B, T = input_ids.shape
        total = T + max_new_tokens
        dt = self.model.compute_dtype or self.lm_head.weight.dtype
        cache = StaticCacheOne(self.config, max_cache_len=total, dtype=dt, batch_size=B)
        pad = self.config.pad_token_id if self.config.pad_token_id is not None else 0
        tokens = torch.full((B, total), pad, dtype=torch.long, device=dev)
        tokens[:, :T] = input_ids
        if eos_token_id is None:
            eos = [-1]
        else:
            eos = list(eos_token_id) if isinstance(eos_token_id, (list, tuple)) else [int(eos_token_id)]
        eos_ids = torch.tensor(eos, dtype=torch.long, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        # a finished row keeps emitting pad_token_id: the step kernel's prompt mask forces the (pad) token already there
        forced = torch.zeros((B, total), dtype=torch.bool, device=dev) if eos_token_id is not None else None
        mask = None
        if attention_mask is not None:
            mask = torch.ones((B, total), dtype=attention_mask.dtype, device=dev)
            mask[:, :T] = attention_mask
        prev = 0
        for cur in range(T, total):
            out = self.model(input_ids=tokens[:, prev:cur], attention_mask=None if mask is None else mask[:, :cur],
                             past_key_values=cache, use_cache=True, cache_position=prev)
            last = out.last_hidden_state[:, -1:, :].contiguous()
            logits = ops.linear(last, _shadow(self.lm_head.weight, last.dtype))[:, -1]
            if forced is not None:
                forced[:, cur] = done
            ops.greedy_step_(logits, tokens, cur, forced, eos_ids, done)
            prev = cur
            if eos_token_id is not None and (cur - T) % 16 == 15 and bool(done.all()):
                break
        return tokens
