"""Pieces shared by the model files: LM head, position-embedding registry, RoPE window."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from .._lib import ACT_GELU_ERF
from ..layers.attention import _shadow
from ..layers.positional_embeddings import (AbsoluteEncoding, RopeSlice, RopeTable, RotaryEmbedding,
                                            SinusoidalEncoding)

POSITION_EMBEDDINGS = {"absolute": AbsoluteEncoding, "sinusoidal": SinusoidalEncoding}


class LMHead(nn.Module):
    """decoder(LN(gelu(dense(h)))) with the vocabulary bias tied to ``decoder.bias``
    (reference VyomAI/models/decoder.py:253-275, VyomAI/models/encoder.py:67-89).
    Two MFMA GEMM launches (GELU fused in the first) and one LayerNorm launch; the logits buffer
    has its row stride padded to 8 elements because vocab_size is odd."""

    def __init__(self, config) -> None:
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.layer_norm = nn.LayerNorm(config.hidden_size, eps=getattr(config, "layer_norm_eps", 1e-6))
        self.decoder = nn.Linear(config.hidden_size, config.vocab_size)
        self.bias = nn.Parameter(torch.zeros(config.vocab_size))
        self.decoder.bias = self.bias

    def forward(self, hidden_state: torch.Tensor) -> torch.Tensor:
        from ..autograd import _wants_grad
        if _wants_grad(hidden_state, self.dense.weight, self.decoder.weight):
            from ..autograd_train import LMHeadFn
            return LMHeadFn.apply(hidden_state, self.dense.weight, self.dense.bias, self.layer_norm.weight,
                                  self.layer_norm.bias, self.decoder.weight, self.bias, self.layer_norm.eps)
        dt = hidden_state.dtype
        x = ops.linear(hidden_state, _shadow(self.dense.weight, dt), _shadow(self.dense.bias, dt), act=ACT_GELU_ERF)
        x, _, _ = ops.layernorm(x, _shadow(self.layer_norm.weight, dt), _shadow(self.layer_norm.bias, dt),
                                self.layer_norm.eps)
        return ops.linear(x, _shadow(self.decoder.weight, dt), _shadow(self.bias, dt))


    def loss(self, hidden_state: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100,
             check_labels: bool = False, shift: bool = True) -> torch.Tensor:
        """Shifted CLM cross-entropy (shift=False: position t against label t, the masked-LM loss of
        Examples/masked_language_modeling.ipynb) fused with the head (no fp32 logits copy): the training-side
        entry point; see autograd_train.LMHeadLossFn.  A label that is neither `ignore_index` nor a
        vocabulary id (torch.cross_entropy device-asserts on it) is never dereferenced: its row counts as
        ignored and the device flag `self.label_error` is raised -- `check_labels=True` (or
        `raise_on_label_error()` whenever convenient: it synchronises) turns that into a ValueError."""
        out = self._loss(hidden_state, labels, ignore_index, shift, None)
        if check_labels:
            self.raise_on_label_error()
        return out

    def _loss(self, hidden_state, labels, ignore_index, shift, sample):
        from ..autograd_train import LMHeadLossFn
        flag = getattr(self, "label_error", None)
        if flag is None or flag.device != hidden_state.device:
            flag = self.label_error = torch.zeros(1, dtype=torch.int32, device=hidden_state.device)
        return LMHeadLossFn.apply(hidden_state, labels, ignore_index, self.dense.weight, self.dense.bias,
                                  self.layer_norm.weight, self.layer_norm.bias, self.decoder.weight, self.bias,
                                  self.layer_norm.eps, flag, shift, sample)

    def mlm_loss_and_sample(self, hidden_state: torch.Tensor, labels: torch.Tensor, temperature: float,
                            ignore_index: int = -100):
        """-> (masked-LM loss, sampled): the unshifted loss of `loss`, and in the same pass over the logits one
        token per labelled position drawn as argmax(logits / temperature + Gumbel noise) -- ELECTRA's replaced
        tokens (reference pretraining/collators.py:76-91) -- with -1 wherever the label is ignore_index.  `sampled`
        (labels' shape, int64) carries no gradient.  The logits are never read again."""
        from .. import rng
        return self._loss(hidden_state, labels, ignore_index, False, (1.0 / float(temperature), *rng.next_offset()))

    def raise_on_label_error(self) -> None:
        flag = getattr(self, "label_error", None)
        if flag is not None and int(flag.item()) != 0:
            flag.zero_()
            raise ValueError(f"labels contain ids outside [0, {self.decoder.weight.shape[0]}) other than "
                             "ignore_index (those rows were treated as ignored)")


class PositionMixin:
    """Builds position embeddings / the RoPE angle table exactly like the reference constructors
    (models/decoder.py:294-304) and serves per-forward windows."""

    def _init_positions(self, config, pos_embedding_type: Optional[str], who: str) -> None:
        cls = POSITION_EMBEDDINGS.get(pos_embedding_type, None)
        self.position_embeddings = cls(config) if cls is not None else None
        if pos_embedding_type == "rope":
            # plain tensor attribute, not a buffer, as in the reference (not in state_dict)
            self.emb_freq = RotaryEmbedding(config)(config.max_position_embeddings)
            self._rope_table = RopeTable(self.emb_freq)
            print(f"{who} Ignoring sinusoidal or absolute position embeddings because rope,is enable")

    # fp32 master weights with bf16 kernels: set by FlatTrainer (None = the parameters' dtype)
    compute_dtype = None

    def _embed(self, emb: nn.Embedding, input_ids: torch.Tensor) -> torch.Tensor:
        """Token embedding through vy_embedding_fwd/bwd (in the compute dtype when a trainer set one)."""
        w = emb.weight
        if not w.is_cuda:
            return emb(input_ids)  # host-side use only (state-dict tooling); kernels need the GPU
        from .. import ops
        from ..layers.attention import _shadow
        dt = self.compute_dtype or w.dtype
        if torch.is_grad_enabled() and w.requires_grad:
            from ..autograd_train import EmbeddingFn
            return EmbeddingFn.apply(input_ids, w, emb.padding_idx, dt)
        return ops.embedding(_shadow(w, dt), input_ids)

    def _cast(self, hidden_state: torch.Tensor) -> torch.Tensor:
        cd = self.compute_dtype
        return hidden_state if cd is None or hidden_state.dtype == cd else hidden_state.to(cd)

    def _positions(self, hidden_state: torch.Tensor, start_pos: int, seqlen: int):
        """-> (hidden_state [+ position info] in the compute dtype, freqs)."""
        if self.position_embeddings is not None:
            pos = self.position_embeddings(start_pos + seqlen)[:, start_pos:start_pos + seqlen, :]
            return self._cast(hidden_state + pos.to(device=hidden_state.device, dtype=hidden_state.dtype)), None
        hidden_state = self._cast(hidden_state)
        if start_pos + seqlen > self.emb_freq.shape[1]:
            raise ValueError(f"position {start_pos + seqlen} exceeds max_position_embeddings {self.emb_freq.shape[1]}")
        return hidden_state, RopeSlice(self._rope_table, start_pos, seqlen)


class SequenceScoreMixin:
    """Per-sequence log-probabilities and the DPO loss over a trunk + RMSNorm + vocabulary table, shared by
    ModelForCausalLM and Qwen3Model.  The model supplies `_score_trunk(input_ids, attention_mask, inputs_embeds)` -> the
    hidden state in front of the final norm, `_score_head()` -> (norm weight, eps, table) and
    `_table_pending(input_ids)`: does this graph's backward also scatter embedding gradients into that table?"""

    def _label_flag(self, dev) -> torch.Tensor:
        flag = getattr(self, "label_error", None)
        if flag is None or flag.device != dev:
            flag = self.label_error = torch.zeros(1, dtype=torch.int32, device=dev)
        return flag

    def sequence_logprobs(self, input_ids: torch.Tensor, selection_mask: torch.Tensor,
                          attention_mask: Optional[torch.Tensor] = None,
                          inputs_embeds: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Masked average log-probability of each sequence -> fp32 (B,): the notebook's
        compute_logprobs(model(input_ids).logits, input_ids, selection_mask)
        (Examples/vyom-ai-llm-sft-dpo-training.ipynb), with the final RMSNorm, the vocabulary GEMM and the
        log-softmax fused.  With grad the logits are overwritten in place by their unit gradient (TiedLMHeadLogprobFn);
        under torch.no_grad() they are only read (vy_logprob_fwd) and freed on return.  A sequence whose mask selects
        nothing scores 0.  `inputs_embeds` replaces the embedding lookup (input_ids still supply the labels)."""
        from ..autograd import _wants_grad
        from ..autograd_train import TiedLMHeadLogprobFn, logprob_rows, tied_head_logprobs
        from .._lib import VyomHipError
        if selection_mask.shape != input_ids.shape:
            raise ValueError(f"selection_mask {tuple(selection_mask.shape)} must match input_ids {tuple(input_ids.shape)}")
        if not input_ids.is_cuda:
            raise VyomHipError("vyomai_amd ops run on MI355X only: sequence_logprobs() got a CPU tensor (no CPU fallback "
                               "exists; move the model and its inputs to 'cuda')")
        hidden = self._score_trunk(input_ids, attention_mask, inputs_embeds)
        labels, w = logprob_rows(input_ids, selection_mask)
        ln_w, eps, table = self._score_head()
        flag = self._label_flag(hidden.device)
        if _wants_grad(hidden, ln_w, table):
            return TiedLMHeadLogprobFn.apply(hidden, labels, w, ln_w, eps, table,
                                             self._table_pending(None if inputs_embeds is not None else input_ids), flag)
        return tied_head_logprobs(hidden, labels, w, ln_w, eps, table, flag)[0]

    def dpo_loss(self, batch, ref_model=None, beta: float = 0.1, ref_logprobs=None):
        """Direct preference optimisation on one collated batch -> (loss, chosen_rewards, rejected_rewards): the
        notebook's compute_dpo_loss_batch (Examples/vyom-ai-llm-sft-dpo-training.ipynb).  `batch` is its dict: chosen,
        rejected (ids) and chosen_mask, rejected_mask, all (B, L) -- dpo_collate pads both sides to one length, so the
        two are scored as ONE 2B-row batch and this module runs once per graph.  The frozen model is `ref_model`,
        scored the same way under torch.no_grad(), or its precomputed scores `ref_logprobs = (chosen, rejected)`.
        loss = mean -logsigmoid(beta * ((pi_c - pi_r) - (ref_c - ref_r))); the rewards are detached means."""
        chosen, rejected = batch["chosen"], batch["rejected"]
        cmask, rmask = batch["chosen_mask"], batch["rejected_mask"]
        if chosen.shape != rejected.shape or cmask.shape != chosen.shape or rmask.shape != rejected.shape:
            raise ValueError(f"dpo_loss needs chosen {tuple(chosen.shape)}, rejected {tuple(rejected.shape)} and their "
                             f"masks {tuple(cmask.shape)}, {tuple(rmask.shape)} padded to one common length, as the "
                             "notebook's dpo_collate does")
        if (ref_model is None) == (ref_logprobs is None):
            raise ValueError("dpo_loss needs exactly one of ref_model and ref_logprobs=(chosen, rejected)")
        B = chosen.shape[0]
        ids = torch.cat([chosen, rejected], dim=0)
        mask = torch.cat([cmask, rmask], dim=0)
        if ref_logprobs is None:
            with torch.no_grad():   # scored first: its logits are gone before the policy's are allocated
                ref = ref_model.sequence_logprobs(ids, mask)
            ref_c, ref_r = ref[:B], ref[B:]
        else:
            ref_c, ref_r = (t.detach().to(device=ids.device, dtype=torch.float32) for t in ref_logprobs)
        pi = self.sequence_logprobs(ids, mask)
        pi_c, pi_r = pi[:B], pi[B:]
        losses = -torch.nn.functional.logsigmoid(beta * ((pi_c - pi_r) - (ref_c - ref_r)))
        return losses.mean(), (pi_c - ref_c).detach().mean(), (pi_r - ref_r).detach().mean()
