"""BERT-style encoder with the reference's API (VyomAI/models/encoder.py)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from ..layers.attention import EncoderAttention, EncoderAttentionGqa
from ..layers.ffn import FeedForward
from ..layers.mask import AttnMask
from ..autograd_train import defer_residual_grads as _defer
from .common import LMHead, PositionMixin


@dataclass
class EncoderOutput(object):
    logits: torch.Tensor  # holds the last hidden state, as in the reference (:168)


@dataclass
class MLMOutput(object):
    hidden_state: torch.Tensor
    logits: torch.Tensor


class EncoderLayer(nn.Module):
    """attention -> feed_forward(out, layer_input).  Reference :30-64."""

    def __init__(self, config, layer_idx: int, attention_type: str = None) -> None:
        super().__init__()
        self.attention = (EncoderAttentionGqa(config, layer_idx=layer_idx) if attention_type == "gqa"
                          else EncoderAttention(config, layer_idx=layer_idx))
        if attention_type == "gqa" and layer_idx == 0:
            print("Encoder Using GQA Attention")
        self.feed_forward = FeedForward(config)
        self.layer_idx = layer_idx

    def forward(self, hidden_state, attention_mask, freqs=None) -> torch.Tensor:
        _defer(hidden_state)  # training: its residual-path gradients are added in the QKV dgrad epilogue
        from .. import encoder_lora_train
        if encoder_lora_train.layer_has_lora(self):
            # (training, and validation under no_grad: the adapter's term in front of each GEMM's epilogue)
            return encoder_lora_train.encoder_layer_forward(self, hidden_state, attention_mask, freqs)
        out = self.attention(hidden_state=hidden_state, attention_mask=attention_mask, freqs=freqs)
        return self.feed_forward(out, hidden_state)


class EncoderModel(nn.Module, PositionMixin):
    """Reference :92-177.  forward(input_ids, attention_mask) -> EncoderOutput(hidden states)."""

    def __init__(self, config, pos_embedding_type: Optional[str] = "absolute", attention_type: str = None) -> None:
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size,
                                            padding_idx=getattr(config, "pad_token_id", None))
        self._init_positions(config, pos_embedding_type, "Encoder")
        self.all_layer = nn.ModuleList(
            [EncoderLayer(config, i, attention_type) for i in range(config.num_hidden_layers)])

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> EncoderOutput:
        _, seqlen = input_ids.shape
        hidden_state = self._embed(self.word_embeddings, input_ids)
        hidden_state, freqs = self._positions(hidden_state, 0, seqlen)
        # the reference builds (1-mask)*finfo.min of shape (B,1,1,L) (:161-164); same information
        # as a key-padding descriptor
        mask = AttnMask.from_padding(attention_mask, causal=False, start_pos=0, query_len=seqlen)
        if mask.keypad is None:
            mask = None
        for layer in self.all_layer:
            hidden_state = layer(hidden_state, mask, freqs)
        return EncoderOutput(hidden_state)

    @classmethod
    def from_config(cls, config, pos_embedding_type: Optional[str] = "absolute", attention_type: str = None):
        return cls(config, pos_embedding_type, attention_type)


class EncoderForMaskedLM(nn.Module):
    """Reference :180-217."""

    def __init__(self, config, pos_embedding_type: Optional[str] = "absolute", attention_type: str = None) -> None:
        super().__init__()
        self.encoder = EncoderModel(config, pos_embedding_type=pos_embedding_type, attention_type=attention_type)
        self.lm_head = LMHead(config=config)

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> MLMOutput:
        out = self.encoder(input_ids=input_ids, attention_mask=attention_mask)
        return MLMOutput(hidden_state=out.logits, logits=self.lm_head(out.logits))

    def mlm_loss(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, labels: torch.Tensor,
                 ignore_index: int = -100) -> torch.Tensor:
        """Mean cross-entropy of position t against labels[t] over labels != ignore_index, the loss of
        Examples/masked_language_modeling.ipynb (nn.CrossEntropyLoss on logits.view(-1, V)), fused with the head."""
        out = self.encoder(input_ids=input_ids, attention_mask=attention_mask)
        return self.lm_head.loss(out.logits, labels, ignore_index=ignore_index, shift=False)

    @classmethod
    def from_config(cls, config, pos_embedding_type: Optional[str] = "absolute", attention_type: str = None):
        return cls(config, pos_embedding_type, attention_type)


class EncoderForSequenceClassification(nn.Module):
    """The classifier of Examples/adapters.ipynb and vyom-ai-classification.ipynb (ClinicModel): the encoder, then
    nn.Linear(hidden_size, num_labels) on the first token's hidden state.  `model` and `output` are the notebook's
    attribute names, so a ClinicModel state dict loads strictly.  Full fine-tuning, or adapters on the encoder:
    add_lora(m.model) freezes the encoder and keeps the head trainable."""

    def __init__(self, config, num_labels: int, pos_embedding_type: Optional[str] = "absolute",
                 attention_type: str = None) -> None:
        super().__init__()
        if int(num_labels) != num_labels or num_labels < 1:
            raise ValueError(f"num_labels {num_labels} must be a positive integer")
        if config.hidden_size % 8:
            raise ValueError(f"hidden_size {config.hidden_size} must be a multiple of 8 (vy_cls_head_fwd)")
        self.model = EncoderModel(config, pos_embedding_type=pos_embedding_type, attention_type=attention_type)
        self.output = nn.Linear(config.hidden_size, int(num_labels))
        self.num_labels = int(num_labels)

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """-> logits (B, num_labels), fp32: output(hidden[:, 0, :]) (vy_cls_head_fwd)."""
        from ..autograd_train import ClsHeadLogitsFn
        hidden = self.model(input_ids=input_ids, attention_mask=attention_mask).logits
        return ClsHeadLogitsFn.apply(hidden, self.output.weight, self.output.bias)

    def classification_loss(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, labels: torch.Tensor,
                            check_labels: bool = False) -> torch.Tensor:
        """Mean nn.CrossEntropyLoss of the logits against labels (B,), fused with the head: the training-side entry
        point, FlatTrainer(m).train_step(lambda: m.classification_loss(ids, mask, labels)).  A label outside
        [0, num_labels) is never dereferenced or clamped: its row counts as ignored and the device flag
        `self.label_error` is raised -- `check_labels=True` (or raise_on_label_error() whenever convenient: it
        synchronises) turns that into a ValueError."""
        from ..autograd_train import ClsHeadLossFn
        hidden = self.model(input_ids=input_ids, attention_mask=attention_mask).logits
        flag = getattr(self, "label_error", None)
        if flag is None or flag.device != hidden.device:
            flag = self.label_error = torch.zeros(1, dtype=torch.int32, device=hidden.device)
        loss = ClsHeadLossFn.apply(hidden, labels, self.output.weight, self.output.bias, flag)
        if check_labels:
            self.raise_on_label_error()
        return loss

    def raise_on_label_error(self) -> None:
        flag = getattr(self, "label_error", None)
        if flag is not None and int(flag.item()) != 0:
            flag.zero_()
            raise ValueError(f"labels contain ids outside [0, {self.num_labels}) (those rows were treated as ignored)")

    @classmethod
    def from_config(cls, config, num_labels: int, pos_embedding_type: Optional[str] = "absolute",
                    attention_type: str = None):
        return cls(config, num_labels, pos_embedding_type, attention_type)
