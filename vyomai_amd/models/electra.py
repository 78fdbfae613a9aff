"""ELECTRA pre-training of the encoder, with the names of Examples/electra-pretraining.ipynb (cells 21, 22, 27, 32):
Discriminator, ElectraModel, ElectraLoss.  Attribute names are the notebook's, so state dicts interchange."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ..pretraining.collators import masked_language_modeling
from .encoder import EncoderModel


class Discriminator(nn.Module):
    """EncoderModel(rope) + nn.Linear(hidden_size, 1): one replaced / original logit per token (cell 21)."""

    def __init__(self, config, pos_embedding_type: Optional[str] = "rope", attention_type: str = None) -> None:
        super().__init__()
        self.discriminator = EncoderModel(config, pos_embedding_type=pos_embedding_type, attention_type=attention_type)
        self.discriminator_head = nn.Linear(config.hidden_size, 1)

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """-> logits [B, L, 1] in the hidden state's dtype (vy_bce_head_fwd without a target; differentiable, so the
        notebook's own loop -- logits, ElectraLoss, backward -- trains).  `loss` fuses the head with its loss."""
        from ..autograd_train import BceHeadLogitsFn
        h = self.discriminator(input_ids=input_ids, attention_mask=attention_mask).logits
        z = BceHeadLogitsFn.apply(h, self.discriminator_head.weight, self.discriminator_head.bias)
        return z.to(h.dtype).unsqueeze(-1)

    def loss(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, disc_labels: torch.Tensor,
             live: torch.Tensor) -> torch.Tensor:
        """Mean binary_cross_entropy_with_logits over the tokens where `live` (cell 27), fused with the head."""
        from ..autograd_train import BceHeadLossFn
        h = self.discriminator(input_ids=input_ids, attention_mask=attention_mask).logits
        return BceHeadLossFn.apply(h, self.discriminator_head.weight, self.discriminator_head.bias, disc_labels, live)[0]


class ElectraModel(nn.Module):
    """Generator (EncoderForMaskedLM) and discriminator side by side (cell 22)."""

    def __init__(self, generator, discriminator) -> None:
        super().__init__()
        self.discriminator_model = discriminator
        self.generator_model = generator

    def get_generator_output(self, input_ids: torch.Tensor, attention_mask: torch.Tensor):
        """The generator's MaskedLMOutput (materialised logits)."""
        return self.generator_model(input_ids=input_ids, attention_mask=attention_mask)

    def get_discriminator_output(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """The discriminator's logits [B, L, 1]."""
        return self.discriminator_model(input_ids=input_ids, attention_mask=attention_mask)

    def tie_word_embeddings(self) -> None:
        """Both word_embeddings.weight become the generator's Parameter (cell 32).  Call before building a trainer."""
        self.discriminator_model.discriminator.word_embeddings.weight = \
            self.generator_model.encoder.word_embeddings.weight

    def electra_loss(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, tokenizer, fraction: float = 0.15,
                     temperature: float = 3, masked=None, sampled: Optional[torch.Tensor] = None,
                     ignore_index: int = -100) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One ELECTRA step's loss (the body of the notebook's training loop, cell 35) without materialised logits and
        without a host synchronisation: mask the inputs, generator trunk, masked-LM loss and replaced-token sampling
        in one pass over the generator logits, scatter the samples into the original ids, discriminator trunk, BCE
        head over the non-pad tokens.  -> (loss, generator_loss, discriminator_loss).  Nothing flows back from the
        discriminator into the generator: the samples are integers.
        masked = (masked_ids, labels, masked_indices) and sampled (the tokens for the masked positions, in order, or a
        full [B, L] tensor with -1 off the mask) inject a fixed draw; the compact form costs a synchronisation."""
        if masked is None:
            masked = masked_language_modeling(input_ids, tokenizer, fraction=fraction, ignore_index=ignore_index)
        masked_ids, labels, masked_indices = masked
        gen = self.generator_model
        hidden = gen.encoder(input_ids=masked_ids, attention_mask=attention_mask).logits
        if sampled is None:
            generator_loss, sampled = gen.lm_head.mlm_loss_and_sample(hidden, labels, temperature, ignore_index)
        else:
            generator_loss = gen.lm_head.loss(hidden, labels, ignore_index=ignore_index, shift=False)
            if sampled.shape != input_ids.shape:
                full = torch.full_like(input_ids, -1)
                full[masked_indices] = sampled.to(input_ids.device)
                sampled = full
        discriminator_input = torch.where(sampled >= 0, sampled, input_ids)
        disc_labels = (input_ids != discriminator_input).float()
        live = input_ids != tokenizer.pad_token_id
        discriminator_loss = self.discriminator_model.loss(discriminator_input, attention_mask, disc_labels, live)
        return generator_loss + discriminator_loss, generator_loss, discriminator_loss


class ElectraLoss:
    """The notebook's loss for users who already hold logits (cell 27): cross-entropy of the generator logits plus
    binary cross-entropy of the discriminator logits over the non-pad tokens.  The fused route is
    ElectraModel.electra_loss."""

    def __init__(self, config) -> None:
        self.config = config
        self.generator_loss = nn.CrossEntropyLoss()   # (the notebook's attribute; ignore_index = -100)

    def __call__(self, generator_logits, generator_label, disc_logits, disc_labels, non_padded_indices):
        F = nn.functional
        V = self.config.vocab_size
        mlm = F.cross_entropy(generator_logits.float().reshape(-1, V), generator_label.reshape(-1),
                              ignore_index=self.generator_loss.ignore_index)
        per_token = F.binary_cross_entropy_with_logits(disc_logits.float().reshape(disc_labels.shape), disc_labels,
                                                       reduction="none")
        rtd = per_token[non_padded_indices].mean()
        return mlm + rtd, mlm, rtd
