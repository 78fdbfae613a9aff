"""Masked-LM and ELECTRA batch corruption with the reference's names (VyomAI/pretraining/collators.py).

GPU tensors go through the kernels (vy_mlm_mask; the sampler is fused into the generator head's loss,
LMHead.mlm_loss_and_sample, and `sample` on its own is vy_xent_sample_fwd's argmax); CPU tensors -- the dataset-worker
case -- take plain torch statements of the same definitions.  `tokenizer` is duck-typed: get_special_tokens_mask,
all_special_ids, mask_token, convert_tokens_to_ids, pad_token_id, __len__."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
from torch.utils.data import Dataset

from .. import ops, rng


_SPECIAL_IDS = {}   # (the special ids, device) -> device list: one upload per tokenizer vocabulary and device


def _special_ids(tokenizer, device) -> torch.Tensor:
    """The tokenizer's special ids as a device list."""
    key = (tuple(sorted(set(int(i) for i in tokenizer.all_special_ids))), device)
    t = _SPECIAL_IDS.get(key)
    if t is None:
        t = _SPECIAL_IDS[key] = torch.tensor(key[0], dtype=torch.long, device=device)
    return t


def masked_language_modeling(input_ids: torch.Tensor, tokenizer, fraction: Optional[float] = 0.15,
                             ignore_index: Optional[int] = -100) -> Tuple[torch.Tensor]:
    """-> (input_ids with `fraction` of the non-special tokens corrupted, labels, masked_indices): of the selected
    tokens 80 % become the mask token, 10 % a uniform random id below len(tokenizer), 10 % stay (reference :9-62)."""
    mask_id = tokenizer.convert_tokens_to_ids(tokenizer.mask_token)
    if input_ids.is_cuda:
        seed, offset = rng.next_offset()
        return ops.mlm_mask(input_ids, _special_ids(tokenizer, input_ids.device), fraction, mask_id, len(tokenizer),
                            ignore_index, seed, offset)
    # the kernel's definition in torch statements: four uniforms per token decide select / mask / random / which id
    u = torch.rand((4, *input_ids.shape))
    special = torch.isin(input_ids, _special_ids(tokenizer, input_ids.device))
    masked_indices = ~special & (u[0] < fraction)
    to_mask = masked_indices & (u[1] < 0.8)
    to_random = masked_indices & ~to_mask & (u[2] < 0.5)
    words = (u[3] * len(tokenizer)).long().clamp_(max=len(tokenizer) - 1)
    out = torch.where(to_mask, torch.full_like(input_ids, mask_id), torch.where(to_random, words, input_ids))
    label = torch.where(masked_indices, input_ids, torch.full_like(input_ids, ignore_index))
    return out, label, masked_indices


def log(t, eps=1e-9) -> torch.Tensor:
    """ln(t + eps): finite at t = 0 (reference :65-67)."""
    return torch.add(t, eps).log()


def noise(t) -> torch.Tensor:
    """Gumbel noise of t's shape (reference :70-73).  On the GPU: the counter-based noise of vy_gumbel_noise (fp32
    arithmetic, cast to t's dtype), the function the fused sampler adds."""
    if t.is_cuda:
        seed, offset = rng.next_offset()
        V = t.shape[-1]
        return ops.gumbel_noise(t.numel() // V, V, seed, offset, t.device).view(t.shape).to(t.dtype)
    u = torch.rand(t.shape, dtype=t.dtype if t.is_floating_point() else torch.float32, device=t.device)
    return log(log(u).neg()).neg()


def sample(t, temperature=1.0) -> torch.Tensor:
    """argmax(t / temperature + noise) over the last dimension (reference :76-78).  On the GPU one launch reads t
    once (vy_xent_sample_fwd with every row live); the scores are fp32 whatever t's dtype."""
    if t.is_cuda and t.dtype in (torch.bfloat16, torch.float32) and t.numel():
        from ..autograd_train import _rehome, _row_stride
        V = t.shape[-1]
        buf = _rehome(t.detach().reshape(-1, V), _row_stride(V), t.dtype)
        M = buf.shape[0]
        seed, offset = rng.next_offset()
        sampled = torch.empty(M, dtype=torch.long, device=t.device)
        scratch = torch.zeros(M + 2, dtype=torch.float32, device=t.device)
        ops.xent_sample_fwd(buf[:, :V], torch.zeros(M, dtype=torch.long, device=t.device), -100, scratch[2:],
                            scratch[0:1], scratch[1:2], sampled, 1.0 / temperature, seed, offset)
        return sampled.view(t.shape[:-1])
    return torch.argmax(torch.add(noise(t), t, alpha=1.0 / temperature), dim=-1)


def electra(logits: Optional[torch.Tensor], input_ids: torch.Tensor, tokenizer, masked_indices: torch.Tensor,
            temperature: int = 3, sampled: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor]:
    """-> (discriminator_input, disc_labels, non_padded_indices) (reference :81-105): the generator's samples
    scattered into the original ids at the masked positions, 1.0 where that changed the token, and the index tuple of
    the non-pad tokens.  sampled: the draw for the masked positions (numel = masked_indices.sum()), instead of
    sampling from `logits`.  The reference ends with torch.nonzero(..., as_tuple=True).to(...), which raises (a tuple
    has no .to); this returns the tuple of index tensors on the logits' device."""
    device = logits.device if logits is not None else input_ids.device
    input_ids = input_ids.to(device)
    masked_indices = masked_indices.to(device)
    if sampled is None:
        sampled = sample(logits[masked_indices], temperature=temperature)
    discriminator_input = input_ids.masked_scatter(masked_indices, sampled.detach().to(device, input_ids.dtype))
    disc_labels = discriminator_input.ne(input_ids).to(torch.float32)
    return discriminator_input, disc_labels, input_ids.ne(tokenizer.pad_token_id).nonzero(as_tuple=True)


class LanguageModeling(Dataset):
    """A text file cut into examples of block_size ids, the tokenizer's special tokens included (reference :108-165).
    The tail that does not fill a block is dropped, as there.  The reference also pickles the examples next to the file
    and never reads them back; that side effect is left out."""

    def __init__(self, tokenizer, file_path: str, block_size: int):
        if not os.path.isfile(file_path):
            raise ValueError(f"LanguageModeling: no text file at {file_path!r}")
        body = block_size - tokenizer.num_special_tokens_to_add(pair=False)
        with open(file_path, encoding="utf-8") as f:
            ids = tokenizer.convert_tokens_to_ids(tokenizer.tokenize(f.read()))
        self.examples = [tokenizer.build_inputs_with_special_tokens(ids[i:i + body])
                         for i in range(0, len(ids) - body + 1, body)]

    def __len__(self) -> int:
        return len(self.examples)

    def __getitem__(self, i):
        return dict(input_ids=torch.as_tensor(self.examples[i], dtype=torch.long))
