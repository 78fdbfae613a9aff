"""Cases of the DPO fixtures (Examples/vyom-ai-llm-sft-dpo-training.ipynb on ModelForCausalLM) shared by the fixture
maker (reference side) and the tests (HIP side): the preference batch in the layout of the notebook's dpo_collate, the
policy's weights and the bar arithmetic.  numpy only.  Configurations, sub-sampling and the AdamW settings are those of
cases_causal_lm.py."""
from __future__ import annotations

import numpy as np

from tests.golden import cases_causal_lm as C
from vyomai_amd import recipe

CASES = C.CASES
PAIRS, L = 4, 24
PROMPT_LEN = (3, 9, 5, 7)           # shared prompt of each pair
RESPONSE_LEN = ((11, 7), (6, 15), (14, 10), (9, 4))   # two responses per pair: unequal, right-padded with pad_token_id 0
CHOSEN = (1, 0, 0, 0)               # which of the two is the chosen one (picked so that the DPO logits take both signs
                                    # and the beta = 1 loss stays clear of ln 2 in both configurations)
DELTA = 1.0                         # policy = recipe weights + DELTA * mean|p| * uniform("dpo.delta." + name)
BETAS = (1.0, 0.1)                  # beta = 0.1 alone sits within 7e-3 of ln 2: it cannot tell a model from no model
GRAD_BETA = 1.0                     # the stored gradients and the training steps use this one
LR, WEIGHT_DECAY, TRAIN_STEPS, TRAINED = C.LR, C.WEIGHT_DECAY, C.TRAIN_STEPS, C.TRAINED
sub_g, sub_h = C.sub_g, C.sub_h


def batch(case: str) -> dict:
    """The notebook's collated batch: chosen / rejected ids (PAIRS, L) int64, chosen_mask / rejected_mask float32 with
    zeros on the prompt, on the one token after it and on the padding."""
    V = CASES[case]["vocab_size"]
    out = {k: np.zeros((PAIRS, L), dtype=np.int64) for k in ("chosen", "rejected")}
    out.update({k + "_mask": np.zeros((PAIRS, L), dtype=np.float32) for k in ("chosen", "rejected")})
    for i in range(PAIRS):
        p = PROMPT_LEN[i]
        prompt = recipe.token_ids(f"dpo.{case}.prompt.{i}", (p,), 3, V)
        for key, r in (("chosen", CHOSEN[i]), ("rejected", 1 - CHOSEN[i])):
            n = RESPONSE_LEN[i][r]
            assert p + n <= L
            out[key][i, :p] = prompt
            out[key][i, p:p + n] = recipe.token_ids(f"dpo.{case}.response.{i}.{r}", (n,), 3, V)
            out[key + "_mask"][i, p + 1:p + n] = 1.0
    return out


def load_reference_weights_(model) -> None:
    """The frozen reference model: the recipe weights."""
    C.load_weights_(model)


def load_policy_weights_(model) -> None:
    """The policy: the recipe weights moved by DELTA * mean|p| * u per parameter, u uniform in [-1, 1)."""
    import torch
    C.load_weights_(model)
    with torch.no_grad():
        for name, p in model.model.named_parameters():
            u = torch.from_numpy(recipe.uniform("dpo.delta.model." + name, tuple(p.shape)))
            p.add_(DELTA * p.abs().mean() * u.to(p.dtype))

