"""Cases of the Qwen3Model training fixtures (qwen3_train.npz) shared by the fixture maker (reference side: the model
cell of Examples/simple_vllm.ipynb, differentiated through its prefill branch) and the tests (HIP side).  The four
configurations, the recipe weights and `build` are those of cases_qwen3.py.  numpy only at import."""
from __future__ import annotations

import numpy as np

from tests.golden import cases_causal_lm as CL
from tests.golden import cases_qwen3 as C
from vyomai_amd import recipe

CASES, TIED, build, cfg = C.CASES, C.TIED, C.build, C.cfg
LENGTHS, L = (24, 17, 9), 24        # true lengths of the three rows, right-padded to L with id 0
LR, WEIGHT_DECAY, TRAIN_STEPS = CL.LR, CL.WEIGHT_DECAY, CL.TRAIN_STEPS
sub_g = CL.sub_g
# (the cases without qk_norm have no q_norm / k_norm: trained() drops those two names)
TRAINED = ("trf_blocks.0.att.q_norm.scale", "trf_blocks.1.att.k_norm.scale", "trf_blocks.0.att.W_key.weight",
           "trf_blocks.1.ff.fc2.weight", "tok_emb.weight", "final_norm.scale")

DPO_CASE = "q"
PAIRS = 4
PROMPT_LEN = (3, 9, 5, 7)
RESPONSE_LEN = ((11, 7), (6, 15), (14, 10), (9, 4))
CHOSEN = (1, 0, 0, 0)
DELTA, BETAS, GRAD_BETA = 1.0, (1.0, 0.1), 1.0


def trained(case: str):
    return tuple(n for n in TRAINED if CASES[case]["qk_norm"] or "_norm.scale" not in n or n == "final_norm.scale")


def train_batch(case: str):
    """-> (ids (3, L) int64, attention_mask (3, L) int64, labels (3, L) int64): -100 on the padding, and from position 12
    on in row 0."""
    V = CASES[case]["vocab_size"]
    x = recipe.token_ids(f"qwen3.train.{case}.ids", (len(LENGTHS), L), 3, V)
    m = np.zeros((len(LENGTHS), L), dtype=np.int64)
    for r, n in enumerate(LENGTHS):
        m[r, :n] = 1
    x[m == 0] = 0
    y = x.copy()
    y[m == 0] = -100
    y[0, 12:] = -100
    return x, m, y


def dpo_batch(case: str = DPO_CASE) -> dict:
    """The layout of cases_dpo.batch (the notebook's dpo_collate) over this model's vocabulary, plus the true lengths
    (chosen_len / rejected_len) the reference side packs its rows by."""
    V = CASES[case]["vocab_size"]
    out = {k: np.zeros((PAIRS, L), dtype=np.int64) for k in ("chosen", "rejected")}
    out.update({k + "_mask": np.zeros((PAIRS, L), dtype=np.float32) for k in ("chosen", "rejected")})
    out.update({k + "_len": np.zeros((PAIRS,), dtype=np.int64) for k in ("chosen", "rejected")})
    for i in range(PAIRS):
        p = PROMPT_LEN[i]
        prompt = recipe.token_ids(f"qwen3.dpo.{case}.prompt.{i}", (p,), 3, V)
        for key, r in (("chosen", CHOSEN[i]), ("rejected", 1 - CHOSEN[i])):
            n = RESPONSE_LEN[i][r]
            assert p + n <= L
            out[key][i, :p] = prompt
            out[key][i, p:p + n] = recipe.token_ids(f"qwen3.dpo.{case}.response.{i}.{r}", (n,), 3, V)
            out[key + "_mask"][i, p + 1:p + n] = 1.0
            out[key + "_len"][i] = p + n
    return out


def build_policy(model_cls, case: str, dtype):
    """The DPO policy: build()'s recipe weights moved by DELTA * mean|p| * u per parameter, u uniform in [-1, 1); the
    frozen model is build() itself."""
    import torch
    m = build(model_cls, case, torch.float32)
    with torch.no_grad():
        for name, p in m.named_parameters():
            u = torch.from_numpy(recipe.uniform("qwen3.dpo.delta." + name, tuple(p.shape)))
            p.add_(DELTA * p.abs().mean() * u)
    if dtype != torch.float32:
        for name, p in m.named_parameters():
            if not name.endswith(".scale"):        # (the RMSNorm scales stay fp32, as the model builds them)
                p.data = p.data.to(dtype)
        for name, b in m.named_buffers():
            b.data = b.data.to(dtype)
    return m
