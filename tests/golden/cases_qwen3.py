"""Cases of Qwen3Model (models/qwen3.py) shared by the fixture maker (reference side: the model cell of
Examples/simple_vllm.ipynb) and the tests (HIP side): cfg dicts, recipe weights, prompts and sub-sampling.  numpy only
at import; torch where a function builds or fills a model."""
from __future__ import annotations

import numpy as np

from vyomai_amd import recipe

B, PROMPT, GREEDY_NEW = 2, 8, 16

_COMMON = dict(vocab_size=512, context_length=128, n_layers=2)
# name -> cfg without "dtype" (cfg() adds it).  q: n_heads * head_dim = 512 != emb_dim, 16 lanes per head in the fused
# qk-norm kernel; r: one KV group, 8 lanes per head; n: no qk_norm (the plain rope-write kernel); t: 4 lanes per head,
# as many KV groups as heads, and the head tied to the embedding table (TIED)
CASES = {
    "q": dict(_COMMON, emb_dim=256, n_heads=4, n_kv_groups=2, head_dim=128, hidden_dim=512, qk_norm=True, rope_base=1e6),
    "r": dict(_COMMON, emb_dim=192, n_heads=4, n_kv_groups=1, head_dim=64, hidden_dim=384, qk_norm=True, rope_base=1e4),
    "n": dict(_COMMON, emb_dim=256, n_heads=4, n_kv_groups=2, head_dim=64, hidden_dim=512, qk_norm=False, rope_base=1e6),
    "t": dict(_COMMON, emb_dim=128, n_heads=2, n_kv_groups=2, head_dim=32, hidden_dim=256, qk_norm=True, rope_base=1e4),
}
TIED = ("t",)


def cfg(case: str, dtype) -> dict:
    return dict(CASES[case], dtype=dtype)


def param_array(name: str, shape) -> np.ndarray:
    """The recipe's value of a parameter of the model.  recipe.param_value alone would take the `scale` vectors for
    biases (values near zero), and the embedding table for a matrix."""
    shape = tuple(shape)
    if name.endswith(".scale"):
        return recipe.uniform(name, shape, 0.1, 1.0)
    if name == "tok_emb.weight":
        return recipe.uniform(name, shape, 1.0)
    return recipe.param_value(name, shape)


def build(model_cls, case: str, dtype):
    """model_cls(cfg) with recipe weights (fp32 values rounded to each parameter's dtype); the head tied for the cases
    in TIED.  Works on either side: the reference's class or this package's."""
    import torch
    m = model_cls(cfg(case, dtype))
    if case in TIED:
        m.out_head.weight = m.tok_emb.weight
    with torch.no_grad():
        for name, p in m.named_parameters():      # (a tied table is listed once, under tok_emb.weight)
            p.copy_(torch.from_numpy(param_array(name, p.shape)).to(p.dtype))
    return m.eval()


def prompts(case: str, seed: int) -> np.ndarray:
    return recipe.token_ids(f"qwen3.{case}.prompt.{seed}", (B, PROMPT), 3, CASES[case]["vocab_size"])


def sub_v(logits):
    """(..., vocab) logits as stored: every 4th vocabulary entry."""
    return logits[..., ::4]
