"""Cases of the per-request LoRA adapters (vyomai_amd/adapters.py, serving.ContinuousBatchEngine(adapters=)) shared by
the fixture maker (reference side) and the tests (HIP side): ModelForCausalLM case "a" of cases_causal_lm.py with two
adapters under the reference's key names.  numpy only.

n1: rank 32, alpha 1 on q, v, o, gate, up, down -- the selection of the reference's Examples/adapters.ipynb (query,
    value, attention output, both MLP sides), so the key part of the packed QKV stays zero.
n2: rank 8, alpha 2 on all seven projections: rank padding.

Values: recipe.uniform scaled to (-0.1, 0.1) and rounded to multiples of 2^-10 -- at most 7 significant bits, so every
value is exact in bf16 and fp16 (the file stores them as fp16) -- with lora_b NOT zero."""
from __future__ import annotations

import numpy as np

from tests.golden import cases_causal_lm as C
from vyomai_amd import recipe

CASE = "a"
KW = C.CASES[CASE]
PREFILL, STEPS, NEW = C.PREFILL, C.STEPS, 8
LONG = 21               # a prompt that crosses a 16-row tile cut
SCALE, GRID = 0.1, 1024.0
ATTN = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj")
MLP = ("mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
ADAPTERS = {
    "n1": dict(rank=32, alpha=1.0, on=("self_attn.q_proj", "self_attn.v_proj", "self_attn.o_proj") + MLP),
    "n2": dict(rank=8, alpha=2.0, on=ATTN + MLP),
}
WHO = ("base",) + tuple(ADAPTERS)


def shapes():
    """projection path inside a layer -> (out_features, in_features)."""
    d, f = KW["hidden_size"], KW["intermediate_size"]
    dh = d // KW["num_attention_heads"]
    kv = KW["num_key_value_heads"] * dh
    return {"self_attn.q_proj": (d, d), "self_attn.k_proj": (kv, d), "self_attn.v_proj": (kv, d),
            "self_attn.o_proj": (d, d), "mlp.gate_proj": (f, d), "mlp.up_proj": (f, d), "mlp.down_proj": (d, f)}


def value(name: str, shape) -> np.ndarray:
    return (np.round(recipe.uniform("lora." + name, shape, SCALE) * GRID) / GRID).astype(np.float32)


def adapter_state(who: str) -> dict:
    """key -> fp32 array: `model.layers.<l>.<projection>.lora_a` (rank, in) / `.lora_b` (out, rank)."""
    spec, sh, out = ADAPTERS[who], shapes(), {}
    for l in range(KW["num_hidden_layers"]):
        for path in spec["on"]:
            out_f, in_f = sh[path]
            key = f"model.layers.{l}.{path}"
            out[key + ".lora_a"] = value(f"{who}.{key}.lora_a", (spec["rank"], in_f))
            out[key + ".lora_b"] = value(f"{who}.{key}.lora_b", (out_f, spec["rank"]))
    return out


def ids() -> np.ndarray:
    """(B, 16): prefill(8) + 8 teacher-forced steps, the rows of cases_causal_lm."""
    return C.ids(CASE)


def prompts(seed: int) -> np.ndarray:
    """(B, 8) greedy prompts."""
    return recipe.token_ids(f"lora.prompt.{seed}", (C.B, PREFILL), 3, KW["vocab_size"])


def long_prompt(seed: int) -> np.ndarray:
    return recipe.token_ids(f"lora.long.{seed}", (LONG,), 3, KW["vocab_size"])


def load(npz, who: str) -> dict:
    """The adapter `who` out of lora.npz as the state dict LoraAdapters.load takes (fp32 arrays)."""
    return {str(k): npz[f"{who}.w.{k}"].astype(np.float32) for k in npz[f"{who}.keys"]}
