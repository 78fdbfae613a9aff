"""Cases of DoRA fine-tuning (vyomai_amd/adapters.py DoraLinear, dora_train.py) shared by the fixture maker (reference
side) and the tests (HIP side): ModelForCausalLM case "a" of cases_causal_lm.py with two adapters under the reference's
key names.  numpy only.

d1: rank 32 on q, v, o, gate, up, down -- the selection of the reference's Examples/adapters.ipynb, so the key part of
    the packed QKV stays plain.
d2: rank 8 on all seven projections.

Values: dora_a and dora_b are recipe.uniform scaled to (-0.1, 0.1) and rounded to multiples of 2^-10, as cases_lora.py
does, with dora_b NOT zero (with dora_b = 0 the gradient of dora_a vanishes and the derivative of the norm is never
exercised).  dora_m is its initial value -- the column norms of the wrapped weight, in fp64 from the recipe's weight --
times a factor in (0.75, 1.25) on the same grid."""
from __future__ import annotations

import numpy as np

from tests.golden import cases_causal_lm as C
from tests.golden import cases_lora as L
from vyomai_amd import recipe

CASE = "a"
KW = C.CASES[CASE]
ADAPTERS = {
    "d1": dict(rank=32, on=("self_attn.q_proj", "self_attn.v_proj", "self_attn.o_proj") + L.MLP),
    "d2": dict(rank=8, on=L.ATTN + L.MLP),
}
LEAVES = ("dora_m", "dora_a", "dora_b")
shapes = L.shapes


def value(name: str, shape) -> np.ndarray:
    return (np.round(recipe.uniform("dora." + name, shape, L.SCALE) * L.GRID) / L.GRID).astype(np.float32)


def adapter_state(who: str) -> dict:
    """key -> fp32 array: `model.layers.<l>.<projection>.dora_m` (1, in) / `.dora_a` (out, rank) / `.dora_b` (rank, in)."""
    spec, sh, out = ADAPTERS[who], shapes(), {}
    for l in range(KW["num_hidden_layers"]):
        for path in spec["on"]:
            out_f, in_f = sh[path]
            key = f"model.layers.{l}.{path}"
            w = recipe.param_value(key + ".weight", (out_f, in_f)).astype(np.float64)
            factor = 1.0 + np.round(recipe.uniform(f"dora.{who}.{key}.dora_m", (1, in_f), 0.25) * L.GRID) / L.GRID
            out[key + ".dora_m"] = (np.sqrt((w * w).sum(axis=0, keepdims=True)) * factor).astype(np.float32)
            out[key + ".dora_a"] = value(f"{who}.{key}.dora_a", (out_f, spec["rank"]))
            out[key + ".dora_b"] = value(f"{who}.{key}.dora_b", (spec["rank"], in_f))
    return out
