"""Cases of encoder LoRA fine-tuning for classification (vyomai_amd/encoder_lora_train.py,
EncoderForSequenceClassification) shared by the fixture maker (reference side) and the tests (HIP side): a
cases.micro_cfg()-sized EncoderModel (d = 64, 4 heads, 2 layers, hidden_dropout_prob = 0) under a ClinicModel-shaped
head (Examples/adapters.ipynb: hidden[:, 0, :] -> nn.Linear(hidden, NUM_LABELS) -> CrossEntropyLoss), with two adapters
under the reference's key names.  numpy only.

MODELS  abs: absolute positions, vanilla attention;  rope_gqa: RoPE, grouped-query attention (2 kv heads).
n5: rank 32, alpha 1 on the notebook's five targets (query, value, attention output, both feed-forward sides; key off).
n6: rank 8, alpha 2 on all six: rank padding, and a packed QKV with every part adapted.

The batch is B = 3 rows of L = 17 tokens under cases.keypad: 51 rows, a ragged last 16-row tile.  Adapter values:
cases_lora.value's grid (exact in bf16), lora_b NOT zero."""
from __future__ import annotations

import numpy as np

from tests.golden import cases
from tests.golden import cases_lora as L
from vyomai_amd import recipe

B, SEQ, NUM_LABELS = 3, 17, 5
LAYERS = 2
LR, WEIGHT_DECAY, TRAIN_STEPS = 1e-3, 0.01, 3
MODELS = {"abs": ("absolute", None), "rope_gqa": ("rope", "gqa")}
QKV = ("attention.query", "attention.key", "attention.value")
REST = ("attention.out.dense", "feed_forward.intermediate", "feed_forward.out")
ADAPTERS = {
    "n5": dict(rank=32, alpha=1.0, on=("attention.query", "attention.value") + REST),
    "n6": dict(rank=8, alpha=2.0, on=QKV + REST),
}
LABELS = np.array([1, 4, 0], dtype=np.int64)


def cfg(model: str):
    c = cases.micro_cfg()
    c.num_hidden_layers, c.hidden_dropout_prob = LAYERS, 0.0
    return cases.with_kv(c, MODELS[model][1])


def shapes(model: str) -> dict:
    """projection path inside a layer -> (out_features, in_features)."""
    c = cfg(model)
    d = c.hidden_size
    kv = d if MODELS[model][1] is None else c.num_key_value_heads * (d // c.num_attention_heads)
    return {"attention.query": (d, d), "attention.key": (kv, d), "attention.value": (kv, d),
            "attention.out.dense": (d, d), "feed_forward.intermediate": (4 * d, d), "feed_forward.out": (d, 4 * d)}


def adapter_state(model: str, who: str, prefix: str = "model.") -> dict:
    """key -> fp32 array: `<prefix>all_layer.<l>.<projection>.lora_a` (rank, in) / `.lora_b` (out, rank)."""
    spec, sh, out = ADAPTERS[who], shapes(model), {}
    for l in range(LAYERS):
        for path in spec["on"]:
            out_f, in_f = sh[path]
            key = f"{prefix}all_layer.{l}.{path}"
            name = f"enc.{who}.all_layer.{l}.{path}"
            out[key + ".lora_a"] = L.value(name + ".lora_a", (spec["rank"], in_f))
            out[key + ".lora_b"] = L.value(name + ".lora_b", (out_f, spec["rank"]))
    return out


def load_weights_(m) -> None:
    """The recipe's values into a classifier (`model` + `output`), reference or HIP side: the same state_dict names."""
    recipe.load_recipe_(m)


def batch():
    """-> (ids (B, L) int64, mask (B, L) int64 right padding, labels (B,) int64)."""
    c = cfg("abs")
    return recipe.token_ids("enc_lora.ids", (B, SEQ), 3, c.vocab_size), cases.keypad(B, SEQ), LABELS.copy()


def trained_keys(model: str, who: str):
    return sorted(adapter_state(model, who)) + ["output.bias", "output.weight"]


def sub_g(a):
    """What the fixture keeps of a gradient or a trained weight: every second row and column of a matrix."""
    a = np.asarray(a)
    return a[::2, ::2] if a.ndim == 2 else a
