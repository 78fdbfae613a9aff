"""Case definitions of the hidden_act fixtures (tests/golden/activations.npz), shared by the generator
(make_golden_acts.py, reference side) and the tests (oracle / HIP side).  numpy only; cases.py stays as it is."""
from __future__ import annotations

import numpy as np

from tests.golden import cases

# every name of the reference's table (VyomAI/layers/ffn.py:7-15) except "gelu", which the older fixtures cover
NAMES = ("leaky_relu", "relu6", "sigmoid", "silu", "swish", "tanh")
# "swish" is nn.SiLU() again: it gets forward fixtures; gradients, layers and models run under "silu"
GRAD_NAMES = ("leaky_relu", "relu6", "sigmoid", "silu", "tanh")
SMOOTH = ("sigmoid", "silu", "tanh")
KINKED = ("leaky_relu", "relu6")
# vy_act codes (include/vyom_hip.h)
CODES = {"silu": 3, "swish": 3, "tanh": 4, "sigmoid": 5, "relu6": 6, "leaky_relu": 7}
# wide-config gradients are stored for these two only (a sub-sampled 3072 x 768 gradient is the bulk of the file)
WIDE_GRAD_NAMES = ("silu", "relu6")

# ---- kink inputs ------------------------------------------------------------------------------------------------------
# relu6 and leaky_relu have step derivatives at 0 (and 6).  The plain recipe inputs give FFN pre-activations of rms 0.46
# and max 2.0 (relu6's upper clamp never fires) whose nearest value to 0 is 2.3e-6 away: inside fp32 summation-order
# noise, where one flipped derivative moves a gradient by far more than any fp32 bar.  So:
#   * FeedForward is also run on a hidden state scaled by KINK_SCALE (about 3 % of the pre-activations above 6, half
#     below 0), under recipe tags chosen so that no reference pre-activation is near a kink;
#   * every fp32 GRADIENT of the two kinked names is taken on inputs whose reference pre-activations keep a margin from
#     both kinks: at least KINK_MIN_MARGIN for the two fixed FeedForward cases below (30x and 390x the reference's own
#     fp32-vs-fp64 pre-activation error), at least MARGIN_FACTOR x that error for the DecoderLayer input, which the
#     generator finds by search.  The generator asserts this and stores margin, error and the pre-activation; the GPU
#     test checks the kernel's pre-activation against it (within margin / 8) before it compares a gradient.
KINKS = (0.0, 6.0)
KINK_SCALE = 12.0
KINK_TAGS = {"micro": "acts.micro.k3", "wide": "acts.wide.k6"}      # of acts.{cfg}.k0 .. k7: margins 1.40e-3 / 1.51e-4
KINK_MIN_MARGIN = 1e-4
MARGIN_FACTOR = 32.0
LAYER_KINK_TAGS = tuple(f"acts.layer.k{i}" for i in range(16))       # the generator takes the first that qualifies
# the wide kink case stores the pre-activation only where it can matter: every element within NEAR_BAND of a kink (index
# and value), plus a sub-sampled grid; the test requires every OTHER element of the kernel's pre-activation to stay
# NEAR_BAND / 2 away from the kinks
NEAR_BAND = 0.05


def cfg_for(tag: str, name: str):
    cfg = cases.micro_cfg() if tag == "micro" else cases.wide_cfg()
    cfg.hidden_act = name
    return cfg


def model_cfg(name: str):
    """The reference tests' Config with two layers and the activation under test."""
    cfg = cases.test_cfg()
    cfg.num_hidden_layers = 2
    cfg.hidden_act = name
    return cfg


def kink_distance(pre) -> np.ndarray:
    """Distance of every pre-activation to the nearest kink."""
    pre = np.asarray(pre, dtype=np.float64)
    return np.minimum(*(np.abs(pre - k) for k in KINKS))


def near_kinks(pre) -> np.ndarray:
    """Flat indices of the pre-activations within NEAR_BAND of a kink."""
    return np.nonzero(kink_distance(pre).reshape(-1) < NEAR_BAND)[0].astype(np.int64)


# ---- sub-sampling (the file stays below 1 MiB) ------------------------------------------------------------------------

def sub_act(y):
    """An activation (..., D): whole up to 1024 elements, else its (rows, D) view with rows ::3, features ::5 (D > 64) or
    rows ::2, features ::2 (the micro width)."""
    if int(np.prod(y.shape)) <= 1024:
        return y
    y2 = y.reshape(-1, y.shape[-1])
    return y2[::3, ::5] if y.shape[-1] > 64 else y2[::2, ::2]


def sub_grad(g):
    """A parameter gradient: whole up to 1024 elements; vectors ::3; matrices up to 64 Ki elements rows ::7, columns ::5
    (cases.sub2), larger ones rows ::29, columns ::13."""
    n = int(np.prod(g.shape))
    if n <= 1024:
        return g
    if g.ndim == 1:
        return g[::3]
    return cases.sub2(g) if n <= 65536 else g[::29, ::13]


def sub_vit(y):
    """(B, 197, D) Vit output: cases.sub's positions, every 16th feature."""
    return cases.sub(y)[..., ::4]


def sub_logits(lg):
    """(B, L, V) logits: every second position, every 797th vocabulary entry."""
    return lg[:, ::2, ::797]
