"""FeedForward with the reference's signature and parameter names (VyomAI/layers/ffn.py:18-40):
LN(dropout(out(act(intermediate(x)))) + input_tensor), width multiplier*hidden (NOT
config.intermediate_size, like the reference :19-23).

MI355X: two MFMA GEMM launches -- bias+activation in the first epilogue, bias+dropout+residual in the
second -- and one LayerNorm launch."""
from __future__ import annotations

from typing import Union

import torch
import torch.nn as nn

from .._lib import (ACT_GELU_ERF, ACT_GELU_TANH, ACT_LEAKY_RELU, ACT_RELU6, ACT_SIGMOID, ACT_SILU,
                    ACT_TANH)

# every name of the reference's table (:7-15) has a fused HIP epilogue ("swish" is silu, leaky_relu has
# nn.LeakyReLU()'s default slope); gelu_tanh is this package's addition for the PaliGemma-shape model.
_FUSED_ACT = {"gelu": ACT_GELU_ERF, "gelu_tanh": ACT_GELU_TANH, "gelu_pytorch_tanh": ACT_GELU_TANH,
              "leaky_relu": ACT_LEAKY_RELU, "relu6": ACT_RELU6, "sigmoid": ACT_SIGMOID,
              "silu": ACT_SILU, "swish": ACT_SILU, "tanh": ACT_TANH}


class FeedForward(nn.Module):
    def __init__(self, config, multiplier: Union[int, float] = 4) -> None:
        super().__init__()
        inner = int(multiplier) * config.hidden_size
        self.intermediate = nn.Linear(config.hidden_size, inner)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.layernorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        name = getattr(config, "hidden_act", None)
        # unknown names fall back to GELU like the reference (:26-29)
        self.act = _FUSED_ACT.get(name, ACT_GELU_ERF)
        self.out = nn.Linear(inner, config.hidden_size)

    def forward(self, hidden_state: torch.Tensor, input_tensor: torch.Tensor) -> torch.Tensor:
        from ..autograd import ffn_block
        if type(self.intermediate) is not nn.Linear or type(self.out) is not nn.Linear:
            from ..encoder_lora_train import refuse_direct_call
            refuse_direct_call("FeedForward.intermediate / out", self.intermediate, self.out)
        return ffn_block(hidden_state, input_tensor, self.intermediate.weight, self.intermediate.bias,
                         self.out.weight, self.out.bias, self.layernorm.weight, self.layernorm.bias,
                         self.layernorm.eps, self.act, self.dropout.p, self.training)
