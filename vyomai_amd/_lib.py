"""ctypes binding of libvyom_hip.so (C ABI in include/vyom_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950) into
``vyomai_amd/lib/``.  There is no fallback: if it is missing or a call fails, the op raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# VY_LIB_PATH: developer knob for A/B runs of two builds of the same ABI on one box (tools/ab_lib.sh)
LIB_PATH = os.environ.get("VY_LIB_PATH") or os.path.join(_HERE, "lib", "libvyom_hip.so")

VY_F32, VY_BF16 = 0, 1
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH = 0, 1, 2
# the reference's other hidden_act choices (vy_act in include/vyom_hip.h; leaky_relu: slope 0.01)
ACT_SILU, ACT_TANH, ACT_SIGMOID, ACT_RELU6, ACT_LEAKY_RELU = 3, 4, 5, 6, 7
ACT_SAVE_DERIV = 0x100   # saved tensor = act'(pre) instead of pre (include/vyom_hip.h)
LORA_EPI_ACT, LORA_EPI_DROP_RES, LORA_EPI_MUL = 0, 1, 2   # vy_lora_expand_epi's modes
MASK_NONE, MASK_CAUSAL, MASK_KEYPAD, MASK_ADDITIVE = 0, 1, 2, 4

_p, _i64, _i, _f, _u64 = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_uint64

# name -> argtypes, exactly the prototypes of include/vyom_hip.h
PROTOTYPES = {
    "vy_linear_fwd": [_p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i, _i, _p],
    "vy_qkv_rope_fwd": [_p, _i64, _p, _i64, _p, _p, _p, _i64,
                        _p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64,
                        _i64, _i64, _i64, _i, _i, _i, _i, _p],
    "vy_attn_fwd": [_p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64,
                    _p, _i64, _i64, _p, _i, _i64, _p, _i64, _p, _i64, _i64,
                    _i64, _i, _i, _i64, _i64, _i, _f, _i, _p],
    "vy_attn_decode": [_p, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64,
                       _p, _i64, _i64, _i, _i, _i64, _i, _f, _i, _p],
    "vy_paged_rope_write": [_p, _i64, _p, _p, _p, _p, _i64, _p, _p, _i64, _i, _i64, _i, _i, _i, _i, _p],
    "vy_paged_qknorm_rope_write": [_p, _i64, _p, _p, _p, _p, _i64, _p, _p, _f, _p, _p, _i64, _i, _i64, _i, _i, _i, _i,
                                   _p],
    "vy_attn_paged_decode": [_p, _i64, _p, _p, _p, _i64, _i, _p, _i64, _p, _i64, _p, _i64, _i64, _i, _i, _i, _f, _i,
                             _p, _i64, _i, _p],
    "vy_attn_paged_prefill": [_p, _i64, _p, _p, _i64, _i, _p, _i64, _p, _p, _i64, _i64, _i64, _p, _i64, _i, _i, _i, _f,
                              _i, _p],
    "vy_paged_gather": [_p, _p, _i64, _i, _p, _i64, _i64, _p, _p, _i, _i, _i, _p],
    "vy_paged_rope_write_fp8": [_p, _i64, _p, _p, _p, _p, _i64, _p, _p, _f, _p, _p, _p, _p, _i64, _i, _i64, _i, _i, _i,
                                _i, _p],
    "vy_attn_paged_decode_fp8": [_p, _i64, _p, _p, _p, _p, _p, _i64, _i, _p, _i64, _p, _i64, _p, _i64, _i64, _i, _i, _i,
                                 _f, _i, _p, _i64, _i, _p],
    "vy_attn_paged_prefill_fp8": [_p, _i64, _p, _p, _p, _p, _i64, _i, _p, _i64, _p, _p, _i64, _i64, _i64, _p, _i64, _i,
                                  _i, _i, _f, _i, _p],
    "vy_layernorm_fwd": [_p, _i64, _p, _p, _p, _i64, _p, _p, _i64, _i64, _f, _i, _p],
    "vy_rmsnorm_fwd": [_p, _i64, _p, _p, _i64, _i64, _i64, _f, _f, _i, _p],
    "vy_gated_act_fwd": [_p, _i64, _p, _i64, _i64, _i64, _i, _i, _p],
    "vy_rmsnorm_bwd": [_p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _p, _f, _p, _i64, _i64, _f, _f, _i, _p],
    "vy_gated_act_bwd": [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i, _i, _p],
    "vy_qknorm_rope_fwd": [_p, _i64, _p, _p, _i64, _i64, _p, _p, _f, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64,
                           _i64, _i64, _i, _i, _i, _i, _p],
    "vy_qknorm_bwd": [_p, _i64, _p, _i64, _p, _p, _f, _p, _p, _f, _p, _i64, _i, _i, _i, _i, _p],
    "vy_rope_fwd": [_p, _i64, _i64, _i64, _p, _p, _i64, _i64, _i, _i64, _i, _i, _i, _p],
    "vy_linear_dgrad": [_p, _i64, _p, _i64, _p, _i64, _i, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _i, _p],
    "vy_linear_wgrad": [_p, _i64, _p, _i64, _p, _i64, _p, _f, _p, _i64, _i64, _i64, _i, _p],
    "vy_linear_wgrad_riders": [_p, _i64, _p, _i64, _p, _i64, _p, _f, _p, _i64, _i64, _i64, _i, _p, _i, _p, _i, _i, _i, _p, _p],
    "vy_linear_wgrad_grouped": [_p, _i, _i, _p],
    "vy_linear_wgrad_grouped_cs": [_p, _i, _p, _i, _i, _p],
    "vy_linear_wgrad_grouped_opt": [_p, _i, _p, _i, _p, _i, _p, _i, _p],
    "vy_layernorm_bwd_partial": [_p, _i64, _p, _i64, _p, _p, _p, _p, _i64, _p, _i64, _i64, _i, _p],
    "vy_layernorm_bwd": [_p, _i64, _p, _i64, _p, _p, _p, _p, _i64, _p, _p, _f, _p, _i64, _i64, _i, _p],
    "vy_attn_bwd": [_p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64,
                    _p, _p, _i64, _i64, _p, _p,
                    _p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64,
                    _i, _i64, _p, _i64, _p, _p, _i64, _i64, _i, _i, _i64, _i64, _i, _f, _i, _p],
    "vy_adamw_step": [_p, _p, _p, _p, _p, _i64, _f, _f, _f, _f, _f, _i64, _f, _p, _p],
    "vy_adamw_step_gated": [_p, _p, _p, _p, _p, _i64, _f, _f, _f, _f, _f, _i64, _f, _p, _p, _p],
    "vy_sumsq": [_p, _i64, _p, _p, _p],
    "vy_linear_dropout_fwd": [_p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _f, _u64, _u64, _i, _p],
    "vy_dropout": [_p, _i64, _p, _i64, _i64, _i64, _f, _u64, _u64, _i, _p],
    "vy_act_bwd": [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i, _i, _p],
    "vy_xent_fwd": [_p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _p, _i, _p],
    "vy_xent_bwd": [_p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _i, _p],
    "vy_xent_fused": [_p, _i64, _p, _i64, _p, _p, _p, _p, _i64, _i64, _p, _i, _p],
    "vy_xent_sample_fwd": [_p, _i64, _p, _i64, _p, _p, _p, _p, _f, _u64, _u64, _i64, _i64, _p, _i, _p],
    "vy_xent_sample_fused": [_p, _i64, _p, _i64, _p, _p, _p, _p, _p, _f, _u64, _u64, _i64, _i64, _p, _i, _p],
    "vy_gumbel_noise": [_p, _i64, _i64, _i64, _u64, _u64, _p],
    "vy_bce_head_fwd": [_p, _i64, _p, _p, _p, _p, _p, _p, _i64, _i64, _i, _p],
    "vy_bce_head_bwd": [_p, _i64, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _i, _i64, _i64, _i, _p],
    "vy_mlm_mask": [_p, _i64, _p, _i, _f, _i64, _i64, _i64, _u64, _u64, _p, _p, _p, _p],
    "vy_logprob_fwd": [_p, _i64, _p, _p, _p, _p, _i64, _i64, _p, _i, _p],
    "vy_logprob_bwd": [_p, _i64, _p, _p, _p, _i64, _i64, _i, _p],
    "vy_logprob_fused": [_p, _i64, _p, _p, _p, _p, _i64, _i64, _p, _i, _p],
    "vy_transpose_batched": [_p, _i, _i, _i, _p],
    "vy_transpose_batched_range": [_p, _i, _i, _i, _i, _p],
    "vy_embedding_fwd": [_p, _i64, _p, _p, _i64, _i64, _i64, _i64, _p, _i, _p],
    "vy_embedding_bwd": [_p, _i64, _p, _p, _i64, _i64, _i64, _i64, _i64, _i, _p],
    "vy_transpose": [_p, _i64, _p, _i64, _i64, _i64, _i, _p],
    "vy_greedy_step": [_p, _i64, _i64, _i64, _i, _p, _i64, _i64, _p, _i64, _p, _i, _p, _p, _p],
    "vy_sampling_probs": [_p, _i64, _i64, _i64, _i, _f, _i, _f, _p, _i64, _p],
    "vy_sample_rows": [_p, _i64, _i64, _i64, _i, _p, _p, _p, _p, _p, _p, _p],
    "vy_spec_verify": [_p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "vy_lora_shrink": [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i, _p],
    "vy_lora_expand": [_p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i, _p],
    "vy_lora_expand_epi": [_p, _i64, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _i64,
                           _i64, _i64, _i, _i, _f, _u64, _u64, _i, _p],
    "vy_cls_head_fwd": [_p, _i64, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i, _p],
    "vy_cls_head_bwd": [_p, _i64, _p, _p, _p, _p, _p, _p, _i, _i64, _i64, _i64, _i64, _i, _p],
    "vy_lora_wgrad": [_p, _i64, _p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64,
                      _i64, _i64, _i64, _f, _i, _i, _p],
    "vy_dora_compose": [_p, _i, _i, _p],
    "vy_dora_bwd": [_p, _i, _i, _p],
    "vy_decoder_step": [_p, _p, _i64, _p, _p, _p, _i64, _p],
    "vy_gemma_decoder_step": [_p, _p, _i64, _p, _i64, _p],
    "vy_quant_rows_fp8": [_p, _i64, _p, _i64, _p, _i64, _i64, _i, _p],
    "vy_gemma_decoder_step_w8": [_p, _p, _p, _i64, _p, _i64, _p],
    "vy_cast": [_p, _p, _i64, _i, _i, _p],
    "vy_ddp_unique_id": [_p],
    "vy_ddp_init": [_p, _i, _i],
    "vy_ddp_all_reduce_async": [_p, _i64, _i, _p],
    "vy_ddp_destroy": [],
    "vy_set_concurrent_chains": [_i],
    "vy_workspace_set": [_p, _p, _i64],
}
OTHER_SYMBOLS = ["vy_last_error", "vy_abi_version", "vy_layernorm_bwd_ws_rows", "vy_decode_ws_bytes",
                 "vy_gemma_ws_bytes", "vy_ddp_world", "vy_ddp_rank", "vy_attn_paged_decode_ws_bytes",
                 "vy_attn_paged_decode_fp8_ws_bytes", "vy_lora_wgrad_chunk_rows", "vy_qknorm_bwd_ws_floats"]
ALL_SYMBOLS = list(PROTOTYPES) + OTHER_SYMBOLS


class VyWgradDesc(C.Structure):
    """vy_wgrad_desc of include/vyom_hip.h."""
    _fields_ = [("dy", _p), ("lddy", _i64), ("x", _p), ("ldx", _i64), ("dw", _p), ("lddw", _i64), ("db", _p),
                ("M", _i64), ("N", _i64), ("K", _i64)]


class VyColsumDesc(C.Structure):
    """vy_colsum_desc of include/vyom_hip.h."""
    _fields_ = [("ws", _p), ("W", C.c_int32), ("N", C.c_int32), ("out0", _p), ("out1", _p), ("acc", C.c_int32)]


class VyAdamwRideDesc(C.Structure):
    """vy_adamw_ride_desc of include/vyom_hip.h (taken: written by the launcher)."""
    _fields_ = [("p", _p), ("g", _p), ("m", _p), ("v", _p), ("p_bf16", _p), ("n", _i64), ("taken", _i64)]


class VyZeroRideDesc(C.Structure):
    """vy_zero_ride_desc of include/vyom_hip.h (taken: written by the launcher)."""
    _fields_ = [("p", _p), ("n", _i64), ("taken", _i64)]


class VyAdamwHyper(C.Structure):
    """vy_adamw_hyper of include/vyom_hip.h."""
    _fields_ = [("lr", _f), ("beta1", _f), ("beta2", _f), ("eps", _f), ("weight_decay", _f), ("grad_scale", _f),
                ("step", _i64)]


class VyDoraDesc(C.Structure):
    """vy_dora_desc of include/vyom_hip.h."""
    _fields_ = [("w", _p), ("ldw", _i64), ("w_dtype", C.c_int32), ("a", _p), ("b", _p), ("m", _p), ("c", _p),
                ("wp", _p), ("ldwp", _i64), ("g", _p), ("ldg", _i64), ("dm", _p), ("da", _p), ("db", _p),
                ("out", _i64), ("in_", _i64), ("r", _i64)]


class VyomHipError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the kernel library; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VyomHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  vyomai_amd has no CPU or PyTorch fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.vy_last_error.restype = C.c_char_p
    lib.vy_last_error.argtypes = []
    lib.vy_abi_version.restype = C.c_int
    lib.vy_layernorm_bwd_ws_rows.restype = C.c_int64
    lib.vy_layernorm_bwd_ws_rows.argtypes = [_i64]
    lib.vy_decode_ws_bytes.restype = C.c_int64
    lib.vy_decode_ws_bytes.argtypes = [C.c_int32] * 7
    lib.vy_attn_paged_decode_ws_bytes.restype = C.c_int64
    lib.vy_attn_paged_decode_ws_bytes.argtypes = [_i64, _i, _i, _i, _i64, _i, _i]
    lib.vy_attn_paged_decode_fp8_ws_bytes.restype = C.c_int64
    lib.vy_attn_paged_decode_fp8_ws_bytes.argtypes = [_i64, _i, _i, _i, _i64, _i, _i]
    lib.vy_lora_wgrad_chunk_rows.restype = C.c_int64
    lib.vy_lora_wgrad_chunk_rows.argtypes = [_i64, _i64, _i64]
    lib.vy_qknorm_bwd_ws_floats.restype = C.c_int64
    lib.vy_qknorm_bwd_ws_floats.argtypes = [_i64, _i, _i, _i]
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise VyomHipError(f"{name} failed ({rc}): {lib.vy_last_error().decode()}")


def dtype_code(torch_dtype) -> int:
    import torch

    if torch_dtype == torch.bfloat16:
        return VY_BF16
    if torch_dtype == torch.float32:
        return VY_F32
    raise VyomHipError(f"vyomai_amd kernels support float32 and bfloat16, got {torch_dtype}")
