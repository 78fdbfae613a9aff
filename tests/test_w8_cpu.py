"""fp8-weight decode, host side without a GPU: the new public symbols are declared, exported and mirrored, the ABI version
stays, and the ctypes mirrors of the two new structs have the size the header's layout gives them."""
import ctypes as C
import re
from pathlib import Path

PUBLIC = {"vy_quant_rows_fp8": 9, "vy_gemma_decoder_step_w8": 7}
DEBUG = ("vy_debug_dec_gemv1_w8", "vy_debug_dec_gemv1_gated_w8", "vy_debug_dec_gemv1_qkv_w8", "vy_debug_gemma_w8_last")


def test_symbols_are_declared_exported_and_mirrored_and_the_abi_version_stays():
    from vyomai_amd import _lib
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in PUBLIC.items():
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert proto, name
        assert name in _lib.PROTOTYPES and name in _lib.ALL_SYMBOLS and hasattr(lib, name), name
        assert len(_lib.PROTOTYPES[name]) == proto.group(1).count(",") + 1 == n_args, name
    for name in DEBUG:                                  # test aids: exported, not part of the header
        assert hasattr(lib, name) and name not in hdr, name
    assert _lib.load().vy_abi_version() == 5, "additive symbols: the ABI version stays"


def test_struct_mirrors_have_the_headers_size():
    from vyomai_amd import decode_plan as D
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    assert re.search(r"typedef struct vy_gemma_w8_layer \{ const float \*s_qkv, \*s_o, \*s_gu, \*s_down; \} vy_gemma_w8_layer;", hdr)
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(D.VyGemmaW8Layer) == 4 * ptr and [f[0] for f in D.VyGemmaW8Layer._fields_] == ["s_qkv", "s_o", "s_gu", "s_down"]
    assert C.sizeof(D.VyGemmaW8) == 3 * ptr and [f[0] for f in D.VyGemmaW8._fields_] == ["layers", "head_codes", "head_scale"]
    # the existing plan struct is untouched by the option
    assert "head_w" in [f[0] for f in D.VyGemmaPlan._fields_] and D.VyGemmaPlan._fields_[-1][0] == "flags"


def test_plan_refuses_what_the_w8_chain_cannot_run_before_touching_a_gpu():
    """weight_dtype is validated first: an unknown value, an fp32 model and batch 2 are ValueErrors on the CPU."""
    import types
    import pytest
    import torch
    from tests.golden import cases
    from vyomai_amd.decode_plan import GemmaDecodePlan
    from vyomai_amd.models import paligemma as P
    vis = P.SiglipVisionConfig(**dict(cases.SIGLIP, num_hidden_layers=1))
    txt = types.SimpleNamespace(**dict(cases.GEMMA, num_hidden_layers=1, vocab_size=512, intermediate_size=2048))
    m = P.PaliGemmaForConditionalGeneration(P.PaliGemmaShape(vis, txt, txt.hidden_size))
    with pytest.raises(ValueError, match="weight_dtype"):
        GemmaDecodePlan(m, [], 1, weight_dtype="int4")
    with pytest.raises(ValueError, match="bf16 model"):
        GemmaDecodePlan(m, [], 1, weight_dtype="fp8")
    with pytest.raises(ValueError, match="batch 1"):
        GemmaDecodePlan(m.to(torch.bfloat16), [], 2, weight_dtype="fp8")
