"""fp8 e4m3 KV pages, host side: the quantisation rule itself (the torch lines of include/vyom_hip.h), the manager's
pages and scales, the C ABI of the three fp8 entry points and the engine's constructor checks -- all without a GPU."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import vyomai_amd as V
from vyomai_amd import _lib, ops

F8 = torch.float8_e4m3fn
NEW = ("vy_paged_rope_write_fp8", "vy_attn_paged_decode_fp8", "vy_attn_paged_decode_fp8_ws_bytes",
       "vy_attn_paged_prefill_fp8")


def quantise(x):
    """The rule: x (..., dh) fp32 values a bf16 page would hold -> (codes e4m3fn (..., dh), scales fp32 (...,))."""
    amax = x.abs().amax(dim=-1)
    s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (x / s.unsqueeze(-1)).clamp(-448, 448).to(F8), s


def config(**kw):
    base = dict(vocab_size=64, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=1, max_position_embeddings=128)
    base.update(kw)
    return V.Config(**base)


# ---- the reference quantiser -------------------------------------------------------------------------------------


def test_quantiser_zero_head_amax_code_round_trip_and_signed_zero():
    codes, s = quantise(torch.zeros(3, 64))
    assert (s == 1).all() and (codes.view(torch.uint8) == 0).all()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(50, 64, generator=g).bfloat16().float() * torch.tensor([0.25, 1.0, 4.0, 1.0, 0.25]).repeat(10)[:, None]
    x[0, 3] = -0.0
    x[1, 5] = 0.0
    codes, s = quantise(x)
    raw = codes.view(torch.uint8)
    amax = x.abs().amax(dim=-1)
    at = x.abs().argmax(dim=-1)
    top = raw[torch.arange(50), at]
    assert ((top & 0x7F) == 126).all()                                   # 448 = 0x7E, with the element's sign
    assert ((top >> 7).bool() == (x[torch.arange(50), at] < 0)).all()
    back = codes.float() * s[:, None]
    assert ((back - x).abs() <= 2.0 ** -4 * amax[:, None]).all()
    assert raw[0, 3] == 0x80 and raw[1, 5] == 0x00
    # the two values the rule was checked on: the top binade's first step, and a tie at the bottom
    assert torch.tensor([448.0, 464.0]).to(F8).view(torch.uint8).tolist() == [126, 126]
    assert torch.tensor([2.0 ** -10]).to(F8).view(torch.uint8).item() == 0


# ---- the manager -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("spelling", ["fp8", "fp8_e4m3", F8])
def test_fp8_manager_pages_scales_and_bytes(spelling):
    cfg = config()
    nb, bs, hk, dh, layers = 5, 16, 1, 32, 2
    mgr = V.PagedKVManager(cfg, nb, bs, "cpu", torch.bfloat16, kv_cache_dtype=spelling)
    assert len(mgr.k_cache) == len(mgr.v_cache) == len(mgr.k_scale) == len(mgr.v_scale) == layers
    for i in range(layers):
        for pages, scales in ((mgr.k_cache[i], mgr.k_scale[i]), (mgr.v_cache[i], mgr.v_scale[i])):
            assert pages.dtype == F8 and pages.shape == (nb, bs, hk, dh) and pages.is_contiguous()
            assert scales.dtype == torch.float32 and scales.shape == (nb, bs, hk)
    assert mgr.kv_bytes == 2 * layers * nb * bs * hk * (dh + 4)
    plain = V.PagedKVManager(cfg, nb, bs, "cpu", torch.bfloat16)
    assert plain.k_scale is None and plain.v_scale is None and plain.k_cache[0].dtype == torch.bfloat16
    assert plain.kv_bytes == 2 * layers * nb * bs * hk * dh * 2
    assert mgr.kv_bytes * 2 * dh == plain.kv_bytes * (dh + 4)             # (dh + 4) / (2 dh) of the bf16 bytes
    # blocks are blocks: the same allocation on both
    for m in (mgr, plain):
        s = V.SequenceState(0, list(range(1, 21)), 4, bs, "cpu")
        m.allocate(s)
        assert s.block_table[:2].tolist() == [0, 1] and set(m.block_to_node) == {0}
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        V.PagedKVManager(cfg, nb, bs, "cpu", torch.bfloat16, kv_cache_dtype="int8")


# ---- ABI ---------------------------------------------------------------------------------------------------------


def test_header_binding_and_library_agree_on_the_fp8_symbols():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    declared = set(re.findall(r"\b(vy_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.ALL_SYMBOLS and hasattr(lib, name), name
        if name in _lib.PROTOTYPES:      # as many argtypes as the header's prototype has parameters
            proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
            assert len(_lib.PROTOTYPES[name]) == proto.count(",") + 1, name
    assert _lib.load().vy_abi_version() == 5


def _buf():
    raw = (ctypes.c_char * 8192)()
    return raw, (ctypes.addressof(raw) + 255) // 256 * 256


def test_fp8_argument_errors_are_reported_without_a_gpu():
    raw, p = _buf()

    def rope(block_size=16, dh=64, qkv=p, ks=p, vs=p, dtype=1, qn=None, kn=None):
        _lib.call("vy_paged_rope_write_fp8", qkv, 256, p, p, p, p, 8, qn, kn, 1e-6, p, p, ks, vs, 4, block_size, 4, 2, 1,
                  dh, dtype, None)

    def decode(block_size=16, dh=64, q=p, ks=p, vs=p, dtype=1, n_split=0):
        _lib.call("vy_attn_paged_decode_fp8", q, 256, None, p, p, ks, vs, 4, block_size, p, 4, p, 16, p, 256, 2, 2, 1, dh,
                  0.125, n_split, None, 0, dtype, None)

    def prefill(block_size=16, dh=64, q=p, ks=p, vs=p, dtype=1):
        _lib.call("vy_attn_paged_prefill_fp8", q, 256, p, p, ks, vs, 4, block_size, p, 4, p, p, 2, 8, 24, p, 256, 2, 1, dh,
                  0.125, dtype, None)

    for fn in (rope, decode, prefill):
        for bad in (12, 4, 512):
            with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*block_size"):
                fn(block_size=bad)
        for bad in (60, 264, 0):
            with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*multiple of 8"):
                fn(dh=bad)
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
            fn(ks=None)
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
            fn(vs=None)
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*dtype"):
            fn(dtype=0)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
        rope(qkv=None)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
        rope(qn=p)                           # the norm weights come as a pair or not at all
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
        decode(q=None)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
        prefill(q=None)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*workspace"):
        decode(n_split=2)                    # a pinned split needs its workspace
    lib = _lib.load()
    assert lib.vy_attn_paged_decode_fp8_ws_bytes(2, 4, 2, 64, 1300, 1, 1) == 0
    assert lib.vy_attn_paged_decode_fp8_ws_bytes(2, 4, 2, 64, 1300, 5, 1) == 2 * 4 * 5 * (64 + 2) * 4
    assert lib.vy_attn_paged_decode_fp8_ws_bytes(2, 4, 2, 64, 1300, 5, 0) == 0


def test_wrappers_pair_fp8_pages_with_scales():
    q = torch.zeros(2, 128, dtype=torch.bfloat16)
    bt, sl = torch.zeros((2, 2), dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    pages = torch.zeros(4, 16, 1, 64, dtype=torch.uint8).view(F8)
    sc = torch.zeros(4, 16, 1)
    with pytest.raises(ValueError, match="need k_scale"):
        ops.attention_paged_decode(q, pages, pages, bt, sl, 1, 2)
    with pytest.raises(ValueError, match="need k_scale"):
        ops.attention_paged_decode(q, pages, pages, bt, sl, 1, 2, k_scale=sc)
    with pytest.raises(ValueError, match="float32"):
        ops.attention_paged_decode(q, pages, pages, bt, sl, 1, 2, k_scale=sc, v_scale=sc[:, :8])
    with pytest.raises(ValueError, match="bfloat16 step"):
        ops.attention_paged_decode(q.float(), pages, pages, bt, sl, 1, 2, k_scale=sc, v_scale=sc)
    bf = torch.zeros(4, 16, 1, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="belong to fp8 pages"):
        ops.attention_paged_decode(q, bf, bf, bt, sl, 1, 2, k_scale=sc, v_scale=sc)
    with pytest.raises(ValueError, match="belong to fp8 pages"):
        ops.attention_paged_prefill(q, bf, bf, bt, torch.zeros(3, dtype=torch.int32), sl, 1, 1, 2, k_scale=sc, v_scale=sc)
    with pytest.raises(_lib.VyomHipError, match="CPU tensor"):          # a well-formed call gets as far as the device check
        ops.attention_paged_decode(q, pages, pages, bt, sl, 1, 2, k_scale=sc, v_scale=sc)


# ---- the engine --------------------------------------------------------------------------------------------------


def test_engine_refuses_fp8_pages_without_varlen_prefill_or_bf16():
    cfg = config()
    model = V.ModelForCausalLM(cfg)                       # fp32 parameters, no compute dtype: computes in fp32
    mgr = V.PagedKVManager(cfg, 4, 8, "cpu", torch.bfloat16, kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="varlen_prefill"):
        V.ContinuousBatchEngine(None, mgr)
    with pytest.raises(ValueError, match="varlen_prefill"):
        V.ContinuousBatchEngine(None, mgr, varlen_prefill=False)
    with pytest.raises(ValueError, match="bfloat16"):
        V.ContinuousBatchEngine(model, mgr, varlen_prefill=True)
    with pytest.raises(ValueError, match="bfloat16"):
        V.ContinuousBatchEngine(None, V.PagedKVManager(cfg, 4, 8, "cpu", torch.float32, kv_cache_dtype="fp8"),
                                varlen_prefill=True)
    model.compute_dtype = model.model.compute_dtype = torch.bfloat16
    for kw in (dict(varlen_prefill=True), dict(max_step_tokens=8), dict(varlen_prefill=True, max_step_tokens=8)):
        eng = V.ContinuousBatchEngine(model, mgr, **kw)
        assert eng.varlen_prefill and eng.kv_mgr is mgr
