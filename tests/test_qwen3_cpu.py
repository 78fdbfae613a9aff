"""Qwen3Model without a GPU: the new symbol in header, binding and library, the state dict against the reference's key
list (tests/golden/qwen3.npz, made by make_golden_qwen3.py), load_weights_into_qwen's name mapping, the config view the
paged-KV manager reads, and the argument rules of vy_paged_qknorm_rope_write."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import vyomai_amd as V
from tests.golden import cases_qwen3 as C
from vyomai_amd import _lib
from vyomai_amd.models import qwen3

NAME = "vy_paged_qknorm_rope_write"
GOLDEN = Path(__file__).resolve().parent / "golden" / "qwen3.npz"


def test_header_binding_and_library_agree_on_the_new_symbol():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    declared = set(re.findall(r"\b(vy_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert NAME in declared and NAME in _lib.ALL_SYMBOLS and NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    proto = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(_lib.PROTOTYPES[NAME]) == proto.count(",") + 1 == 20
    assert _lib.load().vy_abi_version() == 5       # additive symbol: the ABI version stays


def test_argument_errors_are_reported_without_a_gpu():
    raw = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(raw) + 255) // 256 * 256

    def call(block_size=16, dh=64, qkv=p, q_scale=p, k_scale=p, eps=1e-6, ld=256, dtype=1):
        _lib.call(NAME, qkv, ld, p, p, p, p, 8, q_scale, k_scale, eps, p, p, 4, block_size, 4, 2, 1, dh, dtype, None)

    for kw in (dict(block_size=12), dict(block_size=512), dict(dh=60), dict(dh=264), dict(qkv=None), dict(q_scale=None),
               dict(k_scale=None), dict(q_scale=p + 4), dict(qkv=p + 8), dict(eps=-1.0), dict(eps=float("nan")),
               dict(ld=252), dict(ld=257), dict(dtype=7)):
        with pytest.raises(_lib.VyomHipError, match=NAME):
            call(**kw)


@pytest.mark.parametrize("case", list(C.CASES))
def test_state_dict_keys_are_the_references(golden, case):
    m = C.build(V.Qwen3Model, case, torch.float32)
    assert sorted(m.state_dict().keys()) == golden("qwen3")[f"{case}.keys"].tolist()
    assert ("trf_blocks.0.att.q_norm.scale" in m.state_dict()) == bool(C.CASES[case]["qk_norm"])


def test_parameter_dtypes_and_a_strict_round_trip():
    cfg = C.cfg("q", torch.bfloat16)
    m = V.Qwen3Model(cfg)
    sd = m.state_dict()
    for k, v in sd.items():
        assert v.dtype == (torch.float32 if k.endswith(".scale") else torch.bfloat16), k
    assert sd["cos_buf"].shape == (cfg["context_length"], cfg["head_dim"] // 2)
    other = V.Qwen3Model(cfg)
    assert other.load_state_dict(sd, strict=True).missing_keys == []
    assert m.tok_emb.weight.shape == (512, 256) and m.trf_blocks[0].att.W_query.weight.shape == (512, 256)
    assert m.trf_blocks[1].att.out_proj.weight.shape == (256, 512) and m.out_head.weight is not m.tok_emb.weight
    assert isinstance(m.trf_blocks[0].norm1, qwen3.RMSNorm) and qwen3.RMSNorm(8, bias=True).shift.shape == (8,)


def test_config_view():
    raw = C.cfg("q", torch.float32)
    c = V.Qwen3Model(raw).config
    assert (c.num_key_value_heads, c.head_dim, c.hidden_size, c.num_hidden_layers, c.num_attention_heads) == \
        (raw["n_kv_groups"], raw["head_dim"], raw["emb_dim"], raw["n_layers"], raw["n_heads"])
    mgr = V.PagedKVManager(c, max_blocks=3, block_size=8)
    assert len(mgr.k_cache) == 2 and mgr.k_cache[0].shape == (3, 8, 2, 128)      # head_dim is not emb_dim / n_heads


def _hf_dict(m, tied):
    """A Hugging Face-named dict of fresh random tensors shaped like m's parameters."""
    g = torch.Generator().manual_seed(5)
    names = {"tok_emb.weight": "model.embed_tokens.weight", "final_norm.scale": "model.norm.weight",
             "out_head.weight": "lm_head.weight"}
    for l in range(len(m.trf_blocks)):
        for mine, theirs in (("att.W_query", "self_attn.q_proj"), ("att.W_key", "self_attn.k_proj"),
                             ("att.W_value", "self_attn.v_proj"), ("att.out_proj", "self_attn.o_proj"),
                             ("ff.fc1", "mlp.gate_proj"), ("ff.fc2", "mlp.up_proj"), ("ff.fc3", "mlp.down_proj")):
            names[f"trf_blocks.{l}.{mine}.weight"] = f"model.layers.{l}.{theirs}.weight"
        for mine, theirs in (("att.q_norm", "self_attn.q_norm"), ("att.k_norm", "self_attn.k_norm"),
                             ("norm1", "input_layernorm"), ("norm2", "post_attention_layernorm")):
            names[f"trf_blocks.{l}.{mine}.scale"] = f"model.layers.{l}.{theirs}.weight"
    params = {names[n]: torch.randn(p.shape, generator=g) for n, p in m.named_parameters()}
    if tied:
        del params["lm_head.weight"]
    return names, params


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_load_weights_into_qwen(tied):
    cfg = C.cfg("q", torch.bfloat16)
    m = V.Qwen3Model(cfg)
    names, params = _hf_dict(m, tied)
    V.load_weights_into_qwen(m, cfg, params)
    assert (m.out_head.weight is m.tok_emb.weight) == tied
    for n, p in m.named_parameters():
        assert p.dtype == (torch.float32 if n.endswith(".scale") else torch.bfloat16), n
        assert torch.equal(p, params[names[n]].to(p.dtype)), n
    assert len(dict(m.named_parameters())) == len(params)


def test_load_weights_mismatch_names_the_tensor():
    cfg = C.cfg("r", torch.float32)
    m = V.Qwen3Model(cfg)
    _, params = _hf_dict(m, False)
    bad = "model.layers.1.self_attn.k_norm.weight"
    params[bad] = torch.zeros(32)
    with pytest.raises(ValueError, match=re.escape(bad)):
        V.load_weights_into_qwen(m, cfg, params)
    _, params = _hf_dict(m, False)
    del params["model.layers.0.mlp.up_proj.weight"]
    with pytest.raises(KeyError, match="model.layers.0.mlp.up_proj.weight"):
        V.load_weights_into_qwen(m, cfg, params)


def test_forward_needs_the_gpu_and_the_paged_protocol():
    m = C.build(V.Qwen3Model, "t", torch.float32)
    with pytest.raises(_lib.VyomHipError):
        m(torch.zeros(3, dtype=torch.long), [], [], {})
    with pytest.raises(_lib.VyomHipError):
        m.forward_paged(torch.zeros(3, dtype=torch.long), None, {"max_position": 3}, None)


def test_golden_file_is_small():
    assert GOLDEN.stat().st_size < 1_000_000
