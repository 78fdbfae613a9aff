"""CPU-only checks of the RMSNorm + SwiGLU causal LM (models/custom_transformer.py): state_dict layout against the
reference's key list (tests/golden/causal_lm.npz), the strict load that drops the reference's dead trunk, the tied
table, Config defaults, the new C entry points' declarations and argument checks, and the loud failure without a
GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.golden import cases_causal_lm as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VY_ERR_ARG, VY_ERR_UNSUPPORTED = -1, -2


def small():
    import vyomai_amd as V
    return V.ModelForCausalLM(V.Config(**C.CASES["a"]))


def test_fixture_holds_arrays_only(golden):
    g = golden("causal_lm")
    for k, v in g.items():
        assert v.dtype.kind in ("f", "i", "U"), (k, v.dtype)
        assert (v.dtype.kind == "U") == (k in ("ref.keys", "cfg.names", "cfg.values")), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "causal_lm.npz")) < 1_000_000


def test_state_dict_is_the_reference_without_its_dead_trunk(golden):
    m = small()
    ref_keys = set(golden("causal_lm")["ref.keys"].tolist())
    own = set(m.state_dict().keys())
    assert all(k.startswith("model.") or k == "lm_head.weight" for k in own)
    dead = m.dead_trunk_keys()
    # the dead trunk is the top-level copy of model.*: exactly what the reference has and this model lacks
    assert dead == {k[len("model."):] for k in own if k.startswith("model.")}
    assert ref_keys - own == dead and own - ref_keys == set()
    assert not any(n.split(".")[0] in ("embed_tokens", "layers", "norm") for n, _ in m.named_parameters())


def test_strict_load_of_a_reference_keyed_dict(golden):
    m = small()
    own = m.state_dict()
    sd = {}
    for k in golden("causal_lm")["ref.keys"].tolist():
        live = k if k in own else "model." + k
        sd[k] = torch.full_like(own[live], 0.25 if k in own else 7.0)     # the dead trunk carries other values
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(bool((t == 0.25).all()) for t in m.state_dict().values())
    # strict still means strict: a key that is neither live nor the dead trunk's is refused, a missing live key too
    with pytest.raises(RuntimeError, match="Unexpected"):
        m.load_state_dict(dict(sd, **{"model.extra.weight": torch.zeros(1)}), strict=True)
    with pytest.raises(RuntimeError, match="Missing"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "model.norm.weight"}, strict=True)


def test_lm_head_is_the_embedding_table():
    m = small()
    assert m.lm_head.weight is m.model.embed_tokens.weight
    assert m.lm_head.bias is None
    assert m.get_output_embeddings() is m.lm_head and m.get_input_embeddings() is m.model.embed_tokens
    assert sum(1 for _ in m.parameters()) == len(m.state_dict()) - 1    # one parameter under two names
    assert m.model.embed_tokens.padding_idx == 0


def test_config_defaults_equal_the_reference(golden):
    import vyomai_amd as V
    g = golden("causal_lm")
    c = V.Config()
    for name, value in zip(g["cfg.names"].tolist(), g["cfg.values"].tolist()):
        assert repr(getattr(c, name)) == value, (name, getattr(c, name), value)
    assert V.Config(num_key_value_heads=None).num_key_value_heads == 4
    assert V.Config(extra_field=3).extra_field == 3
    a = V.Attention(c, 0)
    assert a.head_dim == 224 and a.q_proj.bias is not None and a.o_proj.bias is None


def test_reference_names_are_exported():
    import vyomai_amd as V
    from vyomai_amd.models import custom_transformer as ct
    for name in ("Config", "MLP", "Attention", "RMSNorm", "DecoderLayer", "BaseModel", "ModelForCausalLM"):
        assert getattr(V, name) is getattr(ct, name)
    src = open(ct.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+transformers", src, re.M)


def test_new_symbols_are_declared_and_exported():
    from vyomai_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vyom_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vy_rmsnorm_bwd", "vy_gated_act_bwd"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES and name in _lib.ALL_SYMBOLS
        assert hasattr(lib, name)
        # one ctypes argument per parameter of the header's prototype
        proto = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(_lib.PROTOTYPES[name]) == proto.count(",") + 1, name
    assert _lib.load().vy_abi_version() == 5


def _aligned_buffer():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_argument_errors_of_the_new_kernels_without_a_gpu():
    """Validation comes before any launch: nothing below reaches the device."""
    from vyomai_amd import _lib
    lib = _lib.load()
    buf, p = _aligned_buffer()
    none = None
    # vy_rmsnorm_bwd(dy, lddy, x, ldx, w, add_to, ldadd, dx, lddx, dw, beta, ws, M, N, eps, w_offset, dtype, stream)
    ok = [p, 64, p, 64, p, none, 0, p, 64, p, 0.0, p, 4, 64, 1e-6, 0.0, _lib.VY_BF16, none]
    for i in (0, 2, 4, 7, 9, 11):        # each required operand NULL in turn
        a = list(ok)
        a[i] = none
        assert lib.vy_rmsnorm_bwd(*a) == VY_ERR_ARG, i
        assert b"null operand" in lib.vy_last_error()
    for i, v in ((1, 60), (3, 60), (8, 60), (13, 60), (6, 60)):     # row strides / N that are not whole 16-byte chunks
        a = list(ok)
        a[i] = v
        if i == 6:
            a[5] = p
        assert lib.vy_rmsnorm_bwd(*a) == VY_ERR_ARG, i
        assert b"multiples of 8" in lib.vy_last_error()
    for i in (0, 2, 4, 7):               # operands off the 16-byte grid
        a = list(ok)
        a[i] = p + 2
        assert lib.vy_rmsnorm_bwd(*a) == VY_ERR_ARG, i
        assert b"16-byte aligned" in lib.vy_last_error()
    a = list(ok)
    a[10] = 0.5
    assert lib.vy_rmsnorm_bwd(*a) == VY_ERR_ARG and b"beta" in lib.vy_last_error()
    a = list(ok)
    a[16] = 7
    assert lib.vy_rmsnorm_bwd(*a) == VY_ERR_ARG and b"dtype" in lib.vy_last_error()
    # vy_gated_act_bwd(d_act, lddo, gate_up, ldg, d_gate_up, lddg, M, I, act, dtype, stream)
    ok = [p, 64, p, 128, p, 128, 4, 64, _lib.ACT_SILU, _lib.VY_BF16, none]
    for i in (0, 2, 4):
        a = list(ok)
        a[i] = none
        assert lib.vy_gated_act_bwd(*a) == VY_ERR_ARG, i
        assert b"null operand" in lib.vy_last_error()
    for i, v in ((1, 68), (3, 132), (5, 132), (7, 60)):
        a = list(ok)
        a[i] = v
        assert lib.vy_gated_act_bwd(*a) == VY_ERR_ARG, i
        assert b"multiples of 8" in lib.vy_last_error()
    a = list(ok)
    a[3] = 64                            # gate_up rows narrower than 2 I
    assert lib.vy_gated_act_bwd(*a) == VY_ERR_ARG and b"row stride" in lib.vy_last_error()
    a = list(ok)
    a[2] = p + 2
    assert lib.vy_gated_act_bwd(*a) == VY_ERR_ARG and b"16-byte aligned" in lib.vy_last_error()
    for act in (_lib.ACT_NONE, 8, 0x40, _lib.ACT_SILU | _lib.ACT_SAVE_DERIV):
        a = list(ok)
        a[8] = act
        assert lib.vy_gated_act_bwd(*a) == VY_ERR_ARG and b"unsupported act" in lib.vy_last_error()
    del buf


def test_forward_launchers_refuse_a_row_stride_below_the_row_width():
    """vy_rmsnorm_fwd and vy_gated_act_fwd refuse what their backward launchers refuse: rows that would overlap.
    Validation comes before any launch: nothing below reaches the device."""
    from vyomai_amd import _lib
    lib = _lib.load()
    buf, p = _aligned_buffer()
    for dtype, vec in ((_lib.VY_BF16, 8), (_lib.VY_F32, 4)):
        # vy_rmsnorm_fwd(x, ldx, w, y, ldy, M, N, eps, w_offset, dtype, stream)
        for ldx, ldy in ((64 - vec, 64), (64, 64 - vec), (0, 64)):
            assert lib.vy_rmsnorm_fwd(p, ldx, p, p, ldy, 4, 64, 1e-6, 1.0, dtype, None) == VY_ERR_ARG, (ldx, ldy)
            assert b"vy_rmsnorm_fwd: row stride below" in lib.vy_last_error(), lib.vy_last_error()
        # vy_gated_act_fwd(gate_up, ldg, out, ldo, M, I, act, dtype, stream)
        for ldg, ldo in ((128 - vec, 64), (64, 64), (128, 64 - vec), (128, 0)):
            assert lib.vy_gated_act_fwd(p, ldg, p, ldo, 4, 64, _lib.ACT_SILU, dtype, None) == VY_ERR_ARG, (ldg, ldo)
            assert b"vy_gated_act_fwd: row stride below" in lib.vy_last_error(), lib.vy_last_error()
    del buf


def test_rmsnorm_launchers_refuse_one_chunk_past_the_widest_row():
    """8200 (bf16) / 8196 (fp32) forward, 8200 / 4100 backward: "too wide", on the host."""
    from tests import prenorm_cases as P
    from vyomai_amd import _lib
    lib = _lib.load()
    buf, p = _aligned_buffer()
    for dtype in P.DTYPES:
        code = _lib.dtype_code(dtype)
        N = P.RMS_FWD_TOO_WIDE[dtype]
        assert lib.vy_rmsnorm_fwd(p, N, p, p, N, 4, N, 1e-6, 1.0, code, None) == VY_ERR_UNSUPPORTED, N
        assert b"too wide" in lib.vy_last_error()
        N = P.RMS_BWD_TOO_WIDE[dtype]
        # vy_rmsnorm_bwd(dy, lddy, x, ldx, w, add_to, ldadd, dx, lddx, dw, beta, ws, M, N, eps, w_offset, dtype, stream)
        assert lib.vy_rmsnorm_bwd(p, N, p, N, p, None, 0, p, N, p, 0.0, p, 4, N, 1e-6, 1.0, code, None) == VY_ERR_UNSUPPORTED, N
        assert b"too wide" in lib.vy_last_error()
    del buf


def test_gated_act_fwd_admits_every_activation_code():
    """vy_gated_act_fwd(gate_up, ldg, out, ldo, M, I, act, dtype, stream): the activation is judged before the
    strides, so a call with a known code and a bad stride fails on the STRIDE -- without a GPU that is as far as a
    call can go -- and an unknown code fails on the code."""
    from vyomai_amd import _lib
    lib = _lib.load()
    buf, p = _aligned_buffer()
    codes = (_lib.ACT_GELU_ERF, _lib.ACT_GELU_TANH, _lib.ACT_SILU, _lib.ACT_TANH, _lib.ACT_SIGMOID, _lib.ACT_RELU6,
             _lib.ACT_LEAKY_RELU)
    for act in codes:
        assert lib.vy_gated_act_fwd(p, 132, p, 64, 4, 64, act, _lib.VY_BF16, None) == VY_ERR_ARG
        assert b"multiples of 8" in lib.vy_last_error(), (act, lib.vy_last_error())
    for act in (_lib.ACT_NONE, 8, 0x40):
        assert lib.vy_gated_act_fwd(p, 132, p, 64, 4, 64, act, _lib.VY_BF16, None) == VY_ERR_ARG
        assert b"unsupported act" in lib.vy_last_error(), (act, lib.vy_last_error())
    del buf


def test_no_cpu_fallback():
    import vyomai_amd as V
    from vyomai_amd._lib import VyomHipError
    m = small().eval()
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(VyomHipError, match="MI355X"):
        m(ids)
    with pytest.raises(VyomHipError, match="MI355X"):
        m.clm_loss(ids, ids)
    with pytest.raises(VyomHipError, match="MI355X"):
        m.generate(ids, max_new_tokens=2)
    with pytest.raises(VyomHipError, match="MI355X"):
        m.model.layers[0](torch.zeros(1, 4, 256))
    with pytest.raises(VyomHipError, match="MI355X"):
        V.RMSNorm(256)(torch.zeros(1, 4, 256))


def test_flat_arena_lays_the_packed_projections_out_adjacently():
    """The trainer's arenas keep q/k/v (weights, then biases) and gate/up back to back, so the packed GEMMs and their
    weight gradients run on views; the tied table is registered once."""
    from vyomai_amd.training import FlatArena
    m = small()
    arena = FlatArena(m, shadow_dtype=torch.bfloat16)
    names = [n for n, _ in arena.items]
    assert names.count("model.embed_tokens.weight") == 1 and "lm_head.weight" not in names
    for layer in m.model.layers:
        a, mlp = layer.self_attn, layer.mlp
        ws = [a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]
        for x, y in zip(ws, ws[1:]):
            assert y.data_ptr() == x.data_ptr() + x.numel() * 4 and y.grad.data_ptr() == x.grad.data_ptr() + x.numel() * 4
        g, u = mlp.gate_proj.weight, mlp.up_proj.weight
        assert u.data_ptr() == g.data_ptr() + g.numel() * 4 and u.grad.data_ptr() == g.grad.data_ptr() + g.numel() * 4
        packed = mlp._packed_gate_up(torch.bfloat16)
        assert packed.shape == (2 * g.shape[0], g.shape[1]) and packed.data_ptr() == g._vy_shadow[1].data_ptr()
        assert torch.equal(packed.float(), torch.cat([g, u]).detach().to(torch.bfloat16).float())
