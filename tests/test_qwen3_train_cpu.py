"""Qwen3Model training without a GPU: the new symbols in header, binding and library, the argument rules of
vy_qknorm_rope_fwd / vy_qknorm_bwd, the module aliases the training functions read, and the fixture file
(tests/golden/qwen3_train.npz, made by make_golden_qwen3_train.py)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import vyomai_amd as V
from tests.golden import cases_qwen3_train as C
from vyomai_amd import _lib

FWD, BWD, WS = "vy_qknorm_rope_fwd", "vy_qknorm_bwd", "vy_qknorm_bwd_ws_floats"
GOLDEN = Path(__file__).resolve().parent / "golden" / "qwen3_train.npz"


def test_header_binding_and_library_agree_on_the_new_symbols():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    declared = set(re.findall(r"\b(vy_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ((FWD, 24), (BWD, 17)):
        assert name in declared and name in _lib.ALL_SYMBOLS and name in _lib.PROTOTYPES and hasattr(lib, name), name
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert len(_lib.PROTOTYPES[name]) == proto.count(",") + 1 == n_args, name
    assert WS in declared and WS in _lib.ALL_SYMBOLS and hasattr(lib, WS)
    assert _lib.load().vy_abi_version() == 5       # additive symbols: the ABI version stays


def test_workspace_size_covers_every_workgroup():
    ws = _lib.load().vy_qknorm_bwd_ws_floats
    assert ws(1, 1, 1, 8) == 16                              # one workgroup, 2 * dh sums
    assert ws(2100, 1, 1, 8) == 17 * 16                      # 4200 units, 256 to a workgroup
    assert ws(150, 4, 2, 64) == 29 * 128                     # 900 units, 32 to a workgroup
    big = ws(16384, 16, 8, 128)
    assert big % 256 == 0 and 3 * 256 <= big <= 1024 * 256   # the slab stays bounded however long the batch
    assert ws(0, 1, 1, 8) == 0 and ws(4, 1, 1, 12) == 0


def _aligned():
    raw = (ctypes.c_char * 8192)()
    return raw, (ctypes.addressof(raw) + 255) // 256 * 256


def test_forward_argument_errors_are_reported_without_a_gpu():
    raw, p = _aligned()

    def call(qkv=p, ld=256, cos=p, table_rows=8, pos0=0, q_scale=p, k_scale=p, eps=1e-6, q=p, q_sl=64, k=p, L=4, h=2, hk=1,
             dh=64, dtype=1):
        _lib.call(FWD, qkv, ld, cos, p, table_rows, pos0, q_scale, k_scale, eps, q, L * h * dh, L * dh, q_sl, k,
                  L * hk * dh, L * dh, dh, 2, L, h, hk, dh, dtype, None)

    for kw in (dict(dh=60), dict(dh=264), dict(h=3, hk=2), dict(ld=248), dict(ld=260), dict(ld=256, dtype=0, dh=64, h=2, hk=2),
               dict(ld=258, dtype=0), dict(qkv=p + 8), dict(q=p + 8), dict(k=p + 4), dict(q_scale=p + 4), dict(k_scale=p + 8),
               dict(cos=p + 4), dict(table_rows=3), dict(pos0=5), dict(dtype=7), dict(qkv=None), dict(q_scale=None),
               dict(k=None), dict(eps=-1.0), dict(eps=float("nan")), dict(q_sl=60)):
        with pytest.raises(_lib.VyomHipError, match=FWD):
            call(**kw)


def test_backward_argument_errors_are_reported_without_a_gpu():
    raw, p = _aligned()

    def call(dqkv=p, ldd=256, qkv=p, ld=256, q_scale=p, k_scale=p, eps=1e-6, dq=p, dk=p, beta=0.0, ws=p, h=2, hk=1, dh=64,
             dtype=1):
        _lib.call(BWD, dqkv, ldd, qkv, ld, q_scale, k_scale, eps, dq, dk, beta, ws, 4, h, hk, dh, dtype, None)

    for kw in (dict(dh=60), dict(dh=264), dict(h=3, hk=2), dict(ld=248), dict(ld=260), dict(ldd=248), dict(ldd=257),
               dict(ldd=258, dtype=0), dict(dqkv=p + 8), dict(qkv=p + 4), dict(q_scale=p + 4), dict(dq=p + 8), dict(dk=p + 4),
               dict(ws=p + 8), dict(ws=None), dict(dtype=7), dict(dqkv=None), dict(k_scale=None), dict(dk=None),
               dict(beta=0.5), dict(eps=-1.0)):
        with pytest.raises(_lib.VyomHipError, match=BWD):
            call(**kw)
    with pytest.raises(_lib.VyomHipError, match="workspace"):
        call(ws=None)


def test_training_entry_points_need_the_gpu():
    m = C.build(V.Qwen3Model, "t", torch.float32)
    ids = torch.zeros((2, 4), dtype=torch.long)
    with pytest.raises(_lib.VyomHipError):
        m.clm_loss(ids, ids)
    with pytest.raises(_lib.VyomHipError):
        m.sequence_logprobs(ids, torch.ones(2, 4))
    with pytest.raises(_lib.VyomHipError):                   # the serving-only forward stays what it was
        m(ids)
    assert V.Qwen3Model.compute_dtype is None


@pytest.mark.parametrize("case", list(C.CASES))
def test_module_aliases_are_the_same_parameters(case):
    m = C.build(V.Qwen3Model, case, torch.float32)
    keys = sorted(m.state_dict().keys())
    n_params = len(list(m.parameters()))
    for blk in m.trf_blocks:
        a, ff = blk.att, blk.ff
        ps = a._params()
        assert len(ps) == 3 and ps[0] is a.W_query.weight and ps[1] is a.W_key.weight and ps[2] is a.W_value.weight
        assert a._fused_qkv is False and a.attention_bias is False
        assert (a.num_attention_heads, a.num_key_value_heads) == (a.num_heads, a.num_kv_groups)
        assert ff.gate_proj is ff.fc1 and ff.up_proj is ff.fc2 and ff.down_proj is ff.fc3
        assert ff.act == _lib.ACT_SILU
        w, b = a._packed()
        assert b is None and torch.equal(w, torch.cat([p.detach() for p in ps]))
        sw, sb = a._packed_shadow(torch.bfloat16)
        assert sb is None and torch.equal(sw, torch.cat([p.detach() for p in ps]).to(torch.bfloat16))
        assert torch.equal(ff._packed_gate_up(torch.float32), torch.cat([ff.fc1.weight.detach(), ff.fc2.weight.detach()]))
    assert sorted(m.state_dict().keys()) == keys and len(list(m.parameters())) == n_params      # no second copy, no new key
    assert not any("gate_proj" in k or "num_" in k for k in keys)


def test_packed_rows_are_a_view_when_the_members_are_adjacent():
    m = C.build(V.Qwen3Model, "q", torch.float32)
    a = m.trf_blocks[0].att
    ps = a._params()
    flat = torch.cat([p.detach().reshape(-1) for p in ps])
    off = 0
    for p in ps:
        p.data = flat[off:off + p.numel()].view(p.shape)
        off += p.numel()
    w = a._packed()[0]
    assert w.data_ptr() == flat.data_ptr() and w.shape == (sum(p.shape[0] for p in ps), ps[0].shape[1])
    with torch.no_grad():
        ps[1].mul_(2.0)
    assert torch.equal(a._packed()[0], torch.cat([p.detach() for p in ps]))


def test_golden_file_is_small_and_holds_the_makers_self_checks(golden):
    assert GOLDEN.stat().st_size < 1_000_000
    g = golden("qwen3_train")
    # the reference alone, as the maker measured it: fp32 against fp64, and its own bf16 against its fp32
    assert float(g["check.worst.f32.grad"]) < 1e-4 and float(g["check.worst.f32.loss"]) < 2e-5
    assert float(g["check.worst.bf16.loss"]) < 3e-2 and 0 < float(g["check.worst.bf16.grad"]) < 3e-2
    for case in C.CASES:
        assert g[f"{case}.train.loss"].shape == (C.TRAIN_STEPS,)
        names = {k[len(case) + 3:] for k in g if k.startswith(f"{case}.d.")}
        assert names == {n for n, _ in C.build(V.Qwen3Model, case, torch.float32).named_parameters()}
        for n in C.trained(case):
            assert f"{case}.train.w.{n}" in g
        for n in names:
            assert f"{case}.gap.d.{n}" in g
    assert {"q.dpo.pi.chosen", "q.dpo.ref.rejected", "q.dpo.loss.1.0", "q.dpo.loss.0.1", "q.dpo.reward.chosen"} <= set(g)
    x, m, y = C.train_batch("q")
    assert m.sum(1).tolist() == list(C.LENGTHS) and (y[m == 0] == -100).all() and (y[0, 12:] == -100).all()
    assert (x[m == 0] == 0).all() and (y[0, :12] == x[0, :12]).all()
