"""LoRA fine-tuning without a GPU: the LoraLinear wrapper and add_lora / lora_state_dict / merge_lora / disable_lora,
every refusal by its message, the identity tile table, and the argument checks of the new ops entries and of
vy_lora_wgrad itself (they come before any launch)."""
import ctypes

import pytest
import torch

import vyomai_amd as V
from tests.golden import cases_causal_lm as C
from tests.golden import cases_lora as L
from vyomai_amd import _lib, adapters, lora_train, ops
from vyomai_amd._lib import VyomHipError

KW = C.CASES[L.CASE]


def model():
    m = V.ModelForCausalLM(V.Config(**KW))
    C.load_weights_(m)
    return m


def test_lora_linear_attributes_and_init():
    torch.manual_seed(0)
    lin = torch.nn.Linear(512, 256, bias=True)
    m = V.LoraLinear(lin, rank=32, alpha=2)
    assert m.linear is lin and (m.in_features, m.out_features, m.rank, m.alpha) == (512, 256, 32, 2)
    assert tuple(m.lora_a.shape) == (32, 512) and tuple(m.lora_b.shape) == (256, 32)
    assert isinstance(m.dropout, torch.nn.Dropout) and m.dropout.p == 0.0
    assert m.weight is lin.weight and m.bias is lin.bias and m.enabled
    assert sorted(m.state_dict()) == ["linear.bias", "linear.weight", "lora_a", "lora_b"]
    assert bool((m.lora_b == 0).all())
    a = m.lora_a.detach()
    # randn / sqrt(rank) over 16384 values: mean 0 +- 4 sigma / sqrt(n), std 1 / sqrt(32) within 5 %
    assert abs(float(a.mean())) < 4 * 32 ** -0.5 / 128 and abs(float(a.std()) * 32 ** 0.5 - 1) < 0.05
    d = V.LoraLinear(torch.nn.Linear(64, 32))
    assert (d.rank, d.alpha) == (32, 1)


def test_lora_linear_refusals():
    lin = torch.nn.Linear(64, 32)
    for kw, match in ((dict(lora_dropout=0.1), "lora_dropout 0.1"), (dict(rank=0), "rank 0 must be"), (dict(rank=65), "rank 65 must be")):
        with pytest.raises(ValueError, match=match):
            V.LoraLinear(lin, **kw)
    with pytest.raises(ValueError, match="in_features 40 must be a multiple of 32"):
        V.LoraLinear(torch.nn.Linear(40, 32))
    with pytest.raises(ValueError, match="out_features 24 a multiple of 16"):
        V.LoraLinear(torch.nn.Linear(64, 24))
    with pytest.raises(ValueError, match="wraps an nn.Linear"):
        V.LoraLinear(V.LoraLinear(lin))
    with pytest.raises(VyomHipError, match="CPU tensor"):
        V.LoraLinear(lin)(torch.zeros(2, 64))


def test_add_lora_keys_and_frozen_base(golden):
    g = golden("lora")
    base_keys = set(model().state_dict())
    for who, spec in L.ADAPTERS.items():
        m = V.add_lora(model(), rank=spec["rank"], alpha=spec["alpha"], targets=spec["on"])
        lora_keys = set(g[f"{who}.keys"].tolist())
        renamed = set()
        for k in base_keys:
            path, leaf = k.rsplit(".", 1)
            renamed.add(f"{path}.linear.{leaf}" if path + ".lora_a" in lora_keys else k)
        assert set(m.state_dict()) == renamed | lora_keys
        assert {n for n, p in m.named_parameters() if p.requires_grad} == lora_keys
        assert set(V.lora_state_dict(m)) == lora_keys
        assert m.model.layers[0].self_attn.q_proj.alpha == spec["alpha"]
    # the packed-QKV and gate/up machinery still finds the base weights
    a = m.model.layers[0].self_attn
    assert [tuple(p.shape) for p in a._params()[:3]] == [(256, 256), (128, 256), (128, 256)]
    assert tuple(a._packed()[0].shape) == (512, 256)
    assert tuple(m.model.layers[0].mlp._packed_gate_up(torch.float32).shape) == (1024, 256)


def test_add_lora_refusals():
    m = model()
    with pytest.raises(ValueError, match="targets .* must be a non-empty subset"):
        V.add_lora(m, targets=("self_attn.q_proj", "lm_head"))
    with pytest.raises(ValueError, match="targets .* must be a non-empty subset"):
        V.add_lora(m, targets=())
    with pytest.raises(ValueError, match="rank 65 must be"):
        V.add_lora(m, rank=65)
    assert all(p.requires_grad for p in m.parameters()), "a refused call changes nothing"
    V.add_lora(m, rank=8, targets=("mlp.down_proj",))
    with pytest.raises(ValueError, match="already carries LoRA adapters"):
        V.add_lora(m, rank=8)
    with pytest.raises(ValueError, match="prepares a ModelForCausalLM, not a Linear"):
        V.add_lora(torch.nn.Linear(64, 64))
    with pytest.raises(ValueError, match="prepares a ModelForCausalLM, not a BaseModel"):
        V.add_lora(m.model)


def test_wrapped_model_refuses_the_cached_and_paged_paths():
    m = V.add_lora(model(), rank=8)
    ids = torch.zeros((1, 4), dtype=torch.long)
    for call, what in ((lambda: m.generate(ids), r"generate\(\)"), (lambda: m.forward_paged(ids[0], None, {}, None), r"forward_paged\(\)")):
        with pytest.raises(VyomHipError, match=what) as e:
            call()
        assert "merge_lora" in str(e.value) and "adapters=" in str(e.value)
    with V.disable_lora(m):      # the base model: the guard lets it through to the device check
        with pytest.raises(VyomHipError, match="CPU tensor"):
            m.generate(ids)
    # a projection wrapped outside a model that adds its term itself still refuses
    from vyomai_amd.layers.attention import _SelfAttentionBase
    other = _SelfAttentionBase()
    other._fused_qkv = False
    other.query = V.LoraLinear(torch.nn.Linear(64, 64), rank=8)
    with pytest.raises(VyomHipError, match="not an nn.Linear"):
        other._plain_projections()


def test_state_dict_round_trips_through_the_serving_store():
    torch.manual_seed(1)
    m = V.add_lora(model(), rank=8, alpha=2.0)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_b"):
                p.copy_(torch.randn_like(p))
    sd = V.lora_state_dict(m)
    store = V.LoraAdapters(model(), 2, device="cpu")
    slot = store.load("tuned", sd, 2.0)
    assert store.r_pad == 32 and float(store.alpha[slot]) == 2.0
    for key in {k.rsplit(".", 1)[0] for k in sd}:
        l, g, part = store.where[key]
        _, col, out_f, _ = store.parts[(l, g)][part]
        assert torch.equal(store.A[l][g][slot, part * 32:part * 32 + 8], sd[key + ".lora_a"])
        assert torch.equal(store.B[l][g][slot, col:col + out_f, :8], sd[key + ".lora_b"])
        assert not bool(store.A[l][g][slot, part * 32 + 8:(part + 1) * 32].any())
    # the training side packs the same operands: layout of lora_train.GroupOperands
    G = lora_train.layer_operands(m.model.layers[1], torch.float32, torch.device("cpu"))
    for g in adapters.GROUPS:
        assert torch.equal(G[g].A[0], store.A[1][g][slot]) and torch.equal(G[g].B[0], store.B[1][g][slot])
        assert torch.equal(G[g].At, G[g].A[0].t()) and G[g].bounds == store.boundaries[1][g]
        want = torch.zeros_like(G[g].Bt)
        for p, c0 in enumerate(G[g].cols):
            c1 = G[g].cols[p + 1] if p + 1 < len(G[g].cols) else G[g].N
            want[p * 32:(p + 1) * 32, c0:c1] = G[g].B[0, c0:c1].t()
        assert torch.equal(G[g].Bt, want), "row p * r_pad + j: column j of B_p in part p's columns, zeros elsewhere"
    assert lora_train.layer_operands(m.model.layers[1], torch.float32, torch.device("cpu"))["qkv"] is G["qkv"], "cached"
    with torch.no_grad():
        m.model.layers[1].self_attn.q_proj.lora_a.mul_(2.0)
    assert lora_train.layer_operands(m.model.layers[1], torch.float32, torch.device("cpu"))["qkv"] is not G["qkv"]


def test_merge_lora_and_disable_lora():
    torch.manual_seed(2)
    m = V.add_lora(model(), rank=8, alpha=0.5, targets=("self_attn.v_proj", "mlp.up_proj"))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_b"):
                p.copy_(torch.randn_like(p))
    want = {}
    for l, layer in enumerate(m.model.layers):
        for name, mod in (("self_attn.v_proj", layer.self_attn.v_proj), ("mlp.up_proj", layer.mlp.up_proj)):
            want[f"model.layers.{l}.{name}.weight"] = (mod.linear.weight + 0.5 * mod.lora_b @ mod.lora_a).detach().clone()
    mods = [x for x in m.modules() if isinstance(x, V.LoraLinear)]
    with V.disable_lora(m):
        assert not any(x.enabled for x in mods) and not lora_train.layer_has_lora(m.model.layers[0])
        with V.disable_lora(m):
            assert not any(x.enabled for x in mods)
        assert not any(x.enabled for x in mods), "nested: still disabled after the inner context"
    assert all(x.enabled for x in mods)
    with pytest.raises(RuntimeError, match="boom"):
        with V.disable_lora(m):
            raise RuntimeError("boom")
    assert all(x.enabled for x in mods) and lora_train.layer_has_lora(m.model.layers[0])
    assert V.merge_lora(m) is m
    assert not any(isinstance(x, V.LoraLinear) for x in m.modules())
    assert set(m.state_dict()) == set(model().state_dict())
    sd = m.state_dict()
    for k, w in want.items():
        assert torch.equal(sd[k], w), k
    assert V.lora_state_dict(m) == {}


@pytest.mark.parametrize("T,want", [(1, [[0, 1, 0]]), (16, [[0, 16, 0]]), (17, [[0, 16, 0], [16, 1, 0]]),
                                    (33, [[0, 16, 0], [16, 16, 0], [32, 1, 0]])])
def test_identity_tiles(T, want):
    t = lora_train.identity_tiles(T)
    assert t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == want
    with pytest.raises(ValueError, match="positive integer"):
        lora_train.identity_tiles(0)


def _operands(M=17, K=64, N=48, r_pad=32, parts=3, dtype=torch.float32):
    z = lambda *s: torch.zeros(*s, dtype=dtype)   # noqa: E731
    return dict(dy=z(M, N), u=z(M, parts * r_pad), x=z(M, K), t=z(M, parts * r_pad),
                dA=[torch.zeros(8, K) for _ in range(parts)], dB=[torch.zeros(16, 8) for _ in range(parts)])


def test_host_checks_of_lora_wgrad():
    o = _operands()

    def call(**kw):
        a = dict(o, boundaries=(16, 32), r_pad=32, alpha=1.0, accumulate=False, name="qkv")
        a.update(kw)
        ops.lora_wgrad(a["dy"], a["u"], a["x"], a["t"], a["dA"], a["dB"], a["boundaries"], a["r_pad"], a["alpha"],
                       a["accumulate"], name=a["name"])

    with pytest.raises(VyomHipError, match="CPU tensor"):     # everything valid: only the device is wrong
        call()
    for kw, match in ((dict(x=torch.zeros(17, 48)), r"\(qkv\): K = 48"),
                      (dict(boundaries=(8, 32)), "boundaries"),
                      (dict(boundaries=(16, 32, 40)), "boundaries"),
                      (dict(r_pad=48), "r_pad 48 must be 32 or 64"),
                      (dict(u=torch.zeros(17, 64)), r"u, t \(M, 3 \* r_pad\)"),
                      (dict(u=torch.zeros(17, 96, dtype=torch.bfloat16)), "must share"),
                      (dict(x=torch.zeros(16, 64)), "over the same 17 rows"),
                      (dict(dy=torch.zeros(17, 96)[:, ::2]), "unit column stride"),
                      (dict(dy=torch.zeros(17, 50)[:, :48]), "16-byte aligned"),
                      (dict(dA=o["dA"][:2]), "one entry per part"),
                      (dict(dA=[None] * 3, dB=[None] * 3), "at least one"),
                      (dict(dA=[None] + o["dA"][1:]), "part 0 has one of dA / dB only"),
                      (dict(dA=[torch.zeros(33, 64)] + o["dA"][1:], dB=[torch.zeros(16, 33)] + o["dB"][1:]), "rank 33 of part 0"),
                      (dict(dB=[torch.zeros(16, 4)] + o["dB"][1:]), r"dB\[0\] must be a contiguous float32 \(16, 8\)"),
                      (dict(dA=[torch.zeros(8, 64, dtype=torch.float64)] + o["dA"][1:]), r"dA\[0\] must be")):
        with pytest.raises(ValueError, match=match):
            call(**kw)


def test_host_checks_of_the_delta_and_dgrad_entries():
    M, K, N = 17, 64, 48
    y, x = torch.zeros(M, N), torch.zeros(M, K)
    A, B, al = torch.zeros(1, 96, K), torch.zeros(1, N, 32), torch.ones(1)
    tiles = lora_train.identity_tiles(M)
    with pytest.raises(VyomHipError, match="CPU tensor"):
        ops.lora_delta_keep_u_(y, x, A, B, al, tiles, 2, (16, 32), name="qkv")
    for args, match in (((y, x[:, :48].contiguous(), A, B, al, tiles, 2, (16, 32)), r"\(qkv\): K = 48"),
                        ((y, x, A, B, al, tiles, 2, (8,)), "boundaries"),
                        ((y, x, A, B, al, tiles, 2, (16,)), r"A must be \(1, 2 \* r_pad, 64\)"),
                        ((y, x, torch.zeros(2, 96, K), B, al, tiles, 2, (16, 32)), r"A must be a contiguous \(1, rows, columns\)"),
                        ((y, x, A, B, torch.ones(2), tiles, 2, (16, 32)), "alpha must be"),
                        ((y, x, A, B, al, tiles, 3, (16, 32)), "tiles must be"),
                        ((y, x.double(), A, B, al, tiles, 2, (16, 32)), "must share")):
        with pytest.raises(ValueError, match=match):
            ops.lora_delta_keep_u_(*args, name="qkv")
    dy, dx = torch.zeros(M, 64), torch.zeros(M, K)
    Bt, At = torch.zeros(96, 64), torch.zeros(K, 96)
    with pytest.raises(VyomHipError, match="CPU tensor"):
        ops.lora_dgrad_(dx, dy, Bt, At, al, tiles, 2, name="qkv")
    for args, match in (((dx, torch.zeros(M, 48), torch.zeros(96, 48), At, al, tiles, 2), "N and R multiples of 32"),
                        ((dx, dy, Bt, torch.zeros(K, 64), al, tiles, 2), "needs Bt"),
                        ((torch.zeros(M, 32), dy, Bt, At, al, tiles, 2), "needs Bt"),
                        ((dx, dy, Bt.t(), At, al, tiles, 2), "Bt must be a contiguous"),
                        ((dx, dy, Bt, At, al.double(), tiles, 2), "alpha must be"),
                        ((dx, dy, Bt, At, al, tiles.long(), 2), "tiles must be")):
        with pytest.raises(ValueError, match=match):
            ops.lora_dgrad_(*args, name="qkv")


def test_vy_lora_wgrad_argument_checks_and_chunk_rule():
    """VY_ERR_ARG before any launch (the pointers are never dereferenced on the host); the symbols are additive."""
    lib = _lib.load()
    assert lib.vy_abi_version() == 5
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)            # 16-byte aligned is not guaranteed: align by hand
    p = (p + 15) // 16 * 16
    good = dict(dy=p, lddy=48, u=p, ldu=96, x=p, ldx=64, t=p, ldt=96, dA=[p, p, p], dB=[p, p, p], rank=[8, 8, 8], M=17, N=48,
                K=64, r_pad=32, b0=16, b1=32, alpha=1.0, acc=0, dtype=_lib.VY_F32)

    def rc(**kw):
        a = dict(good)
        a.update(kw)
        return lib.vy_lora_wgrad(a["dy"], a["lddy"], a["u"], a["ldu"], a["x"], a["ldx"], a["t"], a["ldt"], *a["dA"], *a["dB"],
                                 *a["rank"], a["M"], a["N"], a["K"], a["r_pad"], a["b0"], a["b1"], a["alpha"], a["acc"],
                                 a["dtype"], None)

    bad = [dict(dy=None), dict(u=None), dict(x=None), dict(t=None), dict(dA=[None] * 3, dB=[None] * 3), dict(dA=[None, p, p]),
           dict(M=0), dict(K=48), dict(N=40), dict(b0=8), dict(b1=40), dict(b0=16, b1=16), dict(r_pad=16), dict(r_pad=96),
           dict(rank=[0, 8, 8]), dict(rank=[8, 33, 8]), dict(lddy=47), dict(ldx=63), dict(ldu=95), dict(ldx=66),
           dict(dy=p + 4), dict(dtype=7), dict(acc=2), dict(b0=48, b1=48, dA=[p, p, None], dB=[p, p, None])]
    for kw in bad:
        assert rc(**kw) == -1, kw          # VY_ERR_ARG
        assert b"vy_lora_wgrad" in lib.vy_last_error(), kw
    # valid arguments get as far as the workspace check: this stream has none registered in a process without a GPU.
    # Where there is a GPU an earlier test of the same process may have registered one, and the call would launch on
    # these host pointers: it is made only where there is none.
    if not torch.cuda.is_available():
        assert rc() == -1 and b"workspace" in lib.vy_last_error()
    # the cut of M: chunks of at least 128 rows, whole stages of 32, about 1024 workgroups over the column tiles
    assert ops.lora_wgrad_chunk_rows(256, 48, 64) == 128 and ops.lora_wgrad_chunk_rows(257, 1024, 512) == 128
    assert ops.lora_wgrad_chunk_rows(16384, 1152, 896) == 512 and ops.lora_wgrad_chunk_rows(16384, 9728, 896) == 2368
    assert ops.lora_wgrad_chunk_rows(0, 48, 64) == 0
