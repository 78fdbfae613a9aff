"""Per-request LoRA adapters without a GPU: the adapter store on the CPU (keys, padding, the packed-part layout, every
refusal), and the engine's planner with model=None -- the tiles of the adapted rows, that a step without an adapted row
uploads what an engine without a store uploads, the prefix cache's salt and the hold counts."""
import numpy as np
import pytest
import torch

import vyomai_amd as V
from vyomai_amd import serving

BS = 8
CFG = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
           num_key_value_heads=1, max_position_embeddings=128, eos_token_id=1)
SHAPES = {"self_attn.q_proj": (64, 64), "self_attn.k_proj": (32, 64), "self_attn.v_proj": (32, 64),
          "self_attn.o_proj": (64, 64), "mlp.gate_proj": (128, 64), "mlp.up_proj": (128, 64), "mlp.down_proj": (64, 128)}
_MODEL = []


def host_model():
    if not _MODEL:
        _MODEL.append(V.ModelForCausalLM(V.Config(**CFG)))
    return _MODEL[0]


def manager(blocks=64):
    return V.PagedKVManager(V.Config(**CFG), blocks, BS, "cpu", torch.float32)


def adapter(rank, on=tuple(SHAPES), seed=0, layers=(0, 1)):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for l in layers:
        for path in on:
            out_f, in_f = SHAPES[path]
            sd[f"model.layers.{l}.{path}.lora_a"] = torch.randn(rank, in_f, generator=g)
            sd[f"model.layers.{l}.{path}.lora_b"] = torch.randn(out_f, rank, generator=g)
    return sd


def store(n=4, max_rank=32, names=("n1", "n2")):
    st = V.LoraAdapters(host_model(), n, max_rank=max_rank, device="cpu")
    for k, name in enumerate(names):
        st.load(name, adapter(8 * (k + 1), seed=k), alpha=1.0 + k)
    return st


def engine(st, **kw):
    kw.setdefault("varlen_prefill", True)
    kw.setdefault("eos_token_ids", [])
    return V.ContinuousBatchEngine(None, manager(), adapters=st, **kw)


def tiles_of(md):
    lora = md.get("lora")
    if lora is None:
        return []
    t = lora["tiles"]
    assert t.dtype == torch.int32 and t.shape == (lora["n_tiles"], 3)
    return [tuple(r) for r in t.tolist()]


def check_tiles(tiles, owner_slot):
    """owner_slot: per row of the packed buffer (sid, slot or None).  The tiles never cross a sequence, never exceed 16
    rows, carry their sequence's slot and cover exactly the adapted rows, each once."""
    seen = []
    for row0, n, slot in tiles:
        assert 1 <= n <= 16
        rows = list(range(row0, row0 + n))
        assert len({owner_slot[r][0] for r in rows}) == 1, "a tile crosses a sequence"
        assert all(owner_slot[r][1] == slot for r in rows)
        seen += rows
    assert sorted(seen) == [r for r, (_, slot) in enumerate(owner_slot) if slot is not None]
    assert len(seen) == len(set(seen))


# ---- tiles -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [15, 16, 17, 33])
def test_prompt_chunk_tiles(n):
    st = store()
    eng = engine(st, max_batch_size=4)
    eng.add_sequence(list(range(3, 3 + n)), 4, adapter="n2")
    eng.add_sequence([5, 6, 7], 4)
    eng.add_sequence(list(range(10, 10 + n)), 4, adapter="n1")
    states, md, ids = eng._plan_step()
    tiles = tiles_of(md)
    owner = [(0, 1)] * n + [(1, None)] * 3 + [(2, 0)] * n
    check_tiles(tiles, owner)
    per = -(-n // 16)
    assert len(tiles) == 2 * per and md["lora"]["adapters"] is st
    assert tiles[:per] == [(r, min(16, n - r), 1) for r in range(0, n, 16)]
    assert tiles[per:] == [(n + 3 + r, min(16, n - r), 0) for r in range(0, n, 16)]


def test_decode_rows_and_chunked_prompts():
    """Decoding rows are tiles of one row; under max_step_tokens a prompt's chunk is cut from the chunk's first row."""
    st = store()
    eng = engine(st, max_batch_size=4, max_step_tokens=24)
    a = eng.add_sequence([3, 4, 5], 6, adapter="n1")
    b = eng.add_sequence([6, 7], 6)
    c = eng.add_sequence([8, 9, 10, 11], 6, adapter="n2")
    states, md, _ = eng._plan_step()
    assert tiles_of(md) == [(0, 3, 0), (5, 4, 1)]
    eng._finish_step(states, [20, 21, 22])
    d = eng.add_sequence(list(range(3, 3 + 40)), 3, adapter="n2")
    states, md, _ = eng._plan_step()                       # three decode rows, then 21 of the 40 prompt tokens
    assert [s.id for s in states] == [a, b, c, d] and states[3].chunk_end == 21
    assert tiles_of(md) == [(0, 1, 0), (2, 1, 1), (3, 16, 1), (19, 5, 1)]
    eng._finish_step(states, [23, 24, 25])
    states, md, _ = eng._plan_step()                       # the rest of the prompt: 19 rows from row 3
    assert tiles_of(md) == [(0, 1, 0), (2, 1, 1), (3, 16, 1), (19, 3, 1)]
    owner = [(a, 0), (b, None), (c, 1)] + [(d, 1)] * 19
    check_tiles(tiles_of(md), owner)


def test_speculative_segments_and_the_drafter_without_tiles():
    st = store()
    eng = V.ContinuousBatchEngine(None, manager(), adapters=st, draft_kv_mgr=manager(), num_speculative_tokens=3,
                                  varlen_prefill=True, eos_token_ids=[], max_batch_size=4)
    eng.add_sequence([3, 4, 5], 9, adapter="n1")
    eng.add_sequence([6, 7], 9)
    eng.add_sequence([8, 9, 10, 11], 9, adapter="n2")
    plan = eng._plan_spec_step()
    assert tiles_of(plan["verify"][0]) == [(0, 3, 0), (5, 4, 1)]
    assert all("lora" not in d[0] for d in plan["draft"])
    eng._finish_spec_step(plan, [[0] * 4] * 3, [[30] * 4, [31] * 4, [32] * 4], [[0] * 3] * 3)
    eng.add_sequence(list(range(3, 3 + 17)), 2, adapter="n1")
    plan = eng._plan_spec_step()                           # three segments of g + 1 = 4 rows, then 17 prompt rows
    md = plan["verify"][0]
    assert tiles_of(md) == [(0, 4, 0), (8, 4, 1), (12, 16, 0), (28, 1, 0)]
    assert md["prefill_varlen"]["cu_q"].tolist() == [0, 4, 8, 12, 29]
    for dmd, *_ in plan["draft"]:
        assert "lora" not in dmd, "the drafter serves base weights"


# ---- a step without an adapted row ------------------------------------------------------------------------------


class _Recorded(serving._StepUploads):
    made = []

    def __init__(self):
        super().__init__()
        _Recorded.made.append(self)


@pytest.mark.parametrize("spec", [False, True], ids=["plain", "speculative"])
def test_a_step_without_adapted_rows_uploads_what_an_engine_without_a_store_uploads(monkeypatch, spec):
    monkeypatch.setattr(serving, "_StepUploads", _Recorded)
    kw = dict(varlen_prefill=True, eos_token_ids=[], max_batch_size=4)
    if spec:
        kw.update(num_speculative_tokens=3)
    engines = [V.ContinuousBatchEngine(None, manager(), adapters=ad, **dict(kw, **({"draft_kv_mgr": manager()} if spec else {})))
               for ad in (None, store())]
    seen = []
    for eng in engines:
        _Recorded.made.clear()
        eng.add_sequence([3, 4, 5, 6, 7], 4, sampling=V.SamplingParams(0.7, seed=3))
        eng.add_sequence(list(range(10, 30)), 4)
        for _ in range(2):
            if spec:
                plan = eng._plan_spec_step()
                assert "lora" not in plan["verify"][0]
                eng._finish_spec_step(plan, [[0] * 4] * 2, [[40] * 4, [41] * 4], [[0] * 2] * 3)
            else:
                states, md, _ = eng._plan_step()
                assert "lora" not in md
                eng._finish_step(states, [40, 41])
        seen.append([(dict(u._l64), dict(u._l32)) for u in _Recorded.made])
    assert len(seen[0]) == 2 and seen[0] == seen[1], "entry for entry, in order"
    assert all("tiles" not in name for l64, l32 in seen[1] for name in list(l64) + list(l32))
    # and with one adapted request the same step has exactly one more entry
    eng = V.ContinuousBatchEngine(None, manager(), adapters=store(), **dict(kw, **({"draft_kv_mgr": manager()} if spec else {})))
    _Recorded.made.clear()
    eng.add_sequence([3, 4, 5, 6, 7], 4, sampling=V.SamplingParams(0.7, seed=3), adapter="n1")
    eng.add_sequence(list(range(10, 30)), 4)
    eng._plan_spec_step() if spec else eng._plan_step()
    l64, l32 = dict(_Recorded.made[0]._l64), dict(_Recorded.made[0]._l32)
    name = "v_tiles" if spec else "tiles"
    assert l32.pop(name) == [0, 5, 0]
    assert (l64, l32) == seen[0][0]


# ---- the prefix cache ------------------------------------------------------------------------------------------


def run_one(eng, prompt, adapter=None, gen=2):
    sid = eng.add_sequence(prompt, gen, adapter=adapter)
    while eng.active or eng.waiting_room:
        states, md, _ = eng._plan_step()
        eng._finish_step(states, [50] * sum(s.query_end == s.num_tokens for s in states))
    return sid


def test_prefix_blocks_are_shared_within_one_adapter_only():
    st = store()
    eng = engine(st, max_batch_size=2)
    prompt = list(range(3, 3 + 21))                        # two whole blocks and five tokens
    first = {who: run_one(eng, prompt, who) for who in (None, "n1", "n2")}
    assert all(eng.prompt_tokens_computed[sid] == 21 for sid in first.values()), "no hit across adapters"
    again = {who: run_one(eng, prompt, who) for who in ("n2", None, "n1")}
    assert all(eng.prompt_tokens_computed[sid] == 21 - 16 for sid in again.values()), "a hit within one adapter"
    mgr = eng.kv_mgr
    chains = {who: mgr.match_prefix(prompt, None if who is None else st.uid[who]) for who in (None, "n1", "n2")}
    assert all(len(c) == 2 for c in chains.values())
    assert len({b for c in chains.values() for b in c}) == 6, "three chains of their own blocks"
    # a name loaded again (other weights) is another adapter: no hit; the old chain is unreachable, not wrong
    old = st.uid["n1"]
    st.unload("n1")
    st.load("n1", adapter(4, seed=9))
    assert st.uid["n1"] != old
    sid = run_one(eng, prompt, "n1")
    assert eng.prompt_tokens_computed[sid] == 21
    assert eng.adapter == {} and eng.sampling == {} and st.held == {"n1": 0, "n2": 0}


def test_salt_none_is_the_tree_as_it_was():
    """Key for key: a manager driven without a salt has only block_size-token keys; a salted chain adds one key of
    block_size + 1 entries under the root and ordinary keys below it."""
    mgr = manager()
    toks = list(range(3, 3 + 20))
    plain = serving.SequenceState(0, toks, 4, BS)
    mgr.allocate(plain)
    assert list(mgr.radix_root.children) == [tuple(toks[:8])]
    assert list(mgr.radix_root.children[tuple(toks[:8])].children) == [tuple(toks[8:16])]
    assert mgr.match_prefix(toks) == mgr.match_prefix(toks, None) == [0, 1]
    assert mgr.match_prefix(toks, 7) == []
    salted = serving.SequenceState(1, toks, 4, BS, salt=7)
    mgr.allocate(salted)
    assert sorted(mgr.radix_root.children, key=len) == [tuple(toks[:8]), (7,) + tuple(toks[:8])]
    node = mgr.radix_root.children[(7,) + tuple(toks[:8])]
    assert list(node.children) == [tuple(toks[8:16])]
    assert mgr.match_prefix(toks, 7) == [3, 4] and mgr.match_prefix(toks) == [0, 1] and mgr.match_prefix(toks, 8) == []


# ---- the store -------------------------------------------------------------------------------------------------


def test_layout_padding_and_packed_parts():
    st = V.LoraAdapters(host_model(), 3, max_rank=40, device="cpu")
    assert st.r_pad == 64 and st.dtype == torch.float32 and st.device.type == "cpu"
    sd = adapter(5, on=("self_attn.q_proj", "self_attn.v_proj", "mlp.up_proj", "mlp.down_proj"), layers=(1,))
    sd["model.layers.1.self_attn.q_proj.linear.weight"] = torch.zeros(64, 64)       # the wrapped base weights: ignored
    sd["model.layers.1.self_attn.q_proj.linear.bias"] = torch.zeros(64)
    sd["model.norm.weight"] = torch.ones(64)
    st.load("first", adapter(3, seed=5))
    slot = st.load("x", sd, alpha=2.5)
    assert slot == 1 and st.slots == {"first": 0, "x": 1} and st.alpha.tolist() == [1.0, 2.5, 0.0]
    A, B = st.A[1]["qkv"], st.B[1]["qkv"]
    assert A.shape == (3, 3 * 64, 64) and B.shape == (3, 64 + 32 + 32, 64) and st.boundaries[1]["qkv"] == (64, 96)
    assert torch.equal(A[1, 0:5], sd["model.layers.1.self_attn.q_proj.lora_a"]) and not A[1, 5:128].any()
    assert torch.equal(A[1, 128:133], sd["model.layers.1.self_attn.v_proj.lora_a"]) and not A[1, 133:].any()
    assert torch.equal(B[1, 0:64, :5], sd["model.layers.1.self_attn.q_proj.lora_b"]) and not B[1, :, 5:].any()
    assert not B[1, 64:96].any(), "the key part was not adapted"
    assert torch.equal(B[1, 96:128, :5], sd["model.layers.1.self_attn.v_proj.lora_b"])
    gu_a, gu_b = st.A[1]["gate_up"], st.B[1]["gate_up"]
    assert gu_a.shape == (3, 128, 64) and gu_b.shape == (3, 256, 64) and st.boundaries[1]["gate_up"] == (128,)
    assert not gu_a[1, :64].any() and torch.equal(gu_a[1, 64:69], sd["model.layers.1.mlp.up_proj.lora_a"])
    assert not gu_b[1, :128].any() and torch.equal(gu_b[1, 128:, :5], sd["model.layers.1.mlp.up_proj.lora_b"])
    assert st.A[1]["down"].shape == (3, 64, 128) and st.B[1]["o"].shape == (3, 64, 64) and st.boundaries[1]["o"] == ()
    assert not st.A[1]["o"][1].any() and not any(t[1].any() for t in st.A[0].values()), "layer 0 was not adapted"
    assert st.A[0]["qkv"][0].any(), "the other slot is untouched"
    # a slot that is used again starts from zeros
    st.unload("first")
    assert st.load("y", adapter(2, on=("mlp.down_proj",), layers=(0,))) == 0
    assert not st.A[0]["qkv"][0].any() and st.A[0]["down"][0, :2].any() and not st.A[0]["down"][0, 2:].any()


def test_load_refusals():
    st = V.LoraAdapters(host_model(), 2, max_rank=8, device="cpu")
    ok = adapter(4)
    key = "model.layers.0.self_attn.q_proj"
    cases = {
        "no lora_b": ({k: v for k, v in ok.items() if k != key + ".lora_b"}, r"q_proj\.lora_a has no .*lora_b"),
        "no lora_a": ({k: v for k, v in ok.items() if k != key + ".lora_a"}, r"q_proj\.lora_b has no .*lora_a"),
        "unknown": (dict(ok, **{"model.layers.0.self_attn.p_proj.lora_a": ok[key + ".lora_a"],
                                "model.layers.0.self_attn.p_proj.lora_b": ok[key + ".lora_b"]}), r"p_proj\.lora_a names no"),
        "layer": (dict(ok, **{"model.layers.2.mlp.up_proj.lora_a": torch.zeros(4, 64),
                              "model.layers.2.mlp.up_proj.lora_b": torch.zeros(128, 4)}), r"layers\.2\.mlp\.up_proj"),
        "head": ({"lm_head.lora_a": torch.zeros(4, 64), "lm_head.lora_b": torch.zeros(64, 4)}, "lm_head.lora_a names no"),
        "shape a": (dict(ok, **{key + ".lora_a": torch.zeros(4, 63)}), r"q_proj\.lora_a has shape \(4, 63\)"),
        "shape b": (dict(ok, **{key + ".lora_b": torch.zeros(64, 5)}), r"q_proj\.lora_b has shape \(64, 5\)"),
        "rank": (adapter(9), "lora_a has rank 9, above max_rank 8"),
        "dora": (dict(ok, **{key + ".dora_m": torch.zeros(1, 64)}), r"q_proj\.dora_m: DoRA"),
        "empty": ({"model.norm.weight": torch.ones(64)}, "no lora_a / lora_b keys"),
    }
    for what, (sd, match) in cases.items():
        with pytest.raises(ValueError, match=match):
            st.load("bad", sd)
        assert st.slots == {} and not any(t.any() for l in st.A for t in l.values()), what
    st.load("one", ok)
    with pytest.raises(ValueError, match="'one' is already loaded"):
        st.load("one", ok)
    st.load("two", ok)
    with pytest.raises(ValueError, match="all 2 slots are taken"):
        st.load("three", ok)
    with pytest.raises(ValueError, match="'three' is not loaded"):
        st.unload("three")
    with pytest.raises(ValueError, match="serves ModelForCausalLM and Qwen3Model"):
        V.LoraAdapters(torch.nn.Linear(4, 4), 2)
    for kw in (dict(max_adapters=0), dict(max_adapters=2, max_rank=0)):
        with pytest.raises(ValueError, match="positive integer"):
            V.LoraAdapters(host_model(), device="cpu", **kw)


def test_qwen3_keys():
    cfg = dict(vocab_size=64, context_length=64, emb_dim=64, n_heads=2, n_layers=1, hidden_dim=96, head_dim=48,
               qk_norm=True, n_kv_groups=1, rope_base=10000.0, dtype=torch.bfloat16)
    st = V.LoraAdapters(V.Qwen3Model(cfg), 2, max_rank=8, device="cpu")
    assert st.dtype == torch.bfloat16
    sd = {"trf_blocks.0.att.W_query.lora_a": torch.ones(4, 64), "trf_blocks.0.att.W_query.lora_b": torch.ones(96, 4),
          "trf_blocks.0.ff.fc2.lora_a": torch.ones(8, 64), "trf_blocks.0.ff.fc2.lora_b": torch.ones(96, 8),
          "trf_blocks.0.att.out_proj.lora_a": torch.ones(2, 96), "trf_blocks.0.att.out_proj.lora_b": torch.ones(64, 2)}
    st.load("q", sd)
    assert st.A[0]["qkv"].shape == (2, 96, 64) and st.B[0]["qkv"].shape == (2, 96 + 48 + 48, 32)
    assert st.boundaries[0]["qkv"] == (96, 144) and st.boundaries[0]["gate_up"] == (96,)
    assert st.A[0]["gate_up"][0, 32:40].all() and not st.A[0]["gate_up"][0, :32].any()
    assert st.A[0]["o"].shape == (2, 32, 96) and st.A[0]["o"][0, :2].all()
    with pytest.raises(ValueError, match="model.layers.0.mlp.up_proj.lora_a names no"):
        st.load("other", {"model.layers.0.mlp.up_proj.lora_a": torch.ones(4, 64),
                          "model.layers.0.mlp.up_proj.lora_b": torch.ones(96, 4)})


def test_engine_refusals_and_hold_counts():
    st = store()
    with pytest.raises(ValueError, match="adapters= needs varlen_prefill=True"):
        V.ContinuousBatchEngine(None, manager(), adapters=st)
    with pytest.raises(ValueError, match="adapters= needs varlen_prefill=True"):
        V.ContinuousBatchEngine(None, manager(), adapters=st, varlen_prefill=False)
    bare = V.ContinuousBatchEngine(None, manager(), varlen_prefill=True)
    with pytest.raises(ValueError, match="built without adapters="):
        bare.add_sequence([3, 4], 2, adapter="n1")
    eng = engine(st, max_batch_size=1)
    with pytest.raises(ValueError, match="'n3' is not loaded"):
        eng.add_sequence([3, 4], 2, adapter="n3")
    assert eng.waiting_room == type(eng.waiting_room)() and eng.sampling == {} and eng.adapter == {}
    a = eng.add_sequence([3, 4, 5], 2, adapter="n1")
    b = eng.add_sequence([6, 7, 8], 1, adapter="n1")          # waits: the batch holds one sequence
    assert st.held == {"n1": 2, "n2": 0} and eng.adapter == {a: "n1", b: "n1"}
    with pytest.raises(ValueError, match="'n1' is held by 2"):
        st.unload("n1")
    states, md, _ = eng._plan_step()
    assert [s.id for s in states] == [a]
    eng._finish_step(states, [9])
    with pytest.raises(ValueError, match="'n1' is held by 2"):
        st.unload("n1")
    states, md, _ = eng._plan_step()
    assert eng._finish_step(states, [9]) == {a: [3, 4, 5, 9, 9]}
    assert st.held["n1"] == 1 and eng.adapter == {b: "n1"}
    with pytest.raises(ValueError, match="'n1' is held by 1"):
        st.unload("n1")
    states, md, _ = eng._plan_step()
    assert tiles_of(md) == [(0, 3, 0)]
    eng._finish_step(states, [1])
    assert st.held["n1"] == 0 and eng.adapter == {} and not eng.active
    st.unload("n1")
    assert st.slots == {"n2": 1}
    with pytest.raises(ValueError, match="'n1' is not loaded"):
        eng.add_sequence([3, 4], 2, adapter="n1")


def test_host_shape_rules_name_the_projection():
    """What ops.lora_delta_ can see on the host is refused before anything touches a GPU: K % 32, part widths and
    boundaries % 16, dtypes and the stacks' shapes; n_tiles == 0 returns at once."""
    from vyomai_amd import ops
    y, x = torch.zeros(4, 48), torch.zeros(4, 64)
    A, B = torch.zeros(2, 32, 64), torch.zeros(2, 48, 32)
    al, tl = torch.ones(2), torch.zeros((1, 3), dtype=torch.int32)
    assert ops.lora_delta_(y, x, A, B, al, tl[:0], 0) is y
    bad = {
        r"layer 1 qkv\): K = 48": (y, torch.zeros(4, 48), torch.zeros(2, 32, 48), B, al, tl, 1),
        r"layer 1 qkv\): .*N = 40": (torch.zeros(4, 40), x, A, torch.zeros(2, 40, 32), al, tl, 1),
        "boundaries": (y, x, A, B, al, tl, 1, (8,)),
        "A must be a contiguous": (y, x, A, B, al, tl, 1, (16,)),
        "must share": (y, x.bfloat16(), A, B, al, tl, 1),
        "alpha must be": (y, x, A, B, al.double(), tl, 1),
        "tiles must be": (y, x, A, B, al, tl.long(), 1),
        "r_pad a multiple of 32": (y, x, torch.zeros(2, 16, 64), torch.zeros(2, 48, 16), al, tl, 1),
    }
    for match, args in bad.items():
        with pytest.raises(ValueError, match=match):
            ops.lora_delta_(*args, name="layer 1 qkv")
    with pytest.raises(ValueError, match="in_features 72 must be a multiple of 32"):
        V.LoraAdapters(V.ModelForCausalLM(V.Config(**dict(CFG, hidden_size=72, num_attention_heads=1))), 1, device="cpu")
