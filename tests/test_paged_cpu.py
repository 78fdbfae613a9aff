"""Paged KV cache, host side (vyomai_amd/serving.py): slot mapping, the block manager with its radix prefix cache, the
scheduler's admission, and the C ABI of the three paged entry points -- all without a GPU."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import vyomai_amd as V
from vyomai_amd import _lib, ops

BS = 8
NEW = ("vy_paged_rope_write", "vy_attn_paged_decode", "vy_attn_paged_decode_ws_bytes", "vy_paged_gather")


def config(**kw):
    base = dict(vocab_size=64, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=1, max_position_embeddings=128)
    base.update(kw)
    return V.Config(**base)


def manager(max_blocks, block_size=BS):
    return V.PagedKVManager(config(), max_blocks, block_size, "cpu", torch.float32)


def prompt(n, first=1):
    return list(range(first, first + n))


def state(mgr, tokens, gen=4, sid=0, matched=None):
    return V.SequenceState(sid, tokens, gen, mgr.block_size, "cpu", matched_blocks=matched)


def refs(mgr):
    return {b: n.ref_count for b, n in mgr.block_to_node.items()}


# ---- slot mapping ----------------------------------------------------------------------------------------------


def test_slot_mapping_prefill_prefix_and_decode():
    mgr = manager(8)
    mgr.free_blocks = type(mgr.free_blocks)([5, 2, 7, 0, 1, 3, 4, 6])        # physical order is not logical order
    s = state(mgr, prompt(19))
    mgr.allocate(s)
    s.update_metadata()
    assert s.block_table[:3].tolist() == [5, 2, 7]
    want = [[5, 2, 7][i // BS] * BS + i % BS for i in range(19)]
    assert s.slot_mapping[:19].tolist() == want
    # a decode step covers the last token only
    s.is_prefill = False
    s.num_tokens += 1
    s.slot_mapping.fill_(-7)
    mgr.allocate(s)
    s.update_metadata()
    assert s.slot_mapping[19].item() == 7 * BS + 3 and (s.slot_mapping[:19] == -7).all() and (s.slot_mapping[20:] == -7).all()
    # a prefix hit starts at prefix_len
    mgr.free(s)
    hit = mgr.get_prefix_blocks(prompt(19))
    assert hit == [5, 2]
    t = state(mgr, prompt(19), sid=1, matched=hit)
    assert t.prefix_len == 16 and t.query_start == 16
    t.slot_mapping.fill_(-7)
    mgr.allocate(t)
    t.update_metadata()
    assert (t.slot_mapping[:16] == -7).all()
    assert t.slot_mapping[16:19].tolist() == [int(t.block_table[2]) * BS + i for i in range(3)]


def test_block_size_must_be_a_power_of_two_from_8_to_256():
    for bad in (4, 12, 24, 512, 0):
        with pytest.raises(ValueError, match="block_size"):
            manager(4, bad)
    for good in (8, 16, 256):
        assert manager(2, good).k_cache[0].shape == (2, good, 1, 32)


# ---- manager ---------------------------------------------------------------------------------------------------


def test_allocation_order_and_free():
    mgr = manager(6)
    s = state(mgr, prompt(10), gen=10)
    mgr.allocate(s)
    assert s.block_table[:2].tolist() == [0, 1] and list(mgr.free_blocks) == [2, 3, 4, 5]
    assert set(mgr.block_to_node) == {0}            # only the complete prompt block is registered
    s.num_tokens = 17                                # grows during decode: block 2, filled later, never registered
    mgr.allocate(s)
    assert s.block_table[:3].tolist() == [0, 1, 2] and set(mgr.block_to_node) == {0}
    mgr.free(s)
    assert list(mgr.evictable_blocks) == [0] and list(mgr.free_blocks) == [3, 4, 5, 1, 2] and s.block_count == 0


def test_prefix_hit_returns_the_first_requests_blocks_and_counts_them():
    mgr = manager(8)
    a = state(mgr, prompt(20))
    mgr.allocate(a)
    assert refs(mgr) == {0: 1, 1: 1}
    assert mgr.match_prefix(prompt(20)) == [0, 1] and refs(mgr) == {0: 1, 1: 1}      # matching alone counts nothing
    hit = mgr.get_prefix_blocks(prompt(20))
    assert hit == a.block_table[:2].tolist() and refs(mgr) == {0: 2, 1: 2}
    assert mgr.match_prefix(prompt(8) + prompt(12, first=40)) == [0]                 # diverges in the second block
    assert mgr.match_prefix(prompt(20, first=2)) == []


def test_two_holders_two_frees_evictable_once():
    mgr = manager(8)
    a = state(mgr, prompt(20))
    mgr.allocate(a)
    b = state(mgr, prompt(20), sid=1, matched=mgr.get_prefix_blocks(prompt(20)))
    mgr.allocate(b)
    mgr.free(a)
    assert list(mgr.evictable_blocks) == [] and refs(mgr) == {0: 1, 1: 1}
    mgr.free(b)
    assert list(mgr.evictable_blocks) == [0, 1] and refs(mgr) == {0: 0, 1: 0}
    assert sorted(list(mgr.free_blocks) + list(mgr.evictable_blocks)) == list(range(8))


def test_eviction_is_oldest_first():
    mgr = manager(3)
    for sid, first in enumerate((1, 20, 40)):        # three one-block prompts, freed in this order
        s = state(mgr, prompt(8, first), gen=1, sid=sid)
        mgr.allocate(s)
        mgr.free(s)
    assert list(mgr.evictable_blocks) == [0, 1, 2] and not mgr.free_blocks
    s = state(mgr, prompt(8, 50), gen=1, sid=3)
    mgr.allocate(s)
    assert s.block_table[0].item() == 0 and list(mgr.evictable_blocks) == [1, 2]
    assert mgr.match_prefix(prompt(9, 1)) == [] and mgr.match_prefix(prompt(9, 20)) == [1]


def test_evicting_a_parent_drops_its_subtree():
    mgr = manager(4)
    a = state(mgr, prompt(25), gen=1)                # blocks 0, 1, 2 registered as a chain, block 3 partial
    mgr.allocate(a)
    assert set(mgr.block_to_node) == {0, 1, 2}
    mgr.free(a)
    assert list(mgr.evictable_blocks) == [0, 1, 2] and list(mgr.free_blocks) == [3]
    b = state(mgr, prompt(12, 60), gen=1, sid=1)     # takes 3, then has to evict 0: 1 and 2 go with it
    mgr.allocate(b)
    assert b.block_table[:2].tolist() == [3, 0]
    assert set(mgr.block_to_node) == {3} and not mgr.evictable_blocks and list(mgr.free_blocks) == [1, 2]
    assert not mgr.radix_root.children[tuple(prompt(8, 60))].children
    assert mgr.match_prefix(prompt(25)) == []        # a later identical prompt misses cleanly
    c = state(mgr, prompt(25)[:16], gen=1, sid=2, matched=mgr.get_prefix_blocks(prompt(25)[:16]))
    mgr.allocate(c)
    assert c.prefix_len == 0 and c.block_table[:2].tolist() == [1, 2]


def test_match_is_capped_so_that_one_token_is_computed():
    mgr = manager(8)
    a = state(mgr, prompt(16))
    mgr.allocate(a)
    assert set(mgr.block_to_node) == {0, 1}          # both blocks cached
    assert mgr.match_prefix(prompt(16)) == [0]       # (16 - 1) // 8 = 1
    assert mgr.match_prefix(prompt(17)) == [0, 1]
    with pytest.raises(ValueError):
        state(mgr, prompt(16), matched=[0, 1])


def test_cache_full_raises():
    mgr = manager(2)
    a = state(mgr, prompt(16), gen=8)
    mgr.allocate(a)
    b = state(mgr, prompt(4, 50), sid=1)
    with pytest.raises(RuntimeError, match="KV Cache full!"):
        mgr.allocate(b)                              # nothing free, nothing evictable (a holds both)
    mgr.free(a)
    mgr.allocate(b)                                  # now block 0 is evicted for it (and block 1, its child, freed)
    assert b.block_table[0].item() == 0 and list(mgr.free_blocks) == [1]


# ---- scheduler -------------------------------------------------------------------------------------------------


def test_waiting_request_leaves_no_reference_behind():
    mgr = manager(5)
    eng = V.ContinuousBatchEngine(None, mgr, max_batch_size=4)
    first = state(mgr, prompt(17), gen=1)            # leaves two cached blocks behind
    mgr.allocate(first)
    mgr.free(first)
    sid0 = eng.add_sequence(prompt(17), max_gen_len=15)          # 4 blocks, 2 of them cached
    sid1 = eng.add_sequence(prompt(17), max_gen_len=15)          # would hit the same 2, but 2 more do not fit
    eng._try_schedule_waiting()
    assert list(eng.active) == [sid0] and [r["sid"] for r in eng.waiting_room] == [sid1]
    before = (refs(mgr), list(mgr.free_blocks), list(mgr.evictable_blocks))
    assert before[0] == {0: 1, 1: 1}
    for _ in range(4):
        eng._try_schedule_waiting()
        assert (refs(mgr), list(mgr.free_blocks), list(mgr.evictable_blocks)) == before
        assert [r["sid"] for r in eng.waiting_room] == [sid1]
    mgr.free(eng.active.pop(sid0))
    eng._try_schedule_waiting()
    assert list(eng.active) == [sid1] and refs(mgr) == {0: 1, 1: 1} and eng.active[sid1].prefix_len == 16


def test_max_batch_size_is_respected():
    mgr = manager(32)
    eng = V.ContinuousBatchEngine(None, mgr, max_batch_size=3)
    sids = [eng.add_sequence(prompt(5, 1 + i), max_gen_len=3) for i in range(5)]
    eng._try_schedule_waiting()
    assert list(eng.active) == sids[:3] and len(eng.waiting_room) == 2
    mgr.free(eng.active.pop(sids[1]))
    eng._try_schedule_waiting()
    assert list(eng.active) == [sids[0], sids[2], sids[3]] and len(eng.waiting_room) == 1
    with pytest.raises(ValueError):
        eng.add_sequence(prompt(200), max_gen_len=100)           # can never fit into 32 blocks of 8


def test_eos_defaults_to_the_configs():
    mgr = manager(4)
    assert V.ContinuousBatchEngine(None, mgr).eos_token_ids == {1}
    assert V.ContinuousBatchEngine(None, mgr, eos_token_ids=[7, 9]).eos_token_ids == {7, 9}


# ---- ABI -------------------------------------------------------------------------------------------------------


def test_header_binding_and_library_agree_on_the_new_symbols():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    declared = set(re.findall(r"\b(vy_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.ALL_SYMBOLS and hasattr(lib, name), name
    for name in NEW:
        if name in _lib.PROTOTYPES:      # as many argtypes as the header's prototype has parameters
            proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
            assert len(_lib.PROTOTYPES[name]) == proto.count(",") + 1, name
    assert _lib.load().vy_abi_version() == 5


def _buf():
    raw = (ctypes.c_char * 8192)()
    return raw, (ctypes.addressof(raw) + 255) // 256 * 256


def test_argument_errors_are_reported_without_a_gpu():
    raw, p = _buf()

    def rope(block_size=16, dh=64, qkv=p):
        _lib.call("vy_paged_rope_write", qkv, 256, p, p, p, p, 8, p, p, 4, block_size, 4, 2, 1, dh, 1, None)

    def decode(block_size=16, dh=64, q=p):
        _lib.call("vy_attn_paged_decode", q, 256, None, p, p, 4, block_size, p, 4, p, 16, p, 256, 2, 2, 1, dh, 0.125, 0,
                  None, 0, 1, None)

    def gather(block_size=16, dh=64, k=p):
        _lib.call("vy_paged_gather", k, p, 4, block_size, p, 2, 20, p, p, 1, dh, 1, None)

    for fn in (rope, decode, gather):
        for bad in (12, 4, 512):
            with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*block_size"):
                fn(block_size=bad)
        for bad in (60, 264, 0):
            with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*multiple of 8"):
                fn(dh=bad)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
        rope(qkv=None)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
        decode(q=None)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
        gather(k=None)
    # a pinned split needs its workspace
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*workspace"):
        _lib.call("vy_attn_paged_decode", p, 256, None, p, p, 4, 16, p, 4, p, 16, p, 256, 2, 2, 1, 64, 0.125, 2, None, 0, 1, None)
    lib = _lib.load()
    assert lib.vy_attn_paged_decode_ws_bytes(2, 4, 2, 64, 1300, 1, 1) == 0
    assert lib.vy_attn_paged_decode_ws_bytes(2, 4, 2, 64, 1300, 5, 1) == 2 * 4 * 5 * (64 + 2) * 4


def test_wrappers_raise_value_errors_on_bad_pages():
    q = torch.zeros(2, 128)
    bt, sl = torch.zeros((2, 2), dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="block_size"):
        ops.attention_paged_decode(q, torch.zeros(4, 12, 1, 64), torch.zeros(4, 12, 1, 64), bt, sl, 1, 2)
    with pytest.raises(ValueError, match="head_dim"):
        ops.attention_paged_decode(q, torch.zeros(4, 16, 1, 60), torch.zeros(4, 16, 1, 60), bt, sl, 1, 2)
    with pytest.raises(ValueError, match="block_size"):
        ops.paged_gather(torch.zeros(4, 24, 1, 64), torch.zeros(4, 24, 1, 64), bt[0], 4)


def test_forward_paged_fails_loudly_without_a_gpu():
    cfg = config()
    model = V.ModelForCausalLM(cfg)
    mgr = V.PagedKVManager(cfg, 4, BS, "cpu", torch.float32)
    eng = V.ContinuousBatchEngine(model, mgr)
    eng.add_sequence(prompt(5), max_gen_len=2)
    with pytest.raises(_lib.VyomHipError, match="CPU tensor"):
        eng.step()
