"""vy_attn_paged_prefill and chunked prefill without a GPU: the ABI of the new symbol, its argument errors, and the
scheduler of ContinuousBatchEngine(max_step_tokens=..., varlen_prefill=...) driven through a stub model -- the chunks,
the packed metadata of the one varlen launch, and the rule that a prompt block enters the radix tree only in the step
that writes its last row."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import vyomai_amd as V
from vyomai_amd import _lib

BS = 8
NAME = "vy_attn_paged_prefill"


def config():
    return V.Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                    num_key_value_heads=1, max_position_embeddings=64, eos_token_id=1)


class StubModel:
    """forward_paged records what the engine hands it and answers with logits whose argmax is `token`."""

    def __init__(self, token=7, vocab=64):
        self.token, self.vocab, self.calls = token, vocab, []

    def eval(self):
        return self

    def forward_paged(self, input_ids, positions, metadata, kv_mgr):
        self.calls.append({"input_ids": input_ids.tolist(), "positions": positions.tolist(), "metadata": metadata})
        logits = torch.zeros(metadata["last_rows"].numel(), self.vocab)
        logits[:, self.token] = 1.0
        return logits


def engine(max_blocks=16, **kw):
    mgr = V.PagedKVManager(config(), max_blocks, BS, "cpu", torch.float32)
    stub = StubModel()
    return V.ContinuousBatchEngine(stub, mgr, eos_token_ids=[], **kw), mgr, stub


def slots_of(state, positions):
    return [int(state.block_table[i // BS]) * BS + i % BS for i in positions]


# ---- ABI -------------------------------------------------------------------------------------------------------


def test_header_binding_and_library_agree_on_the_prefill_symbol():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    declared = set(re.findall(r"\b(vy_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert NAME in declared and NAME in _lib.ALL_SYMBOLS and NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    proto = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(_lib.PROTOTYPES[NAME]) == proto.count(",") + 1 == 21
    assert "flash_attn_varlen_func" in hdr
    assert _lib.load().vy_abi_version() == 5            # the symbol is additive


def test_prefill_argument_errors_are_reported_without_a_gpu():
    raw = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(raw) + 255) // 256 * 256

    def prefill(block_size=16, dh=64, q=p, n_seq=2, dtype=1, h=2, hk=1, q_ld=256):
        _lib.call(NAME, q, q_ld, p, p, 4, block_size, p, 4, p, p, n_seq, 16, 32, p, 256, h, hk, dh, 0.125, dtype, None)

    for bad in (12, 4, 512):
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*block_size"):
            prefill(block_size=bad)
    for bad in (60, 264, 0):
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*multiple of 8"):
            prefill(dh=bad)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*null operand"):
        prefill(q=None)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*bad dtype"):
        prefill(dtype=2)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*bad shape"):
        prefill(h=3, hk=2)
    with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*bad shape"):
        prefill(q_ld=100)
    prefill(n_seq=0)                                    # nothing to do: VY_OK, no launch (there is no GPU here)


def test_prefill_wrapper_raises_value_errors_on_bad_pages():
    from vyomai_amd import ops
    q = torch.zeros(4, 128)
    bt, cu, ctx = torch.zeros((1, 2), dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="block_size"):
        ops.attention_paged_prefill(q, torch.zeros(4, 12, 1, 64), torch.zeros(4, 12, 1, 64), bt, cu, ctx, 4, 4, 2)
    with pytest.raises(ValueError, match="head_dim"):
        ops.attention_paged_prefill(q, torch.zeros(4, 16, 1, 60), torch.zeros(4, 16, 1, 60), bt, cu, ctx, 4, 4, 2)
    with pytest.raises(_lib.VyomHipError, match="CPU tensor"):
        ops.attention_paged_prefill(q, torch.zeros(4, 16, 1, 64), torch.zeros(4, 16, 1, 64), bt, cu, ctx, 4, 4, 2)


# ---- scheduler -------------------------------------------------------------------------------------------------


def test_engine_argument_rules():
    mgr = V.PagedKVManager(config(), 4, BS, "cpu", torch.float32)
    with pytest.raises(ValueError, match="max_step_tokens"):
        V.ContinuousBatchEngine(StubModel(), mgr, max_batch_size=4, max_step_tokens=3)
    with pytest.raises(ValueError, match="varlen_prefill"):
        V.ContinuousBatchEngine(StubModel(), mgr, max_batch_size=2, max_step_tokens=3, varlen_prefill=False)
    eng = V.ContinuousBatchEngine(StubModel(), mgr, max_batch_size=3, max_step_tokens=3)
    assert eng.varlen_prefill is True and eng.max_step_tokens == 3
    eng = V.ContinuousBatchEngine(StubModel(), mgr, max_step_tokens=None, varlen_prefill=None)
    assert eng.varlen_prefill is False and eng.max_step_tokens is None


def test_chunked_prefill_beside_a_decoding_sequence():
    """max_step_tokens = 3, one decoding sequence: it takes its token first in every step and the 20-token prompt goes
    in ten chunks of 2, emits nothing until the last one, and is registered block by block as the chunks complete."""
    eng, mgr, stub = engine(max_batch_size=2, max_step_tokens=3)
    dec = eng.add_sequence([50, 51], max_gen_len=30)
    assert eng.step() == {}
    m = stub.calls[0]["metadata"]
    assert stub.calls[0]["input_ids"] == [50, 51] and stub.calls[0]["positions"] == [0, 1]
    pv = m["prefill_varlen"]
    assert pv["cu_q"].tolist() == [0, 2] and pv["ctx_lens"].tolist() == [0] and (pv["max_q"], pv["max_kv"]) == (2, 2)
    assert m["decode"] is None and m["prefill"] == [] and m["last_rows"].tolist() == [1]
    prompt = list(range(1, 21))
    long = eng.add_sequence(prompt, max_gen_len=2)
    for k in range(1, 11):
        assert eng.step() == {}
        call = stub.calls[k]
        m, pv = call["metadata"], call["metadata"]["prefill_varlen"]
        a = 2 * (k - 1)
        sd, sl = eng.active[dec], eng.active[long]
        # the decoder's row comes first, then the chunk
        assert call["input_ids"] == [7, prompt[a], prompt[a + 1]], k
        assert call["positions"] == [1 + k, a, a + 1], k
        assert m["slot_mapping"].tolist() == slots_of(sd, [1 + k]) + slots_of(sl, [a, a + 1]), k
        assert m["decode"]["rows"].tolist() == [0] and m["decode"]["seqlens"].tolist() == [2 + k], k
        assert m["decode"]["block_table"][0, :sd.block_count].tolist() == sd.block_table[:sd.block_count].tolist()
        assert pv["cu_q"].tolist() == [1, 3] and pv["ctx_lens"].tolist() == [a], k
        assert (pv["max_q"], pv["max_kv"]) == (2, a + 2), k
        assert pv["block_table"].shape[0] == 1 and pv["block_table"].dtype == torch.int32
        assert sl.block_count == (a + 2 + BS - 1) // BS, "blocks are allocated up to the chunk's end only"
        assert pv["block_table"][0, :sl.block_count].tolist() == sl.block_table[:sl.block_count].tolist(), k
        assert m["prefill"] == []
        # only the last chunk reaches the prompt's end: one logits row for the decoder before, two then
        assert m["last_rows"].tolist() == ([0] if k < 10 else [0, 2]), k
        assert eng.prompt_tokens_computed[long] == 2 * k, k
        assert sl.is_prefill == (k < 10) and sl.num_computed == 2 * k and sl.num_tokens == (20 if k < 10 else 21), k
        assert sd.num_tokens == 3 + k, "the decoder got its token"
        # the registration invariant: a block is matched only once its last row has been computed
        assert len(mgr.match_prefix(prompt)) == min(2 * k // BS, 2), k
    assert eng.prompt_tokens_computed == {dec: 2, long: 20}
    # both decode now: no varlen entry, and the long request ends at its max_gen_len
    done = eng.step()
    m = stub.calls[11]["metadata"]
    assert "prefill_varlen" not in m and m["decode"]["rows"].tolist() == [0, 1] and m["last_rows"].tolist() == [0, 1]
    assert done == {long: prompt + [7, 7]}


def test_registration_invariant_chunks_of_three_against_blocks_of_eight():
    """Alone, the prompt goes as 3+3+3+3+3+3+2.  Block 0 is allocated by the first chunk and complete in the third
    (position 7), block 1 allocated in the third and complete in the sixth (position 15): match_prefix of the same
    tokens returns 0 blocks until then, never a block with unwritten rows; block 2 (4 prompt tokens) is never registered."""
    eng, mgr, stub = engine(max_batch_size=3, max_step_tokens=3)
    prompt = list(range(1, 21))
    sid = eng.add_sequence(prompt, max_gen_len=2)
    want_chunks = [3, 3, 3, 3, 3, 3, 2]
    done = 0
    for k, n in enumerate(want_chunks):
        assert eng.step() == {}
        call = stub.calls[k]
        assert call["positions"] == list(range(done, done + n)), k
        pv = call["metadata"]["prefill_varlen"]
        assert pv["cu_q"].tolist() == [0, n] and pv["ctx_lens"].tolist() == [done], k
        done += n
        assert call["metadata"]["last_rows"].numel() == (1 if done == 20 else 0)
        matched = mgr.match_prefix(prompt)
        assert len(matched) == min(done // BS, 2), (k, matched)
        assert matched == eng.active[sid].block_table[:len(matched)].tolist()
        assert set(mgr.block_to_node) == set(matched)
    assert eng.prompt_tokens_computed[sid] == 20 and not eng.active[sid].is_prefill


def test_a_sequence_without_budget_sits_the_step_out():
    """Two prompts of 5 under max_step_tokens = 4: 4 + 0, then 1 + 3, then the first decodes and the second ends."""
    eng, mgr, stub = engine(max_batch_size=2, max_step_tokens=4)
    a = eng.add_sequence([10, 11, 12, 13, 14], max_gen_len=4)
    b = eng.add_sequence([20, 21, 22, 23, 24], max_gen_len=4)
    eng.step()
    assert stub.calls[0]["input_ids"] == [10, 11, 12, 13] and stub.calls[0]["metadata"]["last_rows"].numel() == 0
    assert eng.active[b].block_count == 0 and b not in eng.prompt_tokens_computed
    eng.step()
    pv = stub.calls[1]["metadata"]["prefill_varlen"]
    assert stub.calls[1]["input_ids"] == [14, 20, 21, 22] and stub.calls[1]["positions"] == [4, 0, 1, 2]
    assert pv["cu_q"].tolist() == [0, 1, 4] and pv["ctx_lens"].tolist() == [4, 0] and (pv["max_q"], pv["max_kv"]) == (3, 5)
    assert stub.calls[1]["metadata"]["last_rows"].tolist() == [0]
    eng.step()
    m = stub.calls[2]["metadata"]
    assert stub.calls[2]["input_ids"] == [7, 23, 24] and m["decode"]["rows"].tolist() == [0]
    assert m["prefill_varlen"]["cu_q"].tolist() == [1, 3] and m["last_rows"].tolist() == [0, 2]
    assert eng.prompt_tokens_computed == {a: 5, b: 5}


def test_varlen_alone_keeps_the_unchunked_schedule():
    """varlen_prefill=True without a budget: whole prompts, as in the default engine, but described for ONE launch."""
    eng, mgr, stub = engine(varlen_prefill=True)
    eng.add_sequence(list(range(1, 12)), max_gen_len=2)
    eng.add_sequence(list(range(30, 33)), max_gen_len=2)
    eng.step()
    m = stub.calls[0]["metadata"]
    pv = m["prefill_varlen"]
    assert pv["cu_q"].tolist() == [0, 11, 14] and pv["ctx_lens"].tolist() == [0, 0] and (pv["max_q"], pv["max_kv"]) == (11, 11)
    assert pv["block_table"].shape == (2, 2) and pv["block_table"][:, 0].tolist() == [0, 2]
    assert m["last_rows"].tolist() == [10, 13] and m["prefill"] == [] and m["decode"] is None


def test_default_engine_is_unchanged():
    """Both arguments at None: no prefill_varlen key, the per-sequence prefill list of before, whole prompts."""
    eng, mgr, stub = engine(max_step_tokens=None, varlen_prefill=None)
    eng.add_sequence(list(range(1, 12)), max_gen_len=2)
    eng.add_sequence(list(range(30, 33)), max_gen_len=2)
    eng.step()
    m = stub.calls[0]["metadata"]
    assert set(m) == {"positions", "slot_mapping", "last_rows", "max_position", "prefill", "decode"}
    assert m["prefill"] == [(0, 11, 0, None), (11, 3, 0, None)] and m["decode"] is None
    assert m["last_rows"].tolist() == [10, 13] and stub.calls[0]["positions"] == list(range(11)) + list(range(3))
    assert set(mgr.block_to_node) == {0}                # the complete prompt block, registered at allocation
    eng.step()
    m = stub.calls[1]["metadata"]
    assert "prefill_varlen" not in m and m["prefill"] == [] and m["decode"]["rows"].tolist() == [0, 1]


def test_allocate_upto_registers_a_block_an_earlier_chunk_left_part_filled():
    mgr = V.PagedKVManager(config(), 8, BS, "cpu", torch.float32)
    s = V.SequenceState(0, list(range(1, 21)), 4, BS, "cpu")
    mgr.allocate(s, upto=5)
    assert s.block_count == 1 and not mgr.block_to_node and s.num_computed == 0
    mgr.allocate(s, upto=9)                             # block 0 complete now, block 1 allocated and part filled
    assert s.block_count == 2 and set(mgr.block_to_node) == {0}
    mgr.allocate(s, upto=20)
    assert s.block_count == 3 and set(mgr.block_to_node) == {0, 1}
    mgr.allocate(s)                                     # the meaning of before: blocks for num_tokens, nothing new
    assert s.block_count == 3 and set(mgr.block_to_node) == {0, 1}
    assert {b: n.ref_count for b, n in mgr.block_to_node.items()} == {0: 1, 1: 1}
