"""Speculative decoding in ContinuousBatchEngine without a GPU (model=None): the constructor's checks, what a
speculative step plans -- row layout, drafts clipped at the end of a request's life, the drafter's catch-up, the token
budget, the two uploads -- what the host does with accept / alt / draft tokens, and that the default engine is untouched."""
import pytest
import torch

import vyomai_amd as V
from tests.test_serving_sampling_cpu import Uploads

BS = 8


def config(vocab=64, layers=1):
    return V.Config(vocab_size=vocab, hidden_size=64, intermediate_size=128, num_hidden_layers=layers,
                    num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=64, eos_token_id=1)


def manager(blocks=32, bs=BS, dtype=torch.float32, **kw):
    return V.PagedKVManager(config(**kw), blocks, bs, "cpu", dtype)


def engine(g=3, eos=(), **kw):
    kw.setdefault("varlen_prefill", True)
    return V.ContinuousBatchEngine(None, manager(), eos_token_ids=list(eos), draft_kv_mgr=manager(),
                                   num_speculative_tokens=g, **kw)


def finish(eng, plan, accept, alt, drafts):
    """accept / alt per judged sequence (padded to g + 1), drafts per sequence (padded to g) -> the finished dict."""
    g, S = eng.num_speculative_tokens, len(plan["emitting"])
    accept = [list(a) + [0] * (g + 1 - len(a)) for a in accept]
    alt = [list(a) + [-1] * (g + 1 - len(a)) for a in alt]
    drafts = [list(d) + [0] * (g - len(d)) for d in drafts]
    return eng._finish_spec_step(plan, accept, alt, [[drafts[k][i] for k in range(S)] for i in range(g)])


# ---- constructor -----------------------------------------------------------------------------------------------


def test_constructor_checks():
    ok = dict(varlen_prefill=True, draft_kv_mgr=manager(), num_speculative_tokens=4)
    eng = V.ContinuousBatchEngine(None, manager(), **ok)
    assert eng.speculative and eng.drafts_proposed == eng.drafts_accepted == 0

    def bad(match, mgr=None, **kw):
        with pytest.raises(ValueError, match=match):
            V.ContinuousBatchEngine(None, mgr or manager(), **{**ok, **kw})

    bad("varlen_prefill", varlen_prefill=False)
    bad("varlen_prefill", varlen_prefill=None)
    bad("vocabulary", draft_kv_mgr=manager(vocab=65))
    bad("blocks", draft_kv_mgr=manager(blocks=16))
    bad("blocks", draft_kv_mgr=manager(bs=16))
    bad("is on", draft_kv_mgr=V.PagedKVManager(config(), 32, BS, "meta", torch.float32))
    bad("computes in", draft_kv_mgr=manager(dtype=torch.bfloat16))
    bad("draft_kv_mgr", draft_kv_mgr=None)
    for g in (0, 17, -1, 2.5):
        bad("num_speculative_tokens", num_speculative_tokens=g)
    bad("max_step_tokens", max_batch_size=4, max_step_tokens=19)
    V.ContinuousBatchEngine(None, manager(), max_batch_size=4, max_step_tokens=20, **ok)      # 4 * (4 + 1)
    # chunked prefill implies varlen_prefill, as it always did
    assert V.ContinuousBatchEngine(None, manager(), max_batch_size=2, max_step_tokens=10, draft_kv_mgr=manager(),
                                   num_speculative_tokens=4).varlen_prefill
    # a drafter with more layers and its own page dtype is fine as long as the blocks line up
    V.ContinuousBatchEngine(None, manager(), varlen_prefill=True, draft_kv_mgr=manager(layers=2), num_speculative_tokens=1)


# ---- the plan --------------------------------------------------------------------------------------------------


def test_first_step_is_the_plain_prefill():
    eng = engine()
    a, b = eng.add_sequence([10, 11, 12], 8), eng.add_sequence([20, 21], 2)
    plan = eng._plan_spec_step()
    md, ids = plan["verify"]
    assert ids.tolist() == [10, 11, 12, 20, 21] and md["positions"].tolist() == [0, 1, 2, 0, 1]
    assert md["last_rows"].tolist() == [2, 4] and md["decode"] is None
    assert md["prefill_varlen"]["cu_q"].tolist() == [0, 3, 5] and md["prefill_varlen"]["ctx_lens"].tolist() == [0, 0]
    assert plan["n_draft"] == [0, 0] and plan["t_row0"] == [0, 1]
    # the drafter prefills the same segments and has no logits row
    assert len(plan["draft"]) == 1
    dmd, dids, n, _ = plan["draft"][0]
    assert n == 0 and dids.tolist() == ids.tolist() and dmd["last_rows"].numel() == 0
    assert dmd["slot_mapping"].tolist() == md["slot_mapping"].tolist()
    assert dmd["prefill_varlen"]["cu_q"].tolist() == [0, 3, 5]
    assert plan["sampling"]["position0"].tolist() == [3, 2]
    assert finish(eng, plan, [[0], [0]], [[7], [8]], [[], []]) == {}
    assert eng.draft_computed == {a: 3, b: 2} and eng.drafts_proposed == 0


def test_row_layout_clipping_and_catch_up(monkeypatch):
    eng = engine()
    a, b = eng.add_sequence([10, 11, 12], 8), eng.add_sequence([20, 21], 2)
    finish(eng, eng._plan_spec_step(), [[0], [0]], [[7], [8]], [[], []])
    c = eng.add_sequence(list(range(30, 41)), 5)
    count = Uploads(monkeypatch)
    plan = eng._plan_spec_step()
    assert count.take() == (2, 2), "a speculative step makes the two uploads of a plain one"
    # a: 4 tokens of 11 -> 3 drafts; b: 3 of 4 -> g = 0, one row, last token of its life; c: the prompt
    assert [s.id for s in plan["states"]] == [a, b, c] and [s.id for s in plan["emitting"]] == [a, b, c]
    assert plan["n_draft"] == [3, 0, 0] and plan["t_row0"] == [0, 4, 5]
    md, ids = plan["verify"]
    assert ids.tolist() == [7, 0, 0, 0, 8] + list(range(30, 41))
    assert md["positions"].tolist() == [3, 4, 5, 6, 2] + list(range(11))
    assert md["last_rows"].tolist() == [0, 1, 2, 3, 4, 15], "g_s + 1 rows per decoding sequence, one per finishing prompt"
    assert md["prefill_varlen"]["cu_q"].tolist() == [0, 4, 5, 16] and md["prefill_varlen"]["ctx_lens"].tolist() == [3, 2, 0]
    assert md["decode"] is None and md["prefill_varlen"]["max_q"] == 11
    assert plan["scatter"][0].tolist() == [1, 2, 3] and plan["scatter"][1].tolist() == [0, 3, 6]
    sa = eng.active[a]
    assert md["slot_mapping"].tolist()[:4] == sa.slot_mapping[3:7].tolist()
    assert sa.block_count == 1 and eng.active[c].block_count == 2
    # round 0: one catch-up token for a (b does not draft), then c's prompt; rounds 1 and 2: a alone, decode rows
    rounds = plan["draft"]
    assert [r[2] for r in rounds] == [1, 1, 1]
    assert rounds[0][1].tolist() == [7] + list(range(30, 41)) and rounds[0][0]["last_rows"].tolist() == [0]
    assert rounds[0][0]["prefill_varlen"]["ctx_lens"].tolist() == [3, 0]
    assert [r[3]["counter"].tolist() for r in rounds] == [[4], [5], [6]]
    for j in (1, 2):
        dmd, dids, n, _ = rounds[j]
        assert dids is None and dmd["positions"].tolist() == [3 + j] and dmd["decode"]["seqlens"].tolist() == [4 + j]
        assert dmd["slot_mapping"].tolist() == [int(sa.slot_mapping[3 + j])] and dmd["last_rows"].tolist() == [0]
        assert dmd["decode"]["block_table"].tolist() == [sa.block_table.tolist()[:1] + [0] * (dmd["decode"]["block_table"].shape[1] - 1)]
    assert plan["sampling"]["position0"].tolist() == [4, 3, 11]
    # a accepts all three drafts, b emits its last token and leaves, c its first
    out = finish(eng, plan, [[1, 1, 1, 0], [0], [0]], [[-1, -1, -1, 9], [5], [6]], [[41, 42, 43], [], []])
    assert out == {b: [20, 21, 8, 5]}
    assert eng.active[a].tokens[:8].tolist() == [10, 11, 12, 7, 41, 42, 43, 9]
    assert eng.draft_computed == {a: 6, c: 11} and (eng.drafts_proposed, eng.drafts_accepted) == (3, 3)
    # next step: c has more room (3 drafts) than a (8 of 11 -> 2) and leads; a catches up two tokens, c one
    plan = eng._plan_spec_step()
    assert [s.id for s in plan["states"]] == [c, a] and plan["n_draft"] == [3, 2]
    dmd, dids, n, _ = plan["draft"][0]
    assert n == 2 and dids.tolist() == [6, 43, 9] and dmd["positions"].tolist() == [11, 6, 7]
    assert dmd["last_rows"].tolist() == [0, 2] and dmd["prefill_varlen"]["ctx_lens"].tolist() == [11, 6]
    assert [r[2] for r in plan["draft"]] == [2, 2, 1], "a sequence with g_s <= j sits round j out"
    assert plan["draft"][2][3]["counter"].tolist() == [14]
    assert plan["verify"][1].tolist() == [6, 0, 0, 0, 9, 0, 0] and plan["t_row0"] == [0, 4]
    # a rejection at row 1: one draft stays, the drafter's pages are valid up to it
    out = finish(eng, plan, [[1, 0, 1, 0], [1, 1, 0]], [[-1, 33, -1, 3], [-1, -1, 4]], [[51, 52, 53], [61, 62]])
    assert out == {a: [10, 11, 12, 7, 41, 42, 43, 9, 61, 62, 4]}
    assert eng.active[c].tokens[11:14].tolist() == [6, 51, 33] and eng.draft_computed == {c: 13}
    assert (eng.drafts_proposed, eng.drafts_accepted) == (8, 6)
    plan = eng._plan_spec_step()
    assert plan["n_draft"] == [1] and plan["draft"][0][1].tolist() == [33], "one catch-up token after a rejection"


def test_max_gen_len_one_never_drafts():
    eng = engine()
    a = eng.add_sequence([3, 4, 5], 1)
    plan = eng._plan_spec_step()
    assert plan["n_draft"] == [0]
    assert finish(eng, plan, [[0]], [[9]], [[]]) == {a: [3, 4, 5, 9]}
    assert eng.active == {} and eng.sampling == {} and eng.draft_computed == {}


def test_budget_under_max_step_tokens():
    """max_step_tokens 8, g = 3: the decoding sequence takes 1 + 3 rows, the prompt the 4 that are left."""
    eng = engine(max_batch_size=2, max_step_tokens=8)
    a = eng.add_sequence([10, 11, 12], 8)
    finish(eng, eng._plan_spec_step(), [[0]], [[7]], [[]])
    c = eng.add_sequence(list(range(30, 41)), 5)
    plan = eng._plan_spec_step()
    md, ids = plan["verify"]
    assert ids.tolist() == [7, 0, 0, 0, 30, 31, 32, 33] and md["last_rows"].tolist() == [0, 1, 2, 3]
    assert [s.id for s in plan["emitting"]] == [a] and plan["draft"][0][1].tolist() == [7, 30, 31, 32, 33]
    finish(eng, plan, [[0]], [[9]], [[41, 42, 43]])
    assert eng.active[c].num_computed == 4 and eng.active[c].is_prefill and eng.prompt_tokens_computed[c] == 4
    plan = eng._plan_spec_step()
    assert plan["verify"][1].tolist() == [9, 0, 0, 0, 34, 35, 36, 37]
    assert plan["verify"][0]["prefill_varlen"]["ctx_lens"].tolist() == [4, 4]


def test_sampling_parameters_ride_in_the_uploads():
    eng = engine()
    a = eng.add_sequence([10, 11, 12], 8, sampling=V.SamplingParams(0.5, top_k=7, top_p=0.9, seed=(1 << 63) + 5))
    b = eng.add_sequence([20, 21], 8)
    finish(eng, eng._plan_spec_step(), [[0], [0]], [[7], [8]], [[], []])
    plan = eng._plan_spec_step()
    sp = plan["sampling"]
    assert sp["inv_temperature"].tolist() == [2.0, 0.0] and sp["top_k"].tolist() == [7, 0]
    assert sp["seed"].tolist() == [5 - (1 << 63), 0] and sp["n_draft"].tolist() == [3, 3]
    assert sp["t_row0"].tolist() == [0, 4] and sp["position0"].tolist() == [4, 3]
    d0 = plan["draft"][0][3]
    assert d0["inv_temperature"].tolist() == [2.0, 0.0] and d0["counter"].tolist() == [4, 3]
    assert d0["seed"].tolist() == sp["seed"].tolist() and abs(d0["top_p"].tolist()[0] - 0.9) < 1e-6


# ---- the host finish -------------------------------------------------------------------------------------------


def _decoding(eng, prompt=(10, 11, 12), gen=8):
    sid = eng.add_sequence(list(prompt), gen)
    finish(eng, eng._plan_spec_step(), [[0]], [[7]], [[]])
    return sid


def test_finish_first_rejection_and_accept_all():
    eng = engine()
    sid = _decoding(eng)
    plan = eng._plan_spec_step()
    # accept[2] is set, but the first rejection is at row 1: rows after it do not count
    assert finish(eng, plan, [[1, 0, 1, 0]], [[-1, 30, -1, 31]], [[21, 22, 23]]) == {}
    s = eng.active[sid]
    assert s.tokens[:s.num_tokens].tolist() == [10, 11, 12, 7, 21, 30] and eng.draft_computed[sid] == 5
    assert (eng.drafts_proposed, eng.drafts_accepted) == (3, 1)
    plan = eng._plan_spec_step()
    finish(eng, plan, [[1, 1, 1, 0]], [[-1, -1, -1, 31]], [[24, 25, 26]])
    assert s.tokens[:s.num_tokens].tolist() == [10, 11, 12, 7, 21, 30, 24, 25, 26, 31] and eng.draft_computed[sid] == 8
    assert (eng.drafts_proposed, eng.drafts_accepted) == (6, 4)


def test_finish_stop_token_among_accepted_drafts():
    eng = engine(eos=[22])
    sid = _decoding(eng)
    out = finish(eng, eng._plan_spec_step(), [[1, 1, 1, 0]], [[-1, -1, -1, 31]], [[21, 22, 23]])
    assert out == {sid: [10, 11, 12, 7, 21, 22]}, "cut after the first stop token"
    assert eng.active == {} and eng.sampling == {} and eng.draft_computed == {}
    assert len(eng.kv_mgr.free_blocks) + len(eng.kv_mgr.evictable_blocks) == 32
    # a stop token that was drafted but rejected does not stop anything
    sid = _decoding(eng)
    assert finish(eng, eng._plan_spec_step(), [[1, 0, 0, 0]], [[-1, 30, -1, -1]], [[21, 22, 23]]) == {}
    # alt itself may be the stop token
    out = finish(eng, eng._plan_spec_step(), [[0, 0, 0, 0]], [[22, -1, -1, -1]], [[1, 2, 3]])
    assert out == {sid: [10, 11, 12, 7, 21, 30, 22]}


def test_finish_reaches_max_total_len_mid_round():
    """gen = 4 with g = 3: after the first token 3 are left, so 2 drafts + the token after them end the request in the
    middle of a round of three."""
    eng = engine()
    sid = _decoding(eng, gen=4)
    plan = eng._plan_spec_step()
    assert plan["n_draft"] == [2] and plan["verify"][1].tolist() == [7, 0, 0]
    assert [r[2] for r in plan["draft"]] == [1, 1]
    assert finish(eng, plan, [[1, 1, 0]], [[-1, -1, 9]], [[21, 22]]) == {sid: [10, 11, 12, 7, 21, 22, 9]}
    assert eng.active == {}
    # and one that ends by a rejection short of its length goes on
    sid = _decoding(eng, gen=4)
    assert finish(eng, eng._plan_spec_step(), [[0, 0, 0]], [[5, -1, -1]], [[21, 22]]) == {}
    plan = eng._plan_spec_step()
    assert plan["n_draft"] == [1]
    assert finish(eng, plan, [[1, 0]], [[-1, 6]], [[23]]) == {sid: [10, 11, 12, 7, 5, 23, 6]}


# ---- the default engine ----------------------------------------------------------------------------------------


def test_default_arguments_plan_what_they_planned():
    def drive(eng):
        out = []
        eng.add_sequence([10, 11, 12], 8, sampling=V.SamplingParams(0.7, top_k=5, seed=3))
        eng.add_sequence([20, 21], 8)
        for step in range(3):
            states, md, ids = eng._plan_step()
            flat = {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in md.items() if k not in ("decode", "prefill_varlen", "sampling")}
            for key in ("decode", "prefill_varlen", "sampling"):
                if md.get(key) is not None:
                    flat[key] = {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in md[key].items()}
            out.append(([s.id for s in states], ids.tolist(), flat))
            eng._finish_step(states, [7] * md["last_rows"].numel())
            if step == 0:
                eng.add_sequence(list(range(30, 41)), 8)
        return out

    for kw in (dict(), dict(varlen_prefill=True), dict(max_batch_size=4, max_step_tokens=6)):
        old = V.ContinuousBatchEngine(None, manager(), eos_token_ids=[], **kw)
        new = V.ContinuousBatchEngine(None, manager(), eos_token_ids=[], draft_model=None, draft_kv_mgr=None,
                                      num_speculative_tokens=0, **kw)
        assert not new.speculative and drive(old) == drive(new)
