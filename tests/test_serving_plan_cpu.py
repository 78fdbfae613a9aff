"""The shared parts under the serving engine's two step planners, without a GPU (model=None): the packer of the step's
two uploads, the slot formula, and that the plain and the speculative planner -- both built on one segment builder and
one prompt-chunk loop -- plan the same forward where they should."""
import numpy as np
import pytest
import torch

import vyomai_amd as V
from vyomai_amd.serving import _StepUploads
from tests.test_serving_sampling_cpu import Uploads

BS = 8


def manager():
    config = V.Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, max_position_embeddings=64, eos_token_id=1)
    return V.PagedKVManager(config, 32, BS, "cpu", torch.float32)


def bits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


# ---- the packer ------------------------------------------------------------------------------------------------


def test_packer_hands_back_every_entry_by_name(monkeypatch):
    up = _StepUploads()
    up.put64("ids", [5, 6, 7])
    up.put32("pos", [0, 1, 2])
    up.put64("none64", [])
    up.put32("floats", [bits(1 / 0.7), bits(0.9)])
    up.put32("none32", [])
    up.put64("seed", [-(1 << 63), (1 << 63) - 1])
    up.put32("k", [0x7fffffff])
    count = Uploads(monkeypatch)
    at = up.upload("cpu")
    assert count.take() == (2, 2), "one torch.tensor and one .to per buffer"
    want = {"ids": [5, 6, 7], "pos": [0, 1, 2], "none64": [], "none32": [], "seed": [-(1 << 63), (1 << 63) - 1],
            "k": [0x7fffffff], "floats": [bits(1 / 0.7), bits(0.9)]}
    assert sorted(at) == sorted(want)
    for name, values in want.items():
        assert at[name].tolist() == values, name
        assert at[name].dtype == (torch.long if name in ("ids", "none64", "seed") else torch.int32), name
    f = at["floats"].view(torch.float32)
    assert f.tolist() == [float(np.float32(1 / 0.7)), float(np.float32(0.9))]             # bit for bit
    assert at["none32"].view(torch.float32).numel() == 0
    # views, not copies: the entries of one dtype lie behind one another in one tensor
    assert at["pos"].data_ptr() + 3 * 4 == at["floats"].data_ptr() == f.data_ptr()
    assert at["ids"].data_ptr() + 3 * 8 == at["seed"].data_ptr()
    assert count.take() == (0, 0), "handing out views builds and moves nothing"


def test_packer_refuses_a_name_that_was_never_put():
    up = _StepUploads()
    up.put32("pos", [1])
    at = up.upload("cpu")
    for name in ("positions", "", "pos "):
        with pytest.raises(KeyError):
            at[name]
    with pytest.raises(AssertionError, match="already"):          # put twice, one of the two would be lost
        up.put64("pos", [2])


# ---- the two planners ------------------------------------------------------------------------------------------


def _listed(x):
    return x.tolist() if torch.is_tensor(x) else x


@pytest.mark.parametrize("budget", [None, 8], ids=["whole prompts", "max_step_tokens"])
def test_first_speculative_step_verifies_what_the_plain_step_runs(budget):
    """Nothing decodes in a first step, so the verification forward is the plain engine's prefill: every tensor and
    scalar of the metadata, the ids, and the sampling parameters.  8 is the smallest budget a speculative engine of 2
    sequences with g = 3 takes, 2 * (3 + 1): the first prompt's 6 tokens leave 2 of the second's 5, a chunk with no
    logits row.  (max_position: the plain step passes its longest sequence, the verification its furthest segment
    end; the prompt that goes whole is the longest, so they agree.)"""
    kw = dict(max_batch_size=2, eos_token_ids=[], varlen_prefill=True, max_step_tokens=budget)
    plain = V.ContinuousBatchEngine(None, manager(), **kw)
    spec = V.ContinuousBatchEngine(None, manager(), draft_kv_mgr=manager(), num_speculative_tokens=3, **kw)
    for eng in (plain, spec):
        eng.add_sequence([10, 11, 12, 13, 14, 15], 8,
                         sampling=V.SamplingParams(0.7, top_k=12, top_p=0.9, seed=(1 << 63) + 5))
        eng.add_sequence([20, 21, 22, 23, 24], 8)
    states, md, ids = plain._plan_step()
    plan = spec._plan_spec_step()
    vmd, vids = plan["verify"]
    chunked = budget is not None
    assert ids.tolist() == vids.tolist() == [10, 11, 12, 13, 14, 15, 20, 21] + ([] if chunked else [22, 23, 24])
    assert [s.id for s in states] == [s.id for s in plan["states"]] == [0, 1]
    assert [s.chunk_end for s in states] == [s.chunk_end for s in plan["states"]] == [6, 2 if chunked else 5]
    sampling = md.pop("sampling")
    assert sorted(md) == sorted(vmd) and md["decode"] is None and vmd["decode"] is None
    assert md["prefill"] == vmd["prefill"] == []
    for key in ("positions", "slot_mapping", "last_rows", "max_position"):
        assert _listed(md[key]) == _listed(vmd[key]), key
    assert md["last_rows"].tolist() == ([5] if chunked else [5, 10]) and md["max_position"] == 6
    assert sorted(md["prefill_varlen"]) == sorted(vmd["prefill_varlen"])
    for key, value in md["prefill_varlen"].items():
        assert _listed(value) == _listed(vmd["prefill_varlen"][key]), key
    assert md["prefill_varlen"]["cu_q"].tolist() == [0, 6, 8 if chunked else 11]
    # one wire format of the sampling parameters: what vy_sample_rows would get is what vy_spec_verify gets
    judged = plan["sampling"]
    for key in ("inv_temperature", "top_k", "top_p", "seed"):
        assert sampling[key].tolist() == judged[key].tolist() and sampling[key].dtype == judged[key].dtype, key
    assert sampling["counter"].tolist() == judged["position0"].tolist() == ([6] if chunked else [6, 5])
    assert sampling["inv_temperature"].tolist()[0] == float(np.float32(1 / 0.7))
    assert sampling["seed"].tolist()[0] == 5 - (1 << 63)
    # and the drafter prefills the same segments
    dmd, dids, n, _ = plan["draft"][0]
    assert n == 0 and dids.tolist() == ids.tolist()
    assert dmd["prefill_varlen"]["cu_q"].tolist() == md["prefill_varlen"]["cu_q"].tolist()
    # both count the chunk and leave the same state behind
    assert plain.prompt_tokens_computed == spec.prompt_tokens_computed == {0: 6, 1: 2 if chunked else 5}
    assert list(plain.kv_mgr.free_blocks) == list(spec.kv_mgr.free_blocks)


# ---- the slot formula ------------------------------------------------------------------------------------------


def test_map_slots_and_update_metadata_write_their_range_only():
    s = V.SequenceState(0, list(range(20)), 4, BS)
    s.block_table[:3] = torch.tensor([5, 2, 7], dtype=torch.int32)
    s.block_count = 3
    s.slot_mapping.fill_(-1)
    s.map_slots(6, 11)                                  # straddles the boundary between blocks 0 and 1
    want = [int(s.block_table[i // 8]) * 8 + i % 8 for i in range(6, 11)]
    assert want == [46, 47, 16, 17, 18] and s.slot_mapping[6:11].tolist() == want
    assert s.slot_mapping[:6].tolist() == [-1] * 6 and s.slot_mapping[11:].tolist() == [-1] * 13
    # update_metadata(): the same formula over [query_start, query_end), here a chunk in the middle of the prompt
    s.slot_mapping.fill_(-1)
    s.num_computed, s.chunk_end = 14, 19
    assert (s.query_start, s.query_end) == (14, 19)
    s.update_metadata()
    assert s.slot_mapping[14:19].tolist() == [2 * 8 + 6, 2 * 8 + 7, 7 * 8, 7 * 8 + 1, 7 * 8 + 2]
    assert s.slot_mapping[13] == -1 and s.slot_mapping[19] == -1 and int((s.slot_mapping != -1).sum()) == 5
    # a decoding sequence: its last token alone
    s.slot_mapping.fill_(-1)
    s.is_prefill, s.chunk_end = False, None
    s.update_metadata()
    assert s.slot_mapping[19] == 7 * 8 + 3 and int((s.slot_mapping != -1).sum()) == 1
