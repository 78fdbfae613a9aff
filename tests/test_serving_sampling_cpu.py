"""Per-request sampling in the serving engine without a GPU: SamplingParams, the seeds add_sequence hands out, the
parameters a mixed step packs into its two uploads (and that it makes no third), and the C ABI of vy_sample_rows with
its argument errors."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import vyomai_amd as V
from vyomai_amd import _lib, ops, rng

BS = 8
NAME = "vy_sample_rows"


def config():
    return V.Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                    num_key_value_heads=1, max_position_embeddings=64, eos_token_id=1)


def engine(**kw):
    mgr = V.PagedKVManager(config(), 32, BS, "cpu", torch.float32)
    return V.ContinuousBatchEngine(None, mgr, eos_token_ids=[], **kw)


def f32(x):
    return float(np.float32(x))


# ---- SamplingParams --------------------------------------------------------------------------------------------


def test_sampling_params_validation():
    sp = V.SamplingParams()
    assert (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (0.0, 0, 0.0, None) and sp.greedy
    assert sp.inv_temperature == 0.0
    sp = V.SamplingParams(temperature=0.7, top_k=50, top_p=0.9, seed=-1)
    assert not sp.greedy and sp.seed == (1 << 64) - 1 and sp.inv_temperature == f32(1.0 / 0.7)
    assert V.SamplingParams(top_p=1.0).top_p == 1.0 and V.SamplingParams(top_p=0).top_p == 0.0
    for bad in (-0.1, float("inf"), float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            V.SamplingParams(temperature=bad)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            V.SamplingParams(temperature=1.0, top_k=bad)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            V.SamplingParams(temperature=1.0, top_p=bad)
    from vyomai_amd import serving
    assert serving.SamplingParams is V.SamplingParams


def test_add_sequence_resolves_seeds():
    eng = engine()
    rng.manual_seed(1234)
    g = eng.add_sequence([3, 4], 2)
    a = eng.add_sequence([3, 4], 2, sampling=V.SamplingParams(0.8))
    b = eng.add_sequence([3, 4], 2, sampling=V.SamplingParams(0.8, top_k=5))
    c = eng.add_sequence([3, 4], 2, sampling=V.SamplingParams(0.8, seed=77))
    z = eng.add_sequence([3, 4], 2, sampling=V.SamplingParams(0.0, top_k=5))       # temperature 0: greedy, no seed drawn
    assert eng.sampling[g].greedy and eng.sampling[g].seed is None and eng.sampling[z].seed is None
    assert eng.sampling[c].seed == 77 and eng.sampling[b].top_k == 5 and eng.sampling[a].temperature == 0.8
    sa, sb = eng.sampling[a].seed, eng.sampling[b].seed
    assert sa is not None and sb is not None and sa != sb and 0 <= sa < 1 << 64 and 0 <= sb < 1 << 64
    # the same stream again after reseeding, another one after another seed; torch.manual_seed governs the default
    eng2 = engine()
    rng.manual_seed(1234)
    assert [eng2.sampling[eng2.add_sequence([5], 1, sampling=V.SamplingParams(1.0))].seed for _ in range(2)] == [sa, sb]
    rng.manual_seed(1235)
    assert eng2.sampling[eng2.add_sequence([5], 1, sampling=V.SamplingParams(1.0))].seed not in (sa, sb)
    saved = dict(rng._state)
    try:
        rng._state.update(seed=None, offset=0)
        torch.manual_seed(99)
        t1 = eng2.sampling[eng2.add_sequence([5], 1, sampling=V.SamplingParams(1.0))].seed
        rng._state.update(seed=None, offset=0)
        torch.manual_seed(99)
        assert eng2.sampling[eng2.add_sequence([5], 1, sampling=V.SamplingParams(1.0))].seed == t1
        rng._state.update(seed=None, offset=0)
        torch.manual_seed(100)
        assert eng2.sampling[eng2.add_sequence([5], 1, sampling=V.SamplingParams(1.0))].seed != t1
    finally:
        rng._state.update(saved)
    with pytest.raises(ValueError, match="SamplingParams"):
        eng.add_sequence([3], 1, sampling={"temperature": 1.0})


def test_parameters_leave_with_the_request():
    eng = engine()
    sid = eng.add_sequence([3, 4, 5], 1, sampling=V.SamplingParams(0.5, seed=9))
    states, metadata, _ = eng._plan_step()
    assert sid in eng.sampling
    assert eng._finish_step(states, [11]) == {sid: [3, 4, 5, 11]}
    assert eng.sampling == {} and eng.active == {}


# ---- the packed uploads ----------------------------------------------------------------------------------------

SEED_HI = 0xFEDCBA9876543210           # the top bit set: rides as a negative int64


def _mixed(eng, sampled=True):
    """Four requests; after one step the first two decode and the last two (added then) prefill."""
    sp = (lambda *a, **k: V.SamplingParams(*a, **k)) if sampled else (lambda *a, **k: None)
    ids = [eng.add_sequence([10, 11, 12], 8, sampling=sp(0.7, top_k=12, seed=5)),
           eng.add_sequence([20, 21], 8)]
    plan = eng._plan_step()
    eng._finish_step(plan[0], [7, 7])
    ids += [eng.add_sequence(list(range(30, 41)), 8, sampling=sp(3.0, top_p=0.9, seed=SEED_HI)),
            eng.add_sequence([50, 51, 52, 53], 8, sampling=sp(1.0, top_k=2 ** 40, top_p=1.0, seed=1 << 32))]
    return ids, plan


def _check_sampling(m, want):
    """want: per last row (temperature or 0, top_k, top_p, seed, counter)."""
    sp = m["sampling"]
    n = m["last_rows"].numel()
    assert n == len(want) and all(t.numel() == n for t in sp.values())
    assert sp["inv_temperature"].dtype == torch.float32 and sp["top_p"].dtype == torch.float32
    assert sp["top_k"].dtype == torch.int32 and sp["seed"].dtype == torch.long and sp["counter"].dtype == torch.long
    inv = [0.0 if t == 0 else f32(1.0 / t) for t, *_ in want]
    assert sp["inv_temperature"].tolist() == inv                               # bit for bit: fp32 values both
    assert sp["top_k"].tolist() == [min(w[1], 2 ** 31 - 1) for w in want]
    assert sp["top_p"].tolist() == [f32(w[2]) for w in want]
    assert [s & (2 ** 64 - 1) for s in sp["seed"].tolist()] == [w[3] for w in want]
    assert sp["counter"].tolist() == [w[4] for w in want]


class Uploads:
    """Counts what a step builds from host lists and moves to the device."""

    def __init__(self, monkeypatch):
        self.made = self.moved = 0
        real_tensor, real_to = torch.tensor, torch.Tensor.to

        def tensor(*a, **k):
            self.made += 1
            return real_tensor(*a, **k)

        def to(t, *a, **k):
            self.moved += 1
            return real_to(t, *a, **k)

        monkeypatch.setattr(torch, "tensor", tensor)
        monkeypatch.setattr(torch.Tensor, "to", to)

    def take(self):
        out, self.made, self.moved = (self.made, self.moved), 0, 0
        return out


def test_first_step_of_a_mixed_batch():
    eng = engine()
    ids, (states, m, input_ids) = _mixed(eng)
    # both prefill and emit: the sampled request draws position 3, the greedy one rides along with inv_temperature 0
    assert m["last_rows"].tolist() == [2, 4] and input_ids.tolist() == [10, 11, 12, 20, 21]
    _check_sampling(m, [(0.7, 12, 0.0, 5, 3), (0, 0, 0.0, 0, 2)])
    assert m["positions"].tolist() == [0, 1, 2, 0, 1] and m["slot_mapping"].numel() == 5


@pytest.mark.parametrize("kw", [dict(), dict(varlen_prefill=True)], ids=["default", "varlen"])
def test_mixed_step_uploads(kw, monkeypatch):
    eng, ref = engine(**kw), engine(**kw)
    ids, _ = _mixed(eng)
    _mixed(ref, sampled=False)
    count = Uploads(monkeypatch)
    states, m, input_ids = eng._plan_step()
    n_sampled = count.take()
    rstates, rm, rinput = ref._plan_step()
    n_greedy = count.take()
    assert n_sampled == n_greedy == (2, 2), "a sampled step makes the two uploads of a greedy one"
    assert "sampling" not in rm and set(m) == set(rm) | {"sampling"}
    # two decoding rows, then the prompts of 11 and 4: every sequence emits
    assert m["last_rows"].tolist() == rm["last_rows"].tolist() == [0, 1, 12, 16]
    assert input_ids.tolist() == rinput.tolist()
    for key in ("positions", "slot_mapping"):
        assert m[key].tolist() == rm[key].tolist()
    assert m["decode"]["rows"].tolist() == [0, 1] and m["decode"]["seqlens"].tolist() == [4, 3]
    assert m["decode"]["block_table"].tolist() == rm["decode"]["block_table"].tolist()
    if kw:
        assert m["prefill_varlen"]["cu_q"].tolist() == [2, 13, 17]
        assert m["prefill_varlen"]["block_table"].tolist() == rm["prefill_varlen"]["block_table"].tolist()
    _check_sampling(m, [(0.7, 12, 0.0, 5, 4), (0, 0, 0.0, 0, 3), (3.0, 0, 0.9, SEED_HI, 11), (1.0, 2 ** 40, 1.0, 1 << 32, 4)])
    # the next step: all four decode, the counters moved by one
    eng._finish_step(states, [7, 7, 7, 7])
    states, m, _ = eng._plan_step()
    _check_sampling(m, [(0.7, 12, 0.0, 5, 5), (0, 0, 0.0, 0, 4), (3.0, 0, 0.9, SEED_HI, 12), (1.0, 2 ** 40, 1.0, 1 << 32, 5)])


def test_chunked_step_uploads(monkeypatch):
    """max_step_tokens = 6: the two decoding rows, then 4 of the 11-token prompt; the 4-token prompt sits the step out.
    Only the decoding rows emit, and the unfinished chunk draws nothing."""
    eng, ref = engine(max_batch_size=4, max_step_tokens=6), engine(max_batch_size=4, max_step_tokens=6)
    ids, _ = _mixed(eng)
    _mixed(ref, sampled=False)
    count = Uploads(monkeypatch)
    states, m, input_ids = eng._plan_step()
    n_sampled = count.take()
    rm = ref._plan_step()[1]
    assert n_sampled == count.take() == (2, 2)
    assert input_ids.tolist() == [7, 7, 30, 31, 32, 33] and m["last_rows"].tolist() == [0, 1]
    assert m["prefill_varlen"]["cu_q"].tolist() == rm["prefill_varlen"]["cu_q"].tolist() == [2, 6]
    assert m["prefill_varlen"]["block_table"].tolist() == rm["prefill_varlen"]["block_table"].tolist()
    _check_sampling(m, [(0.7, 12, 0.0, 5, 4), (0, 0, 0.0, 0, 3)])
    eng._finish_step(states, [7, 7])
    states, m, _ = eng._plan_step()                     # 2 decode rows + 4 more prompt tokens
    _check_sampling(m, [(0.7, 12, 0.0, 5, 5), (0, 0, 0.0, 0, 4)])
    eng._finish_step(states, [7, 7])
    states, m, input_ids = eng._plan_step()             # the last 3 tokens of the long prompt and 1 of the short one
    assert input_ids.tolist() == [7, 7, 38, 39, 40, 50] and m["last_rows"].tolist() == [0, 1, 4]
    _check_sampling(m, [(0.7, 12, 0.0, 5, 6), (0, 0, 0.0, 0, 5), (3.0, 0, 0.9, SEED_HI, 11)])
    # a step whose emitting rows are all greedy is the greedy step, whatever still prefills beside them
    eng2 = engine(max_batch_size=4, max_step_tokens=4)
    eng2.add_sequence([20, 21], 8)
    eng2._finish_step(eng2._plan_step()[0], [7])
    eng2.add_sequence(list(range(30, 41)), 8, sampling=V.SamplingParams(0.9, seed=3))
    assert "sampling" not in eng2._plan_step()[1]


# ---- ABI -------------------------------------------------------------------------------------------------------


def test_header_binding_and_library_agree_on_the_symbol():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    declared = set(re.findall(r"\b(vy_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert NAME in declared and NAME in _lib.ALL_SYMBOLS and NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    proto = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(_lib.PROTOTYPES[NAME]) == proto.count(",") + 1 == 12
    at = hdr.index("int " + NAME + "(")
    assert "logits_processors.py:13-16" in hdr[hdr.rindex("/* " + NAME, 0, at):at], "the entry cites the reference's lines"
    assert _lib.load().vy_abi_version() == 5            # the symbol is additive


def test_argument_errors_are_reported_without_a_gpu():
    raw = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(raw) + 255) // 256 * 256

    def go(logits=p, ldl=64, R=2, V=37, dtype=1, inv_t=p, top_k=p, top_p=p, seed=p, counter=p, tokens=p):
        _lib.call(NAME, logits, ldl, R, V, dtype, inv_t, top_k, top_p, seed, counter, tokens, None)

    for name in ("logits", "inv_t", "top_k", "top_p", "seed", "counter", "tokens"):
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*vy_sample_rows: null operand"):
            go(**{name: None})
    for bad in (dict(R=0), dict(R=-3), dict(V=0), dict(V=-1), dict(V=0x7ffffff1, ldl=0x7ffffff8), dict(ldl=36)):
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*vy_sample_rows: bad shape"):
            go(**bad)
    for bad in (2, -1):
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*vy_sample_rows: bad dtype"):
            go(dtype=bad)


def test_wrapper_raises_value_errors():
    R, Vv = 3, 16
    x = torch.zeros(R, Vv)
    f, i, l = torch.zeros(R), torch.zeros(R, dtype=torch.int32), torch.zeros(R, dtype=torch.long)
    with pytest.raises(ValueError, match="logits"):
        ops.sample_rows(torch.zeros(Vv), f, i, f, l, l)
    with pytest.raises(ValueError, match="logits"):
        ops.sample_rows(x.t(), f, i, f, l, l)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        ops.sample_rows(x.half(), f, i, f, l, l)
    with pytest.raises(ValueError, match="inv_temperature"):
        ops.sample_rows(x, f.double(), i, f, l, l)
    with pytest.raises(ValueError, match="top_k"):
        ops.sample_rows(x, f, l, f, l, l)
    with pytest.raises(ValueError, match="top_p"):
        ops.sample_rows(x, f, i, f[:2], l, l)
    with pytest.raises(ValueError, match="seed"):
        ops.sample_rows(x, f, i, f, i, l)
    with pytest.raises(ValueError, match="counter"):
        ops.sample_rows(x, f, i, f, l, torch.zeros(2 * R, dtype=torch.long)[::2])
    with pytest.raises(ValueError, match="is on"):
        ops.sample_rows(x, f.to("meta"), i, f, l, l)
    with pytest.raises(_lib.VyomHipError, match="CPU tensor"):       # no fallback
        ops.sample_rows(x, f, i, f, l, l)
