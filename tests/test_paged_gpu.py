"""Paged KV cache on the MI355X: the three kernels of vy_paged.hip against float64 on the same inputs, and the
continuous-batching engine (vyomai_amd/serving.py) against the reference model's greedy ids (tests/golden/causal_lm.npz)
and, in bf16, against the model's own dense forward."""
import math

import pytest
import torch

from tests.attn_range import GAINS, paged_decode_period, stair_levels
from tests.golden import cases_causal_lm as C
from tests.test_causal_lm_gpu import build, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
UNIT = {torch.float32: 2.0 ** -24, BF: 2.0 ** -8}      # unit roundoff of the storage type


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ------------------------------------------------------------------------------------------
# vy_paged_rope_write
# ------------------------------------------------------------------------------------------


@DTYPES
@pytest.mark.parametrize("h,hk,dh", [(4, 2, 64), (2, 1, 224), (8, 2, 128)])
def test_rope_write_vs_fp64(h, hk, dh, dtype):
    """37 tokens of three sequences that start at positions 0, 5 and 100, 16-token blocks in shuffled physical order, one
    token with a negative slot.  Bound (derived): the rotation a c - b s is evaluated in fp32 from exact inputs -- two
    products and a sum, at most 3 * 2^-24 (|a| + |b|), taken as 4 * 2^-24 -- and stored with ONE rounding, u |want|
    with u = 2^-8 (bf16) or 2^-24 (fp32).  The scattered k rows are the bits of the in-place rows, v rows the bits of
    the input; every slot outside slot_mapping, and the slot the dropped token would have taken, keeps its sentinel."""
    from vyomai_amd import ops
    g = torch.Generator().manual_seed(dh + h)
    bs, nblk, table_rows = 16, 12, 160
    seqs = [(0, 20), (5, 16), (100, 1)]                  # (first position, tokens)
    order = torch.randperm(nblk, generator=g).tolist()
    pos, slots = [], []
    for first, n in seqs:
        blocks = [order.pop() for _ in range((first + n + bs - 1) // bs)]
        for p in range(first, first + n):
            pos.append(p)
            slots.append(blocks[p // bs] * bs + p % bs)
    ntok = len(pos)
    assert ntok == 37
    dropped = 11
    want_slots = list(slots)
    slots[dropped] = -1
    qkv = torch.randn(ntok, (h + 2 * hk) * dh, generator=g).to(dtype)
    inv = 1.0 / (1e6 ** (torch.arange(0, dh, 2).float() / dh))
    ang = torch.outer(torch.arange(table_rows).float(), inv)
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    sentinel = 7.5
    kc = torch.full((nblk, bs, hk, dh), sentinel, dtype=dtype, device=DEV)
    vc = torch.full_like(kc, sentinel)
    got = qkv.to(DEV)
    ops.paged_rope_write_(got, torch.tensor(pos, dtype=torch.int32, device=DEV), torch.tensor(slots, device=DEV),
                          cos.to(DEV), sin.to(DEV), h, kc, vc)
    torch.cuda.synchronize()
    got, kc, vc = got.cpu(), kc.cpu(), vc.cpu()
    # q and k heads against the float64 rotation of the same inputs
    x = qkv.double().view(ntok, h + 2 * hk, dh)
    c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    a, b = x[..., :dh // 2], x[..., dh // 2:]
    want = torch.cat([a * c - b * s, b * c + a * s], dim=-1)[:, :h + hk]
    mag = (a.abs() + b.abs())[:, :h + hk].repeat(1, 1, 2)
    g3 = got.view(ntok, h + 2 * hk, dh)
    err = (g3[:, :h + hk].double() - want).abs()
    bound = UNIT[dtype] * want.abs() + 4 * 2.0 ** -24 * mag
    print(f"rope max err / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert (err <= bound).all()
    assert torch.equal(bits(g3[:, h + hk:]), bits(qkv.view(ntok, h + 2 * hk, dh)[:, h + hk:])), "v changed in place"
    # the pages
    kf, vf = kc.view(nblk * bs, hk, dh), vc.view(nblk * bs, hk, dh)
    live = torch.tensor([sl for sl in slots if sl >= 0])
    rows = torch.tensor([t for t, sl in enumerate(slots) if sl >= 0])
    assert torch.equal(bits(kf[live]), bits(g3[rows, h:h + hk]))
    assert torch.equal(bits(vf[live]), bits(g3[rows, h + hk:]))
    untouched = torch.ones(nblk * bs, dtype=torch.bool)
    untouched[live] = False
    assert untouched[want_slots[dropped]]
    fill = torch.full((int(untouched.sum()), hk, dh), sentinel, dtype=dtype)
    assert torch.equal(bits(kf[untouched]), bits(fill)) and torch.equal(bits(vf[untouched]), bits(fill))


# ------------------------------------------------------------------------------------------
# vy_paged_gather
# ------------------------------------------------------------------------------------------


@DTYPES
@pytest.mark.parametrize("hk,dh", [(2, 64), (1, 224)])
def test_gather_equals_indexing(hk, dh, dtype):
    from vyomai_amd import ops
    g = torch.Generator().manual_seed(3)
    bs, nblk = 16, 7
    kc = torch.randn(nblk, bs, hk, dh, generator=g).to(dtype)
    vc = torch.randn(nblk, bs, hk, dh, generator=g).to(dtype)
    table = torch.tensor([5, 0, 6], dtype=torch.int32)
    for S in (1, 15, 16, 17, 40):
        k, v = ops.paged_gather(kc.to(DEV), vc.to(DEV), table.to(DEV), S)
        j = torch.arange(S)
        idx = table[j // bs].long() * bs + j % bs
        for got, pages in ((k, kc), (v, vc)):
            want = pages.view(nblk * bs, hk, dh)[idx].permute(1, 0, 2).contiguous()
            assert got.shape == (hk, S, dh) and torch.equal(bits(got.cpu()), bits(want)), S


# ------------------------------------------------------------------------------------------
# vy_attn_paged_decode
# ------------------------------------------------------------------------------------------

SEQLENS = [1, 15, 16, 17, 255, 256, 257, 600, 1300]


def _decode_case(dh, h, hk, bs, dtype, regime, seed):
    """One batch of the nine lengths: pages in shuffled physical order, NaN in the key rows >= seqlen of every last
    page and in one spare page that every block-table entry past a sequence's pages points at; q rows picked by a
    permutation out of a buffer shaped like the packed QKV rows.  -> inputs and the float64 result per sequence."""
    g = torch.Generator().manual_seed(seed)
    B = len(SEQLENS)
    pages = [(s + bs - 1) // bs for s in SEQLENS]
    nblk = sum(pages) + 1
    order = torch.randperm(nblk, generator=g).tolist()
    poison = order.pop()
    kc = torch.full((nblk, bs, hk, dh), float("nan"))
    vc = torch.full((nblk, bs, hk, dh), float("nan"))
    table = torch.full((B, max(pages) + 2), poison, dtype=torch.int32)
    ks, vs = [], []
    for b, S in enumerate(SEQLENS):
        blocks = [order.pop() for _ in range(pages[b])]
        table[b, :pages[b]] = torch.tensor(blocks, dtype=torch.int32)
        k = torch.randn(S, hk, dh, generator=g)
        if regime == "staircase":   # tests/attn_range.py: a score ramp of one level per trip of the workgroup
            k *= 0.5
            k[..., 0] = stair_levels(S, paged_decode_period(dh, dtype))[:, None]
        k = k.to(dtype).float()
        v = torch.randn(S, hk, dh, generator=g).to(dtype).float()
        slot = torch.tensor([blocks[j // bs] * bs + j % bs for j in range(S)])
        kc.view(-1, hk, dh)[slot] = k
        vc.view(-1, hk, dh)[slot] = v
        ks.append(k)
        vs.append(v)
    kvh = torch.arange(h) // (h // hk)
    qs = []
    for b, S in enumerate(SEQLENS):
        if regime == "flat":
            q = torch.randn(h, dh, generator=g)
        elif regime == "staircase":   # the query row sits at position S - 1: its gain, 4 / 6 / 12 nat a level
            q = torch.randn(h, dh, generator=g)
            q[:, 0] = math.sqrt(dh) * GAINS[(S - 1) % len(GAINS)]
        else:      # peaked: q = 6 k[j*], j* in the sequence's last page (tests/test_decode_kernels_gpu.py's regime)
            jstar = torch.randint((S - 1) // bs * bs, S, (h,), generator=g)
            q = 6.0 * ks[b][jstar, kvh]
        qs.append(q.to(dtype).float())
    rows = B + 3
    q_rows = torch.tensor([7, 2, 11, 0, 5, 9, 1, 10, 4], dtype=torch.int32)
    qbuf = torch.randn(rows, (h + 2 * hk) * dh, generator=g)
    for b in range(B):
        qbuf[q_rows[b], :h * dh] = qs[b].reshape(-1)
    want = []
    for b in range(B):
        kd = ks[b].double()[:, kvh]                                       # (S, h, dh)
        vd = vs[b].double()[:, kvh]
        p = torch.softmax(torch.einsum("hd,shd->hs", qs[b].double(), kd) / math.sqrt(dh), dim=-1)
        want.append(torch.einsum("hs,shd->hd", p, vd).reshape(-1))
    vmax = max(float(v.abs().max()) for v in vs)
    return (qbuf.to(dtype), q_rows, kc.to(dtype), vc.to(dtype), table, torch.tensor(SEQLENS, dtype=torch.int32),
            torch.stack(want), vmax)


@DTYPES
@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("h,hk", [(4, 4), (4, 2), (8, 1)])
@pytest.mark.parametrize("dh", [64, 128, 224])
def test_paged_decode_vs_fp64(dh, h, hk, bs, dtype):
    """Bound (derived, the one of test_decode_attention_every_instantiation): scores, softmax and the weighted sum in
    fp32 -- S * 2^-24 of accumulation with S <= 1300, the error of __expf -- and ONE rounding of the result:
    |got - want| <= r |want| + 1e-4 max|v| with r = 2^-8 for bf16 and 2^-20 for fp32.  The online rescaling and the
    combine of split partials stay in fp32, so the same derivation holds for every n_split; split and unsplit results
    each meet the bound (they are not compared with each other)."""
    from vyomai_amd import ops
    rel = 2.0 ** -8 if dtype == BF else 2.0 ** -20
    for regime in ("flat", "peaked", "staircase"):
        q, q_rows, kc, vc, table, seqlens, want, vmax = _decode_case(dh, h, hk, bs, dtype, regime, seed=dh + 7 * hk + bs)
        qd, rd, kd, vd, td, sd = (t.to(DEV) for t in (q, q_rows, kc, vc, table, seqlens))
        for n_split in (1, 2, 5, 0):
            out = torch.full((q.shape[0], h * dh), 3.25, dtype=dtype, device=DEV)
            ops.attention_paged_decode(qd, kd, vd, td, sd, max(SEQLENS), h, q_rows=rd, out=out, n_split=n_split)
            torch.cuda.synchronize()
            out = out.cpu()
            got = out[q_rows.long()].double()
            what = f"{regime} n_split={n_split}"
            assert torch.isfinite(got).all(), f"{what}: non-finite output (a key row >= seqlen or the poison page took part)"
            err = (got - want).abs()
            bound = rel * want.abs() + 1e-4 * vmax
            worst = float((err / bound).max())
            print(f"{what}: max err / bound {worst:.3f}")
            assert (err <= bound).all(), f"{what}: max err / bound {worst:.2f} (sequence {int((err / bound).max(dim=1).values.argmax())})"
            other = torch.ones(q.shape[0], dtype=torch.bool)
            other[q_rows.long()] = False
            assert (out[other] == 3.25).all(), f"{what}: rows outside q_rows were written"


@DTYPES
def test_paged_decode_seqlen_zero_writes_zeros(dtype):
    from vyomai_amd import ops
    h, hk, dh, bs = 4, 2, 64, 16
    kc = torch.full((3, bs, hk, dh), float("nan"), dtype=dtype, device=DEV)
    q = torch.randn(2, h * dh).to(dtype).to(DEV)
    table = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    for n_split in (1, 2):
        out = torch.full((2, h * dh), 3.25, dtype=dtype, device=DEV)
        ops.attention_paged_decode(q, kc, kc.clone(), table, torch.zeros(2, dtype=torch.int32, device=DEV), 32, h, out=out,
                                   n_split=n_split)
        assert (out == 0).all()


# ------------------------------------------------------------------------------------------
# the engine against the reference's greedy ids (fp32)
# ------------------------------------------------------------------------------------------

_MODELS = {}


def model(case, compute=None):
    key = (case if isinstance(case, str) else "dh128", compute)
    if key not in _MODELS:
        _MODELS[key] = build(C.CASES[case] if isinstance(case, str) else case, compute=compute).eval()
    return _MODELS[key]


def engine(m, block_size, max_blocks=16, dtype=torch.float32, **kw):
    import vyomai_amd as V
    mgr = V.PagedKVManager(m.config, max_blocks, block_size, DEV, dtype)
    return V.ContinuousBatchEngine(m, mgr, **kw), mgr


def drain(eng, limit=200):
    done = {}
    for _ in range(limit):
        if not (eng.active or eng.waiting_room):
            return done
        done.update(eng.step())
    raise AssertionError("the engine did not finish")


FP32_CASES = pytest.mark.parametrize("case,block_size", [("a", 8), ("a", 16), ("b", 8), ("b", 16)])


@FP32_CASES
def test_engine_all_at_once(golden, case, block_size):
    g = golden("causal_lm")
    eng, _ = engine(model(case), block_size, eos_token_ids=[])
    sids = [eng.add_sequence(g[f"{case}.prompt"][r].tolist(), max_gen_len=C.GREEDY_NEW) for r in range(C.B)]
    done = drain(eng)
    for r, sid in enumerate(sids):
        assert done[sid] == g[f"{case}.prompt"][r].tolist() + g[f"{case}.greedy"][r].tolist(), r


@FP32_CASES
def test_engine_staggered_mixed_steps(golden, case, block_size):
    """The second prompt arrives after three steps: its prefill shares a step with the first sequence's decode."""
    g = golden("causal_lm")
    eng, _ = engine(model(case), block_size, eos_token_ids=[])
    sid0 = eng.add_sequence(g[f"{case}.prompt"][0].tolist(), max_gen_len=C.GREEDY_NEW)
    done = {}
    for _ in range(3):
        done.update(eng.step())
    sid1 = eng.add_sequence(g[f"{case}.prompt"][1].tolist(), max_gen_len=C.GREEDY_NEW)
    done.update(drain(eng))
    for r, sid in enumerate((sid0, sid1)):
        assert done[sid] == g[f"{case}.prompt"][r].tolist() + g[f"{case}.greedy"][r].tolist(), r


@FP32_CASES
def test_engine_waiting_room(golden, case, block_size):
    """Blocks for one sequence's whole life only: the second request waits until the first is freed."""
    g = golden("causal_lm")
    total = C.PREFILL + C.GREEDY_NEW
    eng, mgr = engine(model(case), block_size, max_blocks=(total + block_size - 1) // block_size, eos_token_ids=[])
    sids = [eng.add_sequence(g[f"{case}.prompt"][r].tolist(), max_gen_len=C.GREEDY_NEW) for r in range(C.B)]
    done = eng.step()
    assert list(eng.active) == [sids[0]] and len(eng.waiting_room) == 1
    done.update(drain(eng))
    for r, sid in enumerate(sids):
        assert done[sid] == g[f"{case}.prompt"][r].tolist() + g[f"{case}.greedy"][r].tolist(), r
    assert sorted(list(mgr.free_blocks) + list(mgr.evictable_blocks)) == list(range(mgr.max_blocks))


@FP32_CASES
def test_engine_eos(golden, case, block_size):
    """eos = the id golden row 0 produces third (as test_generate_with_a_mask_and_with_eos picks it): that sequence
    finishes there, the other runs on to its own first eos or to the end."""
    g = golden("causal_lm")
    eos = int(g[f"{case}.greedy"][0, 2])
    eng, _ = engine(model(case), block_size, eos_token_ids=[eos])
    sids = [eng.add_sequence(g[f"{case}.prompt"][r].tolist(), max_gen_len=C.GREEDY_NEW) for r in range(C.B)]
    done = drain(eng)
    for r, sid in enumerate(sids):
        row = g[f"{case}.greedy"][r].tolist()
        cut = row.index(eos) + 1 if eos in row else len(row)
        assert done[sid] == g[f"{case}.prompt"][r].tolist() + row[:cut], r
    assert len(done[sids[0]]) <= C.PREFILL + 3 and eng.eos_token_ids == {eos}


@pytest.mark.parametrize("case", ["a", "b"])
def test_engine_prefix_hit(golden, case):
    """The 20-token prompt `prompt || greedy[:12]` twice through one manager (block_size 8): the second request takes
    the first one's two complete blocks, computes 4 prompt tokens, produces the same ids, and its first logits are
    within the fp32 logits bar (rel_err 2e-5) of a cold run of the same request on a fresh manager.  (Contexts here are
    at most 24 tokens, as in every engine test: the split-KV path is covered by test_paged_decode_vs_fp64 alone.)"""
    g = golden("causal_lm")
    ids = g[f"{case}.prompt"][0].tolist() + g[f"{case}.greedy"][0, :12].tolist()
    want = ids + g[f"{case}.greedy"][0, 12:16].tolist()
    eng, mgr = engine(model(case), 8, eos_token_ids=[], record_logits=True)
    first = eng.add_sequence(ids, max_gen_len=4)
    done = eng.step()
    first_blocks = eng.active[first].block_table[:2].tolist()
    done.update(drain(eng))
    assert done[first] == want and eng.prompt_tokens_computed[first] == 20
    warm = eng.add_sequence(ids, max_gen_len=4)
    done = eng.step()
    assert eng.active[warm].block_table[:2].tolist() == first_blocks and eng.active[warm].prefix_len == 16
    assert eng.prompt_tokens_computed[warm] == 4
    done.update(drain(eng))
    assert done[warm] == want
    fresh, _ = engine(model(case), 8, eos_token_ids=[], record_logits=True)
    cold = fresh.add_sequence(ids, max_gen_len=4)
    assert drain(fresh)[cold] == want and fresh.prompt_tokens_computed[cold] == 20
    e = rel_err(eng.logits[warm][0], fresh.logits[cold][0].numpy())
    print(f"first logits after a prefix hit against the cold run: rel_err {e:.3e}")
    assert e < 2e-5, e


# ------------------------------------------------------------------------------------------
# bf16: the engine's logits against the model's dense forward
# ------------------------------------------------------------------------------------------

DH128 = dict(C.CASES["a"], hidden_size=256, num_attention_heads=2, num_key_value_heads=1)


@pytest.mark.parametrize("case", ["a", "b", "dh128"])
def test_engine_bf16_logits_vs_dense_forward(golden, case):
    """No ids against the goldens (argmax ties flip in bf16): every finished sequence goes through the model's dense
    uncached forward, and the engine's per-step last-row logits must be within rel_err 3e-2 -- the bf16 logits bar of
    test_model_bf16_vs_reference -- of the dense logits at the same positions.  The second request arrives after two
    steps, so the mixed step is covered as well."""
    g = golden("causal_lm")
    m = model(DH128 if case == "dh128" else case, compute=BF)
    prompts = g["a.prompt" if case == "dh128" else f"{case}.prompt"]
    eng, _ = engine(m, 16, dtype=BF, eos_token_ids=[], record_logits=True)
    sids = [eng.add_sequence(prompts[0].tolist(), max_gen_len=C.GREEDY_NEW)]
    done = {}
    for _ in range(2):
        done.update(eng.step())
    sids.append(eng.add_sequence(prompts[1].tolist(), max_gen_len=C.GREEDY_NEW))
    done.update(drain(eng))
    for sid in sids:
        seq = done[sid]
        assert len(seq) == C.PREFILL + C.GREEDY_NEW and len(eng.logits[sid]) == C.GREEDY_NEW
        with torch.no_grad():
            dense = m(input_ids=torch.tensor([seq[:-1]], device=DEV), use_cache=False).logits[0, C.PREFILL - 1:]
        e = rel_err(torch.stack(eng.logits[sid]), dense.float().cpu().numpy())
        print(f"bf16 {case} sequence {sid}: engine logits against the dense forward rel_err {e:.3e}")
        assert e < 3e-2, e
