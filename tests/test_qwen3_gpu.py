"""Qwen3Model on the MI355X: vy_paged_qknorm_rope_write against float64 on the same inputs, and the continuous-batching
engine serving Qwen3Model against the REAL reference model's greedy ids and logits (tests/golden/qwen3.npz, made by
make_golden_qwen3.py from the model cell of Examples/simple_vllm.ipynb)."""
import numpy as np
import pytest
import torch

from tests.golden import cases_qwen3 as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
UNIT = {torch.float32: 2.0 ** -24, BF: 2.0 ** -8}      # unit roundoff of the storage type


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def rel_err(got, want):
    got = got.detach().float().cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


# ------------------------------------------------------------------------------------------
# vy_paged_qknorm_rope_write
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h,hk,dh", [(4, 2, 64), (2, 1, 224), (8, 2, 128), (1, 1, 8), (3, 1, 256), (2, 2, 96)])
def test_qknorm_rope_write_vs_fp64(h, hk, dh, dtype):
    """The layout of test_rope_write_vs_fp64: 37 tokens of three sequences that start at positions 0, 5 and 100,
    16-token blocks in shuffled physical order, one token with a negative slot, sentinel-filled pages.  The head widths
    take a lane group of 1 (dh 8), 8, 16, 32 (256) lanes, and the 12-of-16 (96) and 28-of-32 (224) groups with idle
    lanes.  Scales are 1 + 0.1 u; one q head and one k head of one token are all zeros.

    Bound (derived from the kernel's arithmetic, u = 2^-24, relative to the fp64 normalised pair a', b'):
      * sum of dh squares: an fma chain of 8 per lane, then log2(lanes) <= 5 adds -- at most 8 + 5 <= dh roundings on
        any path, all terms non-negative, so a relative error of at most dh u; through rsqrt it is halved: dh/2 u;
      * the mean (a product with the fp32 1/dh, itself rounded) and the eps add, one fma: <= 2 u, halved: 1 u;
      * rsqrt: 2 ulp = 4 u;
      * two products (x * r, then * scale): 2 u;
      * the rotation a' c - b' s: two products and a sum, 3 u (|a'| + |b'|) with |c|, |s| <= 1;
      total (dh/2 + 10) u, taken as (dh/2 + 12) u (|a'| + |b'|), plus ONE rounding at the store: u_store |want| with
      u_store = 2^-8 (bf16) or 2^-24 (fp32).
    v heads in place and in the pages are the bits of the input; k rows in the pages are the bits of the in-place rows;
    every slot outside slot_mapping, and the one the dropped token would have taken, keeps its sentinel."""
    from vyomai_amd import ops
    g = torch.Generator().manual_seed(dh + h)
    bs, nblk, table_rows, eps = 16, 12, 160, 1e-6
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
    dropped, zero_tok = 11, 23
    want_slots = list(slots)
    slots[dropped] = -1
    H3 = h + 2 * hk
    qkv = torch.randn(ntok, H3, dh, generator=g)
    qkv[zero_tok, h - 1] = 0.0                           # the last q head and the first k head of one token
    qkv[zero_tok, h] = 0.0
    qkv = qkv.view(ntok, H3 * dh).to(dtype)
    qs = (1.0 + 0.1 * (2 * torch.rand(dh, generator=g) - 1)).float()
    ks = (1.0 + 0.1 * (2 * torch.rand(dh, generator=g) - 1)).float()
    inv = 1.0 / (1e6 ** (torch.arange(0, dh, 2).float() / dh))
    ang = torch.outer(torch.arange(table_rows).float(), inv)
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    sentinel = 7.5
    kc = torch.full((nblk, bs, hk, dh), sentinel, dtype=dtype, device=DEV)
    vc = torch.full_like(kc, sentinel)
    got = qkv.to(DEV)
    ops.paged_qknorm_rope_write_(got, torch.tensor(pos, dtype=torch.int32, device=DEV), torch.tensor(slots, device=DEV),
                                 cos.to(DEV), sin.to(DEV), qs.to(DEV), ks.to(DEV), eps, h, kc, vc)
    torch.cuda.synchronize()
    got, kc, vc = got.cpu(), kc.cpu(), vc.cpu()
    assert not torch.isnan(got.float()).any() and not torch.isnan(kc.float()).any() and not torch.isnan(vc.float()).any()
    # q and k heads against float64 on the same inputs
    x = qkv.double().view(ntok, H3, dh)[:, :h + hk]
    scale = torch.cat([qs.double().expand(h, dh), ks.double().expand(hk, dh)])           # (h + hk, dh)
    n = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * scale
    c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    a, b = n[..., :dh // 2], n[..., dh // 2:]
    want = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    mag = (a.abs() + b.abs()).repeat(1, 1, 2)
    g3 = got.view(ntok, H3, dh)
    err = (g3[:, :h + hk].double() - want).abs()
    bound = UNIT[dtype] * want.abs() + (dh / 2 + 12) * 2.0 ** -24 * mag
    live_el = bound > 0
    print(f"qknorm + rope max err / bound {float((err[live_el] / bound[live_el]).max()):.3f}")
    assert (err <= bound).all()
    zero = g3[zero_tok, h - 1:h + 1].float()
    assert torch.isfinite(zero).all() and (zero == 0).all(), "an all-zero head must stay zero"
    assert torch.equal(bits(g3[:, h + hk:]), bits(qkv.view(ntok, H3, dh)[:, h + hk:])), "v changed in place"
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
# the engine against the reference's greedy ids and logits
# ------------------------------------------------------------------------------------------

_MODELS = {}


def model(case, dtype=torch.float32):
    import vyomai_amd as V
    if (case, dtype) not in _MODELS:
        _MODELS[case, dtype] = C.build(V.Qwen3Model, case, dtype).to(DEV)
    return _MODELS[case, dtype]


def engine(m, block_size, max_blocks=16, dtype=torch.float32, **kw):
    import vyomai_amd as V
    mgr = V.PagedKVManager(m.config, max_blocks, block_size, DEV, dtype)
    return V.ContinuousBatchEngine(m, mgr, eos_token_ids=[], record_logits=True, **kw), mgr


def drain(eng, limit=200):
    done = {}
    for _ in range(limit):
        if not (eng.active or eng.waiting_room):
            return done
        done.update(eng.step())
    raise AssertionError("the engine did not finish")


def serve(eng, prompts, second_after):
    """Both prompts through the engine, the second one added after `second_after` steps -> ({sid: ids}, sids)."""
    sids, done = [eng.add_sequence(prompts[0].tolist(), max_gen_len=C.GREEDY_NEW)], {}
    for _ in range(second_after):
        done.update(eng.step())
    sids.append(eng.add_sequence(prompts[1].tolist(), max_gen_len=C.GREEDY_NEW))
    done.update(drain(eng))
    return done, sids


SCHEDULES = {"all_at_once": (0, {}), "staggered": (3, {}), "chunked": (0, dict(varlen_prefill=True, max_step_tokens=8))}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("block_size", [8, 16])
@pytest.mark.parametrize("case", list(C.CASES))
def test_engine_fp32_ids_and_logits(golden, case, block_size, schedule):
    """all_at_once: both prompts prefilled in one step; staggered: the second prompt arrives after three steps, so its
    prefill shares a step with the first sequence's decode; chunked: one varlen prefill launch under a budget of 8
    tokens a step, so the second prompt goes in chunks beside the first one's decode.  Ids equal prompt + the
    reference's greedy ids; every step's logits are within the fp32 logits bar (rel_err 2e-5, as
    test_engine_prefix_hit) of the reference's logits at the same position."""
    g = golden("qwen3")
    after, kw = SCHEDULES[schedule]
    eng, _ = engine(model(case), block_size, **kw)
    done, sids = serve(eng, g[f"{case}.prompt"], after)
    for r, sid in enumerate(sids):
        assert done[sid] == g[f"{case}.prompt"][r].tolist() + g[f"{case}.greedy"][r].tolist(), r
        e = rel_err(C.sub_v(torch.stack(eng.logits[sid])), g[f"{case}.logits"][r])
        print(f"{case} bs {block_size} {schedule} sequence {r}: logits rel_err {e:.3e}")
        assert e < 2e-5, e


def test_engine_prefix_hit(golden):
    """Case q, built like the causal LM's test_engine_prefix_hit: the 20-token prompt `prompt || greedy[:12]` twice
    through one manager (block_size 8).  The second request takes the first one's two complete blocks -- pages filled
    through the fused kernel -- computes 4 prompt tokens, produces the same ids, and its first logits are within the
    fp32 logits bar of a cold run of the same request on a fresh manager."""
    g = golden("qwen3")
    ids = g["q.prompt"][0].tolist() + g["q.greedy"][0, :12].tolist()
    want = ids + g["q.greedy"][0, 12:16].tolist()
    eng, mgr = engine(model("q"), 8)
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
    fresh, _ = engine(model("q"), 8)
    cold = fresh.add_sequence(ids, max_gen_len=4)
    assert drain(fresh)[cold] == want and fresh.prompt_tokens_computed[cold] == 20
    e = rel_err(eng.logits[warm][0], fresh.logits[cold][0].numpy())
    print(f"first logits after a prefix hit against the cold run: rel_err {e:.3e}")
    assert e < 2e-5, e
    e = rel_err(C.sub_v(torch.stack(eng.logits[warm])), g["q.logits"][0, 12:16])
    assert e < 2e-5, e


@pytest.mark.parametrize("case", ["q", "r"])
def test_engine_bf16_logits(golden, case):
    """No ids (argmax ties flip in bf16): after every step the test overwrites the id the engine just appended with the
    reference's id at that position, so each sequence's context is the reference's at every step and every logits row
    sits at a position the golden file has.  Per-step logits against the reference's fp32 logits: rel_err 3e-2, the
    project's bf16 logits bar (the maker shows that the reference's own bf16 forward meets it).  The second prompt
    arrives after two steps (a mixed step).  Then row 0's first 23 tokens once more as a prompt: it starts from a
    cached prefix block that the fused kernel wrote in bf16."""
    g = golden("qwen3")
    prompts, greedy = g[f"{case}.prompt"], g[f"{case}.greedy"]
    eng, _ = engine(model(case, BF), 8, dtype=BF)
    rows = {eng.add_sequence(prompts[0].tolist(), max_gen_len=C.GREEDY_NEW): 0}
    steps = 0
    while eng.active or eng.waiting_room:
        eng.step()
        steps += 1
        assert steps < 100
        if steps == 2:
            rows[eng.add_sequence(prompts[1].tolist(), max_gen_len=C.GREEDY_NEW)] = 1
        for sid, s in eng.active.items():
            if not s.is_prefill:
                s.tokens[s.num_tokens - 1] = int(greedy[rows[sid], s.num_tokens - 1 - C.PROMPT])
    for sid, r in rows.items():
        assert len(eng.logits[sid]) == C.GREEDY_NEW
        e = rel_err(C.sub_v(torch.stack(eng.logits[sid])), g[f"{case}.logits"][r])
        print(f"bf16 {case} sequence {r}: per-step logits against the reference's fp32 logits rel_err {e:.3e}")
        assert e < 3e-2, e
    again = eng.add_sequence(prompts[0].tolist() + greedy[0, :15].tolist(), max_gen_len=1)
    drain(eng)
    assert eng.prompt_tokens_computed[again] == C.PROMPT + 15 - 8
    e = rel_err(C.sub_v(eng.logits[again][0]), g[f"{case}.logits"][0, 15])
    print(f"bf16 {case} after a prefix hit: rel_err {e:.3e}")
    assert e < 3e-2, e
