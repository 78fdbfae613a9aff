"""fp8 e4m3 KV pages on the MI355X: the page write against the reference quantiser applied to what the bf16 op writes
(exact), the decode kernel against float64 on the dequantised pages, the prefill kernel against the bf16 kernel on
dequantised pages (exact), and the engine over an fp8 manager against an engine over bf16 pages whose freshly written
rows are replaced by their quantise-dequantise image."""
import math

import pytest
import torch

from tests.attn_range import GAINS, paged_decode_period, stair_levels
from tests.golden import cases_causal_lm as C
from tests.test_causal_lm_gpu import rel_err
from tests.test_paged_gpu import DH128, SEQLENS, drain, model
from tests.test_paged_prefill_gpu import EXTRA, SEGS, _prefill_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
FACTORS = torch.tensor([0.25, 1.0, 4.0])


def quantise(x):
    """The rule of include/vyom_hip.h on CPU: x (..., dh) fp32 -> (codes e4m3fn (..., dh), scales fp32 (...,))."""
    assert x.dtype == torch.float32 and not x.is_cuda
    amax = x.abs().amax(dim=-1)
    s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (x / s.unsqueeze(-1)).clamp(-448, 448).to(F8), s


def dequant_bf16(codes, s):
    return (codes.float() * s.unsqueeze(-1)).to(BF)


def head_factors(shape, g):
    """One of 0.25 / 1 / 4 per leading index, so neighbouring heads carry different scales."""
    return FACTORS[torch.randint(0, 3, shape, generator=g)]


def u8(t):
    return t.contiguous().view(torch.uint8)


def i16(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------
# 1. vy_paged_rope_write_fp8: exact
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("qknorm", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("h,hk,dh", [(4, 2, 64), (2, 1, 224), (8, 2, 128)])
def test_fp8_rope_write_equals_quantised_bf16_pages(h, hk, dh, qknorm):
    """The 37 tokens of test_rope_write_vs_fp64 (three sequences at positions 0 / 5 / 100, shuffled 16-token blocks, one
    negative slot), every input head scaled by 0.25 / 1 / 4, one k head all zeros.  The bf16 op on a copy gives the bf16
    pages; their quantised image is what the fp8 op must have written: codes and scales bit for bit, the in-place q / k
    rows those of the bf16 op, every other slot its sentinel (codes 0x5A, scales 7.5)."""
    from vyomai_amd import ops
    g = torch.Generator().manual_seed(dh + h)
    bs, nblk, table_rows, eps = 16, 12, 160, 1e-6
    order = torch.randperm(nblk, generator=g).tolist()
    pos, slots = [], []
    for first, n in [(0, 20), (5, 16), (100, 1)]:
        blocks = [order.pop() for _ in range((first + n + bs - 1) // bs)]
        for p in range(first, first + n):
            pos.append(p)
            slots.append(blocks[p // bs] * bs + p % bs)
    ntok, H3 = len(pos), h + 2 * hk
    assert ntok == 37
    dropped, zero_tok = 11, 23
    want_slots = list(slots)
    slots[dropped] = -1
    qkv = torch.randn(ntok, H3, dh, generator=g) * head_factors((ntok, H3), g)[..., None]
    qkv[zero_tok, h] = 0.0
    qkv = qkv.view(ntok, H3 * dh).to(BF)
    qs = (1.0 + 0.1 * (2 * torch.rand(dh, generator=g) - 1)).float().to(DEV)
    ks = (1.0 + 0.1 * (2 * torch.rand(dh, generator=g) - 1)).float().to(DEV)
    inv = 1.0 / (1e6 ** (torch.arange(0, dh, 2).float() / dh))
    ang = torch.outer(torch.arange(table_rows).float(), inv)
    cos, sin = ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV)
    posd, slotd = torch.tensor(pos, dtype=torch.int32, device=DEV), torch.tensor(slots, device=DEV)

    kb = torch.full((nblk, bs, hk, dh), 7.5, dtype=BF, device=DEV)
    vb = torch.full_like(kb, 7.5)
    kq = torch.full((nblk, bs, hk, dh), 0x5A, dtype=torch.uint8, device=DEV).view(F8)
    vq = torch.full((nblk, bs, hk, dh), 0x5A, dtype=torch.uint8, device=DEV).view(F8)
    ksc = torch.full((nblk, bs, hk), 7.5, device=DEV)
    vsc = torch.full_like(ksc, 7.5)
    ref, got = qkv.to(DEV), qkv.to(DEV)
    if qknorm:
        ops.paged_qknorm_rope_write_(ref, posd, slotd, cos, sin, qs, ks, eps, h, kb, vb)
        ops.paged_qknorm_rope_write_(got, posd, slotd, cos, sin, qs, ks, eps, h, kq, vq, k_page_scale=ksc, v_page_scale=vsc)
    else:
        ops.paged_rope_write_(ref, posd, slotd, cos, sin, h, kb, vb)
        ops.paged_rope_write_(got, posd, slotd, cos, sin, h, kq, vq, k_scale=ksc, v_scale=vsc)
    torch.cuda.synchronize()
    assert torch.equal(i16(got.cpu()), i16(ref.cpu())), "the in-place rows differ from the bf16 op's"
    live = torch.tensor([sl for sl in slots if sl >= 0])
    untouched = torch.ones(nblk * bs, dtype=torch.bool)
    untouched[live] = False
    assert untouched[want_slots[dropped]]
    zero_slot = slots[zero_tok]
    for what, pb, pq, sc in (("k", kb, kq, ksc), ("v", vb, vq, vsc)):
        pages = pb.cpu().view(nblk * bs, hk, dh)
        codes, scales = u8(pq.cpu()).view(nblk * bs, hk, dh), sc.cpu().view(nblk * bs, hk)
        want_codes, want_scales = quantise(pages[live].float())
        assert torch.equal(scales[live].view(torch.int32), want_scales.view(torch.int32)), f"{what} scales"
        diff = codes[live] != u8(want_codes)
        assert not diff.any(), f"{what} codes: {int(diff.sum())} of {diff.numel()} differ"
        assert len({float(x) for x in want_scales.flatten()}) > 8          # the scales do vary
        assert (codes[untouched] == 0x5A).all() and (scales[untouched] == 7.5).all(), f"{what}: a slot outside the mapping was written"
        if what == "k":
            assert (pages[zero_slot, 0] == 0).all() and scales[zero_slot, 0] == 1.0
            assert (codes[zero_slot, 0] & 0x7F == 0).all()


# ------------------------------------------------------------------------------------------
# 2. vy_attn_paged_decode_fp8: the bound of test_paged_decode_vs_fp64
# ------------------------------------------------------------------------------------------


def _fp8_decode_case(dh, h, hk, bs, regime, seed):
    """test_paged_gpu._decode_case with quantised pages: bf16 randn heads times 0.25 / 1 / 4 through the reference
    quantiser; code 0x7F (NaN) and a NaN scale in every row >= seqlen of a last page and in the spare page that the
    block-table entries past a sequence's pages point at.  The float64 result uses code * scale."""
    g = torch.Generator().manual_seed(seed)
    B = len(SEQLENS)
    pages = [(s + bs - 1) // bs for s in SEQLENS]
    nblk = sum(pages) + 1
    order = torch.randperm(nblk, generator=g).tolist()
    poison = order.pop()
    kc = torch.full((nblk, bs, hk, dh), 0x7F, dtype=torch.uint8)
    vc = torch.full((nblk, bs, hk, dh), 0x7F, dtype=torch.uint8)
    ksc = torch.full((nblk, bs, hk), float("nan"))
    vsc = torch.full((nblk, bs, hk), float("nan"))
    table = torch.full((B, max(pages) + 2), poison, dtype=torch.int32)
    ks, vs = [], []
    for b, S in enumerate(SEQLENS):
        blocks = [order.pop() for _ in range(pages[b])]
        table[b, :pages[b]] = torch.tensor(blocks, dtype=torch.int32)
        slot = torch.tensor([blocks[j // bs] * bs + j % bs for j in range(S)])
        for dst, dsc, keep in ((kc, ksc, ks), (vc, vsc, vs)):
            x = torch.randn(S, hk, dh, generator=g) * head_factors((S, hk), g)[..., None]
            if regime == "staircase" and dst is kc:   # tests/attn_range.py; the level dominates the row's amax
                x *= 0.5
                x[..., 0] = stair_levels(S, paged_decode_period(dh, BF, fp8=True))[:, None]
            x = x.to(BF).float()
            codes, s = quantise(x)
            dst.view(-1, hk, dh)[slot] = u8(codes)
            dsc.view(-1, hk)[slot] = s
            keep.append(codes.float().double() * s.double()[..., None])
    kvh = torch.arange(h) // (h // hk)
    qs = []
    for b, S in enumerate(SEQLENS):
        if regime == "flat":
            q = torch.randn(h, dh, generator=g)
        elif regime == "staircase":
            q = torch.randn(h, dh, generator=g)
            q[:, 0] = math.sqrt(dh) * GAINS[(S - 1) % len(GAINS)]
        else:      # peaked: q = 6 k[j*], j* in the sequence's last page
            jstar = torch.randint((S - 1) // bs * bs, S, (h,), generator=g)
            q = 6.0 * ks[b][jstar, kvh].float()
        qs.append(q.to(BF).float())
    q_rows = torch.tensor([7, 2, 11, 0, 5, 9, 1, 10, 4], dtype=torch.int32)
    qbuf = torch.randn(B + 3, (h + 2 * hk) * dh, generator=g)
    for b in range(B):
        qbuf[q_rows[b], :h * dh] = qs[b].reshape(-1)
    want = []
    for b in range(B):
        kd, vd = ks[b][:, kvh], vs[b][:, kvh]                              # (S, h, dh)
        p = torch.softmax(torch.einsum("hd,shd->hs", qs[b].double(), kd) / math.sqrt(dh), dim=-1)
        want.append(torch.einsum("hs,shd->hd", p, vd).reshape(-1))
    vmax = max(float(v.abs().max()) for v in vs)
    return (qbuf.to(BF), q_rows, kc.view(F8), vc.view(F8), ksc, vsc, table, torch.tensor(SEQLENS, dtype=torch.int32),
            torch.stack(want), vmax)


@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("h,hk", [(4, 2), (8, 1)])
@pytest.mark.parametrize("dh", [64, 128, 224])
def test_fp8_paged_decode_vs_fp64(dh, h, hk, bs):
    """|got - want| <= 2^-8 |want| + 1e-4 max|v|, the bf16 bound of test_paged_decode_vs_fp64 unchanged: the kernel does
    the same fp32 arithmetic on inputs that are exact in fp32 (the codes) and adds at most two fp32 roundings per element
    for the scales, far inside the S * 2^-24 accumulation term the bound carries.  Finite outputs (no row >= seqlen, no
    spare page, codes or scales, took part); rows outside q_rows keep their 3.25."""
    from vyomai_amd import ops
    for regime in ("flat", "peaked", "staircase"):
        q, q_rows, kc, vc, ksc, vsc, table, seqlens, want, vmax = _fp8_decode_case(dh, h, hk, bs, regime, seed=dh + 7 * hk + bs)
        qd, rd, kd, vd, ksd, vsd, td, sd = (t.to(DEV) for t in (q, q_rows, kc, vc, ksc, vsc, table, seqlens))
        for n_split in (1, 2, 5, 0):
            out = torch.full((q.shape[0], h * dh), 3.25, dtype=BF, device=DEV)
            ops.attention_paged_decode(qd, kd, vd, td, sd, max(SEQLENS), h, q_rows=rd, out=out, n_split=n_split,
                                       k_scale=ksd, v_scale=vsd)
            torch.cuda.synchronize()
            out = out.cpu()
            got = out[q_rows.long()].double()
            what = f"{regime} n_split={n_split}"
            assert torch.isfinite(got).all(), f"{what}: non-finite output (a row >= seqlen or the spare page took part)"
            err = (got - want).abs()
            bound = 2.0 ** -8 * want.abs() + 1e-4 * vmax
            worst = float((err / bound).max())
            print(f"{what}: max err / bound {worst:.3f}")
            assert (err <= bound).all(), f"{what}: max err / bound {worst:.2f} (sequence {int((err / bound).max(dim=1).values.argmax())})"
            other = torch.ones(q.shape[0], dtype=torch.bool)
            other[q_rows.long()] = False
            assert (out[other] == 3.25).all(), f"{what}: rows outside q_rows were written"


def test_fp8_paged_decode_seqlen_zero_writes_zeros():
    from vyomai_amd import ops
    h, hk, dh, bs = 4, 2, 64, 16
    kc = torch.full((3, bs, hk, dh), 0x7F, dtype=torch.uint8, device=DEV).view(F8)
    sc = torch.full((3, bs, hk), float("nan"), device=DEV)
    q = torch.randn(2, h * dh).to(BF).to(DEV)
    table = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    for n_split in (1, 2):
        out = torch.full((2, h * dh), 3.25, dtype=BF, device=DEV)
        ops.attention_paged_decode(q, kc, kc.clone(), table, torch.zeros(2, dtype=torch.int32, device=DEV), 32, h, out=out,
                                   n_split=n_split, k_scale=sc, v_scale=sc.clone())
        assert (out == 0).all()


# ------------------------------------------------------------------------------------------
# 3. vy_attn_paged_prefill_fp8: exact against the bf16 kernel on dequantised pages
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("dh", [64, 72, 128, 224])
def test_fp8_paged_prefill_equals_bf16_kernel_on_dequantised_pages(dh, bs):
    """The eleven segments of test_paged_prefill_gpu._prefill_case (both sides of the 64-row and 64-key tiles, segments
    behind a context of 5 .. 600 keys), its pages times 0.25 / 1 / 4 per (slot, head) through the reference quantiser;
    the rows at or past ctx + len and the spare page become code 0x7F with a NaN scale.  The fp8 kernel dequantises a
    fetched row as bf16(code * s) and is the bf16 kernel from there on: equal bit for bit to vy_attn_paged_prefill on
    pages holding (code.float() * s).to(bfloat16); rows outside the segments keep their 3.25."""
    from vyomai_amd import ops
    h, hk = 4, 2
    g = torch.Generator().manual_seed(dh + bs)
    for regime in ("flat", "peaked", "staircase"):
        q, kc, vc, table, cu, ctx, _, _ = _prefill_case(dh, h, hk, bs, BF, regime)
        rows = q.shape[0] - EXTRA
        args = (table.to(DEV), cu.to(DEV), ctx.to(DEV), max(l for _, l in SEGS), max(c + l for c, l in SEGS), h)
        outs, held = [], []
        for pages in (kc, vc):
            x = pages.float() * head_factors(pages.shape[:3], g)[..., None]
            codes, s = quantise(x)
            dead = torch.isnan(x).any(dim=-1)
            assert (u8(codes)[dead] & 0x7F == 0x7F).all() and dead.any()
            s = torch.where(dead, torch.full_like(s, float("nan")), s)
            held.append((codes, s, dequant_bf16(codes, s)))
        (kq, ks, kb), (vq, vs, vb) = held
        qd = q.to(DEV)
        for fp8 in (True, False):
            out = torch.full((q.shape[0], h * dh), 3.25, dtype=BF, device=DEV)
            if fp8:
                ops.attention_paged_prefill(qd, kq.to(DEV), vq.to(DEV), *args, out=out, k_scale=ks.to(DEV), v_scale=vs.to(DEV))
            else:
                ops.attention_paged_prefill(qd, kb.to(DEV), vb.to(DEV), *args, out=out)
            torch.cuda.synchronize()
            outs.append(out.cpu())
        new, old = outs
        assert torch.isfinite(new[:rows].float()).all(), f"{regime}: non-finite output"
        assert (new[rows:] == 3.25).all(), f"{regime}: rows outside the segments were written"
        diff = float((new[:rows].float() - old[:rows].float()).abs().max())
        print(f"{regime}: max |fp8 - bf16 on dequantised pages| {diff:.3e}")
        assert torch.equal(i16(new), i16(old)), f"{regime}: max |fp8 - bf16 on dequantised pages| {diff:.3e}"


# ------------------------------------------------------------------------------------------
# 4. the engine
# ------------------------------------------------------------------------------------------

SCHEDULES = {"varlen": dict(varlen_prefill=True), "chunked": dict(varlen_prefill=True, max_step_tokens=3, max_batch_size=2)}


def _engine_model(case):
    """-> (model, fixture name, key of its prompts): the bf16 causal LMs of test_engine_bf16_logits_vs_dense_forward, or
    the bf16 Qwen3Model of case r (qk-norm, one KV group)."""
    if case == "qwen3":
        from tests.test_qwen3_gpu import model as qwen3_model
        return qwen3_model("r", BF), "qwen3", "r.prompt"
    return model(DH128 if case == "dh128" else case, compute=BF), "causal_lm", "a.prompt" if case == "dh128" else f"{case}.prompt"


def _engine(m, fp8, **kw):
    import vyomai_amd as V
    mgr = V.PagedKVManager(m.config, 16, 16, DEV, BF, kv_cache_dtype="fp8" if fp8 else None)
    return V.ContinuousBatchEngine(m, mgr, eos_token_ids=[], record_logits=True, **kw), mgr


def _requantise_written_rows(monkeypatch):
    """From here on, the two rope-write ops called on bf16 pages replace the rows they have just written by the
    quantise-dequantise image of those rows (the rule, on the host); calls on fp8 pages pass through."""
    from vyomai_amd import ops

    def wrap(fn, slots_at, pages_at):
        def wrapped(*args, **kw):
            out = fn(*args, **kw)
            kc, vc = args[pages_at], args[pages_at + 1]
            if kc.dtype == BF:
                slots = args[slots_at]
                live = slots[slots >= 0]
                for pages in (kc, vc):
                    flat = pages.view(-1, pages.shape[2], pages.shape[3])
                    codes, s = quantise(flat[live].float().cpu())
                    flat[live] = dequant_bf16(codes, s).to(pages.device)
            return out
        return wrapped

    monkeypatch.setattr(ops, "paged_rope_write_", wrap(ops.paged_rope_write_, 2, 6))
    monkeypatch.setattr(ops, "paged_qknorm_rope_write_", wrap(ops.paged_qknorm_rope_write_, 2, 9))


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("case", ["a", "b", "dh128", "qwen3"])
def test_fp8_engine_against_requantised_bf16_pages(golden, monkeypatch, case, schedule):
    """Two requests through an engine over fp8 pages (block size 16, the second arrives after two steps), and the same
    through the reference: an engine over bf16 pages whose written rows are requantised.
    (a) the first logits of the first request, prefilled alone, are equal bit for bit: the codes are equal (test 1) and
        the prefill attention is (test 3);
    (b) every logits row of the fp8 run, i.e. every decode step's too, against the reference engine's first logits on a
        fresh manager for the prompt seq[:PREFILL + i]: rel_err below 3e-2, the bf16 logits bar of
        test_model_bf16_vs_reference -- both sides hold the same quantised cache;
    (c) the run finishes, every block is free or evictable again."""
    m, fixture, key = _engine_model(case)
    prompts = golden(fixture)[key]
    kw = SCHEDULES[schedule]
    eng, mgr = _engine(m, True, **kw)
    sids = [eng.add_sequence(prompts[0].tolist(), max_gen_len=C.GREEDY_NEW)]
    done = {}
    for _ in range(2):
        done.update(eng.step())
    sids.append(eng.add_sequence(prompts[1].tolist(), max_gen_len=C.GREEDY_NEW))
    done.update(drain(eng))
    assert sorted(list(mgr.free_blocks) + list(mgr.evictable_blocks)) == list(range(mgr.max_blocks))
    for sid in sids:
        assert len(done[sid]) == C.PREFILL + C.GREEDY_NEW and len(eng.logits[sid]) == C.GREEDY_NEW

    _requantise_written_rows(monkeypatch)
    ref, _ = _engine(m, False, **kw)
    first = ref.add_sequence(prompts[0].tolist(), max_gen_len=C.GREEDY_NEW)
    for _ in range(2):
        ref.step()
    ref.add_sequence(prompts[1].tolist(), max_gen_len=C.GREEDY_NEW)
    while first not in ref.logits:
        ref.step()
    a, b = eng.logits[sids[0]][0], ref.logits[first][0]
    print(f"{case} {schedule}: first prefill logits, max |fp8 - reference| {float((a - b).abs().max()):.3e}")
    assert torch.equal(a, b), "the prefill step differs: the page write or the prefill attention is incomplete"

    worst = 0.0
    for sid in sids:
        seq = done[sid]
        for i in range(C.GREEDY_NEW):
            replay, _ = _engine(m, False, varlen_prefill=True)
            rid = replay.add_sequence(seq[:C.PREFILL + i], max_gen_len=1)
            drain(replay)
            worst = max(worst, rel_err(eng.logits[sid][i], replay.logits[rid][0].numpy()))
    print(f"{case} {schedule}: fp8 engine logits against the requantised-bf16 replay, largest rel_err {worst:.3e}")
    assert worst < 3e-2, worst


def test_fp8_engine_prefix_hit(golden):
    """The 20-token request of test_engine_prefix_hit twice through one fp8 manager (block size 8): the second takes
    the first one's two blocks -- codes and scales -- computes 4 prompt tokens and runs to its end; then every block is
    free or evictable again."""
    g = golden("causal_lm")
    m = model("a", compute=BF)
    ids = g["a.prompt"][0].tolist() + g["a.greedy"][0, :12].tolist()
    import vyomai_amd as V
    mgr = V.PagedKVManager(m.config, 16, 8, DEV, BF, kv_cache_dtype="fp8")
    eng = V.ContinuousBatchEngine(m, mgr, eos_token_ids=[], varlen_prefill=True)
    first = eng.add_sequence(ids, max_gen_len=4)
    done = eng.step()
    first_blocks = eng.active[first].block_table[:2].tolist()
    done.update(drain(eng))
    assert eng.prompt_tokens_computed[first] == 20 and len(done[first]) == 24
    warm = eng.add_sequence(ids, max_gen_len=4)
    done = eng.step()
    assert eng.active[warm].block_table[:2].tolist() == first_blocks and eng.active[warm].prefix_len == 16
    assert eng.prompt_tokens_computed[warm] == 4
    done.update(drain(eng))
    assert len(done[warm]) == 24
    assert sorted(list(mgr.free_blocks) + list(mgr.evictable_blocks)) == list(range(mgr.max_blocks))
