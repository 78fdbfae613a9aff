"""vy_attn_paged_prefill on the MI355X: the one varlen launch against float64 on the same pages and against the old
path (vy_paged_gather + vy_attn_fwd), and the engine with varlen_prefill / max_step_tokens against the reference
model's greedy ids (fp32) and the model's dense forward (bf16)."""
import functools
import math

import pytest
import torch

from tests.attn_range import paged_decode_period, row_gains, stair_levels
from tests.golden import cases_causal_lm as C
from tests.test_causal_lm_gpu import rel_err
from tests.test_paged_gpu import DH128, drain, engine, model

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])

# (ctx, len): both sides of the 64-row query tile, of the 64-key tile and of both block sizes; 630 rows, <= 640 keys
SEGS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 130), (5, 1), (16, 3), (61, 70), (256, 64), (250, 129), (600, 40)]
EXTRA = 3


@functools.lru_cache(maxsize=3)
def _prefill_case(dh, h, hk, bs, dtype, regime):
    """One batch of the eleven segments, in the manner of test_paged_gpu._decode_case: pages in shuffled physical order,
    NaN in the key rows >= ctx + len of every last page and in a spare page that every block-table entry past a
    sequence's pages points at; q rows inside a buffer shaped like the packed QKV rows, with 3 extra rows at the end.
    -> inputs (host) and the float64 result of every row."""
    g = torch.Generator().manual_seed(dh + 7 * hk + bs + {"flat": 0, "peaked": 1, "staircase": 2}[regime])
    # keys per online-softmax step: the 64-key tile of the bf16 kernel, a trip of paged_dec_kernel on the fp32 path
    period = 64 if dtype == BF else paged_decode_period(dh, dtype)
    n = len(SEGS)
    pages = [(c + l + bs - 1) // bs for c, l in SEGS]
    nblk = sum(pages) + 1
    order = torch.randperm(nblk, generator=g).tolist()
    poison = order.pop()
    kc = torch.full((nblk, bs, hk, dh), float("nan"))
    vc = torch.full((nblk, bs, hk, dh), float("nan"))
    table = torch.full((n, max(pages) + 2), poison, dtype=torch.int32)
    kvh = torch.arange(h) // (h // hk)
    rows = sum(l for _, l in SEGS)
    qbuf = torch.randn(rows + EXTRA, (h + 2 * hk) * dh, generator=g)
    want = torch.zeros(rows, h * dh, dtype=torch.float64)
    cu, vmax = [0], 0.0
    for s, (ctx, ln) in enumerate(SEGS):
        S = ctx + ln
        blocks = [order.pop() for _ in range(pages[s])]
        table[s, :pages[s]] = torch.tensor(blocks, dtype=torch.int32)
        k = torch.randn(S, hk, dh, generator=g)
        if regime == "staircase":   # tests/attn_range.py: one score level per step, gain by the row's position
            k *= 0.5
            k[..., 0] = stair_levels(S, period)[:, None]
        k = k.to(dtype).float()
        v = torch.randn(S, hk, dh, generator=g).to(dtype).float()
        slot = torch.tensor([blocks[j // bs] * bs + j % bs for j in range(S)])
        kc.view(-1, hk, dh)[slot] = k
        vc.view(-1, hk, dh)[slot] = v
        vmax = max(vmax, float(v.abs().max()))
        if regime == "flat":
            q = torch.randn(ln, h, dh, generator=g)
        elif regime == "staircase":
            q = torch.randn(ln, h, dh, generator=g)
            q[..., 0] = math.sqrt(dh) * row_gains(ln, start_pos=ctx)[:, None]
        else:      # peaked: q = 6 k[j*], j* among the row's visible keys [0, ctx + i]
            hi = (ctx + torch.arange(ln) + 1).view(ln, 1).double()
            jstar = (torch.rand(ln, h, generator=g, dtype=torch.float64) * hi).long().clamp_max(hi.long() - 1)
            q = 6.0 * k[jstar, kvh.view(1, h)]
        q = q.to(dtype).float()
        qbuf[cu[-1]:cu[-1] + ln, :h * dh] = q.reshape(ln, -1)
        kd, vd = k.double()[:, kvh], v.double()[:, kvh]                   # (S, h, dh)
        sc = torch.einsum("ihd,shd->ihs", q.double(), kd) / math.sqrt(dh)
        vis = torch.arange(S).view(1, 1, S) <= (ctx + torch.arange(ln)).view(ln, 1, 1)
        p = torch.softmax(sc.masked_fill(~vis, float("-inf")), dim=-1)
        want[cu[-1]:cu[-1] + ln] = torch.einsum("ihs,shd->ihd", p, vd).reshape(ln, -1)
        cu.append(cu[-1] + ln)
    assert cu[-1] == 630 and max(c + l for c, l in SEGS) == 640
    return (qbuf.to(dtype), kc.to(dtype), vc.to(dtype), table, torch.tensor(cu, dtype=torch.int32),
            torch.tensor([c for c, _ in SEGS], dtype=torch.int32), want, vmax)


@DTYPES
@pytest.mark.parametrize("bs", [8, 256])
@pytest.mark.parametrize("h,hk", [(4, 4), (4, 2), (8, 1)])
@pytest.mark.parametrize("dh", [64, 72, 128, 224])
def test_paged_prefill_vs_fp64(dh, h, hk, bs, dtype):
    """|got - want| <= r |want| + a max|v|, derived:
    fp32: r = 2^-20, a = 1e-4 -- the derivation of test_paged_decode_vs_fp64 (scores, softmax and the weighted sum in
    fp32, S * 2^-24 of accumulation with S <= 640, the error of __expf, one rounding of the result).
    bf16: r = 2^-8, a = 2^-8 -- P is rounded to bf16 before the PV MFMA, at most 2^-9 relative per weight; the weights
    sum to 1, so that is at most 2^-9 max|v|; the output rounding adds 2^-9 |want|; the fp32 accumulation and exp2 errors
    are orders below both.
    The output is finite (no key row >= ctx + len and no poison page took part) and the extra rows keep their 3.25."""
    from vyomai_amd import ops
    rel, ab = (2.0 ** -8, 2.0 ** -8) if dtype == BF else (2.0 ** -20, 1e-4)
    for regime in ("flat", "peaked", "staircase"):
        q, kc, vc, table, cu, ctx, want, vmax = _prefill_case(dh, h, hk, bs, dtype, regime)
        rows = want.shape[0]
        out = torch.full((q.shape[0], h * dh), 3.25, dtype=dtype, device=DEV)
        ops.attention_paged_prefill(q.to(DEV), kc.to(DEV), vc.to(DEV), table.to(DEV), cu.to(DEV), ctx.to(DEV),
                                    max(l for _, l in SEGS), max(c + l for c, l in SEGS), h, out=out)
        torch.cuda.synchronize()
        out = out.cpu()
        got = out[:rows].double()
        assert torch.isfinite(got).all(), f"{regime}: non-finite output (a key row >= ctx + len or the poison page took part)"
        assert (out[rows:] == 3.25).all(), f"{regime}: rows outside the segments were written"
        err = (got - want).abs()
        bound = rel * want.abs() + ab * vmax
        ratio = (err / bound).max(dim=1).values
        print(f"{regime}: max err / bound {float(ratio.max()):.3f}")
        assert (err <= bound).all(), f"{regime}: max err / bound {float(ratio.max()):.2f} (row {int(ratio.argmax())})"


@pytest.mark.parametrize("dh", [64, 72, 224])
def test_paged_prefill_agrees_with_gather_and_contiguous_attention(dh):
    """Same pages, old path: vy_paged_gather + causal vy_attn_fwd(start_pos = ctx) per sequence.  At dh = 72 and 224
    both sides run the 16x16x32 tile core (vy_attn_gen.h) over the same 64-key tile walk from key 0 at the same padded
    width (96 and 256), so the rows are equal bit for bit.  At dh = 64 the contiguous side is attn_fwd_mfma_kernel:
    within the project's bf16 attention bar (atol = rtol = 2e-2, test_attention_fwd)."""
    from vyomai_amd import ops
    h, hk, bs = 4, 2, 256
    q, kc, vc, table, cu, ctx, _, _ = _prefill_case(dh, h, hk, bs, BF, "flat")
    qd, kd, vd, td = q.to(DEV), kc.to(DEV), vc.to(DEV), table.to(DEV)
    new = ops.attention_paged_prefill(qd, kd, vd, td, cu.to(DEV), ctx.to(DEV), max(l for _, l in SEGS),
                                      max(c + l for c, l in SEGS), h)
    for s in (SEGS.index((16, 3)), SEGS.index((256, 64)), SEGS.index((250, 129))):
        c, ln = SEGS[s]
        r0 = int(cu[s])
        k3, v3 = ops.paged_gather(kd, vd, td[s].contiguous(), c + ln)
        q4 = qd[r0:r0 + ln, :h * dh].view(ln, h, dh).permute(1, 0, 2).unsqueeze(0)
        old = torch.empty((1, ln, h * dh), dtype=BF, device=DEV)
        ops.attention(q4, k3.unsqueeze(0), v3.unsqueeze(0), causal=True, start_pos=c, out=old)
        if dh == 64:
            torch.testing.assert_close(new[r0:r0 + ln].float(), old[0].float(), atol=2e-2, rtol=2e-2)
        else:
            diff = (new[r0:r0 + ln].float() - old[0].float()).abs().max()
            print(f"dh {dh}, segment {SEGS[s]}: max |new - old| {float(diff):.3e}")
            assert torch.equal(new[r0:r0 + ln], old[0]), f"segment {SEGS[s]}: max |new - old| {float(diff):.3e}"


def test_paged_prefill_no_sequences_is_a_no_op():
    from vyomai_amd import ops
    kc = torch.zeros((2, 16, 1, 64), dtype=BF, device=DEV)
    out = torch.full((4, 128), 3.25, dtype=BF, device=DEV)
    ops.attention_paged_prefill(torch.zeros((4, 256), dtype=BF, device=DEV), kc, kc, torch.zeros((0, 2), dtype=torch.int32, device=DEV),
                                torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                0, 0, 2, out=out)
    assert (out == 3.25).all()


# ------------------------------------------------------------------------------------------
# the engine against the reference's greedy ids (fp32)
# ------------------------------------------------------------------------------------------

FP32_CASES = pytest.mark.parametrize("case,block_size", [("a", 8), ("a", 16), ("b", 8), ("b", 16)])


def _golden_ids(g, case, r):
    return g[f"{case}.prompt"][r].tolist() + g[f"{case}.greedy"][r].tolist()


@FP32_CASES
def test_engine_varlen_all_at_once(golden, case, block_size):
    """varlen_prefill=True alone: both prompts in one step, ONE attention launch per layer for both."""
    g = golden("causal_lm")
    eng, _ = engine(model(case), block_size, eos_token_ids=[], varlen_prefill=True)
    sids = [eng.add_sequence(g[f"{case}.prompt"][r].tolist(), max_gen_len=C.GREEDY_NEW) for r in range(C.B)]
    done = drain(eng)
    for r, sid in enumerate(sids):
        assert done[sid] == _golden_ids(g, case, r), r


@FP32_CASES
def test_engine_chunked_all_at_once(golden, case, block_size):
    """max_step_tokens=3: the first 8-token prompt goes as 3 + 3 + 2 and the second follows in the budget that is left."""
    g = golden("causal_lm")
    assert C.PREFILL == 8
    eng, _ = engine(model(case), block_size, eos_token_ids=[], max_step_tokens=3, max_batch_size=2)
    sids = [eng.add_sequence(g[f"{case}.prompt"][r].tolist(), max_gen_len=C.GREEDY_NEW) for r in range(C.B)]
    seen = []
    for _ in range(3):
        assert eng.step() == {}
        seen.append(eng.prompt_tokens_computed[sids[0]])
    assert seen == [3, 6, 8] and not eng.active[sids[0]].is_prefill
    done = drain(eng)
    for r, sid in enumerate(sids):
        assert done[sid] == _golden_ids(g, case, r), r
        assert eng.prompt_tokens_computed[sid] == C.PREFILL


@FP32_CASES
def test_engine_chunked_staggered(golden, case, block_size):
    """The second prompt arrives after three steps: its chunks share their steps with the first sequence's decode."""
    g = golden("causal_lm")
    eng, _ = engine(model(case), block_size, eos_token_ids=[], max_step_tokens=3, max_batch_size=2)
    sid0 = eng.add_sequence(g[f"{case}.prompt"][0].tolist(), max_gen_len=C.GREEDY_NEW)
    done = {}
    for _ in range(3):
        done.update(eng.step())
    sid1 = eng.add_sequence(g[f"{case}.prompt"][1].tolist(), max_gen_len=C.GREEDY_NEW)
    done.update(eng.step())
    assert eng.active[sid1].is_prefill and eng.prompt_tokens_computed[sid1] == 2 and not eng.active[sid0].is_prefill
    done.update(drain(eng))
    for r, sid in enumerate((sid0, sid1)):
        assert done[sid] == _golden_ids(g, case, r), r


@pytest.mark.parametrize("case", ["a", "b"])
def test_engine_chunked_prefix_hit(golden, case):
    """The 20-token request of test_engine_prefix_hit under max_step_tokens=3 (block_size 8): the warm request takes the
    first one's two blocks, computes its 4 tokens in two chunks (3 + 1), produces the same ids, and its first logits are
    within the fp32 logits bar (rel_err 2e-5) of a cold UNCHUNKED run of the default engine on a fresh manager."""
    g = golden("causal_lm")
    ids = g[f"{case}.prompt"][0].tolist() + g[f"{case}.greedy"][0, :12].tolist()
    want = ids + g[f"{case}.greedy"][0, 12:16].tolist()
    eng, mgr = engine(model(case), 8, eos_token_ids=[], record_logits=True, max_step_tokens=3, max_batch_size=2)
    first = eng.add_sequence(ids, max_gen_len=4)
    done = {}
    while eng.active.get(first) is None or eng.active[first].block_count < 2:       # (the second block: fourth chunk)
        done.update(eng.step())
    first_blocks = eng.active[first].block_table[:2].tolist()
    done.update(drain(eng))
    assert done[first] == want and eng.prompt_tokens_computed[first] == 20
    warm = eng.add_sequence(ids, max_gen_len=4)
    assert eng.step() == {}
    st = eng.active[warm]
    assert st.block_table[:2].tolist() == first_blocks and st.prefix_len == 16
    assert st.is_prefill and eng.prompt_tokens_computed[warm] == 3 and warm not in eng.logits
    assert eng.step() == {}
    assert not st.is_prefill and eng.prompt_tokens_computed[warm] == 4 and len(eng.logits[warm]) == 1
    done = drain(eng)
    assert done[warm] == want
    fresh, _ = engine(model(case), 8, eos_token_ids=[], record_logits=True)
    cold = fresh.add_sequence(ids, max_gen_len=4)
    assert drain(fresh)[cold] == want and fresh.prompt_tokens_computed[cold] == 20
    e = rel_err(eng.logits[warm][0], fresh.logits[cold][0].numpy())
    print(f"first logits after a chunked prefix hit against the cold unchunked run: rel_err {e:.3e}")
    assert e < 2e-5, e


# ------------------------------------------------------------------------------------------
# bf16: the chunked engine's logits against the model's dense forward
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["a", "b", "dh128"])
def test_engine_chunked_bf16_logits_vs_dense_forward(golden, case):
    """The method and bar of test_engine_bf16_logits_vs_dense_forward (rel_err 3e-2 of the dense logits at the same
    positions) with max_step_tokens=3; the second request arrives after two steps, while the first is still in chunks."""
    g = golden("causal_lm")
    m = model(DH128 if case == "dh128" else case, compute=BF)
    prompts = g["a.prompt" if case == "dh128" else f"{case}.prompt"]
    eng, _ = engine(m, 16, dtype=BF, eos_token_ids=[], record_logits=True, max_step_tokens=3, max_batch_size=2)
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
        print(f"bf16 {case} sequence {sid}: chunked engine logits against the dense forward rel_err {e:.3e}")
        assert e < 3e-2, e
