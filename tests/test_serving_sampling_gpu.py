"""Per-request sampling of the serving engine on the MI355X: vy_sample_rows against a restatement built from the two
pinned pieces it combines (the support of vy_sampling_probs, the noise of vy_gumbel_noise), the distribution of its
draws against the softmax over the kept set, and ContinuousBatchEngine with SamplingParams around a tiny
ModelForCausalLM and a tiny Qwen3Model.

Bars.  A sampled token lies in the kept set (ops.sampling_probs(row, 1.0, k, p) > 0) and its fp64 score
logit * inv_t + noise is within 2^-22 max(1, max|s|) of the kept maximum: the bar test_electra_gpu.py holds the Gumbel
sampler to, two fp32 roundings of a fused multiply-add, one on each of the two scores compared (the noise itself is the
kernel's own fp32 value in both).  A greedy token is the lowest index holding the row maximum.  Distribution: Pearson's
chi-square of 16384 draws against the softmax over the kept set, bins with expectation below 5 merged into one, at most
the 0.999 quantile (Wilson-Hilferty); a numpy restatement of the sampler (the Philox restatement of test_electra_gpu.py,
noise row 0, offset = counter) gave 40.35 / 39.28 / 11.35 / 199.84 for the four cases and is held to the bound first."""
import math

import numpy as np
import pytest
import torch

from tests.golden import cases_causal_lm as CL
from tests.golden import cases_qwen3 as CQ
from tests.test_electra_gpu import gumbel64, philox7

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SEED = 0x1234567887654321
MASK64 = (1 << 64) - 1


def i64(x):
    """A 64-bit pattern as the int64 that carries it."""
    return x - (1 << 64) if x >> 63 else x


def inv_t_of(temperature):
    return 0.0 if temperature == 0 else float(np.float32(1.0 / temperature))


def launch(logits, params):
    """params: per row (temperature, top_k, top_p, seed, counter) -> tokens (R,) on the host."""
    from vyomai_amd import ops
    dev = logits.device
    out = ops.sample_rows(logits,
                          torch.tensor([inv_t_of(p[0]) for p in params], dtype=torch.float32, device=dev),
                          torch.tensor([p[1] for p in params], dtype=torch.int32, device=dev),
                          torch.tensor([p[2] for p in params], dtype=torch.float32, device=dev),
                          torch.tensor([i64(p[3]) for p in params], dtype=torch.long, device=dev),
                          torch.tensor([p[4] for p in params], dtype=torch.long, device=dev))
    assert out.dtype == torch.long and out.shape == (len(params),)
    return out.cpu()


def judge(row, param, token, what):
    """The restated rule on one logits row (V,) on the device; raises when it does not accept `token`.
    -> (is the fp64 argmax, shortfall / margin)."""
    from vyomai_amd import ops
    temperature, k, p, seed, counter = param
    V = row.numel()
    assert 0 <= token < V, (what, token)
    x = row.double().cpu()
    if temperature == 0:
        assert token == int((x == x.max()).nonzero()[0]), (what, "greedy: not the lowest index of the maximum", token)
        return True, 0.0
    kept = (ops.sampling_probs(row[None], 1.0, max(k, 0), max(p, 0.0))[0] > 0).cpu()
    assert bool(kept[token]), (what, "token outside the kept set", token, int(kept.sum()))
    s = x * inv_t_of(temperature) + ops.gumbel_noise(1, V, seed, counter, row.device)[0].double().cpu()
    sk = s[kept]
    margin = 2.0 ** -22 * max(1.0, float(sk.abs().max()))
    short = float(sk.max() - s[token])
    assert short <= margin, (what, "score below the kept maximum", short, margin)
    return short == 0.0, short / margin


# ------------------------------------------------------------------------------------------
# 1. the kernel against the restatement
# ------------------------------------------------------------------------------------------

R = 24
TIE_ROW, PEAK_ROW, KTIE_ROW = 5, 9, 7


def row_params(V):
    """(temperature, top_k, top_p) of the 24 rows of one launch."""
    return [(0, 0, 0.0), (0.7, 0, 0.0), (1.0, 0, 0.0), (3.0, 0, 0.0), (1.0, 1, 0.0), (0, 0, 0.0),
            (0.7, 12, 0.0), (1.0, 12, 0.0), (1.0, V, 0.0), (1.0, 0, 0.0), (3.0, V + 5, 0.0), (1.0, 0, 0.5),
            (0.7, 0, 0.9), (1.0, 0, 1.0), (1.5, 12, 0.9), (0.8, 12, 0.5), (0, 0, 0.0), (2.0, 1, 0.0),
            (1.0, 0, 0.0), (0.7, V, 1.0), (1.0, -3, -0.5), (3.0, 0, 0.9), (0.7, 12, 1.0), (0, 12, 0.5)]


def kernel_case(V, dtype):
    """-> (buf (R, ld) on the device, params).  Pad columns hold +60 (even rows) or NaN (odd rows); row 9 has a logit
    raised by 40, row 5 (greedy) an exact tie for the maximum at two indices, row 7 (top_k = 12) three values tied at
    the 12th largest.  Seeds use both 32-bit halves; counters include 0 (a greedy and a sampled row) and 2^32 + 5."""
    from vyomai_amd.autograd_train import _row_stride
    g = torch.Generator().manual_seed(1000 + V)
    x = 2.0 * torch.randn(R, V, generator=g)
    x[PEAK_ROW, V // 3] += 40.0
    for r in (4, 17):                                   # the top_k = 1 rows have one maximum, also after rounding to bf16
        x[r, x[r].argmax()] += 1.0
    x = x.to(dtype)
    x[TIE_ROW, V // 5] = x[TIE_ROW, V - 7] = 25.0
    order = x[KTIE_ROW].float().argsort(descending=True)
    x[KTIE_ROW, order[-1]] = x[KTIE_ROW, order[-2]] = x[KTIE_ROW, order[11]]
    buf = torch.zeros((R, _row_stride(V)), dtype=dtype)
    buf[:, :V] = x
    buf[0::2, V:] = 60.0
    buf[1::2, V:] = float("nan")
    params = []
    for r, (t, k, p) in enumerate(row_params(V)):
        counter = {0: 0, 1: 0, 2: (1 << 32) + 5}.get(r, r * 1000003)
        params.append((t, k, p, (SEED + r * 0x9E3779B97F4A7C15) & MASK64, counter))
    for r in (4, 17):
        assert int((x[r] == x[r].max()).sum()) == 1
    return buf.to(DEV), params


@pytest.mark.parametrize("V,dtype", [(37, torch.float32), (37, BF), (1003, torch.float32), (1003, BF),
                                     (4100, torch.float32), (4100, BF), (151936, torch.float32)],
                         ids=lambda v: {torch.float32: "fp32", BF: "bf16"}.get(v, str(v)))
def test_sample_rows_vs_restatement(V, dtype):
    from vyomai_amd import ops
    buf, params = kernel_case(V, dtype)
    logits = buf[:, :V]
    before = buf.clone()
    got = launch(logits, params)
    assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), "the logits are only read"
    exact, worst = 0, 0.0
    for r in range(R):
        hit, frac = judge(logits[r], params[r], int(got[r]), f"V={V} row {r} {params[r][:3]}")
        exact, worst = exact + hit, max(worst, frac)
    print(f"V={V} {dtype}: {exact}/{R} tokens are the fp64 argmax, largest shortfall {worst:.3f} of the margin")
    top = logits.float().cpu().argmax(-1)
    assert int(got[PEAK_ROW]) == V // 3, "the raised logit wins"
    assert int(got[TIE_ROW]) == V // 5, "the lowest index of a tied maximum"
    for r in (4, 17):
        assert int(got[r]) == int(top[r]), "top_k = 1 is the greedy answer"
    kept = ops.sampling_probs(logits[KTIE_ROW][None], 1.0, 12, 0.0)[0] > 0
    xk = logits[KTIE_ROW].float()
    tied = int((xk >= xk.sort(descending=True).values[11]).sum())
    assert int(kept.sum()) == tied >= 14, "the values tied at the 12th largest are all kept"
    # a greedy row does not read its other parameters: garbage there changes nothing
    assert int(got[23]) == int((logits[23].double() == logits[23].double().max()).nonzero()[0])
    assert torch.equal(got, launch(logits, params)), "two launches differ"
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(V)).tolist()
    moved = launch(buf[perm][:, :V], [params[i] for i in perm])
    assert torch.equal(moved, got[perm]), "a row's token depends on where the row sits in the launch"


def test_sample_rows_unaligned_rows_and_one_column():
    """Rows that start off a 16-byte boundary take the column-by-column path; V = 1 has one answer."""
    buf, params = kernel_case(1003, torch.float32)
    want = launch(buf[:, :1003], params)
    wide = torch.full((R, buf.shape[1] + 3), float("nan"), device=DEV)
    wide[:, 1:1004] = buf[:, :1003]
    assert torch.equal(launch(wide[:, 1:1004], params), want)
    bbuf, bparams = kernel_case(1003, BF)
    bwide = torch.full((R, bbuf.shape[1] + 3), float("nan"), dtype=BF, device=DEV)
    bwide[:, 1:1004] = bbuf[:, :1003]
    assert torch.equal(launch(bwide[:, 1:1004], bparams), launch(bbuf[:, :1003], bparams))
    one = torch.randn(R, 8, device=DEV)[:, :1]
    assert launch(one, [(t, k, p, s, c) for (t, k, p, s, c) in params]).tolist() == [0] * R


# ------------------------------------------------------------------------------------------
# 2. distribution
# ------------------------------------------------------------------------------------------

DRAWS = 16384
DIST = {"a": (37, 1.0, 0, 0.0, 47), "b": (37, 0.7, 0, 0.0, 44), "c": (1003, 1.5, 12, 0.0, 1018), "d": (1003, 0.8, 0, 0.9, 1011)}
PREPARED = {"a": (40.35, 33), "b": (39.28, 30), "c": (11.35, 11), "d": (199.84, 252)}


def kept_numpy(x, k, p):
    """The processors' kept set on fp64 logits: the values >= the k-th largest, then the sorted prefix up to and
    including the first element whose cumulative softmax (of the unscaled, top-k masked logits) exceeds p."""
    kept = np.ones(x.size, dtype=bool)
    if 0 < k < x.size:
        kept = x >= np.sort(x)[-k]
    if 0.0 < p < 1.0:
        order = np.argsort(-np.where(kept, x, -np.inf), kind="stable")[:int(kept.sum())]
        e = np.exp(x[order] - x[order[0]])
        cum = np.cumsum(e / e.sum())
        kept = np.zeros(x.size, dtype=bool)
        kept[order[:int(np.argmax(cum > p)) + 1]] = True
    return kept


def restated_draws(x, inv_t, kept, seed, counters):
    """argmax over the kept columns of x * inv_t + gumbel(u), u from Philox on {column / 4, row 0, offset = counter}."""
    V = x.size
    q = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    off = np.asarray(counters, dtype=np.uint64)[:, None]
    r = philox7(q, 0, off & np.uint64(0xFFFFFFFF), off >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(r, axis=-1).reshape(len(counters), -1)[:, :V]
    s = x.astype(np.float64)[None, :] * inv_t + gumbel64((words >> np.uint64(8)).astype(np.float64) * 2.0 ** -24)
    return np.where(kept[None, :], s, -np.inf).argmax(axis=1)


def chi_square(tokens, x, temperature, kept):
    """-> (statistic, degrees of freedom, 0.999 quantile) against softmax(x / temperature) over the kept set."""
    z = np.where(kept, x.astype(np.float64) / temperature, -np.inf)
    prob = np.exp(z - z.max())
    prob /= prob.sum()
    expect = DRAWS * prob
    counts = np.bincount(tokens, minlength=x.size).astype(np.float64)
    big = expect >= 5.0
    obs, exp = list(counts[big]), list(expect[big])
    if (kept & ~big).any():
        obs.append(counts[kept & ~big].sum())
        exp.append(expect[kept & ~big].sum())
    obs, exp = np.array(obs), np.array(exp)
    df = obs.size - 1
    bound = df * (1 - 2 / (9 * df) + 3.0902 * math.sqrt(2 / (9 * df))) ** 3
    return float(((obs - exp) ** 2 / exp).sum()), df, bound


@pytest.mark.parametrize("case", list(DIST))
def test_sampling_distribution(case):
    from vyomai_amd import ops
    V, temperature, k, p, gen_seed = DIST[case]
    x = (2 * np.random.default_rng(gen_seed).standard_normal(V)).astype(np.float32)
    counters = np.arange(1, DRAWS + 1)
    kept = kept_numpy(x.astype(np.float64), k, p)
    want = restated_draws(x, inv_t_of(temperature), kept, SEED, counters)
    stat, df, bound = chi_square(want, x, temperature, kept)
    print(f"case {case}: restatement chi-square {stat:.2f}, df {df}, bound {bound:.2f} (prepared: {PREPARED[case]})")
    assert kept[want].all()
    assert df == PREPARED[case][1] and stat <= bound, "the restatement moved"
    row = torch.from_numpy(x).to(DEV)
    assert np.array_equal((ops.sampling_probs(row[None], 1.0, k, p)[0] > 0).cpu().numpy(), kept), "kept set"
    logits = row[None].expand(DRAWS, V).contiguous()
    got = launch(logits, [(temperature, k, p, SEED, int(c)) for c in counters]).numpy()
    assert kept[got].all(), "a token outside the kept set was drawn"
    stat, df, bound = chi_square(got, x, temperature, kept)
    same = int((got == want).sum())
    print(f"case {case}: kernel chi-square {stat:.2f}, df {df}, bound {bound:.2f}; {same}/{DRAWS} draws equal the restatement's")
    assert stat <= bound


# ------------------------------------------------------------------------------------------
# 3. the engine
# ------------------------------------------------------------------------------------------

_MODELS = {}


def model(kind, dtype):
    """Tiny models with seeded random weights: ModelForCausalLM case a, Qwen3Model case q."""
    import vyomai_amd as V
    if (kind, dtype) not in _MODELS:
        with torch.random.fork_rng(devices=[]):         # (the weights are drawn on the host)
            torch.manual_seed(20 + len(kind))
            if kind == "causal_lm":
                m = V.ModelForCausalLM(V.Config(**CL.CASES["a"]))
            else:
                m = V.Qwen3Model(CQ.cfg("q", dtype))
        m = m.to(DEV).eval()
        if kind == "causal_lm" and dtype == BF:         # fp32 master weights, bf16 kernels
            m.compute_dtype = m.model.compute_dtype = BF
        _MODELS[kind, dtype] = m
    return _MODELS[kind, dtype]


def requests(sampled=True):
    """Six requests (prompt, SamplingParams or None): two greedy, four sampled."""
    import vyomai_amd as V
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, 512, (n,), generator=g).tolist() for n in (8, 13, 5, 21, 9, 11)]
    sp = [None, V.SamplingParams(0.7, seed=SEED), V.SamplingParams(1.0, top_k=12, seed=5),
          None, V.SamplingParams(1.5, top_p=0.9, seed=(1 << 63) + 11), V.SamplingParams(0.8, top_k=40, top_p=0.5, seed=1 << 32)]
    return [(pr, s if sampled else None) for pr, s in zip(prompts, sp)]


GEN = 6


def serve(m, dtype, reqs, **kw):
    """Two requests at once, then one more after every step: steps mix prefilling and decoding rows.
    -> ({sid: ids}, {sid: recorded logits rows}, sids)."""
    import vyomai_amd as V
    mgr = V.PagedKVManager(m.config, 32, 8, DEV, dtype)
    eng = V.ContinuousBatchEngine(m, mgr, eos_token_ids=[], record_logits=True, **kw)
    sids, done, left = [], {}, list(reqs)
    for _ in range(min(2, len(left))):
        pr, sp = left.pop(0)
        sids.append(eng.add_sequence(pr, max_gen_len=GEN, sampling=sp))
    for _ in range(200):
        if not (eng.active or eng.waiting_room or left):
            break
        done.update(eng.step())
        if left:
            pr, sp = left.pop(0)
            sids.append(eng.add_sequence(pr, max_gen_len=GEN, sampling=sp))
    assert len(done) == len(reqs) and eng.sampling == {}
    return done, eng.logits, sids


@pytest.mark.parametrize("schedule", ["default", "chunked"])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["causal_lm", "qwen3"])
def test_engine_mixed_batch(kind, dtype, schedule, monkeypatch):
    from vyomai_amd import ops
    m = model(kind, dtype)
    kw = dict(max_batch_size=6, max_step_tokens=8) if schedule == "chunked" else dict(max_batch_size=6)
    reqs = requests()
    calls, real = [], ops.sample_rows

    def counted(*a):
        calls.append(a[0].shape[0])
        return real(*a)

    monkeypatch.setattr(ops, "sample_rows", counted)
    done, logits, sids = serve(m, dtype, reqs, **kw)
    assert calls and max(calls) > 1, "mixed steps went through one launch over all rows"
    n_sampled = len(calls)
    # every emitted token is what the restated rule accepts on the recorded logits row, counter = position
    exact = total = 0
    for sid, (pr, sp) in zip(sids, reqs):
        ids = done[sid]
        assert ids[:len(pr)] == pr and len(ids) == len(pr) + GEN and len(logits[sid]) == GEN
        for j in range(GEN):
            pos = len(pr) + j
            row = logits[sid][j].to(DEV)                # (a bf16 row widened to fp32: the same values, so the same rule)
            param = (0, 0, 0.0, 0, 0) if sp is None else (sp.temperature, sp.top_k, sp.top_p, sp.seed, pos)
            hit, _ = judge(row, param, ids[pos], f"{kind} request {sid} position {pos}")
            exact, total = exact + hit, total + 1
    print(f"{kind} {dtype} {schedule}: {exact}/{total} tokens are the fp64 argmax of their restated score")
    # the same engine run twice
    done2, logits2, sids2 = serve(m, dtype, reqs, **kw)
    assert [done2[s] for s in sids2] == [done[s] for s in sids], "two runs differ"
    # greedy requests beside sampled ones produce what an all-greedy engine produces, up to exact ties
    calls.clear()
    gdone, glogits, gsids = serve(m, dtype, requests(sampled=False), **kw)
    assert calls == [], "an all-greedy workload makes no vy_sample_rows call"
    for i in (0, 3):
        a, b = done[sids[i]], gdone[gsids[i]]
        for pos in range(len(a)):
            if a[pos] != b[pos]:                        # a first difference must be an exact tie of the maximum
                j = pos - len(reqs[i][0])
                row = logits[sids[i]][j]
                assert torch.equal(row, glogits[gsids[i]][j]) and row[a[pos]] == row[b[pos]] == row.max(), (i, pos)
                break
    assert n_sampled > 0


@pytest.mark.parametrize("kind", ["causal_lm", "qwen3"])
def test_engine_request_alone_is_reproducible(kind):
    """A request with a fixed seed, alone, twice: identical logits rows, so identical tokens; and its tokens follow
    the restated rule, as they do inside a batch -- the stream is a function of (seed, position)."""
    m = model(kind, torch.float32)
    req = [requests()[4]]
    a, la, sa = serve(m, torch.float32, req)
    b, lb, sb = serve(m, torch.float32, req)
    assert all(torch.equal(x, y) for x, y in zip(la[sa[0]], lb[sb[0]]))
    assert a[sa[0]] == b[sb[0]]
    pr, sp = req[0]
    for j in range(GEN):
        judge(la[sa[0]][j].to(DEV), (sp.temperature, sp.top_k, sp.top_p, sp.seed, len(pr) + j), a[sa[0]][len(pr) + j],
              f"{kind} alone, position {len(pr) + j}")
