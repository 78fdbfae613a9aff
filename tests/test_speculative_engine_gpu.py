"""Speculative decoding in ContinuousBatchEngine on the MI355X, around the tiny models of test_serving_sampling_gpu.py
and drafters with other weights and half the layers: every decision and token follows the restated rule
(tests/spec_rule.py) on the recorded rows, the recorded target and draft rows are the models' dense forward at the same
positions (bars of test_paged_prefill_gpu.py: rel_err 2e-5 in fp32, 3e-2 in bf16), and with the target as its own
drafter a greedy run reproduces the plain engine in fewer steps.

block_size 8, g = 3, generation lengths that are no multiple of g + 1, requests arriving one per step so that prompt
chunks share steps with verification segments, and one request that starts from the prefix-cache blocks an earlier,
finished request left behind."""
import numpy as np
import pytest
import torch

from tests import spec_rule as SR
from tests.golden import cases_causal_lm as CL
from tests.golden import cases_qwen3 as CQ
from tests.test_causal_lm_gpu import rel_err
from tests.test_serving_sampling_gpu import SEED, inv_t_of, judge, model

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
G = 3
GENS = (6, 7, 9, 5, 6, 10, 7)
BAR = {torch.float32: 2e-5, BF: 3e-2}
_DRAFTERS = {}


def drafter(kind, dtype):
    """The target's shape with one layer instead of two, and weights of its own."""
    import vyomai_amd as V
    if (kind, dtype) not in _DRAFTERS:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(77 + len(kind))
            if kind == "causal_lm":
                m = V.ModelForCausalLM(V.Config(**dict(CL.CASES["a"], num_hidden_layers=1)))
            else:
                m = V.Qwen3Model(dict(CQ.cfg("q", dtype), n_layers=1))
        m = m.to(DEV).eval()
        if kind == "causal_lm" and dtype == BF:
            m.compute_dtype = m.model.compute_dtype = BF
        _DRAFTERS[kind, dtype] = m
    return _DRAFTERS[kind, dtype]


def requests(sampled=True):
    """Seven requests (prompt, SamplingParams or None); the last repeats the 21-token prompt of the fourth."""
    import vyomai_amd as V
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, 512, (n,), generator=g).tolist() for n in (8, 13, 5, 21, 9, 11)]
    prompts.append(list(prompts[3]))
    sp = [None, V.SamplingParams(0.7, seed=SEED), V.SamplingParams(1.0, top_k=12, seed=5), None,
          V.SamplingParams(1.5, top_p=0.9, seed=(1 << 63) + 11), V.SamplingParams(0.8, top_k=40, top_p=0.5, seed=1 << 32),
          V.SamplingParams(0.9, seed=77)]
    return [(pr, s if sampled else None) for pr, s in zip(prompts, sp)]


def serve(target, draft, dtype, reqs, gens=GENS, eos=(), fp8=False, **kw):
    """Two requests at once, one more after every step, the last one only when everything else has finished (so that it
    finds the fourth's prompt blocks in the prefix cache).  draft None: the plain engine.  -> (engine, {sid: ids}, sids,
    steps)."""
    import vyomai_amd as V
    mgr = V.PagedKVManager(target.config, 48, 8, DEV, dtype, kv_cache_dtype="fp8" if fp8 else None)
    if draft is not None:
        kw.update(draft_model=draft, draft_kv_mgr=V.PagedKVManager(draft.config, 48, 8, DEV, dtype), num_speculative_tokens=G)
    kw.setdefault("varlen_prefill", True)
    eng = V.ContinuousBatchEngine(target, mgr, eos_token_ids=list(eos), record_logits=True, **kw)
    sids, done, left, steps = [], {}, list(zip(reqs, gens)), 0
    last = left.pop() if len(left) == 7 else None

    def add(item):
        (pr, sp), gen = item
        sids.append(eng.add_sequence(pr, max_gen_len=gen, sampling=sp))

    for _ in range(min(2, len(left))):
        add(left.pop(0))
    for _ in range(300):
        if not (eng.active or eng.waiting_room or left):
            if last is None:
                break
            add(last)
            last = None
        done.update(eng.step())
        steps += 1
        if left:
            add(left.pop(0))
    assert len(done) == len(reqs) and eng.sampling == {} and eng.draft_computed == {} and not eng.active
    return eng, done, sids, steps


def check_rule(eng, done, sids, reqs, gens, what):
    """Every round of every request against the restatement; -> (drafted rows, accepted, in-band rows)."""
    rows = acc = band = 0
    for sid, (pr, sp), gen in zip(sids, reqs, gens):
        ids, rounds = done[sid], eng.rounds[sid]
        assert ids[:len(pr)] == pr
        par = (0, 0, 0.0, 0) if sp is None else (sp.temperature, sp.top_k, sp.top_p, sp.seed)
        at = len(pr)
        for rd in rounds:
            n, g, a, em = rd["position0"], len(rd["draft_tokens"]), rd["accepted"], rd["emitted"]
            assert n == at and ids[at:at + len(em)] == em and 0 <= a <= g <= G and len(em) <= a + 1
            assert rd["target_rows"].shape[0] == g + 1 and rd["draft_rows"].shape[0] == g
            assert em[:min(a, len(em))] == rd["draft_tokens"][:min(a, len(em))]
            for i in range(g):
                x = rd["draft_tokens"][i]
                # the drafter's own draw: vy_sample_rows' rule on its row, counter = the token's position
                judge(rd["draft_rows"][i].to(DEV), par + (n + i,), x, f"{what} request {sid} draft at {n + i}")
                if i > a:
                    continue                            # rows after the first rejection decide nothing
                r = SR.restate(rd["target_rows"][i].double().numpy(), rd["draft_rows"][i].double().numpy(), x,
                               inv_t_of(par[0]), par[1], par[2], par[3], n + i)
                rows, band = rows + 1, band + r["band"]
                if i < a:
                    acc += 1
                    SR.check(r, True, r["greedy_alt"] if r["greedy_alt"] is not None else -1, f"{what} {sid} @{n + i} accepted")
                elif len(em) == a + 1:
                    SR.check(r, False, em[a], f"{what} {sid} @{n + i} rejected")
            if a == g and len(em) == g + 1:             # the token after the last draft: the plain draw
                judge(rd["target_rows"][g].to(DEV), par + (n + g,), em[g], f"{what} request {sid} position {n + g}")
            at += len(em)
        assert at == len(ids) == len(pr) + gen and len(eng.logits[sid]) == gen
    return rows, acc, band


def check_dense(eng, done, sids, reqs, target, draft, dtype, what):
    """The recorded rows against the models' dense forward: the target rows that decided the emitted tokens on the final
    sequence, the draft rows on the prefix plus the drafts of their round."""
    worst_t = worst_d = 0.0
    for sid, (pr, _) in zip(sids, reqs):
        ids = done[sid]
        with torch.no_grad():
            dense = target(input_ids=torch.tensor([ids[:-1]], device=DEV), use_cache=False).logits[0, len(pr) - 1:]
        worst_t = max(worst_t, rel_err(torch.stack(eng.logits[sid]), dense.float().cpu().numpy()))
        for rd in eng.rounds[sid]:
            n, g = rd["position0"], len(rd["draft_tokens"])
            if not g:
                continue
            seq = ids[:n] + rd["draft_tokens"][:g - 1]
            with torch.no_grad():
                dd = draft(input_ids=torch.tensor([seq], device=DEV), use_cache=False).logits[0, n - 1:]
            worst_d = max(worst_d, rel_err(rd["draft_rows"], dd.float().cpu().numpy()))
    print(f"{what}: target rows against the dense forward rel_err {worst_t:.3e}, draft rows {worst_d:.3e}")
    assert worst_t < BAR[dtype] and worst_d < BAR[dtype], (worst_t, worst_d)


@pytest.mark.parametrize("kind,dtype", [("causal_lm", torch.float32), ("causal_lm", BF), ("qwen3", BF)],
                         ids=["causal_lm-fp32", "causal_lm-bf16", "qwen3-bf16"])
def test_rule_and_rows(kind, dtype):
    target, draft = model(kind, dtype), drafter(kind, dtype)
    reqs = requests()
    eng, done, sids, steps = serve(target, draft, dtype, reqs)
    rows, acc, band = check_rule(eng, done, sids, reqs, GENS, f"{kind} {dtype}")
    print(f"{kind} {dtype}: {steps} steps, {eng.drafts_proposed} drafts proposed, {eng.drafts_accepted} accepted; "
          f"{rows} rows judged ({band} inside the band)")
    assert 0 < eng.drafts_accepted <= eng.drafts_proposed and acc == eng.drafts_accepted
    # the last request started from the blocks the fourth left in the prefix cache, in both managers' pages
    assert eng.prompt_tokens_computed[sids[6]] == 21 - 16 and eng.prompt_tokens_computed[sids[3]] == 21
    assert any(len(rd["draft_tokens"]) < G for sid in sids for rd in eng.rounds[sid][1:]), \
        "some round was clipped by the end of its request"
    if kind == "causal_lm":
        check_dense(eng, done, sids, reqs, target, draft, dtype, f"{kind} {dtype}")
    eng2, done2, sids2, steps2 = serve(target, draft, dtype, reqs)
    assert [done2[s] for s in sids2] == [done[s] for s in sids] and steps2 == steps, "two runs differ"


def test_target_as_its_own_drafter_reproduces_the_plain_engine():
    """Greedy, fp32.  The verification rows come from the varlen prefill kernel, the plain engine's from the decode
    kernel; both lie within the fp32 logits bar (rel_err 2e-5) of the dense forward, so a first difference in the ids
    is accepted only where the two tokens' logits lie within twice that bar of each other on the recorded row."""
    target = model("causal_lm", torch.float32)
    reqs = requests(sampled=False)
    eng, done, sids, steps = serve(target, target, torch.float32, reqs)
    plain, pdone, psids, psteps = serve(target, None, torch.float32, reqs)
    for sid, psid, (pr, _) in zip(sids, psids, reqs):
        a, b = done[sid], pdone[psid]
        assert len(a) == len(b)
        for pos in range(len(a)):
            if a[pos] != b[pos]:
                row = eng.logits[sid][pos - len(pr)]
                assert abs(float(row[a[pos]] - row[b[pos]])) <= 2 * 2e-5 * float(row.abs().max()), (sid, pos)
                break
    print(f"drafter = target: {steps} steps against {psteps}, {eng.drafts_accepted}/{eng.drafts_proposed} drafts accepted")
    assert steps < psteps
    assert 0 < eng.drafts_accepted <= eng.drafts_proposed
    check_rule(eng, done, sids, reqs, GENS, "drafter = target")


def test_stop_token_among_accepted_drafts():
    """The stop token is the plain run's third generated token, of the first request whose first two differ from it (else
    the request would already end at its first token; the greedy requests of these random models repeat one token, so
    it is a sampled one).  With the target as its own drafter p = q, every draft is accepted, and the stop token is the
    second draft of the first round."""
    target = model("causal_lm", torch.float32)
    every = requests()[:6]
    _, pdone, psids, _ = serve(target, None, torch.float32, every, GENS[:6])
    tails = [pdone[sid][len(pr):] for sid, (pr, _) in zip(psids, every)]
    print("plain generations:", tails)
    pick = next(i for i, t in enumerate(tails) if t[2] not in t[:2])
    req, gens, stop = [every[pick]], (9,), tails[pick][2]
    pr = req[0][0]
    _, want, wsids, _ = serve(target, None, torch.float32, req, gens, eos=[stop])
    eng, done, sids, _ = serve(target, target, torch.float32, req, gens, eos=[stop])
    assert want[wsids[0]] == pr + tails[pick][:3]
    assert done[sids[0]] == want[wsids[0]], "the request ends at the stop token"
    rd = eng.rounds[sids[0]][-1]
    assert rd["emitted"][-1] == stop and len(rd["emitted"]) <= rd["accepted"], "the stop token was an accepted draft"


def test_max_gen_len_one():
    target, draft = model("causal_lm", torch.float32), drafter("causal_lm", torch.float32)
    reqs, gens = requests()[:3], (1, 1, 1)
    eng, done, sids, steps = serve(target, draft, torch.float32, reqs, gens)
    plain, pdone, psids, _ = serve(target, None, torch.float32, reqs, gens)
    assert eng.drafts_proposed == 0 and [done[s] for s in sids] == [pdone[s] for s in psids]
    check_rule(eng, done, sids, reqs, gens, "max_gen_len 1")


@pytest.mark.parametrize("dtype,fp8", [(torch.float32, False), (BF, True)], ids=["fp32", "bf16-fp8-target-pages"])
def test_chunked_prefill_at_the_minimum_budget(dtype, fp8):
    """max_step_tokens = max_batch_size * (g + 1), the smallest the constructor takes: prompts go in chunks beside the
    verification segments.  The second case keeps the target's pages in fp8 (the drafter's stay bf16)."""
    target, draft = model("causal_lm", dtype), drafter("causal_lm", dtype)
    reqs = requests()
    eng, done, sids, steps = serve(target, draft, dtype, reqs, fp8=fp8, max_batch_size=3, max_step_tokens=3 * (G + 1))
    rows, acc, band = check_rule(eng, done, sids, reqs, GENS, f"chunked {dtype}")
    print(f"chunked {dtype} fp8={fp8}: {steps} steps, {eng.drafts_accepted}/{eng.drafts_proposed} drafts accepted, {rows} rows judged")
    assert eng.drafts_proposed > 0
    if not fp8:
        check_dense(eng, done, sids, reqs, target, draft, dtype, f"chunked {dtype}")
