"""Per-request LoRA adapters in ContinuousBatchEngine on the MI355X: requests under no adapter, n1 and n2 mixed in one
batch over ONE copy of the base weights, against what the REAL reference computes with its linears wrapped by its own
LoraLinear (tests/golden/lora.npz, make_golden_lora.py) -- bars of the engine tests: rel_err 2e-5 in fp32 with equal
greedy ids, 3e-2 in bf16.  block_size 8, two requests at once and one more after every step (the serve() pattern of
test_speculative_engine_gpu.py), late requests once everything else has finished, so that they find prefix blocks.

Rows are compared while the run is on the golden's sequence: up to and including the first generated token that differs
(in fp32 none may differ)."""
import copy

import pytest
import torch

from tests.golden import cases_causal_lm as CL
from tests.golden import cases_lora as L
from tests.golden import cases_qwen3 as CQ
from tests.test_causal_lm_gpu import build, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
BAR = {torch.float32: 2e-5, BF: 3e-2}
_MODELS, _STORES = {}, {}


def target(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = build(CL.CASES[L.CASE], compute=BF if dtype == BF else None).eval()
    return _MODELS[dtype]


def store(golden, dtype):
    import vyomai_amd as V
    if dtype not in _STORES:
        st = V.LoraAdapters(target(dtype), 4, max_rank=32)
        assert st.dtype == dtype and st.device.type == "cuda"
        for who, spec in L.ADAPTERS.items():
            st.load(who, L.load(golden("lora"), who), alpha=spec["alpha"])
        _STORES[dtype] = st
    return _STORES[dtype]


def serve(model, dtype, reqs, adapters=None, late=(), fp8=False, draft=None, blocks=64, **kw):
    """reqs / late: (prompt, adapter name or None, max_gen_len).  -> (engine, {sid: ids}, sids in request order, steps)."""
    import vyomai_amd as V
    mgr = V.PagedKVManager(model.config, blocks, 8, DEV, dtype, kv_cache_dtype="fp8" if fp8 else None)
    if draft is not None:
        kw.update(draft_model=draft, draft_kv_mgr=V.PagedKVManager(draft.config, blocks, 8, DEV, dtype), num_speculative_tokens=3)
    if adapters is not None:
        kw.update(adapters=adapters)
    eng = V.ContinuousBatchEngine(model, mgr, eos_token_ids=[], record_logits=True, varlen_prefill=True, **kw)
    sids, done, left, late, steps = [], {}, list(reqs), list(late), 0

    def add(req):
        pr, who, gen = req
        sids.append(eng.add_sequence(pr, max_gen_len=gen, adapter=who) if adapters is not None else
                    eng.add_sequence(pr, max_gen_len=gen))

    for _ in range(min(2, len(left))):
        add(left.pop(0))
    for _ in range(400):
        if not (eng.active or eng.waiting_room or left):
            if not late:
                break
            add(late.pop(0))
        done.update(eng.step())
        steps += 1
        if left:
            add(left.pop(0))
    assert len(done) == len(sids) and eng.sampling == {} and eng.adapter == {} and not eng.active
    if adapters is not None:
        assert not any(adapters.held.values())
    return eng, done, sids, steps


def golden_requests(g):
    """-> (early, late) requests with what the golden holds for each: (prompt, who, gen, ids, rows)."""
    early, late = [], []
    for b in range(CL.B):
        for who in L.WHO:
            early.append((g["prompt"][b].tolist(), who, L.NEW, g[f"{who}.greedy"][b], g[f"{who}.greedy.logits"][b]))
    long = g["long"].tolist()
    for who, where in (("base", early), ("n1", early), ("n1", late), ("n2", late), ("base", late)):
        where.append((long, who, L.NEW, g[f"{who}.long.greedy"], g[f"{who}.long.logits"]))
    return early, late


def wire(reqs):
    return [(pr, None if who == "base" else who, gen) for pr, who, gen, *_ in reqs]


def follow(eng, done, sid, req, bar, equal_ids, what):
    """The recorded rows of one request against the golden's while the run is on the golden's sequence."""
    pr, who, gen, ids, rows = req
    got = done[sid][len(pr):]
    assert done[sid][:len(pr)] == pr and len(got) == gen == len(eng.logits[sid])
    n = next((i + 1 for i in range(gen) if got[i] != int(ids[i])), gen)
    err = rel_err(torch.stack(eng.logits[sid][:n]), rows[:n])
    assert err < bar, (what, who, err)
    if equal_ids:
        assert got == ids.tolist(), (what, who, got, ids.tolist())
    return err


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_mixed_batch_and_prefix_cache_against_the_golden(golden, dtype):
    g = golden("lora")
    early, late = golden_requests(g)
    st = store(golden, dtype)
    eng, done, sids, steps = serve(target(dtype), dtype, wire(early), st, wire(late))
    worst = max(follow(eng, done, sid, req, BAR[dtype], dtype == torch.float32, f"{dtype}")
                for sid, req in zip(sids, early + late))
    print(f"{dtype}: {len(sids)} requests in {steps} steps, largest rel_err against the golden {worst:.3e}")
    computed = [eng.prompt_tokens_computed[sid] for sid in sids[-5:]]
    # long under base and n1 first; then n1 again and base again start from their own blocks, n2 finds none
    assert computed == [21, 21, 21 - 16, 21, 21 - 16], computed
    # the adapters moved the rows: the n1 / n2 rows are far from the base's golden
    assert rel_err(torch.stack(eng.logits[sids[1]]), g["base.greedy.logits"][0]) > 0.1


def test_chunked_prefill_across_tile_cuts(golden):
    """max_step_tokens 20: the 21-token prompts go in chunks of up to 20 rows (tiles of 16 + 4 and what the decoding
    rows leave), beside decoding rows of other adapters."""
    dtype = torch.float32
    g = golden("lora")
    early, late = golden_requests(g)
    reqs = [r for r in early + late[1:2] if len(r[0]) == L.LONG] + early[:3]
    eng, done, sids, steps = serve(target(dtype), dtype, wire(reqs), store(golden, dtype), max_batch_size=4,
                                   max_step_tokens=20)
    worst = max(follow(eng, done, sid, req, BAR[dtype], True, "chunked") for sid, req in zip(sids, reqs))
    print(f"chunked: {steps} steps, largest rel_err against the golden {worst:.3e}")


def test_speculative_with_a_base_weight_drafter(golden):
    """The drafter is the target itself without adapters (its forwards carry no tiles): the accept / reject rule is exact
    for any drafter, so the greedy ids are the golden's, in fewer steps than the plain engine takes."""
    dtype = torch.float32
    g = golden("lora")
    early, _ = golden_requests(g)
    m, st = target(dtype), store(golden, dtype)
    eng, done, sids, steps = serve(m, dtype, wire(early), st, draft=m)
    _, pdone, psids, psteps = serve(m, dtype, wire(early), st)
    for sid, psid, req in zip(sids, psids, early):
        assert done[sid] == pdone[psid] == req[0] + req[3].tolist(), req[1]
        follow(eng, done, sid, req, BAR[dtype], True, "speculative")
    print(f"speculative: {steps} steps against {psteps}, {eng.drafts_accepted}/{eng.drafts_proposed} drafts accepted")
    assert steps < psteps and 0 < eng.drafts_accepted


def test_fp8_pages(golden, monkeypatch):
    """bf16 with fp8 KV pages against the same engine over bf16 pages whose written rows are requantised (the reference
    of test_paged_fp8_gpu.py): both sides hold the same quantised cache; its bar for engine rows, rel_err 3e-2."""
    from tests.test_paged_fp8_gpu import _requantise_written_rows
    g = golden("lora")
    early, _ = golden_requests(g)
    m, st = target(BF), store(golden, BF)
    eng, done, sids, _ = serve(m, BF, wire(early), st, fp8=True)
    _requantise_written_rows(monkeypatch)
    ref, rdone, rsids, _ = serve(m, BF, wire(early), st)
    worst = 0.0
    for sid, rsid, req in zip(sids, rsids, early):
        a, b = done[sid], rdone[rsid]
        n = next((i + 1 for i in range(L.NEW) if a[len(req[0]) + i] != b[len(req[0]) + i]), L.NEW)
        worst = max(worst, rel_err(torch.stack(eng.logits[sid][:n]), torch.stack(ref.logits[rsid][:n]).numpy()))
    print(f"fp8 pages: largest rel_err against the requantised-bf16 engine {worst:.3e}")
    assert worst < 3e-2, worst


def qwen_adapter(seed, rank, on):
    cfg = CQ.CASES["q"]
    d, q, kv, f = cfg["emb_dim"], cfg["n_heads"] * cfg["head_dim"], cfg["n_kv_groups"] * cfg["head_dim"], cfg["hidden_dim"]
    shapes = {"att.W_query": (q, d), "att.W_key": (kv, d), "att.W_value": (kv, d), "att.out_proj": (d, q),
              "ff.fc1": (f, d), "ff.fc2": (f, d), "ff.fc3": (d, f)}
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for l in range(cfg["n_layers"]):
        for path in on:
            out_f, in_f = shapes[path]
            # multiples of 2^-10 inside (-0.1, 0.1): exact in bf16, as the golden's adapters
            sd[f"trf_blocks.{l}.{path}.lora_a"] = torch.randint(-102, 103, (rank, in_f), generator=gen) / 1024.0
            sd[f"trf_blocks.{l}.{path}.lora_b"] = torch.randint(-102, 103, (out_f, rank), generator=gen) / 1024.0
    return sd


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_qwen3_against_merged_weights(dtype):
    """Qwen3Model case q has no importable reference class: the adapter engine's rows against an engine over a copy of
    the model with W + alpha * lora_b @ lora_a merged into its linears (the re-associated computation, which the golden
    maker holds within 2e-5 of the wrapped one for the reference's own fp32)."""
    import vyomai_amd as V
    base = CQ.build(V.Qwen3Model, "q", dtype).to(DEV)
    every = ("att.W_query", "att.W_key", "att.W_value", "att.out_proj", "ff.fc1", "ff.fc2", "ff.fc3")
    specs = {"n1": (qwen_adapter(1, 32, every[:1] + every[2:]), 1.0), "n2": (qwen_adapter(2, 8, every), 2.0)}
    st = V.LoraAdapters(base, 2, max_rank=32)
    merged = {None: base}
    for who, (sd, alpha) in specs.items():
        st.load(who, sd, alpha=alpha)
        m = copy.deepcopy(base)
        own = dict(m.named_modules())
        with torch.no_grad():
            for key in {k.rsplit(".", 1)[0] for k in sd}:
                w = own[key].weight
                w.copy_((w.float() + alpha * sd[key + ".lora_b"].to(DEV) @ sd[key + ".lora_a"].to(DEV)).to(w.dtype))
        merged[who] = m
    gen = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, 512, (n,), generator=gen).tolist() for n in (8, 13, 5, 21, 9, 17)]
    reqs = [(pr, (None, "n1", "n2")[i % 3], 5) for i, pr in enumerate(prompts)]
    eng, done, sids, _ = serve(base, dtype, reqs, st)
    worst, moved = 0.0, 0.0
    for who, m in merged.items():
        mine = [(sid, req) for sid, req in zip(sids, reqs) if req[1] == who]
        ref, rdone, rsids, _ = serve(m, dtype, [req for _, req in mine])
        for (sid, req), rsid in zip(mine, rsids):
            a, b = done[sid][len(req[0]):], rdone[rsid][len(req[0]):]
            n = next((i + 1 for i in range(5) if a[i] != b[i]), 5)
            worst = max(worst, rel_err(torch.stack(eng.logits[sid][:n]), torch.stack(ref.logits[rsid][:n]).numpy()))
        if who is not None:
            bref, bdone, bsids, _ = serve(base, dtype, [req for _, req in mine])
            moved = max(moved, rel_err(eng.logits[mine[0][0]][0], bref.logits[bsids[0]][0].numpy()))
    print(f"qwen3 {dtype}: largest rel_err against the merged-weight engines {worst:.3e}; adapters moved a row by {moved:.3f}")
    assert worst < BAR[dtype] and moved > 0.05, (worst, moved)


def test_base_requests_launch_what_an_engine_without_a_store_launches(golden, monkeypatch):
    from vyomai_amd import _lib, ops
    names, real = [], _lib.call

    def recorded(name, *args):
        names.append(name)
        return real(name, *args)

    dtype = torch.float32
    g = golden("lora")
    early, late = golden_requests(g)
    reqs = [(pr, None, gen) for pr, who, gen, *_ in early if who == "base"] + [(early[0][0][:5], None, 3)]
    m = target(dtype)
    serve(m, dtype, reqs[:1])                               # (workspaces and cached weight copies exist from here on)
    monkeypatch.setattr(_lib, "call", recorded)
    monkeypatch.setattr(ops, "call", recorded)
    _, done0, sids0, steps0 = serve(m, dtype, reqs)
    without, names[:] = list(names), []
    _, done1, sids1, steps1 = serve(m, dtype, reqs, store(golden, dtype))
    assert names == without and len(names) > 0 and steps0 == steps1
    assert not any("lora" in n for n in names)
    assert [done1[s] for s in sids1] == [done0[s] for s in sids0]
    names[:] = []
    serve(m, dtype, [(pr, "n1", gen) for pr, _, gen in reqs], store(golden, dtype))
    per_layer = names.count("vy_lora_shrink") / (steps0 * m.config.num_hidden_layers)
    assert names.count("vy_lora_shrink") == names.count("vy_lora_expand") and per_layer == 4, per_layer
