"""Speculative decoding: vy_spec_verify against the composition the same rows would otherwise need, and the serving engine
with and without a drafter.   python tools/bench_speculative.py [--iters 500] [--skip-engine] [--skip-kernels]

Kernel (bf16 logits of the engine model's vocabulary, S in {8, 32} sequences, gamma = 4, every sequence with 4 drafts):
  (a) ops.spec_verify, one launch over the S * 5 rows
  (b) the composition: ops.sampling_probs on the S * 5 target rows and on the S * 4 draft rows (fp32 [rows, V]
      probabilities written and read back), gather p(x) / q(x), compare with torch.rand, norm_fn(p - q) on every row
      (the first rejection is not known on the device), torch.multinomial over the S * 5 rows
  (b') the same without torch.multinomial, which checks its input on the host and cannot be captured
Two parameter sets: temperature 0.8 alone, and temperature 0.8 with top_k = 50 and top_p = 0.9 (vy_sampling_probs takes
one set for all rows, so (b) could not serve per-request parameters at all).  (a) and (b') are timed as links of a
captured chain of 50 calls (tools/bench_paged.py's timed_graph); (a) and (b) are also timed eagerly with device events
(tools/bench_sampling.py's timed_eager), figures that carry the host's launch cost.  Three repeats: lowest .. highest.

Engine: the workload of tools/bench_paged.py (6 requests of mixed lengths, 384 requested tokens) on an 8-layer model,
sampled (temperature 0.8, top_p 0.9) and greedy, varlen_prefill=True: no drafter, the target as its own drafter (an upper
bound: acceptance about 1), and a drafter of the target's width with a quarter of its layers and weights of its own.
Tokens per second (requested tokens / wall time), steps, and drafts accepted / proposed.  The weights are random: the
small drafter's acceptance says nothing about a trained pair.
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vyomai_amd as V  # noqa: E402
from vyomai_amd import ops  # noqa: E402
from bench_paged import timed_graph  # noqa: E402
from bench_sampling import timed_eager  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
VOCAB, GAMMA = 32000, 4


def config(layers):
    return V.Config(vocab_size=VOCAB, hidden_size=896, intermediate_size=4864, num_hidden_layers=layers,
                    num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=1024, pad_token_id=0)


def bench_kernel(iters, repeats=3):
    for S in (8, 32):
        g = torch.Generator().manual_seed(S)
        target = (2.0 * torch.randn(S * (GAMMA + 1), VOCAB, generator=g)).to(BF).to(DEV)
        draft = (target.view(S, GAMMA + 1, VOCAB)[:, :GAMMA].transpose(0, 1).float().cpu() +
                 torch.randn(GAMMA, S, VOCAB, generator=g)).to(BF).to(DEV).contiguous()
        t_row0 = torch.arange(S, dtype=torch.int32, device=DEV) * (GAMMA + 1)
        n_draft = torch.full((S,), GAMMA, dtype=torch.int32, device=DEV)
        seed = (torch.arange(S, dtype=torch.long) * 0x9E3779B97F4A7C1 + 12345).to(DEV)
        pos0 = torch.arange(100, 100 + S, dtype=torch.long, device=DEV)
        rows_of = (t_row0.long()[None, :] + torch.arange(GAMMA, device=DEV)[:, None]).view(-1)   # target row of (i, s)
        for name, k, p in (("temperature 0.8", 0, 0.0), ("temperature 0.8, top_k 50, top_p 0.9", 50, 0.9)):
            inv_t = torch.full((S,), 1.0 / 0.8, dtype=torch.float32, device=DEV)
            kk = torch.full((S,), k, dtype=torch.int32, device=DEV)
            pp = torch.full((S,), p, dtype=torch.float32, device=DEV)
            tokens = torch.stack([ops.sample_rows(draft[i], inv_t, kk, pp, seed, pos0 + i) for i in range(GAMMA)])

            def fused():
                return ops.spec_verify(target, draft, tokens, t_row0, n_draft, inv_t, kk, pp, seed, pos0)

            def composed(draw=True):
                P = ops.sampling_probs(target, 0.8, k, p)
                Q = ops.sampling_probs(draft.view(-1, VOCAB), 0.8, k, p)
                x = tokens.view(-1, 1)
                px, qx = P[rows_of].gather(1, x), Q.gather(1, x)
                reject = torch.rand(x.shape, device=DEV) * qx > px
                res = P.clone()
                res[rows_of] = torch.clamp(P[rows_of] - Q, min=0.0)
                res = res / res.sum(-1, keepdim=True)
                return (reject, torch.multinomial(res, 1)) if draw else (reject, res)

            acc = fused()[0][:, :GAMMA].float().mean().item()
            tg = [timed_graph([fused, lambda: composed(False)], 5, iters) for _ in range(repeats)]
            te = [timed_eager([fused, composed]) for _ in range(repeats)]
            rec = {"what": "spec_verify against the composition", "S": S, "gamma": GAMMA, "V": VOCAB, "parameters": name,
                   "accepted_share_of_rows": round(acc, 3)}
            for i, key in enumerate(("spec_verify", "composition")):
                rec[key + "_chain_us" + ("" if i == 0 else "_without_multinomial")] = [round(min(r[i] for r in tg), 2),
                                                                                      round(max(r[i] for r in tg), 2)]
                rec[key + "_eager_us"] = [round(min(r[i] for r in te), 2), round(max(r[i] for r in te), 2)]
            rec["composition_over_spec_verify_chain"] = round(min(r[1] for r in tg) / min(r[0] for r in tg), 2)
            rec["composition_over_spec_verify_eager"] = round(min(r[1] for r in te) / min(r[0] for r in te), 2)
            print(json.dumps(rec), flush=True)


def bench_engine(rounds=3):
    torch.manual_seed(0)
    target = V.ModelForCausalLM(config(8)).to(BF).to(DEV).eval()
    torch.manual_seed(1)
    small = V.ModelForCausalLM(config(2)).to(BF).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    plen, glen = [12, 40, 96, 24, 160, 64], [64, 32, 128, 16, 96, 48]
    prompts = [torch.randint(3, VOCAB, (n,), generator=g).tolist() for n in plen]

    def run(drafter, sampled):
        kw = {}
        if drafter is not None:
            kw = dict(draft_model=drafter, draft_kv_mgr=V.PagedKVManager(drafter.config, 64, 16, DEV, BF),
                      num_speculative_tokens=GAMMA)
        eng = V.ContinuousBatchEngine(target, V.PagedKVManager(target.config, 64, 16, DEV, BF), max_batch_size=8,
                                      eos_token_ids=[], varlen_prefill=True, **kw)
        for i, (p, n) in enumerate(zip(prompts, glen)):
            eng.add_sequence(p, max_gen_len=n, sampling=V.SamplingParams(0.8, top_p=0.9, seed=i + 1) if sampled else None)
        steps = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while eng.active or eng.waiting_room:
            eng.step()
            steps += 1
        torch.cuda.synchronize()
        return time.perf_counter() - t0, steps, eng.drafts_accepted, eng.drafts_proposed

    pairs = (("no drafter", None), ("drafter = target", target), ("drafter: 2 of 8 layers", small))
    for sampled in (True, False):
        for _, d in pairs:
            run(d, sampled)                    # warm-up: every shape of every run
        res = {name: [] for name, _ in pairs}
        for _ in range(rounds):
            for name, d in pairs:
                res[name].append(run(d, sampled))
        base = min(r[0] for r in res["no drafter"])
        for name, _ in pairs:
            t = sorted(r[0] for r in res[name])
            _, steps, acc, prop = res[name][0]
            print(json.dumps({"what": "engine", "requests": "sampled 0.8 / top_p 0.9" if sampled else "greedy",
                              "drafter": name, "requested_tokens": sum(glen), "steps": steps, "rounds": rounds,
                              "seconds": [round(t[0], 4), round(t[-1], 4)],
                              "tokens_per_s": [round(sum(glen) / t[-1], 1), round(sum(glen) / t[0], 1)],
                              "speedup_lowest_times": round(base / t[0], 3),
                              "drafts_accepted": acc, "drafts_proposed": prop,
                              "acceptance": round(acc / prop, 3) if prop else None}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_speculative.py needs the MI355X: there is nothing to time without it")
    if not a.skip_kernels:
        bench_kernel(a.iters)
    if not a.skip_engine:
        bench_engine()
