"""Per-request sampling: vy_sample_rows against torch.argmax and against vy_sampling_probs + torch.multinomial, and the
serving engine all-greedy against all-sampled.   python tools/bench_sampling.py [--iters 1000] [--skip-engine]

Kernels (bf16 logits, R in {8, 32} rows of V in {32000, 151936}):
  (a) torch.argmax                      (b) ops.sampling_probs + torch.multinomial (uniform parameters: what generate() does)
  (c) ops.sample_rows, all rows greedy  (d) temperature only   (e) top_k = 50   (f) top_p = 0.9   (g) both filters
  (h) half the rows greedy, half as (g)
Each is timed as a link of a captured chain of 50 calls, the chains replayed in turn (tools/bench_paged.py's timed_graph).
torch.multinomial checks its input on the host, so the second stage of (b) cannot be captured: the chain of (b) holds
ops.sampling_probs alone (a lower bound of (b)), and ALL variants are also timed eagerly with device events over enough
calls to fill a good fraction of a second -- those figures carry the host's launch cost and, for (b), multinomial's wait.
Bytes are computed from the shapes: every pass over a row reads R * V * 2; (b) also writes (and multinomial reads) the
fp32 [R, V] probabilities.  The one-pass variants are given as a share of the copy ceiling measured in the same run.
The whole measurement is repeated three times; figures are lowest .. highest.

Engine: the workload of tools/bench_paged.py (6 requests of mixed lengths, 384 requested tokens), all-greedy and
all-sampled (temperature 0.8, top_p 0.9) alternating in one call: seconds per run lowest .. highest, and the sampled
run's extra time per step.
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
from bench_paged import copy_ceiling_gbs, timed_graph  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
SHAPES = [(8, 32000), (32, 32000), (8, 151936), (32, 151936)]
# passes over the row: the maximum (nucleus only), 8 radix passes per top-k, 1 + 8 per nucleus, the draw
PASSES = {"c greedy": 1, "d temperature": 1, "e top_k 50": 9, "f top_p 0.9": 11, "g both": 19}


def params(R, temperature, top_k, top_p, greedy_rows=0):
    inv = torch.full((R,), 1.0 / temperature, dtype=torch.float32)
    inv[:greedy_rows] = 0.0
    seed = torch.arange(R, dtype=torch.long) * 0x9E3779B97F4A7C1 + 12345
    return (inv.to(DEV), torch.full((R,), top_k, dtype=torch.int32, device=DEV),
            torch.full((R,), top_p, dtype=torch.float32, device=DEV), seed.to(DEV),
            torch.arange(100, 100 + R, dtype=torch.long, device=DEV))


def timed_eager(fns, seconds=0.25):
    """us per call of each fn, launched eagerly: a trial of 20 calls sizes the run to about `seconds`."""
    out = []
    for f in fns:
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            f()
        torch.cuda.synchronize()
        n = max(20, min(5000, int(seconds / max((time.perf_counter() - t0) / 20, 1e-6))))
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            f()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / n)
    return out


def bench_kernels(iters, repeats=3):
    ceiling = copy_ceiling_gbs()
    print(json.dumps({"what": "copy ceiling", "GBs": round(ceiling, 1)}))
    for R, Vv in SHAPES:
        g = torch.Generator().manual_seed(R + Vv)
        logits = (2.0 * torch.randn(R, Vv, generator=g)).to(BF).to(DEV)
        sets = {"c greedy": params(R, 1.0, 0, 0.0, greedy_rows=R), "d temperature": params(R, 0.8, 0, 0.0),
                "e top_k 50": params(R, 0.8, 50, 0.0), "f top_p 0.9": params(R, 0.8, 0, 0.9),
                "g both": params(R, 0.8, 50, 0.9), "h half greedy, half both": params(R, 0.8, 50, 0.9, greedy_rows=R // 2)}
        names = ["a torch.argmax", "b sampling_probs + multinomial"] + list(sets)
        chain = [lambda: torch.argmax(logits, dim=-1), lambda: ops.sampling_probs(logits, 0.8, 50, 0.9)]
        eager = [chain[0], lambda: torch.multinomial(ops.sampling_probs(logits, 0.8, 50, 0.9), 1)]
        for p in sets.values():
            chain.append(lambda p=p: ops.sample_rows(logits, *p))
            eager.append(chain[-1])
        runs_g = [timed_graph(chain, 5, iters) for _ in range(repeats)]
        runs_e = [timed_eager(eager) for _ in range(repeats)]
        row = R * Vv * 2
        for i, name in enumerate(names):
            tg, te = [r[i] for r in runs_g], [r[i] for r in runs_e]
            rec = {"what": "sampling kernel", "R": R, "V": Vv, "variant": name,
                   "chain_us": [round(min(tg), 2), round(max(tg), 2)], "eager_us": [round(min(te), 2), round(max(te), 2)]}
            if name[0] == "a":
                rec.update(read_bytes=row, write_bytes=R * 8)
            elif name[0] == "b":
                rec.update(chain_holds="sampling_probs alone", read_bytes=(1 + 8 + 9 + 2) * row + R * Vv * 4,
                           write_bytes=R * Vv * 4 + R * 8)
            elif name[0] == "h":
                rec.update(read_bytes=(R // 2) * Vv * 2 * (1 + PASSES["g both"]), write_bytes=R * 8)
            else:
                rec.update(read_bytes=PASSES[name] * row, write_bytes=R * 8)
            if name[0] in "acd":
                rec["share_of_copy_ceiling"] = round(rec["read_bytes"] / min(tg) * 1e-3 / ceiling, 4)
            print(json.dumps(rec))


def bench_engine(rounds=5):
    cfg = V.Config(vocab_size=32000, hidden_size=896, intermediate_size=4864, num_hidden_layers=4,
                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=1024, pad_token_id=0)
    torch.manual_seed(0)
    m = V.ModelForCausalLM(cfg).to(BF).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    plen, glen = [12, 40, 96, 24, 160, 64], [64, 32, 128, 16, 96, 48]
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in plen]

    def run(sampled):
        mgr = V.PagedKVManager(cfg, 64, 16, DEV, BF)
        eng = V.ContinuousBatchEngine(m, mgr, max_batch_size=8, eos_token_ids=[])
        for i, (p, n) in enumerate(zip(prompts, glen)):
            eng.add_sequence(p, max_gen_len=n, sampling=V.SamplingParams(0.8, top_p=0.9, seed=i + 1) if sampled else None)
        steps = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while eng.active or eng.waiting_room:
            eng.step()
            steps += 1
        return time.perf_counter() - t0, steps

    run(False), run(True)                      # warm-up: every shape of both runs
    res = {False: [], True: []}
    for _ in range(rounds):
        for sampled in (False, True):
            res[sampled].append(run(sampled))
    tg, ts = sorted(r[0] for r in res[False]), sorted(r[0] for r in res[True])
    steps = res[True][0][1]
    print(json.dumps({"what": "engine, greedy against sampled", "requests": len(prompts), "requested_tokens": sum(glen),
                      "steps": steps, "rounds": rounds,
                      "greedy_seconds": [round(tg[0], 4), round(tg[len(tg) // 2], 4), round(tg[-1], 4)],
                      "sampled_seconds": [round(ts[0], 4), round(ts[len(ts) // 2], 4), round(ts[-1], 4)],
                      "extra_us_per_step_median": round((ts[len(ts) // 2] - tg[len(tg) // 2]) / steps * 1e6, 1),
                      "extra_us_per_step_lowest": round((ts[0] - tg[0]) / steps * 1e6, 1)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling.py needs the MI355X: there is nothing to time without it")
    if not a.skip_kernels:
        bench_kernels(a.iters)
    if not a.skip_engine:
        bench_engine()
