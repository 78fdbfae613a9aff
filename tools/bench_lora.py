"""Per-request LoRA: the vy_lora_shrink + vy_lora_expand pair against its torch restatement, and the serving engine
without a store, with a store and only base requests, and with every request on one of 4 adapters.
    python tools/bench_lora.py [--iters 1000] [--skip-engine] [--skip-kernels]

Kernels (bf16, the widths of tools/bench_paged.py's model: d = 896, intermediate 4864, 4 heads / 2 KV heads of 224;
rank 32), for each of the four projection groups of a layer (qkv and gate_up packed):
  decode   8 rows, each a tile of its own, 8 slots
  prefill  512 rows, 32 tiles of 16, 2 slots (256 rows each)
  (a) ops.lora_delta_: two launches whatever the number of adapters
  (b) torch: per adapter index_select, per part two matmuls, index_add_ (2 + 3 * parts launches an adapter)
Each is timed as a link of a captured chain of 50 calls, the chains replayed in turn (tools/bench_paged.py's
timed_graph), and eagerly with device events (tools/bench_sampling.py's timed_eager: these figures carry the host's
launch cost).  The whole measurement is repeated three times; figures are lowest .. highest.  Bytes are computed from
the shapes: (a) reads x, the adapters' A and B rows once per tile, u twice, and reads and writes y.

Engine: the workload of tools/bench_paged.py (6 requests of mixed lengths, 384 requested tokens, varlen_prefill), the
three engines alternating in one call: seconds per run lowest / median / highest and tokens/s at the median.  The
engine without a store is the engine as it was before adapters existed: the all-base run under adapters= issues the
same launches (tests/test_lora_engine_gpu.py pins the sequence of names).
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
D, I, R_PAD = 896, 4864, 32
# group -> (K, part widths)
GROUPS = {"qkv": (D, (896, 448, 448)), "o": (D, (D,)), "gate_up": (D, (I, I)), "down": (I, (D,))}
PHASES = {"decode": (8, 8, [(t, 1, t) for t in range(8)]),
          "prefill": (512, 2, [(r, 16, (r // 256) % 2) for r in range(0, 512, 16)])}


def torch_delta_(y, x, A, B, alpha, rows_of, widths):
    """The restatement: per adapter index_select, per part two matmuls, index_add_."""
    for s, idx in rows_of.items():
        xs = x.index_select(0, idx)
        c = 0
        for p, w in enumerate(widths):
            u = xs @ A[s, p * R_PAD:(p + 1) * R_PAD].t()
            y[:, c:c + w].index_add_(0, idx, (u @ B[s, c:c + w].t()) * alpha[s])
            c += w
    return y


def bench_kernels(iters, repeats=3):
    for phase, (T, slots, tiles) in PHASES.items():
        for group, (K, widths) in GROUPS.items():
            g = torch.Generator().manual_seed(T + K)
            N, parts = sum(widths), len(widths)
            x = torch.randn(T, K, generator=g).to(BF).to(DEV)
            y = torch.randn(T, N, generator=g).to(BF).to(DEV)
            A = (torch.randn(slots, parts * R_PAD, K, generator=g) / K ** 0.5).to(BF).to(DEV)
            B = (torch.randn(slots, N, R_PAD, generator=g) / R_PAD ** 0.5).to(BF).to(DEV)
            alpha = torch.full((slots,), 1e-3, device=DEV)        # (small: y stays finite over thousands of additions)
            tl = torch.tensor(tiles, dtype=torch.int32, device=DEV)
            bounds = tuple(sum(widths[:k]) for k in range(1, parts))
            rows_of = {}
            for row0, n, s in tiles:
                rows_of.setdefault(s, []).extend(range(row0, row0 + n))
            rows_of = {s: torch.tensor(r, device=DEV) for s, r in rows_of.items()}
            alpha_l = alpha.tolist()
            fns = [lambda: ops.lora_delta_(y, x, A, B, alpha, tl, len(tiles), bounds),
                   lambda: torch_delta_(y, x, A, B, alpha_l, rows_of, widths)]
            runs_g = [timed_graph(fns, 5, iters) for _ in range(repeats)]
            runs_e = [timed_eager(fns) for _ in range(repeats)]
            es = 2
            read = es * (T * K + len(tiles) * (parts * R_PAD * K + N * R_PAD) + 2 * T * parts * R_PAD + T * N)
            for i, name in enumerate(("a vy_lora_shrink + vy_lora_expand", "b torch per adapter")):
                tg, te = [r[i] for r in runs_g], [r[i] for r in runs_e]
                rec = {"what": "lora delta", "phase": phase, "group": group, "rows": T, "tiles": len(tiles), "slots": slots,
                       "K": K, "N": N, "variant": name, "chain_us": [round(min(tg), 2), round(max(tg), 2)],
                       "eager_us": [round(min(te), 2), round(max(te), 2)]}
                if i == 0:
                    rec.update(read_bytes=read, write_bytes=es * (T * parts * R_PAD + T * N))
                print(json.dumps(rec), flush=True)


def bench_engine(rounds=5):
    cfg = V.Config(vocab_size=32000, hidden_size=896, intermediate_size=4864, num_hidden_layers=4,
                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=1024, pad_token_id=0)
    torch.manual_seed(0)
    m = V.ModelForCausalLM(cfg).to(BF).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    plen, glen = [12, 40, 96, 24, 160, 64], [64, 32, 128, 16, 96, 48]
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in plen]
    store = V.LoraAdapters(m, 4, max_rank=32)
    paths = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
             "mlp.up_proj", "mlp.down_proj")
    for k in range(4):
        sd = {}
        for l, layer in enumerate(m.model.layers):
            for path in paths:
                out_f, in_f = dict(layer.named_modules())[path].weight.shape
                sd[f"model.layers.{l}.{path}.lora_a"] = torch.randn(32, in_f, generator=g) * 0.02
                sd[f"model.layers.{l}.{path}.lora_b"] = torch.randn(out_f, 32, generator=g) * 0.02
        store.load(f"a{k}", sd)

    def run(mode):
        mgr = V.PagedKVManager(cfg, 64, 16, DEV, BF)
        kw = {} if mode == "no store" else {"adapters": store}
        eng = V.ContinuousBatchEngine(m, mgr, max_batch_size=8, eos_token_ids=[], varlen_prefill=True, **kw)
        for i, (p, n) in enumerate(zip(prompts, glen)):
            if mode == "4 adapters":
                eng.add_sequence(p, max_gen_len=n, adapter=f"a{i % 4}")
            else:
                eng.add_sequence(p, max_gen_len=n)
        steps = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while eng.active or eng.waiting_room:
            eng.step()
            steps += 1
        return time.perf_counter() - t0, steps

    modes = ("no store", "store, all base", "4 adapters")
    for mode in modes:                         # warm-up: every shape of every run
        run(mode)
    res = {mode: [] for mode in modes}
    for _ in range(rounds):
        for mode in modes:
            res[mode].append(run(mode))
    tokens = sum(glen)
    for mode in modes:
        t = sorted(r[0] for r in res[mode])
        med = t[len(t) // 2]
        print(json.dumps({"what": "engine", "mode": mode, "requests": len(prompts), "requested_tokens": tokens,
                          "steps": res[mode][0][1], "rounds": rounds,
                          "seconds": [round(t[0], 4), round(med, 4), round(t[-1], 4)],
                          "tokens_per_s_median": round(tokens / med, 1)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora.py needs the MI355X: there is nothing to time without it")
    if not a.skip_kernels:
        bench_kernels(a.iters)
    if not a.skip_engine:
        bench_engine()
