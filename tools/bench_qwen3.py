"""Qwen3Model serving: what the fused qk-norm costs, and the engine on the notebook's 0.6B shape.
python tools/bench_qwen3.py [--iters 1000] [--skip-engine] [--skip-kernel]

(a) vy_paged_qknorm_rope_write against vy_paged_rope_write ALONE on the same buffers (bf16, h / hk / dh = 16 / 8 / 128,
    block_size 256, T = 8, 64 and 4096 tokens): the second kernel is the parent's, it does not normalise, so the ratio is
    the price of the norm inside the launch, not a comparison of two ways to do the same work.  Each is timed as a link
    of a captured chain of 50 calls, the two chains replayed in turn (tools/bench_paged.py, timed_graph); the whole
    measurement is repeated and the lowest and highest figure of each are printed.  bytes = the q, k, v rows read, the
    q, k rows written in place and the k, v rows written to the pages.
(b) ContinuousBatchEngine on Qwen3Model with the notebook's 0.6B cfg (28 layers, emb 1024, hidden 3072, vocabulary
    151936, 16 / 8 heads of 128, qk_norm, block_size 256) and random bf16 weights: six prompts of mixed lengths,
    requested tokens per second, lowest and highest of the repeats.
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
from bench_paged import timed_graph  # noqa: E402
from vyomai_amd import ops  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
QWEN3_06B = {"vocab_size": 151_936, "context_length": 40_960, "emb_dim": 1024, "n_heads": 16, "n_layers": 28,
             "hidden_dim": 3072, "head_dim": 128, "qk_norm": True, "n_kv_groups": 8, "rope_base": 1_000_000.0,
             "dtype": BF}


def bench_kernel(iters, repeats=3):
    h, hk, dh, bs = 16, 8, 128, 256
    for T in (8, 64, 4096):
        g = torch.Generator().manual_seed(T)
        nblk = (T + bs - 1) // bs + 1
        qkv = torch.randn(T, (h + 2 * hk) * dh, generator=g).to(BF).to(DEV)
        pos = torch.arange(T, dtype=torch.int32, device=DEV)
        slots = torch.randperm(nblk * bs, generator=g)[:T].to(DEV)
        inv = 1.0 / (1e6 ** (torch.arange(0, dh, 2).float() / dh))
        ang = torch.outer(torch.arange(max(T, 256)).float(), inv)
        cos, sin = ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV)
        qs = (1.0 + 0.1 * torch.rand(dh, generator=g)).to(DEV)
        ks = (1.0 + 0.1 * torch.rand(dh, generator=g)).to(DEV)
        kc = torch.zeros(nblk, bs, hk, dh, dtype=BF, device=DEV)
        vc = torch.zeros_like(kc)
        a, b = qkv.clone(), qkv.clone()          # each chain rewrites its own buffer in place

        def fused():
            ops.paged_qknorm_rope_write_(a, pos, slots, cos, sin, qs, ks, 1e-6, h, kc, vc)

        def plain():
            ops.paged_rope_write_(b, pos, slots, cos, sin, h, kc, vc)

        runs = [timed_graph([fused, plain], 5, iters) for _ in range(repeats)]
        tf, tp = [r[0] for r in runs], [r[1] for r in runs]
        nbytes = 2 * T * dh * ((h + 2 * hk) + (h + hk) + 2 * hk)
        print(json.dumps({"what": "qk-norm + rope + page write against rope + page write alone", "T": T, "h": h, "hk": hk,
                          "dh": dh, "fused_us": [round(min(tf), 2), round(max(tf), 2)],
                          "rope_write_us": [round(min(tp), 2), round(max(tp), 2)],
                          "fused_GBs": round(nbytes / min(tf) * 1e-3, 1), "rope_write_GBs": round(nbytes / min(tp) * 1e-3, 1),
                          "ratio": round(min(tf) / min(tp), 3)}))


def bench_engine(repeats=3):
    torch.manual_seed(0)
    with torch.device(DEV):
        m = V.Qwen3Model(QWEN3_06B).eval()
    g = torch.Generator().manual_seed(1)
    plen, glen = [12, 40, 96, 24, 160, 64], [64, 32, 128, 16, 96, 48]
    prompts = [torch.randint(3, QWEN3_06B["vocab_size"], (n,), generator=g).tolist() for n in plen]

    def run():
        mgr = V.PagedKVManager(m.config, 32, 256, DEV, BF)
        eng = V.ContinuousBatchEngine(m, mgr, max_batch_size=8, eos_token_ids=[])
        for p, n in zip(prompts, glen):
            eng.add_sequence(p, max_gen_len=n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run()                                 # (every step ends with the device-to-host copy of its ids)
        return time.perf_counter() - t0

    run()                                         # warm-up: every shape of the run
    dts = [run() for _ in range(repeats)]
    print(json.dumps({"what": "engine, Qwen3 0.6B cfg, random bf16 weights", "requests": len(prompts),
                      "requested_tokens": sum(glen), "seconds": [round(min(dts), 4), round(max(dts), 4)],
                      "requested_tokens_per_s": [round(sum(glen) / max(dts), 1), round(sum(glen) / min(dts), 1)]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qwen3.py needs the MI355X: there is nothing to time without it")
    if not a.skip_kernel:
        bench_kernel(a.iters)
    if not a.skip_engine:
        bench_engine()
