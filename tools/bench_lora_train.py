"""One SFT step (clm_loss, AdamW through FlatTrainer) of the tools/bench_causal_lm.py model at that tool's shape -- d = 896,
14 heads over 2 KV heads, I = 4864, V = 32000, B = 32 x L = 512 tokens, bf16 kernels, fp32 masters -- full-weight and
with add_lora at rank 32 on all seven projections, and vy_lora_wgrad alone for the four GEMM groups of a layer.

    python tools/bench_lora_train.py [--layers 24] [--steps 10] [--warmup 3] [--rank 32] [--only full|lora]

Prints, and ends with one JSON line:
  * forward + backward + AdamW ms / step (median of the timed steps, with min and max) of the full-weight model and of
    the wrapped one, and their ratio; the two models are built, trained and freed one after the other;
  * per group (qkv, o, gate_up, down): us per vy_lora_wgrad call (median over batches of launches, with min and max),
    the bytes it has to move -- dY, x, u and t read once, the outputs written -- and that rate in GB/s.
No bar is fixed here; bench.py does not run this model: these numbers never appear in its result line."""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_causal_lm import BF, spread, time_batches  # noqa: E402
from vyomai_amd import ops  # noqa: E402


def step_ms(layers, steps, warmup, B, L, rank):
    """rank None: full-weight."""
    import vyomai_amd as V
    from vyomai_amd.training import FlatTrainer
    cfg = V.Config(vocab_size=32000, hidden_size=896, intermediate_size=4864, num_hidden_layers=layers,
                   num_attention_heads=14, num_key_value_heads=2, max_position_embeddings=max(L, 512))
    torch.manual_seed(0)
    m = V.ModelForCausalLM(cfg).cuda().train()
    if rank is not None:
        V.add_lora(m, rank=rank, alpha=1.0)
        with torch.no_grad():      # lora_b starts at zero: move it, so that every product of the backward is live
            for n, p in m.named_parameters():
                if n.endswith("lora_b"):
                    p.normal_(0.0, 0.02)
    tr = FlatTrainer(m, lr=1e-4, weight_decay=0.01)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (B, L), generator=g).cuda()
    torch.cuda.reset_peak_memory_stats()
    ms, loss = [], None
    for i in range(warmup + steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        loss = tr.train_step(lambda: m.clm_loss(ids, ids))
        e.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(s.elapsed_time(e))
    sp = spread(ms)
    what = "full-weight" if rank is None else f"LoRA rank {rank} on all seven projections"
    trainable = sum(p.numel() for p in m.parameters() if p.requires_grad)
    peak = torch.cuda.max_memory_allocated() / 2**30
    print(f"{what}: {layers} layers, {trainable / 1e6:.1f} M trainable parameters, B x L = {B} x {L}: {sp['median']:.2f} ms / "
          f"step (min {sp['min']:.2f} max {sp['max']:.2f}, n={sp['n']}), loss {loss.item():.4f}, peak memory {peak:.1f} GiB")
    out = {"layers": layers, "trainable": trainable, "B": B, "L": L, "ms_per_step": sp, "final_loss": loss.item(), "peak_GiB": peak}
    del tr, m
    gc.collect()
    torch.cuda.empty_cache()
    return out


def wgrad_alone(M, rank):
    d, I, kv = 896, 4864, 128
    r_pad = 32 if rank <= 32 else 64
    groups = {"qkv": (d, (d, kv, kv)), "o": (d, (d,)), "gate_up": (d, (I, I)), "down": (I, (d,))}
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).cuda()  # noqa: E731
    res = {}
    for name, (K, outs) in groups.items():
        N, R = sum(outs), len(outs) * r_pad
        bounds = tuple(sum(outs[:p]) for p in range(1, len(outs)))
        dy, x, u, t = r(M, N), r(M, K), r(M, R), r(M, R)
        dA = [torch.zeros(rank, K, device="cuda") for _ in outs]
        dB = [torch.zeros(o, rank, device="cuda") for o in outs]
        us = spread(time_batches(lambda: ops.lora_wgrad(dy, u, x, t, dA, dB, bounds, r_pad, 1.0, True, name=name)))
        nbytes = 2 * M * (N + K + 2 * R) + 4 * rank * (N + len(outs) * K)
        chunks = -(-M // ops.lora_wgrad_chunk_rows(M, N, K))
        res[name] = {"us": us, "bytes": nbytes, "GBps": nbytes / us["median"] * 1e-3, "chunks": chunks}
        print(f"vy_lora_wgrad {name:8s} M {M} N {N:5d} K {K:5d}: {us['median']:8.1f} us (min {us['min']:.1f} max {us['max']:.1f}, "
              f"n={us['n']})  {nbytes / 1e6:7.1f} MB  {res[name]['GBps']:7.0f} GB/s  {chunks} chunks of M")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--only", choices=("full", "lora"), help="one of the two models alone (under a profiler)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora_train.py measures on an MI355X: no GPU found")
    out = {"device": torch.cuda.get_device_name(0), "rank": a.rank}
    if a.only is None:
        out["wgrad"] = wgrad_alone(a.B * a.L, a.rank)
    if a.only != "lora":
        out["full"] = step_ms(a.layers, a.steps, a.warmup, a.B, a.L, None)
    if a.only != "full":
        out["lora"] = step_ms(a.layers, a.steps, a.warmup, a.B, a.L, a.rank)
    if a.only is None:
        out["lora_over_full"] = out["lora"]["ms_per_step"]["median"] / out["full"]["ms_per_step"]["median"]
        print(f"LoRA step / full-weight step: {out['lora_over_full']:.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
