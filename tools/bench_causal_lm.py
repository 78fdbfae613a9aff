"""Training step and streaming-kernel rates of the RMSNorm + SwiGLU causal LM (models/custom_transformer.py) at the
Qwen2-0.5B widths: d = 896, 14 heads over 2 KV heads, I = 4864, V = 32000, B = 32 x L = 512 tokens, bf16 kernels with
fp32 master weights under FlatTrainer.

    python tools/bench_causal_lm.py [--layers 24] [--steps 10] [--warmup 3]

Prints, and ends with one JSON line:
  * forward + backward + AdamW ms / step (median of the timed steps, with min and max) and tokens / s;
  * per kernel (vy_rmsnorm_bwd with and without add_to, vy_gated_act_fwd, vy_gated_act_bwd at 16384 rows): us per call
    (median over batches of launches, with min and max), the bytes the algorithm moves over that time, and that rate as
    a share of the copy rate measured by the probe of tools/bench_copy.py (vy_debug_copy, 1 GiB read + 1 GiB write) in
    THIS process.  The RMSNorm operands (29 MB each) fit the 256 MB Infinity Cache between launches, the gated MLP's
    (160 MB each) do not: a share above 1 for the former is the cache, not an error.
bench.py does not run this model: these numbers never appear in its result line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vyomai_amd import _lib, ops  # noqa: E402

BF = torch.bfloat16


def spread(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "n": len(samples)}


def time_batches(fn, inner=20, batches=9, warm=5):
    """us per call: `batches` samples, each the device time of `inner` back-to-back launches."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / inner * 1e3)
    return out


def copy_rate():
    """GB/s (read + write) of the library's copy probe, as tools/bench_copy.py measures it."""
    lib = _lib.load()
    lib.vy_debug_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    n = 1 << 30
    a = torch.zeros(n, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    st = torch.cuda.current_stream().cuda_stream
    us = time_batches(lambda: lib.vy_debug_copy(a.data_ptr(), b.data_ptr(), n, st), inner=10, batches=5, warm=3)
    return {k: (2 * n / v * 1e-3 if k != "n" else v) for k, v in spread(us).items()}, us


def kernels(M, N, I, copy_gbs):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).cuda()  # noqa: E731
    x, dy, add, w = r(M, N), r(M, N), r(M, N), r(N)
    dw = torch.zeros(N, dtype=torch.float32, device="cuda")
    gu, da = r(M, 2 * I), r(M, I)
    rows = [
        ("rmsnorm_bwd", 3 * M * N * 2, lambda: ops.rmsnorm_bwd(dy, x, w, 1e-6, 0.0, dw, True)),
        ("rmsnorm_bwd+add_to", 4 * M * N * 2, lambda: ops.rmsnorm_bwd(dy, x, w, 1e-6, 0.0, dw, True, add_to=add)),
        ("gated_act_fwd(silu)", 3 * M * I * 2, lambda: ops.gated_act(gu, _lib.ACT_SILU)),
        ("gated_act_bwd(silu)", 5 * M * I * 2, lambda: ops.gated_act_bwd(da, gu, _lib.ACT_SILU)),
    ]
    res = {}
    for name, nbytes, fn in rows:
        us = spread(time_batches(fn))
        gbs = nbytes / us["median"] * 1e-3
        res[name] = {"us": us, "bytes": nbytes, "GBps": gbs, "share_of_copy": gbs / copy_gbs}
        print(f"{name:22s} {us['median']:8.1f} us (min {us['min']:.1f} max {us['max']:.1f}, n={us['n']})  "
              f"{nbytes / 1e6:7.1f} MB  {gbs:7.0f} GB/s  {gbs / copy_gbs:5.2f} x copy")
    return res


def train(layers, steps, warmup, B, L):
    import vyomai_amd as V
    from vyomai_amd.training import FlatTrainer
    cfg = V.Config(vocab_size=32000, hidden_size=896, intermediate_size=4864, num_hidden_layers=layers,
                   num_attention_heads=14, num_key_value_heads=2, max_position_embeddings=max(L, 512))
    torch.manual_seed(0)
    m = V.ModelForCausalLM(cfg).cuda().train()
    tr = FlatTrainer(m, lr=1e-4, weight_decay=0.01)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (B, L), generator=g).cuda()
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
    nparam = sum(p.numel() for p in m.parameters())
    print(f"{layers} layers, {nparam / 1e6:.0f} M parameters, B x L = {B} x {L}: {sp['median']:.2f} ms / step "
          f"(min {sp['min']:.2f} max {sp['max']:.2f}, n={sp['n']}), {B * L / sp['median'] * 1e3:.0f} tokens / s, "
          f"loss {loss.item():.4f}, peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    return {"layers": layers, "parameters": nparam, "B": B, "L": L, "ms_per_step": sp,
            "tokens_per_s": B * L / sp["median"] * 1e3, "final_loss": loss.item(),
            "peak_GiB": torch.cuda.max_memory_allocated() / 2**30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)   # Qwen2-0.5B's depth: 24 layers fit beside B = 32 x 512 in bf16
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_causal_lm.py measures on an MI355X: no GPU found")
    cr, _ = copy_rate()
    print(f"copy probe: {cr['median']:.0f} GB/s read + write (min {cr['max']:.0f} max {cr['min']:.0f})")
    out = {"device": torch.cuda.get_device_name(0), "copy_GBps": cr["median"]}
    out["kernels"] = kernels(a.B * a.L, 896, 4864, cr["median"])
    if not a.skip_train:
        out["train"] = train(a.layers, a.steps, a.warmup, a.B, a.L)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
