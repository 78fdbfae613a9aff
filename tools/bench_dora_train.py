"""One SFT step (clm_loss, AdamW through FlatTrainer) of the tools/bench_lora_train.py model at that tool's shape -- d = 896,
14 heads over 2 KV heads, I = 4864, V = 32000, B = 32 x L = 512 tokens, bf16 kernels, fp32 masters -- full-weight, with
add_lora and with add_dora at rank 32 on all seven projections, in one process; and DoRA's two kernels alone.

    python tools/bench_dora_train.py [--layers 24] [--steps 10] [--warmup 3] [--rank 32] [--only full|lora|dora|kernels]

Prints, and ends with one JSON line:
  * forward + backward + AdamW ms / step (median of the timed steps, with min and max) and peak memory of the three
    models, built, trained and freed one after the other, and the LoRA and DoRA steps over the full-weight one;
  * per layer (one table of seven problems, fp32 master W, bf16 W'): us per ops.dora_compose and per ops.dora_bwd call
    (median over batches of launches, with min and max), the bytes each has to move once -- compose: W, a, b, m in, W'
    and c out; backward: G, W, a, b, m, c in, dm, da, db out -- that rate in GB/s, and a torch copy that moves as many
    bytes;
  * the same compose and backward of a layer written in torch ops (fp32, autograd), for the launch-count comparison.
The yardstick is the full-weight step of the same process: the DoRA step is expected to be that plus the two kernels.
No bar is fixed here; bench.py does not run this model: these numbers never appear in its result line."""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_causal_lm import spread, time_batches  # noqa: E402
from vyomai_amd import ops  # noqa: E402

KINDS = {"full": "full-weight", "lora": "LoRA", "dora": "DoRA"}


def step_ms(kind, layers, steps, warmup, B, L, rank):
    import vyomai_amd as V
    from vyomai_amd.training import FlatTrainer
    cfg = V.Config(vocab_size=32000, hidden_size=896, intermediate_size=4864, num_hidden_layers=layers,
                   num_attention_heads=14, num_key_value_heads=2, max_position_embeddings=max(L, 512))
    torch.manual_seed(0)
    m = V.ModelForCausalLM(cfg).cuda().train()
    if kind == "lora":
        V.add_lora(m, rank=rank, alpha=1.0)
    elif kind == "dora":
        V.add_dora(m, rank=rank)
    with torch.no_grad():      # lora_b / dora_b start at zero: move them, so that every product of the backward is live
        for n, p in m.named_parameters():
            if n.endswith(("lora_b", "dora_b")):
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
    what = KINDS[kind] + ("" if kind == "full" else f" rank {rank} on all seven projections")
    trainable = sum(p.numel() for p in m.parameters() if p.requires_grad)
    peak = torch.cuda.max_memory_allocated() / 2**30
    print(f"{what}: {layers} layers, {trainable / 1e6:.1f} M trainable parameters, B x L = {B} x {L}: {sp['median']:.2f} ms / "
          f"step (min {sp['min']:.2f} max {sp['max']:.2f}, n={sp['n']}), loss {loss.item():.4f}, peak memory {peak:.1f} GiB")
    out = {"layers": layers, "trainable": trainable, "B": B, "L": L, "ms_per_step": sp, "final_loss": loss.item(), "peak_GiB": peak}
    del tr, m
    gc.collect()
    torch.cuda.empty_cache()
    return out


def layer_table(rank):
    """The seven projections of one layer as ops.DoraProblem (packed destinations as dora_train.py lays them out)."""
    d, I, kv = 896, 4864, 128
    groups = [(d, (d, kv, kv)), (d, (d,)), (d, (I, I)), (I, (d,))]
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    problems = []
    for K, outs in groups:
        packed = torch.empty((sum(outs), K), dtype=torch.bfloat16, device="cuda")
        row = 0
        for o in outs:
            w = r(o, K) * 0.02
            problems.append(ops.DoraProblem(w=w, a=r(o, rank) * rank ** -0.5, b=r(rank, K) * 0.02, m=w.norm(dim=0), c=z(K),
                                            wp=packed[row:row + o], g=r(o, K), dm=z(K), da=z(o, rank), db=z(rank, K)))
            row += o
    return problems


def torch_compose_and_backward(problems):
    """The same arithmetic of one layer in torch ops: forward to a bf16 W', backward from G through autograd."""
    leaves = [[t.clone().requires_grad_(True) for t in (p.a, p.b, p.m)] for p in problems]

    def run():
        for p, (a, b, m) in zip(problems, leaves):
            D = p.w + a @ b
            wp = (m * (D / D.norm(p=2, dim=0, keepdim=True))).to(torch.bfloat16)
            torch.autograd.grad(wp, (a, b, m), p.g.to(torch.bfloat16))
    return run


def kernels_alone(rank):
    problems = layer_table(rank)
    elems = sum(p.w.numel() for p in problems)
    small = sum(p.a.numel() + p.b.numel() + p.m.numel() for p in problems)
    cols = sum(p.m.numel() for p in problems)
    nbytes = {"compose": 4 * elems + 4 * small + 2 * elems + 4 * cols,
              "bwd": 4 * elems + 4 * elems + 4 * small + 4 * cols + 4 * small}
    fns = {"compose": lambda: ops.dora_compose(problems), "bwd": lambda: ops.dora_bwd(problems, True)}
    res = {}
    ops.dora_compose(problems)
    for name, fn in fns.items():
        us = spread(time_batches(fn))
        src = torch.zeros(nbytes[name] // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        cp = spread(time_batches(lambda: dst.copy_(src)))
        res[name] = {"us": us, "bytes": nbytes[name], "GBps": nbytes[name] / us["median"] * 1e-3, "copy_us": cp,
                     "copy_GBps": nbytes[name] / cp["median"] * 1e-3}
        print(f"vy_dora_{name:7s} one layer, rank {rank}: {us['median']:8.1f} us (min {us['min']:.1f} max {us['max']:.1f}, "
              f"n={us['n']})  {nbytes[name] / 1e6:6.1f} MB  {res[name]['GBps']:6.0f} GB/s; a copy of as many bytes: "
              f"{cp['median']:.1f} us, {res[name]['copy_GBps']:.0f} GB/s")
    us = spread(time_batches(torch_compose_and_backward(problems), inner=5, batches=5, warm=2))
    res["torch_ops"] = {"us": us}
    both = res["compose"]["us"]["median"] + res["bwd"]["us"]["median"]
    print(f"the same compose + backward in torch ops: {us['median']:.1f} us a layer (min {us['min']:.1f} max {us['max']:.1f}) "
          f"against {both:.1f} us for the two kernels (three launches)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--only", choices=tuple(KINDS) + ("kernels",), help="one part alone (under a profiler)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dora_train.py measures on an MI355X: no GPU found")
    out = {"device": torch.cuda.get_device_name(0), "rank": a.rank}
    if a.only in (None, "kernels"):
        out["kernels"] = kernels_alone(a.rank)
    for kind in KINDS:
        if a.only in (None, kind):
            out[kind] = step_ms(kind, a.layers, a.steps, a.warmup, a.B, a.L, a.rank)
    if a.only is None:
        full = out["full"]["ms_per_step"]["median"]
        for kind in ("lora", "dora"):
            out[f"{kind}_over_full"] = out[kind]["ms_per_step"]["median"] / full
        k = out["kernels"]
        out["dora_kernels_ms_per_step"] = (k["compose"]["us"]["median"] + k["bwd"]["us"]["median"]) * a.layers * 1e-3
        print(f"LoRA step / full-weight step: {out['lora_over_full']:.3f}; DoRA step / full-weight step: "
              f"{out['dora_over_full']:.3f}; DoRA's two kernels over {a.layers} layers: {out['dora_kernels_ms_per_step']:.2f} ms")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
