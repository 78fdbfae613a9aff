"""One classification fine-tuning step (classification_loss, AdamW through FlatTrainer) of the encoder of
Examples/adapters.ipynb -- 12 layers, d = 768, 12 heads, B x L = 64 x 128 (the notebook's batch), 151 classes, bf16
kernels, fp32 masters -- with add_lora at rank 32 on the notebook's five targets and full-weight, and vy_lora_expand_epi
alone in both modes beside the three-launch composition it replaces and a copy of as many bytes.

    python tools/bench_encoder_lora.py [--layers 12] [--steps 10] [--warmup 3] [--rank 32] [--only full|lora|kernels]

Prints, and ends with one JSON line:
  * forward + backward + AdamW ms / step (median of the timed steps, with min and max) of the wrapped classifier and of
    the full-weight one, and their ratio; the two models are built, trained and freed one after the other;
  * per epilogue (ACT over M x 4d, DROP_RES over M x d, M = B L): us per vy_lora_expand_epi call, us of the composition
    (vy_lora_expand in place, then the activation / dropout pass and the add as launches of their own), and us of a
    device copy of the bytes the fused call has to move (z and the residual read, the outputs written).
No bar is fixed here; bench.py does not run this model: these numbers never appear in its result line."""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_causal_lm import BF, spread, time_batches  # noqa: E402
from vyomai_amd import _lib, ops  # noqa: E402

CLASSES = 151


def step_ms(layers, steps, warmup, B, L, rank):
    """rank None: full-weight."""
    import vyomai_amd as V
    from vyomai_amd.training import FlatTrainer
    cfg = V.EncoderConfig(num_hidden_layers=layers)
    torch.manual_seed(0)
    m = V.EncoderForSequenceClassification(cfg, CLASSES).cuda().train()
    if rank is not None:
        V.add_lora(m.model, rank=rank, alpha=1.0)
        with torch.no_grad():      # lora_b starts at zero: move it, so that every product of the backward is live
            for n, p in m.named_parameters():
                if n.endswith("lora_b"):
                    p.normal_(0.0, 0.02)
    tr = FlatTrainer(m, lr=1e-4, weight_decay=0.01)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (B, L), generator=g).cuda()
    mask = torch.ones(B, L, dtype=torch.long).cuda()
    labels = torch.randint(0, CLASSES, (B,), generator=g).cuda()
    torch.cuda.reset_peak_memory_stats()
    ms, loss = [], None
    for i in range(warmup + steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        loss = tr.train_step(lambda: m.classification_loss(ids, mask, labels))
        e.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(s.elapsed_time(e))
    sp = spread(ms)
    what = "full-weight" if rank is None else f"LoRA rank {rank} on the notebook's five targets"
    trainable = sum(p.numel() for p in m.parameters() if p.requires_grad)
    peak = torch.cuda.max_memory_allocated() / 2**30
    print(f"{what}: {layers} layers, {trainable / 1e6:.2f} M trainable parameters, B x L = {B} x {L}, dropout "
          f"{cfg.hidden_dropout_prob}: {sp['median']:.2f} ms / step (min {sp['min']:.2f} max {sp['max']:.2f}, n={sp['n']}), "
          f"loss {loss.item():.4f}, peak memory {peak:.1f} GiB")
    out = {"layers": layers, "trainable": trainable, "B": B, "L": L, "ms_per_step": sp, "final_loss": loss.item(), "peak_GiB": peak}
    del tr, m
    gc.collect()
    torch.cuda.empty_cache()
    return out


def kernels_alone(M, rank, d=768):
    from vyomai_amd.lora_train import identity_tiles
    r_pad = 32 if rank <= 32 else 64
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).cuda()  # noqa: E731
    host = identity_tiles(M)
    tiles, n = host.cuda(), host.shape[0]
    al = torch.ones(1, dtype=torch.float32, device="cuda")
    drop = (0.1, 1234, 1)
    res = {}
    for name, N in (("ACT", 4 * d), ("DROP_RES", d)):
        z, u, B, other = r(M, N), r(M, r_pad), r(1, N, r_pad), r(M, N)
        pre, tmp = torch.empty_like(z), torch.empty_like(z)
        if name == "ACT":
            fused = lambda: ops.lora_expand_epi_(z, u, B, al, tiles, n, act=_lib.ACT_GELU_ERF, pre=pre, out=tmp)  # noqa: E731

            # the existing elementwise launches: vy_gated_act_fwd over [z | 1] is act(z), vy_act_bwd of 1 is act'(z)
            zu = torch.cat([z, torch.ones_like(z)], dim=-1).contiguous()
            ones = torch.ones_like(z)

            def composed():
                call_expand(zu[:, :N], u, B, al, tiles, n, N, r_pad)
                ops.gated_act(zu, _lib.ACT_GELU_ERF)
                ops.act_bwd(ones, zu[:, :N], _lib.ACT_GELU_ERF)
            nbytes = 2 * M * N * 3 + 2 * M * r_pad                   # z read; out, pre written; u read
        else:
            fused = lambda: ops.lora_expand_epi_(z, u, B, al, tiles, n, residual=other, dropout=drop, out=tmp)  # noqa: E731

            def composed():
                call_expand(z, u, B, al, tiles, n, N, r_pad)
                y = ops.dropout(z, *drop, out=tmp)
                y.add_(other)                                         # (the add as a launch of its own)
            nbytes = 2 * M * N * 3 + 2 * M * r_pad                   # z, residual read; out written; u read
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t_f = spread(time_batches(fused))
        t_c = spread(time_batches(composed))
        t_copy = spread(time_batches(lambda: dst.copy_(src)))
        print(f"vy_lora_expand_epi {name}: M = {M}, N = {N}, r_pad = {r_pad}: fused {t_f['median']:.1f} us, composition "
              f"{t_c['median']:.1f} us ({t_c['median'] / t_f['median']:.2f} x), copy of {nbytes / 1e6:.1f} MB "
              f"{t_copy['median']:.1f} us")
        res[name] = {"M": M, "N": N, "r_pad": r_pad, "fused_us": t_f, "composed_us": t_c, "copy_us": t_copy, "bytes": nbytes}
    return res


def call_expand(z, u, B, al, tiles, n, N, r_pad):
    _lib.call("vy_lora_expand", z.data_ptr(), z.stride(0), u.data_ptr(), u.stride(0), B.data_ptr(), al.data_ptr(),
              tiles.data_ptr(), n, z.shape[0], N, r_pad, 1, N, N, _lib.dtype_code(z.dtype), ops._stream())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--only", choices=["full", "lora", "kernels"], default=None)
    a = ap.parse_args()
    out = {"tool": "bench_encoder_lora"}
    if a.only in (None, "lora"):
        out["lora"] = step_ms(a.layers, a.steps, a.warmup, a.batch, a.seq, a.rank)
    if a.only in (None, "full"):
        out["full"] = step_ms(a.layers, a.steps, a.warmup, a.batch, a.seq, None)
    if "lora" in out and "full" in out:
        out["lora_over_full"] = out["lora"]["ms_per_step"]["median"] / out["full"]["ms_per_step"]["median"]
        print(f"LoRA step / full-weight step = {out['lora_over_full']:.3f}")
    if a.only in (None, "kernels"):
        out["kernels"] = kernels_alone(a.batch * a.seq, a.rank)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
