"""Qwen3Model training on the MI355X, measured with device events after a warm-up, variants alternating inside one run:

  (a) vy_qknorm_rope_fwd and vy_qknorm_bwd at T = 16384 rows, h / hk / dh = 16 / 8 / 128, bf16: time and bytes/s from the
      algorithmic bytes, next to the copy rate of tools/bench_copy.py's kernel (vy_debug_copy) over as many bytes and to
      the torch composition of the same ops (forward, and autograd backward);
  (b) one full training step of the 0.6B shape (28 layers, vocabulary 151936, tied head, B x L = 8 x 2048) under
      FlatTrainer in bf16: ms / step, tokens / s, and the two kernels' share of it (their stand-alone times x layers).

    python tools/bench_qwen3_train.py [--layers 28] [--batch 8] [--seq 2048] [--iters 20] [--skip-step]

Prints one JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vyomai_amd as V  # noqa: E402
from vyomai_amd import _lib, ops  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
H, HK, DH, EPS = 16, 8, 128, 1e-6


def timed(fns, iters, warmup=3):
    """ms per call of each fn: warm-up, then `iters` rounds in which the variants alternate, each under its own events."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    total = [0.0] * len(fns)
    for _ in range(iters):
        for i, f in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            total[i] += s.elapsed_time(e)
    return [t / iters for t in total]


def torch_fwd(qkv, qs, ks, cos, sin, B, L):
    """The notebook's ops in torch: RMSNorm per head in fp32 rounded to bf16, rotate-half RoPE in bf16."""
    def norm(x, w):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS) * w).to(x.dtype)

    def rope(x):
        a, b = x[..., :DH // 2], x[..., DH // 2:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1)
    q = qkv[..., :H * DH].view(B, L, H, DH).transpose(1, 2)
    k = qkv[..., H * DH:(H + HK) * DH].view(B, L, HK, DH).transpose(1, 2)
    return rope(norm(q, qs)), rope(norm(k, ks))


def kernels(B, L, iters):
    T, W = B * L, (H + 2 * HK) * DH
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn((B, L, W), generator=g, device=DEV).to(BF)
    dq0 = torch.randn((B, L, W), generator=g, device=DEV).to(BF)
    qs, ks = (1 + 0.1 * torch.randn(DH, generator=g, device=DEV)).float(), (1 + 0.1 * torch.randn(DH, generator=g, device=DEV)).float()
    inv = 1.0 / (1e6 ** (torch.arange(0, DH, 2).float() / DH))
    ang = torch.outer(torch.arange(L).float(), inv)
    cos, sin = ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV)
    q = torch.empty((B, H, L, DH), dtype=BF, device=DEV)
    k = torch.empty((B, HK, L, DH), dtype=BF, device=DEV)
    dqs, dks = torch.zeros(DH, device=DEV), torch.zeros(DH, device=DEV)
    dbuf = dq0.clone()
    # algorithmic bytes: the forward reads the q | k columns of the packed rows (the v columns, a third of the row
    # width W here, are never touched) and writes q and k; the backward reads the q | k columns of both tensors and
    # writes the q | k columns of one
    qk_bytes = T * (H + HK) * DH * 2
    fwd_read, fwd_write, bwd_bytes = qk_bytes, qk_bytes, 3 * qk_bytes
    lib = _lib.load()
    lib.vy_debug_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    n_copy = bwd_bytes // 2
    src, dst = torch.zeros(n_copy, dtype=torch.uint8, device=DEV), torch.empty(n_copy, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    cb, sb = cos.to(BF), sin.to(BF)
    leaf = qkv.clone().requires_grad_(True)
    wq, wk = qs.clone().requires_grad_(True), ks.clone().requires_grad_(True)
    gq, gk = torch.randn_like(q), torch.randn_like(k)

    def t_fwd_bwd():
        leaf.grad = wq.grad = wk.grad = None
        a, b = torch_fwd(leaf, wq, wk, cb, sb, B, L)
        torch.autograd.backward([a, b], [gq, gk])

    fns = [lambda: ops.qknorm_rope(qkv, H, HK, DH, qs, ks, EPS, cos, sin, 0, q, k),
           lambda: ops.qknorm_bwd_(dbuf, qkv, H, HK, DH, qs, ks, EPS, dqs, dks, False),
           lambda: lib.vy_debug_copy(src.data_ptr(), dst.data_ptr(), n_copy, st),
           lambda: torch_fwd(qkv, qs, ks, cb, sb, B, L),
           t_fwd_bwd]
    with torch.no_grad():
        t = timed(fns[:4], iters)
    t += timed(fns[4:], iters)
    r = {"T": T, "fwd_ms": t[0], "bwd_ms": t[1], "copy_ms": t[2], "torch_fwd_ms": t[3], "torch_fwd_bwd_ms": t[4],
         "fwd_read_bytes": fwd_read, "fwd_write_bytes": fwd_write, "row_bytes": T * W * 2, "bwd_bytes": bwd_bytes,
         "fwd_TBps": (fwd_read + fwd_write) / t[0] * 1e-9, "bwd_TBps": bwd_bytes / t[1] * 1e-9,
         "copy_TBps": 2 * n_copy / t[2] * 1e-9}
    print(f"(a) T = {T}, h/hk/dh = {H}/{HK}/{DH}, bf16\n"
          f"    vy_qknorm_rope_fwd  {t[0] * 1e3:8.1f} us  reads {fwd_read / 1e6:.1f} MB (q | k columns), writes {fwd_write / 1e6:.1f} MB "
          f"-> {r['fwd_TBps']:.2f} TB/s\n"
          f"    vy_qknorm_bwd       {t[1] * 1e3:8.1f} us  moves {bwd_bytes / 1e6:.1f} MB -> {r['bwd_TBps']:.2f} TB/s (with its column-sum launch)\n"
          f"    copy of {2 * n_copy / 1e6:.1f} MB  {t[2] * 1e3:8.1f} us -> {r['copy_TBps']:.2f} TB/s (read + write)\n"
          f"    torch forward       {t[3] * 1e3:8.1f} us;  torch forward + autograd backward {t[4] * 1e3:8.1f} us")
    return r


def full_step(layers, B, L, iters):
    from vyomai_amd.training import FlatTrainer
    cfg = dict(vocab_size=151936, context_length=L, emb_dim=1024, n_heads=H, n_layers=layers, hidden_dim=3072, head_dim=DH,
               qk_norm=True, n_kv_groups=HK, rope_base=1e6, dtype=torch.float32)
    torch.manual_seed(0)
    m = V.Qwen3Model(cfg)
    m.tie_head()
    with torch.no_grad():
        m.tok_emb.weight.mul_(0.02)
    m = m.to(DEV).train()
    tr = FlatTrainer(m, lr=1e-5)
    ids = torch.randint(3, cfg["vocab_size"], (B, L), device=DEV)
    step = lambda: tr.train_step(lambda: m.clm_loss(ids, ids))  # noqa: E731
    ms = timed([step], iters, warmup=3)[0]
    loss = float(step().item())
    r = {"layers": layers, "B": B, "L": L, "step_ms": ms, "tokens_per_s": B * L / ms * 1e3, "loss": loss,
         "params": sum(p.numel() for p in m.parameters())}
    print(f"(b) {layers} layers, vocabulary {cfg['vocab_size']}, tied, B x L = {B} x {L}, FlatTrainer bf16: {ms:.1f} ms / step, "
          f"{r['tokens_per_s']:.0f} tokens / s (loss {loss:.3f}, {r['params'] / 1e6:.0f} M parameters)")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qwen3_train.py measures on the GPU; there is none here")
    out = {"kernels": kernels(a.batch, a.seq, a.iters)}
    if not a.skip_step:
        out["step"] = full_step(a.layers, a.batch, a.seq, max(3, a.iters // 4))
        share = (out["kernels"]["fwd_ms"] + out["kernels"]["bwd_ms"]) * a.layers / out["step"]["step_ms"]
        out["qknorm_share_of_step"] = share
        print(f"    the two kernels, stand-alone time x {a.layers} layers: {share * 100:.2f} % of the step")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
