"""ELECTRA pre-training step, and the generator-head pass alone, fused against unfused.

Shape: the notebook's (Examples/electra-pretraining.ipynb): roberta-base width (d = 768, 12 heads, V = 50265), a 4-layer
generator and a 6-layer discriminator with RoPE, hidden dropout 0.1, one shared embedding table, B = 64 rows of 128
tokens, bf16 kernels with fp32 master weights under FlatTrainer.

  step      tr.train_step(lambda: model.electra_loss(ids, mask, tokenizer)[0]): device masking, generator, fused
            masked-LM loss + replaced-token sampling, discriminator, BCE head, backward, fused AdamW
  head pass the [B * L, V] bf16 generator logits with 15 % of the rows labelled, three routes over the SAME buffer:
    fused     vy_xent_sample_fused              loss, in-place gradient and the samples in one pass
    unfused   vy_xent_fwd, then the torch statements of the reference's sample() on the gathered labelled rows
              (zeros_like, uniform_, two logs, divide, add, argmax), then vy_xent_bwd
    plain     vy_xent_fused                     the same pass without the sampler (what a labelled row costs extra)
  and the fused / plain pair again with EVERY row labelled, for the cost of one live row with and without the sampler.

    python tools/bench_electra.py [--steps 10] [--warmup 3] [--rounds 3]

The routes alternate for `--rounds` rounds in ONE process; every timed call sits between a pair of events (the copy
that restores the logits before an in-place route is outside them), a round's figure is the median of its calls, a
route's figure the median of its rounds, the run-to-run spread the largest min-to-max range of the round medians of the
routes compared.  Ends with one JSON line; `ok` says: the fused head pass is faster than the unfused one by more than
that spread."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BF = torch.bfloat16


class Tokenizer:
    """What the collators ask of a tokenizer, with roberta-base's special ids."""
    all_special_ids = [0, 1, 2, 3, 50264]
    mask_token = "<mask>"
    pad_token_id = 1

    def __len__(self):
        return 50265

    def convert_tokens_to_ids(self, token):
        return 50264


def event_ms(fn, before=None):
    if before is not None:
        before()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def timed(fn, steps, warmup, before=None):
    for _ in range(warmup):
        event_ms(fn, before)
    return statistics.median(event_ms(fn, before)[0] for _ in range(steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--L", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_electra.py measures on an MI355X: no GPU found")
    import vyomai_amd as V
    from vyomai_amd import ops, rng
    from vyomai_amd.autograd_train import _row_stride
    from vyomai_amd.training import FlatTrainer
    dev = "cuda"
    tok = Tokenizer()
    torch.manual_seed(0)
    rng.manual_seed(0)
    gen_cfg, disc_cfg = V.EncoderConfig(num_hidden_layers=4), V.EncoderConfig(num_hidden_layers=6)
    model = V.ElectraModel(V.EncoderForMaskedLM(gen_cfg, pos_embedding_type="rope"), V.Discriminator(disc_cfg))
    model.tie_word_embeddings()
    model = model.cuda().train()
    tr = FlatTrainer(model, lr=1e-4, weight_decay=0.01)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(4, 50264, (a.B, a.L), generator=g)
    for i in range(a.B):                       # <s> ... </s> <pad>*: unequal lengths, right-padded
        n = int(torch.randint(a.L // 2, a.L + 1, (1,), generator=g))
        ids[i, 0], ids[i, n - 1], ids[i, n:] = 0, 2, 1
    ids = ids.cuda()
    mask = (ids != tok.pad_token_id).long()

    # ---- the head pass alone ----------------------------------------------------------------
    M, Vv = a.B * a.L, gen_cfg.vocab_size
    ld = _row_stride(Vv)
    pristine = torch.zeros((M, ld), dtype=BF, device=dev)
    pristine[:, :Vv] = (2.0 * torch.randn((M, Vv), device=dev)).to(BF)
    buf = pristine.clone()
    logits = buf[:, :Vv]
    lse = torch.empty(M, device=dev)
    sampled = torch.empty(M, dtype=torch.long, device=dev)
    one = torch.ones(1, device=dev)
    temperature = 3.0

    def head_routes(labels):
        live_idx = torch.nonzero(labels != -100).squeeze(1)          # precomputed: the route itself has no host sync
        count = torch.tensor([float(live_idx.numel())], device=dev)

        def fused():
            acc = torch.zeros(1, device=dev)
            ops.xent_sample_fused_(logits, labels, -100, lse, acc, count, one, sampled, 1.0 / temperature, 1, 2)

        def plain():
            acc = torch.zeros(1, device=dev)
            ops.xent_fused_(logits, labels, -100, lse, acc, count, one)

        def unfused():
            acc = torch.zeros(2, device=dev)
            ops.xent_fwd(logits, labels, -100, lse, acc[0:1], acc[1:2])
            rows = logits[live_idx]
            noise = torch.zeros_like(rows).uniform_(0, 1)
            noise = -torch.log(-torch.log(noise + 1e-9) + 1e-9)
            picked = ((rows / temperature) + noise).argmax(dim=-1)
            ops.xent_bwd_(logits, labels, -100, lse, one, acc[1:2])
            return picked
        return {"fused": fused, "unfused": unfused, "plain": plain}, live_idx.numel()

    labels15 = torch.full((M,), -100, dtype=torch.long, device=dev)
    pick = torch.rand(M, generator=g) < 0.15
    labels15[pick.cuda()] = torch.randint(0, Vv, (int(pick.sum()),), generator=g).cuda()
    labels_all = torch.randint(0, Vv, (M,), generator=g).cuda()
    routes15, n15 = head_routes(labels15)
    routes_all, _ = head_routes(labels_all)
    restore = lambda: buf.copy_(pristine)   # noqa: E731
    step = lambda: tr.train_step(lambda: model.electra_loss(ids, mask, tok)[0])   # noqa: E731

    rounds = {k: [] for k in ("step", "fused", "unfused", "plain", "fused_all", "plain_all")}
    for r in range(a.rounds):
        w = a.warmup if r == 0 else 1
        rounds["step"].append(timed(step, a.steps, w))
        for name, fn in routes15.items():
            rounds[name].append(timed(fn, a.steps, w, restore))
        for name in ("fused", "plain"):
            rounds[name + "_all"].append(timed(routes_all[name], a.steps, w, restore))
        print(f"round {r}: " + "  ".join(f"{k} {v[-1]:.3f} ms" for k, v in rounds.items()))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    spread = max(max(rounds[k]) - min(rounds[k]) for k in ("fused", "unfused"))
    ok = med["unfused"] - med["fused"] > spread
    row_us = {"sampled": 1e3 * med["fused_all"] / M, "plain": 1e3 * med["plain_all"] / M}
    print(f"ELECTRA step {med['step']:.2f} ms;  head pass ({n15} of {M} rows live): fused {med['fused']:.3f} ms, unfused "
          f"{med['unfused']:.3f} ms, plain vy_xent_fused {med['plain']:.3f} ms, spread of the A/B {spread:.3f} ms;  "
          f"one live row: {row_us['sampled']:.3f} us with the sampler, {row_us['plain']:.3f} us without")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "B": a.B, "L": a.L, "vocab": Vv, "live_rows": n15,
                      "ms": med, "round_medians_ms": rounds, "spread_ms": spread, "live_row_us": row_us, "ok": ok}))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
