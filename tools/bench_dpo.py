"""DPO step of ModelForCausalLM, fused against the only route the package offered before dpo_loss existed.

Shape: 8 pairs x 512 tokens, the default Config (d = 896, 4 layers, V = 32000), bf16 kernels with fp32 master weights
under FlatTrainer; the frozen model is a second ModelForCausalLM in bf16.  One step = score the frozen model on the 2B
concatenated rows under no_grad, policy forward + backward, fused AdamW (FlatTrainer.train_step).

  fused     model.dpo_loss(batch, ref)           vy_logprob_fwd (frozen) / vy_logprob_fused (policy): no logits kept
  baseline  model(input_ids).logits, then torch log_softmax + gather + masked mean, as the notebook's
            compute_logprobs spells it, on the same concatenated batch, same trainer, same tail

    python tools/bench_dpo.py [--steps 10] [--warmup 3] [--rounds 3]

The two routes alternate for `--rounds` rounds in ONE process; every step is timed with a pair of events around it, a
round's figure is the median of its steps, a route's figure the median of its rounds, and the run-to-run spread is the
largest min-to-max range of the round medians of either route.  Peak memory is torch.cuda.max_memory_allocated over a
route's timed steps (reset before them).  Ends with one JSON line; `ok` says: fused not slower than the baseline beyond
that spread, and its peak memory lower."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BF = torch.bfloat16


def logits_route(model, ref, batch, beta):
    """What a user could write before: materialised logits, torch log_softmax / gather, one 2B-row batch per model."""
    F = torch.nn.functional
    B = batch["chosen"].shape[0]
    ids = torch.cat([batch["chosen"], batch["rejected"]], dim=0)
    mask = torch.cat([batch["chosen_mask"], batch["rejected_mask"]], dim=0)[:, 1:]

    def score(m):
        logp = F.log_softmax(m(input_ids=ids, use_cache=False).logits[:, :-1, :], dim=-1)
        picked = torch.gather(logp, -1, ids[:, 1:].unsqueeze(-1)).squeeze(-1)
        return (picked * mask).sum(-1) / mask.sum(-1)
    with torch.no_grad():
        fr = score(ref)
    pi = score(model)
    return (-F.logsigmoid(beta * ((pi[:B] - pi[B:]) - (fr[:B] - fr[B:])))).mean()


def timed(tr, loss_fn, steps, warmup):
    """-> (ms per step, peak bytes over the timed steps)."""
    for _ in range(warmup):
        tr.train_step(loss_fn)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        loss = tr.train_step(loss_fn)
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    assert torch.isfinite(loss).all()
    return ms, torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--beta", type=float, default=0.1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpo.py measures on an MI355X: no GPU found")
    import vyomai_amd as V
    from vyomai_amd.training import FlatTrainer
    cfg = V.Config()
    torch.manual_seed(0)
    model = V.ModelForCausalLM(cfg).cuda().train()
    ref = V.ModelForCausalLM(cfg).cuda().eval()
    ref.load_state_dict(model.state_dict())
    ref.compute_dtype = ref.model.compute_dtype = BF
    tr = FlatTrainer(model, lr=1e-5, weight_decay=0.01)
    g = torch.Generator().manual_seed(1)
    batch = {}
    for key in ("chosen", "rejected"):       # a quarter prompt, responses of unequal length, right-padded
        ids = torch.randint(3, cfg.vocab_size, (a.pairs, a.L), generator=g)
        mask = torch.zeros(a.pairs, a.L)
        for i in range(a.pairs):
            n = int(torch.randint(a.L // 2, a.L + 1, (1,), generator=g))
            ids[i, n:] = 0
            mask[i, a.L // 4 + 1:n] = 1.0
        batch[key], batch[key + "_mask"] = ids.cuda(), mask.cuda()
    batch["rejected"][:, :a.L // 4] = batch["chosen"][:, :a.L // 4]
    routes = {"fused": lambda: model.dpo_loss(batch, ref, beta=a.beta)[0],
              "baseline": lambda: logits_route(model, ref, batch, a.beta)}
    rounds = {k: [] for k in routes}
    peak = {k: 0 for k in routes}
    for r in range(a.rounds):
        for name, fn in routes.items():
            ms, pk = timed(tr, fn, a.steps, a.warmup if r == 0 else 1)
            rounds[name].append(statistics.median(ms))
            peak[name] = max(peak[name], pk)
            print(f"round {r} {name:8s}: {statistics.median(ms):8.3f} ms / step (min {min(ms):.3f} max {max(ms):.3f}, "
                  f"n={len(ms)}), peak {pk / 2**30:.3f} GiB")
    med = {k: statistics.median(v) for k, v in rounds.items()}
    spread = max(max(v) - min(v) for v in rounds.values())
    ok = med["fused"] <= med["baseline"] + spread and peak["fused"] < peak["baseline"]
    print(f"fused {med['fused']:.3f} ms, baseline {med['baseline']:.3f} ms, spread of the round medians {spread:.3f} ms; "
          f"peak {peak['fused'] / 2**30:.3f} GiB against {peak['baseline'] / 2**30:.3f} GiB")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "L": a.L, "vocab": cfg.vocab_size,
                      "ms_per_step": med, "round_medians_ms": rounds, "spread_ms": spread,
                      "peak_GiB": {k: v / 2**30 for k, v in peak.items()}, "ok": ok}))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
