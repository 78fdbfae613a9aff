"""Paged decode attention against the resident-context kernel on the same keys, and the continuous-batching engine against
generate() on the same prompts.   python tools/bench_paged.py [--iters 1000] [--splits 1 2 4] [--skip-engine] [--prefill] [--fp8]

Kernels: vy_attn_paged_decode (bf16, block_size 256, pages in shuffled physical order) and vy_attn_decode on the same keys
in a contiguous (B, hk, S, dh) cache, each timed as a link of a captured chain of 50 calls, the chains replayed in turn;
bytes = the K and V rows each has to read.
dh = 128 at S = 4096 has no resident-context counterpart and is reported against the 1 GiB copy ceiling measured in the
same run (vy_debug_copy, the probe behind bench.py --full).  Engine: 6 requests of mixed lengths, generated tokens per
second, against generate() on the prompts left-padded into one batch that runs until its longest request is done.
--prefill (instead of the decode kernels): the attention of one layer of a prefill step, (a) the per-sequence path
(vy_paged_gather when the sequence starts behind cached context, then vy_attn_fwd) against (b) the one
vy_attn_paged_prefill launch, on the same pages (bf16, block_size 256, shuffled physical order), both as links of captured
chains replayed in turn; TFLOP/s counts the causal half only (4 h dh sum_i (ctx + i + 1) per sequence); the whole
measurement is repeated and the lowest and highest figure of each variant are printed.  The engine section then adds
one 2048-token request arriving while 7 sequences decode, unchunked and with max_step_tokens = 256: requested tokens per
second and the longest single step().
--fp8: the decode table gets vy_attn_paged_decode_fp8 on the same keys as e4m3 pages with per-(slot, head) scales
(PagedKVManager(kv_cache_dtype="fp8")) as one more link of the same captured chains -- its bytes are the codes plus the
scales, (dh + 4) / (2 dh) of the bf16 bytes -- and the engine workload runs once more over an fp8 manager, both
engines with varlen_prefill=True (fp8 pages need it), each with its manager's kv_bytes.
Prints one JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vyomai_amd as V  # noqa: E402
from vyomai_amd import _lib, ops  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
SHAPES = [  # B, h, hk, dh, S, has a contiguous counterpart
    (32, 12, 12, 64, 640, True), (32, 12, 4, 64, 640, True), (8, 16, 8, 128, 512, True), (8, 16, 8, 128, 4096, False)]


def timed(fns, warmup, iters):
    """us per call of each fn with the host's launch cost in it (long kernels only)."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    out = []
    for f in fns:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            f()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / iters)
    return out


def timed_graph(fns, warmup, iters, reps=50):
    """us per call of each fn as a link of a captured chain of `reps` calls (a Python call costs more host time than
    these kernels take on the device); the chains of the fns are replayed in turn, iters / reps times each."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    graphs = []
    for f in fns:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                f()
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    rounds = max(1, iters // reps)
    total = [0.0] * len(fns)
    for _ in range(rounds):
        for i, g in enumerate(graphs):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            total[i] += s.elapsed_time(e)
    return [t * 1e3 / (rounds * reps) for t in total]


def copy_ceiling_gbs():
    lib = _lib.load()
    lib.vy_debug_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    n = 1 << 30
    a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    b = torch.empty_like(a)
    st = torch.cuda.current_stream().cuda_stream
    t, = timed([lambda: lib.vy_debug_copy(a.data_ptr(), b.data_ptr(), n, st)], 3, 10)
    return 2.0 * n / t * 1e-3


def quantise_pages(pages):
    """The rule of include/vyom_hip.h on bf16 pages (blocks, bs, hk, dh) -> (e4m3 codes, fp32 scales (blocks, bs, hk))."""
    x = pages.float()
    amax = x.abs().amax(dim=-1)
    s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (x / s.unsqueeze(-1)).clamp(-448, 448).to(torch.float8_e4m3fn), s


def bench_kernels(iters, splits=(), fp8=False):
    ceiling = copy_ceiling_gbs()
    print(json.dumps({"what": "copy ceiling", "GBs": round(ceiling, 1)}))
    bs = 256
    for B, h, hk, dh, S, dense in SHAPES:
        g = torch.Generator().manual_seed(S + dh)
        k = torch.randn(B, hk, S, dh, generator=g).to(BF).to(DEV)
        v = torch.randn(B, hk, S, dh, generator=g).to(BF).to(DEV)
        q = torch.randn(B, h * dh, generator=g).to(BF).to(DEV)
        pages = (S + bs - 1) // bs
        nblk = B * pages
        table = torch.randperm(nblk, generator=g).to(torch.int32).view(B, pages)
        kc = torch.zeros(nblk, bs, hk, dh, dtype=BF, device=DEV)
        vc = torch.zeros_like(kc)
        j = torch.arange(S)
        slot = (table[:, j // bs].long() * bs + j % bs).to(DEV)                  # (B, S)
        kc.view(-1, hk, dh)[slot] = k.permute(0, 2, 1, 3)
        vc.view(-1, hk, dh)[slot] = v.permute(0, 2, 1, 3)
        table, seqlens = table.to(DEV), torch.full((B,), S, dtype=torch.int32, device=DEV)
        out = torch.empty(B, h * dh, dtype=BF, device=DEV)
        q4 = q.view(B, h, 1, dh)
        fns = [lambda: ops.attention_paged_decode(q, kc, vc, table, seqlens, S, h, out=out)]
        for n in splits:
            fns.append(lambda n=n: ops.attention_paged_decode(q, kc, vc, table, seqlens, S, h, out=out, n_split=n))
        if fp8:
            (kq, ks), (vq, vs) = quantise_pages(kc), quantise_pages(vc)
            out8 = torch.empty_like(out)
            fns.append(lambda: ops.attention_paged_decode(q, kq, vq, table, seqlens, S, h, out=out8, k_scale=ks, v_scale=vs))
        if dense:
            fns.append(lambda: ops.attention_decode(q4, k, v, S))
        t = timed_graph(fns, 20, iters)
        nbytes = 2 * B * hk * S * dh * 2
        ns = (_lib.load().vy_attn_paged_decode_ws_bytes(B, h, hk, dh, S, 0, 1) // (B * h * (dh + 2) * 4)) or 1
        rec = {"what": "decode attention", "B": B, "h": h, "hk": hk, "dh": dh, "S": S, "n_split": ns,
               "paged_us": round(t[0], 2), "paged_GBs": round(nbytes / t[0] * 1e-3, 1),
               "paged_share_of_copy_ceiling": round(nbytes / t[0] * 1e-3 / ceiling, 3)}
        for n, us in zip(splits, t[1:]):
            rec[f"paged_n_split_{n}_us"] = round(us, 2)
        if fp8:
            us = t[1 + len(splits)]
            nb8 = 2 * B * hk * S * (dh + 4)
            ns8 = (_lib.load().vy_attn_paged_decode_fp8_ws_bytes(B, h, hk, dh, S, 0, 1) // (B * h * (dh + 2) * 4)) or 1
            fns[0]()
            rec.update(fp8_us=round(us, 2), fp8_n_split=ns8, fp8_GBs=round(nb8 / us * 1e-3, 1),
                       fp8_share_of_copy_ceiling=round(nb8 / us * 1e-3 / ceiling, 3), fp8_bytes_ratio=round(nb8 / nbytes, 3),
                       fp8_time_ratio=round(us / t[0], 3), fp8_max_abs_diff=(out8.float() - out.float()).abs().max().item())
        if dense:
            diff = (out.float() - ops.attention_decode(q4, k, v, S).view(B, -1).float()).abs().max().item()
            rec.update(contiguous_us=round(t[-1], 2), ratio=round(t[0] / t[-1], 3), max_abs_diff=diff)
        print(json.dumps(rec))


PREFILL_SHAPES = [(8, 512, 0), (8, 512, 1536), (32, 64, 0)]         # sequences, rows each, cached context
PREFILL_HEADS = [(12, 12, 64), (16, 8, 128), (4, 2, 224)]


def bench_prefill(iters, repeats=3):
    bs = 256
    for h, hk, dh in PREFILL_HEADS:
        for n, rows, ctx in PREFILL_SHAPES:
            g = torch.Generator().manual_seed(rows + dh + ctx)
            S, T = ctx + rows, n * rows
            pages = (S + bs - 1) // bs
            nblk = n * pages
            table = torch.randperm(nblk, generator=g).to(torch.int32).view(n, pages)
            qkv = torch.randn(T, (h + 2 * hk) * dh, generator=g).to(BF).to(DEV)
            kc = torch.randn(nblk, bs, hk, dh, generator=g).to(BF).to(DEV)
            vc = torch.randn(nblk, bs, hk, dh, generator=g).to(BF).to(DEV)
            j = torch.arange(ctx, S)
            slot = (table[:, j // bs].long() * bs + j % bs).to(DEV)              # (n, rows): the step's own rows
            kc.view(-1, hk, dh)[slot] = qkv[:, h * dh:(h + hk) * dh].view(n, rows, hk, dh)
            vc.view(-1, hk, dh)[slot] = qkv[:, (h + hk) * dh:].view(n, rows, hk, dh)
            table = table.to(DEV)
            cu = (torch.arange(n + 1, dtype=torch.int32) * rows).to(DEV)
            ctxs = torch.full((n,), ctx, dtype=torch.int32, device=DEV)
            o_old = torch.empty(T, h * dh, dtype=BF, device=DEV)
            o_new = torch.empty_like(o_old)

            def old():
                for s in range(n):
                    seg = qkv[s * rows:(s + 1) * rows]
                    q4 = seg[:, :h * dh].view(rows, h, dh).permute(1, 0, 2).unsqueeze(0)
                    if ctx:
                        k3, v3 = ops.paged_gather(kc, vc, table[s], S)
                    else:
                        k3 = seg[:, h * dh:(h + hk) * dh].view(rows, hk, dh).permute(1, 0, 2)
                        v3 = seg[:, (h + hk) * dh:].view(rows, hk, dh).permute(1, 0, 2)
                    ops.attention(q4, k3.unsqueeze(0), v3.unsqueeze(0), causal=True, start_pos=ctx,
                                  out=o_old[s * rows:(s + 1) * rows].unsqueeze(0))

            def new():
                ops.attention_paged_prefill(qkv, kc, vc, table, cu, ctxs, rows, S, h, out=o_new)

            runs = [timed_graph([old, new], 3, iters, reps=10) for _ in range(repeats)]
            flops = 4.0 * h * dh * n * (rows * ctx + rows * (rows + 1) / 2)
            t_old, t_new = [r[0] for r in runs], [r[1] for r in runs]
            diff = (o_old.float() - o_new.float()).abs().max().item()
            print(json.dumps({
                "what": "prefill attention", "h": h, "hk": hk, "dh": dh, "sequences": n, "rows": rows, "ctx": ctx,
                "launches_per_seq_path": n * (2 if ctx else 1),
                "per_seq_us": [round(min(t_old), 1), round(max(t_old), 1)],
                "varlen_us": [round(min(t_new), 1), round(max(t_new), 1)],
                "per_seq_TFLOPs": round(flops / min(t_old) * 1e-6, 1), "varlen_TFLOPs": round(flops / min(t_new) * 1e-6, 1),
                "ratio": round(min(t_new) / min(t_old), 3), "max_abs_diff": diff}))


def bench_engine_long_arrival():
    """7 sequences decode, then a 2048-token request arrives: unchunked, its prefill is one long step that every
    decoding sequence waits for; with max_step_tokens = 256 it is spread over 9 steps."""
    cfg = V.Config(vocab_size=32000, hidden_size=896, intermediate_size=4864, num_hidden_layers=4,
                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=4096, pad_token_id=0)
    torch.manual_seed(0)
    m = V.ModelForCausalLM(cfg).to(BF).to(DEV).eval()
    g = torch.Generator().manual_seed(2)
    short = [torch.randint(3, cfg.vocab_size, (32,), generator=g).tolist() for _ in range(7)]
    long = torch.randint(3, cfg.vocab_size, (2048,), generator=g).tolist()
    requested = 7 * 128 + 32

    def run(**kw):
        mgr = V.PagedKVManager(cfg, 256, 16, DEV, BF)
        eng = V.ContinuousBatchEngine(m, mgr, max_batch_size=8, eos_token_ids=[], **kw)
        for p in short:
            eng.add_sequence(p, max_gen_len=128)
        steps = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while eng.active or eng.waiting_room:
            if len(steps) == 8:
                eng.add_sequence(long, max_gen_len=32)
            t1 = time.perf_counter()
            eng.step()                         # (ends with the step's device-to-host copy of the ids)
            steps.append(time.perf_counter() - t1)
        return time.perf_counter() - t0, max(steps), len(steps)

    for name, kw in (("engine, long arrival, unchunked", {}), ("engine, long arrival, max_step_tokens 256", {"max_step_tokens": 256})):
        run(**kw)                              # warm-up: every shape of the run
        res = [run(**kw) for _ in range(3)]
        dt = sorted(r[0] for r in res)[1]
        print(json.dumps({"what": name, "requested_tokens": requested, "steps": res[0][2], "seconds": round(dt, 4),
                          "requested_tokens_per_s": round(requested / dt, 1),
                          "longest_step_ms": [round(min(r[1] for r in res) * 1e3, 2), round(max(r[1] for r in res) * 1e3, 2)]}))


def bench_engine(fp8=False):
    cfg = V.Config(vocab_size=32000, hidden_size=896, intermediate_size=4864, num_hidden_layers=4,
                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=1024, pad_token_id=0)
    torch.manual_seed(0)
    m = V.ModelForCausalLM(cfg).to(BF).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    plen, glen = [12, 40, 96, 24, 160, 64], [64, 32, 128, 16, 96, 48]
    prompts = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in plen]

    def run_engine(kv_cache_dtype=None, **kw):
        mgr = V.PagedKVManager(cfg, 64, 16, DEV, BF, kv_cache_dtype=kv_cache_dtype)
        eng = V.ContinuousBatchEngine(m, mgr, max_batch_size=8, eos_token_ids=[], **kw)
        for p, n in zip(prompts, glen):
            eng.add_sequence(p, max_gen_len=n)
        eng.run()
        return mgr.kv_bytes

    def run_generate():
        L = max(plen)
        ids = torch.zeros((len(prompts), L), dtype=torch.long)
        mask = torch.zeros_like(ids)
        for r, p in enumerate(prompts):
            ids[r, L - len(p):] = torch.tensor(p)
            mask[r, L - len(p):] = 1
        return m.generate(ids.to(DEV), attention_mask=mask.to(DEV), max_new_tokens=max(glen))

    runs = [("engine", run_engine), ("generate", run_generate)]
    if fp8:
        runs = [("engine, varlen prefill, bf16 pages", lambda: run_engine(varlen_prefill=True)),
                ("engine, varlen prefill, fp8 pages", lambda: run_engine("fp8", varlen_prefill=True))]
    for name, fn in runs:
        kv_bytes = fn()                        # warm-up: every shape of the run
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        rec = {"what": name, "requests": len(prompts), "requested_tokens": sum(glen),
               "seconds": round(dt, 4), "requested_tokens_per_s": round(sum(glen) / dt, 1)}
        if fp8:
            rec["kv_bytes"] = kv_bytes
        print(json.dumps(rec))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--prefill", action="store_true", help="time the prefill attention paths instead of the decode kernels")
    ap.add_argument("--fp8", action="store_true", help="add the fp8-page decode kernel and the engine over an fp8 manager")
    ap.add_argument("--splits", type=int, nargs="*", default=[], help="also time these pinned n_split values")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged.py needs the MI355X: there is nothing to time without it")
    if a.prefill:
        bench_prefill(min(a.iters, 200))
    else:
        bench_kernels(a.iters, a.splits, a.fp8)
    if not a.skip_engine:
        bench_engine(a.fp8)
        if a.prefill:
            bench_engine_long_arrival()
