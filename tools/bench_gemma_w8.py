"""Single-sequence Gemma decode on fp8 weights against bf16, BASELINE configs[4] widths, one process, one MI355X:
  python tools/bench_gemma_w8.py [--links-only] [--json PATH]

Links.  Each of the four products of a layer (qkv 2560 x 2048, o_proj 2048 x 2048, gated 2 x 16384 x 2048, down
2048 x 16384) and the vocabulary product (257216 x 2048), through the vy_debug_dec_gemv1* wrappers: bf16 weights
(dec_gemv1_kernel), e4m3fn codes + row scales (dec_gemv1_w8_kernel), and beside them a device copy of the same bytes
(read + write: its rate counts both).  Every link walks a pool of weight copies larger than the 256 MB Infinity Cache,
as the real step does (5.8 GB per token, each byte once); bf16 and w8 alternate round by round, the median round is
reported.  Time per link from device events around 20 launches on one stream.

Whole step.  The native step of the full 18-layer model with random init: GemmaDecodePlan(weight_dtype=None) against
"fp8", alternating, device events around 32 steps; then tokens/s of generate() as tools/bench_paligemma.py takes it.
The bf16 column is the comparison: it must agree with tools/bench_paligemma.py on the same box to the +-3-5 % the README
states for boxes, otherwise the run is not to be trusted."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vyomai_amd import _lib  # noqa: E402
from vyomai_amd.decode_plan import GemmaDecodePlan, quant_rows_fp8  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
P, I32, I64, F32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
H, HK, DH, D, FFN, VOCAB = 8, 1, 256, 2048, 16384, 257216
LINKS = [("qkv", "qkv", (H + 2 * HK) * DH, D), ("o_proj", "plain", D, H * DH), ("gated", "gated", FFN, D),
         ("down", "plain", D, FFN), ("head", "plain", VOCAB, D)]
LAUNCHES, ROUNDS, POOL_BYTES = 20, 7, 640 << 20


def lib():
    l = _lib.load()
    for name, sig in {
        "vy_debug_dec_gemv1": [P, P, P, P, P, I32, I32, P],
        "vy_debug_dec_gemv1_gated": [P, P, P, I32, I32, I32, F32, P],
        "vy_debug_dec_gemv1_qkv": [P, P, P, P, P, P, I64, I32, I32, I32, P, P, I64, I32, I32, F32, P],
        "vy_debug_dec_gemv1_w8": [P, P, P, P, P, P, I32, I32, P],
        "vy_debug_dec_gemv1_gated_w8": [P, P, P, P, I32, I32, I32, F32, P],
        "vy_debug_dec_gemv1_qkv_w8": [P, P, P, P, P, P, P, I64, I32, I32, I32, P, P, I64, I32, I32, F32, P],
    }.items():
        f = getattr(l, name)
        f.argtypes, f.restype = sig, C.c_int
    return l


def timed(fn, n):
    """ms per call of fn(i), i = 0 .. n - 1, device events around the n launches"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def bench_link(l, name, kind, N, K):
    from vyomai_amd import ops
    rows = 2 * N if kind == "gated" else N
    pool = max(2, min(64, POOL_BYTES // (rows * K * 2)))
    g = torch.Generator(device=DEV).manual_seed(N + K)
    w16 = [(torch.randn(rows, K, generator=g, device=DEV) * K ** -0.5).to(BF) for _ in range(pool)]
    w8 = [quant_rows_fp8(w) for w in w16]
    x = torch.randn(K, generator=g, device=DEV).to(BF)
    y = torch.empty(max(N, 4096) + 8, dtype=BF, device=DEV)
    kc, vc = torch.zeros(HK, 384, DH, dtype=BF, device=DEV), torch.zeros(HK, 384, DH, dtype=BF, device=DEV)
    cos, sin = ops.rope_tables(DH, 512, DEV)
    dst16, dst8 = torch.empty_like(w16[0]), torch.empty_like(w8[0][0])
    st = torch.cuda.current_stream().cuda_stream

    def go16(i):
        w = w16[i % pool].data_ptr()
        if kind == "plain":
            rc = l.vy_debug_dec_gemv1(x.data_ptr(), w, None, None, y.data_ptr(), N, K, st)
        elif kind == "gated":
            rc = l.vy_debug_dec_gemv1_gated(x.data_ptr(), w, y.data_ptr(), N, K, 1, 1e-6, st)
        else:
            rc = l.vy_debug_dec_gemv1_qkv(x.data_ptr(), w, None, y.data_ptr(), kc.data_ptr(), vc.data_ptr(), 384 * DH, H, HK, DH,
                                          cos.data_ptr(), sin.data_ptr(), 7, K, 1, 1e-6, st)
        assert rc == 0, (name, rc)

    def go8(i):
        c, s = w8[i % pool]
        if kind == "plain":
            rc = l.vy_debug_dec_gemv1_w8(x.data_ptr(), c.data_ptr(), s.data_ptr(), None, None, y.data_ptr(), N, K, st)
        elif kind == "gated":
            rc = l.vy_debug_dec_gemv1_gated_w8(x.data_ptr(), c.data_ptr(), s.data_ptr(), y.data_ptr(), N, K, 1, 1e-6, st)
        else:
            rc = l.vy_debug_dec_gemv1_qkv_w8(x.data_ptr(), c.data_ptr(), s.data_ptr(), None, y.data_ptr(), kc.data_ptr(),
                                             vc.data_ptr(), 384 * DH, H, HK, DH, cos.data_ptr(), sin.data_ptr(), 7, K, 1, 1e-6, st)
        assert rc == 0, (name, rc)

    runs = {"bf16": go16, "w8": go8, "copy_bf16_bytes": lambda i: dst16.copy_(w16[i % pool]),
            "copy_w8_bytes": lambda i: dst8.copy_(w8[i % pool][0])}
    n = LAUNCHES if rows * K < (1 << 28) else 6
    for fn in runs.values():
        timed(fn, n)                                    # warm-up: code objects, every pool entry touched
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            ms[k].append(timed(fn, n))
    med = {k: statistics.median(v) for k, v in ms.items()}
    b16, b8 = rows * K * 2, rows * K + 4 * rows
    return {"link": name, "N": N, "K": K, "pool": pool, "bf16_us": round(med["bf16"] * 1e3, 2), "w8_us": round(med["w8"] * 1e3, 2),
            "bf16_TBps": round(b16 / med["bf16"] * 1e-9, 2), "w8_TBps": round(b8 / med["w8"] * 1e-9, 2),
            "w8_speedup": round(med["bf16"] / med["w8"], 3),
            "copy_bf16_bytes_us": round(med["copy_bf16_bytes"] * 1e3, 2), "copy_w8_bytes_us": round(med["copy_w8_bytes"] * 1e3, 2),
            "spread_bf16": round((max(ms["bf16"]) - min(ms["bf16"])) / med["bf16"], 3),
            "spread_w8": round((max(ms["w8"]) - min(ms["w8"])) / med["w8"], 3)}


def bench_step(new_tokens=64):
    from vyomai_amd import shapes as cases
    from vyomai_amd.models import paligemma as PG
    torch.manual_seed(0)
    vis, txt = PG.SiglipVisionConfig(**cases.SIGLIP), types.SimpleNamespace(**cases.GEMMA)
    with torch.device(DEV):
        m = PG.PaliGemmaForConditionalGeneration(PG.PaliGemmaShape(vis, txt, txt.hidden_size))
    m = m.to(BF).eval()
    for p in m.parameters():
        if p.dim() > 1:
            torch.nn.init.normal_(p, std=0.02)
    caches = [(torch.zeros(1, txt.num_key_value_heads, 384, txt.head_dim, dtype=BF, device=DEV),
               torch.zeros(1, txt.num_key_value_heads, 384, txt.head_dim, dtype=BF, device=DEV)) for _ in m.layers]
    plans = {"bf16": GemmaDecodePlan(m, caches, 1), "w8": GemmaDecodePlan(m, caches, 1, weight_dtype="fp8")}
    x = (torch.randn(1, txt.hidden_size, device=DEV) * 0.3).to(BF)
    ms = {k: [] for k in plans}
    for k, p in plans.items():
        timed(lambda i: p.step(x, 264 + i), 8)
    for _ in range(ROUNDS):
        for k, p in plans.items():
            ms[k].append(timed(lambda i: p.step(x, 264 + i), 32))
    out = {f"step_{k}_ms": round(statistics.median(v), 4) for k, v in ms.items()}
    out.update({f"step_{k}_weight_bytes": int(sum(p.weight_bytes.values())) for k, p in plans.items()})
    out["step_speedup"] = round(out["step_bf16_ms"] / out["step_w8_ms"], 3)
    del plans
    img = torch.rand(1, 3, 224, 224, device=DEV)
    ids = torch.randint(3, txt.vocab_size, (1, 8), device=DEV)

    def go(n, wd):
        torch.cuda.synchronize()
        t = time.perf_counter()
        m.generate(img, ids, max_new_tokens=n, max_cache_len=384, weight_dtype=wd)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    for name, wd in (("bf16", None), ("w8", "fp8"), ("bf16_again", None), ("w8_again", "fp8")):
        go(4, wd)
        t1 = go(1, wd)
        per = (go(new_tokens, wd) - t1) / (new_tokens - 1)
        out[f"generate_{name}_ms_per_token"] = round(per * 1e3, 4)
        out[f"generate_{name}_tokens_per_sec"] = round(1 / per, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemma_w8 needs a GPU")
    l = lib()
    res = {"links": [bench_link(l, *spec) for spec in LINKS]}
    for r in res["links"]:
        print(json.dumps(r), flush=True)
    if not a.links_only:
        res["step"] = bench_step()
        print(json.dumps(res["step"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
