"""The decode-only kernels (vyomai_amd/csrc/vy_decode.hip) against CPU references in float64.

Part A -- single-query attention (dec_attn_kernel<DH, NW, NP, NT, R>): every instantiation of the dispatch table is
launched through ops.attention_decode at the context lengths on both sides of every NP bucket edge, with the cache rows
past the context filled with NaN, and the test asserts WHICH instantiation ran (vy_debug_decode_attn_last) before it
compares numbers.

Part B -- the native decoder step (vy_decoder_step through DecodePlan.step) against oracle/vyom_oracle.py evaluated in
float64 on the same bf16-rounded weights, cache contents and input rows; the yardstick is the same oracle evaluated in
bf16 on the CPU (the HIP bf16 path is no further from exact arithmetic than the reference's own bf16).
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------
# Part A: single-query attention
# ------------------------------------------------------------------------------------------------------------
NP_BUCKETS = (3, 5, 7, 10, 12)
KPP = {64: 64, 256: 32}          # keys per pass: NW waves x (64 / (DH / 8)) keys = 8 x 8 and 16 x 2
FALLBACK = (0, 0, 0, 0)


def attn_last():
    from vyomai_amd import _lib
    out = (C.c_int * 4)()
    _lib.load().vy_debug_decode_attn_last(out)
    return tuple(out)


def expected_tuple(dh, h, hk, S, B):
    """The dispatch of vy_dec_attn restated from its documentation (not read from the library)."""
    np_ = -(-S // KPP[dh])
    if np_ > 12:
        return FALLBACK
    bucket = next(b for b in NP_BUCKETS if np_ <= b)
    nt = 4 * B * hk * S * dh > (1 << 20)          # K and V rows of one layer, bf16
    rep = h // hk
    r = rep if (dh == 64 and nt and rep in (2, 3, 4)) else 1
    return (dh, bucket, int(nt), r)


def dispatch_table():
    t = set()
    for np_ in NP_BUCKETS:
        t.add((64, np_, 0, 1))
        t.update((64, np_, 1, r) for r in (1, 2, 3, 4))
        t.update((256, np_, nt, 1) for nt in (0, 1))
    return t


def batches(dh, hk, S):
    """(streamed, B) with one layer's rows over 1 MiB and (default loads, B) with them under it, where a batch of at
    most 256 allows."""
    per_row = 4 * hk * S * dh
    out = []
    b_nt = (1 << 20) // per_row + 1
    if b_nt <= 256:
        out.append((1, b_nt))
    b_small = min(3, (1 << 20) // per_row)
    if b_small >= 1:
        out.append((0, b_small))
    return out


HEADS64 = [(12, 12), (12, 6), (12, 4), (8, 2), (8, 1)]      # R = 1, 2, 3, 4 and h / hk = 8 (R = 1, shared KV head)
S64 = [1, 7, 8, 9, 63, 64, 65, 192, 193, 320, 321, 448, 449, 640, 641, 768, 769, 1000]
HEADS256 = [(8, 1), (4, 4)]
S256 = [1, 2, 3, 96, 97, 160, 161, 224, 225, 320, 321, 384, 385]
ATTN_CASES = [(dh, h, hk, S, nt, B) for dh, heads, ss in ((64, HEADS64, S64), (256, HEADS256, S256))
              for (h, hk) in heads for S in ss for (nt, B) in batches(dh, hk, S)]


def _attn_inputs(dh, h, hk, S, B, regime, seed):
    """q (B, h, 1, dh) and K/V caches (B, hk, cap, dh) as strided views: capacity S + 9 rounded up to a multiple of 8,
    a batch stride larger than hk * cap * dh, NaN in every row >= S and in the gap between batch rows."""
    g = torch.Generator().manual_seed(seed)
    cap = (S + 9 + 7) // 8 * 8
    sb = hk * cap * dh + 64
    bufs = []
    for _ in range(2):
        buf = torch.full((B, sb), float("nan"), dtype=BF)
        view = buf.as_strided((B, hk, cap, dh), (sb, cap * dh, dh, 1))
        view[:, :, :S] = torch.randn(B, hk, S, dh, generator=g).to(BF)
        bufs.append((buf, view))
    (kbuf, k), (vbuf, v) = bufs
    if regime == "flat":
        q = torch.randn(B, h, 1, dh, generator=g).to(BF)
    else:
        # peaked: q = 6 * k[j*] for one key j* per (row, head) in the LAST wave pass: score 6 |k|^2 / sqrt(dh) (about 48
        # at dh = 64, 96 at dh = 256) against a spread of 6 for the other keys
        first = (S - 1) // KPP[dh] * KPP[dh]
        jstar = torch.randint(first, S, (B, h), generator=g)
        kvh = torch.arange(h) // (h // hk)
        q = (6.0 * k[torch.arange(B)[:, None], kvh[None, :], jstar].float()).to(BF)[:, :, None, :]
    return q.contiguous(), (kbuf, k), (vbuf, v), cap, sb


def _attn_ref(q, k, v, S, h, hk):
    rep = h // hk
    kd = k[:, :, :S].double().repeat_interleave(rep, 1)
    vd = v[:, :, :S].double().repeat_interleave(rep, 1)
    s = (q.double() @ kd.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    p = torch.softmax(s, -1)
    return (p @ vd).transpose(1, 2).reshape(q.shape[0], 1, -1)        # (B, 1, h * dh)


def _attn_run(dh, h, hk, S, B, regime, seed):
    from vyomai_amd import ops
    q, (kbuf, k), (vbuf, v), cap, sb = _attn_inputs(dh, h, hk, S, B, regime, seed)
    kd, vd = kbuf.to(DEV), vbuf.to(DEV)
    shape, strides = (B, hk, cap, dh), (sb, cap * dh, dh, 1)
    got = ops.attention_decode(q.to(DEV), kd.as_strided(shape, strides), vd.as_strided(shape, strides), S)
    torch.cuda.synchronize()
    return got.cpu(), q, k, v, attn_last()


@pytest.mark.parametrize("dh,h,hk,S,nt,B", ATTN_CASES)
def test_decode_attention_every_instantiation(dh, h, hk, S, nt, B):
    """Bound (derived, not measured): bf16 inputs, scores / softmax / weighted sum in fp32, ONE rounding of the result.
    Against fp64 on the same inputs: |got - want| <= 2^-8 |want| + 1e-4 max|v| -- a bf16 rounding, and S * 2^-24 of
    accumulation plus the error of __expf.  The row-wise kernel behind the fallback cases keeps its probabilities in
    fp32 as well (attn_rowwise_kernel: online softmax in fp32, one rounding at the store), so the same reference and
    the same bound hold for it."""
    want_tuple = expected_tuple(dh, h, hk, S, B)
    assert want_tuple == FALLBACK or want_tuple[2] == nt
    for regime in ("flat", "peaked"):
        got, q, k, v, ran = _attn_run(dh, h, hk, S, B, regime, seed=S * 131 + hk * 7 + B)
        assert ran == want_tuple, f"meant to run {want_tuple}, ran {ran}"
        want = _attn_ref(q, k, v, S, h, hk)
        assert torch.isfinite(got.float()).all(), f"{regime}: non-finite output (a key row >= S took part)"
        err = (got.double() - want).abs()
        bound = 2.0 ** -8 * want.abs() + 1e-4 * v[:, :, :S].float().abs().max().item()
        bad = err > bound
        if bad.any():
            b, _, c = bad.nonzero()[0].tolist()
            raise AssertionError(f"{regime} {want_tuple}: {int(bad.sum())}/{bad.numel()} off; first at row {b} head "
                                 f"{c // dh} col {c % dh}: got {got[b, 0, c].item():.6f} want {want[b, 0, c].item():.6f} "
                                 f"(max err / bound {float((err / bound).max()):.2f})")


def test_decode_attention_cases_cover_the_dispatch_table():
    """Launches every case once more (no comparison) and collects what ran: the set of (DH, NP, NT, R) seen is the whole
    dispatch table of vy_dec_attn, plus the fallback."""
    seen = set()
    for (dh, h, hk, S, nt, B) in ATTN_CASES:
        *_, ran = _attn_run(dh, h, hk, S, B, "flat", seed=1)
        seen.add(ran)
    table = dispatch_table()
    assert FALLBACK in seen
    assert seen - {FALLBACK} == table, (sorted(table - seen), sorted(seen - table - {FALLBACK}))
    assert len(table) == 35


# ------------------------------------------------------------------------------------------------------------
# Part B: the native decoder step (vy_decoder_step) against the oracle in float64
# ------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _fill_(m, seed):
    """Weights of the scale of vyomai_amd.recipe (LayerNorm scale 1 + 0.1 u, biases 0.02 u, embeddings u, matrices
    0.8 u / sqrt(fan_in)), drawn with torch's generator: a 12-layer model in a fraction of a second."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in m.state_dict().items():
            if not t.is_floating_point():
                continue
            u = torch.rand(t.shape, generator=g) * 2 - 1
            leaf = name.rsplit(".", 1)[-1]
            if ("layernorm" in name or "layer_norm" in name) and leaf == "weight":
                t.copy_(1 + 0.1 * u)
            elif leaf == "bias" or t.dim() <= 1:
                t.copy_(0.02 * u)
            elif "embeddings" in name:
                t.copy_(u)
            else:
                t.copy_(u * (0.8 / math.sqrt(t.shape[1])))


def _dec_model(d, ffn, layers, pos_kind, hk, maxpos, vocab=1003):
    """-> (cfg, model on the GPU in bf16, state dict of the bf16-rounded weights on the CPU).  64-wide heads; hk < h
    selects the grouped-query attention class."""
    key = (d, ffn, layers, pos_kind, hk, maxpos, vocab)
    if key not in _MODELS:
        import vyomai_amd as V
        from vyomai_amd.layers.ffn import FeedForward
        h = d // 64
        cfg = V.EncoderConfig(hidden_size=d, num_attention_heads=h, num_hidden_layers=layers, vocab_size=vocab,
                              max_position_embeddings=maxpos, hidden_dropout_prob=0.0)
        if hk != h:
            cfg.num_key_value_heads = hk
        m = V.DecoderModel(cfg, pos_kind, "gqa" if hk != h else None)
        if ffn != 4 * d:
            assert ffn % d == 0
            for layer in m.all_layer:
                layer.feed_forward = FeedForward(cfg, multiplier=ffn // d)
        _fill_(m, seed=d + ffn + hk)
        m = m.to(BF).eval()
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        _MODELS.clear()      # one model at a time on the card
        _MODELS[key] = (cfg, m.to(DEV), sd)
    return _MODELS[key]


def _plan_and_cache(cfg, m, B, cap, pos, seed):
    """A StaticCacheOne whose rows [0, pos) hold random bf16 numbers and whose rows >= pos hold NaN (the step writes row
    pos before it reads it; nothing may read past it) -> (plan, cache, CPU copies of the filled K / V per layer)."""
    from vyomai_amd.decode_plan import DecodePlan
    from vyomai_amd.layers.kv_cache import StaticCacheOne
    cache = StaticCacheOne(cfg, max_cache_len=cap, batch_size=B, dtype=BF)
    plan = DecodePlan(m, cache, B, BF, torch.device("cuda", 0))
    g = torch.Generator().manual_seed(seed)
    filled = []
    for i in range(len(cache.key_cache)):
        kv = []
        for c in (cache.key_cache[i], cache.value_cache[i]):
            t = torch.full(tuple(c.shape), float("nan"), dtype=BF)
            t[:, :, :pos] = torch.randn(t.shape[0], t.shape[1], pos, t.shape[3], generator=g).to(BF)
            c.copy_(t)
            kv.append(t)
        filled.append(tuple(kv))
    return plan, cache, filled


def _oracle_step(sd, cfg, x, filled, pos, pos_kind, dtype):
    """One token through oracle.block x layers + lm_head in `dtype`, on the same weights, cache contents and rows."""
    from oracle import vyom_oracle as O
    c = O.Cfg.of(cfg)
    h = c.num_attention_heads
    hk = getattr(cfg, "num_key_value_heads", h)
    c.num_key_value_heads = hk
    dh = c.hidden_size // h
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    B = x.shape[0]
    cap = filled[0][0].shape[2]
    cache = O.OracleStaticCache(len(filled), B, hk, cap, dh, dtype=dtype)
    for i, (k, v) in enumerate(filled):
        cache.k[i][:, :, :pos] = k[:, :, :pos].to(dtype)
        cache.v[i][:, :, :pos] = v[:, :, :pos].to(dtype)
    freqs = O.rotary_angles(dh, c.max_position_embeddings)[:, pos:pos + 1] if pos_kind == "rope" else None
    hcur = x.to(dtype)[:, None, :]
    with torch.no_grad():
        for i in range(c.num_hidden_layers):
            hcur = O.block(sdd, f"all_layer.{i}.", c, hcur, None, freqs, hk != h, False, cache, i, pos)
        logits = O.lm_head(sdd, "lm_head.", c, hcur)
    return hcur[:, 0].double(), logits[:, 0].double()


def _step_ratios(d, ffn, layers, hk, B, pos, cap, pos_kind="rope", what=""):
    """Runs one native step and both oracles -> {name: (ratio of means, ratio of maxima, [row maximum / reference
    tensor maximum per row])} for the hidden state and the logits; prints the figures (the table of DESIGN section 4)."""
    cfg, m, sd = _dec_model(d, ffn, layers, pos_kind, hk, max(cap, 128))
    g = torch.Generator().manual_seed(1000 * B + pos)
    x = (torch.randn(B, d, generator=g) * 0.5).to(BF)
    plan, cache, filled = _plan_and_cache(cfg, m, B, cap, pos, seed=B + pos)
    logits, hidden = plan.step(x.to(DEV), pos, want_hidden=True)
    torch.cuda.synchronize()
    got = {"hidden": hidden.double().cpu(), "logits": logits.double().cpu()}
    exact = dict(zip(("hidden", "logits"), _oracle_step(sd, cfg, x, filled, pos, pos_kind, torch.float64)))
    refbf = dict(zip(("hidden", "logits"), _oracle_step(sd, cfg, x, filled, pos, pos_kind, BF)))
    out = {}
    for name in ("hidden", "logits"):
        assert torch.isfinite(got[name]).all(), f"{name}: non-finite (a cache row >= pos + 1 took part)"
        e_hip, e_ref = (got[name] - exact[name]).abs(), (refbf[name] - exact[name]).abs()
        rows = e_hip.max(dim=1).values / e_ref.max()
        out[name] = (float(e_hip.mean() / e_ref.mean()), float(e_hip.max() / e_ref.max()), rows.tolist())
        row_mean = float(e_hip.mean(dim=1).max() / e_ref.mean(dim=1).max())
        print(f"RATIO | {what or f'{layers}L d={d} ffn={ffn} h/hk={d // 64}/{hk} B={B} pos={pos}'} | {name} | "
              f"mean {e_hip.mean():.3e} / {e_ref.mean():.3e} = {out[name][0]:.3f} | "
              f"max {e_hip.max():.3e} / {e_ref.max():.3e} = {out[name][1]:.3f} | worst row mean {row_mean:.3f}")
    return out


# Margins against the CPU-bf16 oracle's own error (both against fp64).  Means, and the maximum over the logits: 1.0, the
# HIP step rounds to bf16 at a subset of the points where the reference does and accumulates in fp32 (measured over the
# 116 cases of DESIGN section 4: means 0.62 .. 0.96, logits maximum 0.94 at most).
# Maximum over the hidden state: NOT 1.0.  Measured 0.64 .. 1.51 with a median of exactly 1.000 and a geometric mean of
# 0.98; 27 of the 116 cases are above 1.0.  The rounding point is the one both paths share, the bf16 store of the last
# LayerNorm's output: its half-ulp (0.0078 for |h| in [2, 4), 0.0156 in [4, 8)) is three to six times the error that
# arrives from upstream (mean 0.0025), so a tensor's maximum is whichever of its few largest elements sits next to a
# rounding tie -- in half of the cases the SAME element with the SAME error in both paths (ratio 1.000), otherwise one
# draw each from the same tail, spread evenly around 1 and wider the fewer elements there are.  The maxima pooled over
# the nine (B, pos) cases of a shape agree to 0.1 % (1.000, 1.000, 1.000, 1.001, 1.000, 0.984; 12 layers 1.004).  No
# rounding the reference lacks shows in that.  The bar per batch size is the largest measured ratio x 1.25:
#   B = 1: 1.512 (d = 768, ffn = 9216, MHA, pos 37)   B = 7: 1.468 (d = 768, ffn = 1536, MHA, pos 0)
#   B = 32: 1.177 (12 layers, GQA, pos 511)
MEAN_RATIO = 1.0
MAX_RATIO_LOGITS = 1.0
MAX_RATIO_HIDDEN = {1: 1.25 * 1.512, 7: 1.25 * 1.468, 32: 1.25 * 1.177}


def _assert_ratios(r, B):
    for name, (r_mean, r_max, r_row) in r.items():
        bar = MAX_RATIO_LOGITS if name == "logits" else MAX_RATIO_HIDDEN[B]
        assert r_mean <= MEAN_RATIO, f"{name}: mean error {r_mean:.3f} x the CPU-bf16 oracle's"
        assert r_max <= bar, f"{name}: max error {r_max:.3f} x the CPU-bf16 oracle's (bar {bar:.2f})"
        # per row: a mean cannot see one bad row of 32 (the largest of these is the tensor's ratio; this names the row)
        for b, v in enumerate(r_row):
            assert v <= bar, f"{name}: the max error of row {b} is {v:.3f} x the reference gap's tensor maximum"


# (d, ffn): which instantiations the row is for.  QKV / out-projection / FFN1 run dec_gemm16_kernel<.., U> with
# U = d / 128; the LM-head dense (K = d) and FFN2 (K = ffn) go through a partial-tile producer and
# dec_finish_ln_kernel<KS>:
STEP_SHAPES = [
    (768, 3072),    # U = 6; head: gemm64p<6> 4 chunks, KS = 4;  FFN2: gemm64p<6> 16 chunks, KS = 16
    (512, 2048),    # U = 4; head: gemm64p<8> 2 chunks, KS = 4;  FFN2: gemm64p<8> 8 chunks, KS = 8
    (1024, 4096),   # U = 8; head: gemm64p<8> 4 chunks, KS = 4;  FFN2: gemm64p<8> 16 chunks, KS = 16
    (768, 1536),    # U = 6;                                     FFN2: gemm64p<6> 8 chunks, KS = 8
    (1024, 6144),   # U = 8;                                     FFN2: gemm64p<8> 24 chunks, KS = 24
    (768, 9216),    # U = 6; FFN2: no 64-column tiling (48 / 36 / 72 chunks): dec_gemm16<DEC_PART, 6>, 12 chunks, KS = 16
]


@pytest.mark.parametrize("attn", ["mha", "gqa"])
@pytest.mark.parametrize("d,ffn", STEP_SHAPES)
def test_step_against_fp64(d, ffn, attn):
    """2-layer models, B in {1, 7, 32} x pos in {0, 37, 95}, 96-slot cache: per tensor the mean and the maximum error
    against fp64 are within the margins above of the CPU-bf16 oracle's; per row no maximum exceeds the reference gap's
    tensor maximum by more than the tensor's own margin."""
    hk = d // 64 if attn == "mha" else d // 64 // 4
    for B in (1, 7, 32):
        for pos in (0, 37, 95):
            _assert_ratios(_step_ratios(d, ffn, 2, hk, B, pos, cap=96), B)


@pytest.mark.parametrize("attn", ["mha", "gqa"])
@pytest.mark.parametrize("pos", [511, 639])
def test_step_at_the_benchmark_shape_against_fp64(attn, pos):
    """12 layers, d = 768, B = 32, 640-slot cache, 512 / 640 keys: the decode headline's own shape."""
    _assert_ratios(_step_ratios(768, 3072, 12, 12 if attn == "mha" else 4, 32, pos, cap=640), 32)


# ---- the step does not depend on the environment ---------------------------------------------------------------
# The variables that once selected a decode kernel, a chain of the step or a measurement aid, each at its former
# non-default value.  Nothing reads them any more.
STALE_ENV = {"VY_DEC_WT": "1", "VY_DEC_P64": "0", "VY_DEC_LNFOLD": "0", "VY_DEC_ATTN": "0", "VY_DEC_ATTN_NT": "0",
             "VY_DEC_ATTN_GQ": "0", "VY_DECODE_LEAN": "0", "VY_GEMMA_LEAN": "0", "VY_GEMMA_FUSED": "2",
             "VY_GEMMA_ROPE_FUSED": "0", "VY_GEMMA_PRESCALE": "0", "VY_GREEDY_TWO_STAGE": "0"}


def _first_attn_case(dh, h, hk, nt):
    """The case of Part A with the smallest context (all of them in the first NP bucket) for these heads and K/V policy."""
    case = next(c for c in ATTN_CASES if c[:3] == (dh, h, hk) and c[4] == nt)
    assert expected_tuple(dh, h, hk, case[3], case[5])[1] == NP_BUCKETS[0]
    return case


def _child_main():
    """The (768, 3072), B = 32 step check and one Part-A case per family (each asserts which instantiation ran before it
    compares numbers), run as `python -m tests.test_decode_kernels_gpu` in a fresh process by
    test_step_does_not_depend_on_the_environment (such variables were read once per process)."""
    for hk in (12, 3):
        _assert_ratios(_step_ratios(768, 3072, 2, hk, 32, 37, cap=96), 32)
    for dh, h, hk, nt in ((64, 8, 2, 1),       # R = 4, streamed
                          (64, 12, 12, 0),     # small cache: default loads
                          (256, 8, 1, 0)):
        case = _first_attn_case(dh, h, hk, nt)
        assert expected_tuple(dh, h, hk, case[3], case[5]) == (dh, NP_BUCKETS[0], nt, 4 if nt and dh == 64 else 1)
        test_decode_attention_every_instantiation(*case)
    print("child ok")


def test_step_does_not_depend_on_the_environment():
    """With the old library every one of these would have changed what runs: the seven-link layer, dec_gemm16<DEC_PART>
    at d = 768, the general launchers, and FALLBACK or another tuple from vy_debug_decode_attn_last."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(STALE_ENV)
    r = subprocess.run([sys.executable, "-m", "tests.test_decode_kernels_gpu"], cwd=root, env=e, timeout=300,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- link level: the K / V rows the step writes, exact ----------------------------------------------------
def _link_case(d, hk, B, pos_kind, pos=37, cap=48):
    from tests.test_kernels_gpu import ints, assert_bf16_exact
    from oracle import vyom_oracle as O
    h = d // 64
    cfg, m, sd = _dec_model(d, 4 * d, 1, pos_kind, hk, 128)
    att = m.all_layer[0].attention
    # a ternary QKV weight and an integer bias (K = d <= 1024: dense), integer-valued input rows
    ws = {}
    with torch.no_grad():
        for i, name in enumerate(("query", "key", "value")):
            lin = getattr(att, name)
            ws[name] = (ints(*lin.weight.shape, seed=10 + i), ints(lin.weight.shape[0], seed=20 + i, lo=-2, hi=2))
            lin.weight.copy_(ws[name][0].to(BF))
            lin.bias.copy_(ws[name][1].to(BF))
    x = ints(B, d, seed=B)
    plan, cache, filled = _plan_and_cache(cfg, m, B, cap, pos, seed=3)
    plan.step(x.to(BF).to(DEV), pos)
    torch.cuda.synchronize()
    k_new = x @ ws["key"][0].t() + ws["key"][1]            # (B, hk * 64), exact in fp32
    v_new = x @ ws["value"][0].t() + ws["value"][1]
    assert_bf16_exact(k_new, "k")
    assert_bf16_exact(v_new, "v")
    kc, vc = cache.key_cache[0].cpu(), cache.value_cache[0].cpu()
    for c, (f, what) in zip((kc, vc), zip(filled[0], "kv")):
        keep = torch.ones(cap, dtype=torch.bool)
        keep[pos] = False
        assert torch.equal(c[:, :, keep].view(torch.int16), f[:, :, keep].view(torch.int16)), \
            f"{what} cache: a row other than {pos} changed"
    v_got = vc[:, :, pos].float().reshape(B, -1)
    assert torch.equal(v_got, v_new), f"v row: first wrong (b, col) {(v_got != v_new).nonzero()[0].tolist()}"
    k_got = kc[:, :, pos].float().reshape(B, -1)
    if pos_kind != "rope":
        assert torch.equal(k_got, k_new), f"k row: first wrong (b, col) {(k_got != k_new).nonzero()[0].tolist()}"
        return
    # rotary: the pre-rotation values a, b of a pair are exact integers, so only the rotation's own roundings remain.
    # The bf16 model (oracle.apply_rotary in bf16, and the kernel) multiplies by cos / sin rounded to bf16 and rounds
    # each product; the reference does the same (the products of an 8-bit integer and a bf16 number are exact before
    # that rounding) and adds them in fp64.  What is left is the one rounding of the sum at the store:
    # 2^-8 |a c +- b s| <= 2^-8 sqrt(2) max(|a|, |b|) < 2^-7 max(|a|, |b|)
    kh = k_new.double().view(B, hk, 1, 64)
    emb = torch.cat((O.rotary_angles(64, 128)[:, pos:pos + 1],) * 2, dim=-1)
    cos, sin = emb.cos().to(BF).double().unsqueeze(1), emb.sin().to(BF).double().unsqueeze(1)
    want = (kh * cos).to(BF).double() + (O.rotate_half(kh) * sin).to(BF).double()
    pair = torch.maximum(kh.abs(), O.rotate_half(kh).abs())
    err = (kc[:, :, pos:pos + 1].double() - want).abs()
    worst = float((err / (2.0 ** -7 * pair).clamp_min(1e-30)).max())
    print(f"rotary k row d={d} hk={hk} B={B}: max err / bound {worst:.3f}")
    assert (err <= 2.0 ** -7 * pair).all(), f"k row after rotary: max err / bound {worst:.3f}"


@pytest.mark.parametrize("pos_kind", ["absolute", "rope"])
@pytest.mark.parametrize("d", [512, 768, 1024])
def test_step_writes_exact_kv_rows(d, pos_kind):
    """One-layer models, d in {512, 768, 1024} (dec_gemm16_kernel<DEC_QKV, .., U = 4, 6, 8>), B in {1, 15, 16, 17, 32},
    hk in {h, h / 2, h / 4}: the K and V rows written at `pos` are bit-exact (with rotary: V exact, K within the
    rotation's own roundings), and every other cache row still holds the pattern it was filled with."""
    h = d // 64
    for hk in (h, h // 2, h // 4):
        for B in (1, 15, 16, 17, 32):
            _link_case(d, hk, B, pos_kind)


if __name__ == "__main__":
    _child_main()
