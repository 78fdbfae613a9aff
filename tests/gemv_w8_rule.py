"""The fp8-weight forms of the single-sequence matrix-vector decode kernels held link by link:
dec_gemv1_w8_kernel<EPI, CH, NB, NORM> (vy_decode.hip, B = 1, W = e4m3fn codes with one fp32 scale per output row) and the
row quantiser vy_quant_rows_fp8 (vy_quant.hip).  Shared by test_gemv_w8_rule_cpu.py (an fp32 emulation of the kernels'
arithmetic passes every rule, every planted mutation fails one) and test_gemv_w8_links_gpu.py (the kernels themselves,
through the vy_debug_*_w8 wrappers).  Pure CPU.  The rules, the budgets of the steps after the wave sum, the buffer layout
and the guard tails are those of tests/gemv_rule.py, imported from there; what is new is the left end of the chain:

  y[n] = tail(scale[n] * sum_k value(code[n, k]) x[k])      the scale multiplies the wave sum, never an element

Four kinds of data, each with its own expectation for the scaled sum `want` (fp64):

  exact    ternary codes, integer x, scales 2^-(n % 3): every partial sum is an integer <= 255, the scaled result has at
           most 8 significant bits (checked on the data, element by element): bit-equal
  codes    weights drawn uniformly from the 64 codes with values in +-[1, 16) (multiples of 2^-3), thinned to 1024 per
           row, integer x, power-of-two scales: every partial sum is exact in fp32 in any order (17 bits): round rule
           with delta = 0
  onehot   K = 2048, N = 256: row n holds the single code n at column (37 n) % K (the two NaN codes 0x7F / 0xFF replaced
           by 0), x = 2 everywhere, scale 1: y[n] = 2 value(code), bit-equal, subnormals included
  gauss    Gaussian w quantised by the row rule, Gaussian x: delta = K 2^-24 sum |s c_k x_k| + 2^-23 |want| (fp32
           accumulation in any order, one product with the scale), then the NORM / gelu / rotary budgets unchanged

The quantiser's rule (include/vyom_hip.h), restated with an encoder written out in integer steps:
  s = amax > 0 ? amax / 448 : 1 ;  code = e4m3fn(clamp(w / s, -448, 448)), nearest even
and its error: |code * s - w| <= max(2^-4 |w|, 2^-10 s) (1 + 2^-22): 3 mantissa bits, subnormal step 2^-9."""
import math

import torch

from tests import gemv_rule as R
from tests.gemv_rule import (BF, CAP, D_NORM, EPS, GEMMA_HEADS, HK_HEADS, LEAN_K, SENTINEL, gated_rule, gauss_gated,  # noqa: F401
                             gauss_rope, gelu32, gelu64, layout, outputs_of, rn, rope_rule, rope_tables, round_rule)
from tests.test_kernels_gpu import ints, thin_ternary

F8 = torch.float8_e4m3fn
W8_INST = {2048: "2,1", 4096: "4,1", 8192: "4,2", 16384: "4,4"}
X_TAIL = 16                # NaN elements behind x
MUTATIONS = ("up_gate_scale", "scale_after_round", "scale_block_index", "drop_second_half", "swap_byte_pairs", "fnuz_bias",
             "skip_last_chunk")


# ---------------------------------------------------------------------------------------------------------------
# the quantiser
# ---------------------------------------------------------------------------------------------------------------
def encode_e4m3(q):
    """fp32 in [-448, 448] -> e4m3fn codes (uint8), round to nearest even, written out: below the smallest normal 2^-6
    the code is the count of 2^-9 steps (8 of them are the smallest normal itself), above it 3 mantissa bits of the
    binade, a mantissa that rounds up to 8 carrying into the exponent."""
    a = q.double().abs()
    assert float(a.max()) <= 448.0
    sub = torch.round(a * 512.0)                                   # torch.round: half to even
    m, e = torch.frexp(a.clamp_min(2.0 ** -6))                     # a = m 2^e, m in [0.5, 1)
    E = e - 1
    mant = torch.round((m * 2.0 - 1.0) * 8.0)
    E = torch.where(mant == 8, E + 1, E)
    mant = torch.where(mant == 8, torch.zeros_like(mant), mant)
    norm = (E + 7) * 8 + mant.long()
    code = torch.where(a < 2.0 ** -6, sub.long(), norm)
    return (code + 128 * torch.signbit(q).long()).to(torch.uint8)


def decode_e4m3(codes):
    return codes.contiguous().view(F8).float()


def quant_rows(w):
    """(N, K) fp32 (a bf16 matrix upcast) -> (codes uint8 (N, K), scales fp32 (N,)), every step in fp32 as the kernel."""
    w = w.float()
    amax = w.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / torch.tensor(448.0), torch.ones_like(amax))
    q = (w / s[:, None]).clamp(-448.0, 448.0)
    return encode_e4m3(q), s


def quant_error_ok(w, codes, s):
    w, s = w.double(), s.double()[:, None]
    err = (decode_e4m3(codes).double() * s - w).abs()
    return err <= torch.maximum(2.0 ** -4 * w.abs(), 2.0 ** -10 * s) * (1 + 2.0 ** -22)


# ---------------------------------------------------------------------------------------------------------------
# the case list: gemv_rule.cases() for the lean family, the data kinds above in place of its own
# ---------------------------------------------------------------------------------------------------------------
def _case(kind, K, data, norm=0, **kw):
    c = dict(fam="lean", kind=kind, K=K, M=1, norm=norm, data=data, bias=0, res=0, rope=0, pos=0, heads=None, N=0)
    c.update(kw)
    if kind == "qkv":
        h, hk, dh = c["heads"]
        c["N"] = (h + 2 * hk) * dh
    inst = "dec_gemv1_w8_kernel<%s,%s,%s>" % ({"plain": "GV_PLAIN", "gated": "GV_GATED", "qkv": "GV_QKV"}[kind], W8_INST[K],
                                              "true" if norm else "false")
    tags = [inst, f"K{K}", f"N{c['N']}", data]
    if kind == "qkv":
        tags += ["h%dx%dx%d" % c["heads"], f"rope{c['rope']}", f"pos{c['pos']}"]
    if c["bias"] or c["res"]:
        tags.append(f"bias{c['bias']}res{c['res']}")
    c["id"] = "-".join(tags)
    return c


def cases():
    out = []
    for c in R.cases():
        if c["fam"] != "lean":
            continue
        data = {"int": "exact", "eps": "eps", "gauss": "gauss"}[c["data"]]
        kw = {k: c[k] for k in ("bias", "res", "rope", "pos", "heads")}
        out.append(_case(c["kind"], c["K"], data, norm=c["norm"], N=c["N"], **kw))
    for K in LEAN_K:                # codes: one of each link per K, the larger N
        out.append(_case("plain", K, "codes", N=1028, bias=1, res=1))
        out.append(_case("gated", K, "codes", N=516, norm=(K // 2048) & 1))
        out.append(_case("qkv", K, "codes", norm=(K // 4096) & 1, rope=1, heads=GEMMA_HEADS, pos=37 * ((K // 2048) & 1)))
    out.append(_case("plain", 2048, "onehot", N=256))
    out.append(_case("plain", 4096, "gauss", N=1028, bias=1, res=1))
    out.append(_case("gated", 2048, "gauss", N=516, norm=1))
    out.append(_case("qkv", 8192, "gauss", norm=1, rope=1, heads=GEMMA_HEADS, pos=37))
    assert len({c["id"] for c in out}) == len(out)
    return out


def make_inputs(c):
    """bf16 x with NaN behind K, codes / scales / the codes' fp32 values, and the output buffers as they stand before the
    launch (gemv_rule's: SENTINEL guard tails, NaN-filled caches with an over-wide head stride)."""
    K, N, kind, data = c["K"], c["N"], c["kind"], c["data"]
    seed = sum(map(ord, c["id"])) % 9973
    g = torch.Generator().manual_seed(seed)
    rows = 2 * N if kind == "gated" else N
    scales = 2.0 ** -(torch.arange(rows) % 3).float()
    if data == "gauss":
        x = torch.randn(1, K, generator=g)
        codes, scales = quant_rows((torch.randn(rows, K, generator=g) / math.sqrt(K)).to(BF).float())
    elif data == "onehot":
        assert (K, N, kind) == (2048, 256, "plain")
        x = torch.full((1, K), 2.0)
        n = torch.arange(256)
        codes = torch.zeros(256, K, dtype=torch.uint8)
        codes[n, (37 * n) % K] = torch.where((n & 127) == 127, torch.zeros_like(n), n).to(torch.uint8)
        scales = torch.ones(256)
    else:
        x = ints(1, K, seed=seed)
        if data == "codes":
            idx = torch.randint(0, 32, (rows, K), generator=g)
            val = 2.0 ** (idx // 8).float() * (1.0 + (idx % 8).float() / 8.0)
            sign = 1.0 - 2.0 * torch.randint(0, 2, (rows, K), generator=g).float()
            keep = torch.rand(rows, K, generator=g) < 1024.0 / K
            val = val * sign * keep
        else:
            # gated: 9 weights kept per row, as gemv_rule does, so that the activation is exercised where it bends
            val = thin_ternary(rows, K, K * 1024 / 9 if kind == "gated" else K, seed=seed + 1)
            if data == "eps":
                x = x * 2.0 ** -10
        codes = val.to(F8).view(torch.uint8)
        assert torch.equal(decode_e4m3(codes), val)
    L = layout(c)
    X = torch.full((1, K + X_TAIL), float("nan"), dtype=BF)
    X[:, :K] = x.to(BF)
    inp = dict(x=X, codes=codes.contiguous(), scales=scales.float().contiguous(), wval=decode_e4m3(codes), L=L)
    if c["bias"]:
        inp["bias"] = ints(N, seed=seed + 2, lo=-2, hi=2).to(BF)
    if c["res"]:
        Rr = torch.full((1, L["ldy"]), float("nan"), dtype=BF)
        Rr[:, :N] = ints(1, N, seed=seed + 3, lo=-2, hi=2).to(BF)
        inp["res"] = Rr
    guard = torch.tensor(SENTINEL, dtype=torch.int16).view(BF)
    if kind == "qkv":
        h, hk, dh = c["heads"]
        inp["q"] = guard.repeat(1, L["q_sb"]).contiguous()
        inp["k"] = torch.full((1, L["c_sb"]), float("nan"), dtype=BF)
        inp["v"] = torch.full((1, L["c_sb"]), float("nan"), dtype=BF)
        if c["rope"]:
            inp["cos"], inp["sin"] = rope_tables(dh, CAP)
    else:
        inp["y"] = guard.repeat(1, L["ldy"]).contiguous()
    return inp


# ---------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in fp32 torch
# ---------------------------------------------------------------------------------------------------------------
def lane_dot_w8(x, wval, mut=None):
    """One wave per row: lane l holds the 16 codes at columns 1024 c + 16 l of chunk c (four dwords, the lowest byte
    first) and the matching 16 x, and adds the 16 products into one fp32 sum, chunk after chunk; then the wave sum."""
    nch = x.numel() // 1024
    xv, wv = x.float().view(nch, 64, 16), wval.view(-1, nch, 64, 16)
    if mut == "swap_byte_pairs":       # the two halves of every dword taken in the wrong order
        wv = wv.reshape(-1, nch, 64, 4, 2, 2).flip(4).reshape(-1, nch, 64, 16)
    if mut == "fnuz_bias":
        wv = wv * 2.0
    acc = torch.zeros(wv.shape[0], 64)
    for ch in range(nch - (1 if mut == "skip_last_chunk" else 0)):
        for e in range(8 if mut == "drop_second_half" else 16):
            acc = acc + wv[:, ch, :, e] * xv[ch, :, e]
    return R._wave_sum(acc)


def emulate(c, inp, mut=None):
    """-> the output buffers after the launch.  mut: one of MUTATIONS."""
    K, N, kind, L = c["K"], c["N"], c["kind"], inp["L"]
    out = {k: inp[k].clone() for k in outputs_of(c)}
    x, s = inp["x"][0, :K], inp["scales"]
    late = mut == "scale_after_round"
    raw = lane_dot_w8(x, inp["wval"], mut)
    rr = torch.tensor(1.0)
    if c["norm"]:
        sq = lane_dot_w8(x, x[None].float(), "skip_last_chunk" if mut == "skip_last_chunk" else None)[0]
        ms = sq / torch.tensor(float(K)) + torch.tensor(EPS)
        r = torch.rsqrt(ms)
        rr = r * (1.5 - 0.5 * ms * r * r)
    if kind == "plain":
        y = raw * (1.0 if late else s) * rr
        if "bias" in inp:
            y = y + inp["bias"].float()
        if "res" in inp:
            y = y + inp["res"][0, :N].float()
        out["y"][0, :N] = (y * s if late else y).to(BF)
    elif kind == "gated":
        sg, su = s[:N], (s[:N] if mut == "up_gate_scale" else s[N:])
        if late:
            gate, up = R._r(raw[:N] * rr) * sg, R._r(raw[N:] * rr) * su
        else:
            gate, up = R._r(raw[:N] * sg * rr), R._r(raw[N:] * su * rr)
        out["y"][0, :N] = (gelu32(gate) * up).to(BF)
    else:
        h, hk, dh = c["heads"]
        nq, nkv, half = h * dh, hk * dh, dh // 2
        blk, wv = torch.arange(N // 4)[:, None], torch.arange(4)[None, :]
        n = blk * 4 + wv
        if c["rope"]:
            hd, pi = blk // (dh // 4), blk % (dh // 4)
            n = hd * dh + 2 * pi + (wv & 1) + half * (wv >> 1)
        sn_ = s[blk * 4 + wv if mut == "scale_block_index" else n]
        xx = raw[n] * (1.0 if late else sn_) * rr
        if "bias" in inp:
            xx = xx + inp["bias"].float()[n]
        xx = R._r(xx)
        if late:
            xx = xx * sn_
        o = xx
        if c["rope"]:
            other = xx[:, [2, 3, 0, 1]]
            d = (n % dh) % half
            cs, sn = R._r(inp["cos"][c["pos"], d]), R._r(inp["sin"][c["pos"], d])
            sgn = torch.where((wv < 2).expand_as(n), -1.0, 1.0)
            o = torch.where(n < nq + nkv, R._r(xx * cs) + R._r(sgn * other * sn), xx)
        n, o = n.reshape(-1), o.reshape(-1).to(BF)
        dlow = n % dh
        isq, isk = n < nq, (n >= nq) & (n < nq + nkv)
        out["q"][0, n[isq]] = o[isq]
        koff = c["pos"] * dh + (n - nq) // dh * L["c_sh"] + dlow
        out["k"][0, koff[isk]] = o[isk]
        isv = ~isq & ~isk
        voff = c["pos"] * dh + (n - nq - nkv) // dh * L["c_sh"] + dlow
        out["v"][0, voff[isv]] = o[isv]
    return out


# ---------------------------------------------------------------------------------------------------------------
# the check: fp64 expectation, the rule of every output, untouched bits everywhere else
# ---------------------------------------------------------------------------------------------------------------
def _dot64(x, w):
    return torch.cat([x @ w[r0:r0 + 512].double().t() for r0 in range(0, w.shape[0], 512)], dim=1)


def _exact(got, want, what):
    """bit-equal, after the data itself is checked: every expected value must be a bf16 number"""
    assert torch.equal(rn(want), want), f"{what}: an expected value is not exact in bf16; the test data is wrong"
    return R._hold(got == want, torch.zeros_like(want), what + " (exact)", got, want)


def check(c, inp, out):
    """Holds the output buffers of a case to the rules.  -> the worst (|got - want| - 1/2 ulp) / delta of the case."""
    K, N, kind, L, data = c["K"], c["N"], c["kind"], inp["L"], c["data"]
    what = c["id"]
    x = inp["x"][:, :K].double()
    gauss = data == "gauss"
    s = inp["scales"].double()[None, :]
    pre = s * _dot64(x, inp["wval"])                       # fp64: s * sum c_k x_k
    dpre = torch.zeros_like(pre)
    if gauss:
        dpre = K * 2.0 ** -24 * s * _dot64(x.abs(), inp["wval"].abs()) + 2.0 ** -23 * pre.abs()
    if c["norm"]:
        r = 1.0 / torch.sqrt((x ** 2).mean(-1, keepdim=True) + float(torch.tensor(EPS)))
        pre = pre * r
        dpre = dpre * r + D_NORM * pre.abs()
    inexact = bool(c["norm"]) or gauss
    if "bias" in inp and kind != "gated":
        pre = pre + inp["bias"].double()
        if inexact:
            dpre = dpre + 2.0 ** -23 * (pre.abs() + inp["bias"].double().abs())
    # one rounding of an exactly known value: bit-equal where the value is a bf16 number by construction, else RN of it
    plain_rule = (lambda g_, w_, d_, t: R._hold(*round_rule(g_, w_, d_), t, g_, w_)) if (inexact or data == "codes") else \
                 (lambda g_, w_, d_, t: _exact(g_, w_, t))
    worst = 0.0
    written = {k: torch.zeros_like(inp[k], dtype=torch.bool) for k in outputs_of(c)}
    if kind == "plain":
        want, d = pre, dpre
        if "res" in inp:
            want = pre + inp["res"][:, :N].double()
            d = dpre + (2.0 ** -23 * (want.abs() + pre.abs()) if inexact else 0.0)
        got = out["y"][:, :N].double()
        worst = plain_rule(got, want, d, what)
        written["y"][:, :N] = True
    elif kind == "gated":
        gt, up, dg, du = pre[:, :N], pre[:, N:], dpre[:, :N], dpre[:, N:]
        if data == "exact":
            near = (gt.abs() <= 3).double().mean().item() if not c["norm"] else 1.0
            assert near >= 1 / 3, f"{what}: only {near:.2f} of the gate sums lie in [-3, 3]; the test data is wrong"
        got = out["y"][:, :N].double()
        rule = gauss_gated if gauss else gated_rule
        worst = R._hold(*rule(got, gt, dg, up, du), what, got, gelu64(gt) * up)
        written["y"][:, :N] = True
    else:
        h, hk, dh = c["heads"]
        nq, nkv, half, pos = h * dh, hk * dh, dh // 2, c["pos"]

        def view(buf, heads, sb, sh, row):
            return buf.as_strided((1, heads, dh), (sb, sh, 1), row)

        got = {"q": view(out["q"], h, L["q_sb"], dh, 0), "k": view(out["k"], hk, L["c_sb"], L["c_sh"], pos * dh),
               "v": view(out["v"], hk, L["c_sb"], L["c_sh"], pos * dh)}
        view(written["q"], h, L["q_sb"], dh, 0)[:] = True
        for name in ("k", "v"):
            view(written[name], hk, L["c_sb"], L["c_sh"], pos * dh)[:] = True
        sect = {"q": (0, nq, h), "k": (nq, nq + nkv, hk), "v": (nq + nkv, N, hk)}
        for name, (n0, n1, heads) in sect.items():
            g_ = got[name].double()
            p_, d_ = pre[:, n0:n1].reshape(1, heads, dh), dpre[:, n0:n1].reshape(1, heads, dh)
            w_ = f"{what} {name}"
            if name == "v" or not c["rope"]:
                worst = max(worst, plain_rule(g_, p_, d_, w_))
                continue
            cs, sn = rn(inp["cos"][pos].double()), rn(inp["sin"][pos].double())
            lo, hi, dlo, dhi = p_[..., :half], p_[..., half:], d_[..., :half], d_[..., half:]
            rule = gauss_rope if gauss else rope_rule
            for gg, a, da, b, db, sign in ((g_[..., :half], lo, dlo, hi, dhi, -1.0), (g_[..., half:], hi, dhi, lo, dlo, 1.0)):
                worst = max(worst, R._hold(*rule(gg, a, da, b, db, cs, sn, sign), w_, gg, a * cs + sign * b * sn))
    for k in outputs_of(c):
        same = (R._bits(out[k]) == R._bits(inp[k])) | written[k]
        assert bool(same.all()), f"{what}: {int((~same).sum())} elements of {k} outside the written row and columns changed"
    return worst
