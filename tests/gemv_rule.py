"""The single-sequence matrix-vector decode kernels held link by link: dec_gemv1_kernel<EPI, CH, NB, NORM> (vy_decode.hip,
B = 1) and the PRESCALED / GATED / rope forms of gemv_bf16_kernel (vy_gemm.hip, B <= 4).  Shared by
test_gemv_rule_cpu.py (an fp32 emulation of the kernels' arithmetic passes every rule, every planted mutation fails one)
and test_gemv_links_gpu.py (the kernels themselves, through the vy_debug_* wrappers).  Pure CPU.

Two rules for one output element against an fp64 reference `want`:

  exact   small-integer operands, no irrational factor: every partial sum is an integer far below 2^24, the expectation
          is <= 256 in magnitude (assert_bf16_exact), the result is bit-equal.
  round   |got - want| <= 1/2 ulp_bf16 + delta, the ulp of want's binade (or got's, when the two straddle a binade
          edge); delta is the fp32 error budget of the steps between the exact sum and the store, derived with a
          factor 2 over the count of roundings:
            NORM scale    2^-20 |want|   ms, rsqrtf + one Newton step, one product: at most 8 roundings of 2^-24
            gelu_tanh     2^-20 |g u|    absolute, because 1 + tanh cancels for negative gates
            rotary        2^-23 |want|   one fp32 add of two bf16-rounded products
          Where a value is rounded to bf16 in the MIDDLE of the chain (gate / up before the activation, the projection
          before the rotation) and is itself only known up to the round rule, the result is accepted if it meets the
          final rule for any admissible pair of rounded operands: RN(want - delta), RN(want + delta) each, at most four
          pairs.  (Adding the two budgets would be unsound: a rounding that tips moves the operand by a whole bf16 ulp.)
          Nothing is excluded from any comparison.

Gaussian operands hold the accumulation precision (the integer cases would pass a bf16 accumulator): the sum is within
K 2^-24 sum |w_k x_k| of exact, plain fp32 accumulation in any order, and the later steps are carried by their
Lipschitz constants (gauss_gated / gauss_rope below)."""
import math

import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import assert_bf16_exact, ints, thin_ternary

BF = torch.bfloat16
D_NORM, D_GELU, D_ROPE = 2.0 ** -20, 2.0 ** -20, 2.0 ** -23
EPS = 1e-6
SENTINEL = 0x7E57          # bf16 bit pattern of the guard tails
LEAN_K = (2048, 4096, 8192, 16384)
LEAN_INST = {2048: "4,1", 4096: "8,1", 8192: "8,2", 16384: "8,4"}
GEMMA_HEADS, HK_HEADS = (8, 1, 256), ((4, 2, 128), (2, 2, 64))
MUTATIONS = ("swap_gate_up", "up_at_n", "partner_xor1", "upper_sign", "ignore_c_sh", "mean_half", "no_eps",
             "skip_last_chunk", "bias_block_index", "no_proj_round", "no_gate_round")


# ---------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------
def rn(x):
    """fp64 -> nearest bf16 (ties to even), as fp64.  Every operand here has at most 24 significant bits or is a
    perturbed bound, so the step through fp32 costs nothing that matters."""
    return x.float().to(BF).double()


def ulp_bf16(v):
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 8)


def round_rule(got, want, delta):
    """-> (ok, ratio): ratio = (|got - want| - 1/2 ulp) / delta where delta > 0, else 0 (got must be the rounding)."""
    ulp = torch.maximum(ulp_bf16(want), ulp_bf16(got))
    over = (got - want).abs() - 0.5 * ulp
    ok = over <= delta
    ratio = torch.where(delta > 0, over / delta.clamp_min(1e-300), torch.zeros_like(over))
    return ok, ratio


def gelu64(x):
    return 0.5 * x * (1.0 + torch.tanh(0.79788456080286535588 * (x + 0.044715 * x ** 3)))


def _pairs(a, da, b, db):
    return [(x, y) for x in (rn(a - da), rn(a + da)) for y in (rn(b - db), rn(b + db))]


def _any_pair(got, pairs, f, budget):
    ok = torch.zeros_like(got, dtype=torch.bool)
    ratio = torch.full_like(got, float("inf"))
    for x, y in pairs:
        want = f(x, y)
        o, r = round_rule(got, want, budget(x, y, want))
        ok |= o
        ratio = torch.minimum(ratio, r)
    return ok, ratio


def gated_rule(got, g, dg, u, du):
    return _any_pair(got, _pairs(g, dg, u, du), lambda x, y: gelu64(x) * y, lambda x, y, w: D_GELU * (x * y).abs())


def rope_rule(got, a, da, b, db, c, s, sign):
    """a: this column's projection, b: its partner's, c / s: the bf16-rounded table entries, sign: -1 in the lower half
    of the head, +1 in the upper half (rope2_kernel: lo c - hi s, hi c + lo s, every product rounded to bf16)."""
    return _any_pair(got, _pairs(a, da, b, db), lambda x, y: rn(x * c) + sign * rn(y * s), lambda x, y, w: D_ROPE * w.abs())


def _half(v):
    return 0.5 * ulp_bf16(v.abs() + 2.0 ** -100)


def gauss_gated(got, g, dg, u, du):
    """The rounded gate is within Dg = dg + 1/2 ulp(|g| + dg) of g, the same for up; |gelu_tanh'| <= 1.13 and
    |gelu_tanh(x)| <= |x|: |gelu(g') u' - gelu(g) u| <= 1.13 Dg (|u| + Du) + |g| Du."""
    Dg, Du = dg + _half(g.abs() + dg), du + _half(u.abs() + du)
    want = gelu64(g) * u
    return round_rule(got, want, 1.13 * Dg * (u.abs() + Du) + g.abs() * Du + D_GELU * (g * u).abs())


def gauss_rope(got, a, da, b, db, c, s, sign):
    Da, Db = da + _half(a.abs() + da), db + _half(b.abs() + db)
    want = a * c + sign * b * s
    slack = Da * c.abs() + _half((a.abs() + Da) * c.abs()) + Db * s.abs() + _half((b.abs() + Db) * s.abs())
    return round_rule(got, want, slack + D_ROPE * (want.abs() + slack))


# ---------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------
def _case(fam, kind, K, M=1, norm=0, data="int", **kw):
    c = dict(fam=fam, kind=kind, K=K, M=M, norm=norm, data=data, bias=0, res=0, rope=0, pos=0, heads=None, N=0)
    c.update(kw)
    if kind == "qkv":
        h, hk, dh = c["heads"]
        c["N"] = (h + 2 * hk) * dh
    if fam == "lean":
        inst = "dec_gemv1_kernel<%s,%s,%s>" % ({"plain": "GV_PLAIN", "gated": "GV_GATED", "qkv": "GV_QKV"}[kind],
                                               LEAN_INST[K], "true" if norm else "false")
    else:
        inst = "gemv_bf16_kernel<%s,4,%s,%s>" % ({"plain": "0,NONE", "gated": "0,GELU_TANH", "qkv": "1,NONE"}[kind],
                                                 "true" if norm else "false", "true" if kind == "gated" else "false")
    tags = [inst, f"M{M}", f"K{K}", f"N{c['N']}", data]
    if kind == "qkv":
        tags += ["h%dx%dx%d" % c["heads"], f"rope{c['rope']}", f"pos{c['pos']}"]
    if c["bias"] or c["res"]:
        tags.append(f"bias{c['bias']}res{c['res']}")
    c["id"] = "-".join(tags)
    return c


def cases():
    out = []
    for K in LEAN_K:
        for N in (4, 1028):
            for br in (0, 1):
                out.append(_case("lean", "plain", K, N=N, bias=br, res=br))
        for I in (4, 516):
            for norm in (0, 1):
                out.append(_case("lean", "gated", K, N=I, norm=norm))
        for i, (norm, rope) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            out.append(_case("lean", "qkv", K, norm=norm, rope=rope, heads=GEMMA_HEADS, pos=37 * ((i + K // 2048) & 1)))
    for heads in HK_HEADS:          # hk > 1: the head stride of the cache matters
        for bias in (0, 1):
            for i, (norm, rope) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                out.append(_case("lean", "qkv", 2048, norm=norm, rope=rope, heads=heads, bias=bias, pos=37 * ((i + bias) & 1)))
    out.append(_case("lean", "gated", 2048, N=516, norm=1, data="eps"))
    out.append(_case("lean", "qkv", 2048, norm=1, rope=1, heads=(2, 2, 64), data="eps", pos=37))
    out.append(_case("lean", "gated", 16384, N=516, data="gauss"))
    out.append(_case("lean", "qkv", 2048, rope=1, heads=(4, 2, 128), data="gauss", pos=37))
    # B <= 4: K = 264 a lane tail inside the first 512, 2048 leaves u >= 4 clamped, 4104 a second trip with a tail
    for M in (1, 2, 3, 4):
        for K, heads in ((264, (2, 2, 64)), (2048, (4, 2, 128)), (4104, GEMMA_HEADS)):
            for P in (0, 1):
                out.append(_case("gemv", "plain", K, M=M, norm=P, N=70, bias=M & 1, res=M & 1))
                out.append(_case("gemv", "gated", K, M=M, norm=P, N=70))
                out.append(_case("gemv", "qkv", K, M=M, norm=P, rope=1, heads=heads, bias=(M + 1) & 1, pos=37 * (M & 1)))
    for P in (0, 1):                # EPI == 1 without the rotation: the scatter path
        out.append(_case("gemv", "qkv", 264, M=3, norm=P, rope=0, heads=(2, 2, 64), bias=1, pos=37))
    out.append(_case("gemv", "qkv", 264, M=2, norm=1, rope=1, heads=(2, 2, 64), data="eps", pos=37))
    out.append(_case("gemv", "gated", 264, M=2, N=70, norm=1, data="eps"))
    out.append(_case("gemv", "gated", 4104, M=4, N=70, data="gauss"))
    out.append(_case("gemv", "qkv", 2048, M=3, rope=1, heads=(4, 2, 128), data="gauss", pos=37))
    assert len({c["id"] for c in out}) == len(out)
    return out


def rope_tables(dh, max_pos):
    """fp32 cos / sin, (max_pos, dh / 2), evaluated on the host as vyomai_amd.ops.rope_tables does."""
    inv_freq = 1.0 / (10000 ** (torch.arange(0, dh, 2).float() / dh))
    ang = torch.einsum("i,j->ij", torch.arange(max_pos).float(), inv_freq)
    return ang.cos().contiguous(), ang.sin().contiguous()


CAP = 40                   # cache rows; positions 0 and 37


def layout(c):
    """Strides (in elements) of the buffers of a case."""
    L = dict(ldx=c["K"] + (8 if c["fam"] == "gemv" else 0), ldy=c["N"] + 8)
    if c["kind"] == "qkv":
        h, hk, dh = c["heads"]
        L.update(q_sb=h * dh + 8, c_sh=CAP * dh + 64)
        L["c_sb"] = hk * L["c_sh"] + 64
    return L


def make_inputs(c):
    """bf16 operands and the output buffers as they stand before the launch: guard tails of SENTINEL behind every
    output row, caches NaN-filled with a head stride larger than cap * dh."""
    K, M, N, kind = c["K"], c["M"], c["N"], c["kind"]
    seed = sum(map(ord, c["id"])) % 9973
    g = torch.Generator().manual_seed(seed)
    rows = 2 * N if kind == "gated" else N
    if c["data"] == "gauss":
        x = torch.randn(M, K, generator=g)
        w = torch.randn(rows, K, generator=g) / math.sqrt(K)
    else:
        x = ints(M, K, seed=seed)
        # gated: 9 weights kept per row, gate sums of standard deviation ~2, so that the activation is exercised where it
        # bends (check() asserts that a third of them lie in [-3, 3])
        w = thin_ternary(rows, K, K * 1024 / 9 if kind == "gated" else K, seed=seed + 1)
        if c["data"] == "eps":
            x = x * 2.0 ** -10      # mean x^2 ~ 0.64e-6 beside eps = 1e-6
    L = layout(c)
    X = torch.full((M, L["ldx"]), float("nan"), dtype=BF)
    X[:, :K] = x.to(BF)
    inp = dict(x=X, w=w.to(BF).contiguous(), L=L)
    if c["bias"]:
        inp["bias"] = ints(N, seed=seed + 2, lo=-2, hi=2).to(BF)
    if c["res"]:
        R = torch.full((M, L["ldy"]), float("nan"), dtype=BF)
        R[:, :N] = ints(M, N, seed=seed + 3, lo=-2, hi=2).to(BF)
        inp["res"] = R
    guard = torch.tensor(SENTINEL, dtype=torch.int16).view(BF)
    if kind == "qkv":
        h, hk, dh = c["heads"]
        inp["q"] = guard.repeat(M, L["q_sb"]).contiguous()
        inp["k"] = torch.full((M, L["c_sb"]), float("nan"), dtype=BF)
        inp["v"] = torch.full((M, L["c_sb"]), float("nan"), dtype=BF)
        if c["rope"]:
            inp["cos"], inp["sin"] = rope_tables(dh, CAP)
    else:
        inp["y"] = guard.repeat(M, L["ldy"]).contiguous()
    return inp


def outputs_of(c):
    return ("q", "k", "v") if c["kind"] == "qkv" else ("y",)


# ---------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in fp32 torch
# ---------------------------------------------------------------------------------------------------------------
def _r(t):
    return t.to(BF).float()


def _wave_sum(v):
    lanes = torch.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def lane_dot(x, w, skip_last=False):
    """One wave per row of w: lane l holds the 8 columns at 512 c + 8 l of chunk c and adds pairs of products into one
    fp32 sum, chunk after chunk; then the wave reduction.  (A K that is no multiple of 512 is padded with zeros: the
    lanes past the tail add nothing.)"""
    K = x.numel()
    Kp = -(-K // 512) * 512
    if Kp != K:
        x, w = F.pad(x, (0, Kp - K)), F.pad(w, (0, Kp - K))
    nch = Kp // 512
    xv, wv = x.float().view(nch, 64, 8), w.view(-1, nch, 64, 8)
    acc = torch.zeros(w.shape[0], 64)
    for ch in range(nch - (1 if skip_last else 0)):
        wc = wv[:, ch].float()
        for e in range(0, 8, 2):
            acc = acc + (wc[:, :, e] * xv[ch, :, e] + wc[:, :, e + 1] * xv[ch, :, e + 1])
    return _wave_sum(acc)


def gelu32(x):
    return 0.5 * x * (1.0 + torch.tanh(torch.tensor(0.79788456080286535588, dtype=torch.float32) * (x + 0.044715 * x * x * x)))


def emulate(c, inp, mut=None):
    """-> the output buffers after the launch.  mut: one of MUTATIONS, planted in the arithmetic or the addressing."""
    K, M, N, kind, L = c["K"], c["M"], c["N"], c["kind"], inp["L"]
    out = {k: inp[k].clone() for k in outputs_of(c)}
    skip = mut == "skip_last_chunk"
    for m in range(M):
        x = inp["x"][m, :K]
        acc = lane_dot(x, inp["w"], skip)
        if c["norm"]:
            sq = lane_dot(x, x[None], skip)[0]
            ms = sq / torch.tensor(float(K // 2 if mut == "mean_half" else K)) + (0.0 if mut == "no_eps" else torch.tensor(EPS))
            r = torch.rsqrt(ms)
            acc = acc * (r * (1.5 - 0.5 * ms * r * r))
        if kind == "plain":
            y = acc
            if "bias" in inp:
                y = y + inp["bias"].float()
            if "res" in inp:
                y = y + inp["res"][m, :N].float()
            out["y"][m, :N] = y.to(BF)
        elif kind == "gated":
            gate, up = acc[:N], acc[N:]
            if mut == "up_at_n":
                up = gate
            if mut == "swap_gate_up":
                gate, up = up, gate
            gate, up = (gate if mut == "no_gate_round" else _r(gate)), _r(up)
            out["y"][m, :N] = (gelu32(gate) * up).to(BF)
        else:
            h, hk, dh = c["heads"]
            nq, nkv, half = h * dh, hk * dh, dh // 2
            blk, wv = torch.arange(N // 4)[:, None], torch.arange(4)[None, :]
            n = blk * 4 + wv
            if c["rope"]:
                hd, pi = blk // (dh // 4), blk % (dh // 4)
                n = hd * dh + 2 * pi + (wv & 1) + half * (wv >> 1)
            xx = acc[n]
            if "bias" in inp:
                xx = xx + inp["bias"].float()[blk * 4 + wv if (mut == "bias_block_index" and c["rope"]) else n]
            if mut != "no_proj_round":
                xx = _r(xx)
            o = xx
            if c["rope"]:
                other = xx[:, [1, 0, 3, 2] if mut == "partner_xor1" else [2, 3, 0, 1]]
                d = (n % dh) % half
                cs, sn = _r(inp["cos"][c["pos"], d]), _r(inp["sin"][c["pos"], d])
                lower = (wv < 2).expand_as(n)
                sgn = torch.where(lower, -1.0, -1.0 if mut == "upper_sign" else 1.0)
                rot = _r(xx * cs) + _r(sgn * other * sn)
                o = torch.where(n < nq + nkv, rot, xx)
            n, o = n.reshape(-1), o.reshape(-1).to(BF)
            c_sh = 0 if mut == "ignore_c_sh" else L["c_sh"]
            dlow = n % dh
            isq, isk = n < nq, (n >= nq) & (n < nq + nkv)
            out["q"][m, n[isq]] = o[isq]
            koff = c["pos"] * dh + (n - nq) // dh * c_sh + dlow
            out["k"][m, koff[isk]] = o[isk]
            isv = ~isq & ~isk
            voff = c["pos"] * dh + (n - nq - nkv) // dh * c_sh + dlow
            out["v"][m, voff[isv]] = o[isv]
    return out


# ---------------------------------------------------------------------------------------------------------------
# the check: fp64 expectation, the rule of every output, untouched bits everywhere else
# ---------------------------------------------------------------------------------------------------------------
def _dot64(x, w, absolute=False, exact32=False):
    if exact32:     # integers (times a power of two): every partial sum is exact in fp32
        return (x.float() @ w.float().t()).double()
    x = x.double()
    parts = []
    for r0 in range(0, w.shape[0], 512):
        wc = w[r0:r0 + 512].double()
        parts.append((x.abs() @ wc.abs().t()) if absolute else (x @ wc.t()))
    return torch.cat(parts, dim=1)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _hold(ok, ratio, what, got, want):
    if not bool(ok.all()):
        idx = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((~ok).sum())}/{ok.numel()} outside the rule; first at {idx}: got "
                             f"{float(got[idx])!r} want {float(want[idx])!r} ratio {float(ratio[idx]):.3g}")
    return float(ratio.max()) if ratio.numel() else 0.0


def _exact(got, want, what):
    assert_bf16_exact(want, what)
    ok = got == want
    return _hold(ok, torch.zeros_like(want), what + " (exact)", got, want)


def check(c, inp, out):
    """Holds the output buffers of a case to the rules.  -> the worst (|got - want| - 1/2 ulp) / delta of the case."""
    K, M, N, kind, L = c["K"], c["M"], c["N"], c["kind"], inp["L"]
    what = c["id"]
    x = inp["x"][:, :K]
    gauss = c["data"] == "gauss"
    pre = _dot64(x, inp["w"], exact32=not gauss)
    dpre = torch.zeros_like(pre)
    if gauss:
        dpre = K * 2.0 ** -24 * _dot64(x, inp["w"], absolute=True)
    if c["norm"]:
        r = 1.0 / torch.sqrt((x.double() ** 2).mean(-1, keepdim=True) + float(torch.tensor(EPS)))
        pre = pre * r
        dpre = dpre * r + D_NORM * pre.abs()
    if "bias" in inp and kind != "gated":
        pre = pre + inp["bias"].double()
        if c["norm"] or gauss:
            dpre = dpre + 2.0 ** -23 * (pre.abs() + inp["bias"].double().abs())
    inexact = bool(c["norm"]) or gauss
    worst = 0.0
    written = {k: torch.zeros_like(inp[k], dtype=torch.bool) for k in outputs_of(c)}
    if kind == "plain":
        want, d = pre, dpre
        if "res" in inp:
            want = pre + inp["res"][:, :N].double()
            d = dpre + (2.0 ** -23 * (want.abs() + pre.abs()) if inexact else 0.0)
        got = out["y"][:, :N].double()
        worst = _hold(*round_rule(got, want, d), what, got, want) if inexact else _exact(got, want, what)
        written["y"][:, :N] = True
    elif kind == "gated":
        gt, up, dg, du = pre[:, :N], pre[:, N:], dpre[:, :N], dpre[:, N:]
        if c["data"] == "int":
            near = (_dot64(x, inp["w"][:N], exact32=True).abs() <= 3).double().mean().item()
            assert near >= 1 / 3, f"{what}: only {near:.2f} of the gate sums lie in [-3, 3]; the test data is wrong"
        got = out["y"][:, :N].double()
        rule = gauss_gated if gauss else gated_rule
        worst = _hold(*rule(got, gt, dg, up, du), what, got, gelu64(gt) * up)
        written["y"][:, :N] = True
    else:
        h, hk, dh = c["heads"]
        nq, nkv, half, pos = h * dh, hk * dh, dh // 2, c["pos"]

        def view(buf, heads, sb, sh, row):
            return buf.as_strided((M, heads, dh), (sb, sh, 1), row)

        got = {"q": view(out["q"], h, L["q_sb"], dh, 0), "k": view(out["k"], hk, L["c_sb"], L["c_sh"], pos * dh),
               "v": view(out["v"], hk, L["c_sb"], L["c_sh"], pos * dh)}
        view(written["q"], h, L["q_sb"], dh, 0)[:] = True
        for name in ("k", "v"):
            view(written[name], hk, L["c_sb"], L["c_sh"], pos * dh)[:] = True
        sect = {"q": (0, nq, h), "k": (nq, nq + nkv, hk), "v": (nq + nkv, N, hk)}
        for name, (n0, n1, heads) in sect.items():
            g_ = got[name].double()
            p_, d_ = pre[:, n0:n1].reshape(M, heads, dh), dpre[:, n0:n1].reshape(M, heads, dh)
            w_ = f"{what} {name}"
            if name == "v" or not c["rope"]:
                worst = max(worst, _hold(*round_rule(g_, p_, d_), w_, g_, p_) if inexact else _exact(g_, p_, w_))
                continue
            cs, sn = rn(inp["cos"][pos].double()), rn(inp["sin"][pos].double())
            lo, hi, dlo, dhi = p_[..., :half], p_[..., half:], d_[..., :half], d_[..., half:]
            rule = gauss_rope if gauss else rope_rule
            for gg, a, da, b, db, sign in ((g_[..., :half], lo, dlo, hi, dhi, -1.0), (g_[..., half:], hi, dhi, lo, dlo, 1.0)):
                worst = max(worst, _hold(*rule(gg, a, da, b, db, cs, sn, sign), w_, gg, a * cs + sign * b * sn))
    for k in outputs_of(c):
        same = (_bits(out[k]) == _bits(inp[k])) | written[k]
        assert bool(same.all()), f"{what}: {int((~same).sum())} elements of {k} outside the written row and columns changed"
    return worst
