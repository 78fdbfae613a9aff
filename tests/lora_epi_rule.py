"""vy_lora_expand_epi held to an fp64 restatement from the same storage-dtype inputs.  Shared by
test_encoder_lora_cpu.py (an fp32 emulation of the kernel's arithmetic passes the rule, a delta added behind the
epilogue fails it, and the restatement is the reference's LoraLinear in front of the activation) and
test_encoder_lora_kernels_gpu.py (the kernel itself).  Pure CPU.

The restatement (include/vyom_hip.h), everything in fp64 from z, u, B, res / mul as they are stored:
    v[t, n] = z[t, n] + alpha * sum_{j < r_pad} u[t, part(n) r_pad + j] B[n, j]
    ACT       out = act(v), pre = act'(v)
    DROP_RES  out = keep[t, n] ? v * scale + res : res, scale = fp32(1 / (1 - p)); p = 0: v + res
    MUL       out = v * mul

The bar, derived (eps = 2^-24, the unit roundoff of fp32; nothing below is fitted to what the kernel returns):
  1. the sum.  bf16 products are exact in fp32; an fp32 product is rounded once.  r_pad terms added in fp32 in ANY order
     are within r_pad eps S of the exact sum, S = sum_j |u_j B_j| (Higham's gamma_n to first order, n <= r_pad); the fp32
     products add one more eps S.                                         d_sum = (r_pad + 1) eps S
  2. v = fmaf(alpha, sum, z): one rounding.                              d_v = |alpha| d_sum + eps |v|
  3. ACT: |act(v') - act(v)| <= Lip(act) d_v, and the fp32 evaluation of act / act' itself: at most 16 roundings (erff /
     tanhf / expf count as 4 each at their documented <= 4 ulp), each relative to an intermediate no larger than
     max(1, |v|), doubled as tests/gemv_rule.py doubles its counts.         d_act = Lip d_v + 32 eps max(1, |v|)
     Lip(act) / Lip(act') = sup |act'| / sup |act''|: gelu 1.13 / 0.80 (both forms), silu 1.10 / 0.50, tanh 1 / 0.77,
     sigmoid 0.25 / 0.097, relu6 and leaky_relu 1 / piecewise constant -- their act' may take the value of either side of
     a kink that lies within d_v of v, and nothing else.
     DROP_RES: one product and one sum (or one fma).                        d_drop = scale d_v + 2 eps (|v scale| + |out|)
     A dropped element is res, bit for bit.
     MUL: one product.                                                    d_mul = |mul| d_v + eps |out|
  4. the store: half an ulp of the storage dtype at the larger of |want| and |got| (bf16: at most 2^-8 relative, fp32: eps).
A result passes when |got - want| <= d + half an ulp.  Nothing is excluded from any comparison."""
import math

import torch

BF = torch.bfloat16
EPS32 = 2.0 ** -24
ACT_NAMES = {1: "gelu_erf", 2: "gelu_tanh", 3: "silu", 4: "tanh", 5: "sigmoid", 6: "relu6", 7: "leaky_relu"}
LIP = {1: (1.13, 0.80), 2: (1.13, 0.80), 3: (1.10, 0.50), 4: (1.0, 0.77), 5: (0.25, 0.097), 6: (1.0, None), 7: (1.0, None)}
KINKS = {6: (0.0, 6.0), 7: (0.0,)}
LEAKY = 0.01
_C = 0.79788456080286535588


def act64(code: int, x: torch.Tensor) -> torch.Tensor:
    if code == 1:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if code == 2:
        return 0.5 * x * (1.0 + torch.tanh(_C * (x + 0.044715 * x ** 3)))
    if code == 3:
        return x * torch.sigmoid(x)
    if code == 4:
        return torch.tanh(x)
    if code == 5:
        return torch.sigmoid(x)
    if code == 6:
        return x.clamp(0.0, 6.0)
    if code == 7:
        return torch.where(x > 0, x, LEAKY * x)
    raise ValueError(code)


def act_grad64(code: int, x: torch.Tensor) -> torch.Tensor:
    if code == 1:
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if code == 2:
        t = torch.tanh(_C * (x + 0.044715 * x ** 3))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _C * (1.0 + 3.0 * 0.044715 * x * x)
    if code == 3:
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    if code == 4:
        return 1.0 - torch.tanh(x) ** 2
    if code == 5:
        s = torch.sigmoid(x)
        return s * (1.0 - s)
    if code == 6:
        return ((x > 0) & (x < 6)).double()
    if code == 7:
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, LEAKY))
    raise ValueError(code)


def part_of(N: int, bounds) -> torch.Tensor:
    n = torch.arange(N)
    p = torch.zeros(N, dtype=torch.long)
    for b in bounds:
        p += (n >= b).long()
    return p


def delta64(u, B, bounds, r_pad, absolute=False):
    """-> sum_j u[t, part(n) r_pad + j] B[n, j] in fp64 ((T, N)); absolute: the sum of the |products| (S above)."""
    u, B = u.double(), B.double()
    if absolute:
        u, B = u.abs(), B.abs()
    T, N = u.shape[0], B.shape[0]
    parts = part_of(N, bounds)
    out = torch.zeros((T, N), dtype=torch.float64)
    for p in range(int(parts.max()) + 1):
        cols = parts == p
        out[:, cols] = u[:, p * r_pad:(p + 1) * r_pad] @ B[cols].t()
    return out


def pre_sum(z, u, B, alpha, bounds, r_pad):
    """-> (v, d_v) of steps 1-2."""
    v = z.double() + alpha * delta64(u, B, bounds, r_pad)
    d_sum = (r_pad + 1) * EPS32 * delta64(u, B, bounds, r_pad, absolute=True)
    return v, abs(alpha) * d_sum + EPS32 * v.abs()


def half_ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - (9 if dtype == BF else 25))


def holds(got, want, d, dtype, what):
    """|got - want| <= d + half an ulp of the storage dtype -> the worst (|got - want| - half ulp) / d."""
    got, want = got.double(), want.double()
    over = (got - want).abs() - half_ulp(torch.maximum(got.abs(), want.abs()), dtype)
    ok = over <= d
    if not bool(ok.all()):
        idx = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((~ok).sum())}/{ok.numel()} outside the rule; first at {idx}: got "
                             f"{float(got[idx])!r} want {float(want[idx])!r} budget {float(d[idx]):.3e}")
    return float((over / d.clamp_min(1e-300)).clamp_min(0).max())


def check_act(code, h, pre, z, u, B, alpha, bounds, r_pad, dtype, what=""):
    v, dv = pre_sum(z, u, B, alpha, bounds, r_pad)
    lip, lip2 = LIP[code]
    ev = 32 * EPS32 * v.abs().clamp_min(1.0)
    what = f"{what} ACT {ACT_NAMES[code]}"
    worst = holds(h, act64(code, v), lip * dv + ev, dtype, what + " out")
    if lip2 is not None:
        return max(worst, holds(pre, act_grad64(code, v), lip2 * dv + ev, dtype, what + " pre"))
    # piecewise-constant derivative: the value at v, or that of the other side of a kink within d_v
    g = pre.double()
    ok = torch.zeros_like(g, dtype=torch.bool)
    for vv in (v, v - dv, v + dv):
        ok |= g == act_grad64(code, vv).to(dtype).double()
    assert bool(ok.all()), f"{what} pre: {int((~ok).sum())} derivatives are neither side's value"
    near = sum(int(((v - k).abs() <= dv).sum()) for k in KINKS[code])
    return max(worst, float(near > 0))


def check_drop_res(s, keep, p, z, u, B, alpha, bounds, r_pad, res, dtype, what=""):
    """keep: bool (T, N), the mask vy_dropout exports for the same (seed, offset); p = 0: all True."""
    v, dv = pre_sum(z, u, B, alpha, bounds, r_pad)
    scale = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))) if p > 0 else 1.0
    r = res.double()
    want = torch.where(keep, v * scale + r, r)
    d = torch.where(keep, scale * dv + 2 * EPS32 * ((v * scale).abs() + want.abs()), torch.zeros_like(v))
    assert torch.equal(s[~keep], res[~keep]), f"{what} DROP_RES: a dropped element is not the residual bit for bit"
    return holds(s, want, d, dtype, f"{what} DROP_RES p={p}")


def check_mul(out, z, u, B, alpha, bounds, r_pad, mul, dtype, what=""):
    v, dv = pre_sum(z, u, B, alpha, bounds, r_pad)
    want = v * mul.double()
    return holds(out, want, mul.double().abs() * dv + EPS32 * want.abs(), dtype, f"{what} MUL")


def derivation(r_pad: int, dtype) -> str:
    name = "bf16" if dtype == BF else "fp32"
    return (f"lora_epi_rule: r_pad = {r_pad}, {name}: d_v = |alpha| * {(r_pad + 1)} * 2^-24 * sum|u B| + 2^-24 |v|; "
            f"ACT d = Lip * d_v + 32 * 2^-24 * max(1, |v|); DROP_RES d = scale d_v + 2^-23 (|v scale| + |out|); "
            f"MUL d = |mul| d_v + 2^-24 |out|; + half an ulp of {name} (at most {'2^-8' if dtype == BF else '2^-24'} relative)")


# ---- the kernel's arithmetic in fp32 torch (CPU emulation; mutation: the delta behind the epilogue) ----------------
def emulate(mode, z, u, B, alpha, bounds, r_pad, dtype, code=None, res=None, keep=None, p=0.0, mul=None, mutate=False):
    acc = torch.zeros(z.shape, dtype=torch.float32)
    parts = part_of(B.shape[0], bounds)
    for q in range(int(parts.max()) + 1):
        cols = parts == q
        acc[:, cols] = u[:, q * r_pad:(q + 1) * r_pad].float() @ B[cols].float().t()
    al = torch.tensor(alpha, dtype=torch.float32)
    v = z.float() + al * acc
    if mode == "act":
        if mutate:      # what the causal LM's recipe would do: activation first, the delta added behind it
            return (act64(code, z.double()) + (al * acc).double()).float().to(dtype), act_grad64(code, z.double()).float().to(dtype)
        return act64(code, v.double()).float().to(dtype), act_grad64(code, v.double()).float().to(dtype)
    if mode == "drop_res":
        scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p)) if p > 0 else torch.tensor(1.0)
        if mutate:      # the delta outside the dropout
            return (torch.where(keep, z.float() * scale, torch.zeros(())) + al * acc + res.float()).to(dtype)
        return torch.where(keep, v * scale + res.float(), res.float()).to(dtype)
    return (v * mul.float()).to(dtype)


def make_inputs(T, N, bounds, r_pad, dtype, seed=0):
    """z, u, B, res ~ N(0, 1) scaled so that the delta is of z's size; a second (T, N) tensor for res / mul."""
    g = torch.Generator().manual_seed(1000 * T + N + r_pad + seed)
    parts = 1 + len(bounds)
    z = torch.randn(T, N, generator=g).to(dtype)
    u = torch.randn(T, parts * r_pad, generator=g).to(dtype)
    B = (torch.randn(N, r_pad, generator=g) / math.sqrt(r_pad)).to(dtype)
    other = torch.randn(T, N, generator=g).to(dtype)
    return z, u, B, other
