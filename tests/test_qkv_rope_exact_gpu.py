"""vy_qkv_rope_fwd bit for bit on every GEMM route (tests/qkv_rope_rule.py: rule Q, quarter-turn tables, both dtypes;
rule R, real angles in bf16 arithmetic; the plain integer rule for the non-rotating twin of every case), the standalone
rotation and the rotary backward inside vy_attn_bwd under quarter turns.  No tolerance anywhere: every comparison is
check_exact."""
import functools

import pytest
import torch

from tests import qkv_rope_rule as R
from tests.test_kernels_gpu import check_exact, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
CASES = R.cases()


def _ops():
    from vyomai_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------
# vy_qkv_rope_fwd
# ---------------------------------------------------------------------------------------------------------------
def _shape(c):
    return (c["B"], c["L"], c["K"], c["h"], c["hk"], c["dh"], c["pos0"])


SHAPES = {_shape(c): c for c in CASES}


@functools.lru_cache(maxsize=None)
def _tables(shape, rule):
    c = SHAPES[shape]
    return (R.quarter_tables if rule == "Q" else R.real_tables)(R.table_rows(c), c["dh"])


@functools.lru_cache(maxsize=None)
def _expected(shape, rule):
    """q and the k / v caches of a shape under a rule (None: no rotation), computed once and shared: bf16 holds every
    expected value (integers up to 256, or bf16 results), which is asserted."""
    c = SHAPES[shape]
    cos, sin = _tables(shape, rule) if rule else (None, None)
    q, k, v = R.expect(c, cos, sin, rule or "Q")
    out = []
    for t in (q, R.in_cache(k, c), R.in_cache(v, c)):
        t16 = t.to(BF)
        assert torch.equal(t16.double(), t)
        out.append(t16)
    return tuple(out)


def _buffers(c):
    """-> (q, k, v) views to write and the (qbuf, kbuf, vbuf) allocations that hold them, all zero."""
    B, L, h, hk, dh, dt = c["B"], c["L"], c["h"], c["hk"], c["dh"], c["dtype"]
    cap = c["pos0"] + L + R.GUARD
    if c["store"] == "qpad":            # sequence stride dh + 4: no 16-byte rows
        qbuf = torch.zeros(B, h, L, dh + 4, dtype=dt, device=DEV)
        q = qbuf[..., :dh]
    else:
        q = qbuf = torch.zeros(B, h, L, dh, dtype=dt, device=DEV)
    kv = []
    for _ in range(2):
        if c["store"] == "kvpad":       # head stride cap * dh + 4: a multiple of 4 and not of 8
            buf = torch.zeros(B, hk, cap * dh + 4, dtype=dt, device=DEV)
            cache = buf[:, :, :cap * dh].view(B, hk, cap, dh)
            assert cache.stride(1) % 8 == 4 and cache.stride(0) % 4 == 0
        else:
            cache = buf = torch.zeros(B, hk, cap, dh, dtype=dt, device=DEV)
        kv.append((cache, buf))
    return (q, kv[0][0], kv[1][0]), (qbuf, kv[0][1], kv[1][1])


def _in_buffers(c, want):
    """The expected q / caches laid into zero buffers of the allocations' shapes: every guard element must be zero."""
    q, k, v = want
    B, hk, cap, dh = k.shape
    if c["store"] == "qpad":
        q = torch.cat((q, torch.zeros(*q.shape[:-1], 4, dtype=q.dtype)), dim=-1)
    if c["store"] == "kvpad":
        k, v = (torch.cat((t.reshape(B, hk, cap * dh), torch.zeros(B, hk, 4, dtype=t.dtype)), dim=-1) for t in (k, v))
    return q, k, v


def _launch(c, cos, sin):
    ops = _ops()
    x, w, b, _ = R.operands(c)
    dt, pos0, L = c["dtype"], c["pos0"], c["L"]
    views, bufs = _buffers(c)
    q, kc, vc = views
    args = (x.to(dt).to(DEV), w.to(dt).to(DEV), b.to(dt).to(DEV), c["h"], c["hk"], c["dh"],
            None if cos is None else cos.to(DEV), None if sin is None else sin.to(DEV), pos0, q,
            kc[:, :, pos0:pos0 + L], vc[:, :, pos0:pos0 + L])
    if c["ws"]:
        ops.qkv_rope(*args)
    else:
        # the stream's split-K workspace removed: one workgroup per tile walks all of K
        from vyomai_amd._lib import call
        st = torch.cuda.current_stream()
        call("vy_workspace_set", st.cuda_stream, None, 0)
        ops._WS.pop((st.device_index, st.cuda_stream), None)
        saved, ops._mid_ws = ops._mid_ws, lambda rows: None
        try:
            ops.qkv_rope(*args)
        finally:
            ops._mid_ws = saved
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_qkv_rope_exact(c):
    shape = _shape(c)
    rules = ["Q"] + (["R"] if c["dtype"] == BF else []) + [None]
    for rule in rules:
        cos, sin = _tables(shape, rule) if rule else (None, None)
        got = _launch(c, cos, sin)
        want = _in_buffers(c, _expected(shape, rule))
        rot = R.rotation(c["dh"], rule is not None, c["dtype"])
        what = f"{c['id']} rule {rule or 'plain'} [{R.route_of(c, rule is not None)}, rotation {rot}]"
        for g, w_, name in zip(got, want, ("q (b, head, l, d)", "k cache (b, head, row, d)", "v cache (b, head, row, d)")):
            check_exact(g, w_, f"{what} {name}")


# ---------------------------------------------------------------------------------------------------------------
# vy_rope_fwd, in place on the packed (B, L, (h + 2 hk) dh) buffer the dgrad consumes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("dh", [16, 40, 64, 72, 128, 256])
def test_rope_quarter_turns_exact(dtype, dh):
    ops = _ops()
    B, L, h, hk, pos0 = 2, 37, 3, 1, 7
    W = (h + 2 * hk) * dh
    x = rnd(B, L, W, seed=dh).to(dtype)
    cos, sin = R.quarter_tables(pos0 + L, dh)
    pos = pos0 + torch.arange(L)

    def heads(t):       # (B, L, W) -> the q and k heads (B, h + hk, L, dh): rows W apart, heads dh apart
        return t.view(B, L, h + 2 * hk, dh).permute(0, 2, 1, 3)[:, :h + hk]

    xh = heads(x).double()
    fwd = R.rotate(xh, cos, sin, pos)
    inv = R.rotate(xh, cos, sin, pos, inverse=True)
    assert float((fwd != xh).double().mean()) >= 1 / 3 and float((inv != fwd).double().mean()) >= 1 / 3
    cg, sg = cos.to(DEV), sin.to(DEV)
    for inverse, want in ((False, fwd), (True, inv)):
        buf = x.to(DEV).clone()
        ops.rope_(heads(buf), cg, sg, pos0, inverse=inverse)
        check_exact(heads(buf), want, f"rope_ dh {dh} inverse {inverse} (b, head, l, d)")
        check_exact(buf[..., (h + hk) * dh:], x[..., (h + hk) * dh:], "the v section")
        if not inverse:
            ops.rope_(heads(buf), cg, sg, pos0, inverse=True)
            check_exact(buf, x, f"rope_ dh {dh}: inverse after forward (b, l, column)")


# ---------------------------------------------------------------------------------------------------------------
# the rotary backward of vy_attn_bwd: fused into the dQ / dK stores at dh = 64 (attn_store_scaled_rope), a rotation
# launch behind the general and the fp32 kernels.  Under quarter turns it is a signed permutation of the pair, and
# rounding commutes with that: the call without tables, permuted on the CPU, is the expectation.
# ---------------------------------------------------------------------------------------------------------------
BWD_CASES = [  # B, h, hk, L, causal, keypad, dh, dtype
    (2, 4, 2, 96, True, False, 64, BF),
    (1, 2, 1, 200, True, False, 64, BF),
    (2, 3, 1, 70, False, True, 64, BF),
    (2, 12, 4, 131, False, True, 64, BF),
    (1, 4, 4, 257, True, False, 64, BF),
    (2, 4, 2, 90, True, True, 128, BF),
    (2, 4, 2, 70, True, False, 64, torch.float32),
]


@pytest.mark.parametrize("rp0", [0, 3], ids=["pos0", "pos3"])
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda t: "-".join(str(v).replace("torch.", "") for v in t))
def test_attention_bwd_rope_quarter_turns_exact(case, rp0):
    ops = _ops()
    B, h, hk, L, causal, use_kp, dh, dtype = case
    q, k, v = (rnd(B, n, L, dh, seed=s).to(dtype).to(DEV) for n, s in ((h, 1), (hk, 2), (hk, 3)))
    do = rnd(B, L, h * dh, seed=4).to(dtype).to(DEV)
    keypad = None
    if use_kp:
        keypad = torch.ones(B, L, dtype=torch.uint8)
        keypad[0, L - L // 3:] = 0
        if B > 1:
            keypad[1, L - 7:] = 0
        keypad = keypad.to(DEV)
    cos, sin = R.quarter_tables(rp0 + L, dh)
    lse = torch.zeros(B, h, L, dtype=torch.float32, device=DEV)
    out = ops.attention(q, k, v, causal=causal, keypad=keypad, lse=lse)

    def run(tables):
        dq = torch.zeros(B, h, L, dh, dtype=dtype, device=DEV)
        dk = torch.zeros(B, hk, L, dh, dtype=dtype, device=DEV)
        dv = torch.zeros_like(dk)
        kw = dict(cos=cos.to(DEV), sin=sin.to(DEV), rope_pos0=rp0) if tables else {}
        ops.attention_bwd(q, k, v, out, do, lse, dq, dk, dv, causal=causal, keypad=keypad, **kw)
        torch.cuda.synchronize()
        return dq.cpu(), dk.cpu(), dv.cpu()

    plain, rotated = run(False), run(True)
    pos = rp0 + torch.arange(L)
    for name, a, b in zip(("dq", "dk"), plain, rotated):
        want = R.rotate(a.double(), cos, sin, pos, inverse=True)
        assert float((want != a.double()).double().mean()) >= 1 / 3, name
        check_exact(b, want, f"{name} (b, head, l, d)")
    check_exact(rotated[2], plain[2], "dv (b, head, l, d)")
