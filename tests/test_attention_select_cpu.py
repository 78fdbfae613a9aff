"""Guard of the selector regimes and budget bars (tests/attn_select.py): torch emulations of the dense forward and backward
with exactly the budgeted roundings -- bf16 P for the PV and dV products, bf16 dS, delta from the rounded forward output,
one rounding at each store, fp32 elsewhere -- and faults that can be switched in.  The faithful emulation sits at no more
than half of every bar on every case and regime; every fault that applies to a case lands outside a bar in at least one
regime of that case; on unit-normal data under the old bars a left-out last key goes unnoticed, which is why the regimes
and the bars exist.  No kernel runs here."""
import math

import pytest
import torch

from tests import attn_range as R
from tests import attn_select as A

BF = A.BF


# ---- the emulations ----------------------------------------------------------------------------------------------------------
def kv_heads(c, fault=None):
    """The KV head of every query head: i // (h / hk); the fault "kv_head_mod": i % hk."""
    i = torch.arange(c.h)
    return i % c.hk if fault == "kv_head_mod" else i // (c.h // c.hk)


def emulate_fwd(c, q, k, v, vis, kv_of):
    """Dense equivalent of the tile-wise kernels (the online rescale is a relative rounding of fp32 numbers: see
    tests/test_attention_range_cpu.py for the step-wise emulation).  vis (B, L, S).  -> out (B, L, h dh) in the storage
    type, lse (B, h, L) fp32.  Rows without a visible key: the column mean of V."""
    low = c.dtype == BF
    kf, vf = k.float()[:, kv_of], v.float()[:, kv_of]
    s = (q.float() @ kf.transpose(-1, -2)) * (1.0 / math.sqrt(c.dh))
    s = torch.where(vis[:, None], s, torch.tensor(float("-inf")))
    dead = ~vis.any(-1)[:, None].expand(c.B, c.h, c.L)
    m = torch.where(dead, torch.zeros(()), s.max(-1).values)
    p = torch.exp(s - m[..., None])
    l = torch.where(dead, torch.ones(()), p.sum(-1))
    o = (p.to(BF).float() if low else p) @ vf / l[..., None]
    o = torch.where(dead[..., None], vf.mean(2, keepdim=True).expand_as(o), o)
    return A.merge(o).to(c.dtype), m + torch.log(l)


def emulate_bwd(c, q, k, v, do, out, lse, vis_q, vis_kv, kv_of, store=True):
    """out, lse: what the forward stored.  vis_q / vis_kv: the visibility that the dQ pass and the dK/dV pass apply.
    bf16: a row without a visible key takes no part.  -> dq, dk, dv in the storage type (store=False: dq, dk before the
    store rounding)."""
    low = c.dtype == BF
    scale = 1.0 / math.sqrt(c.dh)
    qf, kf, vf = q.float(), k.float()[:, kv_of], v.float()[:, kv_of]
    dof, of = A.merge_inv(do.float(), c.h), A.merge_inv(out.float(), c.h)
    s = (qf @ kf.transpose(-1, -2)) * scale
    dP = dof @ vf.transpose(-1, -2)
    delta = (dof * of).sum(-1, keepdim=True)

    def p_ds(vis):
        p = torch.where(vis[:, None], torch.exp(s - lse[..., None]), torch.zeros(()))
        ds = p * (dP - delta)
        return (p.to(BF).float(), ds.to(BF).float()) if low else (p, ds)

    def group(t):       # (B, h, S, dh) -> (B, hk, S, dh), summed over the query heads of each KV head
        return torch.zeros(c.B, c.hk, c.S, c.dh).index_add_(1, kv_of, t)

    _, ds = p_ds(vis_q)
    dq = scale * (ds @ kf)
    p, ds = p_ds(vis_kv)
    dk = scale * group(ds.transpose(-1, -2) @ qf)
    dv = group(p.transpose(-1, -2) @ dof)
    if not store:
        return dq, dk, dv.to(c.dtype)
    return dq.to(c.dtype), dk.to(c.dtype), dv.to(c.dtype)


# ---- the faults ----------------------------------------------------------------------------------------------------------------
FWD_FAULTS = ("diag+1", "diag-1", "start-1", "last_key", "keypad+1", "keypad-1", "kv_head_mod", "v_block_rotated")
BWD_FAULTS = ("diag+1", "diag-1", "start-1", "last_key_dq", "last_key_dkdv", "keypad+1", "keypad-1", "kv_head_mod",
              "v_block_rotated", "dkdv_row_late")


def shifted(keypad, by):
    """The key-padding bytes read one key off: byte j is that of key j - by (the ends read as visible)."""
    out = torch.ones_like(keypad)
    if by > 0:
        out[:, by:] = keypad[:, :-by]
    else:
        out[:, :by] = keypad[:, -by:]
    return out


def rotate_v_block(c, v):
    """The V rows of one 16-key block rotated by one against K: the second block, or the first when S < 32."""
    k0 = 16 if c.S >= 32 else 0
    v = v.clone()
    v[:, :, k0:k0 + 16] = torch.roll(v[:, :, k0:k0 + 16], 1, 2)
    return v


def plan(c, f, fault):
    """-> None where the fault does not apply to the case (it changes nothing), else what the emulations take:
    vis_q, vis_kv, kv_of, v, late."""
    vis = A.visible(c, f.keypad)
    d = dict(vis_q=vis, vis_kv=vis, kv_of=kv_heads(c), v=f.v, late=False)
    if fault in ("diag+1", "diag-1"):
        if not c.causal:
            return None
        d["vis_q"] = d["vis_kv"] = A.visible(c, f.keypad, diag=1 if fault == "diag+1" else -1)
    elif fault == "start-1":
        if not (c.causal and c.start):
            return None
        d["vis_q"] = d["vis_kv"] = A.visible(c, f.keypad, diag=-1)
    elif fault in ("last_key", "last_key_dq", "last_key_dkdv"):
        dropped = A.visible(c, f.keypad, drop_last=True)
        if fault != "last_key_dkdv":
            d["vis_q"] = dropped
        if fault != "last_key_dq":
            d["vis_kv"] = dropped
    elif fault in ("keypad+1", "keypad-1"):
        if f.keypad is None:
            return None
        d["vis_q"] = d["vis_kv"] = A.visible(c, shifted(f.keypad, 1 if fault == "keypad+1" else -1))
    elif fault == "kv_head_mod":
        d["kv_of"] = kv_heads(c, fault)
    elif fault == "v_block_rotated":
        d["v"] = rotate_v_block(c, f.v)
    elif fault == "dkdv_row_late":
        d["late"] = True
    else:
        raise ValueError(fault)
    same = (d["vis_q"].equal(vis) and d["vis_kv"].equal(vis) and d["kv_of"].equal(kv_heads(c)) and d["v"] is f.v
            and not d["late"])
    return None if same else d


def run_fwd(c, f, d=None):
    """-> {"out": worst err / bar, "lse": ...} of the emulation under plan d (None: faithful)."""
    d = d or plan_faithful(c, f)
    out, lse = emulate_fwd(c, f.q, f.k, d["v"], d["vis_q"], d["kv_of"])
    return {"out": A.ratio(out, f.want_out, f.out_bar)[0], "lse": A.ratio(lse, f.want_lse, f.lse_bar, where=f.live)[0]}


def run_bwd(c, f, d=None):
    """The backward under plan d after a FAITHFUL forward: the backward tests have to catch a backward fault on their
    own.  -> {"dq": worst err / bar, "dk": ..., "dv": ...}"""
    fa = plan_faithful(c, f)
    out, lse = emulate_fwd(c, f.q, f.k, f.v, fa["vis_q"], fa["kv_of"])
    d = d or fa
    got = emulate_bwd(c, f.q, f.k, d["v"], f.do, out, lse, d["vis_q"], d["vis_kv"], d["kv_of"])
    if d["late"]:
        got = (got[0],) + tuple(torch.cat([torch.zeros_like(g[:, :, :1]), g[:, :, :-1]], 2) for g in got[1:])
    return {n: A.ratio(g, w, b)[0] for n, g, w, b in zip(("dq", "dk", "dv"), got, f.grads, f.bars)}


def plan_faithful(c, f):
    vis = A.visible(c, f.keypad)
    return dict(vis_q=vis, vis_kv=vis, kv_of=kv_heads(c), v=f.v, late=False)


def fmt(r):
    return ", ".join(f"{n} {x:.3g}" for n, x in r.items())


# ---- the generators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.FWD_CASES, ids=A.case_id)
def test_selector_rows_select(c):
    """ramp: every live row puts most of its weight on its last (ramp_desc: first) visible key -- more than 0.9 in 99 % of
    the rows (at dh = 256 the gap is 8 nat and the unit-normal rest of q k has sigma 1.4) --; pair: 0.5 on each target,
    which score exactly 3 amp, every other key at most 2 amp."""
    vis = A.visible(c, A.keypad_of(c.kp, c.B, c.S))
    live = vis.any(-1)
    idx = torch.arange(c.S)
    last = torch.where(vis, idx, torch.full((), -1)).max(-1).values
    first = torch.where(vis, idx, torch.full((), c.S)).min(-1).values
    for regime, key in (("ramp", last), ("ramp_desc", first)):
        if regime not in A.regimes_of(c):
            continue
        f = A.forward_problem(c, regime)
        w = f.p.gather(-1, key.clamp(0, c.S - 1)[:, None, :, None].expand(c.B, c.h, c.L, 1))[..., 0]
        w = w[live[:, None].expand_as(w)]
        assert bool((w > 0.5).all()) and float((w > 0.9).double().mean()) >= 0.99, (regime, float(w.min()))
    f = A.forward_problem(c, "pair")
    a, b = f.targets
    assert bool(((a >= 0) == live[:, None]).all())
    assert float((b >= 0).double().mean()) > (0.8 if c.S >= 64 else 0.25), "too few rows have a partner"
    s = f.q.double() @ R.rep(f.k.double(), c.h // c.hk).transpose(-1, -2)
    amp = A.pair_amp(c.dh)
    two = b >= 0
    for t in (a, b):
        st = s.gather(-1, t.clamp_min(0)[..., None])[..., 0]
        assert bool((st[two] == 3 * amp).all())
        wt = f.p.gather(-1, t.clamp_min(0)[..., None])[..., 0]
        assert bool(((wt[two] - 0.5).abs() < 1e-4).all())
    others = s.masked_fill(~vis[:, None], -1e30).scatter(-1, a.clamp_min(0)[..., None], -1e30).scatter(
        -1, b.clamp_min(0)[..., None], -1e30).max(-1).values
    assert bool((others[two] <= 2 * amp).all())


# ---- the faithful emulation and the faults -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.FWD_CASES, ids=A.case_id)
def test_forward_emulation_and_faults(c):
    caught = {fault: {} for fault in FWD_FAULTS}
    for regime in A.regimes_of(c):
        f = A.forward_problem(c, regime)
        r = run_fwd(c, f)
        print(f"{A.case_id(c)} {regime}: faithful {fmt(r)}")
        assert max(r.values()) <= 0.5, f"{regime}: the faithful emulation sits at {fmt(r)} of the bars"
        for fault in FWD_FAULTS:
            d = plan(c, f, fault)
            if d is not None:
                caught[fault][regime] = max(run_fwd(c, f, d).values())
    for fault, by in caught.items():
        if by:
            print(f"  {fault}: " + ", ".join(f"{r} {x:.3g}" for r, x in by.items()))
            assert max(by.values()) > 1.0, f"{fault} stays inside every bar in every regime: {by}"


@pytest.mark.parametrize("c", A.BWD_CASES, ids=A.case_id)
def test_backward_emulation_and_faults(c):
    caught = {fault: {} for fault in BWD_FAULTS}
    for regime in A.regimes_of(c):
        f = A.backward_problem(c, regime)
        for name, bar, want in zip(("dq", "dk", "dv"), f.bars, f.grads):
            if name in A.SHARP[regime]:
                share = A.sharp_share(bar, want)
                assert share >= 0.9, f"{regime} {name}: the bar is vacuous ({100 * share:.1f} % below 5 % of the largest)"
        r = run_bwd(c, f)
        print(f"{A.case_id(c)} {regime}: faithful {fmt(r)}")
        assert max(r.values()) <= 0.5, f"{regime}: the faithful emulation sits at {fmt(r)} of the bars"
        for fault in BWD_FAULTS:
            d = plan(c, f, fault)
            if d is not None:
                caught[fault][regime] = max(run_bwd(c, f, d).values())
    for fault, by in caught.items():
        if by:
            print(f"  {fault}: " + ", ".join(f"{r} {x:.3g}" for r, x in by.items()))
            assert max(by.values()) > 1.0, f"{fault} stays inside every bar in every regime: {by}"


@pytest.mark.parametrize("c", A.ROPE_CASES, ids=A.case_id)
def test_rope_inverse_bars(c):
    """dh = 64: the rotation acts on the fp32 accumulators and the result is rounded once; otherwise on the stored bf16
    gradients, rounded once more.  The fp32 tables of ops.rope_tables, restated."""
    f = A.backward_problem(c, "pair")
    inv_freq = 1.0 / (10000 ** (torch.arange(0, c.dh, 2).float() / c.dh))
    ang = torch.einsum("i,j->ij", torch.arange(192).float(), inv_freq)
    cos, sin = ang.cos(), ang.sin()
    fa = plan_faithful(c, f)
    out, lse = emulate_fwd(c, f.q, f.k, f.v, fa["vis_q"], fa["kv_of"])
    got = emulate_bwd(c, f.q, f.k, f.v, f.do, out, lse, fa["vis_q"], fa["vis_kv"], fa["kv_of"], store=c.dh != 64)
    wants = [A.rope_inverse(w, cos, sin, 3) for w in f.grads[:2]]
    bars = A.rope_bars(c, f.bars[:2], f.grads[:2], wants, cos, sin, 3)
    for name, g, want, bar, plain in zip(("dq", "dk"), got, wants, bars, f.grads):
        rot = A.rope_inverse(g.float(), cos, sin, 3).float().to(BF)
        r = A.ratio(rot, want, bar)[0]
        miss = A.ratio(A.rope_inverse(g.float(), cos, sin, 4).float().to(BF), want, bar)[0]
        print(f"{A.case_id(c)} {name}: faithful {r:.3g}, rotated by the next position's angle {miss:.3g}")
        assert r <= 0.5 and miss > 1.0
        assert A.sharp_share(bar, want) >= 0.9


def test_left_out_last_key_lands_far_outside_the_new_bars():
    """The figures that the old bars let through (next test), under the new ones: (1, 8, 1, 264, 264, 256), per regime."""
    c = next(x for x in A.BWD_CASES if x.S == 264)
    worst = {}
    for regime in A.regimes_of(c):
        f = A.backward_problem(c, regime)
        r = dict(run_fwd(c, f, plan(c, f, "last_key")))
        r["dq"] = run_bwd(c, f, plan(c, f, "last_key_dq"))["dq"]
        r.update({n: x for n, x in run_bwd(c, f, plan(c, f, "last_key_dkdv")).items() if n != "dq"})
        print(f"{regime}: {fmt(r)}")
        for n, x in r.items():
            worst[n] = max(worst.get(n, 0.0), x)
    assert all(worst[n] > 5.0 for n in ("out", "dq", "dk", "dv")), worst


def test_left_out_last_key_passes_the_old_bars_on_unit_normal_data():
    """(1, 2, 1, 264, 264, 256) causal, unit-normal bf16 data: a forward, a dQ pass and a dK/dV pass that leave out the last
    key of the ragged tile stay inside 2e-2 + 2e-2 |want| and 4e-2 + 3e-2 |want|, the bars of test_attention_fwd and
    test_attention_bwd."""
    c = A.Case("general", 1, 2, 1, 264, 264, 256, True, 0, None, BF)
    f = A.backward_problem(c, "normal")
    old_f = 2e-2 + 2e-2 * f.want_out.abs()
    old_b = [4e-2 + 3e-2 * w.abs() for w in f.grads]
    fa = plan_faithful(c, f)
    out_ok, lse_ok = emulate_fwd(c, f.q, f.k, f.v, fa["vis_q"], fa["kv_of"])
    d = plan(c, f, "last_key")
    out, lse = emulate_fwd(c, f.q, f.k, f.v, d["vis_q"], d["kv_of"])
    r = {"out": A.ratio(out, f.want_out, old_f)[0], "lse": A.ratio(lse, f.want_lse, 2e-2 + 1e-4 * f.want_lse.abs())[0]}
    got = emulate_bwd(c, f.q, f.k, f.v, f.do, out_ok, lse_ok, d["vis_q"], d["vis_kv"], d["kv_of"])
    r.update({n: A.ratio(g, w, b)[0] for n, g, w, b in zip(("dq", "dk", "dv"), got, f.grads, old_b)})
    print("left-out last key, err / old bar: " + fmt(r))
    assert all(r[n] <= 1.0 for n in ("out", "dq", "dk", "dv")), r
    new = dict(run_fwd(c, f, d))
    new.update(run_bwd(c, f, d))
    print("the same, err / new bar (the other regimes: the test above): " + fmt(new))
