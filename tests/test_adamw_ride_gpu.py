"""AdamW riding in the grouped weight-gradient launch (vy_linear_wgrad_grouped_opt, ops.AdamWRide): the rider workgroups
run adamw_kernel's own update, so everything here is held to torch.equal against ops.adamw_step on cloned inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_kernels_gpu import rnd
from vyomai_amd import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CHUNK = 16384   # ADAMW_RIDE_CHUNK of vy_bwd.hip: the elements one rider workgroup steps


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _state(n, seed, shadow=True, lead=0):
    """p, g, m, v (+ shadow) of n elements that start `lead` elements into their allocations."""
    def mk(s, scale=1.0, positive=False):
        t = rnd(lead + n, seed=s) * scale
        return (t.abs() if positive else t).to(DEV)[lead:]
    p, g, m, v = mk(seed), mk(seed + 1, 0.1), mk(seed + 2, 0.01), mk(seed + 3, 1e-3, positive=True)
    pb = torch.zeros(lead + n, dtype=BF, device=DEV)[lead:] if shadow else None
    return [p, g, m, v, pb]


def _clone(st):
    return [None if t is None else t.clone() for t in st]


def _same(a, b, what):
    for name, x, y in zip("p g m v shadow".split(), a, b):
        if x is not None:
            assert torch.equal(x, y), (what, name, (x.float() - y.float()).abs().max().item())


def _hyper(step=1, wd=0.01, gs=1.0):
    return (5e-5, 0.9, 0.999, 1e-8, wd, step, gs)


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("step,wd,gs", [(1, 0.01, 1.0), (7, 0.0, 0.5)])
def test_rider_only_launches_give_adamw_steps_bits(step, wd, gs, shadow):
    """Every range length at which the rider takes another path (scalar tail only, one group of four, a partial pass, a
    whole chunk and a bit, several chunks), alone in a launch; then three ranges of different length in one launch."""
    from vyomai_amd import ops
    hy = _hyper(step, wd, gs)
    lengths = [1, 3, 4, CHUNK - 1, CHUNK + 5, 3 * CHUNK + 2]
    states = [_state(n, seed=100 + 10 * i, shadow=shadow) for i, n in enumerate(lengths)]
    refs = []
    for st in states:
        ref = _clone(st)
        ops.adamw_step(ref[0], ref[1], ref[2], ref[3], ref[4], *hy)
        refs.append(ref)
    together = [_clone(st) for st in states[2:5]]
    for n, st, ref in zip(lengths, states, refs):
        assert ops.linear_wgrad_grouped([ops.AdamWRide(*st, *hy)]) == [n]
        _same(st, ref, f"n = {n}")
    assert ops.linear_wgrad_grouped([ops.AdamWRide(*st, *hy) for st in together]) == lengths[2:5]
    for n, st, ref in zip(lengths[2:5], together, refs[2:5]):
        _same(st, ref, f"three ranges in one launch, n = {n}")


def test_a_range_that_starts_16_bytes_into_an_allocation():
    from vyomai_amd import ops
    hy = _hyper(3)
    st = _state(CHUNK + 9, seed=300, lead=4)   # (the shadow then starts 8 bytes in)
    assert st[0].data_ptr() % 128 == 16 and st[4].data_ptr() % 128 == 8
    ref = _clone(st)
    ops.adamw_step(*ref, *hy)
    assert ops.linear_wgrad_grouped([ops.AdamWRide(*st, *hy)]) == [CHUNK + 9]
    _same(st, ref, "lead 4")


def test_riders_beside_weight_gradients_and_column_sums():
    """2816 x 2816 at M = 2048: 121 tiles, two M-splits, 242 of 256 CUs -- 14 idle, so riders are taken.  The gradients
    start at zero, so the two fp32 atomics per element give the same bits in either order."""
    from vyomai_amd import ops
    M, D, W, N = 2048, 2816, 512, 768
    dy, x = rnd(M, D, seed=1).to(BF).to(DEV), rnd(M, D, seed=2).to(BF).to(DEV)
    ws = rnd(2 * W * N, seed=3).to(DEV)
    hy = _hyper(2)
    lens = [20005, 3 * CHUNK + 2]
    out = {}
    for ride in (False, True):
        dw = torch.zeros(D, D, dtype=torch.float32, device=DEV)
        db = torch.zeros(D, dtype=torch.float32, device=DEV)
        dg = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
        dbeta = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
        states = [_state(n, seed=400 + 10 * i) for i, n in enumerate(lens)]
        refs = [_clone(st) for st in states]
        entries = [(dy, x, dw, db), ops.ColSum(ws, dg, dbeta, True, BF)]
        if ride:
            entries += [ops.AdamWRide(*st, *hy) for st in states]
        taken = ops.linear_wgrad_grouped(entries)
        if ride:
            assert taken == lens, taken
            for st, ref in zip(states, refs):
                ops.adamw_step(*ref, *hy)
                _same(st, ref, "beside real work")
        else:
            assert taken is None
        out[ride] = (dw, db, dg, dbeta)
    for name, a, b in zip(("dw", "db", "dgamma", "dbeta"), out[False], out[True]):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    assert out[True][0].abs().max().item() > 1.0


def test_refusals_leave_every_buffer_untouched():
    from vyomai_amd import _lib, ops
    n = 4096
    st = _state(n + 8, seed=500)
    dw = torch.zeros(256, 256, dtype=torch.float32, device=DEV)
    db = torch.zeros(256, dtype=torch.float32, device=DEV)
    dy, x = rnd(512, 256, seed=5).to(BF).to(DEV), rnd(512, 256, seed=6).to(BF).to(DEV)
    ws = rnd(2 * 64 * 256, seed=7).to(DEV)
    dg, dbeta = torch.zeros(256, device=DEV), torch.zeros(256, device=DEV)
    buffers = st + [dw, db, ws, dg, dbeta]
    before = [t.clone() for t in buffers]
    desc = (_lib.VyWgradDesc * 1)()
    d = desc[0]
    d.dy, d.lddy, d.x, d.ldx, d.dw, d.lddw, d.db, d.M, d.N, d.K = (dy.data_ptr(), 256, x.data_ptr(), 256, dw.data_ptr(),
                                                                   256, db.data_ptr(), 512, 256, 256)
    cs = (_lib.VyColsumDesc * 1)()
    c = cs[0]
    c.ws, c.W, c.N, c.out0, c.out1, c.acc = ws.data_ptr(), 64, 256, dg.data_ptr(), dbeta.data_ptr(), 1
    base = dict(p=st[0].data_ptr(), g=st[1].data_ptr(), m=st[2].data_ptr(), v=st[3].data_ptr(), p_bf16=st[4].data_ptr(), n=n)

    def refused(match, nopt=1, step=1, real=False, **kw):
        opt = (_lib.VyAdamwRideDesc * 9)()
        for o in opt:
            for k, val in {**base, **kw}.items():
                setattr(o, k, val)
        hy = _lib.VyAdamwHyper(5e-5, 0.9, 0.999, 1e-8, 0.01, 1.0, step)
        with pytest.raises(_lib.VyomHipError, match=match):
            _lib.call("vy_linear_wgrad_grouped_opt", C.cast(desc, C.c_void_p) if real else None, 1 if real else 0,
                      C.cast(cs, C.c_void_p) if real else None, 1 if real else 0, C.cast(opt, C.c_void_p), nopt,
                      C.byref(hy), _lib.VY_BF16, ops._stream())

    refused("0..8 AdamW ranges", nopt=9)
    refused("bad arguments", n=0)
    refused("bad arguments", n=-4)
    for k in "pgmv":
        refused("bad arguments", **{k: None})
        refused("aligned", **{k: base[k] + 8})
    refused("aligned", p_bf16=base["p_bf16"] + 4)
    refused("step", step=0)
    for k in ("g", "p", "p_bf16"):
        for target in (dw, db, dg, dbeta, ws):
            refused("intersects", real=True, **{k: target.data_ptr() + 64})   # (the refusal comes before the pointer is used)
    torch.cuda.synchronize()
    for t, b in zip(buffers, before):
        assert torch.equal(t, b)


def _trainer(**kw):
    import vyomai_amd as V
    from vyomai_amd.training import FlatTrainer
    cfg = cases.with_kv(cases.test_cfg(), None)
    cfg.num_hidden_layers, cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size = 3, 512, 8, 2048
    cfg.hidden_dropout_prob, cfg.vocab_size = 0.0, 1000
    m = V.DecoderModel(cfg, "rope", None)
    recipe.load_recipe_(m)
    m = m.to(DEV).train()
    ids = T(recipe.token_ids("ride.ids", (8, 512), 3, cfg.vocab_size)).to(DEV)
    return m, FlatTrainer(m, bucket_bytes=4 << 20, **kw), ids


def _steps_match_adamw_step(m, tr, ids, steps, micro=1):
    """Each optimizer step against ops.adamw_step over snapshots, with the arena's gradients as they stand after it:
    independent of the order of the weight gradients' atomics; a parameter stepped twice or never is a mismatch."""
    from vyomai_amd import ops
    a = tr.arena
    stats = []
    for s in range(steps):
        ref = [a.master.clone(), None, tr.m.clone(), tr.v.clone(), a.shadow.clone()]
        for _ in range(micro):
            tr.train_step(lambda: m.clm_loss(ids, ids))
        torch.cuda.synchronize()
        assert tr.step_count == s + 1
        stats.append(dict(tr.ride_stats))
        scale_dev = None
        if tr.max_grad_norm is not None:
            scale_dev = torch.clamp(tr.max_grad_norm / (tr.last_grad_norm + 1e-6), max=1.0).to(torch.float32).reshape(1)
        for lo, hi in tr._ranges(0, a.numel, touched_only=True):
            ops.adamw_step(ref[0][lo:hi], a.grad[lo:hi], ref[2][lo:hi], ref[3][lo:hi], ref[4][lo:hi], tr.lr, *tr.betas,
                           tr.eps, tr.weight_decay, s + 1, 1.0, scale_dev=scale_dev)
        _same([a.master, None, tr.m, tr.v, a.shadow], ref, f"step {s + 1}")
    return stats


def test_trainer_rides_and_drains_and_every_parameter_is_stepped_once():
    from vyomai_amd import autograd_train as AT
    m, tr, ids = _trainer()
    assert tr._ride
    stats = _steps_match_adamw_step(m, tr, ids, 3)
    print("ride_stats per step:", stats)
    for st in stats:
        assert st["rode_ranges"] >= 1 and st["drained_ranges"] >= 1, st
        assert st["rode_bytes"] + st["drained_bytes"] <= tr.arena.numel * 30
    assert not AT._wgrad_group.rides


@pytest.mark.parametrize("kw", [dict(accumulate_steps=2), dict(max_grad_norm=1.0), dict(overlap_optimizer=False),
                                dict(adamw_ride=False)], ids=lambda kw: next(iter(kw)))
def test_configurations_that_stay_on_the_plain_path(kw):
    from vyomai_amd import autograd_train as AT
    m, tr, ids = _trainer(**kw)
    stats = _steps_match_adamw_step(m, tr, ids, 2, micro=kw.get("accumulate_steps", 1))
    for st in stats:
        assert st["rode_ranges"] == 0 and st["rode_bytes"] == 0, st
    assert not AT._wgrad_group.rides


def test_an_aborted_backward_leaves_no_pending_ranges():
    from vyomai_amd import autograd_train as AT
    m, tr, ids = _trainer()
    tr.zero_grad()
    tr.backward(m.clm_loss(ids, ids))
    assert not AT._wgrad_group.rides      # backward() itself steps what found no seat
    assert tr.ride_stats["rode_ranges"] >= 1 and tr.ride_stats["drained_ranges"] >= 1
    AT._wgrad_group.add_ride("left by a backward that raised", tr)
    tr.zero_grad()
    assert not AT._wgrad_group.rides
    _steps_match_adamw_step(m, tr, ids, 1)
