"""The column sums of the LayerNorm backward (dgamma, dbeta) ride in the grouped weight-gradient launch
(vy_layernorm_bwd_partial + vy_linear_wgrad_grouped_cs) instead of two launches of their own per LayerNorm.  The
summation order is the one of vy_layernorm_bwd's own launches, so the results are held to torch.equal."""
import math

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_kernels_gpu import check, rnd
from vyomai_amd import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _ln_case(M, N, seed):
    dy, x = rnd(M, N, seed=seed).to(BF).to(DEV), rnd(M, N, seed=seed + 1).to(BF).to(DEV)
    gamma = (1.0 + 0.1 * rnd(N, seed=seed + 2)).to(BF).to(DEV)
    xf = x.float()
    mean = xf.mean(-1)
    rstd = torch.rsqrt(xf.var(-1, unbiased=False) + 1e-5)
    return dy, x, gamma, mean.contiguous(), rstd.contiguous()


def _reference(case, N, acc):
    """plain vy_layernorm_bwd onto 3.0-filled gradients -> (dx, dgamma, dbeta), computed once per case."""
    from vyomai_amd import ops
    dg = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
    db = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
    dx = ops.layernorm_bwd(*case, dg, db, accumulate=acc)
    return dx, dg, db


def _wgrad_items():
    items, wants = [], []
    for i, (M, N, K) in enumerate([(512, 256, 256), (300, 520, 264), (512, 256, 512), (64, 56, 8)]):
        dy, x = rnd(M, N, seed=40 + i).to(BF).to(DEV), rnd(M, K, seed=50 + i).to(BF).to(DEV)
        dw = torch.full((N, K), 3.0, dtype=torch.float32, device=DEV)
        items.append((dy, x, dw, None))
        wants.append((dy.double().t() @ x.double()).cpu() + 3.0)
    return items, wants


# 2048 x 768: 512 slab rows in 16 slices; 200 x 776: 50 slab rows, one slice, a ragged 64-column block (776 = 12 * 64 + 8)
@pytest.mark.parametrize("with_wgrads", [True, False])
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("M,N", [(2048, 768), (200, 776)])
def test_partial_plus_grouped_column_sums(M, N, acc, with_wgrads):
    from vyomai_amd import _lib, ops
    case = _ln_case(M, N, seed=7)
    dx_ref, dg_ref, db_ref = _reference(case, N, acc)
    dx, ws = ops.layernorm_bwd_partial(*case)
    assert ws.numel() == 2 * _lib.load().vy_layernorm_bwd_ws_rows(M) * N
    dg = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
    db = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
    items, wants = _wgrad_items() if with_wgrads else ([], [])
    ops.linear_wgrad_grouped(items + [ops.ColSum(ws, dg, db, acc, BF)])
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref)
    assert torch.equal(dg, dg_ref), (dg - dg_ref).abs().max().item()
    assert torch.equal(db, db_ref), (db - db_ref).abs().max().item()
    for (dy, x, dw, _), want in zip(items, wants):
        check(dw, want, 2e-3 * math.sqrt(dy.shape[0]), 1e-3, "dW next to the column sums")


def test_two_slabs_in_one_launch_and_the_fp32_path():
    """Two column-sum descriptors of different shapes in one launch (each workgroup finds its slab); and the fp32 path,
    where the sums stay launches of their own."""
    from vyomai_amd import ops
    entries, refs = [], []
    for (M, N), acc in (((2048, 768), True), ((200, 776), False)):
        case = _ln_case(M, N, seed=11)
        refs.append(_reference(case, N, acc))
        _, ws = ops.layernorm_bwd_partial(*case)
        dg = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
        db = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
        entries.append(ops.ColSum(ws, dg, db, acc, BF))
    ops.linear_wgrad_grouped(entries)
    for e, (_, dg_ref, db_ref) in zip(entries, refs):
        assert torch.equal(e.dgamma, dg_ref) and torch.equal(e.dbeta, db_ref)
    M, N = 200, 776
    dy, x, gamma, mean, rstd = _ln_case(M, N, seed=13)
    case = (dy.float(), x.float(), gamma.float(), mean, rstd)
    _, dg_ref, db_ref = _reference(case, N, True)
    _, ws = ops.layernorm_bwd_partial(*case)
    dg = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
    db = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
    ops.linear_wgrad_grouped([ops.ColSum(ws, dg, db, True, torch.float32)])
    assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref)


def test_decoder_backward_same_layernorm_gradients_and_every_parameter_ready_once():
    """One backward of a 2-layer decoder at 4 x 512 tokens with the column sums grouped, then with the launches of their own:
    every LayerNorm gradient bit for bit the same, and every parameter reported ready exactly once either way (the
    LayerNorm parameters only when the launch that holds their sums has been enqueued).  "Reported" is what the bucket
    reducer counts: a parameter is notified by its kernel's launch and again by autograd's own hook, and the reducer
    drops the repeat (BucketReducer.mark_ready) -- so a report is a notification of a parameter it has not seen yet.
    (While a parameter is deferred the hook's early notification is ignored, BucketReducer._hook: the raw number of
    notifications differs between the two paths by design.)"""
    import vyomai_amd as V
    from vyomai_amd import autograd_train as AT
    from vyomai_amd.training import FlatTrainer
    cfg = cases.with_kv(cases.test_cfg(), None)
    cfg.num_hidden_layers, cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size = 2, 512, 8, 2048
    cfg.hidden_dropout_prob, cfg.vocab_size = 0.0, 1000
    ids = T(recipe.token_ids("lncs.ids", (4, 512), 3, cfg.vocab_size)).to(DEV)
    ln_grads, partial_calls = {}, {}
    old = AT._GROUP_LN_COLSUMS
    real_partial = AT.ops.layernorm_bwd_partial
    try:
        for grouped in (True, False):
            m = V.DecoderModel(cfg, "rope", None)
            recipe.load_recipe_(m)
            m = m.to(DEV).train()
            tr = FlatTrainer(m, lr=1e-3, bucket_bytes=4 << 20)
            counts, early, calls = {}, [], []
            real_ready = tr.reducer.mark_ready

            def spy(p):
                if id(p) not in tr.reducer._seen:
                    counts[id(p)] = counts.get(id(p), 0) + 1
                if any(p is q for *_, members in AT._wgrad_group.colsums for q in members):
                    early.append(p)
                real_ready(p)

            tr.reducer.mark_ready = spy
            for p in tr.arena.params:
                p._vy_ready = spy
            AT._GROUP_LN_COLSUMS = grouped
            AT.ops.layernorm_bwd_partial = lambda *a: (calls.append(1), real_partial(*a))[1]
            tr.zero_grad()
            tr.backward(m.clm_loss(ids, ids))
            assert not AT._wgrad_group.items and not AT._wgrad_group.colsums and not AT._wgrad_group.armed
            torch.cuda.synchronize()
            partial_calls[grouped] = len(calls)
            assert not early, f"{len(early)} LayerNorm parameters were reported ready before their column sums were launched"
            wrong = {n: counts.get(id(p), 0) for n, p in tr.arena.items if p.requires_grad and counts.get(id(p), 0) != 1}
            assert not wrong, (grouped, wrong)
            assert not any(getattr(p, "_vy_deferred", False) for p in tr.arena.params)
            ln_grads[grouped] = {n: p.grad.clone() for n, p in tr.arena.items if "norm" in n.lower()}
    finally:
        AT._GROUP_LN_COLSUMS = old
        AT.ops.layernorm_bwd_partial = real_partial
    assert partial_calls[True] >= 4 and partial_calls[False] == 0, partial_calls   # 2 per layer at least
    assert ln_grads[True] and ln_grads[True].keys() == ln_grads[False].keys()
    for n, g in ln_grads[True].items():
        assert torch.isfinite(g).all() and torch.equal(g, ln_grads[False][n]), n
