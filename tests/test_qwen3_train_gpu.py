"""Qwen3Model training on the MI355X against the REAL reference's autograd (tests/golden/qwen3_train.npz, made by
make_golden_qwen3_train.py from the notebook's model): loss and every gradient through plain autograd and through
FlatTrainer, the padding mask, fp32 and bf16 trainer runs under AdamW, frozen scales, DPO, one block at the Qwen3-0.6B
widths against a plain-torch fp32 restatement, and the state dict on its way back into the served model."""
import math

import numpy as np
import pytest
import torch

import vyomai_amd as V
from tests.golden import cases_qwen3_train as C
from vyomai_amd import recipe
from vyomai_amd._lib import VyomHipError

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CASE_IDS = list(C.CASES)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got = got.detach().float().cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def build(case, dtype=torch.float32):
    return C.build(V.Qwen3Model, case, dtype).to(DEV)


def batch(case):
    return tuple(T(a).to(DEV) for a in C.train_batch(case))


def check_grads(m, g, prefix, bar, what, bars=None):
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        e = rel_err(C.sub_g(n, p.grad), g[f"{prefix}.d.{n}"])
        b = bar if bars is None else bars(n)
        print(f"{what} d {n}: rel_err {e:.3e} (bar {b:.1e})")
        assert e < b, (what, n, e, b)


def check_loss(loss, ref, bar, what):
    print(f"{what}: HIP {loss.item():.7f} reference {ref:.7f}")
    assert abs(loss.item() - ref) < bar * max(1.0, abs(ref)), (what, loss.item(), ref)


# ------------------------------------------------------------------------------------------
# fp32 loss and gradients
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", CASE_IDS)
def test_fp32_loss_and_gradients_through_plain_autograd(golden, case):
    g = golden("qwen3_train")
    m = build(case).train()
    ids, mask, labels = batch(case)
    loss = m.clm_loss(ids, labels)
    check_loss(loss, float(g[f"{case}.loss"]), 2e-5, f"{case} fp32 loss")
    loss.backward()
    check_grads(m, g, case, 1e-4, f"{case} autograd")
    if case in C.TIED:
        assert m.out_head.weight.grad is m.tok_emb.weight.grad


@pytest.mark.parametrize("case", CASE_IDS)
def test_fp32_gradients_in_the_trainers_arena(golden, case):
    """FlatTrainer: the gradients are written straight into the arena, the two qk-norm scales among them, and every
    parameter is reported to the reducer and counted exactly once -- the tied table (case t) by the last of its two
    writers, holding the vocabulary gradient and the embedding scatter."""
    from vyomai_amd.training import FlatTrainer
    g = golden("qwen3_train")
    m = build(case).train()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=torch.float32, overlap_optimizer=False)
    assert m.compute_dtype == torch.float32 and tr.arena.shadow is None
    ids, mask, labels = batch(case)
    tr.zero_grad()
    loss = m.clm_loss(ids, labels)
    check_loss(loss, float(g[f"{case}.loss"]), 2e-5, f"{case} fp32 loss (trainer)")
    tr.backward(loss)
    lo, hi = tr.arena.grad.data_ptr(), tr.arena.grad.data_ptr() + tr.arena.grad.numel() * 4
    for n, p in m.named_parameters():
        assert lo <= p.grad.data_ptr() < hi, n
    check_grads(m, g, case, 1e-4, f"{case} arena")
    # every parameter reported, counted once by the reducer (its _seen guard), and with that every bucket complete
    everyone = {id(p) for p in tr.arena.params}
    assert tr.reducer.touched == everyone and tr.reducer._seen == everyone
    assert tr.reducer._pending == tr.reducer.expect
    a = m.trf_blocks[0].att
    assert a.W_key.weight.grad.data_ptr() == a.W_query.weight.grad.data_ptr() + a.W_query.weight.numel() * 4   # adjacent


@pytest.mark.parametrize("case", CASE_IDS)
def test_padding_mask_gives_the_same_loss(golden, case):
    g = golden("qwen3_train")
    m = build(case)
    ids, mask, labels = batch(case)
    loss = m.clm_loss(ids, labels, attention_mask=mask)
    check_loss(loss, float(g[f"{case}.loss"]), 2e-5, f"{case} fp32 loss with the padding mask")
    loss.backward()
    check_grads(m, g, case, 1e-4, f"{case} masked")
    with torch.no_grad():
        val = m.clm_loss(ids, labels, attention_mask=mask)
    assert not val.requires_grad and abs(val.item() - loss.item()) < 1e-6 * max(1.0, abs(loss.item()))


# ------------------------------------------------------------------------------------------
# trainer runs
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", CASE_IDS)
def test_trainer_fp32_follows_reference_training(golden, case):
    from vyomai_amd.training import FlatTrainer
    g = golden("qwen3_train")
    m = build(case).train()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=torch.float32)
    ids, mask, labels = batch(case)
    for step in range(C.TRAIN_STEPS):
        loss = tr.train_step(lambda: m.clm_loss(ids, labels))
        check_loss(loss, float(g[f"{case}.train.loss"][step]), 2e-5, f"{case} step {step}")
    params = dict(m.named_parameters())
    for name in C.trained(case):
        w = C.sub_g(name, params[name].detach().float().cpu().numpy())
        wr = g[f"{case}.train.w.{name}"]
        print(f"{name}: mean |dw| {np.abs(w - wr).mean():.3e} max {np.abs(w - wr).max():.3e}")
        assert np.abs(w - wr).mean() < 2e-6, (name, np.abs(w - wr).mean())
        assert np.abs(w - wr).max() < 2 * 3 * C.LR + 1e-5, (name, np.abs(w - wr).max())
    # the state dict goes back into the model the engine serves, strictly
    fresh = C.build(V.Qwen3Model, case, torch.float32)
    res = fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(fresh.trf_blocks[1].ff.fc2.weight, m.trf_blocks[1].ff.fc2.weight.detach().cpu())
    served = V.Qwen3Model(C.cfg(case, BF))
    if case in C.TIED:
        served.tie_head()
    served.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    assert served.final_norm.scale.dtype == torch.float32 and served.tok_emb.weight.dtype == BF


@pytest.mark.parametrize("case", CASE_IDS)
def test_trainer_bf16_follows_reference_training(golden, case):
    """bf16 compute from FlatTrainer(model): the losses within 3e-2, and after the first backward every gradient within
    twice the reference's own bf16-versus-fp32 gap for that parameter (floor 3e-2): this path rounds q and k once, after
    the fp32 norm and rotation, where the reference rounds after each of its ops, so the two bf16 runs leave fp32 in
    different places."""
    from vyomai_amd.training import FlatTrainer
    g = golden("qwen3_train")
    m = build(case).train()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, overlap_optimizer=False)
    assert m.compute_dtype == BF and tr.arena.shadow is not None
    ids, mask, labels = batch(case)
    tr.zero_grad()
    loss = m.clm_loss(ids, labels)
    check_loss(loss, float(g[f"{case}.train.loss"][0]), 3e-2, f"{case} bf16 step 0")
    tr.backward(loss)
    check_grads(m, g, case, None, f"{case} bf16", bars=lambda n: max(3e-2, 2 * float(g[f"{case}.gap.d.{n}"])))
    tr.optimizer_step()
    for step in range(1, C.TRAIN_STEPS):
        loss = tr.train_step(lambda: m.clm_loss(ids, labels))
        check_loss(loss, float(g[f"{case}.train.loss"][step]), 3e-2, f"{case} bf16 step {step}")


# ------------------------------------------------------------------------------------------
# frozen scales, refused dtypes
# ------------------------------------------------------------------------------------------


def test_frozen_qk_scales_get_no_gradient(golden):
    from vyomai_amd.training import FlatTrainer
    g = golden("qwen3_train")
    case = "q"
    ids, mask, labels = batch(case)

    def frozen_model():
        m = build(case).train()
        frozen = [s for blk in m.trf_blocks for s in (blk.att.q_norm.scale, blk.att.k_norm.scale)]
        for s in frozen:
            s.requires_grad_(False)
        return m, frozen, [s.detach().clone() for s in frozen]

    m, frozen, before = frozen_model()
    m.clm_loss(ids, labels).backward()
    for s, b in zip(frozen, before):
        assert s.grad is None and torch.equal(s, b)
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert rel_err(C.sub_g(n, p.grad), g[f"{case}.d.{n}"]) < 1e-4, n
    # one frozen, one trained, in one block
    m.trf_blocks[0].att.k_norm.scale.requires_grad_(True)
    m.zero_grad(set_to_none=True)
    m.clm_loss(ids, labels).backward()
    a = m.trf_blocks[0].att
    assert a.q_norm.scale.grad is None
    assert rel_err(a.k_norm.scale.grad, g[f"{case}.d.trf_blocks.0.att.k_norm.scale"]) < 1e-4
    # under the trainer: the arena gradient of a frozen scale stays zero, and the step leaves the scale alone
    m, frozen, before = frozen_model()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=torch.float32, overlap_optimizer=False)
    tr.train_step(lambda: m.clm_loss(ids, labels))
    for s, b in zip(frozen, before):
        assert float(s.grad.abs().max()) == 0.0 and torch.equal(s.detach(), b)
    assert id(frozen[0]) not in tr.reducer.touched
    assert float(m.trf_blocks[0].att.W_key.weight.grad.abs().max()) > 0


def test_bf16_parameters_are_refused_for_training_and_score_under_no_grad(golden):
    g = golden("qwen3_train")
    case = "q"
    m = build(case, BF)
    ids, mask, labels = batch(case)
    with pytest.raises(VyomHipError, match=r"torch\.float32.*load_state_dict"):
        m.clm_loss(ids, labels)
    with pytest.raises(VyomHipError, match=r"torch\.float32"):
        m.sequence_logprobs(ids, mask.float())
    with torch.no_grad():
        val = m.clm_loss(ids, labels)
    check_loss(val, float(g[f"{case}.loss"]), 3e-2, "bf16 validation loss")
    with pytest.raises(ValueError, match="context_length"):
        with torch.no_grad():
            m.forward_hidden(torch.zeros((1, C.CASES[case]["context_length"] + 1), dtype=torch.long, device=DEV))


# ------------------------------------------------------------------------------------------
# DPO
# ------------------------------------------------------------------------------------------


def test_dpo_fp32_vs_reference(golden):
    from vyomai_amd.training import FlatTrainer
    g = golden("qwen3_train")
    case = C.DPO_CASE
    raw = C.dpo_batch(case)
    b = {k: T(v).to(DEV) for k, v in raw.items() if not k.endswith("_len")}
    pol = C.build_policy(V.Qwen3Model, case, torch.float32).to(DEV).train()
    ref = build(case)
    for who, mod in (("pi", pol), ("ref", ref)):
        for k in ("chosen", "rejected"):
            with torch.no_grad():
                lp = mod.sequence_logprobs(b[k], b[k + "_mask"])
            err = float((lp.double().cpu() - T(g[f"{case}.dpo.{who}.{k}"])).abs().max())
            print(f"{who}.{k} log-probs max abs err {err:.3e}")
            assert lp.dtype == torch.float32 and err < 2e-5, (who, k, err)
    for beta in C.BETAS:
        loss, rc, rr = pol.dpo_loss(b, ref, beta=beta)
        for what, got, want in (("loss", loss, g[f"{case}.dpo.loss.{beta}"]), ("chosen reward", rc, g[f"{case}.dpo.reward.chosen"]),
                                ("rejected reward", rr, g[f"{case}.dpo.reward.rejected"])):
            print(f"beta {beta} {what}: HIP {got.item():.7f} reference {float(want):.7f}")
            assert abs(got.item() - float(want)) < 2e-5, (beta, what)
        if beta == C.GRAD_BETA:
            loss.backward()
            check_grads(pol, g, f"{case}.dpo", 1e-4, "dpo")
    with torch.no_grad():
        ids, msk = torch.cat([b["chosen"], b["rejected"]]), torch.cat([b["chosen_mask"], b["rejected_mask"]])
        scores = ref.sequence_logprobs(ids, msk)
        quiet = pol.dpo_loss(b, ref, beta=1.0)
    pre = pol.dpo_loss(b, beta=1.0, ref_logprobs=(scores[:C.PAIRS], scores[C.PAIRS:]))
    with_model = pol.dpo_loss(b, ref, beta=1.0)
    for x, y, z in zip(pre, with_model, quiet):
        assert torch.equal(x.detach(), y.detach()) and torch.equal(y.detach(), z)
    assert not quiet[0].requires_grad and with_model[0].requires_grad
    # and it trains: one FlatTrainer step on the DPO loss
    tr = FlatTrainer(pol, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=torch.float32)
    first = tr.train_step(lambda: pol.dpo_loss(b, ref, beta=1.0)[0])
    second = tr.train_step(lambda: pol.dpo_loss(b, ref, beta=1.0)[0])
    assert abs(first.item() - float(g[f"{case}.dpo.loss.1.0"])) < 2e-5 and second.item() < first.item()


# ------------------------------------------------------------------------------------------
# one block at the Qwen3-0.6B widths
# ------------------------------------------------------------------------------------------


def _block_fp32(sd, x, h, hk, dh, eps, theta):
    """Plain-torch restatement of one Qwen3 block (pre-norm RMSNorm, GQA with the per-head RMSNorm of q and k in front
    of the rotate-half RoPE, causal softmax, SwiGLU) in fp32."""
    B, L, d = x.shape

    def rms(t, w):
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * w

    def rope(t):
        inv = 1.0 / (theta ** (torch.arange(0, dh, 2).float() / dh))
        ang = torch.outer(torch.arange(L).float(), inv)
        c, s = ang.cos(), ang.sin()
        a, b = t[..., :dh // 2], t[..., dh // 2:]
        return torch.cat([a * c - b * s, b * c + a * s], dim=-1)

    n = rms(x, sd["norm1.scale"])
    q = (n @ sd["att.W_query.weight"].T).view(B, L, h, dh).transpose(1, 2)
    k = (n @ sd["att.W_key.weight"].T).view(B, L, hk, dh).transpose(1, 2)
    v = (n @ sd["att.W_value.weight"].T).view(B, L, hk, dh).transpose(1, 2)
    q, k = rope(rms(q, sd["att.q_norm.scale"])), rope(rms(k, sd["att.k_norm.scale"]))
    k, v = k.repeat_interleave(h // hk, dim=1), v.repeat_interleave(h // hk, dim=1)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, h * dh)
    x = x + o @ sd["att.out_proj.weight"].T
    n = rms(x, sd["norm2.scale"])
    return x + (torch.nn.functional.silu(n @ sd["ff.fc1.weight"].T) * (n @ sd["ff.fc2.weight"].T)) @ sd["ff.fc3.weight"].T


def test_block_at_the_qwen3_0p6b_widths_vs_fp32_restatement():
    """One block at the Qwen3-0.6B widths (d = 1024, 16 heads over 8 KV groups, head_dim 128 so n_heads * head_dim = 2048,
    hidden 3072) on 4 x 512 rows, bf16 forward AND backward, fp32 parameters read through bf16 copies: the large-shape
    paths of the GEMMs, the grouped weight gradients, flash attention reading v as a strided view of the packed rows,
    and the two qk-norm kernels at 16 lanes per head.  Bars: those of
    test_layer_at_the_benchmark_size_vs_fp32_restatement (tests/test_causal_lm_gpu.py)."""
    from vyomai_amd.autograd_train import PreNormGatedMlpFn, PreNormQkNormAttentionFn
    from vyomai_amd.layers.mask import AttnMask
    from vyomai_amd.layers.positional_embeddings import RopeSlice
    h, hk, dh, theta = 16, 8, 128, 1e6
    cfg = dict(vocab_size=64, context_length=512, emb_dim=1024, n_heads=h, n_layers=1, hidden_dim=3072, head_dim=dh,
               qk_norm=True, n_kv_groups=hk, rope_base=theta, dtype=torch.float32)
    B, L, d = 4, 512, cfg["emb_dim"]
    model = V.Qwen3Model(cfg)
    blk = model.trf_blocks[0]
    with torch.no_grad():
        for n, p in blk.named_parameters():
            p.copy_(T(recipe.uniform("big.qwen3." + n, tuple(p.shape), 0.1, 1.0) if n.endswith(".scale")
                      else recipe.param_value("big.qwen3." + n, tuple(p.shape))))
    sd = {n: p.detach().clone().requires_grad_(True) for n, p in blk.named_parameters()}
    model = model.to(DEV).train()
    blk = model.trf_blocks[0]
    x0 = T(recipe.uniform("big.qwen3.x", (B, L, d))).to(BF)
    g0 = T(recipe.uniform("big.qwen3.gout", (B, L, d))).to(BF)
    x = x0.to(DEV).requires_grad_(True)
    a, ff = blk.att, blk.ff
    mask = AttnMask(causal=True, start_pos=0, query_len=L, key_len=L)
    y = PreNormQkNormAttentionFn.apply(x, a, mask, RopeSlice(model._rope, 0, L), blk.norm1.scale, blk.norm1.eps,
                                       a.out_proj.weight, a.q_norm.scale, a.k_norm.scale, a.q_norm.eps, *a._params())
    y = PreNormGatedMlpFn.apply(y, ff, blk.norm2.scale, blk.norm2.eps, ff.act, ff.fc1.weight, ff.fc2.weight, ff.fc3.weight)
    (y.float() * g0.to(DEV).float()).sum().backward()
    torch.cuda.synchronize()
    xr = x0.float().requires_grad_(True)
    yr = _block_fp32(sd, xr, h, hk, dh, blk.norm1.eps, theta)
    (yr * g0.float()).sum().backward()

    def rel(p, q):
        return float((p.detach().float().cpu() - q.detach()).abs().max() / (q.detach().abs().max() + 1e-12))

    def rel_rms(p, q):
        p, q = p.detach().float().cpu(), q.detach()
        return float((p - q).pow(2).mean().sqrt() / (q.pow(2).mean().sqrt() + 1e-12))
    print(f"y rel {rel(y, yr):.3e} rms {rel_rms(y, yr):.3e}; dx rel {rel(x.grad, xr.grad):.3e} rms {rel_rms(x.grad, xr.grad):.3e}")
    assert rel(y, yr) < 3e-2, rel(y, yr)
    assert rel_rms(y, yr) < 6e-3, rel_rms(y, yr)
    assert rel(x.grad, xr.grad) < 6e-2, rel(x.grad, xr.grad)
    assert rel_rms(x.grad, xr.grad) < 1.5e-2, rel_rms(x.grad, xr.grad)
    for n, p in blk.named_parameters():
        e = rel(p.grad, sd[n].grad)
        print(f"  d {n}: rel {e:.3e}")
        assert e < 6e-2, (n, e)
