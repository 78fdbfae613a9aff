"""Encoder LoRA fine-tuning for classification on the MI355X against the REAL reference's autograd through its own
EncoderModel and LoraLinear under a ClinicModel-shaped head (tests/golden/encoder_lora.npz,
make_golden_encoder_lora.py): two models (absolute positions + vanilla attention, RoPE + GQA), two adapters (n5: rank 32
on the notebook's five targets, n6: rank 8 on all six), lora_b non-zero, 51 rows -- a ragged last tile.

Bars.  fp32: loss 2e-5 relative, gradients rel_err < 1e-4, the trainer's steps as
test_causal_lm_gpu.test_trainer_fp32_follows_reference_training holds them -- the bars of test_lora_train_gpu.py, the
same arithmetic class.  bf16: loss 3e-2, each gradient within max(6e-2, 2 x the reference's OWN bf16-vs-fp32 gap for
that key); the maker asserts every gap below 3e-2, so the floor decides.  Wrapped vs merged: rel_err 2e-5.  Dropout:
bit-identical reruns, and 1e-5 against the same step through the three-launch composition."""
import copy

import numpy as np
import pytest
import torch

from tests.golden import cases_encoder_lora as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
COMBOS = [(model, who) for model in E.MODELS for who in E.ADAPTERS]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def build(model, compute=None, dropout=0.0):
    import vyomai_amd as V
    pos, attn = E.MODELS[model]
    c = E.cfg(model)
    c.hidden_dropout_prob = dropout
    m = V.EncoderForSequenceClassification(c, E.NUM_LABELS, pos_embedding_type=pos, attention_type=attn)
    E.load_weights_(m)
    m = m.to(DEV)
    if compute is not None:
        m.model.compute_dtype = compute
    return m


def wrapped(model, who, compute=None, dropout=0.0):
    """The notebook's order: the encoder frozen and wrapped, the head left trainable; then the fixture's values."""
    import vyomai_amd as V
    spec = E.ADAPTERS[who]
    m = build(model, compute, dropout)
    V.add_lora(m.model, rank=spec["rank"], alpha=spec["alpha"], targets=spec["on"])
    params = dict(m.named_parameters())
    with torch.no_grad():
        for k, v in E.adapter_state(model, who).items():
            params[k].copy_(T(v))
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == E.trained_keys(model, who)
    return m


def batch():
    return tuple(T(a).to(DEV) for a in E.batch())


def check_grads(m, g, tag, bar_of, what):
    errs, bad = {}, {}
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, f"{n}: a frozen parameter received a gradient"
            continue
        assert p.grad is not None, n
        errs[n] = rel_err(E.sub_g(p.grad.detach().float().cpu().numpy()), g[f"{tag}.d.{n}"])
        print(f"  {what} {tag}: d {n} rel_err {errs[n]:.3e} (bar {bar_of(n):.3e})")
        if not errs[n] < bar_of(n):
            bad[n] = errs[n]
    assert sorted(errs) == sorted(g[f"{tag}.keys"].tolist())
    assert not bad, (what, tag, bad)


@pytest.mark.parametrize("model,who", COMBOS)
def test_fp32_loss_and_gradients_vs_reference(golden, model, who, monkeypatch):
    from vyomai_amd import ops
    g = golden("encoder_lora")
    tag = f"{model}.{who}"
    m = wrapped(model, who).train()
    ids, mask, labels = batch()
    wgrads = []
    real = ops.linear_wgrad
    monkeypatch.setattr(ops, "linear_wgrad", lambda *a, **k: (wgrads.append(a[2].shape), real(*a, **k))[1])
    grouped = ops.linear_wgrad_grouped
    monkeypatch.setattr(ops, "linear_wgrad_grouped", lambda items: (wgrads.append(len(items)), grouped(items))[1])
    with torch.no_grad():
        logits = m(ids, mask)
    e = rel_err(logits, g[f"{tag}.logits"])
    print(f"{tag}: logits rel_err {e:.3e}")
    assert e < 2e-5, e
    ref = float(g[f"{tag}.loss"])
    # the fused head, then the notebook's own loop shape: logits from forward(), torch's loss of them
    for name, run in (("classification_loss", lambda: m.classification_loss(ids, mask, labels)),
                      ("forward + CrossEntropyLoss", lambda: torch.nn.CrossEntropyLoss()(m(ids, mask), labels))):
        m.zero_grad()
        loss = run()
        print(f"{tag} {name}: loss {loss.item():.7f} reference {ref:.7f}")
        assert abs(loss.item() - ref) <= 2e-5 * abs(ref), (name, loss.item(), ref)
        loss.backward()
        check_grads(m, g, tag, lambda n: 1e-4, name)
    assert wgrads == [], f"base weight gradients were launched: {wgrads}"


@pytest.mark.parametrize("model,who", COMBOS)
def test_bf16_loss_and_gradients_vs_reference(golden, model, who):
    g = golden("encoder_lora")
    tag = f"{model}.{who}"
    m = wrapped(model, who, compute=BF).train()
    ids, mask, labels = batch()
    ref = float(g[f"{tag}.loss"])
    loss = m.classification_loss(ids, mask, labels)
    print(f"{tag}: bf16 loss {loss.item():.5f} reference {ref:.5f}")
    assert abs(loss.item() - ref) < 3e-2 * max(1.0, abs(ref))
    loss.backward()
    check_grads(m, g, tag, lambda n: max(6e-2, 2.0 * float(g[f"{tag}.bf16_gap.{n}"])), "bf16")


@pytest.mark.parametrize("model,who", COMBOS)
def test_trainer_fp32_follows_reference_training(golden, model, who):
    from vyomai_amd.training import FlatTrainer
    g = golden("encoder_lora")
    tag = f"{model}.{who}"
    m = wrapped(model, who).train()
    tr = FlatTrainer(m, lr=E.LR, weight_decay=E.WEIGHT_DECAY, compute_dtype=torch.float32)
    frozen = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    ids, mask, labels = batch()
    for step in range(E.TRAIN_STEPS):
        loss = tr.train_step(lambda: m.classification_loss(ids, mask, labels))
        ref = float(g[f"{tag}.train.loss"][step])
        print(f"{tag} step {step}: HIP fp32 loss {loss.item():.7f}  reference loss {ref:.7f}")
        assert abs(loss.item() - ref) < 2e-5 * max(1.0, abs(ref)), (step, loss.item(), ref)
    params = dict(m.named_parameters())
    for n, before in frozen.items():
        assert torch.equal(params[n].detach(), before), f"{n}: a frozen parameter changed"
    for name in g[f"{tag}.keys"].tolist():
        w = E.sub_g(params[name].detach().float().cpu().numpy())
        wr = g[f"{tag}.train.w.{name}"]
        assert np.abs(w - wr).mean() < 2e-6, (name, np.abs(w - wr).mean())
        assert np.abs(w - wr).max() < 2 * 3 * E.LR + 1e-5, (name, np.abs(w - wr).max())


def test_full_fine_tuning_step_runs_without_adapters(golden):
    """vyom-ai-classification.ipynb: the same classifier, every weight trained; its logits are the fixture's base."""
    from vyomai_amd.training import FlatTrainer
    g = golden("encoder_lora")
    ids, mask, labels = batch()
    for model in E.MODELS:
        m = build(model).train()
        with torch.no_grad():
            e = rel_err(m(ids, mask), g[f"{model}.base.logits"])
        assert e < 2e-5, (model, e)
        tr = FlatTrainer(m, lr=E.LR, weight_decay=E.WEIGHT_DECAY, compute_dtype=torch.float32)
        losses = [tr.train_step(lambda: m.classification_loss(ids, mask, labels)).item() for _ in range(3)]
        print(f"{model}: full fine-tuning losses {losses}")
        assert losses[2] < losses[1] < losses[0]


def test_wrapped_vs_merged_and_disabled(golden):
    import vyomai_amd as V
    g = golden("encoder_lora")
    ids, mask, _ = batch()
    for model, who in COMBOS:
        m = wrapped(model, who).eval()
        merged = V.merge_lora(copy.deepcopy(m))
        assert not any(isinstance(x, V.LoraLinear) for x in merged.modules())
        with torch.no_grad():
            a, b = m(ids, mask), merged(ids, mask)
            base = build(model).eval()(ids, mask)
            with V.disable_lora(m):
                off = m(ids, mask)
        e = rel_err(a, b.cpu().numpy())
        print(f"{model}.{who}: wrapped vs merged logits rel_err {e:.3e}")
        assert e < 2e-5, e
        assert rel_err(a, base.cpu().numpy()) > 0.1 and rel_err(b, base.cpu().numpy()) > 0.1, "the adapter must move the logits"
        assert torch.equal(off, base), "under disable_lora the wrapped model computes the base model, bit for bit"
        assert rel_err(base, g[f"{model}.base.logits"]) < 2e-5


def _step(m, seed):
    from vyomai_amd import rng
    ids, mask, labels = batch()
    rng.manual_seed(seed)
    m.zero_grad()
    loss = m.classification_loss(ids, mask, labels)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("model,who", [("abs", "n5"), ("rope_gqa", "n6")])
def test_dropout_is_reproducible_and_the_delta_sits_inside_it(model, who, monkeypatch):
    """hidden_dropout_prob = 0.1 in train(): two runs from the same rng state give identical bits; the same step with
    `o` and `ffn2` computed by the three-launch composition -- plain GEMM, lora_delta_, vy_dropout, add -- gives the same
    adapter gradients in fp32 within 1e-5; with the delta added OUTSIDE the dropout it does not."""
    from vyomai_amd import encoder_lora_train as elt, ops
    from vyomai_amd.layers.attention import _shadow
    m = wrapped(model, who, dropout=0.1).train()
    l1, g1 = _step(m, 77)
    l2, g2 = _step(m, 77)
    assert torch.equal(l1, l2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    l3, _ = _step(m, 78)
    assert not torch.equal(l1, l3), "another seed: another mask"
    m.eval()
    le, _ = _step(m, 77)
    m.train()
    assert not torch.equal(l1, le), "train() drops, eval() does not"

    def composed(inside):
        def out_projection(G, x, w, b, residual, drop, us, g):
            dt = x.dtype
            z = torch.empty((*x.shape[:-1], w.shape[0]), dtype=dt, device=x.device)
            ops.linear(x, _shadow(w, dt), _shadow(b, dt), out=z)
            z2, x2 = z.view(-1, z.shape[-1]), x.view(-1, x.shape[-1])
            if G is None:
                return (ops.dropout(z, *drop) if drop is not None else z) + residual
            tiles, n = elt._tiles(z2.shape[0], z2.device)
            if inside:
                us[g] = ops.lora_delta_keep_u_(z2, x2, G.A, G.B, G.alpha, tiles, n, G.bounds)
                return (ops.dropout(z, *drop) if drop is not None else z) + residual
            y = ops.dropout(z, *drop) if drop is not None else z.clone()
            us[g] = ops.lora_delta_keep_u_(y.view(-1, y.shape[-1]), x2, G.A, G.B, G.alpha, tiles, n, G.bounds)
            return y + residual
        return out_projection

    monkeypatch.setattr(elt, "_out_projection", composed(True))
    lc, gc = _step(m, 77)
    worst = max(rel_err(g1[n], gc[n].cpu().numpy()) for n in g1)
    print(f"{model}.{who}: fused vs three-launch composition: loss {l1.item():.7f} / {lc.item():.7f}, worst gradient rel_err {worst:.3e}")
    assert abs(l1.item() - lc.item()) <= 1e-5 * abs(lc.item()) and worst < 1e-5, worst
    monkeypatch.setattr(elt, "_out_projection", composed(False))
    lo, go = _step(m, 77)
    outside = max(rel_err(g1[n], go[n].cpu().numpy()) for n in g1)
    print(f"{model}.{who}: delta outside the dropout: worst gradient rel_err {outside:.3e}")
    assert outside > 1e-3, "a delta behind the dropout is another function"


def test_refusals_on_the_device():
    import vyomai_amd as V
    from vyomai_amd._lib import VyomHipError
    ids, mask, labels = batch()
    m = wrapped("abs", "n5").train()
    layer = m.model.all_layer[0]
    x = torch.zeros(3, 17, 64, device=DEV)
    with pytest.raises(VyomHipError, match="applied by the EncoderLayer"):
        layer.attention(x, None)
    with pytest.raises(VyomHipError, match="applied by the EncoderLayer"):
        layer.feed_forward(x, x)
    with pytest.raises(VyomHipError, match="applied by the EncoderLayer"):
        layer.attention.out(x, x)
    layer.feed_forward.out.linear.weight.requires_grad_(True)
    with pytest.raises(VyomHipError, match="launches no base weight or bias gradient"):
        m.classification_loss(ids, mask, labels)
    layer.feed_forward.out.linear.weight.requires_grad_(False)
    layer.attention.key = V.DoraLinear(layer.attention.key, rank=8)
    with pytest.raises(VyomHipError, match="mixes LoRA and DoRA"):
        m.classification_loss(ids, mask, labels)
