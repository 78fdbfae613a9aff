"""DoRA fine-tuning of ModelForCausalLM on the MI355X against the REAL reference's autograd through its own DoraLinear
(tests/golden/dora_train.npz, make_golden_dora_train.py): case "a" with the adapters d1 (rank 32 on six projections, the
k part of the packed QKV plain) and d2 (rank 8 on all seven) of cases_dora.py, dora_b non-zero and dora_m moved off its
initial value, everything frozen but dora_m / dora_a / dora_b.

Bars, those of test_lora_train_gpu.py.  fp32: test_causal_lm_gpu.py's test_model_fp32_vs_reference (loss 2e-5 relative,
gradients rel_err < 1e-4) and test_trainer_fp32_follows_reference_training.  bf16: the loss bar of
test_model_bf16_vs_reference; each gradient within max(6e-2, 2 x the reference's OWN bf16-vs-fp32 gap for that key) --
the factor 2 for the other accumulation order; the maker measured gaps up to 4.02e-2, so twice the gap decides the keys
whose gap exceeds 3e-2.  DPO: the fp32 loss bar of test_dpo_gpu.py.  Wrapped vs merged forward: rel_err 2e-5."""
import copy

import numpy as np
import pytest
import torch

from tests.golden import cases_causal_lm as C
from tests.golden import cases_dora as R
from tests.golden import cases_dpo as D
from tests.test_causal_lm_gpu import BF, DEV, T, build, rel_err

pytestmark = pytest.mark.gpu
WHO = tuple(R.ADAPTERS)
VOCAB = (R.KW["vocab_size"], R.KW["hidden_size"])
# the weight-gradient shapes of case "a", by group
GROUP_SHAPES = {"qkv": (512, 256), "o": (256, 256), "gate_up": (1024, 256), "down": (256, 512)}


def wrapped(who, compute=None, targets=None):
    """Case "a" with the adapter `who`: add_dora on its projections (or on `targets`), then the fixture's values."""
    import vyomai_amd as V
    spec = R.ADAPTERS[who]
    m = V.add_dora(build(C.CASES[R.CASE], compute=compute), rank=spec["rank"], targets=targets or spec["on"])
    state = R.adapter_state(who)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.requires_grad:
                p.copy_(T(state[n]))
    return m


def record_wgrads(monkeypatch):
    """ops.linear_wgrad / linear_wgrad_grouped record the (N, K) of every weight gradient they launch."""
    from vyomai_amd import ops
    shapes = []
    real, grouped = ops.linear_wgrad, ops.linear_wgrad_grouped
    monkeypatch.setattr(ops, "linear_wgrad", lambda *a, **k: (shapes.append(tuple(a[2].shape)), real(*a, **k))[1])

    def rec_grouped(items):
        shapes.extend(tuple(it[2].shape) for it in items if isinstance(it, tuple) and not hasattr(it, "_fields"))
        return grouped(items)
    monkeypatch.setattr(ops, "linear_wgrad_grouped", rec_grouped)
    return shapes


def check_dora_grads(m, g, who, bar_of, what):
    errs, bad = {}, {}
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, f"{n}: a frozen parameter received a gradient"
            continue
        assert p.grad is not None, n
        errs[n] = rel_err(C.sub_g(n, p.grad), g[f"{who}.d.{n}"])
        print(f"  {what} {who}: d {n} rel_err {errs[n]:.3e} (bar {bar_of(n):.3e})")
        if not errs[n] < bar_of(n):
            bad[n] = errs[n]
    assert sorted(errs) == sorted(g[f"{who}.keys"].tolist())
    assert not bad, (what, who, bad)


def groups_of(targets):
    from vyomai_amd.adapters import _CAUSAL_LM
    return [g for g, parts in _CAUSAL_LM.items() if any(p in targets for p in parts)]


@pytest.mark.parametrize("who", WHO)
def test_fp32_loss_and_gradients_vs_reference(golden, who, monkeypatch):
    g = golden("dora_train")
    m = wrapped(who).train()
    pids, pmask, plabels = (T(a).to(DEV) for a in C.padded_batch(R.CASE))
    ref = float(g[f"{who}.loss"])
    wgrads = record_wgrads(monkeypatch)
    layers = R.KW["num_hidden_layers"]
    for name, run in (("forward(labels)", lambda: m(input_ids=pids, attention_mask=pmask, labels=plabels, use_cache=False).loss),
                      ("clm_loss", lambda: m.clm_loss(pids, plabels, pmask))):
        m.zero_grad()
        del wgrads[:]
        loss = run()
        print(f"{who} {name}: loss {loss.item():.7f} reference {ref:.7f}")
        assert abs(loss.item() - ref) <= 2e-5 * abs(ref), (name, loss.item(), ref)
        loss.backward()
        check_dora_grads(m, g, who, lambda n: 1e-4, name)
        # weight gradients: exactly one per layer and group with a wrapped part -- so none for the vocabulary, whose
        # shape in case "a" is the packed QKV's (512, 256): the count of that shape is the layers', not one more
        want = sorted(GROUP_SHAPES[x] for x in groups_of(R.ADAPTERS[who]["on"])) * layers
        assert sorted(wgrads) == sorted(want), (name, wgrads)
        assert wgrads.count(VOCAB) == layers


def test_only_the_groups_with_a_wrapped_part_launch_a_weight_gradient(monkeypatch):
    m = wrapped("d2", targets=("self_attn.q_proj",)).train()
    pids, pmask, plabels = (T(a).to(DEV) for a in C.padded_batch(R.CASE))
    wgrads = record_wgrads(monkeypatch)
    m.clm_loss(pids, plabels, pmask).backward()
    assert wgrads == [GROUP_SHAPES["qkv"]] * R.KW["num_hidden_layers"], wgrads
    for n, p in m.named_parameters():
        assert (p.grad is not None and bool(p.grad.abs().max() > 0)) == p.requires_grad, n


@pytest.mark.parametrize("who", WHO)
def test_bf16_loss_and_gradients_vs_reference(golden, who):
    g = golden("dora_train")
    m = wrapped(who, compute=BF).train()
    pids, pmask, plabels = (T(a).to(DEV) for a in C.padded_batch(R.CASE))
    ref = float(g[f"{who}.loss"])
    loss = m.clm_loss(pids, plabels, pmask)
    print(f"{who}: bf16 fused loss {loss.item():.5f} reference {ref:.5f}")
    assert abs(loss.item() - ref) < 3e-2 * max(1.0, abs(ref))
    loss.backward()
    check_dora_grads(m, g, who, lambda n: max(6e-2, 2.0 * float(g[f"{who}.bf16_gap.{n}"])), "bf16 clm_loss")


def test_no_grad_forward_equals_the_merged_model():
    """Validation during fine-tuning: the wrapped model under no_grad (no KV cache) against merge_dora on a copy; the
    merged copy generates, the wrapped one refuses."""
    import vyomai_amd as V
    from vyomai_amd._lib import VyomHipError
    ids = T(C.ids(R.CASE)).to(DEV)
    with torch.no_grad():
        base = build(C.CASES[R.CASE]).eval()(input_ids=ids, use_cache=False).logits.float().cpu().numpy()
    for who in WHO:
        m = wrapped(who).eval()
        merged = V.merge_dora(copy.deepcopy(m))
        assert not any(isinstance(x, V.DoraLinear) for x in merged.modules())
        with torch.no_grad():
            a = m(input_ids=ids, use_cache=False).logits
            b = merged(input_ids=ids, use_cache=False).logits
        e = rel_err(a, b.float().cpu().numpy())
        print(f"{who}: wrapped vs merged logits rel_err {e:.3e}")
        assert e < 2e-5, e
        assert rel_err(a, base) > 0.1, "the adapter must move the logits"
        out = merged.generate(ids[:, :4], max_new_tokens=2)
        assert tuple(out.shape) == (ids.shape[0], 6)
        with pytest.raises(VyomHipError, match="merge_dora"):
            m.generate(ids[:, :4], max_new_tokens=2)
        with torch.no_grad(), pytest.raises(VyomHipError, match="merge_dora"):
            m(input_ids=ids[:, :4], past_key_values=merged(input_ids=ids[:, :4], use_cache=True).past_key_values)


def test_a_bare_dora_linear_call_is_the_composed_projection():
    import vyomai_amd as V
    m = wrapped("d2").eval()
    mod = m.model.layers[1].self_attn.v_proj
    x = torch.randn(3, 5, 256, generator=torch.Generator().manual_seed(4)).to(DEV)
    d = mod.linear.weight.double() + mod.dora_a.double() @ mod.dora_b.double()
    want = x.double() @ (d * (mod.dora_m.double() / (d * d).sum(dim=0).sqrt())).t() + mod.linear.bias.double()
    with torch.no_grad():
        got = mod(x)
        with V.disable_dora(m):
            plain = mod(x)
    assert rel_err(got, want.detach().cpu().numpy()) < 1e-5
    base = x.double() @ mod.linear.weight.double().t() + mod.linear.bias.double()
    assert rel_err(plain, base.detach().cpu().numpy()) < 1e-5, "disabled: the wrapped linear alone"


@pytest.mark.parametrize("who", WHO)
def test_dpo_loss_with_the_adapter_disabled_model_as_reference(golden, who):
    import vyomai_amd as V
    g = golden("dora_train")
    m = wrapped(who).train()
    batch = {k: T(v).to(DEV) for k, v in D.batch(R.CASE).items()}
    ids = torch.cat([batch["chosen"], batch["rejected"]], dim=0)
    mask = torch.cat([batch["chosen_mask"], batch["rejected_mask"]], dim=0)
    with V.disable_dora(m), torch.no_grad():
        ref = m.sequence_logprobs(ids, mask)
        base = build(C.CASES[R.CASE]).eval().sequence_logprobs(ids, mask)
    assert torch.equal(ref, base), "under disable_dora the wrapped model computes the base model"
    loss, _, _ = m.dpo_loss(batch, ref_logprobs=(ref[:D.PAIRS], ref[D.PAIRS:]), beta=D.GRAD_BETA)
    want = float(g[f"{who}.dpo.loss"])
    print(f"{who}: DPO loss {loss.item():.7f} reference {want:.7f}")
    assert abs(loss.item() - want) <= 2e-5 * max(1.0, abs(want)), (loss.item(), want)
    loss.backward()
    for n, p in m.named_parameters():
        assert (p.grad is not None and bool(p.grad.abs().max() > 0)) == p.requires_grad, n


@pytest.mark.parametrize("who", WHO)
def test_trainer_fp32_follows_reference_training(golden, who, monkeypatch):
    """Three FlatTrainer steps follow the reference's three torch.optim.AdamW steps on the adapter parameters, leave the
    base bitwise unchanged and the arena gradients of the frozen parameters zero; the weights are composed once per
    optimizer step and layer, however many forwards run between two steps."""
    from vyomai_amd import ops
    from vyomai_amd.training import FlatTrainer
    g = golden("dora_train")
    m = wrapped(who).train()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=torch.float32)
    frozen = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    ids, labels = (T(a).to(DEV) for a in C.train_batch(R.CASE))
    composes = []
    real = ops.dora_compose
    monkeypatch.setattr(ops, "dora_compose", lambda ps: (composes.append(len(ps)), real(ps))[1])
    per_layer = len(R.ADAPTERS[who]["on"])
    for step in range(C.TRAIN_STEPS):
        with torch.no_grad():       # a validation forward between two steps: nothing is composed again
            m.clm_loss(ids, labels)
        loss = tr.train_step(lambda: m.clm_loss(ids, labels))
        ref = float(g[f"{who}.train.loss"][step])
        print(f"{who} step {step}: HIP fp32 loss {loss.item():.7f}  reference loss {ref:.7f}")
        assert abs(loss.item() - ref) < 2e-5 * max(1.0, abs(ref)), (step, loss.item(), ref)
        assert composes == [per_layer] * (R.KW["num_hidden_layers"] * (step + 1)), composes
        for p, o in zip(tr.arena.params, tr.arena.offsets):
            if not p.requires_grad:
                assert not bool(tr.arena.grad[o:o + p.numel()].any()), "the arena gradient of a frozen parameter was written"
    params = dict(m.named_parameters())
    for n, before in frozen.items():
        assert torch.equal(params[n].detach(), before), f"{n}: a frozen parameter changed"
    for name in g[f"{who}.keys"].tolist():
        w = C.sub_g(name, params[name].detach().float().cpu().numpy())
        wr = g[f"{who}.train.w.{name}"]
        assert np.abs(w - wr).mean() < 2e-6, (name, np.abs(w - wr).mean())
        assert np.abs(w - wr).max() < 2 * 3 * C.LR + 1e-5, (name, np.abs(w - wr).max())


def test_trainer_bf16_steps_reduce_the_loss():
    """FlatTrainer(add_dora(model)) in bf16 compute: the composed weights are bf16, the master and the adapters fp32."""
    from vyomai_amd.training import FlatTrainer
    m = wrapped("d1").train()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=BF)
    ids, labels = (T(a).to(DEV) for a in C.train_batch(R.CASE))
    losses = [tr.train_step(lambda: m.clm_loss(ids, labels)).item() for _ in range(C.TRAIN_STEPS)]
    print(f"bf16 trainer losses {losses}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.3, losses


def test_the_grouped_weight_gradient_launch_gives_the_gradients_of_the_separate_ones(monkeypatch):
    """From 2048 rows on, the G of a group that the full-weight path would put into its grouped launch waits for ONE
    ops.linear_wgrad_grouped call a layer (case "a": the packed gate / up, the only group with 512 x 512 elements).  Both
    routes multiply the same bf16 operands and accumulate in fp32, in another order: the fp32 gradient bar, rel_err 1e-4,
    between them."""
    from vyomai_amd import autograd_train, ops
    ids = torch.randint(3, R.KW["vocab_size"], (17, 128), generator=torch.Generator().manual_seed(5)).to(DEV)   # 2176 rows
    grads, grouped = {}, []
    real = ops.linear_wgrad_grouped
    monkeypatch.setattr(ops, "linear_wgrad_grouped", lambda items: (grouped.append([tuple(it[2].shape) for it in items]),
                                                                      real(items))[1])
    for route, rows in (("grouped", autograd_train._GROUP_MIN_ROWS), ("separate", 10 ** 9)):
        monkeypatch.setattr(autograd_train, "_GROUP_MIN_ROWS", rows)
        m = wrapped("d1", compute=BF).train()
        m.clm_loss(ids, ids).backward()
        grads[route] = {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad}
    assert grouped == [[GROUP_SHAPES["gate_up"]]] * R.KW["num_hidden_layers"], grouped
    for n, got in grads["grouped"].items():
        e = rel_err(got, grads["separate"][n].float().cpu().numpy())
        assert e < 1e-4, (n, e)
