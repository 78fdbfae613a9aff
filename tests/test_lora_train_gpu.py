"""LoRA fine-tuning of ModelForCausalLM on the MI355X against the REAL reference's autograd through its own LoraLinear
(tests/golden/lora_train.npz, make_golden_lora_train.py): case "a" with the adapters n1 (rank 32 on six projections) and
n2 (rank 8 on all seven) of cases_lora.py, lora_b non-zero, everything frozen but lora_a / lora_b.

Bars.  fp32: those of test_causal_lm_gpu.py's test_model_fp32_vs_reference (loss 2e-5 relative, gradients rel_err < 1e-4)
and test_trainer_fp32_follows_reference_training.  bf16: the loss bar of test_model_bf16_vs_reference; each gradient
within max(6e-2, 2 x the reference's OWN bf16-vs-fp32 gap for that key) -- the factor 2 for the other accumulation
order; the maker measured every gap at most 2.4e-2, so the 6e-2 floor decides every key today.  DPO: the fp32 loss bar
of test_dpo_gpu.py.  Wrapped vs merged forward and the served row: rel_err 2e-5, the fp32 bar of the engine tests."""
import copy

import numpy as np
import pytest
import torch

from tests.golden import cases_causal_lm as C
from tests.golden import cases_dpo as D
from tests.golden import cases_lora as L
from tests.test_causal_lm_gpu import BF, DEV, T, build, rel_err

pytestmark = pytest.mark.gpu
WHO = tuple(L.ADAPTERS)


def wrapped(who, compute=None):
    """Case "a" with the adapter `who`: add_lora on its projections, then the fixture's lora_a / lora_b values."""
    import vyomai_amd as V
    spec = L.ADAPTERS[who]
    m = V.add_lora(build(C.CASES[L.CASE], compute=compute), rank=spec["rank"], alpha=spec["alpha"], targets=spec["on"])
    params = dict(m.named_parameters())
    with torch.no_grad():
        for k, v in L.adapter_state(who).items():
            params[k].copy_(T(v))
    return m


def check_lora_grads(m, g, who, bar_of, what):
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


@pytest.mark.parametrize("who", WHO)
def test_fp32_loss_and_gradients_vs_reference(golden, who, monkeypatch):
    from vyomai_amd import ops
    g = golden("lora_train")
    m = wrapped(who).train()
    pids, pmask, plabels = (T(a).to(DEV) for a in C.padded_batch(L.CASE))
    ref = float(g[f"{who}.loss"])
    wgrads = []
    real = ops.linear_wgrad
    monkeypatch.setattr(ops, "linear_wgrad", lambda *a, **k: (wgrads.append(a[2].shape), real(*a, **k))[1])
    grouped = ops.linear_wgrad_grouped
    monkeypatch.setattr(ops, "linear_wgrad_grouped", lambda items: (wgrads.append(len(items)), grouped(items))[1])
    for name, run in (("forward(labels)", lambda: m(input_ids=pids, attention_mask=pmask, labels=plabels, use_cache=False).loss),
                      ("clm_loss", lambda: m.clm_loss(pids, plabels, pmask))):
        m.zero_grad()
        loss = run()
        print(f"{who} {name}: loss {loss.item():.7f} reference {ref:.7f}")
        assert abs(loss.item() - ref) <= 2e-5 * abs(ref), (name, loss.item(), ref)
        loss.backward()
        check_lora_grads(m, g, who, lambda n: 1e-4, name)
    assert wgrads == [], f"base weight gradients were launched: {wgrads}"


@pytest.mark.parametrize("who", WHO)
def test_bf16_loss_and_gradients_vs_reference(golden, who):
    g = golden("lora_train")
    m = wrapped(who, compute=BF).train()
    pids, pmask, plabels = (T(a).to(DEV) for a in C.padded_batch(L.CASE))
    ref = float(g[f"{who}.loss"])
    loss = m.clm_loss(pids, plabels, pmask)
    print(f"{who}: bf16 fused loss {loss.item():.5f} reference {ref:.5f}")
    assert abs(loss.item() - ref) < 3e-2 * max(1.0, abs(ref))
    loss.backward()
    check_lora_grads(m, g, who, lambda n: max(6e-2, 2.0 * float(g[f"{who}.bf16_gap.{n}"])), "bf16 clm_loss")


def test_no_grad_forward_equals_the_merged_model():
    """Validation during fine-tuning: the wrapped model under no_grad (no KV cache) against merge_lora on a copy."""
    import vyomai_amd as V
    ids = T(C.ids(L.CASE)).to(DEV)
    for who in WHO:
        m = wrapped(who).eval()
        merged = V.merge_lora(copy.deepcopy(m))
        assert not any(isinstance(x, V.LoraLinear) for x in merged.modules())
        with torch.no_grad():
            a = m(input_ids=ids, use_cache=False).logits
            b = merged(input_ids=ids, use_cache=False).logits
            base = build(C.CASES[L.CASE]).eval()(input_ids=ids, use_cache=False).logits
        e = rel_err(a, b.float().cpu().numpy())
        print(f"{who}: wrapped vs merged logits rel_err {e:.3e}")
        assert e < 2e-5, e
        assert rel_err(a, base.float().cpu().numpy()) > 0.1, "the adapter must move the logits"


@pytest.mark.parametrize("who", WHO)
def test_dpo_loss_with_the_adapter_disabled_model_as_reference(golden, who):
    import vyomai_amd as V
    g = golden("lora_train")
    m = wrapped(who).train()
    batch = {k: T(v).to(DEV) for k, v in D.batch(L.CASE).items()}
    ids = torch.cat([batch["chosen"], batch["rejected"]], dim=0)
    mask = torch.cat([batch["chosen_mask"], batch["rejected_mask"]], dim=0)
    with V.disable_lora(m), torch.no_grad():
        ref = m.sequence_logprobs(ids, mask)
        base = build(C.CASES[L.CASE]).eval().sequence_logprobs(ids, mask)
    assert torch.equal(ref, base), "under disable_lora the wrapped model computes the base model"
    loss, _, _ = m.dpo_loss(batch, ref_logprobs=(ref[:D.PAIRS], ref[D.PAIRS:]), beta=D.GRAD_BETA)
    want = float(g[f"{who}.dpo.loss"])
    print(f"{who}: DPO loss {loss.item():.7f} reference {want:.7f}")
    assert abs(loss.item() - want) <= 2e-5 * max(1.0, abs(want)), (loss.item(), want)
    loss.backward()
    for n, p in m.named_parameters():
        assert (p.grad is not None and bool(p.grad.abs().max() > 0)) == p.requires_grad, n


@pytest.mark.parametrize("who", WHO)
def test_trainer_fp32_follows_reference_training_and_the_adapter_is_served(golden, who):
    """Three FlatTrainer steps follow the reference's three torch.optim.AdamW steps on the adapter parameters and leave
    the base bitwise unchanged; then the loop closes: lora_state_dict into a LoraAdapters on the UNWRAPPED base, one
    request served with adapter= -- its prefill logits row is the wrapped model's own last-row logits."""
    import vyomai_amd as V
    from tests.test_lora_engine_gpu import serve
    from vyomai_amd.training import FlatTrainer
    g = golden("lora_train")
    m = wrapped(who).train()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=torch.float32)
    frozen = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    ids, labels = (T(a).to(DEV) for a in C.train_batch(L.CASE))
    for step in range(C.TRAIN_STEPS):
        loss = tr.train_step(lambda: m.clm_loss(ids, labels))
        ref = float(g[f"{who}.train.loss"][step])
        print(f"{who} step {step}: HIP fp32 loss {loss.item():.7f}  reference loss {ref:.7f}")
        assert abs(loss.item() - ref) < 2e-5 * max(1.0, abs(ref)), (step, loss.item(), ref)
    params = dict(m.named_parameters())
    for n, before in frozen.items():
        assert torch.equal(params[n].detach(), before), f"{n}: a frozen parameter changed"
    for name in g[f"{who}.keys"].tolist():
        w = C.sub_g(name, params[name].detach().float().cpu().numpy())
        wr = g[f"{who}.train.w.{name}"]
        assert np.abs(w - wr).mean() < 2e-6, (name, np.abs(w - wr).mean())
        assert np.abs(w - wr).max() < 2 * 3 * C.LR + 1e-5, (name, np.abs(w - wr).max())
    # the loop: train -> lora_state_dict -> LoraAdapters.load -> serve
    prompt = L.long_prompt(0).tolist()
    with torch.no_grad():
        own = m.eval()(input_ids=torch.tensor([prompt], device=DEV), use_cache=False).logits[0, -1]
    base = build(C.CASES[L.CASE]).eval()
    store = V.LoraAdapters(base, 1, max_rank=32)
    store.load("tuned", V.lora_state_dict(m), alpha=L.ADAPTERS[who]["alpha"])
    eng, done, sids, _ = serve(base, torch.float32, [(prompt, "tuned", 1), (prompt, None, 1)], store)
    served, plain = eng.logits[sids[0]][0], eng.logits[sids[1]][0]
    e = rel_err(served, own.float().cpu().numpy())
    print(f"{who}: served prefill row vs the wrapped model's last row rel_err {e:.3e}")
    assert e < 2e-5, e
    assert rel_err(plain, own.float().cpu().numpy()) > 1e-2, "the base request's row must differ"
