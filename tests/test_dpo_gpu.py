"""DPO for ModelForCausalLM on the MI355X: the three vy_logprob_* kernels against fp64 torch formulas, sequence_logprobs
and dpo_loss against the REAL reference's notebook functions (tests/golden/dpo.npz, made by make_golden_dpo.py) in fp32
and bf16, and dpo_loss through FlatTrainer.

Bars.  fp32: the bars test_causal_lm_gpu.py holds clm_loss to (losses 2e-5 * max(1, |ref|), gradients rel_err < 1e-4,
trained weights mean 2e-6 / max 2 * 3 * LR + 1e-5).  bf16: nothing here is tighter than the reference holds itself --
the maker measured the reference's own bf16 models against its fp32 models on this batch and stored the gaps; each bar
is 3 x the stored gap of that quantity (the GPU rounds the logits to bf16 before the reduction and accumulates its GEMMs
in another order), gradient bars floored at the bars test_model_bf16_vs_reference applies to the same parameters.  A
reward is the mean difference of two average log-probs, each within the log-prob bar: its bar is twice that one."""
import numpy as np
import pytest
import torch

from tests.golden import cases_dpo as D
from tests.test_causal_lm_gpu import BF, DEV, T, elementwise_bars, rel_err
from tests.test_kernels_gpu import check, rnd

pytestmark = pytest.mark.gpu
PARAM_FLOOR, DX_FLOOR = 6e-2, 5e-2        # test_model_bf16_vs_reference: check_grads bar, input-embedding bar


# ------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------


def _kernel_case(V, dtype, seed):
    """M rows of random logits in a padded buffer whose pad columns inside the last 16-byte chunk hold a value that
    would wreck the row if it were read as a logit; mixed zero / non-zero weights; a label of 0 and of V - 1; an
    out-of-range label on a weightless row (must NOT raise the flag)."""
    from vyomai_amd.autograd_train import _row_stride
    M = 24
    ld = _row_stride(V)
    x = (2.0 * rnd(M, V, seed=seed)).to(dtype)
    buf = torch.zeros((M, ld), dtype=dtype)
    buf[:, :V] = x
    vec = 16 // x.element_size()          # the kernels move 16-byte chunks and own the pad columns inside the last one
    buf[:, V:(V + vec - 1) // vec * vec] = 60.0
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, V, (M,), generator=g)
    labels[0], labels[1] = 0, V - 1
    w = torch.rand(M, generator=g) * 0.3 + 0.01
    w[torch.tensor([2, 5, 6, 11, 23])] = 0.0
    labels[5] = V + 3
    return x, buf, labels, w.float()


def _want(x, labels, w, oob_row=None):
    """fp64: lse, logp, u = w * (onehot - softmax); skipped rows (w == 0, or the flagged one) are zero everywhere."""
    xd = x.double()
    live = w != 0
    if oob_row is not None:
        live[oob_row] = False
    lse = torch.logsumexp(xd, dim=-1)
    safe = labels.clamp(0, x.shape[1] - 1)
    logp = xd.gather(1, safe[:, None])[:, 0] - lse
    u = -torch.softmax(xd, dim=-1)
    u[torch.arange(x.shape[0]), safe] += 1.0
    u = u * w.double()[:, None]
    z = torch.zeros((), dtype=torch.float64)
    return torch.where(live, lse, z), torch.where(live, logp, z), torch.where(live[:, None], u, z)


def _run(kind, V, buf, labels, w):
    """-> (lse, logp, buffer after the call, flag); kind = pair | fused."""
    from vyomai_amd import ops
    b = buf.to(DEV).clone()
    lab, wd = labels.to(DEV), w.to(DEV)
    lse = torch.full((b.shape[0],), 9.0, device=DEV)
    logp = torch.full((b.shape[0],), 9.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    if kind == "fused":
        ops.logprob_fused_(b[:, :V], lab, wd, lse, logp, flag)
    else:
        ops.logprob_fwd(b[:, :V], lab, wd, lse, logp, flag)
        assert torch.equal(b, buf.to(DEV)), "vy_logprob_fwd is read-only"
        ops.logprob_bwd_(b[:, :V], lab, wd, lse)
    torch.cuda.synchronize()
    return lse, logp, b, int(flag.item())


@pytest.mark.parametrize("V", [512, 1000, 1003, 32000, 50265, 65536, 70000])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_logprob_kernels_vs_fp64(V, dtype):
    """Widths on a chunk boundary (512, 1000, 32000, 65536: the widest the fused kernel takes) and ending inside a
    16-byte chunk (1003, 50265).  70000 and fp32 go through the unfused pair only (vy_logprob_fused refuses them)."""
    from vyomai_amd import ops
    from vyomai_amd._lib import VyomHipError
    atol, rtol = elementwise_bars(dtype)
    x, buf, labels, w = _kernel_case(V, dtype, seed=V % 97)
    fused_ok = dtype == BF and V <= 65536
    if not fused_ok:
        with pytest.raises(VyomHipError, match="vy_logprob_fused"):
            ops.logprob_fused_(buf.to(DEV)[:, :V], labels.to(DEV), w.to(DEV), torch.empty(24, device=DEV),
                               torch.empty(24, device=DEV))
    kinds = ("pair", "fused") if fused_ok else ("pair",)
    for oob_row in (None, 7):
        lab = labels.clone()
        if oob_row is not None:
            lab[oob_row] = -1 if V % 2 else V      # just outside either end
        lse64, logp64, u64 = _want(x, lab, w.clone(), oob_row)
        got = {}
        for kind in kinds:
            lse, logp, b, flag = got[kind] = _run(kind, V, buf, lab, w)
            what = f"V={V} {kind} oob={oob_row}"
            assert flag == (0 if oob_row is None else 1), what
            check(lse, lse64, atol, rtol, "lse " + what)
            check(logp, logp64, atol, rtol, "logp " + what)
            check(b[:, :V], u64, atol, rtol, "w * (onehot - softmax) " + what)
            assert not b[:, V:].any(), "pad columns stay zero: " + what
            dead = (w == 0).clone()
            if oob_row is not None:
                dead[oob_row] = True
            assert not b[dead.to(DEV)].any() and not logp[dead.to(DEV)].any(), "skipped rows are zero: " + what
            again = _run(kind, V, buf, lab, w)
            assert all(torch.equal(p, q) for p, q in zip(got[kind][:3], again[:3])), "two runs differ: " + what
        if fused_ok:
            for i, name in enumerate(("lse", "logp", "buffer")):
                check(got["fused"][i], got["pair"][i], atol, rtol, f"fused vs pair {name} V={V} oob={oob_row}")


# ------------------------------------------------------------------------------------------
# model vs the reference's fixtures
# ------------------------------------------------------------------------------------------


def build(case, loader, compute=None):
    import vyomai_amd as V
    m = V.ModelForCausalLM(V.Config(**D.CASES[case]))
    loader(m)
    m = m.to(DEV)
    if compute is not None:          # fp32 master weights, bf16 kernels (what FlatTrainer sets)
        m.compute_dtype = m.model.compute_dtype = compute
    return m


def models(case, compute=None):
    return build(case, D.load_policy_weights_, compute).train(), build(case, D.load_reference_weights_, compute).eval()


def dev_batch(case):
    return {k: T(v).to(DEV) for k, v in D.batch(case).items()}


def cat_batch(batch):
    return torch.cat([batch["chosen"], batch["rejected"]]), torch.cat([batch["chosen_mask"], batch["rejected_mask"]])


def near(got, want, bar, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    print(f"{what}: max abs err {err:.3e} (bar {bar:.3e})")
    assert err <= bar, f"{what}: max abs err {err:.3e} > {bar:.3e}"


def check_scores(g, case, pol, frozen, batch, logp_bar, loss_bar, reward_bar, what):
    """Per-sequence log-probs of both models (with and without grad), losses at both betas and the rewards."""
    ids, mask = cat_batch(batch)
    B = D.PAIRS
    with torch.no_grad():
        pi, fr = pol.sequence_logprobs(ids, mask), frozen.sequence_logprobs(ids, mask)
    pig = pol.sequence_logprobs(ids, mask)
    assert pi.dtype == torch.float32 and pi.shape == (2 * B,) and pig.requires_grad
    for name, got in (("pi.chosen", pi[:B]), ("pi.rejected", pi[B:]), ("ref.chosen", fr[:B]), ("ref.rejected", fr[B:]),
                      ("pi.chosen (grad)", pig[:B]), ("pi.rejected (grad)", pig[B:])):
        want = g[f"{case}.{name.split(' ')[0]}"]
        near(got.detach().cpu().numpy(), want, logp_bar(want), f"{what} {case} {name}")
    for beta in D.BETAS:
        loss, rc, rr = pol.dpo_loss(batch, frozen, beta=beta)
        assert loss.requires_grad and not rc.requires_grad and not rr.requires_grad
        want = float(g[f"{case}.loss.{beta}"])
        near(loss.item(), want, loss_bar(beta, want), f"{what} {case} loss(beta={beta})")
        near(rc.item(), float(g[f"{case}.reward.chosen"]), reward_bar, f"{what} {case} chosen reward")
        near(rr.item(), float(g[f"{case}.reward.rejected"]), reward_bar, f"{what} {case} rejected reward")
    assert int(pol.label_error.item()) == 0 and int(frozen.label_error.item()) == 0


def check_grads(g, case, pol, frozen, batch, param_bar, dx_bar, what):
    """Gradients of the beta = GRAD_BETA loss: the TRAINED parameters, then the input embeddings."""
    pol.zero_grad()
    pol.dpo_loss(batch, frozen, beta=D.GRAD_BETA)[0].backward()
    params = dict(pol.named_parameters())
    errs = {}
    for n in D.TRAINED:
        errs[n] = rel_err(D.sub_g(n, params[n].grad), g[f"{case}.d.{n}"])
        print(f"  {what} {case}: d {n} rel_err {errs[n]:.3e} (bar {param_bar(n):.3e})")
    bad = {n: e for n, e in errs.items() if not e < param_bar(n)}
    assert not bad, (what, bad)
    ids, mask = cat_batch(batch)
    B = D.PAIRS
    dt = pol.model.compute_dtype or torch.float32
    emb = pol.model.embed_tokens.weight.detach()[ids].to(dt).requires_grad_(True)
    pi = pol.sequence_logprobs(ids, mask, inputs_embeds=emb)
    with torch.no_grad():
        fr = frozen.sequence_logprobs(ids, mask)
    z = (pi[:B] - pi[B:]) - (fr[:B] - fr[B:])
    (-torch.nn.functional.logsigmoid(D.GRAD_BETA * z)).mean().backward()
    e = rel_err(D.sub_h(emb.grad), g[f"{case}.dx"])
    print(f"  {what} {case}: input-embedding gradient rel_err {e:.3e} (bar {dx_bar:.3e})")
    assert e < dx_bar, e


@pytest.mark.parametrize("case", ["a", "b"])
def test_dpo_fp32_vs_reference(golden, case):
    g = golden("dpo")
    pol, frozen = models(case)
    batch = dev_batch(case)

    def bar(want):
        return 2e-5 * max(1.0, float(np.abs(want).max()))
    check_scores(g, case, pol, frozen, batch, bar, lambda beta, want: bar(want), 2e-5, "fp32")
    check_grads(g, case, pol, frozen, batch, lambda n: 1e-4, 1e-4, "fp32")


@pytest.mark.parametrize("case", ["a", "b"])
def test_dpo_bf16_vs_reference(golden, case):
    g = golden("dpo")
    pol, frozen = models(case, compute=BF)
    batch = dev_batch(case)
    logp_bar = 3.0 * float(g[f"{case}.gap.logp"])
    check_scores(g, case, pol, frozen, batch, lambda want: logp_bar,
                 lambda beta, want: 3.0 * float(g[f"{case}.gap.loss.{beta}"]), 2.0 * logp_bar, "bf16")
    check_grads(g, case, pol, frozen, batch, lambda n: max(3.0 * float(g[f"{case}.gap.d.{n}"]), PARAM_FLOOR),
                max(3.0 * float(g[f"{case}.gap.dx"]), DX_FLOOR), "bf16")


@pytest.mark.parametrize("compute", [torch.float32, BF], ids=["fp32", "bf16"])
def test_sequence_logprobs_no_grad_equals_grad_and_an_empty_mask_scores_zero(compute):
    """The scoring path (vy_logprob_fwd) against the training path (vy_logprob_fused in bf16) on the same weights, to
    the fused-versus-unfused rounding; a sequence whose mask selects nothing scores exactly 0 on both, and its zero
    score leaves every gradient finite."""
    case = "a"
    pol, _ = models(case, compute=None if compute == torch.float32 else compute)
    ids, mask = cat_batch(dev_batch(case))
    mask = mask.clone()
    mask[3] = 0.0
    mask[6, :] = 0.0
    mask[6, 0] = 1.0     # only the position the shift drops
    with torch.no_grad():
        a = pol.sequence_logprobs(ids, mask)
    b = pol.sequence_logprobs(ids, mask)
    atol, rtol = elementwise_bars(compute)
    check(b, a, atol, rtol, "grad vs no_grad")
    assert a[3].item() == 0.0 and b[3].item() == 0.0 and a[6].item() == 0.0 and b[6].item() == 0.0
    assert float(a[0]) < -1.0
    (b * torch.arange(1.0, 9.0, device=DEV)).sum().backward()
    for n, p in pol.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    # the same input twice: the same bits
    with torch.no_grad():
        assert torch.equal(a, pol.sequence_logprobs(ids, mask))


# ------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------


def test_trainer_direct_gradients_hold_both_table_contributions(golden):
    """dpo_loss under FlatTrainer: one 2B-row graph, the gradients written straight into the arena; the tied table gets
    the vocabulary weight gradient (rows of n scaled per sequence) and the embedding scatter into the one view --
    compared with the reference's gradient -- and is reported ready once, by the last of the two."""
    from vyomai_amd.training import FlatTrainer
    g = golden("dpo")
    case = "a"
    pol, frozen = models(case)
    tr = FlatTrainer(pol, lr=D.LR, weight_decay=D.WEIGHT_DECAY, compute_dtype=torch.float32, overlap_optimizer=False)
    batch = dev_batch(case)
    tr.zero_grad()
    tr.backward(pol.dpo_loss(batch, frozen, beta=D.GRAD_BETA)[0])
    table = pol.model.embed_tokens.weight
    assert table.grad.data_ptr() >= tr.arena.grad.data_ptr() and pol.lm_head.weight.grad is table.grad
    params = dict(pol.named_parameters())
    for n in D.TRAINED:
        e = rel_err(D.sub_g(n, params[n].grad), g[f"{case}.d.{n}"])
        print(f"  arena gradient d {n} rel_err {e:.3e}")
        assert e < 1e-4, (n, e)
    assert float(table.grad[0].abs().max()) > 0     # padding_idx row: no scatter, but the vocabulary gradient is there
    assert tr.reducer.touched == {id(p) for p in tr.arena.params}


def test_trainer_fp32_follows_reference_dpo_training(golden):
    from vyomai_amd.training import FlatTrainer
    g = golden("dpo")
    case = "a"
    pol, frozen = models(case)
    tr = FlatTrainer(pol, lr=D.LR, weight_decay=D.WEIGHT_DECAY, compute_dtype=torch.float32)
    batch = dev_batch(case)
    for step in range(D.TRAIN_STEPS):
        loss = tr.train_step(lambda: pol.dpo_loss(batch, frozen, beta=D.GRAD_BETA)[0])
        ref = float(g[f"{case}.train.loss"][step])
        print(f"step {step}: HIP fp32 DPO loss {loss.item():.7f}  reference loss {ref:.7f}")
        assert abs(loss.item() - ref) < 2e-5 * max(1.0, abs(ref)), (step, loss.item(), ref)
    params = dict(pol.named_parameters())
    for name in D.TRAINED:
        w = D.sub_g(name, params[name].detach().float().cpu().numpy())
        wr = g[f"{case}.train.w.{name}"]
        print(f"{name}: mean |dw| {np.abs(w - wr).mean():.3e} max {np.abs(w - wr).max():.3e}")
        assert np.abs(w - wr).mean() < 2e-6, (name, np.abs(w - wr).mean())
        assert np.abs(w - wr).max() < 2 * 3 * D.LR + 1e-5, (name, np.abs(w - wr).max())


def test_trainer_bf16_follows_reference_dpo_training(golden):
    """Three bf16 steps of dpo_loss through FlatTrainer.train_step follow the golden losses within the bf16 loss bar;
    scoring the frozen model inside the step and passing its precomputed scores give the same bits."""
    from vyomai_amd.training import FlatTrainer
    g = golden("dpo")
    for case in ("a", "b"):
        pol, frozen = models(case)
        frozen.compute_dtype = frozen.model.compute_dtype = BF
        tr = FlatTrainer(pol, lr=D.LR, weight_decay=D.WEIGHT_DECAY)
        batch = dev_batch(case)
        with torch.no_grad():
            fr = frozen.sequence_logprobs(*cat_batch(batch))
            pre = (fr[:D.PAIRS].clone(), fr[D.PAIRS:].clone())
            one = pol.dpo_loss(batch, frozen, beta=D.GRAD_BETA)
            two = pol.dpo_loss(batch, beta=D.GRAD_BETA, ref_logprobs=pre)
        assert all(torch.equal(p, q) for p, q in zip(one, two)), (one, two)
        one = pol.dpo_loss(batch, frozen, beta=D.GRAD_BETA)
        two = pol.dpo_loss(batch, beta=D.GRAD_BETA, ref_logprobs=pre)
        assert all(torch.equal(p, q) for p, q in zip(one, two)), (one, two)
        bar = 3.0 * float(g[f"{case}.gap.loss.{D.GRAD_BETA}"])
        for step in range(D.TRAIN_STEPS):
            loss = tr.train_step(lambda: pol.dpo_loss(batch, ref_logprobs=pre, beta=D.GRAD_BETA)[0] if step == 1
                                 else pol.dpo_loss(batch, frozen, beta=D.GRAD_BETA)[0])
            ref = float(g[f"{case}.train.loss"][step])
            print(f"{case} step {step}: HIP bf16 DPO loss {loss.item():.5f}  reference loss {ref:.5f}  (bar {bar:.2e})")
            assert abs(loss.item() - ref) < bar, (case, step, loss.item(), ref, bar)
        assert pol.model.layers[0].mlp.up_proj.weight.grad.data_ptr() >= tr.arena.grad.data_ptr()
