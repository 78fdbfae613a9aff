"""The RMSNorm + SwiGLU causal LM on the MI355X: the two new streaming kernels against fp64 torch formulas, the model
against the REAL reference's outputs and autograd (tests/golden/causal_lm.npz, made by make_golden_causal_lm.py), the
trainer against the reference under torch.optim.AdamW, and one layer at the benchmark size against a plain-torch fp32
restatement."""
import math

import numpy as np
import pytest
import torch

from tests.golden import cases_causal_lm as C
from tests.test_kernels_gpu import check, rnd
from vyomai_amd import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ACTS = {"gelu": 1, "gelu_tanh": 2, "silu": 3, "tanh": 4, "sigmoid": 5, "relu6": 6, "leaky_relu": 7}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got = got.detach().float().cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def close(got, want, atol, what=""):
    got = got.detach().float().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want).max()
    print(f"{what}: max abs err {err:.3e} (bar {atol})")
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol}"


def elementwise_bars(dtype):
    """(atol, rtol) of an elementwise result against fp64.  fp32: 1e-5 absolute on O(1) data.  bf16: the kernels
    compute in fp32 and round once, so the result is the fp64 value rounded to bf16 give or take the fp32 error: one
    bf16 rounding is at most 2^-8 relative, the bar is 2^-7, plus the fp32 bar as the absolute floor (it covers the
    fp32 arithmetic where the result is small against its terms)."""
    return (1e-5, 0.0) if dtype == torch.float32 else (1e-5, 2.0 ** -7)


def act_fp64(code, x):
    F = torch.nn.functional
    return {1: lambda: F.gelu(x), 2: lambda: F.gelu(x, approximate="tanh"), 3: lambda: F.silu(x), 4: lambda: torch.tanh(x),
            5: lambda: torch.sigmoid(x), 6: lambda: F.relu6(x), 7: lambda: F.leaky_relu(x, 0.01)}[code]()


# ------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_rmsnorm_bwd_vs_fp64(dtype):
    """vy_rmsnorm_bwd: w_offset 0 / 1, with and without add_to, accumulate on and off, row counts that are not a
    multiple of the wave count, every width class of the kernel (1, 2, 4 chunks per lane pipelined; 8 and 16 not)."""
    from vyomai_amd import ops
    eps = 1e-6
    shapes = [(203, 896), (5, 64), (37, 2048), (21, 4096)] + ([(9, 8192), (2051, 448)] if dtype == BF else [(2051, 224)])
    atol, rtol = elementwise_bars(dtype)
    for M, N in shapes:
        x = rnd(M, N, seed=1).to(dtype)
        dy = rnd(M, N, seed=2).to(dtype)
        w = (0.1 * rnd(N, seed=3)).to(dtype)
        add = rnd(M, N, seed=4).to(dtype)
        dw0 = rnd(N, seed=5)
        for w_offset in (0.0, 1.0):
            xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
            y = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * (w_offset + wd)
            (y * dy.double()).sum().backward()
            for with_add in (False, True):
                for acc in (False, True):
                    dw = dw0.clone().to(DEV)
                    dx = ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), eps, w_offset, dw, acc,
                                         add_to=add.to(DEV) if with_add else None)
                    what = f"{M}x{N} w_offset={w_offset} add_to={with_add} accumulate={acc}"
                    check(dx, xd.grad + (add.double() if with_add else 0.0), atol, rtol, "dx " + what)
                    want_dw = wd.grad + (dw0.double() if acc else 0.0)
                    if dtype == BF:   # the reduction bar of test_bwd_kernels_gpu.py's LayerNorm dgamma
                        check(dw, want_dw, 2e-3 * math.sqrt(M), 1e-3, "dw " + what)
                    else:             # a sum of M terms, each inside the fp32 elementwise bar
                        check(dw, want_dw, 1e-5 * max(1.0, math.sqrt(M)), 0.0, "dw " + what)
        # no atomics: the same bits on a second run
        a, b = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), eps, 0.0, a, False)
        ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), eps, 0.0, b, False)
        assert torch.equal(a, b), (M, N)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_gated_act_fwd_and_bwd_every_code_vs_fp64(dtype):
    from vyomai_amd import ops
    atol, rtol = elementwise_bars(dtype)
    for M, I in ((67, 512), (1030, 1216)):
        gu = rnd(M, 2 * I, seed=7).to(dtype)
        d = rnd(M, I, seed=8).to(dtype)
        gu.view(-1)[:16] = T(np.array([0.0, 6.0, -0.0, 3.0, -6.0, 1.0, 0.5, 8.0] * 2, dtype=np.float32)).to(dtype)  # kinks
        for name, code in ACTS.items():
            g64 = gu.double().requires_grad_(True)
            out = act_fp64(code, g64[:, :I]) * g64[:, I:]
            (out * d.double()).sum().backward()
            got = ops.gated_act(gu.to(DEV), code)
            check(got, out, atol, rtol, f"gated_act fwd {name} {M}x{I}")
            dgu = ops.gated_act_bwd(d.to(DEV), gu.to(DEV), code)
            check(dgu, g64.grad, atol, rtol, f"gated_act bwd {name} {M}x{I}")


# ------------------------------------------------------------------------------------------
# model vs the reference's fixtures
# ------------------------------------------------------------------------------------------


def build(kw, compute=None):
    import vyomai_amd as V
    m = V.ModelForCausalLM(V.Config(**kw))
    C.load_weights_(m)
    m = m.to(DEV)
    if compute is not None:          # fp32 master weights, bf16 kernels (what FlatTrainer sets)
        m.compute_dtype = m.model.compute_dtype = compute
    return m


def live_grads(m):
    return {n: p.grad for n, p in m.named_parameters()}


def check_grads(m, g, case, bar, what):
    errs = {}
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        errs[n] = rel_err(C.sub_g(n, p.grad), g[f"{case}.d.{n}"])
        print(f"  {what}: d {n} rel_err {errs[n]:.3e}")
    bad = {n: e for n, e in errs.items() if not e < bar}
    assert not bad, (what, bar, bad)


@pytest.mark.parametrize("case", ["a", "b"])
def test_model_fp32_vs_reference(golden, case):
    g = golden("causal_lm")
    m = build(C.CASES[case]).eval()
    ids = T(C.ids(case)).to(DEV)
    pids, pmask, plabels = (T(a).to(DEV) for a in C.padded_batch(case))
    keep = T(C.padded_batch(case)[1]).bool().numpy()
    with torch.no_grad():
        out = m(input_ids=ids, labels=ids, use_cache=False)
        close(C.sub_h(out.last_hidden_state), g[f"{case}.hidden"], 1e-5, "hidden")
        close(C.sub_h(out.logits), g[f"{case}.logits"], 2e-5, "logits")
        ref = float(g[f"{case}.loss"])
        for name, loss in (("forward", out.loss), ("clm_loss", m.clm_loss(ids, ids))):
            print(f"loss {name}: {loss.item():.7f} reference {ref:.7f}")
            assert abs(loss.item() - ref) <= 2e-5 * abs(ref), (name, loss.item(), ref)
        out = m(input_ids=pids, attention_mask=pmask, labels=plabels, use_cache=False)
        close(C.sub_h(out.last_hidden_state)[T(keep)], g[f"{case}.pad.hidden"][keep], 1e-5, "hidden, padded batch")
        close(C.sub_h(out.logits)[T(keep)], g[f"{case}.pad.logits"][keep], 2e-5, "logits, padded batch")
        ref = float(g[f"{case}.pad.loss"])
        assert abs(out.loss.item() - ref) <= 2e-5 * abs(ref), (out.loss.item(), ref)
        assert abs(m.clm_loss(pids, plabels, pmask).item() - ref) <= 2e-5 * abs(ref)
    # gradients, through the materialised-logits forward and through the fused loss: every parameter, the tied table
    # (vocabulary weight gradient + embedding scatter) among them
    m.train()
    m(input_ids=pids, attention_mask=pmask, labels=plabels, use_cache=False).loss.backward()
    check_grads(m, g, case, 1e-4, "forward(labels)")
    m.zero_grad()
    m.clm_loss(pids, plabels, pmask).backward()
    check_grads(m, g, case, 1e-4, "clm_loss")
    emb = m.model.embed_tokens.weight.detach()[pids].clone().requires_grad_(True)
    m(inputs_embeds=emb, attention_mask=pmask, labels=plabels, use_cache=False).loss.backward()
    e = rel_err(C.sub_h(emb.grad), g[f"{case}.dx"])
    print(f"input-embedding gradient rel_err {e:.3e}")
    assert e < 1e-4, e
    # prefill + cached single-token steps, greedy ids
    m.eval()
    with torch.no_grad():
        out = m(input_ids=ids[:, :C.PREFILL], use_cache=True)
        steps = [out.logits[:, -1:]]
        for t in range(C.PREFILL, C.PREFILL + C.STEPS):
            out = m(input_ids=ids[:, t:t + 1], past_key_values=out.past_key_values, use_cache=True)
            steps.append(out.logits)
        close(torch.cat(steps, dim=1), g[f"{case}.steps"], 2e-5, "cached-step logits")
        toks = m.generate(T(g[f"{case}.prompt"]).to(DEV), max_new_tokens=C.GREEDY_NEW)
    assert np.array_equal(toks[:, :C.PREFILL].cpu().numpy(), g[f"{case}.prompt"])
    assert np.array_equal(toks[:, C.PREFILL:].cpu().numpy(), g[f"{case}.greedy"]), toks[:, C.PREFILL:]


def test_generate_with_a_mask_and_with_eos(golden):
    """generate() under an all-ones attention_mask (single-token steps through the masked attention kernel instead of
    vy_attn_decode) gives the reference's ids too; with eos_token_id a row continues with pad_token_id after its first
    eos while the other rows go on."""
    g = golden("causal_lm")
    m = build(C.CASES["a"]).eval()
    prompt = T(g["a.prompt"]).to(DEV)
    toks = m.generate(prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=C.GREEDY_NEW)
    assert np.array_equal(toks[:, C.PREFILL:].cpu().numpy(), g["a.greedy"])
    want = g["a.greedy"].copy()
    eos = int(want[0, 2])
    for row in want:
        hit = np.nonzero(row == eos)[0]
        if hit.size:
            row[hit[0] + 1:] = 0
    assert (want[0, 3:] == 0).all() and (want != g["a.greedy"]).any()
    toks = m.generate(prompt, max_new_tokens=C.GREEDY_NEW, eos_token_id=eos)
    assert np.array_equal(toks[:, C.PREFILL:].cpu().numpy(), want), toks[:, C.PREFILL:]


@pytest.mark.parametrize("case", ["a", "b"])
def test_model_bf16_vs_reference(golden, case):
    g = golden("causal_lm")
    m = build(C.CASES[case], compute=BF).train()
    ids = T(C.ids(case)).to(DEV)
    pids, pmask, plabels = (T(a).to(DEV) for a in C.padded_batch(case))
    keep = T(C.padded_batch(case)[1]).bool().numpy()
    with torch.no_grad():
        out = m(input_ids=ids, use_cache=False)
        assert out.logits.dtype == BF
        for name, got, want in (("hidden", out.last_hidden_state, g[f"{case}.hidden"]), ("logits", out.logits, g[f"{case}.logits"])):
            e = rel_err(C.sub_h(got), want)
            print(f"bf16 {name} rel_err {e:.3e}")
            assert e < 3e-2, (name, e)
        out = m(input_ids=pids, attention_mask=pmask, use_cache=False)
        e = rel_err(C.sub_h(out.logits)[T(keep)], g[f"{case}.pad.logits"][keep])
        assert e < 3e-2, e
    loss = m.clm_loss(pids, plabels, pmask)
    ref = float(g[f"{case}.pad.loss"])
    print(f"bf16 fused loss {loss.item():.5f} reference {ref:.5f}")
    assert abs(loss.item() - ref) < 3e-2 * max(1.0, abs(ref))
    loss.backward()
    check_grads(m, g, case, 6e-2, "bf16 clm_loss")
    emb = m.model.embed_tokens.weight.detach()[pids].to(BF).requires_grad_(True)
    m(inputs_embeds=emb, attention_mask=pmask, labels=plabels, use_cache=False).loss.backward()
    e = rel_err(C.sub_h(emb.grad), g[f"{case}.dx"])
    print(f"bf16 input-embedding gradient rel_err {e:.3e}")
    assert e < 5e-2, e


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_gated_mlp_block_gelu_vs_reference(golden, dtype):
    """x + MLP(RMSNorm(x)) with hidden_act = gelu (PreNormGatedMlpFn alone) against the reference's classes."""
    import vyomai_amd as V
    from vyomai_amd.autograd_train import PreNormGatedMlpFn
    g = golden("causal_lm")
    cfg = V.Config(**C.MLP_BLOCK)
    norm, mlp = V.RMSNorm(cfg.hidden_size, eps=cfg.rms_norm_eps), V.MLP(cfg)
    for prefix, mod in (("mlp.norm.", norm), ("mlp.mlp.", mlp)):
        for n, t in mod.state_dict().items():
            t.copy_(T(recipe.param_value(prefix + n, tuple(t.shape))))
    norm, mlp = norm.to(DEV), mlp.to(DEV)
    x = T(recipe.uniform("mlp.x", (C.B, C.L, cfg.hidden_size))).to(DEV).to(dtype).requires_grad_(True)
    gout = T(recipe.uniform("mlp.gout", (C.B, C.L, cfg.hidden_size))).to(DEV).to(dtype)
    y = PreNormGatedMlpFn.apply(x, mlp, norm.weight, norm.variance_epsilon, mlp.act, mlp.gate_proj.weight,
                                mlp.up_proj.weight, mlp.down_proj.weight)
    (y.float() * gout.float()).sum().backward()
    by, bx, bp = (1e-5, 1e-4, 1e-4) if dtype == torch.float32 else (3e-2, 5e-2, 6e-2)
    if dtype == torch.float32:
        close(C.sub_h(y), g["mlp.y"], by, "mlp block y")
    else:
        assert rel_err(C.sub_h(y), g["mlp.y"]) < by
    assert rel_err(C.sub_h(x.grad), g["mlp.dx"]) < bx, rel_err(C.sub_h(x.grad), g["mlp.dx"])
    for prefix, mod in (("norm.", norm), ("mlp.", mlp)):
        for n, p in mod.named_parameters():
            e = rel_err(C.sub_g(n, p.grad), g["mlp.d." + prefix + n])
            assert e < bp, (prefix + n, e)


# ------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------


def test_trainer_direct_gradients_hold_both_table_contributions(golden):
    """Under FlatTrainer the gradients are written straight into the arena: the tied table gets the vocabulary weight
    gradient and the embedding scatter, in that order, into the one view -- compared with the reference's gradient."""
    from vyomai_amd.training import FlatTrainer
    g = golden("causal_lm")
    case = "a"
    m = build(C.CASES[case]).train()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=torch.float32, overlap_optimizer=False)
    pids, pmask, plabels = (T(a).to(DEV) for a in C.padded_batch(case))
    tr.zero_grad()
    tr.backward(m.clm_loss(pids, plabels, pmask))
    table = m.model.embed_tokens.weight
    assert table.grad.data_ptr() >= tr.arena.grad.data_ptr() and m.lm_head.weight.grad is table.grad
    check_grads(m, g, case, 1e-4, "arena gradients")
    assert float(table.grad[0].abs().max()) > 0     # padding_idx row: no scatter, but the vocabulary gradient is there
    # every parameter reported exactly once, the table by the LAST of its two writers
    assert tr.reducer.touched == {id(p) for p in tr.arena.params}


def test_trainer_fp32_follows_reference_training(golden):
    from vyomai_amd.training import FlatTrainer
    g = golden("causal_lm")
    case = "a"
    m = build(C.CASES[case]).train()
    tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY, compute_dtype=torch.float32)
    assert tr.arena.shadow is None
    ids, labels = (T(a).to(DEV) for a in C.train_batch(case))
    for step in range(C.TRAIN_STEPS):
        loss = tr.train_step(lambda: m.clm_loss(ids, labels))
        ref = float(g[f"{case}.train.loss"][step])
        print(f"step {step}: HIP fp32 loss {loss.item():.7f}  reference loss {ref:.7f}")
        assert abs(loss.item() - ref) < 2e-5 * max(1.0, abs(ref)), (step, loss.item(), ref)
    params = dict(m.named_parameters())
    for name in C.TRAINED:
        w = C.sub_g(name, params[name].detach().float().cpu().numpy())
        wr = g[f"{case}.train.w.{name}"]
        print(f"{name}: mean |dw| {np.abs(w - wr).mean():.3e} max {np.abs(w - wr).max():.3e}")
        assert np.abs(w - wr).mean() < 2e-6, (name, np.abs(w - wr).mean())
        assert np.abs(w - wr).max() < 2 * 3 * C.LR + 1e-5, (name, np.abs(w - wr).max())


def test_trainer_bf16_follows_reference_training(golden):
    from vyomai_amd.training import FlatTrainer
    g = golden("causal_lm")
    for case in ("a", "b"):
        m = build(C.CASES[case]).train()
        tr = FlatTrainer(m, lr=C.LR, weight_decay=C.WEIGHT_DECAY)
        ids, labels = (T(a).to(DEV) for a in C.train_batch(case))
        for step in range(C.TRAIN_STEPS):
            loss = tr.train_step(lambda: m.clm_loss(ids, labels))
            ref = float(g[f"{case}.train.loss"][step])
            print(f"{case} step {step}: HIP bf16 loss {loss.item():.5f}  reference loss {ref:.5f}")
            assert abs(loss.item() - ref) < 3e-2 * max(1.0, abs(ref)), (case, step, loss.item(), ref)
        assert m.model.layers[0].mlp.up_proj.weight.grad.data_ptr() >= tr.arena.grad.data_ptr()


# ------------------------------------------------------------------------------------------
# one layer at the benchmark size
# ------------------------------------------------------------------------------------------


def _layer_fp32(sd, x, h, hk, dh, eps, theta):
    """Plain-torch restatement of the reference's DecoderLayer (pre-norm RMSNorm, GQA, rotate-half RoPE, causal
    softmax, SwiGLU) in fp32."""
    B, L, d = x.shape

    def rms(t, w):
        return w * (t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps))

    def rot(t):
        a, b = t[..., : dh // 2], t[..., dh // 2:]
        return torch.cat((-b, a), dim=-1)
    inv = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.int64).float() / dh))
    ang = torch.outer(torch.arange(L).float(), inv)
    emb = torch.cat((ang, ang), dim=-1)
    cos, sin = emb.cos()[None, None], emb.sin()[None, None]
    lin = torch.nn.functional.linear
    n = rms(x, sd["input_layernorm.weight"])
    q = lin(n, sd["self_attn.q_proj.weight"], sd["self_attn.q_proj.bias"]).view(B, L, h, dh).transpose(1, 2)
    k = lin(n, sd["self_attn.k_proj.weight"], sd["self_attn.k_proj.bias"]).view(B, L, hk, dh).transpose(1, 2)
    v = lin(n, sd["self_attn.v_proj.weight"], sd["self_attn.v_proj.bias"]).view(B, L, hk, dh).transpose(1, 2)
    q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
    k, v = k.repeat_interleave(h // hk, dim=1), v.repeat_interleave(h // hk, dim=1)
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True)
    x = x + lin(o.transpose(1, 2).reshape(B, L, h * dh), sd["self_attn.o_proj.weight"])
    n = rms(x, sd["post_attention_layernorm.weight"])
    return x + lin(torch.nn.functional.silu(lin(n, sd["mlp.gate_proj.weight"])) * lin(n, sd["mlp.up_proj.weight"]),
                   sd["mlp.down_proj.weight"])


def test_layer_at_the_benchmark_size_vs_fp32_restatement():
    """One DecoderLayer at the Qwen2-0.5B widths (d = 896, 14 heads over 2 KV heads, I = 4864) on 4096 rows, bf16
    forward AND backward: the large-shape paths of the GEMMs, the grouped weight gradients (packed q/k/v and packed
    gate/up among them), flash attention with 7 query heads per KV head, and the two new streaming kernels."""
    import vyomai_amd as V
    from vyomai_amd.layers.mask import AttnMask
    cfg = V.Config(hidden_size=896, intermediate_size=4864, num_attention_heads=14, num_key_value_heads=2,
                   num_hidden_layers=1, vocab_size=64, max_position_embeddings=512)
    B, L, d = 8, 512, cfg.hidden_size
    torch.manual_seed(0)
    model = V.BaseModel(cfg)
    layer = model.layers[0]
    for n, t in layer.state_dict().items():
        t.copy_(T(recipe.param_value("big.clm." + n, tuple(t.shape))))
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in layer.state_dict().items()}
    model = model.to(DEV).train()
    layer = model.layers[0]
    x0 = T(recipe.uniform("big.clm.x", (B, L, d))).to(BF)
    g0 = T(recipe.uniform("big.clm.gout", (B, L, d))).to(BF)
    x = x0.to(DEV).requires_grad_(True)
    mask = AttnMask.from_padding(None, causal=True, start_pos=0, query_len=L)
    y = layer(x, attention_mask=mask, position_embeddings=model._rope_slice(0, L))[0]
    (y.float() * g0.to(DEV).float()).sum().backward()
    torch.cuda.synchronize()
    xr = x0.float().requires_grad_(True)
    yr = _layer_fp32(sd, xr, 14, 2, 64, cfg.rms_norm_eps, cfg.rope_theta)
    (yr * g0.float()).sum().backward()

    def rel(a, b):
        return float((a.detach().float().cpu() - b.detach()).abs().max() / (b.detach().abs().max() + 1e-12))

    def rel_rms(a, b):
        a, b = a.detach().float().cpu(), b.detach()
        return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12))
    print(f"y rel {rel(y, yr):.3e} rms {rel_rms(y, yr):.3e}; dx rel {rel(x.grad, xr.grad):.3e} rms {rel_rms(x.grad, xr.grad):.3e}")
    assert rel(y, yr) < 3e-2, rel(y, yr)
    assert rel_rms(y, yr) < 6e-3, rel_rms(y, yr)
    assert rel(x.grad, xr.grad) < 6e-2, rel(x.grad, xr.grad)
    assert rel_rms(x.grad, xr.grad) < 1.5e-2, rel_rms(x.grad, xr.grad)
    for n, p in layer.named_parameters():
        e = rel(p.grad, sd[n].grad)
        print(f"  d {n}: rel {e:.3e}")
        assert e < 6e-2, (n, e)
