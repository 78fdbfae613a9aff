"""Generate tests/golden/causal_lm.npz by running the REAL reference's ModelForCausalLM
(VyomAI/models/custom_transformer.py; needs `transformers`) on the CPU in fp32.  The reference is imported at run time
only, filled with the deterministic recipe, and only inputs' outputs are stored (float / int arrays, plus two string
arrays: the reference's state_dict keys and its Config defaults).

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python tests/golden/make_golden_causal_lm.py

Keys (case = a | b, see cases_causal_lm.py):
  ref.keys, cfg.names, cfg.values          state_dict keys of the reference model (dead trunk included); Config defaults
  <case>.{hidden,logits,loss}              forward on the full batch        (hidden / logits sub-sampled by sub_h)
  <case>.pad.{hidden,logits,loss}          forward on the left-padded batch (compare unpadded positions only)
  <case>.d.<param>, <case>.dx              gradients of the padded batch's loss: every parameter (sub_g) and the input
                                           embeddings (sub_h)
  <case>.steps                             logits of prefill(8) + 8 single-token steps through DynamicCache
  <case>.prompt, <case>.greedy             prompt and 16 greedy ids (every top-2 margin asserted > 1e-3)
  <case>.train.loss, <case>.train.w.<p>    3 torch.optim.AdamW steps in fp32: losses and final weights (sub_g)
  mlp.{y,dx,d.<param>}                     x + MLP(RMSNorm(x)) with hidden_act = gelu on case a's widths
The maker asserts the greedy margins and that the reference's own bf16 forward stays inside the bf16 bars of the GPU
test (rel_err < 3e-2 on hidden and logits): the bars are attainable by the reference alone.
"""
import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from transformers.cache_utils import DynamicCache  # noqa: E402
from VyomAI.models import custom_transformer as ref  # noqa: E402  (the reference)
from tests.golden import cases_causal_lm as C  # noqa: E402
from vyomai_amd import recipe  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got, want = got.detach().float().numpy(), want.detach().float().numpy()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def build(kw):
    m = ref.ModelForCausalLM(ref.Config(**kw)).eval()
    C.load_weights_(m)
    return m


def live_params(m):
    """name -> parameter of the trunk that forward uses (the tied table once, under its embedding name)."""
    return {"model." + n: p for n, p in m.model.named_parameters()}


def forward(m, ids, mask=None, labels=None):
    hidden = m.model(input_ids=ids, attention_mask=mask, use_cache=False).last_hidden_state
    out = m(input_ids=ids, attention_mask=mask, labels=labels, use_cache=False)
    return hidden, out.logits, out.loss


def greedy(m, prompt):
    """Hand-rolled greedy loop over forward with a DynamicCache -> (ids (B, 16), smallest top-2 margin)."""
    cache, cur, new, margin = DynamicCache(), prompt, [], np.inf
    with torch.no_grad():
        for _ in range(C.GREEDY_NEW):
            lg = m(input_ids=cur, past_key_values=cache, use_cache=True).logits[:, -1]
            top = lg.topk(2, dim=-1).values
            margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
            cur = lg.argmax(-1, keepdim=True)
            new.append(cur)
    return torch.cat(new, dim=1), margin


def case_arrays(name, kw, out):
    m = build(kw)
    ids = T(C.ids(name))
    pids, pmask, plabels = (T(a) for a in C.padded_batch(name))
    with torch.no_grad():
        h, lg, loss = forward(m, ids, None, ids)
        out[f"{name}.hidden"], out[f"{name}.logits"], out[f"{name}.loss"] = C.sub_h(h).numpy(), C.sub_h(lg).numpy(), loss.numpy()
        hp, lgp, lossp = forward(m, pids, pmask, plabels)
        out[f"{name}.pad.hidden"], out[f"{name}.pad.logits"] = C.sub_h(hp).numpy(), C.sub_h(lgp).numpy()
        out[f"{name}.pad.loss"] = lossp.numpy()
        # the reference's own bf16 forward against its fp32 forward: inside the bf16 bars of the GPU test
        mb = build(kw).to(torch.bfloat16)
        hb, lgb, _ = forward(mb, ids, None, None)
        gap_h, gap_l = rel_err(hb, h), rel_err(lgb, lg)
        print(f"{name}: reference bf16 vs fp32: hidden {gap_h:.2e}  logits {gap_l:.2e}")
        assert gap_h < 3e-2 and gap_l < 3e-2, (gap_h, gap_l)
    # gradients of the padded batch's loss
    m.zero_grad()
    m(input_ids=pids, attention_mask=pmask, labels=plabels, use_cache=False).loss.backward()
    for n, p in live_params(m).items():
        out[f"{name}.d.{n}"] = C.sub_g(n, p.grad.detach().numpy()).copy()
    emb = m.model.embed_tokens(pids).detach().requires_grad_(True)
    m(inputs_embeds=emb, attention_mask=pmask, labels=plabels, use_cache=False).loss.backward()
    out[f"{name}.dx"] = C.sub_h(emb.grad).numpy().copy()
    # prefill + cached single-token steps
    with torch.no_grad():
        cache = DynamicCache()
        steps = [m(input_ids=ids[:, :C.PREFILL], past_key_values=cache, use_cache=True).logits[:, -1:]]
        for t in range(C.PREFILL, C.PREFILL + C.STEPS):
            steps.append(m(input_ids=ids[:, t:t + 1], past_key_values=cache, use_cache=True).logits)
        full = m(input_ids=ids, use_cache=False).logits[:, C.PREFILL - 1:]
        stepped = torch.cat(steps, dim=1)
        assert (stepped - full).abs().max() < 1e-5, float((stepped - full).abs().max())
        out[f"{name}.steps"] = stepped.numpy()
    # greedy ids: a prompt whose every step is decided by more than 1e-3
    for seed in range(64):
        prompt = T(C.greedy_prompt(name, seed))
        new, margin = greedy(m, prompt)
        if margin > 1e-3:
            break
    assert margin > 1e-3, margin
    print(f"{name}: greedy prompt seed {seed}, smallest top-2 margin {margin:.3e}")
    out[f"{name}.prompt.seed"] = np.array([seed], dtype=np.int64)
    out[f"{name}.prompt"], out[f"{name}.greedy"] = prompt.numpy(), new.numpy()
    # three AdamW steps in fp32
    m = build(kw).train()
    tids, tlabels = (T(a) for a in C.train_batch(name))
    opt = torch.optim.AdamW(list(m.model.parameters()), lr=C.LR, weight_decay=C.WEIGHT_DECAY)
    losses = []
    for _ in range(C.TRAIN_STEPS):
        opt.zero_grad()
        loss = m(input_ids=tids, labels=tlabels, use_cache=False).loss
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out[f"{name}.train.loss"] = np.array(losses, dtype=np.float64)
    lp = live_params(m)
    for n in C.TRAINED:
        out[f"{name}.train.w.{n}"] = C.sub_g(n, lp[n].detach().numpy()).copy()
    return m


def mlp_block(out):
    """x + MLP(RMSNorm(x)) from the reference's own classes, hidden_act = gelu."""
    cfg = ref.Config(**C.MLP_BLOCK)
    norm, mlp = ref.RMSNorm(cfg.hidden_size, eps=cfg.rms_norm_eps), ref.MLP(cfg)
    for prefix, mod in (("mlp.norm.", norm), ("mlp.mlp.", mlp)):
        for n, t in mod.state_dict().items():
            t.copy_(T(recipe.param_value(prefix + n, tuple(t.shape))))
    x = T(recipe.uniform("mlp.x", (C.B, C.L, cfg.hidden_size))).requires_grad_(True)
    gout = T(recipe.uniform("mlp.gout", (C.B, C.L, cfg.hidden_size)))
    y = x + mlp(norm(x))
    (y * gout).sum().backward()
    out["mlp.y"], out["mlp.dx"] = C.sub_h(y.detach()).numpy().copy(), C.sub_h(x.grad).numpy().copy()
    for prefix, mod in (("norm.", norm), ("mlp.", mlp)):
        for n, p in mod.named_parameters():
            out["mlp.d." + prefix + n] = C.sub_g(n, p.grad.numpy()).copy()


def main():
    import inspect
    out = {}
    for name, kw in C.CASES.items():
        m = case_arrays(name, kw, out)
    out["ref.keys"] = np.array(sorted(m.state_dict().keys()))
    sig = inspect.signature(ref.Config.__init__).parameters
    names = [p for p in sig if p not in ("self", "kwargs")]
    out["cfg.names"] = np.array(names)
    out["cfg.values"] = np.array([repr(sig[n].default) for n in names])
    mlp_block(out)
    out = {k: (v.astype(np.float32) if v.dtype == np.float64 and not k.endswith("train.loss") else v) for k, v in out.items()}
    path = os.path.join(HERE, "causal_lm.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
