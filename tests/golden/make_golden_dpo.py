"""Generate tests/golden/dpo.npz: direct preference optimisation as the REAL reference does it, on the CPU in fp32.
The model is the reference's ModelForCausalLM (VyomAI/models/custom_transformer.py; needs `transformers`), imported at
run time; compute_logprobs, compute_dpo_loss and compute_dpo_loss_batch are obtained by reading
Examples/vyom-ai-llm-sft-dpo-training.ipynb from the same checkout and exec-ing the cells that define them.  Only
inputs' outputs are stored (float arrays).

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python tests/golden/make_golden_dpo.py

Keys (case = a | b of cases_causal_lm.py; the batch, the policy and the frozen model are those of cases_dpo.py):
  <case>.pi.{chosen,rejected}, <case>.ref.{chosen,rejected}   per-sequence average log-probs (PAIRS,), policy / frozen
  <case>.loss.<beta>, <case>.reward.{chosen,rejected}         compute_dpo_loss_batch at beta = 1.0 and 0.1 (fp64 scalars)
  <case>.d.<param>, <case>.dx                                 gradients of the beta = 1 loss: the TRAINED parameters
                                                              (sub_g) and the input embeddings, chosen rows then
                                                              rejected rows (sub_h)
  <case>.train.loss, <case>.train.w.<param>                   3 torch.optim.AdamW steps of DPO (beta = 1) in fp32
  <case>.gap.logp, <case>.gap.loss.<beta>,                    the reference's OWN bf16 models against its fp32 models on
  <case>.gap.d.<param>, <case>.gap.dx                         the same batch: largest absolute gap of the average
                                                              log-probs, gap of the loss, rel_err of each gradient
The maker asserts that the fixtures can tell a working model from none: |loss(beta = 1) - ln 2| > 3e-2 and per-pair DPO
logits of both signs.
"""
import json
import math
import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # before the reference: it has its own `tests` package

from VyomAI.models import custom_transformer as ref  # noqa: E402  (the reference)
from tests.golden import cases_dpo as D  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)
NOTEBOOK = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(ref.__file__)))), "Examples",
                        "vyom-ai-llm-sft-dpo-training.ipynb")
WANTED = ("compute_logprobs", "compute_dpo_loss", "compute_dpo_loss_batch")


def notebook_functions():
    """The notebook's own functions, from the cells that define them (run here, never copied)."""
    ns = {"torch": torch}
    with open(NOTEBOOK) as f:
        cells = json.load(f)["cells"]
    for cell in cells:
        src = "".join(cell["source"])
        if cell["cell_type"] == "code" and any(f"def {name}(" in src for name in WANTED):
            exec(compile(src, NOTEBOOK, "exec"), ns)
    return tuple(ns[name] for name in WANTED)


compute_logprobs, compute_dpo_loss, compute_dpo_loss_batch = notebook_functions()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def build(kw, loader, dtype=torch.float32):
    m = ref.ModelForCausalLM(ref.Config(**kw)).eval()
    loader(m)
    return m.to(dtype)


def live_params(m):
    return {"model." + n: p for n, p in m.model.named_parameters()}


def logprobs(m, batch):
    return tuple(compute_logprobs(m(input_ids=batch[k]).logits, batch[k], batch[k + "_mask"]) for k in ("chosen", "rejected"))


def scores(kw, batch, dtype):
    """Everything one precision gives: log-probs, losses, rewards, gradients of the beta = GRAD_BETA loss."""
    pol, frozen = build(kw, D.load_policy_weights_, dtype), build(kw, D.load_reference_weights_, dtype)
    r = {}
    with torch.no_grad():
        (r["pi.chosen"], r["pi.rejected"]), (r["ref.chosen"], r["ref.rejected"]) = logprobs(pol, batch), logprobs(frozen, batch)
        for beta in D.BETAS:
            loss, rc, rr = compute_dpo_loss_batch(batch, pol, frozen, beta)
            r[f"loss.{beta}"], r["reward.chosen"], r["reward.rejected"] = loss, rc, rr
    pol.zero_grad()
    compute_dpo_loss_batch(batch, pol, frozen, D.GRAD_BETA)[0].backward()
    lp = live_params(pol)
    for n in D.TRAINED:
        r[f"d.{n}"] = T(D.sub_g(n, lp[n].grad.detach().float().numpy()).copy())
    # the input embeddings' gradient: the same loss with the two embedded batches as leaves
    emb = {k: pol.model.embed_tokens(batch[k]).detach().requires_grad_(True) for k in ("chosen", "rejected")}
    pi = [compute_logprobs(pol(inputs_embeds=emb[k]).logits, batch[k], batch[k + "_mask"]) for k in ("chosen", "rejected")]
    with torch.no_grad():
        fr = logprobs(frozen, batch)
    compute_dpo_loss(pi[0], pi[1], fr[0], fr[1], beta=D.GRAD_BETA)[0].backward()
    r["dx"] = D.sub_h(torch.cat([emb["chosen"].grad, emb["rejected"].grad], dim=0))
    return {k: v.detach().double().numpy().copy() for k, v in r.items()}


def case_arrays(name, kw, out):
    batch = {k: T(v) for k, v in D.batch(name).items()}
    f32 = scores(kw, batch, torch.float32)
    for k, v in f32.items():
        out[f"{name}.{k}"] = v
    z = (f32["pi.chosen"] - f32["pi.rejected"]) - (f32["ref.chosen"] - f32["ref.rejected"])
    print(f"{name}: fp32 policy log-probs {f32['pi.chosen']} {f32['pi.rejected']}\n   frozen {f32['ref.chosen']} "
          f"{f32['ref.rejected']}\n   DPO logits {z}  " + "  ".join(f"loss({b}) {float(f32[f'loss.{b}']):.6f}" for b in D.BETAS))
    assert abs(float(f32["loss.1.0"]) - math.log(2.0)) > 3e-2, float(f32["loss.1.0"])
    assert (z > 0).any() and (z < 0).any(), z
    # the reference's own bf16 models against its fp32 ones
    b16 = scores(kw, batch, torch.bfloat16)
    lp_keys = ("pi.chosen", "pi.rejected", "ref.chosen", "ref.rejected")
    out[f"{name}.gap.logp"] = np.float64(max(np.abs(b16[k] - f32[k]).max() for k in lp_keys))
    for beta in D.BETAS:
        out[f"{name}.gap.loss.{beta}"] = np.float64(abs(b16[f"loss.{beta}"] - f32[f"loss.{beta}"]))
    for k in f32:
        if k.startswith("d.") or k == "dx":
            out[f"{name}.gap.{k}"] = np.float64(rel_err(b16[k], f32[k]))
    for k in sorted(out):
        if k.startswith(f"{name}.gap."):
            print(f"   {k} = {float(out[k]):.3e}")
    # three AdamW steps of DPO in fp32
    pol, frozen = build(kw, D.load_policy_weights_).train(), build(kw, D.load_reference_weights_)
    opt = torch.optim.AdamW(list(pol.model.parameters()), lr=D.LR, weight_decay=D.WEIGHT_DECAY)
    losses = []
    for _ in range(D.TRAIN_STEPS):
        opt.zero_grad()
        loss = compute_dpo_loss_batch(batch, pol, frozen, D.GRAD_BETA)[0]
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"   training losses {losses}")
    out[f"{name}.train.loss"] = np.array(losses, dtype=np.float64)
    lp = live_params(pol)
    for n in D.TRAINED:
        out[f"{name}.train.w.{n}"] = D.sub_g(n, lp[n].detach().numpy()).copy()


def main():
    out = {}
    for name, kw in D.CASES.items():
        case_arrays(name, kw, out)
    # scalars, per-sequence numbers and losses stay fp64; tensors are stored in fp32
    narrow = {k for k, v in out.items() if np.ndim(v) >= 1 and not k.endswith((".chosen", ".rejected", "train.loss"))}
    out = {k: np.asarray(v).astype(np.float32) if k in narrow else np.asarray(v, dtype=np.float64) for k, v in out.items()}
    path = os.path.join(HERE, "dpo.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
