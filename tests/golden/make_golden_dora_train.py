"""Generate tests/golden/dora_train.npz by running the REAL reference: its ModelForCausalLM (needs `transformers`), case
"a" filled by cases_causal_lm.load_weights_, its linears wrapped by the reference's DoraLinear with the adapters d1 / d2
of cases_dora.py (dora_b NOT zero, dora_m moved off its initial value), everything frozen but dora_m / dora_a / dora_b as
Examples/adapters.ipynb freezes it, on the CPU in fp32.  The reference is imported at run time only (the DPO functions
are run out of the notebook's own cells, as make_golden_dpo.py does); only inputs and outputs are stored.  This
repository goes BEFORE the reference on the path:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<this repository>:<reference checkout> python tests/golden/make_golden_dora_train.py

Keys (who = d1 | d2):
  <who>.keys                         the adapter's dora_m / dora_a / dora_b state_dict keys, sorted
  <who>.loss                         loss of cases_causal_lm.padded_batch through forward(labels=)
  <who>.d.<key>                      its gradient for every dora parameter (cases_causal_lm.sub_g)
  <who>.bf16_gap.<key>               rel_err of the reference's OWN bf16 gradient against its fp32 one (whole tensors)
  <who>.train.loss, <who>.train.w.<key>   3 torch.optim.AdamW steps (lr, weight decay of cases_causal_lm) on the adapter
                                     parameters over cases_causal_lm.train_batch: losses (fp64) and final weights (sub_g)
  <who>.dpo.loss                     compute_dpo_loss_batch(cases_dpo.batch, wrapped model, the base model, beta = 1)
Asserted here: every stored gradient is non-zero; every column norm of every D = W + dora_a @ dora_b is > 1e-3 (the
reference divides by it without an epsilon; this keeps the missing epsilon from deciding a result); the file < 1 MB.
Printed: the largest bf16 gap.  The run that wrote the committed file printed 4.02e-2, at
model.layers.1.self_attn.k_proj.dora_m of d2 (d1: 3.28e-2 at model.layers.1.mlp.gate_proj.dora_a): below the GPU test's
6e-2 floor, so twice the gap decides the bar of a key only where its gap exceeds 3e-2."""
import json
import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from VyomAI.layers.adapters import DoraLinear  # noqa: E402  (the reference)
from VyomAI.models import custom_transformer as ref  # noqa: E402  (the reference)
from tests.golden import cases_causal_lm as C  # noqa: E402
from tests.golden import cases_dora as R  # noqa: E402
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
    return ns["compute_dpo_loss_batch"]


compute_dpo_loss_batch = notebook_functions()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def base():
    m = ref.ModelForCausalLM(ref.Config(**R.KW)).eval()
    C.load_weights_(m)
    return m


def wrapped(who, dtype=torch.float32):
    """The base model with the adapter's linears replaced by the reference's DoraLinear, everything else frozen."""
    m = base()
    spec, state = R.ADAPTERS[who], R.adapter_state(who)
    for p in m.parameters():
        p.requires_grad_(False)
    for key in sorted({k.rsplit(".", 1)[0] for k in state}):
        owner = m
        for part in key.split(".")[:-1]:
            owner = getattr(owner, part)
        attr = key.split(".")[-1]
        dora = DoraLinear(getattr(owner, attr), rank=spec["rank"])
        with torch.no_grad():
            for leaf in R.LEAVES:
                getattr(dora, leaf).copy_(T(state[f"{key}.{leaf}"]))
            d = dora.linear.weight + dora.dora_a @ dora.dora_b
            assert float(d.norm(p=2, dim=0).min()) > 1e-3, key
        setattr(owner, attr, dora)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted(state)
    return m.to(dtype)


def grads(m, batch):
    pids, pmask, plabels = batch
    m.zero_grad()
    loss = m(input_ids=pids, attention_mask=pmask, labels=plabels, use_cache=False).loss
    loss.backward()
    return loss, {n: p.grad.detach().float().numpy().copy() for n, p in m.named_parameters() if p.requires_grad}


def main():
    out = {}
    batch = tuple(T(a) for a in C.padded_batch(R.CASE))
    tids, tlabels = (T(a) for a in C.train_batch(R.CASE))
    dpo = {k: T(v) for k, v in D.batch(R.CASE).items()}
    largest = ("", 0.0)
    for who in R.ADAPTERS:
        keys = sorted(R.adapter_state(who))
        out[f"{who}.keys"] = np.array(keys)
        m = wrapped(who).train()
        loss, g = grads(m, batch)
        assert sorted(g) == keys
        out[f"{who}.loss"] = loss.detach().numpy()
        _, gb = grads(wrapped(who, torch.bfloat16).train(), batch)
        worst = ("", 0.0)
        for k in keys:
            assert np.abs(g[k]).max() > 0, k
            out[f"{who}.d.{k}"] = C.sub_g(k, g[k]).copy()
            gap = rel_err(gb[k], g[k])
            out[f"{who}.bf16_gap.{k}"] = np.float32(gap)
            worst = max(worst, (k, gap), key=lambda t: t[1])
        largest = max(largest, worst, key=lambda t: t[1])
        print(f"{who}: loss {loss.item():.7f}; reference bf16 vs fp32 gradients: worst {worst[1]:.2e} at {worst[0]}")
        # three AdamW steps on the adapter parameters
        m = wrapped(who).train()
        params = {n: p for n, p in m.named_parameters() if p.requires_grad}
        opt = torch.optim.AdamW(list(params.values()), lr=C.LR, weight_decay=C.WEIGHT_DECAY)
        losses = []
        for _ in range(C.TRAIN_STEPS):
            opt.zero_grad()
            loss = m(input_ids=tids, labels=tlabels, use_cache=False).loss
            loss.backward()
            opt.step()
            losses.append(loss.item())
        out[f"{who}.train.loss"] = np.array(losses, dtype=np.float64)
        for k in keys:
            out[f"{who}.train.w.{k}"] = C.sub_g(k, params[k].detach().numpy()).copy()
        print(f"{who}: train losses {losses}")
        # DPO with the adapter-disabled model -- the base -- as the frozen reference
        with torch.no_grad():
            dl = compute_dpo_loss_batch(dpo, wrapped(who).eval(), base(), D.GRAD_BETA)[0]
        out[f"{who}.dpo.loss"] = np.float64(dl.item())
        print(f"{who}: DPO loss {dl.item():.7f} (ln 2 = {np.log(2):.7f})")
        assert abs(dl.item() - np.log(2)) > 1e-3, "the adapter must move the policy away from its reference"
    print(f"largest bf16 gap: {largest[1]:.2e} at {largest[0]}")
    path = os.path.join(HERE, "dora_train.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
