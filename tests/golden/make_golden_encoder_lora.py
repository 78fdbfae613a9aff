"""Generate tests/golden/encoder_lora.npz by running the REAL reference on the CPU in fp32: its EncoderModel
(VyomAI/models/encoder.py), its linears wrapped by its own LoraLinear (VyomAI/layers/adapters.py) with the adapters n5 /
n6 of cases_encoder_lora.py (lora_b NOT zero), under a ClinicModel-shaped head -- `model` + `output`, hidden[:, 0, :] ->
nn.Linear -> CrossEntropyLoss, as Examples/adapters.ipynb builds it -- everything frozen but lora_a / lora_b and the
head.  The reference is imported at run time only; only inputs and outputs are stored.  This repository goes BEFORE the
reference on the path:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<this repository>:<reference checkout> python tests/golden/make_golden_encoder_lora.py

Keys (model = abs | rope_gqa, who = n5 | n6, tag = <model>.<who>):
  <tag>.keys                  the trained state_dict keys (lora_a / lora_b and output.*), sorted
  <tag>.logits, <tag>.loss    logits (B, NUM_LABELS) and the mean cross-entropy of cases_encoder_lora.batch
  <model>.base.logits         the logits of the unwrapped model
  <tag>.d.<key>               the gradient of every trained key (cases_encoder_lora.sub_g)
  <tag>.bf16_gap.<key>        rel_err of the reference's OWN bf16 gradient against its fp32 one (whole tensors)
  <tag>.train.loss, <tag>.train.w.<key>   3 torch.optim.AdamW steps on the trained keys over the same batch
  <tag>.merged.<linear>.weight            linear.weight + alpha * lora_b @ lora_a of every wrapped linear (sub_g)
Asserted here: every stored gradient is non-zero; every bf16 gap is below 3e-2 (the GPU test's 6e-2 floor decides every
key); the adapter moves the logits; the file < 1 MB."""
import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from VyomAI.layers.adapters import LoraLinear  # noqa: E402  (the reference)
from VyomAI.models import encoder as ref  # noqa: E402  (the reference)
from tests.golden import cases_encoder_lora as E  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


class Classifier(nn.Module):
    """ClinicModel of Examples/adapters.ipynb, by its attribute names: `model`, `output`."""

    def __init__(self, model, hidden, n_classes):
        super().__init__()
        self.model = model
        self.output = nn.Linear(hidden, n_classes)

    def forward(self, ids, mask):
        return self.output(self.model(input_ids=ids, attention_mask=mask).logits[:, 0, :])


def base(model):
    pos, attn = E.MODELS[model]
    c = E.cfg(model)
    m = Classifier(ref.EncoderModel(c, pos_embedding_type=pos, attention_type=attn), c.hidden_size, E.NUM_LABELS).eval()
    E.load_weights_(m)
    return m


def wrapped(model, who, dtype=torch.float32):
    """The encoder frozen and wrapped as the notebook does, then the head (created after the freeze: trainable)."""
    m = base(model)
    spec, state = E.ADAPTERS[who], E.adapter_state(model, who)
    for p in m.model.parameters():
        p.requires_grad_(False)
    for key in sorted({k.rsplit(".", 1)[0] for k in state}):
        owner = m
        for part in key.split(".")[:-1]:
            owner = getattr(owner, part)
        attr = key.split(".")[-1]
        lora = LoraLinear(getattr(owner, attr), rank=spec["rank"], alpha=spec["alpha"])
        with torch.no_grad():
            lora.lora_a.copy_(T(state[key + ".lora_a"]))
            lora.lora_b.copy_(T(state[key + ".lora_b"]))
        setattr(owner, attr, lora)
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == E.trained_keys(model, who)
    m = m.to(dtype)
    if hasattr(m.model, "emb_freq"):
        m.model.emb_freq = m.model.emb_freq.to(dtype) if m.model.emb_freq.is_floating_point() else m.model.emb_freq
    return m


def step(m, ids, mask, labels):
    m.zero_grad()
    logits = m(ids, mask)
    loss = nn.CrossEntropyLoss()(logits.float(), labels)
    loss.backward()
    return logits, loss, {n: p.grad.detach().float().numpy().copy() for n, p in m.named_parameters() if p.requires_grad}


def main():
    out = {}
    ids, mask, labels = (T(a) for a in E.batch())
    for model in E.MODELS:
        with torch.no_grad():
            base_logits = base(model)(ids, mask).numpy()
        out[f"{model}.base.logits"] = base_logits
        for who in E.ADAPTERS:
            tag = f"{model}.{who}"
            keys = E.trained_keys(model, who)
            out[f"{tag}.keys"] = np.array(keys)
            m = wrapped(model, who).train()
            logits, loss, g = step(m, ids, mask, labels)
            assert sorted(g) == keys
            out[f"{tag}.logits"] = logits.detach().numpy()
            out[f"{tag}.loss"] = loss.detach().numpy()
            assert rel_err(out[f"{tag}.logits"], base_logits) > 0.1, "the adapter must move the logits"
            _, _, gb = step(wrapped(model, who, torch.bfloat16).train(), ids, mask, labels)
            worst = ("", 0.0)
            for k in keys:
                assert np.abs(g[k]).max() > 0, k
                out[f"{tag}.d.{k}"] = E.sub_g(g[k]).copy()
                gap = rel_err(gb[k], g[k])
                out[f"{tag}.bf16_gap.{k}"] = np.float32(gap)
                worst = max(worst, (k, gap), key=lambda t: t[1])
            print(f"{tag}: loss {loss.item():.7f}; reference bf16 vs fp32 gradients: worst {worst[1]:.2e} at {worst[0]}")
            assert worst[1] < 3e-2, worst
            for name, mod in m.named_modules():
                if isinstance(mod, LoraLinear):
                    w = mod.linear.weight.detach() + float(mod.alpha) * (mod.lora_b.detach() @ mod.lora_a.detach())
                    out[f"{tag}.merged.{name}.weight"] = E.sub_g(w.numpy()).copy()
            # three AdamW steps on the adapters and the head
            m = wrapped(model, who).train()
            params = {n: p for n, p in m.named_parameters() if p.requires_grad}
            opt = torch.optim.AdamW(list(params.values()), lr=E.LR, weight_decay=E.WEIGHT_DECAY)
            losses = []
            for _ in range(E.TRAIN_STEPS):
                opt.zero_grad()
                loss = nn.CrossEntropyLoss()(m(ids, mask), labels)
                loss.backward()
                opt.step()
                losses.append(loss.item())
            out[f"{tag}.train.loss"] = np.array(losses, dtype=np.float64)
            for k in keys:
                out[f"{tag}.train.w.{k}"] = E.sub_g(params[k].detach().numpy()).copy()
            print(f"{tag}: train losses {losses}")
    path = os.path.join(HERE, "encoder_lora.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
