"""Generate tests/golden/electra.npz: ELECTRA and masked-LM pre-training as the REAL reference does them, on the CPU in
fp32.  The encoders are VyomAI.models.encoder's, the collators VyomAI.pretraining.collators'; Discriminator, ElectraModel
and ElectraLoss are obtained by reading Examples/electra-pretraining.ipynb from the same checkout and exec-ing the cells
that define them.  Only inputs and outputs are stored.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python tests/golden/make_golden_electra.py

The reference's electra() raises on its last statement (torch.nonzero(..., as_tuple=True) is a tuple and has no .to); the
maker then builds that index tuple itself -- it says so when it does -- and everything before it runs as written.

Keys (the case is cases_electra.py's):
  draw.masked_ids, draw.labels, draw.masked     masked_language_modeling under torch.manual_seed(DRAW_SEED)
  draw.sampled                                  sample(generator logits[masked], TEMPERATURE), one id per masked position
  draw.disc_input, draw.disc_labels             electra()'s first two results
  <t>.loss = [total, generator, discriminator]  ElectraLoss, <t> = untied | tied (fp64)
  mlm.loss                                      nn.CrossEntropyLoss of the generator alone on the draw (fp64)
  <t>.d.<param>                                 gradients of the total loss, cases_electra.sub_g
  tied.train.loss, tied.train.w.<param>         TRAIN_STEPS torch.optim.AdamW steps on the fixed draw
  gap.<key>                                     the reference's OWN bf16 models against its fp32 ones: |loss gap| per
                                                loss, rel_err per gradient
"""
import json
import os
import sys
import types

os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # before the reference: it has its own `tests` package

from VyomAI.models import encoder as ref  # noqa: E402  (the reference)
from VyomAI.pretraining import collators as ref_col  # noqa: E402
from tests.golden import cases_electra as E  # noqa: E402

torch.set_num_threads(8)
NOTEBOOK = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(ref.__file__)))), "Examples",
                        "electra-pretraining.ipynb")
WANTED = ("Discriminator", "ElectraModel", "ElectraLoss")


def notebook_classes():
    """The notebook's own classes, from the cells that define them (run here, never copied)."""
    ns = {"torch": torch, "nn": nn, "EncoderModel": ref.EncoderModel, "config": types.SimpleNamespace()}
    with open(NOTEBOOK) as f:
        cells = json.load(f)["cells"]
    for cell in cells:
        src = "".join(cell["source"])
        if cell["cell_type"] == "code" and any(src.lstrip().startswith(f"class {name}") for name in WANTED):
            exec(compile(src, NOTEBOOK, "exec"), ns)
    return tuple(ns[name] for name in WANTED)


Discriminator, ElectraModel, ElectraLoss = notebook_classes()
TOK = E.StubTokenizer()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def build(tied, dtype=torch.float32):
    gen = ref.EncoderForMaskedLM(E.cfg(E.GEN_LAYERS), pos_embedding_type="rope")
    m = ElectraModel(gen, Discriminator(E.cfg(E.DISC_LAYERS)))
    E.load_weights_(m, tied)
    return m.to(dtype)


def electra_fixed(ids, masked, sampled):
    """electra()'s results for a given draw: its own statements up to the one that raises."""
    disc_input = ids.clone()
    disc_input[masked] = sampled
    return disc_input, (ids != disc_input).float(), torch.nonzero(ids != TOK.pad_token_id, as_tuple=True)


def step_loss(m, ids, mask, draw):
    out = m.get_generator_output(draw["masked_ids"], mask)
    disc_input, disc_labels, live = electra_fixed(ids, draw["masked"], draw["sampled"])
    z = m.get_discriminator_output(disc_input, mask)
    return ElectraLoss(E.cfg(E.GEN_LAYERS))(out.logits.float(), draw["labels"], z.float(), disc_labels, live)


def scores(tied, ids, mask, draw, dtype):
    m = build(tied, dtype)
    r = {}
    loss, gl, dl = step_loss(m, ids, mask, draw)
    r["loss"] = torch.stack([loss, gl, dl])
    loss.backward()
    for n, p in m.named_parameters():
        r[f"d.{n}"] = T(E.sub_g(p.grad.detach().float().numpy()).copy())
    return {k: v.detach().double().numpy().copy() for k, v in r.items()}


def main():
    out = {}
    ids, mask = (T(a) for a in E.batch())
    # the draw: the reference's collators on its own generator's logits
    torch.manual_seed(E.DRAW_SEED)
    masked_ids, labels, masked = ref_col.masked_language_modeling(ids, TOK, fraction=E.FRACTION, ignore_index=E.IGNORE)
    gen = build(False).generator_model
    with torch.no_grad():
        logits = gen(masked_ids, mask).logits
    try:
        disc_input, disc_labels, _ = ref_col.electra(logits, ids, TOK, masked, temperature=E.TEMPERATURE)
        sampled = disc_input[masked]
    except AttributeError as e:
        print(f"the reference's electra() raised on its last statement ({e}): the maker builds the index tuple itself")
        torch.manual_seed(E.DRAW_SEED + 1)
        sampled = ref_col.sample(logits[masked], temperature=E.TEMPERATURE)
        disc_input, disc_labels, _ = electra_fixed(ids, masked, sampled)
    draw = {"masked_ids": masked_ids, "labels": labels, "masked": masked, "sampled": sampled}
    n_mask, n_repl = int(masked.sum()), int(disc_labels.sum())
    print(f"draw: {n_mask} masked of {int(mask.sum())} tokens, {n_repl} replaced by the sampler")
    assert n_mask >= 8 and 0 < n_repl <= n_mask and not masked[mask == 0].any()
    for k, v in draw.items():
        out[f"draw.{k}"] = v.numpy().astype(np.int64)
    out["draw.disc_input"], out["draw.disc_labels"] = disc_input.numpy(), disc_labels.numpy()
    mlm = nn.CrossEntropyLoss()(logits.view(-1, E.VOCAB), labels.view(-1))
    out["mlm.loss"] = np.float64(mlm.item())
    with torch.no_grad():
        mlm16 = nn.CrossEntropyLoss()(build(False, torch.bfloat16).generator_model(masked_ids, mask).logits.float()
                                      .view(-1, E.VOCAB), labels.view(-1))
    out["gap.mlm.loss"] = np.float64(abs(mlm16.item() - mlm.item()))
    for tied in (False, True):
        t = "tied" if tied else "untied"
        f32, b16 = scores(tied, ids, mask, draw, torch.float32), scores(tied, ids, mask, draw, torch.bfloat16)
        print(f"{t}: losses fp32 {f32['loss']} bf16 {b16['loss']}  mlm {mlm.item():.6f}")
        for k, v in f32.items():
            out[f"{t}.{k}"] = v
            out[f"gap.{t}.{k}"] = np.abs(b16[k] - v) if k == "loss" else np.float64(rel_err(b16[k], v))
    assert abs(out["untied.loss"][1] - out["mlm.loss"]) < 1e-6
    # AdamW steps on the fixed draw, tied tables
    m = build(True).train()
    opt = torch.optim.AdamW(list(m.parameters()), lr=E.LR, weight_decay=E.WEIGHT_DECAY)
    losses = []
    for _ in range(E.TRAIN_STEPS):
        opt.zero_grad()
        loss = step_loss(m, ids, mask, draw)[0]
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"training losses {losses}")
    out["tied.train.loss"] = np.array(losses, dtype=np.float64)
    for n, p in m.named_parameters():
        out[f"tied.train.w.{n}"] = E.sub_g(p.detach().numpy()).copy()
    for k in sorted(out):
        if k.startswith("gap."):
            print(f"   {k} = {np.asarray(out[k]).max():.3e}")
    wide = {k for k in out if k.endswith("loss") or k.startswith("gap.")}
    out = {k: np.asarray(v, dtype=np.float64) if k in wide else
           (np.asarray(v) if np.asarray(v).dtype.kind in "ib" else np.asarray(v).astype(np.float32)) for k, v in out.items()}
    path = os.path.join(HERE, "electra.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
