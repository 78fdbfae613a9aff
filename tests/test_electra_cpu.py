"""ELECTRA / masked-LM pre-training, the parts that need no GPU: the C ABI, the collators on CPU tensors with the stub
tokenizer of cases_electra.py, the LanguageModeling dataset and the layout of tests/golden/electra.npz."""
import ctypes
import math
import os
import re

import numpy as np
import torch

from tests.golden import cases_electra as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vy_xent_sample_fwd", "vy_xent_sample_fused", "vy_gumbel_noise", "vy_bce_head_fwd", "vy_bce_head_bwd", "vy_mlm_mask")


def test_abi_declares_and_exports_the_new_entry_points():
    from vyomai_amd import _lib
    header = open(os.path.join(ROOT, "include", "vyom_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.vy_abi_version() == 5


def mlm_invariants(ids, out, labels, masked, tok, ignore=-100):
    """What every masked_language_modeling result satisfies, whatever the draw."""
    ids, out, labels, masked = (np.asarray(t) for t in (ids, out, labels, masked))
    special = np.isin(ids, tok.all_special_ids)
    assert masked.dtype == np.bool_ and not (masked & special).any(), "special tokens are never selected"
    assert (labels[masked] == ids[masked]).all() and (labels[~masked] == ignore).all()
    assert (out[~masked] == ids[~masked]).all(), "unselected ids are unchanged"
    assert out.min() >= 0 and out.max() < len(tok)


def mlm_proportions(ids, out, masked, tok, fraction):
    """Shares within 6 binomial standard deviations: selected among the non-special tokens (fraction), and of the
    selection: mask token 0.8, random 0.1, kept 0.1.  A random id equals the original with probability 1 / vocab and
    then counts as kept, the mask id is never drawn as an original (it is special): the expectations move by
    0.1 / vocab, far inside the bars."""
    ids, out, masked = (np.asarray(t) for t in (ids, out, masked))
    mask_id = tok.convert_tokens_to_ids(tok.mask_token)
    n = int((~np.isin(ids, tok.all_special_ids)).sum())
    k = int(masked.sum())
    shares = {"selected": (k / n, fraction, n),
              "mask": (float((out[masked] == mask_id).mean()), 0.8, k),
              "kept": (float((out[masked] == ids[masked]).mean()), 0.1, k)}
    shares["random"] = (1.0 - shares["mask"][0] - shares["kept"][0], 0.1, k)
    for name, (got, p, trials) in shares.items():
        sd = math.sqrt(p * (1 - p) / trials)
        print(f"{name}: {got:.4f} expected {p} ({(got - p) / sd:+.2f} sd)")
        assert abs(got - p) <= 6 * sd, (name, got, p, sd)


def big_ids(n=65536):
    """n tokens in rows of 128: <s> first, </s> and pads at the end of every row, ordinary ids between."""
    from vyomai_amd import recipe
    ids = recipe.token_ids("electra.big", (n // 128, 128), 5, E.VOCAB)
    ids[:, 0], ids[:, 120], ids[:, 121:] = 0, 2, 1
    return torch.from_numpy(ids)


def test_masked_language_modeling_cpu():
    from vyomai_amd.pretraining import masked_language_modeling
    tok = E.StubTokenizer()
    torch.manual_seed(7)
    ids = big_ids()
    out, labels, masked = masked_language_modeling(ids, tok, fraction=0.15)
    assert out.shape == ids.shape and out.dtype == torch.long and labels.dtype == torch.long
    mlm_invariants(ids, out, labels, masked, tok)
    mlm_proportions(ids, out, masked, tok, 0.15)
    out, labels, masked = masked_language_modeling(ids[:2], tok, fraction=0.5, ignore_index=-7)
    mlm_invariants(ids[:2], out, labels, masked, tok, ignore=-7)


def test_noise_and_sample_cpu():
    from vyomai_amd.pretraining import log, noise, sample
    torch.manual_seed(3)
    t = torch.zeros(64, 4096)
    g = noise(t)
    assert g.shape == t.shape and torch.isfinite(g).all() and g.min() >= -3.04 and g.max() <= 20.73
    assert torch.equal(log(torch.tensor([1.0])), torch.log(torch.tensor([1.0]) + 1e-9))
    x = torch.zeros(5, 9)
    x[torch.arange(5), torch.tensor([3, 0, 8, 5, 1])] = 60.0
    assert sample(x, temperature=2.0).tolist() == [3, 0, 8, 5, 1]


def test_electra_with_injected_samples():
    from vyomai_amd.pretraining import electra
    tok = E.StubTokenizer()
    ids, _ = (torch.from_numpy(a) for a in E.batch())
    masked = torch.zeros_like(ids, dtype=torch.bool)
    masked[0, 3], masked[1, 7], masked[2, 4], masked[3, 2] = True, True, True, True
    sampled = torch.tensor([int(ids[0, 3]), 17, 900, int(ids[3, 2]) ^ 1])     # first one "replaced" by itself
    disc_in, disc_labels, live = electra(None, ids, tok, masked, sampled=sampled)
    want = ids.clone()
    want[masked] = sampled
    assert torch.equal(disc_in, want) and disc_in is not ids
    assert disc_labels.dtype == torch.float32 and torch.equal(disc_labels, (ids != want).float())
    assert disc_labels.sum() == 3 and disc_labels[0, 3] == 0      # a sample equal to the original is "original"
    assert isinstance(live, tuple) and len(live) == 2
    assert all(torch.equal(a, b) for a, b in zip(live, torch.nonzero(ids != tok.pad_token_id, as_tuple=True)))
    assert live[0].numel() == sum(E.KEEP)
    # sampling from logits: a peaked row wins whatever the noise
    logits = torch.zeros(*ids.shape, 50)
    logits[..., 11] = 400.0
    disc_in, _, _ = electra(logits, ids, tok, masked, temperature=3)
    assert (disc_in[masked] == 11).all() and torch.equal(disc_in[~masked], ids[~masked])


def test_language_modeling_blocks(tmp_path):
    from vyomai_amd.pretraining import LanguageModeling
    tok = E.StubTokenizer()
    words = [f"w{i}" for i in range(53)]
    path = tmp_path / "corpus.txt"
    path.write_text(" ".join(words), encoding="utf-8")
    ds = LanguageModeling(tok, str(path), block_size=12)       # 10 tokens + <s> </s> per block; the last 3 are dropped
    assert len(ds) == 5
    flat = tok.convert_tokens_to_ids(words)
    for i in range(5):
        item = ds[i]["input_ids"]
        assert item.dtype == torch.long and item.tolist() == [0] + flat[10 * i:10 * i + 10] + [2]
    try:
        LanguageModeling(tok, str(tmp_path / "missing.txt"), 12)
    except ValueError:
        pass
    else:
        raise AssertionError("a missing file must raise ValueError")


def param_shapes():
    """name -> shape of the ElectraModel of the case (built on the CPU: construction needs no kernel)."""
    import vyomai_amd as V
    m = V.ElectraModel(V.EncoderForMaskedLM(E.cfg(E.GEN_LAYERS), pos_embedding_type="rope"),
                       V.Discriminator(E.cfg(E.DISC_LAYERS)))
    return m, {n: tuple(p.shape) for n, p in m.named_parameters()}


def test_fixture_layout(golden):
    g = golden("electra")
    m, shapes = param_shapes()
    for k in ("masked_ids", "labels", "masked", "disc_input", "disc_labels"):
        assert g[f"draw.{k}"].shape == (E.B, E.L), k
    n_mask = int(g["draw.masked"].sum())
    assert g["draw.sampled"].shape == (n_mask,) and n_mask >= 8
    ids, mask = E.batch()
    assert not g["draw.masked"].astype(bool)[mask == 0].any()
    assert (g["draw.labels"][g["draw.masked"].astype(bool)] == ids[g["draw.masked"].astype(bool)]).all()
    assert g["mlm.loss"].shape == () and g["tied.train.loss"].shape == (E.TRAIN_STEPS,)
    # named_parameters lists a shared Parameter once, under the first name: discriminator_model is registered first
    tied_away = "generator_model.encoder.word_embeddings.weight"
    for t in ("untied", "tied"):
        assert g[f"{t}.loss"].shape == (3,) and g[f"gap.{t}.loss"].shape == (3,)
        assert abs(g[f"{t}.loss"][0] - g[f"{t}.loss"][1] - g[f"{t}.loss"][2]) < 1e-6
        for n, s in shapes.items():
            if t == "tied" and n == tied_away:
                assert f"tied.d.{n}" not in g
                continue
            want = E.sub_g(np.zeros(s, dtype=np.float32)).shape
            assert g[f"{t}.d.{n}"].shape == want, (t, n)
            assert g[f"gap.{t}.d.{n}"].shape == (), (t, n)
            if t == "tied":
                assert g[f"tied.train.w.{n}"].shape == want, n
    # the state dict interchanges with the notebook's classes: same names
    assert {"discriminator_model.discriminator.word_embeddings.weight", "generator_model.lm_head.decoder.weight",
            "discriminator_model.discriminator_head.weight", tied_away} <= set(shapes)
    m.tie_word_embeddings()
    assert m.discriminator_model.discriminator.word_embeddings.weight is m.generator_model.encoder.word_embeddings.weight


def test_next_offset_is_shared_with_dropout():
    from vyomai_amd import rng
    rng.manual_seed(5)
    a = rng.next_offset()
    b = rng.next_dropout(0.1)
    c = rng.next_offset()
    assert a[0] == b[1] == c[0] == 5 and len({a[1], b[2], c[1]}) == 3
    assert rng.next_dropout(0.0) is None
    rng.manual_seed(5)
    assert rng.next_offset() == a
