"""DPO for ModelForCausalLM, the parts that need no GPU: the three vy_logprob_* entry points are declared, exported and
validate their arguments before any launch; dpo_loss rejects a batch that was not collated to one length; and
tests/golden/dpo.npz is self-consistent under an fp64 restatement of the notebook's formula and can tell a working model
from none."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests.golden import cases_dpo as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vy_logprob_fwd", "vy_logprob_bwd", "vy_logprob_fused")
BF16, F32 = 1, 0


def test_logprob_symbols_are_declared_and_exported():
    from vyomai_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vyom_hip.h")).read()
    declared = set(re.findall(r"\b(vy_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.PROTOTYPES and name in _lib.ALL_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "vyom-ai-llm-sft-dpo-training.ipynb" in hdr   # the entry points cite the notebook cells they replace


def test_logprob_argument_errors_are_reported_without_a_gpu():
    """Every check below fails before any launch (this machine has no GPU to launch on)."""
    from vyomai_amd import _lib
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    M, V = 2, 16
    with pytest.raises(_lib.VyomHipError, match="vy_logprob_fwd: bad arguments"):
        _lib.call("vy_logprob_fwd", None, 16, p, p, p, p, M, V, None, BF16, None)
    with pytest.raises(_lib.VyomHipError, match="vy_logprob_fwd: bad arguments"):
        _lib.call("vy_logprob_fwd", p, 16, p, None, p, p, M, V, None, BF16, None)     # no weights
    with pytest.raises(_lib.VyomHipError, match="vy_logprob_bwd: bad arguments"):
        _lib.call("vy_logprob_bwd", p, 16, p, p, None, M, V, BF16, None)              # no saved lse
    with pytest.raises(_lib.VyomHipError, match="vy_logprob_fused: bad arguments"):
        _lib.call("vy_logprob_fused", p, 16, None, p, p, p, M, V, None, BF16, None)   # no labels
    with pytest.raises(_lib.VyomHipError, match="vy_logprob_fwd: row stride"):
        _lib.call("vy_logprob_fwd", p, 12, p, p, p, p, M, V, None, BF16, None)        # not a multiple of 8
    with pytest.raises(_lib.VyomHipError, match="vy_logprob_fwd: row stride"):
        _lib.call("vy_logprob_fwd", p, 8, p, p, p, p, M, V, None, BF16, None)         # narrower than the row
    with pytest.raises(_lib.VyomHipError, match="vy_logprob_bwd: row stride"):
        _lib.call("vy_logprob_bwd", p, 18, p, p, p, M, V, F32, None)                  # fp32: not a multiple of 4
    with pytest.raises(_lib.VyomHipError, match="rows must be 16-byte aligned"):
        _lib.call("vy_logprob_fused", p, 12, p, p, p, p, M, V, None, BF16, None)
    with pytest.raises(_lib.VyomHipError, match="rows must be 16-byte aligned"):
        _lib.call("vy_logprob_fused", p + 2, 16, p, p, p, p, M, V, None, BF16, None)
    with pytest.raises(_lib.VyomHipError, match="vy_logprob_fused: bf16 only"):
        _lib.call("vy_logprob_fused", p, 16, p, p, p, p, M, V, None, F32, None)
    with pytest.raises(_lib.VyomHipError, match="exceeds the 65536 columns"):
        _lib.call("vy_logprob_fused", p, 65544, p, p, p, p, M, 65537, None, BF16, None)
    with pytest.raises(_lib.VyomHipError, match="bad dtype"):
        _lib.call("vy_logprob_fwd", p, 16, p, p, p, p, M, V, None, 7, None)


def test_dpo_loss_rejects_unequal_lengths():
    import torch
    import vyomai_amd as V
    m = V.ModelForCausalLM(V.Config(vocab_size=64, hidden_size=64, intermediate_size=64, num_hidden_layers=1,
                                    num_attention_heads=1, num_key_value_heads=1, max_position_embeddings=32))
    batch = {"chosen": torch.zeros(2, 5, dtype=torch.long), "rejected": torch.zeros(2, 6, dtype=torch.long),
             "chosen_mask": torch.ones(2, 5), "rejected_mask": torch.ones(2, 6)}
    with pytest.raises(ValueError, match="dpo_collate"):
        m.dpo_loss(batch, ref_model=m)
    batch = {k: v[:, :5] for k, v in batch.items()}
    with pytest.raises(ValueError, match="exactly one of ref_model and ref_logprobs"):
        m.dpo_loss(batch)
    with pytest.raises(ValueError, match="selection_mask"):
        m.sequence_logprobs(batch["chosen"], torch.ones(2, 4))


def test_logprob_rows_shift_labels_and_mask():
    """The row operands of the kernels: the notebook's shift on labels AND mask, the last position weightless, an empty
    mask all zeros (no 0 / 0)."""
    import torch
    from vyomai_amd.autograd_train import logprob_rows
    ids = torch.arange(10).view(2, 5)
    mask = torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0, 0.0]])
    labels, w = logprob_rows(ids, mask)
    assert labels.tolist() == [1, 2, 3, 4, 0, 6, 7, 8, 9, 0]
    assert w.tolist() == [[0.0, 0.5, 0.5, 0.0, 0.0], [0.0] * 5]
    assert w.dtype == torch.float32


def dpo_fp64(pi_c, pi_r, ref_c, ref_r, beta):
    """The notebook's compute_dpo_loss restated in fp64 numpy -> (loss, chosen reward, rejected reward, DPO logits)."""
    pi_c, pi_r, ref_c, ref_r = (np.asarray(a, dtype=np.float64) for a in (pi_c, pi_r, ref_c, ref_r))
    z = (pi_c - pi_r) - (ref_c - ref_r)
    return np.logaddexp(0.0, -beta * z).mean(), (pi_c - ref_c).mean(), (pi_r - ref_r).mean(), z


@pytest.mark.parametrize("case", ["a", "b"])
def test_golden_agrees_with_an_fp64_restatement(golden, case):
    g = golden("dpo")
    lp = [g[f"{case}.{k}"] for k in ("pi.chosen", "pi.rejected", "ref.chosen", "ref.rejected")]
    for a in lp:
        assert a.shape == (D.PAIRS,) and a.dtype == np.float64 and np.isfinite(a).all()
    for beta in D.BETAS:
        loss, rc, rr, _ = dpo_fp64(*lp, beta)
        assert abs(loss - float(g[f"{case}.loss.{beta}"])) < 1e-6, (beta, loss, float(g[f"{case}.loss.{beta}"]))
        assert abs(rc - float(g[f"{case}.reward.chosen"])) < 1e-6
        assert abs(rr - float(g[f"{case}.reward.rejected"])) < 1e-6
    assert abs(float(g[f"{case}.train.loss"][0]) - float(g[f"{case}.loss.{D.GRAD_BETA}"])) < 1e-6


@pytest.mark.parametrize("case", ["a", "b"])
def test_golden_tells_a_model_from_none(golden, case):
    """beta = 0.1 keeps the loss within 7e-3 of ln 2 whatever the model says; the beta = 1 loss must not, and the
    per-pair DPO logits must take both signs.  Every bar the GPU test reads from the file is there and positive."""
    g = golden("dpo")
    lp = [g[f"{case}.{k}"] for k in ("pi.chosen", "pi.rejected", "ref.chosen", "ref.rejected")]
    z = dpo_fp64(*lp, 1.0)[3]
    assert abs(float(g[f"{case}.loss.1.0"]) - math.log(2.0)) > 3e-2
    assert (z > 0).any() and (z < 0).any(), z
    assert np.abs(lp[0] - lp[2]).min() > 1e-2          # the policy is not the frozen model
    gaps = [f"{case}.gap.logp", f"{case}.gap.dx"] + [f"{case}.gap.loss.{b}" for b in D.BETAS] \
        + [f"{case}.gap.d.{n}" for n in D.TRAINED]
    for k in gaps:
        assert 0.0 < float(g[k]) < 0.1, (k, float(g[k]))
    for n in D.TRAINED:
        assert np.abs(g[f"{case}.d.{n}"]).max() > 0 and g[f"{case}.train.w.{n}"].shape == g[f"{case}.d.{n}"].shape
    assert g[f"{case}.dx"].shape[:2] == (2 * D.PAIRS, D.L)
    assert g[f"{case}.train.loss"].shape == (D.TRAIN_STEPS,)


def test_batch_has_the_collate_layout():
    b = D.batch("a")
    for key in ("chosen", "rejected"):
        ids, mask = b[key], b[key + "_mask"]
        assert ids.shape == mask.shape == (D.PAIRS, D.L) and ids.dtype == np.int64
        for i in range(D.PAIRS):
            p = D.PROMPT_LEN[i]
            assert (ids[i, :p] == b["chosen"][i, :p]).all()            # shared prompt
            assert (mask[i, :p + 1] == 0).all() and mask[i].sum() >= 3  # prompt + 1 masked
            n = int((ids[i] != 0).sum())
            assert (ids[i, n:] == 0).all() and (mask[i, n:] == 0).all() and (mask[i, p + 1:n] == 1).all()
    assert (b["chosen"] != b["rejected"]).any()
