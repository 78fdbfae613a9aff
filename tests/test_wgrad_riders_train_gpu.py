"""The riders of the vocabulary weight gradient inside FlatTrainer: the W^T refresh and the arena zeroing ride in the
head's weight-gradient launch (switch on) or run as the launches they were (switch off).  The work only moves data, so
master parameters, gradients, m, v and every cached W^T must be EQUAL after every step; the loss is compared with
allclose (its sum is a float atomic over rows, not order-fixed with or without riders).

One-layer decoder, d = 768, 12 heads, vocabulary 8200, 8 x 512 tokens: the head takes the 256 x 256 launch (99 tiles x 2
M-splits) and every weight-gradient launch has at most two M-splits, so all gradients are order-free."""
import numpy as np
import pytest
import torch

import vyomai_amd as V
from vyomai_amd import autograd_train as AT
from vyomai_amd import recipe
from vyomai_amd.training import FlatTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build(riders, **kw):
    cfg = V.EncoderConfig(hidden_size=768, num_attention_heads=12, num_hidden_layers=1, vocab_size=8200,
                          max_position_embeddings=512, hidden_dropout_prob=0.0)
    m = V.DecoderModel(cfg, "rope", None)
    recipe.load_recipe_(m)
    m = m.to(DEV).train()
    return m, FlatTrainer(m, lr=LR, wgrad_riders=riders, **kw)


def ids():
    return torch.from_numpy(np.ascontiguousarray(recipe.token_ids("riders.ids", (8, 512), 3, 8200))).to(DEV)


def snapshot(m, tr):
    owners = {id(p) for p in m.parameters()} | {id(mod) for mod in m.modules()}
    wts = [e[3].clone() for e in AT._WT.entries if e[0]() is not None and id(e[0]()) in owners]
    torch.cuda.synchronize()
    return dict(master=tr.arena.master.clone(), grad=tr.arena.grad.clone(), m=tr.m.clone(), v=tr.v.clone(), wt=wts,
                stats=dict(tr.rider_stats))


def same(a, b):
    for k in ("master", "grad", "m", "v"):
        assert torch.equal(a[k], b[k]), k
    assert len(a["wt"]) == len(b["wt"]) and len(a["wt"]) >= 4
    for x, y in zip(a["wt"], b["wt"]):
        assert torch.equal(x, y)


def run(riders, variant):
    """-> [(loss, snapshot)] per step."""
    kw = {"accumulate_steps": 2} if variant == "accumulate" else {}
    m, tr = build(riders, **kw)
    x = ids()
    out = []
    scale = 2.0 if variant == "scaled" else 1.0

    def loss_fn():
        loss = m.clm_loss(x, x)
        return loss * scale if variant == "scaled" else loss

    def boom():
        m.clm_loss(x, x)          # the forward runs (and claims the pending zeroing), then the step fails
        raise ValueError("boom")

    for step in range(4 if variant == "accumulate" else 3):
        if variant == "raises" and step == 1:
            with pytest.raises(ValueError, match="boom"):
                tr.train_step(boom)
            assert AT.lazy_zero.PENDING.ranges is None and AT.lazy_zero.PENDING.claim is None
        if variant == "by_hand":
            tr.zero_grad()
            assert AT.lazy_zero.PENDING.ranges is None      # a user's zero_grad() is eager
            loss = loss_fn()
            tr.backward(loss)
            tr.optimizer_step()
            loss = loss.detach()
        else:
            loss = tr.train_step(loss_fn)
        assert AT.lazy_zero.PENDING.ranges is None
        out.append((float(loss), snapshot(m, tr)))
    return out, tr.arena.numel * 4


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(riders, variant):
        if (riders, variant) not in cache:
            cache[(riders, variant)] = run(riders, variant)
        return cache[(riders, variant)]
    return get


LR = 1e-3


def close_after_accumulation(a, b):
    """accumulate_steps = 2, the step that ends the FIRST window: the second micro-step's atomics land on the first
    one's NON-zero sums, so a gradient is a sum of four addends (2 micro-steps x 2 M-splits) in arrival order and is not
    order-fixed in the parent either.  Bounds from the number format and the optimizer, not from the riders:
      grad    each of the <= 3 roundings of a 4-term sum is at most half an ulp of a partial sum, which no more than
              doubles the largest gradient of the arena: 3 x 2^-24 x 2 max|g|
      m, v    m is (1 - beta1) g after one update, v is (1 - beta2) g^2: the gradient's bound, times 2 max|g| for v
      master  one AdamW update moves a weight by at most lr (1 + weight_decay) whatever its gradient (|m^ / (sqrt(v^) +
              eps)| <= 1 at step 1), so two runs whose gradients differ in their last bits are at most twice that apart.
    From the second window on the two runs' weights differ in their last bits and their bf16 activations with them: only
    the loss and the counters are compared there."""
    gmax = float(b["grad"].abs().max())
    dg = 6 * 2.0 ** -24 * gmax
    got = {k: float((a[k] - b[k]).abs().max()) for k in ("grad", "m", "v", "master")}
    print("accumulate, first window: max |on - off|", got, "gradient bound", dg)
    assert got["grad"] <= dg
    assert got["m"] <= 2 * dg
    assert got["v"] <= 2 * 2 * gmax * dg
    assert got["master"] <= 2 * LR * 1.01
    assert len(a["wt"]) == len(b["wt"])


@pytest.mark.parametrize("variant", ["plain", "scaled", "accumulate", "raises", "by_hand"])
def test_riders_on_equals_off(runs, variant):
    (on, arena_bytes), (off, _) = runs(True, variant), runs(False, variant)
    for step, ((la, a), (lb, b)) in enumerate(zip(on, off)):
        if variant == "accumulate" and step == 1:
            close_after_accumulation(a, b)
        elif variant != "accumulate" or step == 0:     # (accumulation, step 0 adds to zeros: order-free, equal)
            same(a, b)
        assert abs(la - lb) <= (1e-3 if variant == "accumulate" and step > 1 else 1e-5) * abs(lb)
    for step, (_, s) in enumerate(off):
        st = s["stats"]
        assert st["zero_rode_bytes"] == 0 and st["wt_rode_tiles"] == 0
    for step, (_, s) in enumerate(on):
        st = s["stats"]
        print(variant, step, st)
        if variant != "accumulate" or step % 2 == 0:        # (a window's second micro-step fills nothing)
            assert st["zero_rode_bytes"] + st["zero_plain_bytes"] == arena_bytes
        if step == 0:
            continue   # the first step registers the W^T copies and marks the carrier's parameters: nothing to ride yet
        if variant == "accumulate" and step % 2 == 1:
            continue   # the weights did not change: no refresh
        assert st["wt_rode_tiles"] > 0, "the W^T refresh did not ride"
        if variant == "plain" or variant == "raises":
            assert st["zero_rode_bytes"] > 0, "no part of the arena was cleared by riders"
        else:
            # the root of the loss is not the head node (scaled: MulBackward; accumulation: the 1 / k division), or
            # zero_grad() was the user's: the plain fill, all of it
            assert st["zero_rode_bytes"] == 0 and st["zero_plain_bytes"] == arena_bytes


def test_off_is_the_parent_path(runs):
    """Switch off: no W^T tile and no byte rides, the whole arena is filled at once."""
    off, arena_bytes = runs(False, "plain")
    for _, s in off:
        assert s["stats"] == {"zero_rode_bytes": 0, "zero_plain_bytes": arena_bytes, "wt_rode_tiles": 0,
                              "wt_plain_tiles": s["stats"]["wt_plain_tiles"]}
