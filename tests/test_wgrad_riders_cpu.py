"""The riders of the vocabulary weight gradient without a GPU: the new symbols are exported and declared, and the
pending-list logic of the deferred arena zeroing (vyomai_amd/lazy_zero.py: post, claim, settle, flush, drop) on CPU
tensors -- it never calls the kernel library."""
import os
import re

import torch

from vyomai_amd import _lib, lazy_zero

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "vyom_hip.h")).read()
    lib = _lib.load()
    for name in ("vy_linear_wgrad_riders", "vy_transpose_batched_range"):
        assert re.search(r"\bint %s\(" % name, header)
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES["vy_linear_wgrad_riders"]) == 21
    assert lib.vy_abi_version() == 5, "additive symbols: the ABI version stays"
    import ctypes
    assert ctypes.sizeof(_lib.VyZeroRideDesc) == 24


class Node:
    """Stands in for an autograd node (ctx is the node: what forward sets on ctx, loss.grad_fn shows)."""
    zero_claim = None


def arena():
    g = torch.ones(100)
    stats = {"zero_plain_bytes": 0}
    own = [g[10:20], g[50:52]]                                      # what the carrier accumulates into
    rest = [g[lo:hi] for lo, hi in lazy_zero.complement(100, [(50, 52), (10, 20)])]
    return g, stats, own, rest


def test_complement():
    assert lazy_zero.complement(100, [(50, 52), (10, 20)]) == [(0, 10), (20, 50), (52, 100)]
    assert lazy_zero.complement(10, [(0, 10)]) == []
    assert lazy_zero.complement(10, [(0, 4), (4, 6)]) == [(6, 10)]
    assert lazy_zero.complement(10, []) == [(0, 10)]


def test_claim_accepted_only_for_the_root_node():
    p = lazy_zero.PendingZero()
    owner = object()
    g, stats, own, rest = arena()
    p.post(owner, rest, stats)
    node = Node()
    node.zero_claim = p.claim_for(*own)
    assert node.zero_claim is not None and not node.zero_claim.accepted
    assert p.claim_for(*own) is None                                # a list is claimed once
    assert lazy_zero.take(node.zero_claim) is None                  # not before the trainer has accepted it
    claim = p.settle(owner, node)
    assert claim is node.zero_claim and claim.accepted and p.ranges is None
    assert bool((g == 1).all())                                     # nothing filled: the carrier will
    got = lazy_zero.take(claim)
    assert [(r.data_ptr(), r.numel()) for r in got] == [(r.data_ptr(), r.numel()) for r in rest]
    assert lazy_zero.take(claim) is None                            # once
    assert stats["zero_plain_bytes"] == 0


def test_other_root_or_no_claim_is_filled_plainly():
    for root_is_other in (True, False):
        p = lazy_zero.PendingZero()
        owner = object()
        g, stats, own, rest = arena()
        p.post(owner, rest, stats)
        node = Node()
        if root_is_other:
            node.zero_claim = p.claim_for(*own)
        assert p.settle(owner, Node() if root_is_other else node) is None
        want = torch.zeros(100)
        want[10:20] = 1
        want[50:52] = 1
        assert torch.equal(g, want) and stats["zero_plain_bytes"] == 88 * 4
        assert lazy_zero.take(node.zero_claim) is None              # the claim is void
        assert p.ranges is None and p.claim is None


def test_a_target_inside_the_pending_list_is_no_carrier():
    p = lazy_zero.PendingZero()
    g, stats, own, rest = arena()
    p.post(object(), rest, stats)
    assert p.claim_for(g[15:25]) is None                            # meets a pending range: it was not cleared at once
    assert p.claim_for(own[0], None) is not None


def test_settle_of_another_owner_and_root_none():
    p = lazy_zero.PendingZero()
    owner = object()
    g, stats, own, rest = arena()
    p.post(owner, rest, stats)
    node = Node()
    node.zero_claim = p.claim_for(*own)
    assert p.settle(object(), node) is None and p.ranges is not None   # not this owner's list: left alone
    assert p.settle(owner, None) is None                               # a scaled loss (accumulation): plain fill
    assert float(g.sum()) == 12.0 and lazy_zero.take(node.zero_claim) is None


def test_drop_and_repost():
    p = lazy_zero.PendingZero()
    owner = object()
    g, stats, own, rest = arena()
    p.post(owner, rest, stats)
    node = Node()
    node.zero_claim = p.claim_for(*own)
    p.drop(owner)                                                   # the step raised
    assert p.ranges is None and p.claim is None and node.zero_claim.ranges is None
    assert bool((g == 1).all())                                     # dropped, not filled: the next zero_grad() fills all
    assert p.settle(owner, node) is None and lazy_zero.take(node.zero_claim) is None
    # a list somebody left is filled by the next post, never lost
    p.post(owner, rest, stats)
    g2, stats2, _, rest2 = arena()
    p.post(object(), rest2, stats2)
    assert float(g.sum()) == 12.0 and bool((g2 == 1).all()) and stats["zero_plain_bytes"] == 88 * 4


def test_ctx_is_the_grad_fn():
    """What LMHeadLossFn.forward relies on: an attribute set on ctx is visible on the output's grad_fn."""
    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.zero_claim = "mine"
            return x * 2

        @staticmethod
        def backward(ctx, g):
            return g * 2

    x = torch.ones(3, requires_grad=True)
    y = F.apply(x)
    assert getattr(y.grad_fn, "zero_claim", None) == "mine"
    assert getattr((y * 2).grad_fn, "zero_claim", None) is None


def test_carrier_ranges_keep_the_pending_list_aligned():
    """A carrier with an odd number of elements (the vocabulary bias: 50265): its range runs up to the next parameter,
    so every pending range starts on a parameter offset -- 16-byte aligned, as the launcher demands of a zero range."""
    from vyomai_amd.training import ALIGN, FlatTrainer

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(16, 24)
            self.head = torch.nn.Linear(16, 13)
            self.b = torch.nn.Linear(16, 8)

    m = M()
    tr = FlatTrainer(m, compute_dtype=torch.float32)
    assert tr._carriers() == []
    m.head.weight._vy_carrier = m.head.bias._vy_carrier = True
    ranges = tr._carriers()
    offs = dict(zip((id(p) for p in tr.arena.params), tr.arena.offsets))
    assert [lo for lo, _ in ranges] == [offs[id(m.head.weight)], offs[id(m.head.bias)]]
    rest = lazy_zero.complement(tr.arena.numel, ranges)
    assert all(lo % ALIGN == 0 and hi % ALIGN == 0 for lo, hi in ranges + rest)
    assert sum(hi - lo for lo, hi in ranges + rest) == tr.arena.numel
    assert ranges[1][1] - ranges[1][0] > 13          # the pad behind the odd bias stays with it
