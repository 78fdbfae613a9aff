"""The gradient arena's deferred zeroing: who may clear what, and when.

FlatTrainer.train_step() clears at once only the gradients that the vocabulary weight-gradient launch accumulates into
and POSTS the rest of the arena here.  LMHeadLossFn.forward CLAIMS the posted list when its backward will be that
launch; FlatTrainer.backward() SETTLES it: the claim is accepted only if the loss's grad_fn is the claiming node itself
-- then that node's backward is the first thing autograd runs, nothing can write the arena before it, and the launch
clears the ranges with rider workgroups (ops.linear_wgrad_riders).  In every other case the list is filled with plain
launches before autograd starts.  Nothing here calls the kernel library: the plain fill is Tensor.zero_()."""
from __future__ import annotations

from typing import List, Optional

import torch


class ZeroClaim:
    """What a node took from the pending list.  ranges is None once they have been cleared (or the claim was void)."""

    def __init__(self, owner, ranges: List[torch.Tensor], stats: Optional[dict]) -> None:
        self.owner, self.ranges, self.stats, self.accepted = owner, ranges, stats, False


def _meets(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


class PendingZero:
    def __init__(self) -> None:
        self.owner = None
        self.ranges: Optional[List[torch.Tensor]] = None
        self.claim: Optional[ZeroClaim] = None
        self.stats: Optional[dict] = None

    def post(self, owner, ranges: List[torch.Tensor], stats: dict) -> None:
        """ranges: contiguous fp32 views that must be zero before the first kernel that accumulates into them."""
        self.flush()   # (a list somebody else left: it is filled, never lost)
        ranges = [r for r in ranges if r.numel() > 0]
        if ranges:
            self.owner, self.ranges, self.stats = owner, ranges, stats

    def claim_for(self, *targets: Optional[torch.Tensor]) -> Optional[ZeroClaim]:
        """targets: the gradients the claiming launch itself accumulates into.  They must already be clear, i.e. meet
        none of the pending ranges; a list is claimed once."""
        if self.ranges is None or self.claim is not None:
            return None
        if any(t is not None and _meets(t, r) for t in targets for r in self.ranges):
            return None
        self.claim = ZeroClaim(self.owner, self.ranges, self.stats)
        return self.claim

    def settle(self, owner, root) -> Optional[ZeroClaim]:
        """Before owner's loss.backward(): accept the claim if `root` (the loss's grad_fn) carries it, else fill the list
        plainly.  -> the accepted claim (the caller voids it when backward has returned), or None."""
        if self.ranges is None or self.owner is not owner:
            return None
        claim = self.claim
        if claim is not None and root is not None and getattr(root, "zero_claim", None) is claim:
            claim.accepted = True
            self.owner = self.ranges = self.claim = self.stats = None
            return claim
        self.flush()
        return None

    def flush(self) -> None:
        """Fill what is pending with plain launches; a claim on it is void."""
        if self.ranges is not None:
            for r in self.ranges:
                r.zero_()
                if self.stats is not None:
                    self.stats["zero_plain_bytes"] += r.numel() * 4
        if self.claim is not None:
            self.claim.ranges = None
        self.owner = self.ranges = self.claim = self.stats = None

    def drop(self, owner) -> None:
        """A step that raised: nothing stays pending or claimed (the next zero_grad() fills the whole arena)."""
        if self.owner is owner:
            if self.claim is not None:
                self.claim.ranges = None
            self.owner = self.ranges = self.claim = self.stats = None


def take(claim: Optional[ZeroClaim]) -> Optional[List[torch.Tensor]]:
    """The ranges of an accepted claim, once: the caller clears them now."""
    if claim is None or not claim.accepted or claim.ranges is None:
        return None
    ranges, claim.ranges = claim.ranges, None
    return ranges


def complement(total: int, taken) -> list:
    """[0, total) minus the (lo, hi) element ranges in `taken` -> [(lo, hi), ...] in order."""
    out, at = [], 0
    for lo, hi in sorted(taken):
        if lo > at:
            out.append((at, lo))
        at = max(at, hi)
    if at < total:
        out.append((at, total))
    return out


PENDING = PendingZero()
