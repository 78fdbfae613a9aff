"""tests/colsum_rule.py is a reference worth holding the kernels to: every planted mutation of the summation order moves
at least a fifth of the columns on every slab of the GPU test where it changes the sequence of adds at all, plain sums
are not the rule, and the slice rule is the library's."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import colsum_rule as R
from tests import stream_cases as S

ROOT = Path(__file__).resolve().parents[1]
FIFTH = 0.2


def slabs_and_slices():
    """(W, N, slices) of every slab test_colsum_rule_gpu.py sums: the crafted ones, sliced by the rule, and one of the
    two QK-norm slabs per case, always in one slice."""
    out = [(W, N, R.slices_rule(W)) for W, N in R.SLABS]
    out += [(R.qk_slab_rows(*case), case[3], 1) for case in R.QK_CASES]
    return out


def test_the_shapes_reach_every_branch_of_the_order():
    shapes = slabs_and_slices()
    assert [R.qk_slab_rows(*c) for c in R.QK_CASES] == [8, 2, 75, 75]
    for m in R.MUTATIONS:
        assert any(R.mutation_applies(m, W, sl) for W, _, sl in shapes), m
    assert [W for W, _, sl in shapes if R.mutation_applies("floor_rps", W, sl)] == [70]
    assert [W for W, _, sl in shapes if R.mutation_applies("sixteen_slices", W, sl)] == [75, 75]
    assert len(R.slice_sums(np.zeros((70, 1), R.F32), 16)) == 14          # 14 slices of 5 exist, not 16
    assert [w0 for w0, _ in R.slice_sums(np.zeros((64, 1), R.F32), 16)] == list(range(0, 64, 4))


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_moves_a_fifth_of_the_columns(mutation):
    for W, N, slices in slabs_and_slices():
        if not R.mutation_applies(mutation, W, slices):
            continue
        slab = R.slab_data(W, N, R.case_seed(W, N))
        share = R.changed_share(R.ordered_colsum(slab, slices), R.ordered_colsum(slab, slices, mutation=mutation))
        print(f"  {mutation} at {W} x {N} in {slices} slice(s): {share:.2f} of the columns change")
        assert share >= FIFTH, (mutation, W, N, share)


def test_a_mutation_that_does_not_apply_changes_nothing():
    """mutation_applies leaves out only what is the same sequence of adds."""
    for W, N, slices in slabs_and_slices():
        slab = R.slab_data(W, N, R.case_seed(W, N))
        want = R.ordered_colsum(slab, slices)
        for m in ("sequential_rows", "pairwise_groups", "reverse_slices", "floor_rps"):
            if not R.mutation_applies(m, W, slices):
                assert R.changed_share(want, R.ordered_colsum(slab, slices, mutation=m)) == 0.0, (m, W, N)


def test_plain_sums_are_not_the_rule():
    for W, N in R.SLABS:
        if W < 50:
            continue
        slab = R.slab_data(W, N, R.case_seed(W, N))
        want = R.ordered_colsum(slab, R.slices_rule(W))
        plain = np.sum(slab, axis=0, dtype=R.F32)
        rounded = np.sum(slab.astype(np.float64), axis=0).astype(R.F32)
        print(f"  {W} x {N}: np.sum differs in {R.changed_share(want, plain):.2f}, the rounded fp64 sum in "
              f"{R.changed_share(want, rounded):.2f} of the columns")
        assert R.changed_share(want, plain) > 0 and R.changed_share(want, rounded) > 0
        # ... and the rule is a sum: within W roundings of the exact one
        bound = W * 2.0 ** -24 * np.sum(np.abs(slab.astype(np.float64)), axis=0)
        assert np.all(np.abs(want.astype(np.float64) - np.sum(slab.astype(np.float64), axis=0)) <= bound)


def test_accumulate_adds_the_total_onto_the_base():
    slab = R.slab_data(70, 72, 7)
    base = np.full(72, 3.0, R.F32)
    total = R.ordered_colsum(slab, 16)
    assert np.array_equal(R.ordered_colsum(slab, 16, base), base + total)


def test_slice_rule_is_the_librarys():
    src = (ROOT / "vyomai_amd" / "csrc" / "vy_common.h").read_text()
    m = re.search(r"static inline int vy_ln_colsum_slices\(int WB\) \{ return WB >= (\d+) \? (\d+) : (\d+); \}", src)
    assert m, "vy_ln_colsum_slices is no longer the one-line threshold this test reads"
    at, many, few = (int(g) for g in m.groups())
    for W in (63, 64, 65, 70, 512):
        assert R.slices_rule(W) == (many if W >= at else few) == S.ln_colsum_slices(W), W


def test_qk_slab_rows_are_the_librarys():
    from vyomai_amd import _lib
    lib = _lib.load()
    for T, h, hk, dh in R.QK_CASES + ((16384, 16, 8, 128), (4096, 32, 8, 64)):
        assert lib.vy_qknorm_bwd_ws_floats(T, h, hk, dh) == R.qk_slab_rows(T, h, hk, dh) * 2 * dh
