"""The order in which the norm backwards add the rows of their fp32 partial slabs (vyomai_amd/csrc/vy_colsum.h), restated
in numpy float32.  Shared by test_colsum_rule_cpu.py (every planted mutation of the order moves the result; plain sums
would not pass as a reference) and test_colsum_rule_gpu.py (the riding workgroups of the grouped weight-gradient launch
and the stand-alone launches under LayerNorm, RMSNorm and QK-norm give exactly these bits).  Pure CPU.

The order, for a slab of W rows cut into `slices` row slices:

  rps = ceil(W / slices); slice i is rows [i rps, min(W, (i + 1) rps)); a slice that would start at or past W does not
  exist (W = 70: 14 slices of 5).
  Within a slice, row group g = 0..3 starts from 0.f and adds rows w0 + g, w0 + g + 4, ... in increasing order.
  The four group sums are added as ((p0 + p1) + p2) + p3.
  One slice: (base or 0.f) + sum.  Several: the slice sums are added from 0.f in slice order, then (base or 0.f) + total.

The sums hold no product, so there is nothing for the device to contract: an fp32 add in numpy is the device's add, bit
for bit (the library is built without fast-math).  The data is made for the order to matter: standard normal values
scaled by 2^k, k uniform in -6..6, so nearly every add rounds."""
import numpy as np

F32 = np.float32

# the crafted slabs (W, N) of the GPU test.  1 x 64, 3 x 8: groups without a row.  50 x 776: one slice, a ragged
# 64-column block.  63 x 136: one slice, groups of 16 / 16 / 16 / 15 rows, a partial batch of eight loads.  64 x 64:
# sixteen slices of four rows.  70 x 72: 14 slices that exist, 2 that do not.  512 x 768: the training shape's slab.
SLABS = ((1, 64), (3, 8), (50, 776), (63, 136), (64, 64), (70, 72), (512, 768))
# QK-norm (T, h, hk, dh): 8 slab rows; 2 rows with 9 of 16 lanes live; twice 75 rows, which sixteen slices would change
QK_CASES = ((40, 4, 2, 64), (10, 2, 1, 72), (400, 4, 2, 64), (100, 8, 4, 128))
QK_MAX_ROWS = 1024

MUTATIONS = ("sequential_rows", "pairwise_groups", "one_slice", "reverse_slices", "floor_rps", "sixteen_slices")


def slices_rule(W):
    """vy_ln_colsum_slices (vy_common.h): the slices of a LayerNorm or RMSNorm slab.  QK-norm always takes one."""
    return 16 if W >= 64 else 1


def qk_slab_rows(T, h, hk, dh):
    """Rows of the vy_qknorm_bwd slab (vy_qknorm_bwd_ws_floats / (2 dh)): one per workgroup, a workgroup takes `iters`
    whole slices of 256 >> lg (token, head) units."""
    lg = 0
    while (1 << lg) < dh // 8:
        lg += 1
    slices = -(-T * (h + hk) // (256 >> lg))
    iters = -(-slices // QK_MAX_ROWS)
    return -(-slices // iters)


def slab_data(W, N, seed):
    """float32 [W, N]: standard normal times 2^k, k uniform in -6..6."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((W, N)) * 2.0 ** rng.integers(-6, 7, size=(W, N))).astype(F32)


def case_seed(W, N):
    return 1000 * W + N


def _slice_sum(rows, mutation):
    zero = np.zeros(rows.shape[1], F32)
    if mutation == "sequential_rows":
        a = zero
        for w in range(rows.shape[0]):
            a = a + rows[w]
        return a
    p = []
    for g in range(4):
        a = zero
        for w in range(g, rows.shape[0], 4):
            a = a + rows[w]
        p.append(a)
    if mutation == "pairwise_groups":
        return (p[0] + p[1]) + (p[2] + p[3])
    return ((p[0] + p[1]) + p[2]) + p[3]


def slice_sums(slab, slices, mutation=None):
    """-> [(w0, float32 [N])]: the first row and the sum of every slice that exists, in slice order."""
    W = slab.shape[0]
    rps = W // slices if mutation == "floor_rps" else -(-W // slices)
    return [(w0, _slice_sum(slab[w0:min(W, w0 + rps)], mutation)) for w0 in range(0, min(W, slices * rps), rps)]


def add_slices(sums, base=None):
    """Slice sums [N] in slice order (+ base) -> float32 [N]."""
    zero = np.zeros_like(sums[0])
    if len(sums) == 1:
        total = sums[0]
    else:
        total = zero
        for s in sums:
            total = total + s
    return (zero if base is None else base.astype(F32)) + total


def ordered_colsum(slab, slices, base=None, mutation=None):
    """The column sums of slab [W, N] (float32) in the order above -> float32 [N]; base: what an accumulating call adds
    onto.  mutation: one of MUTATIONS, a planted fault of the order."""
    slab = np.ascontiguousarray(slab, dtype=F32)
    assert slab.ndim == 2 and slab.dtype == F32
    if mutation == "one_slice":
        slices = 1
    if mutation == "sixteen_slices":
        slices = 16
    sums = [s for _, s in slice_sums(slab, slices, mutation)]
    if mutation == "reverse_slices":
        sums = sums[::-1]
    return add_slices(sums, base)


def mutation_applies(mutation, W, slices):
    """Whether the fault changes the sequence of adds at all on W rows in `slices` slices (the caller's choice).
      sequential_rows   needs a group with two rows: with at most four rows a slice ((r0 + r1) + r2) + r3 IS the
                        sequential sum (0.f + r = r).
      pairwise_groups   needs four groups with a row: (p0 + p1) + (p2 + 0.f) is ((p0 + p1) + p2) + 0.f.
      one_slice, reverse_slices   need several slices.
      floor_rps         needs W to be no multiple of the slice count.
      sixteen_slices    is for the caller that fixes one slice (QK-norm), where the slice rule would say sixteen."""
    rps = -(-W // slices)
    if mutation == "sequential_rows":
        return min(W, rps) >= 5
    if mutation == "pairwise_groups":
        return min(W, rps) >= 4
    if mutation in ("one_slice", "reverse_slices"):
        return slices > 1
    if mutation == "floor_rps":
        return slices > 1 and W % slices != 0
    if mutation == "sixteen_slices":
        return slices == 1 and slices_rule(W) == 16
    raise ValueError(mutation)


def changed_share(a, b):
    """Share of the columns whose bits differ."""
    return float(np.mean(a.view(np.uint32) != b.view(np.uint32)))
