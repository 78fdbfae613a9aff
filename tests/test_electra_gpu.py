"""ELECTRA / masked-LM pre-training on the MI355X: the Gumbel noise, vy_xent_sample_*, vy_bce_head_*, vy_mlm_mask against
fp64 / numpy restatements, the model against the REAL reference's fixture (tests/golden/electra.npz, made by
make_golden_electra.py) in fp32 and bf16, the shared embedding table under FlatTrainer, and an undirected step.

Bars.  Elementwise results: elementwise_bars (test_causal_lm_gpu.py).  Sums over rows (dw, db, the BCE loss sum): the
bars test_bwd_kernels_gpu.py holds vy_linear_wgrad to at the same dtype (bf16: 2e-3 sqrt(M) absolute + 1e-3 relative;
fp32: 8e-6 sqrt(M) + 1e-5).  Sampler: the winner's fp64 score is within 2^-22 max(1, max|s|) of the row maximum, two
fp32 roundings of a fused multiply-add, one on each of the two scores compared.  Against the plain xent kernels: lse,
count, the gradient and each row's loss term bit for bit; the batch loss_sum, a float atomic in arrival order in both
kernels, within a reordering of its terms.  Model, fp32: losses
2e-5 max(1, |ref|), gradients rel_err < 1e-4, trained weights mean 2e-6 / max 2 * steps * LR + 1e-5 (the bars of
test_causal_lm_gpu.py); bf16: 3 x the reference's own stored bf16-vs-fp32 gap of that quantity, gradient bars floored
at test_dpo_gpu.py's PARAM_FLOOR."""
import math

import numpy as np
import pytest
import torch

from tests.golden import cases_electra as E
from tests.test_causal_lm_gpu import BF, DEV, T, elementwise_bars, rel_err
from tests.test_dpo_gpu import PARAM_FLOOR
from tests.test_electra_cpu import big_ids, mlm_invariants, mlm_proportions
from tests.test_kernels_gpu import check, check_exact, rnd

pytestmark = pytest.mark.gpu
SEED, OFFSET = 0x1234567887654321, (5 << 40) + 77      # both halves of the 64-bit seed and offset in use
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------
# numpy restatements
# ------------------------------------------------------------------------------------------


def philox7(c0, c1, c2, c3, k0, k1):
    """Philox4x32-7 over uint64 arrays holding 32-bit words -> four arrays of words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def noise_u(M, V, seed, offset):
    """The uniforms behind noise(m, v): word v & 3 of Philox on {v / 4, m, offset}, top 24 bits * 2^-24 (fp64)."""
    m = np.arange(M, dtype=np.uint64)[:, None]
    q = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    r = philox7(q, m, offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(r, axis=-1).reshape(M, -1)[:, :V]
    return (words >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def gumbel64(u):
    return -np.log(-np.log(u + 1e-9) + 1e-9)


def mlm_numpy(ids, special, fraction, mask_id, vocab, ignore, seed, offset):
    """vy_mlm_mask restated: one Philox call per token on {i, offset}."""
    flat = ids.reshape(-1)
    i = np.arange(flat.size, dtype=np.uint64)
    r0, r1, r2, r3 = philox7(i, i >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)
    frac = float(np.float32(fraction))                       # the C ABI takes a float
    sel = ~np.isin(flat, special) & (r0.astype(np.float64) < frac * 2.0 ** 32)
    to_mask = sel & (r1.astype(np.float64) < 0.8 * 2.0 ** 32)
    to_rand = sel & ~to_mask & (r2.astype(np.float64) < 0.5 * 2.0 ** 32)
    out = np.where(to_mask, mask_id, np.where(to_rand, ((r3 * np.uint64(vocab)) >> np.uint64(32)).astype(np.int64), flat))
    return out.reshape(ids.shape), np.where(sel, flat, ignore).reshape(ids.shape), sel.reshape(ids.shape)


# ------------------------------------------------------------------------------------------
# 1. noise
# ------------------------------------------------------------------------------------------


def test_gumbel_noise():
    from vyomai_amd import ops
    M, V = 24, 1003
    a = ops.gumbel_noise(M, V, SEED, OFFSET, DEV)
    assert torch.equal(a, ops.gumbel_noise(M, V, SEED, OFFSET, DEV)), "two calls differ"
    assert not torch.equal(a, ops.gumbel_noise(M, V, SEED, OFFSET + 1, DEV)), "another offset gives the same noise"
    assert not torch.equal(a, ops.gumbel_noise(M, V, SEED + 1, OFFSET, DEV)), "another seed gives the same noise"
    g = a.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and g.min() >= -3.04 and g.max() <= 20.73, (g.min(), g.max())
    u = noise_u(M, V, SEED, OFFSET)
    mid = (u >= 2.0 ** -12) & (u <= 1 - 2.0 ** -12)
    want = gumbel64(u)
    err = np.abs(g - want) / np.maximum(1.0, np.abs(want))
    print(f"noise vs fp64 formula: {mid.mean():.4f} of the values checked, max scaled error {err[mid].max():.3e}")
    assert mid.mean() > 0.99 and err[mid].max() <= 1e-5
    # moments of the Gumbel distribution: mean = Euler's constant, variance pi^2 / 6; the standard error of the sample
    # variance is sqrt((mu4 - var^2) / n) with the fourth central moment mu4 = 27 pi^4 / 20 - ... = 14.6114 (kurtosis 5.4)
    big = ops.gumbel_noise(64, 4096, SEED, OFFSET + 9, DEV).double().cpu().numpy().ravel()
    n, var = big.size, math.pi ** 2 / 6
    se_mean, se_var = math.sqrt(var / n), math.sqrt((5.4 - 1.0) * var * var / n)
    print(f"mean {big.mean():.5f} ({(big.mean() - 0.5772) / se_mean:+.2f} se)  var {big.var():.5f} ({(big.var() - var) / se_var:+.2f} se)")
    assert abs(big.mean() - 0.5772) <= 6 * se_mean and abs(big.var() - var) <= 6 * se_var


# ------------------------------------------------------------------------------------------
# 2. vy_xent_sample_*
# ------------------------------------------------------------------------------------------


def _kernel_case(V, dtype, seed):
    """The layout of test_dpo_gpu._kernel_case for cross-entropy: poisoned pad columns inside the last 16-byte chunk,
    labels 0 and V - 1, ignored rows, one out-of-range label; one row with a logit raised by 40."""
    from vyomai_amd.autograd_train import _row_stride
    M = 24
    x = 2.0 * rnd(M, V, seed=seed)
    x[9, V // 3] += 40.0
    x = x.to(dtype)
    buf = torch.zeros((M, _row_stride(V)), dtype=dtype)
    buf[:, :V] = x
    vec = 16 // x.element_size()
    buf[:, V:(V + vec - 1) // vec * vec] = 60.0
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, V, (M,), generator=g)
    labels[0], labels[1] = 0, V - 1
    labels[torch.tensor([2, 5, 6, 11, 23])] = -100
    labels[7] = V + 3                                  # out of range: skipped, raises the flag
    return x, buf, labels


def _xent_run(kind, V, buf, labels, inv_t=None):
    """-> dict(lse, acc = [loss_sum, count], buf, sampled, flag); kind = fwd | fused, sampling when inv_t is given."""
    from vyomai_amd import ops
    b = buf.to(DEV).clone()
    lab = labels.to(DEV)
    M = b.shape[0]
    lse = torch.full((M,), 9.0, device=DEV)
    acc = torch.zeros(2, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    one = torch.ones(1, device=DEV)
    sampled = torch.full((M,), -7, dtype=torch.long, device=DEV)
    extra = () if inv_t is None else (sampled, inv_t, SEED, OFFSET)
    if kind == "fused":
        acc[1] = ((labels != -100) & (labels >= 0) & (labels < V)).sum()
        fn = ops.xent_fused_ if inv_t is None else ops.xent_sample_fused_
        fn(b[:, :V], lab, -100, lse, acc[0:1], acc[1:2], one, *extra, flag)
    else:
        fn = ops.xent_fwd if inv_t is None else ops.xent_sample_fwd
        fn(b[:, :V], lab, -100, lse, acc[0:1], acc[1:2], *extra, flag)
        assert torch.equal(b, buf.to(DEV)), "the forward kernel is read-only"
    torch.cuda.synchronize()
    return dict(lse=lse, acc=acc, buf=b, sampled=sampled, flag=int(flag.item()))


@pytest.mark.parametrize("V", [512, 1003, 50265, 65536, 70000])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_xent_sample_kernels(V, dtype):
    from vyomai_amd import ops
    from vyomai_amd._lib import VyomHipError
    atol, rtol = elementwise_bars(dtype)
    x, buf, labels = _kernel_case(V, dtype, seed=V % 97)
    M = x.shape[0]
    live = (labels != -100) & (labels >= 0) & (labels < V)
    n_live = int(live.sum())
    xd = x.double()
    lse64 = torch.where(live, torch.logsumexp(xd, dim=-1), torch.zeros((), dtype=torch.float64))
    safe = labels.clamp(0, V - 1)
    loss64 = (lse64 - xd.gather(1, safe[:, None])[:, 0])[live].sum()
    grad64 = torch.softmax(xd, dim=-1)
    grad64[torch.arange(M), safe] -= 1.0
    grad64 = torch.where(live[:, None], grad64 / n_live, torch.zeros((), dtype=torch.float64))
    fused_ok = dtype == BF and V <= 65536
    if not fused_ok:
        with pytest.raises(VyomHipError, match="vy_xent_sample_fused"):
            ops.xent_sample_fused_(buf.to(DEV)[:, :V], labels.to(DEV), -100, torch.empty(M, device=DEV),
                                   torch.zeros(1, device=DEV), torch.ones(1, device=DEV), torch.ones(1, device=DEV),
                                   torch.empty(M, dtype=torch.long, device=DEV), 1.0, SEED, OFFSET)
    noise64 = ops.gumbel_noise(M, V, SEED, OFFSET, DEV).double().cpu()
    for temperature in (1, 3):
        inv_t = float(np.float32(1.0 / temperature))
        s64 = xd * inv_t + noise64
        for kind in (("fwd", "fused") if fused_ok else ("fwd",)):
            what = f"V={V} {kind} T={temperature}"
            plain, got = _xent_run(kind, V, buf, labels), _xent_run(kind, V, buf, labels, inv_t)
            assert got["flag"] == 1 and plain["flag"] == 1, what
            check(got["lse"], lse64, atol, rtol, "lse " + what)
            print(f"{what}: loss {(got['acc'][0] / n_live).item():.7f} fp64 {(loss64 / n_live).item():.7f}")
            check(got["acc"][0] / n_live, loss64 / n_live, atol, rtol, "loss " + what)
            assert got["acc"][1].item() == n_live, what
            check_exact(got["lse"], plain["lse"], "lse vs the plain kernel, " + what)
            check_exact(got["acc"][1], plain["acc"][1], "count vs the plain kernel, " + what)
            check_exact(got["buf"], plain["buf"], "buffer vs the plain kernel, " + what)
            # loss_sum is one float atomic per live row, added in the order the rows finish: two runs of the SAME kernel
            # may differ in it.  What a kernel decides is the term of each row, so every row is run alone (one term added
            # to 0: exact) and must agree bit for bit; two orders of those n terms are each within (n - 1) u sum|t| of
            # the exact sum (u = 2^-24), so the batch sums are held to twice that
            for m in live.nonzero()[:, 0].tolist():
                one_p = _xent_run(kind, V, buf[m:m + 1], labels[m:m + 1])
                one_s = _xent_run(kind, V, buf[m:m + 1], labels[m:m + 1], inv_t)
                check_exact(one_s["acc"], one_p["acc"], f"loss term / count of row {m} vs the plain kernel, " + what)
                check_exact(one_s["lse"], one_p["lse"], f"lse of row {m} alone vs the plain kernel, " + what)
                check_exact(one_s["buf"], one_p["buf"], f"buffer of row {m} alone vs the plain kernel, " + what)
            reorder = 2 * (n_live - 1) * 2.0 ** -24 * loss64.abs().item()
            gap = (got["acc"][0] - plain["acc"][0]).abs().item()
            print(f"{what}: loss_sum {got['acc'][0].item():.7f} plain {plain['acc'][0].item():.7f} (reordering bound {reorder:.3e})")
            assert gap <= reorder, ("loss_sum vs the plain kernel beyond a reordering of its terms, " + what, gap, reorder)
            if kind == "fwd":                         # backward of the unfused form is the existing vy_xent_bwd
                ops.xent_bwd_(got["buf"][:, :V], labels.to(DEV), -100, got["lse"], torch.ones(1, device=DEV), got["acc"][1:2])
            check(got["buf"][:, :V], grad64, atol, rtol, "gradient " + what)
            assert not got["buf"][:, V:].any(), "pad columns stay zero: " + what
            k = got["sampled"].cpu()
            assert (k[~live] == -1).all(), "skipped rows give -1: " + what
            kl = k[live]
            assert (kl >= 0).all() and (kl < V).all(), what
            sl = s64[live]
            top = sl.max(dim=-1).values
            margin = 2.0 ** -22 * torch.clamp(sl.abs().max(dim=-1).values, min=1.0)
            short = top - sl.gather(1, kl[:, None])[:, 0]
            print(f"{what}: largest shortfall of a sampled score {short.max().item():.3e} (margin {margin.min().item():.3e}), "
                  f"{int((kl == sl.argmax(dim=-1)).sum())}/{n_live} are the fp64 argmax")
            assert (short <= margin).all(), what
            assert k[9] == V // 3, "the raised logit wins: " + what
            assert torch.equal(got["sampled"], _xent_run(kind, V, buf, labels, inv_t)["sampled"]), "two runs differ: " + what


# ------------------------------------------------------------------------------------------
# 3. sampling distribution
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("temperature", [1, 3])
def test_sampling_distribution(temperature):
    """argmax(x / T + Gumbel) is a draw from softmax(x / T): 8192 identical rows of 8 logits, the counts within 6
    binomial standard deviations (the epsilons of the reference's noise move the probabilities by < 1e-8)."""
    M, V = 8192, 8
    row = torch.tensor([1.5, -0.5, 0.0, 2.5, -2.0, 0.7, 1.0, -1.0])
    p = torch.softmax(row.double() / temperature, dim=-1).numpy()
    for dtype, kind in ((torch.float32, "fwd"), (BF, "fused")):
        buf = torch.zeros((M, 64), dtype=dtype)
        buf[:, :V] = row.to(dtype)
        got = _xent_run(kind, V, buf, torch.zeros(M, dtype=torch.long), float(np.float32(1.0 / temperature)))
        counts = np.bincount(got["sampled"].cpu().numpy(), minlength=V)
        sd = np.sqrt(M * p * (1 - p))
        print(f"T={temperature} {kind}: counts {counts.tolist()} expected {np.round(M * p, 1).tolist()}")
        assert counts.sum() == M and (np.abs(counts - M * p) <= 6 * sd).all(), (counts, M * p, sd)


def test_collators_on_gpu_tensors():
    """The reference-named collators take the kernels on GPU tensors: same invariants, seeded by rng.manual_seed."""
    from vyomai_amd import rng
    from vyomai_amd.pretraining import masked_language_modeling, noise, sample
    tok = E.StubTokenizer()
    ids = T(E.batch()[0]).to(DEV)
    rng.manual_seed(3)
    first = masked_language_modeling(ids, tok, fraction=0.3)
    drawn = sample(torch.zeros(6, 1003, device=DEV, dtype=BF), temperature=2.0)
    rng.manual_seed(3)
    again = masked_language_modeling(ids, tok, fraction=0.3)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert torch.equal(drawn, sample(torch.zeros(6, 1003, device=DEV, dtype=BF), temperature=2.0))
    assert not all(torch.equal(a, b) for a, b in zip(first, masked_language_modeling(ids, tok, fraction=0.3))), "offsets advance"
    mlm_invariants(ids.cpu(), first[0].cpu(), first[1].cpu(), first[2].cpu(), tok)
    assert drawn.shape == (6,) and len(set(drawn.tolist())) > 1 and 0 <= int(drawn.min()) and int(drawn.max()) < 1003
    x = torch.zeros(2, 5, 1003, device=DEV)
    x[..., 700] = 60.0
    assert sample(x, temperature=3).shape == (2, 5) and (sample(x, temperature=3) == 700).all()
    g = noise(torch.empty(3, 7, 50, device=DEV))
    assert g.shape == (3, 7, 50) and g.dtype == torch.float32 and float(g.min()) >= -3.04 and float(g.max()) <= 20.73


# ------------------------------------------------------------------------------------------
# 4. vy_bce_head_*
# ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("M,d", [(1, 64), (51, 768), (300, 1024)])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_bce_head_kernels(M, d, dtype):
    from vyomai_amd import ops
    atol, rtol = elementwise_bars(dtype)
    sum_atol, sum_rtol = (2e-3 * math.sqrt(M), 1e-3) if dtype == BF else (2e-6 * math.sqrt(M) * 4, 1e-5)
    w = (rnd(d, seed=3) / math.sqrt(d)).to(dtype)
    b = torch.tensor([0.25]).to(dtype)
    h = rnd(M, d, seed=4)
    g = torch.Generator().manual_seed(M + d)
    y = (torch.rand(M, generator=g) < 0.4).float()
    live = torch.rand(M, generator=g) < 0.7
    live[0] = True
    if M >= 8:
        unit = w.float() / w.float().pow(2).sum()
        h[3], h[4] = 30.0 * unit, -30.0 * unit       # z = +-30 (+ b): saturated sigmoid, log1p(exp(-30)) ~ 1e-13
        y[3], y[4], live[3], live[4], live[1] = 0.0, 1.0, True, True, False
    h = h.to(dtype)
    hd, wd, bd, yd = h.double(), w.double(), b.double(), y.double()
    z64 = hd @ wd + bd
    loss64 = (z64.clamp_min(0) - z64 * yd + torch.log1p(torch.exp(-z64.abs())))[live].sum()
    # gscale = 0.75 * count: dz = 0.75 (sigmoid(z) - y) is O(1) per row, as the dy of a vy_linear_wgrad case is, so the
    # wgrad bar on the sums over rows binds (with gscale = 0.75 alone |dw| is below the bf16 bar at M = 300)
    count = max(int(live.sum()), 1)
    gscale = 0.75 * count
    dz64 = torch.where(live, (torch.sigmoid(z64) - yd) * gscale / count, torch.zeros((), dtype=torch.float64))
    dh64, dw64, db64 = dz64[:, None] * wd[None, :], dz64 @ hd, dz64.sum().reshape(1)

    hg, wg, bg, yg, lg = h.to(DEV), w.to(DEV), b.to(DEV), y.to(DEV), live.to(DEV).to(torch.uint8)
    z_only = ops.bce_head_fwd(hg, wg, bg)
    acc = torch.zeros(1, device=DEV)
    z = ops.bce_head_fwd(hg, wg, bg, yg, lg, acc)
    assert z.dtype == torch.float32 and z.shape == (M,) and torch.equal(z, z_only)
    check(z, z64, atol, rtol, "z")
    print(f"M={M} d={d}: loss_sum {acc.item():.6f} fp64 {loss64.item():.6f}")
    check(acc, loss64.reshape(1), sum_atol, sum_rtol, "loss_sum")
    gs, cnt = torch.tensor([gscale], device=DEV), torch.tensor([float(live.sum())], device=DEV)
    dw = torch.full((d,), 7.0, device=DEV)
    db = torch.full((1,), 7.0, device=DEV)
    dh = ops.bce_head_bwd(hg, wg, z, yg, lg, gs, cnt, dw, db, accumulate=False)
    assert dh.dtype == dtype and dh.shape == (M, d)
    check(dh, dh64, atol, rtol, "dh")
    assert not dh[~live.to(DEV)].any(), "dead rows of dh are zero"
    print(f"M={M} d={d}: max|dw| {dw64.abs().max().item():.3f} max|db| {db64.abs().max().item():.3f} (absolute bar {sum_atol:.2e})")
    if M > 1:
        assert dw64.abs().max().item() > 10 * sum_atol, "the bar would pass dw == 0"
    check(dw, dw64, sum_atol, sum_rtol, "dw")
    check(db, db64, sum_atol, sum_rtol, "db")
    dh2 = ops.bce_head_bwd(hg, wg, z, yg, lg, gs, cnt, dw, db, accumulate=True)
    assert torch.equal(dh, dh2)
    check(dw, 2 * dw64, 2 * sum_atol, sum_rtol, "dw accumulate")
    check(db, 2 * db64, 2 * sum_atol, sum_rtol, "db accumulate")


# ------------------------------------------------------------------------------------------
# 5. vy_mlm_mask
# ------------------------------------------------------------------------------------------


def test_mlm_mask_kernel():
    from vyomai_amd import ops
    tok = E.StubTokenizer()
    special = torch.tensor(tok.all_special_ids, dtype=torch.long, device=DEV)
    ids = big_ids(4 * 128 * 5)[:, :103].reshape(4, 515).contiguous()       # n = 2060: not a multiple of the block size
    for fraction in (0.15, 0.5):
        out, labels, masked = ops.mlm_mask(ids.to(DEV), special, fraction, 4, E.VOCAB, -100, SEED, OFFSET)
        want = mlm_numpy(ids.numpy(), tok.all_special_ids, fraction, 4, E.VOCAB, -100, SEED, OFFSET)
        assert masked.dtype == torch.bool and out.shape == ids.shape
        for name, a, b in zip(("masked_ids", "labels", "masked"), (out, labels, masked), want):
            assert np.array_equal(a.cpu().numpy(), b), name
        mlm_invariants(ids, out.cpu(), labels.cpu(), masked.cpu(), tok)
    big = big_ids()
    out, labels, masked = ops.mlm_mask(big.to(DEV), special, 0.15, 4, E.VOCAB, -100, SEED, OFFSET + 1)
    mlm_invariants(big, out.cpu(), labels.cpu(), masked.cpu(), tok)
    mlm_proportions(big, out.cpu(), masked.cpu(), tok, 0.15)
    none = torch.empty(0, dtype=torch.long, device=DEV)
    out, labels, masked = ops.mlm_mask(big.to(DEV), none, 0.15, 4, E.VOCAB, -100, SEED, OFFSET + 1)
    assert masked.cpu()[:, 0].any(), "with no special ids <s> can be selected"
    assert np.array_equal(masked.cpu().numpy(), mlm_numpy(big.numpy(), [], 0.15, 4, E.VOCAB, -100, SEED, OFFSET + 1)[2])


# ------------------------------------------------------------------------------------------
# 6. the model against the reference's fixture
# ------------------------------------------------------------------------------------------


def build(tied, compute=None):
    import vyomai_amd as V
    m = V.ElectraModel(V.EncoderForMaskedLM(E.cfg(E.GEN_LAYERS), pos_embedding_type="rope"),
                       V.Discriminator(E.cfg(E.DISC_LAYERS)))
    E.load_weights_(m, tied)
    m = m.to(DEV).train()
    if compute is not None:          # fp32 master weights, bf16 kernels (what FlatTrainer sets)
        for mod in m.modules():
            if hasattr(mod, "compute_dtype"):
                mod.compute_dtype = compute
    return m


@pytest.fixture(scope="module")
def case(golden):
    g = golden("electra")
    ids, mask = (T(a).to(DEV) for a in E.batch())
    masked = tuple(T(g[f"draw.{k}"]).to(DEV) for k in ("masked_ids", "labels")) + (T(g["draw.masked"]).to(DEV).bool(),)
    return g, ids, mask, masked, T(g["draw.sampled"]).to(DEV)


def step(m, case):
    _, ids, mask, masked, sampled = case
    return m.electra_loss(ids, mask, E.StubTokenizer(), masked=masked, sampled=sampled)


@pytest.mark.parametrize("compute", [None, BF], ids=["fp32", "bf16"])
def test_model_vs_reference(case, compute):
    g, ids, mask, masked, sampled = case
    for tied in (False, True):
        t = "tied" if tied else "untied"
        m = build(tied, compute)
        losses = step(m, case)
        pairs = [(f"{t}.loss[{i}]", losses[i], g[f"{t}.loss"][i], g[f"gap.{t}.loss"][i]) for i in range(3)]
        if not tied:
            pairs.append(("mlm.loss", m.generator_model.mlm_loss(masked[0], mask, masked[1]), g["mlm.loss"], g["gap.mlm.loss"]))
        for name, got, ref, gap in pairs:
            bar = 2e-5 * max(1.0, abs(ref)) if compute is None else 3 * float(gap)
            print(f"{name}: {got.item():.7f} reference {float(ref):.7f} bar {bar:.2e}")
            assert abs(got.item() - float(ref)) <= bar, (name, got.item(), float(ref), bar)
        m.zero_grad()
        losses[0].backward()
        worst = 0.0
        for n, p in m.named_parameters():
            e = rel_err(T(E.sub_g(p.grad.detach().float().cpu().numpy())), g[f"{t}.d.{n}"])
            bar = 1e-4 if compute is None else max(3 * float(g[f"gap.{t}.d.{n}"]), PARAM_FLOOR)
            worst = max(worst, e / bar)
            assert e < bar, (t, n, e, bar)
        print(f"{t}: largest gradient rel_err / bar = {worst:.3f}")


def test_discriminator_forward_and_notebook_loss(case):
    """Discriminator.forward (vy_bce_head_fwd without a target) and ElectraLoss's five-argument call on materialised
    logits give the fused step's losses, under no_grad and -- the notebook's own loop -- under autograd, where the
    backward gives the fixture's gradients."""
    import vyomai_amd as V
    from vyomai_amd.pretraining import electra
    g, ids, mask, masked, sampled = case
    m = build(False)
    tok = E.StubTokenizer()
    with torch.no_grad():
        out = m.get_generator_output(masked[0], mask)
        disc_in, disc_labels, live = electra(out.logits, ids, tok, masked[2], sampled=sampled)
        assert np.array_equal(disc_in.cpu().numpy(), g["draw.disc_input"])
        assert np.array_equal(disc_labels.cpu().numpy(), g["draw.disc_labels"])
        z = m.get_discriminator_output(disc_in, mask)
        assert z.shape == (E.B, E.L, 1)
        got = V.ElectraLoss(E.cfg(1))(out.logits, masked[1], z, disc_labels, live)
    for i in range(3):
        ref = float(g["untied.loss"][i])
        assert abs(got[i].item() - ref) <= 2e-5 * max(1.0, abs(ref)), (i, got[i].item(), ref)
    out = m.get_generator_output(masked[0], mask)
    z = m.get_discriminator_output(disc_in, mask)
    assert z.requires_grad
    loss = V.ElectraLoss(E.cfg(1))(out.logits, masked[1], z, disc_labels, live)
    for i in range(3):
        ref = float(g["untied.loss"][i])
        assert abs(loss[i].item() - ref) <= 2e-5 * max(1.0, abs(ref)), (i, loss[i].item(), ref)
    m.zero_grad()
    loss[0].backward()
    for n, p in m.named_parameters():
        e = rel_err(T(E.sub_g(p.grad.detach().float().cpu().numpy())), g[f"untied.d.{n}"])
        assert e < 1e-4, (n, e)


# ------------------------------------------------------------------------------------------
# 7. FlatTrainer with the shared table
# ------------------------------------------------------------------------------------------


def test_trainer_follows_reference_training(case):
    from vyomai_amd.training import FlatTrainer
    g = case[0]
    m = build(True)
    tr = FlatTrainer(m, lr=E.LR, weight_decay=E.WEIGHT_DECAY, compute_dtype=torch.float32)
    for s in range(E.TRAIN_STEPS):
        loss = tr.train_step(lambda: step(m, case)[0])
        ref = float(g["tied.train.loss"][s])
        print(f"step {s}: HIP fp32 loss {loss.item():.7f}  reference loss {ref:.7f}")
        assert abs(loss.item() - ref) < 2e-5 * max(1.0, abs(ref)), (s, loss.item(), ref)
    for n, p in m.named_parameters():
        w, wr = E.sub_g(p.detach().float().cpu().numpy()), g[f"tied.train.w.{n}"]
        assert np.abs(w - wr).mean() < 2e-6, (n, np.abs(w - wr).mean())
        assert np.abs(w - wr).max() < 2 * E.TRAIN_STEPS * E.LR + 1e-5, (n, np.abs(w - wr).max())


def test_trainer_shared_table_reports_after_both_scatters(case):
    from vyomai_amd import autograd_train as AT
    from vyomai_amd.training import FlatTrainer
    g, ids, mask, masked, sampled = case
    m = build(True)
    # small buckets: the table gets one of its own, so launch_order shows when it went out
    tr = FlatTrainer(m, lr=E.LR, weight_decay=E.WEIGHT_DECAY, compute_dtype=torch.float32, overlap_optimizer=False,
                     bucket_bytes=64 << 10)
    table = m.generator_model.encoder.word_embeddings.weight
    assert m.discriminator_model.discriminator.word_embeddings.weight is table
    bucket = tr.reducer.bucket_of[id(table)]
    events = []
    real_bwd, real_launch = AT.ops.embedding_bwd_, tr.reducer._launch

    def spy_bwd(dout, ids_, dw, padding_idx):
        events.append("scatter")
        return real_bwd(dout, ids_, dw, padding_idx)

    def spy_launch(b, notify=True):
        if b == bucket:
            events.append("bucket")
        return real_launch(b, notify)
    AT.ops.embedding_bwd_, tr.reducer._launch = spy_bwd, spy_launch
    try:
        tr.zero_grad()
        tr.backward(step(m, case)[0])
    finally:
        AT.ops.embedding_bwd_ = real_bwd
        del tr.reducer._launch
    assert events == ["scatter", "scatter", "bucket"], events
    assert bucket in tr.reducer.launch_order and tr.reducer.touched == {id(p) for p in tr.arena.params}
    both = table.grad.detach().clone()
    rel = rel_err(T(E.sub_g(both.cpu().numpy())), g["tied.d.discriminator_model.discriminator.word_embeddings.weight"])
    assert rel < 1e-4, rel
    parts = []
    for pick in (1, 2):                       # generator-only, discriminator-only backward
        tr.zero_grad()
        tr.backward(step(m, case)[pick])
        # one of the table's two recorded uses never scatters: it still reports, when the backward pass ends
        assert id(table) in tr.reducer.touched and bucket in tr.reducer.launch_order, pick
        parts.append(table.grad.detach().clone())
    assert float(parts[0].abs().max()) > 0 and float(parts[1].abs().max()) > 0
    e = float((both - (parts[0] + parts[1])).abs().max() / both.abs().max())
    print(f"table gradient vs generator-only + discriminator-only: rel_err {e:.3e}")
    assert e < 1e-4, e


# ------------------------------------------------------------------------------------------
# 8. undirected run
# ------------------------------------------------------------------------------------------


def test_undirected_step(case):
    from vyomai_amd import rng
    _, ids, mask, _, _ = case
    tok = E.StubTokenizer()
    big = big_ids(64 * 128)[:, :64].contiguous()                   # 64 rows of 64 tokens (the position table's length)
    big[:, 47], big[:, 48:] = 2, 1                                 # 46 ordinary tokens per row: the expected share of
    big = big.to(DEV)                                              # selected tokens is 0.15 * 46 / 64 = 0.108
    big_mask = (big != tok.pad_token_id).long()
    m = build(True, BF)
    runs = []
    for _ in range(2):
        rng.manual_seed(11)
        seen = {}
        real = m.discriminator_model.loss
        m.discriminator_model.loss = lambda x, am, y, live: (seen.update(disc_in=x, labels=y), real(x, am, y, live))[1]
        try:
            losses = m.electra_loss(big, big_mask, tok, fraction=0.15, temperature=3)
        finally:
            del m.discriminator_model.loss
        assert all(torch.isfinite(x).all() for x in losses)
        runs.append((seen["disc_in"].clone(), seen["labels"].clone(), [x.item() for x in losses]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "same seed, different draw"
    share = runs[0][1].mean().item()
    print(f"losses {runs[0][2]}  disc_labels.mean() {share:.4f} (selected: about {0.15 * 46 / 64:.4f})")
    assert 0.0 < share <= 0.15
    rng.manual_seed(12)
    other = m.electra_loss(big, big_mask, tok)
    assert other[0].item() != runs[0][2][0]
    # no host synchronisation inside the step: it can be captured (a .item() / .cpu() / tolist() would abort the capture)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        m.electra_loss(big, big_mask, tok)                # warm-up on the capture stream (workspaces, caches)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            captured = m.electra_loss(big, big_mask, tok)
    torch.cuda.current_stream().wait_stream(stream)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in captured)
