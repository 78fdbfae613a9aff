"""The accept / reject / resample rule of vy_spec_verify restated in fp64 numpy (include/vyom_hip.h), shared by
test_spec_verify_gpu.py and test_speculative_engine_gpu.py.  Built from the pinned pieces of the sampling tests: the
Philox restatement and Gumbel transform of test_electra_gpu.py, the kept set of test_serving_sampling_gpu.py.

Margins.  p and q are softmaxes the kernel forms in fp32; a decision is only judged where |u q(x) - p(x)| exceeds
2^-20 max(p(x), q(x)) (inside that band either answer passes), and a residual token passes if its score interval reaches
the maximum when p and q are each perturbed by a relative 2^-20: upper score log(p (1 + e) - q (1 - e)) + noise against
the lower scores log(p (1 - e) - q (1 + e)) + noise of the others."""
import numpy as np

from tests.test_electra_gpu import gumbel64, philox7
from tests.test_serving_sampling_gpu import kept_numpy

E = 2.0 ** -20
M32 = np.uint64(0xFFFFFFFF)


def noise_rows(seed, offsets, V, row):
    """Uniforms (len(offsets), V) of noise row `row` for (seed, offset): word v & 3 of Philox on {v / 4, row, offset}."""
    off = np.asarray(offsets, dtype=np.uint64).reshape(-1, 1)
    q = np.arange((V + 3) // 4, dtype=np.uint64)[None, :]
    r = philox7(q, row, off & M32, off >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(r, axis=-1).reshape(off.shape[0], -1)[:, :V]
    return (words >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def probs(x, inv_t, k, p):
    """-> (softmax of x * inv_t over the kept set, the kept set) for one fp64 row."""
    kept = kept_numpy(x, k, p)
    e = np.exp(np.where(kept, (x - x.max()) * inv_t, -np.inf))
    return e / e.sum(), kept


def lowest_argmax(x):
    return int(np.flatnonzero(x == x.max())[0])


def restate(t, d, x, inv_t, k, p, seed, offset):
    """One drafted row: t / d the target / draft logits as stored (any float array), x the draft token.
    -> dict(accept, band, must_reject, admitted (V,) bool: the tokens alt may be on a rejection, unique, greedy_alt)."""
    t = np.asarray(t, dtype=np.float64)
    if inv_t == 0:
        a = lowest_argmax(t)
        admitted = np.zeros(t.size, dtype=bool)
        admitted[a] = True
        return dict(accept=a == x, band=False, must_reject=False, admitted=admitted, unique=True, greedy_alt=a)
    d = np.asarray(d, dtype=np.float64)
    V = t.size
    P, Kp = probs(t, inv_t, k, p)
    Q, _ = probs(d, inv_t, k, p)
    u = float(noise_rows(seed, [offset], 1, 1)[0, 0])
    must_reject = not (0 <= x < V and Kp[x])
    px, qx = (0.0, 0.0) if must_reject else (P[x], Q[x])
    gap = u * qx - px
    band = (not must_reject) and abs(gap) <= E * max(px, qx)
    g = gumbel64(noise_rows(seed, [offset], V, 2)[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        hi, lo = P * (1 + E) - Q * (1 - E), P * (1 - E) - Q * (1 + E)
        up = np.where(hi > 0, np.log(np.where(hi > 0, hi, 1.0)), -np.inf) + g
        low = np.where(lo > 0, np.log(np.where(lo > 0, lo, 1.0)), -np.inf) + g
    admitted = (up >= low.max()) if np.isfinite(low.max()) else Kp.copy()     # (no column surely has p > q: any of p's)
    return dict(accept=(not must_reject) and not gap > 0, band=band, must_reject=must_reject, admitted=admitted,
                unique=int(admitted.sum()) == 1, greedy_alt=None, u=u, px=px, qx=qx, gap=gap)


def check(r, accept, alt, what):
    """Holds the kernel's (accept, alt) of one drafted row to the restatement r."""
    accept = bool(accept)
    if r["must_reject"]:
        assert not accept, (what, "a draft token outside the target's kept set was accepted")
    elif not r["band"]:
        assert accept == r["accept"], (what, "decision", accept, {k: r.get(k) for k in ("u", "px", "qx", "gap")})
    if r["greedy_alt"] is not None:
        assert alt == r["greedy_alt"], (what, "greedy alt is the arg-max", alt, r["greedy_alt"])
    elif accept:
        assert alt == -1, (what, "an accepted row writes alt = -1", alt)
    else:
        assert 0 <= alt < r["admitted"].size and r["admitted"][alt], (what, "residual token", alt,
                                                                       np.flatnonzero(r["admitted"])[:8])
