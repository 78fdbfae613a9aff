"""vy_spec_verify on the MI355X against the fp64 restatement of tests/spec_rule.py: decisions and residual tokens with
the margins stated there, the row after the last draft bit for bit against vy_sample_rows, and the property the algorithm
exists for -- the emitted token is distributed as the target's own softmax, whatever the drafter proposes.

Inputs are built on the host and the restatement is held to its own conditions before the kernel runs: no drafted row
of the cases lies inside the decision band (nor within 16 times its width), and the score interval admits exactly one
token in at least 95 % of the rejected rows."""
import math

import numpy as np
import pytest
import torch

from tests import spec_rule as SR
from tests.test_serving_sampling_gpu import i64, inv_t_of, kept_numpy, restated_draws

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SEED = 0x1234567887654321
MASK64 = (1 << 64) - 1

GAMMA, S = 4, 8
N_DRAFT = [4, 4, 4, 4, 1, 4, 4, 0]
#          greedy accept-all, greedy rejecting at row 2, temperature, top_k, top_p, both (+ a token outside Kp),
#          identical rows, no draft at all
PARAMS = [(0, 0, 0.0), (0, 0, 0.0), (0.8, 0, 0.0), (1.0, 12, 0.0), (1.2, 0, 0.9), (0.7, 20, 0.8), (1.0, 30, 0.0),
          (0.9, 0, 0.95)]
POS0 = [5, 17, 3, (1 << 32) + 9, 40, 8, 100, 1]
OUTSIDE = (5, 1)            # (sequence, row) whose draft token lies outside the target's kept set
IDENTICAL = 6


def seed_of(s):
    return (SEED + s * 0x9E3779B97F4A7C15) & MASK64


def build_case(V, dtype):
    """-> dict of host tensors: target (rows, ld) and draft (GAMMA, S, ld) with NaN in every pad column and in every row
    that must not be read, tokens (GAMMA, S), t_row0, and the logits as stored, in fp64, per (s, i)."""
    from vyomai_amd.autograd_train import _row_stride
    g = torch.Generator().manual_seed(77 + V)
    ld = _row_stride(V)
    t_row0 = np.concatenate([[0], np.cumsum([n + 1 for n in N_DRAFT])[:-1]]).astype(int).tolist()
    target = torch.full((sum(N_DRAFT) + S, ld), float("nan"), dtype=dtype)
    draft = torch.full((GAMMA, S, ld), float("nan"), dtype=dtype)
    tokens = torch.zeros((GAMMA, S), dtype=torch.long)
    T, D = {}, {}
    for s, n in enumerate(N_DRAFT):
        t = (2.0 * torch.randn(n + 1, V, generator=g)).to(dtype)
        d = t[:n] if s == IDENTICAL else (t[:n].float() + torch.randn(n, V, generator=g)).to(dtype)
        target[t_row0[s]:t_row0[s] + n + 1, :V] = t
        draft[:n, s, :V] = d
        temperature, k, p = PARAMS[s]
        for i in range(n + 1):
            T[s, i] = t[i].double().numpy()
        for i in range(n):
            D[s, i] = d[i].double().numpy()
            if temperature == 0:
                order = np.argsort(-T[s, i], kind="stable")
                tokens[i, s] = int(order[1] if (s, i) == (1, 2) else order[0])
            elif (s, i) == OUTSIDE:
                tokens[i, s] = int(np.argmin(T[s, i]))
            else:       # the drafter's own draw: noise row 0 at the token's position
                x = d[i].float().numpy()
                tokens[i, s] = int(restated_draws(x, inv_t_of(temperature), kept_numpy(D[s, i], k, p), seed_of(s),
                                                  [POS0[s] + i])[0])
    return dict(V=V, target=target, draft=draft, tokens=tokens, t_row0=t_row0, T=T, D=D)


def restate_case(case):
    out = {}
    for s, n in enumerate(N_DRAFT):
        temperature, k, p = PARAMS[s]
        for i in range(n):
            out[s, i] = SR.restate(case["T"][s, i], case["D"][s, i], int(case["tokens"][i, s]), inv_t_of(temperature), k, p,
                                   seed_of(s), POS0[s] + i)
    return out


def conditions(rest):
    """What the inputs must satisfy for the test to say something; -> (rejected sampled rows, of them unique)."""
    for key, r in rest.items():
        assert not r["band"], (key, "a row of the case lies inside the decision band")
        if "gap" in r and not r["must_reject"]:
            assert abs(r["gap"]) > 16 * SR.E * max(r["px"], r["qx"]), (key, "a row of the case lies next to the band")
    rejected = [r for r in rest.values() if r["greedy_alt"] is None and not r["accept"]]
    unique = sum(r["unique"] for r in rejected)
    assert rejected and unique >= 0.95 * len(rejected), (unique, len(rejected))
    return len(rejected), unique


def per_seq(dev):
    return dict(t_row0=None,
                n_draft=torch.tensor(N_DRAFT, dtype=torch.int32, device=dev),
                inv_temperature=torch.tensor([inv_t_of(p[0]) for p in PARAMS], dtype=torch.float32, device=dev),
                top_k=torch.tensor([p[1] for p in PARAMS], dtype=torch.int32, device=dev),
                top_p=torch.tensor([p[2] for p in PARAMS], dtype=torch.float32, device=dev),
                seed=torch.tensor([i64(seed_of(s)) for s in range(S)], dtype=torch.long, device=dev),
                position0=torch.tensor(POS0, dtype=torch.long, device=dev))


def launch(target, draft, tokens, a):
    from vyomai_amd import ops
    accept, alt = ops.spec_verify(target, draft, tokens, a["t_row0"], a["n_draft"], a["inv_temperature"], a["top_k"],
                                  a["top_p"], a["seed"], a["position0"])
    assert accept.dtype == torch.int32 and alt.dtype == torch.long and accept.shape == alt.shape == (S, GAMMA + 1)
    return accept.cpu(), alt.cpu()


@pytest.mark.parametrize("V,dtype", [(517, torch.float32), (517, BF), (4099, torch.float32), (4099, BF)],
                         ids=lambda v: {torch.float32: "fp32", BF: "bf16"}.get(v, str(v)))
def test_spec_verify_vs_restatement(V, dtype):
    from vyomai_amd import ops
    case = build_case(V, dtype)
    rest = restate_case(case)
    n_rej, n_unique = conditions(rest)
    print(f"V={V} {dtype}: {len(rest)} drafted rows, {n_rej} sampled rows rejected, the interval admits one token in {n_unique}")
    assert rest[OUTSIDE]["must_reject"]
    assert all(rest[0, i]["accept"] for i in range(4)) and [rest[1, i]["accept"] for i in range(4)] == [True, True, False, True]
    assert all(rest[IDENTICAL, i]["accept"] for i in range(4)), "identical rows accept: u < 1"
    sampled = [r["accept"] for (s, i), r in rest.items() if r["greedy_alt"] is None and s != IDENTICAL]
    assert any(sampled) and not all(sampled), "the sampled rows hold both decisions"

    tbuf, dbuf, tokens = case["target"].to(DEV), case["draft"].to(DEV), case["tokens"].to(DEV)
    target, draft = tbuf[:, :V], dbuf[:, :, :V]
    a = per_seq(DEV)
    a["t_row0"] = torch.tensor(case["t_row0"], dtype=torch.int32, device=DEV)
    before = (tbuf.clone(), dbuf.clone())
    accept, alt = launch(target, draft, tokens, a)
    assert torch.equal(tbuf.view(torch.uint8), before[0].view(torch.uint8)), "the logits are only read"
    assert torch.equal(dbuf.view(torch.uint8), before[1].view(torch.uint8))
    for (s, i), r in rest.items():
        SR.check(r, int(accept[s, i]), int(alt[s, i]), f"V={V} sequence {s} row {i} {PARAMS[s]}")
    assert accept[0, :4].tolist() == [1, 1, 1, 1] and accept[1, :4].tolist() == [1, 1, 0, 1]
    assert accept[IDENTICAL, :4].tolist() == [1, 1, 1, 1] and int(accept[OUTSIDE]) == 0
    # the row after the last draft is vy_sample_rows' draw, bit for bit, also without any draft
    last = torch.tensor([case["t_row0"][s] + N_DRAFT[s] for s in range(S)], device=DEV)
    want = ops.sample_rows(target[last], a["inv_temperature"], a["top_k"], a["top_p"], a["seed"],
                           a["position0"] + a["n_draft"].long()).cpu()
    for s, n in enumerate(N_DRAFT):
        assert int(alt[s, n]) == int(want[s]) and int(accept[s, n]) == 0, (s, int(alt[s, n]), int(want[s]))
        assert accept[s, n + 1:].tolist() == [0] * (GAMMA - n) and alt[s, n + 1:].tolist() == [-1] * (GAMMA - n)
    again = launch(target, draft, tokens, a)
    assert torch.equal(again[0], accept) and torch.equal(again[1], alt), "two launches differ"
    # rows that start off a 16-byte boundary: every base unaligned, the same answers
    twide = torch.full((tbuf.shape[0], tbuf.shape[1] + 3), float("nan"), dtype=dtype, device=DEV)
    dwide = torch.full((GAMMA, S, dbuf.shape[2] + 3), float("nan"), dtype=dtype, device=DEV)
    twide[:, 1:V + 1], dwide[:, :, 1:V + 1] = target, draft
    moved = launch(twide[:, 1:V + 1], dwide[:, :, 1:V + 1], tokens, a)
    assert torch.equal(moved[0], accept) and torch.equal(moved[1], alt), "an unaligned row base changes the answer"
    # a sequence whose rows would leave the target buffer is not read
    a2 = dict(a, t_row0=a["t_row0"].clone())
    a2["t_row0"][2] = target.shape[0] - 2
    out = launch(target, draft, tokens, a2)
    assert out[0][2].tolist() == [0] * (GAMMA + 1) and out[1][2].tolist() == [-1] * (GAMMA + 1)
    keep = [s for s in range(S) if s != 2]
    assert torch.equal(out[0][keep], accept[keep]) and torch.equal(out[1][keep], alt[keep])


# ------------------------------------------------------------------------------------------
# distribution
# ------------------------------------------------------------------------------------------

DRAWS, DV = 20000, 257
DIST = {"temperature": (0.9, 0, 0.0), "top_k_top_p": (1.1, 40, 0.9)}


def chi_square(tokens, prob, kept, draws):
    """Pearson's statistic with test_sampling_distribution's binning (expectations below 5 merged into one bin) and its
    0.999 quantile (Wilson-Hilferty) -> (statistic, degrees of freedom, bound)."""
    expect = draws * prob
    counts = np.bincount(tokens, minlength=prob.size).astype(np.float64)
    big = expect >= 5.0
    obs, exp = list(counts[big]), list(expect[big])
    if (kept & ~big).any():
        obs.append(counts[kept & ~big].sum())
        exp.append(expect[kept & ~big].sum())
    obs, exp = np.array(obs), np.array(exp)
    df = obs.size - 1
    bound = df * (1 - 2 / (9 * df) + 3.0902 * math.sqrt(2 / (9 * df))) ** 3
    return float(((obs - exp) ** 2 / exp).sum()), df, bound


def dist_rows():
    rng = np.random.default_rng(4242)
    return (2 * rng.standard_normal(DV)).astype(np.float32), (2 * rng.standard_normal(DV)).astype(np.float32)


def restated_emission(t, d, temperature, k, p, seed, positions):
    """The whole round restated for gamma = 1: draft from q (noise row 0), accept on u (row 1), residual (row 2)."""
    inv_t = inv_t_of(temperature)
    P, Kp = SR.probs(t.astype(np.float64), inv_t, k, p)
    Q, Kq = SR.probs(d.astype(np.float64), inv_t, k, p)
    x = restated_draws(d, inv_t, Kq, seed, positions)
    u = SR.noise_rows(seed, positions, 1, 1)[:, 0]
    accept = Kp[x] & ~(u * Q[x] > P[x])
    with np.errstate(divide="ignore"):
        res = np.where(P > Q, np.log(np.where(P > Q, P - Q, 1.0)), -np.inf)
    alt = (res[None, :] + SR.gumbel64(SR.noise_rows(seed, positions, DV, 2))).argmax(axis=1)
    return np.where(accept, x, alt), accept, P, Q, Kp


@pytest.mark.parametrize("case", list(DIST))
def test_emitted_token_follows_the_target(case):
    from vyomai_amd import ops
    temperature, k, p = DIST[case]
    t, d = dist_rows()
    positions = np.arange(1, DRAWS + 1)
    want, want_acc, P, Q, Kp = restated_emission(t, d, temperature, k, p, SEED, positions)
    rate = float(np.minimum(P, Q).sum())
    sd = math.sqrt(DRAWS * rate * (1 - rate))
    stat, df, bound = chi_square(want, P, Kp, DRAWS)
    print(f"{case}: restatement chi-square {stat:.2f}, df {df}, bound {bound:.2f}; accepted {int(want_acc.sum())}, "
          f"expected {DRAWS * rate:.1f} +- {sd:.1f}")
    assert stat <= bound and abs(want_acc.sum() - DRAWS * rate) <= 4 * sd, "the restatement itself misses"

    trow = torch.from_numpy(t).to(DEV)
    drow = torch.from_numpy(d).to(DEV)
    f = lambda v, dt: torch.full((DRAWS,), v, dtype=dt, device=DEV)
    inv_t, kk, pp = f(inv_t_of(temperature), torch.float32), f(k, torch.int32), f(p, torch.float32)
    seed, pos = f(i64(SEED), torch.long), torch.from_numpy(positions).to(DEV)
    dlog = drow[None, None].expand(1, DRAWS, DV).contiguous()
    x = ops.sample_rows(dlog[0], inv_t, kk, pp, seed, pos)
    target = trow[None].expand(2, DV).contiguous()              # every "sequence" owns the same two rows
    accept, alt = ops.spec_verify(target, dlog, x[None].contiguous(), f(0, torch.int32), f(1, torch.int32), inv_t, kk, pp,
                                  seed, pos)
    x, accept, alt = x.cpu().numpy(), accept.cpu().numpy(), alt.cpu().numpy()
    got = np.where(accept[:, 0] == 1, x, alt[:, 0])
    assert Kp[got].all(), "a token outside the target's kept set was emitted"
    assert (alt[accept[:, 0] == 1, 0] == -1).all()
    stat, df, bound = chi_square(got, P, Kp, DRAWS)
    n_acc = int(accept[:, 0].sum())
    print(f"{case}: kernel chi-square {stat:.2f}, df {df}, bound {bound:.2f}; accepted {n_acc}; "
          f"{int((got == want).sum())}/{DRAWS} emissions equal the restatement's")
    assert stat <= bound
    assert abs(n_acc - DRAWS * rate) <= 4 * sd
