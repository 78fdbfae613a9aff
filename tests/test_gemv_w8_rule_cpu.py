"""tests/gemv_w8_rule.py on the CPU: the fp32 emulation of dec_gemv1_w8_kernel passes every rule on every case of the GPU
test's list, every planted mutation of the arithmetic, the scale or the code layout fails at least one case, and the
quantiser's restatement agrees with torch's float8_e4m3fn cast code for code and keeps its error bound."""
import pytest
import torch

from tests import gemv_w8_rule as W

CASES = W.cases()

# the cases a mutation is tried on (kind, substring of the id): the small ones where it can show
MUTANTS = {
    "up_gate_scale": ("gated", "K2048-N4-exact"),
    "scale_after_round": ("plain", "K2048-N4-exact-bias1res1"),
    "scale_block_index": ("qkv", "h2x2x64-rope1-pos37"),
    "drop_second_half": ("plain", "K2048-N4-exact"),
    "swap_byte_pairs": ("plain", "K2048-N4-exact"),
    "fnuz_bias": ("plain", "K2048-N256-onehot"),
    "skip_last_chunk": ("plain", "K2048-N4-exact"),
}


def _pick(kind, frag):
    got = [c for c in CASES if c["kind"] == kind and frag in c["id"]]
    assert got, (kind, frag)
    return got


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_emulation_passes_every_rule(case):
    inp = W.make_inputs(case)
    W.check(case, inp, W.emulate(case, inp))


def test_case_list_covers_every_instantiation_and_data_kind():
    ids = " ".join(c["id"] for c in CASES)
    for K in W.LEAN_K:
        for epi, norms in (("GV_PLAIN", ("false",)), ("GV_GATED", ("false", "true")), ("GV_QKV", ("false", "true"))):
            for norm in norms:
                assert f"dec_gemv1_w8_kernel<{epi},{W.W8_INST[K]},{norm}>" in ids
        for kind in ("exact", "codes"):
            assert any(c["K"] == K and c["data"] == kind for c in CASES)
    assert {c["data"] for c in CASES} == {"exact", "eps", "codes", "onehot", "gauss"}


@pytest.mark.parametrize("mut", W.MUTATIONS)
def test_every_planted_mutation_is_caught(mut):
    assert set(MUTANTS) == set(W.MUTATIONS)
    caught = []
    for case in _pick(*MUTANTS[mut]):
        inp = W.make_inputs(case)
        try:
            W.check(case, inp, W.emulate(case, inp, mut))
        except AssertionError:
            caught.append(case["id"])
    assert caught, f"{mut}: the rules passed the mutated kernel on every case tried"


def test_encoder_agrees_with_the_torch_cast_code_for_code():
    """Every fp32 value that matters: the 256 codes' own values, the midpoints between neighbours (ties go to the even
    code), one fp32 step either side of each midpoint, 464 (saturates to 126 under the clamp), and random values."""
    codes = torch.arange(256, dtype=torch.uint8)
    vals = W.decode_e4m3(codes)
    ok = ~vals.isnan()
    assert torch.equal(W.encode_e4m3(vals[ok]), codes[ok])
    pos = vals[:127]                                           # 0 .. 448, ascending
    mid = (pos[:-1] + pos[1:]) / 2
    g = torch.Generator().manual_seed(5)
    probe = torch.cat([mid, torch.nextafter(mid, mid + 1), torch.nextafter(mid, mid - 1), torch.tensor([464.0, 2.0 ** -11, 3e-4]),
                       (torch.rand(4096, generator=g) * 2 - 1) * 448, torch.randn(4096, generator=g) * 0.01])
    probe = torch.cat([probe, -probe]).clamp(-448.0, 448.0)
    assert torch.equal(W.encode_e4m3(probe), probe.to(W.F8).view(torch.uint8))
    assert int(W.encode_e4m3(torch.tensor([464.0]).clamp(-448.0, 448.0))) == 126


@pytest.mark.parametrize("N,K", [(5, 2048), (36, 4096)])
def test_quantiser_rule_and_error_bound(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * torch.logspace(-3, 2, N)[:, None]).to(W.BF).float()
    w[1] = 0.0                                                 # an all-zero row: scale 1, codes 0
    w[2] = W.decode_e4m3(torch.randint(0, 127, (K,), generator=g).to(torch.uint8)) * 0.125   # code values times 2^-3 ...
    w[2, 0] = -56.0                                            # ... with amax = 448 * 2^-3: lossless
    codes, s = W.quant_rows(w)
    assert float(s[1]) == 1.0 and int(codes[1].max()) == 0
    assert float(s[2]) == 0.125 and torch.equal(W.decode_e4m3(codes[2]) * s[2], w[2])     # lossless
    assert torch.equal(s, torch.where(w.abs().amax(1) > 0, w.abs().amax(1) / 448.0, torch.ones(N)))
    assert torch.equal(codes, (w / s[:, None]).clamp(-448, 448).to(W.F8).view(torch.uint8))
    assert bool(W.quant_error_ok(w, codes, s).all())
    # the bound is a bound of THIS rule: one code off breaks it somewhere
    worse = codes.clone()
    worse[0] = worse[0] + 1
    assert not bool(W.quant_error_ok(w, worse, s).all())
    # a Gaussian row product at K = 2048: the relative RMS error that quantisation alone costs (a figure for DESIGN)
    x = torch.randn(K, generator=g).double()
    row = torch.randn(64, K, generator=g).to(W.BF).float()
    c2, s2 = W.quant_rows(row)
    deq = W.decode_e4m3(c2).double() * s2.double()[:, None]
    rel = ((deq - row.double()) @ x).pow(2).mean().sqrt() / (row.double() @ x).pow(2).mean().sqrt()
    print(f"quantisation alone, Gaussian rows, K = {K}: relative RMS error of a row product {float(rel):.4f}")
    assert 0.01 < float(rel) < 0.05
