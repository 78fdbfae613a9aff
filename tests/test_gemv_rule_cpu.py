"""tests/gemv_rule.py on the CPU: the fp32 emulation of dec_gemv1_kernel / gemv_bf16_kernel passes every rule on every
case of the GPU test's list (the inputs and the budgets are usable before a GPU sees them), and every planted mutation
of the arithmetic or the addressing fails at least one case (the rules can see what they are there to see)."""
import pytest
import torch

from tests import gemv_rule as R

CASES = R.cases()

# the cases a mutation is tried on (ids by substring): the small ones where it can show
MUTANTS = {
    "swap_gate_up": ("gated", "K2048-N516-int"),
    "up_at_n": ("gated", "K2048-N516-int"),
    "partner_xor1": ("qkv", "h2x2x64-rope1-pos37"),
    "upper_sign": ("qkv", "h2x2x64-rope1-pos37"),
    "ignore_c_sh": ("qkv", "h2x2x64"),
    "mean_half": ("plain", "gemv_bf16_kernel<0,NONE,4,true,false>-M1-K264"),
    "no_eps": (None, "eps"),
    "skip_last_chunk": ("plain", "K2048-N4-int"),
    "bias_block_index": ("qkv", "h2x2x64-rope1"),
    "no_proj_round": ("qkv", "true>-M1-K2048-N384-int-h2x2x64-rope1-pos37"),
    "no_gate_round": ("gated", "true>-M1-K2048-N516-int"),
}


def _pick(kind, frag):
    got = [c for c in CASES if (kind is None or c["kind"] == kind) and frag in c["id"]]
    assert got, (kind, frag)
    return got


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_emulation_passes_every_rule(case):
    inp = R.make_inputs(case)
    R.check(case, inp, R.emulate(case, inp))


def test_case_list_covers_every_instantiation():
    ids = " ".join(c["id"] for c in CASES)
    for K in R.LEAN_K:
        for epi, norms in (("GV_PLAIN", ("false",)), ("GV_GATED", ("false", "true")), ("GV_QKV", ("false", "true"))):
            for norm in norms:
                assert f"dec_gemv1_kernel<{epi},{R.LEAN_INST[K]},{norm}>" in ids
    for inst in ("0,NONE,4,false,false", "0,NONE,4,true,false", "0,GELU_TANH,4,false,true", "0,GELU_TANH,4,true,true",
                 "1,NONE,4,false,false", "1,NONE,4,true,false"):
        assert f"gemv_bf16_kernel<{inst}>" in ids


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_planted_mutation_is_caught(mut):
    assert set(MUTANTS) == set(R.MUTATIONS)
    caught = []
    for case in _pick(*MUTANTS[mut]):
        inp = R.make_inputs(case)
        try:
            R.check(case, inp, R.emulate(case, inp, mut))
        except AssertionError:
            caught.append(case["id"])
    assert caught, f"{mut}: the rules passed the mutated kernel on every case tried"


def test_the_rules_themselves():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    assert torch.equal(R.ulp_bf16(t(1.0, 1.99, 2.0, 0.75, -3.0)), t(2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6))
    # half an ulp passes, a whole ulp does not; a result one binade up is judged by its own spacing
    ok, _ = R.round_rule(t(1.0, 1.0078125, 2.0), t(1.00390625, 1.0, 1.9921875), t(0.0, 0.0, 0.0))
    assert ok.tolist() == [True, False, True]
    # rotary: 3 * 0.5 - 2 * 0.25 in the lower half, 2 * 0.5 + 3 * 0.25 in the upper
    c, s = t(0.5), t(0.25)
    assert bool(R.rope_rule(t(1.0), t(3.0), t(0.0), t(2.0), t(0.0), c, s, -1.0)[0])
    assert bool(R.rope_rule(t(1.75), t(2.0), t(0.0), t(3.0), t(0.0), c, s, 1.0)[0])
    assert not bool(R.rope_rule(t(2.0), t(3.0), t(0.0), t(2.0), t(0.0), c, s, -1.0)[0])
