"""tests/qkv_rope_rule.py held on the CPU: the case table against the restated launcher, the helper's sign and pairing
convention against the oracle, and the non-vacuity of every expectation test_qkv_rope_exact_gpu.py compares with -- each
planted mutation of the reference moves at least a third of the elements it touches."""
import functools

import pytest
import torch

from oracle import vyom_oracle as O
from tests import qkv_rope_rule as R

CASES = R.cases()
BF = torch.bfloat16


def test_every_case_declares_the_route_the_launcher_rule_gives():
    for c in CASES:
        assert R.route_of(c, True) == c["route"], (c["id"], R.route_of(c, True))
        assert c["K"] % (8 if c["dtype"] == BF else 4) == 0, c["id"]      # check_operands: 16-byte rows


def test_every_route_is_reached_with_and_without_rotation():
    on = {c["route"] for c in CASES}
    off = {R.route_of(c, False) for c in CASES}
    fused = {c["route"] for c in CASES if R.fused(c["dh"], True, c["dtype"])}
    assert on == set(R.ROUTES), set(R.ROUTES) ^ on
    assert off == set(R.ROUTES), set(R.ROUTES) ^ off
    assert fused == set(R.FUSED_ROUTES), set(R.FUSED_ROUTES) ^ fused
    # the rotation launch behind the GEMM: on the matrix-vector kernel, a mid-size tile, a large kernel and in fp32
    unfused = {c["route"] for c in CASES if R.rotation(c["dh"], True, c["dtype"]) == "rope_qk"}
    assert {"gemv", "mid128", "x3m16_192", "f32"} <= unfused


def test_route_thresholds():
    """The edges of launch_bf16 as test_linear_bf16_exact's LINEAR_EDGES list walks them, for EPI = 1."""
    r = lambda M, N, K, dh=64, rope=True, ws=True: R.route(M, N, K, dh, rope, ws)
    assert r(4, 768, 768) == "skinny16" and r(4, 768, 768, rope=False) == "gemv" and r(5, 768, 768, rope=False) == "skinny16"
    assert r(4, 512, 768, dh=128) == "gemv"
    assert r(32, 6400, 768) == "skinny32" and r(32, 6336, 768) == "skinny16"       # N / 32 < 200
    assert r(32, 8192, 48) == "skinny32" and r(32, 8256, 48) == "tile32x128"
    assert r(33, 768, 72) == "mid128" and r(128, 768, 72) == "mid128"
    assert r(129, 768, 72) == "all256" and r(256, 768, 72) == "all256"
    assert r(257, 768, 72) == "all320" and r(320, 768, 72) == "all320" and r(321, 768, 72) == "mid128"
    assert r(1024, 6144, 264) == "mid128" and r(1025, 6144, 264) == "m16_256"
    assert r(4096, 3071, 768) == "x3m16_192" and r(4096, 3072, 264) == "m16_256" and r(2048, 3072, 768) == "mid128"
    assert r(264, 2048, 2048) == "all320+splitk" and r(264, 2048, 2048, ws=False) == "all320"
    assert r(264, 32768, 2048) == "all320"                                          # 256 tiles: not split
    assert R.splitk_slices(10, 9, 448) == 3 and R.splitk_slices(10, 3, 448) == 1 and R.splitk_slices(80, 9, 448) == 3


@pytest.mark.parametrize("dh,L,pos0", [(64, 19, 7), (16, 5, 0), (72, 9, 3)])
def test_helper_with_real_tables_equals_the_oracle(dh, L, pos0):
    g = torch.Generator().manual_seed(dh + L)
    q = torch.randn(2, 3, L, dh, generator=g, dtype=torch.float64)
    k = torch.randn(2, 1, L, dh, generator=g, dtype=torch.float64)
    cos, sin = R.real_tables(pos0 + L, dh)
    fr = O.rotary_angles(dh, pos0 + L)[:, pos0:pos0 + L]
    wq, wk = O.apply_rotary(q, k, fr)
    pos = pos0 + torch.arange(L)
    for got, want in ((R.rotate(q, cos, sin, pos), wq), (R.rotate(k, cos, sin, pos), wk)):
        assert float((got - want).abs().max()) <= 1e-12
    # the inverse is the transposed rotation: on quarter turns it undoes the forward exactly
    cq, sq = R.quarter_tables(pos0 + L, dh)
    assert torch.equal(R.rotate(R.rotate(q, cq, sq, pos), cq, sq, pos, inverse=True), q)
    # and rule R's arithmetic is the oracle's in bf16
    wq16, _ = O.apply_rotary(q.to(BF), k.to(BF), fr)
    assert torch.equal(R.rotate(q.to(BF), cos, sin, pos, BF), wq16)


def test_real_tables_are_ops_rope_tables():
    from vyomai_amd import ops
    for dh in (16, 64, 72, 128):
        for a, b in zip(R.real_tables(77, dh), ops.rope_tables(dh, 77, "cpu")):
            assert torch.equal(a, b)


def _shape(c):
    return (c["B"], c["L"], c["K"], c["h"], c["hk"], c["dh"], c["pos0"])


SHAPES = {_shape(c): c for c in CASES}        # the store form, the dtype and the workspace do not change the expectation


@functools.lru_cache(maxsize=None)
def _full(shape, mut):
    c = SHAPES[shape]
    cos, sin = R.quarter_tables(R.table_rows(c), c["dh"])
    q, k, v = R.expect(c, cos, sin, "Q", mut)
    return {"q": q, "k": R.in_cache(k, c, mut), "v": R.in_cache(v, c, mut)}


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_every_mutation_moves_a_third_of_what_it_touches(shape):
    c = SHAPES[shape]
    true = _full(shape, None)
    applied = 0
    for mut in R.MUTATIONS:
        bands = R.band(c, mut)
        if bands is None:
            continue
        applied += 1
        other = _full(shape, mut)
        for name, mask in bands.items():
            moved = float((other[name] != true[name])[mask].double().mean())
            assert moved >= 1 / 3, f"{c['id']} {mut}: only {moved:.3f} of the {name} band differs"
        for name in set(true) - set(bands):
            assert torch.equal(other[name], true[name]), (c["id"], mut, name)
    assert applied >= 8


def test_band_mutations_apply_somewhere():
    for mut in R.MUTATIONS:
        hit = [c["id"] for c in SHAPES.values() if R.band(c, mut) is not None]
        assert len(hit) >= 3, (mut, hit)
    # the batch index behind a boundary inside a 256-row block, on both large kernels and on the all-rows tiles
    for route in ("x3m16_192", "m16_256", "all256", "all320", "all256+splitk"):
        assert any(c["route"] == route and R.band(c, "batch_stuck_in_block") is not None for c in CASES), route
    for route in ("x3m16_192", "m16_256", "mid128", "all320"):
        assert any(c["route"] == route and R.band(c, "table_row_mod_256") is not None for c in CASES), route


def test_rule_r_rotates():
    """Real angles: the bf16 expectation is away from the unrotated projection in most of q (position pos0 >= 5)."""
    for shape in ((2, 50, 136, 12, 4, 64, 5), (1, 40, 264, 2, 1, 128, 5)):
        c = SHAPES[shape]
        cos, sin = R.real_tables(R.table_rows(c), c["dh"])
        q, k, _ = R.expect(c, cos, sin, "R")
        q0, k0, _ = R.expect(c, None, None)
        assert float((q != q0).double().mean()) >= 1 / 3 and float((k != k0).double().mean()) >= 1 / 3
