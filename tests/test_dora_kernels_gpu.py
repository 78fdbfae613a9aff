"""vy_dora_compose and vy_dora_bwd through ops.dora_compose / ops.dora_bwd against fp64 torch autograd on the CPU.

The forward, in this test's own words: D = W + a @ b; c = the Euclidean norm of each COLUMN of D (over the output rows,
no epsilon); W' = D with column k scaled by m[k] / c[k].  The backward reference is autograd of sum(G * W') in fp64.

Bars.  c and an fp32 W': rel_err < 1e-5, the project's fp32 forward bar.  A bf16 W': |got - ref| <= 2^-8 |ref| per
element -- the kernel rounds its fp32 value once, and that value may sit on the other side of a rounding boundary from
the fp64 one.  dm, da, db: rel_err < 1e-4, the project's fp32 gradient bar.

Measured on the MI355X, worst over all tables: c 5.2e-8, fp32 W' 1.5e-7, dm 3.3e-7, da 1.1e-6, db 2.9e-7; the bf16 bar
is never exceeded since the compose forms D in fp64 (with an fp32 chain one element of 1032x264r64, where W and a @ b
cancel, missed it by 8.5e-9: the bar has no absolute floor)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ABSENT = None        # a part of a packed group without an adapter: no problem of the launch
SENTINEL = 7.0

# table -> [(in, [(out, r | ABSENT) of each part of one packed destination])]
SINGLE = {"8x8r1": (8, 8, 1), "72x40r8": (72, 40, 8), "264x520r32": (264, 520, 32), "1032x264r64": (1032, 264, 64)}
TABLES = {name: [(i, [(o, r)])] for name, (o, i, r) in SINGLE.items()}
TABLES.update({
    "a.qkv": [(256, [(256, 32), (128, ABSENT), (128, 32)])],
    "a.o": [(256, [(256, 32)])],
    "a.gate_up": [(256, [(512, 32), (512, 32)])],
    "a.down": [(512, [(256, 32)])],
    "mix7": [(8, [(8, 1)]), (40, [(72, 8)]), (520, [(264, 32)]), (264, [(1032, 64)]),
             (256, [(256, 32), (128, ABSENT), (128, 16)]), (512, [(256, 8)])],
})


def rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


_CASES = {}


def case(table: str, wdt):
    """The inputs of a table and their fp64 results, computed once: a list of groups (in, parts); a part is None
    (absent) or a dict of CPU tensors W (in wdt), a, b, m, G and the references c, Wp, dm, da, db."""
    key = (table, wdt)
    if key in _CASES:
        return _CASES[key]
    gen = torch.Generator().manual_seed(sum(map(ord, table)))
    groups = []
    for in_f, parts in TABLES[table]:
        made = []
        for out_f, r in parts:
            if r is ABSENT:
                made.append(None)
                continue
            W = (torch.randn(out_f, in_f, generator=gen) * 0.05).to(wdt)
            a = torch.randn(out_f, r, generator=gen) * r ** -0.5
            b = torch.randn(r, in_f, generator=gen) * 0.05
            D0 = W.double() + a.double() @ b.double()
            m = (D0.pow(2).sum(0).sqrt() * (0.75 + 0.5 * torch.rand(in_f, generator=gen, dtype=torch.float64))).float()
            G = torch.randn(out_f, in_f, generator=gen)
            a64, b64, m64 = (t.double().requires_grad_(True) for t in (a, b, m))
            D = W.double() + a64 @ b64
            c = (D * D).sum(dim=0).sqrt()
            Wp = D * (m64 / c)
            (Wp * G.double()).sum().backward()
            made.append(dict(W=W, a=a, b=b, m=m, G=G, out=out_f, r=r, c=c.detach(), Wp=Wp.detach(), dm=m64.grad,
                             da=a64.grad, db=b64.grad))
        groups.append((in_f, made, [o for o, _ in parts]))
    _CASES[key] = groups
    return groups


def on_gpu(table, wdt, odt, ld_pad, seed_outputs=None):
    """-> (problems, packed destinations, parts) on the GPU; seed_outputs: a generator for non-zero dm / da / db."""
    from vyomai_amd import ops
    problems, dests, flat = [], [], []
    for in_f, made, outs in case(table, wdt):
        dest = torch.full((sum(outs), in_f + ld_pad), SENTINEL, dtype=odt, device=DEV)
        dests.append((dest, in_f, made, outs))
        row = 0
        for part, out_f in zip(made, outs):
            if part is not None:
                r = part["r"]

                def grad_buf(*shape):
                    if seed_outputs is None:
                        return torch.empty(shape, dtype=torch.float32, device=DEV)
                    return torch.randn(shape, generator=seed_outputs).to(DEV)
                problems.append(ops.DoraProblem(
                    w=part["W"].to(DEV), a=part["a"].to(DEV), b=part["b"].to(DEV), m=part["m"].to(DEV),
                    c=torch.empty(in_f, dtype=torch.float32, device=DEV), wp=dest[row:row + out_f, :in_f],
                    g=part["G"].to(DEV), dm=grad_buf(in_f), da=grad_buf(out_f, r), db=grad_buf(r, in_f)))
                flat.append(part)
            row += out_f
    return problems, dests, flat


@pytest.mark.parametrize("ld_pad", (0, 8))
@pytest.mark.parametrize("odt", (torch.float32, BF), ids=("out_fp32", "out_bf16"))
@pytest.mark.parametrize("wdt", (torch.float32, BF), ids=("w_fp32", "w_bf16"))
@pytest.mark.parametrize("table", sorted(TABLES))
def test_compose_and_backward_vs_fp64(table, wdt, odt, ld_pad):
    from vyomai_amd import ops
    problems, dests, flat = on_gpu(table, wdt, odt, ld_pad)
    assert len(problems) <= 8
    ops.dora_compose(problems)
    ops.dora_bwd(problems, accumulate=False)
    torch.cuda.synchronize()
    for p, ref in zip(problems, flat):
        what = f"{table} ({ref['out']}, {p.w.shape[1]}, r {ref['r']})"
        e = rel_err(p.c, ref["c"])
        print(f"{what}: c rel_err {e:.2e}")
        assert e < 1e-5, (what, "c", e)
        got, want = p.wp.double().cpu(), ref["Wp"]
        if odt == torch.float32:
            e = rel_err(p.wp, want)
            print(f"{what}: fp32 W' rel_err {e:.2e}")
            assert e < 1e-5, (what, "Wp", e)
        else:
            over = ((got - want).abs() - 2.0 ** -8 * want.abs()).max().item()
            print(f"{what}: bf16 W' worst |got - ref| - 2^-8 |ref| = {over:.2e}")
            assert over <= 0.0, (what, "Wp bf16", over)
        for name in ("dm", "da", "db"):
            e = rel_err(getattr(p, name), ref[name])
            print(f"{what}: {name} rel_err {e:.2e}")
            assert e < 1e-4, (what, name, e)
    # what the table does not name stays as it was: the rows of an absent part and the columns behind `in`
    for dest, in_f, made, outs in dests:
        assert bool((dest[:, in_f:] == SENTINEL).all()), f"{table}: columns behind in = {in_f} were written"
        row = 0
        for part, out_f in zip(made, outs):
            if part is None:
                assert bool((dest[row:row + out_f] == SENTINEL).all()), f"{table}: rows of an absent part were written"
            row += out_f


@pytest.mark.parametrize("table", ("72x40r8", "a.qkv", "mix7"))
def test_accumulate_adds_onto_a_non_zero_buffer(table):
    from vyomai_amd import ops
    gen = torch.Generator().manual_seed(3)
    problems, _, flat = on_gpu(table, torch.float32, torch.float32, 0, seed_outputs=gen)
    before = [{n: getattr(p, n).clone() for n in ("dm", "da", "db")} for p in problems]
    ops.dora_compose(problems)
    ops.dora_bwd(problems, accumulate=True)
    for p, ref, old in zip(problems, flat, before):
        for name in ("dm", "da", "db"):
            assert bool(old[name].abs().max() > 0)
            e = rel_err(getattr(p, name) - old[name], ref[name])
            print(f"{table}: accumulated {name} minus its old value rel_err {e:.2e}")
            # (the difference carries the rounding of old + new at the magnitude of old: O(1) values, 2^-24 each)
            assert e < 1e-4, (table, name, e)


@pytest.mark.parametrize("table", ("264x520r32", "mix7"))
def test_two_runs_give_the_same_bits(table):
    from vyomai_amd import ops
    runs = []
    for _ in range(2):
        problems, dests, _ = on_gpu(table, torch.float32, BF, 0)
        ops.dora_compose(problems)
        ops.dora_bwd(problems, accumulate=False)
        runs.append([t.clone() for p in problems for t in (p.c, p.dm, p.da, p.db)] + [d[0].clone() for d in dests])
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_bad_arguments_raise():
    from vyomai_amd import ops
    from vyomai_amd._lib import VyomHipError

    def problem(out_f, in_f, r, **kw):
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)   # noqa: E731
        base = dict(w=z(out_f, in_f), a=z(out_f, r), b=z(r, in_f), m=z(in_f), c=z(in_f), wp=z(out_f, in_f), g=z(out_f, in_f),
                    dm=z(in_f), da=z(out_f, r), db=z(r, in_f))
        base.update(kw)
        return ops.DoraProblem(**base)
    for bad in (problem(8, 12, 4), problem(12, 8, 4), problem(8, 8, 65)):
        with pytest.raises((ValueError, VyomHipError)):
            ops.dora_compose([bad])
        with pytest.raises((ValueError, VyomHipError)):
            ops.dora_bwd([bad], accumulate=False)
    with pytest.raises((ValueError, VyomHipError)):
        ops.dora_compose([problem(8, 8, 1)] * 9)
    with pytest.raises((ValueError, VyomHipError)):
        ops.dora_compose([])
    with pytest.raises((ValueError, VyomHipError)):
        ops.dora_compose([problem(8, 8, 1, wp=torch.zeros(8, 8, device=DEV)[:, :4])])
    with pytest.raises((ValueError, VyomHipError)):
        ops.dora_bwd([problem(8, 8, 1, g=torch.zeros(8, 8, dtype=BF, device=DEV))], accumulate=False)
    # the C entry points refuse the same shapes on their own (VY_ERR_ARG), with nothing launched
    import ctypes as C
    from vyomai_amd import _lib
    lib = _lib.load()
    ok = problem(8, 8, 1)
    for field, value in (("in_", 12), ("out", 4), ("r", 0), ("r", 65), ("ldw", 4)):
        d = (_lib.VyDoraDesc * 1)()
        d[0].w, d[0].ldw, d[0].w_dtype = ok.w.data_ptr(), 8, 0
        d[0].a, d[0].b, d[0].m, d[0].c = ok.a.data_ptr(), ok.b.data_ptr(), ok.m.data_ptr(), ok.c.data_ptr()
        d[0].wp, d[0].ldwp, d[0].g, d[0].ldg = ok.wp.data_ptr(), 8, ok.g.data_ptr(), 8
        d[0].dm, d[0].da, d[0].db = ok.dm.data_ptr(), ok.da.data_ptr(), ok.db.data_ptr()
        d[0].out, d[0].in_, d[0].r = 8, 8, 1
        setattr(d[0], field, value)
        st = torch.cuda.current_stream().cuda_stream
        assert lib.vy_dora_compose(C.cast(d, C.c_void_p), 1, 0, st) == -1, field
        assert lib.vy_dora_bwd(C.cast(d, C.c_void_p), 1, 0, st) == -1, field
    torch.cuda.synchronize()
