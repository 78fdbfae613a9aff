"""DoRA fine-tuning without a GPU: the exported names and declared symbols, the DoraLinear wrapper, add_dora /
dora_state_dict / merge_dora / disable_dora, every refusal by its message, and the argument checks of ops.dora_compose /
ops.dora_bwd and of the two C entry points (they come before any launch)."""
import ctypes
import os
import re

import pytest
import torch

import vyomai_amd as V
from tests.golden import cases_causal_lm as C
from tests.golden import cases_dora as R
from vyomai_amd import _lib, dora_train, ops
from vyomai_amd._lib import VyomHipError

KW = C.CASES[R.CASE]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vyom_hip.h")


def model():
    m = V.ModelForCausalLM(V.Config(**KW))
    C.load_weights_(m)
    return m


def test_names_are_exported_and_symbols_declared():
    for name in ("DoraLinear", "add_dora", "dora_state_dict", "merge_dora", "disable_dora"):
        assert hasattr(V, name), name
    assert callable(ops.dora_compose) and callable(ops.dora_bwd)
    lib = _lib.load()
    assert lib.vy_abi_version() == 5, "the additions are additive"
    with open(HEADER) as f:
        text = f.read()
    for name in ("vy_dora_compose", "vy_dora_bwd"):
        assert name in _lib.PROTOTYPES and name in _lib.ALL_SYMBOLS and hasattr(lib, name), name
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text).group(1)
        assert len(_lib.PROTOTYPES[name]) == proto.count(",") + 1, name
    # the descriptor of the binding is the header's, field for field
    body = re.search(r"typedef struct vy_dora_desc \{(.*?)\} vy_dora_desc;", text, re.S).group(1)
    fields = []
    for decl in body.replace("\n", " ").split(";"):
        if decl.strip():
            first, *more = decl.split(",")
            fields += [first.split()[-1].lstrip("*")] + [x.strip().lstrip("*") for x in more]
    assert fields == [n.rstrip("_") for n, _ in _lib.VyDoraDesc._fields_]


def test_dora_linear_attributes_and_init():
    torch.manual_seed(0)
    lin = torch.nn.Linear(512, 256, bias=True)
    m = V.DoraLinear(lin, rank=32)
    assert m.linear is lin and (m.in_features, m.out_features, m.rank) == (512, 256, 32)
    assert tuple(m.dora_m.shape) == (1, 512) and tuple(m.dora_a.shape) == (256, 32) and tuple(m.dora_b.shape) == (32, 512)
    assert m.weight is lin.weight and m.bias is lin.bias and m.enabled
    assert sorted(m.state_dict()) == ["dora_a", "dora_b", "dora_m", "linear.bias", "linear.weight"], "the reference's keys"
    assert all(p.requires_grad for p in (m.dora_m, m.dora_a, m.dora_b))
    assert torch.equal(m.dora_m.detach(), lin.weight.detach().norm(p=2, dim=0, keepdim=True))
    assert bool((m.dora_b == 0).all())
    a = m.dora_a.detach()
    # randn / sqrt(rank) over 8192 values: mean 0 +- 4 sigma / sqrt(n), std 1 / sqrt(32) within 5 %
    assert abs(float(a.mean())) < 4 * 32 ** -0.5 / 90 and abs(float(a.std()) * 32 ** 0.5 - 1) < 0.05
    assert V.DoraLinear(torch.nn.Linear(64, 32)).rank == 32


def test_dora_linear_refusals():
    lin = torch.nn.Linear(64, 32)
    for rank in (0, 65, 2.5):
        with pytest.raises(ValueError, match=f"rank {rank} must be"):
            V.DoraLinear(lin, rank=rank)
    with pytest.raises(ValueError, match="in_features 36 and out_features 32 must be multiples of 8"):
        V.DoraLinear(torch.nn.Linear(36, 32))
    with pytest.raises(ValueError, match="in_features 64 and out_features 20 must be multiples of 8"):
        V.DoraLinear(torch.nn.Linear(64, 20))
    with pytest.raises(ValueError, match="wraps an nn.Linear"):
        V.DoraLinear(V.DoraLinear(lin))
    with pytest.raises(VyomHipError, match="MI355X only: DoraLinear got a CPU tensor"):
        V.DoraLinear(lin)(torch.zeros(2, 64))


def test_add_dora_keys_and_frozen_base():
    base_keys = set(model().state_dict())
    for who, spec in R.ADAPTERS.items():
        m = V.add_dora(model(), rank=spec["rank"], targets=spec["on"])
        dora_keys = set(R.adapter_state(who))
        renamed = set()
        for k in base_keys:
            path, leaf = k.rsplit(".", 1)
            renamed.add(f"{path}.linear.{leaf}" if path + ".dora_a" in dora_keys else k)
        assert set(m.state_dict()) == renamed | dora_keys
        assert {n for n, p in m.named_parameters() if p.requires_grad} == dora_keys
        sd = V.dora_state_dict(m)
        assert set(sd) == dora_keys
        assert all(tuple(sd[k].shape) == R.adapter_state(who)[k].shape for k in sd)
        assert m.model.layers[0].self_attn.q_proj.rank == spec["rank"]
        assert dora_train.layer_has_dora(m.model.layers[1])
    # the packed-QKV and gate/up machinery still finds the base weights
    a = m.model.layers[0].self_attn
    assert [tuple(p.shape) for p in a._params()[:3]] == [(256, 256), (128, 256), (128, 256)]
    assert tuple(a._packed()[0].shape) == (512, 256)
    assert tuple(m.model.layers[0].mlp._packed_gate_up(torch.float32).shape) == (1024, 256)


def test_add_dora_refusals():
    m = model()
    with pytest.raises(ValueError, match="targets .* must be a non-empty subset"):
        V.add_dora(m, targets=("self_attn.q_proj", "lm_head"))
    with pytest.raises(ValueError, match="targets .* must be a non-empty subset"):
        V.add_dora(m, targets=())
    with pytest.raises(ValueError, match="targets .* must be a non-empty subset"):
        V.add_dora(m, targets=("mlp.up_proj", "mlp.up_proj"))
    with pytest.raises(ValueError, match="rank 65 must be"):
        V.add_dora(m, rank=65)
    assert all(p.requires_grad for p in m.parameters()), "a refused call changes nothing"
    assert not any(isinstance(x, V.DoraLinear) for x in m.modules())
    V.add_dora(m, rank=8, targets=("mlp.down_proj",))
    with pytest.raises(ValueError, match="already carries DoRA adapters"):
        V.add_dora(m, rank=8)
    with pytest.raises(ValueError, match="carries DoRA adapters.*merge_dora"):
        V.add_lora(m, rank=8)
    with pytest.raises(ValueError, match="carries LoRA adapters.*merge_lora"):
        V.add_dora(V.add_lora(model(), rank=8, targets=("mlp.up_proj",)), rank=8)
    with pytest.raises(ValueError, match="prepares a ModelForCausalLM, not a Linear"):
        V.add_dora(torch.nn.Linear(64, 64))


def test_wrapped_model_refuses_the_cached_and_paged_paths():
    m = V.add_dora(model(), rank=8)
    ids = torch.zeros((1, 4), dtype=torch.long)
    for call, what in ((lambda: m.generate(ids), r"generate\(\)"), (lambda: m.forward_paged(ids[0], None, {}, None), r"forward_paged\(\)")):
        with pytest.raises(VyomHipError, match=what) as e:
            call()
        assert "merge_dora" in str(e.value)
    with V.disable_dora(m):      # the base model: the guard lets it through to the device check
        with pytest.raises(VyomHipError, match="CPU tensor"):
            m.generate(ids)


def test_merge_dora_vs_the_fp64_formula_and_disable_dora():
    m = V.add_dora(model(), rank=8, targets=("self_attn.v_proj", "mlp.up_proj"))
    state = R.adapter_state("d2")
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.requires_grad:
                p.copy_(torch.from_numpy(state[n]))
    want = {}
    for l, layer in enumerate(m.model.layers):
        for name, mod in (("self_attn.v_proj", layer.self_attn.v_proj), ("mlp.up_proj", layer.mlp.up_proj)):
            d = mod.linear.weight.detach().double() + mod.dora_a.detach().double() @ mod.dora_b.detach().double()
            want[f"model.layers.{l}.{name}.weight"] = d * (mod.dora_m.detach().double() / (d * d).sum(dim=0).sqrt())
    untouched = {k: v.clone() for k, v in m.state_dict().items() if "q_proj" in k}
    mods = [x for x in m.modules() if isinstance(x, V.DoraLinear)]
    assert len(mods) == 4
    with V.disable_dora(m):
        assert not any(x.enabled for x in mods) and not dora_train.layer_has_dora(m.model.layers[0])
        with V.disable_dora(m):
            assert not any(x.enabled for x in mods)
        assert not any(x.enabled for x in mods), "nested: still disabled after the inner context"
    assert all(x.enabled for x in mods)
    with pytest.raises(RuntimeError, match="boom"):
        with V.disable_dora(m):
            raise RuntimeError("boom")
    assert all(x.enabled for x in mods) and dora_train.layer_has_dora(m.model.layers[0])
    assert V.merge_dora(m) is m
    assert not any(isinstance(x, V.DoraLinear) for x in m.modules())
    assert set(m.state_dict()) == set(model().state_dict())
    sd = m.state_dict()
    for k, w in want.items():
        err = float((sd[k].double() - w).abs().max() / w.abs().max())
        assert err < 1e-6, (k, err)          # fp32 arithmetic against fp64
        assert float((sd[k].double() - model().state_dict()[k].double()).abs().max()) > 1e-3, "the merge moved the weight"
    for k, v in untouched.items():
        assert torch.equal(sd[k], v), k
    assert V.dora_state_dict(m) == {}


def test_the_serving_store_still_refuses_dora_keys():
    m = V.add_dora(model(), rank=8)
    store = V.LoraAdapters(model(), 1, device="cpu")
    with pytest.raises(ValueError, match="DoRA renormalises the whole weight"):
        store.load("tuned", V.dora_state_dict(m))
    assert store.slots == {}


def test_host_checks_of_the_ops_entries():
    def problem(out_f=16, in_f=8, r=4, **kw):
        z = lambda *s: torch.zeros(s)   # noqa: E731
        base = dict(w=z(out_f, in_f), a=z(out_f, r), b=z(r, in_f), m=z(1, in_f), c=z(in_f), wp=z(out_f, in_f), g=z(out_f, in_f),
                    dm=z(1, in_f), da=z(out_f, r), db=z(r, in_f))
        base.update(kw)
        return ops.DoraProblem(**base)
    for fn in (ops.dora_compose, lambda ps: ops.dora_bwd(ps, accumulate=False)):
        with pytest.raises(VyomHipError, match="CPU tensor"):      # everything valid: only the device is wrong
            fn([problem()])
        with pytest.raises(ValueError, match="1 to 8 problems"):
            fn([])
        with pytest.raises(ValueError, match="1 to 8 problems"):
            fn([problem()] * 9)


def test_c_entry_points_check_their_arguments_before_any_launch():
    """VY_ERR_ARG with the entry point's name in the message; the pointers are never dereferenced on the host."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def rc(fn, n=1, flag=0, **kw):
        d = (_lib.VyDoraDesc * 1)()
        for name in ("w", "a", "b", "m", "c", "wp", "g", "dm", "da", "db"):
            setattr(d[0], name, p)
        d[0].ldw = d[0].ldwp = d[0].ldg = 8
        d[0].w_dtype, d[0].out, d[0].in_, d[0].r = _lib.VY_F32, 8, 8, 1
        for k, v in kw.items():
            setattr(d[0], k, v)
        return getattr(lib, fn)(ctypes.cast(d, ctypes.c_void_p), n, flag, None)

    shared = [dict(in_=12), dict(in_=0), dict(out=12), dict(out=4), dict(r=0), dict(r=65), dict(ldw=7), dict(w_dtype=3),
              dict(w=None), dict(a=None), dict(b=None), dict(m=None), dict(c=None)]
    for fn, own in (("vy_dora_compose", [dict(wp=None), dict(ldwp=7)]),
                    ("vy_dora_bwd", [dict(g=None), dict(dm=None), dict(da=None), dict(db=None), dict(ldg=7)])):
        for kw in shared + own:
            assert rc(fn, **kw) == -1, (fn, kw)          # VY_ERR_ARG
            assert fn.encode() in lib.vy_last_error(), (fn, kw)
        assert rc(fn, n=0) == -1 and rc(fn, n=9) == -1
        assert rc(fn, flag=2) == -1, "an unknown out_dtype / accumulate"
    assert lib.vy_dora_compose(None, 1, 0, None) == -1
    # (no call with valid arguments here: where a GPU and a registered workspace exist it would launch on host pointers)
