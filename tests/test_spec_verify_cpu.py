"""vy_spec_verify without a GPU: the C ABI (header, binding and library agree; argument errors come back as VY_ERR_ARG
before any launch) and the ValueErrors of ops.spec_verify."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from vyomai_amd import _lib, ops

NAME = "vy_spec_verify"


def test_header_binding_and_library_agree_on_the_symbol():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "vyom_hip.h").read_text()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert NAME in _lib.ALL_SYMBOLS and NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    proto = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(_lib.PROTOTYPES[NAME]) == proto.count(",") + 1 == 21
    at = hdr.index("int " + NAME + "(")
    doc = hdr[hdr.rindex("/* " + NAME, 0, at):at]
    for cite in ("speculative_decoding.py:73-83", "195-230", "logits_processors.py:13-16"):
        assert cite in doc, "the entry cites the reference's lines"
    assert _lib.load().vy_abi_version() == 5            # the symbol is additive


def test_argument_errors_are_reported_without_a_gpu():
    raw = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(raw) + 255) // 256 * 256
    ptrs = ("target", "draft", "tokens", "t_row0", "n_draft", "inv_t", "top_k", "top_p", "seed", "position0", "accept",
            "alt")

    def go(ldt=64, t_rows=10, ldd_i=128, ldd_s=64, S=2, gamma=4, V=37, dtype=1, **kw):
        a = {name: kw.get(name, p) for name in ptrs}
        _lib.call(NAME, a["target"], ldt, t_rows, a["draft"], ldd_i, ldd_s, S, gamma, V, dtype, a["tokens"], a["t_row0"],
                  a["n_draft"], a["inv_t"], a["top_k"], a["top_p"], a["seed"], a["position0"], a["accept"], a["alt"], None)

    for name in ptrs:
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*vy_spec_verify: null operand"):
            go(**{name: None})
    for bad in (dict(gamma=0), dict(gamma=17), dict(gamma=-1), dict(S=0), dict(S=-2), dict(t_rows=0), dict(ldt=36),
                dict(ldd_s=36), dict(ldd_i=-1), dict(V=0), dict(V=0x7ffffff1, ldt=0x7ffffff8, ldd_s=0x7ffffff8)):
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*vy_spec_verify: bad shape"):
            go(**bad)
    for bad in (2, -1):
        with pytest.raises(_lib.VyomHipError, match=r"\(-1\).*vy_spec_verify: bad dtype"):
            go(dtype=bad)


def test_wrapper_raises_value_errors():
    S, G, Vv = 3, 2, 16
    t, d = torch.zeros(S * (G + 1), Vv), torch.zeros(G, S, Vv)
    tok = torch.zeros(G, S, dtype=torch.long)
    f, i, l = torch.zeros(S), torch.zeros(S, dtype=torch.int32), torch.zeros(S, dtype=torch.long)

    def go(t=t, d=d, tok=tok, t_row0=i, n_draft=i, inv_t=f, top_k=i, top_p=f, seed=l, position0=l):
        return ops.spec_verify(t, d, tok, t_row0, n_draft, inv_t, top_k, top_p, seed, position0)

    with pytest.raises(ValueError, match="target logits"):
        go(t=torch.zeros(Vv))
    with pytest.raises(ValueError, match="target logits"):
        go(t=torch.zeros(Vv, S * (G + 1)).t())
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        go(t=t.half(), d=d.half())
    with pytest.raises(ValueError, match="draft logits"):
        go(d=torch.zeros(S, Vv))
    with pytest.raises(ValueError, match="draft logits"):
        go(d=torch.zeros(G, S, Vv + 1))
    with pytest.raises(ValueError, match="draft logits"):
        go(d=torch.zeros(17, S, Vv))
    with pytest.raises(ValueError, match="draft logits are"):
        go(d=d.bfloat16())
    with pytest.raises(ValueError, match="draft_tokens"):
        go(tok=tok.int())
    with pytest.raises(ValueError, match="draft_tokens"):
        go(tok=torch.zeros(S, G, dtype=torch.long))
    with pytest.raises(ValueError, match="t_row0"):
        go(t_row0=l)
    with pytest.raises(ValueError, match="n_draft"):
        go(n_draft=i[:2])
    with pytest.raises(ValueError, match="inv_temperature"):
        go(inv_t=f.double())
    with pytest.raises(ValueError, match="top_k"):
        go(top_k=l)
    with pytest.raises(ValueError, match="top_p"):
        go(top_p=torch.zeros(2 * S)[::2])
    with pytest.raises(ValueError, match="seed"):
        go(seed=i)
    with pytest.raises(ValueError, match="position0"):
        go(position0=i)
    with pytest.raises(ValueError, match="is on"):
        go(seed=l.to("meta"))
    with pytest.raises(ValueError, match="is on"):
        go(d=d.to("meta"))
    with pytest.raises(_lib.VyomHipError, match="CPU tensor"):       # no fallback
        go()
