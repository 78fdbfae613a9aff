"""vy_linear_wgrad_grouped_opt without a GPU: the symbol is exported and declared, the ABI version did not move, and the
host-side refusals (which come before any launch) return VY_ERR_ARG on host memory."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_declared_and_the_abi_version_stays():
    from vyomai_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vyom_hip.h")).read()
    assert re.search(r"\bint\s+vy_linear_wgrad_grouped_opt\s*\(", hdr)
    for name in ("vy_adamw_ride_desc", "vy_adamw_hyper"):
        assert re.search(r"\}\s*%s\s*;" % name, hdr), name
    assert "vy_linear_wgrad_grouped_opt" in _lib.PROTOTYPES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "vy_linear_wgrad_grouped_opt")
    assert _lib.load().vy_abi_version() == 5


class _Host:
    """Host memory standing in for the device arrays: the refusals never touch it."""

    def __init__(self):
        self.buf = (C.c_char * (1 << 16))()
        self.base = (C.addressof(self.buf) + 127) // 128 * 128

    def at(self, off):
        return self.base + off


def _ride(h, n=64, **kw):
    from vyomai_amd import _lib
    d = dict(p=h.at(0), g=h.at(4096), m=h.at(8192), v=h.at(12288), p_bf16=h.at(16384), n=n, taken=-7)
    d.update(kw)
    opt = (_lib.VyAdamwRideDesc * 1)()
    for k, val in d.items():
        setattr(opt[0], k, val)
    return opt


def _hyper(step=1):
    from vyomai_amd import _lib
    return _lib.VyAdamwHyper(5e-5, 0.9, 0.999, 1e-8, 0.01, 1.0, step)


def _call(opt, nopt, hy, descs=None, n=0, cs=None, ncs=0):
    from vyomai_amd import _lib
    _lib.call("vy_linear_wgrad_grouped_opt", C.cast(descs, C.c_void_p) if descs is not None else None, n,
              C.cast(cs, C.c_void_p) if cs is not None else None, ncs, C.cast(opt, C.c_void_p), nopt,
              C.byref(hy) if hy is not None else None, _lib.VY_BF16, None)


@pytest.mark.parametrize("what,kw,match", [
    ("n <= 0", dict(n=0), "bad arguments"),
    ("null p", dict(p=None), "bad arguments"),
    ("null g", dict(g=None), "bad arguments"),
    ("null m", dict(m=None), "bad arguments"),
    ("null v", dict(v=None), "bad arguments"),
    ("p off by 8 bytes", dict(p=8), "aligned"),
    ("g off by 4 bytes", dict(g=4096 + 4), "aligned"),
    ("m off by 8 bytes", dict(m=8192 + 8), "aligned"),
    ("v off by 12 bytes", dict(v=12288 + 12), "aligned"),
    ("shadow off by 4 bytes", dict(p_bf16=16384 + 4), "aligned"),
])
def test_range_refusals(what, kw, match):
    from vyomai_amd import _lib
    h = _Host()
    kw = {k: (h.at(val) if k != "n" and val is not None else val) for k, val in kw.items()}
    with pytest.raises(_lib.VyomHipError, match=match):
        _call(_ride(h, **kw), 1, _hyper())


def test_count_step_and_hyper_refusals():
    from vyomai_amd import _lib
    h = _Host()
    with pytest.raises(_lib.VyomHipError, match="0..8 AdamW ranges"):
        _call(_ride(h), 9, _hyper())
    with pytest.raises(_lib.VyomHipError, match="0..8 AdamW ranges"):
        _call(_ride(h), 1, None)
    with pytest.raises(_lib.VyomHipError, match="step"):
        _call(_ride(h), 1, _hyper(step=0))
    with pytest.raises(_lib.VyomHipError, match="1..8 descriptors"):
        _call(None, 0, None)


def test_a_range_that_meets_an_output_of_the_launch_is_refused():
    """g, p and the shadow against dw, db, out0, out1 and the slab."""
    from vyomai_amd import _lib
    h = _Host()
    desc = (_lib.VyWgradDesc * 1)()
    d = desc[0]
    d.dy, d.lddy, d.x, d.ldx, d.M, d.N, d.K = h.at(32768), 8, h.at(36864), 8, 16, 8, 8
    d.dw, d.lddw, d.db = h.at(20480), 8, h.at(24576)          # dw: 256 bytes, db: 32 bytes
    cs = (_lib.VyColsumDesc * 1)()
    c = cs[0]
    c.ws, c.W, c.N, c.out0, c.out1, c.acc = h.at(40960), 2, 8, h.at(45056), h.at(49152), 1   # slab: 128 bytes
    for field in ("g", "p", "p_bf16"):
        for target in (20480 + 128, 24576 + 16, 45056, 49152 + 16, 40960 + 64):
            with pytest.raises(_lib.VyomHipError, match="intersects"):
                _call(_ride(h, n=4, **{field: h.at(target)}), 1, _hyper(), desc, 1, cs, 1)
    # a range that starts before dw and ends 16 bytes into it
    with pytest.raises(_lib.VyomHipError, match="intersects"):
        _call(_ride(h, n=8, g=h.at(20480 - 16)), 1, _hyper(), desc, 1, cs, 1)
