"""The epilogue's batched second-operand requests (vy_debug_set_epilogue_prefetch) on and off, in one process with
interleaved rounds, on the two launches of the training step they change: the FFN2 dgrad (256 x 256 tiles, * saved act')
and the QKV dgrad (256 x 192 tiles, + two residual gradients), at the benchmark's shapes (32 x 512 rows, d = 768).
  python tools/epilogue_ab.py [rounds] [launches per round]"""
import ctypes as C, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vyomai_amd import ops, _lib
lib = _lib.load()
lib.vy_debug_set_epilogue_prefetch.argtypes = [C.c_int]
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
it = int(sys.argv[2]) if len(sys.argv) > 2 else 50
M, d = 16384, 768
bf, dev = torch.bfloat16, "cuda"
g = torch.Generator().manual_seed(0)
r = lambda *s: torch.randn(*s, generator=g).to(bf).to(dev)
dy_d, dy_3d = r(M, d), r(M, 3 * d)
wqkv_t, w2_t = r(d, 3 * d) / 48, r(4 * d, d) / 28      # W^T layouts: [N_out = in_features][K = out_features]
deriv, res, res2 = r(M, 4 * d), r(M, d), r(M, d)
out_d, out_4d = torch.empty(M, d, dtype=bf, device=dev), torch.empty(M, 4 * d, dtype=bf, device=dev)
cases = {
    "ffn2 dgrad (N 3072, K 768, * saved act')": lambda: ops.linear_dgrad(dy_d, w2_t, pre=deriv, act=_lib.ACT_GELU_ERF | _lib.ACT_SAVE_DERIV, out=out_4d),
    "qkv dgrad  (N 768, K 2304, + 2 residuals)": lambda: ops.linear_dgrad(dy_3d, wqkv_t, add_to=res, add_to2=res2, out=out_d),
    "qkv dgrad  (N 768, K 2304, + 1 residual)": lambda: ops.linear_dgrad(dy_3d, wqkv_t, add_to=res, out=out_d),
}


def t(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e3


for name, fn in cases.items():
    us = {0: [], 1: []}
    for on in (1, 0):                 # warm both paths
        lib.vy_debug_set_epilogue_prefetch(on); fn(); fn()
    torch.cuda.synchronize()
    for rnd_ in range(rounds):
        for on in ((1, 0) if rnd_ % 2 == 0 else (0, 1)):
            lib.vy_debug_set_epilogue_prefetch(on)
            us[on].append(t(fn))
    lib.vy_debug_set_epilogue_prefetch(1)
    f = lambda v: f"median {statistics.median(v):6.1f} us  min {min(v):6.1f}  max {max(v):6.1f}"
    print(f"{name}:  prefetch on: {f(us[1])}  |  off: {f(us[0])}  |  on/off {statistics.median(us[1]) / statistics.median(us[0]):.3f}")
