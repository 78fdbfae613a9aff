"""FFN1 launch per activation code ("Every reference hidden_act"): M = 16384, N = 3072, K = 768, bf16,
with VY_ACT_SAVE_DERIV, as FfnBlockFn issues it.  Codes 1-2 run their compile-time instantiations, 3-7 the one run-time-code
instantiation.  Each code is timed --rounds times in an interleaved order, so the spread of repeated runs of one code is
seen next to the differences between codes.

    python tools/bench_ffn1_act.py                               # this tree's library
    VY_LIB_PATH=<another libvyom_hip.so> python tools/bench_ffn1_act.py --codes 1,2    # same box, another build
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vyomai_amd import ops, _lib  # noqa: E402

NAMES = {0: "none", 1: "gelu_erf", 2: "gelu_tanh", 3: "silu", 4: "tanh", 5: "sigmoid", 6: "relu6", 7: "leaky_relu"}


def timeit(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--codes", default="1,2,3,4,5,6,7")
    a = ap.parse_args()
    M, N, K = 16384, 3072, 768
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(M, K, generator=g).to(bf).to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(bf).to(dev)
    b = torch.randn(N, generator=g).to(bf).to(dev)
    out = torch.empty(M, N, dtype=bf, device=dev)
    pre = torch.empty(M, N, dtype=bf, device=dev)
    codes = [int(c) for c in a.codes.split(",")]
    times = {c: [] for c in codes}
    for _ in range(a.rounds):
        for c in codes:
            times[c].append(timeit(lambda: ops.linear(x, w, b, act=c | _lib.ACT_SAVE_DERIV, pre_out=pre, out=out), a.iters))
    print(f"library: {_lib.LIB_PATH}")
    for c in codes:
        t = times[c]
        print(f"act {c} {NAMES[c]:10s} median {statistics.median(t):7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}  "
              f"({2.0 * M * N * K / statistics.median(t) * 1e-6:6.1f} TFLOP/s)  runs: " + " ".join(f"{v:.1f}" for v in t))


if __name__ == "__main__":
    main()
