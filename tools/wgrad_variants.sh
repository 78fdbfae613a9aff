#!/bin/bash
# The six bf16 weight-gradient kernels, each through the tests and the micro-benchmark.  Two of them run by default; the
# others are reached only through VY_WGRAD_VARIANT (0: 128 x 128 tiles, 8: 256 x 256) and VY_WGRAD_M16 (0: 32x32x16 MFMAs,
# 1: 16x16x32 on the 256 x 256 tiles, 2: everywhere), which the library reads once per process.  The first failing step
# ends the script.
set -e
cd "$(dirname "$0")/.."
for v in 0 8; do
  for m in 0 1 2; do
    echo "== VY_WGRAD_VARIANT=$v VY_WGRAD_M16=$m"
    VY_WGRAD_VARIANT=$v VY_WGRAD_M16=$m timeout -k 10 300 python -m pytest tests/test_bwd_kernels_gpu.py -m gpu -q -x -k wgrad
    VY_WGRAD_VARIANT=$v VY_WGRAD_M16=$m timeout -k 10 300 python tools/bench_wgrad.py
  done
done
