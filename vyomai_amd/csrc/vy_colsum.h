// The ordered column sum of fp32 partial slabs: the one statement of the order in which slab rows are added.
//
// Every norm backward (LayerNorm, RMSNorm, QK-norm) leaves a slab of per-workgroup fp32 partials, W rows of N columns,
// and its parameter gradient is the column sum of that slab.  No atomics: the order is fixed, so the gradient has the
// same bits on every run and from every caller.  The order:
//   - the W rows are cut into `slices` row slices of rps = ceil(W / slices) rows, [w0, w1) = [i rps, min(W, (i + 1) rps));
//     slices whose w0 >= W do not exist (W = 70 has 14 slices of 5, not 16).  LayerNorm and RMSNorm take
//     vy_ln_colsum_slices(W) (vy_common.h), QK-norm always one;
//   - within a slice, row group g = 0..3 starts from 0.f and adds rows w0 + g, w0 + g + 4, ... in increasing order
//     (eight loads are in flight per thread and slab; the adds stay sequential);
//   - the four group sums are added as ((p0 + p1) + p2) + p3;
//   - with one slice the result is (acc ? out : 0.f) + sum; with several, the slice sums are added from 0.f in slice
//     order, then (acc ? out : 0.f) + total.
// Slab s (of S = 1 or 2 summed together), row w, column n lives at ws[s * slab_stride + w * ld + n].
//
// vy_colsum (vy_misc.hip) runs it as launches of its own, the grouped weight-gradient launch (vy_bwd.hip) in spare
// workgroups; both take a slice's sum from the two functions below (in a header: the library is built without
// relocatable device code).  tests/colsum_rule.py restates the order and holds every caller to it bit for bit.
#pragma once
#include "vy_common.h"

// The first half, up to the barrier: the calling thread is column c = threadIdx.x & 63 of row group
// g = (threadIdx.x >> 6) & 3; it adds its rows of slice [w0, w1) of each slab at column n and leaves the group sums in
// red[s][g][c] (0.f where !live or the slice is empty).  The caller holds the __syncthreads() -- the riding workgroup
// shares one between two slices -- and then reads vy_colsum_slice_sum.
template <int S>
__device__ __forceinline__ void vy_colsum_slice_groups(const float* __restrict__ ws, int64_t slab_stride, int ld, int n,
                                                       bool live, int w0, int w1, float (*red)[4][64]) {
  const int c = threadIdx.x & 63, g = (threadIdx.x >> 6) & 3;
  float a[S];
#pragma unroll
  for (int s = 0; s < S; ++s) a[s] = 0.f;
  if (live) {
    // eight rows of every slab requested at once (one round trip for the usual 32-row slice; a loop of dependent
    // 4-byte loads made the LayerNorm's 3 MB reduction an 11.8 us launch, 25 times per step), summed in row order
    for (int wb = w0 + g; wb < w1; wb += 32) {
      float v[S][8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int w = wb + 4 * i;
        const int wc = w < w1 ? w : wb;
#pragma unroll
        for (int s = 0; s < S; ++s) v[s][i] = ws[s * slab_stride + (int64_t)wc * ld + n];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (wb + 4 * i < w1) {
#pragma unroll
          for (int s = 0; s < S; ++s) a[s] += v[s][i];
        }
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) red[s][g][c] = a[s];
}

// The second half, behind the barrier: the slice's sum of slab s at column c.  A group sum starts from +0.f, so neither
// it nor this sum is ever -0.f: 0.f + sum has the bits of sum.
__device__ __forceinline__ float vy_colsum_slice_sum(const float (*red)[4][64], int s, int c) {
  return ((red[s][0][c] + red[s][1][c]) + red[s][2][c]) + red[s][3][c];
}
