// Qwen3's qk_norm in front of the rotation: the arithmetic of ONE (token, head) unit, shared by the serving kernel
// (paged_qknorm_rope_write_kernel, vy_paged.hip) and the training forward (qknorm_rope_fwd_kernel, vy_qknorm.hip).  A
// unit is a group of 1 << lg lanes (dh / 8 of them at work, vy_wave.h: pow2_group_sum); a lane holds columns
// i4 .. i4 + 3 of the lower half of the head (lo) and the same 4 of the upper half (hi).
// The two kernels are NOT bit-equal: hipcc contracts a * c - b * s into an fma for some elements and not for others,
// differently from kernel to kernel (see paged_quant_write_fp8_kernel).
#pragma once
#include "vy_wave.h"

// the lane's share of sum x^2 as an fma chain, then the group sum: every lane of the wave calls this, idle lanes with
// zeros in lo / hi
__device__ __forceinline__ float qk_group_sumsq(const float (&lo)[4], const float (&hi)[4], int lg) {
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) ss = fmaf(lo[e], lo[e], ss);
#pragma unroll
  for (int e = 0; e < 4; ++e) ss = fmaf(hi[e], hi[e], ss);
  return pow2_group_sum(ss, lg);
}

// the rotate_half pairing (d, d + dh/2) with row `pos` of the fp32 tables [rows][half], in fp32
__device__ __forceinline__ void rope_rotate_quads(float (&lo)[4], float (&hi)[4], const float* __restrict__ cos_tab,
                                                  const float* __restrict__ sin_tab, long long pos, int half, int i4) {
  const f32x4 c = *reinterpret_cast<const f32x4*>(cos_tab + pos * half + i4);
  const f32x4 s = *reinterpret_cast<const f32x4*>(sin_tab + pos * half + i4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a = lo[e], bb = hi[e];
    lo[e] = a * c[e] - bb * s[e];
    hi[e] = bb * c[e] + a * s[e];
  }
}

// lo / hi <- rotate(x * rsqrt(ss / dh + eps) * scale): ss is the unit's sum of squares (qk_group_sumsq), scale the fp32
// [dh] weight of the head's kind.  An all-zero head gives 0 * rsqrt(eps) = 0.  The caller rounds once, at its store.
__device__ __forceinline__ void qknorm_rope_quads(float (&lo)[4], float (&hi)[4], float ss, float inv_dh, float eps,
                                                  const float* __restrict__ scale, const float* __restrict__ cos_tab,
                                                  const float* __restrict__ sin_tab, long long pos, int half, int i4) {
  const float r = rsqrtf(fmaf(ss, inv_dh, eps));
  const f32x4 wl = *reinterpret_cast<const f32x4*>(scale + i4);
  const f32x4 wh = *reinterpret_cast<const f32x4*>(scale + half + i4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lo[e] = lo[e] * r * wl[e];
    hi[e] = hi[e] * r * wh[e];
  }
  rope_rotate_quads(lo, hi, cos_tab, sin_tab, pos, half, i4);
}
