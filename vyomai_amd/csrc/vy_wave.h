// Wave reductions on the DPP / permlane path (no LDS round trips), shared by the decode-step kernels (vy_decode.hip),
// the paged-cache attention (vy_paged.hip) and the 16x16x32 attention tile core (vy_attn_gen.h: dec_rows_max /
// dec_rows_sum are its exchanges between the four lane groups of a query row); at the end the lane-group helpers of the
// per-head kernels (vy_paged.hip's rope / quantise writes, vy_qknorm.hip): pow2_group_sum / _max and Quad<T>.
#pragma once
#include "vy_common.h"

// sum over the 64 lanes, result in every lane: four DPP rotations inside each row of 16 lanes, then the two
// half-swaps (v_permlane16_swap, v_permlane32_swap) -- six VALU instructions, no LDS round trips
__device__ __forceinline__ float dec_row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));  // row_ror:2
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));  // row_ror:1
  return v;
}
__device__ __forceinline__ float dec_wave_sum(float v) {
  v = dec_row16_sum(v);
  const unsigned u = __builtin_bit_cast(unsigned, v);
  auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = __builtin_bit_cast(float, (unsigned)s16[0]) + __builtin_bit_cast(float, (unsigned)s16[1]);
  const unsigned w = __builtin_bit_cast(unsigned, v);
  auto s32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __builtin_bit_cast(float, (unsigned)s32[0]) + __builtin_bit_cast(float, (unsigned)s32[1]);
}
// sum over the four 16-lane rows of the wave at each position inside a row (lanes l, l ^ 16, l ^ 32, l ^ 48), in every
// lane: the two half-swaps of dec_wave_sum without the in-row rotations
__device__ __forceinline__ float dec_rows_sum(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = __builtin_bit_cast(float, (unsigned)s16[0]) + __builtin_bit_cast(float, (unsigned)s16[1]);
  const unsigned w = __builtin_bit_cast(unsigned, v);
  auto s32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __builtin_bit_cast(float, (unsigned)s32[0]) + __builtin_bit_cast(float, (unsigned)s32[1]);
}
// the maximum over the same four lanes, in every lane
__device__ __forceinline__ float dec_rows_max(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = fmaxf(__builtin_bit_cast(float, (unsigned)s16[0]), __builtin_bit_cast(float, (unsigned)s16[1]));
  const unsigned w = __builtin_bit_cast(unsigned, v);
  auto s32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned)s32[0]), __builtin_bit_cast(float, (unsigned)s32[1]));
}
__device__ __forceinline__ float dec_row16_max(float v) {
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false)));
  return v;
}
__device__ __forceinline__ float dec_wave_max(float v) {
  v = dec_row16_max(v);
  const unsigned u = __builtin_bit_cast(unsigned, v);
  auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = fmaxf(__builtin_bit_cast(float, (unsigned)s16[0]), __builtin_bit_cast(float, (unsigned)s16[1]));
  const unsigned w = __builtin_bit_cast(unsigned, v);
  auto s32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned)s32[0]), __builtin_bit_cast(float, (unsigned)s32[1]));
}

template <int LPK>
__device__ __forceinline__ float dec_group_sum(float v) {   // sum over the LPK lanes of a key group, in every lane
  if constexpr (LPK == 8) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    return v;
  } else if constexpr (LPK == 16) {
    return dec_row16_sum(v);
  } else if constexpr (LPK == 64) {
    return dec_wave_sum(v);
  } else {   // 32 lanes: a row of 16, then the neighbouring row
    v = dec_row16_sum(v);
    const unsigned u = __builtin_bit_cast(unsigned, v);
    auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return __builtin_bit_cast(float, (unsigned)s16[0]) + __builtin_bit_cast(float, (unsigned)s16[1]);
  }
}
// sum over the lanes that hold the same chunk ch (stride LPK), in every lane
template <int LPK>
__device__ __forceinline__ float dec_stride_sum(float v) {
  if constexpr (LPK == 64) return v;
  if constexpr (LPK == 16) return dec_rows_sum(v);
  if constexpr (LPK == 8) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
    const unsigned u = __builtin_bit_cast(unsigned, v);
    auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __builtin_bit_cast(float, (unsigned)s16[0]) + __builtin_bit_cast(float, (unsigned)s16[1]);
  }
  const unsigned w = __builtin_bit_cast(unsigned, v);
  auto s32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __builtin_bit_cast(float, (unsigned)s32[0]) + __builtin_bit_cast(float, (unsigned)s32[1]);
}

// sum over the 1 << lg lanes of a lane group (aligned to its size inside the wave, at most 32 lanes), in every lane of
// it.  lg is wave-uniform, so the steps are scalar branches; the DPP steps and the row swap read neighbouring lanes,
// so EVERY lane of the wave must arrive here (no early return, no divergent branch around the call).
__device__ __forceinline__ float pow2_group_sum(float v, int lg) {
  if (lg >= 1) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  if (lg >= 2) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  if (lg >= 3) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));  // row_half_mirror
  if (lg >= 4) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
  if (lg >= 5) {   // the neighbouring row of 16
    const unsigned u = __builtin_bit_cast(unsigned, v);
    auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __builtin_bit_cast(float, (unsigned)s16[0]) + __builtin_bit_cast(float, (unsigned)s16[1]);
  }
  return v;
}

// the maximum over the same lane group, under the same rule: every lane of the wave arrives
__device__ __forceinline__ float pow2_group_max(float v, int lg) {
  if (lg >= 1) v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false)));
  if (lg >= 2) v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false)));
  if (lg >= 3) v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false)));
  if (lg >= 4) v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false)));
  if (lg >= 5) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = fmaxf(__builtin_bit_cast(float, (unsigned)s16[0]), __builtin_bit_cast(float, (unsigned)s16[1]));
  }
  return v;
}

// four consecutive elements (8 bytes of bf16, 16 of fp32): half a head is a multiple of 4 elements, not of 8
template <typename T> struct Quad;
template <> struct Quad<float> {
  static __device__ __forceinline__ void load(const float* p, float* v) { Chunk<float>::load(p, v); }
  static __device__ __forceinline__ void store(float* p, const float* v) { Chunk<float>::store(p, v); }
};
template <> struct Quad<bf16> {
  static __device__ __forceinline__ void load(const bf16* p, float* v) {
    const bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)t[e];
  }
  static __device__ __forceinline__ void store(bf16* p, const float* v) {
    bf16x4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = (bf16)v[e];
    *reinterpret_cast<bf16x4*>(p) = t;
  }
};
