// The 64 x 64 transposing tile of vy_transpose_batched, as one device function: transpose_batched_kernel (vy_misc.hip)
// and the transposing rider workgroups of the vocabulary weight gradient (vy_bwd.hip) both call it, so the two cannot
// drift.  block -> matrix by bisection of the tile prefix; 16-byte loads along the input rows, 16-byte stores along the
// output rows, the transposition through LDS (row pitch 66 elements: the eight column reads of a store hit different
// banks).
#pragma once
#include "vy_common.h"

template <typename T>
struct VyTransposeTile {
  static constexpr int PITCH = 66;
  static constexpr int ELEMS = 64 * PITCH;            // LDS elements of one tile
  static constexpr int VEC = 16 / (int)sizeof(T);     // 8 (bf16) or 4 (fp32)
  static constexpr int CPRW = 64 / VEC;               // 16-byte chunks per 64-element row
};

// the descriptor of tile b (workgroup-uniform: the table is read with scalar loads)
__device__ __forceinline__ vy_transpose_desc vy_transpose_find(const vy_transpose_desc* __restrict__ descs, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile0 <= b) lo = mid; else hi = mid - 1;
  }
  return descs[lo];
}

// Tiles first .. first + count - 1 of the table (count <= G) by one workgroup of NT threads: the loads of all of them
// are issued before the one barrier, so a workgroup that is alone on its CU (the riders) has G tiles in flight.
// `lds`: G * VyTransposeTile<T>::ELEMS elements.
template <typename T, int G, int NT>
__device__ __forceinline__ void vy_transpose_tiles(const vy_transpose_desc* __restrict__ descs, int n, int first,
                                                   int count, T* __restrict__ lds) {
  typedef VyTransposeTile<T> TT;
  typedef typename Chunk<T>::Raw Raw;
  constexpr int VEC = TT::VEC, CPRW = TT::CPRW, PITCH = TT::PITCH;
  const int tid = threadIdx.x;
#pragma unroll 1
  for (int g = 0; g < G; ++g) {
    if (g >= count) break;
    const vy_transpose_desc d = vy_transpose_find(descs, n, first + g);
    T* tile = lds + g * TT::ELEMS;
    const int t = first + g - d.tile0;
    const int c0 = (t % d.tiles_c) * 64, r0 = (t / d.tiles_c) * 64;
    const T* in = (const T*)d.in;
    const bool vec_in = (d.ldin % VEC) == 0 && ((uintptr_t)in % 16) == 0;
    for (int c = tid; c < 64 * CPRW; c += NT) {
      const int r = c / CPRW, cc = (c % CPRW) * VEC;
      const int gr = r0 + r, gc = c0 + cc;
      if (gr >= d.R) continue;
      if (vec_in && gc + VEC <= d.C) {
        const Raw raw = *reinterpret_cast<const Raw*>(in + (int64_t)gr * d.ldin + gc);
        const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
        for (int k = 0; k < VEC; ++k) tile[r * PITCH + cc + k] = e[k];
      } else {
        for (int k = 0; k < VEC; ++k)
          if (gc + k < d.C) tile[r * PITCH + cc + k] = in[(int64_t)gr * d.ldin + gc + k];
      }
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int g = 0; g < G; ++g) {
    if (g >= count) break;
    const vy_transpose_desc d = vy_transpose_find(descs, n, first + g);
    const T* tile = lds + g * TT::ELEMS;
    const int t = first + g - d.tile0;
    const int c0 = (t % d.tiles_c) * 64, r0 = (t / d.tiles_c) * 64;
    T* out = (T*)d.out;
    const bool vec_out = (d.ldout % VEC) == 0 && ((uintptr_t)out % 16) == 0;
    for (int c = tid; c < 64 * CPRW; c += NT) {
      const int oc = c / CPRW, rr = (c % CPRW) * VEC;   // output row = input column c0 + oc
      const int gc = c0 + oc, gr = r0 + rr;
      if (gc >= d.C) continue;
      if (vec_out && gr + VEC <= d.R) {
        Raw raw;
        T* e = reinterpret_cast<T*>(&raw);
#pragma unroll
        for (int k = 0; k < VEC; ++k) e[k] = tile[(rr + k) * PITCH + oc];
        *reinterpret_cast<Raw*>(out + (int64_t)gc * d.ldout + gr) = raw;
      } else {
        for (int k = 0; k < VEC; ++k)
          if (gr + k < d.R) out[(int64_t)gc * d.ldout + gr + k] = tile[(rr + k) * PITCH + oc];
      }
    }
  }
}
