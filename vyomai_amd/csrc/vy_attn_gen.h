// The tile core of the 16x16x32 attention forward kernels (bf16): attn_fwd_gen_kernel<96|256> in vy_attn.hip (contiguous
// K/V, the head widths the tuned 32x32x16 kernels of vy_attn_tile.h do not serve) and paged_prefill_kernel<64|96|128|256>
// in vy_paged.hip (packed variable-length segments, keys read through a block table).  A workgroup is 4 waves = 64 query
// rows (16 per wave) of one head; K/V tiles of 64 keys x DHP columns (the head width rounded up, the surplus columns
// zeros) pass through registers into ONE LDS tile pair.
//   * swapped QK^T: A = 16 keys, B = the wave's 16 query rows -> a lane owns ONE query row (r16 = lane & 15) and, per
//     16-key block, the 4 consecutive keys 4 kq .. 4 kq + 3 (kq = lane >> 4): the softmax of a row is 16 register values
//     and the exchanges between the four lane groups (dec_rows_max / dec_rows_sum, vy_wave.h);
//   * P stays in registers as the B operand of O^T = V^T P^T: a k-step of 32 keys takes the lane's 4 + 4 values of two key
//     blocks, i.e. the contraction index is walked in the order the scores already sit in -- and V^T's fragments are read
//     in the same order by two transposing LDS reads (ds_read_b64_tr_b16) of the row-major tile.
// What is written here once: the constants, the Q-fragment load, the register -> LDS tile store, the transposing-read
// address, one tile's step and the epilogue store.  A kernel keeps its argument struct, its grid decode, where a key row
// comes from and when its registers are requested, its visibility predicate, its barriers (in the kernel body, as
// vy_attn_tile.h prescribes for the ring frame) and whatever else only it needs.  Everything is a __forceinline__ member
// that takes the kernel's registers by reference; nothing here knows which kernel calls it.
#pragma once
#include "vy_common.h"
#include "vy_wave.h"
#include <float.h>

namespace {

template <int DHP>
struct AttnGen {
  static constexpr int PITCH = (DHP + 8) * 2;       // bytes per LDS row (16 B of padding: conflict-free fragment reads)
  static constexpr int KS = DHP / 32;               // k-steps of QK^T
  static constexpr int NDB = DHP / 16;              // 16-wide d blocks of O^T
  static constexpr int CPRW = DHP / 8;              // 16-byte chunks per row
  static constexpr int CPT = 64 * CPRW / 256;       // chunks per thread and tile
  static constexpr int LDS_BYTES = 2 * 64 * PITCH;  // the K tile, then the V tile
  static_assert(DHP % 32 == 0 && (64 * CPRW) % 256 == 0, "tile chunks must divide over the workgroup");

  static __device__ __forceinline__ bf16x8 zero8() {
    return bf16x8{(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
  }
  static __device__ __forceinline__ char* v_tile(char* smem) { return smem + 64 * PITCH; }

  // this lane's query row as the B operand of every k-step, zero past the head width
  static __device__ __forceinline__ void load_q(bf16x8 (&qf)[KS], const bf16* Q, int dh, int kq) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = 32 * ks + 8 * kq;
      qf[ks] = d0 < dh ? *reinterpret_cast<const bf16x8*>(Q + d0) : zero8();
    }
  }
  // chunk i of a thread is 16-byte chunk `ch` of tile row `row`: the mapping of the kernels' fetches and of store_tile
  static __device__ __forceinline__ void chunk_of(int tid, int i, int& row, int& ch) {
    const int cidx = tid + 256 * i;
    row = cidx / CPRW;
    ch = cidx - row * CPRW;
  }
  static __device__ __forceinline__ void store_tile(char* kt, char* vt, const bf16x8 (&kreg)[CPT], const bf16x8 (&vreg)[CPT],
                                                    int tid) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      int row, ch;
      chunk_of(tid, i, row, ch);
      *reinterpret_cast<bf16x8*>(kt + row * PITCH + ch * 16) = kreg[i];
      *reinterpret_cast<bf16x8*>(vt + row * PITCH + ch * 16) = vreg[i];
    }
  }
  // transposing-read addresses of the V tile: lane j of a 16-lane group supplies row (j >> 2), columns 4 (j & 3) ..
  static __device__ __forceinline__ unsigned vtr_addr(const char* vt, int r16, int kq) {
    return vy_lds_addr(vt) + (4 * kq + (r16 >> 2)) * PITCH + (4 * (r16 & 3)) * 2;
  }

  // The tile at keys k0 .. k0 + 63, which is in LDS: scores, mask, the running maximum, the rescale of (l, O) and
  // O^T += V^T P^T.  vis(kj) says whether this lane's query row sees key kj; c = scale * log2(e).
  template <typename Vis>
  static __device__ __forceinline__ void step(const char* kt, unsigned vtr, const bf16x8 (&qf)[KS], f32x4 (&o)[NDB],
                                              float& m_run, float& l_run, float c, int k0, int r16, int kq, Vis vis) {
    // S^T = K Q^T: four 16-key blocks
    f32x4 sc[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      sc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kt + (16 * blk + r16) * PITCH + (32 * ks + 8 * kq) * 2);
        sc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], sc[blk], 0, 0, 0);
      }
    }
    // masks: register r of block blk is key k0 + 16 blk + 4 kq + r
    float tmax = -INFINITY;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float tv = vis(k0 + 16 * blk + 4 * kq + r) ? sc[blk][r] : -INFINITY;
        sc[blk][r] = tv;
        tmax = fmaxf(tmax, tv);
      }
    tmax = dec_rows_max(tmax);   // the row's keys are spread over the four lane groups (lane >> 4)
    const float m_new = fmaxf(m_run, tmax * c);   // (-inf * c stays -inf; m_run is finite)
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int n = 0; n < NDB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[n][r] *= alpha;
    float rs = 0.f;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(sc[blk][r], c, -m_run));
        sc[blk][r] = e;
        rs += e;
      }
    l_run += rs;   // this lane group's keys only; the four groups are added at the end (dec_rows_sum)
    // O^T += V^T P^T, k-steps of 32 keys = blocks (2 tt, 2 tt + 1) in the order the scores sit in
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      bf16x8 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) { pf[r] = (bf16)sc[2 * tt][r]; pf[4 + r] = (bf16)sc[2 * tt + 1][r]; }
      vy_static_for<NDB>([&](auto n_c) {
        constexpr int n = decltype(n_c)::value;
        union { struct { s16x4 a, b; } h; bf16x8 v; } u;
        u.h.a = vy_lds_tr16_off<n * 32>(vtr + (32 * tt) * PITCH);
        u.h.b = vy_lds_tr16_off<n * 32>(vtr + (32 * tt + 16) * PITCH);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        vy_tie(u.v);
        o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(u.v, pf, o[n], 0, 0, 0);
      });
    }
  }

  // this lane's columns d = 16 n + 4 kq + r of its row, times inv = 1 / the row total, where they exist
  static __device__ __forceinline__ void store_row(bf16* orow, const f32x4 (&o)[NDB], float inv, int dh, int kq) {
#pragma unroll
    for (int n = 0; n < NDB; ++n) {
      const int d0 = 16 * n + 4 * kq;
      if (d0 < dh) {
        bf16x4 w;
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = (bf16)(o[n][r] * inv);
        *reinterpret_cast<bf16x4*>(orow + d0) = w;
      }
    }
  }
};

}  // namespace
