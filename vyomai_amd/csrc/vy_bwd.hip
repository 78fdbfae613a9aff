// Backward kernels of the block (bf16 storage, fp32 accumulation):
//
//   vy_linear_wgrad  dW[N,K] += dY[M,N]^T . X[M,K]   "TN" GEMM: the contraction index m is the
//                    slow index of BOTH operands, so both MFMA fragments are transposing LDS reads
//                    (ds_read_b64_tr_b16) of row-major [m][n] / [m][k] tiles staged by LDS-DMA.
//                    M is split over workgroups (few (n,k) tiles exist at d=768) and partial tiles
//                    are summed with fp32 atomics shaped as two 128-B row segments per wave
//                    instruction.  db = column sums of dY (separate streaming kernel).
//   vy_attn_bwd      flash attention backward as two MFMA kernels without atomics:
//                      dq kernel:   per 128 query rows, sweep keys (S^T, dP^T, dQ^T products);
//                      dkdv kernel: per 128 keys of one kv head, sweep the n_rep query heads and
//                                   query tiles (S, dP, dV^T, dK^T products), GQA sum in registers.
//                    P is recomputed from the forward's log-sum-exp; the row constants -lse/scale
//                    and -delta are the initial values of the S and dP accumulators.
//
// The backward formulas are the ones autograd derives for the reference modules; the attention
// one is spelled out by the reference author in Examples/vyom-ai-decoder-fused.ipynb cell 7
// (dS = P o (dP - rowsum(dO o O))).
#include "vy_attn_tile.h"
#include "vy_colsum.h"
#include "vy_transpose_tile.h"
#include <float.h>
#include <string.h>

namespace {


__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

__device__ __forceinline__ bf16x8 tr_pair(const char* base, int row_bytes) {
  // two transposing reads 8 rows apart -> the 8 k-elements of one 32x32x16 operand
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VY_LDS s16x4*)(base));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VY_LDS s16x4*)(base + 8 * row_bytes));
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = lo; u.s.b = hi;
  return u.v;
}

// ------------------------------------------------------------------------------------------
// wgrad: dW[n,k] += sum_m dY[m,n] X[m,k]
// tile BT(n) x BT(k), MS rows of m per stage; (BT/64) x 2 waves, each 64(n) x BT/2(k); split over M.
// Two shapes are built: 128 x 128 with 64-row stages in a 2-deep ring (64 KiB of LDS, two workgroups per CU) and
// 256 x 256 with 32-row stages in a 4-deep ring (128 KiB, one workgroup per CU).
// The kernel is three parts: WgradTile (the LDS image of a stage and its writer), one ring in wgrad_tn_bf16_body
// (when a stage is requested, which vmcnt is waited for, where the barrier sits) and a fragment policy per MFMA
// shape, WgradMma32 / WgradMma16 (accumulators, the k-step schedule of one stage, bias gradient, atomic epilogue):
// the 128 x 128 tile runs on mfma_f32_32x32x16_bf16, the 256 x 256 tile on mfma_f32_16x16x32_bf16.
// ------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// One stage of an operand in LDS: MS rows of BT bf16, row-major, staged by LDS-DMA in 1-KiB pieces (wave w owns
// pieces w PP .. w PP + PP - 1), with the 64-byte swizzle (row & 3) << 6 on the source side.  MF16: the
// transposing reads of a 16-lane group take the 4 rows 4 (lane >> 4) + q (and + 16), so the two groups of a 32-lane
// half read DIFFERENT rows of the same columns: a second swizzle bit ((row >> 2) & 1) << 5 puts them in the two
// 32-byte halves of a 64-byte slot (conflict-free).  The dY and the X tile have the same shape, so a lane's row and
// column within a piece are the same for both.
template <int BT, int MS_, bool MF16>
struct WgradTile {
  static constexpr int MS = MS_;                     // rows of m per stage
  static constexpr int NW = BT / 32;                 // waves: (BT/64) x 2
  static constexpr int WKT = BT / 2;                 // k extent of a wave
  static constexpr int ROWB = BT * 2;                // LDS row bytes of either tile
  static constexpr int TILE = MS * ROWB, STAGE = 2 * TILE;   // a stage: the dY tile, then the X tile
  static constexpr int PP = TILE / 1024 / NW;        // LDS-DMA pieces per wave and operand
  static_assert(PP * 1024 * NW == TILE, "tile / wave layout mismatch");

  int wave, nst, m_begin, m_end;
  bool ragged;                                       // the last stage holds fewer than MS rows
  int row[PP];
  const bf16* a_ptr[PP]; const bf16* b_ptr[PP];
  int64_t a_step[PP], b_step[PP];
  const bf16* zero;

  // Per-piece source pointers are advanced by MS rows per stage (one 64-bit add each) instead of being
  // rebuilt from row * ld every stage (the 64-bit multiplies and selects were ~120 instructions per
  // stage and wave, next to 16 MFMAs).  A lane whose columns lie beyond N / K reads the zero page all
  // along; only the LAST stage of a chunk can have rows beyond m_end and takes the checked path.
  __device__ __forceinline__ WgradTile(const bf16* __restrict__ dY, int64_t lddy, const bf16* __restrict__ X, int64_t ldx,
                                       int n0, int k0, int N, int K, int m_begin_, int m_end_, int wave_, int lane) {
    wave = wave_, m_begin = m_begin_, m_end = m_end_;
    nst = (m_end - m_begin + MS - 1) / MS;
    ragged = ((m_end - m_begin) % MS) != 0;
    zero = reinterpret_cast<const bf16*>(vy_zero16);
    sources(dY, lddy, n0, N, lane, a_ptr, a_step);
    sources(X, ldx, k0, K, lane, b_ptr, b_step);
  }
  // the lane's 16 bytes of each of the wave's pieces of stage 0, and the step to the next stage
  __device__ __forceinline__ void sources(const bf16* __restrict__ src, int64_t ld, int c0, int C, int lane,
                                          const bf16* (&ptr)[PP], int64_t (&step)[PP]) {
#pragma unroll
    for (int t = 0; t < PP; ++t) {
      const int P = (wave * PP + t) * 1024 + lane * 16;
      const int r = P / ROWB, off = P % ROWB;
      const int col = (off ^ (((r & 3) << 6) | (MF16 ? ((r >> 2) & 1) << 5 : 0))) >> 1;
      const bool ok = c0 + col < C;
      row[t] = r;
      ptr[t] = ok ? src + (int64_t)(m_begin + r) * ld + c0 + col : zero;
      step[t] = ok ? (int64_t)MS * ld : 0;
    }
  }
  __device__ __forceinline__ void issue(const bf16* (&ptr)[PP], const int64_t (&step)[PP], int s, char* dst) {
    const bool tail = ragged && s == nst - 1;
    const int rows = m_end - (m_begin + s * MS);
#pragma unroll
    for (int t = 0; t < PP; ++t) {
      const bf16* p = (tail && row[t] >= rows) ? zero : ptr[t];
      __builtin_amdgcn_global_load_lds((const VY_GLOBAL void*)p, (VY_LDS void*)(dst + (wave * PP + t) * 1024), 16, 0, 0);
      ptr[t] += step[t];
    }
  }
  // request stage s (stages are requested in order) into the stage region at `dst`
  __device__ __forceinline__ void stage(int s, char* dst) {
    issue(a_ptr, a_step, s, dst);
    issue(b_ptr, b_step, s, dst + TILE);
  }
};

// db[n] partial of one dY fragment (8 m values of one column n per lane): 4 v_dot2_f32_bf16 against ones on the
// otherwise idle VALU
__device__ __forceinline__ float wgrad_db_dot(const bf16x8& a, float s) {
  const bf16x2_t ones2 = {(__bf16)1.0f, (__bf16)1.0f};
  union { bf16x8 v; bf16x2_t h[4]; } u_;
  u_.v = a;
#pragma unroll
  for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_fdot2_f32_bf16(u_.h[e], ones2, s, false);
  return s;
}

// mfma_f32_32x32x16_bf16: 2 x TJ blocks of 32 x 32 per wave, 16 rows of m per k-step.
template <class T>
struct WgradMma32 {
  static constexpr int TJ = T::WKT / 32, KS = T::MS / 16, ROWB = T::ROWB;
  f32x16 acc[2][TJ];
  float sdb[2];
  int fr, fh;
  unsigned a_lds[2], b_lds[TJ];   // LDS byte address of fragment column i / j, row tr_row, stage 0 (X: + TILE)

  __device__ __forceinline__ WgradMma32(const char* smem, int lane, int wn, int wk) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    sdb[0] = sdb[1] = 0.f;
    fr = lane & 31, fh = lane >> 5;
    const int li = lane & 15, g16 = (lane >> 4) & 1;
    const int tr_row = 4 * fh + (li >> 2);                  // + 16*s (second read +8)
    const int tr_sw = ((li >> 2) & 3) << 6;                 // (row & 3) << 6
    const int a_rd = (2 * (wn * 64 + 16 * g16 + 4 * (li & 3)));  // + 64*i, then ^ tr_sw
    const int b_rd = (2 * (wk * T::WKT + 16 * g16 + 4 * (li & 3)));
#pragma unroll
    for (int i = 0; i < 2; ++i) a_lds[i] = vy_lds_addr(smem) + tr_row * ROWB + ((a_rd + 64 * i) ^ tr_sw);
#pragma unroll
    for (int j = 0; j < TJ; ++j) b_lds[j] = vy_lds_addr(smem) + tr_row * ROWB + ((b_rd + 64 * j) ^ tr_sw);
  }
  // The stage at byte offset `off`: fragments of k-step ks+1 are requested before the MFMAs of k-step ks (asm reads +
  // counted lgkmcnt: see vy_common.h -- the builtin form would drain the LDS-DMA prefetch first).  One
  // base address per fragment column; the k-step and the +8 row go into the offset field.
  __device__ __forceinline__ void mma_stage(unsigned off, bool do_db) {
    unsigned a_base[2], b_base[TJ];
#pragma unroll
    for (int i = 0; i < 2; ++i) a_base[i] = a_lds[i] + off;
#pragma unroll
    for (int j = 0; j < TJ; ++j) b_base[j] = b_lds[j] + off;
    bf16x8 af[2][2], bfr[2][TJ];
    auto frags = [&](auto ks_c, bf16x8* a_, bf16x8* b_) {
      constexpr int ks = decltype(ks_c)::value;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        a_[i] = vy_lds_tr16_pair_off<16 * ks * ROWB, (16 * ks + 8) * ROWB>(a_base[i]);
#pragma unroll
      for (int j = 0; j < TJ; ++j)
        b_[j] = vy_lds_tr16_pair_off<T::TILE + 16 * ks * ROWB, T::TILE + (16 * ks + 8) * ROWB>(b_base[j]);
    };
    frags(std::integral_constant<int, 0>{}, af[0], bfr[0]);
    vy_static_for<KS>([&](auto ks_c) {
      constexpr int ks = decltype(ks_c)::value;
      constexpr int c_ = ks & 1;
      if constexpr (ks < KS - 1) {
        frags(std::integral_constant<int, ks + 1>{}, af[c_ ^ 1], bfr[c_ ^ 1]);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * (2 + TJ)) : "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) vy_tie(af[c_][i]);
#pragma unroll
      for (int j = 0; j < TJ; ++j) vy_tie(bfr[c_][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[c_][i], bfr[c_][j], acc[i][j], 0, 0, 0);
      // the dY fragments are already in registers: row n = lane & 31, 8 m values per lane
      if (do_db) {
#pragma unroll
        for (int i = 0; i < 2; ++i) sdb[i] = wgrad_db_dot(af[c_][i], sdb[i]);
      }
    });
  }
  // nw / kw: first dW row / column of the wave's sub-tile
  __device__ __forceinline__ void epilogue(float* __restrict__ dW, int64_t lddw, float* __restrict__ db, bool do_db,
                                           float alpha, int nw, int kw, int N, int K) {
    if (do_db) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float t_ = (sdb[i] + __shfl_xor(sdb[i], 32, 64)) * alpha;   // the one cross-half add
        const int n = nw + 32 * i + fr;
        if (fh == 0 && n < N) atomicAdd(db + n, t_);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int k = kw + 32 * j + fr;
        if (k >= K) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = nw + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fh;
          if (n < N) atomicAdd(dW + (int64_t)n * lddw + k, acc[i][j][r] * alpha);
        }
      }
  }
};

// mfma_f32_16x16x32_bf16 (as in the forward / dgrad GEMMs: fewer cycles per stage and a higher clock, vy_gemm.hip):
// 4 x TJ blocks of 16 x 16 per wave, 32 rows of m per k-step.
template <class T>
struct WgradMma16 {
  static constexpr int TI = 4, TJ = T::WKT / 16, KS = T::MS / 32, JH = TJ / 2, ROWB = T::ROWB;
  f32x4 acc[TI][TJ];
  float sdb[TI];
  int r16, kq;
  unsigned a_lds[TI], b_lds[TJ];   // stage 0, k-step 0, first read (rows 4 kq + q_)

  __device__ __forceinline__ WgradMma16(const char* smem, int lane, int wn, int wk) {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TI; ++i) sdb[i] = 0.f;
    r16 = lane & 15, kq = lane >> 4;
    const int q_ = r16 >> 2, p_ = r16 & 3;
    const int sw16 = (q_ << 6) | ((kq & 1) << 5);
#pragma unroll
    for (int i = 0; i < TI; ++i) a_lds[i] = vy_lds_addr(smem) + (4 * kq + q_) * ROWB + ((2 * (wn * 64 + 16 * i + 4 * p_)) ^ sw16);
#pragma unroll
    for (int j = 0; j < TJ; ++j)
      b_lds[j] = vy_lds_addr(smem) + (4 * kq + q_) * ROWB + ((2 * (wk * T::WKT + 16 * j + 4 * p_)) ^ sw16);
  }
  // The stage at byte offset `off`, per k-step: the dY fragments and the first half of the X fragments, the second half
  // requested before the first half's MFMAs (counted lgkmcnt: two reads per fragment)
  __device__ __forceinline__ void mma_stage(unsigned off, bool do_db) {
    unsigned a_base[TI], b_base[TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) a_base[i] = a_lds[i] + off;
#pragma unroll
    for (int j = 0; j < TJ; ++j) b_base[j] = b_lds[j] + off;
    vy_static_for<KS>([&](auto ks_c) {
      constexpr int ks = decltype(ks_c)::value;
      bf16x8 af[TI], bfr[TJ];
      vy_static_for<TI>([&](auto i_c) {
        constexpr int i = decltype(i_c)::value;
        af[i] = vy_lds_tr16_pair_off<32 * ks * ROWB, (32 * ks + 16) * ROWB>(a_base[i]);
      });
      vy_static_for<TJ>([&](auto j_c) {
        constexpr int j = decltype(j_c)::value;
        bfr[j] = vy_lds_tr16_pair_off<T::TILE + 32 * ks * ROWB, T::TILE + (32 * ks + 16) * ROWB>(b_base[j]);
      });
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * JH) : "memory");
#pragma unroll
      for (int i = 0; i < TI; ++i) vy_tie(af[i]);
#pragma unroll
      for (int j = 0; j < JH; ++j) vy_tie(bfr[j]);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < JH; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = JH; j < TJ; ++j) vy_tie(bfr[j]);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = JH; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      // the dY fragments are already in registers: row n = lane & 15, 8 m values per lane
      if (do_db) {
#pragma unroll
        for (int i = 0; i < TI; ++i) sdb[i] = wgrad_db_dot(af[i], sdb[i]);
      }
    });
  }
  // nw / kw: first dW row / column of the wave's sub-tile
  __device__ __forceinline__ void epilogue(float* __restrict__ dW, int64_t lddw, float* __restrict__ db, bool do_db,
                                           float alpha, int nw, int kw, int N, int K) {
    if (do_db) {
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        float t_ = sdb[i];
        t_ += __shfl_xor(t_, 16, 64);
        t_ += __shfl_xor(t_, 32, 64);
        const int n = nw + 16 * i + r16;
        if (kq == 0 && n < N) atomicAdd(db + n, t_ * alpha);
      }
    }
    // D[n][k] of block (i, j): lane = k index (lane & 15), register r = n row 4 kq + r.  Blocks j and j + 1 trade lane
    // halves (v_permlane32_swap) so that one wave instruction adds rows {r, 4 + r} (then {8 + r, 12 + r}) x 32
    // consecutive k: again two 128-byte row segments
    const bool hi = kq >= 2;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int jp = 0; jp < JH; ++jp) {
        const int k = kw + 16 * (2 * jp + (hi ? 1 : 0)) + r16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned x = __builtin_bit_cast(unsigned, acc[i][2 * jp][r] * alpha);
          const unsigned y = __builtin_bit_cast(unsigned, acc[i][2 * jp + 1][r] * alpha);
          auto sw = __builtin_amdgcn_permlane32_swap(x, y, false, false);
          const int nlo = nw + 16 * i + 4 * (kq & 1) + r;
          if (k < K) {
            if (nlo < N) atomicAdd(dW + (int64_t)nlo * lddw + k, __builtin_bit_cast(float, (unsigned)sw[0]));
            if (nlo + 8 < N) atomicAdd(dW + (int64_t)(nlo + 8) * lddw + k, __builtin_bit_cast(float, (unsigned)sw[1]));
          }
        }
      }
  }
};

// The stage memory of a weight-gradient workgroup: one LDS array per size, so that a workgroup which never runs the tile
// body (a transposing rider, below) can use the same bytes
template <int BYTES>
__device__ __forceinline__ char* wgrad_smem() {
  __shared__ __attribute__((aligned(16))) char smem[BYTES];
  return smem;
}

// The ring: NS stages of LDS, the loads of the next NS-1 stages in flight while a stage is multiplied; a stage is
// waited for with a COUNTED vmcnt (its 2 PP LDS-DMA instructions are the wave's oldest) and one raw s_barrier.
template <int BN, int BKW, int MS, int NS>
__device__ __forceinline__ void wgrad_tn_bf16_body(
    const bf16* __restrict__ dY, int64_t lddy, const bf16* __restrict__ X, int64_t ldx,
    float* __restrict__ dW, int64_t lddw, float* __restrict__ db, const float* __restrict__ alpha_dev,
    int M, int N, int K, int tiles_k, int tiles_nk, int m_chunk, int wg) {
  static_assert(BN == BKW && ((BN == 128 && MS == 64 && NS == 2) || (BN == 256 && MS == 32 && NS == 4)),
                "built shapes: 128 x 128 x 64 in 2 stages, 256 x 256 x 32 in 4");
  // 16 x 16 x 32 MFMAs: 3 % faster on the 256 x 256 tiles (vocabulary projection 1.62 -> 1.57 ms, +0.25 % on the training
  // step), 2-8 % SLOWER on the 128 x 128 tiles (these kernels are bound by the transposing LDS reads and the atomic
  // epilogue, not by the matrix pipe) -- so the MFMA shape follows the tile
  constexpr bool MF16 = BN == 256;
  typedef WgradTile<BN, MS, MF16> Tile;
  typedef std::conditional_t<MF16, WgradMma16<Tile>, WgradMma32<Tile>> Mma;
  constexpr int STAGE = Tile::STAGE, PS = 2 * Tile::PP;   // LDS-DMA instructions per wave and stage
  char* const smem = wgrad_smem<NS * STAGE>();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int split = wg / tiles_nk, t2 = wg - split * tiles_nk;
  const int tile_n = t2 / tiles_k, tile_k = t2 - tile_n * tiles_k;
  const int n0 = tile_n * BN, k0 = tile_k * BKW;
  const int m_begin = split * m_chunk;
  const int m_end = min(M, m_begin + m_chunk);
  if (m_begin >= m_end) return;

  Tile t(dY, lddy, X, ldx, n0, k0, N, K, m_begin, m_end, wave, lane);
  const bool do_db = db != nullptr && tile_k == 0 && wk == 0;   // bias gradient db[n] = sum_m dY[m,n]: the k-tile-0 workgroups
  Mma mma(smem, lane, wn, wk);
  const int nst = t.nst;
#pragma unroll
  for (int s_ = 0; s_ < NS - 1; ++s_)
    if (s_ < nst) t.stage(s_, smem + s_ * STAGE);
  for (int s = 0; s < nst; ++s) {
    const int younger = min(NS - 2, nst - 1 - s);  // stages issued after stage s
    if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PS) : "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (s + NS - 1 < nst) t.stage(s + NS - 1, smem + (s + NS - 1) % NS * STAGE);  // the buffer stage s-1 was read from
    mma.mma_stage(s % NS * STAGE, do_db);
  }
  const float alpha = alpha_dev ? *alpha_dev : 1.0f;
  mma.epilogue(dW, lddw, db, do_db, alpha, n0 + wn * 64, k0 + wk * Tile::WKT, N, K);
}

// Riders of the single-launch 256 x 256 weight gradient (vy_linear_wgrad_riders): the vocabulary projection's 591 tiles
// are 2.31 rounds on 256 CUs, so for about one tile time 177 CUs have nothing to do.  The workgroups behind the
// `items` tile workgroups are dispatched last and move data that no kernel before the launch's end reads or writes:
//   transposing riders  WGRAD_RIDE_TR_TILES consecutive 64 x 64 tiles of a vy_transpose_batched table each (the W^T
//                       refresh), through the stage memory
//   zero riders         one WGRAD_RIDE_ZERO_CHUNK of one fp32 range each (the gradient arena), 16-byte stores
struct ZeroRange { float* p; int64_t n; int blk0; };   // blk0: first chunk of this range
struct WgradRiders {
  ZeroRange z[8]; int nz;
  const vy_transpose_desc* tr; int tr_n, tr_tiles, tr_blocks;   // tr_tiles: the leading tiles that ride; tr_blocks: their workgroups
  int items;                                                    // tile workgroups of the launch (= the grid without riders)
};
constexpr int WGRAD_RIDE_TR_TILES = 8;          // 8 x 8.25 KiB of the 128-KiB stage memory; 64 KiB read + 64 KiB written per rider
constexpr int WGRAD_RIDE_ZERO_CHUNK = 1 << 16;  // floats per zero rider (256 KiB)

template <int NT>
__device__ __forceinline__ void zero_ride_chunk(const ZeroRange& r, int chunk) {
  const int64_t c0 = (int64_t)chunk * WGRAD_RIDE_ZERO_CHUNK;
  const int64_t c1 = c0 + WGRAD_RIDE_ZERO_CHUNK < r.n ? c0 + WGRAD_RIDE_ZERO_CHUNK : r.n;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = c0 + (int64_t)threadIdx.x * 4; i < c1; i += NT * 4) {
    if (i + 3 < c1) {
      *reinterpret_cast<f32x4*>(r.p + i) = z4;
    } else {   // the element-wise tail of a range
      for (int e = 0; e < 4; ++e)
        if (i + e < c1) r.p[i + e] = 0.f;
    }
  }
}

template <int BN, int BKW, int MS, int NS>
__global__ __launch_bounds__(BN * 2, BN == 128 ? 2 : 1) void wgrad_tn_bf16_kernel(
    const bf16* __restrict__ dY, int64_t lddy, const bf16* __restrict__ X, int64_t ldx,
    float* __restrict__ dW, int64_t lddw, float* __restrict__ db, const float* __restrict__ alpha_dev,
    int M, int N, int K, int tiles_k, int tiles_nk, int m_chunk, WgradRiders rd) {
  if constexpr (BN == 256) {
    if ((int)blockIdx.x >= rd.items) {   // (workgroup-uniform) the riders: dispatched behind the tiles, onto the idle CUs
      const int rb = (int)blockIdx.x - rd.items;
      if (rb < rd.tr_blocks) {
        static_assert(WGRAD_RIDE_TR_TILES * VyTransposeTile<bf16>::ELEMS * 2 <= NS * WgradTile<BN, MS, true>::STAGE,
                      "the riders' LDS tiles alias the stage memory");
        const int first = rb * WGRAD_RIDE_TR_TILES;
        vy_transpose_tiles<bf16, WGRAD_RIDE_TR_TILES, BN * 2>(rd.tr, rd.tr_n, first, min(WGRAD_RIDE_TR_TILES, rd.tr_tiles - first),
                                                             reinterpret_cast<bf16*>(wgrad_smem<NS * WgradTile<BN, MS, true>::STAGE>()));
        return;
      }
      const int blk = rb - rd.tr_blocks;
      int d = 0;
#pragma unroll
      for (int i = 1; i < 8; ++i)
        if (i < rd.nz && blk >= rd.z[i].blk0) d = i;
      ZeroRange r = rd.z[0];
#pragma unroll
      for (int i = 1; i < 8; ++i)
        if (d == i) r = rd.z[i];
      zero_ride_chunk<BN * 2>(r, blk - r.blk0);
      return;
    }
  }
  // the tiles keep the block-to-tile mapping of a grid without riders
  wgrad_tn_bf16_body<BN, BKW, MS, NS>(dY, lddy, X, ldx, dW, lddw, db, alpha_dev, M, N, K, tiles_k, tiles_nk, m_chunk,
                                      xcd_remap(blockIdx.x, rd.items));
}

// Several weight gradients in ONE launch (vy_linear_wgrad_grouped): the four GEMMs of a transformer layer
// have 9-36 tiles of 256 x 256 each -- alone, a launch needs 7 M-splits to fill 256 CUs (66 MB of fp32
// atomics); together they are 108 tiles and need 2.  The table travels in the kernel arguments.
struct WgradItem {
  const bf16* dY; const bf16* X; float* dW; float* db;
  int64_t lddy, ldx, lddw;
  int M, N, K, tiles_k, tiles_nk, m_chunk, item0;   // item0: first work item of this GEMM
};
struct WgradGroup { WgradItem g[8]; int n; };

// Column sums of LayerNorm-backward slabs riding in the same launch (vy_linear_wgrad_grouped_cs): a layer's grouped
// launch fills 216 of 256 CUs, and its two LayerNorms' dgamma / dbeta -- 2 x 512 x 768 floats each -- were two launches of
// their own per LayerNorm.  The workgroups behind the `items` weight-gradient ones each take a 64-column block of one
// slab pair, all slices of it, in the summation order of vy_colsum.h.
struct ColsumItem { const float* ws; float* out0; float* out1; int W, N, rps, acc, blk0; };   // blk0: first block of this slab
struct ColsumGroup { ColsumItem c[8]; int n; int items; };

// 512 threads: the two halves of the workgroup take the even and the odd slices, so two slices' rows are in flight at
// once; each half is the 4 row groups x 64 columns of vy_colsum_slice_groups.  A single slice is added to 0.f like any
// other: its sum is never -0.f (vy_colsum.h), so the bits are its own.
__device__ __forceinline__ void colsum_slab_block(const ColsumItem& it, int blk) {
  __shared__ float red[2][2][4][64];
  const int tid = threadIdx.x;
  const int c = tid & 63, h = tid >> 8;
  const int n = blk * 64 + c;
  const int W = it.W, N = it.N, rps = it.rps;
  float ta = 0.f, tb = 0.f;
  for (int s0 = 0; s0 * rps < W; s0 += 2) {
    const int w0 = (s0 + h) * rps, w1 = min(W, w0 + rps);
    vy_colsum_slice_groups<2>(it.ws, (int64_t)W * N, N, n, n < N, w0, w1, red[h]);
    __syncthreads();
    if (tid < 64) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        if ((s0 + hh) * rps < W) {
          ta += vy_colsum_slice_sum(red[hh], 0, c);
          tb += vy_colsum_slice_sum(red[hh], 1, c);
        }
    }
    __syncthreads();
  }
  if (tid < 64 && n < N) {
    if (it.out0) it.out0[n] = (it.acc ? it.out0[n] : 0.f) + ta;
    if (it.out1) it.out1[n] = (it.acc ? it.out1[n] : 0.f) + tb;
  }
}

// AdamW riding in the same launch (vy_linear_wgrad_grouped_opt): the optimizer is the one large HBM-only stream of the
// training step without a data dependence on this launch, and the weight-gradient tiles are MFMA / LDS-ingest bound.
// The workgroups behind the column-sum ones each step one chunk of ADAMW_RIDE_CHUNK elements of one range with the
// body of adamw_kernel (VyAdamw4, vy_common.h).  No device gate, no device scale: those stay on the plain launch.
struct AdamwRange { float* p; const float* g; float* m; float* v; bf16* pb; int64_t n; int blk0; };   // blk0: first chunk of this range
struct AdamwGroup { AdamwRange r[8]; VyAdamwScalars s; int n; int blk0; };                            // blk0: first AdamW workgroup of the launch

// A workgroup is alone on its CU (the kernel's registers and LDS allow one), so the loads in flight are what its 8 waves
// issue before their first use: ADAMW_RIDE_UNROLL independent groups of four 16-byte loads per thread, 128 KiB per CU.
constexpr int ADAMW_RIDE_UNROLL = 4;
constexpr int ADAMW_RIDE_PASS = 512 * 4 * ADAMW_RIDE_UNROLL;   // elements the workgroup steps per pass
constexpr int ADAMW_RIDE_CHUNK = 2 * ADAMW_RIDE_PASS;          // elements per workgroup (16384: 480 KiB of traffic)

__device__ __forceinline__ void adamw_ride_chunk(const AdamwRange& r, const VyAdamwScalars& s, int chunk) {
  const int64_t c0 = (int64_t)chunk * ADAMW_RIDE_CHUNK;
  const int64_t c1 = c0 + ADAMW_RIDE_CHUNK < r.n ? c0 + ADAMW_RIDE_CHUNK : r.n;
  const int tid = threadIdx.x;
  for (int64_t i0 = c0; i0 < c1; i0 += ADAMW_RIDE_PASS) {
    if (i0 + ADAMW_RIDE_PASS <= c1) {
      VyAdamw4 a[ADAMW_RIDE_UNROLL];
#pragma unroll
      for (int u = 0; u < ADAMW_RIDE_UNROLL; ++u) {
        const int64_t i = i0 + (int64_t)(u * 512 + tid) * 4;
        a[u].load(r.p + i, r.g + i, r.m + i, r.v + i);
      }
#pragma unroll
      for (int u = 0; u < ADAMW_RIDE_UNROLL; ++u) {
        const int64_t i = i0 + (int64_t)(u * 512 + tid) * 4;
        a[u].step(s);
        a[u].store(r.p + i, r.m + i, r.v + i, r.pb ? r.pb + i : nullptr);
      }
    } else {   // the last, partial pass of a range: whole groups of four, then adamw_kernel's element-wise tail
#pragma unroll 1
      for (int u = 0; u < ADAMW_RIDE_UNROLL; ++u) {
        const int64_t i = i0 + (int64_t)(u * 512 + tid) * 4;
        if (i + 3 < c1) {
          VyAdamw4 a;
          a.load(r.p + i, r.g + i, r.m + i, r.v + i);
          a.step(s);
          a.store(r.p + i, r.m + i, r.v + i, r.pb ? r.pb + i : nullptr);
        } else if (i < c1) {
          vy_adamw_tail(r.p + i, r.g + i, r.m + i, r.v + i, r.pb ? r.pb + i : nullptr, (int)(c1 - i), s);
        }
      }
    }
  }
}

template <int BN, int BKW, int MS, int NS>
__global__ __launch_bounds__(BN * 2, 1) void wgrad_tn_bf16_grouped_kernel(WgradGroup grp, ColsumGroup cs, AdamwGroup opt) {
  if ((int)blockIdx.x >= opt.blk0) {   // (workgroup-uniform) the AdamW workgroups: dispatched last of all
    const int blk = (int)blockIdx.x - opt.blk0;
    int d = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i)
      if (i < opt.n && blk >= opt.r[i].blk0) d = i;
    AdamwRange r = opt.r[0];
#pragma unroll
    for (int i = 1; i < 8; ++i)
      if (d == i) r = opt.r[i];
    adamw_ride_chunk(r, opt.s, blk - r.blk0);
    return;
  }
  if ((int)blockIdx.x >= cs.items) {   // (workgroup-uniform) the column-sum workgroups: dispatched behind the tiles, onto the idle CUs
    const int blk = (int)blockIdx.x - cs.items;
    int d = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i)
      if (i < cs.n && blk >= cs.c[i].blk0) d = i;
    ColsumItem it = cs.c[0];
#pragma unroll
    for (int i = 1; i < 8; ++i)
      if (d == i) it = cs.c[i];
    colsum_slab_block(it, blk - it.blk0);
    return;
  }
  const int id = xcd_remap(blockIdx.x, cs.items);
  int d = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i)
    if (i < grp.n && id >= grp.g[i].item0) d = i;
  // (selected with a uniform loop: the descriptor lives in SGPRs after this)
  WgradItem it = grp.g[0];
#pragma unroll
  for (int i = 1; i < 8; ++i)
    if (d == i) it = grp.g[i];
  wgrad_tn_bf16_body<BN, BKW, MS, NS>(it.dY, it.lddy, it.X, it.ldx, it.dW, it.lddw, it.db, nullptr, it.M, it.N, it.K,
                                      it.tiles_k, it.tiles_nk, it.m_chunk, id - it.item0);
}

// db[n] += sum_m dY[m,n]: block = 64 lanes x 8 columns, 256 rows per block
__global__ __launch_bounds__(64) void colsum_bf16_kernel(const bf16* __restrict__ dY, int64_t lddy,
                                                         float* __restrict__ db, int M, int N) {
  const int c0 = (blockIdx.x * 64 + threadIdx.x) * 8;
  if (c0 >= N) return;
  const int m0 = blockIdx.y * 256, m1 = min(M, m0 + 256);
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int m = m0; m < m1; ++m) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(dY + (int64_t)m * lddy + c0);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (c0 + e < N) atomicAdd(db + c0 + e, s[e]);
}

// ------------------------------------------------------------------------------------------
// attention backward
// ------------------------------------------------------------------------------------------
struct BwdParams {
  const bf16* q; int64_t q_sb, q_sh, q_sl;
  const bf16* k; int64_t k_sb, k_sh, k_sl;
  const bf16* v; int64_t v_sb, v_sh, v_sl;
  const bf16* o; const bf16* dout; int64_t o_sb, o_sl;
  const float* lse; float* delta;
  bf16* dq; int64_t dq_sb, dq_sh, dq_sl;
  bf16* dk; int64_t dk_sb, dk_sh, dk_sl;
  bf16* dv; int64_t dv_sb, dv_sh, dv_sl;
  int mask_kind; int start_pos;
  const uint8_t* keypad; int64_t kp_sb;
  int B, h, hk, L, S;
  float scale;
  const float* cos_tab; const float* sin_tab; int rope_pos0;  // NULL: no RoPE backward fused
};

// ---- dq kernel: forward structure, no online softmax --------------------------------------
// K/V tiles of 64 keys run through a 3-deep LDS-DMA ring with counted vmcnt waits (as in the
// forward kernel); masks are per-lane bit words, P is recomputed as exp2(fma(s, c, -lse*log2e)).
__global__ __launch_bounds__(256, 3) void attn_bwd_dq_kernel(BwdParams p) {
  constexpr int DH = 64, RB = 128, NS = 3, KPW = 256;
  typedef AttnStage<RB, NS> Stage;
  constexpr int TILE = Stage::TILE;
  __shared__ __attribute__((aligned(16))) char smem[2 * NS * TILE + KPW * 8];  // K ring, V ring, key-padding words
  const AttnLane ln;
  const AttnQBlock blk(p, ln);
  const int wave = ln.wave, fr = ln.fr, fh = ln.fh;
  const int head = blk.head, b = blk.b, q0 = blk.q0, qi = blk.qi, qrow = blk.qrow;
  const bf16 *Q = blk.Q, *Kb = blk.Kb, *Vb = blk.Vb;
  const bf16* dO = p.dout + (int64_t)b * p.o_sb + (int64_t)qrow * p.o_sl + head * DH;
  bf16x8 qf[4], gf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    qf[ks] = *reinterpret_cast<const bf16x8*>(Q + ks * 16 + fh * 8);
    gf[ks] = *reinterpret_cast<const bf16x8*>(dO + ks * 16 + fh * 8);
  }
  const int64_t stat = ((int64_t)b * p.h + head) * p.L + qrow;
  const float c = p.scale * LOG2E;
  float neg_lse = -p.lse[stat] * LOG2E;  // p = exp2(c*s + neg_lse)
  // -delta = -sum_d dO*O of this lane's query row: the dO fragments are already here, O costs four
  // more 16-byte loads, the two lane halves (d 8fh..8fh+7 of every 16) are added by one exchange.
  // Written to the workspace for the dK/dV kernel, which is launched after this one.
  float neg_delta;
  {
    const bf16* Op = p.o + (int64_t)b * p.o_sb + (int64_t)qrow * p.o_sl + head * DH;
    float acc_ = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 of = *reinterpret_cast<const bf16x8*>(Op + ks * 16 + fh * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc_ += (float)of[e] * (float)gf[ks][e];
    }
    acc_ += __shfl_xor(acc_, 32, 64);
    neg_delta = -acc_;
    if (fh == 0 && qi < p.L) p.delta[stat] = neg_delta;
  }
  const bool causal = p.mask_kind & VY_MASK_CAUSAL;
  const bool haskp = p.mask_kind & VY_MASK_KEYPAD;
  const uint8_t* kp = haskp ? p.keypad + (int64_t)b * p.kp_sb : nullptr;

  const Stage st_w(ln, SwDual{}, SwRows<RB>{});   // K: dual-use image; V: row reads only
  auto stage = [&](int tile, int buf) { st_w.issue(smem, wave, buf, tile * 64, p.S, Kb, p.k_sl, Vb, p.v_sl); };
  const int k_sw = dual_sw(fr), v_sw = SwRows<RB>::key(fr);
  unsigned k_lds[2][2];  // K^T fragment of d block n, rows t_row (+8), K ring buffer 0
  attn_tr_bases(k_lds, smem, ln);
  f32x16 dq[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[n][r] = 0.f;

  const int nt = blk.key_tiles(p, causal);
  const int wave_first = q0 + wave * 32, wave_last = wave_first + 31;
  unsigned long long* kpbits = reinterpret_cast<unsigned long long*>(smem + 2 * NS * TILE);
  if (haskp) attn_keypad_words(kpbits, kp, nt, p.S, ln);

  auto compute = [&](int tile, int buf) {
    const int k0 = tile * 64;
    if (causal && k0 > p.start_pos + wave_last) return;
    const char* kb_ = smem + buf * TILE;
    const char* vb_ = smem + (NS + buf) * TILE;
    unsigned long long vis = ~0ull;
    if (haskp) vis = kpbits[tile];
    const bool need_mask = (k0 + 64 > p.S) || (causal && k0 + 63 > p.start_pos + wave_first) || vis != ~0ull;
    const unsigned long long lm = need_mask ? attn_key_bits(k0, fh, p.S, causal, qi + p.start_pos, vis) : ~0ull;
    const unsigned lmw[2] = {(unsigned)lm, (unsigned)(lm >> 32)};
    // one 32-key block at a time: scores and dP of a block are turned into dS (8 registers) before the next block's
    // accumulators exist -- both blocks' st / dp tiles live at once cost 32 more registers, the difference between two
    // and three waves per SIMD
    bf16x8 ds[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x16 st, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = neg_delta; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kb_ + (32 * kb + fr) * RB + (((2 * ks + fh) ^ k_sw) << 4));
        const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vb_ + (32 * kb + fr) * RB + (((2 * ks + fh) ^ v_sw) << 4));
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], st, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, gf[ks], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) ds[kb][r >> 3][r & 7] = (bf16)(attn_p<true>(st[r], c, neg_lse, lmw[kb], r) * dp[r]);
    }
    // dQ^T[d][q] += K^T[d][key] . dS^T[key][q]; K^T fragments by asm transposing reads, one ahead.
    // Base addresses per (d block, row / row+8); key block and k-step go into the offset field.
    unsigned kbase[2][2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int u = 0; u < 2; ++u) kbase[n][u] = k_lds[n][u] + buf * TILE;
    auto kfrag = [&](auto f_c) {
      constexpr int f = decltype(f_c)::value;
      return attn_tr_frag<(32 * ((f >> 1) & 1) + 16 * (f & 1)) * RB>(kbase[f >> 2]);
    };
    bf16x8 kfr[2];
    kfr[0] = kfrag(std::integral_constant<int, 0>{});
    auto step = [&](auto f_c) {
      constexpr int f = decltype(f_c)::value;
      if constexpr (f + 1 < 8) {
        kfr[(f + 1) & 1] = kfrag(std::integral_constant<int, f + 1>{});
        vy_lgkm_wait<2>(kfr[f & 1]);
      } else {
        vy_lgkm_wait<0>(kfr[f & 1]);
      }
      dq[f >> 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[f & 1], ds[(f >> 1) & 1][f & 1], dq[f >> 2], 0, 0, 0);
    };
    vy_static_for<8>(step);
  };

  typedef AttnRing<NS, Stage::DMA> Ring;
#pragma unroll
  for (int s_ = 0; s_ < Ring::AHEAD; ++s_)
    if (s_ < nt) stage(s_, s_);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) { vy_tie(qf[ks]); vy_tie(gf[ks]); }   // retire the ordinary loads
  vy_tie(neg_lse); vy_tie(neg_delta);
  for (int t = 0; t < nt; ++t) {
    Ring::arrive(t, nt);
    if (t + Ring::AHEAD < nt) stage(t + Ring::AHEAD, (t + Ring::AHEAD) % NS);
    compute(t, t % NS);
  }
  if (qi < p.L) {
    bf16* D = p.dq + (int64_t)b * p.dq_sb + (int64_t)head * p.dq_sh + (int64_t)qi * p.dq_sl;
    attn_store_scaled_rope(D, dq, p.scale, p.cos_tab, p.sin_tab, (int64_t)p.rope_pos0 + qi, fh);
  }
}

// ---- dk/dv kernel ----------------------------------------------------------------------------
// workgroup = 128 keys of one (batch, kv head); wave w owns keys [k0+32w, +32) and keeps dK^T and
// dV^T for them in registers while the workgroup sweeps (query head of the group) x (64-row query
// tile).  Q and dO tiles are staged by LDS-DMA into dual-use images (row + transposed reads)
// through a 3-deep ring; the tile's row statistics (lse, -delta) ride along as one 4-byte-per-lane
// LDS-DMA per wave, so the loop holds no ordinary load and is paced by counted vmcnt waits only.
__global__ __launch_bounds__(256, 2) void attn_bwd_dkdv_kernel(BwdParams p) {
  constexpr int DH = 64, RB = 128, QR = 64, NS = 3;
  typedef AttnStage<RB, NS> Stage;
  constexpr int QT = Stage::TILE;                                  // one 64-row tile = 8 KiB
  constexpr int ST_OFF = 2 * NS * QT;                              // NS x [lse 64 floats][-delta 64 floats]
  __shared__ __attribute__((aligned(16))) char smem[2 * NS * QT + NS * 512];
  const AttnLane ln;
  const int lane = ln.lane, wave = ln.wave, fr = ln.fr, fh = ln.fh;
  // grid (hk*B, key blocks): key block 0 sees every query row under a causal mask -> all of them first
  const int kblk = blockIdx.y, kvh = (int)blockIdx.x % p.hk, b = (int)blockIdx.x / p.hk;
  const int n_rep = p.h / p.hk;
  const int key0 = kblk * 128 + wave * 32;
  const int kj = key0 + fr;                       // this lane's key (column of S)
  const int krow = kj < p.S ? kj : p.S - 1;
  const bf16* Kp = p.k + (int64_t)b * p.k_sb + (int64_t)kvh * p.k_sh + (int64_t)krow * p.k_sl;
  const bf16* Vp = p.v + (int64_t)b * p.v_sb + (int64_t)kvh * p.v_sh + (int64_t)krow * p.v_sl;
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    kf[ks] = *reinterpret_cast<const bf16x8*>(Kp + ks * 16 + fh * 8);
    vf[ks] = *reinterpret_cast<const bf16x8*>(Vp + ks * 16 + fh * 8);
  }
  const bool causal = p.mask_kind & VY_MASK_CAUSAL;
  const bool haskp = p.mask_kind & VY_MASK_KEYPAD;
  const bool key_dead = (kj >= p.S) || (haskp && !p.keypad[(int64_t)b * p.kp_sb + krow]);
  const bool any_dead = __any(key_dead);
  const float c = p.scale * LOG2E;

  f32x16 dk[2], dv[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[n][r] = 0.f; dv[n][r] = 0.f; }

  // query tiles that can see any key of this block: rows >= block_first_key - start_pos
  const int nqt = (p.L + QR - 1) / QR;
  int qt_first = 0;
  if (causal) {
    const int first_row = kblk * 128 - p.start_pos;
    qt_first = first_row > 0 ? first_row / QR : 0;
  }
  const int per_head = nqt > qt_first ? nqt - qt_first : 0;
  const int total = per_head * n_rep;

  const Stage st_w(ln, SwDual{}, SwDual{});   // Q and dO: dual-use images
  const float* stat_src = (wave & 1) ? p.delta : p.lse;
  auto stage = [&](int it, int buf) {
    const int hh = it / per_head, qt = qt_first + (it - hh * per_head);
    const int head = kvh * n_rep + hh;
    st_w.issue(smem, wave, buf, qt * QR, p.L, p.q + (int64_t)b * p.q_sb + (int64_t)head * p.q_sh, p.q_sl,
               p.dout + (int64_t)b * p.o_sb + head * DH, p.o_sl);
    // row statistics: even waves bring lse, odd waves -delta (both pairs write the same bytes)
    int sr = qt * QR + lane;
    sr = sr < p.L ? sr : p.L - 1;
    __builtin_amdgcn_global_load_lds((const VY_GLOBAL void*)(stat_src + ((int64_t)b * p.h + head) * p.L + sr),
                                     (VY_LDS void*)(smem + ST_OFF + buf * 512 + (wave & 1) * 256), 4, 0, 0);
  };
  const int r_sw = dual_sw(fr);
  unsigned t_lds[2][2];  // transposed fragment of d block n, rows t_row (+8), ring buffer 0
  attn_tr_bases(t_lds, smem, ln);
  auto compute = [&](int it, int buf) {
    const int hh = it / per_head, qt = qt_first + (it - hh * per_head);
    const char* qb_ = smem + buf * QT;
    const char* gb_ = smem + (NS + buf) * QT;
    const float* stl = reinterpret_cast<const float*>(smem + ST_OFF + buf * 512);
    unsigned qbase_[2][2], gbase[2][2];  // transposed-read bases of this buffer (Q ring / dO ring)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        qbase_[n][u] = t_lds[n][u] + buf * QT;
        gbase[n][u] = t_lds[n][u] + (NS + buf) * QT;
      }
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int qbase = qt * QR + 32 * blk;
      // wave-uniform skips: block beyond L, or every key of this wave above the block's last diagonal
      if (qbase >= p.L || (causal && key0 > qbase + 31 + p.start_pos)) continue;
      // register r <-> query row qbase + (r&3) + 8(r>>2) + 4fh: row constants straight from LDS
      f32x16 st, dp, nl;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(stl + 32 * blk + 8 * rg + 4 * fh);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(stl + 64 + 32 * blk + 8 * rg + 4 * fh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          st[4 * rg + e] = 0.f;
          nl[4 * rg + e] = l4[e] * -LOG2E;
          dp[4 * rg + e] = d4[e];
        }
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 qa = *reinterpret_cast<const bf16x8*>(qb_ + (32 * blk + fr) * RB + (((2 * ks + fh) ^ r_sw) << 4));
        const bf16x8 ga = *reinterpret_cast<const bf16x8*>(gb_ + (32 * blk + fr) * RB + (((2 * ks + fh) ^ r_sw) << 4));
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], st, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga, vf[ks], dp, 0, 0, 0);
      }
      const bool need_mask = any_dead || qbase + 32 > p.L || (causal && key0 + 31 > qbase + p.start_pos);
      bf16x8 pf[2], dsf[2];
      if (need_mask) {
        // rows of this block the lane's key may see: [kj - start_pos - qbase, L - qbase)
        unsigned rm = (unsigned)range_bits64(causal ? kj - p.start_pos - qbase : 0, min(32, p.L - qbase));
        rm = key_dead ? 0u : rm >> (4 * fh);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pr = attn_p<true>(st[r], c, nl[r], rm, r);
          pf[r >> 3][r & 7] = (bf16)pr;
          dsf[r >> 3][r & 7] = (bf16)(pr * dp[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pr = attn_p<false>(st[r], c, nl[r], 0u, r);
          pf[r >> 3][r & 7] = (bf16)pr;
          dsf[r >> 3][r & 7] = (bf16)(pr * dp[r]);
        }
      }
      // dV^T[d][key] += dO^T[d][q] . P[q][key];   dK^T[d][key] += Q^T[d][q] . dS[q][key]
      auto frag = [&](auto f_c, const unsigned (&base)[2][2]) {
        constexpr int f = decltype(f_c)::value;
        return attn_tr_frag<16 * (f & 1) * RB>(base[f >> 1], 32 * blk * RB);
      };
      bf16x8 gfr[2], qfr[2];
      gfr[0] = frag(std::integral_constant<int, 0>{}, gbase);
      qfr[0] = frag(std::integral_constant<int, 0>{}, qbase_);
      auto step = [&](auto f_c) {
        constexpr int f = decltype(f_c)::value;
        if constexpr (f + 1 < 4) {
          gfr[(f + 1) & 1] = frag(std::integral_constant<int, f + 1>{}, gbase);
          qfr[(f + 1) & 1] = frag(std::integral_constant<int, f + 1>{}, qbase_);
          vy_lgkm_wait<4>(gfr[f & 1], qfr[f & 1]);
        } else {
          vy_lgkm_wait<0>(gfr[f & 1], qfr[f & 1]);
        }
        dv[f >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gfr[f & 1], pf[f & 1], dv[f >> 1], 0, 0, 0);
        dk[f >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[f & 1], dsf[f & 1], dk[f >> 1], 0, 0, 0);
      };
      vy_static_for<4>(step);
    }
  };

  typedef AttnRing<NS, Stage::DMA + 1> Ring;   // + the statistics rider
#pragma unroll
  for (int s_ = 0; s_ < Ring::AHEAD; ++s_)
    if (s_ < total) stage(s_, s_);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) { vy_tie(kf[ks]); vy_tie(vf[ks]); }   // retire the ordinary loads
  for (int it = 0; it < total; ++it) {
    Ring::arrive(it, total);
    if (it + Ring::AHEAD < total) stage(it + Ring::AHEAD, (it + Ring::AHEAD) % NS);
    compute(it, it % NS);
  }
  if (kj < p.S) {
    bf16* DK = p.dk + (int64_t)b * p.dk_sb + (int64_t)kvh * p.dk_sh + (int64_t)kj * p.dk_sl;
    bf16* DV = p.dv + (int64_t)b * p.dv_sb + (int64_t)kvh * p.dv_sh + (int64_t)kj * p.dv_sl;
    attn_store_scaled_rope(DK, dk, p.scale, p.cos_tab, p.sin_tab, (int64_t)p.rope_pos0 + kj, fh);
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      bf16x4 vl, vh;
#pragma unroll
      for (int e = 0; e < 4; ++e) { vl[e] = (bf16)dv[0][4 * rg + e]; vh[e] = (bf16)dv[1][4 * rg + e]; }
      *reinterpret_cast<bf16x4*>(DV + 8 * rg + 4 * fh) = vl;
      *reinterpret_cast<bf16x4*>(DV + 32 + 8 * rg + 4 * fh) = vh;
    }
  }
}

// ------------------------------------------------------------------------------------------
// fp32 weight gradient (the 1e-5 parity path trains too): dW[n][k] += alpha * sum_m dY[m][n] X[m][k], plain FMAs --
// 64 x 64 output tile per workgroup, 4 x 4 per thread, rows in steps of 16 through LDS, M split over workgroups that
// add into dW with fp32 atomics (dW is zeroed first when beta = 0).  The bias gradient is the column sum of the same
// dY tiles, taken by the k-tile-0 workgroups while they stage them.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wgrad_tn_f32_kernel(const float* __restrict__ dY, int64_t lddy,
                                                           const float* __restrict__ X, int64_t ldx, float* dW, int64_t lddw,
                                                           float* db, const float* alpha_dev, int M, int N, int K, int tiles_k,
                                                           int tiles, int m_chunk) {
  __shared__ float sy[16][64], sx[16][64];
  __shared__ float sb[4][64];
  const int tid = threadIdx.x;
  const int tile = (int)blockIdx.x % tiles, split = (int)blockIdx.x / tiles;
  const int n0 = (tile / tiles_k) * 64, k0 = (tile % tiles_k) * 64;
  const int m_begin = split * m_chunk, m_end = min(M, m_begin + m_chunk);
  const int tx = tid & 15, ty = tid >> 4;      // k / n micro-tile of the thread
  const int lc = tid & 63, lr = tid >> 6;      // staging: column, row group
  float acc[4][4] = {};
  float colsum = 0.f;
  for (int m0 = m_begin; m0 < m_end; m0 += 16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * i + lr, m = m0 + r;
      const bool ok = m < m_end;
      const float yv = ok && n0 + lc < N ? dY[(int64_t)m * lddy + n0 + lc] : 0.f;
      sy[r][lc] = yv;
      colsum += yv;
      sx[r][lc] = ok && k0 + lc < K ? X[(int64_t)m * ldx + k0 + lc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&sy[kk][4 * ty]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&sx[kk][4 * tx]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  const float alpha = alpha_dev ? *alpha_dev : 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + 4 * ty + i;
    if (n >= N) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + 4 * tx + j;
      if (k < K) atomicAdd(dW + (int64_t)n * lddw + k, alpha * acc[i][j]);
    }
  }
  if (db && k0 == 0) {
    sb[lr][lc] = colsum;
    __syncthreads();
    if (tid < 64 && n0 + tid < N) atomicAdd(db + n0 + tid, alpha * (sb[0][tid] + sb[1][tid] + sb[2][tid] + sb[3][tid]));
  }
}

int wgrad_f32(const char* who, const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, float* db,
              float beta, const float* alpha_dev, int64_t M, int64_t N, int64_t K, hipStream_t st) {
  if (beta == 0.f) {
    if (hipMemset2DAsync(dw, lddw * sizeof(float), 0, K * sizeof(float), N, st) != hipSuccess)
      VY_FAIL(VY_ERR_LAUNCH, "%s: memset failed", who);
    if (db && hipMemsetAsync(db, 0, N * sizeof(float), st) != hipSuccess) VY_FAIL(VY_ERR_LAUNCH, "%s: memset failed", who);
  }
  const int tiles_k = (int)vy_cdiv(K, 64), tiles = (int)vy_cdiv(N, 64) * tiles_k;
  int64_t splits = vy_cdiv(1024, tiles);
  const int64_t max_splits = vy_cdiv(M, 64);
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  const int64_t m_chunk = vy_cdiv(vy_cdiv(M, splits), 16) * 16;
  splits = vy_cdiv(M, m_chunk);
  hipLaunchKernelGGL(wgrad_tn_f32_kernel, dim3((unsigned)(tiles * splits)), dim3(256), 0, st, (const float*)dy, lddy,
                     (const float*)x, ldx, dw, lddw, db, alpha_dev, (int)M, (int)N, (int)K, tiles_k, tiles, (int)m_chunk);
  VY_CHECK_LAUNCH(who);
  return VY_OK;
}

// bf16 operands: N may be odd (vocabulary) as long as every dY row is readable up to the next multiple of 8
bool wgrad_bf16_operands_ok(const void* dy, int64_t lddy, const void* x, int64_t ldx, int64_t N, int64_t K) {
  return !(K % 8 || lddy % 8 || ldx % 8 || lddy < vy_cdiv(N, 8) * 8 || (uintptr_t)dy % 16 || (uintptr_t)x % 16);
}

// M rows in `want` chunks of whole 64-row blocks, none shorter than 256 rows (>= 4 stages of 64 rows) unless M is
struct WgradSplit { int64_t splits, m_chunk; };
WgradSplit wgrad_split(int64_t M, int64_t want) {
  const int64_t max_splits = vy_cdiv(M, 256);
  if (want > max_splits) want = max_splits;
  if (want < 1) want = 1;
  const int64_t m_chunk = vy_cdiv(vy_cdiv(M, want), 64) * 64;
  return {vy_cdiv(M, m_chunk), m_chunk};
}

}  // namespace

// ---- how much AdamW rides in a grouped launch (the one statement of the rule) --------------------------------
// budget = idle CUs x what one CU streams x how long the longest weight-gradient workgroup runs.
// ADAMW_RIDE_CU_BYTES_PER_US: one rider workgroup per CU, 40 workgroups on an otherwise idle chip stream 18.6 GB/s each
// (tools/bench_adamw_ride.py, DESIGN section 3 "AdamW in the grouped launch"); beside the tiles they share L2 and HBM with
// the tiles' loads, and the grouped kernel already grows at 16, so 16 it is.  ADAMW_RIDE_ITEM_US: wgrad_tn_bf16_grouped_kernel<256,256,32,4> at the
// benchmark layer (108 tiles x 2 M-splits, 8192 rows per workgroup) takes 276 us (profiles/r04_train_step_kernel_stats.csv);
// every workgroup is a 256 x 256 tile, so its time scales with its rows.
constexpr double ADAMW_RIDE_CU_BYTES_PER_US = 16000.0;
constexpr double ADAMW_RIDE_ITEM_US = 276.0;
constexpr int64_t ADAMW_RIDE_ITEM_ROWS = 8192;
constexpr int ADAMW_RIDE_MIN_IDLE_CUS = 8;
constexpr int VY_CUS = 256;

// bytes a launch of `items` weight-gradient workgroups of at most `rows` rows may carry (items = 0: no limit, nothing to slow down)
static int64_t adamw_ride_budget(int64_t items, int64_t rows) {
  if (items == 0) return INT64_MAX;
  const int64_t idle = VY_CUS - items;
  if (idle < ADAMW_RIDE_MIN_IDLE_CUS) return 0;
  return (int64_t)((double)idle * ADAMW_RIDE_CU_BYTES_PER_US * ADAMW_RIDE_ITEM_US * (double)rows / (double)ADAMW_RIDE_ITEM_ROWS);
}

static bool ranges_meet(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  if (!a || !b || abytes <= 0 || bbytes <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// ---- how much rides behind the single-launch 256 x 256 weight gradient (vy_linear_wgrad_riders) ------------------
// The riders are dispatched behind ALL tile workgroups, so what they find idle is the last round's remainder:
// 256 - items % 256 CUs for one tile time (none when the last round is full).  The tile time is ADAMW_RIDE_ITEM_US
// scaled by the workgroup's rows, as above.  WGRAD_RIDE_CU_BYTES_PER_US: see DESIGN section 3 "Riders in the
// vocabulary weight gradient" (tools/bench_wgrad_riders.py).
constexpr double WGRAD_RIDE_CU_BYTES_PER_US = 12000.0;

static int64_t wgrad_ride_budget(int64_t items, int64_t rows) {
  const int64_t last = items % VY_CUS;
  if (last == 0) return 0;
  const int64_t idle = VY_CUS - last;
  if (idle < ADAMW_RIDE_MIN_IDLE_CUS) return 0;
  return (int64_t)((double)idle * WGRAD_RIDE_CU_BYTES_PER_US * ADAMW_RIDE_ITEM_US * (double)rows / (double)ADAMW_RIDE_ITEM_ROWS);
}

// vy_linear_wgrad and vy_linear_wgrad_riders.  The riders (zero / ntr / tr_taken all optional) are carried by the `big`
// bf16 branch only, as far as wgrad_ride_budget goes: the leading transposing tiles of the table, then the zero ranges in
// order, a range that does not fit whole gives its leading chunks.  Every other path carries nothing and reports 0.
static int linear_wgrad_impl(const char* who, const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw,
                             int64_t lddw, float* db, float beta, const float* alpha_dev, int64_t M, int64_t N, int64_t K,
                             int dtype, vy_zero_ride_desc* zero, int32_t nzero, const vy_transpose_desc* tr_dev,
                             int32_t tr_n, int32_t tr_total, int32_t* tr_taken, void* stream) {
  for (int i = 0; i < nzero; ++i) zero[i].taken = 0;
  if (tr_taken) *tr_taken = 0;
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "%s: bad dtype %d", who, dtype);
  if (!dy || !x || !dw || M <= 0 || N <= 0 || K <= 0) VY_FAIL(VY_ERR_ARG, "%s: bad arguments", who);
  if (dtype == VY_F32) {
    if (beta != 0.f && beta != 1.f) VY_FAIL(VY_ERR_ARG, "%s: beta must be 0 or 1", who);
    return wgrad_f32(who, dy, lddy, x, ldx, dw, lddw, db, beta, alpha_dev, M, N, K, (hipStream_t)stream);
  }
  if (!wgrad_bf16_operands_ok(dy, lddy, x, ldx, N, K))
    VY_FAIL(VY_ERR_ARG, "%s: K and leading dimensions must be multiples of 8 (lddy >= roundup8(N)), operands 16-byte aligned", who);
  if (beta != 0.f && beta != 1.f) VY_FAIL(VY_ERR_ARG, "%s: beta must be 0 or 1", who);
  hipStream_t st = (hipStream_t)stream;
  if (beta == 0.f) {
    if (hipMemset2DAsync(dw, lddw * sizeof(float), 0, K * sizeof(float), N, st) != hipSuccess)
      VY_FAIL(VY_ERR_LAUNCH, "%s: memset failed", who);
    if (db && hipMemsetAsync(db, 0, N * sizeof(float), st) != hipSuccess)
      VY_FAIL(VY_ERR_LAUNCH, "%s: memset failed", who);
  }
  // default: tile 128(n) x 128(k), 4 waves, 2 stages = 64 KiB of LDS: TWO workgroups per CU, which hides the
  // load latency better than one 256 x 128 workgroup (8 waves, 96 KiB) or a deeper ring with one
  // workgroup per CU -- measured inside the training step: 256-wide 142/165 us vs 96/125 us (QKV /
  // FFN1), 3- and 4-stage rings +45 %; 32-row stages (three workgroups per CU) 6 % faster on the FFN shapes alone, no
  // difference inside the training step (that code is in the history).
  // The vocabulary projection (N = 50265: every tile reduces all M rows, so the 256 KiB atomic epilogue of a
  // 256 x 256 tile is paid once per 512 stages) takes the 256 x 256 tile, 32-row stages, 4-deep ring, one workgroup
  // per CU (7.8 instead of 15.6 LDS-DMA bytes per kFLOP): +9 %
  const bool big = N >= 8192 && M >= 4096;
  const int BT = big ? 256 : 128;
  const int tiles_k = (int)vy_cdiv(K, BT), tiles = (int)vy_cdiv(N, BT) * tiles_k;
  // 128 x 128: ~1.5 workgroups per CU; 256 x 256: at most one round of 256 workgroups
  const WgradSplit sp = wgrad_split(M, big ? 256 / tiles : vy_cdiv(384, tiles));
  const int64_t items = tiles * sp.splits;
  WgradRiders rd;
  memset(&rd, 0, sizeof(rd));
  rd.items = (int)items;
  int64_t riders = 0;
  if (big) {
    int64_t left = wgrad_ride_budget(items, sp.m_chunk);
    if (tr_dev && tr_n > 0 && tr_total > 0) {
      const int64_t tile_bytes = 2 * 64 * 64 * 2;   // read + written, bf16
      // with both tables present each may use half of the budget, and the zero ranges what the transposes leave of theirs
      const int64_t mine = nzero > 0 ? left / 2 : left;
      int64_t take = tr_total;
      if (mine / tile_bytes < take) take = mine / tile_bytes / WGRAD_RIDE_TR_TILES * WGRAD_RIDE_TR_TILES;
      if (take > 0) {
        rd.tr = tr_dev; rd.tr_n = tr_n; rd.tr_tiles = (int)take; rd.tr_blocks = (int)vy_cdiv(take, WGRAD_RIDE_TR_TILES);
        riders += rd.tr_blocks;
        left -= take * tile_bytes;
        if (tr_taken) *tr_taken = (int32_t)take;
      }
    }
    int64_t chunks = 0;
    for (int i = 0; i < nzero; ++i) {
      int64_t take = zero[i].n;
      if (left / 4 < take) take = left / 4 / WGRAD_RIDE_ZERO_CHUNK * WGRAD_RIDE_ZERO_CHUNK;
      if (take <= 0) break;
      ZeroRange& r = rd.z[rd.nz++];
      r.p = zero[i].p; r.n = take; r.blk0 = (int)chunks;
      chunks += vy_cdiv(take, WGRAD_RIDE_ZERO_CHUNK);
      zero[i].taken = take;
      left -= take * 4;
      if (take < zero[i].n) break;
    }
    for (int i = rd.nz; i < 8; ++i) rd.z[i] = rd.z[0];
    riders += chunks;
  }
  if (items + riders > INT32_MAX) VY_FAIL(VY_ERR_ARG, "%s: too many workgroups", who);
  auto kernel = big ? wgrad_tn_bf16_kernel<256, 256, 32, 4> : wgrad_tn_bf16_kernel<128, 128, 64, 2>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(items + riders)), dim3(BT * 2), 0, st, (const bf16*)dy, lddy, (const bf16*)x,
                     ldx, dw, lddw, db, alpha_dev, (int)M, (int)N, (int)K, tiles_k, tiles, (int)sp.m_chunk, rd);
  VY_CHECK_LAUNCH(who);
  return VY_OK;
}

extern "C" int vy_linear_wgrad(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw,
                               int64_t lddw, float* db, float beta, const float* alpha_dev, int64_t M,
                               int64_t N, int64_t K, int dtype, void* stream) {
  return linear_wgrad_impl("vy_linear_wgrad", dy, lddy, x, ldx, dw, lddw, db, beta, alpha_dev, M, N, K, dtype, nullptr, 0,
                           nullptr, 0, 0, nullptr, stream);
}

extern "C" int vy_linear_wgrad_riders(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw,
                                      float* db, float beta, const float* alpha_dev, int64_t M, int64_t N, int64_t K,
                                      int dtype, vy_zero_ride_desc* zero, int32_t nzero,
                                      const vy_transpose_desc* tr_descs_dev, int32_t tr_n, int32_t tr_total_tiles,
                                      int tr_dtype, int32_t* tr_taken, void* stream) {
  const char* who = "vy_linear_wgrad_riders";
  if (nzero < 0 || nzero > 8 || (nzero > 0 && !zero)) VY_FAIL(VY_ERR_ARG, "%s: 0..8 zero ranges", who);
  if (tr_n < 0 || tr_total_tiles < 0 || (tr_n > 0 && (!tr_descs_dev || tr_total_tiles <= 0)))
    VY_FAIL(VY_ERR_ARG, "%s: bad transpose table", who);
  if (!dy || !x || !dw || M <= 0 || N <= 0 || K <= 0) VY_FAIL(VY_ERR_ARG, "%s: bad arguments", who);
  const int64_t esz = dtype == VY_F32 ? 4 : 2;
  for (int i = 0; i < nzero; ++i) {
    const vy_zero_ride_desc& z = zero[i];
    if (!z.p || z.n <= 0) VY_FAIL(VY_ERR_ARG, "%s: zero range %d: bad arguments", who, i);
    if ((uintptr_t)z.p % 16) VY_FAIL(VY_ERR_ARG, "%s: zero range %d must be 16-byte aligned", who, i);
    // no data dependence on this launch: a rider writes nothing the tiles read or accumulate into
    if (ranges_meet(z.p, z.n * 4, dw, ((N - 1) * lddw + K) * 4) || ranges_meet(z.p, z.n * 4, db, N * 4) ||
        ranges_meet(z.p, z.n * 4, dy, ((M - 1) * lddy + N) * esz) || ranges_meet(z.p, z.n * 4, x, ((M - 1) * ldx + K) * esz))
      VY_FAIL(VY_ERR_ARG, "%s: zero range %d intersects an operand or a gradient of the same launch", who, i);
  }
  // (the transposes' destinations live in a device table: that they meet none of dw, db, dy, x is the caller's to guarantee)
  if (tr_n > 0 && tr_dtype != VY_BF16) { tr_descs_dev = nullptr; tr_n = 0; }   // the riders transpose bf16 only: nothing rides
  return linear_wgrad_impl(who, dy, lddy, x, ldx, dw, lddw, db, beta, alpha_dev, M, N, K, dtype, zero, nzero, tr_descs_dev,
                           tr_n, tr_total_tiles, tr_taken, stream);
}


static int wgrad_grouped(const char* who, const vy_wgrad_desc* descs, int32_t n, const vy_colsum_desc* cs, int32_t ncs,
                        vy_adamw_ride_desc* opt, int32_t nopt, const vy_adamw_hyper* hy, int dtype, void* stream) {
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "%s: bad dtype %d", who, dtype);
  if (nopt < 0 || nopt > 8 || (nopt > 0 && (!opt || !hy))) VY_FAIL(VY_ERR_ARG, "%s: 0..8 AdamW ranges (with their hyper-parameters)", who);
  if (n < 0 || n > 8 || (n > 0 && !descs) || ncs < 0 || ncs > 8 || (ncs > 0 && !cs) || n + ncs + nopt == 0)
    VY_FAIL(VY_ERR_ARG, "%s: 1..8 descriptors", who);
  for (int i = 0; i < ncs; ++i)
    if (!cs[i].ws || cs[i].W <= 0 || cs[i].N <= 0 || (cs[i].acc != 0 && cs[i].acc != 1))
      VY_FAIL(VY_ERR_ARG, "%s: column-sum descriptor %d: bad arguments", who, i);
  for (int i = 0; i < n; ++i) {
    const vy_wgrad_desc& d = descs[i];
    if (!d.dy || !d.x || !d.dw || d.M <= 0 || d.N <= 0 || d.K <= 0) VY_FAIL(VY_ERR_ARG, "%s: descriptor %d: bad arguments", who, i);
  }
  if (nopt > 0 && hy->step <= 0) VY_FAIL(VY_ERR_ARG, "%s: AdamW step must be >= 1", who);
  for (int i = 0; i < nopt; ++i) {
    const vy_adamw_ride_desc& o = opt[i];
    if (!o.p || !o.g || !o.m || !o.v || o.n <= 0) VY_FAIL(VY_ERR_ARG, "%s: AdamW range %d: bad arguments", who, i);
    if ((uintptr_t)o.p % 16 || (uintptr_t)o.g % 16 || (uintptr_t)o.m % 16 || (uintptr_t)o.v % 16 || (uintptr_t)o.p_bf16 % 8)
      VY_FAIL(VY_ERR_ARG, "%s: AdamW range %d: p, g, m, v must be 16-byte aligned (p_bf16: 8-byte)", who, i);
    // no data dependence on this launch: what a rider reads or the next forward reads from it is not written here
    const void* mine[3] = {o.g, o.p, o.p_bf16};
    const int64_t mine_bytes[3] = {o.n * 4, o.n * 4, o.n * 2};
    for (int k = 0; k < 3; ++k) {
      bool hit = false;
      for (int j = 0; j < n; ++j) {
        const vy_wgrad_desc& d = descs[j];
        hit = hit || ranges_meet(mine[k], mine_bytes[k], d.dw, ((d.N - 1) * d.lddw + d.K) * 4) ||
              ranges_meet(mine[k], mine_bytes[k], d.db, d.N * 4);
      }
      for (int j = 0; j < ncs; ++j) {
        const vy_colsum_desc& c = cs[j];
        hit = hit || ranges_meet(mine[k], mine_bytes[k], c.out0, (int64_t)c.N * 4) ||
              ranges_meet(mine[k], mine_bytes[k], c.out1, (int64_t)c.N * 4) ||
              ranges_meet(mine[k], mine_bytes[k], c.ws, 2 * (int64_t)c.W * c.N * 4);
      }
      if (hit) VY_FAIL(VY_ERR_ARG, "%s: AdamW range %d intersects a gradient or slab of the same launch", who, i);
    }
  }
  for (int i = 0; i < nopt; ++i) opt[i].taken = 0;
  if (dtype == VY_F32) {   // the parity path: one plain launch per descriptor
    for (int i = 0; i < nopt; ++i) {
      vy_adamw_ride_desc& o = opt[i];
      if (int rc = vy_adamw_step(o.p, o.g, o.m, o.v, o.p_bf16, o.n, hy->lr, hy->beta1, hy->beta2, hy->eps, hy->weight_decay,
                                 hy->step, hy->grad_scale, nullptr, stream)) return rc;
      o.taken = o.n;
    }
    for (int i = 0; i < ncs; ++i)
      if (int rc = vy_colsum("vy_layernorm_bwd", cs[i].ws, 2, (int64_t)cs[i].W * cs[i].N, cs[i].N, cs[i].W, cs[i].N,
                             vy_ln_colsum_slices(cs[i].W), cs[i].out0, cs[i].out1, cs[i].acc, (hipStream_t)stream)) return rc;
    for (int i = 0; i < n; ++i) {
      const vy_wgrad_desc& d = descs[i];
      if (!d.dy || !d.x || !d.dw || d.M <= 0 || d.N <= 0 || d.K <= 0) VY_FAIL(VY_ERR_ARG, "%s: descriptor %d: bad arguments", who, i);
      if (int rc = wgrad_f32(who, d.dy, d.lddy, d.x, d.ldx, d.dw, d.lddw, d.db, 1.f, nullptr, d.M, d.N, d.K, (hipStream_t)stream)) return rc;
    }
    return VY_OK;
  }
  int64_t tiles_total = 0;
  for (int i = 0; i < n; ++i) {
    const vy_wgrad_desc& d = descs[i];
    if (!d.dy || !d.x || !d.dw || d.M <= 0 || d.N <= 0 || d.K <= 0) VY_FAIL(VY_ERR_ARG, "%s: descriptor %d: bad arguments", who, i);
    if (!wgrad_bf16_operands_ok(d.dy, d.lddy, d.x, d.ldx, d.N, d.K))
      VY_FAIL(VY_ERR_ARG, "%s: descriptor %d: K and leading dimensions must be multiples of 8, operands 16-byte aligned", who, i);
    tiles_total += vy_cdiv(d.N, 256) * vy_cdiv(d.K, 256);
  }
  WgradGroup grp;
  memset(&grp, 0, sizeof(grp));   // (n == 0: column sums only)
  grp.n = n;
  int64_t items = 0, rows_max = 0;
  for (int i = 0; i < n; ++i) {
    const vy_wgrad_desc& d = descs[i];
    const int64_t tiles_k = vy_cdiv(d.K, 256), tiles = vy_cdiv(d.N, 256) * tiles_k;
    const WgradSplit sp = wgrad_split(d.M, 256 / tiles_total);   // at most one round of workgroups (the column sums do not count: they are short)
    rows_max = sp.m_chunk > rows_max ? sp.m_chunk : rows_max;
    WgradItem& it = grp.g[i];
    it.dY = (const bf16*)d.dy; it.X = (const bf16*)d.x; it.dW = d.dw; it.db = d.db;
    it.lddy = d.lddy; it.ldx = d.ldx; it.lddw = d.lddw;
    it.M = (int)d.M; it.N = (int)d.N; it.K = (int)d.K;
    it.tiles_k = (int)tiles_k; it.tiles_nk = (int)tiles; it.m_chunk = (int)sp.m_chunk; it.item0 = (int)items;
    items += tiles * sp.splits;
  }
  for (int i = n; i < 8; ++i) grp.g[i] = grp.g[0];
  ColsumGroup cg;
  memset(&cg, 0, sizeof(cg));
  cg.n = ncs; cg.items = (int)items;
  int64_t blocks = 0;
  for (int i = 0; i < ncs; ++i) {
    ColsumItem& c = cg.c[i];
    c.ws = cs[i].ws; c.out0 = cs[i].out0; c.out1 = cs[i].out1;
    c.W = cs[i].W; c.N = cs[i].N; c.acc = cs[i].acc;
    c.rps = (int)vy_cdiv(c.W, vy_ln_colsum_slices(c.W));
    c.blk0 = (int)blocks;
    blocks += vy_cdiv(c.N, 64);
  }
  // the AdamW ranges, in order, as far as the budget goes: a range that does not fit whole gives its leading chunks
  AdamwGroup og;
  memset(&og, 0, sizeof(og));
  int64_t chunks = 0;
  if (nopt > 0) {
    const float bc1 = 1.0f - powf(hy->beta1, (float)hy->step);   // (as vy_adamw_step computes them)
    const float bc2s = sqrtf(1.0f - powf(hy->beta2, (float)hy->step));
    og.s = {hy->lr, hy->beta1, hy->beta2, hy->eps, hy->weight_decay, bc1, bc2s, hy->grad_scale};
    int64_t left = adamw_ride_budget(items, rows_max);
    for (int i = 0; i < nopt && og.n < 8; ++i) {
      const vy_adamw_ride_desc& o = opt[i];
      const int64_t per = o.p_bf16 ? 30 : 28;   // bytes of traffic per element
      int64_t take = o.n;
      if (left / per < take) take = left / per / ADAMW_RIDE_CHUNK * ADAMW_RIDE_CHUNK;
      if (take <= 0) break;
      AdamwRange& r = og.r[og.n++];
      r.p = o.p; r.g = o.g; r.m = o.m; r.v = o.v; r.pb = (bf16*)o.p_bf16; r.n = take; r.blk0 = (int)chunks;
      chunks += vy_cdiv(take, ADAMW_RIDE_CHUNK);
      opt[i].taken = take;
      left -= take * per;
      if (take < o.n) break;
    }
    for (int i = og.n; i < 8; ++i) og.r[i] = og.r[0];
  }
  og.blk0 = (int)(items + blocks);
  if (items + blocks + chunks > INT32_MAX) VY_FAIL(VY_ERR_ARG, "%s: too many workgroups", who);
  if (items + blocks + chunks == 0) return VY_OK;   // (riders only and a budget of none cannot happen: n = 0 has no limit)
  hipLaunchKernelGGL((wgrad_tn_bf16_grouped_kernel<256, 256, 32, 4>), dim3((unsigned)(items + blocks + chunks)), dim3(512), 0,
                     (hipStream_t)stream, grp, cg, og);
  VY_CHECK_LAUNCH(who);
  return VY_OK;
}

extern "C" int vy_linear_wgrad_grouped(const vy_wgrad_desc* descs, int32_t n, int dtype, void* stream) {
  if (!descs || n <= 0 || n > 8) VY_FAIL(VY_ERR_ARG, "vy_linear_wgrad_grouped: 1..8 descriptors");
  return wgrad_grouped("vy_linear_wgrad_grouped", descs, n, nullptr, 0, nullptr, 0, nullptr, dtype, stream);
}

extern "C" int vy_linear_wgrad_grouped_cs(const vy_wgrad_desc* descs, int32_t n, const vy_colsum_desc* cs, int32_t ncs,
                                          int dtype, void* stream) {
  return wgrad_grouped("vy_linear_wgrad_grouped_cs", descs, n, cs, ncs, nullptr, 0, nullptr, dtype, stream);
}

extern "C" int vy_linear_wgrad_grouped_opt(const vy_wgrad_desc* descs, int32_t n, const vy_colsum_desc* cs, int32_t ncs,
                                           vy_adamw_ride_desc* opt, int32_t nopt, const vy_adamw_hyper* hyper, int dtype,
                                           void* stream) {
  return wgrad_grouped("vy_linear_wgrad_grouped_opt", descs, n, cs, ncs, opt, nopt, hyper, dtype, stream);
}

// ------------------------------------------------------------------------------------------
// Attention backward for the other head widths (any multiple of 8 up to 256; 72 runs as 96): the structure of
// attn_fwd_gen_kernel (vy_attn.hip) -- register-staged 64-row tiles in LDS, mfma_f32_16x16x32_bf16, a lane owns one
// row of the "B side" and 4 consecutive rows of the "A side" per 16 x 16 block, products that feed the next MFMA stay
// in registers with the contraction walked in the order the values sit in, transposed operands by
// ds_read_b64_tr_b16.  Not tuned like the dh = 64 kernels: it exists so that models with 72 / 128 / 256-wide heads
// train on the MFMA path at all.
//   dq kernel   (64 query rows per workgroup, keys swept):  S^T = K Q^T, dP^T = V dO^T (accumulator initialised with
//               -delta), dS^T = P o (dP - delta), dQ^T += K^T dS^T;  delta = rowsum(dO o O) computed here and left in
//               delta_ws for the second kernel
//   dkdv kernel (64 keys per workgroup, query heads of the KV group and query rows swept):  S = Q K^T, dP = dO V^T,
//               dV^T += dO^T P, dK^T += Q^T dS
// Rows without a visible key contribute nothing (as in the dh = 64 kernels).
// ------------------------------------------------------------------------------------------
namespace {

template <int DHP>
struct GenBwd {
  static constexpr int PITCH = (DHP + 8) * 2, KS = DHP / 32, NDB = DHP / 16, CPRW = DHP / 8, CPT = 64 * CPRW / 256;
};

__device__ __forceinline__ float gen_groups_sum(float v) {   // over the four 16-lane groups, result in every lane
  const unsigned u = __builtin_bit_cast(unsigned, v);
  auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = __builtin_bit_cast(float, (unsigned)s16[0]) + __builtin_bit_cast(float, (unsigned)s16[1]);
  const unsigned w = __builtin_bit_cast(unsigned, v);
  auto s32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __builtin_bit_cast(float, (unsigned)s32[0]) + __builtin_bit_cast(float, (unsigned)s32[1]);
}

// stage a 64-row tile of a [rows][dh] tensor (row stride `sl` elements) into LDS, zero beyond dh / beyond `nrows`
template <int DHP>
__device__ __forceinline__ void gen_stage(char* dst, const bf16* src, int64_t sl, int row0, int nrows, int dh, int tid,
                                          bf16x8 (&reg)[GenBwd<DHP>::CPT]) {
  (void)dst;
  constexpr int CPRW = GenBwd<DHP>::CPRW, CPT = GenBwd<DHP>::CPT;
  const bf16x8 zero8 = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int cidx = tid + 256 * i;
    const int row = cidx / CPRW, ch = cidx - row * CPRW;
    const int r = row0 + row;
    const bool ok = ch * 8 < dh && r < nrows;
    reg[i] = ok ? *reinterpret_cast<const bf16x8*>(src + (int64_t)r * sl + ch * 8) : zero8;
  }
}
template <int DHP>
__device__ __forceinline__ void gen_store(char* dst, int tid, const bf16x8 (&reg)[GenBwd<DHP>::CPT]) {
  constexpr int CPRW = GenBwd<DHP>::CPRW, CPT = GenBwd<DHP>::CPT, PITCH = GenBwd<DHP>::PITCH;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int cidx = tid + 256 * i;
    const int row = cidx / CPRW, ch = cidx - row * CPRW;
    *reinterpret_cast<bf16x8*>(dst + row * PITCH + ch * 16) = reg[i];
  }
}

template <int DHP>
__global__ __launch_bounds__(256) void attn_bwd_gen_dq_kernel(BwdParams p, int dh) {
  typedef GenBwd<DHP> G;
  constexpr int PITCH = G::PITCH, KS = G::KS, NDB = G::NDB, CPT = G::CPT;
  __shared__ __attribute__((aligned(16))) char smem[2 * 64 * PITCH];
  char* kt = smem;
  char* vt = smem + 64 * PITCH;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  // heads on x, long rows first (see attn_fwd_gen_kernel)
  const int head = (int)blockIdx.x % p.h, b = (int)blockIdx.x / p.h;
  const int kvh = head / (p.h / p.hk);
  const int q0 = ((int)gridDim.y - 1 - (int)blockIdx.y) * 64;
  const int qi = q0 + wave * 16 + r16;
  const int qrow = qi < p.L ? qi : p.L - 1;
  const bf16* Q = p.q + (int64_t)b * p.q_sb + (int64_t)head * p.q_sh + (int64_t)qrow * p.q_sl;
  const bf16* dO = p.dout + (int64_t)b * p.o_sb + (int64_t)qrow * p.o_sl + head * dh;
  const bf16* Op = p.o + (int64_t)b * p.o_sb + (int64_t)qrow * p.o_sl + head * dh;
  const bf16* Kb = p.k + (int64_t)b * p.k_sb + (int64_t)kvh * p.k_sh;
  const bf16* Vb = p.v + (int64_t)b * p.v_sb + (int64_t)kvh * p.v_sh;
  const bool causal = p.mask_kind & VY_MASK_CAUSAL;
  const bool haskp = p.mask_kind & VY_MASK_KEYPAD;
  const uint8_t* kp = haskp ? p.keypad + (int64_t)b * p.kp_sb : nullptr;
  const bf16x8 zero8 = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
  bf16x8 qf[KS], gf[KS];
  float dacc = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d0 = 32 * ks + 8 * kq;
    qf[ks] = d0 < dh ? *reinterpret_cast<const bf16x8*>(Q + d0) : zero8;
    gf[ks] = d0 < dh ? *reinterpret_cast<const bf16x8*>(dO + d0) : zero8;
    const bf16x8 of = d0 < dh ? *reinterpret_cast<const bf16x8*>(Op + d0) : zero8;
#pragma unroll
    for (int e = 0; e < 8; ++e) dacc += (float)of[e] * (float)gf[ks][e];
  }
  const float neg_delta = -gen_groups_sum(dacc);
  const int64_t stat = ((int64_t)b * p.h + head) * p.L + qrow;
  if (kq == 0 && qi < p.L) p.delta[stat] = neg_delta;
  const float c = p.scale * LOG2E;
  const float neg_lse = -p.lse[stat] * LOG2E;
  f32x4 dq[NDB];
#pragma unroll
  for (int n = 0; n < NDB; ++n) dq[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  int nt = (p.S + 63) / 64;
  if (causal) nt = max(1, min(nt, (min(p.S, p.start_pos + q0 + 64) + 63) / 64));
  const unsigned ktr = vy_lds_addr(kt) + (4 * kq + (r16 >> 2)) * PITCH + (4 * (r16 & 3)) * 2;
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * 64;
    bf16x8 kreg[CPT], vreg[CPT];
    gen_stage<DHP>(kt, Kb, p.k_sl, k0, p.S, dh, tid, kreg);
    gen_stage<DHP>(vt, Vb, p.v_sl, k0, p.S, dh, tid, vreg);
    __syncthreads();
    gen_store<DHP>(kt, tid, kreg);
    gen_store<DHP>(vt, tid, vreg);
    __syncthreads();
    f32x4 ds[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {neg_delta, neg_delta, neg_delta, neg_delta};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kt + (16 * blk + r16) * PITCH + (32 * ks + 8 * kq) * 2);
        const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vt + (16 * blk + r16) * PITCH + (32 * ks + 8 * kq) * 2);
        sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, gf[ks], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kj = k0 + 16 * blk + 4 * kq + r;
        bool vis = kj < p.S && qi < p.L;
        if (causal) vis = vis && kj <= qi + p.start_pos;
        if (haskp) vis = vis && kp[kj < p.S ? kj : 0] != 0;
        const float pr = vis ? __builtin_amdgcn_exp2f(fmaf(sc[r], c, neg_lse)) : 0.f;
        ds[blk][r] = pr * dp[r];
      }
    }
    // dQ^T += K^T dS^T: k-steps of 32 keys = blocks (2 tt, 2 tt + 1) in the order the values sit in
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      bf16x8 sf;
#pragma unroll
      for (int r = 0; r < 4; ++r) { sf[r] = (bf16)ds[2 * tt][r]; sf[4 + r] = (bf16)ds[2 * tt + 1][r]; }
      vy_static_for<NDB>([&](auto n_c) {
        constexpr int n = decltype(n_c)::value;
        union { struct { s16x4 a, b; } h; bf16x8 v; } u;
        u.h.a = vy_lds_tr16_off<n * 32>(ktr + (32 * tt) * PITCH);
        u.h.b = vy_lds_tr16_off<n * 32>(ktr + (32 * tt + 16) * PITCH);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        vy_tie(u.v);
        dq[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(u.v, sf, dq[n], 0, 0, 0);
      });
    }
  }
  if (qi < p.L) {
    bf16* D = p.dq + (int64_t)b * p.dq_sb + (int64_t)head * p.dq_sh + (int64_t)qi * p.dq_sl;
#pragma unroll
    for (int n = 0; n < NDB; ++n) {
      const int d0 = 16 * n + 4 * kq;
      if (d0 < dh) {
        bf16x4 w;
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = (bf16)(dq[n][r] * p.scale);
        *reinterpret_cast<bf16x4*>(D + d0) = w;
      }
    }
  }
}

template <int DHP>
__global__ __launch_bounds__(256) void attn_bwd_gen_dkdv_kernel(BwdParams p, int dh) {
  typedef GenBwd<DHP> G;
  constexpr int PITCH = G::PITCH, KS = G::KS, NDB = G::NDB, CPT = G::CPT;
  __shared__ __attribute__((aligned(16))) char smem[2 * 64 * PITCH + 2 * 64 * 4];
  char* qt = smem;
  char* gt = smem + 64 * PITCH;
  float* lse_s = reinterpret_cast<float*>(smem + 2 * 64 * PITCH);   // -lse * log2e of the tile's query rows
  float* del_s = lse_s + 64;                                          // -delta
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int kvh = (int)blockIdx.x % p.hk, b = (int)blockIdx.x / p.hk;   // KV heads on x; the first key tiles see the most rows
  const int nrep = p.h / p.hk;
  const int k0 = (int)blockIdx.y * 64;
  const int kj = k0 + wave * 16 + r16;
  const int krow = kj < p.S ? kj : p.S - 1;
  const bf16* Kp = p.k + (int64_t)b * p.k_sb + (int64_t)kvh * p.k_sh + (int64_t)krow * p.k_sl;
  const bf16* Vp = p.v + (int64_t)b * p.v_sb + (int64_t)kvh * p.v_sh + (int64_t)krow * p.v_sl;
  const bool causal = p.mask_kind & VY_MASK_CAUSAL;
  const bool haskp = p.mask_kind & VY_MASK_KEYPAD;
  const bool key_vis = kj < p.S && (!haskp || p.keypad[(int64_t)b * p.kp_sb + krow] != 0);
  const bf16x8 zero8 = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
  bf16x8 kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d0 = 32 * ks + 8 * kq;
    kf[ks] = d0 < dh ? *reinterpret_cast<const bf16x8*>(Kp + d0) : zero8;
    vf[ks] = d0 < dh ? *reinterpret_cast<const bf16x8*>(Vp + d0) : zero8;
  }
  f32x4 dk[NDB], dv[NDB];
#pragma unroll
  for (int n = 0; n < NDB; ++n) { dk[n] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[n] = dk[n]; }
  const float c = p.scale * LOG2E;
  // query rows that can see a key of this tile: causal => q + start_pos >= k0
  const int qstart = causal ? max(0, k0 - p.start_pos) & ~63 : 0;
  const unsigned qtr = vy_lds_addr(qt) + (4 * kq + (r16 >> 2)) * PITCH + (4 * (r16 & 3)) * 2;
  const unsigned gtr = vy_lds_addr(gt) + (4 * kq + (r16 >> 2)) * PITCH + (4 * (r16 & 3)) * 2;
  for (int hh = 0; hh < nrep; ++hh) {
    const int head = kvh * nrep + hh;
    const bf16* Qb = p.q + (int64_t)b * p.q_sb + (int64_t)head * p.q_sh;
    const bf16* Gb = p.dout + (int64_t)b * p.o_sb + head * dh;
    const int64_t stat0 = ((int64_t)b * p.h + head) * p.L;
    for (int q0 = qstart; q0 < p.L; q0 += 64) {
      bf16x8 qreg[CPT], greg[CPT];
      gen_stage<DHP>(qt, Qb, p.q_sl, q0, p.L, dh, tid, qreg);
      gen_stage<DHP>(gt, Gb, p.o_sl, q0, p.L, dh, tid, greg);
      float ls = 0.f, dl = 0.f;
      if (tid < 64) {
        const int qq = q0 + tid;
        ls = qq < p.L ? -p.lse[stat0 + qq] * LOG2E : 0.f;
        dl = qq < p.L ? p.delta[stat0 + qq] : 0.f;
      }
      __syncthreads();
      gen_store<DHP>(qt, tid, qreg);
      gen_store<DHP>(gt, tid, greg);
      if (tid < 64) { lse_s[tid] = ls; del_s[tid] = dl; }
      __syncthreads();
      // S[q][key] and dP[q][key]: A = Q / dO rows of the tile, B = this lane's key
      f32x4 pr[4], dsv[4];
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        f32x4 sc = {0.f, 0.f, 0.f, 0.f};
        f32x4 dp;
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[r] = del_s[16 * blk + 4 * kq + r];   // -delta of the lane's query rows
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 qf = *reinterpret_cast<const bf16x8*>(qt + (16 * blk + r16) * PITCH + (32 * ks + 8 * kq) * 2);
          const bf16x8 gf = *reinterpret_cast<const bf16x8*>(gt + (16 * blk + r16) * PITCH + (32 * ks + 8 * kq) * 2);
          sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf[ks], sc, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf, vf[ks], dp, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = q0 + 16 * blk + 4 * kq + r;
          bool vis = key_vis && qq < p.L;
          if (causal) vis = vis && kj <= qq + p.start_pos;
          const float pv = vis ? __builtin_amdgcn_exp2f(fmaf(sc[r], c, lse_s[16 * blk + 4 * kq + r])) : 0.f;
          pr[blk][r] = pv;
          dsv[blk][r] = pv * dp[r];
        }
      }
      // dV^T += dO^T P, dK^T += Q^T dS: k-steps of 32 query rows = blocks (2 tt, 2 tt + 1)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        bf16x8 pf, sf;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pf[r] = (bf16)pr[2 * tt][r]; pf[4 + r] = (bf16)pr[2 * tt + 1][r];
          sf[r] = (bf16)dsv[2 * tt][r]; sf[4 + r] = (bf16)dsv[2 * tt + 1][r];
        }
        vy_static_for<NDB>([&](auto n_c) {
          constexpr int n = decltype(n_c)::value;
          union { struct { s16x4 a, b; } h; bf16x8 v; } ug, uq;
          ug.h.a = vy_lds_tr16_off<n * 32>(gtr + (32 * tt) * PITCH);
          ug.h.b = vy_lds_tr16_off<n * 32>(gtr + (32 * tt + 16) * PITCH);
          uq.h.a = vy_lds_tr16_off<n * 32>(qtr + (32 * tt) * PITCH);
          uq.h.b = vy_lds_tr16_off<n * 32>(qtr + (32 * tt + 16) * PITCH);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          vy_tie(ug.v); vy_tie(uq.v);
          dv[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ug.v, pf, dv[n], 0, 0, 0);
          dk[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(uq.v, sf, dk[n], 0, 0, 0);
        });
      }
    }
  }
  if (kj < p.S) {
    bf16* DK = p.dk + (int64_t)b * p.dk_sb + (int64_t)kvh * p.dk_sh + (int64_t)kj * p.dk_sl;
    bf16* DV = p.dv + (int64_t)b * p.dv_sb + (int64_t)kvh * p.dv_sh + (int64_t)kj * p.dv_sl;
#pragma unroll
    for (int n = 0; n < NDB; ++n) {
      const int d0 = 16 * n + 4 * kq;
      if (d0 < dh) {
        bf16x4 wk_, wv_;
#pragma unroll
        for (int r = 0; r < 4; ++r) { wk_[r] = (bf16)(dk[n][r] * p.scale); wv_[r] = (bf16)dv[n][r]; }
        *reinterpret_cast<bf16x4*>(DK + d0) = wk_;
        *reinterpret_cast<bf16x4*>(DV + d0) = wv_;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// fp32 attention backward (any head width up to 256; the parity path -- plain FMAs, expf, no atomics):
//   dq kernel:    16 query rows per workgroup, keys in chunks of 64.  Phase A, thread (row, 4 keys): s = q . k,
//                 dp = dO . v, P = exp(s * scale - lse), dS = P (dp - delta) -> LDS.  Phase B, thread (row, every
//                 16th column): dq += dS K.  delta = rowsum(dO o O) is computed here and left in delta_ws.
//   dk/dv kernel: 16 keys per workgroup, the query heads of the KV group and their rows in chunks of 64; the same two
//                 phases with the roles exchanged: dv += P^T dO, dk += dS^T Q.
// A row without a visible key got the reference's uniform softmax over ALL keys in the forward (scores +
// finfo.min collapse to finfo.min: attention.py:133-137) and autograd differentiates exactly that: P = 1 / S for every
// key of such a row (its lse is ~ -FLT_MAX).
// ------------------------------------------------------------------------------------------
constexpr int F32_PITCH = 260;
__device__ __forceinline__ float f32_prob(bool dead, bool vis, bool in_range, float s, float scale, float lse, float inv_s) {
  if (dead) return in_range ? inv_s : 0.f;
  return vis ? expf(fmaf(s, scale, -lse)) : 0.f;
}

__global__ __launch_bounds__(256) void attn_bwd_f32_dq_kernel(BwdParams p, int dh) {
  __shared__ __attribute__((aligned(16))) float sq[16][F32_PITCH], sg[16][F32_PITCH];
  __shared__ float sds[16][65];
  __shared__ float s_lse[16], s_del[16];
  const float* Qp = reinterpret_cast<const float*>(p.q);
  const float* Kp = reinterpret_cast<const float*>(p.k);
  const float* Vp = reinterpret_cast<const float*>(p.v);
  const float* Op = reinterpret_cast<const float*>(p.o);
  const float* Gp = reinterpret_cast<const float*>(p.dout);
  const int tid = threadIdx.x;
  const int head = (int)blockIdx.x % p.h, b = (int)blockIdx.x / p.h;
  const int kvh = head / (p.h / p.hk);
  const int q0 = (int)blockIdx.y * 16;
  const float* Kb = Kp + (int64_t)b * p.k_sb + (int64_t)kvh * p.k_sh;
  const float* Vb = Vp + (int64_t)b * p.v_sb + (int64_t)kvh * p.v_sh;
  const bool causal = p.mask_kind & VY_MASK_CAUSAL;
  const bool haskp = p.mask_kind & VY_MASK_KEYPAD;
  const uint8_t* kp = haskp ? p.keypad + (int64_t)b * p.kp_sb : nullptr;
  const int r = tid >> 4, c = tid & 15;
  const int qi = q0 + r;
  const int64_t stat = ((int64_t)b * p.h + head) * p.L + (qi < p.L ? qi : p.L - 1);
  {
    float part = 0.f;
    const float* Qr = Qp + (int64_t)b * p.q_sb + (int64_t)head * p.q_sh + (int64_t)(qi < p.L ? qi : 0) * p.q_sl;
    const float* Gr = Gp + (int64_t)b * p.o_sb + (int64_t)(qi < p.L ? qi : 0) * p.o_sl + head * dh;
    const float* Or = Op + (int64_t)b * p.o_sb + (int64_t)(qi < p.L ? qi : 0) * p.o_sl + head * dh;
    for (int d = c; d < F32_PITCH; d += 16) {
      const bool ok = d < dh && qi < p.L;
      const float g = ok ? Gr[d] : 0.f;
      sq[r][d] = ok ? Qr[d] : 0.f;
      sg[r][d] = g;
      part += ok ? g * Or[d] : 0.f;
    }
#pragma unroll
    for (int o_ = 8; o_ > 0; o_ >>= 1) part += __shfl_xor(part, o_, 64);
    if (c == 0) {
      s_del[r] = part;
      s_lse[r] = qi < p.L ? p.lse[stat] : 0.f;
      if (qi < p.L) p.delta[stat] = part;
    }
  }
  __syncthreads();
  const float lse = s_lse[r], delta = s_del[r];
  const bool dead = haskp && lse < -1e37f;
  const float inv_s = 1.f / (float)p.S;
  float dq[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) dq[i] = 0.f;
  // with key padding every key is walked (dead rows); pure causal stops at the block's diagonal
  const int s_hi = causal && !haskp ? min(p.S, p.start_pos + q0 + 16) : p.S;
  const int dh4 = (dh + 3) & ~3;   // the LDS rows are zero beyond dh; global rows are read in float4s up to roundup4(dh) <= row stride
  for (int k0 = 0; k0 < s_hi; k0 += 64) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kj = k0 + 4 * c + e;
      const int kjc = kj < p.S ? kj : p.S - 1;
      const float* Kr = Kb + (int64_t)kjc * p.k_sl;
      const float* Vr = Vb + (int64_t)kjc * p.v_sl;
      float s = 0.f, dp = 0.f;
      for (int d = 0; d < dh4; d += 4) {
        const f32x4 kv = *reinterpret_cast<const f32x4*>(Kr + d), vv = *reinterpret_cast<const f32x4*>(Vr + d);
        const f32x4 qv = *reinterpret_cast<const f32x4*>(&sq[r][d]), gv = *reinterpret_cast<const f32x4*>(&sg[r][d]);
#pragma unroll
        for (int t = 0; t < 4; ++t) { s = fmaf(qv[t], kv[t], s); dp = fmaf(gv[t], vv[t], dp); }
      }
      bool vis = kj < p.S && qi < p.L;
      if (causal) vis = vis && kj <= qi + p.start_pos;
      if (haskp) vis = vis && kp[kjc] != 0;
      const float pr = f32_prob(dead, vis, kj < p.S && qi < p.L, s, p.scale, lse, inv_s);
      sds[r][4 * c + e] = pr * (dp - delta);
    }
    __syncthreads();
    const int jn = min(64, p.S - k0);
    for (int j = 0; j < jn; ++j) {
      const float w = sds[r][j];
      const float* Kr = Kb + (int64_t)(k0 + j) * p.k_sl;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int d = c + 16 * i;
        if (d < dh) dq[i] = fmaf(w, Kr[d], dq[i]);
      }
    }
    __syncthreads();
  }
  if (qi < p.L) {
    float* D = reinterpret_cast<float*>(p.dq) + (int64_t)b * p.dq_sb + (int64_t)head * p.dq_sh + (int64_t)qi * p.dq_sl;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int d = c + 16 * i;
      if (d < dh) D[d] = dq[i] * p.scale;
    }
  }
}

__global__ __launch_bounds__(256) void attn_bwd_f32_dkdv_kernel(BwdParams p, int dh) {
  __shared__ __attribute__((aligned(16))) float sk[16][F32_PITCH], sv[16][F32_PITCH];
  __shared__ float sp[16][65], sds[16][65];
  __shared__ float s_lse[64], s_del[64];
  const float* Qp = reinterpret_cast<const float*>(p.q);
  const float* Kp = reinterpret_cast<const float*>(p.k);
  const float* Vp = reinterpret_cast<const float*>(p.v);
  const float* Gp = reinterpret_cast<const float*>(p.dout);
  const int tid = threadIdx.x;
  const int kvh = (int)blockIdx.x % p.hk, b = (int)blockIdx.x / p.hk;
  const int nrep = p.h / p.hk;
  const int k0 = (int)blockIdx.y * 16;
  const bool causal = p.mask_kind & VY_MASK_CAUSAL;
  const bool haskp = p.mask_kind & VY_MASK_KEYPAD;
  const int r = tid >> 4, c = tid & 15;
  const int kj = k0 + r;
  const int kjc = kj < p.S ? kj : p.S - 1;
  {
    const float* Kr = Kp + (int64_t)b * p.k_sb + (int64_t)kvh * p.k_sh + (int64_t)kjc * p.k_sl;
    const float* Vr = Vp + (int64_t)b * p.v_sb + (int64_t)kvh * p.v_sh + (int64_t)kjc * p.v_sl;
    for (int d = c; d < F32_PITCH; d += 16) {
      const bool ok = d < dh && kj < p.S;
      sk[r][d] = ok ? Kr[d] : 0.f;
      sv[r][d] = ok ? Vr[d] : 0.f;
    }
  }
  const bool key_vis = kj < p.S && (!haskp || p.keypad[(int64_t)b * p.kp_sb + kjc] != 0);
  const float inv_s = 1.f / (float)p.S;
  float dk[16], dv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dk[i] = 0.f; dv[i] = 0.f; }
  const int qstart = causal && !haskp ? max(0, k0 - p.start_pos) & ~63 : 0;
  const int dh4 = (dh + 3) & ~3;
  for (int hh = 0; hh < nrep; ++hh) {
    const int head = kvh * nrep + hh;
    const float* Qb = Qp + (int64_t)b * p.q_sb + (int64_t)head * p.q_sh;
    const float* Gb = Gp + (int64_t)b * p.o_sb + head * dh;
    const int64_t stat0 = ((int64_t)b * p.h + head) * p.L;
    for (int q0 = qstart; q0 < p.L; q0 += 64) {
      __syncthreads();   // the previous chunk's phase B has read sp / sds / (first trip: sk / sv are written)
      if (tid < 64) {
        const int qq = q0 + tid;
        s_lse[tid] = qq < p.L ? p.lse[stat0 + qq] : 0.f;
        s_del[tid] = qq < p.L ? p.delta[stat0 + qq] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ql = 4 * c + e, qq = q0 + ql;
        const int qc = qq < p.L ? qq : p.L - 1;
        const float* Qr = Qb + (int64_t)qc * p.q_sl;
        const float* Gr = Gb + (int64_t)qc * p.o_sl;
        float s = 0.f, dp = 0.f;
        for (int d = 0; d < dh4; d += 4) {
          const f32x4 qv = *reinterpret_cast<const f32x4*>(Qr + d), gv = *reinterpret_cast<const f32x4*>(Gr + d);
          const f32x4 kv = *reinterpret_cast<const f32x4*>(&sk[r][d]), vv = *reinterpret_cast<const f32x4*>(&sv[r][d]);
#pragma unroll
          for (int t = 0; t < 4; ++t) { s = fmaf(qv[t], kv[t], s); dp = fmaf(gv[t], vv[t], dp); }
        }
        const float lse = s_lse[ql];
        const bool dead = haskp && lse < -1e37f;
        bool vis = key_vis && qq < p.L;
        if (causal) vis = vis && kj <= qq + p.start_pos;
        const float pr = f32_prob(dead, vis, kj < p.S && qq < p.L, s, p.scale, lse, inv_s);
        sp[r][ql] = pr;
        sds[r][ql] = pr * (dp - s_del[ql]);
      }
      __syncthreads();
      const int jn = min(64, p.L - q0);
      for (int j = 0; j < jn; ++j) {
        const float pw = sp[r][j], dw_ = sds[r][j];
        const float* Qr = Qb + (int64_t)(q0 + j) * p.q_sl;
        const float* Gr = Gb + (int64_t)(q0 + j) * p.o_sl;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int d = c + 16 * i;
          if (d < dh) { dv[i] = fmaf(pw, Gr[d], dv[i]); dk[i] = fmaf(dw_, Qr[d], dk[i]); }
        }
      }
    }
  }
  if (kj < p.S) {
    float* DK = reinterpret_cast<float*>(p.dk) + (int64_t)b * p.dk_sb + (int64_t)kvh * p.dk_sh + (int64_t)kj * p.dk_sl;
    float* DV = reinterpret_cast<float*>(p.dv) + (int64_t)b * p.dv_sb + (int64_t)kvh * p.dv_sh + (int64_t)kj * p.dv_sl;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int d = c + 16 * i;
      if (d < dh) { DK[d] = dk[i] * p.scale; DV[d] = dv[i]; }
    }
  }
}

}  // namespace

extern "C" int vy_attn_bwd(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sl, const void* k,
                           int64_t k_sb, int64_t k_sh, int64_t k_sl, const void* v, int64_t v_sb,
                           int64_t v_sh, int64_t v_sl, const void* out, const void* dout, int64_t o_sb,
                           int64_t o_sl, const float* lse, float* delta_ws, void* dq, int64_t dq_sb,
                           int64_t dq_sh, int64_t dq_sl, void* dk, int64_t dk_sb, int64_t dk_sh,
                           int64_t dk_sl, void* dv, int64_t dv_sb, int64_t dv_sh, int64_t dv_sl,
                           int mask_kind, int64_t start_pos, const uint8_t* keypad, int64_t kp_sb,
                           const float* cos_tab, const float* sin_tab, int64_t rope_pos0, int64_t B,
                           int h, int hk, int64_t L, int64_t S, int dh, float scale, int dtype, void* stream) {
  const char* who = "vy_attn_bwd";
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "%s: bad dtype %d", who, dtype);
  if (dh != 64 && (dh % 8 || dh > 256 || dh < 8)) VY_FAIL(VY_ERR_UNSUPPORTED, "%s: head_dim %d (multiples of 8 up to 256)", who, dh);
  if (mask_kind & VY_MASK_ADDITIVE) VY_FAIL(VY_ERR_UNSUPPORTED, "%s: generic additive masks have no backward; use causal/key-padding descriptors", who);
  if (!q || !k || !v || !out || !dout || !lse || !delta_ws || !dq || !dk || !dv) VY_FAIL(VY_ERR_ARG, "%s: null tensor", who);
  if (B <= 0 || h <= 0 || hk <= 0 || h % hk || L <= 0 || S <= 0) VY_FAIL(VY_ERR_ARG, "%s: bad sizes", who);
  if ((mask_kind & VY_MASK_KEYPAD) && !keypad) VY_FAIL(VY_ERR_ARG, "%s: keypad mask requested but NULL", who);
  if ((mask_kind & VY_MASK_KEYPAD) && S > 16384) VY_FAIL(VY_ERR_UNSUPPORTED, "%s: key-padding masks cover at most 16384 keys", who);
  const int64_t s8[] = {q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, o_sb, o_sl,
                        dq_sb, dq_sh, dq_sl, dk_sb, dk_sh, dk_sl, dv_sb, dv_sh, dv_sl};
  for (int64_t x : s8)
    if (x % 8) VY_FAIL(VY_ERR_ARG, "%s: strides must be multiples of 8 elements", who);
  BwdParams p;
  p.q = (const bf16*)q; p.q_sb = q_sb; p.q_sh = q_sh; p.q_sl = q_sl;
  p.k = (const bf16*)k; p.k_sb = k_sb; p.k_sh = k_sh; p.k_sl = k_sl;
  p.v = (const bf16*)v; p.v_sb = v_sb; p.v_sh = v_sh; p.v_sl = v_sl;
  p.o = (const bf16*)out; p.dout = (const bf16*)dout; p.o_sb = o_sb; p.o_sl = o_sl;
  p.lse = lse; p.delta = delta_ws;
  p.dq = (bf16*)dq; p.dq_sb = dq_sb; p.dq_sh = dq_sh; p.dq_sl = dq_sl;
  p.dk = (bf16*)dk; p.dk_sb = dk_sb; p.dk_sh = dk_sh; p.dk_sl = dk_sl;
  p.dv = (bf16*)dv; p.dv_sb = dv_sb; p.dv_sh = dv_sh; p.dv_sl = dv_sl;
  p.mask_kind = mask_kind; p.start_pos = (int)start_pos; p.keypad = keypad; p.kp_sb = kp_sb;
  p.B = (int)B; p.h = h; p.hk = hk; p.L = (int)L; p.S = (int)S; p.scale = scale;
  if ((cos_tab == nullptr) != (sin_tab == nullptr)) VY_FAIL(VY_ERR_ARG, "%s: cos/sin must both be given", who);
  p.cos_tab = cos_tab; p.sin_tab = sin_tab; p.rope_pos0 = (int)rope_pos0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VY_F32 || dh != 64) {
    if (dtype == VY_F32) {
      // the parity path: plain fp32 kernels (the BwdParams pointers are fp32 here)
      const dim3 gq((unsigned)(h * B), (unsigned)((L + 15) / 16), 1), gk((unsigned)(hk * B), (unsigned)((S + 15) / 16), 1), block(256);
      hipLaunchKernelGGL(attn_bwd_f32_dq_kernel, gq, block, 0, st, p, dh);
      VY_CHECK_LAUNCH("vy_attn_bwd(dq)");
      hipLaunchKernelGGL(attn_bwd_f32_dkdv_kernel, gk, block, 0, st, p, dh);
      VY_CHECK_LAUNCH("vy_attn_bwd(dkdv)");
    } else {
      // other head widths: the general kernels
      const dim3 gq((unsigned)(h * B), (unsigned)((L + 63) / 64), 1), gk((unsigned)(hk * B), (unsigned)((S + 63) / 64), 1), block(256);
      if (dh <= 96) hipLaunchKernelGGL(attn_bwd_gen_dq_kernel<96>, gq, block, 0, st, p, dh);
      else if (dh <= 128) hipLaunchKernelGGL(attn_bwd_gen_dq_kernel<128>, gq, block, 0, st, p, dh);
      else hipLaunchKernelGGL(attn_bwd_gen_dq_kernel<256>, gq, block, 0, st, p, dh);
      VY_CHECK_LAUNCH("vy_attn_bwd(dq)");
      if (dh <= 96) hipLaunchKernelGGL(attn_bwd_gen_dkdv_kernel<96>, gk, block, 0, st, p, dh);
      else if (dh <= 128) hipLaunchKernelGGL(attn_bwd_gen_dkdv_kernel<128>, gk, block, 0, st, p, dh);
      else hipLaunchKernelGGL(attn_bwd_gen_dkdv_kernel<256>, gk, block, 0, st, p, dh);
      VY_CHECK_LAUNCH("vy_attn_bwd(dkdv)");
    }
    // neither family fuses the rotary inverse: dq, then dk, are rotated back afterwards
    if (!cos_tab) return VY_OK;
    const int rc = vy_rope_fwd(dq, dq_sb, dq_sh, dq_sl, cos_tab, sin_tab, rope_pos0, B, h, L, dh, 1, dtype, stream);
    if (rc != VY_OK) return rc;
    return vy_rope_fwd(dk, dk_sb, dk_sh, dk_sl, cos_tab, sin_tab, rope_pos0, B, hk, S, dh, 1, dtype, stream);
  }
  // (delta = rowsum(dO * O) is computed by the dQ kernel for its own rows and left in delta_ws for the dK/dV kernel)
  hipLaunchKernelGGL(attn_bwd_dq_kernel, dim3((unsigned)(h * B), (unsigned)((L + 127) / 128), 1), dim3(256), 0, st, p);
  VY_CHECK_LAUNCH("vy_attn_bwd(dq)");
  hipLaunchKernelGGL(attn_bwd_dkdv_kernel, dim3((unsigned)(hk * B), (unsigned)((S + 127) / 128), 1), dim3(256), 0, st, p);
  VY_CHECK_LAUNCH("vy_attn_bwd(dkdv)");
  return VY_OK;
}
