// The tile core of the tuned attention kernels (bf16, 32x32x16 MFMAs): attn_fwd_mfma_kernel<64|128> in vy_attn.hip,
// attn_bwd_dq_kernel and attn_bwd_dkdv_kernel in vy_bwd.hip.  What the four share is written here once; a kernel keeps
// its LDS budget, the swizzle of each operand, its schedule inside a stage and its epilogue.  A STAGE is a pair of
// 64-row x RB-byte operand tiles (K/V for the forward and dQ, Q/dO for dK/dV) written by LDS-DMA into a ring of NS
// stages: operand A's NS tiles, then operand B's.  The two compiler facts of DESIGN.md section 3, stated once:
//   (1) LDS reads that must overlap the MFMAs are asm reads retired by COUNTED lgkmcnt waits tied to the fragment
//       registers (attn_tr_frag, vy_lds_read128_off, vy_lgkm_wait) -- and a kernel has ONE __shared__ object;
//   (2) every ordinary (VGPR-destination) load is retired between the ring's prologue and its loop (AttnRing):
//       a load whose first use is inside the loop becomes a vmcnt(0) there and drains the ring.
// Everything is a __forceinline__ function or member that takes the kernel's registers by reference.
#pragma once
#include "vy_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// lane geometry of the 32x32x16 layout.  fr / fh: fragment row and k half (A/B operands, and column / row-quad of an
// accumulator); li / g16: lane inside a 16-lane group of a transposing read and the group's parity
struct AttnLane {
  int lane, wave, fr, fh, li, g16;
  __device__ __forceinline__ AttnLane() {
    lane = threadIdx.x & 63; wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    fr = lane & 31; fh = lane >> 5; li = lane & 15; g16 = (lane >> 4) & 1;
  }
  __device__ __forceinline__ int t_row() const { return 4 * fh + (li >> 2); }   // row this lane supplies to a transposing read
};

// accumulator register r of a 32x32 block <-> row (r&3) + 8(r>>2) + 4fh: the bit of r in a word already shifted by 4fh
__device__ __forceinline__ constexpr int attn_reg_bit(int r) { return (r & 3) + 8 * (r >> 2); }

// ---- operand swizzles: (row of the tile, byte offset in the row) -> element offset in the SOURCE row ---------------
// chunk swizzle of a 128-B-row LDS image that is read BOTH by rows (ds_read_b128) and transposed
// (ds_read_b64_tr_b16): conflict-free for both ("dual-use image")
__device__ __forceinline__ int dual_sw(int row) {
  const int v = (row >> 1) & 7;
  return ((v & 1) << 2) | (v >> 1);
}
template <int RB>
struct SwRows {  // read by rows only: 16-byte chunk ^ (row>>1)&7 (128-B rows) or row&15 (256-B rows)
  static __device__ __forceinline__ int key(int row) { return RB == 128 ? ((row >> 1) & 7) : (row & 15); }
  __device__ __forceinline__ int operator()(int row, int off) const { return (((off >> 4) ^ key(row)) << 4) >> 1; }
};
template <int RB>
struct SwTr64 {  // read transposed only: swizzled in 64-byte units, the four rows of a transposed read hit distinct banks
  __device__ __forceinline__ int operator()(int row, int off) const {
    return (off ^ (RB == 128 ? (((row >> 1) & 1) << 6) : ((row & 3) << 6))) >> 1;
  }
};
struct SwDual {
  __device__ __forceinline__ int operator()(int row, int off) const { return (((off >> 4) ^ dual_sw(row)) << 4) >> 1; }
};

// ---- the stage writer -----------------------------------------------------------------------------
// A tile is TILE / 1024 LDS-DMA pieces of 1 KiB (64 lanes x 16 bytes); wave w writes pieces NP w .. NP w + NP - 1 of
// both operands: DMA = 2 NP LDS-DMA instructions per wave and stage.  Lane byte P of the image belongs to tile row
// P / RB; the swizzle says which 16 bytes of that source row go there; rows beyond `bound` are clamped to the last row
// (masked later, never skipped).  WHOLE adds the forward's fast path: per-lane source pointers of tile 0, to which a
// tile whose 64 rows all exist adds a wave-uniform offset (two 64-bit adds per piece instead of clamp and multiplies).
template <int RB, int NS, bool WHOLE = false>
struct AttnStage {
  static constexpr int TILE = 64 * RB, NP = TILE / 1024 / 4, DMA = 2 * NP;
  int row[NP], aoff[NP], boff[NP];
  const bf16* a0[WHOLE ? NP : 1];
  const bf16* b0[WHOLE ? NP : 1];

  template <typename SA, typename SB>
  __device__ __forceinline__ AttnStage(const AttnLane& ln, SA sa, SB sb) {
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int P = (ln.wave * NP + t) * 1024 + ln.lane * 16;
      row[t] = P / RB;
      aoff[t] = sa(P / RB, P % RB);
      boff[t] = sb(P / RB, P % RB);
    }
  }
  __device__ __forceinline__ void whole_tiles(const bf16* A, int64_t a_sl, const bf16* B, int64_t b_sl, int bound) {
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int r0 = row[t] < bound ? row[t] : bound - 1;
      a0[t] = A + (int64_t)r0 * a_sl + aoff[t];
      b0[t] = B + (int64_t)r0 * b_sl + boff[t];
    }
  }
  static __device__ __forceinline__ void dma(const bf16* src, char* smem, int slot, int piece) {
    __builtin_amdgcn_global_load_lds((const VY_GLOBAL void*)src, (VY_LDS void*)(smem + slot * TILE + piece * 1024), 16, 0, 0);
  }
  // rows row0 .. row0 + 63 of A and B (row strides a_sl / b_sl, rows clamped to bound - 1) into buffer buf
  __device__ __forceinline__ void issue(char* smem, int wave, int buf, int row0, int bound, const bf16* A, int64_t a_sl,
                                        const bf16* B, int64_t b_sl) const {
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      int r = row0 + row[t];
      r = r < bound ? r : bound - 1;
      dma(A + (int64_t)r * a_sl + aoff[t], smem, buf, wave * NP + t);
      dma(B + (int64_t)r * b_sl + boff[t], smem, NS + buf, wave * NP + t);
    }
  }
  // tile `tile` of whole_tiles()' operands, every row of which exists: a_tile / b_tile = elements per 64 rows
  __device__ __forceinline__ void issue_whole(char* smem, int wave, int buf, int tile, int64_t a_tile, int64_t b_tile) const {
    const int64_t ao = (int64_t)tile * a_tile, bo = (int64_t)tile * b_tile;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      dma(a0[t] + ao, smem, buf, wave * NP + t);
      dma(b0[t] + bo, smem, NS + buf, wave * NP + t);
    }
  }
};

// ---- the ring -------------------------------------------------------------------------------------
// Loads run AHEAD = NS - 1 stages ahead of the MFMAs.  A stage is DMA LDS-DMA instructions per wave, then the OLDEST
// outstanding memory operations of that wave, so stage t is waited for with a counted vmcnt that leaves the NS - 2
// younger stages in flight (vmcnt(0) once fewer follow: exact for NS = 3), and one raw s_barrier; nothing in the loop
// drains the memory pipe.  The frame is the same in every kernel and stays there -- the stage and compute lambdas
// must be called from the kernel itself (inlined through a template frame they changed the loop's code):
//     for (s < AHEAD) if (s < n) stage(s, s);            prologue
//     <issue and/or vy_tie every ordinary load>          fact (2): retired before the loop, after the first requests
//     for (t < n) { Ring::arrive(t, n);  if (t + AHEAD < n) stage(t + AHEAD, (t + AHEAD) % NS);  compute(t, t % NS); }
template <int NS, int DMA>
struct AttnRing {
  static constexpr int AHEAD = NS - 1;
  static __device__ __forceinline__ void arrive(int t, int n) {
    if (t + NS - 2 < n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * DMA) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
};

// ---- mask words -----------------------------------------------------------------------------------
// visibility bits [lo, hi) of a 32- or 64-wide index range (lo/hi may lie outside it)
__device__ __forceinline__ unsigned long long range_bits64(int lo, int hi) {
  const unsigned long long up = hi >= 64 ? ~0ull : (hi <= 0 ? 0ull : ((1ull << hi) - 1ull));
  const unsigned long long dn = lo >= 64 ? 0ull : (lo <= 0 ? ~0ull : (~0ull << lo));
  return up & dn;
}
// key-padding mask -> one 64-bit visibility word per key tile, built once before the ring (an ordinary load inside
// the tile loop would make the compiler drain the LDS-DMA ring with vmcnt(0) every tile)
__device__ __forceinline__ void attn_keypad_words(unsigned long long* words, const uint8_t* kp, int nt, int S, const AttnLane& ln) {
  for (int t = ln.wave; t < nt; t += 4) {
    const int kj = t * 64 + ln.lane;
    const bool vis = kj < S && kp[kj < S ? kj : 0] != 0;
    const unsigned long long bits = __ballot(vis);
    if (ln.lane == 0) words[t] = bits;
  }
  __syncthreads();
}
// The lane's keys of tile k0 as one bit word (query row qi, a lane's keys start at k0 + 4fh): key offset kofs =
// 32kb + attn_reg_bit(r) is visible iff kofs <= klim (end of the sequence, causal diagonal) and the padding word says so.
__device__ __forceinline__ unsigned long long attn_key_bits(int k0, int fh, int S, bool causal, int diag, unsigned long long vis) {
  int klim = S - 1 - k0 - 4 * fh;
  if (causal) klim = min(klim, diag - k0 - 4 * fh);
  return range_bits64(0, klim + 1) & (vis >> (4 * fh));
}

// ---- transposed fragments of a dual-use image (128-byte rows, SwDual) ----------------------------------
// LDS byte addresses of the transposed fragment of d block n, rows t_row (+ 8u), buffer 0 of the first ring
__device__ __forceinline__ void attn_tr_bases(unsigned (&base)[2][2], const char* smem, const AttnLane& ln) {
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = ln.t_row() + 8 * u, chunk = 4 * n + 2 * ln.g16 + ((ln.li & 3) >> 1);
      base[n][u] = vy_lds_addr(smem) + row * 128 + ((chunk ^ dual_sw(row)) << 4) + 8 * (ln.li & 1);
    }
}
// rows r and r + 8 of a transposed 16-row block (base[0], base[1]), `add` + OFF bytes on (OFF goes into the offset
// field): one MFMA fragment, two asm reads, NO wait -- the caller retires them with vy_lgkm_wait<N>(fragment), fact (1)
template <int OFF>
__device__ __forceinline__ bf16x8 attn_tr_frag(const unsigned (&base)[2], unsigned add = 0) {
  union { struct { s16x4 a, b; } s_; bf16x8 v; } u;
  u.s_.a = vy_lds_tr16_off<OFF>(base[0] + add);
  u.s_.b = vy_lds_tr16_off<OFF>(base[1] + add);
  return u.v;
}

// ---- backward pieces ---------------------------------------------------------------------------------
// P recomputed from the raw score: exp2(s c - lse log2e).  Masked: select by bit, never multiply (a score may be +inf)
template <bool MASKED>
__device__ __forceinline__ float attn_p(float s, float c, float neg_lse, unsigned word, int r) {
  const float pr = __builtin_amdgcn_exp2f(fmaf(s, c, neg_lse));
  if (MASKED) return ((word >> attn_reg_bit(r)) & 1u) ? pr : 0.f;
  return pr;
}

// RoPE is an orthogonal map, so its backward is the transposed rotation of the gradient pair (d, d+32): lo' = lo*c + hi*s,
// hi' = hi*c - lo*s, with the same storage-rounded cos/sin the forward used.  pos = token position, d0 = first of the 4
// consecutive d (< 32) of this quad.
__device__ __forceinline__ void rope_bwd_quad(const float* cos_tab, const float* sin_tab, int64_t pos, int d0, float (&lo)[4], float (&hi)[4]) {
  const f32x4 c4 = *reinterpret_cast<const f32x4*>(cos_tab + pos * 32 + d0);
  const f32x4 s4 = *reinterpret_cast<const f32x4*>(sin_tab + pos * 32 + d0);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float c = vy_round_bf16(c4[e]), s = vy_round_bf16(s4[e]);
    const float a = lo[e], b = hi[e];
    lo[e] = fmaf(a, c, b * s);      // spelled out: the contraction the compiler chose decides the last bit
    hi[e] = fmaf(b, c, -(a * s));
  }
}
// dQ / dK epilogue (dh = 64): this lane's row of the transposed accumulator, scaled, rotated back when cos_tab is
// given (pos = the row's token position), stored as two bf16x4 per register quad
__device__ __forceinline__ void attn_store_scaled_rope(bf16* D, const f32x16 (&acc)[2], float scale, const float* cos_tab,
                                                       const float* sin_tab, int64_t pos, int fh) {
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    float lo[4], hi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { lo[e] = acc[0][4 * rg + e] * scale; hi[e] = acc[1][4 * rg + e] * scale; }
    if (cos_tab) rope_bwd_quad(cos_tab, sin_tab, pos, 8 * rg + 4 * fh, lo, hi);
    bf16x4 wl, wh;
#pragma unroll
    for (int e = 0; e < 4; ++e) { wl[e] = (bf16)lo[e]; wh[e] = (bf16)hi[e]; }
    *reinterpret_cast<bf16x4*>(D + 8 * rg + 4 * fh) = wl;
    *reinterpret_cast<bf16x4*>(D + 32 + 8 * rg + 4 * fh) = wh;
  }
}

// ---- grid decode of the kernels that own query rows (forward, dQ) -------------------------------------
// grid = (h*B, query blocks of 128 rows): the dispatcher walks x first, so ALL the heaviest query blocks (most keys
// under a causal mask) of every (batch, head) start before any lighter one -- longest-processing-time order; with
// (query block, head, batch) order the last (batch, head) groups still start full-length workgroups at the very end
// and causal ran as long as full.  P is AttnParams or BwdParams: they keep their own layouts (a common base would move
// the kernel arguments of every other kernel that takes them).
struct AttnQBlock {
  int head, b, kvh, q0, qi, qrow;
  const bf16 *Q, *Kb, *Vb;   // this lane's query row; the (batch, kv head) bases of K and V
  template <typename P>
  __device__ __forceinline__ AttnQBlock(const P& p, const AttnLane& ln) {
    const int nqb = (p.L + 127) / 128;
    head = (int)blockIdx.x % p.h; b = (int)blockIdx.x / p.h;
    kvh = head / (p.h / p.hk);   // GQA: repeat_kv is never materialised
    q0 = (nqb - 1 - (int)blockIdx.y) * 128;
    qi = q0 + ln.wave * 32 + ln.fr; qrow = qi < p.L ? qi : p.L - 1;
    Q = (const bf16*)p.q + (int64_t)b * p.q_sb + (int64_t)head * p.q_sh + (int64_t)qrow * p.q_sl;
    Kb = (const bf16*)p.k + (int64_t)b * p.k_sb + (int64_t)kvh * p.k_sh;
    Vb = (const bf16*)p.v + (int64_t)b * p.v_sb + (int64_t)kvh * p.v_sh;
  }
  // key tiles a block walks: under a pure causal mask, keys beyond the diagonal of its last row are never visible
  template <typename P>
  __device__ __forceinline__ int key_tiles(const P& p, bool causal) const {
    int nt = (p.S + 63) / 64;
    if (causal) nt = max(1, min(nt, (min(p.S, p.start_pos + q0 + 128) + 63) / 64));
    return nt;
  }
};

}  // namespace
