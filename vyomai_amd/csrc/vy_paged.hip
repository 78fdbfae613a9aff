// Paged KV cache (reference Examples/simple_vllm.ipynb cell 2): the per-token RoPE + scatter of a packed step's K/V rows
// into pages, single-query attention through a block table, and the gather of one sequence's pages for a prefill that
// starts from cached prefix blocks.  Cache layout per layer: k_cache / v_cache (max_blocks, block_size, hk, dh), contiguous;
// slot s = block * block_size + offset names row s of the (max_blocks * block_size, hk, dh) view.
//
// vy_attn_paged_decode follows dec_attn_kernel's R > 1 case (vy_decode.hip): a workgroup serves the query heads of one KV
// head from ONE read of its K/V rows, K/V go straight to registers, reductions stay on the DPP / permlane path
// (vy_wave.h).  What differs: the context is not bounded, so a lane group walks its keys with an fp32 online softmax (a
// running maximum per lane group, rescaled once per U keys, no cross-lane traffic inside the loop but the dot product's
// group sum), and a long context is split over workgroups whose fp32 (m, l, o) partials a second small launch combines.
#include "vy_attn_gen.h"
#include "vy_common.h"
#include "vy_qknorm.h"
#include "vy_wave.h"
#include <float.h>

namespace {

constexpr int PD_NW = 4;          // waves per workgroup
constexpr int PD_U = 4;           // keys per lane group and loop trip: 2 * U 16-byte loads in flight per lane
constexpr int PD_U_FP8 = 8;       // fp8 pages: a lane's 8 codes of a key are 8 bytes, so twice the keys keep the same bytes in flight
constexpr int PD_MAX_SPLIT = 32;
constexpr int PD_TARGET_WGS = 512;   // two workgroups per CU
constexpr float PF_LOG2E = 1.4426950408889634f;

struct PagedDecArgs {
  const void* q; long long q_ld; const int* q_rows;
  const void* kc; const void* vc;
  const int* bt; long long bt_stride; const int* seqlens;
  void* out; long long o_ld;
  float* ws_ml; float* ws_o;           // n_split > 1: [B][h][n_split]{m, l} and [B][h][n_split][dh]
  int h, hk, dh, R, lbs, max_blocks, n_split;
  float scale;
  const int* cu_q;                     // PF kernels only: first packed row of each sequence (n_seq + 1 entries)
  const float* ks; const float* vs;    // F8 kernels only: the scale of every (slot, KV head), [max_blocks << lbs][hk]
};

// 8 e4m3fn codes (two dwords) -> fp32, exact: v_cvt_pk_f32_fp8 on either half of a dword
__device__ __forceinline__ void fp8x8_unpack(const u32x2& t, float* v) {
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)t[w], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)t[w], true);
    v[4 * w] = lo[0]; v[4 * w + 1] = lo[1]; v[4 * w + 2] = hi[0]; v[4 * w + 3] = hi[1];
  }
}

// lane = (key group g, 16-byte chunk ch of the head): LPK lanes per key (the chunks of the head, rounded up to a power of
// two: lanes past the head's last chunk idle), KPW = 64 / LPK keys per wave instruction.  A wave takes CK = U * KPW
// CONSECUTIVE keys per trip, aligned to CK: KPW divides every block_size (>= 8), so the keys of one wave instruction sit
// in one page and the block-table entry is wave-uniform (a scalar load); where the whole trip sits in one page
// (block_size >= CK) it is loaded once for the trip.  RT query heads per workgroup (R rounded up to 1, 2, 4 or 8; the
// heads past R compute on head 0's query and store nothing).
// PF (the fp32 path of vy_attn_paged_prefill): row blockIdx.y of sequence blockIdx.z's query segment is a single-query
// problem -- packed row cu_q[z] + y, keys [0, ctx[z] + y + 1) with seqlens = the context lengths -- and is never split.
// F8 (vy_attn_paged_decode_fp8, T = bf16): the pages hold e4m3fn codes and a scale per (slot, KV head).  The lane mapping
// stays -- a lane's chunk is its 8 codes of the key, an 8-byte load -- with PD_U_FP8 keys per trip requested together
// and worked off PD_U at a time, so the live fp32 values are those of the bf16 kernel.  The codes are exact in fp32:
// score = (scale * k_s) * (q . codes); v_s is folded into the weight of the accumulate, not into l.  The scale of a
// key is read at the row the codes are read at, so never at or past k1 either.
template <typename T, int LPK, int RT, bool PF = false, bool F8 = false>
__global__ __launch_bounds__(64 * PD_NW) void paged_dec_kernel(const PagedDecArgs p) {
  using CH = Chunk<T>;
  using Raw = typename CH::Raw;
  using KRaw = std::conditional_t<F8, u32x2, Raw>;    // a lane's chunk of a key row as it sits in the pages
  using KT = std::conditional_t<F8, unsigned char, T>;
  constexpr int VEC = CH::VEC, NW = PD_NW, U = F8 ? PD_U_FP8 : PD_U, UC = PD_U, KPW = 64 / LPK, CK = U * KPW, DHP = LPK * VEC;
  static_assert(!F8 || (std::is_same<T, bf16>::value && !PF), "fp8 pages: bf16 queries, decode only");
  __shared__ float red_m[RT][NW], red_l[RT][NW];
  __shared__ float red_o[RT][NW][DHP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z, split = PF ? 0 : (int)blockIdx.y;
  const int ngrp = (p.R + RT - 1) / RT;
  const int kvh = (int)blockIdx.x / ngrp, r0 = ((int)blockIdx.x - kvh * ngrp) * RT;
  const int nr = p.R - r0 < RT ? p.R - r0 : RT;
  const int head0 = kvh * p.R + r0;
  const int g = lane / LPK, ch = lane % LPK;
  const int nch = p.dh / VEC;
  const bool lane_on = ch < nch;
  const int chc = lane_on ? ch : nch - 1;
  const int bs = 1 << p.lbs;
  int S = p.seqlens[b];
  const long long cap = p.bt_stride << p.lbs;       // keys the row of the block table can name
  long long qr;
  if constexpr (PF) {
    const int row0 = p.cu_q[b], i = (int)blockIdx.y;
    if (i >= p.cu_q[b + 1] - row0) return;          // (the whole workgroup, before any barrier)
    const long long Sl = (long long)(S < 0 ? 0 : S) + i + 1;
    S = Sl > cap ? (int)cap : (int)Sl;
    qr = (long long)row0 + i;
  } else {
    if (S > cap) S = (int)cap;
    qr = p.q_rows ? p.q_rows[b] : b;
  }
  // this workgroup's keys [k0, k1): equal shares of the sequence, rounded up to whole trips
  const int per = ((S + p.n_split - 1) / p.n_split + NW * CK - 1) / (NW * CK) * (NW * CK);
  const int k0 = split * per;
  const int k1 = k0 + per < S ? k0 + per : S;

  const T* qb = (const T*)p.q + qr * p.q_ld + chc * VEC;
  Raw q8[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) q8[r] = *reinterpret_cast<const Raw*>(qb + (long long)(head0 + (r < nr ? r : 0)) * p.dh);
  const int* bt = p.bt + (long long)b * p.bt_stride;
  const KT* kc = (const KT*)p.kc + (long long)kvh * p.dh + chc * VEC;
  const KT* vc = (const KT*)p.vc + (long long)kvh * p.dh + chc * VEC;
  const long long row_stride = (long long)p.hk * p.dh;

  float m[RT], l[RT], acc[RT][VEC];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    m[r] = -FLT_MAX; l[r] = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[r][e] = 0.f;
  }
  if (k0 < k1) {
    // the last wave instruction that holds a key of the range: later ones re-read its rows (never a row >= k1, never
    // a block-table entry past the sequence's pages) and are masked
    const int last_pb = (k1 - 1) & ~(KPW - 1);
    for (int base = k0 + wave * CK; base < k1; base += NW * CK) {
      int pbc[U], blk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) pbc[u] = base + u * KPW < last_pb ? base + u * KPW : last_pb;
      if ((pbc[0] >> p.lbs) == (pbc[U - 1] >> p.lbs)) {
        const int e = bt[pbc[0] >> p.lbs];
#pragma unroll
        for (int u = 0; u < U; ++u) blk[u] = e;
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) blk[u] = bt[pbc[u] >> p.lbs];
      }
      KRaw kr[U], vr[U];
      float ksc[U], vsc[U];                 // F8 only
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = blk[u] < 0 ? 0 : blk[u] < p.max_blocks ? blk[u] : p.max_blocks - 1;   // memory safety only
        const int j = pbc[u] + g < k1 ? pbc[u] + g : k1 - 1;
        const long long slot = ((long long)e << p.lbs) + (j & (bs - 1));
        const long long off = slot * row_stride;
        kr[u] = *reinterpret_cast<const KRaw*>(kc + off);
        vr[u] = *reinterpret_cast<const KRaw*>(vc + off);
        if constexpr (F8) {
          ksc[u] = p.ks[slot * p.hk + kvh] * p.scale;
          vsc[u] = p.vs[slot * p.hk + kvh];
        }
      }
#pragma unroll
      for (int u0 = 0; u0 < U; u0 += UC) {   // (one pass unless F8)
        float kf[UC][VEC], vf[UC][VEC];
        bool ok[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u) {
          if constexpr (F8) {
            fp8x8_unpack(kr[u0 + u], kf[u]);
            fp8x8_unpack(vr[u0 + u], vf[u]);
          } else {
            CH::unpack(kr[u0 + u], kf[u]);
            CH::unpack(vr[u0 + u], vf[u]);
          }
          ok[u] = base + (u0 + u) * KPW + g < k1;
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          float qf[VEC];
          CH::unpack(q8[r], qf);
          float sc[UC], mx = m[r];
#pragma unroll
          for (int u = 0; u < UC; ++u) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) d = fmaf(qf[e], kf[u][e], d);
            if constexpr (F8) d = dec_group_sum<LPK>(lane_on ? d : 0.f) * ksc[u0 + u];
            else d = dec_group_sum<LPK>(lane_on ? d : 0.f) * p.scale;
            sc[u] = ok[u] ? d : -FLT_MAX;
            mx = fmaxf(mx, sc[u]);
          }
          const float alpha = __expf(m[r] - mx);
          m[r] = mx;
          l[r] *= alpha;
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[r][e] *= alpha;
#pragma unroll
          for (int u = 0; u < UC; ++u) {
            const float pv = ok[u] ? __expf(sc[u] - mx) : 0.f;
            l[r] += pv;
            const float pw = F8 ? (ok[u] ? pv * vsc[u0 + u] : 0.f) : pv;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[r][e] = fmaf(pw, vf[u][e], acc[r][e]);
          }
        }
      }
    }
  }
  // the lane groups of the workgroup to one (m, l, o) per head: maximum over the waves, every group rescaled to it
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const float mw = dec_wave_max(m[r]);
    if (lane == 0) red_m[r][wave] = mw;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    float M = red_m[r][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) M = fmaxf(M, red_m[r][w]);
    const float f = __expf(m[r] - M);     // (a group without keys: l = 0 and o = 0, whatever f is)
    const float lw = dec_wave_sum(ch == 0 ? l[r] * f : 0.f);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[r][e] = dec_stride_sum<LPK>(acc[r][e] * f);
    if (lane == 0) red_l[r][wave] = lw;
    if (g == 0) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) red_o[r][wave][ch * VEC + e] = acc[r][e];
    }
  }
  __syncthreads();
  for (int t = tid; t < nr * p.dh; t += 64 * NW) {
    const int r = t / p.dh, c = t - r * p.dh;
    float M = red_m[r][0], L = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) { M = fmaxf(M, red_m[r][w]); L += red_l[r][w]; o += red_o[r][w][c]; }
    const int head = head0 + r;
    if (p.n_split == 1) {
      VyT<T>::st((T*)p.out + qr * p.o_ld + (long long)head * p.dh + c, L > 0.f ? o / L : 0.f);   // seqlen 0: zeros
    } else {
      const long long idx = ((long long)b * p.h + head) * p.n_split + split;
      p.ws_o[idx * p.dh + c] = o;
      if (c == 0) { p.ws_ml[idx * 2] = M; p.ws_ml[idx * 2 + 1] = L; }
    }
  }
}

// out[b][head] = sum_s o_s e^(m_s - M) / sum_s l_s e^(m_s - M): one workgroup per (head, sequence)
template <typename T>
__global__ __launch_bounds__(64) void paged_combine_kernel(const float* __restrict__ ws_ml, const float* __restrict__ ws_o,
                                                           T* __restrict__ out, long long o_ld,
                                                           const int* __restrict__ q_rows, int n_split, int h, int dh) {
  const int head = blockIdx.x, b = blockIdx.y;
  const long long idx0 = ((long long)b * h + head) * n_split;
  const long long qr = q_rows ? q_rows[b] : b;
  float M = -FLT_MAX;
  for (int s = 0; s < n_split; ++s) M = fmaxf(M, ws_ml[(idx0 + s) * 2]);
  for (int c = threadIdx.x; c < dh; c += 64) {
    float L = 0.f, o = 0.f;
    for (int s = 0; s < n_split; ++s) {
      const float f = __expf(ws_ml[(idx0 + s) * 2] - M);
      L += ws_ml[(idx0 + s) * 2 + 1] * f;
      o += ws_o[(idx0 + s) * dh + c] * f;
    }
    VyT<T>::st(out + qr * o_ld + (long long)head * dh + c, L > 0.f ? o / L : 0.f);
  }
}

// What follows the rotation in both rope-write kernels: the lane holds columns i4 .. i4 + 3 of the lower half (lo) and
// the same 4 of the upper half (hi) of head hd of token t's packed row; k and v heads go into slot slots[t] of the pages
// (k: rounded exactly as the in-place store rounds them; v: the loaded bits).
template <typename T>
__device__ __forceinline__ void page_store_quads(const float (&lo)[4], const float (&hi)[4], int i4, int hd, long long t,
                                                 const long long* __restrict__ slots, T* __restrict__ kc,
                                                 T* __restrict__ vc, long long n_slots, int h, int hk, int dh) {
  if (hd < h) return;
  const long long slot = slots[t];
  if (slot < 0 || slot >= n_slots) return;
  const bool isk = hd < h + hk;
  T* dst = (isk ? kc : vc) + (slot * hk + (isk ? hd - h : hd - h - hk)) * dh;
  Quad<T>::store(dst + i4, lo);
  Quad<T>::store(dst + (dh >> 1) + i4, hi);
}

// row positions[t] of the tables, clamped into them (memory safety only)
__device__ __forceinline__ long long table_pos(const int* __restrict__ positions, long long t, long long table_rows) {
  const long long pos = positions[t];
  return pos < 0 ? 0 : pos < table_rows ? pos : table_rows - 1;
}

// thread = (token, head of the packed row, 4 columns of the lower half and the same 4 of the upper half)
template <typename T>
__global__ __launch_bounds__(256) void paged_rope_write_kernel(T* __restrict__ qkv, long long ld,
                                                               const int* __restrict__ positions,
                                                               const long long* __restrict__ slots,
                                                               const float* __restrict__ cos_tab,
                                                               const float* __restrict__ sin_tab, long long table_rows,
                                                               T* __restrict__ kc, T* __restrict__ vc, long long n_slots,
                                                               long long total, int h, int hk, int dh) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int half = dh >> 1, qn = half >> 2, H3 = h + 2 * hk;
  const int i4 = (int)(idx % qn) * 4;
  const long long rest = idx / qn;
  const int hd = (int)(rest % H3);
  const long long t = rest / H3;
  T* row = qkv + t * ld + (long long)hd * dh;
  float lo[4], hi[4];
  Quad<T>::load(row + i4, lo);
  Quad<T>::load(row + half + i4, hi);
  if (hd < h + hk) {   // q and k heads: the pairing d, d + dh/2 and the formula of rope2_kernel (vy_misc.hip), in fp32, one rounding
    rope_rotate_quads(lo, hi, cos_tab, sin_tab, table_pos(positions, t, table_rows), half, i4);
    Quad<T>::store(row + i4, lo);
    Quad<T>::store(row + half + i4, hi);
  }
  page_store_quads(lo, hi, i4, hd, t, slots, kc, vc, n_slots, h, hk, dh);
}

// paged_rope_write_kernel with the per-head RMSNorm of q and k in front of the rotation (Qwen3's qk_norm).  A (token,
// head) unit is a group of 1 << lg lanes -- the head's dh / 8 column pairs of the mapping above, rounded up to a power of
// two, so a group never straddles a wave; the surplus lanes (4 of 16 at dh = 96, 4 of 32 at dh = 224) and the lanes past
// the last unit load nothing, take part in the reduction with zeros and store nothing.  Per q / k head, all in fp32:
// sum of squares (8 per lane as an fma chain, then the group sum), r = rsqrt(sum / dh + eps), n = x * r * scale, the
// rotation of n, ONE rounding at the store.  An all-zero head gives 0 * rsqrt(eps) = 0.  v heads are neither normalised
// nor rotated; they go through the page store as they were loaded.
template <typename T>
__global__ __launch_bounds__(256) void paged_qknorm_rope_write_kernel(T* __restrict__ qkv, long long ld,
                                                                      const int* __restrict__ positions,
                                                                      const long long* __restrict__ slots,
                                                                      const float* __restrict__ cos_tab,
                                                                      const float* __restrict__ sin_tab, long long table_rows,
                                                                      const float* __restrict__ q_scale,
                                                                      const float* __restrict__ k_scale, float eps,
                                                                      float inv_dh, T* __restrict__ kc, T* __restrict__ vc,
                                                                      long long n_slots, long long units, int lg, int h,
                                                                      int hk, int dh) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int half = dh >> 1, qn = half >> 2, H3 = h + 2 * hk;
  const long long unit = idx >> lg;
  const int ch = (int)(idx & ((1 << lg) - 1));
  const bool on = unit < units && ch < qn;
  const long long uc = on ? unit : 0;                 // (an idle lane computes on unit 0's indices and touches no memory)
  const int i4 = on ? ch * 4 : 0;
  const int hd = (int)(uc % H3);
  const long long t = uc / H3;
  T* row = qkv + t * ld + (long long)hd * dh;
  float lo[4] = {0.f, 0.f, 0.f, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    Quad<T>::load(row + i4, lo);
    Quad<T>::load(row + half + i4, hi);
  }
  const float ss = qk_group_sumsq(lo, hi, lg);        // every lane of the wave, also the idle ones
  if (!on) return;
  if (hd < h + hk) {
    qknorm_rope_quads(lo, hi, ss, inv_dh, eps, hd < h ? q_scale : k_scale, cos_tab, sin_tab,
                      table_pos(positions, t, table_rows), half, i4);
    Quad<T>::store(row + i4, lo);
    Quad<T>::store(row + half + i4, hi);
  }
  page_store_quads(lo, hi, i4, hd, t, slots, kc, vc, n_slots, h, hk, dh);
}

// The second launch of vy_paged_rope_write_fp8 (bf16 rows).  The first is the bf16 kernel above -- the plain one or the
// qk-norm one -- with no page to store to (n_slots = 0), so the in-place rows ARE that entry point's: hipcc contracts
// a * c - b * s into an fma for some elements and not for others, differently from kernel to kernel, and a rotation
// written out a second time next to the quantisation would not give the same bits.  This kernel then reads what a bf16
// page would hold -- the rotated k heads in place, the v heads as they came -- and applies the rule of
// include/vyom_hip.h.  A (token, k or v head) unit is a group of 1 << lg lanes, the head's dh / 8 16-byte chunks rounded
// up to a power of two as in paged_qknorm_rope_write_kernel: surplus lanes and lanes past the last unit load nothing,
// reach the maximum with zeros and store nothing.  Per head: amax over the group, s = amax / 448 (1 for an all-zero
// head), an IEEE fp32 division per element, the clamp, v_cvt_pk_fp8_f32 (round to nearest even); the lane's 8 codes are
// one 8-byte store, lane 0 of the unit stores the scale.
__global__ __launch_bounds__(256) void paged_quant_write_fp8_kernel(const bf16* __restrict__ qkv, long long ld,
                                                                    const long long* __restrict__ slots,
                                                                    unsigned char* __restrict__ kc,
                                                                    unsigned char* __restrict__ vc, float* __restrict__ ksc,
                                                                    float* __restrict__ vsc, long long n_slots,
                                                                    long long units, int lg, int h, int hk, int dh) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long unit = idx >> lg;
  const int ch = (int)(idx & ((1 << lg) - 1));
  const bool on = unit < units && ch * 8 < dh;
  const long long uc = on ? unit : 0;                 // (an idle lane computes on unit 0's indices and touches no memory)
  const int hd = (int)(uc % (2 * hk));                // k heads, then v heads
  const long long t = uc / (2 * hk);
  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (on) Chunk<bf16>::load(qkv + t * ld + (long long)(h + hd) * dh + ch * 8, x);
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(x[e]));
  amax = pow2_group_max(amax, lg);                    // every lane of the wave, also the idle ones
  if (!on) return;
  const long long slot = slots[t];
  if (slot < 0 || slot >= n_slots) return;
  const bool isk = hd < hk;
  const long long head = slot * hk + (isk ? hd : hd - hk);
  const float s = amax > 0.f ? amax / 448.0f : 1.0f;
  float c[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) c[e] = fminf(fmaxf(x[e] / s, -448.0f), 448.0f);
  u32x2 w;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    int d = __builtin_amdgcn_cvt_pk_fp8_f32(c[4 * k], c[4 * k + 1], 0, false);
    d = __builtin_amdgcn_cvt_pk_fp8_f32(c[4 * k + 2], c[4 * k + 3], d, true);
    w[k] = (unsigned)d;
  }
  *reinterpret_cast<u32x2*>((isk ? kc : vc) + head * dh + ch * 8) = w;
  if (ch == 0) (isk ? ksc : vsc)[head] = s;
}

// thread = (K or V, key j, KV head, 16-byte chunk): out[kvh][j] = cache[block_table[j / block_size]][j % block_size][kvh]
template <typename T>
__global__ __launch_bounds__(256) void paged_gather_kernel(const T* __restrict__ kc, const T* __restrict__ vc,
                                                           const int* __restrict__ bt, T* __restrict__ ko,
                                                           T* __restrict__ vo, long long S, int lbs, int hk, int dh,
                                                           int max_blocks) {
  using CH = Chunk<T>;
  const int nch = dh / CH::VEC;
  const long long per = S * hk * nch;
  long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * per) return;
  const bool isv = idx >= per;
  if (isv) idx -= per;
  const int c = (int)(idx % nch);
  const long long rest = idx / nch;
  const int kvh = (int)(rest % hk);
  const long long j = rest / hk;
  const int blk = bt[j >> lbs];
  typename CH::Raw v = {};
  if (blk >= 0 && blk < max_blocks)
    v = *reinterpret_cast<const typename CH::Raw*>((isv ? vc : kc) + ((((long long)blk << lbs) + (j & ((1 << lbs) - 1))) * hk + kvh) * dh + c * CH::VEC);
  *reinterpret_cast<typename CH::Raw*>((isv ? vo : ko) + ((long long)kvh * S + j) * dh + c * CH::VEC) = v;
}

int log2_block_size(int block_size) {   // 8 .. 256, a power of two; else -1
  for (int l = 3; l <= 8; ++l)
    if (block_size == (1 << l)) return l;
  return -1;
}

// the page and head geometry every entry point of this file accepts; `fn` names the entry in the message
int paged_check_geometry(const char* fn, int block_size, int dh, int* lbs) {
  *lbs = log2_block_size(block_size);
  if (*lbs < 0) VY_FAIL(VY_ERR_ARG, "%s: block_size %d must be a power of two from 8 to 256", fn, block_size);
  if (dh <= 0 || dh % 8 || dh > 256) VY_FAIL(VY_ERR_ARG, "%s: dh %d must be a multiple of 8 up to 256", fn, dh);
  return VY_OK;
}

// the argument checks of the two rope-write entry points.  `null_operand`: one of the entry's pointers is null;
// `ptrs`: the entry's 16-byte-aligned pointers or-ed together; eps: vy_paged_rope_write has none and passes 0
int paged_check_rope_write(const char* fn, bool null_operand, uintptr_t ptrs, int64_t ld, int64_t table_rows, float eps,
                           int64_t max_blocks, int block_size, int64_t T, int h, int hk, int dh) {
  if (null_operand) VY_FAIL(VY_ERR_ARG, "%s: null operand", fn);
  int lbs;
  if (const int rc = paged_check_geometry(fn, block_size, dh, &lbs)) return rc;
  if (T <= 0 || h <= 0 || hk <= 0 || max_blocks <= 0 || table_rows <= 0 || ld < (int64_t)(h + 2 * hk) * dh)
    VY_FAIL(VY_ERR_ARG, "%s: bad shape (T %lld, h %d, hk %d, ld %lld)", fn, (long long)T, h, hk, (long long)ld);
  if (!(eps >= 0.f)) VY_FAIL(VY_ERR_ARG, "%s: eps %g must not be negative", fn, (double)eps);
  if (ld % 4 || (ptrs & 15)) VY_FAIL(VY_ERR_ARG, "%s: ld must be a multiple of 4, operands 16-byte aligned", fn);
  return VY_OK;
}

// lanes per key for a head width: the head's 16-byte chunks rounded up to a power of two, at least 8
int pd_lpk(int dh, int dtype) {
  const int nch = dh / (dtype == VY_BF16 ? 8 : 4);
  int lpk = 8;
  while (lpk < nch) lpk *= 2;
  return lpk;
}
int pd_rt(int R) { return R > 4 ? 8 : R > 2 ? 4 : R; }

// workgroups over the context.  A split costs a second, dependent launch: at 512-640 keys it added 1-5 us to a 10-12 us
// unsplit call and never paid; at 4096 keys (dh = 128, 64 workgroups unsplit) it takes 68 us to 28-29 us (DESIGN.md,
// "Paged KV cache": the table of tools/bench_paged.py --splits).  So only a context of 16 loop trips or more is split:
// towards two workgroups per CU, at least 8 trips each.
int pd_splits(int64_t B, int h, int hk, int dh, int64_t max_seqlen, int n_split, int dtype, int U = PD_U) {
  if (n_split > 0) return n_split < PD_MAX_SPLIT ? n_split : PD_MAX_SPLIT;
  const int R = h / hk, rt = pd_rt(R);
  const int64_t wgs = B * hk * ((R + rt - 1) / rt);
  const int64_t trip = (int64_t)PD_NW * U * (64 / pd_lpk(dh, dtype));
  if (max_seqlen < 16 * trip) return 1;
  int64_t ns = PD_TARGET_WGS / wgs;
  if (ns > max_seqlen / (8 * trip)) ns = max_seqlen / (8 * trip);
  if (ns > PD_MAX_SPLIT) ns = PD_MAX_SPLIT;
  return ns < 1 ? 1 : (int)ns;
}

template <typename T, int LPK, bool F8 = false>
void paged_dec_launch(const PagedDecArgs& a, int64_t B, hipStream_t st) {
  const int rt = pd_rt(a.R);
  const dim3 grid((unsigned)(a.hk * ((a.R + rt - 1) / rt)), (unsigned)a.n_split, (unsigned)B), block(64 * PD_NW);
  if (rt == 1) hipLaunchKernelGGL((paged_dec_kernel<T, LPK, 1, false, F8>), grid, block, 0, st, a);
  else if (rt == 2) hipLaunchKernelGGL((paged_dec_kernel<T, LPK, 2, false, F8>), grid, block, 0, st, a);
  else if (rt == 4) hipLaunchKernelGGL((paged_dec_kernel<T, LPK, 4, false, F8>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((paged_dec_kernel<T, LPK, 8, false, F8>), grid, block, 0, st, a);
}

// ------------------------------------------------------------------------------------------
// vy_attn_paged_prefill, bf16: the 16x16x32 tile core of vy_attn_gen.h (64 query rows per workgroup, 16 per wave,
// register-staged 64-key tiles, the swapped QK^T, P in registers, V^T through ds_read_b64_tr_b16), which
// attn_fwd_gen_kernel (vy_attn.hip) runs over contiguous K/V, over packed variable-length query segments.  The Q
// fragments, the tile store, one tile's step and the epilogue store are AttnGen<DHP>'s.  This kernel owns:
//   * the fetch: key kj of sequence s is row table[s][kj / bs] * bs + kj % bs of the pages.  The registers of tile
//     t + 1 are requested right after tile t has been stored to LDS, so the two dependent loads (table entry, then the
//     row) fly under tile t's MFMAs and softmax -- there is no LDS-DMA ring here that an ordinary load would drain
//     (vy_attn_tile.h, fact (2));
//   * the predicate: always causal at offset ctx[s], and every row sees its own key -- so there is no key padding and
//     no row without a visible key;
//   * key rows at or past ctx + len are staged as zeros, never read: the tail of a last page may hold anything and
//     0 * NaN in the PV MFMA is NaN.
// F8 (vy_attn_paged_prefill_fp8): the fetch requests a chunk's 8 codes and its slot's scale instead of 8 bf16; they stay
// as they came until the tile is stored, where each value becomes bf16_rne(float(code) * s) -- the requests still fly
// under the previous tile's step.  A chunk that is staged as zeros has codes 0 and scale 0.  The core sees a bf16 tile.
// ------------------------------------------------------------------------------------------
struct PagedPfArgs {
  const bf16* q; long long q_ld;
  const void* kc; const void* vc;
  const int* bt; long long bt_stride;
  const int* cu_q; const int* ctx;
  bf16* out; long long o_ld;
  int h, hk, dh, lbs, max_blocks;
  float scale;
  const float* ks; const float* vs;    // F8 only: [max_blocks << lbs][hk]
};

__device__ __forceinline__ bf16x8 fp8x8_dequant_bf16(const u32x2& codes, float s) {
  float f[8];
  fp8x8_unpack(codes, f);
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (bf16)(f[e] * s);
  return r;
}

template <int DHP, bool F8 = false>
__global__ __launch_bounds__(256) void paged_prefill_kernel(const PagedPfArgs p) {
  using G = AttnGen<DHP>;
  __shared__ __attribute__((aligned(16))) char smem[G::LDS_BYTES];
  char* kt = smem;
  char* vt = G::v_tile(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  // heads on x (whole heads per XCD, vy_attn.hip), long rows first
  const int head = (int)blockIdx.x % p.h, s = (int)blockIdx.x / p.h;
  const int kvh = head / (p.h / p.hk);
  const int q0 = ((int)gridDim.y - 1 - (int)blockIdx.y) * 64;
  const int row0 = p.cu_q[s], len = p.cu_q[s + 1] - row0;
  if (q0 >= len) return;                     // (the whole workgroup, before the first barrier)
  const int cap = (int)(p.bt_stride << p.lbs);        // keys the row of the block table can name (<= 2^30)
  int ctx = p.ctx[s];
  ctx = ctx < 0 ? 0 : ctx < cap ? ctx : cap;          // memory safety only
  const int S = len < cap - ctx ? ctx + len : cap;
  const int dh = p.dh, bs = 1 << p.lbs;
  const int qi = q0 + wave * 16 + r16;
  const int qrow = qi < len ? qi : len - 1;
  const bf16* Q = p.q + ((long long)row0 + qrow) * p.q_ld + (long long)head * dh;
  const int* bt = p.bt + (long long)s * p.bt_stride;
  const long long row_stride = (long long)p.hk * dh;
  using KT = std::conditional_t<F8, unsigned char, bf16>;
  const KT* Kb = (const KT*)p.kc + (long long)kvh * dh;
  const KT* Vb = (const KT*)p.vc + (long long)kvh * dh;

  bf16x8 qf[G::KS];
  G::load_q(qf, Q, dh, kq);
  f32x4 o[G::NDB];
#pragma unroll
  for (int n = 0; n < G::NDB; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -FLT_MAX, l_run = 0.f;
  const float c = p.scale * PF_LOG2E;
  const int kv_end = S < ctx + q0 + 64 ? S : ctx + q0 + 64;
  const int nt = (kv_end + 63) / 64;         // >= 1: S >= 1
  const unsigned vtr = G::vtr_addr(vt, r16, kq);

  // the tile's 16-byte chunks -> registers: zero beyond the head width and at or beyond key S
  bf16x8 kreg[G::CPT], vreg[G::CPT];
  u32x2 kq8[G::CPT], vq8[G::CPT];            // F8 only: the codes and scales as fetched
  float ksc[G::CPT], vsc[G::CPT];
  auto fetch = [&](int k0) {
    int ent[G::CPT];
#pragma unroll
    for (int i = 0; i < G::CPT; ++i) {
      const int kj = k0 + (tid + 256 * i) / G::CPRW;
      ent[i] = bt[(kj < S ? kj : S - 1) >> p.lbs];
    }
#pragma unroll
    for (int i = 0; i < G::CPT; ++i) {
      int row, ch;
      G::chunk_of(tid, i, row, ch);
      const int kj = k0 + row;
      const bool ok = ch * 8 < dh && kj < S;
      const int kjc = kj < S ? kj : S - 1;
      const int e = ent[i] < 0 ? 0 : ent[i] < p.max_blocks ? ent[i] : p.max_blocks - 1;   // memory safety only
      const long long slot = ((long long)e << p.lbs) + (kjc & (bs - 1));
      const long long off = slot * row_stride + (ch * 8 < dh ? ch * 8 : 0);
      if constexpr (F8) {
        kq8[i] = ok ? *reinterpret_cast<const u32x2*>(Kb + off) : u32x2{0u, 0u};
        vq8[i] = ok ? *reinterpret_cast<const u32x2*>(Vb + off) : u32x2{0u, 0u};
        ksc[i] = ok ? p.ks[slot * p.hk + kvh] : 0.f;
        vsc[i] = ok ? p.vs[slot * p.hk + kvh] : 0.f;
      } else {
        kreg[i] = ok ? *reinterpret_cast<const bf16x8*>(Kb + off) : G::zero8();
        vreg[i] = ok ? *reinterpret_cast<const bf16x8*>(Vb + off) : G::zero8();
      }
    }
  };
  fetch(0);

  for (int t = 0; t < nt; ++t) {
    const int k0 = t * 64;
    __syncthreads();   // the previous tile's fragments have been read
    if constexpr (F8) {
#pragma unroll
      for (int i = 0; i < G::CPT; ++i) {
        kreg[i] = fp8x8_dequant_bf16(kq8[i], ksc[i]);
        vreg[i] = fp8x8_dequant_bf16(vq8[i], vsc[i]);
      }
    }
    G::store_tile(kt, vt, kreg, vreg, tid);
    __syncthreads();
    if (t + 1 < nt) fetch(k0 + 64);
    // (& and not &&: both compares of every key are evaluated, nothing short-circuits -- the form the compiler schedules best)
    G::step(kt, vtr, qf, o, m_run, l_run, c, k0, r16, kq, [&](int kj) { return (kj < S) & (kj <= qi + ctx); });
  }
  const float inv = 1.0f / dec_rows_sum(l_run);   // row totals over the four lane groups
  if (qi < len) G::store_row(p.out + ((long long)row0 + qi) * p.o_ld + (long long)head * dh, o, inv, dh, kq);
}

template <int LPK>
void paged_prefill_f32_launch(const PagedDecArgs& a, int64_t n_seq, int64_t max_q, hipStream_t st) {
  const int rt = pd_rt(a.R);
  const dim3 grid((unsigned)(a.hk * ((a.R + rt - 1) / rt)), (unsigned)max_q, (unsigned)n_seq), block(64 * PD_NW);
  if (rt == 1) hipLaunchKernelGGL((paged_dec_kernel<float, LPK, 1, true>), grid, block, 0, st, a);
  else if (rt == 2) hipLaunchKernelGGL((paged_dec_kernel<float, LPK, 2, true>), grid, block, 0, st, a);
  else if (rt == 4) hipLaunchKernelGGL((paged_dec_kernel<float, LPK, 4, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((paged_dec_kernel<float, LPK, 8, true>), grid, block, 0, st, a);
}

// vy_attn_paged_decode (fp8 = false, no scales) and vy_attn_paged_decode_fp8 behind one set of checks; `fn` names the entry
int paged_decode(const char* fn, bool fp8, const void* q, int64_t q_ld, const int32_t* q_rows, const void* k_cache,
                 const void* v_cache, const float* k_scale, const float* v_scale, int64_t max_blocks, int block_size,
                 const int32_t* block_table, int64_t bt_stride, const int32_t* seqlens, int64_t max_seqlen, void* out,
                 int64_t o_ld, int64_t B, int h, int hk, int dh, float scale, int n_split, void* ws, int64_t ws_bytes,
                 int dtype, void* stream) {
  if (!q || !k_cache || !v_cache || !block_table || !seqlens || !out || (fp8 && (!k_scale || !v_scale)))
    VY_FAIL(VY_ERR_ARG, "%s: null operand", fn);
  int lbs;
  if (const int rc = paged_check_geometry(fn, block_size, dh, &lbs)) return rc;
  if (dtype != VY_BF16 && (fp8 || dtype != VY_F32)) VY_FAIL(VY_ERR_ARG, "%s: bad dtype %d", fn, dtype);
  const int vec = dtype == VY_BF16 ? 8 : 4;
  if (B <= 0 || B > 65535 || h <= 0 || hk <= 0 || h % hk || max_blocks <= 0 || max_blocks > INT32_MAX || bt_stride <= 0 ||
      max_seqlen < 0 || max_seqlen > (1 << 30) || n_split < 0 || q_ld % vec || o_ld < (int64_t)h * dh)
    VY_FAIL(VY_ERR_ARG, "%s: bad shape (B %lld, h %d, hk %d, max_blocks %lld, bt_stride %lld, n_split %d)", fn,
            (long long)B, h, hk, (long long)max_blocks, (long long)bt_stride, n_split);
  if (((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) VY_FAIL(VY_ERR_ARG, "%s: q / caches must be 16-byte aligned", fn);
  int ns = pd_splits(B, h, hk, dh, max_seqlen, n_split, dtype, fp8 ? PD_U_FP8 : PD_U);
  const int64_t need = B * h * ns * (int64_t)(dh + 2) * 4;
  if (ns > 1 && (!ws || ws_bytes < need)) {
    if (n_split > 0) VY_FAIL(VY_ERR_ARG, "%s: n_split %d needs %lld bytes of workspace", fn, ns, (long long)need);
    ns = 1;   // automatic split without scratch: one workgroup per (sequence, KV head)
  }
  PagedDecArgs a{q, q_ld, q_rows, k_cache, v_cache, block_table, bt_stride, seqlens, out, o_ld,
                 (float*)ws, ws ? (float*)ws + B * h * ns * 2 : nullptr,
                 h, hk, dh, h / hk, lbs, (int)max_blocks, ns, scale, nullptr, k_scale, v_scale};
  hipStream_t st = (hipStream_t)stream;
  const int lpk = pd_lpk(dh, dtype);
  if (fp8) {
    if (lpk == 8) paged_dec_launch<bf16, 8, true>(a, B, st);
    else if (lpk == 16) paged_dec_launch<bf16, 16, true>(a, B, st);
    else paged_dec_launch<bf16, 32, true>(a, B, st);
  } else if (dtype == VY_BF16) {
    if (lpk == 8) paged_dec_launch<bf16, 8>(a, B, st);
    else if (lpk == 16) paged_dec_launch<bf16, 16>(a, B, st);
    else paged_dec_launch<bf16, 32>(a, B, st);
  } else {
    if (lpk == 8) paged_dec_launch<float, 8>(a, B, st);
    else if (lpk == 16) paged_dec_launch<float, 16>(a, B, st);
    else if (lpk == 32) paged_dec_launch<float, 32>(a, B, st);
    else paged_dec_launch<float, 64>(a, B, st);
  }
  VY_CHECK_LAUNCH(fn);
  if (ns > 1) {
    const dim3 grid((unsigned)h, (unsigned)B), block(64);
    if (dtype == VY_BF16)
      hipLaunchKernelGGL(paged_combine_kernel<bf16>, grid, block, 0, st, a.ws_ml, a.ws_o, (bf16*)out, o_ld, q_rows, ns, h, dh);
    else
      hipLaunchKernelGGL(paged_combine_kernel<float>, grid, block, 0, st, a.ws_ml, a.ws_o, (float*)out, o_ld, q_rows, ns, h, dh);
    VY_CHECK_LAUNCH(fn);
  }
  return VY_OK;
}

// vy_attn_paged_prefill (fp8 = false, no scales) and vy_attn_paged_prefill_fp8 behind one set of checks
int paged_prefill(const char* fn, bool fp8, const void* q, int64_t q_ld, const void* k_cache, const void* v_cache,
                  const float* k_scale, const float* v_scale, int64_t max_blocks, int block_size,
                  const int32_t* block_table, int64_t bt_stride, const int32_t* cu_q, const int32_t* ctx_lens,
                  int64_t n_seq, int64_t max_q, int64_t max_kv, void* out, int64_t o_ld, int h, int hk, int dh,
                  float scale, int dtype, void* stream) {
  // (no sequences: the three per-sequence arrays may be empty, i.e. null)
  if (!q || !k_cache || !v_cache || !out || (n_seq > 0 && (!block_table || !cu_q || !ctx_lens)) ||
      (fp8 && (!k_scale || !v_scale)))
    VY_FAIL(VY_ERR_ARG, "%s: null operand", fn);
  int lbs;
  if (const int rc = paged_check_geometry(fn, block_size, dh, &lbs)) return rc;
  if (dtype != VY_BF16 && (fp8 || dtype != VY_F32)) VY_FAIL(VY_ERR_ARG, "%s: bad dtype %d", fn, dtype);
  if (n_seq < 0 || n_seq > 65535 || h <= 0 || hk <= 0 || h % hk || max_blocks <= 0 || max_blocks > INT32_MAX || bt_stride <= 0 ||
      bt_stride > ((int64_t)1 << 30) / block_size || max_q < 0 || max_q > 65535 * 64 || max_kv < 0 || max_kv > (1 << 30) ||
      q_ld % (dtype == VY_BF16 ? 8 : 4) || q_ld < (int64_t)h * dh || (dtype == VY_BF16 && o_ld % 4) || o_ld < (int64_t)h * dh ||
      (int64_t)h * n_seq > INT32_MAX)
    VY_FAIL(VY_ERR_ARG, "%s: bad shape (n_seq %lld, max_q %lld, max_kv %lld, h %d, hk %d, max_blocks %lld, "
            "bt_stride %lld, q_ld %lld, o_ld %lld)", fn, (long long)n_seq, (long long)max_q, (long long)max_kv, h, hk,
            (long long)max_blocks, (long long)bt_stride, (long long)q_ld, (long long)o_ld);
  if ((((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) || (dtype == VY_BF16 && ((uintptr_t)out & 7)))
    VY_FAIL(VY_ERR_ARG, "%s: q / caches must be 16-byte aligned, out 8-byte aligned", fn);
  if (n_seq == 0 || max_q == 0) return VY_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VY_F32) {
    // the parity path: every row a single-query problem of the decode kernel, online softmax in fp32, one rounding
    if (max_q > 65535) VY_FAIL(VY_ERR_ARG, "%s: fp32 segments hold at most 65535 rows, max_q is %lld", fn, (long long)max_q);
    PagedDecArgs a{q, q_ld, nullptr, k_cache, v_cache, block_table, bt_stride, ctx_lens, out, o_ld, nullptr, nullptr,
                   h, hk, dh, h / hk, lbs, (int)max_blocks, 1, scale, cu_q};
    const int lpk = pd_lpk(dh, dtype);
    if (lpk == 8) paged_prefill_f32_launch<8>(a, n_seq, max_q, st);
    else if (lpk == 16) paged_prefill_f32_launch<16>(a, n_seq, max_q, st);
    else if (lpk == 32) paged_prefill_f32_launch<32>(a, n_seq, max_q, st);
    else paged_prefill_f32_launch<64>(a, n_seq, max_q, st);
  } else {
    const PagedPfArgs a{(const bf16*)q, q_ld, k_cache, v_cache, block_table, bt_stride, cu_q,
                        ctx_lens, (bf16*)out, o_ld, h, hk, dh, lbs, (int)max_blocks, scale, k_scale, v_scale};
    const dim3 grid((unsigned)(h * n_seq), (unsigned)vy_cdiv(max_q, 64)), block(256);
    if (fp8) {
      if (dh <= 64) hipLaunchKernelGGL((paged_prefill_kernel<64, true>), grid, block, 0, st, a);
      else if (dh <= 96) hipLaunchKernelGGL((paged_prefill_kernel<96, true>), grid, block, 0, st, a);
      else if (dh <= 128) hipLaunchKernelGGL((paged_prefill_kernel<128, true>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((paged_prefill_kernel<256, true>), grid, block, 0, st, a);
    } else if (dh <= 64) hipLaunchKernelGGL(paged_prefill_kernel<64>, grid, block, 0, st, a);
    else if (dh <= 96) hipLaunchKernelGGL(paged_prefill_kernel<96>, grid, block, 0, st, a);
    else if (dh <= 128) hipLaunchKernelGGL(paged_prefill_kernel<128>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(paged_prefill_kernel<256>, grid, block, 0, st, a);
  }
  VY_CHECK_LAUNCH(fn);
  return VY_OK;
}

int64_t paged_decode_ws_bytes(int64_t B, int h, int hk, int dh, int64_t max_seqlen, int n_split, int dtype, int U) {
  if (B <= 0 || h <= 0 || hk <= 0 || h % hk || dh <= 0 || dh % 8 || dh > 256 || n_split < 0) return 0;
  const int ns = pd_splits(B, h, hk, dh, max_seqlen, n_split, dtype, U);
  return ns == 1 ? 0 : B * h * ns * (int64_t)(dh + 2) * 4;
}

}  // namespace

extern "C" int64_t vy_attn_paged_decode_ws_bytes(int64_t B, int h, int hk, int dh, int64_t max_seqlen, int n_split,
                                                 int dtype) {
  return paged_decode_ws_bytes(B, h, hk, dh, max_seqlen, n_split, dtype, PD_U);
}

extern "C" int64_t vy_attn_paged_decode_fp8_ws_bytes(int64_t B, int h, int hk, int dh, int64_t max_seqlen, int n_split,
                                                     int dtype) {
  if (dtype != VY_BF16) return 0;
  return paged_decode_ws_bytes(B, h, hk, dh, max_seqlen, n_split, dtype, PD_U_FP8);
}

extern "C" int vy_attn_paged_decode(const void* q, int64_t q_ld, const int32_t* q_rows, const void* k_cache,
                                    const void* v_cache, int64_t max_blocks, int block_size,
                                    const int32_t* block_table, int64_t bt_stride, const int32_t* seqlens,
                                    int64_t max_seqlen, void* out, int64_t o_ld, int64_t B, int h, int hk, int dh,
                                    float scale, int n_split, void* ws, int64_t ws_bytes, int dtype, void* stream) {
  return paged_decode("vy_attn_paged_decode", false, q, q_ld, q_rows, k_cache, v_cache, nullptr, nullptr, max_blocks,
                      block_size, block_table, bt_stride, seqlens, max_seqlen, out, o_ld, B, h, hk, dh, scale, n_split, ws,
                      ws_bytes, dtype, stream);
}

extern "C" int vy_attn_paged_decode_fp8(const void* q, int64_t q_ld, const int32_t* q_rows, const void* k_cache,
                                        const void* v_cache, const float* k_scale, const float* v_scale,
                                        int64_t max_blocks, int block_size, const int32_t* block_table,
                                        int64_t bt_stride, const int32_t* seqlens, int64_t max_seqlen, void* out,
                                        int64_t o_ld, int64_t B, int h, int hk, int dh, float scale, int n_split,
                                        void* ws, int64_t ws_bytes, int dtype, void* stream) {
  return paged_decode("vy_attn_paged_decode_fp8", true, q, q_ld, q_rows, k_cache, v_cache, k_scale, v_scale, max_blocks,
                      block_size, block_table, bt_stride, seqlens, max_seqlen, out, o_ld, B, h, hk, dh, scale, n_split, ws,
                      ws_bytes, dtype, stream);
}

extern "C" int vy_attn_paged_prefill(const void* q, int64_t q_ld, const void* k_cache, const void* v_cache,
                                     int64_t max_blocks, int block_size, const int32_t* block_table, int64_t bt_stride,
                                     const int32_t* cu_q, const int32_t* ctx_lens, int64_t n_seq, int64_t max_q,
                                     int64_t max_kv, void* out, int64_t o_ld, int h, int hk, int dh, float scale,
                                     int dtype, void* stream) {
  return paged_prefill("vy_attn_paged_prefill", false, q, q_ld, k_cache, v_cache, nullptr, nullptr, max_blocks, block_size,
                       block_table, bt_stride, cu_q, ctx_lens, n_seq, max_q, max_kv, out, o_ld, h, hk, dh, scale, dtype,
                       stream);
}

extern "C" int vy_attn_paged_prefill_fp8(const void* q, int64_t q_ld, const void* k_cache, const void* v_cache,
                                         const float* k_scale, const float* v_scale, int64_t max_blocks, int block_size,
                                         const int32_t* block_table, int64_t bt_stride, const int32_t* cu_q,
                                         const int32_t* ctx_lens, int64_t n_seq, int64_t max_q, int64_t max_kv, void* out,
                                         int64_t o_ld, int h, int hk, int dh, float scale, int dtype, void* stream) {
  return paged_prefill("vy_attn_paged_prefill_fp8", true, q, q_ld, k_cache, v_cache, k_scale, v_scale, max_blocks,
                       block_size, block_table, bt_stride, cu_q, ctx_lens, n_seq, max_q, max_kv, out, o_ld, h, hk, dh,
                       scale, dtype, stream);
}

extern "C" int vy_paged_rope_write_fp8(void* qkv, int64_t ld, const int32_t* positions, const int64_t* slot_mapping,
                                       const float* cos_tab, const float* sin_tab, int64_t table_rows,
                                       const float* q_scale, const float* k_norm_scale, float eps, void* k_cache,
                                       void* v_cache, float* k_scale, float* v_scale, int64_t max_blocks,
                                       int block_size, int64_t T, int h, int hk, int dh, int dtype, void* stream) {
  if (const int rc = paged_check_rope_write(
          "vy_paged_rope_write_fp8",
          !qkv || !positions || !slot_mapping || !cos_tab || !sin_tab || !k_cache || !v_cache || !k_scale || !v_scale ||
              !q_scale != !k_norm_scale,
          (uintptr_t)cos_tab | (uintptr_t)sin_tab | (uintptr_t)q_scale | (uintptr_t)k_norm_scale | (uintptr_t)qkv |
              (uintptr_t)k_cache | (uintptr_t)v_cache,
          ld, table_rows, eps, max_blocks, block_size, T, h, hk, dh))
    return rc;
  if (dtype != VY_BF16) VY_FAIL(VY_ERR_ARG, "vy_paged_rope_write_fp8: bad dtype %d (bf16 rows only)", dtype);
  int lg = 0;                                         // lanes per (token, head): dh / 8 rounded up to a power of two
  while ((1 << lg) < dh / 8) ++lg;
  const int64_t blocks = vy_cdiv((T * (h + 2 * hk)) << lg, 256);
  if (blocks > INT32_MAX) VY_FAIL(VY_ERR_ARG, "vy_paged_rope_write_fp8: T %lld is more than one launch holds", (long long)T);
  hipStream_t st = (hipStream_t)stream;
  // the in-place rows: the bf16 entry point's own kernel, with no slot in range
  if (q_scale)
    hipLaunchKernelGGL(paged_qknorm_rope_write_kernel<bf16>, dim3((unsigned)blocks), dim3(256), 0, st, (bf16*)qkv, ld, positions,
                       (const long long*)slot_mapping, cos_tab, sin_tab, table_rows, q_scale, k_norm_scale, eps,
                       1.0f / (float)dh, (bf16*)nullptr, (bf16*)nullptr, (long long)0, (long long)(T * (h + 2 * hk)), lg, h, hk, dh);
  else {
    const int64_t total = T * (h + 2 * hk) * (dh / 8);
    hipLaunchKernelGGL(paged_rope_write_kernel<bf16>, dim3((unsigned)vy_cdiv(total, 256)), dim3(256), 0, st, (bf16*)qkv, ld,
                       positions, (const long long*)slot_mapping, cos_tab, sin_tab, table_rows, (bf16*)nullptr,
                       (bf16*)nullptr, (long long)0, (long long)total, h, hk, dh);
  }
  VY_CHECK_LAUNCH("vy_paged_rope_write_fp8 (rotation)");
  const int64_t units = T * 2 * hk;
  hipLaunchKernelGGL(paged_quant_write_fp8_kernel, dim3((unsigned)vy_cdiv(units << lg, 256)), dim3(256), 0, st,
                     (const bf16*)qkv, ld, (const long long*)slot_mapping, (unsigned char*)k_cache, (unsigned char*)v_cache,
                     k_scale, v_scale, (long long)(max_blocks * block_size), (long long)units, lg, h, hk, dh);
  VY_CHECK_LAUNCH("vy_paged_rope_write_fp8");
  return VY_OK;
}

extern "C" int vy_paged_rope_write(void* qkv, int64_t ld, const int32_t* positions, const int64_t* slot_mapping,
                                   const float* cos_tab, const float* sin_tab, int64_t table_rows, void* k_cache,
                                   void* v_cache, int64_t max_blocks, int block_size, int64_t T, int h, int hk, int dh,
                                   int dtype, void* stream) {
  if (const int rc = paged_check_rope_write(
          "vy_paged_rope_write", !qkv || !positions || !slot_mapping || !cos_tab || !sin_tab || !k_cache || !v_cache,
          (uintptr_t)cos_tab | (uintptr_t)sin_tab | (uintptr_t)qkv | (uintptr_t)k_cache | (uintptr_t)v_cache, ld, table_rows,
          0.f, max_blocks, block_size, T, h, hk, dh))
    return rc;
  const int64_t total = T * (h + 2 * hk) * (dh / 8);
  const dim3 grid((unsigned)vy_cdiv(total, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_slots = max_blocks * block_size;
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(paged_rope_write_kernel<bf16>, grid, block, 0, st, (bf16*)qkv, ld, positions,
                       (const long long*)slot_mapping, cos_tab, sin_tab, table_rows, (bf16*)k_cache, (bf16*)v_cache, n_slots,
                       total, h, hk, dh);
  else if (dtype == VY_F32)
    hipLaunchKernelGGL(paged_rope_write_kernel<float>, grid, block, 0, st, (float*)qkv, ld, positions,
                       (const long long*)slot_mapping, cos_tab, sin_tab, table_rows, (float*)k_cache, (float*)v_cache,
                       n_slots, total, h, hk, dh);
  else VY_FAIL(VY_ERR_ARG, "vy_paged_rope_write: bad dtype %d", dtype);
  VY_CHECK_LAUNCH("vy_paged_rope_write");
  return VY_OK;
}

extern "C" int vy_paged_qknorm_rope_write(void* qkv, int64_t ld, const int32_t* positions, const int64_t* slot_mapping,
                                          const float* cos_tab, const float* sin_tab, int64_t table_rows,
                                          const float* q_scale, const float* k_scale, float eps, void* k_cache,
                                          void* v_cache, int64_t max_blocks, int block_size, int64_t T, int h, int hk,
                                          int dh, int dtype, void* stream) {
  if (const int rc = paged_check_rope_write(
          "vy_paged_qknorm_rope_write",
          !qkv || !positions || !slot_mapping || !cos_tab || !sin_tab || !q_scale || !k_scale || !k_cache || !v_cache,
          (uintptr_t)cos_tab | (uintptr_t)sin_tab | (uintptr_t)q_scale | (uintptr_t)k_scale | (uintptr_t)qkv |
              (uintptr_t)k_cache | (uintptr_t)v_cache,
          ld, table_rows, eps, max_blocks, block_size, T, h, hk, dh))
    return rc;
  int lg = 0;                                         // lanes per (token, head): dh / 8 rounded up to a power of two
  while ((1 << lg) < dh / 8) ++lg;
  const int64_t units = T * (h + 2 * hk);
  const int64_t blocks = vy_cdiv(units << lg, 256);
  if (blocks > INT32_MAX) VY_FAIL(VY_ERR_ARG, "vy_paged_qknorm_rope_write: T %lld is more than one launch holds", (long long)T);
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_slots = max_blocks * block_size;
  const float inv_dh = 1.0f / (float)dh;
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(paged_qknorm_rope_write_kernel<bf16>, grid, block, 0, st, (bf16*)qkv, ld, positions,
                       (const long long*)slot_mapping, cos_tab, sin_tab, table_rows, q_scale, k_scale, eps, inv_dh,
                       (bf16*)k_cache, (bf16*)v_cache, n_slots, units, lg, h, hk, dh);
  else if (dtype == VY_F32)
    hipLaunchKernelGGL(paged_qknorm_rope_write_kernel<float>, grid, block, 0, st, (float*)qkv, ld, positions,
                       (const long long*)slot_mapping, cos_tab, sin_tab, table_rows, q_scale, k_scale, eps, inv_dh,
                       (float*)k_cache, (float*)v_cache, n_slots, units, lg, h, hk, dh);
  else VY_FAIL(VY_ERR_ARG, "vy_paged_qknorm_rope_write: bad dtype %d", dtype);
  VY_CHECK_LAUNCH("vy_paged_qknorm_rope_write");
  return VY_OK;
}

extern "C" int vy_paged_gather(const void* k_cache, const void* v_cache, int64_t max_blocks, int block_size,
                               const int32_t* block_table, int64_t n_blocks, int64_t S, void* k_out, void* v_out,
                               int hk, int dh, int dtype, void* stream) {
  if (!k_cache || !v_cache || !block_table || !k_out || !v_out) VY_FAIL(VY_ERR_ARG, "vy_paged_gather: null operand");
  int lbs;
  if (const int rc = paged_check_geometry("vy_paged_gather", block_size, dh, &lbs)) return rc;
  if (S <= 0 || hk <= 0 || max_blocks <= 0 || max_blocks > INT32_MAX || S > n_blocks * block_size)
    VY_FAIL(VY_ERR_ARG, "vy_paged_gather: bad shape (S %lld, %lld blocks of %d, hk %d)", (long long)S, (long long)n_blocks, block_size, hk);
  if (((uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)k_out | (uintptr_t)v_out) & 15)
    VY_FAIL(VY_ERR_ARG, "vy_paged_gather: operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype == VY_BF16 ? 8 : 4;
  const dim3 grid((unsigned)vy_cdiv(2 * S * hk * (dh / vec), 256)), block(256);
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(paged_gather_kernel<bf16>, grid, block, 0, st, (const bf16*)k_cache, (const bf16*)v_cache, block_table,
                       (bf16*)k_out, (bf16*)v_out, (long long)S, lbs, hk, dh, (int)max_blocks);
  else if (dtype == VY_F32)
    hipLaunchKernelGGL(paged_gather_kernel<float>, grid, block, 0, st, (const float*)k_cache, (const float*)v_cache,
                       block_table, (float*)k_out, (float*)v_out, (long long)S, lbs, hk, dh, (int)max_blocks);
  else VY_FAIL(VY_ERR_ARG, "vy_paged_gather: bad dtype %d", dtype);
  VY_CHECK_LAUNCH("vy_paged_gather");
  return VY_OK;
}
