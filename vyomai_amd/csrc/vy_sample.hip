// Sampling front end of the generate loops: the per-token work after the LM head.
//   vy_greedy_step     reference models/decoder.py:478-507 (top-1, prompt forcing, EOS bookkeeping)
//   vy_sampling_probs  reference logits_processors.py:13-16, 59-63, 73-81, 92-102
//   vy_sample_rows     the same processors (:13-16, 59-63, 73-81, 92-102) and their multinomial draw, per row of a
//                      serving step: Examples/simple_vllm.ipynb decodes greedily, this is its step with sampling
//   vy_spec_verify     reference speculative_decoding.py:73-83, 195-230 (accept / reject / resample of a round's drafts)
//                      with the same processors, for every drafted token of a serving step in one launch
// One 1024-thread workgroup per row.  Selection (k-th largest value, nucleus cut) is a radix search over
// 4-bit digits of an order-preserving key: every thread keeps the 16 bin counts / masses of its own
// elements in registers and the workgroup adds them in a fixed order -- no atomics, so the result
// does not depend on scheduling.  The row is re-read from L2 for every pass (V = 50265 bf16 = 100 KB).
#include "vy_common.h"

namespace {

constexpr int ST = 1024, SW = ST / 64;

__device__ __forceinline__ unsigned fkey(float v) {   // larger float <=> larger key
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
template <typename T> __device__ __forceinline__ float ldf(const T* p, int i);
template <> __device__ __forceinline__ float ldf<float>(const float* p, int i) { return p[i]; }
template <> __device__ __forceinline__ float ldf<bf16>(const bf16* p, int i) { return (float)p[i]; }

// sum of NR per-thread values over the workgroup, in a fixed order; every thread gets the result
template <int NR, typename A>
__device__ __forceinline__ void block_sum(A (&v)[NR], A* red /* [SW][NR] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    A x = v[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane == 0) red[wave * NR + r] = x;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    A x = 0;
#pragma unroll 1   // (unrolled, the SW * NR loads are all hoisted and the selection kernels spill 600 bytes a lane)
    for (int w = 0; w < SW; ++w) x += red[w * NR + r];
    v[r] = x;
  }
  __syncthreads();
}
__device__ __forceinline__ float block_max(float m, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  m = vy_wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < SW; ++w) r = fmaxf(r, red[w]);
  __syncthreads();
  return r;
}

template <typename T>
__global__ __launch_bounds__(ST) void greedy_step_kernel(const T* __restrict__ logits, int64_t ldl, int V,
                                                         int64_t* __restrict__ tokens, int64_t ldt, int64_t cur_pos,
                                                         const uint8_t* __restrict__ text_mask, int64_t ldm,
                                                         const int64_t* __restrict__ eos_ids, int n_eos,
                                                         uint8_t* __restrict__ eos_reached, int32_t* __restrict__ not_done) {
  __shared__ float bv[SW];
  __shared__ int bi[SW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool forced = text_mask && text_mask[(int64_t)b * ldm + cur_pos];
  int best_i = 0x7fffffff;
  float best_v = -INFINITY;
  if (!forced) {   // block-uniform
    const T* row = logits + (int64_t)b * ldl;
    auto take = [&](float v, int i) {
      if (v > best_v || (v == best_v && i < best_i) || best_i == 0x7fffffff) { best_v = v; best_i = i; }
    };
    int i0 = 0;
    if constexpr (std::is_same<T, bf16>::value) {
      // 16-byte chunks, all of a thread's chunks requested before the first compare (V = 50265: 7 per thread;
      // one 2-byte load per trip made this kernel 24 us of dependent round trips)
      if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
        const int nch = V >> 3;
        constexpr int CPT = 8;
        for (int c0 = 0; c0 < nch; c0 += ST * CPT) {
          bf16x8 ch[CPT];
#pragma unroll
          for (int u = 0; u < CPT; ++u) {
            const int c = c0 + u * ST + tid;
            if (c < nch) ch[u] = *reinterpret_cast<const bf16x8*>(row + (int64_t)c * 8);
          }
#pragma unroll
          for (int u = 0; u < CPT; ++u) {
            const int c = c0 + u * ST + tid;
            if (c < nch) {
#pragma unroll
              for (int e = 0; e < 8; ++e) take((float)ch[u][e], c * 8 + e);
            }
          }
        }
        i0 = nch << 3;
      }
    }
    for (int i = i0 + tid; i < V; i += ST) take(ldf(row, i), i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best_v, o, 64);
      const int oi = __shfl_xor(best_i, o, 64);
      if (oi != 0x7fffffff && (best_i == 0x7fffffff || ov > best_v || (ov == best_v && oi < best_i))) { best_v = ov; best_i = oi; }
    }
    if (lane == 0) { bv[wave] = best_v; bi[wave] = best_i; }
    __syncthreads();
  }
  if (tid == 0) {
    int64_t next;
    if (forced) {
      next = tokens[(int64_t)b * ldt + cur_pos];
    } else {
      float v = bv[0];
      int i = bi[0];
      for (int w = 1; w < SW; ++w)
        if (bi[w] != 0x7fffffff && (i == 0x7fffffff || bv[w] > v || (bv[w] == v && bi[w] < i))) { v = bv[w]; i = bi[w]; }
      next = i == 0x7fffffff ? 0 : i;   // a row of NaNs has no maximum: token 0, not an out-of-range id
      tokens[(int64_t)b * ldt + cur_pos] = next;
    }
    bool eos = eos_reached[b];
    if (!forced)
      for (int e = 0; e < n_eos; ++e) eos |= (next == eos_ids[e]);
    eos_reached[b] = eos;
    if (!eos && not_done) atomicAdd(not_done, 1);
  }
}

// ---- two-stage top-1 for wide vocabularies ---------------------------------------------------------
// One workgroup per row walks 100 KB (V = 50265) to 514 KB (V = 257216, one sequence) of logits: 13 / 35 us of a
// decode step.  Here stage 1 spreads a row over chunks of 8192 logits (one 256-thread workgroup each, every load
// issued before the first compare) and leaves a (value, index) candidate per chunk; stage 2 is greedy_step_kernel's
// bookkeeping on <= 64 candidates per row.  Same order (value descending, index ascending; a row of NaNs -> 0).
constexpr int GP_CHUNK = 8192, GP_MAXCH = 64, GP_MAXB = 256;
__device__ float g_gp_v[GP_MAXB * GP_MAXCH];
__device__ int g_gp_i[GP_MAXB * GP_MAXCH];

__device__ __forceinline__ void gp_take(float v, int i, float& bv, int& bi) {
  if (v > bv || (v == bv && i < bi) || bi == 0x7fffffff) { bv = v; bi = i; }
}
__device__ __forceinline__ void gp_merge(float ov, int oi, float& bv, int& bi) {
  if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
}

template <typename T>
__global__ __launch_bounds__(256) void greedy_part_kernel(const T* __restrict__ logits, int64_t ldl, int V, int nch,
                                                          const uint8_t* __restrict__ text_mask, int64_t ldm, int64_t cur_pos) {
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (text_mask && text_mask[(int64_t)b * ldm + cur_pos]) return;   // forced position: stage 2 copies the prompt token
  const T* row = logits + (int64_t)b * ldl;
  const int lo = ch * GP_CHUNK, hi = min(V, lo + GP_CHUNK);
  int best_i = 0x7fffffff;
  float best_v = -INFINITY;
  if constexpr (std::is_same<T, bf16>::value) {
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
      constexpr int CPT = GP_CHUNK / 8 / 256;   // 4 chunks of 8 per thread
      bf16x8 c8[CPT];
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int e0 = lo + (u * 256 + tid) * 8;
        c8[u] = *reinterpret_cast<const bf16x8*>(row + (e0 + 8 <= V ? e0 : 0));
      }
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int e0 = lo + (u * 256 + tid) * 8;
        if (e0 + 8 <= V) {
#pragma unroll
          for (int e = 0; e < 8; ++e) gp_take((float)c8[u][e], e0 + e, best_v, best_i);
        } else {
          for (int e = e0; e < hi; ++e) gp_take(ldf(row, e), e, best_v, best_i);
        }
      }
    } else {
      for (int i = lo + tid; i < hi; i += 256) gp_take(ldf(row, i), i, best_v, best_i);
    }
  } else {
    for (int i = lo + tid; i < hi; i += 256) gp_take(ldf(row, i), i, best_v, best_i);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best_v, o, 64);
    const int oi = __shfl_xor(best_i, o, 64);
    gp_merge(ov, oi, best_v, best_i);
  }
  if (lane == 0) { bv[wave] = best_v; bi[wave] = best_i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) gp_merge(bv[w], bi[w], best_v, best_i);
    g_gp_v[b * GP_MAXCH + ch] = best_v;
    g_gp_i[b * GP_MAXCH + ch] = best_i;
  }
}

__global__ __launch_bounds__(64) void greedy_finish_kernel(int nch, int64_t* __restrict__ tokens, int64_t ldt, int64_t cur_pos,
                                                           const uint8_t* __restrict__ text_mask, int64_t ldm,
                                                           const int64_t* __restrict__ eos_ids, int n_eos,
                                                           uint8_t* __restrict__ eos_reached, int32_t* __restrict__ not_done) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool forced = text_mask && text_mask[(int64_t)b * ldm + cur_pos];
  float best_v = -INFINITY;
  int best_i = 0x7fffffff;
  if (!forced) {
    if (lane < nch) { best_v = g_gp_v[b * GP_MAXCH + lane]; best_i = g_gp_i[b * GP_MAXCH + lane]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best_v, o, 64);
      const int oi = __shfl_xor(best_i, o, 64);
      gp_merge(ov, oi, best_v, best_i);
    }
  }
  if (lane == 0) {
    int64_t next;
    if (forced) {
      next = tokens[(int64_t)b * ldt + cur_pos];
    } else {
      next = best_i == 0x7fffffff ? 0 : best_i;
      tokens[(int64_t)b * ldt + cur_pos] = next;
    }
    bool eos = eos_reached[b];
    if (!forced)
      for (int e = 0; e < n_eos; ++e) eos |= (next == eos_ids[e]);
    eos_reached[b] = eos;
    if (!eos && not_done) atomicAdd(not_done, 1);
  }
}

// ---- selection shared by vy_sampling_probs and vy_sample_rows ----------------------------------------
// -> the key of the smallest kept value (0: the whole row is kept).  m is the row maximum and is read only when top_p is
// on.  Every thread returns the same key; fred / ired are free again on return.
template <typename T>
__device__ __forceinline__ unsigned select_keep_key(const T* __restrict__ row, int V, int top_k, float top_p, float m,
                                                    float* fred /* [SW * 16] */, int* ired /* [SW * 16] */) {
  const int tid = threadIdx.x;
  // ---- top-k: key of the k-th largest value (values equal to it are all kept, reference :59-63) ----
  unsigned keep_key = 0;
  if (top_k > 0 && top_k < V) {
    unsigned prefix = 0;
    int kk = top_k;
    for (int shift = 28; shift >= 0; shift -= 4) {
      int cnt[16];
#pragma unroll
      for (int d = 0; d < 16; ++d) cnt[d] = 0;
      for (int i = tid; i < V; i += ST) {
        const unsigned key = fkey(ldf(row, i));
        const bool match = shift == 28 || ((key ^ prefix) >> (shift + 4)) == 0;
        const int dg = (key >> shift) & 15;
#pragma unroll
        for (int d = 0; d < 16; ++d) cnt[d] += (match && dg == d);
      }
      block_sum<16, int>(cnt, ired);
      int acc = 0, sel = 0;
#pragma unroll
      for (int d = 15; d >= 0; --d) {
        if (acc >= 0) {
          if (acc + cnt[d] >= kk) { sel = d; kk -= acc; acc = -1; }
          else acc += cnt[d];
        }
      }
      prefix |= (unsigned)sel << shift;
    }
    keep_key = prefix;
  }

  // ---- nucleus: the sorted prefix up to and including the first element whose cumulative softmax of the
  //      unscaled (top-k masked) logits exceeds top_p (reference :74-80) ----
  if (top_p > 0.f && top_p < 1.f) {
    float z[1] = {0.f};
    for (int i = tid; i < V; i += ST) {
      const float v = ldf(row, i);
      if (fkey(v) >= keep_key) z[0] += expf(v - m);
    }
    block_sum<1, float>(z, fred);
    const float target = top_p * z[0];
    unsigned prefix = 0;
    float above = 0.f;
    for (int shift = 28; shift >= 0; shift -= 4) {
      float mass[16];
#pragma unroll
      for (int d = 0; d < 16; ++d) mass[d] = 0.f;
      for (int i = tid; i < V; i += ST) {
        const float v = ldf(row, i);
        const unsigned key = fkey(v);
        const bool match = key >= keep_key && (shift == 28 || ((key ^ prefix) >> (shift + 4)) == 0);
        const int dg = (key >> shift) & 15;
        const float e = match ? expf(v - m) : 0.f;
#pragma unroll
        for (int d = 0; d < 16; ++d) mass[d] += (dg == d) ? e : 0.f;
      }
      block_sum<16, float>(mass, fred);
      int sel = -1, lowest = 0;
      bool have_low = false;
#pragma unroll
      for (int d = 15; d >= 0; --d) {
        if (sel < 0) {
          if (above + mass[d] > target) sel = d;
          else above += mass[d];
        }
        if (mass[d] > 0.f) { lowest = d; have_low = true; }
      }
      // the parent bin crossed the target; if rounding of the finer sums hides that, the crossing
      // element is the last one of the bin
      if (sel < 0) { sel = have_low ? lowest : 0; above -= mass[sel]; }
      prefix |= (unsigned)sel << shift;
    }
    keep_key = prefix > keep_key ? prefix : keep_key;
  }

  return keep_key;
}

template <typename T>
__global__ __launch_bounds__(ST) void sampling_probs_kernel(const T* __restrict__ logits, int64_t ldl, int V,
                                                            float inv_t, int top_k, float top_p,
                                                            float* __restrict__ probs, int64_t ldp) {
  __shared__ float fred[SW * 16];
  __shared__ int ired[SW * 16];
  const int tid = threadIdx.x;
  const T* row = logits + (int64_t)blockIdx.x * ldl;
  float* out = probs + (int64_t)blockIdx.x * ldp;

  float m = -INFINITY;
  for (int i = tid; i < V; i += ST) m = fmaxf(m, ldf(row, i));
  m = block_max(m, fred);
  const unsigned keep_key = select_keep_key(row, V, top_k, top_p, m, fred, ired);

  float zt[1] = {0.f};
  for (int i = tid; i < V; i += ST) {
    const float v = ldf(row, i);
    if (fkey(v) >= keep_key) zt[0] += expf((v - m) * inv_t);
  }
  block_sum<1, float>(zt, fred);
  const float rz = 1.0f / zt[0];
  for (int i = tid; i < V; i += ST) {
    const float v = ldf(row, i);
    out[i] = fkey(v) >= keep_key ? expf((v - m) * inv_t) * rz : 0.f;
  }
}

// ---- per-request sampling of the serving engine: one launch for the step's rows ---------------------
// Row r draws argmax over its kept columns of fmaf(logit, inv_temperature[r], gumbel(seed[r], counter[r], noise row 0,
// column)): Gumbel-max needs no normaliser, so nothing is written but the token.  inv_temperature[r] == 0 is a greedy
// row (plain arg-max; its other parameters are not read).  A row without a filter is read once; a filtered row runs
// select_keep_key first (re-reading the row from L2) and pays for noise only on the columns it kept.  One workgroup per
// row: every branch on the row's parameters is workgroup-uniform.
template <typename T> struct Quad;
template <> struct Quad<float> { typedef f32x4 Raw; };
template <> struct Quad<bf16> { typedef bf16x4 Raw; };

template <typename T, bool SAMPLE>
__device__ __forceinline__ void scan_row(const T* __restrict__ row, int V, float inv_t, unsigned keep_key, const VyNoise& nz,
                                         int64_t nrow, float& best_v, int& best_i) {
  typedef typename Quad<T>::Raw Raw;
  constexpr int U = 4;   // quads in flight per thread: all loads of a trip are issued before the first compare
  const int tid = threadIdx.x, nq = (V + 3) >> 2;
  // whole quads of an aligned row are one load; the tail quad and unaligned rows go column by column
  const int nvec = (reinterpret_cast<uintptr_t>(row) & (sizeof(Raw) - 1)) == 0 ? V >> 2 : 0;
  for (int q0 = 0; q0 < nq; q0 += ST * U) {
    float v[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * ST + tid;
      if (q < nvec) {
        const Raw t = *reinterpret_cast<const Raw*>(row + (int64_t)q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][e] = (float)t[e];
      } else if (q < nq) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[u][e] = q * 4 + e < V ? ldf(row, q * 4 + e) : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * ST + tid;
      if (q >= nq) continue;
      if constexpr (SAMPLE) {
        bool kept[4], any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) { kept[e] = q * 4 + e < V && fkey(v[u][e]) >= keep_key; any |= kept[e]; }
        if (any) {
          uint32_t r[4];
          vy_noise_words(nz, nrow, q, r);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (kept[e]) gp_take(fmaf(v[u][e], inv_t, vy_gumbel(r[e])), q * 4 + e, best_v, best_i);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (q * 4 + e < V) gp_take(v[u][e], q * 4 + e, best_v, best_i);
      }
    }
  }
}

// the workgroup's best (value, index): highest value, lowest index among equal ones -> the index (0x7fffffff: nothing
// comparable in the row).  ALL: every thread gets it and fred / ired are free again on return; else thread 0 alone.
template <bool ALL>
__device__ __forceinline__ int block_best(float best_v, int best_i, float* fred, int* ired) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best_v, o, 64);
    const int oi = __shfl_xor(best_i, o, 64);
    gp_merge(ov, oi, best_v, best_i);
  }
  if (lane == 0) { fred[wave] = best_v; ired[wave] = best_i; }
  __syncthreads();
  if (ALL || threadIdx.x == 0) {
    if (ALL) { best_v = fred[0]; best_i = ired[0]; }
    for (int w = 1; w < SW; ++w) gp_merge(fred[w], ired[w], best_v, best_i);
  }
  if (ALL) __syncthreads();
  return best_i;
}

// One row's draw with the parameters of entry r (vy_sample_rows' rule; vy_spec_verify's row after the last draft is
// this very code, so the two give the same token bit for bit).  The noise offset is counter[r] + counter_add.  Thread 0
// holds the token.
template <typename T>
__device__ __forceinline__ int draw_row(const T* __restrict__ row, int V, int r, const float* __restrict__ inv_temperature,
                                        const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                        const int64_t* __restrict__ seed, const int64_t* __restrict__ counter,
                                        int64_t counter_add, float* fred, int* ired) {
  const int tid = threadIdx.x;
  const float inv_t = inv_temperature[r];
  int best_i = 0x7fffffff;
  float best_v = -INFINITY;
  if (inv_t == 0.f) {
    scan_row<T, false>(row, V, 0.f, 0u, VyNoise{}, 0, best_v, best_i);
  } else {
    const int k = top_k[r];
    const float p = top_p[r];
    const bool k_on = k > 0 && k < V, p_on = p > 0.f && p < 1.f;
    unsigned keep_key = 0;
    if (k_on || p_on) {
      float m = -INFINITY;
      if (p_on) {
        for (int i = tid; i < V; i += ST) m = fmaxf(m, ldf(row, i));
        m = block_max(m, fred);
      }
      keep_key = select_keep_key(row, V, k, p, m, fred, ired);
    }
    scan_row<T, true>(row, V, inv_t, keep_key, vy_make_noise((uint64_t)seed[r], (uint64_t)(counter[r] + counter_add)), 0,
                      best_v, best_i);
  }
  const int best = block_best<false>(best_v, best_i, fred, ired);
  return best == 0x7fffffff ? 0 : best;   // nothing comparable in the row (NaNs): token 0, as vy_greedy_step
}

template <typename T>
__global__ __launch_bounds__(ST) void sample_rows_kernel(const T* __restrict__ logits, int64_t ldl, int V,
                                                         const float* __restrict__ inv_temperature,
                                                         const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                         const int64_t* __restrict__ seed, const int64_t* __restrict__ counter,
                                                         int64_t* __restrict__ tokens) {
  __shared__ float fred[SW * 16];
  __shared__ int ired[SW * 16];
  const int r = blockIdx.x;
  const int tok = draw_row(logits + (int64_t)r * ldl, V, r, inv_temperature, top_k, top_p, seed, counter, 0, fred, ired);
  if (threadIdx.x == 0) tokens[r] = tok;
}

// ---- speculative decoding: accept / reject / resample for every drafted token of a step ---------------
// Workgroup (s, i) judges row i of sequence s: target row t = target[t_row0[s] + i], draft row d = draft[i][s], draft token
// x = draft_tokens[i][s].  The rows of a sequence are independent (the first rejection is a scan the host does).
//   i <  n_draft[s], greedy:  a = argmax t;  accept iff a == x;  alt = a.
//   i <  n_draft[s], sampled: p / q = the softmax of t / d at the request's temperature over the set its top_k / top_p keep
//                             (the values vy_sampling_probs would write, never stored);  reject iff x is outside p's set or
//                             u q(x) > p(x), u from noise row 1;  alt = Gumbel-max draw from max(p - q, 0) with noise row 2
//                             (from p if no column has p > q);  an accepted row writes alt = -1.
//   i == n_draft[s]:          alt = draw_row on t with counter position0[s] + n_draft[s] -- vy_sample_rows' token.
//   i >  n_draft[s], or a sequence whose rows would leave the target buffer: accept 0, alt -1, nothing read.
// Every branch is on values all threads hold alike (block_sum / block_max / block_best<true> hand every thread the same
// result).
template <typename T>
__device__ __forceinline__ float kept_prob(const T* __restrict__ row, int c, float m, float inv_t, unsigned key, float rz) {
  const float v = ldf(row, c);
  return fkey(v) >= key ? expf((v - m) * inv_t) * rz : 0.f;
}

template <typename T>
__global__ __launch_bounds__(ST) void spec_verify_kernel(const T* __restrict__ target, int64_t ldt, int64_t t_rows,
                                                         const T* __restrict__ draft, int64_t ldd_i, int64_t ldd_s, int S,
                                                         int gamma, int V, const int64_t* __restrict__ draft_tokens,
                                                         const int32_t* __restrict__ t_row0, const int32_t* __restrict__ n_draft,
                                                         const float* __restrict__ inv_temperature,
                                                         const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                         const int64_t* __restrict__ seed, const int64_t* __restrict__ position0,
                                                         int32_t* __restrict__ accept, int64_t* __restrict__ alt) {
  __shared__ float fred[SW * 16];
  __shared__ int ired[SW * 16];
  const int s = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  const int n = n_draft[s];
  const int64_t r0 = t_row0[s];
  const int64_t out = (int64_t)s * (gamma + 1) + i;
  if (n < 0 || n > gamma || i > n || r0 < 0 || r0 + n >= t_rows) {
    if (tid == 0) { accept[out] = 0; alt[out] = -1; }
    return;
  }
  const T* trow = target + (r0 + i) * ldt;
  if (i == n) {
    const int tok = draw_row(trow, V, s, inv_temperature, top_k, top_p, seed, position0, n, fred, ired);
    if (tid == 0) { accept[out] = 0; alt[out] = tok; }
    return;
  }
  const int64_t x = draft_tokens[(int64_t)i * S + s];
  const float inv_t = inv_temperature[s];
  int best_i = 0x7fffffff;
  float best_v = -INFINITY;
  if (inv_t == 0.f) {
    scan_row<T, false>(trow, V, 0.f, 0u, VyNoise{}, 0, best_v, best_i);
    const int best = block_best<false>(best_v, best_i, fred, ired);
    const int a = best == 0x7fffffff ? 0 : best;
    if (tid == 0) { accept[out] = a == x; alt[out] = a; }
    return;
  }
  const T* drow = draft + i * ldd_i + s * ldd_s;
  const int k = top_k[s];
  const float tp = top_p[s];
  float mt = 0.f, md = 0.f, rzt = 0.f, rzd = 0.f;
  unsigned keyt = 0, keyd = 0;
#pragma unroll 1   // (one copy of the selection code serves both rows)
  for (int w = 0; w < 2; ++w) {
    const T* row = w ? drow : trow;
    float m = -INFINITY;
    for (int c = tid; c < V; c += ST) m = fmaxf(m, ldf(row, c));
    m = block_max(m, fred);
    const unsigned key = select_keep_key(row, V, k, tp, m, fred, ired);
    float z[1] = {0.f};
    for (int c = tid; c < V; c += ST) {
      const float v = ldf(row, c);
      if (fkey(v) >= key) z[0] += expf((v - m) * inv_t);
    }
    block_sum<1, float>(z, fred);
    if (w) { md = m; keyd = key; rzd = 1.0f / z[0]; }
    else { mt = m; keyt = key; rzt = 1.0f / z[0]; }
  }
  const bool in_range = x >= 0 && x < V;
  const bool in_kp = in_range && fkey(ldf(trow, in_range ? (int)x : 0)) >= keyt;
  const float px = in_range ? kept_prob(trow, (int)x, mt, inv_t, keyt, rzt) : 0.f;
  const float qx = in_range ? kept_prob(drow, (int)x, md, inv_t, keyd, rzd) : 0.f;
  const VyNoise nz = vy_make_noise((uint64_t)seed[s], (uint64_t)(position0[s] + i));
  uint32_t uw[4];
  vy_noise_words(nz, 1, 0, uw);
  const float u = (float)(uw[0] >> 8) * 5.9604644775390625e-8f;
  if (in_kp && !(u * qx > px)) {
    if (tid == 0) { accept[out] = 1; alt[out] = -1; }
    return;
  }
  // rejected: Gumbel-max over the columns with p > q of log(p - q) + noise row 2
  const int nq = (V + 3) >> 2;
  for (int q = tid; q < nq; q += ST) {
    float diff[4];
    bool any = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = q * 4 + e;
      diff[e] = c < V ? kept_prob(trow, c, mt, inv_t, keyt, rzt) - kept_prob(drow, c, md, inv_t, keyd, rzd) : 0.f;
      any |= diff[e] > 0.f;
    }
    if (any) {
      uint32_t r[4];
      vy_noise_words(nz, 2, q, r);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (diff[e] > 0.f) gp_take(logf(diff[e]) + vy_gumbel(r[e]), q * 4 + e, best_v, best_i);
    }
  }
  int best = block_best<true>(best_v, best_i, fred, ired);
  if (best == 0x7fffffff) {   // p <= q everywhere (rounding only: both sum to one): draw from p
    best_v = -INFINITY;
    scan_row<T, true>(trow, V, inv_t, keyt, nz, 2, best_v, best_i);
    best = block_best<false>(best_v, best_i, fred, ired);
  }
  if (tid == 0) { accept[out] = 0; alt[out] = best == 0x7fffffff ? 0 : best; }
}

}  // namespace

extern "C" int vy_greedy_step(const void* logits, int64_t ldl, int64_t B, int64_t V, int dtype, int64_t* tokens,
                              int64_t ldt, int64_t cur_pos, const uint8_t* text_mask, int64_t ldm,
                              const int64_t* eos_ids, int32_t n_eos, uint8_t* eos_reached, int32_t* not_done,
                              void* stream) {
  if (!logits || !tokens || !eos_reached || B <= 0 || V <= 0 || V > 0x7ffffff0 || cur_pos < 0 || cur_pos >= ldt ||
      n_eos < 0 || (n_eos > 0 && !eos_ids))
    VY_FAIL(VY_ERR_ARG, "vy_greedy_step: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_greedy_step: bad dtype %d", dtype);
  // wide rows: two stages (see greedy_part_kernel); small V or B > GP_MAXB: one workgroup per row
  const int64_t nch = (V + GP_CHUNK - 1) / GP_CHUNK;
  if (V >= 2 * GP_CHUNK && nch <= GP_MAXCH && B <= GP_MAXB) {
    const dim3 grid((unsigned)nch, (unsigned)B);
    if (dtype == VY_BF16)
      hipLaunchKernelGGL(greedy_part_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)logits, ldl, (int)V, (int)nch, text_mask,
                         ldm, cur_pos);
    else
      hipLaunchKernelGGL(greedy_part_kernel<float>, grid, dim3(256), 0, st, (const float*)logits, ldl, (int)V, (int)nch,
                         text_mask, ldm, cur_pos);
    hipLaunchKernelGGL(greedy_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, (int)nch, tokens, ldt, cur_pos, text_mask, ldm,
                       eos_ids, (int)n_eos, eos_reached, not_done);
    VY_CHECK_LAUNCH("vy_greedy_step");
    return VY_OK;
  }
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(greedy_step_kernel<bf16>, dim3((unsigned)B), dim3(ST), 0, st, (const bf16*)logits, ldl, (int)V, tokens,
                       ldt, cur_pos, text_mask, ldm, eos_ids, (int)n_eos, eos_reached, not_done);
  else if (dtype == VY_F32)
    hipLaunchKernelGGL(greedy_step_kernel<float>, dim3((unsigned)B), dim3(ST), 0, st, (const float*)logits, ldl, (int)V,
                       tokens, ldt, cur_pos, text_mask, ldm, eos_ids, (int)n_eos, eos_reached, not_done);
  else VY_FAIL(VY_ERR_ARG, "vy_greedy_step: bad dtype %d", dtype);
  VY_CHECK_LAUNCH("vy_greedy_step");
  return VY_OK;
}

extern "C" int vy_sampling_probs(const void* logits, int64_t ldl, int64_t B, int64_t V, int dtype, float temperature,
                                 int32_t top_k, float top_p, float* probs, int64_t ldp, void* stream) {
  if (!logits || !probs || B <= 0 || V <= 0 || V > 0x7ffffff0 || ldp < V || ldl < V)
    VY_FAIL(VY_ERR_ARG, "vy_sampling_probs: bad arguments");
  if (!(temperature > 0.f)) VY_FAIL(VY_ERR_ARG, "vy_sampling_probs: temperature must be positive");
  if (top_k < 0 || !(top_p >= 0.f)) VY_FAIL(VY_ERR_ARG, "vy_sampling_probs: top_k and top_p must not be negative");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(sampling_probs_kernel<bf16>, dim3((unsigned)B), dim3(ST), 0, st, (const bf16*)logits, ldl, (int)V,
                       1.0f / temperature, (int)top_k, top_p, probs, ldp);
  else if (dtype == VY_F32)
    hipLaunchKernelGGL(sampling_probs_kernel<float>, dim3((unsigned)B), dim3(ST), 0, st, (const float*)logits, ldl, (int)V,
                       1.0f / temperature, (int)top_k, top_p, probs, ldp);
  else VY_FAIL(VY_ERR_ARG, "vy_sampling_probs: bad dtype %d", dtype);
  VY_CHECK_LAUNCH("vy_sampling_probs");
  return VY_OK;
}

extern "C" int vy_sample_rows(const void* logits, int64_t ldl, int64_t R, int64_t V, int dtype,
                              const float* inv_temperature, const int32_t* top_k, const float* top_p,
                              const int64_t* seed, const int64_t* counter, int64_t* tokens, void* stream) {
  if (!logits || !inv_temperature || !top_k || !top_p || !seed || !counter || !tokens)
    VY_FAIL(VY_ERR_ARG, "vy_sample_rows: null operand");
  if (R <= 0 || R > INT32_MAX || V <= 0 || V > 0x7ffffff0 || ldl < V)
    VY_FAIL(VY_ERR_ARG, "vy_sample_rows: bad shape (R %lld, V %lld, ldl %lld)", (long long)R, (long long)V, (long long)ldl);
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_sample_rows: bad dtype %d", dtype);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(sample_rows_kernel<bf16>, dim3((unsigned)R), dim3(ST), 0, st, (const bf16*)logits, ldl, (int)V,
                       inv_temperature, top_k, top_p, seed, counter, tokens);
  else
    hipLaunchKernelGGL(sample_rows_kernel<float>, dim3((unsigned)R), dim3(ST), 0, st, (const float*)logits, ldl, (int)V,
                       inv_temperature, top_k, top_p, seed, counter, tokens);
  VY_CHECK_LAUNCH("vy_sample_rows");
  return VY_OK;
}

extern "C" int vy_spec_verify(const void* target_logits, int64_t ldt, int64_t t_rows, const void* draft_logits, int64_t ldd_i,
                              int64_t ldd_s, int64_t S, int64_t gamma, int64_t V, int dtype, const int64_t* draft_tokens,
                              const int32_t* t_row0, const int32_t* n_draft, const float* inv_temperature,
                              const int32_t* top_k, const float* top_p, const int64_t* seed, const int64_t* position0,
                              int32_t* accept, int64_t* alt, void* stream) {
  if (!target_logits || !draft_logits || !draft_tokens || !t_row0 || !n_draft || !inv_temperature || !top_k || !top_p ||
      !seed || !position0 || !accept || !alt)
    VY_FAIL(VY_ERR_ARG, "vy_spec_verify: null operand");
  if (S <= 0 || S > INT32_MAX || gamma < 1 || gamma > 16 || t_rows <= 0 || t_rows > INT32_MAX)
    VY_FAIL(VY_ERR_ARG, "vy_spec_verify: bad shape (S %lld, gamma %lld, target rows %lld)", (long long)S, (long long)gamma,
            (long long)t_rows);
  if (V <= 0 || V > 0x7ffffff0 || ldt < V || ldd_s < V || ldd_i < 0)
    VY_FAIL(VY_ERR_ARG, "vy_spec_verify: bad shape (V %lld, ldt %lld, ldd %lld / %lld)", (long long)V, (long long)ldt,
            (long long)ldd_i, (long long)ldd_s);
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_spec_verify: bad dtype %d", dtype);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)S, (unsigned)gamma + 1);
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(spec_verify_kernel<bf16>, grid, dim3(ST), 0, st, (const bf16*)target_logits, ldt, t_rows,
                       (const bf16*)draft_logits, ldd_i, ldd_s, (int)S, (int)gamma, (int)V, draft_tokens, t_row0, n_draft,
                       inv_temperature, top_k, top_p, seed, position0, accept, alt);
  else
    hipLaunchKernelGGL(spec_verify_kernel<float>, grid, dim3(ST), 0, st, (const float*)target_logits, ldt, t_rows,
                       (const float*)draft_logits, ldd_i, ldd_s, (int)S, (int)gamma, (int)V, draft_tokens, t_row0, n_draft,
                       inv_temperature, top_k, top_p, seed, position0, accept, alt);
  VY_CHECK_LAUNCH("vy_spec_verify");
  return VY_OK;
}
