// Training side of Qwen3's qk_norm: the per-head RMSNorm of q and k between the packed QKV GEMM and the rotation, as a
// forward that leaves the raw projection untouched (it is the backward's saved activation) and a backward that keeps no
// statistics.  Both are streaming kernels over (token, head) units on the lane mapping of
// paged_qknorm_rope_write_kernel (vy_paged.hip): a unit is a group of 1 << lg lanes -- dh / 8 of them at work, rounded up
// to a power of two so that a group never straddles a wave -- and a lane holds 8 columns of its head: in the forward 4 of
// the lower half and the same 4 of the upper half (the rotation's pairs), in the backward, which rotates nothing, 8 in a
// row.  Idle lanes load nothing, enter the group sums with zeros and store nothing.
#include "vy_common.h"
#include "vy_qknorm.h"
#include "vy_wave.h"

namespace {

constexpr int QKN_MAX_BLOCKS = 1024;   // workgroups of the backward (4 per CU: one round) = rows of its partial-sum slab

// q (B, h, L, dh) and k (B, hk, L, dh), strides {batch, head, token}, <- rotate(x * rsqrt(mean x^2 + eps) * scale) of
// the q and k heads of the packed rows qkv[B * L][ld]: fp32 from the load to the one rounding at the store.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const T* __restrict__ qkv, long long ld,
                                                              const float* __restrict__ cos_tab,
                                                              const float* __restrict__ sin_tab, long long pos0,
                                                              const float* __restrict__ q_scale,
                                                              const float* __restrict__ k_scale, float eps, float inv_dh,
                                                              T* __restrict__ q, long long q_sb, long long q_sh,
                                                              long long q_sl, T* __restrict__ k, long long k_sb,
                                                              long long k_sh, long long k_sl, long long units, long long L,
                                                              int lg, int h, int hk, int dh) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int half = dh >> 1, qn = half >> 2, H2 = h + hk;
  const long long unit = idx >> lg;
  const int ch = (int)(idx & ((1 << lg) - 1));
  const bool on = unit < units && ch < qn;
  const long long uc = on ? unit : 0;                 // (an idle lane computes on unit 0's indices and touches no memory)
  const int i4 = on ? ch * 4 : 0;
  const int hd = (int)(uc % H2);
  const long long t = uc / H2;
  const T* row = qkv + t * ld + (long long)hd * dh;
  float lo[4] = {0.f, 0.f, 0.f, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    Quad<T>::load(row + i4, lo);
    Quad<T>::load(row + half + i4, hi);
  }
  const float ss = qk_group_sumsq(lo, hi, lg);        // every lane of the wave, also the idle ones
  if (!on) return;
  const long long b = t / L, l = t - b * L;
  const bool isq = hd < h;
  qknorm_rope_quads(lo, hi, ss, inv_dh, eps, isq ? q_scale : k_scale, cos_tab, sin_tab, pos0 + l, half, i4);
  T* dst = isq ? q + b * q_sb + (long long)hd * q_sh + l * q_sl : k + b * k_sb + (long long)(hd - h) * k_sh + l * k_sl;
  Quad<T>::store(dst + i4, lo);
  Quad<T>::store(dst + half + i4, hi);
}

// eight consecutive elements: one 16-byte chunk of bf16, two of fp32
template <typename T>
__device__ __forceinline__ void load8(const T* p, float* v) {
  Chunk<T>::load(p, v);
  if constexpr (Chunk<T>::VEC == 4) Chunk<T>::load(p + 4, v + 4);
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float* v) {
  Chunk<T>::store(p, v);
  if constexpr (Chunk<T>::VEC == 4) Chunk<T>::store(p + 4, v + 4);
}

// The q and k columns of dqkv[T][ldd] hold dy, the gradient of the NORMALISED heads (vy_attn_bwd has un-rotated it);
// they are overwritten with dx = r g dy - x r^3 / dh sum(x g dy), r = rsqrt(mean x^2 + eps) recomputed from the saved
// raw rows qkv[T][ld].  Nothing is rotated here, so a lane holds 8 CONSECUTIVE columns (16-byte loads in bf16) of its
// unit.  A workgroup owns `iters` consecutive slices of 256 >> lg units and loads a slice ahead of the one it works on; a
// lane keeps its 8 columns over all of them, so its share of the two scale gradients (sum of dy x r over the q units,
// over the k units) stays in registers until the end, where the lanes of the workgroup that hold the same columns are added through LDS in group
// order and the 2 dh sums go to row blockIdx.x of the slab ws: no atomics, the same bits every run.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_bwd_kernel(T* __restrict__ dqkv, long long ldd, const T* __restrict__ qkv,
                                                         long long ld, const float* __restrict__ q_scale,
                                                         const float* __restrict__ k_scale, float eps, float inv_dh,
                                                         float* __restrict__ ws, long long units, int iters, int lg,
                                                         int h, int hk, int dh) {
  __shared__ float red[16][256];
  const int tid = threadIdx.x;
  const int qn = dh >> 3, H2 = h + hk;
  const int gpb = 256 >> lg;                          // units of one slice
  const int grp = tid >> lg, ch = tid & ((1 << lg) - 1);
  const bool lane_on = ch < qn;
  const int c8 = lane_on ? ch * 8 : 0;
  float gq[8], gk[8], accq[8], acck[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) gq[e] = gk[e] = accq[e] = acck[e] = 0.f;
  if (lane_on) {
    load8(q_scale + c8, gq);
    load8(k_scale + c8, gk);
  }
  const long long u0 = (long long)blockIdx.x * iters * gpb + grp;
  float xn[8], dn[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) xn[e] = dn[e] = 0.f;
  if (lane_on && u0 < units) {
    const long long t = u0 / H2;
    const long long col = (long long)(u0 - t * H2) * dh + c8;
    load8(qkv + t * ld + col, xn);
    load8(dqkv + t * ldd + col, dn);
  }
  for (int it = 0; it < iters; ++it) {                // (block-uniform trip count: every lane reaches the group sums)
    const long long unit = u0 + (long long)it * gpb;
    const bool on = lane_on && unit < units;
    const long long uc = on ? unit : 0;
    const int hd = (int)(uc % H2);
    const long long t = uc / H2;
    T* drow = dqkv + t * ldd + (long long)hd * dh;
    float x[8], d[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { x[e] = xn[e]; d[e] = dn[e]; xn[e] = dn[e] = 0.f; }
    const long long un = unit + gpb;                  // the next slice's unit: another row of dqkv than the one stored below
    if (it + 1 < iters && lane_on && un < units) {
      const long long tn = un / H2;
      const long long col = (long long)(un - tn * H2) * dh + c8;
      load8(qkv + tn * ld + col, xn);
      load8(dqkv + tn * ldd + col, dn);
    }
    const bool isq = hd < h;
    float ss = 0.f, sg = 0.f, gd[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gd[e] = (isq ? gq[e] : gk[e]) * d[e];
      ss = fmaf(x[e], x[e], ss);
      sg = fmaf(x[e], gd[e], sg);
    }
    ss = pow2_group_sum(ss, lg);
    sg = pow2_group_sum(sg, lg);
    const float r = rsqrtf(fmaf(ss, inv_dh, eps));
    const float cf = r * r * r * inv_dh * sg;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o[e] = r * gd[e] - x[e] * cf;
      const float a = d[e] * x[e] * r;                // (an idle lane or a unit past the end adds 0)
      accq[e] += isq ? a : 0.f;
      acck[e] += isq ? 0.f : a;
    }
    if (on) store8(drow + c8, o);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[e][tid] = accq[e];
    red[8 + e][tid] = acck[e];
  }
  __syncthreads();
  float* slab = ws + (long long)blockIdx.x * 2 * dh;
  for (int j = tid; j < 2 * dh; j += 256) {           // j: column of dq_scale, then of dk_scale
    const int c = j < dh ? j : j - dh;
    const int e = (j < dh ? 0 : 8) + (c & 7);
    const int lane = c >> 3;
    float a = 0.f;
    for (int g = 0; g < gpb; ++g) a += red[e][(g << lg) + lane];
    slab[j] = a;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int lane_log2(int dh) {                               // lanes per (token, head): dh / 8 rounded up to a power of two
  int lg = 0;
  while ((1 << lg) < dh / 8) ++lg;
  return lg;
}

// slices of 256 >> lg units per workgroup, and the number of workgroups
void bwd_plan(int64_t units, int lg, int* iters, int64_t* blocks) {
  const int64_t slices = vy_cdiv(units, 256 >> lg);
  *iters = (int)vy_cdiv(slices, QKN_MAX_BLOCKS);
  *blocks = vy_cdiv(slices, *iters);
}

int check_heads(const char* who, int h, int hk, int dh, float eps, int dtype) {
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "%s: bad dtype %d", who, dtype);
  if (dh <= 0 || dh % 8 || dh > 256) VY_FAIL(VY_ERR_ARG, "%s: head_dim %d (multiples of 8 up to 256)", who, dh);
  if (h <= 0 || hk <= 0 || h % hk) VY_FAIL(VY_ERR_ARG, "%s: h %d must be a positive multiple of hk %d", who, h, hk);
  if (!(eps >= 0.f)) VY_FAIL(VY_ERR_ARG, "%s: eps must be >= 0", who);
  return VY_OK;
}

int check_ld(const char* who, const char* name, int64_t ld, int64_t W, int dtype) {
  const int vec = dtype == VY_BF16 ? 8 : 4;
  if (ld < W || ld % vec) VY_FAIL(VY_ERR_ARG, "%s: %s %lld must be a multiple of %d, at least %lld", who, name, (long long)ld, vec, (long long)W);
  return VY_OK;
}

}  // namespace

extern "C" int vy_qknorm_rope_fwd(const void* qkv, int64_t ld, const float* cos_tab, const float* sin_tab,
                                  int64_t table_rows, int64_t pos0, const float* q_scale, const float* k_scale, float eps,
                                  void* q, int64_t q_sb, int64_t q_sh, int64_t q_sl, void* k, int64_t k_sb, int64_t k_sh,
                                  int64_t k_sl, int64_t B, int64_t L, int h, int hk, int dh, int dtype, void* stream) {
  const char* who = "vy_qknorm_rope_fwd";
  if (!qkv || !cos_tab || !sin_tab || !q_scale || !k_scale || !q || !k) VY_FAIL(VY_ERR_ARG, "%s: null operand", who);
  if (B <= 0 || L <= 0) VY_FAIL(VY_ERR_ARG, "%s: empty shape", who);
  if (int rc = check_heads(who, h, hk, dh, eps, dtype)) return rc;
  if (int rc = check_ld(who, "ld", ld, (int64_t)(h + 2 * hk) * dh, dtype)) return rc;
  const int vec = dtype == VY_BF16 ? 8 : 4;
  const int64_t st8[] = {q_sb, q_sh, q_sl, k_sb, k_sh, k_sl};
  for (int64_t s : st8)
    if (s < 0 || s % vec) VY_FAIL(VY_ERR_ARG, "%s: q / k strides must be non-negative multiples of %d elements", who, vec);
  if (!aligned16(qkv) || !aligned16(cos_tab) || !aligned16(sin_tab) || !aligned16(q_scale) || !aligned16(k_scale) ||
      !aligned16(q) || !aligned16(k))
    VY_FAIL(VY_ERR_ARG, "%s: operands must be 16-byte aligned", who);
  if (pos0 < 0 || table_rows < pos0 + L) VY_FAIL(VY_ERR_ARG, "%s: the tables hold %lld rows, positions reach %lld", who, (long long)table_rows, (long long)(pos0 + L));
  const int lg = lane_log2(dh);
  const int64_t units = B * L * (h + hk);
  const int64_t blocks = vy_cdiv(units << lg, 256);
  if (blocks > INT32_MAX) VY_FAIL(VY_ERR_ARG, "%s: B * L %lld is more than one launch holds", who, (long long)(B * L));
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t st = (hipStream_t)stream;
  const float inv_dh = 1.0f / (float)dh;
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel<bf16>, grid, block, 0, st, (const bf16*)qkv, ld, cos_tab, sin_tab, pos0, q_scale,
                       k_scale, eps, inv_dh, (bf16*)q, q_sb, q_sh, q_sl, (bf16*)k, k_sb, k_sh, k_sl, units, L, lg, h, hk, dh);
  else
    hipLaunchKernelGGL(qknorm_rope_fwd_kernel<float>, grid, block, 0, st, (const float*)qkv, ld, cos_tab, sin_tab, pos0,
                       q_scale, k_scale, eps, inv_dh, (float*)q, q_sb, q_sh, q_sl, (float*)k, k_sb, k_sh, k_sl, units, L, lg, h,
                       hk, dh);
  VY_CHECK_LAUNCH(who);
  return VY_OK;
}

extern "C" int64_t vy_qknorm_bwd_ws_floats(int64_t T, int h, int hk, int dh) {
  if (T <= 0 || h <= 0 || hk <= 0 || dh <= 0 || dh % 8 || dh > 256) return 0;
  int iters;
  int64_t blocks;
  bwd_plan(T * (h + hk), lane_log2(dh), &iters, &blocks);
  return blocks * 2 * dh;
}

extern "C" int vy_qknorm_bwd(void* dqkv, int64_t ldd, const void* qkv, int64_t ld, const float* q_scale,
                             const float* k_scale, float eps, float* dq_scale, float* dk_scale, float beta, float* ws,
                             int64_t T, int h, int hk, int dh, int dtype, void* stream) {
  const char* who = "vy_qknorm_bwd";
  if (!dqkv || !qkv || !q_scale || !k_scale || !dq_scale || !dk_scale) VY_FAIL(VY_ERR_ARG, "%s: null operand", who);
  if (!ws) VY_FAIL(VY_ERR_ARG, "%s: null workspace (vy_qknorm_bwd_ws_floats)", who);
  if (T <= 0) VY_FAIL(VY_ERR_ARG, "%s: empty shape", who);
  if (beta != 0.f && beta != 1.f) VY_FAIL(VY_ERR_ARG, "%s: beta must be 0 or 1", who);
  if (int rc = check_heads(who, h, hk, dh, eps, dtype)) return rc;
  const int64_t W = (int64_t)(h + 2 * hk) * dh;
  if (int rc = check_ld(who, "ld", ld, W, dtype)) return rc;
  if (int rc = check_ld(who, "ldd", ldd, W, dtype)) return rc;
  if (!aligned16(dqkv) || !aligned16(qkv) || !aligned16(q_scale) || !aligned16(k_scale) || !aligned16(dq_scale) ||
      !aligned16(dk_scale) || !aligned16(ws))
    VY_FAIL(VY_ERR_ARG, "%s: operands must be 16-byte aligned", who);
  const int lg = lane_log2(dh);
  const int64_t units = T * (h + hk);
  int iters;
  int64_t blocks;
  bwd_plan(units, lg, &iters, &blocks);
  hipStream_t st = (hipStream_t)stream;
  const float inv_dh = 1.0f / (float)dh;
  const dim3 grid((unsigned)blocks), block(256);
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(qknorm_bwd_kernel<bf16>, grid, block, 0, st, (bf16*)dqkv, ldd, (const bf16*)qkv, ld, q_scale, k_scale,
                       eps, inv_dh, ws, units, iters, lg, h, hk, dh);
  else
    hipLaunchKernelGGL(qknorm_bwd_kernel<float>, grid, block, 0, st, (float*)dqkv, ldd, (const float*)qkv, ld, q_scale,
                       k_scale, eps, inv_dh, ws, units, iters, lg, h, hk, dh);
  VY_CHECK_LAUNCH(who);
  // the slab's columns [0, dh) are dq_scale's partials, [dh, 2 dh) dk_scale's: two slabs of row length 2 dh, dh apart,
  // summed in the order of vy_colsum.h -- in ONE slice whatever the row count
  return vy_colsum(who, ws, 2, dh, 2 * dh, (int)blocks, dh, 1, dq_scale, dk_scale, beta == 1.f, st);
}
