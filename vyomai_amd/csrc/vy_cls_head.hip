// Sequence-classification head of the encoder (Examples/adapters.ipynb and vyom-ai-classification.ipynb, ClinicModel:
// hidden[:, 0, :] -> nn.Linear(hidden, n_classes) -> CrossEntropyLoss), without an MFMA tile: B is a few dozen rows.
//   vy_cls_head_fwd   logits[b, c] = h[b, 0, :] . W[c] + bias[c] (fp32); with labels also lse, the mean loss and the
//                     in-place dlogits = (softmax - onehot) / count
//   vy_cls_head_bwd   dW, dbias, and dh (B, L, d): row 0 of every sequence = dlogits @ W, every other row zero
// Every sum runs in a fixed order (b ascending, c ascending, a wave's shuffle tree): no atomics, two calls give the same
// bits.  The rule: include/vyom_hip.h.
#include "vy_common.h"

namespace {

// grid ceil(C / 4), one wave per class: the wave walks the B first rows
template <typename T>
__global__ __launch_bounds__(256) void cls_logits_kernel(const T* __restrict__ h, int64_t ldb, const T* __restrict__ w,
                                                         const T* __restrict__ bias, float* __restrict__ logits, int B,
                                                         int C, int d) {
  constexpr int VEC = Chunk<T>::VEC;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const T* wrow = w + (int64_t)c * d;
  const float bc = bias ? VyT<T>::ld(bias + c) : 0.f;
  for (int b = 0; b < B; ++b) {
    const T* row = h + (int64_t)b * ldb;
    float acc = 0.f;
    for (int k = lane; k < d / VEC; k += 64) {
      float x[VEC], wv[VEC];
      Chunk<T>::load(row + k * VEC, x);
      Chunk<T>::load(wrow + k * VEC, wv);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc = fmaf(x[e], wv[e], acc);
    }
    acc = vy_wave_sum(acc);
    if (lane == 0) logits[(int64_t)b * C + c] = acc + bc;
  }
}

// one workgroup, one wave per row at a time; rowloss: B floats of LDS
__global__ __launch_bounds__(256) void cls_xent_kernel(float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                       float* __restrict__ lse, float* __restrict__ loss, int B, int C,
                                                       int* __restrict__ err) {
  extern __shared__ float rowloss[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float cnt = 0.f;                                                   // rows with a label inside [0, C): the mean's divisor
  for (int b = lane; b < B; b += 64) cnt += (labels[b] >= 0 && labels[b] < C) ? 1.f : 0.f;
  cnt = vy_wave_sum(cnt);                                            // (integers: exact, the same in every wave)
  const float inv = 1.0f / fmaxf(cnt, 1.0f);
  for (int b = wave; b < B; b += 4) {
    float* row = logits + (int64_t)b * C;
    const int64_t lab = labels[b];
    const bool ok = lab >= 0 && lab < C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, row[c]);
    mx = vy_wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(row[c] - mx);
    s = vy_wave_sum(s);
    const float l = mx + logf(s);
    if (lane == 0) {
      lse[b] = l;
      rowloss[b] = ok ? l - row[lab] : 0.f;
      if (!ok && err) *err = 1;                                      // never dereferenced, never clamped: the row is ignored
    }
    for (int c = lane; c < C; c += 64) row[c] = ok ? (expf(row[c] - l) - (c == lab ? 1.f : 0.f)) * inv : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int b = 0; b < B; ++b) t += rowloss[b];
    *loss = t * inv;
  }
}

// grid ceil(C / 4) + ceil(B L / 4).  The first blocks: one wave per class, dW[c, :] and dbias[c] summed over b in order.
// The others: one wave per row of dh; row 0 of a sequence sums over c in order, the others are zeros.
template <typename T>
__global__ __launch_bounds__(256) void cls_bwd_kernel(const T* __restrict__ h, int64_t ldb, const T* __restrict__ w,
                                                      const float* __restrict__ dlogits, const float* __restrict__ gscale,
                                                      T* __restrict__ dh, float* __restrict__ dw, float* __restrict__ db,
                                                      int accumulate, int B, int L, int C, int d, int wblocks) {
  constexpr int VEC = Chunk<T>::VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float gs = gscale ? *gscale : 1.0f;
  if ((int)blockIdx.x < wblocks) {
    const int c = blockIdx.x * 4 + wave;
    if (c >= C) return;
    for (int k = lane; k < d / VEC; k += 64) {
      float acc[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
      for (int b = 0; b < B; ++b) {
        const float g = dlogits[(int64_t)b * C + c];
        float x[VEC];
        Chunk<T>::load(h + (int64_t)b * ldb + k * VEC, x);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = fmaf(g, x[e], acc[e]);
      }
      float* dst = dw + (int64_t)c * d + k * VEC;
#pragma unroll
      for (int e = 0; e < VEC; ++e) dst[e] = accumulate ? dst[e] + gs * acc[e] : gs * acc[e];
    }
    if (lane == 0 && db) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += dlogits[(int64_t)b * C + c];
      db[c] = accumulate ? db[c] + gs * s : gs * s;
    }
    return;
  }
  const int64_t m = (int64_t)(blockIdx.x - wblocks) * 4 + wave;      // row of the (B L, d) gradient
  if (m >= (int64_t)B * L) return;
  T* drow = dh + m * d;
  const int b = (int)(m / L);
  const bool first = m == (int64_t)b * L;
  for (int k = lane; k < d / VEC; k += 64) {
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    if (first) {
      for (int c = 0; c < C; ++c) {
        const float g = dlogits[(int64_t)b * C + c];
        float wv[VEC];
        Chunk<T>::load(w + (int64_t)c * d + k * VEC, wv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = fmaf(g, wv[e], acc[e]);
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] *= gs;
    }
    Chunk<T>::store(drow + k * VEC, acc);
  }
}

bool cls_shape_ok(int64_t B, int64_t L, int64_t C, int64_t d, int64_t ldb) {
  return B > 0 && B <= 8192 && L > 0 && C > 0 && C <= INT32_MAX / 4 && d > 0 && d % 8 == 0 && d <= INT32_MAX &&
         ldb >= d && ldb % 8 == 0 && B * L <= INT32_MAX;
}

}  // namespace

extern "C" int vy_cls_head_fwd(const void* h, int64_t ldb, const void* w, const void* bias, float* logits,
                               const int64_t* labels, float* lse, float* loss, int32_t* err_flag, int64_t B, int64_t C,
                               int64_t d, int dtype, void* stream) {
  if (!h || !w || !logits) VY_FAIL(VY_ERR_ARG, "vy_cls_head_fwd: null operand");
  if (labels && (!lse || !loss)) VY_FAIL(VY_ERR_ARG, "vy_cls_head_fwd: labels need lse and loss");
  if (!cls_shape_ok(B, 1, C, d, ldb) || (uintptr_t)h % 16 || (uintptr_t)w % 16)
    VY_FAIL(VY_ERR_ARG, "vy_cls_head_fwd: bad shape (B %lld in [1, 8192], C %lld, d %lld and the stride %lld multiples of 8, "
            "rows 16-byte aligned)", (long long)B, (long long)C, (long long)d, (long long)ldb);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)vy_cdiv(C, 4)), block(256);
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(cls_logits_kernel<bf16>, grid, block, 0, st, (const bf16*)h, ldb, (const bf16*)w, (const bf16*)bias,
                       logits, (int)B, (int)C, (int)d);
  else if (dtype == VY_F32)
    hipLaunchKernelGGL(cls_logits_kernel<float>, grid, block, 0, st, (const float*)h, ldb, (const float*)w,
                       (const float*)bias, logits, (int)B, (int)C, (int)d);
  else
    VY_FAIL(VY_ERR_ARG, "vy_cls_head_fwd: bad dtype %d", dtype);
  VY_CHECK_LAUNCH("vy_cls_head_fwd");
  if (labels) {
    hipLaunchKernelGGL(cls_xent_kernel, dim3(1), block, (size_t)B * sizeof(float), st, logits, labels, lse, loss, (int)B,
                       (int)C, err_flag);
    VY_CHECK_LAUNCH("vy_cls_head_fwd (loss)");
  }
  return VY_OK;
}

extern "C" int vy_cls_head_bwd(const void* h, int64_t ldb, const void* w, const float* dlogits, const float* gscale,
                               void* dh, float* dw, float* db, int accumulate, int64_t B, int64_t L, int64_t C, int64_t d,
                               int dtype, void* stream) {
  if (!h || !w || !dlogits || !dh || !dw) VY_FAIL(VY_ERR_ARG, "vy_cls_head_bwd: null operand");
  if (!cls_shape_ok(B, L, C, d, ldb) || (uintptr_t)h % 16 || (uintptr_t)w % 16 || (uintptr_t)dh % 16 ||
      (accumulate != 0 && accumulate != 1))
    VY_FAIL(VY_ERR_ARG, "vy_cls_head_bwd: bad shape (B %lld in [1, 8192], L %lld, C %lld, d %lld and the stride %lld "
            "multiples of 8, rows 16-byte aligned, accumulate 0 / 1)", (long long)B, (long long)L, (long long)C,
            (long long)d, (long long)ldb);
  hipStream_t st = (hipStream_t)stream;
  const int wblocks = (int)vy_cdiv(C, 4);
  const dim3 grid((unsigned)(wblocks + vy_cdiv(B * L, 4))), block(256);
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(cls_bwd_kernel<bf16>, grid, block, 0, st, (const bf16*)h, ldb, (const bf16*)w, dlogits, gscale,
                       (bf16*)dh, dw, db, accumulate, (int)B, (int)L, (int)C, (int)d, wblocks);
  else if (dtype == VY_F32)
    hipLaunchKernelGGL(cls_bwd_kernel<float>, grid, block, 0, st, (const float*)h, ldb, (const float*)w, dlogits, gscale,
                       (float*)dh, dw, db, accumulate, (int)B, (int)L, (int)C, (int)d, wblocks);
  else
    VY_FAIL(VY_ERR_ARG, "vy_cls_head_bwd: bad dtype %d", dtype);
  VY_CHECK_LAUNCH("vy_cls_head_bwd");
  return VY_OK;
}
