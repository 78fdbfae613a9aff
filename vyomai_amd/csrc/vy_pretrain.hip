// Encoder pre-training kernels (masked-LM / ELECTRA): the Gumbel-noise export, the discriminator head with its
// binary cross-entropy, and the masked-LM corruption of a batch of token ids.
#include "vy_common.h"

namespace {

// ---- Gumbel noise export (tests; the sampler inside vy_xent_sample_* calls the same vy_gumbel) ----
__global__ __launch_bounds__(256) void gumbel_noise_kernel(float* __restrict__ out, int64_t ld, int64_t M, int V,
                                                           VyNoise nz) {
  const int nq = (V + 3) / 4;
  const int64_t total = M * nq;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / nq;
    const int q = (int)(i - m * nq);
    uint32_t r[4];
    vy_noise_words(nz, m, q, r);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (q * 4 + e < V) out[m * ld + q * 4 + e] = vy_gumbel(r[e]);
  }
}

// ---- discriminator head: z = h . w + b, BCE-with-logits over the live rows ---------------------------
// One wave per row, four rows per workgroup; h is read once per pass.
template <typename T>
__global__ __launch_bounds__(256) void bce_head_fwd_kernel(const T* __restrict__ h, int64_t ldh, const T* __restrict__ w,
                                                           const T* __restrict__ b, float* __restrict__ z,
                                                           const float* __restrict__ target,
                                                           const uint8_t* __restrict__ live, float* __restrict__ loss_sum,
                                                           int64_t M, int d) {
  constexpr int VEC = Chunk<T>::VEC;
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const T* row = h + m * ldh;
  float acc = 0.f;
  for (int c = lane; c < d / VEC; c += 64) {
    float x[VEC], wv[VEC];
    Chunk<T>::load(row + c * VEC, x);
    Chunk<T>::load(w + c * VEC, wv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc = fmaf(x[e], wv[e], acc);
  }
  acc = vy_wave_sum(acc);
  if (lane == 0) {
    const float zz = acc + (b ? VyT<T>::ld(b) : 0.f);
    z[m] = zz;
    if (target && live[m]) atomicAdd(loss_sum, fmaxf(zz, 0.f) - zz * target[m] + log1pf(expf(-fabsf(zz))));
  }
}

// dz[m] = (sigmoid(z) - y) * gscale / max(count, 1) on live rows; dh = dz * w; dw / db: per-lane register partials over
// the rows a wave visits, summed over the workgroup's waves in LDS, then one fp32 atomic per column and workgroup.
template <typename T, int CH>
__global__ __launch_bounds__(256) void bce_head_bwd_kernel(const T* __restrict__ h, int64_t ldh, const T* __restrict__ w,
                                                           const float* __restrict__ z, const float* __restrict__ target,
                                                           const uint8_t* __restrict__ live,
                                                           const float* __restrict__ gscale, const float* __restrict__ count,
                                                           T* __restrict__ dh, int64_t lddh, float* __restrict__ dw,
                                                           float* __restrict__ db, int64_t M, int d) {
  constexpr int VEC = Chunk<T>::VEC;
  __shared__ float part[4][64 * VEC + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = d / VEC;
  const float sc = *gscale / fmaxf(*count, 1.0f);
  float wv[CH][VEC], acc[CH][VEC];
  float dbacc = 0.f;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = lane + i * 64;
#pragma unroll
    for (int e = 0; e < VEC; ++e) { acc[i][e] = 0.f; wv[i][e] = 0.f; }
    if (c < nch) Chunk<T>::load(w + c * VEC, wv[i]);
  }
  for (int64_t m = (int64_t)blockIdx.x * 4 + wave; m < M; m += (int64_t)gridDim.x * 4) {
    float dz = 0.f;
    if (live[m]) dz = (vy_sigmoid(z[m]) - target[m]) * sc;
    dbacc += dz;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = lane + i * 64;
      if (c < nch) {
        float x[VEC], o[VEC];
        if (dz != 0.f) Chunk<T>::load(h + m * ldh + c * VEC, x);   // dz is wave-uniform
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          o[e] = dz != 0.f ? dz * wv[i][e] : 0.f;   // dead rows: +0, whatever the sign of w
          if (dz != 0.f) acc[i][e] = fmaf(dz, x[e], acc[i][e]);
        }
        Chunk<T>::store(dh + m * lddh + c * VEC, o);
      }
    }
  }
  // the workgroup's four waves -> one partial per column (64 * VEC columns at a time), then the atomics
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < VEC; ++e) part[wave][e * 64 + lane] = acc[i][e];   // [e][lane]: a wave's lanes hit 64 banks
    __syncthreads();
    for (int j = threadIdx.x; j < 64 * VEC; j += 256) {
      const int col = i * 64 * VEC + (j & 63) * VEC + (j >> 6);
      if (col < d) atomicAdd(dw + col, part[0][j] + part[1][j] + part[2][j] + part[3][j]);
    }
  }
  __syncthreads();
  if (lane == 0) part[wave][0] = dbacc;   // every lane of a wave holds the same sum
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(db, part[0][0] + part[1][0] + part[2][0] + part[3][0]);
}

// ---- masked-LM corruption of a batch (reference pretraining/collators.py:9-62) -------------------------
__global__ __launch_bounds__(256) void mlm_mask_kernel(const int64_t* __restrict__ ids, int64_t n,
                                                       const int64_t* __restrict__ special, int n_special,
                                                       uint64_t thr_select, int64_t mask_id, uint32_t vocab,
                                                       int64_t ignore_index, VyNoise nz, int64_t* __restrict__ masked_ids,
                                                       int64_t* __restrict__ labels, uint8_t* __restrict__ masked) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = ids[i];
    bool is_special = false;
    for (int k = 0; k < n_special; ++k) is_special |= special[k] == id;
    uint32_t r[4];
    vy_philox7((uint32_t)i, (uint32_t)((uint64_t)i >> 32), nz.off_lo, nz.off_hi, nz.seed_lo, nz.seed_hi, r);
    const bool sel = !is_special && (uint64_t)r[0] < thr_select;
    int64_t out = id;
    if (sel) {
      if (r[1] < 3435973837u) out = mask_id;                      // r1 < 0.8 * 2^32
      else if (r[2] < 2147483648u) out = __umulhi(r[3], vocab);   // r2 < 0.5 * 2^32: a uniform id below vocab
    }
    masked_ids[i] = out;
    labels[i] = sel ? id : ignore_index;
    masked[i] = sel ? 1 : 0;
  }
}

template <typename T>
int bce_bwd_launch(const void* h, int64_t ldh, const void* w, const float* z, const float* target, const uint8_t* live,
                   const float* gscale, const float* count, void* dh, int64_t lddh, float* dw, float* db, int64_t M,
                   int64_t d, hipStream_t st) {
  constexpr int VEC = Chunk<T>::VEC;
  const int nch = (int)(d / VEC);
  const int64_t want = vy_cdiv(M, 4);
  const dim3 grid((unsigned)(want < 256 ? want : 256)), block(256);
#define BCE_GO(CH)                                                                                                  \
  hipLaunchKernelGGL((bce_head_bwd_kernel<T, CH>), grid, block, 0, st, (const T*)h, ldh, (const T*)w, z, target, live, \
                     gscale, count, (T*)dh, lddh, dw, db, M, (int)d)
  if (nch <= 64) BCE_GO(1);
  else if (nch <= 128) BCE_GO(2);
  else if (nch <= 256) BCE_GO(4);
  else if (nch <= 512) BCE_GO(8);
  else VY_FAIL(VY_ERR_UNSUPPORTED, "vy_bce_head_bwd: d=%ld exceeds the %d columns a wave keeps in registers", (long)d, 512 * VEC);
#undef BCE_GO
  VY_CHECK_LAUNCH("vy_bce_head_bwd");
  return VY_OK;
}

}  // namespace

extern "C" int vy_gumbel_noise(float* out, int64_t ld, int64_t M, int64_t V, uint64_t seed, uint64_t offset,
                               void* stream) {
  if (!out || M <= 0 || V <= 0 || ld < V || V > INT32_MAX - 8) VY_FAIL(VY_ERR_ARG, "vy_gumbel_noise: bad arguments");
  const int64_t want = vy_cdiv(M * vy_cdiv(V, 4), 256);
  hipLaunchKernelGGL(gumbel_noise_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, (hipStream_t)stream,
                     out, ld, M, (int)V, vy_make_noise(seed, offset));
  VY_CHECK_LAUNCH("vy_gumbel_noise");
  return VY_OK;
}

extern "C" int vy_bce_head_fwd(const void* h, int64_t ldh, const void* w, const void* b, float* z, const float* target,
                               const uint8_t* live, float* loss_sum, int64_t M, int64_t d, int dtype, void* stream) {
  if (!h || !w || !z || M <= 0 || d <= 0 || ldh < d) VY_FAIL(VY_ERR_ARG, "vy_bce_head_fwd: bad arguments");
  if (target && (!live || !loss_sum)) VY_FAIL(VY_ERR_ARG, "vy_bce_head_fwd: target needs live and loss_sum");
  if (d % 8 || ldh % 8 || (uintptr_t)h % 16 || (uintptr_t)w % 16 || d > INT32_MAX)
    VY_FAIL(VY_ERR_ARG, "vy_bce_head_fwd: d and the row stride must be multiples of 8, rows 16-byte aligned");
  const dim3 grid((unsigned)vy_cdiv(M, 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VY_BF16) hipLaunchKernelGGL(bce_head_fwd_kernel<bf16>, grid, block, 0, st, (const bf16*)h, ldh, (const bf16*)w, (const bf16*)b, z, target, live, loss_sum, M, (int)d);
  else if (dtype == VY_F32) hipLaunchKernelGGL(bce_head_fwd_kernel<float>, grid, block, 0, st, (const float*)h, ldh, (const float*)w, (const float*)b, z, target, live, loss_sum, M, (int)d);
  else VY_FAIL(VY_ERR_ARG, "vy_bce_head_fwd: bad dtype %d", dtype);
  VY_CHECK_LAUNCH("vy_bce_head_fwd");
  return VY_OK;
}

extern "C" int vy_bce_head_bwd(const void* h, int64_t ldh, const void* w, const float* z, const float* target,
                               const uint8_t* live, const float* gscale, const float* count, void* dh, int64_t lddh,
                               float* dw, float* db, int accumulate, int64_t M, int64_t d, int dtype, void* stream) {
  if (!h || !w || !z || !target || !live || !gscale || !count || !dh || !dw || !db || M <= 0 || d <= 0 || ldh < d ||
      lddh < d)
    VY_FAIL(VY_ERR_ARG, "vy_bce_head_bwd: bad arguments");
  if (d % 8 || ldh % 8 || lddh % 8 || (uintptr_t)h % 16 || (uintptr_t)w % 16 || (uintptr_t)dh % 16)
    VY_FAIL(VY_ERR_ARG, "vy_bce_head_bwd: d and the row strides must be multiples of 8, rows 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) {
    if (hipMemsetAsync(dw, 0, (size_t)d * sizeof(float), st) != hipSuccess || hipMemsetAsync(db, 0, sizeof(float), st) != hipSuccess)
      VY_FAIL(VY_ERR_LAUNCH, "vy_bce_head_bwd: clearing dw / db failed");
  }
  if (dtype == VY_BF16) return bce_bwd_launch<bf16>(h, ldh, w, z, target, live, gscale, count, dh, lddh, dw, db, M, d, st);
  if (dtype == VY_F32) return bce_bwd_launch<float>(h, ldh, w, z, target, live, gscale, count, dh, lddh, dw, db, M, d, st);
  VY_FAIL(VY_ERR_ARG, "vy_bce_head_bwd: bad dtype %d", dtype);
}

extern "C" int vy_mlm_mask(const int64_t* ids, int64_t n, const int64_t* special_ids, int32_t n_special, float fraction,
                           int64_t mask_id, int64_t vocab, int64_t ignore_index, uint64_t seed, uint64_t offset,
                           int64_t* masked_ids, int64_t* labels, uint8_t* masked, void* stream) {
  if (!ids || !masked_ids || !labels || !masked || n <= 0 || n_special < 0 || (n_special > 0 && !special_ids))
    VY_FAIL(VY_ERR_ARG, "vy_mlm_mask: bad arguments");
  if (!(fraction >= 0.f && fraction <= 1.f)) VY_FAIL(VY_ERR_ARG, "vy_mlm_mask: fraction=%g outside [0, 1]", (double)fraction);
  if (vocab <= 0 || vocab > (int64_t)UINT32_MAX) VY_FAIL(VY_ERR_ARG, "vy_mlm_mask: bad vocabulary size %ld", (long)vocab);
  // r0 < fraction * 2^32 for an integer r0: r0 < ceil(fraction * 2^32)
  const uint64_t thr = (uint64_t)ceil((double)fraction * 4294967296.0);
  const int64_t want = vy_cdiv(n, 256);
  hipLaunchKernelGGL(mlm_mask_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, (hipStream_t)stream, ids,
                     n, special_ids, (int)n_special, thr, mask_id, (uint32_t)vocab, ignore_index,
                     vy_make_noise(seed, offset), masked_ids, labels, masked);
  VY_CHECK_LAUNCH("vy_mlm_mask");
  return VY_OK;
}
