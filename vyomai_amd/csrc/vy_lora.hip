// Per-request LoRA delta of a serving step (serving.ContinuousBatchEngine with adapters=): after a projection's own
// GEMM, y[t, :] += alpha[s] * (x[t, :] @ A[s].T) @ B[s].T for the rows t of requests that carry adapter slot s
// (reference layers/adapters.py LoraLinear.forward: linear(x) + scale * F.linear(F.linear(x, lora_a), lora_b)).
//   vy_lora_shrink   u[t, 0:R] = x[t, 0:K] @ A[slot].T          one workgroup per (tile, 16 columns of R)
//   vy_lora_expand   y[t, n] += alpha[slot] * u[t, part(n)] . B[slot][n]   one wave per (tile, 16 columns of N)
// The rule (tiles, the rounding of u, what is skipped): include/vyom_hip.h.
//
// Both are 16 x 16 MFMA tiles whose operands come straight from global memory: the weight rows (A[slot] / B[slot]) are
// the MFMA's A operand and the activation rows (x / u) its B operand, so lane l reads 16 contiguous bytes of weight
// row l & 15 and of activation row l & 15 at k = 8 (l >> 4) (bf16; 4 (l >> 4) in fp32) -- no LDS, no transpose -- and
// the result has the activation row on the lane (lane & 15) and FOUR CONSECUTIVE output columns 4 (lane >> 4) + reg in
// its registers: one 8-byte (bf16) / 16-byte (fp32) access per lane for u and for the read-modify-write of y.
// fp32 runs on mfma_f32_16x16x4f32, four per 16-byte fragment (element j of every lane is one k of one MFMA; which k
// goes to which MFMA does not matter as long as both operands agree).  Every element of u / y is written by one lane.
#include "vy_common.h"

namespace {

constexpr int LW = 4;   // waves per workgroup

template <typename T> struct LoraFrag;
template <> struct LoraFrag<bf16> {
  static constexpr int KS = 32, VEC = 8;     // k per step of one wave, elements per 16-byte fragment
  typedef bf16x8 V;
  typedef bf16x4 Out;
  static __device__ __forceinline__ f32x4 mma(const V& w, const V& a, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, c, 0, 0, 0);
  }
  static __device__ __forceinline__ Out pack(const f32x4& v) {
    Out o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (bf16)v[e];
    return o;
  }
  static __device__ __forceinline__ f32x4 unpack(const Out& o) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)o[e];
    return v;
  }
};
template <> struct LoraFrag<float> {
  static constexpr int KS = 16, VEC = 4;
  typedef f32x4 V;
  typedef f32x4 Out;
  static __device__ __forceinline__ f32x4 mma(const V& w, const V& a, f32x4 c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j], a[j], c, 0, 0, 0);
    return c;
  }
  static __device__ __forceinline__ Out pack(const f32x4& v) { return v; }
  static __device__ __forceinline__ f32x4 unpack(const Out& o) { return o; }
};

struct LoraTile {
  int row0, nrows, slot;
};
// false: the tile is skipped unread (its slot is outside [0, slots) or its rows leave [0, T) or a tile of 16)
__device__ __forceinline__ bool lora_tile(const int32_t* __restrict__ tiles, int t, int64_t T, int slots, LoraTile& tl) {
  tl.row0 = tiles[3 * t];
  tl.nrows = tiles[3 * t + 1];
  tl.slot = tiles[3 * t + 2];
  return tl.slot >= 0 && tl.slot < slots && tl.nrows >= 1 && tl.nrows <= 16 && tl.row0 >= 0 &&
         (int64_t)tl.row0 + tl.nrows <= T;
}

// grid (n_tiles, R / 16); the workgroup's LW waves take the k-steps w, w + LW, ... and wave 0 adds the four partial
// tiles in wave order (a fixed order: the result does not depend on scheduling)
template <typename T>
__global__ __launch_bounds__(64 * LW) void lora_shrink_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ A,
                                                              const int32_t* __restrict__ tiles, T* __restrict__ u,
                                                              int64_t ldu, int64_t rows, int K, int R, int slots) {
  using F = LoraFrag<T>;
  __shared__ f32x4 part[LW][64];
  LoraTile tl;
  if (!lora_tile(tiles, blockIdx.x, rows, slots, tl)) return;       // (the same answer in every lane of the workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kq = (lane >> 4) * F::VEC;
  const int c0 = blockIdx.y * 16;
  const bool live = r < tl.nrows;
  const T* wrow = A + ((int64_t)tl.slot * R + c0 + r) * K + kq;
  const T* xrow = x + (int64_t)(tl.row0 + (live ? r : 0)) * ldx + kq;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  typename F::V zero;
#pragma unroll
  for (int e = 0; e < F::VEC; ++e) zero[e] = (T)0.f;
  const int steps = (K / F::KS + LW - 1 - wave) / LW;
  const auto ld = [&](const T* row, int i) {                         // the fragment of this wave's k-step i
    return *reinterpret_cast<const typename F::V*>(row + (wave + i * LW) * F::KS);
  };
  int i = 0;
  for (; i + 4 <= steps; i += 4) {                                   // four steps' loads in flight
    typename F::V w[4], a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = ld(wrow, i + j);
      a[j] = ld(xrow, i + j);                                        // (a dead lane re-reads the tile's row 0)
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = F::mma(w[j], live ? a[j] : zero, acc);
  }
  for (; i < steps; ++i) acc = F::mma(ld(wrow, i), live ? ld(xrow, i) : zero, acc);
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && live) {
    f32x4 s = part[0][lane];
#pragma unroll
    for (int w = 1; w < LW; ++w) s += part[w][lane];
    *reinterpret_cast<typename F::Out*>(u + (int64_t)(tl.row0 + r) * ldu + c0 + (lane >> 4) * 4) = F::pack(s);
  }
}

// grid (n_tiles, ceil(N / 16 / LW)); wave w of a workgroup owns columns 16 (LW blockIdx.y + w) .. + 15
template <typename T>
__global__ __launch_bounds__(64 * LW) void lora_expand_kernel(T* __restrict__ y, int64_t ldy, const T* __restrict__ u,
                                                              int64_t ldu, const T* __restrict__ B,
                                                              const float* __restrict__ alpha,
                                                              const int32_t* __restrict__ tiles, int64_t rows, int N,
                                                              int r_pad, int slots, int bound0, int bound1) {
  using F = LoraFrag<T>;
  LoraTile tl;
  if (!lora_tile(tiles, blockIdx.x, rows, slots, tl)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.y * LW + wave) * 16;
  if (n0 >= N) return;                                               // (no barrier in this kernel)
  const int r = lane & 15, kq = (lane >> 4) * F::VEC;
  const bool live = r < tl.nrows;
  const int part = (n0 >= bound0) + (n0 >= bound1);                  // (boundaries are multiples of 16: one part a wave)
  const T* wrow = B + ((int64_t)tl.slot * N + n0 + r) * r_pad + kq;
  const T* urow = u + (int64_t)(tl.row0 + (live ? r : 0)) * ldu + (int64_t)part * r_pad + kq;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  typename F::V zero;
#pragma unroll
  for (int e = 0; e < F::VEC; ++e) zero[e] = (T)0.f;
  for (int k = 0; k < r_pad; k += F::KS) {
    const typename F::V w = *reinterpret_cast<const typename F::V*>(wrow + k);
    typename F::V a = *reinterpret_cast<const typename F::V*>(urow + k);
    if (!live) a = zero;
    acc = F::mma(w, a, acc);
  }
  if (live) {
    const float al = alpha[tl.slot];
    typename F::Out* dst = reinterpret_cast<typename F::Out*>(y + (int64_t)(tl.row0 + r) * ldy + n0 + (lane >> 4) * 4);
    f32x4 v = F::unpack(*dst);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(al, acc[e], v[e]);
    *dst = F::pack(v);
  }
}

bool lora_aligned(const void* p, int64_t ld, int dtype, int bytes) {
  const int64_t es = dtype == VY_BF16 ? 2 : 4;
  return ((uintptr_t)p % bytes) == 0 && (ld * es) % bytes == 0;
}

}  // namespace

extern "C" int vy_lora_shrink(const void* x, int64_t ldx, const void* A, const int32_t* tiles, int64_t n_tiles, void* u,
                              int64_t ldu, int64_t T, int64_t K, int64_t R, int64_t slots, int dtype, void* stream) {
  if (n_tiles == 0) return VY_OK;
  if (!x || !A || !tiles || !u) VY_FAIL(VY_ERR_ARG, "vy_lora_shrink: null operand");
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_lora_shrink: bad dtype %d", dtype);
  if (n_tiles < 0 || n_tiles > INT32_MAX || T <= 0 || T > INT32_MAX || slots <= 0 || slots > INT32_MAX)
    VY_FAIL(VY_ERR_ARG, "vy_lora_shrink: bad shape (tiles %lld, T %lld, slots %lld)", (long long)n_tiles, (long long)T,
            (long long)slots);
  if (K <= 0 || K % 32 || K > INT32_MAX || R <= 0 || R % 32 || R / 16 > 65535 || ldx < K || ldu < R)
    VY_FAIL(VY_ERR_ARG, "vy_lora_shrink: bad shape (K %lld and R %lld must be multiples of 32, ldx %lld, ldu %lld)",
            (long long)K, (long long)R, (long long)ldx, (long long)ldu);
  const int out_bytes = dtype == VY_BF16 ? 8 : 16;
  if (!lora_aligned(x, ldx, dtype, 16) || !lora_aligned(A, K, dtype, 16) || !lora_aligned(u, ldu, dtype, out_bytes))
    VY_FAIL(VY_ERR_ARG, "vy_lora_shrink: x and A rows must be 16-byte aligned, u rows %d-byte aligned", out_bytes);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)n_tiles, (unsigned)(R / 16));
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(lora_shrink_kernel<bf16>, grid, dim3(64 * LW), 0, st, (const bf16*)x, ldx, (const bf16*)A, tiles,
                       (bf16*)u, ldu, T, (int)K, (int)R, (int)slots);
  else
    hipLaunchKernelGGL(lora_shrink_kernel<float>, grid, dim3(64 * LW), 0, st, (const float*)x, ldx, (const float*)A, tiles,
                       (float*)u, ldu, T, (int)K, (int)R, (int)slots);
  VY_CHECK_LAUNCH("vy_lora_shrink");
  return VY_OK;
}

extern "C" int vy_lora_expand(void* y, int64_t ldy, const void* u, int64_t ldu, const void* B, const float* alpha,
                              const int32_t* tiles, int64_t n_tiles, int64_t T, int64_t N, int64_t r_pad, int64_t slots,
                              int64_t bound0, int64_t bound1, int dtype, void* stream) {
  if (n_tiles == 0) return VY_OK;
  if (!y || !u || !B || !alpha || !tiles) VY_FAIL(VY_ERR_ARG, "vy_lora_expand: null operand");
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_lora_expand: bad dtype %d", dtype);
  if (n_tiles < 0 || n_tiles > INT32_MAX || T <= 0 || T > INT32_MAX || slots <= 0 || slots > INT32_MAX)
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand: bad shape (tiles %lld, T %lld, slots %lld)", (long long)n_tiles, (long long)T,
            (long long)slots);
  if (N <= 0 || N % 16 || N > INT32_MAX || vy_cdiv(N, 16 * LW) > 65535 || r_pad <= 0 || r_pad % 32 || r_pad > INT32_MAX ||
      ldy < N)
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand: bad shape (N %lld must be a multiple of 16, r_pad %lld of 32, ldy %lld)",
            (long long)N, (long long)r_pad, (long long)ldy);
  // part(n) = (n >= bound0) + (n >= bound1); a boundary that is not used is N
  if (bound0 <= 0 || bound0 > N || bound1 < bound0 || bound1 > N || bound0 % 16 || bound1 % 16)
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand: boundaries %lld, %lld must be multiples of 16 with 0 < b0 <= b1 <= N = %lld",
            (long long)bound0, (long long)bound1, (long long)N);
  const int64_t parts = 1 + (bound0 < N) + (bound1 < N);
  if (ldu < parts * r_pad)
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand: ldu %lld is below %lld parts of r_pad %lld", (long long)ldu, (long long)parts,
            (long long)r_pad);
  const int out_bytes = dtype == VY_BF16 ? 8 : 16;
  if (!lora_aligned(u, ldu, dtype, 16) || !lora_aligned(B, r_pad, dtype, 16) || !lora_aligned(y, ldy, dtype, out_bytes))
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand: u and B rows must be 16-byte aligned, y rows %d-byte aligned", out_bytes);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)n_tiles, (unsigned)vy_cdiv(N, 16 * LW));
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(lora_expand_kernel<bf16>, grid, dim3(64 * LW), 0, st, (bf16*)y, ldy, (const bf16*)u, ldu,
                       (const bf16*)B, alpha, tiles, T, (int)N, (int)r_pad, (int)slots, (int)bound0, (int)bound1);
  else
    hipLaunchKernelGGL(lora_expand_kernel<float>, grid, dim3(64 * LW), 0, st, (float*)y, ldy, (const float*)u, ldu,
                       (const float*)B, alpha, tiles, T, (int)N, (int)r_pad, (int)slots, (int)bound0, (int)bound1);
  VY_CHECK_LAUNCH("vy_lora_expand");
  return VY_OK;
}
