// Per-request LoRA delta of a serving step (serving.ContinuousBatchEngine with adapters=): after a projection's own
// GEMM, y[t, :] += alpha[s] * (x[t, :] @ A[s].T) @ B[s].T for the rows t of requests that carry adapter slot s
// (reference layers/adapters.py LoraLinear.forward: linear(x) + scale * F.linear(F.linear(x, lora_a), lora_b)).
//   vy_lora_shrink   u[t, 0:R] = x[t, 0:K] @ A[slot].T          one workgroup per (tile, 16 columns of R)
//   vy_lora_expand   y[t, n] += alpha[slot] * u[t, part(n)] . B[slot][n]   one wave per (tile, 16 columns of N)
//   vy_lora_expand_epi   the same tile, then the activation or the dropout + residual of the GEMM it follows
//                        (encoder LoRA fine-tuning: the reference applies the adapter before either)
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

// The expand tile both expand kernels share: wave w of a workgroup owns columns 16 (LW blockIdx.y + w) .. + 15 of the
// tile's rows.  false: nothing to do (a skipped tile, columns past N); otherwise acc holds the four sums of row
// tl.row0 + (lane & 15), columns n0 + 4 (lane >> 4) + reg -- zeros in a dead lane (live false), which stores nothing.
template <typename T>
__device__ __forceinline__ bool lora_expand_tile(const T* __restrict__ u, int64_t ldu, const T* __restrict__ B,
                                                 const int32_t* __restrict__ tiles, int64_t rows, int N, int r_pad,
                                                 int slots, int bound0, int bound1, LoraTile& tl, int& n0, bool& live,
                                                 f32x4& acc) {
  using F = LoraFrag<T>;
  if (!lora_tile(tiles, blockIdx.x, rows, slots, tl)) return false;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  n0 = (blockIdx.y * LW + wave) * 16;
  if (n0 >= N) return false;                                         // (no barrier in these kernels)
  const int r = lane & 15, kq = (lane >> 4) * F::VEC;
  live = r < tl.nrows;
  const int part = (n0 >= bound0) + (n0 >= bound1);                  // (boundaries are multiples of 16: one part a wave)
  const T* wrow = B + ((int64_t)tl.slot * N + n0 + r) * r_pad + kq;
  const T* urow = u + (int64_t)(tl.row0 + (live ? r : 0)) * ldu + (int64_t)part * r_pad + kq;
  acc = f32x4{0.f, 0.f, 0.f, 0.f};
  typename F::V zero;
#pragma unroll
  for (int e = 0; e < F::VEC; ++e) zero[e] = (T)0.f;
  for (int k = 0; k < r_pad; k += F::KS) {
    const typename F::V w = *reinterpret_cast<const typename F::V*>(wrow + k);
    typename F::V a = *reinterpret_cast<const typename F::V*>(urow + k);
    if (!live) a = zero;
    acc = F::mma(w, a, acc);
  }
  return true;
}

// grid (n_tiles, ceil(N / 16 / LW))
template <typename T>
__global__ __launch_bounds__(64 * LW) void lora_expand_kernel(T* __restrict__ y, int64_t ldy, const T* __restrict__ u,
                                                              int64_t ldu, const T* __restrict__ B,
                                                              const float* __restrict__ alpha,
                                                              const int32_t* __restrict__ tiles, int64_t rows, int N,
                                                              int r_pad, int slots, int bound0, int bound1) {
  using F = LoraFrag<T>;
  LoraTile tl;
  int n0;
  bool live;
  f32x4 acc;
  if (!lora_expand_tile(u, ldu, B, tiles, rows, N, r_pad, slots, bound0, bound1, tl, n0, live, acc)) return;
  if (live) {
    const int lane = threadIdx.x & 63, r = lane & 15;
    const float al = alpha[tl.slot];
    typename F::Out* dst = reinterpret_cast<typename F::Out*>(y + (int64_t)(tl.row0 + r) * ldy + n0 + (lane >> 4) * 4);
    f32x4 v = F::unpack(*dst);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(al, acc[e], v[e]);
    *dst = F::pack(v);
  }
}

// vy_lora_expand_epi: the expand tile with the epilogue of the GEMM it follows.  v = fmaf(alpha, acc, z) in fp32 is
// never rounded before the epilogue.  z and out may be the same buffer (every element is read and written by one
// lane), so neither is __restrict__.
//   MODE VY_LORA_EPI_ACT       out = act(v), pre = act'(v)            (ACT: a vy_act or VY_ACT_RUNTIME with `code`)
//   MODE VY_LORA_EPI_DROP_RES  out = keep(row, col) ? v * scale + res : res; thr == 0: v + res
//   MODE VY_LORA_EPI_MUL       out = v * pre                          (the backward's twin of ACT: pre is read)
// A lane's four columns are one half of an 8-column Philox chunk: the lot of column c is lot c & 7 of chunk c >> 3.
template <typename T, int MODE, int ACT>
__global__ __launch_bounds__(64 * LW) void lora_expand_epi_kernel(const T* z, int64_t ldz, T* out, int64_t ldo, T* pre,
                                                                  int64_t ldp, const T* res, int64_t ldr,
                                                                  const T* __restrict__ u, int64_t ldu,
                                                                  const T* __restrict__ B, const float* __restrict__ alpha,
                                                                  const int32_t* __restrict__ tiles, int64_t rows, int N,
                                                                  int r_pad, int slots, int bound0, int bound1, int code,
                                                                  VyDrop d) {
  using F = LoraFrag<T>;
  LoraTile tl;
  int n0;
  bool live;
  f32x4 acc;
  if (!lora_expand_tile(u, ldu, B, tiles, rows, N, r_pad, slots, bound0, bound1, tl, n0, live, acc)) return;
  if (!live) return;
  const int lane = threadIdx.x & 63;
  const int64_t row = tl.row0 + (lane & 15);
  const int col = n0 + (lane >> 4) * 4;
  const float al = alpha[tl.slot];
  f32x4 v = F::unpack(*reinterpret_cast<const typename F::Out*>(z + row * ldz + col));
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = fmaf(al, acc[e], v[e]);
  if constexpr (MODE == VY_LORA_EPI_ACT) {
    f32x4 h, g;
    vy_act_dispatch<ACT>(code, [&](auto a) {
      constexpr int A = decltype(a)::value;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h[e] = vy_act_fwd<A>(v[e]);
        g[e] = vy_act_grad<A>(v[e]);
      }
    });
    *reinterpret_cast<typename F::Out*>(out + row * ldo + col) = F::pack(h);
    *reinterpret_cast<typename F::Out*>(pre + row * ldp + col) = F::pack(g);
  } else if constexpr (MODE == VY_LORA_EPI_MUL) {
    const f32x4 g = F::unpack(*reinterpret_cast<const typename F::Out*>(pre + row * ldp + col));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= g[e];
    *reinterpret_cast<typename F::Out*>(out + row * ldo + col) = F::pack(v);
  } else {
    const f32x4 rs = F::unpack(*reinterpret_cast<const typename F::Out*>(res + row * ldr + col));
    f32x4 s;
    if (d.thr == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = v[e] + rs[e];
    } else {
      uint32_t lots[4];
      vy_drop_lots(d, row, col >> 3, lots);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = vy_drop_keep(d, lots, (col + e) & 7) ? v[e] * d.scale + rs[e] : rs[e];
    }
    *reinterpret_cast<typename F::Out*>(out + row * ldo + col) = F::pack(s);
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

namespace {

template <typename T>
int lora_expand_epi_launch(const void* z, int64_t ldz, void* out, int64_t ldo, void* pre, int64_t ldp, const void* res,
                           int64_t ldr, const void* u, int64_t ldu, const void* B, const float* alpha,
                           const int32_t* tiles, dim3 grid, int64_t T_, int N, int r_pad, int slots, int bound0, int bound1,
                           int mode, int act, const VyDrop& d, hipStream_t st) {
#define EPI_GO(MODE, ACT)                                                                                              \
  hipLaunchKernelGGL((lora_expand_epi_kernel<T, MODE, ACT>), grid, dim3(64 * LW), 0, st, (const T*)z, ldz, (T*)out, ldo, \
                     (T*)pre, ldp, (const T*)res, ldr, (const T*)u, ldu, (const T*)B, alpha, tiles, T_, N, r_pad, slots,  \
                     bound0, bound1, act, d)
  if (mode == VY_LORA_EPI_DROP_RES) EPI_GO(VY_LORA_EPI_DROP_RES, VY_ACT_NONE);
  else if (mode == VY_LORA_EPI_MUL) EPI_GO(VY_LORA_EPI_MUL, VY_ACT_NONE);
  else if (act == VY_ACT_GELU_ERF) EPI_GO(VY_LORA_EPI_ACT, VY_ACT_GELU_ERF);
  else if (act == VY_ACT_GELU_TANH) EPI_GO(VY_LORA_EPI_ACT, VY_ACT_GELU_TANH);
  else EPI_GO(VY_LORA_EPI_ACT, VY_ACT_RUNTIME);
#undef EPI_GO
  VY_CHECK_LAUNCH("vy_lora_expand_epi");
  return VY_OK;
}

}  // namespace

extern "C" int vy_lora_expand_epi(const void* z, int64_t ldz, void* out, int64_t ldo, void* pre, int64_t ldp,
                                  const void* res, int64_t ldr, const void* u, int64_t ldu, const void* B,
                                  const float* alpha, const int32_t* tiles, int64_t n_tiles, int64_t T, int64_t N,
                                  int64_t r_pad, int64_t slots, int64_t bound0, int64_t bound1, int mode, int act,
                                  float p_drop, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  if (n_tiles == 0) return VY_OK;
  if (!z || !out || !u || !B || !alpha || !tiles) VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: null operand");
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: bad dtype %d", dtype);
  if (mode == VY_LORA_EPI_ACT) {
    if (act != VY_ACT_GELU_ERF && act != VY_ACT_GELU_TANH && !vy_act_is_runtime(act))
      VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: ACT mode takes every vy_act but VY_ACT_NONE, got %d", act);
    if (!pre || ldp < N) VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: ACT mode writes pre (ldp %lld)", (long long)ldp);
  } else if (mode == VY_LORA_EPI_DROP_RES) {
    if (!res || ldr < N) VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: DROP_RES mode reads res (ldr %lld)", (long long)ldr);
    if (!(p_drop >= 0.f && p_drop < 1.f)) VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: p_drop=%g outside [0, 1)", (double)p_drop);
  } else if (mode == VY_LORA_EPI_MUL) {
    if (!pre || ldp < N) VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: MUL mode reads pre (ldp %lld)", (long long)ldp);
  } else {
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: bad mode %d", mode);
  }
  if (n_tiles < 0 || n_tiles > INT32_MAX || T <= 0 || T > INT32_MAX || slots <= 0 || slots > INT32_MAX)
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: bad shape (tiles %lld, T %lld, slots %lld)", (long long)n_tiles, (long long)T,
            (long long)slots);
  if (N <= 0 || N % 16 || N > INT32_MAX || vy_cdiv(N, 16 * LW) > 65535 || r_pad <= 0 || r_pad % 32 || r_pad > INT32_MAX ||
      ldz < N || ldo < N)
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: bad shape (N %lld must be a multiple of 16, r_pad %lld of 32, ldz %lld, ldo %lld)",
            (long long)N, (long long)r_pad, (long long)ldz, (long long)ldo);
  if (bound0 <= 0 || bound0 > N || bound1 < bound0 || bound1 > N || bound0 % 16 || bound1 % 16)
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: boundaries %lld, %lld must be multiples of 16 with 0 < b0 <= b1 <= N = %lld",
            (long long)bound0, (long long)bound1, (long long)N);
  const int64_t parts = 1 + (bound0 < N) + (bound1 < N);
  if (ldu < parts * r_pad)
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: ldu %lld is below %lld parts of r_pad %lld", (long long)ldu, (long long)parts,
            (long long)r_pad);
  const int out_bytes = dtype == VY_BF16 ? 8 : 16;
  if (!lora_aligned(u, ldu, dtype, 16) || !lora_aligned(B, r_pad, dtype, 16) || !lora_aligned(z, ldz, dtype, out_bytes) ||
      !lora_aligned(out, ldo, dtype, out_bytes) || (pre && !lora_aligned(pre, ldp, dtype, out_bytes)) ||
      (res && !lora_aligned(res, ldr, dtype, out_bytes)))
    VY_FAIL(VY_ERR_ARG, "vy_lora_expand_epi: u and B rows must be 16-byte aligned, z / out / pre / res rows %d-byte aligned",
            out_bytes);
  const VyDrop d = vy_make_drop(mode == VY_LORA_EPI_DROP_RES ? p_drop : 0.f, seed, offset);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)n_tiles, (unsigned)vy_cdiv(N, 16 * LW));
  if (dtype == VY_BF16)
    return lora_expand_epi_launch<bf16>(z, ldz, out, ldo, pre, ldp, res, ldr, u, ldu, B, alpha, tiles, grid, T, (int)N,
                                        (int)r_pad, (int)slots, (int)bound0, (int)bound1, mode, act, d, st);
  return lora_expand_epi_launch<float>(z, ldz, out, ldo, pre, ldp, res, ldr, u, ldu, B, alpha, tiles, grid, T, (int)N,
                                       (int)r_pad, (int)slots, (int)bound0, (int)bound1, mode, act, d, st);
}
