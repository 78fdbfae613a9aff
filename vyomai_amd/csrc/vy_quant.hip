// Row quantiser of the fp8-weight decode step: W (N, K) bf16 / fp32 -> (N, K) OCP e4m3fn codes + one fp32 scale per row.
// The rule is the KV pages' (paged_quant_write_fp8_kernel, vy_paged.hip), per output row instead of per head:
//   s = amax > 0 ? amax / 448 : 1 ;  code = cvt_pk_fp8_f32(clamp(w / s, -448, 448))   (IEEE division, nearest even)
// One workgroup per row, the row read twice (amax, then the codes); no atomics.  Runs once per plan build, never per token.
#include "vy_common.h"
#include "vy_wave.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const T* __restrict__ w, long long ldw,
                                                             unsigned char* __restrict__ codes, long long ldc,
                                                             float* __restrict__ scales, int K) {
  __shared__ float red[4];
  const long long row = blockIdx.x;
  const T* wr = w + row * ldw;
  const int quads = K >> 2;
  float amax = 0.f;
  for (int qd = threadIdx.x; qd < quads; qd += 256) {
#pragma unroll
    for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf((float)wr[4 * qd + e]));
  }
  amax = dec_wave_max(amax);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float s = amax > 0.f ? amax / 448.0f : 1.0f;
  unsigned* cr = reinterpret_cast<unsigned*>(codes + row * ldc);
  for (int qd = threadIdx.x; qd < quads; qd += 256) {
    float c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = fminf(fmaxf((float)wr[4 * qd + e] / s, -448.0f), 448.0f);
    int d = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
    d = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], d, true);
    cr[qd] = (unsigned)d;
  }
  if (threadIdx.x == 0) scales[row] = s;
}

}  // namespace

extern "C" int vy_quant_rows_fp8(const void* w, int64_t ldw, void* codes, int64_t ldc, float* scales, int64_t N, int64_t K,
                                 int dtype, void* stream) {
  const char* who = "vy_quant_rows_fp8";
  if (!w || !codes || !scales) VY_FAIL(VY_ERR_ARG, "%s: null operand", who);
  if (N <= 0 || K <= 0 || N > 0x7fffffffLL || K > 0x7fffffffLL || ldw < K || ldc < K) VY_FAIL(VY_ERR_ARG, "%s: bad shape", who);
  // a thread stores four codes as one dword
  if (K % 4 || ldc % 4 || ((uintptr_t)codes & 3)) VY_FAIL(VY_ERR_UNSUPPORTED, "%s: K, ldc and the codes need 4-byte granularity", who);
  const dim3 grid((unsigned)N), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(quant_rows_fp8_kernel<bf16>, grid, block, 0, st, (const bf16*)w, (long long)ldw, (unsigned char*)codes,
                       (long long)ldc, scales, (int)K);
  else if (dtype == VY_F32)
    hipLaunchKernelGGL(quant_rows_fp8_kernel<float>, grid, block, 0, st, (const float*)w, (long long)ldw, (unsigned char*)codes,
                       (long long)ldc, scales, (int)K);
  else VY_FAIL(VY_ERR_ARG, "%s: bad dtype %d", who, dtype);
  VY_CHECK_LAUNCH(who);
  return VY_OK;
}
