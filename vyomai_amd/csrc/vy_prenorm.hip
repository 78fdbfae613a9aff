// Backward streaming kernels of the pre-norm residual blocks (RMSNorm -> attention / gated MLP -> residual add):
// vy_rmsnorm_bwd and vy_gated_act_bwd.  Both are one pass over their operands with 16-byte accesses per lane;
// the RMSNorm backward keeps the row in registers (one wave per row) like rmsnorm_fwd_kernel / layernorm_bwd_kernel.
#include "vy_common.h"

namespace {

// ---- RMSNorm backward ----------------------------------------------------------------------
// y = x r (w_offset + w), r = rsqrt(mean x^2 + eps); with g = w_offset + w:
//   dx = r g dy - x r^3 / N * sum(x g dy) (+ add_to)        dw[n] = sum_rows dy x r
// No saved statistics: sum x^2 and sum x g dy come out of the same pass over the registers, r takes the Newton step
// of the forward.  Wave w of the grid walks rows w, w + W, ...; a lane always owns the same columns, so the dw
// partials accumulate in registers; the block's 4 waves are summed through LDS and one slab row per block goes to ws.
// PIPE (rows up to 4 chunks per lane): the loads of the next row are issued before the reductions of the current
// one and the weights stay in registers.  Wider rows hold too much for that: the weights are re-read per row (they
// stay in L1 / L2) and the loads are not pipelined.
template <typename T, int CH, bool PIPE>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(
    const T* __restrict__ dy, int64_t lddy, const T* __restrict__ x, int64_t ldx, const T* __restrict__ w,
    const T* __restrict__ add_to, int64_t ldadd, T* __restrict__ dx, int64_t lddx, float* __restrict__ ws,
    int64_t M, int N, int W, float eps, float w_offset) {
  constexpr int VEC = Chunk<T>::VEC;
  typedef typename Chunk<T>::Raw Raw;
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nch = N / VEC;
  float dw[CH][VEC];
  float g[PIPE ? CH : 1][VEC];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = lane + 64 * c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) dw[c][e] = 0.f;
    if constexpr (PIPE) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) g[c][e] = 0.f;
      if (ch < nch) {
        Chunk<T>::load(w + (int64_t)ch * VEC, g[c]);
#pragma unroll
        for (int e = 0; e < VEC; ++e) g[c][e] += w_offset;
      }
    }
  }
  Raw xr[CH], dr[CH], xn[PIPE ? CH : 1], dn[PIPE ? CH : 1];
  auto fetch = [&](int64_t row, Raw* xa, Raw* da) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = lane + 64 * c;
      if (ch < nch) {
        xa[c] = *reinterpret_cast<const Raw*>(x + row * ldx + (int64_t)ch * VEC);
        da[c] = *reinterpret_cast<const Raw*>(dy + row * lddy + (int64_t)ch * VEC);
      }
    }
  };
  if constexpr (PIPE) {
    if (wid < M) fetch(wid, xr, dr);
  }
  for (int64_t row = wid; row < M; row += W) {
    const bool more = row + W < M;
    if constexpr (PIPE) {
      if (more) fetch(row + W, xn, dn);
    } else {
      fetch(row, xr, dr);
    }
    float q = 0.f, s = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = lane + 64 * c;
      if (ch < nch) {
        float xv[VEC], dv[VEC], gv[VEC];
        Chunk<T>::unpack(xr[c], xv);
        Chunk<T>::unpack(dr[c], dv);
        if constexpr (!PIPE) Chunk<T>::load(w + (int64_t)ch * VEC, gv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float ge = PIPE ? g[PIPE ? c : 0][e] : w_offset + gv[e];
          q += xv[e] * xv[e];
          s += xv[e] * ge * dv[e];
        }
      }
    }
    const float ms = vy_wave_sum(q) / (float)N + eps;
    float r = rsqrtf(ms);
    r = r * (1.5f - 0.5f * ms * r * r);
    const float cf = r * r * r * (vy_wave_sum(s) / (float)N);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = lane + 64 * c;
      if (ch < nch) {
        float xv[VEC], dv[VEC], gv[VEC], o[VEC];
        Chunk<T>::unpack(xr[c], xv);
        Chunk<T>::unpack(dr[c], dv);
        if constexpr (!PIPE) Chunk<T>::load(w + (int64_t)ch * VEC, gv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float ge = PIPE ? g[PIPE ? c : 0][e] : w_offset + gv[e];
          o[e] = r * ge * dv[e] - xv[e] * cf;
          dw[c][e] += dv[e] * xv[e] * r;
        }
        if (add_to) {
          float av[VEC];
          Chunk<T>::load(add_to + row * ldadd + (int64_t)ch * VEC, av);
#pragma unroll
          for (int e = 0; e < VEC; ++e) o[e] += av[e];
        }
        Chunk<T>::store(dx + row * lddx + (int64_t)ch * VEC, o);
      }
    }
    if constexpr (PIPE) {
      if (more) {
#pragma unroll
        for (int c = 0; c < CH; ++c) { xr[c] = xn[c]; dr[c] = dn[c]; }
      }
    }
  }
  // waves 1..3 hand their partials to wave 0 through LDS, one chunk at a time (a whole row of partials of the
  // widest instantiation would not fit); wave 0 adds them in wave order and writes the block's slab row
  __shared__ float red[3][VEC * 64];
  const int wv = threadIdx.x >> 6;
  float* slab = ws + (int64_t)blockIdx.x * N;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = lane + 64 * c;
    if (wv > 0) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) red[wv - 1][e * 64 + lane] = dw[c][e];
    }
    __syncthreads();
    if (wv == 0 && ch < nch) {
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = ((dw[c][e] + red[0][e * 64 + lane]) + red[1][e * 64 + lane]) + red[2][e * 64 + lane];
#pragma unroll
      for (int e0 = 0; e0 < VEC; e0 += 4) Chunk<float>::store(slab + (int64_t)ch * VEC + e0, o + e0);
    }
    __syncthreads();
  }
}

template <typename T>
int rms_bwd_dispatch(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* w, const void* add_to,
                     int64_t ldadd, void* dx, int64_t lddx, float* dw, float beta, float* ws, int64_t M, int64_t N,
                     float eps, float w_offset, hipStream_t st) {
  constexpr int VEC = Chunk<T>::VEC;
  const int nch = (int)(N / VEC);
  const int WB = (int)vy_layernorm_bwd_ws_rows(M);  // blocks = slab rows
  const int W = WB * 4;
  const dim3 grid((unsigned)WB), block(256);
#define RMS_GO(CH, PIPE)                                                                                       \
  hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, CH, PIPE>), grid, block, 0, st, (const T*)dy, lddy, (const T*)x, ldx, \
                     (const T*)w, (const T*)add_to, ldadd, (T*)dx, lddx, ws, M, (int)N, W, eps, w_offset)
  if (nch <= 64) RMS_GO(1, true);
  else if (nch <= 128) RMS_GO(2, true);
  else if (nch <= 256) RMS_GO(4, true);
  else if (nch <= 512) RMS_GO(8, false);
  else RMS_GO(16, false);
#undef RMS_GO
  VY_CHECK_LAUNCH("vy_rmsnorm_bwd");
  // dw: the ordered column sum of the one [WB][N] slab (vy_colsum.h), sliced as the LayerNorm backward's
  return vy_colsum("vy_rmsnorm_bwd", ws, 1, 0, (int)N, WB, (int)N, vy_ln_colsum_slices(WB), dw, nullptr, beta == 1.f, st);
}

// ---- gated activation backward ---------------------------------------------------------------
// out = act(gate) * up  ->  d_gate = d_out * up * act'(gate), d_up = d_out * act(gate); d_gate_up has gate_up's
// [gate | up] layout.  bf16 takes the reduced-cost functors (their error is below bf16 rounding), fp32 the exact
// ones (the 1e-5 parity path), as act_bwd_kernel does.
template <typename T, int ACT>
__global__ void gated_act_bwd_kernel(const T* __restrict__ dout, int64_t lddo, const T* __restrict__ gu, int64_t ldg,
                                     T* __restrict__ dgu, int64_t lddg, int64_t M, int I, int code) {
  constexpr int VEC = Chunk<T>::VEC;
  const int nch = I / VEC;
  const int64_t total = M * nch;
  vy_act_dispatch<ACT>(code, [&](auto a_) {
    constexpr int A = decltype(a_)::value;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t m = i / nch;
      const int c = (int)(i - m * nch) * VEC;
      float d[VEC], a[VEC], b[VEC], og[VEC], ou[VEC];
      Chunk<T>::load(dout + m * lddo + c, d);
      Chunk<T>::load(gu + m * ldg + c, a);
      Chunk<T>::load(gu + m * ldg + I + c, b);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float f, df;
        if constexpr (sizeof(T) == 2) { f = vy_act_fwd_fast<A>(a[e]); df = vy_act_grad_fast<A>(a[e]); }
        else { f = vy_act_fwd<A>(a[e]); df = vy_act_grad<A>(a[e]); }
        og[e] = d[e] * b[e] * df;
        ou[e] = d[e] * f;
      }
      Chunk<T>::store(dgu + m * lddg + c, og);
      Chunk<T>::store(dgu + m * lddg + I + c, ou);
    }
  });
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int vy_rmsnorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* w,
                              const void* add_to, int64_t ldadd, void* dx, int64_t lddx, float* dw, float beta,
                              float* ws, int64_t M, int64_t N, float eps, float w_offset, int dtype, void* stream) {
  if (!dy || !x || !w || !dx || !dw || !ws || M <= 0 || N <= 0) VY_FAIL(VY_ERR_ARG, "vy_rmsnorm_bwd: null operand or empty shape");
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_rmsnorm_bwd: bad dtype %d", dtype);
  if (beta != 0.f && beta != 1.f) VY_FAIL(VY_ERR_ARG, "vy_rmsnorm_bwd: beta must be 0 or 1");
  const int vec = dtype == VY_BF16 ? 8 : 4;
  if (N % vec || ldx % vec || lddy % vec || lddx % vec || (add_to && ldadd % vec))
    VY_FAIL(VY_ERR_ARG, "vy_rmsnorm_bwd: N/ld must be multiples of %d", vec);
  if (ldx < N || lddy < N || lddx < N || (add_to && ldadd < N)) VY_FAIL(VY_ERR_ARG, "vy_rmsnorm_bwd: row stride below N");
  if (!aligned16(dy) || !aligned16(x) || !aligned16(w) || !aligned16(dx) || !aligned16(add_to) || !aligned16(ws))
    VY_FAIL(VY_ERR_ARG, "vy_rmsnorm_bwd: operands must be 16-byte aligned");
  if (N / vec > 1024) VY_FAIL(VY_ERR_UNSUPPORTED, "vy_rmsnorm_bwd: N=%ld too wide", (long)N);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VY_BF16)
    return rms_bwd_dispatch<bf16>(dy, lddy, x, ldx, w, add_to, ldadd, dx, lddx, dw, beta, ws, M, N, eps, w_offset, st);
  return rms_bwd_dispatch<float>(dy, lddy, x, ldx, w, add_to, ldadd, dx, lddx, dw, beta, ws, M, N, eps, w_offset, st);
}

extern "C" int vy_gated_act_bwd(const void* d_act, int64_t lddo, const void* gate_up, int64_t ldg, void* d_gate_up,
                                int64_t lddg, int64_t M, int64_t I, int act, int dtype, void* stream) {
  if (!d_act || !gate_up || !d_gate_up || M <= 0 || I <= 0) VY_FAIL(VY_ERR_ARG, "vy_gated_act_bwd: null operand or empty shape");
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_gated_act_bwd: bad dtype %d", dtype);
  if (act != VY_ACT_GELU_ERF && act != VY_ACT_GELU_TANH && !vy_act_is_runtime(act))
    VY_FAIL(VY_ERR_ARG, "vy_gated_act_bwd: unsupported act %d", act);
  const int vec = dtype == VY_BF16 ? 8 : 4;
  if (I % vec || lddo % vec || ldg % vec || lddg % vec) VY_FAIL(VY_ERR_ARG, "vy_gated_act_bwd: I/ld must be multiples of %d", vec);
  if (lddo < I || ldg < 2 * I || lddg < 2 * I) VY_FAIL(VY_ERR_ARG, "vy_gated_act_bwd: row stride below the row width");
  if (!aligned16(d_act) || !aligned16(gate_up) || !aligned16(d_gate_up))
    VY_FAIL(VY_ERR_ARG, "vy_gated_act_bwd: operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t want = vy_cdiv(M * (I / vec), 256);
  const dim3 grid((unsigned)(want < 8192 ? want : 8192)), block(256);
#define GB_GO(T, A)                                                                                               \
  hipLaunchKernelGGL((gated_act_bwd_kernel<T, A>), grid, block, 0, st, (const T*)d_act, lddo, (const T*)gate_up, ldg, \
                     (T*)d_gate_up, lddg, M, (int)I, act)
  if (dtype == VY_BF16 && act == VY_ACT_GELU_ERF) GB_GO(bf16, VY_ACT_GELU_ERF);
  else if (dtype == VY_BF16 && act == VY_ACT_GELU_TANH) GB_GO(bf16, VY_ACT_GELU_TANH);
  else if (dtype == VY_F32 && act == VY_ACT_GELU_ERF) GB_GO(float, VY_ACT_GELU_ERF);
  else if (dtype == VY_F32 && act == VY_ACT_GELU_TANH) GB_GO(float, VY_ACT_GELU_TANH);
  else if (dtype == VY_BF16) GB_GO(bf16, VY_ACT_RUNTIME);
  else GB_GO(float, VY_ACT_RUNTIME);
#undef GB_GO
  VY_CHECK_LAUNCH("vy_gated_act_bwd");
  return VY_OK;
}
