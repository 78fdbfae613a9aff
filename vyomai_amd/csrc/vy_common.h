// Common device/host helpers for libvyom_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <stdio.h>
#include <math.h>
#include "../../include/vyom_hip.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define VY_LDS __attribute__((address_space(3)))
#define VY_GLOBAL __attribute__((address_space(1)))

// ---- transposing LDS reads that the compiler's waitcnt pass cannot see ----------------------
// hipcc cannot tell what the ds_read_b64_tr_b16 *builtin* aliases, so whenever LDS-DMA
// (global_load ... lds, counted by vmcnt) is in flight it puts s_waitcnt vmcnt(0) in front of the
// read: the prefetch of the next tile is drained before the current tile's MFMAs even start.
// The asm form is invisible to that pass.  Its result is NOT tracked either: retire the reads with
// vy_lgkm_wait<N>(frags...) (N = LDS reads issued after the ones needed) before the first use.
// A compiler-issued lgkmcnt wait in between only ever over-waits (LDS returns in order).
__device__ __forceinline__ s16x4 vy_lds_tr16(const char* p) {
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"((unsigned)(uintptr_t)(VY_LDS const char*)p) : "memory");
  return r;
}
// the same with a compile-time byte offset in the instruction's 16-bit offset field: the asm form
// hides the address from the compiler, so it cannot fold constants into that field itself and would
// spend a v_add per read
template <int OFF>
__device__ __forceinline__ s16x4 vy_lds_tr16_off(unsigned lds_addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field is 16 bits");
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lds_addr), "n"(OFF) : "memory");
  return r;
}
template <int OFF0, int OFF1>
__device__ __forceinline__ bf16x8 vy_lds_tr16_pair_off(unsigned lds_addr) {
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = vy_lds_tr16_off<OFF0>(lds_addr);
  u.s.b = vy_lds_tr16_off<OFF1>(lds_addr);
  return u.v;
}
// ds_read_b128 in the same hidden form: hipcc retires its own LDS reads with lgkmcnt(0), which also
// waits for the fragments just requested for the NEXT k-step; hidden reads are retired by the caller
// with a counted lgkmcnt, so a k-step's MFMAs wait only for their own operands.
template <int OFF>
__device__ __forceinline__ bf16x8 vy_lds_read128_off(unsigned lds_addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field is 16 bits");
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(lds_addr), "n"(OFF) : "memory");
  return r;
}
__device__ __forceinline__ unsigned vy_lds_addr(const char* p) { return (unsigned)(uintptr_t)(VY_LDS const char*)p; }
// rows r and r+8 of a transposed 16-row block -> one MFMA A/B fragment (2 LDS reads, no wait)
__device__ __forceinline__ bf16x8 vy_lds_tr16_pair(const char* p0, const char* p1) {
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = vy_lds_tr16(p0);
  u.s.b = vy_lds_tr16(p1);
  return u.v;
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): a loop whose index is a constant
// expression in the body (instruction offset fields, register-array indices)
template <int N, typename F>
__device__ __forceinline__ void vy_static_for(F&& f) {
  if constexpr (N > 0) {
    vy_static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}
template <typename T>
__device__ __forceinline__ void vy_tie(T& v) { asm volatile("" : "+v"(v)); }
template <int N, typename... T>
__device__ __forceinline__ void vy_lgkm_wait(T&... v) {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  // tie every fragment to this point: the MFMAs that read them cannot be scheduled above the wait
  (vy_tie(v), ...);
}

// host-side error plumbing -------------------------------------------------------------
void vy_set_error(const char* fmt, ...);
#define VY_FAIL(code, ...)      \
  do {                          \
    vy_set_error(__VA_ARGS__);  \
    return (code);              \
  } while (0)
#define VY_CHECK_LAUNCH(name)                                             \
  do {                                                                    \
    hipError_t e_ = hipGetLastError();                                    \
    if (e_ != hipSuccess)                                                 \
      VY_FAIL(VY_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e_));      \
  } while (0)

static inline int64_t vy_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Row slices of a LayerNorm- or RMSNorm-backward slab of WB rows; the order of the sum itself is stated in vy_colsum.h.
static inline int vy_ln_colsum_slices(int WB) { return WB >= 64 ? 16 : 1; }
// internal (vy_misc.hip): the ordered column sums of S = 1 or 2 slabs, W rows in `slices` slices, as launches of their
// own; out0 / out1 may be null.  With several slices the first row of each slice is overwritten with the slice's sum.
// `who` names the caller in a launch error.
int vy_colsum(const char* who, float* ws, int S, int64_t slab_stride, int ld, int W, int N, int slices, float* out0,
              float* out1, int acc, hipStream_t st);

// 16 zero bytes: source for out-of-range chunks of LDS-DMA loads (one copy per translation unit:
// the library is built without relocatable device code).
static __device__ __attribute__((aligned(16))) uint32_t vy_zero16[4] = {0, 0, 0, 0};

// ---- AdamW, one element group ----------------------------------------------------------------
// The per-element update of vy_adamw_step, shared by adamw_kernel (vy_misc.hip) and the AdamW workgroups that ride in
// the grouped weight-gradient launch (vy_bwd.hip): one body, so both give the same bits.  The launch-uniform scalars:
struct VyAdamwScalars { float lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale; };

// One element:  g' = g gscale;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g' g';
//               p = p (1 - lr wd) - (lr / bc1) (m / (sqrt(v) / bc2_sqrt + eps)).
// Which products are fused into an fma is spelled out and contraction is off: left to the compiler it depends on the
// code around the call (the riders' copy differed from adamw_kernel's by an ulp of v).  The spelling is the one the
// compiler had chosen for adamw_kernel when the update lived there, so its results are what they were -- including
// that the groups of four and the element-wise tail fuse the second moment differently (VEC).
template <bool VEC>
__device__ __forceinline__ void vy_adamw_element(float& p, float g, float& m, float& v, const VyAdamwScalars& s) {
#pragma clang fp contract(off)
  const float keep = __builtin_fmaf(-s.lr, s.wd, 1.0f);
  const float rate = s.lr / s.bc1;
  const float gg = g * s.gscale;
  const float t = (1.0f - s.b2) * gg;
  m = __builtin_fmaf(1.0f - s.b1, gg, s.b1 * m);
  v = VEC ? __builtin_fmaf(s.b2, v, t * gg) : __builtin_fmaf(t, gg, s.b2 * v);
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = __builtin_fmaf(keep, p, -(rate * (m / denom)));
}

// Four consecutive elements.  The optimizer state is touched once per step: streamed both ways (nt), so that it does
// not take the Infinity Cache away from the backward kernels' hand-offs.  The bf16 working copy keeps the default
// policy: the next forward reads it.  load / step / store are separate so that a caller can have several groups'
// loads in flight before the first use.
struct VyAdamw4 {
  f32x4 p, g, m, v;
  __device__ __forceinline__ void load(const float* pp, const float* gp, const float* mp, const float* vp) {
    p = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pp));
    g = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(gp));
    m = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(mp));
    v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vp));
  }
  __device__ __forceinline__ void step(const VyAdamwScalars& s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = p[e], me = m[e], ve = v[e];
      vy_adamw_element<true>(pe, g[e], me, ve, s);
      p[e] = pe; m[e] = me; v[e] = ve;
    }
  }
  __device__ __forceinline__ void store(float* pp, float* mp, float* vp, bf16* pb) const {
    __builtin_nontemporal_store(p, reinterpret_cast<f32x4*>(pp));
    __builtin_nontemporal_store(m, reinterpret_cast<f32x4*>(mp));
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(vp));
    if (pb) {
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (bf16)p[e];
      *reinterpret_cast<bf16x4*>(pb) = o;
    }
  }
};

// the last n < 4 elements of a range, one at a time (pb: nullable)
__device__ __forceinline__ void vy_adamw_tail(float* p, const float* g, float* m, float* v, bf16* pb, int n,
                                              const VyAdamwScalars& s) {
  for (int e = 0; e < 4 && e < n; ++e) {
    float pv = p[e], mv = m[e], vv = v[e];
    vy_adamw_element<false>(pv, g[e], mv, vv, s);
    p[e] = pv; m[e] = mv; v[e] = vv;
    if (pb) pb[e] = (bf16)pv;
  }
}

// device helpers ------------------------------------------------------------------------
__device__ __forceinline__ float vy_gelu_erf(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}
__device__ __forceinline__ float vy_gelu_erf_grad(float x) {
  // d/dx [x Phi(x)] = Phi(x) + x phi(x)
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}
__device__ __forceinline__ float vy_gelu_tanh(float x) {
  const float c = 0.79788456080286535588f;
  return 0.5f * x * (1.0f + tanhf(c * (x + 0.044715f * x * x * x)));
}
__device__ __forceinline__ float vy_gelu_tanh_grad(float x) {
  const float c = 0.79788456080286535588f;
  const float u = c * (x + 0.044715f * x * x * x);
  const float t = tanhf(u);
  return 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * c * (1.0f + 3.0f * 0.044715f * x * x);
}
// bf16-path GELU: erf by Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7, far below a bf16 ulp) --
// one rcp, one exp2, five fma instead of ocml's erff; the exponential exp(-x^2/2) is shared
// with the Gaussian factor of the derivative.
__device__ __forceinline__ void vy_phi_fast(float x, float& cdf, float& gauss) {
  const float ax = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
  gauss = __expf(-ax * ax);  // exp(-x^2/2)
  float poly = 1.061405429f;
  poly = poly * t - 1.453152027f;
  poly = poly * t + 1.421413741f;
  poly = poly * t - 0.284496736f;
  poly = poly * t + 0.254829592f;
  const float erf_abs = 1.0f - poly * t * gauss;
  cdf = 0.5f * (1.0f + copysignf(erf_abs, x));
}
__device__ __forceinline__ float vy_gelu_erf_fast(float x) {
  float cdf, g;
  vy_phi_fast(x, cdf, g);
  return x * cdf;
}
__device__ __forceinline__ float vy_gelu_erf_grad_fast(float x) {
  float cdf, g;
  vy_phi_fast(x, cdf, g);
  return cdf + x * 0.39894228040143267794f * g;
}

// ---- the reference's other hidden_act choices (VyomAI/layers/ffn.py:7-15) -----------------------
// sigmoid as 1 / (1 + e^-x) and tanh as 1 - 2 / (1 + e^2x): e^t = inf gives 0 / 1 / -1, never inf - inf or inf / inf.
// Derivatives at the kinks are torch's: relu6' = 1 iff 0 < x < 6, leaky_relu' = 1 iff x > 0 (slope 0.01 otherwise).
constexpr float VY_LEAKY_SLOPE = 0.01f;
__device__ __forceinline__ float vy_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float vy_sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float vy_tanh_fast(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }
__device__ __forceinline__ float vy_relu6(float x) { return fminf(fmaxf(x, 0.0f), 6.0f); }
__device__ __forceinline__ float vy_relu6_grad(float x) { return (x > 0.0f && x < 6.0f) ? 1.0f : 0.0f; }
__device__ __forceinline__ float vy_leaky_relu(float x) { return x > 0.0f ? x : VY_LEAKY_SLOPE * x; }
__device__ __forceinline__ float vy_leaky_relu_grad(float x) { return x > 0.0f ? 1.0f : VY_LEAKY_SLOPE; }

// ACT value of the one kernel instantiation per family that takes the activation as a run-time code (every vy_act
// above VY_ACT_GELU_TANH): not a vy_act, never crosses the C ABI
constexpr int VY_ACT_RUNTIME = 0x40;

template <int ACT>
__device__ __forceinline__ float vy_act_fwd(float x) {
  static_assert(ACT != VY_ACT_RUNTIME, "resolve the run-time code with vy_act_dispatch first");
  if constexpr (ACT == VY_ACT_GELU_ERF) return vy_gelu_erf(x);
  else if constexpr (ACT == VY_ACT_GELU_TANH) return vy_gelu_tanh(x);
  else if constexpr (ACT == VY_ACT_SILU) return x * vy_sigmoid(x);
  else if constexpr (ACT == VY_ACT_TANH) return tanhf(x);
  else if constexpr (ACT == VY_ACT_SIGMOID) return vy_sigmoid(x);
  else if constexpr (ACT == VY_ACT_RELU6) return vy_relu6(x);
  else if constexpr (ACT == VY_ACT_LEAKY_RELU) return vy_leaky_relu(x);
  else return x;
}
template <int ACT>
__device__ __forceinline__ float vy_act_grad(float x) {
  static_assert(ACT != VY_ACT_RUNTIME, "resolve the run-time code with vy_act_dispatch first");
  if constexpr (ACT == VY_ACT_GELU_ERF) return vy_gelu_erf_grad(x);
  else if constexpr (ACT == VY_ACT_GELU_TANH) return vy_gelu_tanh_grad(x);
  else if constexpr (ACT == VY_ACT_SILU) { const float s = vy_sigmoid(x); return s * (1.0f + x * (1.0f - s)); }
  else if constexpr (ACT == VY_ACT_TANH) { const float t = tanhf(x); return 1.0f - t * t; }
  else if constexpr (ACT == VY_ACT_SIGMOID) { const float s = vy_sigmoid(x); return s * (1.0f - s); }
  else if constexpr (ACT == VY_ACT_RELU6) return vy_relu6_grad(x);
  else if constexpr (ACT == VY_ACT_LEAKY_RELU) return vy_leaky_relu_grad(x);
  else return 1.0f;
}

// f(integral_constant<int, A>) with A = ACT, or, for ACT == VY_ACT_RUNTIME, A = the activation `code` names: the body
// is compiled once per run-time code and the switch sits outside the element loops.  `code` is a kernel argument, so
// the branch is scalar (wave-uniform).  The host admits only known codes; anything else would take the last case.
template <int ACT, typename F>
__device__ __forceinline__ void vy_act_dispatch(int code, F&& f) {
  if constexpr (ACT != VY_ACT_RUNTIME) {
    f(std::integral_constant<int, ACT>{});
  } else {
    switch (code) {
      case VY_ACT_SILU: f(std::integral_constant<int, VY_ACT_SILU>{}); break;
      case VY_ACT_TANH: f(std::integral_constant<int, VY_ACT_TANH>{}); break;
      case VY_ACT_SIGMOID: f(std::integral_constant<int, VY_ACT_SIGMOID>{}); break;
      case VY_ACT_RELU6: f(std::integral_constant<int, VY_ACT_RELU6>{}); break;
      default: f(std::integral_constant<int, VY_ACT_LEAKY_RELU>{}); break;
    }
  }
}
// the codes the run-time instantiation serves (host side)
static inline bool vy_act_is_runtime(int act) { return act >= VY_ACT_SILU && act <= VY_ACT_LEAKY_RELU; }

__device__ __forceinline__ float vy_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float vy_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// reduced-cost variants for bf16 storage (results are rounded to 8 bits of mantissa anyway)
template <int ACT>
__device__ __forceinline__ float vy_act_fwd_fast(float x) {
  if constexpr (ACT == VY_ACT_GELU_ERF) return vy_gelu_erf_fast(x);
  else if constexpr (ACT == VY_ACT_SILU) return x * vy_sigmoid_fast(x);
  else if constexpr (ACT == VY_ACT_TANH) return vy_tanh_fast(x);
  else if constexpr (ACT == VY_ACT_SIGMOID) return vy_sigmoid_fast(x);
  else return vy_act_fwd<ACT>(x);
}
template <int ACT>
__device__ __forceinline__ float vy_act_grad_fast(float x) {
  if constexpr (ACT == VY_ACT_GELU_ERF) return vy_gelu_erf_grad_fast(x);
  else if constexpr (ACT == VY_ACT_SILU) { const float s = vy_sigmoid_fast(x); return s * (1.0f + x * (1.0f - s)); }
  else if constexpr (ACT == VY_ACT_TANH) { const float t = vy_tanh_fast(x); return 1.0f - t * t; }
  else if constexpr (ACT == VY_ACT_SIGMOID) { const float s = vy_sigmoid_fast(x); return s * (1.0f - s); }
  else return vy_act_grad<ACT>(x);
}

// Round an fp32 value to bf16 and back.  Goes through the bit pattern: clang evaluates __bf16
// expressions with excess precision, so a plain (float)(bf16)x round trip may be elided.
__device__ __forceinline__ float vy_round_bf16(float x) {
  const bf16 b = (bf16)x;
  const unsigned short u = __builtin_bit_cast(unsigned short, b);
  return __builtin_bit_cast(float, (unsigned)u << 16);
}

// ---- dropout: counter-based keep mask ----------------------------------------------------------
// nn.Dropout(hidden_dropout_prob) in AttentionSelfOutput / FeedForward (reference layers/attention.py:70,
// layers/ffn.py:38).  The mask is a pure function of (seed, offset, row, column): Philox4x32-7 on the
// counter {column / 8, row, offset} gives eight 16-bit lots for the eight columns of a 16-byte bf16
// chunk; an element is dropped when its lot is below thr = round(p * 65536).  The forward epilogue,
// vy_dropout (backward: the same mask on the incoming gradient) and the tests' mask export all call
// this one function, so nothing has to be stored.
struct VyDrop {
  uint32_t thr;       // 0 = no dropout
  float scale;        // 1 / (1 - p)
  uint32_t seed_lo, seed_hi, off_lo, off_hi;
};
__host__ inline VyDrop vy_make_drop(float p, uint64_t seed, uint64_t offset) {
  VyDrop d{};
  if (p > 0.f) {
    double t = (double)p * 65536.0 + 0.5;
    d.thr = t >= 65536.0 ? 65536u : (uint32_t)t;
    d.scale = p < 1.f ? 1.0f / (1.0f - p) : 0.f;
    d.seed_lo = (uint32_t)seed; d.seed_hi = (uint32_t)(seed >> 32);
    d.off_lo = (uint32_t)offset; d.off_hi = (uint32_t)(offset >> 32);
  }
  return d;
}
__device__ __forceinline__ void vy_philox7(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                           uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the eight lots of the chunk holding columns 8 * chunk .. 8 * chunk + 7 of row m
__device__ __forceinline__ void vy_drop_lots(const VyDrop& d, int64_t m, int chunk, uint32_t (&r)[4]) {
  vy_philox7((uint32_t)chunk, (uint32_t)m, d.off_lo, d.off_hi ^ (uint32_t)((uint64_t)m >> 32), d.seed_lo, d.seed_hi, r);
}
__device__ __forceinline__ bool vy_drop_keep(const VyDrop& d, const uint32_t (&r)[4], int e) {   // e = column & 7
  return ((r[e >> 1] >> (16 * (e & 1))) & 0xffffu) >= d.thr;
}

// ---- Gumbel noise: counter-based, for sampling replaced tokens (ELECTRA) -------------------------
// noise(t) = -log(-log(u + 1e-9) + 1e-9), u uniform on [0, 1) (reference pretraining/collators.py:65-73, epsilons
// included: they keep g inside [-3.04, 20.73] for every u).  A pure function of (seed, offset, row, column):
// Philox4x32-7 on the counter {column / 4, row, offset}, one 32-bit word per column, its top 24 bits the uniform.
// The row kernels (vy_xent_sample_*) and the export (vy_gumbel_noise) both call this one function.
struct VyNoise {
  uint32_t seed_lo, seed_hi, off_lo, off_hi;
};
__host__ __device__ inline VyNoise vy_make_noise(uint64_t seed, uint64_t offset) {
  return VyNoise{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
}
// the four words of columns 4 * quad .. 4 * quad + 3 of row m
__device__ __forceinline__ void vy_noise_words(const VyNoise& n, int64_t m, int quad, uint32_t (&r)[4]) {
  vy_philox7((uint32_t)quad, (uint32_t)m, n.off_lo, n.off_hi ^ (uint32_t)((uint64_t)m >> 32), n.seed_lo, n.seed_hi, r);
}
__device__ __forceinline__ float vy_gumbel(uint32_t word) {
  const float t = (float)(word >> 8) * 5.9604644775390625e-8f + 1e-9f;   // u = word's top 24 bits * 2^-24 (exact)
  // -log(t): near t = 1 the result is small against t, so from 1/2 up it is taken as log1p of t - 1 (exact there)
  const float inner = t < 0.5f ? -logf(t) : -log1pf(t - 1.0f);
  return -logf(inner + 1e-9f);
}

// load/store helpers templated on the storage type
template <typename T> struct VyT;
template <> struct VyT<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct VyT<bf16> {
  static __device__ __forceinline__ float ld(const bf16* p) { return (float)*p; }
  static __device__ __forceinline__ void st(bf16* p, float v) { *p = (bf16)v; }
};

// 16-byte accesses of the row / streaming kernels (vy_misc.hip, vy_prenorm.hip)
template <typename T> struct Chunk;  // one 16-byte chunk = VEC elements
template <> struct Chunk<bf16> {
  static constexpr int VEC = 8;
  typedef bf16x8 Raw;
  static __device__ __forceinline__ void unpack(const Raw& t, float* v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  }
  static __device__ __forceinline__ void load(const bf16* p, float* v) {
    bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  }
  static __device__ __forceinline__ void store(bf16* p, const float* v) {
    bf16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (bf16)v[e];
    *reinterpret_cast<bf16x8*>(p) = t;
  }
};
template <> struct Chunk<float> {
  static constexpr int VEC = 4;
  typedef f32x4 Raw;
  static __device__ __forceinline__ void unpack(const Raw& t, float* v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t[e];
  }
  static __device__ __forceinline__ void load(const float* p, float* v) {
    f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t[e];
  }
  static __device__ __forceinline__ void store(float* p, const float* v) {
    f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = t;
  }
};
