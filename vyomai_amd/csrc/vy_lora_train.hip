// Low-rank weight gradients of LoRA fine-tuning (vyomai_amd/lora_train.py): both adapter gradients of one GEMM group
// in one launch pair,
//   dB_p[n, j] (+)= alpha * sum_m dY[m, col0_p + n] * u[m, p r_pad + j]        (out_p, rank_p)
//   dA_p[j, k] (+)= alpha * sum_m t[m, p r_pad + j]  * x[m, k]                 (rank_p, K)
// for the parts p of a packed projection (the rule: include/vyom_hip.h).  Both products contract over the ROW index m
// of a wide operand (dY: N columns; x: K columns) and a thin one (u / t: R = parts * r_pad columns), so one kernel
// serves both: a workgroup owns 64 columns of dY (job B) or of x (job A) and one chunk of M, stages 32 rows of its wide
// columns and of all R thin columns row-major in LDS, and each of its four waves multiplies its 16 wide columns with
// the thin columns that belong to them (job B: the r_pad columns of the wave's part; job A: all R).
//   bf16: mfma_f32_16x16x32_bf16; both fragments are 8 values of m for one column, read from the row-major images with
//         ds_read_b64_tr_b16 (rows 4 g + q and 16 + 4 g + q for the 16-lane group g: the same permutation of m in both
//         operands).  LDS rows are 32 bytes longer than their data, so the row stride is an odd multiple of 32 bytes
//         and the 8 rows x 32 bytes a 32-lane half reads fall into 64 different banks.
//   fp32: mfma_f32_16x16x4f32, eight per stage, single-float reads of the same images.  The parity path.
// Determinism: the cut of M depends on (M, N, K) alone (vy_lora_wgrad_chunk_rows); every workgroup stores its fp32
// tile to the stream workspace, [chunk][N r_pad + R K], and lora_wgrad_finish adds the chunks in chunk order, scales by
// alpha and writes (or adds to) the columns j < rank_p of the outputs.  No atomics, the same bits every run.
#include "vy_common.h"

float* vy_stream_ws(hipStream_t st, int64_t need);   // vy_gemm.hip: the workspace registered for the stream, or null

namespace {

constexpr int WG = 256;      // four waves
constexpr int MS = 32;       // rows of m per stage
constexpr int WC = 64;       // wide columns per workgroup, 16 per wave
constexpr int MAXR = 192;    // 3 parts x r_pad 64
constexpr int MAXT = MAXR / 16;

struct WgradArgs {
  const void* wide[2];       // [0] job B: dY, [1] job A: x
  const void* thin[2];       // [0] u, [1] t
  int64_t ldw[2], ldt[2];
  float* dA[3];
  float* dB[3];
  int rank[3], col0[4];      // col0[p]: first column of part p; col0[parts ..] = N
  int M, N, K, R, r_pad, rows, chunks, tilesB;
  int64_t slab;              // floats per chunk of the workspace: N r_pad + R K
  float* ws;
  float alpha;
  int accumulate;
};

template <typename T> struct WFrag;
template <> struct WFrag<bf16> {
  bf16x8 v;
  // 8 values of m (rows 4 g .. 4 g + 3, 16 + 4 g .. + 3) of column col + (lane & 15)
  __device__ __forceinline__ void load(const char* img, int rowb, int col, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const char* a = img + (4 * g + q) * rowb + (col + 4 * p) * 2;
    v = vy_lds_tr16_pair(a, a + 16 * rowb);
  }
  __device__ __forceinline__ void wait() { vy_lgkm_wait<0>(v); }
  static __device__ __forceinline__ f32x4 mma(const WFrag& a, const WFrag& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0);
  }
};
template <> struct WFrag<float> {
  float v[MS / 4];
  __device__ __forceinline__ void load(const char* img, int rowb, int col, int lane) {
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int s = 0; s < MS / 4; ++s) v[s] = *reinterpret_cast<const float*>(img + (4 * s + g) * rowb + (col + c) * 4);
  }
  __device__ __forceinline__ void wait() {}
  static __device__ __forceinline__ f32x4 mma(const WFrag& a, const WFrag& b, f32x4 c) {
#pragma unroll
    for (int s = 0; s < MS / 4; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[s], b.v[s], c, 0, 0, 0);
    return c;
  }
};

// grid (tiles of dY + tiles of x, chunks of M); dynamic LDS: MS rows of the wide image, then MS rows of the thin one
template <typename T>
__global__ __launch_bounds__(WG) void lora_wgrad_kernel(const WgradArgs a) {
  constexpr int ES = (int)sizeof(T), VEC = 16 / ES;
  constexpr int WROW = WC * ES + 32;                 // bf16: 160 bytes = 5 x 32
  constexpr int CW = WC / VEC;                       // 16-byte pieces per wide row
  constexpr int NWL = MS * CW / WG;                  // wide pieces per thread and stage (1 / 2)
  constexpr int NTL = MS * (MAXR / VEC) / WG;        // thin pieces per thread and stage at most (3 / 6)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int trow = a.R * ES + 32;                    // R / 16 is even: an odd multiple of 32 bytes too
  char* wide_s = smem;
  char* thin_s = smem + MS * WROW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int job = (int)blockIdx.x < a.tilesB ? 0 : 1;
  const int c0 = ((int)blockIdx.x - (job ? a.tilesB : 0)) * WC;
  const int C = job ? a.K : a.N;
  const T* wide = reinterpret_cast<const T*>(a.wide[job]);
  const T* thin = reinterpret_cast<const T*>(a.thin[job]);
  const int64_t ldw = a.ldw[job], ldt = a.ldt[job];
  const int m_begin = (int)blockIdx.y * a.rows;
  const int m_end = min(a.M, m_begin + a.rows);
  const int nst = (m_end - m_begin + MS - 1) / MS;
  const int CT = a.R / VEC, thin_total = MS * CT;

  // the wave's 16 wide columns and the thin columns they meet
  const int cw = c0 + 16 * wave;
  bool active = cw < C;
  int j0 = 0, nt = a.R / 16, part = 0;
  if (job == 0) {
    part = (cw >= a.col0[1]) + (cw >= a.col0[2]);
    j0 = part * a.r_pad;
    nt = a.r_pad / 16;
    active = active && a.dB[part] != nullptr;
  }
  const int tpp = a.r_pad / 16;                      // thin 16-column tiles per part
  f32x4 acc[MAXT];
#pragma unroll
  for (int i = 0; i < MAXT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 wreg[NWL], treg[NTL];
  const u32x4 zero = {0u, 0u, 0u, 0u};
  const auto fetch = [&](int s) {
    const int m0 = m_begin + s * MS;
#pragma unroll
    for (int i = 0; i < NWL; ++i) {
      const int c = tid + i * WG, r = c / CW, col = c0 + (c % CW) * VEC;
      wreg[i] = (m0 + r < m_end && col < C) ? *reinterpret_cast<const u32x4*>(wide + (int64_t)(m0 + r) * ldw + col) : zero;
    }
#pragma unroll
    for (int i = 0; i < NTL; ++i) {
      const int c = tid + i * WG, r = c / CT, col = (c % CT) * VEC;
      treg[i] = (c < thin_total && m0 + r < m_end) ? *reinterpret_cast<const u32x4*>(thin + (int64_t)(m0 + r) * ldt + col)
                                                    : zero;
    }
  };
  const auto put = [&]() {
#pragma unroll
    for (int i = 0; i < NWL; ++i) {
      const int c = tid + i * WG;
      *reinterpret_cast<u32x4*>(wide_s + (c / CW) * WROW + (c % CW) * 16) = wreg[i];
    }
#pragma unroll
    for (int i = 0; i < NTL; ++i) {
      const int c = tid + i * WG;
      if (c < thin_total) *reinterpret_cast<u32x4*>(thin_s + (c / CT) * trow + (c % CT) * 16) = treg[i];
    }
  };

  fetch(0);
  for (int s = 0; s < nst; ++s) {
    put();
    __syncthreads();
    if (s + 1 < nst) fetch(s + 1);                   // the next stage's global loads fly under this stage's MFMAs
    if (active) {                                    // (wave-uniform: every lane of the wave takes the LDS reads)
      WFrag<T> fw;
      fw.load(wide_s, WROW, 16 * wave, lane);
      fw.wait();
#pragma unroll
      for (int jt = 0; jt < MAXT; ++jt) {
        if (jt >= nt) continue;
        if (job == 1 && a.dA[jt / tpp] == nullptr) continue;     // a part without an adapter
        WFrag<T> ft;
        ft.load(thin_s, trow, j0 + 16 * jt, lane);
        ft.wait();
        // D[i][j]: i = the first operand's column 4 (lane >> 4) + reg, j = the second operand's column lane & 15
        acc[jt] = job == 0 ? WFrag<T>::mma(ft, fw, acc[jt]) : WFrag<T>::mma(fw, ft, acc[jt]);
      }
    }
    __syncthreads();
  }
  if (!active) return;
  float* slab = a.ws + (int64_t)blockIdx.y * a.slab;
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int jt = 0; jt < MAXT; ++jt) {
    if (jt >= nt) continue;
    if (job == 0) {                                  // [n][r_pad]: four consecutive j of one n
      *reinterpret_cast<f32x4*>(slab + (int64_t)(cw + c) * a.r_pad + 16 * jt + 4 * g) = acc[jt];
    } else {                                         // [R][K]: four consecutive k of one j
      if (a.dA[jt / tpp] == nullptr) continue;
      *reinterpret_cast<f32x4*>(slab + (int64_t)a.N * a.r_pad + (int64_t)(16 * jt + c) * a.K + cw + 4 * g) = acc[jt];
    }
  }
}

// one thread per element of a slab: the chunks added in chunk order, alpha, the padded columns dropped
__global__ __launch_bounds__(WG) void lora_wgrad_finish(const WgradArgs a) {
  const int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (e >= a.slab) return;
  const int64_t nb = (int64_t)a.N * a.r_pad;
  float* dst;
  if (e < nb) {
    const int n = (int)(e / a.r_pad), j = (int)(e % a.r_pad);
    const int p = (n >= a.col0[1]) + (n >= a.col0[2]);
    if (a.dB[p] == nullptr || j >= a.rank[p]) return;
    dst = a.dB[p] + (int64_t)(n - a.col0[p]) * a.rank[p] + j;
  } else {
    const int64_t f = e - nb;
    const int jf = (int)(f / a.K), k = (int)(f % a.K);
    const int p = jf / a.r_pad, j = jf % a.r_pad;
    if (a.dA[p] == nullptr || j >= a.rank[p]) return;
    dst = a.dA[p] + (int64_t)j * a.K + k;
  }
  float s = a.ws[e];
  for (int ch = 1; ch < a.chunks; ++ch) s += a.ws[(int64_t)ch * a.slab + e];
  s *= a.alpha;
  *dst = a.accumulate ? *dst + s : s;
}

bool rows_aligned(const void* p, int64_t ld, int es) { return ((uintptr_t)p % 16) == 0 && (ld * es) % 16 == 0; }

}  // namespace

// rows of m per chunk: about four workgroups per CU over the whole grid, at least 128 rows, whole stages of 32
extern "C" int64_t vy_lora_wgrad_chunk_rows(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const int64_t tiles = vy_cdiv(N, WC) + vy_cdiv(K, WC);
  const int64_t want = vy_cdiv(1024, tiles);
  const int64_t rows = vy_cdiv(vy_cdiv(M, want), MS) * MS;
  return rows < 128 ? 128 : rows;
}

extern "C" int vy_lora_wgrad(const void* dy, int64_t lddy, const void* u, int64_t ldu, const void* x, int64_t ldx,
                             const void* t, int64_t ldt, float* dA0, float* dA1, float* dA2, float* dB0, float* dB1,
                             float* dB2, int64_t rank0, int64_t rank1, int64_t rank2, int64_t M, int64_t N, int64_t K,
                             int64_t r_pad, int64_t bound0, int64_t bound1, float alpha, int accumulate, int dtype,
                             void* stream) {
  if (!dy || !u || !x || !t) VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: null operand");
  if (dtype != VY_BF16 && dtype != VY_F32) VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: bad dtype %d", dtype);
  if (accumulate != 0 && accumulate != 1) VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: accumulate %d must be 0 or 1", accumulate);
  if (M <= 0 || M > INT32_MAX || K <= 0 || K % 32 || K > INT32_MAX || N <= 0 || N % 16 || N > INT32_MAX)
    VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: bad shape (M %lld, K %lld must be a multiple of 32, N %lld of 16)", (long long)M,
            (long long)K, (long long)N);
  if (r_pad != 32 && r_pad != 64) VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: r_pad %lld must be 32 or 64", (long long)r_pad);
  if (bound0 <= 0 || bound0 > N || bound1 < bound0 || bound1 > N || bound0 % 16 || bound1 % 16 ||
      (bound0 == bound1 && bound0 < N))
    VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: boundaries %lld, %lld must be multiples of 16 with 0 < b0 < b1 < N = %lld (a "
            "boundary that is not used is N): every part's width is a multiple of 16", (long long)bound0,
            (long long)bound1, (long long)N);
  const int parts = 1 + (bound0 < N) + (bound1 < N);
  const int64_t R = parts * r_pad;
  float* dA[3] = {dA0, dA1, dA2};
  float* dB[3] = {dB0, dB1, dB2};
  const int64_t rank[3] = {rank0, rank1, rank2};
  bool any = false;
  for (int p = 0; p < 3; ++p) {
    if ((dA[p] == nullptr) != (dB[p] == nullptr))
      VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: part %d has one of dA / dB only (a part without an adapter has neither)", p);
    if (dA[p] && p >= parts) VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: part %d given, the boundaries name %d part(s)", p, parts);
    if (dA[p] && (rank[p] < 1 || rank[p] > r_pad))
      VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: rank %lld of part %d is outside [1, r_pad = %lld]", (long long)rank[p], p,
              (long long)r_pad);
    any = any || dA[p];
  }
  if (!any) VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: null operand (no part has outputs)");
  if (lddy < N || ldx < K || ldu < R || ldt < R)
    VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: row strides (dy %lld, x %lld, u %lld, t %lld) are below the widths (%lld, %lld, "
            "%lld)", (long long)lddy, (long long)ldx, (long long)ldu, (long long)ldt, (long long)N, (long long)K,
            (long long)R);
  const int es = dtype == VY_BF16 ? 2 : 4;
  if (!rows_aligned(dy, lddy, es) || !rows_aligned(u, ldu, es) || !rows_aligned(x, ldx, es) || !rows_aligned(t, ldt, es))
    VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: rows of dy, u, x and t must be 16-byte aligned");
  for (int p = 0; p < 3; ++p)
    if (((uintptr_t)dA[p] | (uintptr_t)dB[p]) % 4) VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: outputs must be 4-byte aligned");

  WgradArgs a{};
  a.wide[0] = dy, a.wide[1] = x, a.thin[0] = u, a.thin[1] = t;
  a.ldw[0] = lddy, a.ldw[1] = ldx, a.ldt[0] = ldu, a.ldt[1] = ldt;
  for (int p = 0; p < 3; ++p) a.dA[p] = dA[p], a.dB[p] = dB[p], a.rank[p] = (int)rank[p];
  a.col0[0] = 0, a.col0[1] = (int)bound0, a.col0[2] = (int)bound1, a.col0[3] = (int)N;
  a.M = (int)M, a.N = (int)N, a.K = (int)K, a.R = (int)R, a.r_pad = (int)r_pad;
  a.rows = (int)vy_lora_wgrad_chunk_rows(M, N, K);
  a.chunks = (int)vy_cdiv(M, a.rows);
  a.tilesB = (int)vy_cdiv(N, WC);
  a.slab = N * r_pad + R * K;
  a.alpha = alpha, a.accumulate = accumulate;
  hipStream_t st = (hipStream_t)stream;
  const int64_t need = a.slab * a.chunks * (int64_t)sizeof(float);
  a.ws = vy_stream_ws(st, need);
  if (!a.ws)
    VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: the stream has no workspace of %lld bytes (vy_workspace_set): %d chunks of M "
            "leave their partial sums there", (long long)need, a.chunks);
  const int64_t fin = vy_cdiv(a.slab, WG);
  if (fin > INT32_MAX) VY_FAIL(VY_ERR_ARG, "vy_lora_wgrad: N r_pad + R K = %lld is too large", (long long)a.slab);
  const dim3 grid((unsigned)(a.tilesB + vy_cdiv(K, WC)), (unsigned)a.chunks);
  const size_t lds = (size_t)MS * (WC * es + 32) + (size_t)MS * (R * es + 32);
  if (dtype == VY_BF16)
    hipLaunchKernelGGL(lora_wgrad_kernel<bf16>, grid, dim3(WG), lds, st, a);
  else
    hipLaunchKernelGGL(lora_wgrad_kernel<float>, grid, dim3(WG), lds, st, a);
  VY_CHECK_LAUNCH("vy_lora_wgrad");
  hipLaunchKernelGGL(lora_wgrad_finish, dim3((unsigned)fin), dim3(WG), 0, st, a);
  VY_CHECK_LAUNCH("vy_lora_wgrad (finish)");
  return VY_OK;
}
