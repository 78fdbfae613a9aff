// DoRA fine-tuning: the weight-sized arithmetic of the reference's DoraLinear (VyomAI/layers/adapters.py:50-75),
// vy_dora_compose and vy_dora_bwd (the rule: include/vyom_hip.h).  Everything here is out x in x r work, independent of
// the batch: W' is composed once per optimizer step and the plain block kernels run on it.
//
// One tile step serves all three kernels (dora_d): a workgroup of 256 threads holds 32 rows of dora_a and 32 columns
// of dora_b in LDS, thread (tx, ty) forms D = W + a b for column tx of rows 4 ty .. 4 ty + 3 -- one LDS read of b per
// four fmas, the a reads are broadcasts.  The compose accumulates D and its squares in fp64 (why: dora_d), the backward
// in fp32.  The three kernels differ in what they walk and own:
//   compose     a stripe of 32 columns, all rows, twice: the sum of squares, then the scaled store;
//   bwd (cols)  the same stripe, twice: p = sum_n G D (then dm), then dD and db = a^T dD in registers per thread, the
//               eight row groups of the workgroup added through LDS in group order;
//   bwd (rows)  a block of 32 rows, all columns: dD goes through LDS and thread (row, j) owns da[row, j].
// Every output has one owner and a fixed summation order: no atomics.
#include "vy_common.h"

float* vy_stream_ws(hipStream_t st, int64_t need);   // vy_gemm.hip: the workspace registered for the stream, or null

namespace {

constexpr int WG = 256;
constexpr int CS = 32;    // columns of a tile (tx)
constexpr int RT = 32;    // rows of a tile
constexpr int RPT = 4;    // rows per thread: RT / (WG / CS)
static_assert(RT == RPT * (WG / CS), "a tile is 8 row groups of RPT rows");

struct DoraItem {
  const void* W; const float* A; const float* B; const float* Mv; float* C;
  void* Wp; const float* G; float* dM; float* dA; float* dB; float* P;
  int64_t ldw, ldwp, ldg;
  int out, in, r, w_bf16;
  int blk_c, blk_r;     // first workgroup of this problem in a column-stripe / a row-block launch
};
struct DoraTable { DoraItem g[8]; int n; };

// the problem of workgroup blk, copied through constant indices (a run-time index into the kernel arguments would put
// the table into scratch memory)
template <bool ROWS>
__device__ __forceinline__ DoraItem dora_find(const DoraTable& t, int blk) {
  DoraItem it = t.g[0];
#pragma unroll
  for (int k = 1; k < 8; ++k)
    if (k < t.n && blk >= (ROWS ? t.g[k].blk_r : t.g[k].blk_c)) it = t.g[k];
  return it;
}

__device__ __forceinline__ float dora_ldw(const DoraItem& it, int n, int k) {
  const int64_t at = (int64_t)n * it.ldw + k;
  return it.w_bf16 ? (float)static_cast<const bf16*>(it.W)[at] : static_cast<const float*>(it.W)[at];
}

// rows n0 .. n0 + RT - 1 of dora_a; ranks r .. RP - 1 and rows past `out` are zero
template <int RP>
__device__ __forceinline__ void dora_load_a(float (*as)[RP], const DoraItem& it, int n0) {
  for (int i = threadIdx.x; i < RT * RP; i += WG) {
    const int row = i / RP, j = i % RP, n = n0 + row;
    as[row][j] = (n < it.out && j < it.r) ? it.A[(int64_t)n * it.r + j] : 0.f;
  }
}

// columns k0 .. k0 + CS - 1 of dora_b; ranks r .. RP - 1 and columns past `in` are zero
template <int RP>
__device__ __forceinline__ void dora_load_b(float (*bs)[CS + 1], const DoraItem& it, int k0) {
  for (int i = threadIdx.x; i < RP * CS; i += WG) {
    const int j = i / CS, kk = i % CS, k = k0 + kk;
    bs[j][kk] = (j < it.r && k < it.in) ? it.B[(int64_t)j * it.in + k] : 0.f;
  }
}

// D[n0 + 4 ty + i, k] for i < RPT: W + the fma chain over j in order (0 outside the matrix), in ACC.
// ACC = float in the backward.  ACC = double in the compose: a bf16 W' is held to 2^-8 |W'| PER ELEMENT, a bar without an
// absolute floor, and where W and a b cancel the fp32 chain's error -- ~1e-8 absolute, whatever the element's size --
// is more than the 2^-16 relative that a value beside a bf16 rounding boundary has to spare (measured: missed by
// 8.5e-9 at (1032, 264, 64)).  Products of fp32 values are exact in fp64; the cost (conversions, the fp64 fma rate) has
// not been measured.
template <int RP, typename ACC>
__device__ __forceinline__ void dora_d(ACC (&d)[RPT], const float (*as)[RP], const float (*bs)[CS + 1],
                                       const DoraItem& it, int n0, int k, bool colok) {
  const int tx = threadIdx.x & (CS - 1), r0 = (threadIdx.x / CS) * RPT;
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int n = n0 + r0 + i;
    d[i] = (colok && n < it.out) ? (ACC)dora_ldw(it, n, k) : (ACC)0;
  }
#pragma unroll 8
  for (int j = 0; j < RP; ++j) {
    const ACC bj = (ACC)bs[j][tx];
#pragma unroll
    for (int i = 0; i < RPT; ++i) d[i] = __builtin_fma((ACC)as[r0 + i][j], bj, d[i]);
  }
}

__device__ __forceinline__ void dora_ldg(float (&g)[RPT], const DoraItem& it, int n0, int k, bool colok) {
  const int r0 = (threadIdx.x / CS) * RPT;
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int n = n0 + r0 + i;
    g[i] = (colok && n < it.out) ? it.G[(int64_t)n * it.ldg + k] : 0.f;
  }
}

// the eight row groups' partial sums of one column, added in group order -> every thread of the column
template <typename ACC>
__device__ __forceinline__ ACC dora_col_sum(ACC (*red)[CS], ACC v) {
  const int tx = threadIdx.x & (CS - 1), ty = threadIdx.x / CS;
  __syncthreads();
  red[ty][tx] = v;
  __syncthreads();
  ACC s = red[0][tx];
#pragma unroll
  for (int g = 1; g < WG / CS; ++g) s += red[g][tx];
  return s;
}

template <int RP, typename TO>
__global__ __launch_bounds__(WG) void dora_compose_kernel(DoraTable t) {
  __shared__ float as[RT][RP];
  __shared__ float bs[RP][CS + 1];
  __shared__ double red[WG / CS][CS];
  const DoraItem it = dora_find<false>(t, blockIdx.x);
  const int k0 = ((int)blockIdx.x - it.blk_c) * CS;
  const int tx = threadIdx.x & (CS - 1), r0 = (threadIdx.x / CS) * RPT;
  const int k = k0 + tx;
  const bool colok = k < it.in;
  dora_load_b<RP>(bs, it, k0);
  double ss = 0.0;
  for (int n0 = 0; n0 < it.out; n0 += RT) {
    __syncthreads();
    dora_load_a<RP>(as, it, n0);
    __syncthreads();
    double d[RPT];
    dora_d<RP, double>(d, as, bs, it, n0, k, colok);
#pragma unroll
    for (int i = 0; i < RPT; ++i) ss = __builtin_fma(d[i], d[i], ss);
  }
  const float c = (float)sqrt(dora_col_sum(red, ss));
  if (colok && threadIdx.x < CS) it.C[k] = c;
  const float scale = colok ? it.Mv[k] / c : 0.f;
  TO* wp = static_cast<TO*>(it.Wp);
  for (int n0 = 0; n0 < it.out; n0 += RT) {
    __syncthreads();
    dora_load_a<RP>(as, it, n0);
    __syncthreads();
    double d[RPT];
    dora_d<RP, double>(d, as, bs, it, n0, k, colok);
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int n = n0 + r0 + i;
      if (colok && n < it.out) VyT<TO>::st(wp + (int64_t)n * it.ldwp + k, scale * (float)d[i]);
    }
  }
}

template <int RP>
__global__ __launch_bounds__(WG) void dora_bwd_cols_kernel(DoraTable t, int accumulate) {
  __shared__ float as[RT][RP];
  __shared__ float bs[RP][CS + 1];
  __shared__ float red[WG / CS][CS];
  __shared__ float acc[RP][CS];
  const DoraItem it = dora_find<false>(t, blockIdx.x);
  const int k0 = ((int)blockIdx.x - it.blk_c) * CS;
  const int tx = threadIdx.x & (CS - 1), ty = threadIdx.x / CS, r0 = ty * RPT;
  const int k = k0 + tx;
  const bool colok = k < it.in;
  dora_load_b<RP>(bs, it, k0);
  float pa = 0.f;
  for (int n0 = 0; n0 < it.out; n0 += RT) {
    __syncthreads();
    dora_load_a<RP>(as, it, n0);
    __syncthreads();
    float d[RPT], g[RPT];
    dora_d<RP, float>(d, as, bs, it, n0, k, colok);
    dora_ldg(g, it, n0, k, colok);
#pragma unroll
    for (int i = 0; i < RPT; ++i) pa = __builtin_fmaf(g[i], d[i], pa);
  }
  const float p = dora_col_sum(red, pa);
  const float c = colok ? it.C[k] : 1.f;
  if (colok && threadIdx.x < CS) {
    it.P[k] = p;
    const float dm = p / c;
    it.dM[k] = accumulate ? it.dM[k] + dm : dm;
  }
  const float s = colok ? it.Mv[k] / c : 0.f;
  const float q = p / (c * c);
  float db[RP];
#pragma unroll
  for (int j = 0; j < RP; ++j) db[j] = 0.f;
  for (int n0 = 0; n0 < it.out; n0 += RT) {
    __syncthreads();
    dora_load_a<RP>(as, it, n0);
    __syncthreads();
    float d[RPT], g[RPT];
    dora_d<RP, float>(d, as, bs, it, n0, k, colok);
    dora_ldg(g, it, n0, k, colok);
#pragma unroll
    for (int i = 0; i < RPT; ++i) d[i] = s * (g[i] - q * d[i]);     // dD
#pragma unroll
    for (int j = 0; j < RP; ++j) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) db[j] = __builtin_fmaf(as[r0 + i][j], d[i], db[j]);
    }
  }
  for (int g = 0; g < WG / CS; ++g) {
    if (ty == g) {
#pragma unroll
      for (int j = 0; j < RP; ++j) acc[j][tx] = g ? acc[j][tx] + db[j] : db[j];
    }
    __syncthreads();
  }
  if (colok)
    for (int j = ty; j < it.r; j += WG / CS) {
      float* o = it.dB + (int64_t)j * it.in + k;
      *o = accumulate ? *o + acc[j][tx] : acc[j][tx];
    }
}

template <int RP>
__global__ __launch_bounds__(WG) void dora_bwd_rows_kernel(DoraTable t, int accumulate) {
  __shared__ float as[RT][RP];
  __shared__ float bs[RP][CS + 1];
  __shared__ float dd[RT][CS + 1];
  constexpr int JG = 8, NU = RP / JG;     // thread (row, jl) owns da[row, jl + JG u], u < NU
  static_assert(RT * JG == WG, "one thread per (row, rank group)");
  const DoraItem it = dora_find<true>(t, blockIdx.x);
  const int n0 = ((int)blockIdx.x - it.blk_r) * RT;
  const int tx = threadIdx.x & (CS - 1), r0 = (threadIdx.x / CS) * RPT;
  const int row = threadIdx.x / JG, jl = threadIdx.x % JG;
  dora_load_a<RP>(as, it, n0);
  float acc[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) acc[u] = 0.f;
  for (int k0 = 0; k0 < it.in; k0 += CS) {
    __syncthreads();
    dora_load_b<RP>(bs, it, k0);
    __syncthreads();
    const int k = k0 + tx;
    const bool colok = k < it.in;
    float d[RPT], g[RPT];
    dora_d<RP, float>(d, as, bs, it, n0, k, colok);
    dora_ldg(g, it, n0, k, colok);
    const float c = colok ? it.C[k] : 1.f;
    const float s = colok ? it.Mv[k] / c : 0.f;
    const float q = colok ? it.P[k] / (c * c) : 0.f;
#pragma unroll
    for (int i = 0; i < RPT; ++i) dd[r0 + i][tx] = s * (g[i] - q * d[i]);
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < CS; ++kk) {
      const float v = dd[row][kk];
#pragma unroll
      for (int u = 0; u < NU; ++u) acc[u] = __builtin_fmaf(v, bs[jl + JG * u][kk], acc[u]);
    }
  }
  const int n = n0 + row;
  if (n < it.out) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int j = jl + JG * u;
      if (j < it.r) {
        float* o = it.dA + (int64_t)n * it.r + j;
        *o = accumulate ? *o + acc[u] : acc[u];
      }
    }
  }
}

// -> VY_OK with the table filled, or the error code (the message is set)
int dora_table(const char* fn, const vy_dora_desc* descs, int32_t n, bool bwd, DoraTable& t, int& rp, int64_t& cols) {
  if (!descs || n < 1 || n > 8) VY_FAIL(VY_ERR_ARG, "%s: 1..8 descriptors", fn);
  int64_t blk_c = 0, blk_r = 0, rmax = 0;
  cols = 0;
  for (int i = 0; i < n; ++i) {
    const vy_dora_desc& d = descs[i];
    if (!d.w || !d.a || !d.b || !d.m || !d.c) VY_FAIL(VY_ERR_ARG, "%s: problem %d has a null operand (w, a, b, m, c)", fn, i);
    if (bwd ? (!d.g || !d.dm || !d.da || !d.db) : !d.wp)
      VY_FAIL(VY_ERR_ARG, "%s: problem %d has a null operand (%s)", fn, i, bwd ? "g, dm, da, db" : "wp");
    if (d.w_dtype != VY_F32 && d.w_dtype != VY_BF16) VY_FAIL(VY_ERR_ARG, "%s: problem %d: bad w_dtype %d", fn, i, d.w_dtype);
    if (d.in < 8 || d.out < 8 || d.in % 8 || d.out % 8 || d.in > (1 << 24) || d.out > (1 << 24))
      VY_FAIL(VY_ERR_ARG, "%s: problem %d: in %lld and out %lld must be positive multiples of 8", fn, i, (long long)d.in,
              (long long)d.out);
    if (d.r < 1 || d.r > 64) VY_FAIL(VY_ERR_ARG, "%s: problem %d: r %lld is outside 1..64", fn, i, (long long)d.r);
    if (d.ldw < d.in || (bwd ? d.ldg < d.in : d.ldwp < d.in))
      VY_FAIL(VY_ERR_ARG, "%s: problem %d: a row stride is below in = %lld", fn, i, (long long)d.in);
    DoraItem& it = t.g[i];
    it.W = d.w, it.A = d.a, it.B = d.b, it.Mv = d.m, it.C = d.c;
    it.Wp = d.wp, it.G = d.g, it.dM = d.dm, it.dA = d.da, it.dB = d.db, it.P = nullptr;
    it.ldw = d.ldw, it.ldwp = d.ldwp, it.ldg = d.ldg;
    it.out = (int)d.out, it.in = (int)d.in, it.r = (int)d.r, it.w_bf16 = d.w_dtype == VY_BF16;
    it.blk_c = (int)blk_c, it.blk_r = (int)blk_r;
    blk_c += vy_cdiv(d.in, CS), blk_r += vy_cdiv(d.out, RT);
    cols += d.in;
    rmax = d.r > rmax ? d.r : rmax;
  }
  t.n = n;
  rp = rmax <= 8 ? 8 : rmax <= 16 ? 16 : rmax <= 32 ? 32 : 64;
  return VY_OK;
}

int dora_blocks(const DoraTable& t, bool rows) {
  const DoraItem& l = t.g[t.n - 1];
  return rows ? l.blk_r + (int)vy_cdiv(l.out, RT) : l.blk_c + (int)vy_cdiv(l.in, CS);
}

template <typename TO>
void compose_launch(int rp, int blocks, hipStream_t st, const DoraTable& t) {
  switch (rp) {
    case 8: hipLaunchKernelGGL((dora_compose_kernel<8, TO>), dim3(blocks), dim3(WG), 0, st, t); break;
    case 16: hipLaunchKernelGGL((dora_compose_kernel<16, TO>), dim3(blocks), dim3(WG), 0, st, t); break;
    case 32: hipLaunchKernelGGL((dora_compose_kernel<32, TO>), dim3(blocks), dim3(WG), 0, st, t); break;
    default: hipLaunchKernelGGL((dora_compose_kernel<64, TO>), dim3(blocks), dim3(WG), 0, st, t); break;
  }
}

}  // namespace

extern "C" int vy_dora_compose(const vy_dora_desc* descs, int32_t n, int out_dtype, void* stream) {
  if (out_dtype != VY_F32 && out_dtype != VY_BF16) VY_FAIL(VY_ERR_ARG, "vy_dora_compose: bad out_dtype %d", out_dtype);
  DoraTable t{};
  int rp;
  int64_t cols;
  const int rc = dora_table("vy_dora_compose", descs, n, false, t, rp, cols);
  if (rc != VY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VY_BF16) compose_launch<bf16>(rp, dora_blocks(t, false), st, t);
  else compose_launch<float>(rp, dora_blocks(t, false), st, t);
  VY_CHECK_LAUNCH("vy_dora_compose");
  return VY_OK;
}

extern "C" int vy_dora_bwd(const vy_dora_desc* descs, int32_t n, int accumulate, void* stream) {
  if (accumulate != 0 && accumulate != 1) VY_FAIL(VY_ERR_ARG, "vy_dora_bwd: accumulate %d must be 0 or 1", accumulate);
  DoraTable t{};
  int rp;
  int64_t cols;
  const int rc = dora_table("vy_dora_bwd", descs, n, true, t, rp, cols);
  if (rc != VY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* ws = vy_stream_ws(st, cols * (int64_t)sizeof(float));
  if (!ws)
    VY_FAIL(VY_ERR_ARG, "vy_dora_bwd: the stream has no workspace of %lld bytes (vy_workspace_set): p = sum_n G D stays "
            "there between the two launches", (long long)(cols * (int64_t)sizeof(float)));
  for (int i = 0; i < n; ++i) {
    t.g[i].P = ws;
    ws += t.g[i].in;
  }
  const int bc = dora_blocks(t, false), br = dora_blocks(t, true);
  switch (rp) {
    case 8: hipLaunchKernelGGL(dora_bwd_cols_kernel<8>, dim3(bc), dim3(WG), 0, st, t, accumulate); break;
    case 16: hipLaunchKernelGGL(dora_bwd_cols_kernel<16>, dim3(bc), dim3(WG), 0, st, t, accumulate); break;
    case 32: hipLaunchKernelGGL(dora_bwd_cols_kernel<32>, dim3(bc), dim3(WG), 0, st, t, accumulate); break;
    default: hipLaunchKernelGGL(dora_bwd_cols_kernel<64>, dim3(bc), dim3(WG), 0, st, t, accumulate); break;
  }
  VY_CHECK_LAUNCH("vy_dora_bwd (columns)");
  switch (rp) {
    case 8: hipLaunchKernelGGL(dora_bwd_rows_kernel<8>, dim3(br), dim3(WG), 0, st, t, accumulate); break;
    case 16: hipLaunchKernelGGL(dora_bwd_rows_kernel<16>, dim3(br), dim3(WG), 0, st, t, accumulate); break;
    case 32: hipLaunchKernelGGL(dora_bwd_rows_kernel<32>, dim3(br), dim3(WG), 0, st, t, accumulate); break;
    default: hipLaunchKernelGGL(dora_bwd_rows_kernel<64>, dim3(br), dim3(WG), 0, st, t, accumulate); break;
  }
  VY_CHECK_LAUNCH("vy_dora_bwd (rows)");
  return VY_OK;
}
