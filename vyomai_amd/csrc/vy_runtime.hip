// Native decode driver (host code): chains the kernel launchers for one single-token step so the
// Python side makes ONE call per generated token.  See include/vyom_hip.h (vy_decoder_step).
#include "vy_common.h"

int vy_qkv_rope_fwd_ex(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias,
                       const float* cos_tab, const float* sin_tab, int64_t pos0, const int* pos_dev, void* q,
                       int64_t q_sb, int64_t q_sh, int64_t q_sl, void* k, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                       void* v, int64_t v_sb, int64_t v_sh, int64_t v_sl, int64_t B, int64_t L, int64_t K, int h,
                       int hk, int dh, int dtype, void* stream);
int vy_attn_decode_ex(const void* q, int64_t q_sb, int64_t q_sh, const void* k, int64_t k_sb, int64_t k_sh,
                      int64_t k_sl, const void* v, int64_t v_sb, int64_t v_sh, int64_t v_sl, void* out,
                      int64_t o_sb, int64_t B, int h, int hk, int64_t S, const int* pos_dev, int dh, float scale,
                      int dtype, void* stream);

// general M <= 4 matrix-vector launchers (vy_gemm.hip); prescaled: the weights carry the preceding RMSNorm's (1 + w)
int vy_gemv_norm(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, int prescaled, float eps,
                 const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t M, int64_t N, int64_t K, void* stream);
int vy_gemv_qkv_norm(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, int prescaled, float eps,
                     void* q, int64_t q_sb, int64_t q_sh, void* k, int64_t k_sb, int64_t k_sh, int64_t k_sl, void* v,
                     int64_t v_sb, int64_t v_sh, int64_t v_sl, int64_t B, int64_t K, int h, int hk, int dh,
                     const float* cos_tab, const float* sin_tab, int64_t pos, void* stream);
int vy_gemv_gated(const void* x, int64_t ldx, const void* w, int64_t ldw, int prescaled, float eps, void* y, int64_t ldy,
                  int64_t M, int64_t I, int64_t K, int act, void* stream);
int vy_rope_qk(void* q, int64_t q_sb, int64_t q_sh, int64_t q_sl, int hq, void* k, int64_t k_sb, int64_t k_sh,
               int64_t k_sl, int hk, const float* cos_tab, const float* sin_tab, int64_t pos0, int64_t B, int64_t L, int dh,
               int dtype, hipStream_t st);
int64_t vy_splitk_ws_floats(int64_t N);
int vy_linear_res_ln_skinny(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias,
                            const void* residual, int64_t ldr, const void* gamma, const void* beta, float eps,
                            void* y, int64_t ldy, float* part, int64_t M, int64_t N, int64_t K, void* stream);

// lean decode kernels (vy_decode.hip)
bool vy_dec_supported(int B, int d, int h, int hk, int dh, int ffn, int dtype);
int vy_dec_qkv(const void* x, const void* w, const void* bias, const float* cos_tab, const float* sin_tab, int64_t pos0,
               const int* pos_dev, void* q, void* k, void* v, int64_t c_sb, int64_t c_sh, int64_t c_sl, int B, int d, int h,
               int hk, hipStream_t st);
int vy_dec_linear_ex(const void* x, int ldx, const void* w, const void* bias, const void* residual, int ldr, const void* ln_g,
                     const void* ln_b, float ln_eps, void* y, int ldy, int B, int N, int K, int act, hipStream_t st);
int vy_dec_linear_res_ln(const void* x, int ldx, const void* w, const void* bias, const void* residual, int ldr,
                         const void* gamma, const void* beta, float eps, void* y, int ldy, float* part, int B, int N, int K,
                         int act, hipStream_t st);

// test aids, not part of include/vyom_hip.h (the lean-against-general tests): 0 = the general launchers where the
// decode-only kernels / the B = 1 straight-line kernels would run
static int g_decode_lean = 1;
static int g_gemma_lean = 1;
extern "C" int vy_debug_set_decode_lean(int v) { g_decode_lean = v; return 0; }
extern "C" int vy_debug_set_gemma_lean(int v) { g_gemma_lean = v; return 0; }
// what the last vy_gemma_decoder_step ran: {chain (0 = MFMA chain, 1 = fused matrix-vector chain), layers whose four
// products all ran the lean B = 1 kernels, prescaled, rope_fused}.  Host-side statics only.
static int g_gemma_last[4];
extern "C" void vy_debug_gemma_last(int out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = g_gemma_last[i];
}

int vy_dec_gemv1(const void* x, const void* w, const void* bias, const void* residual, void* y, int N, int K, hipStream_t st);
int vy_dec_gemv1_gated(const void* x, const void* wgu, void* y, int I, int K, int prescaled, float eps, hipStream_t st);
int vy_dec_gemv1_qkv(const void* x, const void* w, const void* bias, void* q, void* k, void* v, int64_t c_sh, int h, int hk,
                     int dh, const float* cos_tab, const float* sin_tab, int64_t pos, int K, int prescaled, float eps,
                     hipStream_t st);
int vy_dec_gemv1_w8(const void* x, const void* codes, const float* scales, const void* bias, const void* residual, void* y, int N,
                    int K, hipStream_t st);
int vy_dec_gemv1_gated_w8(const void* x, const void* codes, const float* scales, void* y, int I, int K, int prescaled, float eps,
                          hipStream_t st);
int vy_dec_gemv1_qkv_w8(const void* x, const void* codes, const float* scales, const void* bias, void* q_out, void* k, void* v,
                        int64_t c_sh, int h, int hk, int dh, const float* cos_tab, const float* sin_tab, int64_t pos, int K,
                        int prescaled, float eps, hipStream_t st);

namespace {
inline int64_t esize(int dtype) { return dtype == VY_BF16 ? 2 : 4; }
inline int64_t up(int64_t x) { return (x + 255) / 256 * 256; }

// The workspace of a plan, carved once: byte offsets of its buffers (each rounded up to 256 bytes) and the size the
// *_ws_bytes entry point reports -- the step and the size query cannot disagree.
struct WsCarver {
  int64_t at = 0;
  int64_t take(int64_t bytes) { const int64_t o = at; at += up(bytes); return o; }
};
struct DecodeWs {
  // q, attention output, s (pre-LN), a (post-LN), two ping-pong hidden buffers, mid (ffn), split-K partials
  int64_t q, ao, s, a, hb[2], mid, part, bytes;
  DecodeWs(int64_t B, int64_t d, int64_t h, int64_t dh, int64_t ffn, int dtype) {
    const int64_t e = esize(dtype), lean_part = 24 * 32 * d;   // dec_finish_ln_kernel: up to 24 partial tiles of 32 rows
    WsCarver c;
    q = c.take(B * h * dh * e);
    ao = c.take(B * d * e);
    s = c.take(B * d * e);
    a = c.take(B * d * e);
    hb[0] = c.take(B * d * e);
    hb[1] = c.take(B * d * e);
    mid = c.take(B * ffn * e);
    part = c.take((vy_splitk_ws_floats(d) > lean_part ? vy_splitk_ws_floats(d) : lean_part) * 4);
    bytes = c.at + 4096;
  }
};
struct GemmaWs {
  // normed input, q, attention output, x after attention, two ping-pong layer outputs, [gate|up], act
  int64_t n, q, ao, x1, hb[2], gu, act, bytes;
  GemmaWs(int64_t B, int64_t d, int64_t h, int64_t dh, int64_t ffn, int dtype) {
    const int64_t e = esize(dtype);
    WsCarver c;
    n = c.take(B * d * e);
    q = c.take(B * h * dh * e);
    ao = c.take(B * h * dh * e);
    x1 = c.take(B * d * e);
    hb[0] = c.take(B * d * e);
    hb[1] = c.take(B * d * e);
    gu = c.take(2 * B * ffn * e);
    act = c.take(B * ffn * e);
    bytes = c.at + 4096;
  }
};
}  // namespace

extern "C" int64_t vy_decode_ws_bytes(int32_t B, int32_t d, int32_t h, int32_t hk, int32_t dh, int32_t ffn,
                                      int32_t dtype) {
  return DecodeWs(B, d, h, dh, ffn, dtype).bytes;
}

extern "C" int vy_decoder_step(const vy_decode_plan* p, const void* x, int64_t pos, const int32_t* pos_dev,
                               void* hidden_out, void* logits, int64_t ldv, void* stream) {
  const char* who = "vy_decoder_step";
  if (!p || !x || !p->layers || !p->ws) VY_FAIL(VY_ERR_ARG, "%s: null plan/input/workspace", who);
  const DecodeWs ws(p->B, p->d, p->h, p->dh, p->ffn, p->dtype);
  if (p->ws_bytes < ws.bytes) VY_FAIL(VY_ERR_ARG, "%s: workspace too small", who);
  const int64_t e = esize(p->dtype);
  const int B = p->B, d = p->d, h = p->h, hk = p->hk, dh = p->dh;
  char* w = (char*)p->ws;
  void *q = w + ws.q, *ao = w + ws.ao, *s = w + ws.s, *a = w + ws.a, *mid = w + ws.mid;
  void* hb[2] = {w + ws.hb[0], w + ws.hb[1]};
  float* part = (float*)(w + ws.part);
  // M <= 32 rows in bf16: the two N = d projections (24 workgroups as plain skinny GEMMs) run split-K
  // over ~all CUs, their bias + residual + LayerNorm fused into the kernel that adds the partials
  const bool splitk = p->dtype == VY_BF16 && B <= 32 && d % 32 == 0 && d <= 8192 && p->ffn % 16 == 0;
  const float scale = 1.0f / sqrtf((float)dh);
  // the decode-only kernels of vy_decode.hip (short dependent chains): bf16, 64-wide heads, K of every projection a
  // chunk size they exist for (vy_debug_set_decode_lean(0): the general launchers, for the equality test)
  const bool lean = g_decode_lean && vy_dec_supported(B, d, h, hk, dh, p->ffn, p->dtype);
  hipStream_t hst = (hipStream_t)stream;
  const void* cur = x;
  for (int l = 0; l < p->num_layers; ++l) {
    const vy_decode_layer& L = p->layers[l];
    if (!pos_dev && pos < 0) VY_FAIL(VY_ERR_ARG, "%s: negative position", who);
    // K/V of this token go straight into the cache at index pos (host offset, or the kernel adds
    // *pos_dev itself when the step is being captured into a graph)
    const int64_t hpos = pos_dev ? 0 : pos;
    void* kdst = (char*)L.kcache + hpos * L.c_sl * e;
    void* vdst = (char*)L.vcache + hpos * L.c_sl * e;
    if (lean) {
      int rc = vy_dec_qkv(cur, L.wqkv, L.bqkv, p->cos_tab, p->sin_tab, pos, pos_dev, q, kdst, vdst, L.c_sb, L.c_sh, L.c_sl, B,
                          d, h, hk, hst);
      if (rc) return rc;
      rc = vy_attn_decode_ex(q, (int64_t)h * dh, dh, L.kcache, L.c_sb, L.c_sh, L.c_sl, L.vcache, L.c_sb, L.c_sh,
                             L.c_sl, ao, d, B, h, hk, pos + 1, pos_dev, dh, scale, p->dtype, stream);
      if (rc) return rc;
      // LN1's output feeds FFN1 only (the FFN residual is the layer input): the out-projection keeps whole rows per
      // workgroup (K = d is one chunk: 16-column workgroups, bias + residual in the epilogue) and FFN1 normalises its
      // input rows on the way in -- no split-K partials, no finish + LayerNorm launch: 6 links per layer instead of 7
      rc = vy_dec_linear_ex(ao, d, L.wo, L.bo, cur, d, nullptr, nullptr, 0.f, s, d, B, d, d, VY_ACT_NONE, hst);
      if (rc) return rc;
      rc = vy_dec_linear_ex(s, d, L.w1, L.b1, nullptr, 0, L.ln1_w, L.ln1_b, p->eps_attn, mid, p->ffn, B, p->ffn, d, p->act, hst);
      if (rc) return rc;
      void* nxt_l = hb[l & 1];   // FFN residual = the LAYER INPUT (reference models/decoder.py:241-250)
      rc = vy_dec_linear_res_ln(mid, p->ffn, L.w2, L.b2, cur, d, L.ln2_w, L.ln2_b, p->eps_ffn, nxt_l, d, part, B, d, p->ffn,
                                VY_ACT_NONE, hst);
      if (rc) return rc;
      cur = nxt_l;
      continue;
    }
    int rc = vy_qkv_rope_fwd_ex(cur, d, L.wqkv, d, L.bqkv, p->cos_tab, p->sin_tab, pos, pos_dev, q, (int64_t)h * dh,
                                dh, dh, kdst, L.c_sb, L.c_sh, L.c_sl, vdst, L.c_sb, L.c_sh, L.c_sl, B, 1, d, h, hk,
                                dh, p->dtype, stream);
    if (rc) return rc;
    rc = vy_attn_decode_ex(q, (int64_t)h * dh, dh, L.kcache, L.c_sb, L.c_sh, L.c_sl, L.vcache, L.c_sb, L.c_sh,
                           L.c_sl, ao, d, B, h, hk, pos + 1, pos_dev, dh, scale, p->dtype, stream);
    if (rc) return rc;
    if (splitk) {
      rc = vy_linear_res_ln_skinny(ao, d, L.wo, d, L.bo, cur, d, L.ln1_w, L.ln1_b, p->eps_attn, a, d, part, B, d, d, stream);
      if (rc) return rc;
    } else {
      rc = vy_linear_fwd(ao, d, L.wo, d, L.bo, cur, d, s, d, nullptr, B, d, d, VY_ACT_NONE, p->dtype, stream);
      if (rc) return rc;
      rc = vy_layernorm_fwd(s, d, L.ln1_w, L.ln1_b, a, d, nullptr, nullptr, B, d, p->eps_attn, p->dtype, stream);
      if (rc) return rc;
    }
    rc = vy_linear_fwd(a, d, L.w1, d, L.b1, nullptr, 0, mid, p->ffn, nullptr, B, p->ffn, d, p->act, p->dtype, stream);
    if (rc) return rc;
    // FFN residual = the LAYER INPUT (reference models/decoder.py:241-250)
    void* nxt = hb[l & 1];
    if (splitk) {
      rc = vy_linear_res_ln_skinny(mid, p->ffn, L.w2, p->ffn, L.b2, cur, d, L.ln2_w, L.ln2_b, p->eps_ffn, nxt, d, part, B,
                                   d, p->ffn, stream);
      if (rc) return rc;
    } else {
      rc = vy_linear_fwd(mid, p->ffn, L.w2, p->ffn, L.b2, cur, d, s, d, nullptr, B, d, p->ffn, VY_ACT_NONE, p->dtype, stream);
      if (rc) return rc;
      rc = vy_layernorm_fwd(s, d, L.ln2_w, L.ln2_b, nxt, d, nullptr, nullptr, B, d, p->eps_ffn, p->dtype, stream);
      if (rc) return rc;
    }
    cur = nxt;
  }
  if (hidden_out && hidden_out != cur) {
    if (hipMemcpyAsync(hidden_out, cur, B * (int64_t)d * e, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
      VY_FAIL(VY_ERR_LAUNCH, "%s: copy of the hidden state failed", who);
  }
  if (logits) {
    int rc;
    if (lean) {   // LayerNorm(gelu(dense)) of the LM head: partial tile + finish
      rc = vy_dec_linear_res_ln(cur, d, p->head_wd, p->head_bd, nullptr, 0, p->head_ln_w, p->head_ln_b, p->eps_head, a, d,
                                part, B, d, d, VY_ACT_GELU_ERF, hst);
      if (rc) return rc;
    } else {
      rc = vy_linear_fwd(cur, d, p->head_wd, d, p->head_bd, nullptr, 0, s, d, nullptr, B, d, d, VY_ACT_GELU_ERF,
                         p->dtype, stream);
      if (rc) return rc;
      rc = vy_layernorm_fwd(s, d, p->head_ln_w, p->head_ln_b, a, d, nullptr, nullptr, B, d, p->eps_head, p->dtype, stream);
      if (rc) return rc;
    }
    rc = vy_linear_fwd(a, d, p->head_wv, d, p->head_bias, nullptr, 0, logits, ldv, nullptr, B, p->vocab, d,
                       VY_ACT_NONE, p->dtype, stream);
    if (rc) return rc;
  }
  return VY_OK;
}

extern "C" int64_t vy_gemma_ws_bytes(int32_t B, int32_t d, int32_t h, int32_t dh, int32_t ffn, int32_t dtype) {
  return GemmaWs(B, d, h, dh, ffn, dtype).bytes;
}

extern "C" int vy_gemma_decoder_step(const vy_gemma_plan* p, const void* x, int64_t pos, void* logits, int64_t ldv,
                                     void* stream) {
  const char* who = "vy_gemma_decoder_step";
  if (!p || !x || !p->layers || !p->ws || !logits) VY_FAIL(VY_ERR_ARG, "%s: null plan/input/workspace/output", who);
  if (pos < 0) VY_FAIL(VY_ERR_ARG, "%s: negative position", who);
  const GemmaWs ws(p->B, p->d, p->h, p->dh, p->ffn, p->dtype);
  if (p->ws_bytes < ws.bytes) VY_FAIL(VY_ERR_ARG, "%s: workspace too small", who);
  const int64_t e = esize(p->dtype);
  const int B = p->B, d = p->d, h = p->h, hk = p->hk, dh = p->dh, ffn = p->ffn;
  char* w = (char*)p->ws;
  void *n = w + ws.n, *q = w + ws.q, *ao = w + ws.ao, *x1 = w + ws.x1, *gu = w + ws.gu, *act = w + ws.act;
  void* hb[2] = {w + ws.hb[0], w + ws.hb[1]};
  const float scale = 1.0f / sqrtf((float)dh);
  const void* cur = x;
  int rc;
  // Three chains, chosen by plan and shape only.  Single-sequence bf16 decode (B <= 4) is a chain of matrix-vector
  // products with the GeGLU folded into the gate/up product and the rotary embedding into the QKV product: 7 launches
  // per layer, 5 when the plan's weights are pre-scaled (no RMSNorm launches).  (Folding the RMSNorm itself into the products
  // measured SLOWER, 2.05 vs 1.76 ms per token: every one of the N waves redoes the normalisation of its input.)
  const bool fused = p->dtype == VY_BF16 && B <= 4 && d % 8 == 0 && ffn % 8 == 0 && ((int64_t)h * dh) % 8 == 0;
  // a plan whose weights already carry the norms' (1 + w) can only run on the chain that skips the RMSNorm launches: on
  // any other chain the factor would be applied twice and the tokens would be wrong without a word
  if ((p->flags & VY_GEMMA_PRESCALED) && !fused)
    VY_FAIL(VY_ERR_ARG, "%s: the plan's weights are pre-scaled by the RMSNorm weights, which needs the fused matrix-vector "
            "chain (bf16, B <= 4, d / ffn / h*dh multiples of 8)", who);
  const bool prescaled = fused && (p->flags & VY_GEMMA_PRESCALED);
  const bool rope_fused = fused && p->cos_tab && dh % 4 == 0 && (dh & (dh - 1)) == 0;
  const bool lean1 = fused && g_gemma_lean && B == 1;
  g_gemma_last[0] = fused; g_gemma_last[1] = 0; g_gemma_last[2] = prescaled; g_gemma_last[3] = rope_fused;
  for (int l = 0; l < p->num_layers; ++l) {
    const vy_gemma_layer& L = p->layers[l];
    void* kdst = (char*)L.kcache + pos * L.c_sl * e;
    void* vdst = (char*)L.vcache + pos * L.c_sl * e;
    void* nxt = hb[l & 1];
    if (fused) {
      // prescaled: the weights carry the norms' (1 + w), the products scale themselves by the row's rsqrt(mean x^2):
      // no RMSNorm launch; rope_fused: rotary pairs swapped inside the QKV product's workgroups: no RoPE launch
      hipStream_t hs = (hipStream_t)stream;
      const void* qin = cur;
      if (!prescaled) {
        if ((rc = vy_rmsnorm_fwd(cur, d, L.ln_in, n, d, B, d, p->eps, 1.0f, p->dtype, stream))) return rc;
        qin = n;
      }
      // one sequence: the straight-line matrix-vector kernels of vy_decode.hip (they accept power-of-two head widths only,
      // so the rotary embedding is always fused there); a shape they do not cover runs the layer on the general kernels
      rc = lean1 ? vy_dec_gemv1_qkv(qin, L.wqkv, L.bqkv, q, kdst, vdst, L.c_sh, h, hk, dh, p->cos_tab, p->sin_tab, pos, d, prescaled,
                                    p->eps, hs)
                 : VY_ERR_UNSUPPORTED;
      if (rc != VY_OK && rc != VY_ERR_UNSUPPORTED) return rc;
      const bool lean_layer = rc == VY_OK;
      if (!lean_layer) {
        if ((rc = vy_gemv_qkv_norm(qin, d, L.wqkv, d, L.bqkv, prescaled, p->eps, q, (int64_t)h * dh, dh, kdst, L.c_sb, L.c_sh,
                                   L.c_sl, vdst, L.c_sb, L.c_sh, L.c_sl, B, d, h, hk, dh, rope_fused ? p->cos_tab : nullptr,
                                   p->sin_tab, pos, stream))) return rc;
        if (p->cos_tab && !rope_fused &&
            (rc = vy_rope_qk(q, (int64_t)h * dh, dh, dh, h, kdst, L.c_sb, L.c_sh, L.c_sl, hk, p->cos_tab, p->sin_tab,
                             pos, B, 1, dh, p->dtype, hs))) return rc;
      }
      if ((rc = vy_attn_decode_ex(q, (int64_t)h * dh, dh, L.kcache, L.c_sb, L.c_sh, L.c_sl, L.vcache, L.c_sb, L.c_sh, L.c_sl,
                                  ao, (int64_t)h * dh, B, h, hk, pos + 1, nullptr, dh, scale, p->dtype, stream))) return rc;
      int lean_links = lean_layer;
      rc = lean_layer ? vy_dec_gemv1(ao, L.wo, L.bo, cur, x1, d, h * dh, hs) : VY_ERR_UNSUPPORTED;
      lean_links += rc == VY_OK && lean_layer;
      if (rc == VY_ERR_UNSUPPORTED)
        rc = vy_gemv_norm(ao, (int64_t)h * dh, L.wo, (int64_t)h * dh, L.bo, 0, 0.f, cur, d, x1, d, B, d, (int64_t)h * dh, stream);
      if (rc) return rc;
      const void* gin = x1;
      if (!prescaled) {
        if ((rc = vy_rmsnorm_fwd(x1, d, L.ln_post, n, d, B, d, p->eps, 1.0f, p->dtype, stream))) return rc;
        gin = n;
      }
      rc = lean_layer ? vy_dec_gemv1_gated(gin, L.wgu, act, ffn, d, prescaled, p->eps, hs) : VY_ERR_UNSUPPORTED;
      lean_links += rc == VY_OK && lean_layer;
      if (rc == VY_ERR_UNSUPPORTED)
        rc = vy_gemv_gated(gin, d, L.wgu, d, prescaled, p->eps, act, ffn, B, ffn, d, VY_ACT_GELU_TANH, stream);
      if (rc) return rc;
      rc = lean_layer ? vy_dec_gemv1(act, L.wdown, nullptr, x1, nxt, d, ffn, hs) : VY_ERR_UNSUPPORTED;
      lean_links += rc == VY_OK && lean_layer;
      if (rc == VY_ERR_UNSUPPORTED) rc = vy_gemv_norm(act, ffn, L.wdown, ffn, nullptr, 0, 0.f, x1, d, nxt, d, B, d, ffn, stream);
      if (rc) return rc;
      g_gemma_last[1] += lean_links == 4;
      cur = nxt;
      continue;
    }
    if ((rc = vy_rmsnorm_fwd(cur, d, L.ln_in, n, d, B, d, p->eps, 1.0f, p->dtype, stream))) return rc;
    if ((rc = vy_qkv_rope_fwd_ex(n, d, L.wqkv, d, L.bqkv, p->cos_tab, p->sin_tab, pos, nullptr, q, (int64_t)h * dh, dh, dh,
                                 kdst, L.c_sb, L.c_sh, L.c_sl, vdst, L.c_sb, L.c_sh, L.c_sl, B, 1, d, h, hk, dh, p->dtype,
                                 stream))) return rc;
    if ((rc = vy_attn_decode_ex(q, (int64_t)h * dh, dh, L.kcache, L.c_sb, L.c_sh, L.c_sl, L.vcache, L.c_sb, L.c_sh, L.c_sl,
                                ao, (int64_t)h * dh, B, h, hk, pos + 1, nullptr, dh, scale, p->dtype, stream))) return rc;
    if ((rc = vy_linear_fwd(ao, (int64_t)h * dh, L.wo, (int64_t)h * dh, L.bo, cur, d, x1, d, nullptr, B, d, (int64_t)h * dh,
                            VY_ACT_NONE, p->dtype, stream))) return rc;
    if ((rc = vy_rmsnorm_fwd(x1, d, L.ln_post, n, d, B, d, p->eps, 1.0f, p->dtype, stream))) return rc;
    if ((rc = vy_linear_fwd(n, d, L.wgu, d, nullptr, nullptr, 0, gu, 2 * (int64_t)ffn, nullptr, B, 2 * (int64_t)ffn, d,
                            VY_ACT_NONE, p->dtype, stream))) return rc;
    if ((rc = vy_gated_act_fwd(gu, 2 * (int64_t)ffn, act, ffn, B, ffn, VY_ACT_GELU_TANH, p->dtype, stream))) return rc;
    if ((rc = vy_linear_fwd(act, ffn, L.wdown, ffn, nullptr, x1, d, nxt, d, nullptr, B, d, ffn, VY_ACT_NONE, p->dtype,
                            stream))) return rc;
    cur = nxt;
  }
  if ((rc = vy_rmsnorm_fwd(cur, d, p->norm_w, n, d, B, d, p->eps, 1.0f, p->dtype, stream))) return rc;
  return vy_linear_fwd(n, d, p->head_w, d, nullptr, nullptr, 0, logits, ldv, nullptr, B, p->vocab, d, VY_ACT_NONE,
                       p->dtype, stream);
}

// what the last vy_gemma_decoder_step_w8 ran: {layers whose four links ran the fp8-weight kernels, the head ran one}
static int g_gemma_w8_last[2];
extern "C" void vy_debug_gemma_w8_last(int out[2]) {
  out[0] = g_gemma_w8_last[0];
  out[1] = g_gemma_w8_last[1];
}
// and its launches in order, for the test of the chain: 1 = RMSNorm, 2 = qkv (w8), 3 = attention, 4 = plain product (w8),
// 5 = gated product (w8); at most 64 are kept.  -> how many the step made.  Host-side statics only.
static int g_gemma_w8_trace[64], g_gemma_w8_trace_n;
extern "C" int vy_debug_gemma_w8_trace(int* out, int cap) {
  for (int i = 0; i < g_gemma_w8_trace_n && i < 64 && i < cap; ++i) out[i] = g_gemma_w8_trace[i];
  return g_gemma_w8_trace_n;
}
static void w8_note(int code) {
  if (g_gemma_w8_trace_n < 64) g_gemma_w8_trace[g_gemma_w8_trace_n] = code;
  ++g_gemma_w8_trace_n;
}

// The single-sequence step on fp8 weights: the plan's wqkv / wo / wgu / wdown are e4m3fn codes, `w8` holds their row
// scales and a quantised copy of the vocabulary matrix.  ONE chain, the lean bf16 one launch for launch (qkv, attention,
// o_proj, gated, down; RMSNorm launches in front of qkv and gated unless the plan is pre-scaled), then the final RMSNorm
// and the vocabulary product as one more matrix-vector launch.  Every shape is checked before the first launch: no
// kernel that takes bf16 weights may ever see the codes.
extern "C" int vy_gemma_decoder_step_w8(const vy_gemma_plan* p, const vy_gemma_w8* w8, const void* x, int64_t pos,
                                        void* logits, int64_t ldv, void* stream) {
  const char* who = "vy_gemma_decoder_step_w8";
  if (!p || !w8 || !x || !p->layers || !p->ws || !logits || !w8->layers || !w8->head_codes || !w8->head_scale)
    VY_FAIL(VY_ERR_ARG, "%s: null plan/scales/input/workspace/output", who);
  if (pos < 0) VY_FAIL(VY_ERR_ARG, "%s: negative position", who);
  const GemmaWs ws(p->B, p->d, p->h, p->dh, p->ffn, p->dtype);
  if (p->ws_bytes < ws.bytes) VY_FAIL(VY_ERR_ARG, "%s: workspace too small", who);
  const int d = p->d, h = p->h, hk = p->hk, dh = p->dh, ffn = p->ffn;
  auto k_ok = [](int64_t K) { return K == 2048 || K == 4096 || K == 8192 || K == 16384; };
  g_gemma_w8_last[0] = g_gemma_w8_last[1] = g_gemma_w8_trace_n = 0;
  if (p->dtype != VY_BF16 || p->B != 1)
    VY_FAIL(VY_ERR_UNSUPPORTED, "%s: fp8 weights serve bf16 activations at B = 1 only (dtype %d, B = %d)", who, p->dtype, p->B);
  if (!k_ok(d) || !k_ok((int64_t)h * dh) || !k_ok(ffn))
    VY_FAIL(VY_ERR_UNSUPPORTED, "%s: d = %d, h * dh = %d, ffn = %d: every K must be 2048, 4096, 8192 or 16384", who, d, h * dh, ffn);
  if (!p->cos_tab || !p->sin_tab || dh % 4 || (dh & (dh - 1)))
    VY_FAIL(VY_ERR_UNSUPPORTED, "%s: the rotary embedding is fused: tables and a power-of-two head width (dh = %d)", who, dh);
  if (p->vocab % 4 || ldv < p->vocab || ffn % 4)
    VY_FAIL(VY_ERR_UNSUPPORTED, "%s: vocab = %d (ldv %lld), ffn = %d: multiples of 4", who, p->vocab, (long long)ldv, ffn);
  char* w = (char*)p->ws;
  void *n = w + ws.n, *q = w + ws.q, *ao = w + ws.ao, *x1 = w + ws.x1, *act = w + ws.act;
  void* hb[2] = {w + ws.hb[0], w + ws.hb[1]};
  const bool prescaled = p->flags & VY_GEMMA_PRESCALED;
  const float scale = 1.0f / sqrtf((float)dh);
  hipStream_t hs = (hipStream_t)stream;
  // the launchers' own refusal (an operand off its 16-byte alignment) ends the step: there is no other kernel for codes
#define W8_LINK(code, call)                                                                              \
  do {                                                                                                   \
    rc = (call);                                                                                         \
    if (rc == VY_ERR_UNSUPPORTED) VY_FAIL(rc, "%s: layer %d: x and the codes must be 16-byte aligned", who, l); \
    if (rc) return rc;                                                                                   \
    w8_note(code);                                                                                       \
  } while (0)
  const void* cur = x;
  int rc, l;
  for (l = 0; l < p->num_layers; ++l) {
    const vy_gemma_layer& L = p->layers[l];
    const vy_gemma_w8_layer& S = w8->layers[l];
    if (!S.s_qkv || !S.s_o || !S.s_gu || !S.s_down) VY_FAIL(VY_ERR_ARG, "%s: layer %d: null scales", who, l);
    void* kdst = (char*)L.kcache + pos * L.c_sl * 2;
    void* vdst = (char*)L.vcache + pos * L.c_sl * 2;
    void* nxt = hb[l & 1];
    const void* qin = cur;
    if (!prescaled) {
      if ((rc = vy_rmsnorm_fwd(cur, d, L.ln_in, n, d, 1, d, p->eps, 1.0f, p->dtype, stream))) return rc;
      w8_note(1);
      qin = n;
    }
    W8_LINK(2, vy_dec_gemv1_qkv_w8(qin, L.wqkv, S.s_qkv, L.bqkv, q, kdst, vdst, L.c_sh, h, hk, dh, p->cos_tab, p->sin_tab, pos, d,
                                prescaled, p->eps, hs));
    if ((rc = vy_attn_decode_ex(q, (int64_t)h * dh, dh, L.kcache, L.c_sb, L.c_sh, L.c_sl, L.vcache, L.c_sb, L.c_sh, L.c_sl, ao,
                                (int64_t)h * dh, 1, h, hk, pos + 1, nullptr, dh, scale, p->dtype, stream))) return rc;
    w8_note(3);
    W8_LINK(4, vy_dec_gemv1_w8(ao, L.wo, S.s_o, L.bo, cur, x1, d, h * dh, hs));
    const void* gin = x1;
    if (!prescaled) {
      if ((rc = vy_rmsnorm_fwd(x1, d, L.ln_post, n, d, 1, d, p->eps, 1.0f, p->dtype, stream))) return rc;
      w8_note(1);
      gin = n;
    }
    W8_LINK(5, vy_dec_gemv1_gated_w8(gin, L.wgu, S.s_gu, act, ffn, d, prescaled, p->eps, hs));
    W8_LINK(4, vy_dec_gemv1_w8(act, L.wdown, S.s_down, nullptr, x1, nxt, d, ffn, hs));
    g_gemma_w8_last[0] += 1;
    cur = nxt;
  }
  if ((rc = vy_rmsnorm_fwd(cur, d, p->norm_w, n, d, 1, d, p->eps, 1.0f, p->dtype, stream))) return rc;
  w8_note(1);
  W8_LINK(4, vy_dec_gemv1_w8(n, w8->head_codes, w8->head_scale, nullptr, nullptr, logits, p->vocab, d, hs));
#undef W8_LINK
  g_gemma_w8_last[1] = 1;
  return VY_OK;
}
