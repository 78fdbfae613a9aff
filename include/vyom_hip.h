/*
 * vyom_hip.h -- C ABI of libvyom_hip.so, the MI355X (gfx950 / CDNA4) kernel library
 * behind vyomai_amd's mirror of the VyomAI layer API.
 *
 * The reference (Ajax0564/VyomAI) has no FFI: its hot path is the Python class API of
 * VyomAI/layers consumed by VyomAI/models.  Each entry point
 * below replaces the torch ops that one reference call site issues; the citation after
 * "replaces:" is path:line in the reference checkout.
 *
 * Conventions (every function):
 *   - plain device pointers + explicit sizes/strides (in ELEMENTS unless noted), no torch types;
 *   - `dtype`: VY_F32 or VY_BF16 -- the storage type of activations/weights; accumulation,
 *     softmax and norm statistics are always fp32;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised;
 *   - no device allocation inside; callers pass workspaces;
 *   - returns 0 on success, a negative vy_status otherwise; vy_last_error() describes it.
 */
#ifndef VYOM_HIP_H
#define VYOM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { VY_F32 = 0, VY_BF16 = 1 } vy_dtype;

typedef enum {
  VY_OK = 0,
  VY_ERR_ARG = -1,       /* bad shape / alignment / null pointer */
  VY_ERR_UNSUPPORTED = -2,
  VY_ERR_LAUNCH = -3     /* hipGetLastError() after the launch */
} vy_status;

/* Activation fused into a GEMM epilogue: the reference's hidden_act table (VyomAI/layers/ffn.py:7-15) plus the tanh GELU.
 * silu is x * sigmoid(x) ("swish" is the same function); leaky_relu has nn.LeakyReLU()'s default slope 0.01.  Derivatives
 * at the kinks follow torch: relu6' = 1 iff 0 < x < 6, leaky_relu' = 1 iff x > 0 (else 0.01).  Codes 0-2 are compiled
 * into the kernels; the others share one instantiation per kernel family that switches on the code at run time.
 * Additions to this enum are backward-compatible (old codes keep their values and kernels), so they do not move
 * vy_abi_version().  An entry point given a code it does not know returns VY_ERR_ARG.
 * The gated MLP's standalone kernels (vy_gated_act_fwd, vy_gated_act_bwd) take every code, the new ones through the
 * run-time-switched instantiation; the decode driver's fused matrix-vector form (vy_gemv_gated) takes gelu_tanh only. */
typedef enum {
  VY_ACT_NONE = 0, VY_ACT_GELU_ERF = 1, VY_ACT_GELU_TANH = 2,
  VY_ACT_SILU = 3, VY_ACT_TANH = 4, VY_ACT_SIGMOID = 5, VY_ACT_RELU6 = 6, VY_ACT_LEAKY_RELU = 7
} vy_act;
/* OR-ed into `act` of vy_linear_fwd / vy_linear_dgrad (training): the tensor saved for backward is act'(x W^T + b)
 * instead of the pre-activation -- the forward epilogue has Phi and the Gaussian of the erf GELU at hand anyway, and
 * the dgrad epilogue (dX = (dY W) * act') becomes one multiply per element instead of an erf + exp evaluation.
 * vy_linear_fwd: pre_out receives act' (rounded to the storage type); vy_linear_dgrad: `pre` holds act'. */
#define VY_ACT_SAVE_DERIV 0x100

/* attention mask descriptor bits (vy_attn_fwd / vy_attn_bwd) */
enum {
  VY_MASK_NONE = 0,
  VY_MASK_CAUSAL = 1,   /* key j visible to query i iff j <= i + start_pos              */
  VY_MASK_KEYPAD = 2,   /* uint8 keep[B][S]; 0 = masked with finfo.min like the reference */
  VY_MASK_ADDITIVE = 4  /* generic fp32 additive mask (B,1,Lm,S), Lm in {1, L}            */
};

const char* vy_last_error(void);
int vy_abi_version(void);

/* Launch-sizing hint: the caller is about to run `n` independent launch chains side by side on `n` streams (the
 * training forward as two batch halves, vyomai_amd/ops.py `lanes`), so each launch should size its grid for 1/n of
 * the 256 CUs: a 128-tile launch of 256 x 192 tiles is then a full share, not a half-empty chip.  n = 1 (the default)
 * restores whole-chip sizing.  Process-global, read on the host when a launch is sized; results never depend on it. */
int vy_set_concurrent_chains(int n);

/* Scratch for the launches on `stream` (the library never allocates device memory): mid-size GEMMs (32 < M <= ~2304 rows,
 * fewer than 300 tiles of 128 x 128) split K over workgroups and keep fp32 partial tiles here between their two launches
 * -- 64 KiB per (tile, slice), the widest launch (16 slices of 16 tiles of 320 x 128) needs 42 MiB; the host layer registers 64 MiB.  One workspace per stream (launches on one stream are
 * ordered, so they can share it); ws = NULL or bytes = 0 removes the entry.  Without a workspace such GEMMs run unsplit:
 * results are the same up to the fp32 summation order over K. */
int vy_workspace_set(void* stream, void* ws, int64_t bytes);

/* ------------------------------------------------------------------------------------------
 * vy_linear_fwd:  Y[M,N] = act(X[M,K] . W[N,K]^T + bias[N]) + residual[M,N]
 * replaces: nn.Linear call sites -- AttentionSelfOutput.dense + residual add
 *   (VyomAI/layers/attention.py:69-71), FeedForward.intermediate + GELU and FeedForward.out +
 *   residual (VyomAI/layers/ffn.py:35-39), LMHead.dense/decoder (VyomAI/models/decoder.py:267-275).
 * `pre_out` (nullable, [M,ldy]) receives X.W^T+bias before the activation (saved for backward).
 * bias/residual/pre_out may be NULL.  K % 8 == 0 (bf16) / K % 4 == 0 (f32); rows 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int vy_linear_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias,
                  const void* residual, int64_t ldr, void* y, int64_t ldy, void* pre_out,
                  int64_t M, int64_t N, int64_t K, int act, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * vy_qkv_rope_fwd: fused Q/K/V projection + bias + rotary embedding + head split.
 * replaces: self.query/key/value (or self.qkv + chunk), rearrange 'b l (h d) -> b h l d',
 *   apply_rotary_pos_emb and the KV-cache slice write
 *   (VyomAI/layers/attention.py:114-126, 607-617; VyomAI/models/decoder.py:91-105;
 *    VyomAI/layers/positional_embeddings.py:155-182; VyomAI/layers/kv_cache.py:355-356).
 * w: packed [(h + 2*hk)*dh, K] rows = [Wq; Wk; Wv]; bias likewise or NULL.
 * cos/sin: fp32 tables [>= pos0+L][dh/2] (angles' cos/sin, half width) or NULL for no RoPE;
 *          row (pos0 + l) is used for token l.
 * q/k/v outputs are (B, heads, *, dh) with element strides {batch, head, token}; writing K/V
 * straight into a static cache is done by pointing k/v at cache[:, :, start_pos] with the
 * cache's strides.
 * ------------------------------------------------------------------------------------------ */
int vy_qkv_rope_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias,
                    const float* cos_tab, const float* sin_tab, int64_t pos0,
                    void* q, int64_t q_sb, int64_t q_sh, int64_t q_sl,
                    void* k, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                    void* v, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                    int64_t B, int64_t L, int64_t K, int h, int hk, int dh, int dtype,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * vy_attn_fwd: softmax(Q K^T / sqrt(dh) + mask) V, flash style, heads merged on output.
 * replaces: repeat_kv + F.scaled_dot_product_attention + rearrange 'b h l d -> b l (h d)'
 *   (VyomAI/layers/attention.py:8-19, 128-132, 205-213, 283-287, 368-377, 619-623;
 *    VyomAI/models/decoder.py:107-111, 190-199).
 * q (B,h,L,dh), k/v (B,hk,S,dh) with element strides {batch, head, token}; kv head of query
 * head i is i / (h/hk).  out is (B, L, h*dh) with strides {o_sb, o_sl}.
 * mask_kind: OR of VY_MASK_*; keypad uint8 [B][S] (stride kp_sb); additive fp32 with strides
 * {am_sb, am_sl} (am_sl = 0 broadcasts one row).  Masked scores take finfo(fp32).min exactly as
 * the reference's (1-mask)*finfo.min does, so a fully masked row averages V.
 * lse (nullable) fp32 [B,h,L]: natural-log sum-exp of the scaled, masked scores (for backward).
 * ------------------------------------------------------------------------------------------ */
int vy_attn_fwd(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sl,
                const void* k, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                const void* v, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                void* out, int64_t o_sb, int64_t o_sl, float* lse,
                int mask_kind, int64_t start_pos, const uint8_t* keypad, int64_t kp_sb,
                const float* addmask, int64_t am_sb, int64_t am_sl,
                int64_t B, int h, int hk, int64_t L, int64_t S, int dh, float scale, int dtype,
                void* stream);

/* ------------------------------------------------------------------------------------------
 * vy_attn_decode: one query token per sequence against a KV cache (L == 1, no mask).
 * replaces: the L==1 branch of DecoderAttention*.forward (mask=None, VyomAI/models/decoder.py:
 *   355-356, 105-111) reading StaticCacheOne/DynamicCacheOne prefixes (VyomAI/layers/kv_cache.py:
 *   229-236, 358-361).  q (B,h,1,dh) strides {q_sb,q_sh}; k/v cache strides {batch, head, token};
 *   S = start_pos + 1 keys are attended.  out (B,1,h*dh) row stride o_sb.
 * ------------------------------------------------------------------------------------------ */
int vy_attn_decode(const void* q, int64_t q_sb, int64_t q_sh,
                   const void* k, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                   const void* v, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                   void* out, int64_t o_sb, int64_t B, int h, int hk, int64_t S, int dh,
                   float scale, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Paged KV cache (Examples/simple_vllm.ipynb cell 2).  Per layer k_cache / v_cache are (max_blocks, block_size, hk, dh),
 * contiguous; slot = block * block_size + offset.  block_size: a power of two from 8 to 256; dh: a multiple of 8 up to
 * 256; bf16 and fp32.  Anything else is VY_ERR_ARG before a launch.  None of these entry points allocates.
 *
 * vy_paged_rope_write: after the packed QKV projection of a step's T tokens (qkv[T][ld], rows [q heads; k heads; v
 *   heads] of dh columns): token t's q and k heads are rotated IN PLACE with row positions[t] (int32, device) of the
 *   fp32 cos / sin tables [table_rows][dh/2] (rotate_half pairing d, d + dh/2, evaluated in fp32, one rounding), then its
 *   rotated k heads and its v heads are stored into slot slot_mapping[t] (int64, device) of the pages.  A negative slot
 *   (or one past the pages) writes nothing; a position outside the table is clamped into it.
 *   replaces: apply_rope on q and k with the gathered metadata['cos'] / ['sin'] rows and the
 *   `k_cache[b_idx, o_idx] = k`, `v_cache[b_idx, o_idx] = v` scatters of GroupedQueryAttention.forward.
 *
 * vy_paged_qknorm_rope_write: vy_paged_rope_write with the per-head RMSNorm of Qwen3's qk_norm in front of the rotation,
 *   in the same launch: every q head is replaced by n = x * rsqrt(mean_d(x^2) + eps) * q_scale, every k head by the same
 *   with k_scale (fp32 [dh], device, 16-byte aligned, shared by all heads of their kind; eps >= 0), and n is what gets
 *   rotated, stored in place and, for k, stored into the slot.  Everything between the load and the one store is fp32.
 *   v heads are neither normalised nor rotated.  An all-zero head stays zero (0 * rsqrt(eps)).  Shapes, alignment, slot
 *   and position rules are those of vy_paged_rope_write.
 *   replaces: `q, k = self.q_norm(q), self.k_norm(k)` (RMSNorm.forward on the (tokens, heads, head_dim) views) plus
 *   everything vy_paged_rope_write replaces.  The notebook's bf16 model rounds to bf16 after the norm and rotates in
 *   bf16 with bf16 tables; here there is one rounding, at the store.
 *
 * vy_attn_paged_decode: one query token per sequence against its pages.  q row of sequence b: q + row * q_ld with
 *   row = q_rows ? q_rows[b] : b (int32, device), heads of dh columns side by side; out (row stride o_ld >= h * dh) is
 *   written at the same rows.  block_table int32 [B][bt_stride] and seqlens int32 [B] live on the device; keys
 *   [0, seqlens[b]) are attended, entries of the table at or past ceil(seqlen / block_size) are never read, seqlen 0
 *   writes zeros.  max_seqlen (host, >= every seqlen) only sizes the launch.  n_split workgroups share a context
 *   (0 = chosen from B, hk and max_seqlen); with more than one, fp32 partials go through ws (at least
 *   vy_attn_paged_decode_ws_bytes of the same arguments; an automatic split without it runs unsplit).
 *   Memory safety only, not a service to the caller: a seqlen above bt_stride * block_size is cut to it, a negative one
 *   counts as 0, a block-table entry outside [0, max_blocks) is clamped into it -- all silently, the result is then
 *   not meaningful.
 *   replaces: flash_attn_with_kvcache(q.unsqueeze(1), k_cache, v_cache, cache_seqlens=..., block_table=...,
 *   causal=True) in the same forward.
 *
 * vy_attn_paged_prefill: causal attention of packed, variable-length query segments against the pages, all prefilling
 *   sequences of a step in ONE launch.  Rows cu_q[s] .. cu_q[s+1] - 1 of q (q + row * q_ld, heads of dh columns side by
 *   side, as vy_attn_paged_decode reads it) belong to sequence s; row i of the segment sits at position ctx_lens[s] + i
 *   and attends to keys [0, ctx_lens[s] + i] of the sequence, read through block_table[s].  ALL keys come from the pages
 *   (vy_paged_rope_write has stored the step's own rows before), so a segment may start anywhere in its sequence:
 *   behind cached prefix blocks, or behind an earlier chunk of the same prompt.  ctx_lens[s] is arbitrary (no multiple
 *   of block_size).  out (row stride o_ld >= h * dh) is written at the same rows, no other row is touched.  cu_q
 *   (n_seq + 1 entries), ctx_lens and block_table int32 [n_seq][bt_stride] live on the device; max_q (>= every segment
 *   length) and max_kv (>= every ctx + length) are host values that only size the launch.  n_seq == 0 is VY_OK without
 *   a launch.  bf16: 64 query rows per workgroup on the MFMA path, every admitted dh; fp32 (parity): one single-query
 *   problem per row, online softmax in fp32, one rounding.  Key rows at or past ctx + length are never read (the tail of
 *   a last page may hold anything).
 *   Memory safety only, as in vy_attn_paged_decode: a key range past bt_stride * block_size is cut to it, a negative
 *   ctx counts as 0, a block-table entry outside [0, max_blocks) is clamped into it -- silently.
 *   replaces: flash_attn_varlen_func(q, k, v, cu_seqlens_q=..., cu_seqlens_k=..., causal=True) of
 *   GroupedQueryAttention.forward in the same notebook -- and, with the keys coming from the pages, also serves what
 *   that call cannot: query segments that start in the middle of a sequence (prefix hits, chunked prefill).
 *
 * vy_paged_gather: keys [0, S) of ONE sequence (block_table: its n_blocks entries, device) copied from the pages into
 *   contiguous (hk, S, dh) buffers, K and V in one launch -- the keys of a prefill that starts from cached prefix blocks.
 *   The rows of a block-table entry outside [0, max_blocks) are written as zeros (memory safety only, silently).
 *
 * fp8 pages (vy_paged_rope_write_fp8, vy_attn_paged_decode_fp8, vy_attn_paged_prefill_fp8): k_cache / v_cache keep their
 *   shape and hold OCP e4m3fn codes, one byte an element; k_scale / v_scale are fp32 (max_blocks, block_size, hk), one
 *   scale per slot and KV head, at the same indices.  The quantisation rule, for the dh values x of one head of one token
 *   as a bf16 page would hold them (k: after the rotation's one bf16 rounding; v: as loaded):
 *       amax = max |x|;  s = amax > 0 ? amax / 448.0f : 1.0f;  code = e4m3fn_rne(clamp(x / s, -448, 448))
 *   with IEEE fp32 divisions; the dequantised value is float(code) * s, an fp32 product.  In torch:
 *   (x / s).clamp(-448, 448).to(torch.float8_e4m3fn).  The three entry points are bf16 only (dtype VY_F32 is
 *   VY_ERR_ARG), a null scale array is VY_ERR_ARG, every other argument and rule is the bf16 twin's.
 *   vy_paged_rope_write_fp8: the arguments of vy_paged_qknorm_rope_write plus the scale arrays; q_scale and k_norm_scale
 *     both null select the plain rotation of vy_paged_rope_write (one null alone is VY_ERR_ARG).  The in-place q / k rows
 *     are bit for bit those of the bf16 entry points (their own kernel runs first, without a page to store to; a second
 *     launch quantises what a bf16 page would hold); a k or v head goes to its slot as dh codes and one scale; a negative
 *     or out-of-range slot stores neither.
 *   vy_attn_paged_decode_fp8 (+ _ws_bytes: its own trip length, so its own automatic split): score = scale * k_s *
 *     (q . codes), out = sum p v_s codes / sum p, fp32 throughout.  Rows at or past seqlen are never read, codes or scales.
 *   vy_attn_paged_prefill_fp8: a fetched key row is dequantised in registers as bf16_rne(float(code) * s); from there on
 *     it is vy_attn_paged_prefill, so it equals that entry on bf16 pages holding those values bit for bit.
 * ------------------------------------------------------------------------------------------ */
int vy_paged_rope_write(void* qkv, int64_t ld, const int32_t* positions, const int64_t* slot_mapping,
                        const float* cos_tab, const float* sin_tab, int64_t table_rows, void* k_cache,
                        void* v_cache, int64_t max_blocks, int block_size, int64_t T, int h, int hk, int dh,
                        int dtype, void* stream);
int vy_paged_qknorm_rope_write(void* qkv, int64_t ld, const int32_t* positions, const int64_t* slot_mapping,
                               const float* cos_tab, const float* sin_tab, int64_t table_rows,
                               const float* q_scale, const float* k_scale, float eps, void* k_cache,
                               void* v_cache, int64_t max_blocks, int block_size, int64_t T, int h, int hk, int dh,
                               int dtype, void* stream);
int vy_attn_paged_decode(const void* q, int64_t q_ld, const int32_t* q_rows, const void* k_cache,
                         const void* v_cache, int64_t max_blocks, int block_size,
                         const int32_t* block_table, int64_t bt_stride, const int32_t* seqlens,
                         int64_t max_seqlen, void* out, int64_t o_ld, int64_t B, int h, int hk, int dh,
                         float scale, int n_split, void* ws, int64_t ws_bytes, int dtype, void* stream);
int64_t vy_attn_paged_decode_ws_bytes(int64_t B, int h, int hk, int dh, int64_t max_seqlen, int n_split, int dtype);
int vy_attn_paged_prefill(const void* q, int64_t q_ld, const void* k_cache, const void* v_cache,
                          int64_t max_blocks, int block_size, const int32_t* block_table, int64_t bt_stride,
                          const int32_t* cu_q, const int32_t* ctx_lens, int64_t n_seq, int64_t max_q,
                          int64_t max_kv, void* out, int64_t o_ld, int h, int hk, int dh, float scale,
                          int dtype, void* stream);
int vy_paged_gather(const void* k_cache, const void* v_cache, int64_t max_blocks, int block_size,
                    const int32_t* block_table, int64_t n_blocks, int64_t S, void* k_out, void* v_out,
                    int hk, int dh, int dtype, void* stream);
int vy_paged_rope_write_fp8(void* qkv, int64_t ld, const int32_t* positions, const int64_t* slot_mapping,
                            const float* cos_tab, const float* sin_tab, int64_t table_rows,
                            const float* q_scale, const float* k_norm_scale, float eps, void* k_cache,
                            void* v_cache, float* k_scale, float* v_scale, int64_t max_blocks, int block_size,
                            int64_t T, int h, int hk, int dh, int dtype, void* stream);
int vy_attn_paged_decode_fp8(const void* q, int64_t q_ld, const int32_t* q_rows, const void* k_cache,
                             const void* v_cache, const float* k_scale, const float* v_scale, int64_t max_blocks,
                             int block_size, const int32_t* block_table, int64_t bt_stride, const int32_t* seqlens,
                             int64_t max_seqlen, void* out, int64_t o_ld, int64_t B, int h, int hk, int dh,
                             float scale, int n_split, void* ws, int64_t ws_bytes, int dtype, void* stream);
int64_t vy_attn_paged_decode_fp8_ws_bytes(int64_t B, int h, int hk, int dh, int64_t max_seqlen, int n_split, int dtype);
int vy_attn_paged_prefill_fp8(const void* q, int64_t q_ld, const void* k_cache, const void* v_cache,
                              const float* k_scale, const float* v_scale, int64_t max_blocks, int block_size,
                              const int32_t* block_table, int64_t bt_stride, const int32_t* cu_q,
                              const int32_t* ctx_lens, int64_t n_seq, int64_t max_q, int64_t max_kv, void* out,
                              int64_t o_ld, int h, int hk, int dh, float scale, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * vy_layernorm_fwd: y = (x - mean) * rstd * gamma + beta over the last dim (biased variance).
 * replaces: nn.LayerNorm in AttentionSelfOutput / FeedForward / LMHead
 *   (VyomAI/layers/attention.py:71, VyomAI/layers/ffn.py:39, VyomAI/models/decoder.py:270).
 * mean/rstd (nullable) fp32 [M] are saved for backward.
 * ------------------------------------------------------------------------------------------ */
int vy_layernorm_fwd(const void* x, int64_t ldx, const void* gamma, const void* beta, void* y,
                     int64_t ldy, float* mean, float* rstd, int64_t M, int64_t N, float eps,
                     int dtype, void* stream);

/* vy_rmsnorm_fwd: y = x * rsqrt(mean(x^2) + eps) * (w_offset + w); Gemma uses w_offset = 1
 * (Examples/paligemma.ipynb cell 11, GemmaRMSNorm).  Statistics in fp32.
 * N, ldx, ldy: multiples of 8 (bf16) / 4 (f32); N <= 8192.  A row stride below N (rows would overlap) is VY_ERR_ARG. */
int vy_rmsnorm_fwd(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int64_t M,
                   int64_t N, float eps, float w_offset, int dtype, void* stream);

/* vy_gated_act_fwd: out[m, i] = act(gate_up[m, i]) * gate_up[m, I + i] -- the GeGLU of GemmaMLP
 * (Examples/paligemma.ipynb cell 11: gelu_tanh(gate_proj(x)) * up_proj(x)) and the SwiGLU of the custom
 * transformer's MLP (VyomAI/models/custom_transformer.py:88) after one packed [gate; up] projection.  Any vy_act
 * but VY_ACT_NONE.  ldg < 2 I or ldo < I (rows would overlap) is VY_ERR_ARG, as in vy_gated_act_bwd. */
int vy_gated_act_fwd(const void* gate_up, int64_t ldg, void* out, int64_t ldo, int64_t M, int64_t I,
                     int act, int dtype, void* stream);

/* vy_rmsnorm_bwd: backward of y = x * r * (w_offset + w), r = rsqrt(mean(x^2) + eps), from x alone (no saved
 * statistics: the row is held in registers, sum x^2 and sum x*g*dy come from the same pass, g = w_offset + w):
 *   dx = r*g*dy - x * r^3/N * sum(x*g*dy) + add_to        dw[n] (+)= sum_rows dy*x*r
 * replaces: the autograd of RMSNorm.forward (VyomAI/models/custom_transformer.py:236-241) at its three call sites
 *   (:269, :286, :488) and the `residual + hidden_states` adds of DecoderLayer (:282, :288): add_to (nullable,
 *   [M,N]) carries the residual branch's gradient into the same store.
 * dw fp32 [N], overwritten (beta = 0) or accumulated (beta = 1), deterministic: per-block partials in `ws` (fp32,
 * at least vy_layernorm_bwd_ws_rows(M) * N elements) are added up in a fixed order, no atomics.
 * N, every ld: multiples of 8 (bf16) / 4 (f32); operands 16-byte aligned; N <= 8192 (bf16) / 4096 (f32) as forward. */
int vy_rmsnorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* w,
                   const void* add_to, int64_t ldadd, void* dx, int64_t lddx, float* dw, float beta,
                   float* ws, int64_t M, int64_t N, float eps, float w_offset, int dtype, void* stream);

/* vy_gated_act_bwd: backward of vy_gated_act_fwd from the saved gate_up[M,2I]:
 *   d_gate_up[m, i] = d_act[m, i] * up * act'(gate)      d_gate_up[m, I + i] = d_act[m, i] * act(gate)
 * replaces: the autograd of `self.act_fn(self.gate_proj(x)) * self.up_proj(x)` (VyomAI/models/custom_transformer.py:88).
 * act' at the kinks as in vy_act (torch's conventions).  Every ld a multiple of 8 (bf16) / 4 (f32), 16-byte aligned. */
int vy_gated_act_bwd(const void* d_act, int64_t lddo, const void* gate_up, int64_t ldg, void* d_gate_up,
                     int64_t lddg, int64_t M, int64_t I, int act, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Qwen3's qk_norm on the training side (Examples/simple_vllm.ipynb cell 2, GroupedQueryAttention.forward).
 * qkv[T][ld] are the packed rows of the plain bias-free QKV GEMM, T = B * L, columns [q heads | k heads | v heads] of dh
 * each, W = (h + 2 hk) * dh <= ld; q_scale / k_scale are fp32 [dh], shared by all heads of their kind.  bf16 and fp32;
 * dh a multiple of 8 up to 256; h a multiple of hk; ld / ldd (and the q / k strides) multiples of 8 (bf16) or 4 (fp32)
 * elements; every pointer 16-byte aligned; eps >= 0.  Anything else is VY_ERR_ARG before a launch.  Neither allocates.
 *
 * vy_qknorm_rope_fwd: for every q and k head of every row, in fp32 from the load to the ONE rounding at the store:
 *   n = x * rsqrt(mean_d(x^2) + eps) * scale, rotated (rotate_half pairing d, d + dh/2) with row pos0 + l of the fp32
 *   cos / sin tables [table_rows][dh/2] (table_rows >= pos0 + L), written to q (B,h,L,dh) / k (B,hk,L,dh) through
 *   element strides {batch, head, token} as vy_qkv_rope_fwd writes them.  The rows of qkv are NOT modified: they are the
 *   saved activation of vy_qknorm_bwd.  The v heads are not touched (vy_attn_fwd / vy_attn_bwd read them in place:
 *   v_sb = L * ld, v_sh = dh, v_sl = ld).  An all-zero head gives zeros.
 *   replaces: `queries = self.q_norm(queries)`, `keys = self.k_norm(keys)` and the two apply_rope calls of
 *   GroupedQueryAttention.forward (prefill branch).  The notebook's bf16 model rounds after each of them.
 *
 * vy_qknorm_bwd: dqkv[T][ldd], layout [dq | dk | dv], holds in its q and k columns the gradient dy of the NORMALISED
 *   heads (vy_attn_bwd leaves it there, un-rotated through its cos / sin arguments).  They are overwritten IN PLACE by
 *   the gradient of the raw projection, dx = r g dy - x r^3 / dh * sum_d(x g dy) with r = rsqrt(mean_d(x^2) + eps)
 *   recomputed from qkv (no saved statistics); the dv columns and any pad columns past W keep their bits.
 *   dq_scale / dk_scale (fp32 [dh]) = beta * themselves + sum over (token, head) of dy * x * r, beta 0 or 1.  The sums
 *   are deterministic: per-workgroup partials go to ws (vy_qknorm_bwd_ws_floats(T, h, hk, dh) floats, 16-byte aligned)
 *   and a second small launch adds them in a fixed order -- no atomics.
 *   replaces: the autograd of the two RMSNorm.forward calls above.
 * ------------------------------------------------------------------------------------------ */
int vy_qknorm_rope_fwd(const void* qkv, int64_t ld, const float* cos_tab, const float* sin_tab, int64_t table_rows,
                       int64_t pos0, const float* q_scale, const float* k_scale, float eps,
                       void* q, int64_t q_sb, int64_t q_sh, int64_t q_sl, void* k, int64_t k_sb, int64_t k_sh,
                       int64_t k_sl, int64_t B, int64_t L, int h, int hk, int dh, int dtype, void* stream);
int64_t vy_qknorm_bwd_ws_floats(int64_t T, int h, int hk, int dh);
int vy_qknorm_bwd(void* dqkv, int64_t ldd, const void* qkv, int64_t ld, const float* q_scale, const float* k_scale,
                  float eps, float* dq_scale, float* dk_scale, float beta, float* ws, int64_t T, int h, int hk,
                  int dh, int dtype, void* stream);

/* vy_rope_fwd: in-place rotary embedding on a (B,heads,L,dh) tensor (strides as above);
 * used when the fused epilogue does not apply.  `inverse` != 0 applies the transpose rotation
 * (the backward of RoPE).  replaces: VyomAI/layers/positional_embeddings.py:155-182. */
int vy_rope_fwd(void* x, int64_t sb, int64_t sh, int64_t sl, const float* cos_tab,
                const float* sin_tab, int64_t pos0, int64_t B, int heads, int64_t L, int dh,
                int inverse, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward / training entry points (bf16 storage, fp32 accumulation).
 * They mirror what autograd derives for the reference modules; the fusion groups follow the
 * author's own fused notebook (Examples/vyom-ai-decoder-fused.ipynb cells 2-7, 11).
 * ------------------------------------------------------------------------------------------ */

/* dX[M,K] = dY[M,N] . W[N,K]  (+ add_to[M,K] + add_to2[M,K]); optional GELU backward: when `pre` is
 * given the result is multiplied by gelu'(pre[M,K]) (pre = saved pre-activation of the consumer of
 * dX).  wt is W transposed, i.e. stored [K,N] row-major (the trainer keeps both copies).  The two
 * addends are the residual-path gradients a layer input collects besides the QKV projection's
 * (add_to2 needs add_to). */
int vy_linear_dgrad(const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const void* pre,
                    int64_t ldpre, int act, const void* add_to, int64_t ldadd, const void* add_to2,
                    int64_t ldadd2, void* dx, int64_t lddx, int64_t M, int64_t N, int64_t K, int dtype,
                    void* stream);

/* dW[N,K] (fp32, accumulate when beta != 0) = alpha * dY[M,N]^T . X[M,K];  db[N] (fp32) likewise
 * alpha * colsum(dY).  alpha_dev: optional DEVICE fp32 scalar (NULL = 1), e.g. the upstream
 * gradient of a loss whose unit gradient is already stored in dY -- no host sync to read it.
 * dtype VY_BF16: MFMA kernels (K, lddy, ldx multiples of 8).  VY_F32: the parity path, plain FMAs
 * (any K; the reference's autograd of nn.Linear in full precision). */
int vy_linear_wgrad(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw,
                    int64_t lddw, float* db, float beta, const float* alpha_dev, int64_t M, int64_t N,
                    int64_t K, int dtype, void* stream);

/* Several weight gradients in one launch: dW_i += dY_i^T X_i and db_i += column sums of dY_i (db_i may be NULL)
 * for 1..8 GEMMs, accumulating (the beta = 1 form of vy_linear_wgrad).  The four projections of a
 * transformer layer (reference: the autograd of the nn.Linear layers at layers/attention.py:87-95, :57-72,
 * layers/ffn.py:19-40) are small as wgrad problems -- 9 to 36 output tiles of 256 x 256 -- and filling the
 * chip one at a time costs M-splits, i.e. fp32 atomic traffic; together they need a quarter of it. */
typedef struct vy_wgrad_desc {
  const void* dy; int64_t lddy;
  const void* x; int64_t ldx;
  float* dw; int64_t lddw;
  float* db;
  int64_t M, N, K;
} vy_wgrad_desc;
int vy_linear_wgrad_grouped(const vy_wgrad_desc* descs, int32_t n, int dtype, void* stream);

/* The same launch with the column sums of up to 8 LayerNorm-backward slabs riding in it (n may be 0 when ncs > 0):
 * out0[N] / out1[N] (fp32, added to when acc = 1, either may be NULL) = the column sums of the two [W, N] slabs
 * vy_layernorm_bwd_partial left in ws, i.e. the dgamma / dbeta that vy_layernorm_bwd computes with two launches of
 * its own per LayerNorm -- bit for bit, the summation order is the same.  bf16: extra workgroups of the grouped launch,
 * on the CUs the weight-gradient tiles leave idle; fp32: the separate launches. */
typedef struct vy_colsum_desc {
  float* ws; int32_t W, N;
  float* out0; float* out1;
  int32_t acc;
} vy_colsum_desc;
int vy_linear_wgrad_grouped_cs(const vy_wgrad_desc* descs, int32_t n, const vy_colsum_desc* cs, int32_t ncs, int dtype,
                               void* stream);

/* The same launch with AdamW riding in it: up to 8 ranges of a flat arena are stepped -- the update of vy_adamw_step
 * (below), bit for bit, without its device scale and gate -- by workgroups dispatched behind the weight-gradient and
 * column-sum ones, on the CUs the tiles leave idle.  The optimizer is an HBM stream and the tiles are not HBM-bound.
 * The ranges must have no data dependence on the launch: a range's g, p and p_bf16 may not intersect any dw, db,
 * out0 / out1 or slab of it (VY_ERR_ARG), and the caller orders the launch behind the kernels that wrote g.
 * How much rides is the launcher's decision: (256 - weight-gradient workgroups) idle CUs x a measured per-CU streaming
 * rate x the estimated duration of the longest weight-gradient workgroup, none when fewer than 8 CUs are idle; the
 * ranges are taken in order and `taken` (out) says how many leading elements of each were stepped -- n, 0, or a whole
 * number of chunks of the last range that fit.  The caller keeps the rest for a later launch or vy_adamw_step.  A launch
 * without weight gradients (n = 0; ncs may be 0 too) takes every range whole.  Range starts: 16-byte aligned in the
 * four fp32 arrays, 8-byte in p_bf16 (nullable).  fp32: the riders run as plain vy_adamw_step launches, all taken.
 * vy_linear_wgrad_grouped and _cs are this entry point with nopt = 0. */
typedef struct vy_adamw_ride_desc {
  float* p; const float* g; float* m; float* v;
  void* p_bf16;
  int64_t n;
  int64_t taken;
} vy_adamw_ride_desc;
typedef struct vy_adamw_hyper {
  float lr, beta1, beta2, eps, weight_decay;
  float grad_scale;
  int64_t step;
} vy_adamw_hyper;
int vy_linear_wgrad_grouped_opt(const vy_wgrad_desc* descs, int32_t n, const vy_colsum_desc* cs, int32_t ncs,
                                vy_adamw_ride_desc* opt, int32_t nopt, const vy_adamw_hyper* hyper, int dtype,
                                void* stream);

/* vy_linear_wgrad with data movement riding in it.  Only the 256 x 256 bf16 launch (N >= 8192, M >= 4096: the vocabulary
 * projection) carries anything: its workgroups are dispatched in rounds of 256, and the workgroups appended behind them
 * land on the 256 - items % 256 CUs that the last round leaves idle.  Two tables, both optional:
 *   zero       up to 8 fp32 ranges {p, n} (p 16-byte aligned) to clear, e.g. the gradient arena before the kernels that
 *              accumulate into it.  A range that meets dw, db, dy or x of this launch is refused (VY_ERR_ARG).
 *   transposes the device table of vy_transpose_batched (below): tr_n descriptors, tr_total_tiles tiles, tr_dtype.  The
 *              table lives on the device, so that no destination meets dw, db, dy or x is the CALLER's to guarantee.
 * Nothing a rider writes may be read or written by anything else before the launch has ended (the riders' only ordering
 * is the stream's kernel boundary).  How much rides is the launcher's decision: idle CUs x a measured per-CU rate x the
 * estimated duration of one tile workgroup, none when the last round is full or leaves fewer than 8 CUs idle.  With
 * both tables present each may use half of that, the zero ranges also what the transposes leave of their half.  The
 * leading *tr_taken (out, nullable) tiles of the table ride: all, or a multiple of 8; the caller runs the rest with
 * vy_transpose_batched_range(first = *tr_taken).  The zero ranges are taken in order: zero[i].taken (out) leading
 * elements of each were cleared -- n, 0, or whole 65536-element chunks of the last range that fit; the caller clears
 * the rest.  fp32, a bf16 launch of the 128 x 128 tiles and an fp32
 * table carry nothing and report 0.  dw / db are what vy_linear_wgrad computes, bit for bit where that is itself
 * order-fixed: the tiles keep their block-to-tile mapping. */
typedef struct vy_zero_ride_desc {
  float* p;
  int64_t n;
  int64_t taken;
} vy_zero_ride_desc;
struct vy_transpose_desc;
int vy_linear_wgrad_riders(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw,
                           float* db, float beta, const float* alpha_dev, int64_t M, int64_t N, int64_t K, int dtype,
                           vy_zero_ride_desc* zero, int32_t nzero, const struct vy_transpose_desc* tr_descs_dev,
                           int32_t tr_n, int32_t tr_total_tiles, int tr_dtype, int32_t* tr_taken, void* stream);

/* LayerNorm backward: dx = rstd*(g - mean(g) - xhat*mean(g*xhat)), g = dy*gamma;
 * dgamma/dbeta fp32 [N] accumulated (beta) from per-block partials in `ws`
 * (ws: fp32, at least 2 * ws_rows * N elements; ws_rows = vy_layernorm_bwd_ws_rows(M)). */
int64_t vy_layernorm_bwd_ws_rows(int64_t M);
int vy_layernorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* gamma,
                     const float* mean, const float* rstd, void* dx, int64_t lddx, float* dgamma,
                     float* dbeta, float beta, float* ws, int64_t M, int64_t N, int dtype,
                     void* stream);
/* dx only: the per-block partials stay in ws ([2][ws_rows][N]) for vy_linear_wgrad_grouped_cs to sum. */
int vy_layernorm_bwd_partial(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* gamma,
                             const float* mean, const float* rstd, void* dx, int64_t lddx, float* ws, int64_t M,
                             int64_t N, int dtype, void* stream);

/* Flash attention backward.  dO/O are (B,L,h*dh) (strides {sb,sl}); dq/dk/dv use q/k/v layouts.
 * delta_ws: fp32 [B,h,L] scratch.  dk/dv are (B,hk,S,dh): the n_rep query heads of one kv head
 * are summed in-kernel.  Same mask descriptor as the forward.  cos_tab/sin_tab (nullable): when
 * q/k were rotated by RoPE (row rope_pos0 + token of the tables), the inverse rotation is applied
 * to dq and dk (in the epilogues at dh = 64 bf16, by rotation launches otherwise), so they are
 * gradients w.r.t. the un-rotated projections.
 * bf16: dh = 64 (tuned kernels) or any multiple of 8 up to 256 (general MFMA kernels; SigLIP's 72 runs
 * as 96 columns).  fp32: the parity path (plain FMAs, expf), dh a multiple of 8 up to 256 -- there a
 * row without a visible key is differentiated as the uniform softmax the forward returned for it
 * (reference layers/attention.py:133-137 under autograd); the bf16 kernels give such rows no gradient. */
int vy_attn_bwd(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_sl,
                const void* k, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                const void* v, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                const void* out, const void* dout, int64_t o_sb, int64_t o_sl, const float* lse,
                float* delta_ws,
                void* dq, int64_t dq_sb, int64_t dq_sh, int64_t dq_sl,
                void* dk, int64_t dk_sb, int64_t dk_sh, int64_t dk_sl,
                void* dv, int64_t dv_sb, int64_t dv_sh, int64_t dv_sl,
                int mask_kind, int64_t start_pos, const uint8_t* keypad, int64_t kp_sb,
                const float* cos_tab, const float* sin_tab, int64_t rope_pos0,
                int64_t B, int h, int hk, int64_t L, int64_t S, int dh, float scale, int dtype,
                void* stream);

/* ---- data-parallel gradient exchange (RCCL) --------------------------------------------------------------------
 * Replaces what the reference gets from accelerate / torch DDP (Examples/vyom-ai-decoder_clm.ipynb cell 31,
 * Examples/vyom-ai-accelerate-multimodel-2t4.ipynb cells 1-2): one process per GPU, one communicator per process.
 *   vy_ddp_unique_id   rank 0 fills 128 bytes; the host hands them to every rank (any side channel: torch.distributed's
 *                      store, MPI, a file)
 *   vy_ddp_init        collective; binds the communicator to the calling thread's current HIP device
 *   vy_ddp_all_reduce_async  in-place SUM of `count` elements (VY_F32 | VY_BF16) enqueued on `stream`: the caller orders
 *                      it behind the kernels that wrote the bucket and ahead of its consumers with events / stream waits
 *                      (there is no separate wait call: completion is stream order)
 * RCCL is bound at run time (the copy already in the process, e.g. torch's, else librccl.so): where it is absent these
 * return VY_ERR_UNSUPPORTED.  The number of CUs RCCL's channel kernels occupy beside the backward GEMMs is RCCL's own
 * knob (NCCL_MAX_NCHANNELS / NCCL_MIN_NCHANNELS in the environment of the process), read at vy_ddp_init. */
int vy_ddp_unique_id(void* id128);
int vy_ddp_init(const void* id128, int rank, int world);
int vy_ddp_world(void);   /* 0 before vy_ddp_init */
int vy_ddp_rank(void);    /* -1 before vy_ddp_init */
int vy_ddp_all_reduce_async(void* buf, int64_t count, int dtype, void* stream);
int vy_ddp_destroy(void);

/* Fused AdamW over a flat fp32 parameter arena; also refreshes the bf16 working copy.
 * p, m, v fp32 [n]; g fp32 [n]; p_bf16 (nullable) bf16 [n].  Matches torch.optim.AdamW. */
int vy_adamw_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int64_t step,
                  float grad_scale, const float* grad_scale_dev, void* stream);
/* The same with a gate (nullable): one fp32 on the device; when it reads 0 the launch changes nothing.  Data-parallel
 * training with parameters that some ranks' batches do not reach (the reference's multimodal model under
 * find_unused_parameters=True, Examples/vyom-ai-accelerate-multimodel-2t4.ipynb cell 1): whether such a parameter is
 * updated is decided by a flag all-reduced over the ranks, read here on the device. */
int vy_adamw_step_gated(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int64_t step,
                        float grad_scale, const float* grad_scale_dev, const float* gate, void* stream);
/* grad_scale_dev (nullable): one fp32 on the device multiplied into grad_scale by the kernel -- the
 * clip_grad_norm_ coefficient min(1, max_norm / (norm + 1e-6)) of the reference's training loops
 * (Examples/vyomai-fused-kernals-2t4.ipynb cell 0) without a host round trip. */

/* out[0] = sum_i x[i]^2 over an fp32 arena (global gradient norm, same loops).  ws: >= 1024 floats of
 * scratch.  Two launches, fixed summation order (run-to-run identical). */
int vy_sumsq(const float* x, int64_t n, float* out, float* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dropout of the two hidden-state sites of a block.
 * replaces: self.dropout(hidden_states) between dense and the residual add in AttentionSelfOutput
 *   (VyomAI/layers/attention.py:55,69-71) and FeedForward (VyomAI/layers/ffn.py:24,37-39), p =
 *   config.hidden_dropout_prob (VyomAI/utils.py:96, default 0.1), active in train().
 * The keep mask is a pure function of (seed, offset, row, column) -- Philox4x32-7 on the counter
 * {column / 8, row, offset}, sixteen bits per element, drop when below round(p * 65536) -- so the forward
 * epilogue, the backward pass and a test all regenerate it; nothing is stored.
 * vy_linear_dropout_fwd: Y = dropout(X . W^T + bias) / (1 - p) + residual   (vy_linear_fwd with the
 *   mask applied in the epilogue, before the residual add).
 * vy_dropout: y = x * keep / (1 - p) as its own pass over an [M, N] view (backward: the same mask on the
 *   incoming gradient; x = ones gives the mask).
 * ------------------------------------------------------------------------------------------ */
int vy_linear_dropout_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias,
                          const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t M, int64_t N,
                          int64_t K, float p_drop, uint64_t seed, uint64_t offset, int dtype, void* stream);
int vy_dropout(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t M, int64_t N, float p_drop,
               uint64_t seed, uint64_t offset, int dtype, void* stream);

/* dx = dy * act'(pre), elementwise over [M,N] row-major views (GELU backward outside a GEMM). */
int vy_act_bwd(const void* dy, int64_t lddy, const void* pre, int64_t ldpre, void* dx, int64_t lddx,
               int64_t M, int64_t N, int act, int dtype, void* stream);

/* Softmax cross-entropy over the vocabulary, ignore_index aware (the CLM loss of
 * Examples/vyom-ai-decoder_clm.ipynb cell 29 after the label shift).
 * fwd: lse[m] = logsumexp(logits[m,:V]); loss_sum += sum_m (lse[m] - logits[m,label]) and
 *      count += #(label != ignore) -- both fp32 scalars on the device, accumulated atomically
 *      (zero them first).
 * bwd: logits[m,:] <- (softmax(logits[m,:]) - onehot(label)) * (*gscale) / (*count), in place
 *      (rows with label == ignore become 0); gscale/count are device pointers: no host sync. */
int vy_xent_fwd(const void* logits, int64_t ld, const int64_t* labels, int64_t ignore_index, float* lse,
                float* loss_sum, float* count, int64_t M, int64_t V, int32_t* err_flag, int dtype, void* stream);
int vy_xent_bwd(void* logits, int64_t ld, const int64_t* labels, int64_t ignore_index, const float* lse,
                const float* gscale, const float* count, int64_t M, int64_t V, int dtype, void* stream);
/* Both in ONE pass over the logits (bf16, V <= 65536): `count` (device scalar: the number of rows
 * with label != ignore) is an INPUT here; lse and loss_sum as in vy_xent_fwd, then the row is
 * overwritten in place as in vy_xent_bwd.  The logits cross HBM once in each direction. */
int vy_xent_fused(void* logits, int64_t ld, const int64_t* labels, int64_t ignore_index, float* lse,
                  float* loss_sum, const float* count, const float* gscale, int64_t M, int64_t V,
                  int32_t* err_flag, int dtype, void* stream);
/* vy_xent_fwd / vy_xent_fused that also sample one replacement token per live row: ELECTRA's generator step,
 * replaces sample(logits[masked_indices], temperature) = argmax(t / temperature + noise(t)) with
 * noise(t) = -log(-log(uniform + 1e-9) + 1e-9) (VyomAI/pretraining/collators.py:65-78,88-91): a zeros_like, a
 * uniform_, two logs, an add and an argmax over the gathered rows, i.e. a second pass over the generator logits.
 * sampled[m] = argmax_v fp32(logits[m,v] * inv_temperature + noise(m,v)), the lowest index among equal maxima;
 * skipped rows (ignore_index, or an out-of-range label, which still raises err_flag) get -1, as does a row whose scores are all NaN.  noise(m,v) is a pure
 * function of (seed, offset, m, v): Philox4x32-7 on the counter {v / 4, m, offset}, word v & 3, u = its top 24
 * bits * 2^-24.  lse, each row's term of loss_sum and (fused) the in-place unit gradient are those of vy_xent_fwd /
 * vy_xent_fused bit for bit (loss_sum itself is, there as here, a float atomic over rows in arrival order); the limits
 * are theirs (fused: bf16, V <= 65536); backward of the unfused form is vy_xent_bwd. */
int vy_xent_sample_fwd(const void* logits, int64_t ld, const int64_t* labels, int64_t ignore_index, float* lse,
                       float* loss_sum, float* count, int64_t* sampled, float inv_temperature, uint64_t seed,
                       uint64_t offset, int64_t M, int64_t V, int32_t* err_flag, int dtype, void* stream);
int vy_xent_sample_fused(void* logits, int64_t ld, const int64_t* labels, int64_t ignore_index, float* lse,
                         float* loss_sum, const float* count, const float* gscale, int64_t* sampled,
                         float inv_temperature, uint64_t seed, uint64_t offset, int64_t M, int64_t V,
                         int32_t* err_flag, int dtype, void* stream);
/* out[m, v] (fp32, row stride ld) = noise(m, v) of the two calls above, for tests (as vy_dropout exports the mask). */
int vy_gumbel_noise(float* out, int64_t ld, int64_t M, int64_t V, uint64_t seed, uint64_t offset, void* stream);

/* ELECTRA's discriminator head and loss: replaces nn.Linear(hidden_size, 1) (Examples/electra-pretraining.ipynb
 * cell 21, Discriminator.discriminator_head) and binary_cross_entropy_with_logits over the non-pad tokens (cell 27,
 * ElectraLoss.__call__).  An N = 1 GEMM wastes an MFMA tile; these read h once per pass, one wave per row.
 * fwd: z[m] (fp32) = h[m,:] . w + b (w [d], b [1] in h's dtype, b nullable; fp32 accumulation).  With target (fp32
 *      0 / 1) and live (uint8) given, loss_sum += sum over live rows of max(z,0) - z y + log1p(exp(-|z|)) (fp32 device
 *      scalar, atomic: zero it first); target == NULL only writes z (Discriminator.forward).
 * bwd: dz[m] = (sigmoid(z[m]) - y[m]) * (*gscale) / max(*count, 1) on live rows, 0 elsewhere; dh[m,:] = dz[m] w in h's
 *      dtype (dead rows are written as zeros); dw[d] / db[1] (fp32) = sum_m dz[m] h[m,:] / sum_m dz[m], added to what
 *      is there when accumulate != 0 (the convention of vy_linear_wgrad's beta), by fp32 atomics.  gscale / count:
 *      device scalars, no host sync.  d % 8 == 0, rows 16-byte aligned.  bwd keeps a wave's share of w and of the dw
 *      partials in registers: d <= 4096 in bf16, d <= 2048 in fp32 (VY_ERR_UNSUPPORTED beyond); fwd takes any d. */
int vy_bce_head_fwd(const void* h, int64_t ldh, const void* w, const void* b, float* z, const float* target,
                    const uint8_t* live, float* loss_sum, int64_t M, int64_t d, int dtype, void* stream);
int vy_bce_head_bwd(const void* h, int64_t ldh, const void* w, const float* z, const float* target,
                    const uint8_t* live, const float* gscale, const float* count, void* dh, int64_t lddh, float* dw,
                    float* db, int accumulate, int64_t M, int64_t d, int dtype, void* stream);

/* Masked-LM corruption of n token ids in one launch: replaces masked_language_modeling
 * (VyomAI/pretraining/collators.py:9-62) -- the per-row tolist() round trip through
 * tokenizer.get_special_tokens_mask, three bernoulli draws and a randint -- with the same distribution (not the same
 * random stream, as with dropout).  One Philox4x32-7 call per token on the counter {i, offset}: token i is selected
 * iff its id is not in special_ids[n_special] (device, may be empty) and r0 < fraction * 2^32; a selected token
 * becomes mask_id if r1 < 0.8 * 2^32, else umulhi(r3, vocab) if r2 < 0.5 * 2^32, else stays.  labels = ids on
 * selected tokens and ignore_index elsewhere; masked (uint8) marks the selection. */
int vy_mlm_mask(const int64_t* ids, int64_t n, const int64_t* special_ids, int32_t n_special, float fraction,
                int64_t mask_id, int64_t vocab, int64_t ignore_index, uint64_t seed, uint64_t offset,
                int64_t* masked_ids, int64_t* labels, uint8_t* masked, void* stream);

/* A label that is neither ignore_index nor inside [0, V) (torch.cross_entropy device-asserts on it) is
 * never dereferenced: the row counts as ignored (zero loss, zero gradient) and *err_flag (nullable,
 * device int32) is set to 1 for the host to report. */

/* Per-row log-probability of the label, for per-SEQUENCE scores (direct preference optimisation:
 * Examples/vyom-ai-llm-sft-dpo-training.ipynb, the cells defining compute_logprobs -- log_softmax, gather and
 * the mask -- and, through it, compute_dpo_loss_batch).  weight[m] (fp32) is the row's share of its sequence's
 * masked average; rows with weight == 0 are skipped.  Nothing is reduced across rows: the caller sums
 * weight * logp over each sequence in a fixed order, so two runs agree bit for bit.
 * fwd:   read-only; lse[m] = logsumexp(logits[m,:V]), logp[m] = logits[m,label] - lse[m]; skipped rows get
 *        lse = logp = 0.
 * bwd:   logits[m,:] <- weight[m] * (onehot(label) - softmax(logits[m,:])), in place, from the saved lse (the
 *        sign of a log-probability, not of a loss); pad columns and skipped rows become 0.
 * fused: both in ONE pass (bf16, V <= 65536): the logits cross HBM once in each direction.
 * A label outside [0, V) on a row with weight != 0 is never dereferenced: the row counts as skipped and
 * *err_flag (nullable, device int32) is set to 1. */
int vy_logprob_fwd(const void* logits, int64_t ld, const int64_t* labels, const float* weight, float* lse,
                   float* logp, int64_t M, int64_t V, int32_t* err_flag, int dtype, void* stream);
int vy_logprob_bwd(void* logits, int64_t ld, const int64_t* labels, const float* weight, const float* lse,
                   int64_t M, int64_t V, int dtype, void* stream);
int vy_logprob_fused(void* logits, int64_t ld, const int64_t* labels, const float* weight, float* lse,
                     float* logp, int64_t M, int64_t V, int32_t* err_flag, int dtype, void* stream);

/* Token embedding (nn.Embedding: VyomAI/models/decoder.py:287, encoder.py:41, multimodel.py):
 * fwd: out[m,:] = table[ids[m],:] (bf16 or fp32).  Ids outside [0,V) give a zero row and set the
 *      optional device flag *err_flag to 1 (the host cannot check ids without a sync).
 * bwd: dW[ids[m],:] += dOut[m,:] in fp32 (atomics), except for id == padding_idx (pass -1 for none). */
int vy_embedding_fwd(const void* table, int64_t ldt, const int64_t* ids, void* out, int64_t ldo,
                     int64_t M, int64_t d, int64_t V, int32_t* err_flag, int dtype, void* stream);
int vy_embedding_bwd(const void* dout, int64_t lddo, const int64_t* ids, float* dw, int64_t lddw,
                     int64_t padding_idx, int64_t M, int64_t d, int64_t V, int dtype, void* stream);

/* out[c, r] = in[r, c] for a [R,C] matrix (bf16 or f32): keeps W^T copies for dgrad. */
int vy_transpose(const void* in, int64_t ldin, void* out, int64_t ldout, int64_t R, int64_t C,
                 int dtype, void* stream);

/* Many transposes in one launch: descs_dev is a DEVICE array of n descriptors; tile0 is the running
 * sum of ceil(R/64)*ceil(C/64) over the preceding descriptors, tiles_c = ceil(C/64), total_tiles the
 * sum over all.  Used once per training step for every W^T the dgrad GEMMs read. */
typedef struct vy_transpose_desc {
  const void* in; void* out;      /* in: [R,C] row-major (ldin); out: [C,R] (ldout) */
  int64_t ldin, ldout;
  int32_t R, C, tile0, tiles_c;
} vy_transpose_desc;              /* 48 bytes */
int vy_transpose_batched(const vy_transpose_desc* descs_dev, int32_t n, int32_t total_tiles, int dtype,
                         void* stream);
/* Tiles first .. first + count - 1 of the same table (what vy_linear_wgrad_riders did not take). */
int vy_transpose_batched_range(const vy_transpose_desc* descs_dev, int32_t n, int32_t first, int32_t count, int dtype,
                               void* stream);

/* Sampling front end of the generate loops.
 * vy_greedy_step replaces reference models/decoder.py:478-507 (topk(k=1), the where() that forces prompt
 *   tokens, the token write, the isin()/or of the EOS bookkeeping and the all() reduction) for one
 *   generated position: for row b, next = argmax_v logits[b,v] (lowest index among equal maxima) unless
 *   text_mask[b,cur_pos] != 0 (the row is still inside its prompt), then next = tokens[b,cur_pos];
 *   tokens[b,cur_pos] = next; eos_reached[b] |= !forced && next in eos_ids[0..n_eos); *not_done (may be
 *   NULL; zeroed by the caller) += number of rows with eos_reached[b] == 0 afterwards.
 * vy_sampling_probs replaces reference logits_processors.py LogitsProcessor.__call__ for the five
 *   processors: probs = softmax(mask(logits) / temperature) in fp32.  top_k > 0 keeps the values >= the
 *   k-th largest (:59-63); 0 < top_p < 1 keeps the descending-sorted prefix up to and including the first
 *   element whose cumulative softmax of the unscaled, top-k-masked logits exceeds top_p (:73-81, :92-102);
 *   masked entries get probability exactly 0 (the reference writes -1e20 into them).  Equal logits at
 *   the nucleus cut are all kept (the reference keeps an implementation-defined subset of a tie). */
int vy_greedy_step(const void* logits, int64_t ldl, int64_t B, int64_t V, int dtype, int64_t* tokens,
                   int64_t ldt, int64_t cur_pos, const uint8_t* text_mask, int64_t ldm,
                   const int64_t* eos_ids, int32_t n_eos, uint8_t* eos_reached, int32_t* not_done, void* stream);
int vy_sampling_probs(const void* logits, int64_t ldl, int64_t B, int64_t V, int dtype, float temperature,
                      int32_t top_k, float top_p, float* probs, int64_t ldp, void* stream);
/* vy_sample_rows: the processors above (reference logits_processors.py:13-16, 59-63, 73-81, 92-102) and their
 *   torch.multinomial draw (:48-49) for the R rows of one serving step, every row with its own parameters (all five
 *   arrays: device, length R), in ONE launch that writes nothing but tokens[r] in [0, V).
 *   inv_temperature[r] == 0: a greedy row, tokens[r] = argmax_v logits[r, v], lowest index among equal maxima; the
 *   row's other parameters are not read.  Otherwise tokens[r] = argmax over the kept columns v of
 *   fmaf(logits[r, v], inv_temperature[r], noise(v)), lowest index among equal scores, where the kept set is exactly
 *   the support of vy_sampling_probs for top_k[r] / top_p[r] (<= 0 or >= V, <= 0 or >= 1: that filter is off; the two
 *   kernels share the selection code) and noise(v) is vy_gumbel_noise's value at row 0, column v for
 *   (seed[r], offset = counter[r]) -- the noise row is always 0, so a draw does not depend on where the row sits in
 *   the launch.  seed[r] carries the 64-bit seed's bit pattern.  argmax(x / T + Gumbel) is a draw from
 *   softmax(x / T) over the kept set.  A row without a filter is read once; columns V .. ldl - 1 are never read.
 *   inv_temperature must be >= 0 and not NaN (the caller's duty: the kernel cannot report it).
 *   VY_ERR_ARG: a null pointer, R <= 0, V <= 0, V > 0x7ffffff0, ldl < V, an unknown dtype. */
int vy_sample_rows(const void* logits, int64_t ldl, int64_t R, int64_t V, int dtype, const float* inv_temperature,
                   const int32_t* top_k, const float* top_p, const int64_t* seed, const int64_t* counter,
                   int64_t* tokens, void* stream);
/* vy_spec_verify: the accept / reject / resample rule of speculative decoding (reference speculative_decoding.py:73-83
 *   norm_fn, :195-230 the rejection loop and the adjusted draw; the processors logits_processors.py:13-16, 59-63, 73-81,
 *   92-102 and their multinomial draw :48-49) for every drafted token of every sequence of one serving step, every
 *   sequence with its own parameters, in ONE launch: grid (S, gamma + 1), one workgroup per (sequence s, row i).  No
 *   probability tensor is written.
 *   target_logits: (t_rows, V), leading dimension ldt; sequence s owns rows t_row0[s] .. t_row0[s] + n_draft[s].
 *   draft_logits: row (i, s) starts at i * ldd_i + s * ldd_s elements; rows with i >= n_draft[s] are never read.
 *   draft_tokens: (gamma, S) int64, contiguous.  Per sequence (device, length S): n_draft int32 in [0, gamma],
 *   inv_temperature, top_k, top_p, seed as for vy_sample_rows, position0 = the position of the first drafted token.
 *   accept: (S, gamma + 1) int32, alt: (S, gamma + 1) int64 -- the token to emit if the round ends at row i.
 *   Row i < n_draft[s], x = draft_tokens[i][s], t / d the target / draft row:
 *     greedy (inv_temperature[s] == 0): a = argmax t, lowest index among equal maxima; accept = (a == x); alt = a.
 *     sampled: p(c) = [c in Kp] exp((t_c - max t) inv_t) / Zp and q(c) likewise from d, Kp / Kq the kept sets of
 *       vy_sampling_probs for top_k[s] / top_p[s], Zp summed as vy_sampling_probs sums it.  u = the top 24 bits of
 *       word 0 of quad 0 of noise row 1 for (seed[s], offset = position0[s] + i), times 2^-24.  Rejected iff x lies
 *       outside Kp or u q(x) > p(x) (the reference's r > p / q without the division).  A rejected row's alt = argmax
 *       over the columns with p(c) > q(c) of log(p(c) - q(c)) + noise(row 2, column c, same seed and offset), lowest
 *       index among equal scores: a Gumbel-max draw from norm_fn(p - q); if no column has p > q (rounding only), the
 *       draw is from p with the same noise.  An accepted row writes alt = -1.
 *   Row i == n_draft[s]: accept = 0 and alt = exactly vy_sample_rows' token for that target row with
 *     counter = position0[s] + n_draft[s] (the same code, noise row 0), so n_draft[s] == 0 is the plain step's draw.
 *   Rows i > n_draft[s], and every row of a sequence with n_draft outside [0, gamma] or rows outside [0, t_rows):
 *     accept = 0, alt = -1, nothing is read.
 *   Noise rows 1 and 2 are Philox counters disjoint from row 0, which drew the draft at that position.
 *   VY_ERR_ARG: a null pointer, S <= 0, gamma < 1, gamma > 16, t_rows <= 0, V <= 0, V > 0x7ffffff0, ldt < V,
 *   ldd_s < V, ldd_i < 0, an unknown dtype. */
int vy_spec_verify(const void* target_logits, int64_t ldt, int64_t t_rows, const void* draft_logits, int64_t ldd_i,
                   int64_t ldd_s, int64_t S, int64_t gamma, int64_t V, int dtype, const int64_t* draft_tokens,
                   const int32_t* t_row0, const int32_t* n_draft, const float* inv_temperature, const int32_t* top_k,
                   const float* top_p, const int64_t* seed, const int64_t* position0, int32_t* accept, int64_t* alt,
                   void* stream);

/* vy_lora_shrink / vy_lora_expand: the per-request LoRA delta of a serving step (reference layers/adapters.py
 *   LoraLinear.forward: linear(x) + scale * F.linear(F.linear(x, lora_a), lora_b); lora_dropout is the identity at
 *   inference), added in place AFTER the projection's own GEMM, whatever its epilogue did (bias, residual):
 *     u[t, 0:R]  = x[t, 0:K] @ A[slot].T                                              (shrink)
 *     y[t, n]   += alpha[slot] * sum_{j < r_pad} u[t, part(n) * r_pad + j] * B[slot][n, j]     (expand)
 *   for the rows t of the tiles.  tiles: device int32 (n_tiles, 3) = (row0, nrows, slot): nrows <= 16 consecutive rows
 *   of the packed buffer that belong to one request.  A tile is skipped UNREAD -- no load, no store -- when slot lies
 *   outside [0, slots), when nrows lies outside [1, 16] or when its rows leave [0, T).  Rows outside every tile, the
 *   columns N .. ldy - 1 of y and everything behind row T are never written.  Two tiles must not share a row.
 *   A: (slots, R, K) contiguous, R = parts * r_pad, the lora_a of a packed projection's parts stacked ([A_q; A_k; A_v],
 *   [A_gate; A_up]), each part's rank padded with zero rows to r_pad.  B: (slots, N, r_pad) contiguous, the parts'
 *   lora_b stacked along N, padded with zero columns.  part(n) = (n >= bound0) + (n >= bound1); a boundary that is not
 *   used is passed as N.  alpha: fp32 (slots).  x, A, u, B, y share `dtype`.
 *   Rounding: products accumulate in fp32 (bf16: mfma_f32_16x16x32_bf16; fp32: mfma_f32_16x16x4f32, a k-ordered fma
 *   chain per quarter of K, the quarters added in order); u is stored in `dtype` -- in bf16 that is the reference's own
 *   rounding of F.linear(x, lora_a) -- and y = round(fmaf(alpha, sum, y)), rounded once.
 *   Shape limits: K % 32 == 0, r_pad % 32 == 0, N % 16 == 0, boundaries % 16 == 0 with 0 < bound0 <= bound1 <= N,
 *   ldu >= R; rows of x, A, u (as expand reads it) and B 16-byte aligned, rows of u (as shrink writes it) and y aligned
 *   to four elements.  n_tiles == 0 launches nothing.  VY_ERR_ARG otherwise, and for a null pointer or unknown dtype. */
int vy_lora_shrink(const void* x, int64_t ldx, const void* A, const int32_t* tiles, int64_t n_tiles, void* u,
                   int64_t ldu, int64_t T, int64_t K, int64_t R, int64_t slots, int dtype, void* stream);
int vy_lora_expand(void* y, int64_t ldy, const void* u, int64_t ldu, const void* B, const float* alpha,
                   const int32_t* tiles, int64_t n_tiles, int64_t T, int64_t N, int64_t r_pad, int64_t slots,
                   int64_t bound0, int64_t bound1, int dtype, void* stream);

/* vy_lora_expand_epi: vy_lora_expand with the epilogue of the GEMM it follows, for LoRA fine-tuning of the post-LN
 *   encoder block (vyomai_amd/encoder_lora_train.py).  The reference wraps the nn.Linear itself (layers/adapters.py:21-47,
 *   LoraLinear.forward; Examples/adapters.ipynb wraps query / value / attention.output.dense / intermediate.dense /
 *   output.dense), so the adapter's term sits INSIDE whatever follows the linear: the activation of FeedForward
 *   (layers/ffn.py:34-36) and the dropout of AttentionSelfOutput and FeedForward (layers/attention.py:69-72,
 *   layers/ffn.py:37-40).  z (T, N) is the base GEMM's output with its bias and nothing else, in `dtype`; per element
 *     v = fmaf(alpha[slot], sum_{j < r_pad} u[t, part(n) * r_pad + j] * B[slot][n, j], (float)z[t, n])      fp32, not rounded
 *   VY_LORA_EPI_ACT:      out = act(v), pre = act'(v) -- every vy_act but VY_ACT_NONE, the exact (not the reduced-cost)
 *     functions of the GEMM epilogue, so pre is what vy_linear_dgrad takes with pre= and act | 0x100.
 *   VY_LORA_EPI_DROP_RES: out = keep(t, n) ? v * scale + res[t, n] : res[t, n], the mask of vy_dropout for the same
 *     (p_drop, seed, offset) with t the row of the (T, N) matrix; p_drop == 0 is out = v + res.  0 <= p_drop < 1.
 *   VY_LORA_EPI_MUL:      out = v * pre[t, n], pre read-only: the backward's twin of ACT.  With z the base dgrad of the
 *     GEMM behind the activation, u = dY @ B and B := the transposed stacked A (r_pad := R, no boundaries), out is the
 *     gradient of the pre-activation, (dY W + alpha (dY B) A) * act'(v): the adapter's term has to be inside the product.
 *   out may be z (every element is read and written by one lane); pre and res may not overlap out.  Each result is
 *   rounded to `dtype` once.  Tiles, boundaries, skipped tiles, shape limits and alignment: vy_lora_expand's, with z, out,
 *   pre and res in the place of y.  pre is null in DROP_RES mode, res in the others.  VY_ERR_ARG: an unknown mode or act, a
 *   missing pre / res, p_drop outside [0, 1), and everything vy_lora_expand refuses. */
enum { VY_LORA_EPI_ACT = 0, VY_LORA_EPI_DROP_RES = 1, VY_LORA_EPI_MUL = 2 };
int vy_lora_expand_epi(const void* z, int64_t ldz, void* out, int64_t ldo, void* pre, int64_t ldp, const void* res,
                       int64_t ldr, const void* u, int64_t ldu, const void* B, const float* alpha, const int32_t* tiles,
                       int64_t n_tiles, int64_t T, int64_t N, int64_t r_pad, int64_t slots, int64_t bound0,
                       int64_t bound1, int mode, int act, float p_drop, uint64_t seed, uint64_t offset, int dtype,
                       void* stream);

/* vy_cls_head_fwd / vy_cls_head_bwd: the sequence-classification head of Examples/adapters.ipynb and
 *   vyom-ai-classification.ipynb (ClinicModel: hidden[:, 0, :] -> nn.Linear(hidden, n_classes) -> CrossEntropyLoss).
 *   h: the encoder's hidden state (B, L, d) in `dtype`, ldb = the stride between sequences (L * d); only row 0 of each
 *   sequence is read.  w (C, d) contiguous and bias (C, nullable) in `dtype`.
 * fwd: logits[b, c] (fp32, (B, C) contiguous) = h[b, 0, :] . w[c] + bias[c], fp32 accumulation.  With labels (int64,
 *      B): lse[b] (fp32), *loss = sum_b (lse[b] - logits[b, label_b]) / count and, IN PLACE, logits <- dlogits =
 *      (softmax - onehot) / count, count = the rows whose label lies in [0, C) (at least 1).  A label outside [0, C) is
 *      never dereferenced and never clamped: its row adds no loss, gets a zero gradient and sets *err_flag = 1 (nullable;
 *      the flag of the vy_xent entry points).
 * bwd: dw[c, :] = g * sum_b dlogits[b, c] h[b, 0, :], db[c] = g * sum_b dlogits[b, c] (fp32, contiguous, db nullable;
 *      added to what is there when accumulate == 1), dh (B, L, d) contiguous in `dtype`: dh[b, 0, :] = g * dlogits[b] @ w
 *      and every other row zero, written by the same launch.  g = *gscale (device fp32, null = 1).
 * Determinism: sums over b and over c run in ascending order, the d-sum of a logit in one wave's shuffle tree; no
 *      atomics: two calls give the same bits.  1 <= B <= 8192, C >= 1, d % 8 == 0, ldb % 8 == 0, h / w / dh 16-byte
 *      aligned.  VY_ERR_ARG otherwise, for a null operand and an unknown dtype. */
int vy_cls_head_fwd(const void* h, int64_t ldb, const void* w, const void* bias, float* logits, const int64_t* labels,
                    float* lse, float* loss, int32_t* err_flag, int64_t B, int64_t C, int64_t d, int dtype, void* stream);
int vy_cls_head_bwd(const void* h, int64_t ldb, const void* w, const float* dlogits, const float* gscale, void* dh,
                    float* dw, float* db, int accumulate, int64_t B, int64_t L, int64_t C, int64_t d, int dtype,
                    void* stream);

/* vy_lora_wgrad: both low-rank weight gradients of one GEMM group of LoRA fine-tuning (vyomai_amd/lora_train.py), for
 *   the parts p of a packed projection (part(n) and bound0 / bound1 as in vy_lora_expand; a boundary that is not used
 *   is N, so parts = 1 + (bound0 < N) + (bound1 < N) <= 3; col0_p is the part's first column):
 *     dB_p[n, j] (+)= alpha * sum_m dY[m, col0_p + n] * u[m, p * r_pad + j]     fp32 (out_p, rank_p), row stride rank_p
 *     dA_p[j, k] (+)= alpha * sum_m t[m, p * r_pad + j]  * x[m, k]              fp32 (rank_p, K),     row stride K
 *   dY (M, N) is the gradient of the group's output, x (M, K) its input, u (M, R) what vy_lora_shrink left in the
 *   forward and t (M, R) = dY @ B per part; R = parts * r_pad; dY, u, x, t share `dtype`.  A part whose dA_p and dB_p
 *   are both null has no adapter and is neither written nor multiplied.  rank_p <= r_pad: the columns j >= rank_p of
 *   u / t never reach an output.  accumulate = 1 adds to the outputs, 0 overwrites them.
 *   Rounding: products are exact and accumulate in fp32 (bf16: mfma_f32_16x16x32_bf16, fp32: mfma_f32_16x16x4f32).
 *   Determinism: M is cut into chunks of vy_lora_wgrad_chunk_rows(M, N, K) rows -- the shapes alone decide -- whose fp32
 *   partial tiles go to the stream's workspace (vy_workspace_set; (N * r_pad + R * K) * chunks floats are needed) and
 *   are added in chunk order by a second launch: no atomics, two runs give the same bits.
 *   VY_ERR_ARG: a null operand, no part with outputs, one of dA_p / dB_p without the other, M <= 0, K % 32, N or a
 *   boundary not a multiple of 16, r_pad other than 32 or 64, rank_p outside [1, r_pad], row strides below the widths,
 *   rows of dY, u, x, t not 16-byte aligned, accumulate other than 0 / 1, an unknown dtype, no workspace of that size. */
int vy_lora_wgrad(const void* dy, int64_t lddy, const void* u, int64_t ldu, const void* x, int64_t ldx, const void* t,
                  int64_t ldt, float* dA0, float* dA1, float* dA2, float* dB0, float* dB1, float* dB2, int64_t rank0,
                  int64_t rank1, int64_t rank2, int64_t M, int64_t N, int64_t K, int64_t r_pad, int64_t bound0,
                  int64_t bound1, float alpha, int accumulate, int dtype, void* stream);
int64_t vy_lora_wgrad_chunk_rows(int64_t M, int64_t N, int64_t K);

/* DoRA fine-tuning (vyomai_amd/dora_train.py): the reference's DoraLinear (VyomAI/layers/adapters.py:50-75) is a
 *   re-parameterisation of the weight,
 *     D = W + dora_a @ dora_b   (out, in)      c[k] = ||D[:, k]||_2, no epsilon      W'[n, k] = dora_m[k] * D[n, k] / c[k]
 *   with dora_a (out, r), dora_b (r, in), dora_m (in).  Both entry points take a table of 1..8 problems, so that the
 *   seven projections of a decoder layer are one call.  w: (out, in) in w_dtype (VY_F32 | VY_BF16), row stride ldw;
 *   a, b, m, c and every gradient: fp32, contiguous.  D = W + an fma chain over j = 0..r-1 in that order; it is never
 *   written to memory.
 *   vy_dora_compose: D and the sum of its squares over the rows accumulate in fp64 (a bf16 W' is held to 2^-8 |W'| per
 *     element, which an fp32 chain misses where W and a b cancel; fp32 products are exact in fp64), c (written) is the
 *     square root rounded to fp32; wp (out, in) in out_dtype, row stride ldwp -- a part of a packed projection points
 *     into its row block of the packed buffer -- = fp32(D) * (m / c) in fp32, rounded once more at a bf16 store.  Rows and columns outside (out, in) are never written.  g, dm, da, db are ignored.
 *   vy_dora_bwd: with g = dL/dW' (out, in) fp32, row stride ldg, p[k] = sum_n g[n, k] D[n, k] and s[k] = m[k] / c[k]:
 *       dm[k] (+)= p[k] / c[k]        dD[n, k] = s[k] * (g[n, k] - (p[k] / c[k]^2) * D[n, k])
 *       da (out, r) (+)= dD @ b^T     db (r, in) (+)= a^T @ dD
 *     D is recomputed in fp32; c is read (what vy_dora_compose left); wp is ignored.  accumulate = 1 adds to dm / da /
 *     db, 0 overwrites them.
 *     Two launches: a column-stripe pass owns p, dm and db (p goes to the stream's workspace, vy_workspace_set: the sum
 *     of the problems' `in` floats), a row-block pass owns da.  Every output element has one owner that sums in a fixed
 *     order: no atomics, two runs give the same bits.
 *   VY_ERR_ARG: n outside 1..8, a null operand, in or out not a positive multiple of 8, r outside 1..64, a row stride
 *   below `in`, an unknown dtype, accumulate other than 0 / 1, vy_dora_bwd on a stream without that workspace. */
typedef struct vy_dora_desc {
  const void* w; int64_t ldw; int32_t w_dtype;
  const float* a; const float* b; const float* m;
  float* c;
  void* wp; int64_t ldwp;
  const float* g; int64_t ldg;
  float* dm; float* da; float* db;
  int64_t out, in, r;
} vy_dora_desc;
int vy_dora_compose(const vy_dora_desc* descs, int32_t n, int out_dtype, void* stream);
int vy_dora_bwd(const vy_dora_desc* descs, int32_t n, int accumulate, void* stream);

/* y = x converted between fp32 and bf16 (n elements). src_dtype -> dst_dtype. */
int vy_cast(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Native decode driver: one call runs a whole single-token step (L == 1) of the GPT-style
 * decoder -- every layer's QKV+RoPE (K/V appended to the static cache in place), cached
 * attention, out-projection + residual + LayerNorm, FFN + residual + LayerNorm, then the LM head
 * -- as ~8 launches per layer with no host work in between.
 * replaces: the per-token body of DecoderModel.generate / DecoderModel.forward for seqlen == 1
 *   (VyomAI/models/decoder.py:343-374, 477-488) and DecoderLayer.forward (:222-250).
 * All pointers are device pointers; weights are `dtype` (bf16 or f32) in nn.Linear layout.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void *wqkv, *bqkv;          /* packed [(h+2hk)*dh, d], [(h+2hk)*dh] (bias may be NULL) */
  const void *wo, *bo, *ln1_w, *ln1_b;
  const void *w1, *b1, *w2, *b2, *ln2_w, *ln2_b;
  void *kcache, *vcache;            /* (B, hk, cap, dh) */
  int64_t c_sb, c_sh, c_sl;         /* cache element strides {batch, head, token} */
} vy_decode_layer;

typedef struct {
  int32_t num_layers, B, d, h, hk, dh, ffn, vocab, act, dtype;
  float eps_attn, eps_ffn, eps_head;
  const float *cos_tab, *sin_tab;   /* NULL: no RoPE (additive position encodings) */
  const vy_decode_layer* layers;    /* host array [num_layers] */
  const void *head_wd, *head_bd, *head_ln_w, *head_ln_b, *head_wv, *head_bias;
  void* ws; int64_t ws_bytes;       /* device workspace, >= vy_decode_ws_bytes(...) */
} vy_decode_plan;

int64_t vy_decode_ws_bytes(int32_t B, int32_t d, int32_t h, int32_t hk, int32_t dh, int32_t ffn,
                           int32_t dtype);
/* x: (B, d) input embeddings (+ position info); pos: index of this token (keys 0..pos are
 * attended); hidden_out (nullable): (B, d) last hidden state; logits (nullable): (B, ldv).
 * pos_dev (nullable): device int32 holding the position -- when given, every kernel reads the
 * position on the device and `pos` is ignored, so one captured hipGraph of this call can be
 * replayed for every token (bf16, head_dim 64 models). */
int vy_decoder_step(const vy_decode_plan* plan, const void* x, int64_t pos, const int32_t* pos_dev,
                    void* hidden_out, void* logits, int64_t ldv, void* stream);

/* ------------------------------------------------------------------------------------------
 * vy_gemma_decoder_step: one single-token step of a Gemma-style decoder stack (BASELINE configs[4], the
 * PaliGemma-shape language model; Examples/paligemma.ipynb cells 11-13): per layer
 *   n = RMSNorm(x) ; q,k,v = n Wqkv^T (+b) with RoPE, k/v written into the cache at `pos` ;
 *   x = x + attn(q, K[0..pos], V[0..pos]) Wo^T ; n = RMSNorm(x) ; x = x + (gelu_tanh(n Wg^T) * n Wu^T) Wd^T
 * then the final RMSNorm and the (tied) vocabulary projection.  Same launches as the Python layer
 * (models/paligemma.py GemmaDecoderLayer), one C call per generated token instead of ~150.
 * -------------------------------------------------------------------------------------------- */
typedef struct vy_gemma_layer {
  const void* wqkv; const void* bqkv;      /* packed [q;k;v] projection, bias may be NULL */
  const void* wo; const void* bo;
  const void* ln_in; const void* ln_post;  /* RMSNorm weights (applied as 1 + w) */
  const void* wgu;                         /* packed [gate; up], [2*ffn, d] */
  const void* wdown;                       /* [d, ffn] */
  void* kcache; void* vcache;              /* (B, hk, cap, dh) */
  int64_t c_sb, c_sh, c_sl;
} vy_gemma_layer;
typedef struct vy_gemma_plan {
  int32_t num_layers, B, d, h, hk, dh, ffn, vocab, dtype;
  float eps;
  const float* cos_tab; const float* sin_tab;
  const vy_gemma_layer* layers;
  const void* norm_w; const void* head_w;  /* final RMSNorm, [vocab, d] projection */
  void* ws; int64_t ws_bytes;              /* >= vy_gemma_ws_bytes(...) */
  int32_t flags;                           /* VY_GEMMA_PRESCALED: every layer's wqkv / wgu is already multiplied by
                                              (1 + ln_in) / (1 + ln_post) along K (bf16, B <= 4): the step skips the
                                              RMSNorm launches and scales each product by rsqrt(mean x^2 + eps) */
} vy_gemma_plan;
#define VY_GEMMA_PRESCALED 1
int64_t vy_gemma_ws_bytes(int32_t B, int32_t d, int32_t h, int32_t dh, int32_t ffn, int32_t dtype);
/* x: (B, d) embeddings of the current token (already scaled by sqrt(d)); keys 0..pos are attended;
 * logits: (B, ldv). */
int vy_gemma_decoder_step(const vy_gemma_plan* plan, const void* x, int64_t pos, void* logits, int64_t ldv,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight-only fp8 for the single-sequence step (B = 1 is a weight stream: half the bytes per token).
 *
 * vy_quant_rows_fp8: w (N, K) bf16 or fp32, leading dimension ldw -> codes (N, K) OCP e4m3fn bytes, leading
 * dimension ldc, and one fp32 scale per row.  The rule of the fp8 KV pages, per output row:
 *   s = amax > 0 ? amax / 448 : 1 ;  code = e4m3fn(clamp(w / s, -448, 448))   IEEE fp32 division, nearest even
 * so that w ~ code * s with |code * s - w| <= max(2^-4 |w|, 2^-10 s).  K, ldc multiples of 4.  Once per plan.
 *
 * vy_gemma_decoder_step_w8: vy_gemma_decoder_step on a plan whose wqkv / wo / wgu / wdown point at such codes
 * (leading dimension K bytes); `w8` carries their row scales (s_gu: 2 ffn of them, gate rows then up rows) and a
 * quantised copy of the vocabulary matrix.  Biases, norm weights, caches, tables and workspace as in the bf16
 * plan; VY_GEMMA_PRESCALED as there (the codes then quantise the fp32 product W (1 + ln)).  Each product
 * accumulates code * x in fp32 and multiplies the sum by the row's scale once; everything after that is the bf16
 * step's arithmetic.  One chain only: bf16 activations, B = 1, d, h * dh and ffn each one of 2048 / 4096 / 8192 /
 * 16384, dh a power of two with the rotary tables given, vocab a multiple of 4.  Anything else returns
 * VY_ERR_UNSUPPORTED with a message before the first launch: no kernel that expects bf16 weights reads codes.
 * -------------------------------------------------------------------------------------------- */
int vy_quant_rows_fp8(const void* w, int64_t ldw, void* codes, int64_t ldc, float* scales, int64_t N, int64_t K,
                      int dtype, void* stream);
typedef struct vy_gemma_w8_layer { const float *s_qkv, *s_o, *s_gu, *s_down; } vy_gemma_w8_layer;
typedef struct vy_gemma_w8 {
  const vy_gemma_w8_layer* layers;
  const void* head_codes; const float* head_scale;   /* [vocab, d] codes, [vocab] scales */
} vy_gemma_w8;
int vy_gemma_decoder_step_w8(const vy_gemma_plan* plan, const vy_gemma_w8* w8, const void* x, int64_t pos,
                             void* logits, int64_t ldv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VYOM_HIP_H */
