/* chitu_hip.h -- C ABI of libchitu_hip.so: the MI355X (gfx950) decode hot path of
 * thu-pacman/chitu, re-written as hand-authored HIP kernels.
 *
 * Conventions (the contract a binding must follow):
 *   - every pointer is a DEVICE pointer unless stated; the caller owns and allocates all
 *     inputs, outputs and scratch (reference ownership rule: csrc/common.h:46-55,
 *     fused_moe.py:489-506).  Kernels never allocate and never synchronise.
 *   - `stream` is a hipStream_t; launches are enqueued on it and are hipGraph-capturable.
 *   - return value: 0 = enqueued; <0 = argument error (CHITU_ERR_*); >0 = hipError_t.
 *     Nothing here calls exit() (the reference's ASSERTWITH does, csrc/common.h:20-30).
 *   - tensors are dense row-major ("contiguous" in the reference's asserts) unless a
 *     stride argument is given.  fp8 = OCP e4m3fn bytes (torch.float8_e4m3fn), bf16 =
 *     raw uint16 bits.  `act_dtype`: 0 = bf16, 1 = f16, 2 = f32.
 */
#ifndef CHITU_HIP_H
#define CHITU_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_ABI_VERSION 13  /* 13: + chitu_hip_gqa_prefill_paged (the GQA / MHA flash prefill with its keys read through the block table: continued and chunked prefill over the paged bf16 K / V cache), additive only.  12: + chitu_hip_speculative_verify_sampled (verification against a draft that was itself sampled: accept with min(1, p / q), replace from max(p - q, 0), in 128-bit integers), additive only.  11: + chitu_hip_speculative_verify (draft verification of speculative decoding with sampling, next to chitu_hip_sample), additive only.  10: + chitu_hip_mla_decode_multi, chitu_hip_mla_decode_multi_kv_fp8 (q_len <= 8 query tokens per sequence on the MLA paged decode), additive only.  9: + chitu_hip_gqa_decode_multi, chitu_hip_gqa_decode_multi_kv_fp8 (q_len <= 8 query tokens per sequence on the GQA / MHA paged decode), additive only.  8: + chitu_hip_gqa_decode_window, chitu_hip_gqa_decode_kv_fp8_window, chitu_hip_gqa_prefill_window (sliding window and soft cap of the GQA / MHA decode and prefill), additive only.  7: + the five entries of the fp8 K / V cache of the GQA / MHA decode (chitu_hip_gqa_kv_quant_fp8 / _dequant_fp8 / _append_fp8, chitu_hip_gqa_qkv_post_kv_fp8, chitu_hip_gqa_decode_kv_fp8), additive only; chitu_hip_gqa_decode now also refuses q / cache bases that are not 16-byte aligned (it always loaded 16 bytes).  6: + the four entries of the fp8 latent KV cache (chitu_hip_mla_kv_quant_fp8 / _dequant_fp8 / _append_fp8, chitu_hip_mla_decode_kv_fp8), additive only.  5: + chitu_hip_moe_gemm1_silu_mxfp4_tiled / chitu_hip_moe_gemm2_mxfp4_tiled (prefill form of the MXFP4 experts), additive only.  4: + the five MXFP4 (W4A8) expert entries chitu_hip_*_mxfp4, additive only.  3 (round 6): + chitu_hip_mla_decode_merge_uv_quant_fp8 / _tickets_bytes; INTEGRATION.md lists what 2 -> 3 removed or tightened */

/* ---- fused MoE: token alignment -------------------------------------------------
 * Replaces chitu_backend.cuda_moe_align_block_size (reference csrc/binding.cpp:11,
 * csrc/moe_kernel.h:7-11, kernel csrc/moe_align_kernel.cu:27-120) and the Triton
 * 4-stage path chitu/fused_moe.py:314-442.  Stable (flat token order inside each expert
 * segment) => bit-identical to the Triton path.
 *   topk_ids            [numel] integers, ids_dtype: 0=u8 1=i8 2=i16 3=i32 4=i64
 *   sorted_token_ids    [sorted_cap]  (cap >= numel + E*(block-1)); padding = numel
 *   expert_ids          [expert_ids_cap] one expert per block of `block_size` slots
 *   num_tokens_post_pad [1]; cumsum [num_experts+1]
 *   fill_sentinels      0: caller pre-filled sorted=numel / expert_ids=0 as the reference
 *                          allocator does (fused_moe.py:493-502); 1: the kernel does it.
 * Limits: 1 <= num_experts <= 1024 (reference CUDA kernel: <= 256). */
int chitu_hip_moe_align_block_size(const void* topk_ids, int ids_dtype, int64_t numel,
                                   int32_t num_experts, int32_t block_size,
                                   int32_t* sorted_token_ids, int64_t sorted_cap,
                                   int32_t* expert_ids, int64_t expert_ids_cap,
                                   int32_t* num_tokens_post_pad, int32_t* cumsum,
                                   int32_t fill_sentinels, void* stream);
/* Same launch with the expert-parallel remap folded in: expert_map [num_experts] i32 on the device
 * (local expert id, or -1 for an expert held by another rank) is applied to EVERY entry of expert_ids,
 * exactly as `expert_ids = expert_map[expert_ids]` does after the sort (chitu/fused_moe.py:516-517):
 * blocks of expert e carry expert_map[e], the unused tail carries expert_map[0] (the allocator's zeros
 * mapped).  expert_map == NULL: identical to chitu_hip_moe_align_block_size. */
int chitu_hip_moe_align_block_size_mapped(const void* topk_ids, int ids_dtype, int64_t numel,
                                          int32_t num_experts, int32_t block_size,
                                          int32_t* sorted_token_ids, int64_t sorted_cap,
                                          int32_t* expert_ids, int64_t expert_ids_cap,
                                          int32_t* num_tokens_post_pad, int32_t* cumsum,
                                          int32_t fill_sentinels, const int32_t* expert_map,
                                          void* stream);

/* ---- FP8 activation quantisation ---------------------------------------------------
 * mode 0 replaces act_quant_deepseek_v3 (chitu/ops.py:330-353, kernel
 *        chitu/triton_kernels.py:193-214): s = max|x|/448, y = x/s, no eps, no clamp.
 * mode 1 replaces per_token_group_quant_fp8 (chitu/fused_moe.py:713-793, kernel :670-710):
 *        s = max(max|x|, eps)/448, y = clamp(x/s, +-448).
 *   x [rows, cols] act_dtype; y_fp8 [rows, cols] e4m3fn; scales [rows, cols/group] f32.
 * group_size must be 128 and divide cols (the reference asserts this, ops.py:345-348). */
int chitu_hip_act_quant_fp8(const void* x, int act_dtype, int64_t rows, int64_t cols,
                            int32_t group_size, int32_t mode, float eps, void* y_fp8,
                            float* scales, void* stream);

/* ---- FP8 weight de-quantisation -------------------------------------------------------
 * Replaces weight_dequant_deepseek_v3 (chitu/ops.py:357-392, kernel triton_kernels.py:217-247)
 * when soft = 0, and weight_dequant_soft_fp8_deepseek_v3 (chitu/ops.py:396-449, kernels
 * triton_kernels.py:250-287: bit placement * (s * 2^120)) when soft = 1.
 *   w_fp8 [batch, rows, cols]; scales [batch, ceil(rows/128), ceil(cols/128)] f32;
 *   y [batch, rows, cols] of out_dtype (0 bf16, 1 f16, 2 f32). */
int chitu_hip_weight_dequant_fp8(const void* w_fp8, const float* scales, int64_t batch,
                                 int64_t rows, int64_t cols, int32_t block_size, int32_t soft,
                                 int out_dtype, void* y, void* stream);

/* ---- FP8 x FP8 block-scaled GEMM (W8A8) --------------------------------------------------
 * Replaces fp8_gemm_deepseek_v3 (chitu/ops.py:453-483, kernel triton_kernels.py:302-365):
 *   out[m][n] = sum_kb dot(a[m, kb], b[n, kb]) * a_scale[m, kb] * b_scale[n/128, kb]
 *   a_fp8 [M, K]; a_scale [M, K/128] f32; b_fp8 [N, K]; b_scale [ceil(N/128), K/128] f32;
 *   out [M, N] of out_dtype.  K % 128 == 0.  Built for decode (M <= 64 per weight pass).
 * workspace: optional device scratch for cross-workgroup split-K partials
 * (needs 8 * M * N * 4 bytes at most); NULL/too small => no cross-workgroup split. */
int chitu_hip_fp8_gemm_blockscale(const void* a_fp8, const float* a_scale, const void* b_fp8,
                                  const float* b_scale, void* out, int out_dtype, int64_t M,
                                  int64_t N, int64_t K, void* workspace,
                                  int64_t workspace_bytes, void* stream);
/* The same GEMM on TILE-MAJOR activations, the layout the fused decode step keeps its fp8 activations in between two of
 * its own launches (never across the drop-in op surface, which stays row-major like the reference's):
 *   a_fp8   [ceil(M/16)][K/16][16 rows][16 B]   -- the 16 tokens of a tile side by side for every 16-byte k chunk
 *   a_scale [ceil(M/16)][K/128][16 rows] f32
 * so that a 16-lane group of the MFMA B-operand load (one k chunk, 16 tokens) reads 256 contiguous bytes instead of 16 B
 * from each of 16 rows, and a block's 16 scales one 64-B segment (the activation loads were 2.9 of the 9.9 us of the wqkv_a
 * launch at bs 16).  Written by chitu_hip_rmsnorm / chitu_hip_comm_allreduce_rmsnorm with quant_mode + 4 and by
 * chitu_hip_mla_merge_absorb_uv_quant_fp8_tm.  M < 128; same arithmetic, bit-identical output. */
int chitu_hip_fp8_gemm_blockscale_tm(const void* a_fp8, const float* a_scale, const void* b_fp8,
                                     const float* b_scale, void* out, int out_dtype, int64_t M,
                                     int64_t N, int64_t K, void* workspace,
                                     int64_t workspace_bytes, void* stream);
/* The same contraction with the K range cut over num_splits (2..16) workgroups per output tile and the fp32 partial
 * planes as the OUTPUT: partials [num_splits, M, N], plane s = the contribution of its K blocks, no reduce launch.
 * For the dense GEMMs whose N cannot fill 256 CUs on its own (wqkv_a: 2112 rows = 132 tiles); the consumer sums
 * the planes in plane order (chitu_hip_mla_qkv_post with num_partials). */
int chitu_hip_fp8_gemm_blockscale_partials(const void* a_fp8, const float* a_scale, const void* b_fp8,
                                           const float* b_scale, float* partials, int64_t M, int64_t N,
                                           int64_t K, int32_t num_splits, void* stream);

/* ---- FP8-weight x bf16-activation GEMM ("soft fp8") ------------------------------------
 * Replaces soft_fp8_gemm_deepseek_v3 (chitu/ops.py:487-511, kernel triton_kernels.py:388-508):
 * weights decoded to bf16 as bits((b&0x80)<<24 | (b&0x7f)<<20) * (b_scale * 2^120), bf16 dot,
 * fp32 accumulate.  a_bf16 [M, K]; b_fp8 [N, K]; b_scale [ceil(N/128), K/128]; out [M, N]. */
int chitu_hip_soft_fp8_gemm(const void* a_bf16, const void* b_fp8, const float* b_scale,
                            void* out, int out_dtype, int64_t M, int64_t N, int64_t K,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* ---- paged KV append ----------------------------------------------------------------------
 * Replaces append_to_paged_kv_cache (chitu/ops.py:51-91, kernel triton_kernels.py:18-48):
 *   cache[page_table[b][L_b / page_size]][L_b % page_size] = this_kv[b],  L_b = old_seq_lens[b]
 *   kv_cache [num_pages, page_size, row_bytes] bytes; page_table [batch, pages_per_seq] i32;
 *   this_kv [batch, row_bytes]; old_seq_lens [batch] i32.  Out-of-table positions are dropped. */
int chitu_hip_append_paged_kv(void* kv_cache, int64_t num_pages, int32_t page_size,
                              int64_t row_bytes, const int32_t* page_table,
                              int32_t pages_per_seq, const void* this_kv,
                              const int32_t* old_seq_lens, int32_t batch, void* stream);

/* ---- rotary embedding ---------------------------------------------------------------------
 * Replaces apply_rotary_pos_emb (chitu/ops.py:311-326; kernels triton_kernels.py:51-190; torch
 * form ops.py:243-272).  layout 0 = "llama" interleaved (re, im) pairs, 1 = "hf-llama" halves.
 *   q [batch, q_heads, head_dim], k [batch, k_heads, head_dim] (element strides given),
 *   cos/sin [batch, head_dim/2] f32; fp32 math, one rounding to act_dtype. */
int chitu_hip_rope(const void* q, const void* k, void* out_q, void* out_k, const float* cos,
                   const float* sin, int act_dtype, int32_t batch, int32_t q_heads,
                   int32_t k_heads, int32_t head_dim, int64_t q_sb, int64_t q_sh, int64_t k_sb,
                   int64_t k_sh, int64_t oq_sb, int64_t oq_sh, int64_t ok_sb, int64_t ok_sh,
                   int32_t layout, void* stream);

/* ---- fused MoE, fp8 W8A8 with 128x128 block scales (decode) -------------------------------
 * Together these replace fused_experts_impl (chitu/fused_moe.py:1130-1307): the two
 * invoke_fused_moe_kernel calls (:796-891, Triton kernel :62-307), SiluAndMul (:24-39), the
 * activation re-quantisation (:829 -> :713-793) and moe_sum (:1299-1305).  All take the outputs
 * of chitu_hip_moe_align_block_size run with block_size = 16 (one MFMA tile of sorted slots).
 *   sorted_token_ids / expert_ids / num_tokens_post_pad: from moe_align (block 16); expert -1
 *   (expert_map, not on this rank) writes zeros like write_zeros_to_output (:40-59).
 *   max_mblocks: grid bound, min(len(expert_ids), numel) is always enough.
 *
 * gemm1:  c1[slot, :] = bf16( sum_kb dot(a[slot/topk, kb], w1[e, :, kb]) * a_s * w1_s )
 *   a_fp8 [tokens, K], a_scale [tokens, K/128]; w1 [E, N, K] fp8, w1_scale [E, ceil(N/128), K/128];
 *   out_bf16 [numel, N] with numel = tokens*topk (row = flat slot id t*topk+k).
 * silu_mul_quant:  h = bf16(bf16(silu(c1[:, :I])) * c1[:, I:]); per-128 group
 *   s = max(max|h|, eps)/448, q = clamp(h/s) -> e4m3 (quant_mode 1, the MoE rule) or s = max|h|/448,
 *   q = h/s (quant_mode 0, act_quant_deepseek_v3: dense / shared-expert MLP, model_deepseek_v3.py:936-949).
 *   c1 [rows, 2I]; q [rows, I]; scales [rows, I/128].
 * gemm2:  c3[slot, :] = bf16( (sum_kb dot(h[slot, kb], w2[e, :, kb]) * h_s * w2_s) * topk_w[slot] )
 *   h_fp8 [numel, I]; w2 [E, N, I]; out [numel, N]; topk_weights [numel] of weights_dtype.
 * moe_sum: out[t, :] = bf16( sum_k float(c3[t, k, :]) ).
 */
int chitu_hip_moe_gemm1_fp8(const void* a_fp8, const float* a_scale, const void* w1_fp8,
                            const float* w1_scale, const int32_t* sorted_token_ids,
                            const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                            void* out_bf16, int64_t numel, int32_t topk, int64_t N, int64_t K,
                            int64_t max_mblocks, void* stream);
int chitu_hip_moe_silu_mul_quant_fp8(const void* c1_bf16, int64_t rows, int64_t inter_size,
                                     int32_t quant_mode, float eps, void* q_fp8, float* scales,
                                     void* stream);
int chitu_hip_moe_gemm2_fp8(const void* h_fp8, const float* h_scale, const void* w2_fp8,
                            const float* w2_scale, const int32_t* sorted_token_ids,
                            const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                            const void* topk_weights, int weights_dtype,
                            int32_t mul_routed_weight, void* out_bf16, int64_t numel, int64_t N,
                            int64_t inter_size, int64_t max_mblocks, void* stream);
/* Two-launch form of gemm1 -> silu_mul_quant -> gemm2 (same arithmetic and rounding points):
 * gemm1_silu: a wave owns the gate tile and the up tile of the same 16 columns of W1 [E, 2I, K] and
 *   writes h[slot, :] = bf16(bf16(silu(bf16(gate))) * bf16(up)) as bf16 [numel, I]; inter_size % 16 == 0.
 * gemm2_quant: per_token_group_quant_fp8 (eps rule, 128-wide groups) of h in the prologue, then gemm2.
 *   inter_size % 128 == 0 and <= 512 (CHITU_ERR_UNSUPPORTED otherwise: wider experts take the three-launch form). */
int chitu_hip_moe_gemm1_silu_fp8(const void* a_fp8, const float* a_scale, const void* w1_fp8,
                                 const float* w1_scale, const int32_t* sorted_token_ids,
                                 const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                 void* h_bf16, int64_t numel, int32_t topk, int64_t inter_size, int64_t K,
                                 int64_t max_mblocks, void* stream);

/* The same two grouped GEMMs tiled for PREFILL-sized batches (block_m = 64 or 128 sorted slots x 128 weight rows per workgroup
 * through LDS; fused_moe.py:62-307 runs BLOCK_SIZE_M = 64): sorted_token_ids / expert_ids / num_tokens_post_pad must come from
 * chitu_hip_moe_align_block_size with block_size = block_m (128: one block, i.e. one pass over its weights, for an expert with
 * up to 128 slots; all-padding 16-slot sub-tiles are skipped); max_mblocks <= 65535.  Same outputs for either block_m.
 *   gemm1_silu_tiled: h[slot, :] = bf16(bf16(silu(bf16(gate))) * bf16(up)) as bf16 [numel, I]; I % 128 == 0, K % 128 == 0.
 *   gemm2_tiled: out[slot, :] = bf16((h_fp8[slot] . W2[e]^T, block-scaled) * routed_weight[slot]); h quantised by the
 *   caller (chitu_hip_act_quant_fp8 mode 1); I % 128 == 0, N % 8 == 0.
 * Same rounding points as the decode kernels; the order of the sum inside a 128-block differs (<= 1e-5 of the result). */
int chitu_hip_moe_gemm1_silu_fp8_tiled(const void* a_fp8, const float* a_scale, const void* w1_fp8,
                                       const float* w1_scale, const int32_t* sorted_token_ids,
                                       const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                       void* h_bf16, int64_t numel, int32_t topk, int64_t inter_size, int64_t K,
                                       int64_t max_mblocks, int32_t block_m, void* stream);
int chitu_hip_moe_gemm2_fp8_tiled(const void* h_fp8, const float* h_scale, const void* w2_fp8,
                                  const float* w2_scale, const int32_t* sorted_token_ids,
                                  const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                  const void* topk_weights, int weights_dtype, int32_t mul_routed_weight,
                                  void* out_bf16, int64_t numel, int64_t N, int64_t inter_size,
                                  int64_t max_mblocks, int32_t block_m, void* stream);
int chitu_hip_moe_gemm2_quant_fp8(const void* h_bf16, const void* w2_fp8, const float* w2_scale,
                                  const int32_t* sorted_token_ids, const int32_t* expert_ids,
                                  const int32_t* num_tokens_post_pad, const void* topk_weights,
                                  int weights_dtype, int32_t mul_routed_weight, void* out_bf16,
                                  int64_t numel, int64_t N, int64_t inter_size, int64_t max_mblocks,
                                  float eps, void* stream);
int chitu_hip_moe_sum(const void* c3_bf16, void* out_bf16, int64_t tokens, int32_t topk, int64_t N,
                      void* stream);

/* ---- fused MoE with MXFP4 expert weights, W4A8 (csrc/moe_mxfp4.hip) -----------------------------
 * OCP MX v1.0 weights: packed e2m1, two per byte (low nibble = even k), uint8 [E, rows, K/2], with one E8M0 scale byte per 32
 * consecutive k of a row, uint8 [E, rows, K/32] (value 2^(byte - 127); 0xFF = NaN).  Activations are e4m3 with per-128-group
 * fp32 scales exactly as in the fp8 entries above; the 128-wide block dot is one v_mfma_scale_f32_16x16x128_f8f6f4 with the
 * weights' own scale bytes as the hardware scale operand, its fp32 result is multiplied by the activation's group scale and
 * accumulated in fp32.  Everything else (padding slots, expert -1 = zeros, the num_tokens_post_pad early exit, rounding
 * points) is the fp8 entries'.  sorted_token_ids / expert_ids / num_tokens_post_pad: moe_align with block_size 16.
 * K % 128 == 0 and inter_size % 128 == 0, one expert's matrix below 2^31 bytes (CHITU_ERR_UNSUPPORTED otherwise).
 *   chitu_hip_moe_gemm1_silu_mxfp4  replaces chitu_hip_moe_gemm1_silu_fp8 for MXFP4 W1 [E, 2I, K/2].
 *   chitu_hip_moe_gemm2_quant_mxfp4 replaces chitu_hip_moe_gemm2_quant_fp8 for MXFP4 W2 [E, N, I/2]; inter_size <= 512.
 *   chitu_hip_moe_gemm_mxfp4        replaces chitu_hip_moe_gemm1_fp8 (a_div = topk, mul_routed_weight = 0) and
 *     chitu_hip_moe_gemm2_fp8 (a_div = 1) of the three-launch form: out[slot, :] = bf16((a[slot / a_div] . W[e]^T) * weight).
 *   chitu_hip_quant_mxfp4           new: no reference counterpart.  src_kind 0 / 1 / 2: bf16 / f16 / f32 [rows, cols]; 3: e4m3
 *     [rows, cols] times the fp32 scale of its [128, 128] block, block_scale [rows / rows_per_matrix,
 *     ceil(rows_per_matrix / 128), cols / 128].  Per 32-block: byte = clamp(exponent field of max|v| - 2, 0, 254), i.e. the OCP
 *     shared exponent floor(log2 max|v|) - 2 (an all-zero block gets byte 0); elements = round-to-nearest-even of
 *     v * 2^(127 - byte) onto {0, .5, 1, 1.5, 2, 3, 4, 6}, saturated at 6.  cols % 32 == 0 (kind 3: % 128).
 *   chitu_hip_dequant_mxfp4         new: no reference counterpart.  out bf16 [rows, cols] = e2m1 x 2^(byte - 127), exact for
 *     bytes 2..252 (outside that range the product may leave bf16's normal range: unspecified); 0xFF -> NaN. */
int chitu_hip_moe_gemm1_silu_mxfp4(const void* a_fp8, const float* a_scale, const void* w1_fp4,
                                   const void* w1_scale_e8m0, const int32_t* sorted_token_ids,
                                   const int32_t* expert_ids, const int32_t* num_tokens_post_pad, void* h_bf16,
                                   int64_t numel, int32_t topk, int64_t inter_size, int64_t K,
                                   int64_t max_mblocks, void* stream);
int chitu_hip_moe_gemm2_quant_mxfp4(const void* h_bf16, const void* w2_fp4, const void* w2_scale_e8m0,
                                    const int32_t* sorted_token_ids, const int32_t* expert_ids,
                                    const int32_t* num_tokens_post_pad, const void* topk_weights,
                                    int32_t weights_dtype, int32_t mul_routed_weight, void* out_bf16,
                                    int64_t numel, int64_t N, int64_t inter_size, int64_t max_mblocks, float eps,
                                    void* stream);
int chitu_hip_moe_gemm_mxfp4(const void* a_fp8, const float* a_scale, int32_t a_div, const void* w_fp4,
                             const void* w_scale_e8m0, const int32_t* sorted_token_ids, const int32_t* expert_ids,
                             const int32_t* num_tokens_post_pad, const void* topk_weights, int32_t weights_dtype,
                             int32_t mul_routed_weight, void* out_bf16, int64_t numel, int64_t N, int64_t K,
                             int64_t max_mblocks, void* stream);
int chitu_hip_quant_mxfp4(const void* src, int32_t src_kind, const float* block_scale, int64_t rows, int64_t cols,
                          int64_t rows_per_matrix, void* packed_fp4, void* scale_e8m0, void* stream);
int chitu_hip_dequant_mxfp4(const void* packed_fp4, const void* scale_e8m0, int64_t rows, int64_t cols,
                            void* out_bf16, void* stream);

/* ---- fused MoE with MXFP4 expert weights, PREFILL-sized batches (csrc/moe_mxfp4_tiled.hip) ---------
 * The two grouped GEMMs above tiled for compute: block_m (64 or 128) sorted slots x 128 weight rows per workgroup, both
 * operand tiles and the E8M0 bytes staged in LDS by LDS-DMA.  sorted_token_ids / expert_ids / num_tokens_post_pad: moe_align
 * with block_size = block_m; a block whose first slot is padding is skipped, expert -1 writes zeros, as in the fp8 tiled
 * entries, whose argument lists these share (weight and scale pointers exchanged for the MXFP4 pair).  Arithmetic: the block
 * dot and the ascending fmaf chain of the streaming entries, one chain per output (no K split): the same bits as
 * chitu_hip_moe_gemm1_silu_mxfp4 / chitu_hip_moe_gemm_mxfp4 launched without their K split.
 * K % 128 == 0, inter_size % 128 == 0, N % 8 == 0, block_m in {64, 128}, one expert's matrix and the activation matrix below
 * 2^31 bytes (CHITU_ERR_UNSUPPORTED otherwise); numel == 0 or max_mblocks == 0 is CHITU_OK with nothing launched.
 *   chitu_hip_moe_gemm1_silu_mxfp4_tiled  new: no reference counterpart; tiled form of chitu_hip_moe_gemm1_silu_mxfp4
 *     (h = bf16(bf16(silu(bf16(g))) * bf16(u)), bf16 [numel, I]), the MXFP4 counterpart of chitu_hip_moe_gemm1_silu_fp8_tiled.
 *   chitu_hip_moe_gemm2_mxfp4_tiled       new: no reference counterpart; tiled form of chitu_hip_moe_gemm_mxfp4 with
 *     a_div = 1 (out[slot, :] = bf16((h_fp8[slot] . W2[e]^T) * routed_weight[slot]); h quantised by the caller with
 *     chitu_hip_act_quant_fp8 mode 1), the MXFP4 counterpart of chitu_hip_moe_gemm2_fp8_tiled. */
int chitu_hip_moe_gemm1_silu_mxfp4_tiled(const void* a_fp8, const float* a_scale, const void* w1_fp4,
                                         const void* w1_scale_e8m0, const int32_t* sorted_token_ids,
                                         const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                         void* h_bf16, int64_t numel, int32_t topk, int64_t inter_size, int64_t K,
                                         int64_t max_mblocks, int32_t block_m, void* stream);
int chitu_hip_moe_gemm2_mxfp4_tiled(const void* h_fp8, const float* h_scale, const void* w2_fp4,
                                    const void* w2_scale_e8m0, const int32_t* sorted_token_ids,
                                    const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                    const void* topk_weights, int weights_dtype, int32_t mul_routed_weight,
                                    void* out_bf16, int64_t numel, int64_t N, int64_t inter_size,
                                    int64_t max_mblocks, int32_t block_m, void* stream);

/* ---- fused MoE with bf16 ACTIVATIONS: bf16 experts and soft-fp8 experts (csrc/moe_bf16.hip) --------
 * The two modes of fused_moe_kernel (chitu/fused_moe.py:62-307) that do not quantise the activations:
 *   weight_kind 0 -- bf16 weights, `accumulator += tl.dot(a, b)` (:298): fused_experts(use_fp8_w8a8=False), what the
 *     reference's MoEDeepSeekV3.forward runs for scale-less checkpoints (model_deepseek_v3.py:950-956) and, on every
 *     non-NVIDIA device, for soft-fp8 ones after weight_dequant_soft_fp8 (:975-993);
 *   weight_kind 1 -- fp8 e4m3fn weights + [128,128] block scales decoded to bf16 in registers,
 *     b = bf16(bits(((w & 0x80) << 24) | ((w & 0x7f) << 20)) * (scale * 2^120)) (:232-276): fused_experts(
 *     use_fp8_w8a8=True, soft_fp8=True), the NVIDIA branch (:968-974) -- same values as kind 0 on the dequantised weights.
 * One grouped GEMM over moe_align (block 16) output, fp32 accumulation over the whole K, one rounding to bf16:
 *   out[slot, :] = bf16( (a[slot / a_div, :] . w[e, :, :]^T) * (mul_routed_weight ? topk_weights[slot] : 1) )
 *   a bf16 [rows, K] (a_div = topk for the first GEMM, 1 for the second); w [E, Nw, K]; w_scale [E, ceil(Nw/128), K/128]
 *   (kind 1 only); out bf16 [numel, n_out]; expert -1 (expert_map: another rank's) writes zeros.
 *   silu = 1: Nw = 2*n_out (gate rows | up rows) and out = bf16(bf16(silu(bf16(g))) * bf16(u)) -- GEMM1 followed by
 *   SiluAndMul on bf16 tensors (fused_moe.py:24-39, :1262-1265) in one launch; silu = 0: Nw = n_out.
 *   K % 128 == 0; kind 1 with silu: n_out % 128 == 0.  Sum over the top-k with chitu_hip_moe_sum. */
int chitu_hip_moe_gemm_bf16(const void* a_bf16, int32_t a_div, const void* w, const float* w_scale,
                            int32_t weight_kind, const int32_t* sorted_token_ids, const int32_t* expert_ids,
                            const int32_t* num_tokens_post_pad, const void* topk_weights, int32_t weights_dtype,
                            int32_t mul_routed_weight, int32_t silu, void* out_bf16, int64_t numel, int64_t n_out,
                            int64_t K, int64_t max_mblocks, void* stream);

/* ---- GQA / MHA decode: RoPE(q in place, k) + paged append of k and v in one launch ----------------
 * Replaces apply_rotary_pos_emb (ops.py:311-326) + the two in-place appends of attn_with_kvcache
 * (attn_backend.py:108-115) in Attention.decode_forward_paged (models/model.py:167-198), same arithmetic.
 *   qkv [batch, q_heads + 2*kv_heads, head_dim] bf16 rows (row stride in elements): q heads rotated IN
 *   PLACE; k heads rotated into k_cache, v heads copied into v_cache [num_pages, page_size, kv_heads, head_dim]
 *   at row (page_table[b][L/page], L%page), L = old_seq_lens[b].  layout 0 = interleaved pairs, 1 = half-split. */
int chitu_hip_gqa_qkv_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                           int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                           void* k_cache, void* v_cache, int64_t num_pages, int32_t page_size,
                           const int32_t* page_table, int32_t pages_per_seq, const int32_t* old_seq_lens,
                           int32_t batch, void* stream);

/* Gate/up projection of an unquantised SwiGLU MLP with SiluAndMul in the epilogue (FeedForward,
 * models/model.py:212-214): out[m, n] = bf16( bf16(silu(bf16(x[m] . w13[n]))) * bf16(x[m] . w13[inter + n]) ),
 * x [M, K] bf16, w13 [2*inter, K] bf16 (w1 rows then w3 rows), out [M, inter] bf16; K % 64 == 0. */
int chitu_hip_bf16_gemm_silu(const void* x_bf16, const void* w13_bf16, void* out_bf16, int64_t M, int64_t inter,
                             int64_t K, void* stream);

/* ---- [top-k sum +] residual add + RMSNorm + act_quant as the prologue of the W8A8 GEMM that consumes it (batch 1-2) ----
 * TransformerBlockDeepSeekV3.forward (model_deepseek_v3.py:1107-1113): x = x + ffn(...); attn(attn_norm(x)) with the first
 * linear of the attention (wqkv_a; linear_deepseek_v3 :98-100 = act_quant_deepseek_v3 + fp8_gemm_deepseek_v3) in ONE launch:
 *   a[m]       = add_terms == 1 ? add[m] : bf16(sum_k float(add[m, k, :]))   (the experts' top-k sum, fused_moe.py:1299-1305)
 *   sum_out[m] = bf16(x[m] + a[m])                                          (the new residual stream; must not overlap x or add)
 *   y[m]       = bf16((sum_out[m] * rsqrt(mean(sum_out[m]^2) + eps)) * norm_weight);  (q, s) = act_quant(y, 128)
 *   out        = fp8_gemm(q, s, w_fp8, w_scale)                              [M, N], out_dtype as chitu_hip_fp8_gemm_blockscale
 * Bit-identical to chitu_hip_rmsnorm(add, add_terms, quant_mode = 1) followed by chitu_hip_fp8_gemm_blockscale (same
 * summation orders, same K split).  M == 1 (any add_terms <= 16) or M == 2 with add_terms == 1; K % 128 == 0, K <= 8192; a
 * shape whose GEMM runs as one workgroup per 16 output rows with 4 or 8 waves of K split (wqkv_a of R1 / V2-Lite, w1w3 of a
 * dense layer); anything else: CHITU_ERR_UNSUPPORTED (use the two launches).  add row / term strides in elements. */
int chitu_hip_fp8_gemm_add_norm(const void* x_bf16, int64_t x_row_stride, const void* add_bf16, int64_t add_row_stride,
                                int32_t add_terms, int64_t add_term_stride, void* sum_out_bf16, int64_t sum_row_stride,
                                const void* norm_weight_bf16, float eps, const void* w_fp8, const float* w_scale, void* out,
                                int32_t out_dtype, int64_t M, int64_t N, int64_t K, void* stream);

/* ---- residual add + RMSNorm as the prologue of the bf16 GEMM that consumes it (decode batches of 1-4 rows) -------
 * TransformerBlock (models/model.py:246-251): h = x + attention(attention_norm(x)); out = h + ffn(ffn_norm(h)) --
 * the add and the norm (RMSNorm.forward, models/model.py:29-78) in front of a layer's qkv projection and of its
 * gate/up projection, folded into those launches:
 *   sum_out[m] = bf16(x[m] + add[m])                       (the new residual stream; must NOT overlap x or add, taken
 *                                                           from their first to their last row, gaps included: every
 *                                                           workgroup of the GEMM re-reads both while workgroup 0 writes
 *                                                           sum_out -- an overlapping sum_out is CHITU_ERR_BAD_ARG)
 *   y[m]       = bf16((sum_out[m] * rsqrt(mean(sum_out[m]^2) + eps)) * norm_weight)
 *   out        = y . w^T                                   (chitu_hip_bf16_gemm_add_norm)
 *   out        = silu(y . w1^T) * (y . w3^T)               (chitu_hip_bf16_gemm_silu_add_norm, w13 = [w1; w3])
 * Bit-identical to chitu_hip_rmsnorm(add = ...) followed by chitu_hip_bf16_gemm / chitu_hip_bf16_gemm_silu (same
 * summation orders).  M <= 4, K % 64 == 0, 512 <= K <= 8192, M * K <= 24576 and at least 4 waves of K split for the
 * shape; anything else: CHITU_ERR_UNSUPPORTED (use the two launches).  Row strides in elements, multiples of 8. */
/* (round 6) add_terms 1 | 2, add_term_stride (elements): with two terms the residual is bf16(float(add[r]) + float(add[r] + stride)) --
 * chitu_hip_moe_sum's arithmetic for a top-2 MoE whose un-summed outputs [M, 2, K] are handed over (fused_experts(reduce_topk=False)). */
int chitu_hip_bf16_gemm_add_norm(const void* x_bf16, int64_t x_row_stride, const void* add_bf16,
                                 int64_t add_row_stride, int32_t add_terms, int64_t add_term_stride,
                                 void* sum_out_bf16, int64_t sum_row_stride,
                                 const void* norm_weight_bf16, float eps, const void* w_bf16, void* out,
                                 int32_t out_dtype, int64_t M, int64_t N, int64_t K, void* stream);
/* chitu_hip_bf16_gemm_add_norm for the merged q|k|v projection of a GQA / MHA layer with chitu_hip_gqa_qkv_post
 * (layout 0: interleaved rotary pairs) applied in the epilogue: qkv_out [M, (q_heads + 2*kv_heads) * head_dim] receives
 * the ROTATED q heads only; the rotated k heads and the v heads go straight into the token's page rows of k_cache /
 * v_cache (Attention.decode_forward_paged, models/model.py:167-198).  Bit-identical to the three separate launches.
 * head_dim % 16 == 0; other limits as chitu_hip_bf16_gemm_add_norm. */
int chitu_hip_bf16_gemm_add_norm_qkv_post(const void* x_bf16, int64_t x_row_stride, const void* add_bf16,
                                          int64_t add_row_stride, void* sum_out_bf16, int64_t sum_row_stride,
                                          const void* norm_weight_bf16, float eps, const void* wqkv_bf16,
                                          void* qkv_out_bf16, int64_t M, int64_t K, int32_t q_heads, int32_t kv_heads,
                                          int32_t head_dim, const float* cos, const float* sin, void* k_cache,
                                          void* v_cache, int64_t num_pages, int32_t page_size,
                                          const int32_t* page_table, int32_t pages_per_seq,
                                          const int32_t* old_seq_lens, void* stream);
int chitu_hip_bf16_gemm_silu_add_norm(const void* x_bf16, int64_t x_row_stride, const void* add_bf16,
                                      int64_t add_row_stride, void* sum_out_bf16, int64_t sum_row_stride,
                                      const void* norm_weight_bf16, float eps, const void* w13_bf16,
                                      void* out_bf16, int64_t M, int64_t inter, int64_t K, void* stream);

/* ---- SiluAndMul (unquantised MLPs: Llama FeedForward, models/model.py:212-214; fused_moe.py:24-39)
 *   out[r, :] = bf16( bf16(silu(x[r, :d])) * x[r, d:2d] ),  x [rows, 2d] bf16, out [rows, d] bf16, d % 8 == 0. */
int chitu_hip_silu_and_mul(const void* x_bf16, void* out_bf16, int64_t rows, int64_t d, void* stream);

/* ---- decode-step prologue: embedding lookup + rotary-row gather in one launch -----------------------
 * Replaces VocabParallelEmbedding.forward's mask / lookup / zero-fill (chitu/tensor_parallel.py:199-208; the
 * all-reduce that follows stays the caller's) and prepare_freqs_cis_decode's gather of the rotary row of every
 * sequence's current position (chitu/models/model.py:429-448):
 *   h[b, :] = vocab_start <= tokens[b] < vocab_start + vocab_local ? embed[tokens[b] - vocab_start, :] : 0
 *   cos_out[b, :] = cos_table[positions[b], :], sin_out likewise ([table_rows, half] f32; skipped when cos_out NULL)
 *   tokens [batch] i64, embed [vocab_local, dim] bf16 (dim % 8 == 0), h [batch, dim] bf16, positions [batch] i32. */
int chitu_hip_embed_rope_gather(const int64_t* tokens, const void* embed_bf16, int64_t vocab_start,
                                int64_t vocab_local, int32_t dim, void* h_bf16, const int32_t* positions,
                                const float* cos_table, const float* sin_table, int64_t table_rows,
                                int32_t half, float* cos_out, float* sin_out, int32_t batch, void* stream);

/* ---- launch-variant override (tests, tuning sweeps) -------------------------------------------------
 * Several ops choose between launch variants of IDENTICAL results (K-split width, ring depth, key-based vs
 * generic routing kernel, candidate vs radix sampler ...) by a shape heuristic.  This entry forces one, so the
 * equivalence tests can run every variant and a sweep can time them; value -1 restores the heuristic.  Process-wide,
 * not thread-safe, never needed in production.  option: 0 MoE GEMM1 K-split waves, 1 GEMM1 tiles per workgroup,
 * 2 GEMM1 ring depth, 3 GEMM2 config (NT*10 + ROUNDS), 4 int8 MoE K-split waves, 5 generic routing kernel (1),
 * 6 ticket-based route + align (1), 7 radix-only sampler (1), 8 dense fp8 GEMM K-split waves, 9 its whole-K-in-flight
 * form for <= 8 blocks per wave (0 = off), 10 / 11 the same two for the bf16 GEMM, 12 K-split waves of the bf16 SwiGLU GEMM,
 * 13 the tiled (compute-shaped) form of the dense fp8 GEMM for M >= 128 (0 = keep streaming the weights per 64 rows),
 * 14 the same for the bf16 GEMM (0 = per 32 rows), 15 the in-routing sort of the one-workgroup route + align launch (0 = the
 * general sort after the routing barrier), 16 the token-tile height of the tiled fp8 GEMM (64 | 128; heuristic: 64 for small grids). */
int chitu_hip_debug_option(int32_t option, int32_t value);

/* ---- arithmetic self-test ----------------------------------------------------------------------
 * The quantising kernels divide a group's values by its scale with a refined-reciprocal +
 * residual-correction sequence instead of the IEEE division expansion, and round to bf16 with
 * v_cvt_pk_bf16_f32 instead of integer arithmetic.  This entry checks both on the device, element
 * by element, against the slow definitions: mismatches[0] += #(fast quotient != num/den bitwise),
 * [1] += #(their e4m3 encodings differ), [2] += #(hardware bf16 != software RNE), over the pairs
 * whose divisor is in the fast path's range [2^-60, 2^60] (callers keep |num/den| and |num| * 2^-24
 * inside the normal range, as the kernels' |x| <= 448 * scale does).  mismatches: 3 x u64, caller-zeroed. */
int chitu_hip_selftest_arith(const float* num, const float* den, int64_t n, uint64_t* mismatches,
                             void* stream);

/* Host-only (no launch): the XCD-blocked tile order of the prefill-shaped dense GEMM (csrc/gemm_common.h::xcd_tile_of:
 * workgroup b runs on XCD b % 8, so each XCD is given one rectangle of a tiles_m x tiles_n grid).  *grid_out = workgroups
 * launched (8 * Mt * Nt); tile_of_wg (may be NULL; capacity >= *grid_out pairs) receives (tile_m, tile_n) per workgroup,
 * (-1, -1) for padding workgroups.  Exists so that the map can be tested without a GPU. */
int chitu_hip_selftest_xcd_tile_order(int32_t tiles_m, int32_t tiles_n, int32_t* grid_out, int32_t* tile_of_wg,
                                      int64_t capacity);

/* ---- fused MoE with INT8 W8A8 experts (BASELINE config 4: Mixtral-8x7B W8A8) ----------------------
 * The reference has no int8-W8A8 fused path (Mixtral loops over experts, model_hf_mixtral.py:76-94, each
 * linear a W8A8Linear after simple_w8a8, quantize/w8a8.py:38-164); these run the same per-expert arithmetic
 * grouped over moe_align's sorted slots (block 16):
 *   gemm1_silu: a[slot, :] = bf16( bf16(silu(g)) * u ), g/u = bf16( (q_x[token] . w1[e, n | I+n]) * s_x[token] * s_w1[e, n | I+n] )
 *     a_int8 [tokens, K] + a_scale [tokens] (chitu_hip_quant_act_int8 of the hidden states); w1 [E, 2I, K] int8,
 *     w1_scale [E, 2I] f32; h_bf16 [numel, I].
 *   gemm2: out[slot, :] = bf16( bf16( (q_a[slot] . w2[e, n]) * s_a[slot] * s_w2[e, n] ) * topk_weights[slot] )
 *     a_int8 [numel, I] + a_scale [numel] (chitu_hip_quant_act_int8 of a); w2 [E, N, I] int8, w2_scale [E, N].
 *   Sum over the top-k with chitu_hip_moe_sum.  K % 128 == 0, I % 128 == 0; int32 accumulation is exact. */
int chitu_hip_moe_i8_gemm1_silu(const void* a_int8, const float* a_scale, const void* w1_int8,
                                const float* w1_scale, const int32_t* sorted_token_ids,
                                const int32_t* expert_ids, const int32_t* num_tokens_post_pad, void* h_bf16,
                                int64_t numel, int32_t topk, int64_t inter_size, int64_t K, int64_t max_mblocks,
                                void* stream);
int chitu_hip_moe_i8_gemm2(const void* a_int8, const float* a_scale, const void* w2_int8, const float* w2_scale,
                           const int32_t* sorted_token_ids, const int32_t* expert_ids,
                           const int32_t* num_tokens_post_pad, const void* topk_weights, int weights_dtype,
                           int32_t mul_routed_weight, void* out_bf16, int64_t numel, int64_t N,
                           int64_t inter_size, int64_t max_mblocks, void* stream);

/* ---- MLA absorb-mode paged decode attention ------------------------------------------------
 * Replaces mla_decode (chitu/triton_decode_attention.py:259-290: _mla_attn_kernel :20-130 +
 * _mla_softmax_reducev_kernel :185-232) as called from TritonAttnBackend.mla_attn_with_kvcache
 * (chitu/attn_backend.py:707-774), and the third-party flash_mla / flashinfer MLA calls
 * (attn_backend.py:561-571, 678-684):
 *   out[b,h,:] = softmax_t(scale * (q_nope[b,h,:].c[t,:C] + q_pe[b,h,:].c[t,C:])) . c[t,:C]
 *   q_nope [batch, heads, C=512] bf16 (element strides given, multiples of 8); q_pe [batch, heads, R=64];
 *   kv_cache [num_pages, page_size, C+R] bf16 (one layer), page_size % 64 == 0, base 16-byte aligned (the 64-key tiles
 *   go global -> LDS by LDS-DMA, 16 bytes per lane; the launch needs 152 KB of the CU's 160 KB of LDS);
 *   block_table [batch, table_stride] i32; seqlens [batch] i32 = tokens to attend (incl. the
 *   row appended this step -- append is chitu_hip_append_paged_kv); out [batch, heads, C] bf16.
 *   num_splits: KV splits per sequence (graph-static; any value >= 1 gives the same result up to
 *   fp32 rounding).  workspace: >= chitu_hip_mla_decode_workspace_bytes when num_splits > 1;
 *   it then holds part_o [batch, heads, num_splits, C] bf16 (each split's normalised output) followed by
 *   part_lse [batch, heads, num_splits] f32.  out_bf16 == NULL (num_splits > 1 only): skip the merge pass and leave the
 *   partials for chitu_hip_mla_merge_absorb_uv_quant_fp8. */
int chitu_hip_mla_decode_workspace_bytes(int32_t batch, int32_t heads, int32_t num_splits,
                                         int64_t* bytes);
int chitu_hip_mla_decode(const void* q_nope, int64_t qn_stride_b, int64_t qn_stride_h,
                         const void* q_pe, int64_t qp_stride_b, int64_t qp_stride_h,
                         const void* kv_cache, int64_t num_pages, int32_t page_size,
                         const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                         float softmax_scale, void* out_bf16, int32_t batch, int32_t heads,
                         int32_t kv_lora_rank, int32_t rope_dim, int32_t num_splits,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---- FP8 latent KV cache of the MLA paged decode (csrc/mla_kv_fp8.hip, csrc/mla_decode_kv_fp8.hip) --------
 * One cached token is 656 bytes: [0, 512) kv_norm(kv_c) as 512 OCP e4m3fn codes | [512, 528) four fp32 scales, one per 128
 * latent channels, each an exact power of two | [528, 656) rope(k_pe), 64 bf16, copied unchanged.  Per group: amax = max|x|,
 * e = the smallest integer with amax <= 448 * 2^e clamped to e >= -64 (amax == 0: -64), scale = 2^e, code = RNE_e4m3(x * 2^-e)
 * (never overflows); NaN / Inf inputs are unspecified.  code * scale is exactly representable in bf16: dequantisation is exact.
 * A layer's cache is uint8 [num_pages, page_size, 656], base 16-byte aligned.
 *   chitu_hip_mla_kv_quant_fp8    new: no reference counterpart.  src bf16 [rows, 576] with a row stride in elements (% 8,
 *     base 16-byte aligned) -> dst bytes [rows, 656] with a row stride in bytes (>= 656, % 16, base 16-byte aligned); bytes
 *     of a destination row beyond 656 are not written.
 *   chitu_hip_mla_kv_dequant_fp8  new: no reference counterpart.  The inverse: byte rows (stride as above) -> bf16 [rows, 576]
 *     contiguous.  Exact.
 *   chitu_hip_mla_kv_append_fp8   new: no reference counterpart.  Quantises row b of src bf16 [batch, 576] (row stride in
 *     elements) into position old_seq_lens[b] of sequence b's page: cache[table[b][L / page_size]][L % page_size].  Any
 *     page_size >= 1.  A table entry outside [0, num_pages), a negative length or a position beyond pages_per_seq writes nothing.
 *   chitu_hip_mla_decode_kv_fp8   new: no reference counterpart.  chitu_hip_mla_decode's argument list and contract with
 *     kv_cache reading 656-byte rows (page_size % 64 == 0; 159 KB of LDS).  q stays bf16; the latent is widened to bf16 in LDS
 *     (exact) and everything behind that is chitu_hip_mla_decode's arithmetic in its order: the output, and with num_splits > 1
 *     the workspace (same layout, same consumers), are bit-identical to chitu_hip_mla_decode on the dequantised cache. */
int chitu_hip_mla_kv_quant_fp8(const void* src_bf16, int64_t src_stride, void* dst_u8, int64_t dst_stride_bytes,
                               int64_t rows, void* stream);
int chitu_hip_mla_kv_dequant_fp8(const void* src_u8, int64_t src_stride_bytes, void* dst_bf16, int64_t rows,
                                 void* stream);
int chitu_hip_mla_kv_append_fp8(const void* src_bf16, int64_t src_stride, void* kv_cache_u8, int64_t num_pages,
                                int32_t page_size, const int32_t* block_table, int32_t pages_per_seq,
                                const int32_t* old_seq_lens, int32_t batch, void* stream);
int chitu_hip_mla_decode_kv_fp8(const void* q_nope, int64_t qn_stride_b, int64_t qn_stride_h,
                                const void* q_pe, int64_t qp_stride_b, int64_t qp_stride_h,
                                const void* kv_cache, int64_t num_pages, int32_t page_size,
                                const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                                float softmax_scale, void* out_bf16, int32_t batch, int32_t heads,
                                int32_t kv_lora_rank, int32_t rope_dim, int32_t num_splits,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Multi-token MLA paged decode (csrc/mla_decode_multi.hip, csrc/mla_decode_multi_kv_fp8.hip) ----------------------------
 * q_len = T in 1 .. 8 query tokens per sequence over the latent cache: the verify step of speculative decoding (DeepSeek-V3's
 * multi-token-prediction head exists for it; the reference's FlashMLA backend sizes its metadata by mtp_size,
 * chitu/attn_backend.py:523-527).  chitu_hip_mla_decode's argument list, contract, workspace layout and limits with
 * qn_stride_t / qp_stride_t after the batch strides and q_len after batch:
 *   q_nope [batch, T, heads, 512], q_pe [batch, T, heads, 64] bf16 (element strides, multiples of 8, 16-byte bases);
 *   seqlens[b] = L counts ALL keys of sequence b, the T rows appended this step included; block_table [batch, table_stride],
 *   one row per sequence; out [batch, T, heads, 512] bf16 contiguous.
 *   Query token t sits at position L - T + t and sees keys k <= L - T + t: query (b, t) is chitu_hip_mla_decode on a row of
 *   length L_t = L - T + t + 1 over the same table.  L_t <= 0 gives zero rows.
 *   One workgroup takes 16 heads x TWO query tokens x one KV split, so a sequence's pages are read ceil(T / 2) times, not T.
 *   workspace (num_splits > 1): chitu_hip_mla_decode_workspace_bytes(batch * T, heads, num_splits), the same layout with
 *   batch * T rows in (b, t) order -- chitu_hip_mla_merge_absorb_uv_quant_fp8[_tm] consumes it unchanged when called with
 *   batch * T; out_bf16 == NULL leaves the partials.
 *   q_len outside 1 .. 8: CHITU_ERR_BAD_ARG.
 *   Bit-identity: at q_len == 1 the output and the workspace are the bits of chitu_hip_mla_decode / _kv_fp8 at the same
 *   num_splits.  At num_splits == 1 every row (b, t) is the bits of chitu_hip_mla_decode on the expanded problem (batch * T
 *   rows, lengths L_t).  At num_splits > 1 the same holds, workspace included, where ceil(L_t / 64) is equal for all t of a
 *   sequence; where the tokens straddle a 64-key tile boundary the earlier tokens' split ranges are not those of their own
 *   single-token launch and the result is equal within the attention's rounding only.
 *   chitu_hip_mla_decode_multi          bf16 cache [num_pages, page_size, 576].
 *   chitu_hip_mla_decode_multi_kv_fp8   656-byte fp8 rows; bit-identical to the bf16 entry on the dequantised cache. */
int chitu_hip_mla_decode_multi(const void* q_nope, int64_t qn_stride_b, int64_t qn_stride_t, int64_t qn_stride_h,
                               const void* q_pe, int64_t qp_stride_b, int64_t qp_stride_t, int64_t qp_stride_h,
                               const void* kv_cache, int64_t num_pages, int32_t page_size,
                               const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                               float softmax_scale, void* out_bf16, int32_t batch, int32_t q_len, int32_t heads,
                               int32_t kv_lora_rank, int32_t rope_dim, int32_t num_splits,
                               void* workspace, int64_t workspace_bytes, void* stream);
int chitu_hip_mla_decode_multi_kv_fp8(const void* q_nope, int64_t qn_stride_b, int64_t qn_stride_t, int64_t qn_stride_h,
                                      const void* q_pe, int64_t qp_stride_b, int64_t qp_stride_t, int64_t qp_stride_h,
                                      const void* kv_cache, int64_t num_pages, int32_t page_size,
                                      const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                                      float softmax_scale, void* out_bf16, int32_t batch, int32_t q_len, int32_t heads,
                                      int32_t kv_lora_rank, int32_t rope_dim, int32_t num_splits,
                                      void* workspace, int64_t workspace_bytes, void* stream);

/* MLA absorb-mode causal prefill attention (MQA, head dims 576 / 512): the attn_varlen_func call of
 * AttentionDeepSeekV3.prefill_forward (chitu/models/model_deepseek_v3.py:589-599; chitu/attn_backend.py:39-90).
 *   out[t,h,:] = softmax over keys s <= t of the same sequence ( scale * q[t,h,:] . kv[s,:] ) . kv[s,:512]
 *   q [T, heads, 576] bf16 (token / head strides in elements, multiples of 8); kv [T, 576] bf16 (row stride);
 *   cu_seqlens [n_seq + 1] i32 (device); max_seqlen bounds the grid; out [T, heads, 512] bf16 contiguous.
 * Per query token the arithmetic and its order are chitu_hip_mla_decode's with num_splits = 1. */
int chitu_hip_mla_prefill(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* kv_bf16,
                          int64_t kv_stride_t, const int32_t* cu_seqlens, int32_t n_seq, int32_t max_seqlen,
                          float softmax_scale, void* out_bf16, int32_t heads, int32_t kv_lora_rank,
                          int32_t rope_dim, void* stream);
/* The same contract (attn_varlen_func for the absorb-mode MQA shape, model_deepseek_v3.py:589-599; attn_backend.py:39-90;
 * the reference runs it on third-party flash_attn) on the flash kernel: 8 query tokens x 16 heads = 128 Q rows per workgroup,
 * S^T = K Q^T with Q in registers, in-lane softmax with deferred rescale, O^T = V^T P^T accumulated in the AGPR file, 32-key
 * blocks by LDS-DMA into a 4-slot ring.  Equal to chitu_hip_mla_prefill within the attention bar (1e-2 of the peak), not bit for bit.
 * All three base pointers 16-byte aligned. */
int chitu_hip_mla_prefill_flash(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* kv_bf16,
                          int64_t kv_stride_t, const int32_t* cu_seqlens, int32_t n_seq, int32_t max_seqlen,
                          float softmax_scale, void* out_bf16, int32_t heads, int32_t kv_lora_rank,
                          int32_t rope_dim, void* stream);

/* Causal GQA / MHA prefill attention, head_dim 128: the attn_varlen_func call of Attention.prefill_forward
 * (chitu/models/model.py:104-132; chitu/attn_backend.py:39-90; the reference runs it on third-party flash_attn, :167-206).
 *   out[t,h,:] = softmax over keys s <= t of the same sequence ( scale * q[t,h,:] . k[s,h/G,:] ) . v[s,h/G,:],  G = q_heads / kv_heads
 *   q [T, q_heads, 128], k / v [T, kv_heads, 128] bf16 (token / head strides in elements, multiples of 8; 16-byte aligned
 *   bases); cu_seqlens [n_seq + 1] i32 (device); max_seqlen bounds the grid; out [T, q_heads, 128] bf16 contiguous.
 * G must be a power of two <= 32.  Flash form (csrc/gqa_prefill_flash.hip): KV read once per 128 / G query tokens. */
int chitu_hip_gqa_prefill(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_bf16,
                          int64_t k_stride_t, int64_t k_stride_h, const void* v_bf16, int64_t v_stride_t,
                          int64_t v_stride_h, const int32_t* cu_seqlens, int32_t n_seq, int32_t max_seqlen,
                          float softmax_scale, void* out_bf16, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                          void* stream);

/* chitu_hip_gqa_prefill_window: chitu_hip_gqa_prefill over a sliding window and / or with a soft cap -- window_size = (window_left, 0) and softcap of the same
 * attn_varlen_func call (chitu/attn_backend.py:39-90, the window rule :67-69; the arithmetic is RefAttnBackend._attention,
 * :294-392, which FlashAttnBackend forwards to flash_attn, :167-206).  The argument list above with two more before the stream:
 *   window_left = W >= 0: query position p (inside its own sequence) sees the keys p - W .. p; W = 0: only itself; -1: no window.
 *   softcap = c > 0: the score is c * tanh(softmax_scale * q.k / c), before the mask and the softmax; 0: off.
 * window_left < -1 or softcap < 0 (or NaN): CHITU_ERR_BAD_ARG.  (-1, 0) launches chitu_hip_gqa_prefill's own kernel.  A workgroup
 * starts at the 64-key tile that holds its lowest visible key, so the work per query token is bounded by W + 128 keys. */
int chitu_hip_gqa_prefill_window(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_bf16,
                                 int64_t k_stride_t, int64_t k_stride_h, const void* v_bf16, int64_t v_stride_t,
                                 int64_t v_stride_h, const int32_t* cu_seqlens, int32_t n_seq, int32_t max_seqlen,
                                 float softmax_scale, void* out_bf16, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                                 int32_t window_left, float softcap, void* stream);

/* chitu_hip_gqa_prefill_paged: chitu_hip_gqa_prefill_window with the keys read through a block table -- continued / chunked prefill over
 * the paged K / V cache.  The seqlen_q != seqlen_k, bottom-right aligned causal case of attn_varlen_func (chitu/attn_backend.py:39-90,
 * separate cu_seqlens_q / cu_seqlens_k) and of attn_with_kvcache at any seqlen_q (chitu/attn_backend.py:92-164); the reference forwards
 * both to flash_attn, the arithmetic is RefAttnBackend._attention, :294-392.
 *   q [T, q_heads, 128] bf16, ragged by cu_seqlens_q [n_seq + 1] i32 (strides and alignment as in chitu_hip_gqa_prefill);
 *   k_cache / v_cache [num_pages, page_size, kv_heads, 128] bf16, page_size % 16 == 0, block_table rows [table_stride] i32 per
 *   sequence as in chitu_hip_gqa_decode; seqlens_k[s] = L_s counts ALL keys of sequence s, the n_s = cu_seqlens_q[s + 1] -
 *   cu_seqlens_q[s] rows of this call included (appended before the call, as for chitu_hip_gqa_decode_multi); max_seqlen_q bounds the
 *   grid; out [T, q_heads, 128] bf16 contiguous.
 *   Query i of sequence s sits at position L_s - n_s + i and sees key k iff k <= L_s - n_s + i and, with window_left = W >= 0,
 *   k >= L_s - n_s + i - W.  A query at a negative position gives zeros.  softcap as in chitu_hip_gqa_prefill_window; (-1, 0.0)
 *   launch the kernel without the window / cap code.
 * Memory: rows at positions >= L_s and rows before a block's window are never read, whatever they hold, and neither is a table
 * entry of a page that holds no key in [lowest visible key, L_s) (tile rows outside repeat key L_s - 1 / the lowest visible key).
 * Without window and cap: with n_s = L_s the output is bit-identical to chitu_hip_gqa_prefill on the same rows laid out contiguously,
 * under any block table; with a prefix L_s - n_s that is a multiple of 128 it is bit-identical to rows [L_s - n_s, L_s) of
 * chitu_hip_gqa_prefill on the whole sequence (64-key tiles start at key 0, query blocks of 128 / G at the first new token).  Other
 * prefixes: within the attention bar (1e-2 of the peak) -- the wave-wide rescale vote sees other rows.
 * window_left < -1, softcap < 0 or NaN, strides not multiples of 8, bases not 16-byte aligned, table_stride < 1: CHITU_ERR_BAD_ARG;
 * head_dim != 128, G not a power of two <= 32, page_size % 16 != 0: CHITU_ERR_UNSUPPORTED; all before any launch.  One launch
 * (csrc/gqa_prefill_flash.hip, kPaged); the pages are read once per 128 / G query tokens. */
int chitu_hip_gqa_prefill_paged(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_cache,
                                const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                                const int32_t* block_table, int32_t table_stride, const int32_t* cu_seqlens_q,
                                const int32_t* seqlens_k, int32_t n_seq, int32_t max_seqlen_q, float softmax_scale,
                                void* out_bf16, int32_t q_heads, int32_t head_dim, int32_t window_left, float softcap,
                                void* stream);

/* chitu_hip_mla_decode (num_splits >= 2) AND the merge + W_UV projection + act_quant of the entry below in ONE launch:
 * AttentionDeepSeekV3.decode_forward's mla_attn_with_kvcache -> einsum("bshc,hdc->bshd") -> act_quant of wo's input
 * (chitu/models/model_deepseek_v3.py:672-699, chitu/attn_backend.py:707-774).  Every split workgroup publishes its partial
 * rows, counts itself on its (sequence, head block)'s word in `tickets`, waits for the other splits (bounded: 200 ms, then
 * the word tickets[bytes/4 - 1] is set and stays set) and finishes one head.  Outputs are bit-identical to chitu_hip_mla_decode(
 * out_bf16 = NULL) followed by chitu_hip_mla_merge_absorb_uv_quant_fp8[_tm] (tile_major = 1).
 *   tickets: chitu_hip_mla_decode_tickets_bytes() bytes of device memory, zero when first used and never written by anyone
 *   else (the kernel leaves it zero); launches that share it must not overlap.  batch * ceil(heads/16) <= 4096.
 *   Other arguments: as the two entries it replaces; workspace as chitu_hip_mla_decode_workspace_bytes. */
int chitu_hip_mla_decode_tickets_bytes(int64_t* bytes);
int chitu_hip_mla_decode_merge_uv_quant_fp8(const void* q_nope, int64_t qn_stride_b, int64_t qn_stride_h, const void* q_pe,
                                            int64_t qp_stride_b, int64_t qp_stride_h, const void* kv_cache,
                                            int64_t num_pages, int32_t page_size, const int32_t* block_table,
                                            int32_t table_stride, const int32_t* seqlens, float softmax_scale,
                                            int32_t batch, int32_t heads, int32_t kv_lora_rank, int32_t rope_dim,
                                            int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                            const void* w_fp8, int64_t w_stride_h, const float* scale,
                                            int64_t scale_offset, int64_t scale_stride_h, int64_t scale_stride_k,
                                            void* q_fp8, float* q_scales, int32_t tile_major, uint32_t* tickets,
                                            void* stream);

/* Split-KV merge + W_UV projection (model_deepseek_v3.py:697) + act_quant of wo's input in one
 * launch, for small batches (one workgroup per (head, token)): the same arithmetic and rounding
 * points as chitu_hip_mla_decode's merge pass followed by chitu_hip_absorb_uv_quant_fp8.
 * workspace: as left by chitu_hip_mla_decode(out_bf16 = NULL) with the same batch/heads/num_splits
 * (>= 2); weight/scale arguments as chitu_hip_absorb_uv_quant_fp8; K must be 512. */
/* ..._tm: the same launch writing q / scales TILE-MAJOR (see chitu_hip_fp8_gemm_blockscale_tm): q_fp8 holds
 * ceil(batch/16)*16 rows of heads*128 bytes, q_scales [ceil(batch/16), heads, 16]. */
int chitu_hip_mla_merge_absorb_uv_quant_fp8_tm(const void* workspace, int32_t num_splits,
                                               const void* w_fp8, int64_t w_stride_h, const float* scale,
                                               int64_t scale_offset, int64_t scale_stride_h,
                                               int64_t scale_stride_k, void* q_fp8, float* q_scales,
                                               int32_t batch, int32_t heads, int32_t K, void* stream);
int chitu_hip_mla_merge_absorb_uv_quant_fp8(const void* workspace, int32_t num_splits,
                                            const void* w_fp8, int64_t w_stride_h, const float* scale,
                                            int64_t scale_offset, int64_t scale_stride_h,
                                            int64_t scale_stride_k, void* q_fp8, float* q_scales,
                                            int32_t batch, int32_t heads, int32_t K, void* stream);

/* ---- RMSNorm (+ fused FP8 quantisation of its output) ----------------------------------------
 * Replaces RMSNorm.forward (chitu/models/model.py:29-78: F.rms_norm in fp32, one rounding) and,
 * when quant_mode != 0, also the act-quant launch of the fp8 linear that consumes it
 * (chitu/models/model_deepseek_v3.py:98-100).  quant_mode 1 = act_quant_deepseek_v3 rule,
 * 2 = per_token_group_quant_fp8 rule (eps = quant_eps); the codes are those of the bf16-rounded y.
 * quant_mode + 4 (5, 6; only with add_bf16): the same codes and scales written TILE-MAJOR for
 * chitu_hip_fp8_gemm_blockscale_tm -- q_fp8 ceil(rows/16)*16*dim bytes, q_scales ceil(rows/16)*(dim/128)*16 floats.
 *   add_bf16 (optional): residual branch folded in first, x <- bf16(x + add) -- the reference's
 *   `x = x + attn(...)` / `x = x + ffn(...)` (model_deepseek_v3.py:1107-1113); sum_out receives it.
 *   add_terms > 1 (<= 16): the residual of row r is first formed as bf16(sum_k float(add[r*add_row_stride +
 *   k*add_term_stride + :])) -- chitu_hip_moe_sum's arithmetic, i.e. the fused MoE's top-k sum
 *   (fused_moe.py:1299-1305) folded into the norm that consumes it; add_terms == 1: plain residual.
 *   x [rows, dim] bf16 (row stride given); weight [dim] bf16; y [rows, dim] bf16 or NULL;
 *   q_fp8 [rows, dim], q_scales [rows, dim/128] (dim % 128 == 0 when quantising); dim <= 8192.  * quant_mode 3 (round 6; residual-add form with one term, row-major): the per-token INT8 quantisation of the rounded y
 * instead (quant_act of the reference's W8A8Linear, chitu/quantize/w8a8.py:18-26: scale = max(|y|, 1e-5) / 127 over the row,
 * code = clamp(rint(y / scale), -128, 127)): q_fp8 then holds int8 codes [rows, dim], q_scales one fp32 per row.
 */
int chitu_hip_rmsnorm(const void* x_bf16, int64_t x_row_stride, const void* add_bf16,
                      int64_t add_row_stride, int32_t add_terms, int64_t add_term_stride,
                      void* sum_out_bf16, int64_t sum_row_stride,
                      const void* weight_bf16, void* y_bf16, int64_t y_row_stride, int64_t rows,
                      int32_t dim, float eps, void* q_fp8, float* q_scales, int32_t quant_mode,
                      float quant_eps, void* stream);

/* ---- MLA absorb projections with in-register FP8 dequant ---------------------------------------
 * Replaces weight_dequant(wkv_b) + einsum("shd,hdc->shc") / einsum("bshc,hdc->bshd")
 * (chitu/models/model_deepseek_v3.py:511-531, 697; kernel triton_kernels.py:217-247):
 *   out[b,h,n] = bf16( sum_k x[b,h,k] * bf16(float(w[h,n,k]) * scale[off + h*sh + (n/128)*sn + (k/128)*sk]) )
 *   x [batch, heads, K] bf16 (strides in elements, multiples of 8); w [heads, N, K] fp8 with head
 *   stride w_stride_h elements (so a row-slice of wkv_b can be passed in place); K % 64 == 0;
 *   out [batch, heads, N] bf16 (strides multiples of 4). */
int chitu_hip_absorb_bmm_fp8(const void* x_bf16, int64_t x_stride_b, int64_t x_stride_h,
                             const void* w_fp8, int64_t w_stride_h, const float* scale,
                             int64_t scale_offset, int64_t scale_stride_h, int64_t scale_stride_n, int64_t scale_stride_k,
                             void* out_bf16, int64_t out_stride_b, int64_t out_stride_h,
                             int32_t batch, int32_t heads, int32_t N, int32_t K, void* stream);

/* chitu_hip_absorb_bmm_fp8 plus, in the same launch, RoPE applied IN PLACE to q_pe [batch, heads, 64]
 * (interleaved pairs, cos/sin [batch, 32] f32; the q half of chitu_hip_mla_kv_prep, same arithmetic):
 * both consume wq_b's output, so they share one launch on the decode path. */
int chitu_hip_absorb_bmm_rope_fp8(const void* x_bf16, int64_t x_stride_b, int64_t x_stride_h,
                                  const void* w_fp8, int64_t w_stride_h, const float* scale,
                                  int64_t scale_offset, int64_t scale_stride_h, int64_t scale_stride_n,
                                  int64_t scale_stride_k, void* out_bf16, int64_t out_stride_b,
                                  int64_t out_stride_h, int32_t batch, int32_t heads, int32_t N, int32_t K,
                                  void* q_pe_bf16, int64_t q_pe_stride_b, int64_t q_pe_stride_h,
                                  const float* cos, const float* sin, int32_t rope_dim, void* stream);

/* chitu_hip_absorb_bmm_rope_fp8 plus, still in the same launch, the KV half of chitu_hip_mla_kv_prep: kv_norm(kv_c),
 * RoPE(k_pe) and the page append of every token's kv_in row [kv_c (512) | k_pe (64)] (row stride kv_row_stride
 * elements, a multiple of 8).  The decode path of models WITHOUT a q low-rank projection (DeepSeek-V2-Lite,
 * q_lora_rank == 0; the reference asserts q_lora_rank > 0, model_deepseek_v3.py:477): their q, kv_c and k_pe all come
 * out of one merged GEMM, so everything that consumes its output fits one launch.  N % 16 == 0, kv_lora_rank == 512,
 * rope_dim == 64 (CHITU_ERR_UNSUPPORTED otherwise).  Same arithmetic as the two separate entries, bit for bit. */
int chitu_hip_absorb_bmm_rope_kv_fp8(const void* x_bf16, int64_t x_stride_b, int64_t x_stride_h,
                                     const void* w_fp8, int64_t w_stride_h, const float* scale,
                                     int64_t scale_offset, int64_t scale_stride_h, int64_t scale_stride_n,
                                     int64_t scale_stride_k, void* out_bf16, int64_t out_stride_b,
                                     int64_t out_stride_h, int32_t batch, int32_t heads, int32_t N, int32_t K,
                                     void* q_pe_bf16, int64_t q_pe_stride_b, int64_t q_pe_stride_h,
                                     const float* cos, const float* sin, int32_t rope_dim, const void* kv_in_bf16,
                                     int64_t kv_row_stride, const void* kv_norm_weight_bf16, float eps,
                                     void* kv_cache, int64_t num_pages, int32_t page_size,
                                     const int32_t* page_table, int32_t pages_per_seq,
                                     const int32_t* old_seq_lens, int32_t kv_lora_rank, void* stream);

/* ---- skinny bf16 GEMM (router scores, LM head) ---------------------------------------------
 * Replaces the F.linear calls on bf16 weights on the decode path: gate scores
 * (chitu/models/model_deepseek_v3.py:820) and the LM head (tensor_parallel.py:93, model.py:468-475).
 *   out[m][n] = sum_k x[m][k] * w[n][k];  x [M, K] bf16, w [N, K] bf16, K % 64 == 0.
 *   num_splits == 1: out [M, N] of out_dtype is written.  num_splits > 1 (tiny N): K is split across
 *   workgroups and fp32 partials [num_splits, M, N] are written to `partials` for the consumer
 *   (chitu_hip_gate_route sums them in order); `out` is ignored. */
int chitu_hip_bf16_gemm(const void* x_bf16, const void* w_bf16, void* out, int out_dtype, int64_t M,
                        int64_t N, int64_t K, int32_t num_splits, float* partials, void* stream);

/* ---- fused MoE routing ------------------------------------------------------------------------
 * Replaces everything after the score GEMM in GateDeepSeekV3.forward
 * (chitu/models/model_deepseek_v3.py:821-842; ~16 torch launches): score function, bias, group-limited
 * top-k, weight gather / normalise / scale.  Ties go to the lower index (torch.topk: unspecified).
 *   logits: bf16 [tokens, E] when num_partials == 0, else fp32 [num_partials, tokens, E] summed here
 *   and rounded to bf16 like F.linear's output.  bias_bf16 [E] or NULL.  score_func 1 = sigmoid
 *   (bf16 pipeline, weights normalised), 0 = softmax (fp32 pipeline), 2 = softmax followed by renormalising the
 *   selected weights in fp32 (Mixtral's router, chitu/models/model_hf_mixtral.py:58-64).
 *   out_weights_bf16 / out_ids (int64) [tokens, out_stride]: slots 0..topk-1 sorted by descending
 *   selection score; if extra_expert_id >= 0, slots topk .. topk+extra_count-1 = (extra_expert_id + i,
 *   extra_weight) -- used to
 *   run the always-on shared expert (stacked last, model_deepseek_v3.py:883-919) through the same
 *   grouped GEMMs as the routed ones. */
int chitu_hip_gate_route(const void* logits, int32_t num_partials, int64_t tokens, int32_t num_experts,
                         const void* bias_bf16, int32_t n_groups, int32_t topk_groups, int32_t topk,
                         int32_t score_func, float route_scale, void* out_weights_bf16,
                         int64_t* out_ids, int32_t out_stride, int32_t extra_expert_id,
                         float extra_weight, int32_t extra_count, void* stream);
/* chitu_hip_gate_route and chitu_hip_moe_align_block_size_mapped in ONE launch (decode batches): the routing
 * workgroups (one per token) publish their ids and take a ticket; the last to arrive sorts the whole
 * [tokens * out_stride] id array (sentinels written by the kernel, fill_sentinels = 1 semantics).  Outputs
 * are those of the two separate launches, bit for bit.  align_num_experts covers every id that can appear
 * (routed + always-on slots), <= 1024; out_stride must equal topk + extra slots.  `ticket`: one
 * zero-initialised uint32 in device memory, reset by the kernel; launches sharing it must not overlap. */
int chitu_hip_gate_route_align(const void* logits, int32_t num_partials, int64_t tokens, int32_t num_experts,
                               const void* bias_bf16, int32_t n_groups, int32_t topk_groups, int32_t topk,
                               int32_t score_func, float route_scale, void* out_weights_bf16,
                               int64_t* out_ids, int32_t out_stride, int32_t extra_expert_id,
                               float extra_weight, int32_t extra_count, int32_t align_num_experts,
                               int32_t align_block_size, int32_t* sorted_token_ids, int64_t sorted_cap,
                               int32_t* expert_ids, int64_t expert_ids_cap, int32_t* num_tokens_post_pad,
                               int32_t* cumsum, const int32_t* expert_map, uint32_t* ticket, void* stream);

/* ---- MLA decode KV prep (kv_norm + RoPE + append, fused) ------------------------------------
 * Replaces four launches of AttentionDeepSeekV3.decode_forward_paged: apply_rotary_pos_emb on
 * (q_pe, k_pe) (chitu/models/model_deepseek_v3.py:493-500), kv_norm (:684), torch.cat (:686) and
 * append_to_paged_kv_cache (attn_backend.py:720-722).  Same arithmetic as the separate ops.
 *   kv_in_bf16: row b holds [kv_c (512) | k_pe (64)] (the tail of wqkv_a's output), row stride given;
 *   q_pe_bf16 [batch, heads, 64] rotated IN PLACE (strides in elements); cos/sin [batch, 32] f32;
 *   kv_cache [num_pages, page_size, 576] bf16: row (page_table[b][L/page], L%page), L = old_seq_lens[b],
 *   receives [rmsnorm(kv_c) * w | rope(k_pe)]. */
int chitu_hip_mla_kv_prep(const void* kv_in_bf16, int64_t kv_row_stride, void* q_pe_bf16,
                          int64_t q_stride_b, int64_t q_stride_h, int32_t heads, const float* cos,
                          const float* sin, const void* kv_norm_weight_bf16, float eps, void* kv_cache,
                          int64_t num_pages, int32_t page_size, const int32_t* page_table,
                          int32_t pages_per_seq, const int32_t* old_seq_lens, int32_t batch,
                          int32_t kv_lora_rank, int32_t rope_dim, void* stream);

/* Everything that consumes wqkv_a's output row [q_a (q_lora_rank) | kv_c (512) | k_pe (64)] in one
 * launch: q_norm + act_quant of q_a (= chitu_hip_rmsnorm quant_mode 1 -> q_fp8 [batch, q_lora_rank],
 * q_scales [batch, q_lora_rank/128], the input of the wq_b GEMM; model_deepseek_v3.py:480-487) and the
 * kv half of chitu_hip_mla_kv_prep (kv_norm + RoPE(k_pe) + page append).  q_pe is NOT rotated here
 * (it does not exist yet): use chitu_hip_absorb_bmm_rope_fp8 after wq_b.
 *   qkv_a: num_partials == 0: the GEMM's bf16 output [batch, row_stride]; num_partials >= 1: the fp32 split-K
 *   planes [num_partials, batch, row_stride] of chitu_hip_fp8_gemm_blockscale_partials -- each value is then
 *   bf16(plane 0 + plane 1 + ...), the rounding the GEMM's own epilogue would apply (q_lora_rank <= 2048). */
int chitu_hip_mla_qkv_post(const void* qkv_a, int32_t num_partials, int64_t row_stride, int32_t q_lora_rank,
                           const void* q_norm_weight_bf16, float q_eps, void* q_fp8, float* q_scales,
                           const void* kv_norm_weight_bf16, float kv_eps, const float* cos,
                           const float* sin, void* kv_cache, int64_t num_pages, int32_t page_size,
                           const int32_t* page_table, int32_t pages_per_seq,
                           const int32_t* old_seq_lens, int32_t batch, int32_t kv_lora_rank,
                           int32_t rope_dim, void* stream);

/* chitu_hip_mla_qkv_post AND the wq_b GEMM in one launch (decode, batch <= 32, q_lora_rank <= 2048):
 *   out[batch, N] = fp8_gemm(act_quant(q_norm(qkv_a[:, :q_lora_rank])), wq_b)   (model_deepseek_v3.py:488 with the
 *   linear's act_quant + fp8 GEMM, triton_kernels.py:194-216 / :302-365), and every token's
 *   [kv_norm(kv_c) | RoPE(k_pe)] row appended to its page (model_deepseek_v3.py:493-496, :684-686).
 * q_norm + act_quant run as the GEMM's prologue in every workgroup (per element the arithmetic of
 * chitu_hip_rmsnorm quant_mode 1; the mean square is summed in this kernel's own fixed order, so the rounded norm
 * can differ from chitu_hip_mla_qkv_post's in the last bf16 bit of a few elements).  wq_b [N, q_lora_rank] e4m3 with
 * scales [ceil(N/128), q_lora_rank/128]; out_dtype 0 bf16 / 1 f16 / 2 f32.  Other shapes: CHITU_ERR_UNSUPPORTED
 * (use chitu_hip_mla_qkv_post + chitu_hip_fp8_gemm_blockscale). */
int chitu_hip_mla_q_proj(const void* qkv_a_bf16, int64_t row_stride, int32_t q_lora_rank,
                         const void* q_norm_weight_bf16, float q_eps, const void* wq_b_fp8,
                         const float* wq_b_scale, void* out, int32_t out_dtype, int64_t N,
                         const void* kv_norm_weight_bf16, float kv_eps, const float* cos, const float* sin,
                         void* kv_cache, int64_t num_pages, int32_t page_size, const int32_t* page_table,
                         int32_t pages_per_seq, const int32_t* old_seq_lens, int32_t batch,
                         int32_t kv_lora_rank, int32_t rope_dim, void* stream);

/* ---- W_UV absorb projection fused with the FP8 quantisation of wo's input ---------------------
 * chitu_hip_absorb_bmm_fp8 for N = 128 (einsum "bshc,hdc->bshd", model_deepseek_v3.py:697) followed by
 * act_quant_deepseek_v3 of the bf16-rounded result (model_deepseek_v3.py:98-100 inside wo):
 *   q_fp8 [batch, heads*128] e4m3, q_scales [batch, heads] (one 128-group per head). */
int chitu_hip_absorb_uv_quant_fp8(const void* x_bf16, int64_t x_stride_b, int64_t x_stride_h,
                                  const void* w_fp8, int64_t w_stride_h, const float* scale,
                                  int64_t scale_offset, int64_t scale_stride_h, int64_t scale_stride_k,
                                  void* q_fp8, float* q_scales, int32_t batch, int32_t heads, int32_t K,
                                  void* stream);

/* ---- INT8 W8A8 linear (per-token activations x per-output-channel weights) --------------------
 * Replaces quant_act (chitu/quantize/w8a8.py:18-26) and the closed w8a8gemm.mm / w8a8gemv.mv behind
 * W8A8Linear.forward (chitu/quantize/w8a8.py:97-132; contract pinned by test/pytest/test_w8a8.py:13-48).
 *   quant_act_int8: s[row] = clamp(max|x[row]|, 1e-5)/127, q = int8(round_half_even(x/s)).
 *   w8a8_int8_gemm: out[m][n] = (sum_k a[m][k]*b[n][k] exact in i32) * a_scale[m] * b_scale[n] (+ bias[n]);
 *   a_int8 [M, K], b_int8 [N, K] (K % 128 == 0), scales f32, bias optional (bias_dtype), out of out_dtype. */
int chitu_hip_quant_act_int8(const void* x, int act_dtype, int64_t rows, int64_t cols, void* q_int8,
                             float* scales, void* stream);
int chitu_hip_w8a8_int8_gemm(const void* a_int8, const float* a_scale, const void* b_int8,
                             const float* b_scale, const void* bias, int bias_dtype, void* out,
                             int out_dtype, int64_t M, int64_t N, int64_t K, void* stream);

/* ---- GQA / MHA paged decode attention (head_dim 128) ------------------------------------------
 * Replaces the third-party flash_attn.flash_attn_with_kvcache call behind
 * FlashAttnBackend.attn_with_kvcache (chitu/attn_backend.py:208-243; contract :92-164) on the paged,
 * single-query path used by Attention.decode_forward_paged (chitu/models/model.py:167-198):
 *   out[b,h,:] = softmax_t(scale * q[b,h,:].K[t, h/(Hq/Hkv), :]) . V[t, h/(Hq/Hkv), :],  t < seqlens[b]
 *   q [batch, q_heads, 128] bf16 (element strides, multiples of 8); k_cache / v_cache
 *   [num_pages, page_size, kv_heads, 128] bf16, page_size % 16 == 0; block_table [batch, table_stride] i32;
 *   seqlens [batch] i32 = tokens to attend INCLUDING the row appended this step (append =
 *   chitu_hip_append_paged_kv on each cache); out [batch, q_heads, 128] bf16; q_heads/kv_heads <= 16.
 *   workspace >= batch*q_heads*num_splits*129*4 bytes when num_splits > 1. */
int chitu_hip_gqa_decode(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h, const void* k_cache,
                         const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                         const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                         float softmax_scale, void* out_bf16, int32_t batch, int32_t q_heads,
                         int32_t head_dim, int32_t num_splits, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ---- FP8 K / V cache of the GQA / MHA paged decode (csrc/gqa_kv_fp8.hip, csrc/gqa_decode_kv_fp8.hip) --------
 * K and V stay two caches of the shape above with byte rows: uint8 [num_pages, page_size, kv_heads, 144], base 16-byte aligned.
 * One (token, kv head) row: [0, 128) the head's channels as OCP e4m3fn codes, order unchanged | [128, 132) one fp32 scale, an
 * exact power of two | [132, 144) zero, written by every producer and read by nobody.  amax = max|x| over the head, e = the
 * smallest integer with amax <= 448 * 2^e clamped to e >= -64 (amax == 0: -64), scale = 2^e, code = RNE_e4m3(x * 2^-e) (never
 * overflows; the rule of the MLA cache above); NaN / Inf inputs are unspecified.  code * scale is a bf16 number: dequantisation
 * is exact.  head_dim 128 only.
 *   chitu_hip_gqa_kv_quant_fp8    new: no reference counterpart.  src bf16 [rows, kv_heads, 128] with a row stride in elements
 *     (>= kv_heads * 128, % 8, base 16-byte aligned) -> dst bytes [rows, kv_heads, 144] with a row stride in bytes
 *     (>= kv_heads * 144, % 16, base 16-byte aligned); bytes of a destination row beyond kv_heads * 144 are not written.
 *   chitu_hip_gqa_kv_dequant_fp8  new: no reference counterpart.  The inverse: byte rows (stride as above) -> bf16
 *     [rows, kv_heads, 128] contiguous.  Exact.
 *   chitu_hip_gqa_kv_append_fp8   new: no reference counterpart.  Quantises row b of k and of v (bf16 [batch, kv_heads, 128],
 *     row strides in elements) into position old_seq_lens[b] of sequence b's page in k_cache and in v_cache:
 *     cache[table[b][L / page_size]][L % page_size], one launch.  Any page_size >= 1.  A table entry outside [0, num_pages), a
 *     negative length or a position beyond pages_per_seq writes nothing (the rules of chitu_hip_append_paged_kv).
 *   chitu_hip_gqa_qkv_post_kv_fp8 new: no reference counterpart.  chitu_hip_gqa_qkv_post's argument list with byte-row caches:
 *     RoPE on q in place and on k, the rotated k rounded to bf16 exactly as chitu_hip_gqa_qkv_post rounds it and then
 *     quantised, v quantised, both written straight into the page rows -- bit for bit the quantiser's image of the rows
 *     chitu_hip_gqa_qkv_post writes.  Both rotary layouts; head_dim 128.
 *   chitu_hip_gqa_decode_kv_fp8   new: no reference counterpart.  chitu_hip_gqa_decode's argument list and contract (grid, split
 *     arithmetic, workspace layout, limits) with k_cache / v_cache reading 144-byte rows.  q stays bf16; codes are widened to
 *     bf16 in registers (exact) and everything behind that is chitu_hip_gqa_decode's arithmetic in its order: the output, and
 *     with num_splits > 1 the workspace, are bit-identical to chitu_hip_gqa_decode on the dequantised cache.  Bytes past a
 *     sequence's length are never used, whatever they hold. */
int chitu_hip_gqa_kv_quant_fp8(const void* src_bf16, int64_t src_stride, void* dst_u8, int64_t dst_stride_bytes,
                               int64_t rows, int32_t kv_heads, void* stream);
int chitu_hip_gqa_kv_dequant_fp8(const void* src_u8, int64_t src_stride_bytes, void* dst_bf16, int64_t rows,
                                 int32_t kv_heads, void* stream);
int chitu_hip_gqa_kv_append_fp8(const void* k_bf16, int64_t k_stride, const void* v_bf16, int64_t v_stride,
                                void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                int32_t kv_heads, const int32_t* block_table, int32_t pages_per_seq,
                                const int32_t* old_seq_lens, int32_t batch, void* stream);
int chitu_hip_gqa_qkv_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                  int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                  void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                  const int32_t* page_table, int32_t pages_per_seq,
                                  const int32_t* old_seq_lens, int32_t batch, void* stream);
int chitu_hip_gqa_decode_kv_fp8(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h, const void* k_cache,
                                const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                                const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                                float softmax_scale, void* out_bf16, int32_t batch, int32_t q_heads,
                                int32_t head_dim, int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                void* stream);

/* ---- Sliding-window and soft-capped GQA / MHA paged decode (csrc/gqa_decode_tile.h, kWin) ----------------------------------
 * window_size = (window_left, 0) and softcap of attn_with_kvcache (chitu/attn_backend.py:92-164, the window rule :136-138;
 * FlashAttnBackend forwards both to flash_attn, :208-243; the arithmetic is RefAttnBackend._attention, :294-392).
 * chitu_hip_gqa_decode's / chitu_hip_gqa_decode_kv_fp8's argument list, contract, workspace and limits with two more arguments
 * before the stream:
 *   window_left = W >= 0: the query (position L - 1, L = seqlens[b]) sees the keys w0 = max(0, L - 1 - W) .. L - 1; W = 0: only
 *     the row appended this step; -1: no window.
 *   softcap = c > 0: the score is c * tanh(softmax_scale * q.k / c), before the mask and the softmax; 0: off.
 * window_left < -1 or softcap < 0 (or NaN): CHITU_ERR_BAD_ARG.  (-1, 0) launches the plain entry's own kernel: same bits,
 * workspace partials included.  With a window the 16-token steps [w0 / 16, ceil(L / 16)) are divided among the splits the way
 * [0, ceil(L / 16)) is without one, so for w0 % 16 == 0 and page_size 16 the call equals, bit for bit, the plain call on the
 * table shifted left by w0 / 16 pages with length L - w0.  Rows before w0 are as free as rows past L: whatever they hold (NaN
 * rows, NaN codes and scales) is never used, and a table entry of a page wholly before the window is never read.
 *   chitu_hip_gqa_decode_window          bf16 caches.
 *   chitu_hip_gqa_decode_kv_fp8_window   144-byte fp8 rows; bit-identical to the bf16 entry on the dequantised cache. */
int chitu_hip_gqa_decode_window(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h, const void* k_cache,
                                const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                                const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                                float softmax_scale, void* out_bf16, int32_t batch, int32_t q_heads,
                                int32_t head_dim, int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                int32_t window_left, float softcap, void* stream);
int chitu_hip_gqa_decode_kv_fp8_window(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h, const void* k_cache,
                                       const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                                       const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                                       float softmax_scale, void* out_bf16, int32_t batch, int32_t q_heads,
                                       int32_t head_dim, int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                       int32_t window_left, float softcap, void* stream);

/* ---- Multi-token GQA / MHA paged decode (csrc/gqa_decode_multi.hip) -------------------------------------------------------
 * The `seqlen > 1` half of attn_with_kvcache (chitu/attn_backend.py:92-164: q (batch, seqlen, nheads, headdim), k / v of
 * seqlen_new rows appended at cache_seqlens, the causal mask aligned to the bottom right, the window formula for seqlen_q > 1;
 * the arithmetic is RefAttnBackend._attention, :294-392) for q_len = T in 1 .. 8: the verify step of speculative decoding.
 * chitu_hip_gqa_decode_window's argument list, contract, workspace layout and limits with q_stride_t after q_stride_b and q_len
 * after batch:
 *   q [batch, T, q_heads, 128] bf16 (element strides, multiples of 8); seqlens[b] = L counts ALL keys of sequence b, the T rows
 *   appended this step included; out [batch, T, q_heads, 128] bf16 contiguous.
 *   Query token t sits at position L - T + t and sees key k iff k <= L - T + t and, with window_left = W >= 0,
 *   k >= L - T + t - W: query (b, t) is chitu_hip_gqa_decode_window on a row of length L - T + t + 1 over the same table.  A query
 *   with no visible key (L - T + t < 0) gives zeros.  softcap as in chitu_hip_gqa_decode_window; (-1, 0.0) are neutral and launch
 *   the kernel without the window / cap code.
 *   16 / (q_heads / kv_heads) query tokens share one wave's K / V walk (the q heads of a group and those tokens fill the 16 MFMA
 *   columns), so the pages are read ceil(T / that) times instead of T times.
 *   workspace >= batch*T*q_heads*num_splits*129*4 bytes when num_splits > 1: one row of partials per (b, t, h).
 *   q_len outside 1 .. 8: CHITU_ERR_BAD_ARG.  At q_len == 1 the output and the workspace are bit-identical to
 *   chitu_hip_gqa_decode / _window (and _kv_fp8 / _kv_fp8_window) at the same num_splits; at q_len > 1 they are NOT the bits of
 *   batch * T single-token rows (the wave-wide rescale vote sees the other tokens' columns).
 *   chitu_hip_gqa_decode_multi          bf16 caches.
 *   chitu_hip_gqa_decode_multi_kv_fp8   144-byte fp8 rows; bit-identical to the bf16 entry on the dequantised cache. */
int chitu_hip_gqa_decode_multi(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_t, int64_t q_stride_h,
                               const void* k_cache, const void* v_cache, int64_t num_pages, int32_t page_size,
                               int32_t kv_heads, const int32_t* block_table, int32_t table_stride,
                               const int32_t* seqlens, float softmax_scale, void* out_bf16, int32_t batch,
                               int32_t q_len, int32_t q_heads, int32_t head_dim, int32_t num_splits, void* workspace,
                               int64_t workspace_bytes, int32_t window_left, float softcap, void* stream);
int chitu_hip_gqa_decode_multi_kv_fp8(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_t, int64_t q_stride_h,
                                      const void* k_cache, const void* v_cache, int64_t num_pages, int32_t page_size,
                                      int32_t kv_heads, const int32_t* block_table, int32_t table_stride,
                                      const int32_t* seqlens, float softmax_scale, void* out_bf16, int32_t batch,
                                      int32_t q_len, int32_t q_heads, int32_t head_dim, int32_t num_splits,
                                      void* workspace, int64_t workspace_bytes, int32_t window_left, float softcap,
                                      void* stream);

/* ---- token sampling (the step after the path) -----------------------------------
 * Replaces NormalExecutor.update_response's device work (chitu/executor.py:82-112) and
 * top_k_top_p_min_p_sampling_from_probs_torch (chitu/utils.py:62-81: full sort + cumsum + multinomial).
 *   frequency_penalty: logits[row, t] -= penalties[row] once per occurrence of t in
 *     tokens[offsets[row] .. offsets[row+1]) for rows with penalties[row] > 0 (executor.py:89-102);
 *     logits [rows, row_stride] f32 in place, tokens i32 (ids outside [0, vocab) ignored).
 *   sample: one token per row, out_tokens [rows] i64.
 *     top_ks == NULL: greedy for every row = first index of the row maximum (executor.py:103-104).
 *     else per row: top_k == 1 -> arg-max; otherwise weights e = exp(x/T - max) (probs_mode 0: `logits`
 *     are logits, temperatures [rows]) or p / max p (probs_mode 1: `logits` are probabilities,
 *     temperatures may be NULL); the entry at position pos of the descending order (ties: lower
 *     index first) is kept iff pos < top_k (top_k <= 0: no limit) and the exclusive cumulative
 *     weight before it is <= top_p * sum(weights) (top_p >= 1: no limit) -- utils.py:72-76;
 *     the token is the inverse CDF of uniforms[row] in [0, 1) over the kept weights in index
 *     order.  Weights are accumulated as integers (scaled by 2^40), so results are deterministic.
 *     n_kept_out [rows] i32 / kept_mass_out [rows] f32 (kept weight / total) are optional.
 *   logits of act_dtype (0 bf16, 1 f16, 2 f32), row_stride in elements, any vocab > 0. */
int chitu_hip_frequency_penalty(float* logits, int64_t row_stride, int64_t rows, int32_t vocab,
                                const int32_t* tokens, const int32_t* offsets, const float* penalties,
                                void* stream);
int chitu_hip_sample(const void* logits, int act_dtype, int64_t row_stride, int64_t rows, int32_t vocab,
                     const float* temperatures, const int32_t* top_ks, const float* top_ps,
                     const float* uniforms, int32_t probs_mode, int64_t* out_tokens,
                     int32_t* n_kept_out, float* kept_mass_out, void* stream);
/*   chitu_hip_speculative_verify  new: no reference counterpart.  Draft verification of speculative decoding with sampling:
 *     the draft d of a row is accepted with probability p(d), p being the distribution chitu_hip_sample draws from for that row;
 *     a rejected row emits a draw from p with d removed and the rest renormalised, so every emitted token is distributed as p.
 *     logits [rows, vocab], act_dtype, row_stride, temperatures / top_ks / top_ps [rows] and probs_mode as chitu_hip_sample
 *     (all arrays required; temperatures may be NULL in probs_mode); rows = bs * q_len, 2 <= q_len <= 8, row b * q_len + t
 *     judges the token after position t of sequence b.  drafts [rows] i32: the proposed token, < 0 for none (each sequence's
 *     last row).  uniforms [rows, 2] f32 in [0, 1): (u_acc, u_alt).  In the sampler's integers (K the kept set, w_i = floor(e_i *
 *     2^40), S = sum_K w_i, target(u, s) = min(floor(u * s), s - 1)): top_k == 1 or S == 0 -> accepted iff d == arg-max, token
 *     = arg-max; else w_d = d's kept weight (0 if d is not kept or >= vocab), accepted iff target(u_acc, S) < w_d with token = d,
 *     otherwise token = inverse CDF in index order over K \ {d} at target(u_alt, S - w_d); d < 0 -> not accepted, token =
 *     chitu_hip_sample's for u_alt.  out [bs, q_len + 1] i64: n_ok = leading accepted rows among the first q_len - 1 of the
 *     sequence; out[b] = [n_ok + 1, token of rows 0 .. n_ok, -1 ...].  accepted_out [rows] i32 / row_tokens_out [rows] i64
 *     (the per-row results) are optional.  Two launches on `stream`; rows == 0 launches nothing. */
int chitu_hip_speculative_verify(const void* logits, int act_dtype, int64_t row_stride, int64_t rows, int32_t vocab,
                                 const float* temperatures, const int32_t* top_ks, const float* top_ps,
                                 const int32_t* drafts, const float* uniforms, int32_t q_len, int32_t probs_mode,
                                 int64_t* out, int32_t* accepted_out, int64_t* row_tokens_out, void* stream);
/*   chitu_hip_speculative_verify_sampled  new: no reference counterpart.  The same verification for a draft d that was DRAWN from a
 *     draft model's distribution q: accepted with probability min(1, p(d) / q(d)); a rejected row emits a draw from max(p - q, 0),
 *     renormalised, so every emitted token is distributed as p for ANY q, provided q is what d was drawn from.  Arguments as
 *     chitu_hip_speculative_verify, plus draft_logits [rows, vocab] with its own draft_act_dtype and draft_row_stride, indexed by
 *     the same row b * q_len + t; temperatures / top_ks / top_ps / probs_mode apply to both rows of a pair (the drafter samples
 *     under the request's parameters).  The draft row of a row without a draft (drafts < 0, each sequence's last) is never read
 *     and may hold anything.  vocab <= 2^21.  In integers, with K_p, w_i, S_p the kept set, weights and sum of the target row as
 *     above, K_q, v_i, S_q the same of the draft row and U(u) = min(floor(u * 2^24), 2^24 - 1): top_k == 1, S_p == 0 or S_q == 0
 *     -> accepted iff d == arg-max of the target row, token = that arg-max; d < 0 -> not accepted, token = chitu_hip_sample's
 *     for u_alt on the target row; else with w_d, v_d the kept weights of d (0 if not kept or >= vocab): accepted iff
 *     U(u_acc) * v_d * S_p < 2^24 * w_d * S_q with token = d, otherwise r_i = max(0, w_i * S_q - v_i * S_p), R = sum r_i and token
 *     = inverse CDF over r in index order at floor(U(u_alt) * R / 2^24) (R == 0, which no rejection of a d drawn from q gives:
 *     the arg-max).  All products in unsigned 128-bit integers.  out / accepted_out / row_tokens_out and the two launches as
 *     chitu_hip_speculative_verify. */
int chitu_hip_speculative_verify_sampled(const void* logits, int act_dtype, int64_t row_stride, const void* draft_logits,
                                         int draft_act_dtype, int64_t draft_row_stride, int64_t rows, int32_t vocab,
                                         const float* temperatures, const int32_t* top_ks, const float* top_ps,
                                         const int32_t* drafts, const float* uniforms, int32_t q_len, int32_t probs_mode,
                                         int64_t* out, int32_t* accepted_out, int64_t* row_tokens_out, void* stream);

/* ---- in-graph tensor-parallel collectives over xGMI (csrc/comm.hip) --------------------------------
 * Replace the NCCL calls of the reference's decode step -- dist.all_reduce after every RowParallelLinear
 * (chitu/tensor_parallel.py:157-169) and after the MoE (chitu/models/model_deepseek_v3.py:1010-1011), the
 * all_gather_into_tensor of a gather_output ColumnParallelLinear (tensor_parallel.py:94-102) -- with plain
 * kernel launches that a hipGraph captures like any other (the reference captures its NCCL calls into the
 * step's CUDA graph, chitu/models/model.py:554-617).
 * SETUP entries (these DO allocate / synchronise; call them once, outside any capture):
 *   comm_create: one uncached device buffer on the current device for rank `rank` of `world` (<= 8) ranks:
 *     all-reduce of up to max_rows x max_dim bf16 (max_dim <= 8192), all-gather of up to gather_bytes per rank;
 *     every wait inside the kernels gives up after timeout_ms and sets a sticky error word (comm_status).
 *   comm_ipc_handle / comm_open_peer: the 64-byte hipIpcMemHandle_t of this rank's buffer / map a peer's
 *     (ranks in different processes; exchange the handles over any host channel, e.g. the process group's
 *     store).  comm_local_ptr / comm_set_peer: the same for ranks that share one process (raw pointers).
 *     Every rank must have created (and thereby zeroed) its buffer before any peer launches a collective.
 *   comm_status: blocking read of the error word (0 = fine, bit 0 = a wait timed out).
 *   comm_poll_error: NON-blocking read of the pinned host copy of that word (the kernel that times out stores
 *     both); a serving loop calls it between steps -- where the reference would see NCCL's watchdog abort the
 *     process (its all_reduce never returns garbage silently) -- without synchronising the stream.
 * COLLECTIVES (enqueue only; every rank of the group must issue the same sequence of calls):
 *   comm_allreduce_rmsnorm -- one launch for [top-k sum ->] all-reduce -> residual add -> RMSNorm -> fp8 quant:
 *     part_r = terms > 1 ? bf16(sum_k float(part[row*part_row_stride + k*term_stride + :])) : part[row]
 *              (terms <= 16: chitu_hip_moe_sum's arithmetic, fused_moe.py:1299-1305)
 *     a      = bf16(sum over ranks r = 0..world-1, in that order, of float(part_r))   -- identical on every rank
 *     v      = x ? bf16(x + a) : a            -> sum_out [rows, dim]   (optional when a weight is given)
 *     weight: y = rmsnorm(v) * weight -> y_bf16 and / or (q_fp8, q_scales), exactly chitu_hip_rmsnorm's
 *     arithmetic and quant modes; weight == NULL: plain all-reduce (y, q must be NULL, sum_out required).
 *     rows <= max_rows, dim <= max_dim, dim % 8 == 0 (CHITU_ERR_UNSUPPORTED otherwise: use the library path).
 *   comm_all_gather: out[row, r*cols + j] = in_r[row, j] (rank-major concat of the last dimension);
 *     in bf16 [rows, cols] (row stride given, cols % 8 == 0, rows*cols*2 <= gather_bytes); out_dtype 0 = bf16,
 *     2 = f32 (the logits' `.float()`, models/model.py:475, rides along); out [rows, world*cols] dense.
 *   phase (both): 0 = the whole collective; 1 = contribute only (push this rank's data, signal, return);
 *     2 = complete only (wait for the peers, reduce / gather, advance the call counter) -- issue it after a
 *     phase-1 launch with the same arguments.  Split phases let work sit between the push and the wait. */
int chitu_hip_comm_create(int32_t rank, int32_t world, int32_t max_rows, int32_t max_dim,
                          int64_t gather_bytes, int32_t timeout_ms, void** comm_out);
int chitu_hip_comm_ipc_handle(void* comm, void* handle_out_64);
int chitu_hip_comm_open_peer(void* comm, int32_t peer, const void* handle_64);
int chitu_hip_comm_local_ptr(void* comm, void** ptr_out);
int chitu_hip_comm_set_peer(void* comm, int32_t peer, void* ptr);
int chitu_hip_comm_status(void* comm, uint32_t* err_out);
int chitu_hip_comm_poll_error(void* comm, uint32_t* err_out);
/* All-reduces of >= min_bytes per rank take the two-shot form (reduce-scatter + all-gather inside the same launch: 2/world
 * of the bytes per xGMI link, one more flag hop; bit-identical to the one-shot form).  Default 256 KB; same value on every
 * rank; host-side, set before capture.  With it, phase 3 = "wait for hop 1, reduce my slice, send hop 2" of a split launch
 * (1 = hop 1, 3, 2 = wait for hop 2 + finish). */
int chitu_hip_comm_set_two_shot(void* comm, int64_t min_bytes);
int chitu_hip_comm_destroy(void* comm);
int chitu_hip_comm_allreduce_rmsnorm(void* comm, const void* part_bf16, int64_t part_row_stride,
                                     int32_t terms, int64_t term_stride, const void* x_bf16,
                                     int64_t x_row_stride, void* sum_out_bf16, int64_t sum_row_stride,
                                     const void* weight_bf16, void* y_bf16, int64_t y_row_stride,
                                     int64_t rows, int32_t dim, float eps, void* q_fp8, float* q_scales,
                                     int32_t quant_mode, float quant_eps, int32_t phase, void* stream);
int chitu_hip_comm_all_gather(void* comm, const void* in_bf16, int64_t in_row_stride, int64_t rows,
                              int64_t cols, void* out, int32_t out_dtype, int32_t phase, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_H */
