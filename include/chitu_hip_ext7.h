/* chitu_hip_ext7.h -- the seventh set of additions to the C ABI of libchitu_hip.so.
 *
 * chitu_hip.h is frozen at ABI version 13, chitu_hip_ext.h .. chitu_hip_ext6.h at version 1 each: bindings and checks pin the
 * text of all seven.  Entry points added after them live here, are exported from the same library under the prefix
 * chitu_ext7_, and follow chitu_hip.h's conventions: device pointers owned by the caller, launches enqueued on `stream`
 * (hipGraph-capturable), return value 0 = enqueued, <0 = argument error (CHITU_ERR_BAD_ARG -1, CHITU_ERR_UNSUPPORTED -2),
 * >0 = hipError_t.  Additive only: an entry, once declared here, keeps its argument list; CHITU_HIP_EXT7_VERSION counts the
 * additions.
 */
#ifndef CHITU_HIP_EXT7_H
#define CHITU_HIP_EXT7_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT7_VERSION 1  /* 1: the four entries of the partial rotary width (GLM-4 dense models) */

/* ---- RoPE over the first rotary_dim channels of a 128-channel head (GLM-4-9B: rotary_dim 64, interleaved pairs) -----------
 * Every entry takes `int32_t rotary_dim` (R) directly after `layout`.  cos / sin are fp32 [rows, R / 2], row stride R / 2.
 * With layout 0 the pairs (2 i, 2 i + 1), i < R / 2, of a head rotate by entry i of the row as chitu_hip_rope states it:
 *   r0 = x0 c - x1 s, r1 = x1 c + x0 s    fp32, products rounded separately, one rounding to bf16
 * and the channels R .. 127 are the prepared channels themselves, bit for bit (with a bias: the bf16-rounded x + b).  This is
 * Hugging Face's modeling_glm.apply_rotary_pos_emb, not the reference's torch branch of rotary_type "glm4"
 * (chitu/ops.py:268-305), which pairs element j of its permuted vector with frequency j / 2.
 *   R must be a multiple of 8 in [8, 128] (rows of R / 2 floats stay 16-byte aligned, 8-channel lanes are whole): anything
 *   else is CHITU_ERR_BAD_ARG.  layout 1 (half split) with R < 128: CHITU_ERR_UNSUPPORTED.  R == 128: bit for bit the entry
 *   named below as replaced, in either layout.  head_dim 128 only (anything else: CHITU_ERR_UNSUPPORTED); every base pointer
 *   16-byte aligned; arguments are checked before the zero-size return and nothing is launched for zero rows.
 *   chitu_ext7_gqa_qkv_bias_post         replaces chitu_ext5_gqa_qkv_bias_post where the width is partial: its argument
 *     list plus rotary_dim; the same launch (one workgroup per row), bias, range rules and check order.
 *   chitu_ext7_gqa_qkv_bias_post_kv_fp8  replaces chitu_ext5_gqa_qkv_bias_post_kv_fp8 likewise: the partly rotated k head,
 *     rounded to bf16, and the v head are quantised into the 144-byte rows (chitu_hip_gqa_kv_quant_fp8).
 *   chitu_ext7_qkv_bias_rope             replaces chitu_ext5_qkv_bias_rope likewise: the prefill form, no cache, 16 heads
 *     per workgroup; bit for bit the decode entries' q and page rows.
 *   chitu_ext7_rope                      replaces chitu_hip_rope (reference: chitu/ops.py:243-326, apply_rotary_pos_emb)
 *     for rotary_type "glm4": chitu_hip_rope's argument list plus rotary_dim.  act_dtype 0 (bf16) and head_dim 128 only
 *     (anything else: CHITU_ERR_UNSUPPORTED); strides in elements, multiples of 8 (a 2-D k: k_heads 1, head strides
 *     0); one 16-lane row per head, 16 heads per workgroup. */
int chitu_ext7_gqa_qkv_bias_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                                 const float* cos, const float* sin, int32_t layout, int32_t rotary_dim, void* k_cache,
                                 void* v_cache, int64_t num_pages, int32_t page_size, const int32_t* page_table,
                                 int32_t pages_per_seq, const int32_t* old_seq_lens, int32_t batch, const void* bias_bf16,
                                 void* stream);
int chitu_ext7_gqa_qkv_bias_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                        int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                        int32_t rotary_dim, void* k_cache_u8, void* v_cache_u8, int64_t num_pages,
                                        int32_t page_size, const int32_t* page_table, int32_t pages_per_seq,
                                        const int32_t* old_seq_lens, int32_t batch, const void* bias_bf16, void* stream);
int chitu_ext7_qkv_bias_rope(const void* qkv_bf16, int64_t row_stride, int64_t head_stride, const void* bias_bf16,
                             const float* cos, const float* sin, void* out_q_bf16, void* out_k_bf16, void* out_v_bf16,
                             int64_t rows, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t layout,
                             int32_t rotary_dim, void* stream);
int chitu_ext7_rope(const void* q, const void* k, void* out_q, void* out_k, const float* cos, const float* sin,
                    int act_dtype, int32_t batch, int32_t q_heads, int32_t k_heads, int32_t head_dim, int64_t q_sb,
                    int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t oq_sb, int64_t oq_sh, int64_t ok_sb, int64_t ok_sh,
                    int32_t layout, int32_t rotary_dim, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT7_H */
