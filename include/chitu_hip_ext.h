/* chitu_hip_ext.h -- additions to the C ABI of libchitu_hip.so after CHITU_HIP_ABI_VERSION 13.
 *
 * chitu_hip.h is frozen at ABI version 13 (94 entry points): bindings and checks pin its text.  Entry points added after
 * that live here, are exported from the same library under the prefix chitu_ext_, and follow chitu_hip.h's conventions:
 * device pointers owned by the caller, launches enqueued on `stream` (hipGraph-capturable), return value 0 = enqueued,
 * <0 = argument error (CHITU_ERR_BAD_ARG -1, CHITU_ERR_UNSUPPORTED -2), >0 = hipError_t.  Additive only: an entry, once
 * declared here, keeps its argument list; CHITU_HIP_EXT_VERSION counts the additions.
 */
#ifndef CHITU_HIP_EXT_H
#define CHITU_HIP_EXT_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT_VERSION 1  /* 1: the three entries of the per-head QK-norm (Qwen3 dense models) */

/* ---- per-head QK-norm fused with RoPE and the paged K / V append (Qwen3) ----------------------------------------------
 * New: no reference counterpart (the reference has no Qwen3 model).  Qwen3 applies an RMSNorm with a learned [128] weight to
 * every q head and every k head, after the projection and before RoPE.  One head x of 128 bf16 channels, weight w (bf16):
 *   rr = rsqrtf(sum x_i^2 / 128 + eps) in fp32, n_i = bf16((x_i * rr) * w_i) (chitu_hip_rmsnorm's order, one rounding), then
 *   RoPE on n as chitu_hip_rope states it (products rounded separately, one rounding to bf16).  layout 0 = interleaved
 *   pairs, 1 = half-split; cos / sin fp32 [rows, 64].  All three entries share the arithmetic bit for bit.  head_dim 128
 *   only (anything else: CHITU_ERR_UNSUPPORTED); every base pointer 16-byte aligned; nothing is launched for zero rows.
 *   chitu_ext_gqa_qkv_norm_post         new: no reference counterpart.  chitu_hip_gqa_qkv_post's argument list, then
 *     q_norm_weight, k_norm_weight [128] bf16 and eps.  q heads are normalised and rotated IN PLACE; k heads are normalised,
 *     rotated and stored to the token's bf16 page row; v heads are copied.  The range rules are chitu_hip_gqa_qkv_post's: a
 *     negative length, a position beyond pages_per_seq or a table entry outside [0, num_pages) writes nothing to the caches
 *     and still produces q.
 *   chitu_ext_gqa_qkv_norm_post_kv_fp8  new: no reference counterpart.  The same over the 144-byte rows of the fp8 K / V
 *     cache (chitu_hip_gqa_kv_quant_fp8): k rounded to bf16 exactly as above and then quantised, v quantised, the 12 zero
 *     bytes written -- bit for bit the quantiser's image of the rows chitu_ext_gqa_qkv_norm_post writes.
 *   chitu_ext_qk_norm_rope              new: no reference counterpart.  The prefill form, no cache: q [rows, q_heads, 128]
 *     and k [rows, k_heads, 128] with row and head strides in elements (multiples of 8) -> out_q, out_k, the whole prompt
 *     in one launch. */
int chitu_ext_gqa_qkv_norm_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                void* k_cache, void* v_cache, int64_t num_pages, int32_t page_size,
                                const int32_t* page_table, int32_t pages_per_seq, const int32_t* old_seq_lens,
                                int32_t batch, const void* q_norm_weight_bf16, const void* k_norm_weight_bf16,
                                float eps, void* stream);
int chitu_ext_gqa_qkv_norm_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                       int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                       void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                       const int32_t* page_table, int32_t pages_per_seq,
                                       const int32_t* old_seq_lens, int32_t batch, const void* q_norm_weight_bf16,
                                       const void* k_norm_weight_bf16, float eps, void* stream);
int chitu_ext_qk_norm_rope(const void* q_bf16, const void* k_bf16, void* out_q_bf16, void* out_k_bf16,
                           const float* cos, const float* sin, const void* q_norm_weight_bf16,
                           const void* k_norm_weight_bf16, float eps, int64_t rows, int32_t q_heads, int32_t k_heads,
                           int32_t head_dim, int64_t q_sb, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t oq_sb,
                           int64_t oq_sh, int64_t ok_sb, int64_t ok_sh, int32_t layout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT_H */
