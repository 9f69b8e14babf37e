/* chitu_hip_ext5.h -- the fifth set of additions to the C ABI of libchitu_hip.so.
 *
 * chitu_hip.h is frozen at ABI version 13, chitu_hip_ext.h .. chitu_hip_ext4.h at version 1 each: bindings and checks pin the
 * text of all five.  Entry points added after them live here, are exported from the same library under the prefix
 * chitu_ext5_, and follow chitu_hip.h's conventions: device pointers owned by the caller, launches enqueued on `stream`
 * (hipGraph-capturable), return value 0 = enqueued, <0 = argument error (CHITU_ERR_BAD_ARG -1, CHITU_ERR_UNSUPPORTED -2),
 * >0 = hipError_t.  Additive only: an entry, once declared here, keeps its argument list; CHITU_HIP_EXT5_VERSION counts the
 * additions.
 */
#ifndef CHITU_HIP_EXT5_H
#define CHITU_HIP_EXT5_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT5_VERSION 1  /* 1: the three entries of the q / k / v projection bias (Qwen2 dense models) */

/* ---- q / k / v projection bias fused with RoPE and the paged K / V append (Qwen2, Qwen2.5, R1-Distill-Qwen) -------------
 * New: no reference counterpart (the reference adds the bias inside torch's linear).  bias is ONE bf16 row
 * [(q_heads + 2 kv_heads) * 128], laid out like a row of qkv: this rank's q heads, then k heads, then v heads.  For every
 * head of every row
 *   y_i = bf16_rne(float(x_i) + float(b_i))     one fp32 add, one rounding -- a bf16 torch.add
 *   q and k heads: RoPE on y widened back to fp32 as chitu_hip_rope states it (products rounded separately, one rounding to
 *   bf16; layout 0 = interleaved pairs, 1 = half split; cos / sin fp32 [rows, 64]);  v heads: y itself.
 * All three entries share the arithmetic bit for bit.  This is not the single rounding of an fp32 accumulator plus bias:
 * the GEMM in front has already rounded x to bf16.  head_dim 128 only (anything else: CHITU_ERR_UNSUPPORTED); every base
 * pointer 16-byte aligned; nothing is launched for zero rows.
 *   chitu_ext5_gqa_qkv_bias_post         new: no reference counterpart.  chitu_hip_gqa_qkv_post's argument list, then bias
 *     (in front of the stream).  q heads are biased and rotated IN PLACE; k heads are biased, rotated and stored to the token's
 *     bf16 page row; biased v heads are stored to theirs; the k and v heads of the qkv row stay as they were.  q and every
 *     cache byte are, bit for bit, chitu_hip_gqa_qkv_post's on the bf16 sum qkv + bias.  The range rules are
 *     chitu_hip_gqa_qkv_post's: a negative length, a position beyond pages_per_seq or a table entry outside [0, num_pages)
 *     writes nothing to the caches and still produces q.
 *   chitu_ext5_gqa_qkv_bias_post_kv_fp8  new: no reference counterpart.  chitu_hip_gqa_qkv_post_kv_fp8's argument list,
 *     then bias (in front of the stream): the same over the 144-byte rows of the fp8 K / V cache
 *     (chitu_hip_gqa_kv_quant_fp8) -- the rotated k head rounded to bf16 as above and the v head y are quantised, the 12
 *     zero bytes written.  Bit for bit chitu_hip_gqa_qkv_post_kv_fp8 on qkv + bias.
 *   chitu_ext5_qkv_bias_rope             new: no reference counterpart.  The prefill form, no cache: qkv [rows, q_heads +
 *     2 kv_heads, 128] with row and head strides in elements (multiples of 8) -> contiguous out_q [rows, q_heads, 128],
 *     out_k and out_v [rows, kv_heads, 128], the whole prompt in one launch. */
int chitu_ext5_gqa_qkv_bias_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                                 const float* cos, const float* sin, int32_t layout, void* k_cache, void* v_cache,
                                 int64_t num_pages, int32_t page_size, const int32_t* page_table, int32_t pages_per_seq,
                                 const int32_t* old_seq_lens, int32_t batch, const void* bias_bf16, void* stream);
int chitu_ext5_gqa_qkv_bias_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                        int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                        void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                        const int32_t* page_table, int32_t pages_per_seq, const int32_t* old_seq_lens,
                                        int32_t batch, const void* bias_bf16, void* stream);
int chitu_ext5_qkv_bias_rope(const void* qkv_bf16, int64_t row_stride, int64_t head_stride, const void* bias_bf16,
                             const float* cos, const float* sin, void* out_q_bf16, void* out_k_bf16, void* out_v_bf16,
                             int64_t rows, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t layout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT5_H */
