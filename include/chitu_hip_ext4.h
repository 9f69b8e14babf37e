/* chitu_hip_ext4.h -- the fourth set of additions to the C ABI of libchitu_hip.so.
 *
 * chitu_hip.h is frozen at ABI version 13, chitu_hip_ext.h, chitu_hip_ext2.h and chitu_hip_ext3.h at version 1 each: bindings
 * and checks pin the text of all four.  Entry points added after them live here, are exported from the same library under the
 * prefix chitu_ext4_, and follow chitu_hip.h's conventions: device pointers owned by the caller, launches enqueued on `stream`
 * (hipGraph-capturable), return value 0 = enqueued, <0 = argument error (CHITU_ERR_BAD_ARG -1, CHITU_ERR_UNSUPPORTED -2),
 * >0 = hipError_t.  Additive only: an entry, once declared here, keeps its argument list; CHITU_HIP_EXT4_VERSION counts the
 * additions.
 */
#ifndef CHITU_HIP_EXT4_H
#define CHITU_HIP_EXT4_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT4_VERSION 1  /* 1: the flash GQA prefill kernels at every group size up to 32 */

/* ---- causal GQA / MHA flash prefill, head_dim 128, at any group size G = q_heads / kv_heads <= 32 ---------------------------
 * chitu_hip_gqa_prefill, chitu_hip_gqa_prefill_window and chitu_hip_gqa_prefill_paged take G in {1, 2, 4, 8, 16, 32} and keep
 * refusing every other one.  These two entries run the same kernel (csrc/gqa_prefill_flash.hip) with the same arguments, the
 * same meaning of each and the same host checks, and take every 1 <= G <= 32: Q row R of a workgroup's 128 is head R % G of
 * its token R / G, 128 / G tokens per workgroup, and the 128 - (128 / G) * G rows left over compute as copies of the last one
 * and store nothing.  At a power of two they launch exactly what the old entries launch.
 *   chitu_ext4_gqa_prefill        the argument list of chitu_hip_gqa_prefill_window; window_left = -1 with softcap = 0 selects
 *     the kernels of chitu_hip_gqa_prefill (no window or cap code).
 *   chitu_ext4_gqa_prefill_paged  the argument list of chitu_hip_gqa_prefill_paged.
 * Checked on the host before anything is launched and before the zero-size return: a null pointer, a negative count,
 * q_heads % kv_heads != 0, window_left < -1, a negative or NaN softcap, a stride that is no multiple of 8 elements or a
 * pointer not 16-byte aligned: CHITU_ERR_BAD_ARG; head_dim != 128, G > 32 or (paged) a page_size that is no multiple of 16:
 * CHITU_ERR_UNSUPPORTED; n_seq == 0 or max_seqlen == 0 launches nothing and returns 0. */
int chitu_ext4_gqa_prefill(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_bf16, int64_t k_stride_t,
    int64_t k_stride_h, const void* v_bf16, int64_t v_stride_t, int64_t v_stride_h, const int32_t* cu_seqlens, int32_t n_seq,
    int32_t max_seqlen, float softmax_scale, void* out_bf16, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
    int32_t window_left, float softcap, void* stream);
int chitu_ext4_gqa_prefill_paged(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_cache,
    const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads, const int32_t* block_table,
    int32_t table_stride, const int32_t* cu_seqlens_q, const int32_t* seqlens_k, int32_t n_seq, int32_t max_seqlen_q,
    float softmax_scale, void* out_bf16, int32_t q_heads, int32_t head_dim, int32_t window_left, float softcap, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT4_H */
