/* chitu_hip_ext2.h -- the second set of additions to the C ABI of libchitu_hip.so.
 *
 * chitu_hip.h is frozen at ABI version 13 (94 entry points) and chitu_hip_ext.h at CHITU_HIP_EXT_VERSION 1 (three entries):
 * bindings and checks pin the text of both.  Entry points added after them live here, are exported from the same library
 * under the prefix chitu_ext2_, and follow chitu_hip.h's conventions: device pointers owned by the caller, launches enqueued
 * on `stream` (hipGraph-capturable), return value 0 = enqueued, <0 = argument error (CHITU_ERR_BAD_ARG -1,
 * CHITU_ERR_UNSUPPORTED -2), >0 = hipError_t.  Additive only: an entry, once declared here, keeps its argument list;
 * CHITU_HIP_EXT2_VERSION counts the additions.
 */
#ifndef CHITU_HIP_EXT2_H
#define CHITU_HIP_EXT2_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT2_VERSION 1  /* 1: the two entries of the continued MLA prefill (DeepSeek-V3) */

/* ---- continued prefill over the paged latent KV cache (MLA) -----------------------------------------------------------
 * New: no reference counterpart (the reference prefills a prompt in one piece).  A chunk of n new tokens behind P cached ones
 * attends over all L = P + n latent rows of its sequence.  Two launches: the rows are first gathered out of the pages into one
 * contiguous bf16 buffer, then the flash prefill kernel of chitu_hip_mla_prefill_flash runs with separate query and key
 * extents.  kv_lora_rank 512 and rope_dim 64 only (anything else: CHITU_ERR_UNSUPPORTED); every base pointer 16-byte
 * aligned; a null pointer, a misaligned pointer or a bad stride: CHITU_ERR_BAD_ARG; nothing is launched for zero rows.
 *   chitu_ext2_mla_kv_gather               new: no reference counterpart.  cache: the pages of one layer, contiguous,
 *     [num_pages, page_size, 576] bf16 (cache_fp8 = 0) or [num_pages, page_size, 656] bytes (cache_fp8 = 1, the rows of
 *     chitu_hip_mla_kv_quant_fp8).  cu_seqlens_k [n_seq + 1] int32, non-decreasing, cu_seqlens_k[0] = 0: output row
 *     cu_seqlens_k[s] + t, t < L_s, is row t of sequence s, read from page block_table[s * table_stride + t / page_size] at
 *     row t % page_size -- copied (bf16) or widened exactly as chitu_hip_mla_kv_dequant_fp8 widens it (fp8) -- and written
 *     to out_bf16 + row * out_stride (elements; >= 576, a multiple of 8).  total_rows = cu_seqlens_k[n_seq], known to the
 *     host: the grid.  Any page_size >= 1.  A table entry outside [0, num_pages), or a position beyond table_stride pages,
 *     refuses nothing and writes a row of zeros (the range rule of chitu_hip_gqa_qkv_post); rows of a page at or beyond L_s
 *     and pages that no sequence references are never read; output rows at or beyond cu_seqlens_k[n_seq] are not written.
 *   chitu_ext2_mla_prefill_flash_continue  new: no reference counterpart.  chitu_hip_mla_prefill_flash with seqlen_q !=
 *     seqlen_k, the causal mask aligned bottom-right (the contract of chitu/attn_backend.py:39-90): sequence s has
 *     n_s = cu_seqlens_q[s + 1] - cu_seqlens_q[s] query rows in q / out and L_s = cu_seqlens_k[s + 1] - cu_seqlens_k[s] >= n_s
 *     key rows in kv_bf16 (stride kv_stride_t elements); query i is position L_s - n_s + i and sees keys 0 .. L_s - n_s + i.
 *     max_seqlen_q >= every n_s.  q [sum n, heads, 576] with strides in elements (multiples of 8), out [sum n, heads, 512]
 *     contiguous.  With L_s = n_s for every s the output equals chitu_hip_mla_prefill_flash's bit for bit; otherwise every
 *     row at a position >= 8 * ceil((L_s - n_s) / 8) equals that row of the whole-sequence call bit for bit, and the fewer
 *     than 8 rows in front of it agree within the attention bar.  L_s < n_s is outside the contract: the last L_s query rows
 *     are computed as if n_s were L_s, the first n_s - L_s output rows are not written, nothing else is touched. */
int chitu_ext2_mla_kv_gather(const void* cache, int32_t cache_fp8, int64_t num_pages, int32_t page_size,
                             const int32_t* block_table, int32_t table_stride, const int32_t* cu_seqlens_k,
                             int32_t n_seq, int64_t total_rows, void* out_bf16, int64_t out_stride,
                             int32_t kv_lora_rank, int32_t rope_dim, void* stream);
int chitu_ext2_mla_prefill_flash_continue(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h,
                                          const void* kv_bf16, int64_t kv_stride_t, const int32_t* cu_seqlens_q,
                                          const int32_t* cu_seqlens_k, int32_t n_seq, int32_t max_seqlen_q,
                                          float softmax_scale, void* out_bf16, int32_t heads, int32_t kv_lora_rank,
                                          int32_t rope_dim, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT2_H */
