/* chitu_hip_ext3.h -- the third set of additions to the C ABI of libchitu_hip.so.
 *
 * chitu_hip.h is frozen at ABI version 13, chitu_hip_ext.h at CHITU_HIP_EXT_VERSION 1 and chitu_hip_ext2.h at
 * CHITU_HIP_EXT2_VERSION 1: bindings and checks pin the text of all three.  Entry points added after them live here, are
 * exported from the same library under the prefix chitu_ext3_, and follow chitu_hip.h's conventions: device pointers owned by
 * the caller, launches enqueued on `stream` (hipGraph-capturable), return value 0 = enqueued, <0 = argument error
 * (CHITU_ERR_BAD_ARG -1, CHITU_ERR_UNSUPPORTED -2), >0 = hipError_t.  Additive only: an entry, once declared here, keeps its
 * argument list; CHITU_HIP_EXT3_VERSION counts the additions.
 */
#ifndef CHITU_HIP_EXT3_H
#define CHITU_HIP_EXT3_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT3_VERSION 1  /* 1: the two prefill-shaped grouped GEMMs of bf16 experts (Qwen3-MoE) */

/* ---- fused MoE on bf16 experts with bf16 activations, tiled for compute (prefill) ------------------------------------------
 * chitu/fused_moe.py:62-307 fused_moe_kernel with use_fp8_w8a8 = False, for hundreds of tokens and more: the entries of
 * chitu_hip_moe_gemm1_silu_fp8_tiled / chitu_hip_moe_gemm2_fp8_tiled without the scale pointers.  sorted_token_ids,
 * expert_ids, num_tokens_post_pad come from chitu_hip_moe_align_block_size[_mapped] run with block size block_m (64 or 128);
 * a workgroup multiplies block_m sorted slots by 128 weight rows per 64-element K block, fp32 accumulation across the whole
 * contraction, no scales.  Slots >= numel (padding) are never stored, 16-slot groups of padding are not multiplied, and the
 * slots of a block whose expert id is negative (an expert of another rank) are zero-filled.
 *   chitu_ext3_moe_gemm1_silu_bf16_tiled   a [numel / topk, K] bf16 (slot s reads row s / topk), w1 [E, 2 * inter_size, K]
 *     bf16 (gate rows, then up rows) -> h [numel, inter_size] bf16 = bf16(bf16(silu(bf16(g))) * bf16(u)), the rounding points
 *     of chitu_hip_moe_gemm_bf16 with silu = 1.
 *   chitu_ext3_moe_gemm2_bf16_tiled        h [numel, inter_size] bf16, w2 [E, N, inter_size] bf16 -> out [numel, N] bf16 =
 *     bf16(acc * routed weight of the slot) (mul_routed_weight = 0: times 1); topk_weights [numel] of weights_dtype (0 bf16,
 *     1 f16, 2 f32).
 * Checked on the host before anything is launched: a null pointer, a matrix pointer not 16-byte aligned or an index pointer
 * not 4-byte aligned, block_m not 64 or 128, max_mblocks > 65535: CHITU_ERR_BAD_ARG; K % 128, inter_size % 128 or N % 8
 * nonzero, or an expert's weights / the activation matrix of 2 GiB or more: CHITU_ERR_UNSUPPORTED; numel == 0 launches
 * nothing and returns 0. */
int chitu_ext3_moe_gemm1_silu_bf16_tiled(const void* a_bf16, const void* w1_bf16, const int32_t* sorted_token_ids,
    const int32_t* expert_ids, const int32_t* num_tokens_post_pad, void* h_bf16, int64_t numel, int32_t topk,
    int64_t inter_size, int64_t K, int64_t max_mblocks, int32_t block_m, void* stream);
int chitu_ext3_moe_gemm2_bf16_tiled(const void* h_bf16, const void* w2_bf16, const int32_t* sorted_token_ids,
    const int32_t* expert_ids, const int32_t* num_tokens_post_pad, const void* topk_weights, int weights_dtype,
    int32_t mul_routed_weight, void* out_bf16, int64_t numel, int64_t N, int64_t inter_size, int64_t max_mblocks,
    int32_t block_m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT3_H */
