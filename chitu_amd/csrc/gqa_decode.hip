// GQA / MHA paged decode attention (head_dim 128) for gfx950 -- the non-MLA decode path.
//
// Replaces (reference, read-only) the third-party call behind
//   FlashAttnBackend.attn_with_kvcache   chitu/attn_backend.py:208-243  (flash_attn.flash_attn_with_kvcache)
//   contract text                        chitu/attn_backend.py:92-164
// as used by Attention.decode_forward_paged (chitu/models/model.py:167-198, model_hf_llama.py:218-252):
//   out[b,h,:] = softmax_t(scale * q[b,h,:] . K[t, h/g, :]) . V[t, h/g, :],  t < seqlens[b]
// over a paged cache [pages, page_size, kv_heads, 128] (page_size % 16 == 0; the reference uses 256).
// The in-place append of this step's k/v (contract :108-115) is chitu_hip_append_paged_kv, run first.
//
// One wave per (KV split, sequence, kv head); the q heads of the group (<= 16) ride in the MFMA N
// dimension.  Per 16 tokens: K rows are loaded straight into A fragments (16 B per lane, 64 B
// contiguous per token per instruction), S^T = K Q^T by 4 x v_mfma_f32_16x16x32_bf16, so a lane holds
// S[4 tokens][one head] and P is already the A fragment of v_mfma_f32_16x16x16_bf16; V's 16 x 128
// sub-tile goes through a wave-private 4 KB LDS slab and is read back transposed
// (ds_read_b64_tr_b16).  Wave-local online softmax with deferred max; splits merged by a second tiny
// kernel (LSE), like the MLA path.
//
// The kernel itself lives in gqa_decode_tile.h: chitu_hip_gqa_decode_kv_fp8 (gqa_decode_kv_fp8.hip) is the same kernel over fp8 rows.
#include "gqa_decode_tile.h"

namespace chitu {

// out[b,h,:] = sum_s w_s part_o[b,h,s,:] / sum_s w_s, w_s = exp(lse_s - max lse).  grid (batch*heads); one wave.
// Nothing in here is a chain of dependent loads: the lse values are read one per lane, the weights travel by
// shuffle, and the rows of part_o are read with data-independent addresses (8 in flight per lane); the two
// halves of the wave take the even and the odd splits and are added at the end.
__global__ __launch_bounds__(64) void gqa_merge_kernel(const float* __restrict__ part_o,
                                                       const float* __restrict__ part_lse,
                                                       bf16_t* __restrict__ out, int num_splits) {
    const int64_t bh = blockIdx.x;
    const int lane = threadIdx.x, half = lane >> 5, col = (lane & 31) * 4;
    const float* lse = part_lse + bh * num_splits;
    float ls[4], m = -INFINITY;  // num_splits <= 256
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int s = lane + 64 * i;
        ls[i] = s < num_splits ? lse[s] : -INFINITY;
        m = __builtin_fmaxf(m, ls[i]);
    }
    m = wave_reduce_max(m);
    float w[4], wsum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = ls[i] == -INFINITY ? 0.f : __expf(ls[i] - m);
        wsum += w[i];
    }
    wsum = wave_reduce_sum(wsum);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* rows = part_o + bh * num_splits * kHd + col;
    // The trip count is the SAME for both halves (s0 is wave-uniform, the half enters through `s`): the __shfl below
    // is a ds_bpermute, which returns 0 for a source lane that has left the loop, so a half that exits one
    // iteration early (num_splits % 16 == 1) would drop the weights the other half still fetches from its lanes.
    for (int s0 = 0; s0 < num_splits; s0 += 16) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(rows + (int64_t)min(s0 + half + 2 * u, num_splits - 1) * kHd);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int s = s0 + half + 2 * u;  // uniform per half
            const float ws_all = s < 64 ? w[0] : s < 128 ? w[1] : s < 192 ? w[2] : w[3];
            const float ws = __shfl(ws_all, s & 63, 64);
            if (s < num_splits && ws > 0.f) {  // an empty split's row is never used (it may hold anything)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += ws * v[u][i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += __shfl_xor(acc[i], 32, 64);
    if (half) return;
    const float inv = wsum > 0.f ? 1.0f / wsum : 0.f;
    i32x2 o2;
    o2[0] = (int)f32x2_to_bf16x2(acc[0] * inv, acc[1] * inv);
    o2[1] = (int)f32x2_to_bf16x2(acc[2] * inv, acc[3] * inv);
    *reinterpret_cast<i32x2*>(out + bh * kHd + col) = o2;
}

void launch_gqa_merge(const float* part_o, const float* part_lse, bf16_t* out, int64_t bh, int num_splits, hipStream_t st) {
    hipLaunchKernelGGL(gqa_merge_kernel, dim3((unsigned)bh), dim3(64), 0, st, part_o, part_lse, out, num_splits);
}

}  // namespace chitu

extern "C" int chitu_hip_gqa_decode(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h,
                                    const void* k_cache, const void* v_cache, int64_t num_pages,
                                    int32_t page_size, int32_t kv_heads, const int32_t* block_table,
                                    int32_t table_stride, const int32_t* seqlens, float softmax_scale,
                                    void* out_bf16, int32_t batch, int32_t q_heads, int32_t head_dim,
                                    int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    return chitu::gqa_decode_launch<false>(q_bf16, q_stride_b, q_stride_h, k_cache, v_cache, num_pages, page_size, kv_heads,
                                           block_table, table_stride, seqlens, softmax_scale, out_bf16, batch, q_heads, head_dim,
                                           num_splits, workspace, workspace_bytes, -1, 0.0f, stream);
}

// Sliding-window / soft-capped form (gqa_decode_tile.h, kWin): FlashAttnBackend.attn_with_kvcache's window_size = (W, 0) and
// softcap (chitu/attn_backend.py:208-243, contract :92-164; RefAttnBackend._attention :294-392 is the arithmetic).
extern "C" int chitu_hip_gqa_decode_window(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h,
                                           const void* k_cache, const void* v_cache, int64_t num_pages,
                                           int32_t page_size, int32_t kv_heads, const int32_t* block_table,
                                           int32_t table_stride, const int32_t* seqlens, float softmax_scale,
                                           void* out_bf16, int32_t batch, int32_t q_heads, int32_t head_dim,
                                           int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                           int32_t window_left, float softcap, void* stream) {
    return chitu::gqa_decode_launch<false>(q_bf16, q_stride_b, q_stride_h, k_cache, v_cache, num_pages, page_size, kv_heads,
                                           block_table, table_stride, seqlens, softmax_scale, out_bf16, batch, q_heads, head_dim,
                                           num_splits, workspace, workspace_bytes, window_left, softcap, stream);
}
