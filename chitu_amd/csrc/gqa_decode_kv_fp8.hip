// GQA / MHA paged decode attention over the fp8 K / V cache (new: no reference counterpart).
//
// chitu_hip_gqa_decode's argument list, grid, split arithmetic, workspace layout, empty-split LSE = -inf, merge kernel and
// limits (group <= 16, page_size % 16 == 0, num_splits <= 256); k_cache / v_cache are the byte rows [pages, page, Hkv, 144] of
// gqa_kv_fp8.hip, q stays bf16.  The kernel is gqa_decode_kernel<true> of gqa_decode_tile.h: the fp8 rows are widened in
// registers into the bf16 kernel's own A fragments and V slab image, so the output is bit-identical to chitu_hip_gqa_decode on
// the dequantised cache at the same num_splits.  Bytes past a sequence's length may hold anything (NaN codes and NaN scales
// included): K re-reads the last valid row, V rows past the end are never loaded.
#include "gqa_decode_tile.h"

extern "C" int chitu_hip_gqa_decode_kv_fp8(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h,
                                           const void* k_cache, const void* v_cache, int64_t num_pages,
                                           int32_t page_size, int32_t kv_heads, const int32_t* block_table,
                                           int32_t table_stride, const int32_t* seqlens, float softmax_scale,
                                           void* out_bf16, int32_t batch, int32_t q_heads, int32_t head_dim,
                                           int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
    return chitu::gqa_decode_launch<true>(q_bf16, q_stride_b, q_stride_h, k_cache, v_cache, num_pages, page_size, kv_heads,
                                          block_table, table_stride, seqlens, softmax_scale, out_bf16, batch, q_heads, head_dim,
                                          num_splits, workspace, workspace_bytes, -1, 0.0f, stream);
}

// The same over a sliding window and / or with a soft cap: chitu_hip_gqa_decode_window's arguments and rules on the fp8 rows
// (the reference's window_size / softcap of attn_with_kvcache, chitu/attn_backend.py:92-164).  Bytes before the window are as
// free as the bytes past the end: V rows there are staged as code 0 x scale 1, K re-reads the window's first row.
extern "C" int chitu_hip_gqa_decode_kv_fp8_window(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h,
                                                  const void* k_cache, const void* v_cache, int64_t num_pages,
                                                  int32_t page_size, int32_t kv_heads, const int32_t* block_table,
                                                  int32_t table_stride, const int32_t* seqlens, float softmax_scale,
                                                  void* out_bf16, int32_t batch, int32_t q_heads, int32_t head_dim,
                                                  int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                                  int32_t window_left, float softcap, void* stream) {
    return chitu::gqa_decode_launch<true>(q_bf16, q_stride_b, q_stride_h, k_cache, v_cache, num_pages, page_size, kv_heads,
                                          block_table, table_stride, seqlens, softmax_scale, out_bf16, batch, q_heads, head_dim,
                                          num_splits, workspace, workspace_bytes, window_left, softcap, stream);
}
