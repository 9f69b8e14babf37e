// Gather of the paged latent KV cache into contiguous bf16 rows (new: no reference counterpart): the first of the two launches
// of the continued MLA prefill (chitu_hip_ext2.h).  mla_prefill_flash_pipe_kernel streams its keys by LDS-DMA from rows a fixed
// stride apart; instead of teaching that kernel the block table, every sequence's L rows are copied out of the pages once per
// layer -- L * 1152 bytes written, at most that read, against L * n * 2 * (576 + 512) * heads flops of attention behind it.
//
//   out[cu_seqlens_k[s] + t, :576] = row t of sequence s = cache[table[s][t / page_size]][t % page_size],   t < L_s
//
// bf16 pages are copied: 72 chunks of 16 bytes per row.  fp8 pages (656-byte rows, mla_kv_fp8.h) are widened by the rule of
// mla_kv_dequant_fp8_kernel -- lane i takes codes 8 i .. 8 i + 7 and their group's scale to one 16-byte chunk (kv_fp8_widen8:
// exact), lanes 0 .. 7 copy the eight rope chunks -- so the buffer holds, bit for bit, what chitu_hip_mla_kv_dequant_fp8 writes.
// One wave per output row, four rows per workgroup; the row's sequence by binary search over cu_seqlens_k (wave-uniform).
// Only rows t < L_s of pages the table names within ceil(L_s / page_size) entries are read; a table entry outside
// [0, num_pages) or a position beyond the table's width gives a row of zeros (the range rule of chitu_hip_gqa_qkv_post).
#include "common.h"
#include "mla_kv_fp8.h"
#include "chitu_hip_ext2.h"

namespace chitu {

constexpr int kGatherRow = 576;  // bf16 elements of an output row: 72 chunks of 16 bytes

template <bool kFp8>
__global__ __launch_bounds__(256) void mla_kv_gather_kernel(const uint8_t* __restrict__ cache, int64_t num_pages, int page_size,
                                                            const int32_t* __restrict__ table, int table_stride,
                                                            const int32_t* __restrict__ cu_k, int n_seq, int64_t total_rows,
                                                            bf16_t* __restrict__ out, int64_t out_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= total_rows || row >= (int64_t)cu_k[n_seq]) return;
    // the last s with cu_k[s] <= row: zero-length sequences (equal neighbours) are stepped over
    int lo = 0, hi = n_seq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)cu_k[mid] <= row) lo = mid;
        else hi = mid;
    }
    const int64_t t = row - (int64_t)cu_k[lo];
    bf16_t* dst = out + row * out_stride;
    const int64_t pidx = t / page_size;
    int64_t page = -1;
    if (t >= 0 && pidx < table_stride) page = table[(int64_t)lo * table_stride + pidx];
    if (page < 0 || page >= num_pages) {
        const i32x4 z = {0, 0, 0, 0};
        *reinterpret_cast<i32x4*>(dst + lane * 8) = z;
        if (lane < 8) *reinterpret_cast<i32x4*>(dst + 512 + lane * 8) = z;
        return;
    }
    const int64_t src_row = page * page_size + (t % page_size);
    if constexpr (kFp8) {
#pragma clang fp contract(off)
        const uint8_t* src = cache + src_row * (int64_t)kKvFp8Row;
        const i32x2 codes = *reinterpret_cast<const i32x2*>(src + lane * 8);
        const float s = *reinterpret_cast<const float*>(src + kKvFp8ScaleOff + (lane >> 4) * 4);
        i32x4 rope;
        if (lane < 8) rope = *reinterpret_cast<const i32x4*>(src + kKvFp8RopeOff + lane * 16);
        *reinterpret_cast<i32x4*>(dst + lane * 8) = kv_fp8_widen8((uint32_t)codes[0], (uint32_t)codes[1], s);
        if (lane < 8) *reinterpret_cast<i32x4*>(dst + 512 + lane * 8) = rope;
    } else {
        const bf16_t* src = reinterpret_cast<const bf16_t*>(cache) + src_row * (int64_t)kGatherRow;
        const i32x4 a = *reinterpret_cast<const i32x4*>(src + lane * 8);
        i32x4 b;
        if (lane < 8) b = *reinterpret_cast<const i32x4*>(src + 512 + lane * 8);
        *reinterpret_cast<i32x4*>(dst + lane * 8) = a;
        if (lane < 8) *reinterpret_cast<i32x4*>(dst + 512 + lane * 8) = b;
    }
}

}  // namespace chitu

extern "C" int chitu_ext2_mla_kv_gather(const void* cache, int32_t cache_fp8, int64_t num_pages, int32_t page_size,
                                        const int32_t* block_table, int32_t table_stride, const int32_t* cu_seqlens_k,
                                        int32_t n_seq, int64_t total_rows, void* out_bf16, int64_t out_stride,
                                        int32_t kv_lora_rank, int32_t rope_dim, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(cache && block_table && cu_seqlens_k && out_bf16 && (cache_fp8 == 0 || cache_fp8 == 1));
    CHITU_REQUIRE(num_pages >= 0 && page_size >= 1 && table_stride >= 1 && n_seq >= 0 && total_rows >= 0 && total_rows < (1ll << 31));
    if (kv_lora_rank != 512 || rope_dim != 64) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(out_stride >= kGatherRow && out_stride % 8 == 0);
    CHITU_REQUIRE((((uintptr_t)cache | (uintptr_t)out_bf16) & 15) == 0);  // rows are 72 (bf16) / 41 (fp8) chunks of 16 bytes
    if (n_seq == 0 || total_rows == 0) return CHITU_OK;
    const dim3 grid((unsigned)((total_rows + 3) / 4));
    if (cache_fp8)
        hipLaunchKernelGGL(mla_kv_gather_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)cache, num_pages,
                           (int)page_size, block_table, (int)table_stride, cu_seqlens_k, (int)n_seq, total_rows, (bf16_t*)out_bf16,
                           out_stride);
    else
        hipLaunchKernelGGL(mla_kv_gather_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)cache, num_pages,
                           (int)page_size, block_table, (int)table_stride, cu_seqlens_k, (int)n_seq, total_rows, (bf16_t*)out_bf16,
                           out_stride);
    CHITU_RETURN_LAUNCH_STATUS();
}
