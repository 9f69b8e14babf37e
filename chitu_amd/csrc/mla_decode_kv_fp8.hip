// MLA (absorb mode) paged decode attention over the FP8 latent KV cache (new: no reference counterpart).
//
// chitu_hip_mla_decode's and chitu_hip_mla_decode_multi's contracts, grids, pairing of query tokens and split logic (mla_decode.hip:
// kTok = 1 and 2) with the cache holding 656-byte rows
// (mla_kv_fp8.hip: 512 e4m3 codes | four power-of-two fp32 scales | 64 bf16 rope values): 0.569 of the bytes a bf16 row streams.
// q stays bf16.  The latent is widened to bf16 as code * 2^e, which is exact, so the tile the MFMAs read holds the very bits
// chitu_hip_mla_kv_dequant_fp8 would have written to a bf16 cache; the tile step and the epilogue behind it are the ones
// mla_decode_kernel runs (mla_decode_tile.h), so the output is bit-identical to chitu_hip_mla_decode on the dequantised cache at
// the same num_splits (tests/test_gpu_mla_kv_fp8.py), chitu_hip_mla_decode_multi_kv_fp8's to chitu_hip_mla_decode_multi's, and at
// q_len == 1 to chitu_hip_mla_decode_kv_fp8's (tests/test_gpu_mla_multi.py).
//
// How bytes move.  LDS holds ONE bf16 tile image (mla_decode_tile.h: [64][1152 B], chunk c of row r at c ^ kv_swz(r)) and TWO
// fp8 staging buffers [64][656 B] = 41 KiB each: 73.7 + 2 x 42.0 KB + P, the softmax exchange and the page ids = 158.75 KB of
// the CU's 160.  (Two images do not fit beside a staging buffer.)  Per tile:
//   wait for the tile's DMA | barrier | request the NEXT tile into the other staging buffer | widen staging -> image | barrier
//   | multiply
// so a tile's bytes are in flight while the previous tile is widened and multiplied, as in the bf16 kernel; the price of the
// format is the widening pass (10 ds_read_b128 + 18 ds_write_b128 and ~300 VALU instructions per thread and tile) and one more
// barrier per tile.
//
// Staging layout: the 41 16-byte chunks of a row back to back, rows back to back -- 2624 chunks = exactly 41 DMA pieces of
// 1 KiB (lds_dma.h), piece n lane i = staging chunk 64 n + i = (row q / 41, chunk q % 41).  No swizzle.  The only reader is the
// widening pass: 32 lanes take the 32 code chunks of one row (a ds_read_b128 group of 16 lanes reads chunks
// of one row: 16 distinct slots of the 256-byte bank row wherever the row starts), 8 lanes the 8 rope chunks of one row (a
// group spans 2 rows of 656 = 2 * 256 + 144 bytes: 2-way, 2 of the pass's 10 reads).  Its writes into the image are the side
// that matters: code chunk p becomes image chunks 2 p and 2 p + 1, and the 16 lanes of a ds_write_b128 group hold 16 values of
// p, i.e. only 8 distinct even slots.  So the lanes 16-31 and 48-63 store their ODD chunk first: every group then covers 16
// distinct slots (the image's XOR swizzle permutes slots inside a row and keeps that).  Checked for every group, with the
// coverage of the image, in tests/test_mla_kv_fp8_host.py.
#include "common.h"
#include "lds_dma.h"
#include "mla_decode_tile.h"
#include "mla_kv_fp8.h"

namespace chitu {

constexpr int kRowChunks = kKvFp8Row / 16;       // 41
constexpr int kStageU = kTile * kKvFp8Row;       // 41984 = 41 pieces of 1 KiB
constexpr int kStagePieces = kStageU / 1024;     // 41: wave w requests pieces w, w + 4, ...
constexpr int kStageChunks = kStageU / 16;       // 2624
constexpr int kStages = 2;                       // staging buffers: tile t + 1 lands while tile t is widened and multiplied

using MlaLdsFp8 = MlaLds<kTileU + kStages * kStageU>;  // one tile image, then the staging buffers

// The widening pass: staging buffer `stage` ([64][656 B], complete and visible) -> the bf16 tile image `image`
__device__ __forceinline__ void mla_kv_fp8_widen_tile(const uint8_t* stage, uint8_t* image, int tid, int lane) {
    const int odd_first = (lane >> 4) & 1;  // which of its two image chunks a lane stores first (see the layout note above)
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // the codes: chunk p (16 codes) of row r -> image chunks 2 p, 2 p + 1; 32 lanes per row
        const int c = tid + i * 256, row = c >> 5, pos = c & 31;
        const uint8_t* srow = stage + row * kKvFp8Row;
        const i32x4 raw = *reinterpret_cast<const i32x4*>(srow + pos * 16);
        const float s = *reinterpret_cast<const float*>(srow + kKvFp8ScaleOff + (pos >> 3) * 4);
        // (the halves are exchanged as codes, 4 selects, not as bf16, 8)
        const i32x4 first = kv_fp8_widen8((uint32_t)(odd_first ? raw[2] : raw[0]), (uint32_t)(odd_first ? raw[3] : raw[1]), s);
        const i32x4 second = kv_fp8_widen8((uint32_t)(odd_first ? raw[0] : raw[2]), (uint32_t)(odd_first ? raw[1] : raw[3]), s);
        uint8_t* img = image + row * kRowU;
        const int sw = kv_swz(row);
        *reinterpret_cast<i32x4*>(img + (((2 * pos + odd_first) ^ sw) << 4)) = first;
        *reinterpret_cast<i32x4*>(img + (((2 * pos + 1 - odd_first) ^ sw) << 4)) = second;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // the rope part: 8 chunks of a row, copied to image chunks 64 .. 71
        const int c = tid + i * 256, row = c >> 3, pos = c & 7;
        *reinterpret_cast<i32x4*>(image + row * kRowU + (((64 + pos) ^ kv_swz(row)) << 4)) =
            *reinterpret_cast<const i32x4*>(stage + row * kKvFp8Row + kKvFp8RopeOff + pos * 16);
    }
}

// kTok = 1: grid (num_splits, batch, ceil(heads / 16)); kTok = 2: grid z = ceil(heads / 16) * ceil(T / 2) (mla_decode.hip); block 256
template <int kTok>
__global__ __launch_bounds__(256, 1) void mla_decode_kv_fp8_kernel(
    const bf16_t* __restrict__ q_nope, MlaQStride<kTok> qn, const bf16_t* __restrict__ q_pe, MlaQStride<kTok> qp,
    const uint8_t* __restrict__ cache, int64_t num_pages, int page_size,
    const int32_t* __restrict__ block_table, int table_stride, const int32_t* __restrict__ seqlens,
    float scale, bf16_t* __restrict__ part_o, float* __restrict__ part_lse, bf16_t* __restrict__ out,
    int H, int num_splits, MlaQLen<kTok> ql) {
    static_assert(kTok == 1 || kTok == 2);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* kv_lds = smem;            // [64][kRowU] the bf16 image
    uint8_t* stage0 = smem + kTileU;   // [kStages][64][656] fp8 rows as they are cached
    bf16_t* p_lds = reinterpret_cast<bf16_t*>(smem + MlaLdsFp8::kP);
    float* red_max = reinterpret_cast<float*>(smem + MlaLdsFp8::kRedMax);
    float* red_sum = reinterpret_cast<float*>(smem + MlaLdsFp8::kRedSum);
    int* pages_lds = reinterpret_cast<int*>(smem + MlaLdsFp8::kPages);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int split = blockIdx.x, b = blockIdx.y, T = mla_q_len(ql);
    const MlaPair pr = mla_pair_of_block<kTok>((int)blockIdx.z, T);
    const int h0 = pr.hb * 16;
    const int row0 = b * T + pr.t0, row1 = b * T + pr.t1;  // the query rows of this workgroup's tokens (kTok = 1: b)
    const int32_t* tbl = block_table + (int64_t)b * table_stride;
    const int max_page_idx = table_stride - 1;
    const int L = max(seqlens[b], 0);  // a corrupt negative length is an empty sequence
    const int Lt0 = L - T + pr.t0 + 1;               // keys token t0 sees (<= 0: none; kTok = 1: L)
    const int Lt1 = pr.two ? L - T + pr.t1 + 1 : 0;  // the pair's second token; an odd T's last workgroup has none
    const MlaSplit sp = mla_split_range(L, split, num_splits);
    const int tile0 = sp.tile0, tile1 = sp.tile1;
    if (tile0 >= tile1) {
        mla_publish_empty_split(part_o, part_lse, out, row0, H, h0, split, num_splits, tid);
        if (kTok == 2 && pr.two) mla_publish_empty_split(part_o, part_lse, out, row1, H, h0, split, num_splits, tid);
        return;
    }
    // (the first tile is requested before the page list is filled: its page id comes from the table)
    auto tile_src = [&](int tile) {
        return mla_tile_src(cache, kKvFp8Row, num_pages, page_size, tbl, max_page_idx, pages_lds, sp.pages_in_lds && tile > tile0, tile, tile0);
    };
    // this wave's pieces of a tile: piece n = wave + 4 i (n < 41); lane's staging chunk 64 n + lane -> (row, byte offset in the row)
    int prow[11];
    uint32_t poff[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) {
        const int qi = min(64 * (wave + 4 * i) + lane, kStageChunks - 1);
        prow[i] = qi / kRowChunks;
        poff[i] = (uint32_t)((qi % kRowChunks) << 4);
    }
    const uint32_t lds_stage = lds_offset_of(stage0);
    // rows past the sequence end (L: the longest length of a pair) re-read the tile's last valid row: finite, and their
    // probabilities are exactly 0
    auto issue = [&](const uint8_t* src, int valid, int buf) {
        const uint8_t* sb = uniform_ptr(src);
#pragma unroll
        for (int i = 0; i < 11; ++i)
            if (wave + 4 * i < kStagePieces)
                glds16_sbase<true>(sb, (uint32_t)(min(prow[i], valid - 1) * kKvFp8Row) + poff[i], lds_stage + (uint32_t)(buf * kStageU + (wave + 4 * i) * 1024));
    };
    issue(tile_src(tile0), min(kTile, L - tile0 * kTile), 0);
    // Q (per token 16 heads x 576): 1152 chunks of 16 B, <= 5 per thread and token, coalesced, into the image, token k's heads as
    // rows 16 k .. 16 k + 15 (kv_swz reads bits 1 and 3 of the row: both blocks swizzle alike); every wave then reads all of it
    // back.  (An odd T's last workgroup reads its one token twice and uses it once.)
#pragma unroll
    for (int k = 0; k < kTok; ++k)
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int c = tid + i * 256;
            if (c < 16 * 72)
                mla_q_store(kv_lds + k * 16 * kRowU, c,
                            *reinterpret_cast<const i32x4*>(mla_q_chunk_src<kTok>(q_nope, qn, q_pe, qp, b, k ? pr.t1 : pr.t0, h0, H, c)));
        }
    mla_fill_page_list(pages_lds, tbl, max_page_idx, page_size, sp, tid);  // the following tiles' page ids

    f32x4 o[kTok][8];
    float m_run[kTok][4], l_run[kTok][4];
#pragma unroll
    for (int k = 0; k < kTok; ++k) {
#pragma unroll
        for (int c = 0; c < 8; ++c) o[k][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            m_run[k][r] = -INFINITY;
            l_run[k][r] = 0.f;
        }
    }
    const MlaFrag frag = mla_frag(wave, j, g);

    __syncthreads();  // Q and the page list are visible
    s16x8 qf[kTok][18];
#pragma unroll
    for (int k = 0; k < kTok; ++k) mla_q_frags(qf[k], kv_lds + k * 16 * kRowU, j, g);

    for (int tile = tile0; tile < tile1; ++tile) {
        const int buf = (tile - tile0) & (kStages - 1);
        glds_wait_all();   // this wave's pieces of the tile
        __syncthreads();   // everyone's; the image (Q, or the previous tile), the other staging buffer (widened one tile ago)
                           // and the softmax exchange areas are free
        if (tile + 1 < tile1) issue(tile_src(tile + 1), min(kTile, L - (tile + 1) * kTile), buf ^ 1);
        mla_kv_fp8_widen_tile(stage0 + buf * kStageU, kv_lds, tid, lane);
        __syncthreads();   // the image is complete
        if constexpr (kTok == 1)
            mla_tile_step(kv_lds, qf[0], frag, min(kTile, L - tile * kTile), scale, p_lds, red_max, red_sum, o[0], m_run[0],
                          l_run[0], wave, j, g);
        else
            mla_pair_tile_steps(kv_lds, frag, tile, Lt0, Lt1, scale, p_lds, red_max, red_sum, qf, o, m_run, l_run, wave, j, g);
    }

    bf16_t* o_lds = reinterpret_cast<bf16_t*>(kv_lds);
    if constexpr (kTok == 2) {
        mla_token_epilogue(o[0], m_run[0], l_run[0], part_o, part_lse, out, o_lds, row0, H, h0, split, num_splits, tid, wave, j, g);
        if (pr.two) mla_token_epilogue(o[1], m_run[1], l_run[1], part_o, part_lse, out, o_lds, row1, H, h0, split, num_splits, tid, wave, j, g);
    } else {  // every key of a non-empty split is one the token sees: 1 / l_run needs no guard
        float inv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) inv[r] = 1.0f / l_run[0][r];
        if (num_splits == 1) {
            mla_store_out_rows(out, o[0], inv, b, H, h0, wave, j, g);
            return;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // the fp32 LSE of the split's rows
            const int h = h0 + g * 4 + r;
            if (wave == 0 && j == 0 && h < H) part_lse[((int64_t)b * H + h) * num_splits + split] = m_run[0][r] + __logf(l_run[0][r]);
        }
        mla_store_partial_rows(part_o, o_lds, o[0], inv, b, H, h0, split, num_splits, tid, wave, j, g);
    }
}

}  // namespace chitu

extern "C" int chitu_hip_mla_decode_kv_fp8(const void* q_nope, int64_t qn_stride_b, int64_t qn_stride_h,
                                           const void* q_pe, int64_t qp_stride_b, int64_t qp_stride_h,
                                           const void* kv_cache, int64_t num_pages, int32_t page_size,
                                           const int32_t* block_table, int32_t table_stride,
                                           const int32_t* seqlens, float softmax_scale, void* out_bf16,
                                           int32_t batch, int32_t heads, int32_t kv_lora_rank,
                                           int32_t rope_dim, int32_t num_splits, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(out_bf16 || num_splits > 1);  // no out: leave the split partials for a fused consumer
    if (int rc = mla_decode_check_args(q_nope, q_pe, kv_cache, block_table, seqlens, batch, heads, num_pages, page_size, table_stride,
                                       kv_lora_rank, rope_dim, num_splits, 1))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    return mla_decode_launch(mla_decode_kv_fp8_kernel<1>, MlaLdsFp8::kBytes, (unsigned)((heads + 15) / 16), batch, batch, heads,
                             num_splits, workspace, workspace_bytes, out_bf16, st,
                             [&](auto kernel, dim3 grid, int lds, bf16_t* part_o, float* part_lse) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, (const bf16_t*)q_nope, MlaQStride<1>{qn_stride_b, qn_stride_h},
                           (const bf16_t*)q_pe, MlaQStride<1>{qp_stride_b, qp_stride_h}, (const uint8_t*)kv_cache, num_pages,
                           (int)page_size, block_table, (int)table_stride, seqlens, softmax_scale, part_o, part_lse,
                           (bf16_t*)out_bf16, (int)heads, (int)num_splits, MlaQLen<1>{});
    });
}

extern "C" int chitu_hip_mla_decode_multi_kv_fp8(const void* q_nope, int64_t qn_stride_b, int64_t qn_stride_t, int64_t qn_stride_h,
                                                 const void* q_pe, int64_t qp_stride_b, int64_t qp_stride_t, int64_t qp_stride_h,
                                                 const void* kv_cache, int64_t num_pages, int32_t page_size,
                                                 const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                                                 float softmax_scale, void* out_bf16, int32_t batch, int32_t q_len, int32_t heads,
                                                 int32_t kv_lora_rank, int32_t rope_dim, int32_t num_splits, void* workspace,
                                                 int64_t workspace_bytes, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(out_bf16 || num_splits > 1);  // no out: leave the split partials for a fused consumer
    if (int rc = mla_decode_multi_check_args(q_nope, q_pe, kv_cache, block_table, seqlens, batch, q_len, heads, num_pages, page_size,
                                             table_stride, kv_lora_rank, rope_dim, num_splits, qn_stride_b, qn_stride_t, qn_stride_h,
                                             qp_stride_b, qp_stride_t, qp_stride_h))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    return mla_decode_launch(mla_decode_kv_fp8_kernel<2>, MlaLdsFp8::kBytes, (unsigned)(((heads + 15) / 16) * ((q_len + 1) / 2)),
                             batch * q_len, batch, heads, num_splits, workspace, workspace_bytes, out_bf16, st,
                             [&](auto kernel, dim3 grid, int lds, bf16_t* part_o, float* part_lse) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, (const bf16_t*)q_nope,
                           MlaQStride<2>{qn_stride_b, qn_stride_t, qn_stride_h}, (const bf16_t*)q_pe,
                           MlaQStride<2>{qp_stride_b, qp_stride_t, qp_stride_h}, (const uint8_t*)kv_cache, num_pages, (int)page_size,
                           block_table, (int)table_stride, seqlens, softmax_scale, part_o, part_lse, (bf16_t*)out_bf16, (int)heads,
                           (int)num_splits, MlaQLen<2>{(int)q_len});
    });
}
