// Multi-token MLA (absorb mode) paged decode attention over the FP8 latent KV cache: q_len = T <= 8 query tokens per sequence.
//
// chitu_hip_mla_decode_multi's contract, grid, pairing of query tokens and split logic (mla_decode_multi.hip) with the cache
// holding 656-byte rows; the staging, its layout and the widening pass are mla_decode_kv_fp8_kernel's (mla_decode_kv_fp8.hip: ONE
// bf16 tile image, TWO fp8 staging buffers), and once a tile's image is complete it is multiplied once per token of the pair by
// mla_tile_step, as in the bf16 entry.  The widening is exact, so the output and the workspace are bit-identical to
// chitu_hip_mla_decode_multi on the dequantised cache, and at q_len == 1 to chitu_hip_mla_decode_kv_fp8
// (tests/test_gpu_mla_multi.py).  The DMA's row clamp uses L, the longest length of the pair.
#include "common.h"
#include "lds_dma.h"
#include "mla_decode_tile.h"
#include "mla_kv_fp8.h"

namespace chitu {

// (the staging constants of mla_decode_kv_fp8.hip)
constexpr int kRowChunks = kKvFp8Row / 16;       // 41
constexpr int kStageU = kTile * kKvFp8Row;       // 41984 = 41 pieces of 1 KiB
constexpr int kStagePieces = kStageU / 1024;     // 41: wave w requests pieces w, w + 4, ...
constexpr int kStageChunks = kStageU / 16;       // 2624
constexpr int kStages = 2;                       // staging buffers: tile t + 1 lands while tile t is widened and multiplied

// grid (num_splits, batch, ceil(heads/16) * ceil(T/2)); block 256
__global__ __launch_bounds__(256, 1) void mla_decode_multi_kv_fp8_kernel(
    const bf16_t* __restrict__ q_nope, int64_t qn_sb, int64_t qn_st, int64_t qn_sh, const bf16_t* __restrict__ q_pe,
    int64_t qp_sb, int64_t qp_st, int64_t qp_sh, const uint8_t* __restrict__ cache, int64_t num_pages, int page_size,
    const int32_t* __restrict__ block_table, int table_stride, const int32_t* __restrict__ seqlens,
    float scale, bf16_t* __restrict__ part_o, float* __restrict__ part_lse, bf16_t* __restrict__ out,
    int H, int T, int num_splits) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* kv_lds = smem;                                               // [64][kRowU] the bf16 image
    uint8_t* stage0 = smem + kTileU;                                      // [kStages][64][656] fp8 rows as they are cached
    bf16_t* p_lds = reinterpret_cast<bf16_t*>(smem + kTileU + kStages * kStageU);   // [16][72]
    float* red_max = reinterpret_cast<float*>(smem + kTileU + kStages * kStageU + 16 * kPStride * 2);  // [4][16]
    float* red_sum = red_max + 64;                                        // [4][16]
    int* pages_lds = reinterpret_cast<int*>(red_sum + 64);                // [kMaxTilesLds]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int split = blockIdx.x, b = blockIdx.y;
    const MlaPair pr = mla_pair_of_block((int)blockIdx.z, T);
    const int h0 = pr.hb * 16;
    const int32_t* tbl = block_table + (int64_t)b * table_stride;
    const int max_page_idx = table_stride - 1;
    const int L = max(seqlens[b], 0);  // a corrupt negative length is an empty sequence
    const int Lt0 = L - T + pr.t0 + 1;                    // keys token t0 sees (<= 0: none)
    const int Lt1 = pr.two ? L - T + pr.t1 + 1 : 0;       // the pair's second token; an odd T's last workgroup has none
    const int n_tiles = (L + kTile - 1) / kTile;
    const int tile0 = (int)((unsigned)n_tiles * (unsigned)split / (unsigned)num_splits);
    const int tile1 = (int)((unsigned)n_tiles * (unsigned)(split + 1) / (unsigned)num_splits);
    if (tile0 >= tile1) {
        mla_publish_empty_split(part_o, part_lse, out, b * T + pr.t0, H, h0, split, num_splits, tid);
        if (pr.two) mla_publish_empty_split(part_o, part_lse, out, b * T + pr.t1, H, h0, split, num_splits, tid);
        return;
    }
    const bool pages_in_lds = (tile1 - tile0) <= kMaxTilesLds;
    auto page_src = [&](int64_t page, int t0) -> const uint8_t* {
        if (page < 0 || page >= num_pages) page = 0;  // corrupt table: stay in bounds
        return cache + (page * page_size + (t0 % page_size)) * (int64_t)kKvFp8Row;
    };
    auto tile_src = [&](int tile) -> const uint8_t* {
        const int t0 = tile * kTile;
        return page_src(pages_in_lds && tile > tile0 ? pages_lds[tile - tile0] : tbl[min(t0 / page_size, max_page_idx)], t0);
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
    // rows past the sequence end (L, the longest length of the pair) re-read the tile's last valid row
    auto issue = [&](const uint8_t* src, int valid, int buf) {
        const uint8_t* sb = uniform_ptr(src);
#pragma unroll
        for (int i = 0; i < 11; ++i)
            if (wave + 4 * i < kStagePieces)
                glds16_sbase<true>(sb, (uint32_t)(min(prow[i], valid - 1) * kKvFp8Row) + poff[i], lds_stage + (uint32_t)(buf * kStageU + (wave + 4 * i) * 1024));
    };
    issue(tile_src(tile0), min(kTile, L - tile0 * kTile), 0);
    {   // Q of both tokens (2 x 16 heads x 576) into the image, token k's heads as rows 16 k .. 16 k + 15 (kv_swz reads bits 1 and
        // 3 of the row: both blocks swizzle alike); every wave then reads all of it back
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int t = k ? pr.t1 : pr.t0;  // (an odd T's last workgroup reads its one token twice and uses it once)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int c = tid + i * 256;
                if (c < 16 * 72) {
                    const int row = c / 72, col = c % 72;
                    const int h = min(h0 + row, H - 1);
                    const bf16_t* src = col < 64 ? q_nope + b * qn_sb + t * qn_st + h * qn_sh + col * 8
                                                 : q_pe + b * qp_sb + t * qp_st + h * qp_sh + (col - 64) * 8;
                    mla_q_store(kv_lds + k * 16 * kRowU, c, *reinterpret_cast<const i32x4*>(src));
                }
            }
        }
    }
    if (pages_in_lds && tile1 - tile0 > 1) {  // page ids of the following tiles
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (tid + i * 256 < tile1 - tile0)
                pages_lds[tid + i * 256] = tbl[min(((tile0 + tid + i * 256) * kTile) / page_size, max_page_idx)];
    }

    MlaTokenState s0, s1;
    mla_token_init(s0);
    mla_token_init(s1);
    const MlaFrag frag = mla_frag(wave, j, g);
    // the widening pass: which of its two image chunks a lane stores first (the layout note of mla_decode_kv_fp8.hip)
    const int odd_first = (lane >> 4) & 1;

    __syncthreads();  // Q and the page list are visible
    mla_q_frags(s0.qf, kv_lds, j, g);
    mla_q_frags(s1.qf, kv_lds + 16 * kRowU, j, g);

    for (int tile = tile0; tile < tile1; ++tile) {
        const int buf = (tile - tile0) & (kStages - 1);
        glds_wait_all();   // this wave's pieces of the tile
        __syncthreads();   // everyone's; the image (Q, or the previous tile), the other staging buffer (widened one tile ago)
                           // and the softmax exchange areas are free
        if (tile + 1 < tile1) issue(tile_src(tile + 1), min(kTile, L - (tile + 1) * kTile), buf ^ 1);
        const uint8_t* stage = stage0 + buf * kStageU;
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // the codes: chunk p (16 codes) of row r -> image chunks 2 p, 2 p + 1; 32 lanes per row
            const int c = tid + i * 256, row = c >> 5, pos = c & 31;
            const uint8_t* srow = stage + row * kKvFp8Row;
            const i32x4 raw = *reinterpret_cast<const i32x4*>(srow + pos * 16);
            const float s = *reinterpret_cast<const float*>(srow + kKvFp8ScaleOff + (pos >> 3) * 4);
            // (the halves are exchanged as codes, 4 selects, not as bf16, 8)
            const i32x4 first = kv_fp8_widen8((uint32_t)(odd_first ? raw[2] : raw[0]), (uint32_t)(odd_first ? raw[3] : raw[1]), s);
            const i32x4 second = kv_fp8_widen8((uint32_t)(odd_first ? raw[0] : raw[2]), (uint32_t)(odd_first ? raw[1] : raw[3]), s);
            uint8_t* img = kv_lds + row * kRowU;
            const int sw = kv_swz(row);
            *reinterpret_cast<i32x4*>(img + (((2 * pos + odd_first) ^ sw) << 4)) = first;
            *reinterpret_cast<i32x4*>(img + (((2 * pos + 1 - odd_first) ^ sw) << 4)) = second;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {  // the rope part: 8 chunks of a row, copied to image chunks 64 .. 71
            const int c = tid + i * 256, row = c >> 3, pos = c & 7;
            *reinterpret_cast<i32x4*>(kv_lds + row * kRowU + (((64 + pos) ^ kv_swz(row)) << 4)) =
                *reinterpret_cast<const i32x4*>(stage + row * kKvFp8Row + kKvFp8RopeOff + pos * 16);
        }
        __syncthreads();   // the image is complete
        mla_pair_tile_steps(kv_lds, frag, tile, Lt0, Lt1, scale, p_lds, red_max, red_sum, s0, s1, wave, j, g);
    }

    mla_token_epilogue(s0, part_o, part_lse, out, reinterpret_cast<bf16_t*>(kv_lds), b * T + pr.t0, H, h0, split, num_splits, tid, wave, j, g);
    if (pr.two)
        mla_token_epilogue(s1, part_o, part_lse, out, reinterpret_cast<bf16_t*>(kv_lds), b * T + pr.t1, H, h0, split, num_splits, tid, wave, j, g);
}

}  // namespace chitu

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
    if (batch == 0) return CHITU_OK;
    const int32_t rows = batch * q_len;
    bf16_t* part_o = nullptr;
    float* part_lse = nullptr;
    if (num_splits > 1)
        if (int rc = mla_decode_carve_workspace(workspace, workspace_bytes, rows, heads, num_splits, &part_o, &part_lse)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the opt-in above 64 KB of dynamic LDS is set on every call (per device and cheap, as in mla_decode.hip)
    const size_t lds = kTileU + kStages * kStageU + 16 * kPStride * 2 + 2 * 64 * sizeof(float) + kMaxTilesLds * sizeof(int);
    (void)hipFuncSetAttribute((const void*)mla_decode_multi_kv_fp8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid((unsigned)num_splits, (unsigned)batch, (unsigned)(((heads + 15) / 16) * ((q_len + 1) / 2)));
    hipLaunchKernelGGL(mla_decode_multi_kv_fp8_kernel, grid, dim3(256), lds, st, (const bf16_t*)q_nope, qn_stride_b, qn_stride_t,
                       qn_stride_h, (const bf16_t*)q_pe, qp_stride_b, qp_stride_t, qp_stride_h, (const uint8_t*)kv_cache, num_pages,
                       (int)page_size, block_table, (int)table_stride, seqlens, softmax_scale, part_o, part_lse, (bf16_t*)out_bf16,
                       (int)heads, (int)q_len, (int)num_splits);
    if (num_splits > 1 && out_bf16) launch_mla_merge(part_o, part_lse, (bf16_t*)out_bf16, (int64_t)rows * heads, (int)num_splits, st);
    CHITU_RETURN_LAUNCH_STATUS();
}
