// Multi-token MLA (absorb mode) paged decode attention for gfx950: q_len = T <= 8 query tokens per sequence over the bf16 latent
// cache -- the verify step of speculative decoding (the reference's FlashMLA backend sizes its metadata by mtp_size for it,
// chitu/attn_backend.py:523-527).
//
// seqlens[b] = L counts ALL keys of sequence b, the T rows appended this step included.  Query token t sits at position
// L - T + t and sees keys k <= L - T + t: query (b, t) is chitu_hip_mla_decode (mla_decode.hip) on a row of length
// L_t = L - T + t + 1 over the same table; L_t <= 0 gives zero rows.
//
// Design.  One workgroup (4 waves) = 16 heads x TWO query tokens x one KV split of one sequence; grid (num_splits, batch,
// ceil(heads / 16) * ceil(T / 2)).  Each 64-key tile is staged exactly as mla_decode_kernel stages it (same image, same LDS-DMA,
// same two buffers) and then multiplied once per token of the pair: mla_tile_step (mla_decode_tile.h) with that token's own Q
// fragments, accumulators and running max / sum, and its own valid = min(64, L_t - tile * 64).  A token with valid <= 0 skips
// the step (workgroup-uniform: the barriers inside stay matched).  The pages of a sequence are therefore read ceil(T / 2) times
// instead of T times.  The DMA's row clamp uses L, the longest length: rows in [L_t, L) are real rows whose probability is
// exactly 0 for token t.  The split range [tile0, tile1) comes from ceil(L / 64).
//
// What is bit-identical to what (tests/test_gpu_mla_multi.py):
//   q_len == 1                     output and workspace are the bits of chitu_hip_mla_decode at the same num_splits.
//   num_splits == 1, any T         row (b, t) is the bits of chitu_hip_mla_decode on the expanded problem (batch * T rows, each
//                                  table row repeated T times, lengths L_t).
//   num_splits > 1, all tokens of a sequence ending in one 64-key tile (ceil(L_t / 64) equal for all t): rows and workspace
//                                  partials are the bits of the expanded call -- the split ranges coincide.
//   num_splits > 1, tokens straddling a tile boundary: the earlier tokens' split ranges are those of ceil(L / 64) tiles, not of
//                                  their own single-token launch (ceil(L_t / 64)); the result is the same attention summed in
//                                  another grouping, equal within the attention bar only (no bit claim).
// A token with no valid key in its split publishes LSE = -inf and zero rows, as mla_publish_empty_split does for 16 rows.
//
// Registers: two tokens cost 2 x (72 Q + 32 accumulator + 8 state); with one wave per SIMD (launch bound 256, 1) the 512
// registers hold them beside the addressing: no scratch (the compile's resource report; DESIGN 3.8 quotes it).
#include "common.h"
#include "lds_dma.h"
#include "mla_decode_tile.h"

namespace chitu {

constexpr int kDmaPiecesM = kTileU / 1024 / 4;  // 18 per wave

// grid (num_splits, batch, ceil(heads/16) * ceil(T/2)); block 256, one workgroup per CU (152 KB LDS)
__global__ __launch_bounds__(256, 1) void mla_decode_multi_kernel(
    const bf16_t* __restrict__ q_nope, int64_t qn_sb, int64_t qn_st, int64_t qn_sh, const bf16_t* __restrict__ q_pe,
    int64_t qp_sb, int64_t qp_st, int64_t qp_sh, const bf16_t* __restrict__ cache, int64_t num_pages, int page_size,
    const int32_t* __restrict__ block_table, int table_stride, const int32_t* __restrict__ seqlens,
    float scale, bf16_t* __restrict__ part_o, float* __restrict__ part_lse, bf16_t* __restrict__ out,
    int H, int T, int num_splits) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* kv_lds = smem;                                               // [2][64][kRowU]
    bf16_t* p_lds = reinterpret_cast<bf16_t*>(smem + 2 * kTileU);         // [16][72]
    float* red_max = reinterpret_cast<float*>(smem + 2 * kTileU + 16 * kPStride * 2);  // [4][16]
    float* red_sum = red_max + 64;                                        // [4][16]
    int* pages_lds = reinterpret_cast<int*>(red_sum + 64);                // [kMaxTilesLds]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int split = blockIdx.x, b = blockIdx.y;
    const MlaPair pr = mla_pair_of_block((int)blockIdx.z, T);
    const int h0 = pr.hb * 16;
    const int32_t* tbl = block_table + (int64_t)b * table_stride;
    const int max_page_idx = table_stride - 1;
    // as in mla_decode_kernel: the table's first 256 entries are requested beside seqlens, not behind it
    int L_raw;
    asm volatile("s_load_dword %0, %1, 0x0" : "=&s"(L_raw) : "s"(seqlens + b) : "memory");
    int spec[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        asm volatile("global_load_dword %0, %1, off" : "=v"(spec[k]) : "v"(tbl + min(lane + 64 * k, max_page_idx)) : "memory");
    // Q of both tokens (2 x 16 heads x 576): 2 x 1152 chunks of 16 B, <= 5 per thread and token, coalesced; it passes through
    // buffer 1 (free until the second tile is requested; 36 KB of its 72) on its way to the registers of the four waves
    i32x4 qreg[2][5];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int t = k ? pr.t1 : pr.t0;  // (an odd T's last workgroup reads its one token twice and uses it once)
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int c = min(tid + i * 256, 16 * 72 - 1);
            const int row = c / 72, col = c % 72;
            const int h = min(h0 + row, H - 1);
            const bf16_t* src = col < 64 ? q_nope + b * qn_sb + t * qn_st + h * qn_sh + col * 8
                                         : q_pe + b * qp_sb + t * qp_st + h * qp_sh + (col - 64) * 8;
            qreg[k][i] = *reinterpret_cast<const i32x4*>(src);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(L_raw)::"memory");
    const int L = max(L_raw, 0);  // a corrupt negative length is an empty sequence
    const int Lt0 = L - T + pr.t0 + 1;                    // keys token t0 sees (<= 0: none)
    const int Lt1 = pr.two ? L - T + pr.t1 + 1 : 0;       // the pair's second token; an odd T's last workgroup has none
    const int n_tiles = (L + kTile - 1) / kTile;
    const int tile0 = (int)((unsigned)n_tiles * (unsigned)split / (unsigned)num_splits);
    const int tile1 = (int)((unsigned)n_tiles * (unsigned)(split + 1) / (unsigned)num_splits);
    const bool pages_in_lds = (tile1 - tile0) <= kMaxTilesLds;
    const int p_first = (tile0 * kTile) / page_size;
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(spec[0]), "+v"(spec[1]), "+v"(spec[2]), "+v"(spec[3])::"memory");
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 5; ++i) asm volatile("" : "+v"(qreg[k][i]));
    int first_pg;
    if (p_first < 256) {
        const int pick = p_first < 64 ? spec[0] : p_first < 128 ? spec[1] : p_first < 192 ? spec[2] : spec[3];
        first_pg = __builtin_amdgcn_readlane(pick, p_first & 63);
    } else {
        first_pg = tbl[min(p_first, max_page_idx)];
    }
    auto page_src = [&](int64_t page, int t0) -> const bf16_t* {
        if (page < 0 || page >= num_pages) page = 0;  // corrupt table: stay in bounds
        return cache + (page * page_size + (t0 % page_size)) * (int64_t)kD;
    };
    auto tile_src = [&](int tile) -> const bf16_t* {
        const int t0 = tile * kTile;
        return page_src(pages_in_lds ? pages_lds[tile - tile0] : tbl[min(t0 / page_size, max_page_idx)], t0);
    };
    // this wave's 18 pieces of a tile: piece n = wave + 4 i; lane's image chunk 64 n + lane -> (row, source byte offset)
    int prow[kDmaPiecesM];
    uint32_t pswz[kDmaPiecesM];
#pragma unroll
    for (int i = 0; i < kDmaPiecesM; ++i) {
        const int qi = 64 * (wave + 4 * i) + lane;
        prow[i] = qi / 72;
        pswz[i] = (uint32_t)(((qi % 72) ^ kv_swz(prow[i])) << 4);
    }
    const uint32_t lds0 = lds_offset_of(smem);
    // rows past the sequence end (L, the longest length of the pair) re-read the tile's last valid row
    auto issue = [&](const bf16_t* src, int valid, int buf) {
        const bf16_t* sb = uniform_ptr(src);
#pragma unroll
        for (int i = 0; i < kDmaPiecesM; ++i)
            glds16_sbase<true>(sb, (uint32_t)(min(prow[i], valid - 1) * kRowU) + pswz[i],
                             lds0 + (uint32_t)(buf * kTileU + (wave + 4 * i) * 1024));
    };
    if (tile0 >= tile1) {  // an empty split publishes LSE = -inf and zero rows for both tokens
        mla_publish_empty_split(part_o, part_lse, out, b * T + pr.t0, H, h0, split, num_splits, tid);
        if (pr.two) mla_publish_empty_split(part_o, part_lse, out, b * T + pr.t1, H, h0, split, num_splits, tid);
        return;
    }
    issue(page_src(first_pg, tile0 * kTile), min(kTile, L - tile0 * kTile), 0);
    {   // Q into buffer 1, in the tile image's own layout: token k's 16 heads are rows 16 k .. 16 k + 15 (kv_swz reads bits 1 and
        // 3 of the row, so both blocks swizzle alike)
        uint8_t* q_lds = kv_lds + kTileU;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int c = tid + i * 256;
                if (c < 16 * 72) mla_q_store(q_lds + k * 16 * kRowU, c, qreg[k][i]);
            }
    }
    if (pages_in_lds && tile1 - tile0 > 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (tid + i * 256 < tile1 - tile0)
                pages_lds[tid + i * 256] = tbl[min(((tile0 + tid + i * 256) * kTile) / page_size, max_page_idx)];
    }

    MlaTokenState s0, s1;
    mla_token_init(s0);
    mla_token_init(s1);
    const MlaFrag frag = mla_frag(wave, j, g);

    __syncthreads();  // Q and the page list are visible (the first tile may still be in flight)
    mla_q_frags(s0.qf, kv_lds + kTileU, j, g);
    mla_q_frags(s1.qf, kv_lds + kTileU + 16 * kRowU, j, g);
    if (tile0 + 1 < tile1) {
        __syncthreads();  // every wave has its copies of Q: buffer 1 may be overwritten
        issue(tile_src(tile0 + 1), min(kTile, L - (tile0 + 1) * kTile), 1);
    }

    for (int tile = tile0; tile < tile1; ++tile) {
        const int buf = (tile - tile0) & 1;
        if (tile == tile0 && tile0 + 1 < tile1)
            asm volatile("s_waitcnt vmcnt(18)" ::: "memory");  // the first tile's pieces; the second tile's 18 stay in flight
        else
            glds_wait_all();  // this wave's pieces of the tile
        __syncthreads();   // everyone's; the other buffer and the softmax exchange areas of the previous tile are free
        if (tile > tile0 && tile + 1 < tile1) issue(tile_src(tile + 1), min(kTile, L - (tile + 1) * kTile), buf ^ 1);
        const uint8_t* kv = kv_lds + buf * kTileU;
        mla_pair_tile_steps(kv, frag, tile, Lt0, Lt1, scale, p_lds, red_max, red_sum, s0, s1, wave, j, g);
    }

    // (the partial transpose goes through the first buffer: at an odd tile count the last tile was multiplied there, and
    // mla_store_partial_rows meets before it writes)
    mla_token_epilogue(s0, part_o, part_lse, out, reinterpret_cast<bf16_t*>(kv_lds), b * T + pr.t0, H, h0, split, num_splits, tid, wave, j, g);
    if (pr.two)
        mla_token_epilogue(s1, part_o, part_lse, out, reinterpret_cast<bf16_t*>(kv_lds), b * T + pr.t1, H, h0, split, num_splits, tid, wave, j, g);
}

}  // namespace chitu

extern "C" int chitu_hip_mla_decode_multi(const void* q_nope, int64_t qn_stride_b, int64_t qn_stride_t, int64_t qn_stride_h,
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
    const size_t lds = 2 * kTileU + 16 * kPStride * 2 + 2 * 64 * sizeof(float) + kMaxTilesLds * sizeof(int);
    (void)hipFuncSetAttribute((const void*)mla_decode_multi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid((unsigned)num_splits, (unsigned)batch, (unsigned)(((heads + 15) / 16) * ((q_len + 1) / 2)));
    hipLaunchKernelGGL(mla_decode_multi_kernel, grid, dim3(256), lds, st, (const bf16_t*)q_nope, qn_stride_b, qn_stride_t, qn_stride_h,
                       (const bf16_t*)q_pe, qp_stride_b, qp_stride_t, qp_stride_h, (const bf16_t*)kv_cache, num_pages, (int)page_size,
                       block_table, (int)table_stride, seqlens, softmax_scale, part_o, part_lse, (bf16_t*)out_bf16, (int)heads,
                       (int)q_len, (int)num_splits);
    if (num_splits > 1 && out_bf16) launch_mla_merge(part_o, part_lse, (bf16_t*)out_bf16, (int64_t)rows * heads, (int)num_splits, st);
    CHITU_RETURN_LAUNCH_STATUS();
}
