// Fused MoE for PREFILL-sized batches with MXFP4 expert weights (W4A8), gfx950: the two grouped GEMMs of moe_mxfp4.hip tiled
// for compute the way moe_tiled.hip tiles the fp8 ones -- TM sorted slots (64 or 128, the moe_align block) x 128 weight rows
// per workgroup, both operand tiles of a 128-wide K block staged in LDS by LDS-DMA, a ring of three stages, every wave
// multiplying 2 weight-row tiles x TM/16 slot tiles per block.  New: no reference counterpart (the reference has no 4-bit
// float expert mode); tiled form of moe_mx_gemm1_silu_kernel and moe_mx_gemm_kernel, which give every 16-slot tile its own
// stream of the expert's weights.
//   GEMM1 + SiLU:  64 gate rows [n0, n0+64) and the 64 up rows [I+n0, I+n0+64) of W1 [E, 2I, K/2]; wave w owns gate rows 16w..
//                  and the matching up rows: h = bf16(bf16(silu(bf16(g))) * bf16(u)) -> bf16 [numel, I]
//   GEMM2:         128 rows of W2 [E, N, I/2]; out[slot, n] = bf16(acc * routed_weight[slot]); h quantised by the caller
// Arithmetic: moe_mxfp4.hip's, rounding point for rounding point -- one mx_dot (mxfp4_common.h) per K block and fragment pair,
// acc = fmaf(dot, a_scale[slot row][kb], acc), K blocks ascending, one chain per output element (no K split, no atomics).
// With the streaming kernels at WK = 1 that is the same chain over the same block dots: the outputs are the same bits.
//
// Tiles.  Activations: moe_tiled.hip's [TM][128 B] image (lds_dma.h: chunks XOR-permuted on the source side), 16 KB at TM = 128.
// Weights: a row's K block is 64 B = 4 chunks of 16 B = the four 32-element MX blocks, and lane (j, g) of the FP4 operand reads
// chunk g of row j -- [128 rows][64 B] unpadded, chunk c of row r stored at c ^ (-(r >> 2) & 3): under ds_read_b128's lane
// groups the sixteen (row, chunk) pairs of a group then hit the sixteen 16-byte slots of the 256-B bank row once each
// (tests/test_mxfp4_tiled_host.py).  One DMA piece = 16 rows; the four lanes of a row read its half line (a 128-B line holds
// two K blocks of a row: the other half is the next step's, an L2 hit).  The E8M0 bytes -- 4 B per row and K block -- and the
// slots' activation scales ride with the tile as 4-byte DMA pieces: the K loop holds no load the compiler would wait for
// (its vmcnt wait would drain the DMA queue, moe_tiled.hip).  A stage is 8 + TM/8 + 2 KB: three stages = 54 KB (TM 64) or
// 78 KB (TM 128), two workgroups per CU either way.
#include "common.h"
#include "gemm_common.h"
#include "lds_dma.h"
#include "mxfp4_common.h"

namespace chitu {

#ifndef CHITU_MOE_MX_TILED_NREP
#define CHITU_MOE_MX_TILED_NREP 4  // 1: a workgroup per tile always (A/B builds)
#endif

constexpr int kMxTiledRing = 3;

// [rows][64 B] weight K-block tile: DMA piece n covers rows 16 n .. 16 n + 15, lane i -> row 16 n + (i >> 2), position i & 3
__device__ __forceinline__ int mx_tile_src_chunk(int lane) { return (lane & 3) ^ ((-(lane >> 4)) & 3); }
// byte offset inside a 16-row tile of lane (j, g)'s fragment (chunk g of row j)
__device__ __forceinline__ int mx_tile_frag_off(int j, int g) { return j * 64 + ((g ^ ((-(j >> 2)) & 3)) << 4); }

// grid: GEMM1 form 1-D (XCD-ordered (m-block, n-tile) pairs, moe_tiled.hip); GEMM2 form (weight-row tile groups, max m-blocks);
// block 256.  SILU: Nw = 2I rows per expert, a workgroup covers output columns [64 t, 64 t + 64); `out` = h [numel, I].
// else: Nw = N rows per expert, a workgroup covers rows [128 NREP t, +128 NREP); `out` = [numel, Nw] scaled by the routed weight.
// row_div: activation row of slot s = s / row_div (topk for GEMM1: the token; 1 for GEMM2: the slot's own h row).  K = the
// contraction length in ELEMENTS (a weight row is K/2 bytes, its scales K/32).  NREP (GEMM2 form only): consecutive 128-row
// tiles walked with one pipeline, a tile's C stored when its last K block is done (moe_tiled.hip says why: K = 256 at TP=8).
template <bool SILU, int NREP = 1, int TM = 64>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void moe_mx_gemm_tiled_kernel(
    const fp8_t* __restrict__ Xq, const float* __restrict__ Xs, const uint8_t* __restrict__ W, const uint8_t* __restrict__ Ws,
    const int32_t* __restrict__ sorted_ids, const int32_t* __restrict__ expert_ids,
    const int32_t* __restrict__ num_post_pad, bf16_t* __restrict__ out, const void* __restrict__ topk_w, int w_dt,
    int numel, int row_div, int Nw, int K) {
    static_assert(TM == 64 || TM == 128, "slot tiles of 64 or 128");
    static_assert(!SILU || NREP == 1, "the GEMM1 form keeps one tile per workgroup");
    constexpr int R = kMxTiledRing;
    __shared__ __attribute__((aligned(16))) uint8_t sW[R][128 * 64];
    __shared__ __attribute__((aligned(16))) uint8_t sX[R][TM * 128];
    __shared__ __attribute__((aligned(16))) float sS[R][4 * 64];      // activation scales: wave w's piece = slots (TM / 4) w ..
    __shared__ __attribute__((aligned(16))) uint32_t sE[R][4 * 64];   // E8M0 dwords: wave w's piece = its own 2 x 16 weight rows
    constexpr int MT = TM / 16;  // slot tiles per workgroup (every wave multiplies all of them)
    int mb, ntile;
    if (SILU) {
        const int n_tiles = Nw >> 7;  // (2I / 128) = I / 64 output-column tiles
        const int L = blockIdx.x, run = L / (8 * n_tiles), within = L % (8 * n_tiles);
        const int nb = (*num_post_pad + TM - 1) / TM, C = (nb + 7) >> 3;
        if (run >= C) return;
        mb = (within & 7) * C + run;
        ntile = within >> 3;
        if (mb >= nb) return;
    } else {
        mb = blockIdx.y;
        ntile = blockIdx.x;
        if (mb * TM >= *num_post_pad) return;
    }
    // a block whose first slot is already padding holds no token at all (real slots come first in an expert's segment)
    if (sorted_ids[mb * TM] >= numel) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int e = expert_ids[mb];
    const int I = Nw >> 1;
    const int n0 = SILU ? ntile * 64 : ntile * 128 * NREP;
    const int KB = K >> 7;

    // this lane's output slots (token column j of each slot tile)
    int slot[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) slot[mt] = sorted_ids[mb * TM + mt * 16 + j];
    // 16-slot sub-tiles that hold a token (real slots come first in a block): the others are neither multiplied nor stored
    int mt_valid = 0;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
        if (__builtin_amdgcn_ballot_w64(slot[mt] < numel) != 0) mt_valid = mt + 1;
    if (e < 0) {  // another rank's expert (expert parallelism): its slots are zero-filled
        const int cols = SILU ? 64 : 128 * NREP, ldo = SILU ? I : Nw;
        for (int idx = tid; idx < TM * (cols / 8); idx += 256) {
            const int r = idx / (cols / 8), c = idx % (cols / 8);
            const int s = sorted_ids[mb * TM + r];
            if (s < numel && n0 + c * 8 + 7 < ldo) *reinterpret_cast<i32x4*>(out + (size_t)s * ldo + n0 + c * 8) = i32x4{0, 0, 0, 0};
        }
        return;
    }

    // the wave's two weight-row tiles inside the staged 128 rows
    const int wrow0 = SILU ? 16 * wave : 32 * wave, wrow1 = SILU ? 64 + 16 * wave : 32 * wave + 16;
    // staged row r (0 .. 127) of repetition rep -> the expert's weight row; rows past the matrix re-read its last row (never stored)
    auto w_row = [&](int r, int rep) -> int {
        const int row = SILU ? (r < 64 ? n0 + r : I + n0 + (r - 64)) : n0 + rep * 128 + r;
        return min(row, Nw - 1);
    };
    // staging roles: wave w brings weight pieces 2 w, 2 w + 1 (16 rows each), activation pieces (TM / 32) w .. (8 rows each,
    // lds_dma.h), the E8M0 dwords of its OWN 32 weight rows (lanes 0-31; the upper half repeats them into the piece's unused
    // part) and the activation scales of TM / 4 slots -- the same number of pieces for every wave keeps the counted wait below
    // one constant.  32-bit byte offsets from the expert's first row / the activation matrix: the launcher bounds both.
    constexpr int XP = TM / 32;
    const uint8_t* We = W + (size_t)e * Nw * (K >> 1);
    const uint8_t* Se = Ws + (size_t)e * Nw * (K >> 5);
    uint32_t woff[2], eoff, xoff[XP];
    auto set_w_offsets = [&](int rep) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            woff[i] = (uint32_t)(w_row((wave * 2 + i) * 16 + (lane >> 2), rep) * (K >> 1) + mx_tile_src_chunk(lane) * 16);
        const int q = lane & 31;
        eoff = (uint32_t)(w_row(q < 16 ? wrow0 + q : wrow1 + (q - 16), rep) * (K >> 5));
    };
    set_w_offsets(0);
#pragma unroll
    for (int i = 0; i < XP; ++i) {
        const int n = wave * XP + i;
        const int s = sorted_ids[mb * TM + n * 8 + (lane >> 3)];
        xoff[i] = (uint32_t)((min(s, numel - 1) / row_div) * K + kblock_src_chunk(lane, n) * 16);
    }
    const uint32_t soff = (uint32_t)((min(sorted_ids[mb * TM + wave * (TM / 4) + (lane & (TM / 4 - 1))], numel - 1) / row_div) * KB * 4);
    const uint32_t ldsW = lds_offset_of(&sW[0][0]), ldsX = lds_offset_of(&sX[0][0]), ldsS = lds_offset_of(&sS[0][0]),
                   ldsE = lds_offset_of(&sE[0][0]);

    constexpr int kPieces = 2 + XP + 2;  // DMA pieces per wave and stage
    auto issue = [&](int stage, int kb) {
        const uint32_t b = (uint32_t)stage;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            glds16_sbase(uniform_ptr(We + (size_t)kb * 64), woff[i], ldsW + b * (128 * 64) + (uint32_t)((wave * 2 + i) * 1024));
#pragma unroll
        for (int i = 0; i < XP; ++i)
            glds16_sbase(uniform_ptr(Xq + (size_t)kb * 128), xoff[i], ldsX + b * (TM * 128) + (uint32_t)((wave * XP + i) * 1024));
        glds4_sbase(uniform_ptr(Se + (size_t)kb * 4), eoff, ldsE + b * 1024 + (uint32_t)(wave * 256));
        glds4_sbase(uniform_ptr(Xs + kb), soff, ldsS + b * 1024 + (uint32_t)(wave * 256));
    };
    const int xfoff = kblock_frag_off(j, g);   // activation fragment inside a 16-slot tile (second half: ^ 64)
    const int wfoff = mx_tile_frag_off(j, g);  // weight fragment inside a 16-row tile

    f32x4 acc[2][MT];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the slots' routed weights (GEMM2 form), fetched once up front: a load inside the step loop would bring a wait that
    // also drains the next step's DMA
    float rw[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) rw[mt] = 1.f;
    if (!SILU && topk_w) {
        if (w_dt == 2) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) rw[mt] = ((const float*)topk_w)[min(slot[mt], numel - 1)];
        } else {
            uint16_t raw[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) raw[mt] = ((const uint16_t*)topk_w)[min(slot[mt], numel - 1)];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) rw[mt] = w_dt == 0 ? bf16_to_f32(raw[mt]) : f16_to_f32(raw[mt]);
        }
    }
    // C tile (nt, mt): lane holds weight rows 4g .. 4g+3 of the tile for slot column j
    auto store_tile = [&](int nb) {  // nb = first weight row (GEMM2) / output column (GEMM1) of the finished tile
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int s = slot[mt];
            if (s >= numel) continue;
            const float rwm = rw[mt];
            if (SILU) {
                const int n = nb + 16 * wave + 4 * g;  // output column of r = 0
                uint16_t h[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float gv = round_bf16(acc[0][mt][r]), uv = round_bf16(acc[1][mt][r]);  // GEMM1's bf16 output
                    const float sl = round_bf16(gv / (1.0f + expf(-gv)));
                    h[r] = f32_to_bf16(sl * uv);
                }
                bf16_t* dst = out + (size_t)s * I + n;
                if (n + 3 < I) {
                    i32x2 o;
                    o[0] = (int)((uint32_t)h[0] | ((uint32_t)h[1] << 16));
                    o[1] = (int)((uint32_t)h[2] | ((uint32_t)h[3] << 16));
                    *reinterpret_cast<i32x2*>(dst) = o;
                } else {
                    for (int r = 0; r < 4 && n + r < I; ++r) dst[r] = h[r];
                }
            } else {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int n = nb + 32 * wave + 16 * nt + 4 * g;
                    uint16_t h[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[r] = f32_to_bf16(acc[nt][mt][r] * rwm);
                    bf16_t* dst = out + (size_t)s * Nw + n;
                    if (n + 3 < Nw) {
                        i32x2 o;
                        o[0] = (int)((uint32_t)h[0] | ((uint32_t)h[1] << 16));
                        o[1] = (int)((uint32_t)h[2] | ((uint32_t)h[3] << 16));
                        *reinterpret_cast<i32x2*>(dst) = o;
                    } else {
                        for (int r = 0; r < 4 && n + r < Nw; ++r) dst[r] = h[r];
                    }
                }
            }
        }
    };

    // (tile, K block) steps: the next two steps' operands are in flight while this one is multiplied
    const int reps = NREP == 1 ? 1 : min(NREP, (Nw - n0 + 127) >> 7);
    const int steps = reps * KB;
    int ikb = 0, irep = 0, istage = 0;  // the issue pointer runs R - 1 steps ahead of the multiply pointer
    auto issue_next = [&]() {
        if (NREP > 1 && ikb == 0 && irep > 0) set_w_offsets(irep);
        issue(istage, ikb);
        if (++ikb == KB) ikb = 0, ++irep;
        if (++istage == R) istage = 0;
    };
    // every load of the prologue is consumed HERE, ahead of the first request: a wait of the compiler's placed behind it would,
    // counting in order, wait for the tiles as well
#pragma unroll
    for (int i = 0; i < 2; ++i) asm volatile("" ::"v"(woff[i]));
#pragma unroll
    for (int i = 0; i < XP; ++i) asm volatile("" ::"v"(xoff[i]));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) asm volatile("" ::"v"(rw[mt]), "v"(slot[mt]));
    asm volatile("" ::"v"(soff), "v"(eoff));
    issue_next();
    if (steps > 1) issue_next();
    int rep = 0, kb = 0, buf = 0;
    for (int t = 0; t < steps; ++t) {
        // stage t has landed (this wave's pieces; stage t + 1, requested a step ago, may still be in flight) ...
        if (t + 1 < steps) glds_wait_leaving<kPieces>();
        else glds_wait_all();
        __syncthreads();  // ... and everyone's; everyone is done with stage t - 1, whose buffer the request below overwrites
        if (t + R - 1 < steps) issue_next();
        i32x4 wa[2];
        uint32_t wsc[2];
        wa[0] = *reinterpret_cast<const i32x4*>(&sW[buf][wrow0 * 64 + wfoff]);
        wa[1] = *reinterpret_cast<const i32x4*>(&sW[buf][wrow1 * 64 + wfoff]);
        // the lane's scale byte: the E8M0 of MX block g (k = 32g ..) of weight row j of the tile
        wsc[0] = (sE[buf][wave * 64 + j] >> (8 * g)) & 0xffu;
        wsc[1] = (sE[buf][wave * 64 + 16 + j] >> (8 * g)) & 0xffu;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (TM > 64 && mt >= mt_valid) continue;  // (wave-uniform) a sub-tile of padding only
            const uint8_t* xr = &sX[buf][mt * 16 * 128];
            const i32x8 xb = cat8(*reinterpret_cast<const i32x4*>(xr + xfoff), *reinterpret_cast<const i32x4*>(xr + (xfoff ^ 64)));
            // wave w's scale piece holds slots (TM / 4) w ..: sub-tile mt's 16 values sit in piece mt / (TM / 64) at (mt % (TM / 64)) * 16
            const float sc = sS[buf][(mt / (TM / 64)) * 64 + (mt % (TM / 64)) * 16 + j];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const f32x4 d = mx_dot(wa[nt], xb, wsc[nt]);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[nt][mt][r] = __builtin_fmaf(d[r], sc, acc[nt][mt][r]);
            }
        }
        if (kb == KB - 1) {  // this tile's last K block: its C leaves now, under the next tile's loads
            store_tile(n0 + rep * 128);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (++kb == KB) kb = 0, ++rep;
        if (++buf == R) buf = 0;
    }
}

}  // namespace chitu

extern "C" int chitu_hip_moe_gemm1_silu_mxfp4_tiled(const void* a_fp8, const float* a_scale, const void* w1_fp4,
                                                    const void* w1_scale_e8m0, const int32_t* sorted_token_ids,
                                                    const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                                    void* h_bf16, int64_t numel, int32_t topk, int64_t inter_size,
                                                    int64_t K, int64_t max_mblocks, int32_t block_m, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(a_fp8 && a_scale && w1_fp4 && w1_scale_e8m0 && sorted_token_ids && expert_ids && num_tokens_post_pad && h_bf16);
    CHITU_REQUIRE(numel >= 0 && numel < (1ll << 31) && topk >= 1 && inter_size >= 1 && K >= 1 && max_mblocks >= 0);
    if (K % 128 != 0 || inter_size % 128 != 0 || inter_size >= (1 << 29) || K >= (1 << 30)) return CHITU_ERR_UNSUPPORTED;
    if (2 * inter_size * (K / 2) >= (1ll << 31) || (numel / topk + 1) * K >= (1ll << 31)) return CHITU_ERR_UNSUPPORTED;  // 32-bit tile offsets
    if (block_m != 64 && block_m != 128) return CHITU_ERR_UNSUPPORTED;  // the moe_align block size the ids were sorted with
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    CHITU_REQUIRE(max_mblocks <= 65535);
    const dim3 grid((unsigned)((inter_size / 64) * ((max_mblocks + 7) / 8 * 8)));  // (m-block, n-tile) pairs in XCD order, see moe_tiled.hip
#define LAUNCH1X(TMV)                                                                                                      \
    hipLaunchKernelGGL((moe_mx_gemm_tiled_kernel<true, 1, TMV>), grid, dim3(256), 0, (hipStream_t)stream, (const fp8_t*)a_fp8, \
                       a_scale, (const uint8_t*)w1_fp4, (const uint8_t*)w1_scale_e8m0, sorted_token_ids, expert_ids,       \
                       num_tokens_post_pad, (bf16_t*)h_bf16, (const void*)nullptr, 0, (int)numel, (int)topk,               \
                       (int)(2 * inter_size), (int)K)
    if (block_m == 128) LAUNCH1X(128);
    else LAUNCH1X(64);
#undef LAUNCH1X
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_moe_gemm2_mxfp4_tiled(const void* h_fp8, const float* h_scale, const void* w2_fp4,
                                               const void* w2_scale_e8m0, const int32_t* sorted_token_ids,
                                               const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                               const void* topk_weights, int weights_dtype, int32_t mul_routed_weight,
                                               void* out_bf16, int64_t numel, int64_t N, int64_t inter_size,
                                               int64_t max_mblocks, int32_t block_m, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(h_fp8 && h_scale && w2_fp4 && w2_scale_e8m0 && sorted_token_ids && expert_ids && num_tokens_post_pad && out_bf16);
    CHITU_REQUIRE(numel >= 0 && numel < (1ll << 31) && N >= 1 && inter_size >= 1 && max_mblocks >= 0);
    CHITU_REQUIRE(!mul_routed_weight || (topk_weights && weights_dtype >= 0 && weights_dtype <= 2));
    if (inter_size % 128 != 0 || N % 8 != 0 || N >= (1 << 30) || inter_size >= (1 << 30)) return CHITU_ERR_UNSUPPORTED;
    if (N * (inter_size / 2) >= (1ll << 31) || (numel + 1) * inter_size >= (1ll << 31)) return CHITU_ERR_UNSUPPORTED;  // 32-bit tile offsets
    if (block_m != 64 && block_m != 128) return CHITU_ERR_UNSUPPORTED;  // the moe_align block size the ids were sorted with
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    CHITU_REQUIRE(max_mblocks <= 65535);
    const int n_tiles = (int)((N + 127) / 128);
#define LAUNCH2X(NREPV, TMV)                                                                                               \
    hipLaunchKernelGGL((moe_mx_gemm_tiled_kernel<false, NREPV, TMV>),                                                      \
                       dim3((unsigned)((n_tiles + NREPV - 1) / NREPV), (unsigned)max_mblocks), dim3(256), 0, (hipStream_t)stream, \
                       (const fp8_t*)h_fp8, h_scale, (const uint8_t*)w2_fp4, (const uint8_t*)w2_scale_e8m0, sorted_token_ids, \
                       expert_ids, num_tokens_post_pad, (bf16_t*)out_bf16,                                                 \
                       mul_routed_weight ? topk_weights : (const void*)nullptr, (int)weights_dtype, (int)numel, 1, (int)N, \
                       (int)inter_size)
    // few K blocks (R1 at TP=8: two): four tiles per workgroup through one pipeline; long K: a tile per workgroup
    if (inter_size <= 512 && n_tiles >= 8 && CHITU_MOE_MX_TILED_NREP > 1) {
        if (block_m == 128) LAUNCH2X(CHITU_MOE_MX_TILED_NREP, 128);
        else LAUNCH2X(CHITU_MOE_MX_TILED_NREP, 64);
    } else {
        if (block_m == 128) LAUNCH2X(1, 128);
        else LAUNCH2X(1, 64);
    }
#undef LAUNCH2X
    CHITU_RETURN_LAUNCH_STATUS();
}
