// What the two prefill-shaped grouped expert GEMMs share -- moe_tiled.hip (fp8 experts) and moe_mxfp4_tiled.hip (MXFP4 experts):
// the walk over (m-block, weight-row tile) pairs, the slot gather, the zero fill for another rank's expert, the activation-side
// staging, the (tile, K block) step sequencing of the LDS-DMA ring, the epilogue, and the launchers' argument checks.
// A workgroup multiplies TM sorted slots (64 or 128, the moe_align block) by 128 weight rows per 128-wide K block; every wave
// multiplies 2 weight-row tiles x TM/16 slot tiles.
//   GEMM1 + SiLU:  the 128 weight rows are 64 gate rows [n0, n0+64) and the 64 up rows [I+n0, I+n0+64) of W1 [E, 2I, K];
//                  wave w owns gate rows 16w.. and the matching up rows, so g and u of one output meet in one lane:
//                  h = bf16(bf16(silu(bf16(g))) * bf16(u)) -> bf16 [numel, I]   (moe_gemm1_silu_kernel's rounding points)
//   GEMM2:         128 rows of W2 [E, N, I]; out[slot, n] = bf16(acc * routed_weight[slot]) (moe_gemm2_kernel's)
//
// A weight format is a small struct F (MoeFp8Tile, MoeMxTile) that owns what differs -- the weight tile's LDS image, where its
// scales come from, the block product and how it is folded into the accumulator:
//   F::kRing, F::kPieces        ring stages; DMA pieces per wave and stage that the format brings itself
//   F::kActScales               the activations are fp8 with one fp32 scale per (row, 128-wide K block) that rides with the tile
//                               (MoeBf16Tile, moe_bf16_tiled.hip: false -- bf16 activations, a K block is 128 BYTES = 64 elements,
//                               `K` and `Xq` are then the row length in bytes and the matrix as bytes; sS and Xs are not touched)
//   f.init(c)                   the expert's base pointers, the wave's staging offsets of the first tile
//   f.set_w_offsets(c, rep)     ... and of tile `rep` of an NREP walk
//   f.consume_offsets()         its part of the fence ahead of the first request
//   f.issue_weights(c, stage, kb), f.issue_weight_scales(c, stage, kb)   its DMA pieces, ahead of / behind the activation tile's
//   f.first_scales(c)           scales that do not ride with the tile: those of step 0 ...
//   f.load(c, buf, more, nkb, nrep)   ... and of the next step (`more`: there is one); the wave's weight fragments of stage buf
//   f.fold(acc0, acc1, xb0, xb1, sc)  both weight-row tiles times one slot tile, folded with the slots' scale sc
//   F::mark(t, n), F::mark_fold(v)    probe stamps (MoeTiledNoProbe: none)
#pragma once
#include "common.h"
#include "gemm_common.h"
#include "lds_dma.h"

namespace chitu {

// a workgroup's place in the GEMM, as the weight format sees it
template <bool SILU>
struct MoeTileCtx {
    int wave, lane, j, g;  // lane (j, g) = (lane & 15, lane >> 4) of the MFMA fragments
    int e, n0, I, Nw, K, KB;
    // staged row r (0 .. 127) of repetition rep -> the expert's weight row; rows past the matrix re-read its last row (never stored)
    __device__ __forceinline__ int w_row(int r, int rep) const {
        const int row = SILU ? (r < 64 ? n0 + r : I + n0 + (r - 64)) : n0 + rep * 128 + r;
        return min(row, Nw - 1);
    }
    // the wave's two weight-row tiles inside the staged 128 rows
    __device__ __forceinline__ int wrow0() const { return SILU ? 16 * wave : 32 * wave; }
    __device__ __forceinline__ int wrow1() const { return SILU ? 64 + 16 * wave : 32 * wave + 16; }
};

struct MoeTiledNoProbe {
    static __device__ __forceinline__ void mark(int, int) {}
    static __device__ __forceinline__ void mark_fold(float) {}
};

// grid: GEMM1 form 1-D (XCD-ordered (m-block, n-tile) pairs); GEMM2 form (weight-row tile groups, max m-blocks); block 256.
//   SILU: Nw = 2I rows per expert, a workgroup covers output columns [64 t, 64 t + 64); `out` = h [numel, I].
//   else: Nw = N rows per expert, a workgroup covers rows [128 NREP t, +128 NREP); `out` = [numel, Nw] scaled by the routed weight.
// row_div: activation row of slot s = s / row_div (topk for GEMM1: the token; 1 for GEMM2: the slot's own h row).  K = the
// contraction length in elements.
// NREP (GEMM2 form only): consecutive 128-row weight tiles a workgroup walks with ONE pipeline -- (tile, K block) pairs are
// one sequence of steps, the next step's operands are in flight while this one is multiplied, a tile's C is stored when its
// last K block is done.  With K = 256 (two K blocks, R1 at TP=8) a workgroup per tile is all prologue and epilogue: its
// dependent chain (padded count -> expert id -> slot ids -> rows -> LDS -> MFMA -> store) is paid once per NREP tiles.
// sX, sS: the kernel's rings of activation tiles ([TM][128 B] K blocks, lds_dma.h) and of the slots' activation scales; the
// __global__ wrapper owns every __shared__ array, so its LDS budget (two workgroups per CU) is read off in one place.
template <bool SILU, int NREP, int TM, class F>
__device__ __forceinline__ void moe_tiled_body(F& f, uint8_t (*sX)[TM * 128], float (*sS)[4 * 64], const fp8_t* __restrict__ Xq,
                                               const float* __restrict__ Xs, const int32_t* __restrict__ sorted_ids,
                                               const int32_t* __restrict__ expert_ids, const int32_t* __restrict__ num_post_pad,
                                               bf16_t* __restrict__ out, const void* __restrict__ topk_w, int w_dt, int numel,
                                               int row_div, int Nw, int K) {
    static_assert(TM == 64 || TM == 128, "slot tiles of 64 or 128");
    static_assert(!SILU || NREP == 1, "the GEMM1 form keeps one tile per workgroup");
    constexpr int R = F::kRing;
    // GEMM1 form: a 1-D grid walked XCD-aware.  Workgroup L of every run of 8 * n_tiles goes to XCD L % 8 (round-robin
    // dispatch); XCD x is given the CONTIGUOUS m-blocks [x C, x C + C) (C = an eighth of the padded blocks), one per run, all
    // n-tiles of it inside the run: the n-tiles of one m-block -- they stage the same gathered activation rows, 459 KB per 64
    // slots at K = 7168 -- share one L2, and so do the m-blocks of one expert (consecutive in the sorted order).
    // (Also measured and not kept: the XCD sequence in groups of four m-blocks, n-tile by n-tile, so that the blocks of one
    // expert stream the same weight rows back to back: 275 vs 270-274 us.)
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
    // a block whose first slot is already padding holds no token at all (real slots come first in an expert's segment):
    // nothing to multiply, nothing to store
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
    if (e < 0) {  // another rank's expert (expert parallelism): its slots are zero-filled, fused_moe.py:40-59
        const int cols = SILU ? 64 : 128 * NREP, ldo = SILU ? I : Nw;
        for (int idx = tid; idx < TM * (cols / 8); idx += 256) {
            const int r = idx / (cols / 8), c = idx % (cols / 8);
            const int s = sorted_ids[mb * TM + r];
            if (s < numel && n0 + c * 8 + 7 < ldo) *reinterpret_cast<i32x4*>(out + (size_t)s * ldo + n0 + c * 8) = i32x4{0, 0, 0, 0};
        }
        return;
    }

    // staging roles (LDS-DMA pieces, lds_dma.h): wave w brings the format's weight pieces of its share of the 128 rows and the
    // activation pieces (TM / 32) w .. (8 rows each); byte offsets from the expert's first weight row / the activation matrix
    // (32-bit: the launcher bounds both), rows past the matrix re-read its last row, padded slots a valid row (never stored)
    const MoeTileCtx<SILU> c{wave, lane, j, g, e, n0, I, Nw, K, KB};
    f.init(c);
    constexpr int XP = TM / 32;  // activation pieces per wave
    uint32_t xoff[XP];
#pragma unroll
    for (int i = 0; i < XP; ++i) {
        const int n = wave * XP + i;
        const int s = sorted_ids[mb * TM + n * 8 + (lane >> 3)];
        xoff[i] = (uint32_t)((min(s, numel - 1) / row_div) * K + kblock_src_chunk(lane, n) * 16);
    }
    // the slots' activation scales ride with the tile: every wave brings the block's values of TM / 4 slots (one 4-byte DMA
    // piece; the other lanes repeat them into the piece's unused part -- the same number of pieces for every wave keeps the
    // counted wait below one constant).  As plain loads one step ahead they put a vmcnt(0) of the compiler's into the MFMA
    // stream (fp8_gemm_tiled.hip).
    uint32_t soff = 0, ldsS = 0;
    if constexpr (F::kActScales) {
        soff = (uint32_t)((min(sorted_ids[mb * TM + wave * (TM / 4) + (lane & (TM / 4 - 1))], numel - 1) / row_div) * KB * 4);
        ldsS = lds_offset_of(&sS[0][0]);
    }
    const uint32_t ldsX = lds_offset_of(&sX[0][0]);

    constexpr int kPieces = F::kPieces + XP + (F::kActScales ? 1 : 0);  // DMA pieces per wave and stage
    auto issue = [&](int stage, int kb) {
        const uint32_t b = (uint32_t)stage;
        f.issue_weights(c, b, kb);
#pragma unroll
        for (int i = 0; i < XP; ++i)
            glds16_sbase(uniform_ptr(Xq + (size_t)kb * 128), xoff[i], ldsX + b * (TM * 128) + (uint32_t)((wave * XP + i) * 1024));
        f.issue_weight_scales(c, b, kb);
        if constexpr (F::kActScales) glds4_sbase(uniform_ptr(Xs + kb), soff, ldsS + b * 1024 + (uint32_t)(wave * 256));
    };
    const int xfoff = kblock_frag_off(j, g);  // this lane's activation fragment inside a 16-slot tile (second half: ^ 64)

    f32x4 acc[2][MT];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the slots' routed weights (GEMM2 form), fetched once up front: fetched when a tile leaves (round 5a) they were loads inside
    // the step loop, whose wait also drained the next step's DMA
    float rw[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) rw[mt] = 1.f;
    if (!SILU && topk_w) {  // (one uniform branch per element type: the loads of a lane are in flight together)
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
        const int ldo = SILU ? I : Nw;
        auto store4 = [&](bf16_t* dst, int n, const uint16_t (&h)[4]) {  // output columns n .. n + 3 of one slot row
            if (n + 3 < ldo) {
                i32x2 o;
                o[0] = (int)((uint32_t)h[0] | ((uint32_t)h[1] << 16));
                o[1] = (int)((uint32_t)h[2] | ((uint32_t)h[3] << 16));
                *reinterpret_cast<i32x2*>(dst) = o;
            } else {
                for (int r = 0; r < 4 && n + r < ldo; ++r) dst[r] = h[r];
            }
        };
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
                    const float gv = round_bf16(acc[0][mt][r]), uv = round_bf16(acc[1][mt][r]);  // GEMM1's bf16 output (c1)
                    const float sl = round_bf16(gv / (1.0f + expf(-gv)));
                    h[r] = f32_to_bf16(sl * uv);
                }
                store4(out + (size_t)s * I + n, n, h);
            } else {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int n = nb + 32 * wave + 16 * nt + 4 * g;
                    uint16_t h[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[r] = f32_to_bf16(acc[nt][mt][r] * rwm);
                    store4(out + (size_t)s * Nw + n, n, h);
                }
            }
        }
    };

    // (tile, K block) steps: the next step's operands land while this one is multiplied
    const int reps = NREP == 1 ? 1 : min(NREP, (Nw - n0 + 127) >> 7);
    const int steps = reps * KB;
    // the issue pointer runs R - 1 steps ahead of the multiply pointer
    int ikb = 0, irep = 0, istage = 0;
    auto issue_next = [&]() {
        if (NREP > 1 && ikb == 0 && irep > 0) f.set_w_offsets(c, irep);
        issue(istage, ikb);
        if (++ikb == KB) ikb = 0, ++irep;
        if (++istage == R) istage = 0;
    };
    // every load of the prologue is consumed HERE, ahead of the first request: a wait of the compiler's placed behind it would,
    // counting in order, wait for the tiles as well
    f.consume_offsets();
#pragma unroll
    for (int i = 0; i < XP; ++i) asm volatile("" ::"v"(xoff[i]));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) asm volatile("" ::"v"(rw[mt]), "v"(slot[mt]));
    if constexpr (F::kActScales) asm volatile("" ::"v"(soff));
    issue_next();
    if (R == 3 && steps > 1) issue_next();
    f.first_scales(c);
    int rep = 0, kb = 0, buf = 0;
    for (int t = 0; t < steps; ++t) {
        int nkb = kb + 1, nrep = rep;
        if (nkb == KB) nkb = 0, nrep = rep + 1;
        // stage t has landed (this wave's pieces; stage t + 1, requested a step ago, may still be in flight) ...
        F::mark(t, 0);
        if (R == 3 && t + 1 < steps) glds_wait_leaving<kPieces>();
        else glds_wait_all();
        F::mark(t, 1);
        __syncthreads();  // ... and everyone's; everyone is done with stage t - 1, whose buffer the request below overwrites
        F::mark(t, 2);
        if (t + R - 1 < steps) issue_next();
        F::mark(t, 3);
        f.load(c, buf, t + 1 < steps, nkb, nrep);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (TM > 64 && mt >= mt_valid) continue;  // (wave-uniform) a sub-tile of padding only
            const uint8_t* xr = &sX[buf][mt * 16 * 128];
            const i32x4 xb0 = *reinterpret_cast<const i32x4*>(xr + xfoff), xb1 = *reinterpret_cast<const i32x4*>(xr + (xfoff ^ 64));
            // wave w's scale piece holds slots (TM / 4) w ..: sub-tile mt's 16 values sit in piece mt / (TM / 64) at (mt % (TM / 64)) * 16
            float sc = 1.f;
            if constexpr (F::kActScales) sc = sS[buf][(mt / (TM / 64)) * 64 + (mt % (TM / 64)) * 16 + j];
            f.fold(acc[0][mt], acc[1][mt], xb0, xb1, sc);
        }
        F::mark_fold(acc[1][0][3]);
        F::mark(t, 4);
        if (kb == KB - 1) {  // this tile's last K block: its C leaves now, under the next tile's loads
            store_tile(n0 + rep * 128);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        kb = nkb, rep = nrep;
        if (++buf == R) buf = 0;
    }
}

// ---------------------------------------------------------------- launchers
// The argument checks of the tiled entries, in the order their return codes are documented in.  min_k: the smallest contraction
// length the entry takes as an argument at all (below it: CHITU_ERR_BAD_ARG); w_row_bytes: bytes of one weight row.  *launch
// is set when there is work to launch; otherwise the entry returns the result as it is.
static inline int moe_tiled_gemm1_args(bool pointers, int64_t numel, int32_t topk, int64_t inter_size, int64_t K, int64_t min_k,
                                       int64_t w_row_bytes, int64_t max_mblocks, int32_t block_m, bool* launch) {
    *launch = false;
    CHITU_REQUIRE(pointers);
    CHITU_REQUIRE(numel >= 0 && numel < (1ll << 31) && topk >= 1 && inter_size >= 1 && K >= min_k && max_mblocks >= 0);
    if (K % 128 != 0 || inter_size % 128 != 0 || inter_size >= (1 << 29) || K >= (1 << 30)) return CHITU_ERR_UNSUPPORTED;
    if (2 * inter_size * w_row_bytes >= (1ll << 31) || (numel / topk + 1) * K >= (1ll << 31)) return CHITU_ERR_UNSUPPORTED;  // 32-bit tile offsets
    if (block_m != 64 && block_m != 128) return CHITU_ERR_UNSUPPORTED;  // the moe_align block size the ids were sorted with
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    CHITU_REQUIRE(max_mblocks <= 65535);
    *launch = true;
    return CHITU_OK;
}
static inline int moe_tiled_gemm2_args(bool pointers, bool routed_weights, int64_t numel, int64_t N, int64_t inter_size, int64_t min_k,
                                       int64_t w_row_bytes, int64_t max_mblocks, int32_t block_m, bool* launch) {
    *launch = false;
    CHITU_REQUIRE(pointers);
    CHITU_REQUIRE(numel >= 0 && numel < (1ll << 31) && N >= 1 && inter_size >= min_k && max_mblocks >= 0);
    CHITU_REQUIRE(routed_weights);
    if (inter_size % 128 != 0 || N % 8 != 0 || N >= (1 << 30) || inter_size >= (1 << 30)) return CHITU_ERR_UNSUPPORTED;
    if (N * w_row_bytes >= (1ll << 31) || (numel + 1) * inter_size >= (1ll << 31)) return CHITU_ERR_UNSUPPORTED;  // 32-bit tile offsets
    if (block_m != 64 && block_m != 128) return CHITU_ERR_UNSUPPORTED;  // the moe_align block size the ids were sorted with
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    CHITU_REQUIRE(max_mblocks <= 65535);
    *launch = true;
    return CHITU_OK;
}
// GEMM1 form: (m-block, n-tile) pairs in XCD order, see moe_tiled_body
static inline dim3 moe_tiled_gemm1_grid(int64_t inter_size, int64_t max_mblocks) {
    return dim3((unsigned)((inter_size / 64) * ((max_mblocks + 7) / 8 * 8)));
}
// GEMM2 form, from the launcher's own inter_size, n_tiles and block_m.  LAUNCH(NREPV, TMV) launches one instantiation on
// dim3((n_tiles + NREPV - 1) / NREPV, max_mblocks).
// few K blocks (R1 at TP=8: two): `nrep` (a build constant, 4) tiles per workgroup through one pipeline; long K: a tile per workgroup
#define MOE_TILED_DISPATCH_GEMM2(LAUNCH, nrep)                           \
    do {                                                                 \
        if (inter_size <= 512 && n_tiles >= 8 && (nrep) > 1) {           \
            if (block_m == 128) LAUNCH(nrep, 128);                       \
            else LAUNCH(nrep, 64);                                       \
        } else {                                                         \
            if (block_m == 128) LAUNCH(1, 128);                          \
            else LAUNCH(1, 64);                                          \
        }                                                                \
    } while (0)

}  // namespace chitu
