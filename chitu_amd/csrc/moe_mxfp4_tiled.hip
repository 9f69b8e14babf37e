// Fused MoE for PREFILL-sized batches with MXFP4 expert weights (W4A8), gfx950: the two grouped GEMMs of moe_mxfp4.hip tiled
// for compute the way moe_tiled.hip tiles the fp8 ones -- TM sorted slots (64 or 128, the moe_align block) x 128 weight rows
// per workgroup, both operand tiles of a 128-wide K block staged in LDS by LDS-DMA, a ring of three stages, every wave
// multiplying 2 weight-row tiles x TM/16 slot tiles per block.  New: no reference counterpart (the reference has no 4-bit
// float expert mode); tiled form of moe_mx_gemm1_silu_kernel and moe_mx_gemm_kernel, which give every 16-slot tile its own
// stream of the expert's weights.  The tile walk, the step sequencing and the epilogue are moe_tiled_common.h's, shared with
// moe_tiled.hip; this file holds the MXFP4 weight tile, its E8M0 scales and the launchers.
//   GEMM1 + SiLU:  64 gate rows [n0, n0+64) and the 64 up rows [I+n0, I+n0+64) of W1 [E, 2I, K/2]
//   GEMM2:         128 rows of W2 [E, N, I/2]; h quantised by the caller
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
#include "moe_tiled_common.h"
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

// The MXFP4 side of moe_tiled_body (moe_tiled_common.h).  Staging roles: wave w brings weight pieces 2 w, 2 w + 1 (16 rows
// each) and the E8M0 dwords of its OWN 32 weight rows (lanes 0-31; the upper half repeats them into the piece's unused part).
// K = the contraction length in ELEMENTS (a weight row is K/2 bytes, its scales K/32).
template <bool SILU>
struct MoeMxTile : MoeTiledNoProbe {
    static constexpr int kRing = kMxTiledRing, kPieces = 2 + 1;
    static constexpr bool kActScales = true;
    using Ctx = MoeTileCtx<SILU>;
    uint8_t (*sW)[128 * 64];
    uint32_t (*sE)[4 * 64];
    const uint8_t *W, *Ws, *We, *Se;
    uint32_t ldsW, ldsE, woff[2], eoff;
    int wfoff;  // this lane's weight fragment inside a 16-row tile
    i32x4 wa[2];
    uint32_t wsc[2];

    __device__ __forceinline__ MoeMxTile(uint8_t (*sW_)[128 * 64], uint32_t (*sE_)[4 * 64], const uint8_t* W_, const uint8_t* Ws_)
        : sW(sW_), sE(sE_), W(W_), Ws(Ws_) {}
    __device__ __forceinline__ void set_w_offsets(const Ctx& c, int rep) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            woff[i] = (uint32_t)(c.w_row((c.wave * 2 + i) * 16 + (c.lane >> 2), rep) * (c.K >> 1) + mx_tile_src_chunk(c.lane) * 16);
        const int q = c.lane & 31;
        eoff = (uint32_t)(c.w_row(q < 16 ? c.wrow0() + q : c.wrow1() + (q - 16), rep) * (c.K >> 5));
    }
    __device__ __forceinline__ void init(const Ctx& c) {
        We = W + (size_t)c.e * c.Nw * (c.K >> 1);
        Se = Ws + (size_t)c.e * c.Nw * (c.K >> 5);
        set_w_offsets(c, 0);
        ldsW = lds_offset_of(&sW[0][0]);
        ldsE = lds_offset_of(&sE[0][0]);
        wfoff = mx_tile_frag_off(c.j, c.g);
    }
    __device__ __forceinline__ void consume_offsets() const {
#pragma unroll
        for (int i = 0; i < 2; ++i) asm volatile("" ::"v"(woff[i]));
        asm volatile("" ::"v"(eoff));
    }
    __device__ __forceinline__ void issue_weights(const Ctx& c, uint32_t b, int kb) const {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            glds16_sbase(uniform_ptr(We + (size_t)kb * 64), woff[i], ldsW + b * (128 * 64) + (uint32_t)((c.wave * 2 + i) * 1024));
    }
    __device__ __forceinline__ void issue_weight_scales(const Ctx& c, uint32_t b, int kb) const {
        glds4_sbase(uniform_ptr(Se + (size_t)kb * 4), eoff, ldsE + b * 1024 + (uint32_t)(c.wave * 256));
    }
    __device__ __forceinline__ void first_scales(const Ctx&) const {}  // they ride with the tile
    __device__ __forceinline__ void load(const Ctx& c, int buf, bool, int, int) {
        wa[0] = *reinterpret_cast<const i32x4*>(&sW[buf][c.wrow0() * 64 + wfoff]);
        wa[1] = *reinterpret_cast<const i32x4*>(&sW[buf][c.wrow1() * 64 + wfoff]);
        // the lane's scale byte: the E8M0 of MX block g (k = 32g ..) of weight row j of the tile
        wsc[0] = (sE[buf][c.wave * 64 + c.j] >> (8 * c.g)) & 0xffu;
        wsc[1] = (sE[buf][c.wave * 64 + 16 + c.j] >> (8 * c.g)) & 0xffu;
    }
    __device__ __forceinline__ void fold(f32x4& acc0, f32x4& acc1, const i32x4& xb0, const i32x4& xb1, float sc) const {
        const i32x8 xb = cat8(xb0, xb1);
        const f32x4 d0 = mx_dot(wa[0], xb, wsc[0]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc0[r] = __builtin_fmaf(d0[r], sc, acc0[r]);
        const f32x4 d1 = mx_dot(wa[1], xb, wsc[1]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc1[r] = __builtin_fmaf(d1[r], sc, acc1[r]);
    }
};

// grid, arguments, NREP: moe_tiled_body (moe_tiled_common.h; moe_tiled.hip says why: K = 256 at TP=8)
template <bool SILU, int NREP = 1, int TM = 64>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void moe_mx_gemm_tiled_kernel(
    const fp8_t* __restrict__ Xq, const float* __restrict__ Xs, const uint8_t* __restrict__ W, const uint8_t* __restrict__ Ws,
    const int32_t* __restrict__ sorted_ids, const int32_t* __restrict__ expert_ids,
    const int32_t* __restrict__ num_post_pad, bf16_t* __restrict__ out, const void* __restrict__ topk_w, int w_dt,
    int numel, int row_div, int Nw, int K) {
    constexpr int R = kMxTiledRing;
    __shared__ __attribute__((aligned(16))) uint8_t sW[R][128 * 64];
    __shared__ __attribute__((aligned(16))) uint8_t sX[R][TM * 128];
    __shared__ __attribute__((aligned(16))) float sS[R][4 * 64];      // activation scales: wave w's piece = slots (TM / 4) w ..
    __shared__ __attribute__((aligned(16))) uint32_t sE[R][4 * 64];   // E8M0 dwords: wave w's piece = its own 2 x 16 weight rows
    MoeMxTile<SILU> f(sW, sE, W, Ws);
    moe_tiled_body<SILU, NREP, TM>(f, sX, sS, Xq, Xs, sorted_ids, expert_ids, num_post_pad, out, topk_w, w_dt, numel, row_div, Nw, K);
}

}  // namespace chitu

extern "C" int chitu_hip_moe_gemm1_silu_mxfp4_tiled(const void* a_fp8, const float* a_scale, const void* w1_fp4,
                                                    const void* w1_scale_e8m0, const int32_t* sorted_token_ids,
                                                    const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                                    void* h_bf16, int64_t numel, int32_t topk, int64_t inter_size,
                                                    int64_t K, int64_t max_mblocks, int32_t block_m, void* stream) {
    using namespace chitu;
    bool launch;
    const int rc = moe_tiled_gemm1_args(a_fp8 && a_scale && w1_fp4 && w1_scale_e8m0 && sorted_token_ids && expert_ids && num_tokens_post_pad && h_bf16,
                                        numel, topk, inter_size, K, /*min_k*/ 1, /*w_row_bytes*/ K / 2, max_mblocks, block_m, &launch);
    if (!launch) return rc;
    const dim3 grid = moe_tiled_gemm1_grid(inter_size, max_mblocks);
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
    bool launch;
    const int rc = moe_tiled_gemm2_args(h_fp8 && h_scale && w2_fp4 && w2_scale_e8m0 && sorted_token_ids && expert_ids && num_tokens_post_pad && out_bf16,
                                        !mul_routed_weight || (topk_weights && weights_dtype >= 0 && weights_dtype <= 2), numel, N, inter_size,
                                        /*min_k*/ 1, /*w_row_bytes*/ inter_size / 2, max_mblocks, block_m, &launch);
    if (!launch) return rc;
    const int n_tiles = (int)((N + 127) / 128);
#define LAUNCH2X(NREPV, TMV)                                                                                               \
    hipLaunchKernelGGL((moe_mx_gemm_tiled_kernel<false, NREPV, TMV>),                                                      \
                       dim3((unsigned)((n_tiles + NREPV - 1) / NREPV), (unsigned)max_mblocks), dim3(256), 0, (hipStream_t)stream, \
                       (const fp8_t*)h_fp8, h_scale, (const uint8_t*)w2_fp4, (const uint8_t*)w2_scale_e8m0, sorted_token_ids, \
                       expert_ids, num_tokens_post_pad, (bf16_t*)out_bf16,                                                 \
                       mul_routed_weight ? topk_weights : (const void*)nullptr, (int)weights_dtype, (int)numel, 1, (int)N, \
                       (int)inter_size)
    MOE_TILED_DISPATCH_GEMM2(LAUNCH2X, CHITU_MOE_MX_TILED_NREP);
#undef LAUNCH2X
    CHITU_RETURN_LAUNCH_STATUS();
}
