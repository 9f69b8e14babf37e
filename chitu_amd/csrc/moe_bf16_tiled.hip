// Fused MoE for PREFILL-sized batches on bf16 experts with bf16 activations: the two grouped GEMMs tiled for compute
// (64 or 128 sorted slots x 128 weight rows per workgroup), gfx950.
//
// Replaces (reference, read-only), for hundreds of tokens and more on unquantised experts:
//   chitu/fused_moe.py:62-307     fused_moe_kernel with use_fp8_w8a8 = False (Triton grouped GEMM, BLOCK_SIZE_M = 64 tiles)
//   chitu/fused_moe.py:24-39      SiluAndMul (fused into GEMM1's epilogue)
// The streaming kernels (moe_bf16.hip) give every 16-slot tile its own pass over the expert's weights: right when an expert
// sees a handful of tokens, eight passes over 9.4 MB per expert when a 2048-token prompt puts ~128 slots on every expert of a
// 128-expert, top-8 layer (Qwen3-30B-A3B).  Here a workgroup stages a TM-slot activation tile (rows gathered through
// sorted_token_ids) and a 128-row weight tile of the tile's expert in LDS per 128-BYTE K block (64 bf16: the dense tile step of
// bf16_gemm_tiled.hip), and every wave multiplies 2 weight-row tiles x TM / 16 slot tiles per block with
// v_mfma_f32_16x16x32_bf16.  The tile walk (XCD-aware for GEMM1, the NREP walk for GEMM2), the slot gather, the zero fill, the
// LDS-DMA ring's step sequencing and the epilogue with its rounding points are moe_tiled_common.h's, shared with the fp8 and
// MXFP4 experts; the body counts in bytes, so for this format `K` is the row length in bytes and a K block is 128 of them.
// This file holds the bf16 weight tile and the launchers.  There are no scales: the accumulators run in fp32 across the whole
// K, so on data whose products and sums are exact in fp32 the outputs equal moe_gemm_bf16_kernel's bit for bit.
#include "moe_tiled_common.h"
#include "chitu_hip_ext3.h"

namespace chitu {

#ifndef CHITU_MOE_BF16_TILED_NREP
#define CHITU_MOE_BF16_TILED_NREP 4  // 1: a workgroup per tile always (A/B builds)
#endif

// stages of (W tile + X tile): 24 KB each at 64 slots (three: 72 KB), 32 KB at 128 (two: 64 KB) -- two workgroups per CU
constexpr int moe_bf16_ring_of(int tm) { return tm == 128 ? 2 : 3; }

// The bf16 side of moe_tiled_body.  Weight tile: [128 rows][128 B] like the activation tile, wave w brings pieces 4 w .. 4 w + 3
// (8 rows each).  Lane (j, g) of a 16-row tile holds chunks g and g + 4 of row j: elements [8g, 8g + 8) of each 32-element
// half, one MFMA operand per half (bf16_gemm_tiled.hip); weights are the A operand, so C rows are weight rows.
template <bool SILU, int TM>
struct MoeBf16Tile : MoeTiledNoProbe {
    static constexpr int kRing = moe_bf16_ring_of(TM), kPieces = 4;
    static constexpr bool kActScales = false;
    using Ctx = MoeTileCtx<SILU>;
    uint8_t (*sW)[128 * 128];
    const uint8_t *W, *We;
    uint32_t ldsW, woff[4];
    int foff;  // this lane's fragment inside a 16-row tile (second half: ^ 64)
    s16x8 wa[2][2];

    __device__ __forceinline__ MoeBf16Tile(uint8_t (*sW_)[128 * 128], const uint8_t* W_) : sW(sW_), W(W_) {}
    // (c.K: bytes per weight row)
    __device__ __forceinline__ void set_w_offsets(const Ctx& c, int rep) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = c.wave * 4 + i;
            woff[i] = (uint32_t)(c.w_row(n * 8 + (c.lane >> 3), rep) * c.K + kblock_src_chunk(c.lane, n) * 16);
        }
    }
    __device__ __forceinline__ void init(const Ctx& c) {
        We = W + (size_t)c.e * c.Nw * c.K;
        set_w_offsets(c, 0);
        ldsW = lds_offset_of(&sW[0][0]);
        foff = kblock_frag_off(c.j, c.g);
    }
    __device__ __forceinline__ void consume_offsets() const {
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" ::"v"(woff[i]));
    }
    __device__ __forceinline__ void issue_weights(const Ctx& c, uint32_t b, int kb) const {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            glds16_sbase(uniform_ptr(We + (size_t)kb * 128), woff[i], ldsW + b * (128 * 128) + (uint32_t)((c.wave * 4 + i) * 1024));
    }
    __device__ __forceinline__ void issue_weight_scales(const Ctx&, uint32_t, int) const {}
    __device__ __forceinline__ void first_scales(const Ctx&) {}
    __device__ __forceinline__ void load(const Ctx& c, int buf, bool, int, int) {
        const uint8_t* w0 = &sW[buf][c.wrow0() * 128];
        const uint8_t* w1 = &sW[buf][c.wrow1() * 128];
        wa[0][0] = *reinterpret_cast<const s16x8*>(w0 + foff);
        wa[0][1] = *reinterpret_cast<const s16x8*>(w0 + (foff ^ 64));
        wa[1][0] = *reinterpret_cast<const s16x8*>(w1 + foff);
        wa[1][1] = *reinterpret_cast<const s16x8*>(w1 + (foff ^ 64));
    }
    __device__ __forceinline__ void fold(f32x4& acc0, f32x4& acc1, const i32x4& xb0, const i32x4& xb1, float) const {
        const s16x8 x0 = __builtin_bit_cast(s16x8, xb0), x1 = __builtin_bit_cast(s16x8, xb1);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[0][0], x0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[1][0], x0, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[0][1], x1, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[1][1], x1, acc1, 0, 0, 0);
    }
};

// grid, arguments, NREP: moe_tiled_body (moe_tiled_common.h); K in ELEMENTS here, bytes from the body on
template <bool SILU, int NREP = 1, int TM = 64>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void moe_bf16_tiled_kernel(
    const bf16_t* __restrict__ X, const bf16_t* __restrict__ W, const int32_t* __restrict__ sorted_ids,
    const int32_t* __restrict__ expert_ids, const int32_t* __restrict__ num_post_pad, bf16_t* __restrict__ out,
    const void* __restrict__ topk_w, int w_dt, int numel, int row_div, int Nw, int K) {
    constexpr int kRing = moe_bf16_ring_of(TM);
    __shared__ __attribute__((aligned(16))) uint8_t sW[kRing][128 * 128];
    __shared__ __attribute__((aligned(16))) uint8_t sX[kRing][TM * 128];
    MoeBf16Tile<SILU, TM> f(sW, reinterpret_cast<const uint8_t*>(W));
    moe_tiled_body<SILU, NREP, TM>(f, sX, static_cast<float(*)[4 * 64]>(nullptr), reinterpret_cast<const fp8_t*>(X),
                                   static_cast<const float*>(nullptr), sorted_ids, expert_ids, num_post_pad, out, topk_w, w_dt, numel,
                                   row_div, Nw, 2 * K);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace chitu

extern "C" int chitu_ext3_moe_gemm1_silu_bf16_tiled(const void* a_bf16, const void* w1_bf16, const int32_t* sorted_token_ids,
                                                    const int32_t* expert_ids, const int32_t* num_tokens_post_pad, void* h_bf16,
                                                    int64_t numel, int32_t topk, int64_t inter_size, int64_t K, int64_t max_mblocks,
                                                    int32_t block_m, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(a_bf16 && w1_bf16 && sorted_token_ids && expert_ids && num_tokens_post_pad && h_bf16);
    CHITU_REQUIRE(aligned16(a_bf16) && aligned16(w1_bf16) && aligned16(h_bf16));
    CHITU_REQUIRE(aligned4(sorted_token_ids) && aligned4(expert_ids) && aligned4(num_tokens_post_pad));
    CHITU_REQUIRE(numel >= 0 && numel < (1ll << 31) && topk >= 1 && inter_size >= 1 && K >= 1 && max_mblocks >= 0);
    CHITU_REQUIRE(block_m == 64 || block_m == 128);  // the moe_align block size the ids were sorted with
    CHITU_REQUIRE(max_mblocks <= 65535);
    if (K % 128 != 0 || inter_size % 128 != 0 || inter_size >= (1 << 29) || K >= (1 << 29)) return CHITU_ERR_UNSUPPORTED;
    // 32-bit byte offsets inside one expert's W1 and inside the activation matrix
    if (2 * inter_size * 2 * K >= (1ll << 31) || (numel / topk + 1) * 2 * K >= (1ll << 31)) return CHITU_ERR_UNSUPPORTED;
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    const dim3 grid = moe_tiled_gemm1_grid(inter_size, max_mblocks);
#define LAUNCH1T(TMV)                                                                                                          \
    hipLaunchKernelGGL((moe_bf16_tiled_kernel<true, 1, TMV>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a_bf16,   \
                       (const bf16_t*)w1_bf16, sorted_token_ids, expert_ids, num_tokens_post_pad, (bf16_t*)h_bf16,              \
                       (const void*)nullptr, 0, (int)numel, (int)topk, (int)(2 * inter_size), (int)K)
    if (block_m == 128) LAUNCH1T(128);
    else LAUNCH1T(64);
#undef LAUNCH1T
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_ext3_moe_gemm2_bf16_tiled(const void* h_bf16, const void* w2_bf16, const int32_t* sorted_token_ids,
                                               const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                               const void* topk_weights, int weights_dtype, int32_t mul_routed_weight,
                                               void* out_bf16, int64_t numel, int64_t N, int64_t inter_size, int64_t max_mblocks,
                                               int32_t block_m, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(h_bf16 && w2_bf16 && sorted_token_ids && expert_ids && num_tokens_post_pad && out_bf16);
    CHITU_REQUIRE(aligned16(h_bf16) && aligned16(w2_bf16) && aligned16(out_bf16));
    CHITU_REQUIRE(aligned4(sorted_token_ids) && aligned4(expert_ids) && aligned4(num_tokens_post_pad));
    CHITU_REQUIRE(!mul_routed_weight || (topk_weights && weights_dtype >= 0 && weights_dtype <= 2 &&
                                         ((uintptr_t)topk_weights & (weights_dtype == 2 ? 3 : 1)) == 0));
    CHITU_REQUIRE(numel >= 0 && numel < (1ll << 31) && N >= 1 && inter_size >= 1 && max_mblocks >= 0);
    CHITU_REQUIRE(block_m == 64 || block_m == 128);
    CHITU_REQUIRE(max_mblocks <= 65535);
    if (inter_size % 128 != 0 || N % 8 != 0 || N >= (1 << 29) || inter_size >= (1 << 29)) return CHITU_ERR_UNSUPPORTED;
    // 32-bit byte offsets inside one expert's W2 and inside h
    if (N * 2 * inter_size >= (1ll << 31) || (numel + 1) * 2 * inter_size >= (1ll << 31)) return CHITU_ERR_UNSUPPORTED;
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    const int n_tiles = (int)((N + 127) / 128);
#define LAUNCH2T(NREPV, TMV)                                                                                               \
    hipLaunchKernelGGL((moe_bf16_tiled_kernel<false, NREPV, TMV>),                                                         \
                       dim3((unsigned)((n_tiles + NREPV - 1) / NREPV), (unsigned)max_mblocks), dim3(256), 0, (hipStream_t)stream, \
                       (const bf16_t*)h_bf16, (const bf16_t*)w2_bf16, sorted_token_ids, expert_ids, num_tokens_post_pad,   \
                       (bf16_t*)out_bf16, mul_routed_weight ? topk_weights : (const void*)nullptr, (int)weights_dtype,     \
                       (int)numel, 1, (int)N, (int)inter_size)
    // few K blocks (an expert of up to 512 columns: at most eight) and more tiles than one group: NREP consecutive tiles per
    // workgroup through one pipeline, the last group ragged; long K: a tile per workgroup
    if (inter_size <= 512 && n_tiles > CHITU_MOE_BF16_TILED_NREP && CHITU_MOE_BF16_TILED_NREP > 1) {
        if (block_m == 128) LAUNCH2T(CHITU_MOE_BF16_TILED_NREP, 128);
        else LAUNCH2T(CHITU_MOE_BF16_TILED_NREP, 64);
    } else {
        if (block_m == 128) LAUNCH2T(1, 128);
        else LAUNCH2T(1, 64);
    }
#undef LAUNCH2T
    CHITU_RETURN_LAUNCH_STATUS();
}
