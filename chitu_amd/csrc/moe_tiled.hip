// Fused MoE for PREFILL-sized batches: the two grouped FP8 GEMMs tiled for compute (64 sorted slots x 128 weight rows
// per workgroup), gfx950.
//
// Replaces (reference, read-only), for hundreds of tokens and more:
//   chitu/fused_moe.py:62-307     fused_moe_kernel (Triton grouped GEMM, BLOCK_SIZE_M = 64 tiles -- the tile height
//                                 this file uses too: moe_align_block_size is run with block 64 here)
//   chitu/fused_moe.py:24-39      SiluAndMul (fused into GEMM1's epilogue)
// The decode kernels (moe.hip) give every 16-slot tile its own stream of the expert's weights: right when an expert
// sees 1-3 tokens, 4.2 GB of L2 -> CU traffic per layer at 2048 prompt tokens (64 tokens per expert:
// profiles/r02_prefill_*: 1.3 ms of a 2.0 ms layer).  Here a workgroup stages a 64-slot activation tile (rows gathered
// through sorted_token_ids) and a 128-row weight tile of the tile's expert in LDS per 128-wide K block, double-buffered
// like fp8_gemm_tiled.hip, and every wave multiplies 2 weight-row tiles x 4 slot tiles per block.  The tile walk, the step
// sequencing and the epilogue (both forms, with their rounding points) are moe_tiled_common.h's, shared with the MXFP4
// experts (moe_mxfp4_tiled.hip); this file holds the fp8 weight tile, its block scales and the launchers.
#include "moe_tiled_common.h"

namespace chitu {

// Slots per tile = the moe_align block size of this path: a template parameter TM, 64 or 128 (the launcher is told which).
//   64 (rounds 2-5): a 2048-token prompt puts ~72 slots on every expert of a 257-expert layer, i.e. two 64-slot blocks on most of
//   them, and the second block streams the expert's weights again -- 1.41 GB fetched per GEMM1 launch against 1.08 GB algorithmic.
//   128 (round 6): one block for nearly every expert, its weights streamed once; the block's all-padding 16-slot sub-tiles are
//   SKIPPED (wave-uniform count of the sub-tiles that hold a token), so the padded half costs loads of a repeated row and no MFMA /
//   scale fold -- round 5 built 128-slot tiles without the skip (and under a compiler-placed wait in the K loop) and measured
//   them slower; two stages instead of three keep two workgroups on a CU (66 KB each).  profiles/r05_ab_moe_tiled.txt, r06_ab_moe_tiled128.txt
// Both tiles of a K block arrive by LDS-DMA (lds_dma.h): unpadded [rows][128 B] with the 16-byte chunks XOR-permuted on the
// source side -- no staging registers, no ds_write pass, conflict-free fragment reads.

// probe builds (-DCHITU_PROBE, tools/probe_tiled_steps.py moe): shader-clock stamps of workgroup (0, 0)'s thread 0 at five points of
// steps 8 .. 13 -- top, own DMA pieces landed, barrier passed, next stage requested, block multiplied
#ifdef CHITU_PROBE
#define MOE_TILED_MARK(t, n)                                                                                                  \
    do {                                                                                                                      \
        if ((t) >= 8 && (t) < 14 && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) g_probe_marks[((t) - 8) * 5 + (n)] = __builtin_readcyclecounter(); \
    } while (0)
#else
#define MOE_TILED_MARK(t, n) do {} while (0)
#endif
#ifndef CHITU_MOE_TILED_NREP
#define CHITU_MOE_TILED_NREP 4  // 1: a workgroup per tile always (A/B builds, tools/build_variant.sh)
#endif

constexpr int moe_ring_of(int tm) { return tm == 128 ? 2 : 3; }  // stages of (W tile + X tile + scales): 25 KB each at 64 slots, 33 KB at 128
struct MoeTileScales {  // the weight tile's block scales of a K block (workgroup-uniform: scalar loads)
    float ws0, ws1;
};

// The fp8 side of moe_tiled_body (moe_tiled_common.h).  Weight tile: [128 rows][128 B] like the activation tile, wave w brings
// pieces 4 w .. 4 w + 3 (8 rows each).  Block scales: one per (128 rows, K block), two scalar loads per step fetched one step
// ahead.  Scales: (dot * a_s[slot row]) * w_s per K block, the reference's order (fused_moe.py:281).
template <bool SILU, int TM>
struct MoeFp8Tile {
    static constexpr int kRing = moe_ring_of(TM), kPieces = 4;
    static constexpr bool kActScales = true;
    using Ctx = MoeTileCtx<SILU>;
    uint8_t (*sW)[128 * 128];
    const fp8_t *W, *We;
    const float *Ws, *wsp0, *wsp1;
    uint32_t ldsW, woff[4];
    int foff;  // this lane's fragment inside a 16-row tile (second half: ^ 64)
    MoeTileScales cur, nxt;
    i32x4 wa[2][2];

    __device__ __forceinline__ MoeFp8Tile(uint8_t (*sW_)[128 * 128], const fp8_t* W_, const float* Ws_) : sW(sW_), W(W_), Ws(Ws_) {}
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
        const float* wsb = Ws + (size_t)c.e * ((c.Nw + 127) >> 7) * c.KB;
        wsp0 = wsb + (size_t)(c.n0 >> 7) * c.KB;
        wsp1 = SILU ? wsb + (size_t)((c.I + c.n0) >> 7) * c.KB : wsp0;
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
    __device__ __forceinline__ void issue_weight_scales(const Ctx&, uint32_t, int) const {}  // scalar loads: fetch_scales
    __device__ __forceinline__ void fetch_scales(const Ctx& c, int kb, int rep) {
        nxt.ws0 = wsp0[(size_t)rep * c.KB + kb];  // one 128-row tile = one row of block scales
        nxt.ws1 = SILU ? wsp1[kb] : nxt.ws0;
    }
    __device__ __forceinline__ void first_scales(const Ctx& c) { fetch_scales(c, 0, 0); }
    __device__ __forceinline__ void load(const Ctx& c, int buf, bool more, int nkb, int nrep) {
        cur = nxt;
        if (more) fetch_scales(c, nkb, nrep);
        const uint8_t* w0 = &sW[buf][c.wrow0() * 128];
        const uint8_t* w1 = &sW[buf][c.wrow1() * 128];
        wa[0][0] = *reinterpret_cast<const i32x4*>(w0 + foff);
        wa[0][1] = *reinterpret_cast<const i32x4*>(w0 + (foff ^ 64));
        wa[1][0] = *reinterpret_cast<const i32x4*>(w1 + foff);
        wa[1][1] = *reinterpret_cast<const i32x4*>(w1 + (foff ^ 64));
    }
    __device__ __forceinline__ void fold(f32x4& acc0, f32x4& acc1, const i32x4& xb0, const i32x4& xb1, float sc) const {
        const f32x4 d0 = mfma_fp8_k128(wa[0][0], wa[0][1], xb0, xb1);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc0[r] += (d0[r] * sc) * cur.ws0;
        const f32x4 d1 = mfma_fp8_k128(wa[1][0], wa[1][1], xb0, xb1);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc1[r] += (d1[r] * sc) * cur.ws1;
    }
    static __device__ __forceinline__ void mark(int t, int n) { MOE_TILED_MARK(t, n); }
    static __device__ __forceinline__ void mark_fold(float v) {
#ifdef CHITU_PROBE
        if (v == 12345.678f) g_probe_marks[31] = 1;  // (the stamp behind it waits for a fold of this step)
#endif
    }
};

// grid, arguments, NREP: moe_tiled_body (moe_tiled_common.h)
template <bool SILU, int NREP = 1, int TM = 64>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void moe_gemm_tiled_kernel(
    const fp8_t* __restrict__ Xq, const float* __restrict__ Xs, const fp8_t* __restrict__ W, const float* __restrict__ Ws,
    const int32_t* __restrict__ sorted_ids, const int32_t* __restrict__ expert_ids,
    const int32_t* __restrict__ num_post_pad, bf16_t* __restrict__ out, const void* __restrict__ topk_w, int w_dt,
    int numel, int row_div, int Nw, int K) {
    // a ring of kMoeRing stages (one K block of both operand tiles + the slots' scales each): 25 KB a stage, two resident
    // workgroups per CU; two stages are in flight while one is multiplied.  (Measured against a ring of two once the K loop held
    // no compiler wait any more: within noise -- at 2048 tokens these launches are HBM-bound, profiles/r05_ab_moe_tiled.txt.)
    constexpr int kMoeRing = moe_ring_of(TM);
    __shared__ __attribute__((aligned(16))) uint8_t sW[kMoeRing][128 * 128];
    __shared__ __attribute__((aligned(16))) uint8_t sX[kMoeRing][TM * 128];
    __shared__ __attribute__((aligned(16))) float sS[kMoeRing][4 * 64];  // the K block's activation scales: wave w's piece = slots (TM / 4) w ..
    MoeFp8Tile<SILU, TM> f(sW, W, Ws);
    moe_tiled_body<SILU, NREP, TM>(f, sX, sS, Xq, Xs, sorted_ids, expert_ids, num_post_pad, out, topk_w, w_dt, numel, row_div, Nw, K);
}

}  // namespace chitu

extern "C" int chitu_hip_moe_gemm1_silu_fp8_tiled(const void* a_fp8, const float* a_scale, const void* w1_fp8,
                                                  const float* w1_scale, const int32_t* sorted_token_ids,
                                                  const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                                  void* h_bf16, int64_t numel, int32_t topk, int64_t inter_size,
                                                  int64_t K, int64_t max_mblocks, int32_t block_m, void* stream) {
    using namespace chitu;
    bool launch;
    const int rc = moe_tiled_gemm1_args(a_fp8 && a_scale && w1_fp8 && w1_scale && sorted_token_ids && expert_ids && num_tokens_post_pad && h_bf16,
                                        numel, topk, inter_size, K, /*min_k*/ 128, /*w_row_bytes*/ K, max_mblocks, block_m, &launch);
    if (!launch) return rc;
    const dim3 grid = moe_tiled_gemm1_grid(inter_size, max_mblocks);
#define LAUNCH1T(TMV)                                                                                                              \
    hipLaunchKernelGGL((moe_gemm_tiled_kernel<true, 1, TMV>), grid, dim3(256), 0, (hipStream_t)stream, (const fp8_t*)a_fp8, a_scale, \
                       (const fp8_t*)w1_fp8, w1_scale, sorted_token_ids, expert_ids, num_tokens_post_pad, (bf16_t*)h_bf16,           \
                       (const void*)nullptr, 0, (int)numel, (int)topk, (int)(2 * inter_size), (int)K)
    if (block_m == 128) LAUNCH1T(128);
    else LAUNCH1T(64);
#undef LAUNCH1T
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_moe_gemm2_fp8_tiled(const void* h_fp8, const float* h_scale, const void* w2_fp8,
                                             const float* w2_scale, const int32_t* sorted_token_ids,
                                             const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                             const void* topk_weights, int weights_dtype, int32_t mul_routed_weight,
                                             void* out_bf16, int64_t numel, int64_t N, int64_t inter_size,
                                             int64_t max_mblocks, int32_t block_m, void* stream) {
    using namespace chitu;
    bool launch;
    const int rc = moe_tiled_gemm2_args(h_fp8 && h_scale && w2_fp8 && w2_scale && sorted_token_ids && expert_ids && num_tokens_post_pad && out_bf16,
                                        !mul_routed_weight || (topk_weights && weights_dtype >= 0 && weights_dtype <= 2), numel, N, inter_size,
                                        /*min_k*/ 128, /*w_row_bytes*/ inter_size, max_mblocks, block_m, &launch);
    if (!launch) return rc;
    const int n_tiles = (int)((N + 127) / 128);
#define LAUNCH2T(NREPV, TMV)                                                                                               \
    hipLaunchKernelGGL((moe_gemm_tiled_kernel<false, NREPV, TMV>),                                                         \
                       dim3((unsigned)((n_tiles + NREPV - 1) / NREPV), (unsigned)max_mblocks), dim3(256), 0, (hipStream_t)stream, \
                       (const fp8_t*)h_fp8, h_scale, (const fp8_t*)w2_fp8, w2_scale, sorted_token_ids, expert_ids,         \
                       num_tokens_post_pad, (bf16_t*)out_bf16, mul_routed_weight ? topk_weights : (const void*)nullptr,    \
                       (int)weights_dtype, (int)numel, 1, (int)N, (int)inter_size)
    MOE_TILED_DISPATCH_GEMM2(LAUNCH2T, CHITU_MOE_TILED_NREP);
#undef LAUNCH2T
    CHITU_RETURN_LAUNCH_STATUS();
}

CHITU_PROBE_READER(moe_tiled)
