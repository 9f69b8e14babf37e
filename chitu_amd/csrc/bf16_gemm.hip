// Skinny bf16 GEMM for decode on gfx950: the dense linears of an unquantised model (qkv, wo, gate/up + SiLU, down, LM head)
// and the router score GEMM of every MoE model.
//
// out[m][n] = sum_k x[m][k] * w[n][k]; the weight-streaming body of stream_gemm.h with Bf16Line: k-block = 64 elements = one
// 128-B line of a weight row.  Full-line layout (gemm_common.h): lane (j, g) loads 16 B of weight row n0 + 8*half + j/2 at
// element ((j%2)*4 + g)*8 of the block, so a wave-load takes whole lines from 8 rows; MFMA A-row j then holds K elements
// [0,32) (even j) or [32,64) (odd j) of weight row j/2, the block product is taken with the two activation fragments
// x[0..31], x[32..63] and the halves are added in-lane at the end.  bf16 has no per-block scales, so the four accumulators
// run across the whole K range.
// The router's N = n_experts is tiny (16 row tiles), so there K is also split across workgroups (num_splits) and the fp32
// partials are summed, in order, by the routing kernel itself (gate.hip; no separate reduce launch).
#include "common.h"
#include "gemm_common.h"
#include "stream_gemm.h"

namespace chitu {

// The plain kernel keeps its own body -- StreamLane, stream_ring and stream_gemm of stream_gemm.h written out (the shared
// half-fold apart), held to the machine code it was measured with: through the shared pieces the Llama-3-8B decode step
// measured 0.5 - 0.7 % slower (w2, wo, LM head).  It is the one launch here whose share of the K range is a
// run-time 64-bit division (S is a launch argument) and the one with a grid split-K.
// S > 1 (grid.y): K cut over S workgroups per tile, fp32 planes [S][M][N] left in `partial`.
// DEEP (single token tile, <= 8 K blocks per wave): the wave's whole K range in one round trip
// (a ring of 8 for the long-K form was measured: slower, Llama-3-8B bs 1 3.46 -> 3.50 ms/step)
template <int MT, int WK, bool DEEP = false>
__global__ __launch_bounds__(64 * WK) void bf16_gemm_kernel(const bf16_t* __restrict__ X,
                                                            const bf16_t* __restrict__ W,
                                                            void* __restrict__ out, int out_dt,
                                                            float* __restrict__ partial, int M, int N,
                                                            int K, int S, int m_base) {
    __shared__ float red[WK > 1 ? WK * MT * 256 : 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: SGPR index math
    const int j = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int KB = K >> 6;
    const int T = S * WK;
    const int t = blockIdx.y * WK + wave;
    const int kb0 = (int)((long)KB * t / T), kb1 = (int)((long)KB * (t + 1) / T);
    const int eoff = ((j & 1) * 4 + g) * 8;
    const bf16_t* wp0 = W + (size_t)min(n0 + (j >> 1), N - 1) * K + eoff;
    const bf16_t* wp1 = W + (size_t)min(n0 + 8 + (j >> 1), N - 1) * K + eoff;
    const bf16_t* xp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xp[mt] = X + (size_t)min(m_base + mt * 16 + j, M - 1) * K + g * 8;
    f32x4 e0[MT], o0[MT], e1[MT], o1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) e0[mt] = o0[mt] = e1[mt] = o1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    using Stage = Bf16Line::Stage<MT, 2>;
    auto load = [&](Stage& st, int kb) {
        const int off = kb << 6;
        st.w[0] = __builtin_nontemporal_load(reinterpret_cast<const s16x8*>(wp0 + off));
        st.w[1] = __builtin_nontemporal_load(reinterpret_cast<const s16x8*>(wp1 + off));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            st.x[mt][0] = *reinterpret_cast<const s16x8*>(xp[mt] + off);
            st.x[mt][1] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 32);
        }
    };
    auto compute = [&](const Stage& st) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            e0[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(st.w[0], st.x[mt][0], e0[mt], 0, 0, 0);
            o0[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(st.w[0], st.x[mt][1], o0[mt], 0, 0, 0);
            e1[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(st.w[1], st.x[mt][0], e1[mt], 0, 0, 0);
            o1[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(st.w[1], st.x[mt][1], o1[mt], 0, 0, 0);
        }
    };
    constexpr int D = Bf16Line::depth<2, MT>(DEEP);
    Stage ring[D];  // stream_ring<D>, written out
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (kb0 + d < kb1) load(ring[d], kb0 + d);
    for (int kb = kb0; kb < kb1; kb += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (kb + d < kb1) {
                compute(ring[d]);
                if (kb + d + D < kb1) load(ring[d], kb + d + D);
            }
        }
    }
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = fold_halves(e0[mt], o0[mt], e1[mt], o1[mt]);
    gemm_epilogue_v2<MT, WK>(acc, red, out, out_dt, partial, M, N, S, m_base, n0);
}

// Gate/up projection of an unquantised SwiGLU MLP with SiluAndMul in the epilogue: W = [w1 | w3] rows (2*inter x K),
// h = bf16(bf16(silu(bf16(g))) * bf16(u)) in one launch.
template <int MT, int WK>
__global__ __launch_bounds__(64 * WK) void bf16_gemm_silu_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                                                                 bf16_t* __restrict__ out, int M, int inter, int K,
                                                                 int m_base) {
    stream_gemm_silu<Bf16Line, MT, WK>(X, W, NoScale{}, out, M, inter, K, m_base);
}

}  // namespace chitu

extern "C" int chitu_hip_bf16_gemm(const void* x_bf16, const void* w_bf16, void* out, int out_dtype,
                                   int64_t M, int64_t N, int64_t K, int32_t num_splits,
                                   float* partials, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(x_bf16 && w_bf16 && M >= 0 && N >= 1 && K >= 64 && N < (1 << 30) && K < (1 << 30));
    CHITU_REQUIRE(num_splits >= 1 && num_splits <= 64);
    CHITU_REQUIRE(num_splits > 1 ? partials != nullptr : (out != nullptr && out_dtype >= 0 && out_dtype <= 2));
    if (K % 64 != 0) return CHITU_ERR_UNSUPPORTED;
    if (M == 0) return CHITU_OK;
    hipStream_t st = (hipStream_t)stream;
    const int KB = (int)(K / 64);
    const int tiles = (int)((N + 15) / 16);
    if (num_splits > KB) return CHITU_ERR_BAD_ARG;
    if ((M >= 256 || (M >= 128 && N >= 1024)) && K < (1 << 23) && debug_option(kOptBf16GemmTiled) != 0) {  // (32-bit byte offsets inside a tile)
        // prefill-sized M: a GEMM, not a weight stream (bf16_gemm_tiled.hip); a 128-row prompt against the 256-row router
        // matrix would be two workgroups -- that one stays with the split-K stream.  num_splits > 1: the K range cut over
        // that many workgroups per tile, fp32 planes left in `partials` (the router of a long prompt: few tiles, long K)
        launch_bf16_gemm_tiled((const bf16_t*)x_bf16, (const bf16_t*)w_bf16, out, out_dtype, M, N, K, num_splits, partials, st);
        CHITU_RETURN_LAUNCH_STATUS();
    }
    const int S = num_splits;
    int WK = stream_wk(tiles, KB, S);
    debug_override(kOptBf16GemmWK, WK);
    while (WK > 1 && WK * S > KB) WK >>= 1;
    const dim3 grid((unsigned)tiles, (unsigned)S);
    const int per_wave = KB / (WK * S);
    // the 8-deep ring (the wave's whole K range in one round trip) for a single token tile on grids of at most one workgroup
    // per CU: its register count admits one 8-wave workgroup per CU, so a larger grid would run in rounds (Llama-3-8B's qkv
    // projection, 384 workgroups; see bf16_norm_gemm.hip).  Option 11: 0 never, 1 always, -1 this heuristic.
    const int deep_opt = debug_option(kOptBf16GemmDeep);
    const bool deep = WK == 8 && per_wave > 4 && per_wave <= 8 && (deep_opt < 0 ? (int64_t)tiles * S <= 256 : deep_opt != 0);
    stream_walk_m(M, WK, [&](int mbase, auto mt, auto wk) {
        constexpr int MT = decltype(mt)::value, WKV = decltype(wk)::value;
        if (MT == 1 && deep)
            hipLaunchKernelGGL((bf16_gemm_kernel<1, 8, true>), grid, dim3(512), 0, st, (const bf16_t*)x_bf16,
                               (const bf16_t*)w_bf16, out, out_dtype, partials, (int)M, (int)N, (int)K, S, mbase);
        else
            hipLaunchKernelGGL((bf16_gemm_kernel<MT, WKV>), grid, dim3(64 * WKV), 0, st, (const bf16_t*)x_bf16,
                               (const bf16_t*)w_bf16, out, out_dtype, partials, (int)M, (int)N, (int)K, S, mbase);
    });
    // num_splits > 1: partials [S][M][N] are left for the consumer (chitu_hip_gate_route) to sum.
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_bf16_gemm_silu(const void* x_bf16, const void* w13_bf16, void* out_bf16, int64_t M,
                                        int64_t inter, int64_t K, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(x_bf16 && w13_bf16 && out_bf16 && M >= 0 && inter >= 1 && K >= 64 && inter < (1 << 29) && K < (1 << 30));
    if (K % 64 != 0) return CHITU_ERR_UNSUPPORTED;
    if (M == 0) return CHITU_OK;
    hipStream_t st = (hipStream_t)stream;
    const int KB = (int)(K / 64);
    const int tiles = (int)((inter + 15) / 16);
    int WK = stream_wk(tiles, KB);
    debug_override(kOptBf16SiluWK, WK);
    while (WK > 1 && WK > KB) WK >>= 1;
    const dim3 grid((unsigned)tiles);
    stream_walk_m(M, WK, [&](int mbase, auto mt, auto wk) {
        constexpr int MT = decltype(mt)::value, WKV = decltype(wk)::value;
        hipLaunchKernelGGL((bf16_gemm_silu_kernel<MT, WKV>), grid, dim3(64 * WKV), 0, st, (const bf16_t*)x_bf16,
                           (const bf16_t*)w13_bf16, (bf16_t*)out_bf16, (int)M, (int)inter, (int)K, mbase);
    });
    CHITU_RETURN_LAUNCH_STATUS();
}
