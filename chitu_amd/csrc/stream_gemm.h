// The decode-shaped dense GEMM, stated once: out[m][n] = sum_k x[m][k] * w[n][k] as a weight stream.
//
// A workgroup owns 16 output rows (columns of `out`) and up to 32 tokens; K is split over its WK <= 8 waves, whose fp32
// partial sums are added through LDS in wave order.  Every wave keeps a register ring of D K steps in flight: all D stages
// are requested before the first product, and a stage is requested again as soon as it has been multiplied.  M is walked in
// 32-row launches.  Weights are read in the full-line layout of gemm_common.h: the 16 lanes j of a lane group g read whole
// 128-byte lines of 8 weight rows (row group 0: n0 + j/2, row group 1: n0 + 8 + j/2), MFMA A-row j then holds one HALF of a
// line of weight row j/2 (even j the first, odd j the second), the step's product is taken once with the activations of
// either half into separate accumulators (e: valid on even A-rows, o: on odd ones) and the halves are added in-lane at the
// end (fold_halves).
//
// What a weight format adds is a LINE POLICY (Bf16Line below, Int8Line in w8a16_gemm.hip): an object built per lane that says
//   weight_t, Scale          element type of W; the per-column scale of the epilogue (NoScale | RowScale, gemm_common.h)
//   depth<NW, MT>()          ring depth for NW row groups per stage (2: plain, 4: gate + up) and MT token tiles
//   Stage<MT, NW>            what a wave holds of one K step
//   steps()                  K steps of a row
//   w_off() / x_off()        the lane's element offset inside a weight row's / an activation row's step
//   load(stage, wp, xp, s)   request step s
//   mfma(stage, e, o, s)     e[r][mt], o[r][mt] += the step's product of row group r and token tile mt
// Two bodies use it: stream_gemm (plain, gemm_epilogue_v2) and stream_gemm_silu (gate / up pairs, silu_reduce_store).  The
// __global__ kernels of w8a16_gemm.hip and bf16_gemm_silu_kernel (bf16_gemm.hip) are argument lists around them;
// bf16_gemm_kernel, the one form with a grid split-K, keeps its own body there.
#pragma once
#include <type_traits>

#include "common.h"
#include "gemm_common.h"
#include "gemm_plan.h"  // the host side: stream_wk, stream_walk_m

namespace chitu {

// f(0), ..., f(N - 1) with the index as a std::integral_constant: a loop unrolled in the source
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// the share [first, last) of `steps` K steps that belongs to wave t of T
__device__ __forceinline__ void stream_share(int steps, int t, int T, int& first, int& last) {
    first = steps * t / T;
    last = steps * (t + 1) / T;
}

// The register ring: D stages in flight before the first product, each requested again once it has been used.
template <int D, class Stage, class Load, class Compute>
__device__ __forceinline__ void stream_ring(int first, int last, Load load, Compute compute) {
    Stage ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (first + d < last) load(ring[d], first + d);
    for (int s = first; s < last; s += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (s + d < last) {
                compute(ring[d], s + d);
                if (s + d + D < last) load(ring[d], s + d + D);
            }
        }
    }
}

// bf16 weights.  K step = 64 elements = one 128-byte line of a weight row: lane (j, g) holds elements ((j%2)*4 + g)*8 .. +7,
// so A-row j is K elements [0,32) (even j) or [32,64) (odd j) of weight row j/2, multiplied with the activation fragments
// x[8g ..] and x[32 + 8g ..].  No scales: the accumulators run across the whole K range.
struct Bf16Line {
    using weight_t = bf16_t;
    using Scale = NoScale;
    // plain: 4, or 8 = DEEP (single token tile, <= 8 K blocks per wave): the wave's whole K range in one round trip
    // (a ring of 8 for the long-K form was measured: slower, Llama-3-8B bs 1 3.46 -> 3.50 ms/step)
    template <int NW, int MT>
    static constexpr int depth(bool deep) {
        return NW == 2 ? (deep ? 8 : 4) : MT >= 2 ? 2 : 3;
    }
    template <int MT, int NW>
    struct Stage {
        s16x8 w[NW];
        s16x8 x[MT][2];
    };
    int K, eoff, g8;
    __device__ __forceinline__ Bf16Line(int K_, int j, int g) : K(K_), eoff(((j & 1) * 4 + g) * 8), g8(g * 8) {}
    __device__ __forceinline__ int steps() const { return K >> 6; }
    __device__ __forceinline__ int w_off() const { return eoff; }
    __device__ __forceinline__ int x_off() const { return g8; }
    template <int MT, int NW>
    __device__ __forceinline__ void load(Stage<MT, NW>& st, const bf16_t* const (&wp)[NW], const bf16_t* const (&xp)[MT],
                                         int s) const {
        const int off = s << 6;
#pragma unroll
        for (int r = 0; r < NW; ++r) st.w[r] = __builtin_nontemporal_load(reinterpret_cast<const s16x8*>(wp[r] + off));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            st.x[mt][0] = *reinterpret_cast<const s16x8*>(xp[mt] + off);
            st.x[mt][1] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 32);
        }
    }
    template <int MT, int NW>
    __device__ __forceinline__ void mfma(const Stage<MT, NW>& st, f32x4 (&e)[NW][MT], f32x4 (&o)[NW][MT], int) const {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < NW; ++r) {
                e[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(st.w[r], st.x[mt][0], e[r][mt], 0, 0, 0);
                o[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(st.w[r], st.x[mt][1], o[r][mt], 0, 0, 0);
            }
        }
    }
};

// What a lane of either body sets up: its geometry, its share of the K steps, its NW clamped weight-row pointers (NW == 4:
// rows [0, rows) are the gate matrix, [rows, 2 rows) the up matrix, row groups 2 and 3 the up rows of 0 and 1), its MT
// clamped activation-row pointers and zeroed accumulators.
template <class L, int MT, int NW, int WK>
struct StreamLane {
    int lane, wave, j, g, n0, first, last;
    L line;
    const typename L::weight_t* wp[NW];
    const bf16_t* xp[MT];
    f32x4 e[NW][MT], o[NW][MT];
    __device__ __forceinline__ StreamLane(const bf16_t* X, const typename L::weight_t* W, int M, int rows, int K, int m_base)
        : lane(threadIdx.x & 63), wave(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)),  // wave-uniform: SGPR index math
          j(lane & 15), g(lane >> 4), n0(blockIdx.x * 16), line(K, j, g) {
        stream_share(line.steps(), wave, WK, first, last);
        // (unrolled in the source: around a loop LICM re-associates `base + row * K + lane offset` to hoist `base + lane
        // offset`, which the kernels this replaced did not have)
        static_for<NW>([&](auto r) {
            wp[r] = W + (size_t)((r >> 1) * rows + min(n0 + (r & 1) * 8 + (j >> 1), rows - 1)) * K + line.w_off();
        });
        static_for<MT>([&](auto mt) { xp[mt] = X + (size_t)min(m_base + mt * 16 + j, M - 1) * K + line.x_off(); });
#pragma unroll
        for (int r = 0; r < NW; ++r)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) e[r][mt] = o[r][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    template <int D>
    __device__ __forceinline__ void run() {
        using Stage = typename L::template Stage<MT, NW>;
        stream_ring<D, Stage>(
            first, last, [&](Stage& st, int s) { line.load(st, wp, xp, s); },
            [&](const Stage& st, int s) { line.mfma(st, e, o, s); });
    }
};

// ---------------------------------------------------------------- plain: out = x . W^T (* scale)
// (No grid split-K: that is bf16_gemm_kernel's, which keeps its own body -- bf16_gemm.hip.)
template <class L, int MT, int WK>
__device__ __forceinline__ void stream_gemm(const bf16_t* __restrict__ X, const typename L::weight_t* __restrict__ W,
                                            typename L::Scale scale, void* __restrict__ out, int out_dt, int M, int N, int K,
                                            int m_base) {
    __shared__ float red[WK > 1 ? WK * MT * 256 : 1];
    StreamLane<L, MT, 2, WK> ln(X, W, M, N, K, m_base);
    ln.template run<L::template depth<2, MT>(false)>();
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = fold_halves(ln.e[0][mt], ln.o[0][mt], ln.e[1][mt], ln.o[1][mt]);
    gemm_epilogue_v2<MT, WK>(acc, red, out, out_dt, nullptr, M, N, 1, m_base, ln.n0, scale);
}

// h = bf16( bf16(silu(bf16(g * gs))) * bf16(u * us) ): FeedForward (models/model.py:212-214: F.silu(w1 x) * w3 x, every
// torch op rounding once) on the scaled accumulators; gs = us = 1 for unscaled weights.  The one statement of the chain.
__device__ __forceinline__ float w8a16_silu_mul(float gacc, float gs, float uacc, float us) {
    const float gv = round_bf16(gacc * gs), uv = round_bf16(uacc * us);
    return round_bf16(gv / (1.0f + expf(-gv))) * uv;
}

// Epilogue of the gate / up bodies: K-split reduce of both accumulators over the workgroup's waves (LDS, wave order, on
// wave 0), the rounding chain, then per token two 2-column stores.  red: [WK][MT][2][64] f32x4.  scale: gate scales at
// [0, inter), up scales at [inter, 2 inter).
template <int MT, int WK, class Scale = NoScale>
__device__ __forceinline__ void silu_reduce_store(f32x4 (&ag)[MT], f32x4 (&au)[MT], float* red, bf16_t* out, int M, int inter,
                                                  int m_base, int n0, Scale scale = Scale{}) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: SGPR index math
    const int j = lane & 15, g = lane >> 4;
    if (WK > 1) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            *reinterpret_cast<f32x4*>(&red[((wave * MT + mt) * 128 + lane) * 4]) = ag[mt];
            *reinterpret_cast<f32x4*>(&red[((wave * MT + mt) * 128 + 64 + lane) * 4]) = au[mt];
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            ag[mt] = au[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < WK; ++w) {
                const f32x4 vg = *reinterpret_cast<const f32x4*>(&red[((w * MT + mt) * 128 + lane) * 4]);
                const f32x4 vu = *reinterpret_cast<const f32x4*>(&red[((w * MT + mt) * 128 + 64 + lane) * 4]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ag[mt][r] += vg[r];
                    au[mt][r] += vu[r];
                }
            }
        }
    }
    const auto sg = scale.cols(n0, g, inter), su = scale.shifted(inter).cols(n0, g, inter);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m_base + mt * 16 + j;
        if (m >= M) continue;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const int n = n0 + h2 * 8 + 2 * g;
            float hv[2];
#pragma unroll
            for (int q = 0; q < 2; ++q)
                hv[q] = w8a16_silu_mul(ag[mt][2 * h2 + q], sg[2 * h2 + q], au[mt][2 * h2 + q], su[2 * h2 + q]);
            bf16_t* dst = out + (size_t)m * inter + n;
            if (n + 1 < inter && (inter & 1) == 0) *reinterpret_cast<uint32_t*>(dst) = f32x2_to_bf16x2(hv[0], hv[1]);
            else {
                if (n < inter) dst[0] = f32_to_bf16(hv[0]);
                if (n + 1 < inter) dst[1] = f32_to_bf16(hv[1]);
            }
        }
    }
}

// ---------------------------------------------------------------- gate / up: h = silu(x . W1^T) * (x . W3^T)
// W = [w1; w3] (2 inter x K): a wave owns gate tile [n0, n0+16) and up tile [inter+n0, inter+n0+16) and shares the
// activation fragments between them.
template <class L, int MT, int WK>
__device__ __forceinline__ void stream_gemm_silu(const bf16_t* __restrict__ X, const typename L::weight_t* __restrict__ W,
                                                 typename L::Scale scale, bf16_t* __restrict__ out, int M, int inter, int K,
                                                 int m_base) {
    __shared__ float red[WK > 1 ? WK * MT * 512 : 1];
    StreamLane<L, MT, 4, WK> ln(X, W, M, inter, K, m_base);
    ln.template run<L::template depth<4, MT>(false)>();
    f32x4 ag[MT], au[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        ag[mt] = fold_halves(ln.e[0][mt], ln.o[0][mt], ln.e[1][mt], ln.o[1][mt]);
        au[mt] = fold_halves(ln.e[2][mt], ln.o[2][mt], ln.e[3][mt], ln.o[3][mt]);
    }
    silu_reduce_store<MT, WK>(ag, au, red, out, M, inter, m_base, ln.n0, scale);
}

}  // namespace chitu
