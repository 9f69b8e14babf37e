// W8A16 weight-only int8 linears (include/chitu_hip_ext6.h), gfx950: bf16 activations x int8 weights, one fp32 scale per
// output row applied to the fp32 accumulator, one rounding.
//
// Replaces (reference, read-only) chitu/quantize/w8a16.py::WeightOnlyLinear.forward, which calls the third-party
// EETQ.w8_a16_gemm.  That kernel's arithmetic is closed; the contract here is the reference's own Triton use_int8_w8a16 branch
// (chitu/fused_moe.py:226-227, 293-294): accumulate x * q in fp32, multiply the accumulator by the row scale.
//
// The decode-shaped kernels have the structure of bf16_gemm_kernel / bf16_gemm_silu_kernel (gate.hip): 16 output rows per
// workgroup, K split over up to 8 waves and reduced through LDS in wave order, a register ring of in-flight loads, M walked
// in 32-row launches.  The K step is 128 elements = one 128-byte line of an int8 row, in the full-line layout of
// gemm_common.h: lane (j, g) loads 16 bytes of weight row n0 + 8*half + j/2 at byte ((j%2)*4 + g)*16 of the step, so a
// wave-load takes whole lines from 8 rows.  MFMA A-row j then holds K elements [0,64) (even j) or [64,128) (odd j) of weight
// row j/2; a lane's 16 bytes are widened to two bf16 operands (elements 0-7 and 8-15 of its 16) and the step's product is
// taken with four activation fragments -- x[16g .. 16g+7], x[16g+8 .. 16g+15] of the first half (valid on even A-rows) and
// the same of the second half (valid on odd A-rows) -- the halves added in-lane at the end, as the bf16 kernel does.
// K % 128 == 64: the last step is a half line; odd-j lanes re-read the first half (never used: only the "even" products are
// issued for that step) so that no lane reads past its row.
// Every int8 value is exactly a bf16 number and every product exactly an fp32 number: v_mfma_f32_16x16x32_bf16 as is.
#include "common.h"
#include "gemm_common.h"
#include "../../include/chitu_hip_ext6.h"

namespace chitu {

// 4 int8 bytes -> 4 bf16 (exact): sign-extend, convert, keep the high half of the fp32 (|v| <= 128 has <= 8 significant bits)
__device__ __forceinline__ uint32_t widen_pair(int w, int b) {
    const float lo = (float)((int)((uint32_t)w << (24 - 8 * b)) >> 24), hi = (float)((int)((uint32_t)w << (16 - 8 * b)) >> 24);
    return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}
__device__ __forceinline__ s16x8 widen8(int w0, int w1) {
    i32x4 r;
    r[0] = (int)widen_pair(w0, 0);
    r[1] = (int)widen_pair(w0, 2);
    r[2] = (int)widen_pair(w1, 0);
    r[3] = (int)widen_pair(w1, 2);
    return __builtin_bit_cast(s16x8, r);
}

// what a wave needs of one 128-element K step: its 16 bytes of two weight row groups, four activation fragments per token tile
template <int MT, int NW>
struct W8A16Stage {
    i32x4 w[NW];
    s16x8 x[MT][4];  // [0], [1]: elements 16g.. and 16g+8.. of the first half; [2], [3]: the same of the second half
};

template <int MT>
__device__ __forceinline__ void w8a16_load_x(s16x8 (&x)[MT][4], const bf16_t* const (&xp)[MT], int off, bool full) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        x[mt][0] = *reinterpret_cast<const s16x8*>(xp[mt] + off);
        x[mt][1] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 8);
        if (full) {  // wave-uniform: the half-line tail has no second half
            x[mt][2] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 64);
            x[mt][3] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 72);
        }
    }
}

// the step's product for one weight row group: e += even-row halves, o += odd-row halves
template <int MT>
__device__ __forceinline__ void w8a16_mfma(const i32x4& w, const s16x8 (&x)[MT][4], f32x4 (&e)[MT], f32x4 (&o)[MT], bool full) {
    const s16x8 lo = widen8(w[0], w[1]), hi = widen8(w[2], w[3]);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        e[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, x[mt][0], e[mt], 0, 0, 0);
        e[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, x[mt][1], e[mt], 0, 0, 0);
        if (full) {
            o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, x[mt][2], o[mt], 0, 0, 0);
            o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, x[mt][3], o[mt], 0, 0, 0);
        }
    }
}

// the wave's share [s0, s1) of the NB = ceil(K / 128) steps; steps >= K / 128 are the half-line tail
struct W8A16Steps {
    int s0, s1, full_steps;
};
__device__ __forceinline__ W8A16Steps w8a16_steps(int K, int wave, int WK) {
    const int full_steps = K >> 7, NB = full_steps + ((K >> 6) & 1);
    return W8A16Steps{NB * wave / WK, NB * (wave + 1) / WK, full_steps};
}

template <int MT, int WK>
__global__ __launch_bounds__(64 * WK) void w8a16_gemm_kernel(const bf16_t* __restrict__ X, const int8_t* __restrict__ W,
                                                             const float* __restrict__ scale, void* __restrict__ out,
                                                             int out_dt, int M, int N, int K, int m_base) {
    __shared__ float red[WK > 1 ? WK * MT * 256 : 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: SGPR index math
    const int j = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const W8A16Steps ws = w8a16_steps(K, wave, WK);
    const int boff = g * 16, hoff = (j & 1) * 64;  // byte of the lane inside a half line; its half
    const int8_t* wp0 = W + (size_t)min(n0 + (j >> 1), N - 1) * K + boff;
    const int8_t* wp1 = W + (size_t)min(n0 + 8 + (j >> 1), N - 1) * K + boff;
    const bf16_t* xp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xp[mt] = X + (size_t)min(m_base + mt * 16 + j, M - 1) * K + g * 16;
    f32x4 e0[MT], o0[MT], e1[MT], o1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) e0[mt] = o0[mt] = e1[mt] = o1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    using Stage = W8A16Stage<MT, 2>;
    auto load = [&](Stage& st, int s) {
        const bool full = s < ws.full_steps;
        const int off = (s << 7) + (full ? hoff : 0);
        st.w[0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp0 + off));
        st.w[1] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp1 + off));
        w8a16_load_x<MT>(st.x, xp, s << 7, full);
    };
    auto compute = [&](const Stage& st, int s) {
        const bool full = s < ws.full_steps;
        w8a16_mfma<MT>(st.w[0], st.x, e0, o0, full);
        w8a16_mfma<MT>(st.w[1], st.x, e1, o1, full);
    };
    // the bf16 kernel's depths.  Rings of 6 and 8 for the single token tile were measured against 4 on the Llama-3-8B and
    // Qwen2-7B shapes (tools/w8a16_ab.py): none faster, wqkv and w2 2 - 8 % slower (180 / 228 VGPRs against 132)
    constexpr int D = MT >= 2 ? 2 : 4;
    Stage ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (ws.s0 + d < ws.s1) load(ring[d], ws.s0 + d);
    for (int s = ws.s0; s < ws.s1; s += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (s + d < ws.s1) {
                compute(ring[d], s + d);
                if (s + d + D < ws.s1) load(ring[d], s + d + D);
            }
        }
    }
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
        acc[mt] = f32x4{e0[mt][0] + o0[mt][1], e0[mt][2] + o0[mt][3], e1[mt][0] + o1[mt][1], e1[mt][2] + o1[mt][3]};
    // K-split reduce in wave order, then token tile mt is scaled and stored by wave mt % WK
    float sc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = scale[min(w8_out_col(n0, g, r), N - 1)];
    auto store = [&](int mt, const f32x4& v) {
        const int m = m_base + mt * 16 + j;
        if (m >= M) return;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = n0 + h * 8 + 2 * g;
            const float a = v[2 * h] * sc[2 * h], b = v[2 * h + 1] * sc[2 * h + 1];
            if (out_dt == 2) {
                float* dst = (float*)out + (size_t)m * N + n;
                if (n < N) dst[0] = a;
                if (n + 1 < N) dst[1] = b;
            } else {
                uint16_t* dst = (uint16_t*)out + (size_t)m * N + n;
                const uint16_t ha = out_dt == 0 ? f32_to_bf16(a) : f32_to_f16(a);
                const uint16_t hb = out_dt == 0 ? f32_to_bf16(b) : f32_to_f16(b);
                if (n + 1 < N && (N & 1) == 0) *reinterpret_cast<uint32_t*>(dst) = (uint32_t)ha | ((uint32_t)hb << 16);
                else {
                    if (n < N) dst[0] = ha;
                    if (n + 1 < N) dst[1] = hb;
                }
            }
        }
    };
    if (WK > 1) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f32x4*>(&red[((wave * MT + mt) * 64 + lane) * 4]) = acc[mt];
        __syncthreads();
        for (int mt = wave; mt < MT; mt += WK) {
            f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < WK; ++w) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&red[((w * MT + mt) * 64 + lane) * 4]);
#pragma unroll
                for (int r = 0; r < 4; ++r) sum[r] += v[r];
            }
            store(mt, sum);
        }
    } else {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) store(mt, acc[mt]);
    }
}

// h = bf16( bf16(silu(bf16(g))) * bf16(u) ): bf16_gemm_silu_kernel's chain (gate.hip) on the scaled accumulators
__device__ __forceinline__ float w8a16_silu_mul(float gacc, float gs, float uacc, float us) {
    const float gv = round_bf16(gacc * gs), uv = round_bf16(uacc * us);
    return round_bf16(gv / (1.0f + expf(-gv))) * uv;
}

// Gate / up projection over w13 = [w1; w3] (int8 [2 inter, K]) with SiluAndMul in the epilogue: a wave owns gate tile
// [n0, n0+16) and up tile [inter+n0, inter+n0+16) and shares the activation fragments between them.
template <int MT, int WK>
__global__ __launch_bounds__(64 * WK) void w8a16_gemm_silu_kernel(const bf16_t* __restrict__ X, const int8_t* __restrict__ W,
                                                                  const float* __restrict__ scale, bf16_t* __restrict__ out,
                                                                  int M, int inter, int K, int m_base) {
    __shared__ float red[WK > 1 ? WK * MT * 512 : 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: SGPR index math
    const int j = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const W8A16Steps ws = w8a16_steps(K, wave, WK);
    const int boff = g * 16, hoff = (j & 1) * 64;
    const int r0 = min(n0 + (j >> 1), inter - 1), r1 = min(n0 + 8 + (j >> 1), inter - 1);
    const int8_t* gp0 = W + (size_t)r0 * K + boff;
    const int8_t* gp1 = W + (size_t)r1 * K + boff;
    const int8_t* up0 = W + (size_t)(inter + r0) * K + boff;
    const int8_t* up1 = W + (size_t)(inter + r1) * K + boff;
    const bf16_t* xp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xp[mt] = X + (size_t)min(m_base + mt * 16 + j, M - 1) * K + g * 16;
    f32x4 ge0[MT], go0[MT], ge1[MT], go1[MT], ue0[MT], uo0[MT], ue1[MT], uo1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
        ge0[mt] = go0[mt] = ge1[mt] = go1[mt] = ue0[mt] = uo0[mt] = ue1[mt] = uo1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    using Stage = W8A16Stage<MT, 4>;
    auto load = [&](Stage& st, int s) {
        const bool full = s < ws.full_steps;
        const int off = (s << 7) + (full ? hoff : 0);
        st.w[0] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(gp0 + off));
        st.w[1] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(gp1 + off));
        st.w[2] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(up0 + off));
        st.w[3] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(up1 + off));
        w8a16_load_x<MT>(st.x, xp, s << 7, full);
    };
    auto compute = [&](const Stage& st, int s) {
        const bool full = s < ws.full_steps;
        w8a16_mfma<MT>(st.w[0], st.x, ge0, go0, full);
        w8a16_mfma<MT>(st.w[1], st.x, ge1, go1, full);
        w8a16_mfma<MT>(st.w[2], st.x, ue0, uo0, full);
        w8a16_mfma<MT>(st.w[3], st.x, ue1, uo1, full);
    };
    constexpr int D = MT >= 2 ? 2 : 3;
    Stage ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (ws.s0 + d < ws.s1) load(ring[d], ws.s0 + d);
    for (int s = ws.s0; s < ws.s1; s += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (s + d < ws.s1) {
                compute(ring[d], s + d);
                if (s + d + D < ws.s1) load(ring[d], s + d + D);
            }
        }
    }
    f32x4 ag[MT], au[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        ag[mt] = f32x4{ge0[mt][0] + go0[mt][1], ge0[mt][2] + go0[mt][3], ge1[mt][0] + go1[mt][1], ge1[mt][2] + go1[mt][3]};
        au[mt] = f32x4{ue0[mt][0] + uo0[mt][1], ue0[mt][2] + uo0[mt][3], ue1[mt][0] + uo1[mt][1], ue1[mt][2] + uo1[mt][3]};
    }
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
    float sg[4], su[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = min(w8_out_col(n0, g, r), inter - 1);
        sg[r] = scale[c];
        su[r] = scale[inter + c];
    }
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

// out[i] = bf16(q[i]), 16 bytes in, 32 bytes out per thread
__global__ __launch_bounds__(256) void w8a16_widen_kernel(const int8_t* __restrict__ W, bf16_t* __restrict__ out, int64_t chunks) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    const i32x4 w = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(W + c * 16));
    s16x8* dst = reinterpret_cast<s16x8*>(out + c * 16);
    dst[0] = widen8(w[0], w[1]);
    dst[1] = widen8(w[2], w[3]);
}

// the epilogue of the widen + tiled-GEMM form: one thread per output element (pairs of them for silu = false would save
// nothing measurable: the launch is a fraction of the GEMM in front of it)
template <bool SILU>
__global__ __launch_bounds__(256) void w8a16_scale_round_kernel(const float* __restrict__ acc, const float* __restrict__ scale,
                                                                void* __restrict__ out, int out_dt, int64_t M, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * N) return;
    const int64_t m = i / N, n = i - m * N;
    if (SILU) {
        const float* row = acc + m * 2 * N;
        ((bf16_t*)out)[i] = f32_to_bf16(w8a16_silu_mul(row[n], scale[n], row[N + n], scale[N + n]));
        return;
    }
    const float v = acc[i] * scale[n];
    if (out_dt == 2) ((float*)out)[i] = v;
    else ((uint16_t*)out)[i] = out_dt == 0 ? f32_to_bf16(v) : f32_to_f16(v);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// K-split width of both streaming launchers (mirrored by chitu_amd.ops.w8a16_plan): the widest power of two <= 8 that leaves
// every wave a step and the launch at most 4096 waves' worth of workgroups x waves, as chitu_hip_bf16_gemm chooses
static inline int w8a16_wk(int64_t tiles, int64_t K) {
    const int NB = (int)(K / 128 + (K % 128 ? 1 : 0));
    int WK = 8;
    while (WK > 1 && (WK > NB || tiles * WK > 4096)) WK >>= 1;
    return WK;
}

}  // namespace chitu

extern "C" int chitu_ext6_w8a16_gemm(const void* x_bf16, const void* w_int8, const float* scale_f32, void* out,
                                     int32_t out_dtype, int64_t M, int64_t N, int64_t K, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(x_bf16 && w_int8 && scale_f32 && out);
    CHITU_REQUIRE(aligned16(x_bf16) && aligned16(w_int8) && aligned16(scale_f32) && aligned16(out));
    CHITU_REQUIRE(out_dtype >= 0 && out_dtype <= 2);
    CHITU_REQUIRE(M >= 0 && M < (1 << 30) && N >= 1 && N < (1 << 30) && K >= 1 && K < (1 << 30));
    if (K % 64 != 0) return CHITU_ERR_UNSUPPORTED;
    if (M == 0) return CHITU_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = (N + 15) / 16;
    const int WK = w8a16_wk(tiles, K);
    const dim3 grid((unsigned)tiles);
#define LAUNCH(MT, WKV)                                                                                          \
    hipLaunchKernelGGL((w8a16_gemm_kernel<MT, WKV>), grid, dim3(64 * WKV), 0, st, (const bf16_t*)x_bf16,           \
                       (const int8_t*)w_int8, scale_f32, out, (int)out_dtype, (int)M, (int)N, (int)K, mbase)
#define LAUNCH_WK(MT)                      \
    switch (WK) {                          \
        case 8: LAUNCH(MT, 8); break;      \
        case 4: LAUNCH(MT, 4); break;      \
        case 2: LAUNCH(MT, 2); break;      \
        default: LAUNCH(MT, 1); break;     \
    }
    for (int64_t mb = 0; mb < M; mb += 32) {
        const int mbase = (int)mb;
        if (M - mb <= 16) { LAUNCH_WK(1) } else { LAUNCH_WK(2) }
    }
#undef LAUNCH_WK
#undef LAUNCH
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_ext6_w8a16_gemm_silu(const void* x_bf16, const void* w13_int8, const float* scale_f32, void* out_bf16,
                                          int64_t M, int64_t inter, int64_t K, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(x_bf16 && w13_int8 && scale_f32 && out_bf16);
    CHITU_REQUIRE(aligned16(x_bf16) && aligned16(w13_int8) && aligned16(scale_f32) && aligned16(out_bf16));
    CHITU_REQUIRE(M >= 0 && M < (1 << 30) && inter >= 1 && inter < (1 << 29) && K >= 1 && K < (1 << 30));
    if (K % 64 != 0) return CHITU_ERR_UNSUPPORTED;
    if (M == 0) return CHITU_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = (inter + 15) / 16;
    const int WK = w8a16_wk(tiles, K);
    const dim3 grid((unsigned)tiles);
#define LAUNCHS(MT, WKV)                                                                                         \
    hipLaunchKernelGGL((w8a16_gemm_silu_kernel<MT, WKV>), grid, dim3(64 * WKV), 0, st, (const bf16_t*)x_bf16,      \
                       (const int8_t*)w13_int8, scale_f32, (bf16_t*)out_bf16, (int)M, (int)inter, (int)K, mbase)
#define LAUNCHS_WK(MT)                   \
    switch (WK) {                        \
        case 8: LAUNCHS(MT, 8); break;   \
        case 4: LAUNCHS(MT, 4); break;   \
        case 2: LAUNCHS(MT, 2); break;   \
        default: LAUNCHS(MT, 1); break;  \
    }
    for (int64_t mb = 0; mb < M; mb += 32) {
        const int mbase = (int)mb;
        if (M - mb <= 16) { LAUNCHS_WK(1) } else { LAUNCHS_WK(2) }
    }
#undef LAUNCHS_WK
#undef LAUNCHS
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_ext6_w8a16_widen(const void* w_int8, void* out_bf16, int64_t N, int64_t K, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(w_int8 && out_bf16 && aligned16(w_int8) && aligned16(out_bf16));
    CHITU_REQUIRE(N >= 0 && N < (1 << 30) && K >= 1 && K < (1 << 30));
    if (K % 16 != 0) return CHITU_ERR_UNSUPPORTED;
    if (N == 0) return CHITU_OK;
    const int64_t chunks = N * K / 16, blocks = (chunks + 255) / 256;
    CHITU_REQUIRE(blocks < (1ll << 31));
    hipLaunchKernelGGL(w8a16_widen_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const int8_t*)w_int8,
                       (bf16_t*)out_bf16, chunks);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_ext6_w8a16_scale_round(const float* acc_f32, const float* scale_f32, void* out, int32_t out_dtype,
                                            int64_t M, int64_t N, int32_t silu, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(acc_f32 && scale_f32 && out && aligned16(acc_f32) && aligned16(scale_f32) && aligned16(out));
    CHITU_REQUIRE(out_dtype >= 0 && out_dtype <= 2 && (silu == 0 || (silu == 1 && out_dtype == 0)));
    CHITU_REQUIRE(M >= 0 && M < (1 << 30) && N >= 1 && N < (1 << 29));
    if (M == 0) return CHITU_OK;
    const int64_t blocks = (M * N + 255) / 256;
    CHITU_REQUIRE(blocks < (1ll << 31));
    if (silu)
        hipLaunchKernelGGL(w8a16_scale_round_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc_f32,
                           scale_f32, out, (int)out_dtype, M, N);
    else
        hipLaunchKernelGGL(w8a16_scale_round_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc_f32,
                           scale_f32, out, (int)out_dtype, M, N);
    CHITU_RETURN_LAUNCH_STATUS();
}
