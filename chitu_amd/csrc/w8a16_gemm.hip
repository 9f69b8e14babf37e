// W8A16 weight-only int8 linears (include/chitu_hip_ext6.h), gfx950: bf16 activations x int8 weights, one fp32 scale per
// output row applied to the fp32 accumulator, one rounding.
//
// Replaces (reference, read-only) chitu/quantize/w8a16.py::WeightOnlyLinear.forward, which calls the third-party
// EETQ.w8_a16_gemm.  That kernel's arithmetic is closed; the contract here is the reference's own Triton use_int8_w8a16 branch
// (chitu/fused_moe.py:226-227, 293-294): accumulate x * q in fp32, multiply the accumulator by the row scale.
//
// The decode-shaped kernels are the weight-streaming bodies of stream_gemm.h (the bf16 kernels' of bf16_gemm.hip: 16 output
// rows per workgroup, K split over up to 8 waves and reduced through LDS in wave order, a register ring of in-flight loads, M
// walked in 32-row launches) with the Int8Line policy below.  The K step is 128 elements = one 128-byte line of an int8 row,
// in the full-line layout of gemm_common.h: lane (j, g) loads 16 bytes of weight row n0 + 8*half + j/2 at byte
// ((j%2)*4 + g)*16 of the step, so a wave-load takes whole lines from 8 rows.  MFMA A-row j then holds K elements [0,64)
// (even j) or [64,128) (odd j) of weight row j/2; a lane's 16 bytes are widened to two bf16 operands (elements 0-7 and 8-15
// of its 16) and the step's product is taken with four activation fragments -- x[16g .. 16g+7], x[16g+8 .. 16g+15] of the
// first half (valid on even A-rows) and the same of the second half (valid on odd A-rows) -- the halves added in-lane at the
// end, as the bf16 kernel does.
// K % 128 == 64: the last step is a half line; odd-j lanes re-read the first half (never used: only the "even" products are
// issued for that step) so that no lane reads past its row.
// Every int8 value is exactly a bf16 number and every product exactly an fp32 number: v_mfma_f32_16x16x32_bf16 as is.
#include "common.h"
#include "gemm_common.h"
#include "stream_gemm.h"
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

// int8 weights as a line policy of stream_gemm.h.  K step = 128 elements = one 128-byte line of a weight row; steps >=
// K / 128 are the half-line tail.  A stage holds the lane's 16 bytes of every row group and four activation fragments per
// token tile -- [0], [1]: elements 16g.. and 16g+8.. of the first half; [2], [3]: the same of the second half.
struct Int8Line {
    using weight_t = int8_t;
    using Scale = RowScale;
    // the bf16 kernels' depths but for two token tiles of the plain form.  Rings of 6 and 8 for the single token tile were
    // measured against 4 on the Llama-3-8B and Qwen2-7B shapes (tools/w8a16_ab.py): none faster, wqkv and w2 2 - 8 % slower
    // (180 / 228 VGPRs against 132)
    template <int NW, int MT>
    static constexpr int depth(bool) {
        return MT >= 2 ? 2 : NW == 2 ? 4 : 3;
    }
    template <int MT, int NW>
    struct Stage {
        i32x4 w[NW];
        s16x8 x[MT][4];
    };
    int full_steps, tail, boff, hoff;  // hoff: the lane's half of a full line
    __device__ __forceinline__ Int8Line(int K, int j, int g) : full_steps(K >> 7), tail((K >> 6) & 1), boff(g * 16), hoff((j & 1) * 64) {}
    __device__ __forceinline__ int steps() const { return full_steps + tail; }
    __device__ __forceinline__ int w_off() const { return boff; }
    __device__ __forceinline__ int x_off() const { return boff; }
    template <int MT, int NW>
    __device__ __forceinline__ void load(Stage<MT, NW>& st, const int8_t* const (&wp)[NW], const bf16_t* const (&xp)[MT],
                                         int s) const {
        const bool full = s < full_steps;  // wave-uniform: the half-line tail has no second half
        const int off = s << 7, woff = off + (full ? hoff : 0);
#pragma unroll
        for (int r = 0; r < NW; ++r) st.w[r] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[r] + woff));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            st.x[mt][0] = *reinterpret_cast<const s16x8*>(xp[mt] + off);
            st.x[mt][1] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 8);
            if (full) {
                st.x[mt][2] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 64);
                st.x[mt][3] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 72);
            }
        }
    }
    // e += even-row halves, o += odd-row halves (a full step only)
    template <int MT, int NW>
    __device__ __forceinline__ void mfma(const Stage<MT, NW>& st, f32x4 (&e)[NW][MT], f32x4 (&o)[NW][MT], int s) const {
        const bool full = s < full_steps;
#pragma unroll
        for (int r = 0; r < NW; ++r) {
            const s16x8 lo = widen8(st.w[r][0], st.w[r][1]), hi = widen8(st.w[r][2], st.w[r][3]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                e[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, st.x[mt][0], e[r][mt], 0, 0, 0);
                e[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, st.x[mt][1], e[r][mt], 0, 0, 0);
                if (full) {
                    o[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, st.x[mt][2], o[r][mt], 0, 0, 0);
                    o[r][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, st.x[mt][3], o[r][mt], 0, 0, 0);
                }
            }
        }
    }
};

template <int MT, int WK>
__global__ __launch_bounds__(64 * WK) void w8a16_gemm_kernel(const bf16_t* __restrict__ X, const int8_t* __restrict__ W,
                                                             const float* __restrict__ scale, void* __restrict__ out,
                                                             int out_dt, int M, int N, int K, int m_base) {
    stream_gemm<Int8Line, MT, WK>(X, W, RowScale{scale}, out, out_dt, M, N, K, m_base);
}

// Gate / up projection over w13 = [w1; w3] (int8 [2 inter, K]) with SiluAndMul in the epilogue
template <int MT, int WK>
__global__ __launch_bounds__(64 * WK) void w8a16_gemm_silu_kernel(const bf16_t* __restrict__ X, const int8_t* __restrict__ W,
                                                                  const float* __restrict__ scale, bf16_t* __restrict__ out,
                                                                  int M, int inter, int K, int m_base) {
    stream_gemm_silu<Int8Line, MT, WK>(X, W, RowScale{scale}, out, M, inter, K, m_base);
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
    const int WK = stream_wk(tiles, (K + 127) / 128);  // (mirrored by chitu_amd.ops.w8a16_plan)
    const dim3 grid((unsigned)tiles);
    stream_walk_m(M, WK, [&](int mbase, auto mt, auto wk) {
        constexpr int MT = decltype(mt)::value, WKV = decltype(wk)::value;
        hipLaunchKernelGGL((w8a16_gemm_kernel<MT, WKV>), grid, dim3(64 * WKV), 0, st, (const bf16_t*)x_bf16,
                           (const int8_t*)w_int8, scale_f32, out, (int)out_dtype, (int)M, (int)N, (int)K, mbase);
    });
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
    const int WK = stream_wk(tiles, (K + 127) / 128);
    const dim3 grid((unsigned)tiles);
    stream_walk_m(M, WK, [&](int mbase, auto mt, auto wk) {
        constexpr int MT = decltype(mt)::value, WKV = decltype(wk)::value;
        hipLaunchKernelGGL((w8a16_gemm_silu_kernel<MT, WKV>), grid, dim3(64 * WKV), 0, st, (const bf16_t*)x_bf16,
                           (const int8_t*)w13_int8, scale_f32, (bf16_t*)out_bf16, (int)M, (int)inter, (int)K, mbase);
    });
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
