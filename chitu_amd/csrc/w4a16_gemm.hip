// W4A16 group-128 weight-only int4 linears (include/chitu_hip_ext9.h), gfx950: bf16 activations x 4-bit codes, one fp32 scale
// per weight row and 128 input channels.
//
// The format most quantised Llama / Qwen checkpoints are published in (GPTQ sym=true: code u in 0..15, value u - 8).  The
// reference serves it through third-party CUDA kernels only (AutoGPTQ, awq_inference_engine); the contract here is stated in
// the header: per group an fp32 sum of exact products x * (u - 8), one fp32 multiply-add with the group scale, one rounding.
//
// The decode-shaped kernels are the weight-streaming bodies of stream_gemm.h with the Int4Line policy below.  The K step is
// 256 channels = one 128-byte line of a packed row, in the full-line layout of gemm_common.h: lane (j, g) loads 16 bytes of
// weight row n0 + 8*half + j/2 at byte (j%2)*64 + g*16 of the step.  MFMA A-row j then holds 128 channels -- even j the first
// half of the line, odd j the second -- which is exactly ONE scale group: the step's products go into a fresh accumulator
// (pe with the activations of the first half, valid on even A-rows; po with those of the second, valid on odd ones) and
// that is folded into the running e / o accumulators with the A-row's group scale, the fold the block-fp8 GEMMs do.
//
// Packed layout (quantize/w4a16.py::pack_w4a16 is its only other statement).  Channel k of a row sits in byte
// (k / 8) * 4 + k % 4, low nibble for k % 8 < 4, high nibble otherwise, as the two's-complement nibble of u - 8 (u ^ 8).  A
// dword therefore holds 8 consecutive channels: (w << 4) & 0xf0f0f0f0 is channels 0-3 and w & 0xf0f0f0f0 channels 4-7, each a
// signed byte 16 * (u - 8), which one sign-extending byte convert turns into an fp32 whose high half is the exact bf16; a
// byte permute packs two of them.  3 + 8 + 4 VALU operations per 8 codes, no subtraction of the zero point and no table;
// the factor 16 leaves through the group scale (s / 16 is exact).  A lane's dword q is the MFMA operand of K elements
// 8q .. 8q+7 of its 32 channels, multiplied with the activation fragment x[32g + 8q ..].
// Scales: fp32 [ceil(rows / 2)][ceil(K / 256)][2][2] -- for a row pair and a K step, {row 2p: group 2s, 2s+1; row 2p+1:
// group 2s, 2s+1}, zero where a row or a group does not exist.  Lane (j, g) holds accumulator A-rows 4g .. 4g+3 = rows 2g,
// 2g+1 of the row group in both halves: its four scales of a step are ONE 16-byte load.  w13 = [w1; w3] stores the pairs of
// w1 and of w3 one after the other (ceil(inter / 2) each).
// K % 256 == 128: the last step is a half line; odd-j lanes re-read the first half (never used: only the "even" products are
// issued for that step) so that no lane reads past its row.
#include "common.h"
#include "gemm_common.h"
#include "stream_gemm.h"
#include "../../include/chitu_hip_ext9.h"

namespace chitu {

// fp32 of signed byte b of t: v_cvt_f32_i32 with a sign-extending byte select
__device__ __forceinline__ float sbyte_f32(uint32_t t, int b) { return (float)(int)(int8_t)(t >> (8 * b)); }
// the high halves of two fp32 as one bf16 pair (exact values: truncation is the conversion)
__device__ __forceinline__ int pack_hi(float lo, float hi) {
    return (int)__builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
// one dword = 8 codes -> 8 bf16 of 16 * (u - 8), channels in order
__device__ __forceinline__ s16x8 widen_nibbles(int w) {
    const uint32_t lo = ((uint32_t)w << 4) & 0xf0f0f0f0u, hi = (uint32_t)w & 0xf0f0f0f0u;
    i32x4 r;
    r[0] = pack_hi(sbyte_f32(lo, 0), sbyte_f32(lo, 1));
    r[1] = pack_hi(sbyte_f32(lo, 2), sbyte_f32(lo, 3));
    r[2] = pack_hi(sbyte_f32(hi, 0), sbyte_f32(hi, 1));
    r[3] = pack_hi(sbyte_f32(hi, 2), sbyte_f32(hi, 3));
    return __builtin_bit_cast(s16x8, r);
}

// The group scales of a launch: q as laid out above, `pairs` row pairs per matrix (the up matrix of w13 starts `pairs`
// further down), `steps` K steps per pair.  To the epilogues it is NoScale: the accumulators arrive scaled.
struct GroupScale : NoScale {
    const f32x4* q;
    int pairs, steps;
};

// int4 codes as a line policy of stream_gemm.h.  K step = 256 channels = one 128-byte line of a packed row; step K / 256 is
// the half-line tail.  A stage holds the lane's 16 bytes and its four scales of every row group and eight activation fragments
// per token tile -- [0..3]: channels 32g + 8q .. of the first half; [4..7]: the same of the second half.
struct Int4Line {
    using weight_t = uint8_t;
    using Scale = GroupScale;
    static __device__ __forceinline__ int w_stride(int K) { return K >> 1; }
    // Int8Line's depths for the plain form (4, two token tiles 2: 248 / 236 VGPRs, no spill).  The gate / up form holds four
    // row groups per stage: at Int8Line's 3 / 2 its 8-wave kernels (256 registers a lane) spilled 49 / 109 VGPRs, so it runs
    // at 2, two token tiles at 1 (212 / 236 VGPRs, no spill) -- DESIGN 3.25
    template <int NW, int MT>
    static constexpr int depth(bool) {
        return NW == 2 ? (MT >= 2 ? 2 : 4) : MT >= 2 ? 1 : 2;
    }
    template <int MT, int NW>
    struct Stage {
        i32x4 w[NW];
        f32x4 sc[NW];
        s16x8 x[MT][8];
    };
    int full_steps, tail, g, boff, hoff;  // hoff: the lane's half of a full line
    const f32x4* sp[4];                   // the lane's scale rows: row pair (n0 + 8 (r & 1)) / 2 + g of matrix r / 2
    __device__ __forceinline__ Int4Line(int K, int j, int g_)
        : full_steps(K >> 8), tail((K >> 7) & 1), g(g_), boff(g_ * 16), hoff((j & 1) * 64) {}
    template <int NW>
    __device__ __forceinline__ void bind(const GroupScale& s, int, int n0) {
        static_for<NW>([&](auto r) { sp[r] = s.q + (size_t)((r >> 1) * s.pairs + min(((n0 + (r & 1) * 8) >> 1) + g, s.pairs - 1)) * s.steps; });
    }
    __device__ __forceinline__ int steps() const { return full_steps + tail; }
    __device__ __forceinline__ int w_off() const { return boff; }
    __device__ __forceinline__ int x_off() const { return boff * 2; }
    template <int MT, int NW>
    __device__ __forceinline__ void load(Stage<MT, NW>& st, const uint8_t* const (&wp)[NW], const bf16_t* const (&xp)[MT],
                                         int s) const {
        const bool full = s < full_steps;  // wave-uniform: the half-line tail has no second half
        const int off = s << 8, woff = (s << 7) + (full ? hoff : 0);
#pragma unroll
        for (int r = 0; r < NW; ++r) {
            st.w[r] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[r] + woff));
            st.sc[r] = sp[r][s];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            static_for<4>([&](auto q) { st.x[mt][q] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 8 * q); });
            if (full) static_for<4>([&](auto q) { st.x[mt][4 + q] = *reinterpret_cast<const s16x8*>(xp[mt] + off + 128 + 8 * q); });
        }
    }
    // e += scale * even-row halves, o += scale * odd-row halves (a full step only).  Elements 1, 3 of e and 0, 2 of o belong
    // to the other half's rows: fold_halves never reads them and they stay zero.
    template <int MT, int NW>
    __device__ __forceinline__ void mfma(const Stage<MT, NW>& st, f32x4 (&e)[NW][MT], f32x4 (&o)[NW][MT], int s) const {
        const bool full = s < full_steps;
        const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < NW; ++r) {
            const s16x8 a[4] = {widen_nibbles(st.w[r][0]), widen_nibbles(st.w[r][1]), widen_nibbles(st.w[r][2]), widen_nibbles(st.w[r][3])};
            const f32x4 sc = st.sc[r] * 0.0625f;  // the operands are 16 (u - 8)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                f32x4 pe = z;
                static_for<4>([&](auto q) { pe = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[q], st.x[mt][q], pe, 0, 0, 0); });
                e[r][mt][0] = __builtin_fmaf(pe[0], sc[0], e[r][mt][0]);
                e[r][mt][2] = __builtin_fmaf(pe[2], sc[2], e[r][mt][2]);
                if (full) {
                    f32x4 po = z;
                    static_for<4>([&](auto q) { po = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[q], st.x[mt][4 + q], po, 0, 0, 0); });
                    o[r][mt][1] = __builtin_fmaf(po[1], sc[1], o[r][mt][1]);
                    o[r][mt][3] = __builtin_fmaf(po[3], sc[3], o[r][mt][3]);
                }
            }
        }
    }
};

template <int MT, int WK>
__global__ __launch_bounds__(64 * WK) void w4a16_gemm_kernel(const bf16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                             GroupScale scale, void* __restrict__ out, int out_dt, int M, int N,
                                                             int K, int m_base) {
    stream_gemm<Int4Line, MT, WK>(X, W, scale, out, out_dt, M, N, K, m_base);
}

// Gate / up projection over w13 = [w1; w3] (packed [2 inter, K / 2]) with SiluAndMul in the epilogue
template <int MT, int WK>
__global__ __launch_bounds__(64 * WK) void w4a16_gemm_silu_kernel(const bf16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                                  GroupScale scale, bf16_t* __restrict__ out, int M, int inter,
                                                                  int K, int m_base) {
    stream_gemm_silu<Int4Line, MT, WK>(X, W, scale, out, M, inter, K, m_base);
}

// out[n][k] = bf16(float(u - 8) * s[n][k / 128]): 16 bytes = 32 channels of one group in, 64 bytes out per thread
__global__ __launch_bounds__(256) void w4a16_widen_kernel(const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                          bf16_t* __restrict__ out, int64_t chunks, int chunks_per_row, int steps) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    const int64_t n = c / chunks_per_row;
    const int grp = (int)(c - n * chunks_per_row) >> 2;  // 4 chunks of 32 channels per group
    const float s = scale[(((n >> 1) * steps + (grp >> 1)) * 2 + (n & 1)) * 2 + (grp & 1)];
    const i32x4 w = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(W + c * 16));
    i32x4* dst = reinterpret_cast<i32x4*>(out + c * 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        i32x4 r;
#pragma unroll
        for (int p = 0; p < 4; ++p) {  // channels 2p, 2p+1 of the dword: nibbles at bits 8 (2p % 4) + 4 (2p / 4) and 8 further up
            const int sh = 28 - 16 * (p & 1) - 4 * (p >> 1);
            const float a = (float)((int)((uint32_t)w[q] << sh) >> 28) * s, b = (float)((int)((uint32_t)w[q] << (sh - 8)) >> 28) * s;
            r[p] = (int)f32x2_to_bf16x2(a, b);
        }
        dst[q] = r;
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace chitu

extern "C" int chitu_ext9_w4a16_gemm(const void* x_bf16, const void* w_packed, const float* scale_f32, void* out,
                                     int32_t out_dtype, int64_t M, int64_t N, int64_t K, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(x_bf16 && w_packed && scale_f32 && out);
    CHITU_REQUIRE(aligned16(x_bf16) && aligned16(w_packed) && aligned16(scale_f32) && aligned16(out));
    CHITU_REQUIRE(out_dtype >= 0 && out_dtype <= 2);
    CHITU_REQUIRE(M >= 0 && M < (1 << 30) && N >= 1 && N < (1 << 30) && K >= 1 && K < (1 << 30));
    if (K % 128 != 0) return CHITU_ERR_UNSUPPORTED;
    if (M == 0) return CHITU_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = (N + 15) / 16, steps = (K + 255) / 256;
    const int WK = stream_wk(tiles, steps);  // (mirrored by chitu_amd.ops.w4a16_plan)
    const GroupScale gs{{}, (const f32x4*)scale_f32, (int)((N + 1) / 2), (int)steps};
    const dim3 grid((unsigned)tiles);
    stream_walk_m(M, WK, [&](int mbase, auto mt, auto wk) {
        constexpr int MT = decltype(mt)::value, WKV = decltype(wk)::value;
        hipLaunchKernelGGL((w4a16_gemm_kernel<MT, WKV>), grid, dim3(64 * WKV), 0, st, (const bf16_t*)x_bf16,
                           (const uint8_t*)w_packed, gs, out, (int)out_dtype, (int)M, (int)N, (int)K, mbase);
    });
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_ext9_w4a16_gemm_silu(const void* x_bf16, const void* w13_packed, const float* scale_f32, void* out_bf16,
                                          int64_t M, int64_t inter, int64_t K, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(x_bf16 && w13_packed && scale_f32 && out_bf16);
    CHITU_REQUIRE(aligned16(x_bf16) && aligned16(w13_packed) && aligned16(scale_f32) && aligned16(out_bf16));
    CHITU_REQUIRE(M >= 0 && M < (1 << 30) && inter >= 1 && inter < (1 << 29) && K >= 1 && K < (1 << 30));
    if (K % 128 != 0) return CHITU_ERR_UNSUPPORTED;
    if (M == 0) return CHITU_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = (inter + 15) / 16, steps = (K + 255) / 256;
    const int WK = stream_wk(tiles, steps);
    const GroupScale gs{{}, (const f32x4*)scale_f32, (int)((inter + 1) / 2), (int)steps};
    const dim3 grid((unsigned)tiles);
    stream_walk_m(M, WK, [&](int mbase, auto mt, auto wk) {
        constexpr int MT = decltype(mt)::value, WKV = decltype(wk)::value;
        hipLaunchKernelGGL((w4a16_gemm_silu_kernel<MT, WKV>), grid, dim3(64 * WKV), 0, st, (const bf16_t*)x_bf16,
                           (const uint8_t*)w13_packed, gs, (bf16_t*)out_bf16, (int)M, (int)inter, (int)K, mbase);
    });
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_ext9_w4a16_widen(const void* w_packed, const float* scale_f32, void* out_bf16, int64_t N, int64_t K,
                                      void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(w_packed && scale_f32 && out_bf16 && aligned16(w_packed) && aligned16(scale_f32) && aligned16(out_bf16));
    CHITU_REQUIRE(N >= 0 && N < (1 << 30) && K >= 1 && K < (1 << 30));
    if (K % 128 != 0) return CHITU_ERR_UNSUPPORTED;
    if (N == 0) return CHITU_OK;
    const int64_t chunks = N * K / 32, blocks = (chunks + 255) / 256;
    CHITU_REQUIRE(blocks < (1ll << 31));
    hipLaunchKernelGGL(w4a16_widen_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)w_packed,
                       scale_f32, (bf16_t*)out_bf16, chunks, (int)(K / 32), (int)((K + 255) / 256));
    CHITU_RETURN_LAUNCH_STATUS();
}
