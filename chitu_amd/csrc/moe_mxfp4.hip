// Fused MoE for decode with MXFP4 expert weights (W4A8) on gfx950: grouped GEMMs of e4m3 activations (per-128-group fp32
// scales, as in moe.hip) with OCP MX v1.0 weights -- packed e2m1, two per byte (low nibble = even k), one E8M0 scale byte per
// 32 consecutive k of a row.  New: no reference counterpart (the reference has no 4-bit float expert mode); the arithmetic
// around the weight operand is moe.hip's, rounding point for rounding point.
//
// The 128-wide block dot is ONE v_mfma_scale_f32_16x16x128_f8f6f4 per (weight fragment, activation fragment): A = the e2m1
// weights (format 4, four VGPRs) with their own E8M0 bytes as the hardware scale operand, B = the e4m3 activations with unit
// scale 0x7f.  Lane map, measured with exact data (tests/test_gpu_moe_mxfp4.py): lane (j, g) of the FP4 operand carries
// k = 32g .. 32g+31 of its row's block -- its 16 bytes are exactly one aligned MX block and carry the lane's one scale byte --,
// while lane (j, g) of the FP8 operand carries k = 16g .. 16g+15 in its first four registers and k = 64+16g .. 64+16g+15 in
// the last four (the fragment mfma_fp8_k128 and w8a8_block_dot already load).  The fp32 block result is multiplied by the
// activation's group scale and accumulated in fp32, K blocks ascending.
//
// Streaming mirrors moe.hip: a wave owns 16 weight rows, a register ring of weight loads runs several steps ahead, loads are
// non-temporal and every wave-load takes whole 128-B lines (gemm_common.h: 6.5-6.8 TB/s against <= 5.1 for half lines).  A
// row's line is now 256 k = TWO K blocks, so a step is a K-block pair: lane (j, g) loads 16 B of weight row n0 + 8*half + j/2
// at byte ((j%2)*4 + g)*16 of the line, MFMA A-row j holds block 2p + j%2 of weight row j/2, the step is multiplied with the
// activation fragments of block 2p (valid on even A-rows) and 2p + 1 (valid on odd A-rows) and the halves are added in-lane:
// out row 2g + {0,1} = e[0] + o[1], e[2] + o[3] (same picture as w8a8_block_dot, one K block further apart).  An odd number
// of K blocks ends in a half step: the odd lanes re-read the even block and their product is dropped.  No atomics anywhere.
#include "common.h"
#include "gemm_common.h"
#include "mxfp4_common.h"  // mx_dot (the scaled MFMA with its scale-register guard), cat8

namespace chitu {

// One step (K blocks 2p, 2p + 1) of NT 16-row tiles sharing one activation row per lane.
template <int NT>
struct MxStage {
    i32x4 w[NT][2];       // [tile][half]: 16 B = 32 e2m1 of row n0 + 8*half + j/2, K block 2p + j%2, k = 32g..
    uint32_t sc[NT][2];   // the dword holding that block's E8M0 byte (byte g)
    i32x4 x[4];           // activations: block 2p (x[0], x[1]) and 2p + 1 (x[2], x[3]): k = 16g.. and 64 + 16g.. of the block
    float xs[2];
};

// acc[t] += sum over steps [s0, s1) of the NT tiles whose lane rows start at Wb + wo[t][h] (bytes) / Sb + so[t][h].
// xrow = the lane's activation row + 16 g; xsrow = its group scales.  KB = K / 128.
template <int NT, int D>
__device__ __forceinline__ void mx_stream(const uint8_t* __restrict__ Wb, const uint8_t* __restrict__ Sb, const int (&wo)[NT][2],
                                          const int (&so)[NT][2], const fp8_t* __restrict__ xrow, const float* __restrict__ xsrow,
                                          int KB, int s0, int s1, int j, int g, f32x4 (&acc)[NT]) {
    auto load = [&](MxStage<NT>& st, int p) {
        const bool two = 2 * p + 1 < KB;    // wave-uniform; false on the half step that ends an odd KB
        const int c = two ? (j & 1) : 0;
        const int woff = p * 128 + c * 64 + g * 16, soff = p * 8 + c * 4;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                st.w[t][h] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(Wb + wo[t][h] + woff));
                st.sc[t][h] = *reinterpret_cast<const uint32_t*>(Sb + so[t][h] + soff);
            }
        const int kbe = 2 * p, kbo = two ? 2 * p + 1 : 2 * p;
        st.x[0] = *reinterpret_cast<const i32x4*>(xrow + (kbe << 7));
        st.x[1] = *reinterpret_cast<const i32x4*>(xrow + (kbe << 7) + 64);
        st.x[2] = *reinterpret_cast<const i32x4*>(xrow + (kbo << 7));
        st.x[3] = *reinterpret_cast<const i32x4*>(xrow + (kbo << 7) + 64);
        st.xs[0] = xsrow[kbe];
        st.xs[1] = xsrow[kbo];
    };
    auto compute = [&](const MxStage<NT>& st, int p) {
        const bool two = 2 * p + 1 < KB;
        const i32x8 xe = cat8(st.x[0], st.x[1]), xo = cat8(st.x[2], st.x[3]);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t sc = (st.sc[t][h] >> (8 * g)) & 0xffu;
                const f32x4 e = mx_dot(st.w[t][h], xe, sc);
                acc[t][2 * h] = __builtin_fmaf(e[0], st.xs[0], acc[t][2 * h]);
                acc[t][2 * h + 1] = __builtin_fmaf(e[2], st.xs[0], acc[t][2 * h + 1]);
                if (two) {
                    const f32x4 o = mx_dot(st.w[t][h], xo, sc);
                    acc[t][2 * h] = __builtin_fmaf(o[1], st.xs[1], acc[t][2 * h]);
                    acc[t][2 * h + 1] = __builtin_fmaf(o[3], st.xs[1], acc[t][2 * h + 1]);
                }
            }
    };
    MxStage<NT> ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (s0 + d < s1) load(ring[d], s0 + d);
    for (int p = s0; p < s1; p += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (p + d < s1) {
                compute(ring[d], p + d);
                if (p + d + D < s1) load(ring[d], p + d + D);
            }
        }
    }
}

// lane's byte offsets of its two rows (half 0: n0 + j/2, half 1: n0 + 8 + j/2; clamped to the matrix) inside one expert
__device__ __forceinline__ void mx_lane_rows(int n0, int n_rows, int K, int j, int (&wo)[2], int (&so)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = min(n0 + 8 * h + (j >> 1), n_rows - 1);
        wo[h] = r * (K >> 1);
        so[h] = r * (K >> 5);
    }
}

// K-split reduce over the workgroup's waves (LDS, fixed wave order); true on the wave that holds the sum
template <int WK, int NT>
__device__ __forceinline__ bool mx_reduce(f32x4 (&acc)[NT], float* red, int wave, int lane) {
    if (WK == 1) return true;
#pragma unroll
    for (int t = 0; t < NT; ++t) *reinterpret_cast<f32x4*>(&red[((wave * NT + t) * 64 + lane) * 4]) = acc[t];
    __syncthreads();
    if (wave != 0) return false;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < WK; ++w) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(&red[((w * NT + t) * 64 + lane) * 4]);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] += v[r];
        }
    }
    return true;
}

// ---------------------------------------------------------------- plain grouped GEMM (GEMM1 or GEMM2 of the three-launch form)
// out[slot, :] = bf16( (a[slot / a_div] . W[e]^T) * (mul_weight ? topk_w[slot] : 1) ).  grid (ceil(N/16), max_mblocks); block
// 64*WK (WK waves split the steps).  Padding slots read the tile's first row; expert -1 writes zeros.
template <int WK, int D>
__global__ __launch_bounds__(64 * WK) void moe_mx_gemm_kernel(
    const fp8_t* __restrict__ Xq, const float* __restrict__ Xs, int a_div, const uint8_t* __restrict__ W,
    const uint8_t* __restrict__ Ws, const int32_t* __restrict__ sorted_ids, const int32_t* __restrict__ expert_ids,
    const int32_t* __restrict__ num_post_pad, const void* __restrict__ topk_w, int w_dt, int mul_weight,
    bf16_t* __restrict__ out, int numel, int N, int K) {
    __shared__ float red[WK > 1 ? WK * 256 : 1];
    const int mb = blockIdx.y;
    if (mb * 16 >= *num_post_pad) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int KB = K >> 7, steps = (KB + 1) >> 1;
    const int slot = sorted_ids[mb * 16 + j];
    const bool valid = slot < numel;
    const int e = expert_ids[mb];
    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    if (e >= 0) {
        const int slot0 = __builtin_amdgcn_readfirstlane(slot);
        const int row = (valid ? slot : min(slot0, numel - 1)) / a_div;
        int wo[1][2], so[1][2];
        mx_lane_rows(n0, N, K, j, wo[0], so[0]);
        mx_stream<1, D>(W + (size_t)e * N * (K >> 1), Ws + (size_t)e * N * (K >> 5), wo, so, Xq + (size_t)row * K + g * 16,
                        Xs + (size_t)row * KB, KB, steps * wave / WK, steps * (wave + 1) / WK, j, g, acc);
    }
    if (!mx_reduce<WK, 1>(acc, red, wave, lane)) return;
    if (!valid) return;
    const float rw = mul_weight ? moe_routed_weight(topk_w, w_dt, slot) : 1.0f;
    moe_store_tile(out + (size_t)slot * N, n0, g, N, acc[0], rw);
}

// ---------------------------------------------------------------- GEMM1 + SiLU-and-mul
// A wave owns the gate tile [n0, n0+16) and the up tile [I+n0, I+n0+16) of W1 [E, 2I, K/2]: both share the activation
// fragments; h = bf16(bf16(silu(bf16(g))) * bf16(u)) is written as bf16 [numel, I] (moe_gemm1_silu_kernel's epilogue).
// grid (I/16, max_mblocks); block 64*WK.
template <int WK, int D>
__global__ __launch_bounds__(64 * WK) void moe_mx_gemm1_silu_kernel(
    const fp8_t* __restrict__ Xq, const float* __restrict__ Xs, const uint8_t* __restrict__ W,
    const uint8_t* __restrict__ Ws, const int32_t* __restrict__ sorted_ids, const int32_t* __restrict__ expert_ids,
    const int32_t* __restrict__ num_post_pad, bf16_t* __restrict__ out, int numel, int topk, int I, int K) {
    __shared__ float red[WK > 1 ? WK * 512 : 1];
    const int mb = blockIdx.y;
    if (mb * 16 >= *num_post_pad) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int N = 2 * I;
    const int KB = K >> 7, steps = (KB + 1) >> 1;
    const int slot = sorted_ids[mb * 16 + j];
    const bool valid = slot < numel;
    const int e = expert_ids[mb];
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (e >= 0) {
        const int slot0 = __builtin_amdgcn_readfirstlane(slot);
        const int token = (valid ? slot : min(slot0, numel - 1)) / topk;
        int wo[2][2], so[2][2];
        mx_lane_rows(n0, N, K, j, wo[0], so[0]);
        mx_lane_rows(I + n0, N, K, j, wo[1], so[1]);
        mx_stream<2, D>(W + (size_t)e * N * (K >> 1), Ws + (size_t)e * N * (K >> 5), wo, so, Xq + (size_t)token * K + g * 16,
                        Xs + (size_t)token * KB, KB, steps * wave / WK, steps * (wave + 1) / WK, j, g, acc);
    }
    if (!mx_reduce<WK, 2>(acc, red, wave, lane)) return;
    if (!valid) return;
    f32x4 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float gv = round_bf16(acc[0][r]), uv = round_bf16(acc[1][r]);  // GEMM1's bf16 output
        const float sl = round_bf16(gv / (1.0f + expf(-gv)));
        h[r] = round_bf16(sl * uv);
    }
    moe_store_tile(out + (size_t)slot * I, n0, g, I, h, 1.0f);
}

// ---------------------------------------------------------------- GEMM2 with the fp8 re-quantisation of h in its prologue
// moe_gemm2_q_kernel with MXFP4 weights: the 16 x I tile of h (bf16, moe_mx_gemm1_silu_kernel's output) is quantised once
// per workgroup with per_token_group_quant_fp8's rule and parked in LDS in MFMA-fragment order (chunk g of half-blocks 2kb
// and 2kb + 1 = the fp8 operand's k = 16g.. and 64 + 16g..).  KB = I/128 <= 4, so a tile's weights are one or two
// steps, all requested before the first is consumed; ROUNDS rounds of NT tiles per wave, one round requested ahead.
// grid (ceil(n_tiles / (4*NT*ROUNDS)), max_mblocks); block 256.
template <int KB, int NT, int ROUNDS>
__global__ __launch_bounds__(256) void moe_mx_gemm2_q_kernel(
    const bf16_t* __restrict__ Hb, const uint8_t* __restrict__ W, const uint8_t* __restrict__ Ws,
    const int32_t* __restrict__ sorted_ids, const int32_t* __restrict__ expert_ids,
    const int32_t* __restrict__ num_post_pad, const void* __restrict__ topk_w, int w_dt,
    bf16_t* __restrict__ out, int numel, int N, int mul_weight, float eps) {
    constexpr int I = KB * 128;
    constexpr int S = (KB + 1) / 2;        // steps (K-block pairs)
    constexpr int HPW = (2 * KB + 3) / 4;  // half-blocks per wave
    __shared__ float amax_lds[2 * KB][16];
    __shared__ i32x4 xq_lds[2 * KB][64];
    const int mb = blockIdx.y;
    if (mb * 16 >= *num_post_pad) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int slot = sorted_ids[mb * 16 + j];
    const bool valid = slot < numel;
    const int e = expert_ids[mb];
    auto tile_of = [&](int r) { return ((blockIdx.x * ROUNDS + r) * 4 + wave) * NT; };
    if (e < 0) {  // expert not on this rank (expert_map): the slot's contribution is zero
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int n0 = (tile_of(r) + t) * 16;
                if (n0 < N && valid) moe_store_tile(out + (size_t)slot * N, n0, g, N, f32x4{0.f, 0.f, 0.f, 0.f}, 1.0f);
            }
        return;
    }
    const int row = valid ? slot : 0;
    const bf16_t* hrow = Hb + (size_t)row * I;
    i32x4 hraw[HPW][2];
#pragma unroll
    for (int q = 0; q < HPW; ++q) {
        const int hb = min(wave + 4 * q, 2 * KB - 1);
        hraw[q][0] = *reinterpret_cast<const i32x4*>(hrow + hb * 64 + g * 16);
        hraw[q][1] = *reinterpret_cast<const i32x4*>(hrow + hb * 64 + g * 16 + 8);
    }
    const int last_tile = (N - 1) >> 4;
    const uint8_t* We = W + (size_t)e * N * (I / 2);
    const uint8_t* Se = Ws + (size_t)e * N * (I / 32);
    struct Frag {
        i32x4 w[S][2];
        uint32_t sc[S][2];
    };
    Frag wf[ROUNDS > 1 ? 2 : 1][NT];
    auto load_round = [&](Frag (&dst)[NT], int r) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n0 = min(tile_of(r) + t, last_tile) * 16;  // tail tiles re-read the last one, never stored
            int wo[2], so[2];
            mx_lane_rows(n0, N, I, j, wo, so);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int c = (2 * s + 1 < KB) ? (j & 1) : 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    dst[t].w[s][h] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(We + wo[h] + s * 128 + c * 64 + g * 16));
                    dst[t].sc[s][h] = *reinterpret_cast<const uint32_t*>(Se + so[h] + s * 8 + c * 4);
                }
            }
        }
    };
    load_round(wf[0], 0);
    const float rw = (mul_weight && valid) ? moe_routed_weight(topk_w, w_dt, slot) : 1.0f;
    float hv[HPW][16];
#pragma unroll
    for (int q = 0; q < HPW; ++q) {
        const int hb = wave + 4 * q;
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t u = (uint32_t)hraw[q][i >> 3][(i >> 1) & 3];
            hv[q][i] = (i & 1) ? __uint_as_float(u & 0xffff0000u) : __uint_as_float(u << 16);
            amax = __builtin_fmaxf(amax, __builtin_fabsf(hv[q][i]));
        }
        amax = __builtin_fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = __builtin_fmaxf(amax, __shfl_xor(amax, 32, 64));
        if (g == 0 && hb < 2 * KB) amax_lds[hb][j] = amax;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < HPW; ++q) {
        const int hb = wave + 4 * q;
        if (hb < 2 * KB) {
            const float sc = __builtin_fmaxf(__builtin_fmaxf(amax_lds[hb & ~1][j], amax_lds[hb | 1][j]), eps) / 448.0f;
            float lo[8], hi[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                lo[i] = hv[q][i];
                hi[i] = hv[q][8 + i];
            }
            const i32x2 a = quant8_fp8<true>(lo, sc), b = quant8_fp8<true>(hi, sc);
            xq_lds[hb][lane] = i32x4{a[0], a[1], b[0], b[1]};
        }
    }
    __syncthreads();
    i32x8 x[KB];
    float xs[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        x[kb] = cat8(xq_lds[2 * kb][lane], xq_lds[2 * kb + 1][lane]);
        xs[kb] = __builtin_fmaxf(__builtin_fmaxf(amax_lds[2 * kb][j], amax_lds[2 * kb + 1][j]), eps) / 448.0f;
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (r + 1 < ROUNDS) load_round(wf[(r + 1) & 1], r + 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n0 = (tile_of(r) + t) * 16;
            const Frag& f = wf[r & 1][t];
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t sc = (f.sc[s][h] >> (8 * g)) & 0xffu;
                    const f32x4 ev = mx_dot(f.w[s][h], x[2 * s], sc);
                    acc[2 * h] = __builtin_fmaf(ev[0], xs[2 * s], acc[2 * h]);
                    acc[2 * h + 1] = __builtin_fmaf(ev[2], xs[2 * s], acc[2 * h + 1]);
                    constexpr int kLast = KB - 1;
                    const int ko = 2 * s + 1 < KB ? 2 * s + 1 : kLast;  // (an index inside x[] on the half step too)
                    if (2 * s + 1 < KB) {
                        const f32x4 ov = mx_dot(f.w[s][h], x[ko], sc);
                        acc[2 * h] = __builtin_fmaf(ov[1], xs[ko], acc[2 * h]);
                        acc[2 * h + 1] = __builtin_fmaf(ov[3], xs[ko], acc[2 * h + 1]);
                    }
                }
            if (valid && n0 < N) moe_store_tile(out + (size_t)slot * N, n0, g, N, acc, rw);
        }
    }
}

// ---------------------------------------------------------------- quantise / dequantise (OCP MX v1.0)
// e2m1 magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}: round-to-nearest-even on that grid, saturating at 6.  Ties go to the code with
// an even mantissa bit: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4.
__device__ __forceinline__ uint32_t e2m1_code(float q) {
    const float a = __builtin_fabsf(q);
    const uint32_t m = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
    return m | ((__float_as_uint(q) >> 28) & 8u);
}

__device__ __forceinline__ float e2m1_value(uint32_t code) {
    const uint32_t ex = (code >> 1) & 3u, man = code & 1u;
    const uint32_t bits = ex ? (((ex + 126u) << 23) | (man << 22)) : (man ? 0x3f000000u : 0u);
    return __uint_as_float(bits | ((code & 8u) << 28));
}

// One thread per 32-block.  src_kind 0/1/2: bf16 / f16 / f32 [rows, K]; 3: e4m3 [rows, K] times the fp32 scale of its
// [128, 128] block (scale tensors of rows_per_mat-row matrices stacked: [rows / rows_per_mat, ceil(rows_per_mat/128), K/128]).
// Shared exponent X = floor(log2(amax)) - 2 (the fp32 exponent field of amax, so a denormal amax counts as 2^-127), byte =
// clamp(X + 127, 0, 254); an all-zero block gets byte 0.  Elements = RNE(v * 2^-X) on the e2m1 grid, saturated.
__global__ __launch_bounds__(256) void mx_quant_kernel(const void* __restrict__ src, int src_kind,
                                                       const float* __restrict__ block_scale, int64_t rows, int K,
                                                       int64_t rows_per_mat, uint8_t* __restrict__ packed,
                                                       uint8_t* __restrict__ scales) {
    const int bpr = K >> 5;
    const int64_t n_blocks = rows * bpr;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = b / bpr;
        const int kb32 = (int)(b % bpr);
        const int64_t base = row * K + kb32 * 32;
        float v[32];
        if (src_kind == 3) {
            const int64_t mat = row / rows_per_mat, r = row % rows_per_mat;
            const float s = block_scale[(mat * ((rows_per_mat + 127) >> 7) + (r >> 7)) * (K >> 7) + (kb32 >> 2)];
            const uint32_t* p = reinterpret_cast<const uint32_t*>((const fp8_t*)src + base);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t u = p[i];
                v[4 * i] = fp8_to_f32<0>(u) * s;
                v[4 * i + 1] = fp8_to_f32<1>(u) * s;
                v[4 * i + 2] = fp8_to_f32<2>(u) * s;
                v[4 * i + 3] = fp8_to_f32<3>(u) * s;
            }
        } else if (src_kind == 2) {
#pragma unroll
            for (int i = 0; i < 32; ++i) v[i] = ((const float*)src)[base + i];
        } else {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const uint16_t u = ((const uint16_t*)src)[base + i];
                v[i] = src_kind == 0 ? bf16_to_f32(u) : f16_to_f32(u);
            }
        }
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) amax = __builtin_fmaxf(amax, __builtin_fabsf(v[i]));
        int byte = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 2;
        byte = byte < 0 ? 0 : (byte > 254 ? 254 : byte);
        const float inv = __uint_as_float((uint32_t)(254 - byte) << 23);  // 2^(127 - byte): byte <= 253 here, a normal number
        i32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t wv = 0;
#pragma unroll
            for (int n = 0; n < 8; ++n) wv |= e2m1_code(v[8 * i + n] * inv) << (4 * n);
            o[i] = (int)wv;
        }
        *reinterpret_cast<i32x4*>(packed + (base >> 1)) = o;
        scales[b] = (uint8_t)byte;
    }
}

// packed [rows, K/2] + scales [rows, K/32] -> bf16 [rows, K]: e2m1 value x 2^(byte - 127), exact (two significant bits);
// byte 0xFF -> NaN.
__global__ __launch_bounds__(256) void mx_dequant_kernel(const uint8_t* __restrict__ packed, const uint8_t* __restrict__ scales,
                                                         int64_t n_blocks, bf16_t* __restrict__ out) {
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (int64_t)gridDim.x * blockDim.x) {
        const i32x4 raw = *reinterpret_cast<const i32x4*>(packed + b * 16);
        const int byte = scales[b];
        bf16_t* dst = out + b * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t o[4];
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const float val = byte == 0xff ? __uint_as_float(0x7fc00000u)
                                               : ldexpf(e2m1_value(((uint32_t)raw[i] >> (4 * n)) & 0xfu), byte - 127);
                const uint32_t hbits = f32_to_bf16(val);
                if (n & 1) o[n >> 1] |= hbits << 16; else o[n >> 1] = hbits;
            }
            *reinterpret_cast<i32x4*>(dst + 8 * i) = i32x4{(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
        }
    }
}

}  // namespace chitu

extern "C" int chitu_hip_moe_gemm_mxfp4(const void* a_fp8, const float* a_scale, int32_t a_div, const void* w_fp4,
                                        const void* w_scale_e8m0, const int32_t* sorted_token_ids, const int32_t* expert_ids,
                                        const int32_t* num_tokens_post_pad, const void* topk_weights, int32_t weights_dtype,
                                        int32_t mul_routed_weight, void* out_bf16, int64_t numel, int64_t N, int64_t K,
                                        int64_t max_mblocks, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(a_fp8 && a_scale && w_fp4 && w_scale_e8m0 && sorted_token_ids && expert_ids);
    CHITU_REQUIRE(num_tokens_post_pad && out_bf16 && (topk_weights || !mul_routed_weight));
    CHITU_REQUIRE(numel >= 0 && a_div >= 1 && N >= 1 && K >= 1 && max_mblocks >= 0);
    CHITU_REQUIRE(weights_dtype >= 0 && weights_dtype <= 2);
    if (K % 128 != 0 || N * (K / 2) > 0x7fffffffLL) return CHITU_ERR_UNSUPPORTED;
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    const int n_tiles = (int)((N + 15) / 16);
    const dim3 grid((unsigned)n_tiles, (unsigned)max_mblocks);
    const int64_t wgs = (int64_t)n_tiles * (numel < max_mblocks ? numel : max_mblocks);
    const int steps = (int)((K / 128 + 1) / 2);
    int WK = wgs <= 512 ? 8 : wgs <= 1024 ? 4 : wgs <= 2048 ? 2 : 1;
    debug_override(kOptMoeGemm1WK, WK);
    while (WK > 1 && WK > steps) WK >>= 1;
    hipStream_t st = (hipStream_t)stream;
#define LAUNCHP(WKV)                                                                                                   \
    hipLaunchKernelGGL((moe_mx_gemm_kernel<WKV, 3>), grid, dim3(64 * WKV), 0, st, (const fp8_t*)a_fp8, a_scale, (int)a_div, \
                       (const uint8_t*)w_fp4, (const uint8_t*)w_scale_e8m0, sorted_token_ids, expert_ids,              \
                       num_tokens_post_pad, topk_weights, (int)weights_dtype, (int)mul_routed_weight, (bf16_t*)out_bf16, \
                       (int)numel, (int)N, (int)K)
    switch (WK) {
        case 8: LAUNCHP(8); break;
        case 4: LAUNCHP(4); break;
        case 2: LAUNCHP(2); break;
        default: LAUNCHP(1); break;
    }
#undef LAUNCHP
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_moe_gemm1_silu_mxfp4(const void* a_fp8, const float* a_scale, const void* w1_fp4,
                                              const void* w1_scale_e8m0, const int32_t* sorted_token_ids,
                                              const int32_t* expert_ids, const int32_t* num_tokens_post_pad, void* h_bf16,
                                              int64_t numel, int32_t topk, int64_t inter_size, int64_t K,
                                              int64_t max_mblocks, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(a_fp8 && a_scale && w1_fp4 && w1_scale_e8m0 && sorted_token_ids && expert_ids);
    CHITU_REQUIRE(num_tokens_post_pad && h_bf16);
    CHITU_REQUIRE(numel >= 0 && topk >= 1 && inter_size >= 1 && K >= 1 && max_mblocks >= 0);
    if (K % 128 != 0 || inter_size % 128 != 0 || 2 * inter_size * (K / 2) > 0x7fffffffLL) return CHITU_ERR_UNSUPPORTED;
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    const int n_tiles = (int)(inter_size / 16);
    const int64_t wgs = 2 * (int64_t)n_tiles * (numel < max_mblocks ? numel : max_mblocks);
    const int steps = (int)((K / 128 + 1) / 2);
    // Sweep on MI355X (tools/moe_mxfp4_ab.py --opt, R1 TP=8 shapes, us per launch, WK 1 / 2 / 4 / 8): bs 16 (wgs 4128) 64.9 / 61.8 /
    // 55.0 / 56.1; bs 8 . / 37.4 / 33.0 / 33.4; bs 4 . / 23.2 / 22.4 / 22.1; bs 2 . / 19.8 / 16.4 / 15.4; bs 1 30.1 / 17.7 / 12.6 / 11.1.
    // A workgroup streams half the bytes of the fp8 kernel's, so the K split pays up to twice the grid; beyond bs 16 the
    // thresholds are the fp8 kernel's doubled, not measured.
    int WK = wgs <= 640 ? 8 : wgs <= 6400 ? 4 : wgs <= 12800 ? 2 : 1;
    debug_override(kOptMoeGemm1WK, WK);
    while (WK > 1 && WK > steps) WK >>= 1;
    int D = WK >= 4 ? 2 : 3;
    debug_override(kOptMoeGemm1D, D);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_tiles, (unsigned)max_mblocks);
#define LAUNCH1S(WKV, DV)                                                                                              \
    hipLaunchKernelGGL((moe_mx_gemm1_silu_kernel<WKV, DV>), grid, dim3(64 * WKV), 0, st, (const fp8_t*)a_fp8, a_scale, \
                       (const uint8_t*)w1_fp4, (const uint8_t*)w1_scale_e8m0, sorted_token_ids, expert_ids,            \
                       num_tokens_post_pad, (bf16_t*)h_bf16, (int)numel, (int)topk, (int)inter_size, (int)K)
    if (WK == 8) { if (D == 2) LAUNCH1S(8, 2); else LAUNCH1S(8, 3); }
    else if (WK == 4) { if (D == 2) LAUNCH1S(4, 2); else LAUNCH1S(4, 3); }
    else if (WK == 2) { if (D == 2) LAUNCH1S(2, 2); else LAUNCH1S(2, 3); }
    else { if (D == 2) LAUNCH1S(1, 2); else LAUNCH1S(1, 3); }
#undef LAUNCH1S
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_moe_gemm2_quant_mxfp4(const void* h_bf16, const void* w2_fp4, const void* w2_scale_e8m0,
                                               const int32_t* sorted_token_ids, const int32_t* expert_ids,
                                               const int32_t* num_tokens_post_pad, const void* topk_weights,
                                               int32_t weights_dtype, int32_t mul_routed_weight, void* out_bf16,
                                               int64_t numel, int64_t N, int64_t inter_size, int64_t max_mblocks, float eps,
                                               void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(h_bf16 && w2_fp4 && w2_scale_e8m0 && sorted_token_ids && expert_ids);
    CHITU_REQUIRE(num_tokens_post_pad && out_bf16 && (topk_weights || !mul_routed_weight));
    CHITU_REQUIRE(numel >= 0 && N >= 1 && inter_size >= 1 && max_mblocks >= 0);
    CHITU_REQUIRE(weights_dtype >= 0 && weights_dtype <= 2);
    if (inter_size % 128 != 0 || inter_size > 512) return CHITU_ERR_UNSUPPORTED;  // wider experts: the three-launch form
    if (N * (inter_size / 2) > 0x7fffffffLL) return CHITU_ERR_UNSUPPORTED;
    if (numel == 0 || max_mblocks == 0) return CHITU_OK;
    hipStream_t st = (hipStream_t)stream;
    const int n_tiles = (int)((N + 15) / 16);
    const int KB = (int)(inter_size / 128);
    const int64_t mbs = numel < max_mblocks ? numel : max_mblocks;
#define LAUNCH2Q(KBV, NTV, RV)                                                                                         \
    hipLaunchKernelGGL((moe_mx_gemm2_q_kernel<KBV, NTV, RV>),                                                          \
                       dim3((unsigned)((n_tiles + 4 * NTV * RV - 1) / (4 * NTV * RV)), (unsigned)max_mblocks), dim3(256), 0, st, \
                       (const bf16_t*)h_bf16, (const uint8_t*)w2_fp4, (const uint8_t*)w2_scale_e8m0, sorted_token_ids, \
                       expert_ids, num_tokens_post_pad, topk_weights, (int)weights_dtype, (bf16_t*)out_bf16, (int)numel, \
                       (int)N, (int)mul_routed_weight, eps)
    // sweep on MI355X (tools/moe_mxfp4_ab.py --opt, us; NT,ROUNDS): bs 16: 2,4 24.4 | 2,8 26.2 | 4,4 26.8 | 4,1 27.1 | 4,2 27.5 | 2,1 28.2;
    // bs 8: 2,4 14.5 | 2,8 15.8 | 4,1 16.6; bs 4: 2,4 9.7 | 4,2 10.3 | 4,1 10.8 | 2,1 11.3; bs 2: 2,1 7.9 | 2,4 8.2 | 4,1 8.2;
    // bs 1: 2,1 6.5 | 4,1 6.7 | 2,4 7.7
    const bool many = (int64_t)n_tiles * mbs > 10000;
    int cfg = many ? 24 : 21;  // NT*10 + ROUNDS
    debug_override(kOptMoeGemm2Cfg, cfg);
    switch (KB) {
        case 1: LAUNCH2Q(1, 4, 1); break;
        case 2:
            if (cfg == 44) LAUNCH2Q(2, 4, 4);
            else if (cfg == 42) LAUNCH2Q(2, 4, 2);
            else if (cfg == 24) LAUNCH2Q(2, 2, 4);
            else if (cfg == 28) LAUNCH2Q(2, 2, 8);
            else if (cfg == 21) LAUNCH2Q(2, 2, 1);
            else LAUNCH2Q(2, 4, 1);
            break;
        case 3: LAUNCH2Q(3, 2, 1); break;
        default: LAUNCH2Q(4, 2, 1); break;
    }
#undef LAUNCH2Q
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_quant_mxfp4(const void* src, int32_t src_kind, const float* block_scale, int64_t rows, int64_t cols,
                                     int64_t rows_per_matrix, void* packed_fp4, void* scale_e8m0, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(src && packed_fp4 && scale_e8m0 && rows >= 0 && cols >= 1);
    CHITU_REQUIRE(src_kind >= 0 && src_kind <= 3);
    if (src_kind == 3) CHITU_REQUIRE(block_scale && rows_per_matrix >= 1 && rows % rows_per_matrix == 0);
    if (cols % 32 != 0 || (src_kind == 3 && cols % 128 != 0) || cols > 0x7fffffffLL) return CHITU_ERR_UNSUPPORTED;
    if (rows == 0) return CHITU_OK;
    const int64_t n_blocks = rows * (cols / 32);
    int64_t blocks = (n_blocks + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(mx_quant_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, (int)src_kind,
                       block_scale, rows, (int)cols, src_kind == 3 ? rows_per_matrix : rows, (uint8_t*)packed_fp4,
                       (uint8_t*)scale_e8m0);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_dequant_mxfp4(const void* packed_fp4, const void* scale_e8m0, int64_t rows, int64_t cols,
                                       void* out_bf16, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(packed_fp4 && scale_e8m0 && out_bf16 && rows >= 0 && cols >= 1);
    if (cols % 32 != 0) return CHITU_ERR_UNSUPPORTED;
    if (rows == 0) return CHITU_OK;
    const int64_t n_blocks = rows * (cols / 32);
    int64_t blocks = (n_blocks + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(mx_dequant_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)packed_fp4, (const uint8_t*)scale_e8m0, n_blocks, (bf16_t*)out_bf16);
    CHITU_RETURN_LAUNCH_STATUS();
}
