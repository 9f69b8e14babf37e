// FP8 K / V cache rows of the GQA / MHA paged decode (new: no reference counterpart): quantiser, dequantiser, page append, and
// the decode layer's RoPE + append launch with quantising stores.
//
// The K cache and the V cache keep the shape the cache manager allocates, [pages, page, Hkv, 144] bytes instead of
// [pages, page, Hkv, 128] bf16.  One (token, kv head) row = 144 bytes:
//   [  0, 128)  the head's 128 channels as OCP e4m3fn codes, channel order unchanged
//   [128, 132)  one fp32 scale, an exact power of two
//   [132, 144)  zero (written by every producer, read by nobody): rows stay 16-byte aligned
// The scale rule is mla_kv_fp8.hip's with the head as the group: amax = max |x|, e = the smallest integer with
// amax <= 448 * 2^e (clamped to e >= -64; amax == 0 gives -64), scale = 2^e, code = RNE_e4m3(x * 2^-e).  Both products are exact,
// and code * 2^e is a bf16 number: an fp8 cache and its dequantised bf16 image hold the same values.  NaN / Inf inputs are
// unspecified.  144 / 256 = 0.5625 of the bf16 cache's bytes.
//
// One 16-lane DPP row per head, 8 channels per lane: amax is four row rotations on the VALU; a wave takes four heads.
#include "gqa_kv_fp8.h"

namespace chitu {

// grid ceil(rows * Hkv / 16), block 256: 16-lane row r of block i takes head 16 i + r of the [rows, Hkv] heads
__global__ __launch_bounds__(256) void gqa_kv_quant_fp8_kernel(const bf16_t* __restrict__ src, int64_t src_stride,
                                                               uint8_t* __restrict__ dst, int64_t dst_stride, int64_t heads,
                                                               int Hkv) {
    const int l = threadIdx.x & 15;
    const int64_t u = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (u >= heads) return;
    const int64_t t = u / Hkv;
    const int h = (int)(u % Hkv);
    float v[8];
    bf16x8_to_f32(*reinterpret_cast<const i32x4*>(src + t * src_stride + h * 128 + l * 8), v);
    gqa_kv_fp8_quant_head(l, v, dst + t * dst_stride + (int64_t)h * kGqaKvFp8Row);
}

__global__ __launch_bounds__(256) void gqa_kv_dequant_fp8_kernel(const uint8_t* __restrict__ src, int64_t src_stride,
                                                                 bf16_t* __restrict__ dst, int64_t heads, int Hkv) {
    const int l = threadIdx.x & 15;
    const int64_t u = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (u >= heads) return;
    const uint8_t* row = src + (u / Hkv) * src_stride + (u % Hkv) * kGqaKvFp8Row;
    const i32x2 codes = *reinterpret_cast<const i32x2*>(row + l * 8);
    const float s = *reinterpret_cast<const float*>(row + kGqaKvFp8ScaleOff);
    *reinterpret_cast<i32x4*>(dst + u * 128 + l * 8) = kv_fp8_widen8((uint32_t)codes[0], (uint32_t)codes[1], s);
}

// Byte offset of position old_lens[b] of sequence b in a [pages, page, Hkv, 144] cache, or -1 where paged_token_row
// (common.h) refuses: nothing is written.
__device__ __forceinline__ int64_t gqa_kv_fp8_token_off(int b, int64_t num_pages, int page_size, int Hkv,
                                                        const int32_t* __restrict__ table, int pages_per_seq,
                                                        const int32_t* __restrict__ old_lens) {
    int64_t trow;
    if (!paged_token_row(b, old_lens[b], num_pages, page_size, table, pages_per_seq, trow)) return -1;
    return trow * (int64_t)Hkv * kGqaKvFp8Row;
}

// grid (ceil(batch * Hkv / 16), 2), block 256; blockIdx.y: 0 = K, 1 = V
__global__ __launch_bounds__(256) void gqa_kv_append_fp8_kernel(const bf16_t* __restrict__ k, int64_t k_stride,
                                                                const bf16_t* __restrict__ v, int64_t v_stride,
                                                                uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache,
                                                                int64_t num_pages, int page_size, int Hkv,
                                                                const int32_t* __restrict__ table, int pages_per_seq,
                                                                const int32_t* __restrict__ old_lens, int batch) {
    const int l = threadIdx.x & 15;
    const int u = (int)blockIdx.x * 16 + (int)(threadIdx.x >> 4);
    if (u >= batch * Hkv) return;
    const int b = u / Hkv, h = u % Hkv;
    const int64_t off = gqa_kv_fp8_token_off(b, num_pages, page_size, Hkv, table, pages_per_seq, old_lens);
    if (off < 0) return;
    const bf16_t* src = blockIdx.y == 0 ? k + b * k_stride : v + b * v_stride;
    uint8_t* cache = blockIdx.y == 0 ? k_cache : v_cache;
    float x[8];
    bf16x8_to_f32(*reinterpret_cast<const i32x4*>(src + h * 128 + l * 8), x);
    gqa_kv_fp8_quant_head(l, x, cache + off + (int64_t)h * kGqaKvFp8Row);
}

// gqa_qkv_post_kernel (kv.hip) with quantising stores: RoPE on q in place, RoPE on k rounded to bf16 exactly as that kernel
// rounds it and then quantised, v quantised, both straight into the token's page rows.  grid (batch), block 256; qkv row =
// [hq | hkv | hkv] heads of 128 bf16.  The k and v heads are taken by 16-lane rows, 8 channels per lane: with interleaved pairs
// (layout 0) a lane owns 4 whole pairs; with the half-split layout (1) lane l's partner values are lane (l ^ 8)'s chunk, which
// it loads as well.
__global__ __launch_bounds__(256) void gqa_qkv_post_kv_fp8_kernel(
    bf16_t* __restrict__ qkv, int64_t row_stride, int hq, int hkv, const float* __restrict__ cos,
    const float* __restrict__ sin, int layout, uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache,
    int64_t num_pages, int page_size, const int32_t* __restrict__ table, int pages_per_seq,
    const int32_t* __restrict__ old_lens) {
#pragma clang fp contract(off)  // products rounded separately, like rope_kernel / gqa_qkv_post_kernel
    constexpr int d = 128, half = 64;
    const int b = blockIdx.x;
    bf16_t* row = qkv + (int64_t)b * row_stride;
    const float* cb = cos + (int64_t)b * half;
    const float* sb = sin + (int64_t)b * half;
    for (int idx = threadIdx.x; idx < hq * half; idx += 256) {
        const int h = idx / half, i = idx % half;
        const int i0 = layout == 0 ? 2 * i : i, i1 = layout == 0 ? 2 * i + 1 : i + half;
        bf16_t* src = row + h * d;
        const float x0 = bf16_to_f32(src[i0]), x1 = bf16_to_f32(src[i1]);
        const float c = cb[i], s = sb[i];
        src[i0] = f32_to_bf16(x0 * c - x1 * s);
        src[i1] = f32_to_bf16(x1 * c + x0 * s);
    }
    const int64_t off = gqa_kv_fp8_token_off(b, num_pages, page_size, hkv, table, pages_per_seq, old_lens);
    if (off < 0) return;
    const int l = threadIdx.x & 15;
    for (int u = threadIdx.x >> 4; u < 2 * hkv; u += 16) {  // uniform per 16-lane row
        const bf16_t* src = row + (hq + u) * d;
        float x[8];
        bf16x8_to_f32(*reinterpret_cast<const i32x4*>(src + l * 8), x);
        if (u >= hkv) {
            gqa_kv_fp8_quant_head(l, x, v_cache + off + (int64_t)(u - hkv) * kGqaKvFp8Row);
            continue;
        }
        float r[8];
        if (layout == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float c = cb[l * 4 + k], s = sb[l * 4 + k];
                r[2 * k] = round_bf16(x[2 * k] * c - x[2 * k + 1] * s);
                r[2 * k + 1] = round_bf16(x[2 * k + 1] * c + x[2 * k] * s);
            }
        } else {
            float y[8];
            bf16x8_to_f32(*reinterpret_cast<const i32x4*>(src + (l ^ 8) * 8), y);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float c = cb[(l & 7) * 8 + k], s = sb[(l & 7) * 8 + k];
                // l < 8: x is x0 (channel i), y is x1 (channel i + 64); else the other way round
                r[k] = l < 8 ? round_bf16(x[k] * c - y[k] * s) : round_bf16(x[k] * c + y[k] * s);
            }
        }
        gqa_kv_fp8_quant_head(l, r, k_cache + off + (int64_t)u * kGqaKvFp8Row);
    }
}

}  // namespace chitu

extern "C" int chitu_hip_gqa_kv_quant_fp8(const void* src_bf16, int64_t src_stride, void* dst_u8, int64_t dst_stride_bytes,
                                          int64_t rows, int32_t kv_heads, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(src_bf16 && dst_u8 && rows >= 0 && kv_heads >= 1 && rows * kv_heads < (1ll << 34));
    CHITU_REQUIRE(src_stride >= (int64_t)kv_heads * 128 && src_stride % 8 == 0 && ((uintptr_t)src_bf16 & 15) == 0);  // 16-byte loads
    CHITU_REQUIRE(dst_stride_bytes >= (int64_t)kv_heads * kGqaKvFp8Row && dst_stride_bytes % 16 == 0 && ((uintptr_t)dst_u8 & 15) == 0);
    if (rows == 0) return CHITU_OK;
    const int64_t heads = rows * kv_heads;
    hipLaunchKernelGGL(gqa_kv_quant_fp8_kernel, dim3((unsigned)((heads + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src_bf16, src_stride, (uint8_t*)dst_u8, dst_stride_bytes, heads, (int)kv_heads);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_gqa_kv_dequant_fp8(const void* src_u8, int64_t src_stride_bytes, void* dst_bf16, int64_t rows,
                                            int32_t kv_heads, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(src_u8 && dst_bf16 && rows >= 0 && kv_heads >= 1 && rows * kv_heads < (1ll << 34));
    CHITU_REQUIRE(src_stride_bytes >= (int64_t)kv_heads * kGqaKvFp8Row && src_stride_bytes % 16 == 0 && ((uintptr_t)src_u8 & 15) == 0);
    CHITU_REQUIRE(((uintptr_t)dst_bf16 & 15) == 0);
    if (rows == 0) return CHITU_OK;
    const int64_t heads = rows * kv_heads;
    hipLaunchKernelGGL(gqa_kv_dequant_fp8_kernel, dim3((unsigned)((heads + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)src_u8, src_stride_bytes, (bf16_t*)dst_bf16, heads, (int)kv_heads);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_gqa_kv_append_fp8(const void* k_bf16, int64_t k_stride, const void* v_bf16, int64_t v_stride,
                                           void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                           int32_t kv_heads, const int32_t* block_table, int32_t pages_per_seq,
                                           const int32_t* old_seq_lens, int32_t batch, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(k_bf16 && v_bf16 && k_cache_u8 && v_cache_u8 && block_table && old_seq_lens);
    CHITU_REQUIRE(num_pages >= 0 && page_size >= 1 && pages_per_seq >= 1 && batch >= 0 && kv_heads >= 1);
    CHITU_REQUIRE((int64_t)batch * kv_heads < (1ll << 31));
    CHITU_REQUIRE(k_stride >= (int64_t)kv_heads * 128 && k_stride % 8 == 0 && v_stride >= (int64_t)kv_heads * 128 && v_stride % 8 == 0);
    CHITU_REQUIRE((((uintptr_t)k_bf16 | (uintptr_t)v_bf16) & 15) == 0);
    CHITU_REQUIRE((((uintptr_t)k_cache_u8 | (uintptr_t)v_cache_u8) & 15) == 0);  // rows are 9 x 16 bytes: every row is then aligned
    if (batch == 0) return CHITU_OK;
    hipLaunchKernelGGL(gqa_kv_append_fp8_kernel, dim3((unsigned)((batch * kv_heads + 15) / 16), 2), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)k_bf16, k_stride, (const bf16_t*)v_bf16, v_stride, (uint8_t*)k_cache_u8,
                       (uint8_t*)v_cache_u8, num_pages, (int)page_size, (int)kv_heads, block_table, (int)pages_per_seq,
                       old_seq_lens, (int)batch);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_gqa_qkv_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                             int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                             void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                             const int32_t* page_table, int32_t pages_per_seq,
                                             const int32_t* old_seq_lens, int32_t batch, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(qkv_bf16 && cos && sin && k_cache_u8 && v_cache_u8 && page_table && old_seq_lens);
    CHITU_REQUIRE(batch >= 0 && q_heads >= 1 && kv_heads >= 1 && num_pages >= 1 && page_size >= 1);
    CHITU_REQUIRE(pages_per_seq >= 1 && (layout == 0 || layout == 1));
    if (head_dim != 128 || row_stride % 8 != 0 || row_stride < (int64_t)(q_heads + 2 * kv_heads) * head_dim)
        return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE((((uintptr_t)qkv_bf16 | (uintptr_t)k_cache_u8 | (uintptr_t)v_cache_u8) & 15) == 0);
    if (batch == 0) return CHITU_OK;
    hipLaunchKernelGGL(gqa_qkv_post_kv_fp8_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv_bf16,
                       row_stride, (int)q_heads, (int)kv_heads, cos, sin, (int)layout, (uint8_t*)k_cache_u8, (uint8_t*)v_cache_u8,
                       num_pages, (int)page_size, page_table, (int)pages_per_seq, old_seq_lens);
    CHITU_RETURN_LAUNCH_STATUS();
}
