// FP8 latent KV cache rows of the MLA paged decode (new: no reference counterpart): quantiser, dequantiser, page append.
//
// One cached token = 656 bytes:
//   [  0, 512)  kv_norm(kv_c), 512 x OCP e4m3fn codes
//   [512, 528)  four fp32 scales, one per 128 latent channels, each an exact power of two
//   [528, 656)  rope(k_pe), 64 x bf16, copied unchanged
// Per 128-channel group: amax = max |x|, e = the smallest integer with amax <= 448 * 2^e (clamped to e >= -64; amax == 0 gives
// -64), scale = 2^e, code = RNE_e4m3(x * 2^-e) -- never overflows by construction.  Both products (x * 2^-e here, code * 2^e in the
// dequantiser and in mla_decode_kv_fp8.hip) are exact: a code has 4 significant bits, so code * 2^e is a bf16 number and an fp8
// cache and its dequantised bf16 image hold the same values.  NaN / Inf inputs are unspecified.
//
// One wave per row, 8 latent channels per lane: a group is one 16-lane DPP row, so amax is four row rotations on the VALU.
#include "common.h"
#include "mla_kv_fp8.h"

namespace chitu {

// Row `src` (576 bf16, 16-byte aligned) -> 656 bytes at `dst` (16-byte aligned).  All 64 lanes of one wave.
__device__ __forceinline__ void kv_fp8_quant_row(int lane, const bf16_t* __restrict__ src, uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
    const i32x4 raw = *reinterpret_cast<const i32x4*>(src + lane * 8);
    uint32_t rope = 0;
    if (lane < 32) rope = *reinterpret_cast<const uint32_t*>(src + 512 + lane * 2);
    float v[8], amax = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t u = (uint32_t)raw[k];
        v[2 * k] = __uint_as_float(u << 16);
        v[2 * k + 1] = __uint_as_float(u & 0xffff0000u);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) amax = __builtin_fmaxf(amax, __builtin_fabsf(v[k]));
    amax = row16_reduce_max(amax);
    const int e = kv_fp8_exponent(amax);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e: e in [-64, 120]
    i32x2 codes;
    codes[0] = (int)(f32x2_to_fp8x2(v[0] * inv, v[1] * inv) | (f32x2_to_fp8x2(v[2] * inv, v[3] * inv) << 16));
    codes[1] = (int)(f32x2_to_fp8x2(v[4] * inv, v[5] * inv) | (f32x2_to_fp8x2(v[6] * inv, v[7] * inv) << 16));
    *reinterpret_cast<i32x2*>(dst + lane * 8) = codes;
    if ((lane & 15) == 0) *reinterpret_cast<uint32_t*>(dst + kKvFp8ScaleOff + (lane >> 4) * 4) = (uint32_t)(e + 127) << 23;
    if (lane < 32) *reinterpret_cast<uint32_t*>(dst + kKvFp8RopeOff + lane * 4) = rope;
}

// grid ceil(rows / 4), block 256: wave w of block i takes row 4 i + w
__global__ __launch_bounds__(256) void mla_kv_quant_fp8_kernel(const bf16_t* __restrict__ src, int64_t src_stride,
                                                               uint8_t* __restrict__ dst, int64_t dst_stride, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= rows) return;
    kv_fp8_quant_row(lane, src + t * src_stride, dst + t * dst_stride);
}

__global__ __launch_bounds__(256) void mla_kv_dequant_fp8_kernel(const uint8_t* __restrict__ src, int64_t src_stride,
                                                                 bf16_t* __restrict__ dst, int64_t rows) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= rows) return;
    const uint8_t* row = src + t * src_stride;
    const i32x2 codes = *reinterpret_cast<const i32x2*>(row + lane * 8);
    const float s = *reinterpret_cast<const float*>(row + kKvFp8ScaleOff + (lane >> 4) * 4);
    bf16_t* out = dst + t * 576;
    *reinterpret_cast<i32x4*>(out + lane * 8) = kv_fp8_widen8((uint32_t)codes[0], (uint32_t)codes[1], s);
    if (lane < 32) *reinterpret_cast<uint32_t*>(out + 512 + lane * 2) = *reinterpret_cast<const uint32_t*>(row + kKvFp8RopeOff + lane * 4);
}

// Row b of the source -> position old_lens[b] of sequence b's page.  The indexing and the out-of-range rules are
// paged_token_row's (common.h): where it refuses, nothing is written.
__global__ __launch_bounds__(256) void mla_kv_append_fp8_kernel(const bf16_t* __restrict__ src, int64_t src_stride,
                                                                uint8_t* __restrict__ cache, int64_t num_pages, int page_size,
                                                                const int32_t* __restrict__ table, int pages_per_seq,
                                                                const int32_t* __restrict__ old_lens, int batch) {
    const int lane = threadIdx.x & 63;
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= batch) return;
    int64_t trow;
    if (!paged_token_row(b, old_lens[b], num_pages, page_size, table, pages_per_seq, trow)) return;
    kv_fp8_quant_row(lane, src + (int64_t)b * src_stride, cache + trow * (int64_t)kKvFp8Row);
}

}  // namespace chitu

extern "C" int chitu_hip_mla_kv_quant_fp8(const void* src_bf16, int64_t src_stride, void* dst_u8, int64_t dst_stride_bytes,
                                          int64_t rows, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(src_bf16 && dst_u8 && rows >= 0 && rows < (1ll << 31));
    CHITU_REQUIRE(src_stride >= 576 && src_stride % 8 == 0 && ((uintptr_t)src_bf16 & 15) == 0);  // 16-byte loads
    CHITU_REQUIRE(dst_stride_bytes >= kKvFp8Row && dst_stride_bytes % 16 == 0 && ((uintptr_t)dst_u8 & 15) == 0);
    if (rows == 0) return CHITU_OK;
    hipLaunchKernelGGL(mla_kv_quant_fp8_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src_bf16, src_stride, (uint8_t*)dst_u8, dst_stride_bytes, rows);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_mla_kv_dequant_fp8(const void* src_u8, int64_t src_stride_bytes, void* dst_bf16, int64_t rows,
                                            void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(src_u8 && dst_bf16 && rows >= 0 && rows < (1ll << 31));
    CHITU_REQUIRE(src_stride_bytes >= kKvFp8Row && src_stride_bytes % 16 == 0 && ((uintptr_t)src_u8 & 15) == 0);
    CHITU_REQUIRE(((uintptr_t)dst_bf16 & 15) == 0);
    if (rows == 0) return CHITU_OK;
    hipLaunchKernelGGL(mla_kv_dequant_fp8_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)src_u8, src_stride_bytes, (bf16_t*)dst_bf16, rows);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_mla_kv_append_fp8(const void* src_bf16, int64_t src_stride, void* kv_cache_u8, int64_t num_pages,
                                           int32_t page_size, const int32_t* block_table, int32_t pages_per_seq,
                                           const int32_t* old_seq_lens, int32_t batch, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(src_bf16 && kv_cache_u8 && block_table && old_seq_lens);
    CHITU_REQUIRE(num_pages >= 0 && page_size >= 1 && pages_per_seq >= 1 && batch >= 0);
    CHITU_REQUIRE(src_stride >= 576 && src_stride % 8 == 0 && ((uintptr_t)src_bf16 & 15) == 0);
    CHITU_REQUIRE(((uintptr_t)kv_cache_u8 & 15) == 0);  // rows are 41 x 16 bytes: every row is then 16-byte aligned
    if (batch == 0) return CHITU_OK;
    hipLaunchKernelGGL(mla_kv_append_fp8_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src_bf16, src_stride, (uint8_t*)kv_cache_u8, num_pages, (int)page_size, block_table,
                       (int)pages_per_seq, old_seq_lens, (int)batch);
    CHITU_RETURN_LAUNCH_STATUS();
}
