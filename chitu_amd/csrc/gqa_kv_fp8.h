// The fp8 K / V cache row of the GQA / MHA paged decode (gqa_kv_fp8.hip states the format) as its producers and its reader
// (gqa_decode_tile.h) share it.  The scale rule and the widening convert are the MLA cache's: mla_kv_fp8.h.
#pragma once
#include "common.h"
#include "mla_kv_fp8.h"

namespace chitu {

constexpr int kGqaKvFp8Row = 144;       // bytes per (token, kv head): 9 chunks of 16
constexpr int kGqaKvFp8ScaleOff = 128;  // one fp32 power-of-two scale, then 12 zero bytes

// One head = one 16-lane DPP row: lane l (0..15) holds channels 8 l .. 8 l + 7 of the head as fp32 values of bf16 numbers, and all
// 16 lanes of the row are active.  Writes the 144 bytes at `dst` (16-byte aligned): codes, scale, zero pad.
__device__ __forceinline__ void gqa_kv_fp8_quant_head(int l, const float (&v)[8], uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) amax = __builtin_fmaxf(amax, __builtin_fabsf(v[k]));
    amax = row16_reduce_max(amax);
    const int e = kv_fp8_exponent(amax);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e: e in [-64, 120]
    i32x2 codes;
    codes[0] = (int)(f32x2_to_fp8x2(v[0] * inv, v[1] * inv) | (f32x2_to_fp8x2(v[2] * inv, v[3] * inv) << 16));
    codes[1] = (int)(f32x2_to_fp8x2(v[4] * inv, v[5] * inv) | (f32x2_to_fp8x2(v[6] * inv, v[7] * inv) << 16));
    *reinterpret_cast<i32x2*>(dst + l * 8) = codes;
    if (l == 0) *reinterpret_cast<i32x4*>(dst + kGqaKvFp8ScaleOff) = i32x4{(int)((uint32_t)(e + 127) << 23), 0, 0, 0};
}

// 8 bf16 (one 16-byte chunk) -> fp32
__device__ __forceinline__ void bf16x8_to_f32(const i32x4 raw, float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t u = (uint32_t)raw[k];
        v[2 * k] = __uint_as_float(u << 16);
        v[2 * k + 1] = __uint_as_float(u & 0xffff0000u);
    }
}

}  // namespace chitu
