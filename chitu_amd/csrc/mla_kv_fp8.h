// The fp8 latent KV cache row (mla_kv_fp8.hip states the format) as its producers and its reader share it, and the two pieces of
// arithmetic every fp8 KV cache of this library is built from (the GQA rows of gqa_kv_fp8.h included): the scale's exponent and the
// exact widening convert.
#pragma once
#include "common.h"

namespace chitu {

constexpr int kKvFp8Row = 656;       // bytes per cached token: 41 chunks of 16
constexpr int kKvFp8ScaleOff = 512;  // four fp32 power-of-two scales
constexpr int kKvFp8RopeOff = 528;   // 64 bf16

// 8 codes x their group's scale -> 8 bf16, on gfx950's scaled packed convert (v_cvt_scalef32_pk_bf16_fp8: two codes per
// instruction, the scale's exponent applied in the conversion).  The scale is a power of two and code * 2^e has 4 significant
// bits, so the result is exact and equals bf16(f32(code) * scale) bit for bit (the CPU reference of the tests).
__device__ __forceinline__ i32x4 kv_fp8_widen8(uint32_t w0, uint32_t w1, float s) {
    i32x4 r;
    r[0] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w0, s, false));
    r[1] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w0, s, true));
    r[2] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w1, s, false));
    r[3] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w1, s, true));
    return r;
}

// The scale rule of every fp8 KV cache row (MLA latent groups, GQA heads): e = the smallest integer with amax <= 448 * 2^e.
// e from amax's own bits (no division): amax = 1.m * 2^(E - 127), 448 = 1.75 * 2^8, so e = E - 135, one more when 1.m > 1.75.
// A zero or denormal amax (E == 0) lies below 448 * 2^-64: clamped.
__device__ __forceinline__ int kv_fp8_exponent(float amax) {
    const uint32_t u = __float_as_uint(amax);
    const int E = (int)(u >> 23) & 0xff;
    if (E == 0) return -64;
    return max(E - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0), -64);
}

}  // namespace chitu
