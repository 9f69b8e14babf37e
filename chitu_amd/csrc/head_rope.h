// RoPE on one head held by a 16-lane DPP row, 8 channels per lane (gqa_kv_fp8.h's lane mapping), as the launches that rotate
// q and k and append k and v share it: qk_norm.hip (behind the head norm) and qkv_bias.hip (behind the bias).
// The arithmetic is rope_kernel's (kv.hip): products rounded separately, r0 = n0 c - n1 s, r1 = n1 c + n0 s, one rounding to
// bf16.  layout 0: interleaved pairs, 1: half split.
#pragma once
#include "gqa_kv_fp8.h"

namespace chitu {

// The cos / sin values of one lane's channels.  layout 0: lane l owns the pairs 4 l .. 4 l + 3 (c[0..3]); layout 1: its
// channels 8 l + k rotate by entry 8 (l & 7) + k (c[0..7]).
struct QkRot {
    float c[8], s[8];
};

__device__ __forceinline__ QkRot qk_load_rot(int l, const float* __restrict__ cb, const float* __restrict__ sb, int layout) {
    QkRot t;
    const int at = layout == 0 ? 4 * l : 8 * (l & 7);
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cb + at), s0 = *reinterpret_cast<const f32x4*>(sb + at);
    f32x4 c1 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    if (layout != 0) {
        c1 = *reinterpret_cast<const f32x4*>(cb + at + 4);
        s1 = *reinterpret_cast<const f32x4*>(sb + at + 4);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) t.c[k] = c0[k], t.s[k] = s0[k], t.c[4 + k] = c1[k], t.s[4 + k] = s1[k];
    return t;
}

// All 16 lanes of the row active; n: lane l's channels 8 l .. 8 l + 7 as fp32 values of bf16 numbers.  Returns the lane's 8
// rotated channels as bf16 bits.  With the half-split layout lane l's partner is lane (l ^ 8)'s chunk, fetched by one row
// rotation (row_ror:8) per channel instead of a second load.
__device__ __forceinline__ i32x4 rope_head_row16(int l, const float (&n)[8], const QkRot& t, int layout) {
#pragma clang fp contract(off)  // products rounded separately, like rope_kernel / gqa_qkv_post_kernel
    i32x4 o;
    if (layout == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[k] = (int)f32x2_to_bf16x2(n[2 * k] * t.c[k] - n[2 * k + 1] * t.s[k], n[2 * k + 1] * t.c[k] + n[2 * k] * t.s[k]);
    } else {
        float r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float y = dpp_row<0x128>(n[k]);  // row_ror:8 = lane l ^ 8
            // l < 8: n is x0 (channel i), y is x1 (channel i + 64); else the other way round
            r[k] = l < 8 ? n[k] * t.c[k] - y * t.s[k] : n[k] * t.c[k] + y * t.s[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (int)f32x2_to_bf16x2(r[2 * k], r[2 * k + 1]);
    }
    return o;
}

}  // namespace chitu
