// The MXFP4 x e4m3 block dot shared by the W4A8 expert kernels (moe_mxfp4.hip: decode-shaped streaming; moe_mxfp4_tiled.hip:
// prefill-shaped tiles): ONE v_mfma_scale_f32_16x16x128_f8f6f4 per 128-wide K block and fragment pair, A = e2m1 weights with
// their own E8M0 bytes as the hardware scale, B = e4m3 activations with unit scale 0x7f.  Lane map (pinned with exact data by
// tests/test_gpu_moe_mxfp4.py): lane (j, g) of the FP4 operand carries k = 32g .. 32g+31 of row j and that block's one scale
// byte; lane (j, g) of the FP8 operand carries k = 16g .. 16g+15 (first four registers) and 64+16g .. (last four) of column j;
// lane (j, g) of the result holds rows 4g .. 4g+3 of column j.
#pragma once
#include "common.h"
#include "gemm_common.h"

namespace chitu {

// The scale registers must outlive the instruction's ISSUE: the hardware goes on reading them while the MFMA runs (measured:
// the compiler re-used the A-scale register in the very next instruction, and every weight row but the first of the tile came
// out with that new value as its exponent), and hipcc tracks no such hazard for the two scale operands.  Guard: one real VALU
// instruction reads the result (an identity DPP move, which the compiler cannot fold away and in front of which it does insert
// the MFMA -> VALU wait), and an empty asm statement takes that move's output AND both scale registers as operands: the scale
// registers stay allocated until the result has left the matrix pipe.
__device__ __forceinline__ f32x4 mx_dot(const i32x4& w, const i32x8& x, uint32_t scale_byte) {
    const i32x8 a = {w[0], w[1], w[2], w[3], 0, 0, 0, 0};  // fp4: the instruction reads the first four registers only
    const int sa = (int)scale_byte, sb = 0x7f;
    f32x4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, x, f32x4{0.f, 0.f, 0.f, 0.f}, 4 /* A: e2m1 */, 0 /* B: e4m3 */, 0,
                                                               sa, 0, sb);
    int first = __builtin_amdgcn_update_dpp(0, __float_as_int(d[0]), 0xE4 /* quad_perm:[0,1,2,3] */, 0xf, 0xf, false);
    asm volatile("" : "+v"(first) : "v"(sa), "v"(sb));
    d[0] = __int_as_float(first);
    return d;
}

__device__ __forceinline__ i32x8 cat8(const i32x4& a, const i32x4& b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }

}  // namespace chitu
