/* chitu_hip_ext6.h -- the sixth set of additions to the C ABI of libchitu_hip.so.
 *
 * chitu_hip.h is frozen at ABI version 13, chitu_hip_ext.h .. chitu_hip_ext5.h at version 1 each: bindings and checks pin the
 * text of all six.  Entry points added after them live here, are exported from the same library under the prefix
 * chitu_ext6_, and follow chitu_hip.h's conventions: device pointers owned by the caller, launches enqueued on `stream`
 * (hipGraph-capturable), return value 0 = enqueued, <0 = argument error (CHITU_ERR_BAD_ARG -1, CHITU_ERR_UNSUPPORTED -2),
 * >0 = hipError_t.  Additive only: an entry, once declared here, keeps its argument list; CHITU_HIP_EXT6_VERSION counts the
 * additions.
 */
#ifndef CHITU_HIP_EXT6_H
#define CHITU_HIP_EXT6_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT6_VERSION 1  /* 1: the four entries of the W8A16 weight-only int8 linears (Llama-family dense models) */

/* ---- W8A16: bf16 activations x int8 weights with one fp32 scale per output row ------------------------------------------
 * Replaces (reference, read-only) chitu/quantize/w8a16.py::WeightOnlyLinear.forward -> EETQ.w8_a16_gemm, whose arithmetic is
 * closed; the pinned definition is the reference's own Triton use_int8_w8a16 branch (chitu/fused_moe.py:226-227,293-294):
 *   acc[m][n] = sum_k float(x[m][k]) * float(q[n][k])     fp32; every product is exact (bf16 x int8), any summation order
 *   out[m][n] = round( acc[m][n] * s[n] )                 one fp32 multiply, one rounding to out_dtype
 * q is int8 [N, K] row-major ([out, in], like W8A8Linear.weight), s fp32 [N], x bf16 [M, K] contiguous.  Every base pointer
 * 16-byte aligned; K a multiple of 64 (anything else: CHITU_ERR_UNSUPPORTED); N arbitrary (rows are clamped on load, stores
 * masked); arguments are checked before the zero-size return and nothing is launched for M == 0.
 *   chitu_ext6_w8a16_gemm        the decode-shaped weight stream: 16 output rows per workgroup, K split over up to 8 waves
 *     and reduced through LDS in wave order, a register ring of in-flight 16-byte non-temporal weight loads (whole 128-byte
 *     lines of 8 rows per wave-load; a K % 128 == 64 tail is one half line), the int8 bytes widened to bf16 in registers for
 *     v_mfma_f32_16x16x32_bf16, M walked in 32-row launches.  out_dtype 0 bf16, 1 f16, 2 f32.  Correct for every M; a
 *     caller with a prefill-sized M takes the widen + tiled GEMM + scale_round form instead (it reads the weights once).
 *   chitu_ext6_w8a16_gemm_silu   the same over w13 = [w1; w3] (int8 [2 inter, K], s [2 inter]) with SiluAndMul in the
 *     epilogue, the rounding chain of chitu_hip_bf16_gemm_silu on the scaled accumulators:
 *       g = acc_g * s[n], u = acc_u * s[inter + n], h = bf16( bf16(silu(bf16(g))) * bf16(u) ), out bf16 [M, inter].
 *   chitu_ext6_w8a16_widen       out[n][k] = bf16(q[n][k]), exact, no scale: the MFMA operand of the tiled bf16 GEMM
 *     (chitu_hip_bf16_gemm with an fp32 output) for prefill-sized M.  K a multiple of 16.
 *   chitu_ext6_w8a16_scale_round the epilogue of that form: acc fp32 [M, N] (silu = 0) -> out[m][n] = round(acc * s[n]) in
 *     out_dtype; silu = 1: acc fp32 [M, 2 N], s [2 N] -> out bf16 [M, N] by the chain above (out_dtype must be 0). */
int chitu_ext6_w8a16_gemm(const void* x_bf16, const void* w_int8, const float* scale_f32, void* out, int32_t out_dtype,
                          int64_t M, int64_t N, int64_t K, void* stream);
int chitu_ext6_w8a16_gemm_silu(const void* x_bf16, const void* w13_int8, const float* scale_f32, void* out_bf16, int64_t M,
                               int64_t inter, int64_t K, void* stream);
int chitu_ext6_w8a16_widen(const void* w_int8, void* out_bf16, int64_t N, int64_t K, void* stream);
int chitu_ext6_w8a16_scale_round(const float* acc_f32, const float* scale_f32, void* out, int32_t out_dtype, int64_t M,
                                 int64_t N, int32_t silu, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT6_H */
