/* chitu_hip_ext9.h -- the ninth set of additions to the C ABI of libchitu_hip.so.
 *
 * chitu_hip.h is frozen at ABI version 13, the earlier chitu_hip_ext*.h at the versions they state: bindings and checks pin
 * their text.  Entry points added after them live here, are exported from the same library under the prefix chitu_ext9_,
 * and follow chitu_hip.h's conventions: device pointers owned by the caller, launches enqueued on `stream`
 * (hipGraph-capturable), return value 0 = enqueued, <0 = argument error (CHITU_ERR_BAD_ARG -1, CHITU_ERR_UNSUPPORTED -2),
 * >0 = hipError_t.  Additive only: an entry, once declared here, keeps its argument list; CHITU_HIP_EXT9_VERSION counts the
 * additions.
 */
#ifndef CHITU_HIP_EXT9_H
#define CHITU_HIP_EXT9_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT9_VERSION 1  /* 1: the three entries of the W4A16 group-128 int4 linears (Llama-family dense models) */

/* ---- W4A16 g128: bf16 activations x int4 codes with one fp32 scale per weight row and 128 input channels -----------------
 * The format of GPTQ sym=true checkpoints (bits 4, group 128): code u[n][k] in 0..15 with value u - 8 (zero point 8), scale
 * s[n][k / 128] fp32, K a multiple of 128 (anything else: CHITU_ERR_UNSUPPORTED).  The reference serves it only through
 * third-party CUDA kernels (AutoGPTQ, awq_inference_engine); two contracts are pinned here.
 *
 * The STREAMING contract (chitu_ext9_w4a16_gemm, chitu_ext9_w4a16_gemm_silu):
 *   p[m][n][g] = sum_{k in group g} float(x[m][k]) * float(u[n][k] - 8)   fp32; every product is exact, any summation order
 *   out[m][n]  = round( sum_g s[n][g] * p[m][n][g] )                      one fp32 multiply(-add) per group, the groups in
 *                                                                         the kernel's own order, one rounding to out_dtype
 * The TILED contract (chitu_ext9_w4a16_widen followed by chitu_hip_bf16_gemm / chitu_hip_bf16_gemm_silu, what a caller with
 * a prefill-sized M takes): W'[n][k] = bf16( float(u[n][k] - 8) * s[n][k / 128] ), one fp32 multiply and one rounding, then
 * "the bf16 launch on W', bit for bit".  It differs from the streaming contract by the rounding of W' (relative 2^-9 per
 * weight), nothing else.
 *
 * Layout (chitu_amd/quantize/w4a16.py::pack_w4a16 / unpack_w4a16 define it; nothing else may assume it).
 *   w_packed  uint8 [N][K / 2]: channel k of a row in byte (k / 8) * 4 + k % 4, the low nibble for k % 8 < 4 and the high one
 *             otherwise, stored as the two's-complement nibble of u - 8 (= u ^ 8).
 *   scale_f32 fp32 [ceil(N / 2)][ceil(K / 256)][2][2]: {s[2p][2t], s[2p][2t+1], s[2p+1][2t], s[2p+1][2t+1]} for row pair p
 *             and K step t, 0 where the row or the group does not exist.  For w13 = [w1; w3] the ceil(inter / 2) pairs of
 *             w1 are followed by those of w3.
 * x bf16 [M, K] contiguous; every base pointer 16-byte aligned; N arbitrary (rows are clamped on load, stores masked);
 * arguments are checked before the zero-size return and nothing is launched for M == 0.
 *   chitu_ext9_w4a16_gemm        the decode-shaped weight stream: 16 output rows per workgroup, K split over up to 8 waves
 *     and reduced through LDS in wave order, a register ring of in-flight 16-byte non-temporal weight loads (whole 128-byte
 *     lines = 256 channels of 8 rows per wave-load; a K % 256 == 128 tail is one half line), the codes widened to bf16 in
 *     registers for v_mfma_f32_16x16x32_bf16, each step's product scaled by its group's scale as it is added, M walked in
 *     32-row launches.  out_dtype 0 bf16, 1 f16, 2 f32.  Correct for every M.
 *   chitu_ext9_w4a16_gemm_silu   the same over w13 = [w1; w3] (packed [2 inter, K / 2]) with SiluAndMul in the epilogue, the
 *     rounding chain of chitu_hip_bf16_gemm_silu on the scaled accumulators g, u:
 *       h = bf16( bf16(silu(bf16(g))) * bf16(u) ), out bf16 [M, inter].
 *   chitu_ext9_w4a16_widen       out[n][k] = W'[n][k] as above, bf16 [N, K] row-major (one matrix: for w13 one call per
 *     half). */
int chitu_ext9_w4a16_gemm(const void* x_bf16, const void* w_packed, const float* scale_f32, void* out, int32_t out_dtype,
                          int64_t M, int64_t N, int64_t K, void* stream);
int chitu_ext9_w4a16_gemm_silu(const void* x_bf16, const void* w13_packed, const float* scale_f32, void* out_bf16, int64_t M,
                               int64_t inter, int64_t K, void* stream);
int chitu_ext9_w4a16_widen(const void* w_packed, const float* scale_f32, void* out_bf16, int64_t N, int64_t K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT9_H */
