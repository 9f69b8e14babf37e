/* chitu_hip_ext8.h -- the eighth set of additions to the C ABI of libchitu_hip.so.
 *
 * chitu_hip.h is frozen at ABI version 13, chitu_hip_ext.h .. chitu_hip_ext7.h at version 1 each: bindings and checks pin the
 * text of all eight.  Entry points added after them live here, are exported from the same library under the prefix
 * chitu_ext8_, and follow chitu_hip.h's conventions: device pointers owned by the caller, launches enqueued on `stream`
 * (hipGraph-capturable), return value 0 = enqueued, <0 = argument error (CHITU_ERR_BAD_ARG -1, CHITU_ERR_UNSUPPORTED -2),
 * >0 = hipError_t.  Additive only: an entry, once declared here, keeps its argument list; CHITU_HIP_EXT8_VERSION counts the
 * additions.
 */
#ifndef CHITU_HIP_EXT8_H
#define CHITU_HIP_EXT8_H

#include "chitu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHITU_HIP_EXT8_VERSION 1  /* 1: log-probabilities of chosen tokens and the top-N alternatives */

/* ---- log-softmax statistics of logits rows: the chosen token's log-probability and the N most likely tokens ---------------
 * (new: the reference reports no log-probabilities.)  For every row r of logits [rows, vocab] (act_dtype 2 = fp32 or 0 = bf16,
 * anything else CHITU_ERR_UNSUPPORTED; row_stride in elements, >= vocab; any element-aligned base; read only), in fp32:
 *   logZ[r]                = max_j x[r, j] + log sum_j exp(x[r, j] - max)
 *   token_logprobs[r * token_logprobs_stride] = x[r, tokens[r]] - logZ[r]     NaN, and nothing read, for an id outside [0, vocab)
 *   top_ids[r * top_stride + p], top_logprobs[r * top_stride + p], p < top_n: the top_n largest logits in descending order,
 *                            equal values by the lower id first (the sampler's tie rule); id -1 and -inf for p >= vocab.
 * A -inf logit has the log-probability -inf; a row of nothing but -inf gives NaN everywhere.  tokens (int64 [rows]) and
 * token_logprobs are both given or both NULL; top_n in [0, 20] (else CHITU_ERR_BAD_ARG), top_ids / top_logprobs may be NULL
 * when it is 0; strides in elements.
 *
 * One launch over (ceil(vocab / 8192), rows) workgroups: every workgroup reads its 8192-element slice once, leaves (max, sum of
 * exp, its own top_n, the token's logit) in `partials`, and the last workgroup of a row to count itself on tickets[r] merges the
 * row.  The result does not depend on which workgroup that is.  `tickets` holds one zero-initialised 32-bit word per row, which
 * the merging workgroup sets back to zero: nothing has to be cleared between launches or graph replays; launches that share
 * tickets or partials must not overlap.  chitu_ext8_logprobs_workspace_bytes gives the sizes both must at least have
 * (tickets_bytes, partials_bytes: what the caller provides; smaller is CHITU_ERR_BAD_ARG).  Nothing is launched for zero rows;
 * vocab < 1 is CHITU_ERR_BAD_ARG. */
int chitu_ext8_logprobs_workspace_bytes(int64_t rows, int32_t vocab, int32_t top_n, int64_t* tickets_bytes,
                                        int64_t* partials_bytes);
int chitu_ext8_logprobs(const void* logits, int act_dtype, int64_t row_stride, int64_t rows, int32_t vocab,
                        const int64_t* tokens, float* token_logprobs, int64_t token_logprobs_stride, int32_t top_n,
                        int32_t* top_ids, float* top_logprobs, int64_t top_stride, uint32_t* tickets, int64_t tickets_bytes,
                        void* partials, int64_t partials_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHITU_HIP_EXT8_H */
