// The total order on floats that the sampler and the logprobs kernel rank logits by (sample.hip, logprobs.hip).
#pragma once

#include "common.h"

namespace chitu {

// total order on floats as unsigned integers (larger float <-> larger key).  Every NaN, whichever its sign bit and payload,
// takes the one top key, above +inf: a NaN logit is the arg-max and the first NaN wins, as in torch.argmax.  (Without the
// NaN test a NaN with the sign bit set -- 0xffc00000, what inf - inf gives on x86 -- would sort below -inf.)
// ordered_key_inv gives a NaN back for the top key.  v != v is one compare; the library is built without fast-math.
__device__ __forceinline__ uint32_t ordered_key(float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return v != v ? 0xffffffffu : k;
}
__device__ __forceinline__ float ordered_key_inv(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

}  // namespace chitu
