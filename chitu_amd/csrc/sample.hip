// Token sampling for the decode step: frequency penalty, greedy argmax, temperature softmax with
// top-k / top-p filtering and one draw per row -- the step right after the hot path.
//
// Replaces (reference, read-only):
//   chitu/executor.py:82-112   NormalExecutor.update_response: index_add_ of -frequency_penalty per
//                              generated token, argmax if all rows are greedy, else
//                              softmax(logits / temperature) -> top_k_top_p_min_p_sampling_from_probs_torch
//   chitu/utils.py:62-81       full descending sort of [bs, vocab], cumsum, two masks, multinomial
//
// The reference sorts the whole vocabulary to cut a prefix of the sorted order.  Here the prefix is
// found without sorting: the kept set is {elements with weight > tau} plus the first c ties at tau,
// and (tau, c) comes from a 3-level radix descent (10 bits per level) over the 30-bit float pattern of
// the weight e = exp(x - max) in (0, 1].  Each level is one pass over the row (L2-resident, 517 KB at
// vocab 129280) into a 1024-bin LDS histogram of (count, fixed-point sum); sums are integers
// (weights scaled by 2^40), so the result does not depend on the order atomics land in and two runs
// agree bit for bit.  A prefix position `pos` of the descending order is kept iff pos < top_k and
// exclusive_cumsum(pos) <= top_p * Z -- the two masks of utils.py:72-76 (ties in sorted order broken
// by lower index; torch.sort leaves that order unspecified).  The draw is an inverse CDF over the
// kept weights in INDEX order with a caller-supplied uniform u in [0, 1): same distribution as
// torch.multinomial on the masked probabilities, and reproducible given u.
//
// One workgroup (1024 threads) per row; rows are independent.
//
// chitu_hip_speculative_verify (below, new: no reference counterpart) is the same row with a draft token: the passes are
// shared, and the acceptance test sits between the kept prefix and the draw.
#include <type_traits>

#include "common.h"

namespace chitu {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / 64;
constexpr int kSampleBins = 1024;
constexpr float kSampleFixScale = 1099511627776.0f;  // 2^40: weights in (0, 1] -> integers <= 2^40

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_row_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_row_u64(uint64_t v) {
    return ((uint64_t)dpp_row_u32<CTRL>((uint32_t)(v >> 32)) << 32) | dpp_row_u32<CTRL>((uint32_t)v);
}
// Sum over the 64 lanes, result in every lane (wave-uniform): DPP rotations inside each 16-lane row,
// then the four row results through v_readlane.  Must be called by the whole wave.
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    v += dpp_row_u64<0x128>(v);  // row_ror:8
    v += dpp_row_u64<0x124>(v);  // row_ror:4
    v += dpp_row_u64<0x122>(v);  // row_ror:2
    v += dpp_row_u64<0x121>(v);  // row_ror:1
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    uint64_t s = 0;
#pragma unroll
    for (int l = 0; l < 64; l += 16)
        s += ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, l) << 32) | (uint32_t)__builtin_amdgcn_readlane(lo, l);
    return s;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int off) {
    return ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), off, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
}
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int off) {
    return ((uint64_t)(uint32_t)__shfl_up((int)(v >> 32), off, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, off, 64);
}

// total order on floats as unsigned integers (larger float <-> larger key).  Every NaN, whichever its sign bit and payload,
// takes the one top key, above +inf: a NaN logit is the arg-max and the first NaN wins, as in torch.argmax.  (Without the
// NaN test a NaN with the sign bit set -- 0xffc00000, what inf - inf gives on x86 -- would sort below -inf.)
// ordered_key_inv gives a NaN back for the top key.  v != v is one compare; this file is built without fast-math.
__device__ __forceinline__ uint32_t ordered_key(float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return v != v ? 0xffffffffu : k;
}
__device__ __forceinline__ float ordered_key_inv(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Four consecutive elements i0 .. i0+3 of a row (i0 % 4 == 0, i0 < vocab); returns how many are in
// range.  `vec` bit 0: the row start is 16-B (f32) / 8-B (16-bit types) aligned, so one wide load is legal.  DT 3: the element
// type is a run-time value (act_dtype) in vec's bits above bit 0 -- the verification against a sampled draft reads two rows of
// independent types and is compiled once.
template <int DT>
__device__ __forceinline__ int load4(const void* row, int i0, int vocab, int vec, float (&v)[4]) {
    const int n = min(4, vocab - i0);
    const int dt = DT == 3 ? (vec >> 1) : DT;
    const bool wide = (vec & 1) && n == 4;
    if (dt == 2) {
        const float* p = reinterpret_cast<const float*>(row) + i0;
        if (wide) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = t[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < n ? p[k] : 0.f;
        }
    } else {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(row) + i0;
        uint16_t h[4];
        if (wide) {
            const i32x2 t = *reinterpret_cast<const i32x2*>(p);
            h[0] = (uint16_t)((uint32_t)t[0] & 0xffffu);
            h[1] = (uint16_t)((uint32_t)t[0] >> 16);
            h[2] = (uint16_t)((uint32_t)t[1] & 0xffffu);
            h[3] = (uint16_t)((uint32_t)t[1] >> 16);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) h[k] = k < n ? p[k] : (uint16_t)0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = dt == 0 ? bf16_to_f32(h[k]) : f16_to_f32(h[k]);
    }
    return n;
}

// One pass over a row: every wave visits its 256-element chunks (wave w: [256 w + 4096 j, + 256)), a lane
// four consecutive elements per chunk.  The loads of U chunks are issued before the first is consumed:
// a pass is otherwise one dependent HBM / L2 round trip per chunk (measured: 25 us per pass over
// 129280 floats with one load in flight per lane).  body(i0, v[4], n) is called by the WHOLE wave for
// every chunk (n = 0 for lanes past the end of the row), so it may use wave-wide operations.
constexpr int kSampleUnroll = 8;
template <int DT, int U, typename F>
__device__ __forceinline__ void for_each_quad(const void* row, int vocab, int vec, F&& body) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = wave * 256; base < vocab; base += kSampleThreads * 4 * U) {  // wave-uniform trip count
        float v[U][4];
        int n[U];
        auto load_all = [&](auto dt) {
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int i0 = base + q * kSampleThreads * 4 + lane * 4;
                n[q] = i0 < vocab ? load4<decltype(dt)::value>(row, i0, vocab, vec & 1, v[q]) : 0;
            }
        };
        if constexpr (DT == 3) {  // one branch around the U loads, so they stay in flight together
            if ((vec >> 1) == 2) load_all(std::integral_constant<int, 2>{});
            else if ((vec >> 1) == 0) load_all(std::integral_constant<int, 0>{});
            else load_all(std::integral_constant<int, 1>{});
        } else {
            load_all(std::integral_constant<int, DT>{});
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            if (base + q * kSampleThreads * 4 < vocab)  // wave-uniform
                body(base + q * kSampleThreads * 4 + lane * 4, v[q], n[q]);
        }
    }
}

// x = logits / temperature (executor.py:106, an IEEE f32 division) in logits mode; the probability
// itself in probs mode (utils.py:62 takes probabilities).
__device__ __forceinline__ float sample_x(float v, float temperature, int probs_mode) {
    // v / 1.0f == v bit for bit: greedy batches and unit temperatures skip the ~10-instruction IEEE
    // division (the passes over a row are VALU-bound: one workgroup per row)
    return (probs_mode || temperature == 1.0f) ? v : v / temperature;
}
// weight in [0, 1] relative to the row maximum m: exp(x - m) (softmax numerator) or p / max p.  The
// same expression is evaluated in every pass, so every pass sees the same bits.
__device__ __forceinline__ float sample_e(float x, float m, int probs_mode) {
#pragma clang fp contract(off)
    const float e = probs_mode ? x / m : __expf(x - m);
    return __builtin_fminf(__builtin_fmaxf(e, 0.f), 1.f);  // NaN -> 0
}
__device__ __forceinline__ uint64_t sample_fix(float e) { return (uint64_t)(e * kSampleFixScale); }

struct SampleShared {
    uint32_t cnt[kSampleBins];
    uint64_t sum[kSampleBins];
    uint64_t wave_u64[kSampleWaves];
    uint32_t wave_u32[kSampleWaves];
    uint64_t seg_strict[kSampleWaves];
    uint32_t seg_ties[kSampleWaves];
    uint64_t seg_draft[kSampleWaves];       // chitu_hip_speculative_verify: the draft's entry, found by the segment pass
    uint32_t seg_ties_below[kSampleWaves];  // and the ties at tau below the draft's index
    // boundary bin of the current level
    int b_found;
    uint32_t b_bin, b_cexcl, b_cnt;
    uint64_t b_sexcl, b_sum, total;
};

// One histogram level: elements whose key >> (shift + 10) == prefix (level 1: all) are binned by
// (key >> shift) & 1023 with (count, fixed-point sum).  Lanes of a wave that hit the same bin as the
// wave's first active lane are combined in registers first (two rounds): flat distributions put
// most of the vocabulary in a handful of bins and same-address LDS atomics serialise.
template <int DT>
__device__ __forceinline__ void sample_hist_level(SampleShared& sh, const void* row, int vocab, int vec,
                                                  float temperature, float m, int probs_mode, int shift,
                                                  bool use_prefix, uint32_t prefix) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int b = tid; b < kSampleBins; b += kSampleThreads) {
        sh.cnt[b] = 0;
        sh.sum[b] = 0;
    }
    __syncthreads();
    for_each_quad<DT, kSampleUnroll>(row, vocab, vec, [&](int i0, const float (&v)[4], int n) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = sample_e(sample_x(v[k], temperature, probs_mode), m, probs_mode);
            const uint32_t key = __float_as_uint(e);
            const uint64_t w = sample_fix(e);
            bool act = k < n && (!use_prefix || (key >> (shift + 10)) == prefix);
            const int b = (int)((key >> shift) & (kSampleBins - 1));
            uint64_t rem = __builtin_amdgcn_ballot_w64(act);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (rem == 0) break;  // wave-uniform
                const int leader = __builtin_amdgcn_readfirstlane(__builtin_ctzll(rem));
                const int lb = __builtin_amdgcn_readlane(b, leader);
                const bool same = act && b == lb;
                const uint64_t smask = __builtin_amdgcn_ballot_w64(same);
                const uint64_t ws = wave_sum_u64(same ? w : 0ull);
                if (lane == leader) {
                    atomicAdd(&sh.cnt[lb], (uint32_t)__builtin_popcountll(smask));
                    atomicAdd(reinterpret_cast<unsigned long long*>(&sh.sum[lb]), (unsigned long long)ws);
                }
                act = act && !same;
                rem &= ~smask;
            }
            if (act) {
                atomicAdd(&sh.cnt[b], 1u);
                atomicAdd(reinterpret_cast<unsigned long long*>(&sh.sum[b]), (unsigned long long)w);
            }
        }
    });
    __syncthreads();
}

// Walk the bins from the largest weight down: the boundary bin is the first whose inclusive count
// reaches k_rem or whose inclusive sum exceeds p_rem (everything before it is kept whole).  Thread t
// owns bin 1023 - t.  Leaves {b_found, b_bin, b_cexcl, b_sexcl, b_cnt, b_sum, total} in LDS.
// `p_from_total`: level 1 derives p_rem = floor(top_p * total) once the total is known.
__device__ __forceinline__ void sample_find_boundary(SampleShared& sh, uint32_t k_rem, uint64_t& p_rem,
                                                     bool p_from_total, float top_p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = kSampleBins - 1 - tid;
    const uint32_t c_own = sh.cnt[b];
    const uint64_t s_own = sh.sum[b];
    uint32_t c = c_own;
    uint64_t s = s_own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t c2 = (uint32_t)__shfl_up((int)c, off, 64);
        const uint64_t s2 = shfl_up_u64(s, off);
        if (lane >= off) {
            c += c2;
            s += s2;
        }
    }
    if (lane == 63) {
        sh.wave_u32[wave] = c;
        sh.wave_u64[wave] = s;
    }
    if (tid == 0) sh.b_found = 0;
    __syncthreads();
    uint32_t co = 0;
    uint64_t so = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) {
        if (w < wave) {
            co += sh.wave_u32[w];
            so += sh.wave_u64[w];
        }
        tot += sh.wave_u64[w];
    }
    if (p_from_total) {
        // floor(top_p * Z) in f64: one IEEE multiply of two exactly-converted operands
        // (top_p >= 1 keeps everything: the mathematical meaning of utils.py:72, whose f32 cumsum can
        // overshoot 1.0 by an ulp)
        const double pz = (double)__builtin_fmaxf(top_p, 0.f) * (double)tot;
        p_rem = (top_p >= 1.0f || pz >= 18446744073709549568.0) ? ~0ull : (uint64_t)pz;
    }
    const uint32_t c_incl = c + co, c_excl = c_incl - c_own;
    const uint64_t s_incl = s + so, s_excl = s_incl - s_own;
    const bool cond = c_incl >= k_rem || s_incl > p_rem;
    const bool cond_prev = c_excl >= k_rem || s_excl > p_rem;
    if (cond && !cond_prev) {  // exactly one bin (an empty bin has cond == cond_prev)
        sh.b_found = 1;
        sh.b_bin = (uint32_t)b;
        sh.b_cexcl = c_excl;
        sh.b_sexcl = s_excl;
        sh.b_cnt = c_own;
        sh.b_sum = s_own;
    }
    if (tid == 0) sh.total = tot;
    __syncthreads();
}

// ---------------------------------------------------------------- candidate fast path
// Peaked rows (what a language model emits) keep a few dozen tokens out of 129280, so the prefix can be
// cut from a short candidate list instead of three histogram passes over the row:
//   pass 1  Z = sum of the fixed-point weights, and how many weights reach each of five thresholds
//           2^-4 .. 2^-20 of the maximum (register counters, no atomics);
//   pass 2  the elements above the lowest threshold that admits <= kCandCap of them are appended
//           (key, index) to LDS (one LDS atomic per wave-load);
//   then    a bitonic sort in the specification's order (key descending, index ascending), a scan of
//           the exact integer weights for the top-k / top-p cut, a second sort of the kept entries by
//           index and a scan for the inverse CDF.
// The list provably holds the whole kept prefix iff the cut falls inside it, or it is as long as
// top_k, or its mass already exceeds top_p * Z, or it is the whole row; otherwise (flat rows, huge
// top_k, no limits at all) the radix descent below runs.  Both paths evaluate the same integer
// specification (oracle/sampling.py::sample_fixed_point), so which one ran cannot be told from the
// result.
constexpr int kCandCap = 1024;
constexpr int kCandLevels = 5;
__device__ __forceinline__ uint32_t cand_threshold_key(int j) { return (uint32_t)(127 - 4 * (j + 1)) << 23; }  // bits of 2^-(4j+4)

__device__ __forceinline__ uint64_t block_sum_u64(SampleShared& sh, uint64_t v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_sum_u64(v);
    __syncthreads();  // earlier readers of wave_u64 are done
    if (lane == 0) sh.wave_u64[wave] = v;
    __syncthreads();
    uint64_t s = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) s += sh.wave_u64[w];
    return s;
}

// exclusive prefix sum over the workgroup's threads (thread order); `total` = sum over all threads
__device__ __forceinline__ uint64_t block_excl_scan_u64(SampleShared& sh, uint64_t v, uint64_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = shfl_up_u64(incl, off);
        if (lane >= off) incl += o;
    }
    __syncthreads();
    if (lane == 63) sh.wave_u64[wave] = incl;
    __syncthreads();
    uint64_t before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) {
        if (w < wave) before += sh.wave_u64[w];
        tot += sh.wave_u64[w];
    }
    total = tot;
    return before + incl - v;
}

// in-place bitonic sort of a[0 .. n) in LDS, n a power of two <= kSampleThreads, one element per thread
template <bool DESCENDING>
__device__ __forceinline__ void bitonic_sort_lds(uint64_t* a, int n) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int p = tid ^ j;
            if (tid < n && p > tid) {
                const uint64_t x = a[tid], y = a[p];
                const bool first_half = (tid & k) == 0;
                const bool swap = (DESCENDING == first_half) ? x < y : x > y;
                if (swap) {
                    a[tid] = y;
                    a[p] = x;
                }
            }
            __syncthreads();
        }
    }
}

// The integer position in [0, s) that a uniform u in [0, 1) selects, s > 0 (oracle/sampling.py::sample_fixed_point).
__device__ __forceinline__ uint64_t sample_target(float u, uint64_t s) {
    const double t = (double)__builtin_fminf(__builtin_fmaxf(u, 0.f), 1.f) * (double)s;
    uint64_t target = t >= (double)s ? s - 1 : (uint64_t)t;
    if (target >= s) target = s - 1;
    return target;
}

// One row of chitu_hip_sample, or (VERIFY) of chitu_hip_speculative_verify: the sample row with a draft.  Both kernels run
// the passes below on it; what VERIFY adds is compiled out of the sample kernel (if constexpr).
struct SampleRow {
    const void* row;
    int vocab;
    int vec;  // load4's
    float temperature;
    int probs_mode;
    int top_k;
    float top_p;
    float u;  // the draw's uniform (VERIFY: u_alt, which draws the replacement / bonus token)
    int row_id;
    int64_t arg_max;
    float m;  // the row maximum of x
    int64_t* token_out;  // this row's slot (VERIFY: the token, bit 32 set when the draft was accepted)
    int32_t* n_kept_out;
    float* kept_mass_out;
    // VERIFY only
    int draft;    // the proposed token; < 0: none (the bonus row), the row is a plain draw
    float u_acc;  // accepted iff target(u_acc, S) < w_draft
    int32_t* accepted_out;
    int64_t* row_token_out;
};

constexpr int64_t kVerifyAcceptedBit = (int64_t)1 << 32;  // tokens are < 2^31

// Called by one thread of the row's workgroup.
template <bool VERIFY>
__device__ __forceinline__ void sample_emit(const SampleRow& r, int64_t token, bool accepted) {
    if constexpr (VERIFY) {
        *r.token_out = accepted ? (token | kVerifyAcceptedBit) : token;
        if (r.accepted_out) r.accepted_out[r.row_id] = accepted ? 1 : 0;
        if (r.row_token_out) r.row_token_out[r.row_id] = token;
    } else {
        *r.token_out = token;
    }
}

// Pass 0: the row maximum of x and its (lowest) index -> r.m, r.arg_max.  Must be called by the whole workgroup.
template <int DT>
__device__ __forceinline__ void sample_row_max(SampleShared& sh, SampleRow& r) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float temperature = r.temperature;
    const int probs_mode = r.probs_mode;
    uint64_t best = 0;
    for_each_quad<DT, kSampleUnroll>(r.row, r.vocab, r.vec, [&](int i0, const float (&v)[4], int n) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                const uint64_t key = ((uint64_t)ordered_key(sample_x(v[k], temperature, probs_mode)) << 32) |
                                     (uint32_t)(0xffffffffu - (uint32_t)(i0 + k));
                best = key > best ? key : best;
            }
        }
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = shfl_xor_u64(best, off);
        best = o > best ? o : best;
    }
    if (lane == 0) sh.wave_u64[wave] = best;
    __syncthreads();
    best = sh.wave_u64[0];
#pragma unroll
    for (int w = 1; w < kSampleWaves; ++w) best = sh.wave_u64[w] > best ? sh.wave_u64[w] : best;
    __syncthreads();  // wave_u64 is reused below
    r.arg_max = (int64_t)(0xffffffffu - (uint32_t)best);
    r.m = ordered_key_inv((uint32_t)(best >> 32));
}

// Returns true when the token (and the optional statistics) have been written; false = not applicable,
// nothing written, the caller runs the radix descent.  Must be called by the whole workgroup.
// VERIFY: membership and weight of the draft come from the sorted list; a rejected draft's entry is
// left out of the second sort, so the inverse CDF runs over the kept set without it.
template <int DT, bool VERIFY>
__device__ __forceinline__ bool sample_candidates(SampleShared& sh, const SampleRow& r) {
    const void* row = r.row;
    const int vocab = r.vocab, probs_mode = r.probs_mode, top_k = r.top_k;
    const int vec = r.vec;
    const float temperature = r.temperature, m = r.m, top_p = r.top_p;
    const int tid = threadIdx.x, lane = tid & 63;
    uint64_t* arr = sh.sum;  // the histogram's sum array doubles as the sort buffer (kCandCap == kSampleBins)
    // ---- pass 1: Z and the five threshold counts (21 bits each: vocab < 2^21 per the entry point)
    uint64_t z = 0, ca = 0, cb = 0;
    for_each_quad<DT, kSampleUnroll>(row, vocab, vec, [&](int i0, const float (&v)[4], int n) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                const float e = sample_e(sample_x(v[k], temperature, probs_mode), m, probs_mode);
                const uint32_t key = __float_as_uint(e);
                z += sample_fix(e);
                ca += (uint64_t)(key >= cand_threshold_key(0)) | ((uint64_t)(key >= cand_threshold_key(1)) << 21) |
                      ((uint64_t)(key >= cand_threshold_key(2)) << 42);
                cb += (uint64_t)(key >= cand_threshold_key(3)) | ((uint64_t)(key >= cand_threshold_key(4)) << 21);
            }
        }
    });
    z = block_sum_u64(sh, z);
    ca = block_sum_u64(sh, ca);
    cb = block_sum_u64(sh, cb);
    const uint32_t counts[kCandLevels] = {(uint32_t)(ca & 0x1fffffu), (uint32_t)((ca >> 21) & 0x1fffffu),
                                          (uint32_t)((ca >> 42) & 0x1fffffu), (uint32_t)(cb & 0x1fffffu),
                                          (uint32_t)((cb >> 21) & 0x1fffffu)};
    if (z == 0 || counts[0] > (uint32_t)kCandCap) return false;
    int level = 0;
#pragma unroll
    for (int j = 1; j < kCandLevels; ++j)
        if (counts[j] <= (uint32_t)kCandCap) level = j;
    const uint32_t tkey = cand_threshold_key(level);
    const int n_cand = (int)counts[level];
    uint64_t p_rem;
    {
        const double pz = (double)__builtin_fmaxf(top_p, 0.f) * (double)z;  // as sample_find_boundary
        p_rem = (top_p >= 1.0f || pz >= 18446744073709549568.0) ? ~0ull : (uint64_t)pz;
    }
    const uint32_t k_eff = top_k <= 0 ? 0xffffffffu : (uint32_t)top_k;
    // ---- pass 2: append (key, index) of every weight >= the threshold; one LDS atomic per wave-load
    if (tid == 0) sh.b_cnt = 0;
    __syncthreads();
    for_each_quad<DT, kSampleUnroll>(row, vocab, vec, [&](int i0, const float (&v)[4], int n) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t key = 0;
            if (k < n) key = __float_as_uint(sample_e(sample_x(v[k], temperature, probs_mode), m, probs_mode));
            const bool take = k < n && key >= tkey;
            const uint64_t mask = __builtin_amdgcn_ballot_w64(take);
            if (mask) {  // wave-uniform
                uint32_t start = 0;
                if (lane == 0) start = atomicAdd(&sh.b_cnt, (uint32_t)__builtin_popcountll(mask));
                start = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
                const uint64_t below = lane == 0 ? 0ull : (mask & (~0ull >> (64 - lane)));
                if (take)
                    arr[start + (uint32_t)__builtin_popcountll(below)] =
                        ((uint64_t)key << 32) | (uint32_t)(0xffffffffu - (uint32_t)(i0 + k));
            }
        }
    });
    int npow = 64;
    while (npow < n_cand) npow <<= 1;
    __syncthreads();
    if (tid >= n_cand && tid < npow) arr[tid] = 0ull;  // below every real entry (a real key is >= the threshold > 0)
    __syncthreads();
    bitonic_sort_lds<true>(arr, npow);  // key descending, ties: lower index first
    // ---- the cut: position < top_k and exclusive cumulative weight <= top_p * Z (utils.py:72-76)
    const uint64_t mine = tid < n_cand ? arr[tid] : 0ull;
    const uint32_t my_key = (uint32_t)(mine >> 32);
    const uint32_t my_idx = 0xffffffffu - (uint32_t)mine;
    const uint64_t w = tid < n_cand ? sample_fix(__uint_as_float(my_key)) : 0ull;
    uint64_t s_cand;
    const uint64_t excl = block_excl_scan_u64(sh, w, s_cand);
    const bool kept = tid < n_cand && (uint32_t)tid < k_eff && excl <= p_rem;
    const uint64_t packed = block_sum_u64(sh, kept ? ((w << 11) | 1ull) : 0ull);  // w <= 2^40, <= 1024 kept: 51 + 11 bits
    const int n_kept = (int)(packed & 0x7ffu);
    const uint64_t s_kept = packed >> 11;
    const bool sufficient = n_kept < n_cand || (uint32_t)n_cand >= k_eff || s_cand > p_rem || n_cand == vocab;
    if (!sufficient) return false;
    if (tid == 0) {
        if (r.n_kept_out) r.n_kept_out[r.row_id] = n_kept;
        if (r.kept_mass_out) r.kept_mass_out[r.row_id] = (float)((double)s_kept / (double)z);
    }
    if (s_kept == 0) {
        if (tid == 0) sample_emit<VERIFY>(r, r.arg_max, VERIFY && (int64_t)r.draft == r.arg_max);
        return true;
    }
    uint64_t s_draw = s_kept;  // the mass the token is drawn from
    int n_draw = n_kept;
    bool in_draw = kept;
    if constexpr (VERIFY) {
        if (r.draft >= 0) {  // workgroup-uniform
            const bool is_draft = kept && my_idx == (uint32_t)r.draft;
            const uint64_t w_d = block_sum_u64(sh, is_draft ? w : 0ull);  // a kept candidate's weight is > 0: 0 = not kept
            if (sample_target(r.u_acc, s_kept) < w_d) {  // probability w_d / S; w_d == S always accepts
                if (tid == 0) sample_emit<VERIFY>(r, (int64_t)r.draft, true);
                return true;
            }
            s_draw -= w_d;
            n_draw -= w_d ? 1 : 0;
            in_draw = kept && !is_draft;
        }
    }
    const uint64_t target = sample_target(r.u, s_draw);
    // ---- inverse CDF over the kept entries in INDEX order: sort them by index, scan, pick
    __syncthreads();
    if (tid < npow) arr[tid] = in_draw ? (((uint64_t)my_idx << 32) | my_key) : ~0ull;
    __syncthreads();
    bitonic_sort_lds<false>(arr, npow);
    const uint64_t ent = tid < n_draw ? arr[tid] : 0ull;
    const uint64_t w2 = tid < n_draw ? sample_fix(__uint_as_float((uint32_t)ent)) : 0ull;
    uint64_t unused_total;
    const uint64_t excl2 = block_excl_scan_u64(sh, w2, unused_total);
    if (tid < n_draw && excl2 <= target && target < excl2 + w2) sample_emit<VERIFY>(r, (int64_t)(ent >> 32), false);
    return true;
}

// The kept prefix of a row from the radix descent: the kept set is {key > tau} plus the first c_keep ties at tau in index
// order, every tie weighs e_tau, the kept mass is s_kept.  (keep_all: tau = 0, e_tau = 0, c_keep = all.)
struct SampleCut {
    uint32_t tau, c_keep;
    uint64_t e_tau, s_kept;
};

// Radix descent for (tau, c_keep); writes the optional statistics.  Must be called by the whole workgroup.
template <int DT>
__device__ __forceinline__ SampleCut sample_radix_cut(SampleShared& sh, const SampleRow& r) {
    const void* row = r.row;
    const int vocab = r.vocab, probs_mode = r.probs_mode, top_k = r.top_k;
    const int vec = r.vec;
    const float temperature = r.temperature, m = r.m, top_p = r.top_p;
    uint32_t k_rem = top_k <= 0 ? 0xffffffffu : (uint32_t)top_k;  // <= 0: no top-k limit
    uint64_t p_rem = 0;
    uint32_t tau = 0, c_above = 0, c_keep = 0xffffffffu;
    uint64_t s_above = 0, e_tau = 0, z_total = 0;
    bool keep_all = false;
    sample_hist_level<DT>(sh, row, vocab, vec, temperature, m, probs_mode, 20, false, 0u);
    sample_find_boundary(sh, k_rem, p_rem, true, top_p);
    z_total = sh.total;
    if (!sh.b_found) {
        keep_all = true;
    } else {
        uint32_t prefix = sh.b_bin;
        c_above = sh.b_cexcl;
        s_above = sh.b_sexcl;
        k_rem -= sh.b_cexcl;
        p_rem -= sh.b_sexcl;
#pragma unroll 1
        for (int shift = 10; shift >= 0; shift -= 10) {
            __syncthreads();  // every thread has read the previous level's result
            sample_hist_level<DT>(sh, row, vocab, vec, temperature, m, probs_mode, shift, true, prefix);
            sample_find_boundary(sh, k_rem, p_rem, false, top_p);
            // the parent bin met the condition as a whole, so one of its children does
            prefix = (prefix << 10) | sh.b_bin;
            c_above += sh.b_cexcl;
            s_above += sh.b_sexcl;
            k_rem -= sh.b_cexcl;
            p_rem -= sh.b_sexcl;
        }
        tau = prefix;
        const uint32_t c_tau = sh.b_cnt;
        e_tau = c_tau ? sh.b_sum / c_tau : 0;  // all entries of the bin share one key, hence one weight
        // tie j (0-based) is kept iff j < k_rem and s_above + j * e_tau <= p, i.e. j <= p_rem / e_tau
        uint64_t c_p = e_tau ? p_rem / e_tau + 1 : (uint64_t)c_tau;
        c_p = c_p < c_tau ? c_p : c_tau;
        c_keep = (uint32_t)(c_p < k_rem ? c_p : k_rem);
    }
    const uint64_t s_kept = keep_all ? z_total : s_above + (uint64_t)c_keep * e_tau;
    if (threadIdx.x == 0) {
        if (r.n_kept_out) r.n_kept_out[r.row_id] = keep_all ? vocab : (int32_t)(c_above + c_keep);
        if (r.kept_mass_out) r.kept_mass_out[r.row_id] = z_total ? (float)((double)s_kept / (double)z_total) : 0.f;
    }
    return SampleCut{tau, c_keep, e_tau, s_kept};
}

// Segment pass: kept strict mass and tie count of each wave's contiguous segment -> sh.seg_strict / seg_ties.
// VERIFY: also, per segment, the ties at tau with an index below the draft (summed: the draft's rank among the ties)
// and the draft's own entry -- its weight if it is above tau, or that it is a tie -> sh.seg_ties_below / seg_draft.
constexpr uint64_t kDraftIsTie = 1ull << 62;  // weights are <= 2^40
template <int DT, bool VERIFY>
__device__ __forceinline__ void sample_segment_pass(SampleShared& sh, const SampleRow& r, const SampleCut& cut, int seg_begin,
                                                    int seg_end) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t tau = cut.tau;
    uint64_t strict = 0, draft_entry = 0;
    uint32_t ties = 0, ties_below = 0;
    for (int base = seg_begin; base < seg_end; base += 256) {
        const int i0 = base + lane * 4;
        if (i0 < seg_end) {
            float v[4];
            const int n = load4<DT>(r.row, i0, r.vocab, r.vec, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float e = sample_e(sample_x(v[k], r.temperature, r.probs_mode), r.m, r.probs_mode);
                const uint32_t key = __float_as_uint(e);
                if (k < n) {
                    if (key > tau) strict += sample_fix(e);
                    ties += key == tau ? 1u : 0u;
                    if constexpr (VERIFY) {
                        ties_below += (key == tau && i0 + k < r.draft) ? 1u : 0u;
                        if (i0 + k == r.draft) draft_entry = key > tau ? sample_fix(e) : (key == tau ? kDraftIsTie : 0ull);
                    }
                }
            }
        }
    }
    strict = wave_sum_u64(strict);
    ties = (uint32_t)wave_sum_u64((uint64_t)ties);
    if constexpr (VERIFY) {
        draft_entry = wave_sum_u64(draft_entry);  // one lane of one wave at the most holds the draft
        ties_below = (uint32_t)wave_sum_u64((uint64_t)ties_below);
    }
    if (lane == 0) {
        sh.seg_strict[wave] = strict;
        sh.seg_ties[wave] = ties;
        if constexpr (VERIFY) {
            sh.seg_draft[wave] = draft_entry;
            sh.seg_ties_below[wave] = ties_below;
        }
    }
}

// Rescan: the one wave whose segment holds `target` walks it with prefix sums and emits the token.  `run` / `ties_run`:
// kept mass / ties before the segment.  VERIFY: the rejected draft's index weighs nothing.  Called by that wave alone.
template <int DT, bool VERIFY>
__device__ __forceinline__ void sample_rescan(const SampleRow& r, const SampleCut& cut, int seg_begin, int seg_end, uint64_t run,
                                              uint32_t ties_run, uint64_t target) {
    const int lane = threadIdx.x & 63;
    const uint32_t tau = cut.tau, c_keep = cut.c_keep;
    const uint64_t e_tau = cut.e_tau;
    for (int base = seg_begin; base < seg_end; base += 256) {
        const int i0 = base + lane * 4;
        float v[4];
        const int n = i0 < seg_end ? load4<DT>(r.row, i0, r.vocab, r.vec, v) : 0;
        uint64_t w4[4];
        bool tie4[4];
        uint32_t t_l = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = sample_e(sample_x(v[k], r.temperature, r.probs_mode), r.m, r.probs_mode);
            const uint32_t key = __float_as_uint(e);
            tie4[k] = k < n && key == tau;
            w4[k] = (k < n && key > tau) ? sample_fix(e) : 0ull;
            t_l += tie4[k] ? 1u : 0u;
        }
        // exclusive prefix of the tie counts over the lanes (index order = lane order)
        uint32_t t_incl = t_l;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)t_incl, off, 64);
            if (lane >= off) t_incl += o;
        }
        uint32_t rank = ties_run + t_incl - t_l;
        uint64_t s_l = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (tie4[k]) {
                if (rank < c_keep) w4[k] = e_tau;
                ++rank;
            }
            if constexpr (VERIFY) {
                if (i0 + k == r.draft) w4[k] = 0ull;
            }
            s_l += w4[k];
        }
        uint64_t s_incl = s_l;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t o = shfl_up_u64(s_incl, off);
            if (lane >= off) s_incl += o;
        }
        const uint64_t hit = __builtin_amdgcn_ballot_w64(run + s_incl > target);
        if (hit) {
            const int first = __builtin_ctzll(hit);
            if (lane == first) {
                uint64_t acc = run + s_incl - s_l;
                int pick = 0;
                bool done = false;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    acc += w4[k];
                    if (!done && acc > target) {
                        pick = k;
                        done = true;
                    }
                }
                sample_emit<VERIFY>(r, (int64_t)(i0 + pick), false);
            }
            return;
        }
        run += (uint64_t)(((uint64_t)(uint32_t)__shfl((int)(s_incl >> 32), 63, 64) << 32) |
                          (uint32_t)__shfl((int)(uint32_t)s_incl, 63, 64));
        ties_run += (uint32_t)__shfl((int)t_incl, 63, 64);
    }
    if (lane == 0) sample_emit<VERIFY>(r, r.arg_max, false);  // unreachable: the segment sums add up to the drawn mass
}

// Everything after pass 0 for a row that is not greedy.  Must be called by the whole workgroup.
template <int DT, bool VERIFY>
__device__ __forceinline__ void sample_row_draw(SampleShared& sh, const SampleRow& r, int use_candidates) {
    const int tid = threadIdx.x, wave = tid >> 6;
    // ---- short candidate list first (peaked rows); the radix descent below is the general path
    if (use_candidates && r.vocab < (1 << 21) && sample_candidates<DT, VERIFY>(sh, r)) return;
    __syncthreads();  // the candidate path's LDS (sh.sum, counters) is about to be reused

    const SampleCut cut = sample_radix_cut<DT>(sh, r);
    if (cut.s_kept == 0) {  // no positive weight at all (NaN row / all-zero probabilities)
        if (tid == 0) sample_emit<VERIFY>(r, r.arg_max, VERIFY && (int64_t)r.draft == r.arg_max);
        return;
    }
    uint64_t target = 0;
    if constexpr (!VERIFY) target = sample_target(r.u, cut.s_kept);

    // ---- inverse CDF in index order.  Segment pass: kept mass and tie count of each wave's contiguous
    // segment; then the one wave whose segment holds `target` rescans it with prefix sums.
    const int seg_len = ((r.vocab + kSampleWaves - 1) / kSampleWaves + 255) / 256 * 256;
    const int seg_begin = min(wave * seg_len, r.vocab), seg_end = min(seg_begin + seg_len, r.vocab);
    sample_segment_pass<DT, VERIFY>(sh, r, cut, seg_begin, seg_end);
    __syncthreads();
    uint64_t w_d = 0;  // VERIFY: the rejected draft's kept weight, which its segment loses
    int draft_wave = -1;
    if constexpr (VERIFY) {
        if (r.draft >= 0) {  // workgroup-uniform
            uint64_t entry = 0;
            uint32_t rank = 0;
#pragma unroll
            for (int w = 0; w < kSampleWaves; ++w) {
                entry += sh.seg_draft[w];
                rank += sh.seg_ties_below[w];
            }
            // a tie at tau is kept iff its rank among the ties in index order is below c_keep, as in the draw
            w_d = (entry & kDraftIsTie) ? (rank < cut.c_keep ? cut.e_tau : 0ull) : entry;
            if (sample_target(r.u_acc, cut.s_kept) < w_d) {  // probability w_d / S; w_d == S always accepts
                if (tid == 0) sample_emit<VERIFY>(r, (int64_t)r.draft, true);
                return;
            }
            draft_wave = r.draft / seg_len;
        }
        target = sample_target(r.u, cut.s_kept - w_d);
    }
    int wsel = -1;
    uint64_t run = 0;        // kept mass before the selected segment
    uint32_t ties_run = 0;   // ties before it
    {
        uint64_t cum = 0;
        uint32_t tb = 0;
#pragma unroll
        for (int w = 0; w < kSampleWaves; ++w) {
            const uint32_t st = sh.seg_ties[w];
            const uint64_t left = (uint64_t)cut.c_keep > (uint64_t)tb ? (uint64_t)cut.c_keep - tb : 0ull;
            const uint64_t kt = left < st ? left : (uint64_t)st;
            uint64_t s = sh.seg_strict[w] + kt * cut.e_tau;
            if constexpr (VERIFY) {
                if (w == draft_wave) s -= w_d;
            }
            if (wsel < 0 && target < cum + s) {
                wsel = w;
                run = cum;
                ties_run = tb;
            }
            cum += s;
            tb += st;
        }
    }
    if (wsel < 0) {  // unreachable (the segment sums add up to the drawn mass); keep the launch well-defined
        if (tid == 0) sample_emit<VERIFY>(r, r.arg_max, false);
        return;
    }
    if (wave != wsel) return;
    sample_rescan<DT, VERIFY>(r, cut, seg_begin, seg_end, run, ties_run, target);
}

template <int DT>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(
    const void* __restrict__ logits, int64_t row_stride, int vocab, const float* __restrict__ temperatures,
    const int32_t* __restrict__ top_ks, const float* __restrict__ top_ps, const float* __restrict__ uniforms,
    int probs_mode, int64_t* __restrict__ out_tokens, int32_t* __restrict__ n_kept_out,
    float* __restrict__ kept_mass_out, int use_candidates) {
    __shared__ SampleShared sh;
    const int row_id = blockIdx.x;
    const int elem = DT == 2 ? 4 : 2;
    const bool greedy_all = top_ks == nullptr;
    SampleRow r = {};
    r.row = reinterpret_cast<const char*>(logits) + (int64_t)row_id * row_stride * elem;
    r.vocab = vocab;
    r.vec = (reinterpret_cast<uintptr_t>(r.row) & (uintptr_t)(4 * elem - 1)) == 0;
    r.top_k = greedy_all ? 1 : top_ks[row_id];
    r.temperature = (greedy_all || probs_mode) ? 1.0f : temperatures[row_id];
    r.probs_mode = probs_mode;
    r.row_id = row_id;
    r.token_out = out_tokens + row_id;
    r.n_kept_out = n_kept_out;
    r.kept_mass_out = kept_mass_out;
    sample_row_max<DT>(sh, r);
    if (r.top_k == 1) {  // greedy row (executor.py:103-104; a top_k of 1 keeps only the first sorted entry)
        if (threadIdx.x == 0) {
            out_tokens[row_id] = r.arg_max;
            if (n_kept_out) n_kept_out[row_id] = 1;
            if (kept_mass_out) kept_mass_out[row_id] = 0.f;
        }
        return;
    }
    r.top_p = top_ps[row_id];
    r.u = uniforms[row_id];
    sample_row_draw<DT, false>(sh, r, use_candidates);
}

// ---------------------------------------------------------------- speculative decoding: draft verification
// Row stage of chitu_hip_speculative_verify (new: no reference counterpart): row (b, t) of T rows per sequence is the
// sample row with the deterministic draft drafts[row] for its token.  The draft distribution is a point mass, so
// rejection sampling against the row's distribution p is: accept d with probability p(d) = w_d / S (in the sampler's
// integers: target(u_acc, S) < w_d), otherwise draw from p without d, renormalised (the inverse CDF over K \ {d} at
// target(u_alt, S - w_d)).  Lossless: P(emit d) = p(d), and P(emit x != d) = (1 - p(d)) * p(x) / (1 - p(d)) = p(x).
// Greedy (top_k == 1) and degenerate (S == 0) rows accept iff d == argmax and emit the arg-max; a row without a draft
// (d < 0, the bonus row) is chitu_hip_sample's row for u_alt.  The specification is tests/spec_verify_ref.py.
// The row writes its token into out[b, 1 + t], with kVerifyAcceptedBit set when the draft was accepted; the sequence
// stage (next launch) turns that into the result.
template <int DT>
__global__ __launch_bounds__(kSampleThreads) void verify_rows_kernel(
    const void* __restrict__ logits, int64_t row_stride, int vocab, const float* __restrict__ temperatures,
    const int32_t* __restrict__ top_ks, const float* __restrict__ top_ps, const int32_t* __restrict__ drafts,
    const float* __restrict__ uniforms, int q_len, int probs_mode, int64_t* __restrict__ out,
    int32_t* __restrict__ accepted_out, int64_t* __restrict__ row_tokens_out, int use_candidates) {
    __shared__ SampleShared sh;
    const int row_id = blockIdx.x;
    const int elem = DT == 2 ? 4 : 2;
    SampleRow r = {};
    r.row = reinterpret_cast<const char*>(logits) + (int64_t)row_id * row_stride * elem;
    r.vocab = vocab;
    r.vec = (reinterpret_cast<uintptr_t>(r.row) & (uintptr_t)(4 * elem - 1)) == 0;
    r.top_k = top_ks[row_id];
    r.temperature = probs_mode ? 1.0f : temperatures[row_id];
    r.probs_mode = probs_mode;
    r.row_id = row_id;
    r.token_out = out + (int64_t)(row_id / q_len) * (q_len + 1) + 1 + row_id % q_len;
    r.n_kept_out = nullptr;
    r.kept_mass_out = nullptr;
    r.draft = drafts[row_id];
    r.accepted_out = accepted_out;
    r.row_token_out = row_tokens_out;
    sample_row_max<DT>(sh, r);
    if (r.top_k == 1) {
        if (threadIdx.x == 0) sample_emit<true>(r, r.arg_max, (int64_t)r.draft == r.arg_max);
        return;
    }
    r.top_p = top_ps[row_id];
    r.u_acc = uniforms[2 * (int64_t)row_id];
    r.u = uniforms[2 * (int64_t)row_id + 1];
    sample_row_draw<DT, true>(sh, r, use_candidates);
}

// Sequence stage: one thread per sequence.  n_ok = the leading accepted rows among the first T - 1; the sequence emits
// tok[0 .. n_ok] (the accepted drafts, then the replacement or bonus token): out[b] = [n_ok + 1, tok[0 .. n_ok], -1 ...].
constexpr int kVerifyMaxQ = 8;  // the larger of the two multi-token decodes' query lengths (kGqaMultiMaxQ, kMlaMultiMaxQ)
__global__ __launch_bounds__(256) void verify_sequences_kernel(int64_t* __restrict__ out, int bs, int q_len) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bs) return;
    int64_t* o = out + (int64_t)b * (q_len + 1);
    int64_t v[kVerifyMaxQ];
#pragma unroll
    for (int t = 0; t < kVerifyMaxQ; ++t) v[t] = t < q_len ? o[1 + t] : 0;
    int n_ok = 0;
    bool leading = true;
#pragma unroll
    for (int t = 0; t < kVerifyMaxQ - 1; ++t) {
        leading = leading && t < q_len - 1 && (v[t] & kVerifyAcceptedBit) != 0;
        n_ok += leading ? 1 : 0;
    }
    o[0] = n_ok + 1;
#pragma unroll
    for (int t = 0; t < kVerifyMaxQ; ++t)
        if (t < q_len) o[1 + t] = t <= n_ok ? (v[t] & ~kVerifyAcceptedBit) : (int64_t)-1;
}

// ---------------------------------------------------------------- speculative decoding: verification against a sampled draft
// Row stage of chitu_hip_speculative_verify_sampled (new: no reference counterpart): the draft d of row (b, t) was DRAWN from the
// draft model's distribution q for that position, so the row comes with q's logits, and q is cut under the row's own temperature /
// top_k / top_p exactly as p is (the drafter samples under the request's parameters).  With w_i, S_p the kept integer weights of
// the target row and v_i, S_q those of the draft row, and U(u) = min(floor(u * 2^24), 2^24 - 1):
//     accepted iff U(u_acc) * v_d * S_p < 2^24 * w_d * S_q                  (probability min(1, p(d) / q(d)) on the 2^-24 grid)
//     else token = inverse CDF in index order over r_i = max(0, w_i * S_q - v_i * S_p) at floor(U(u_alt) * R / 2^24), R = sum r_i
// -- the residual max(p - q, 0), renormalised, in integers (p_i - q_i = r_i / (S_p * S_q)).  The products reach 2^125, so the
// arithmetic is unsigned __int128 (multiplies, adds, subtracts, compares and shifts only: no 128-bit division).  Greedy rows, rows
// with S_p == 0 or S_q == 0 and rows without a draft are verify_rows_kernel's.  The specification is tests/spec_verify_sampled_ref.py.
//
// Passes over the pair after the two radix cuts (each wave owns one contiguous segment of the vocabulary, as in the draw):
//   count     ties at either cut per segment, and the draft's entry in both rows -> the acceptance test;
//   residual  (rejected rows only) r_i of the segment summed in 128 bits; a tie's rank among its row's ties in index order decides
//             whether it is kept, hence the count pass first;
//   rescan    the one wave whose segment holds the position walks it with prefix sums and emits the token.
// Every pass loads a lane's four elements of BOTH rows before it uses either.
typedef unsigned __int128 u128;
constexpr int kRuntimeDT = 3;  // load4: both rows' element types are run-time values, so the pair kernel is compiled once

struct VerifyPairShared {
    SampleShared s;
    uint32_t ties_p[kSampleWaves], ties_q[kSampleWaves];    // ties at the row's tau inside the segment
    uint32_t below_p[kSampleWaves], below_q[kSampleWaves];  // of those, the ones below the draft's index
    uint64_t draft_p[kSampleWaves], draft_q[kSampleWaves];  // the draft's entry: its weight above tau, or kDraftIsTie
    uint64_t res_lo[kSampleWaves], res_hi[kSampleWaves];    // the segment's residual sum
};

__device__ __forceinline__ u128 make_u128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | (u128)lo; }
__device__ __forceinline__ u128 shfl_up_u128(u128 v, int off) {
    return make_u128(shfl_up_u64((uint64_t)(v >> 64), off), shfl_up_u64((uint64_t)v, off));
}
__device__ __forceinline__ u128 shfl_xor_u128(u128 v, int off) {
    return make_u128(shfl_xor_u64((uint64_t)(v >> 64), off), shfl_xor_u64((uint64_t)v, off));
}
__device__ __forceinline__ uint64_t shfl_lane_u64(uint64_t v, int l) {
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), l, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, l, 64);
}

// U(u): the uniform on the 2^-24 grid (u * 2^24 is exact in f32; NaN -> 0)
__device__ __forceinline__ uint64_t verify_grid(float u) {
    const float c = __builtin_fminf(__builtin_fmaxf(u, 0.f), 1.f);
    const uint32_t g = (uint32_t)(c * 16777216.0f);
    return g < 16777215u ? g : 16777215u;
}

// The kept weights of a lane's four elements of both rows (0 where the element is not kept or past the row's end), with the
// ranks of the ties: ties_p / ties_q are the ties before this chunk and are advanced past it.  Whole wave.
__device__ __forceinline__ void pair_kept_quad(const SampleRow& rp, const SampleRow& rq, const SampleCut& cp, const SampleCut& cq,
                                               int i0, int seg_end, uint32_t& ties_p, uint32_t& ties_q, uint64_t (&wp)[4],
                                               uint64_t (&wq)[4]) {
    const int lane = threadIdx.x & 63;
    float vp[4] = {0.f, 0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 0;
    if (i0 < seg_end) {
        n = load4<kRuntimeDT>(rp.row, i0, rp.vocab, rp.vec, vp);
        load4<kRuntimeDT>(rq.row, i0, rq.vocab, rq.vec, vq);
    }
    bool tp[4], tq[4];
    uint64_t t_l = 0;  // this lane's ties: p's in the low word, q's in the high word
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ep = sample_e(sample_x(vp[k], rp.temperature, rp.probs_mode), rp.m, rp.probs_mode);
        const float eq = sample_e(sample_x(vq[k], rq.temperature, rq.probs_mode), rq.m, rq.probs_mode);
        const uint32_t kp = __float_as_uint(ep), kq = __float_as_uint(eq);
        tp[k] = k < n && kp == cp.tau;
        tq[k] = k < n && kq == cq.tau;
        wp[k] = (k < n && kp > cp.tau) ? sample_fix(ep) : 0ull;
        wq[k] = (k < n && kq > cq.tau) ? sample_fix(eq) : 0ull;
        t_l += (tp[k] ? 1ull : 0ull) + (tq[k] ? (1ull << 32) : 0ull);
    }
    uint64_t t_incl = t_l;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = shfl_up_u64(t_incl, off);
        if (lane >= off) t_incl += o;
    }
    const uint64_t t_excl = t_incl - t_l;
    uint32_t rank_p = ties_p + (uint32_t)t_excl, rank_q = ties_q + (uint32_t)(t_excl >> 32);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (tp[k]) {
            if (rank_p < cp.c_keep) wp[k] = cp.e_tau;
            ++rank_p;
        }
        if (tq[k]) {
            if (rank_q < cq.c_keep) wq[k] = cq.e_tau;
            ++rank_q;
        }
    }
    const uint64_t t_all = shfl_lane_u64(t_incl, 63);
    ties_p += (uint32_t)t_all;
    ties_q += (uint32_t)(t_all >> 32);
}

__device__ __forceinline__ u128 pair_residual(uint64_t w, uint64_t v, uint64_t s_p, uint64_t s_q) {
    const u128 a = (u128)w * s_q, b = (u128)v * s_p;
    return a > b ? a - b : (u128)0;
}

__global__ __launch_bounds__(kSampleThreads) void verify_sampled_rows_kernel(
    const void* __restrict__ logits, int64_t row_stride, const void* __restrict__ draft_logits, int64_t draft_row_stride, int vocab,
    const float* __restrict__ temperatures, const int32_t* __restrict__ top_ks, const float* __restrict__ top_ps,
    const int32_t* __restrict__ drafts, const float* __restrict__ uniforms, int q_len, int probs_mode, int64_t* __restrict__ out,
    int32_t* __restrict__ accepted_out, int64_t* __restrict__ row_tokens_out, int use_candidates, int dt_p, int dt_q) {
    __shared__ VerifyPairShared vs;
    SampleShared& sh = vs.s;
    const int row_id = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int elem_p = dt_p == 2 ? 4 : 2, elem_q = dt_q == 2 ? 4 : 2;
    SampleRow r = {};
    r.row = reinterpret_cast<const char*>(logits) + (int64_t)row_id * row_stride * elem_p;
    r.vocab = vocab;
    r.vec = ((reinterpret_cast<uintptr_t>(r.row) & (uintptr_t)(4 * elem_p - 1)) == 0 ? 1 : 0) | (dt_p << 1);
    r.top_k = top_ks[row_id];
    r.temperature = probs_mode ? 1.0f : temperatures[row_id];
    r.probs_mode = probs_mode;
    r.row_id = row_id;
    r.token_out = out + (int64_t)(row_id / q_len) * (q_len + 1) + 1 + row_id % q_len;
    r.n_kept_out = nullptr;
    r.kept_mass_out = nullptr;
    r.draft = drafts[row_id];
    r.accepted_out = accepted_out;
    r.row_token_out = row_tokens_out;
    sample_row_max<kRuntimeDT>(sh, r);
    if (r.top_k == 1) {
        if (tid == 0) sample_emit<true>(r, r.arg_max, (int64_t)r.draft == r.arg_max);
        return;
    }
    r.top_p = top_ps[row_id];
    r.u_acc = uniforms[2 * (int64_t)row_id];
    r.u = uniforms[2 * (int64_t)row_id + 1];
    if (r.draft < 0) {  // the bonus row: chitu_hip_sample's row for u_alt; its draft row is never read
        sample_row_draw<kRuntimeDT, true>(sh, r, use_candidates);
        return;
    }
    SampleRow rq = r;
    rq.row = reinterpret_cast<const char*>(draft_logits) + (int64_t)row_id * draft_row_stride * elem_q;
    rq.vec = ((reinterpret_cast<uintptr_t>(rq.row) & (uintptr_t)(4 * elem_q - 1)) == 0 ? 1 : 0) | (dt_q << 1);
    sample_row_max<kRuntimeDT>(sh, rq);
    const SampleCut cp = sample_radix_cut<kRuntimeDT>(sh, r);
    __syncthreads();  // every thread has read the target row's last level
    const SampleCut cq = sample_radix_cut<kRuntimeDT>(sh, rq);
    const uint64_t s_p = cp.s_kept, s_q = cq.s_kept;
    if (s_p == 0 || s_q == 0) {  // a row without positive weight: the greedy rule
        if (tid == 0) sample_emit<true>(r, r.arg_max, (int64_t)r.draft == r.arg_max);
        return;
    }
    const int seg_len = ((vocab + kSampleWaves - 1) / kSampleWaves + 255) / 256 * 256;
    const int seg_begin = min(wave * seg_len, vocab), seg_end = min(seg_begin + seg_len, vocab);

    // ---- count pass
    {
        uint64_t ties = 0, below = 0, dp = 0, dq = 0;  // p's counts in the low words, q's in the high words
        for (int base = seg_begin; base < seg_end; base += 256) {
            const int i0 = base + lane * 4;
            if (i0 < seg_end) {
                float vp[4], vq[4];
                const int n = load4<kRuntimeDT>(r.row, i0, vocab, r.vec, vp);
                load4<kRuntimeDT>(rq.row, i0, vocab, rq.vec, vq);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float ep = sample_e(sample_x(vp[k], r.temperature, probs_mode), r.m, probs_mode);
                    const float eq = sample_e(sample_x(vq[k], rq.temperature, probs_mode), rq.m, probs_mode);
                    const uint32_t kp = __float_as_uint(ep), kq = __float_as_uint(eq);
                    if (k < n) {
                        const uint64_t t = (kp == cp.tau ? 1ull : 0ull) + (kq == cq.tau ? (1ull << 32) : 0ull);
                        ties += t;
                        if (i0 + k < r.draft) below += t;
                        if (i0 + k == r.draft) {
                            dp = kp > cp.tau ? sample_fix(ep) : (kp == cp.tau ? kDraftIsTie : 0ull);
                            dq = kq > cq.tau ? sample_fix(eq) : (kq == cq.tau ? kDraftIsTie : 0ull);
                        }
                    }
                }
            }
        }
        ties = wave_sum_u64(ties);
        below = wave_sum_u64(below);
        dp = wave_sum_u64(dp);  // one lane of one wave at the most holds the draft
        dq = wave_sum_u64(dq);
        if (lane == 0) {
            vs.ties_p[wave] = (uint32_t)ties;
            vs.ties_q[wave] = (uint32_t)(ties >> 32);
            vs.below_p[wave] = (uint32_t)below;
            vs.below_q[wave] = (uint32_t)(below >> 32);
            vs.draft_p[wave] = dp;
            vs.draft_q[wave] = dq;
        }
    }
    __syncthreads();
    uint32_t ties_p = 0, ties_q = 0;  // ties before this wave's segment
    {
        uint64_t ent_p = 0, ent_q = 0;
        uint32_t rank_p = 0, rank_q = 0;
#pragma unroll
        for (int w = 0; w < kSampleWaves; ++w) {
            ent_p += vs.draft_p[w];
            ent_q += vs.draft_q[w];
            rank_p += vs.below_p[w];
            rank_q += vs.below_q[w];
            if (w < wave) {
                ties_p += vs.ties_p[w];
                ties_q += vs.ties_q[w];
            }
        }
        // a tie at tau is kept iff its rank among the row's ties in index order is below c_keep
        const uint64_t w_d = (ent_p & kDraftIsTie) ? (rank_p < cp.c_keep ? cp.e_tau : 0ull) : ent_p;
        const uint64_t v_d = (ent_q & kDraftIsTie) ? (rank_q < cq.c_keep ? cq.e_tau : 0ull) : ent_q;
        // U < 2^24, v_d <= 2^40, S < 2^61 (vocab <= 2^21): both sides are below 2^125
        const u128 lhs = (u128)(verify_grid(r.u_acc) * v_d) * s_p;
        const u128 rhs = ((u128)w_d * s_q) << 24;
        if (lhs < rhs) {
            if (tid == 0) sample_emit<true>(r, (int64_t)r.draft, true);
            return;
        }
    }

    // ---- residual pass
    {
        u128 res = 0;
        uint32_t tp = ties_p, tq = ties_q;
        for (int base = seg_begin; base < seg_end; base += 256) {
            uint64_t wp[4], wq[4];
            pair_kept_quad(r, rq, cp, cq, base + lane * 4, seg_end, tp, tq, wp, wq);
#pragma unroll
            for (int k = 0; k < 4; ++k) res += pair_residual(wp[k], wq[k], s_p, s_q);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) res += shfl_xor_u128(res, off);
        if (lane == 0) {
            vs.res_lo[wave] = (uint64_t)res;
            vs.res_hi[wave] = (uint64_t)(res >> 64);
        }
    }
    __syncthreads();
    u128 total = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) total += make_u128(vs.res_hi[w], vs.res_lo[w]);
    // floor(U * R / 2^24) without a 128-bit division or a product above 2^128
    const uint64_t g = verify_grid(r.u);
    const u128 target = (total >> 24) * g + (((total & (u128)0xffffffu) * g) >> 24);
    int wsel = -1;
    u128 run = 0;
    {
        u128 cum = 0;
#pragma unroll
        for (int w = 0; w < kSampleWaves; ++w) {
            const u128 s = make_u128(vs.res_hi[w], vs.res_lo[w]);
            if (wsel < 0 && target < cum + s) {
                wsel = w;
                run = cum;
            }
            cum += s;
        }
    }
    if (wsel < 0) {  // R == 0: the caller's draft was not drawn from the draft row; keep the launch defined
        if (tid == 0) sample_emit<true>(r, r.arg_max, false);
        return;
    }
    if (wave != wsel) return;

    // ---- rescan by the wave whose segment holds the position
    for (int base = seg_begin; base < seg_end; base += 256) {
        const int i0 = base + lane * 4;
        uint64_t wp[4], wq[4];
        pair_kept_quad(r, rq, cp, cq, i0, seg_end, ties_p, ties_q, wp, wq);
        u128 r4[4], s_l = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r4[k] = pair_residual(wp[k], wq[k], s_p, s_q);
            s_l += r4[k];
        }
        u128 s_incl = s_l;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u128 o = shfl_up_u128(s_incl, off);
            if (lane >= off) s_incl += o;
        }
        const uint64_t hit = __builtin_amdgcn_ballot_w64(run + s_incl > target);
        if (hit) {
            if (lane == __builtin_ctzll(hit)) {
                u128 acc = run + s_incl - s_l;
                int pick = 0;
                bool done = false;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    acc += r4[k];
                    if (!done && acc > target) {
                        pick = k;
                        done = true;
                    }
                }
                sample_emit<true>(r, (int64_t)(i0 + pick), false);
            }
            return;
        }
        run += make_u128(shfl_lane_u64((uint64_t)(s_incl >> 64), 63), shfl_lane_u64((uint64_t)s_incl, 63));
    }
    if (lane == 0) sample_emit<true>(r, r.arg_max, false);  // unreachable: the segment sums add up to R
}

// logits[row, token] -= penalty[row] once per occurrence of `token` in the row's generated tokens
// (executor.py:89-102: index_add_ with duplicates = frequency penalty), rows with penalty <= 0
// untouched (the reference's `> 0` test).  All addends of one address are equal, so the atomic
// order cannot change the result.
__global__ __launch_bounds__(256) void frequency_penalty_kernel(float* __restrict__ logits, int64_t row_stride,
                                                                int vocab, const int32_t* __restrict__ tokens,
                                                                const int32_t* __restrict__ offsets,
                                                                const float* __restrict__ penalties) {
    const int row = blockIdx.x;
    const float p = penalties[row];
    if (!(p > 0.f)) return;
    const int beg = offsets[row], end = offsets[row + 1];
    float* lr = logits + (int64_t)row * row_stride;
    for (int i = beg + threadIdx.x; i < end; i += blockDim.x) {
        const int t = tokens[i];
        if (t >= 0 && t < vocab) atomicAdd(lr + t, -p);
    }
}

}  // namespace chitu

extern "C" int chitu_hip_frequency_penalty(float* logits, int64_t row_stride, int64_t rows, int32_t vocab,
                                           const int32_t* tokens, const int32_t* offsets,
                                           const float* penalties, void* stream) {
    CHITU_REQUIRE(logits && tokens && offsets && penalties && rows >= 0 && vocab > 0 && row_stride >= vocab);
    if (rows == 0) return CHITU_OK;
    hipLaunchKernelGGL(chitu::frequency_penalty_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                       logits, row_stride, (int)vocab, tokens, offsets, penalties);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_sample(const void* logits, int act_dtype, int64_t row_stride, int64_t rows,
                                int32_t vocab, const float* temperatures, const int32_t* top_ks,
                                const float* top_ps, const float* uniforms, int32_t probs_mode,
                                int64_t* out_tokens, int32_t* n_kept_out, float* kept_mass_out,
                                void* stream) {
    CHITU_REQUIRE(logits && out_tokens && rows >= 0 && vocab > 0 && row_stride >= vocab);
    CHITU_REQUIRE(act_dtype >= 0 && act_dtype <= 2);
    CHITU_REQUIRE(probs_mode == 0 || probs_mode == 1);
    // greedy for every row: top_ks == NULL; otherwise all four per-row arrays are required
    if (top_ks != nullptr) CHITU_REQUIRE(top_ps && uniforms && (probs_mode || temperatures));
    if (rows == 0) return CHITU_OK;
    const int use_candidates = chitu::debug_option(chitu::kOptSampleRadix) > 0 ? 0 : 1;  // test / A-B override: radix descent only
#define LAUNCH(DT)                                                                                          \
    hipLaunchKernelGGL(chitu::sample_kernel<DT>, dim3((unsigned)rows), dim3(chitu::kSampleThreads), 0,      \
                       (hipStream_t)stream, logits, row_stride, (int)vocab, temperatures, top_ks, top_ps,   \
                       uniforms, (int)probs_mode, out_tokens, n_kept_out, kept_mass_out, use_candidates)
    if (act_dtype == 0) LAUNCH(0);
    else if (act_dtype == 1) LAUNCH(1);
    else LAUNCH(2);
#undef LAUNCH
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_speculative_verify(const void* logits, int act_dtype, int64_t row_stride, int64_t rows, int32_t vocab,
                                            const float* temperatures, const int32_t* top_ks, const float* top_ps,
                                            const int32_t* drafts, const float* uniforms, int32_t q_len, int32_t probs_mode,
                                            int64_t* out, int32_t* accepted_out, int64_t* row_tokens_out, void* stream) {
    CHITU_REQUIRE(logits && out && rows >= 0 && vocab > 0 && row_stride >= vocab);
    CHITU_REQUIRE(act_dtype >= 0 && act_dtype <= 2);
    CHITU_REQUIRE(probs_mode == 0 || probs_mode == 1);
    CHITU_REQUIRE(top_ks && top_ps && drafts && uniforms && (probs_mode || temperatures));
    CHITU_REQUIRE(q_len >= 2 && q_len <= chitu::kVerifyMaxQ && rows % q_len == 0);
    CHITU_REQUIRE(rows <= 0x7fffffff);
    if (rows == 0) return CHITU_OK;
    const int use_candidates = chitu::debug_option(chitu::kOptSampleRadix) > 0 ? 0 : 1;  // as chitu_hip_sample
#define LAUNCH(DT)                                                                                              \
    hipLaunchKernelGGL(chitu::verify_rows_kernel<DT>, dim3((unsigned)rows), dim3(chitu::kSampleThreads), 0,     \
                       (hipStream_t)stream, logits, row_stride, (int)vocab, temperatures, top_ks, top_ps, drafts, \
                       uniforms, (int)q_len, (int)probs_mode, out, accepted_out, row_tokens_out, use_candidates)
    if (act_dtype == 0) LAUNCH(0);
    else if (act_dtype == 1) LAUNCH(1);
    else LAUNCH(2);
#undef LAUNCH
    // the kernel boundary orders the two stages (a hand-off inside one launch loses to it here: DESIGN 3.9)
    const int bs = (int)(rows / q_len);
    hipLaunchKernelGGL(chitu::verify_sequences_kernel, dim3((unsigned)((bs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, bs,
                       (int)q_len);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_hip_speculative_verify_sampled(const void* logits, int act_dtype, int64_t row_stride, const void* draft_logits,
                                                    int draft_act_dtype, int64_t draft_row_stride, int64_t rows, int32_t vocab,
                                                    const float* temperatures, const int32_t* top_ks, const float* top_ps,
                                                    const int32_t* drafts, const float* uniforms, int32_t q_len, int32_t probs_mode,
                                                    int64_t* out, int32_t* accepted_out, int64_t* row_tokens_out, void* stream) {
    CHITU_REQUIRE(logits && draft_logits && out && rows >= 0 && vocab > 0 && row_stride >= vocab && draft_row_stride >= vocab);
    CHITU_REQUIRE(vocab <= (1 << 21));  // S < 2^61 keeps every product of the rule below 2^128
    CHITU_REQUIRE(act_dtype >= 0 && act_dtype <= 2 && draft_act_dtype >= 0 && draft_act_dtype <= 2);
    CHITU_REQUIRE(probs_mode == 0 || probs_mode == 1);
    CHITU_REQUIRE(top_ks && top_ps && drafts && uniforms && (probs_mode || temperatures));
    CHITU_REQUIRE(q_len >= 2 && q_len <= chitu::kVerifyMaxQ && rows % q_len == 0);
    CHITU_REQUIRE(rows <= 0x7fffffff);
    if (rows == 0) return CHITU_OK;
    const int use_candidates = chitu::debug_option(chitu::kOptSampleRadix) > 0 ? 0 : 1;  // the rows without a draft: as chitu_hip_sample
    hipLaunchKernelGGL(chitu::verify_sampled_rows_kernel, dim3((unsigned)rows), dim3(chitu::kSampleThreads), 0,
                       (hipStream_t)stream, logits, row_stride, draft_logits, draft_row_stride, (int)vocab, temperatures, top_ks,
                       top_ps, drafts, uniforms, (int)q_len, (int)probs_mode, out, accepted_out, row_tokens_out, use_candidates,
                       (int)act_dtype, (int)draft_act_dtype);
    // the sequence stage is chitu_hip_speculative_verify's
    const int bs = (int)(rows / q_len);
    hipLaunchKernelGGL(chitu::verify_sequences_kernel, dim3((unsigned)((bs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, bs,
                       (int)q_len);
    CHITU_RETURN_LAUNCH_STATUS();
}
