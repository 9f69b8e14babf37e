// Log-probabilities of the tokens a decode step emits: logZ of every logits row, the chosen token's log-probability and the
// N <= 20 most likely tokens (the `logprobs` / `top_logprobs` a serving API reports).  New: the reference reports none; the
// library form is torch.log_softmax + torch.topk on [bs, vocab], a full descending sort per step.
//
// sample.hip gives a row to one workgroup, which is right for its 3-level radix descent but would make this job four or five
// dependent passes over a 517 KB row (vocab 129280, fp32) from one CU.  Here a row is cut into slices of 8192 elements, the
// grid is (slices, rows), and a workgroup of 256 threads reads its slice ONCE: 32 values per thread (eight 16-byte loads at
// fp32, four at bf16) plus at most one element of the unaligned head / tail, all requested before the first is looked at.
// Everything a slice contributes comes out of those registers:
//   m_s = max, sum_s = sum exp(x - m_s)       fixed tree: per thread in register order, DPP rows, readlane, four waves in LDS
//   its own top N as (key, ~id) words          N rounds of a workgroup arg-max over the threads' best not-yet-taken value; the
//                                              winner's owner alone rescans its 33 values for its next best.  key is
//                                              ordered_key(x), so one unsigned 64-bit maximum is "larger value, then lower id"
//   x[tokens[r]] if the id lies in the slice   one load by thread 0
// and goes to the row's record in `partials`.  The workgroups of a row count themselves on tickets[r] with the release / ticket /
// acquire hand-off of gate.hip's route_align_tail (partials cross XCDs, whose L2s are not coherent with each other); the last to
// arrive merges:
//   M = max m_s, Z = sum_s sum_s * exp(m_s - M) in SLICE order, logZ = M + log Z   -- independent of who came last
//   the slices' candidates (S * N, 320 at DeepSeek's vocabulary) are ranked by counting: a candidate's position is the number of
//   candidates that beat it, and it is written there if that is < N.  Words are unique (ids are), so the order is exact.
// and sets the ticket back to 0, so neither a second launch nor a graph replay needs a memset.
#include <type_traits>

#include "chitu_hip_ext8.h"
#include "common.h"
#include "ordered_key.h"

namespace chitu {

constexpr int kLpThreads = 256;
constexpr int kLpPerThread = 32;                      // values of the aligned body per thread
constexpr int kLpSlice = kLpThreads * kLpPerThread;   // 8192 elements per workgroup
constexpr int kLpMaxTop = 20;
constexpr int kLpRecHead = 4;                         // words of a slice record before its candidates: m_s, sum_s, token logit, -
constexpr int kLpCandChunk = 512;                     // candidates ranked against per LDS fill

static inline int lp_rec_words(int top_n) { return kLpRecHead + 2 * top_n; }

struct LpArgs {
    const void* logits;
    int64_t row_stride;
    int64_t row0;          // first row of this launch (a launch holds at most 65535 rows)
    int vocab;
    const int64_t* tokens;
    float* token_lp;
    int64_t token_lp_stride;
    int top_n;
    int32_t* top_ids;
    float* top_lp;
    int64_t top_stride;
    uint32_t* tickets;
    uint32_t* partials;
    int rec_words;
};

struct LpShared {
    float mx[4], sm[4], mmx[4];
    uint64_t best[2][4];
    float w[kLpThreads];
    uint64_t cand[kLpCandChunk];
    int last;
};

__device__ __forceinline__ float lp_readlane(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
template <int CTRL>
__device__ __forceinline__ uint64_t lp_dpp_u64(uint64_t v) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, false);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, false);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t lp_max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Workgroup reductions, result in every thread: DPP rotations inside each 16-lane row, the four rows through readlane in lane
// order, the four waves through `red` in wave order.  `red` is not reused before the next barrier of the caller.
__device__ __forceinline__ float lp_block_max(float v, float* red, int lane, int wave) {
    v = row16_reduce_max(v);
    v = __builtin_fmaxf(__builtin_fmaxf(lp_readlane(v, 0), lp_readlane(v, 16)), __builtin_fmaxf(lp_readlane(v, 32), lp_readlane(v, 48)));
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return __builtin_fmaxf(__builtin_fmaxf(red[0], red[1]), __builtin_fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float lp_block_sum(float v, float* red, int lane, int wave) {
    v = row16_reduce_sum(v);
    v = ((lp_readlane(v, 0) + lp_readlane(v, 16)) + lp_readlane(v, 32)) + lp_readlane(v, 48);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ uint64_t lp_wave_max_u64(uint64_t v) {
    v = lp_max_u64(v, lp_dpp_u64<0x128>(v));  // row_ror:8
    v = lp_max_u64(v, lp_dpp_u64<0x124>(v));  // row_ror:4
    v = lp_max_u64(v, lp_dpp_u64<0x122>(v));  // row_ror:2
    v = lp_max_u64(v, lp_dpp_u64<0x121>(v));  // row_ror:1
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    uint64_t r = 0;
#pragma unroll
    for (int l = 0; l < 64; l += 16)
        r = lp_max_u64(r, ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, l) << 32) | (uint32_t)__builtin_amdgcn_readlane(lo, l));
    return r;
}

// The last workgroup of a row: every slice record of the row is visible (the caller's acquire).  rec: the row's S records.
__device__ __forceinline__ void lp_merge(const LpArgs& a, LpShared& sh, const uint32_t* rec, int64_t r, int64_t tk, int S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.top_n, W = a.rec_words;
    // word c of the row's S * N candidates (slice c / N, entry c % N); 0 beyond them
    auto cand = [&](int c) {
        return c < S * N ? reinterpret_cast<const uint64_t*>(rec + (int64_t)(c / N) * W + kLpRecHead)[c % N] : (uint64_t)0;
    };
    uint64_t mine = cand(tid);  // requested now: in flight while logZ is formed
    // ---- logZ.  A record starts with (m_s, sum_s): one 8-byte load
    auto head = [&](int s) { return *reinterpret_cast<const uint64_t*>(rec + (int64_t)s * W); };
    float lm = -INFINITY;
    for (int s = tid; s < S; s += kLpThreads) lm = __builtin_fmaxf(lm, __uint_as_float((uint32_t)head(s)));
    const float M = lp_block_max(lm, sh.mmx, lane, wave);
    float Z = 0.f;
    for (int s0 = 0; s0 < S; s0 += kLpThreads) {
        float w = 0.f;
        if (s0 + tid < S) {
            const uint64_t h = head(s0 + tid);
            const float ms = __uint_as_float((uint32_t)h), ss = __uint_as_float((uint32_t)(h >> 32));
            const float t = ss * expf(ms - M);
            w = ss == 0.f ? 0.f : t;  // (a slice of nothing but -inf: exactly 0, whatever M is)
        }
        __syncthreads();
        sh.w[tid] = w;
        __syncthreads();
        const int n = min(kLpThreads, S - s0);
        for (int i = 0; i < n; ++i) Z += sh.w[i];  // slice order, the same chain in every thread
    }
    const float logZ = M + logf(Z);  // an all -inf row: -inf + log 0 = -inf, and -inf - logZ below is the NaN asked for
    if (tid == 0 && a.token_lp) {
        float lp = __builtin_nanf("");
        if (tk >= 0 && tk < a.vocab)
            lp = __uint_as_float(__hip_atomic_load(rec + (tk / kLpSlice) * W + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) - logZ;
        a.token_lp[r * a.token_lp_stride] = lp;
    }
    // ---- top N: rank every candidate among all S * N by counting (0 words are empty entries)
    const int C = S * N;
    for (int c0 = 0; c0 < C; c0 += kLpThreads) {
        if (c0 > 0) mine = cand(c0 + tid);
        int rank = 0;
        for (int j0 = 0; j0 < C; j0 += kLpCandChunk) {
            const int n = min(kLpCandChunk, C - j0);
            __syncthreads();
            for (int u = tid; u < n; u += kLpThreads) sh.cand[u] = cand(j0 + u);
            __syncthreads();
            if (c0 + wave * 64 < C) {  // (a wave without candidates of its own only fills)
#pragma unroll 8
                for (int i = 0; i < n; ++i) rank += sh.cand[i] > mine ? 1 : 0;
            }
        }
        if (mine != 0 && rank < N) {
            a.top_ids[r * a.top_stride + rank] = (int32_t)~(uint32_t)mine;
            a.top_lp[r * a.top_stride + rank] = ordered_key_inv((uint32_t)(mine >> 32)) - logZ;
        }
    }
    if (tid >= a.vocab && tid < N) {  // fewer tokens than positions
        a.top_ids[r * a.top_stride + tid] = -1;
        a.top_lp[r * a.top_stride + tid] = -INFINITY;
    }
}

template <int DT>  // 0: bf16, 2: fp32 (the C ABI's act_dtype codes)
__global__ __launch_bounds__(kLpThreads) void logprobs_kernel(const LpArgs a) {
    constexpr int A = DT == 2 ? 4 : 8;       // elements per 16 bytes
    constexpr int Q = kLpPerThread / A;      // 16-byte loads per thread
    using elem_t = typename std::conditional<DT == 2, float, uint16_t>::type;
    using vec_t = typename std::conditional<DT == 2, f32x4, i32x4>::type;
    __shared__ LpShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = gridDim.x, s = blockIdx.x, N = a.top_n;
    const int64_t r = a.row0 + blockIdx.y;
    const int64_t tk = a.tokens ? a.tokens[r] : -1;
    const int b = s * kLpSlice, len = min(a.vocab - b, kLpSlice);  // 1 <= len: the grid has ceil(vocab / 8192) slices
    const elem_t* p = reinterpret_cast<const elem_t*>(a.logits) + r * a.row_stride + b;
    // [0, nh) scalar head up to the first 16-byte boundary, nvec whole vectors, nt < A tail elements
    const int mis = (int)((reinterpret_cast<uintptr_t>(p) / sizeof(elem_t)) % A);
    const int nh = min(len, (A - mis) % A);
    const int nvec = (len - nh) / A;
    const int nt = len - nh - nvec * A;

    // ---- every load of the slice, then the first use
    vec_t raw[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if constexpr (DT == 2) raw[q] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        else raw[q] = i32x4{(int)0xff80ff80, (int)0xff80ff80, (int)0xff80ff80, (int)0xff80ff80};
        if (q * kLpThreads + tid < nvec) raw[q] = *reinterpret_cast<const vec_t*>(p + nh + (q * kLpThreads + tid) * A);
    }
    const bool has_extra = tid < nh + nt;
    const int xoff = tid < nh ? tid : nh + nvec * A + (tid - nh);  // < len where has_extra
    elem_t xraw = 0, tok_raw = 0;
    if (has_extra) xraw = p[xoff];
    const bool own_tok = tk >= b && tk < (int64_t)b + len;
    if (tid == 0 && own_tok) tok_raw = p[tk - b];

    float x[kLpPerThread + 1];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if constexpr (DT == 2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) x[q * 4 + k] = raw[q][k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[q * 8 + 2 * k] = __uint_as_float((uint32_t)raw[q][k] << 16);
                x[q * 8 + 2 * k + 1] = __uint_as_float((uint32_t)raw[q][k] & 0xffff0000u);
            }
        }
    }
    auto to_f32 = [](elem_t v) {
        if constexpr (DT == 2) return v;
        else return bf16_to_f32(v);
    };
    x[kLpPerThread] = has_extra ? to_f32(xraw) : -INFINITY;

    // ---- m_s and sum_s
    float tm = x[0];
#pragma unroll
    for (int i = 1; i <= kLpPerThread; ++i) tm = __builtin_fmaxf(tm, x[i]);
    const float m = lp_block_max(tm, sh.mx, lane, wave);
    const float mz = m == -INFINITY ? 0.f : m;  // nothing but -inf here: every term is exp(-inf) = 0, not exp(NaN)
    float ts = 0.f;
#pragma unroll
    for (int i = 0; i <= kLpPerThread; ++i) ts += expf(x[i] - mz);
    const float sum = lp_block_sum(ts, sh.sm, lane, wave);

    // ---- the slice's top N.  Word of an element: ordered_key(x) << 32 | ~id; key 0 (no float has it) marks a slot without one.
    uint64_t mine = 0;
    if (N > 0) {
        uint32_t key[kLpPerThread + 1];
#pragma unroll
        for (int i = 0; i < kLpPerThread; ++i) key[i] = (i / A) * kLpThreads + tid < nvec ? ordered_key(x[i]) : 0u;
        key[kLpPerThread] = has_extra ? ordered_key(x[kLpPerThread]) : 0u;
        const uint32_t nid0 = ~(uint32_t)(b + nh + tid * A);  // ~id of body value i: nid0 - ((i / A) * 256 * A + i % A)
        const uint32_t nidx = ~(uint32_t)(b + xoff);
        // this thread's largest word below `below` (first: of all)
        auto scan = [&](bool first, uint64_t below) {
            uint64_t best = 0;
#pragma unroll
            for (int i = 0; i <= kLpPerThread; ++i) {
                const uint32_t nid = i < kLpPerThread ? nid0 - (uint32_t)((i / A) * kLpThreads * A + i % A) : nidx;
                const uint64_t c = ((uint64_t)key[i] << 32) | nid;
                if ((first || c < below) && c > best) best = c;
            }
            return (best >> 32) != 0 ? best : (uint64_t)0;
        };
        uint64_t local = scan(true, 0);
        for (int n = 0; n < N; ++n) {
            const uint64_t wmax = lp_wave_max_u64(local);
            if (lane == 0) sh.best[n & 1][wave] = wmax;
            __syncthreads();  // (round n + 2 writes this buffer again only after everyone passed round n + 1's barrier)
            const uint64_t win = lp_max_u64(lp_max_u64(sh.best[n & 1][0], sh.best[n & 1][1]), lp_max_u64(sh.best[n & 1][2], sh.best[n & 1][3]));
            if (win == 0) break;  // fewer than N elements in the slice; the same in every thread
            if (tid == n) mine = win;
            if (local == win) local = scan(false, win);  // ids are unique: one thread owns the winner
        }
    }

    // ---- publish, take the ticket (route_align_tail's sequence), the last one merges
    uint32_t* rowrec = a.partials + r * S * a.rec_words;
    uint32_t* rec = rowrec + (int64_t)s * a.rec_words;
    if (tid == 0) {
        rec[0] = __float_as_uint(m);
        rec[1] = __float_as_uint(sum);
        rec[2] = __float_as_uint(to_f32(tok_raw));
    }
    if (tid < N) reinterpret_cast<uint64_t*>(rec + kLpRecHead)[tid] = mine;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's record stores have left the CU
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-back is complete before the ticket
        const uint32_t t = __hip_atomic_fetch_add(a.tickets + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == (uint32_t)S - 1 ? 1 : 0;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(a.tickets + r, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the next launch starts from 0
        }
        sh.last = last;
    }
    __syncthreads();
    if (!sh.last) return;
    lp_merge(a, sh, rowrec, r, tk, S);
}

}  // namespace chitu

using namespace chitu;

extern "C" int chitu_ext8_logprobs_workspace_bytes(int64_t rows, int32_t vocab, int32_t top_n, int64_t* tickets_bytes,
                                                   int64_t* partials_bytes) {
    CHITU_REQUIRE(tickets_bytes && partials_bytes && rows >= 0 && vocab >= 1 && top_n >= 0 && top_n <= kLpMaxTop);
    const int64_t S = ((int64_t)vocab + kLpSlice - 1) / kLpSlice;
    *tickets_bytes = rows * 4;
    *partials_bytes = rows * S * lp_rec_words(top_n) * 4;
    return CHITU_OK;
}

extern "C" int chitu_ext8_logprobs(const void* logits, int act_dtype, int64_t row_stride, int64_t rows, int32_t vocab,
                                   const int64_t* tokens, float* token_logprobs, int64_t token_logprobs_stride, int32_t top_n,
                                   int32_t* top_ids, float* top_logprobs, int64_t top_stride, uint32_t* tickets,
                                   int64_t tickets_bytes, void* partials, int64_t partials_bytes, void* stream) {
    int64_t need_t = 0, need_p = 0;
    const int st = chitu_ext8_logprobs_workspace_bytes(rows, vocab, top_n, &need_t, &need_p);
    if (st != CHITU_OK) return st;
    CHITU_REQUIRE(logits && row_stride >= vocab && (tokens != nullptr) == (token_logprobs != nullptr));
    CHITU_REQUIRE(top_n == 0 || (top_ids && top_logprobs && top_stride >= top_n));
    CHITU_REQUIRE(tickets && partials && tickets_bytes >= need_t && partials_bytes >= need_p);
    CHITU_REQUIRE(((uintptr_t)tickets & 3) == 0 && ((uintptr_t)partials & 7) == 0);
    if (act_dtype != 0 && act_dtype != 2) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(((uintptr_t)logits & (act_dtype == 2 ? 3 : 1)) == 0);
    if (rows == 0) return CHITU_OK;
    const int S = ceil_div_i(vocab, kLpSlice);
    LpArgs a{logits, row_stride, 0, vocab, tokens, token_logprobs, token_logprobs_stride, top_n, top_ids, top_logprobs,
             top_stride, tickets, reinterpret_cast<uint32_t*>(partials), lp_rec_words(top_n)};
    for (int64_t r0 = 0; r0 < rows; r0 += 65535) {  // (the grid's y extent)
        a.row0 = r0;
        const dim3 grid((unsigned)S, (unsigned)(rows - r0 < 65535 ? rows - r0 : 65535));
        if (act_dtype == 2) hipLaunchKernelGGL(logprobs_kernel<2>, grid, dim3(kLpThreads), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(logprobs_kernel<0>, grid, dim3(kLpThreads), 0, (hipStream_t)stream, a);
    }
    CHITU_RETURN_LAUNCH_STATUS();
}
