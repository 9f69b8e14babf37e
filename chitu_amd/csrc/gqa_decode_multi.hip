// Multi-token GQA / MHA paged decode (head_dim 128): q_len = T <= 8 query tokens per sequence, the `seqlen > 1` half of the
// attn_with_kvcache contract (reference, read-only: chitu/attn_backend.py:92-164; the causal mask is aligned to the bottom right,
// the window formula is the one written there for seqlen_q > 1).  What a speculative-decoding verify step needs.
//
// seqlens[b] = L counts all keys of sequence b, the T appended ones included.  Query token t sits at position L - T + t and sees
// key k iff k <= L - T + t and, with window_left = W >= 0, k >= L - T + t - W: query (b, t) is the single-token decode of a row of
// length L_t = L - T + t + 1 over the same table.  A query with no visible key (L_t <= 0) gives zeros.
//
// The kernel is gqa_decode_kernel of gqa_decode_tile.h with the 16 columns of the MFMA N dimension shared by tpt = 16 / G query
// tokens (G = Hq / Hkv): column j < tpt * G is token tile * tpt + j / G, head kvh * G + j % G; ceil(T / tpt) tiles ride in
// grid.z.  The K / V walk, the LDS slab and the MFMA count per step are that kernel's; a tile walks the 16-token steps from its
// smallest first visible key to its largest L_t (divided among the splits by the same 32-bit arithmetic), V rows outside that
// union are staged as zeros, K re-reads a row inside it, and the score mask is per column.  m_run / l_run are per column as
// they are there; the rescale vote stays wave-wide, and a column that did not ask for it gets alpha = exp(m - max(m, mx)) of
// its own maximum, which is exactly 1 when the step showed it nothing larger.
//
// It is a sibling of that kernel that repeats its body, not a further template parameter of it nor a caller of shared pieces: the
// four existing instantiations had to stay the code they were, and the compiler does not keep them so -- moving that kernel's
// UNCHANGED body into a __device__ __forceinline__ function that the kernel calls already gives its instantiations another
// register allocation and schedule (tried three ways; about 1500 differing lines in gqa_decode.hip's assembly).  The two bodies are
// therefore edited in lockstep, and the T == 1 identity below is the test that holds them together: at T == 1 the columns, the
// walk, the mask and every operation's order are that kernel's: output and workspace are bit-identical to chitu_hip_gqa_decode / _window /
// _kv_fp8 / _kv_fp8_window at the same num_splits.  At T > 1 they are not the expanded single-token launches' bits (the vote
// sees other tokens' columns).  The fp8 form widens codes in registers into the same fragments: bit-identical to the bf16 form
// on the dequantised cache.
#include "gqa_decode_tile.h"

namespace chitu {

constexpr int kGqaMultiMaxQ = 8;

// grid (num_splits, batch * kv_heads, ceil(T / tpt)); block 64.
template <bool kFp8, bool kWin>
__global__ __launch_bounds__(64) void gqa_decode_multi_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_st, int64_t q_sh,
    const std::conditional_t<kFp8, uint8_t, bf16_t>* __restrict__ kc, const std::conditional_t<kFp8, uint8_t, bf16_t>* __restrict__ vc,
    int64_t num_pages, int page_size, int Hkv, const int32_t* __restrict__ table, int table_stride,
    const int32_t* __restrict__ seqlens, float scale, float* __restrict__ part_o, float* __restrict__ part_lse,
    bf16_t* __restrict__ out, int Hq, int T, int num_splits, int window_left, float softcap) {
    constexpr int kRow = kFp8 ? kGqaKvFp8Row : kHd;  // elements (fp8: bytes) of one (token, kv head) row
    __shared__ __attribute__((aligned(16))) uint8_t vlds[16 * kVRowB];
    const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
    const int split = blockIdx.x, b = blockIdx.y / Hkv, kvh = blockIdx.y % Hkv;
    const int G = Hq / Hkv;  // q heads per kv head (<= 16)
    const int tpt = 16 / G;  // query tokens per tile
    const int tok0 = blockIdx.z * tpt, tok1 = min(tok0 + tpt, T) - 1;  // the tile's first and last query token
    const int L = max(seqlens[b], 0);  // a corrupt negative length is an empty sequence, not a huge unsigned range
    // the tile's union range of keys [u0, Lt): from its first query's first visible key up to its last query's position
    // (L - T + tok - W is taken in 64 bits, where it cannot wrap, and clamped before it is narrowed); Lt == 0 gives u0 == 0
    const int Lt = max(L - T + tok1 + 1, 0);
    const int u0 = kWin && window_left >= 0 ? (int)max((int64_t)L - T + tok0 - window_left, (int64_t)0) : 0;
    const int n16 = (Lt + 15) >> 4;
    const int f16 = u0 >> 4;  // u0 < Lt whenever Lt > 0
    // this lane's column: its query token and that query's own visible keys [c0, c1)
    const int jt = j / G, tok = tok0 + jt;
    const bool live = jt < tpt && tok < T;
    const int c1 = live ? max(L - T + tok + 1, 0) : 0;
    const int c0 = kWin && window_left >= 0 ? (int)max((int64_t)L - T + tok - window_left, (int64_t)0) : 0;
    // 32-bit unsigned quotients: a 64-bit division is a software loop on the kernel's critical chain (the launcher bounds
    // 16-token steps x splits below 2^31)
    int s0i = (int)((unsigned)(n16 - f16) * (unsigned)split / (unsigned)num_splits);
    int s1i = (int)((unsigned)(n16 - f16) * (unsigned)(split + 1) / (unsigned)num_splits);
    if constexpr (kWin) s0i += f16, s1i += f16;
    const float cap_inv = kWin && softcap > 0.f ? 1.0f / softcap : 0.f;
    const int32_t* tbl = table + (int64_t)b * table_stride;
    const int64_t tok_stride = (int64_t)Hkv * kRow;

    // Q^T fragments (B operand): lane holds q[token tok][head j % G][kk*32 + g*8 ..], zero for a column without a query
    s16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        qf[kk] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (live) qf[kk] = *reinterpret_cast<const s16x8*>(q + b * q_sb + tok * q_st + (kvh * G + j - jt * G) * q_sh + kk * 32 + g * 8);
    }
    f32x4 o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    // the prefetched step: bf16 rows as they are; fp8 rows as codes (8 per chunk) + scales, widened when they are consumed
    std::conditional_t<kFp8, i32x2, s16x8> kf[4];
    std::conditional_t<kFp8, i32x2, i32x4> vr[4];
    float ks = 1.f, vs[4] = {1.f, 1.f, 1.f, 1.f};
    auto issue = [&](int step) {
        const int t0 = step * 16;
        int64_t page = tbl[t0 / page_size];
        if (page < 0 || page >= num_pages) page = 0;
        const int64_t base = (page * page_size + (t0 % page_size)) * tok_stride + (int64_t)kvh * kRow;
        // rows past the union's end re-read its last row, kWin: rows before it its first row, u0 <= Lt - 1 (masked below)
        const int tk = kWin ? max(min(j, Lt - 1 - t0), u0 - t0) : min(j, Lt - 1 - t0);
        if constexpr (kFp8) {
            const uint8_t* krow = kc + base + (int64_t)max(tk, 0) * tok_stride;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) kf[kk] = *reinterpret_cast<const i32x2*>(krow + kk * 32 + g * 8);
            ks = *reinterpret_cast<const float*>(krow + kGqaKvFp8ScaleOff);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + i * 64, row = c >> 4, col = c & 15;
                // V rows outside the union are staged as zeros (0 * garbage must stay 0): code 0 x scale 1, whatever the bytes hold
                vr[i] = i32x2{0, 0};
                vs[i] = 1.f;
                if (t0 + row < Lt && (!kWin || t0 + row >= u0)) {
                    const uint8_t* vrow = vc + base + (int64_t)row * tok_stride;
                    vr[i] = *reinterpret_cast<const i32x2*>(vrow + col * 8);
                    vs[i] = *reinterpret_cast<const float*>(vrow + kGqaKvFp8ScaleOff);
                }
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                kf[kk] = *reinterpret_cast<const s16x8*>(kc + base + (int64_t)max(tk, 0) * tok_stride + kk * 32 + g * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + i * 64, row = c >> 4, col = c & 15;
                vr[i] = i32x4{0, 0, 0, 0};  // V rows outside the union are staged as zeros (0 * garbage must stay 0)
                if (t0 + row < Lt && (!kWin || t0 + row >= u0))
                    vr[i] = *reinterpret_cast<const i32x4*>(vc + base + (int64_t)row * tok_stride + col * 8);
            }
        }
    };
    if (s0i < s1i) issue(s0i);
    for (int step = s0i; step < s1i; ++step) {
        const int t0 = step * 16;
        s16x8 kcur[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if constexpr (kFp8) kcur[kk] = __builtin_bit_cast(s16x8, kv_fp8_widen8((uint32_t)kf[kk][0], (uint32_t)kf[kk][1], ks));
            else kcur[kk] = kf[kk];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + i * 64;
            i32x4 w;
            if constexpr (kFp8) w = kv_fp8_widen8((uint32_t)vr[i][0], (uint32_t)vr[i][1], vs[i]);
            else w = vr[i];
            *reinterpret_cast<i32x4*>(vlds + (c >> 4) * kVRowB + (c & 15) * 16) = w;
        }
        if (step + 1 < s1i) issue(step + 1);
        // ---- S^T = K Q^T : lane holds S[token t0 + 4g + r][column j]
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kcur[kk], qf[kk], s, 0, 0, 0);
        float sv[4], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = t0 + g * 4 + r;
            if constexpr (kWin) {
                float x = s[r] * scale;
                if (softcap > 0.f) {  // c * tanh(x / c), tanh(y) = 1 - 2 / (1 + e^2y); |y| <= 15 keeps e^2y finite, tanh(15) rounds to 1
                    const float y = __builtin_fminf(__builtin_fmaxf(x * cap_inv, -15.f), 15.f);
                    x = softcap * (1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * y)));
                }
                sv[r] = t >= c0 && t < c1 ? x : -INFINITY;  // the column's own keys
            } else {
                sv[r] = t < c1 ? s[r] * scale : -INFINITY;
            }
            mx = __builtin_fmaxf(mx, sv[r]);
        }
        float al[4] = {1.f, 1.f, 1.f, 1.f};
        const bool rescale = __any(mx > m_run + kGqaDefer);
        if (rescale) {
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = __builtin_fmaxf(m_run, mx);
            const float alpha = m_new == -INFINITY ? 1.f : __expf(m_run - m_new);  // a column the step shows nothing: exp(0)
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r) al[r] = __shfl(alpha, g * 4 + r, 64);
        }
        const float m_safe = m_run == -INFINITY ? 0.f : m_run;
        s16x4g pa;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __expf(sv[r] - m_safe);
            l_run += p;
            pa[r] = (short)f32_to_bf16(p);
        }
        // ---- O += P V : B fragment = 4 token rows at one head-dim column (transpose read)
        const uint8_t* vbase = vlds + (g * 4 + (j >> 2)) * kVRowB + (j & 3) * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const s16x4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4g*)(vbase + c * 32));
            if (rescale) {
#pragma unroll
                for (int r = 0; r < 4; ++r) o[c][r] *= al[r];
            }
            o[c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa, vb, o[c], 0, 0, 0);
        }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    // lane holds O[column 4g+r][dim c*16 + j]; its (m, l) are for column j -> fetch those of columns 4g+r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int cc = g * 4 + r, ct = cc / G, otok = tok0 + ct;
        const float l = __shfl(l_run, cc, 64), m = __shfl(m_run, cc, 64);
        if (ct >= tpt || otok >= T) continue;
        const int64_t row = ((int64_t)b * T + otok) * Hq + kvh * G + (cc - ct * G);  // (b, t, h)
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        if (num_splits == 1) {
#pragma unroll
            for (int c = 0; c < 8; ++c) out[row * kHd + c * 16 + j] = f32_to_bf16(o[c][r] * inv);
        } else {
            float* dst = part_o + (row * num_splits + split) * kHd;
#pragma unroll
            for (int c = 0; c < 8; ++c) dst[c * 16 + j] = o[c][r] * inv;
            if (j == 0) part_lse[row * num_splits + split] = l > 0.f ? m + __logf(l) : -INFINITY;
        }
    }
}

// gqa_decode_launch's argument checks, workspace carve-up and two launches, over batch * q_len output rows.
template <bool kFp8>
static inline int gqa_decode_multi_launch(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_t, int64_t q_stride_h,
                                          const void* k_cache, const void* v_cache, int64_t num_pages, int32_t page_size,
                                          int32_t kv_heads, const int32_t* block_table, int32_t table_stride,
                                          const int32_t* seqlens, float softmax_scale, void* out_bf16, int32_t batch,
                                          int32_t q_len, int32_t q_heads, int32_t head_dim, int32_t num_splits, void* workspace,
                                          int64_t workspace_bytes, int32_t window_left, float softcap, void* stream) {
    using cache_t = std::conditional_t<kFp8, uint8_t, bf16_t>;
    CHITU_REQUIRE(q_bf16 && k_cache && v_cache && block_table && seqlens && out_bf16);
    CHITU_REQUIRE(batch >= 0 && q_heads >= 1 && kv_heads >= 1 && num_pages >= 1 && table_stride >= 1);
    CHITU_REQUIRE(q_heads % kv_heads == 0 && num_splits >= 1 && num_splits <= 256);
    CHITU_REQUIRE(q_len >= 1 && q_len <= kGqaMultiMaxQ);
    CHITU_REQUIRE(window_left >= -1 && softcap >= 0.f);  // (a NaN cap fails the comparison)
    if (head_dim != kHd || q_heads / kv_heads > 16) return CHITU_ERR_UNSUPPORTED;
    if (page_size < 16 || page_size % 16 != 0) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(q_stride_b % 8 == 0 && q_stride_t % 8 == 0 && q_stride_h % 8 == 0);
    // 16-byte fragment loads of q, K and V (fp8: 8-byte code loads; its rows are 9 x 16 bytes, so every row stays aligned)
    CHITU_REQUIRE((((uintptr_t)q_bf16 | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0);
    CHITU_REQUIRE((int64_t)table_stride * (page_size / 16) * (num_splits + 1) < (1ll << 31));  // 32-bit split arithmetic
    if (batch == 0) return CHITU_OK;
    const int64_t rows = (int64_t)batch * q_len * q_heads;
    float* part_o = nullptr;
    float* part_lse = nullptr;
    if (num_splits > 1) {
        const int64_t need = rows * num_splits * (kHd + 1) * 4;
        CHITU_REQUIRE(workspace && workspace_bytes >= need);
        part_o = (float*)workspace;
        part_lse = part_o + rows * num_splits * kHd;
    }
    hipStream_t st = (hipStream_t)stream;
    const int tpt = 16 / (q_heads / kv_heads);
    const dim3 grid((unsigned)num_splits, (unsigned)(batch * kv_heads), (unsigned)((q_len + tpt - 1) / tpt));
#define CHITU_GQA_MULTI_LAUNCH(WIN)                                                                                            \
    hipLaunchKernelGGL((gqa_decode_multi_kernel<kFp8, WIN>), grid, dim3(64), 0, st, (const bf16_t*)q_bf16, q_stride_b,          \
                       q_stride_t, q_stride_h, (const cache_t*)k_cache, (const cache_t*)v_cache, num_pages, (int)page_size,     \
                       (int)kv_heads, block_table, (int)table_stride, seqlens, softmax_scale, part_o, part_lse,                 \
                       (bf16_t*)out_bf16, (int)q_heads, (int)q_len, (int)num_splits, (int)window_left, softcap)
    if (window_left < 0 && softcap == 0.f) CHITU_GQA_MULTI_LAUNCH(false);
    else CHITU_GQA_MULTI_LAUNCH(true);
#undef CHITU_GQA_MULTI_LAUNCH
    if (num_splits > 1) launch_gqa_merge(part_o, part_lse, (bf16_t*)out_bf16, rows, (int)num_splits, st);
    CHITU_RETURN_LAUNCH_STATUS();
}

}  // namespace chitu

extern "C" int chitu_hip_gqa_decode_multi(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_t, int64_t q_stride_h,
                                          const void* k_cache, const void* v_cache, int64_t num_pages, int32_t page_size,
                                          int32_t kv_heads, const int32_t* block_table, int32_t table_stride,
                                          const int32_t* seqlens, float softmax_scale, void* out_bf16, int32_t batch,
                                          int32_t q_len, int32_t q_heads, int32_t head_dim, int32_t num_splits, void* workspace,
                                          int64_t workspace_bytes, int32_t window_left, float softcap, void* stream) {
    return chitu::gqa_decode_multi_launch<false>(q_bf16, q_stride_b, q_stride_t, q_stride_h, k_cache, v_cache, num_pages, page_size,
                                                 kv_heads, block_table, table_stride, seqlens, softmax_scale, out_bf16, batch, q_len,
                                                 q_heads, head_dim, num_splits, workspace, workspace_bytes, window_left, softcap,
                                                 stream);
}

extern "C" int chitu_hip_gqa_decode_multi_kv_fp8(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_t, int64_t q_stride_h,
                                                 const void* k_cache, const void* v_cache, int64_t num_pages, int32_t page_size,
                                                 int32_t kv_heads, const int32_t* block_table, int32_t table_stride,
                                                 const int32_t* seqlens, float softmax_scale, void* out_bf16, int32_t batch,
                                                 int32_t q_len, int32_t q_heads, int32_t head_dim, int32_t num_splits,
                                                 void* workspace, int64_t workspace_bytes, int32_t window_left, float softcap,
                                                 void* stream) {
    return chitu::gqa_decode_multi_launch<true>(q_bf16, q_stride_b, q_stride_t, q_stride_h, k_cache, v_cache, num_pages, page_size,
                                                kv_heads, block_table, table_stride, seqlens, softmax_scale, out_bf16, batch, q_len,
                                                q_heads, head_dim, num_splits, workspace, workspace_bytes, window_left, softcap,
                                                stream);
}
