// The GQA / MHA paged decode kernel (head_dim 128) for both cache formats, and its launcher (gqa_decode.hip states the algorithm).
//
// kFp8 == false: bf16 rows [pages, page, Hkv, 128] -- chitu_hip_gqa_decode, gqa_decode.hip.
// kFp8 == true : byte rows [pages, page, Hkv, 144] of gqa_kv_fp8.h (128 e4m3 codes | one fp32 power-of-two scale | 12 zero bytes)
//                -- chitu_hip_gqa_decode_kv_fp8, gqa_decode_kv_fp8.hip.  A lane loads the 8 codes of each 16-byte bf16 chunk it
//                loads in the bf16 form (same token, same channels: 8 B instead of 16) plus the row's scale, and widens them in
//                registers (kv_fp8_widen8: exact, code * 2^e is a bf16 number) into the SAME A fragments and the SAME V slab
//                image.  Everything from the first MFMA on is one code path, so the output -- and the workspace partials -- are
//                bit-identical to the bf16 kernel on the dequantised cache at the same num_splits.  No LDS pass and no barrier
//                is added; K is widened where the bf16 form copies its prefetched fragments, V where it stores them to the slab.
//
// kWin == true : the sliding-window / soft-capped form of either (chitu_hip_gqa_decode_window, chitu_hip_gqa_decode_kv_fp8_window;
//                the reference's semantics, attn_backend.py:55-69 / RefAttnBackend._attention :294-392).  window_left = W >= 0:
//                the query (position L - 1) sees the keys w0 = max(0, L - 1 - W) .. L - 1.  The wave walks the 16-token steps
//                [w0 >> 4, n16) only, divided among the splits as [0, n16) is without a window; keys below w0 in the first step
//                are masked like the keys past the end (score -inf, V row staged as zeros, K re-reads a row of the window), and a
//                page wholly before the window is never named.  softcap = c > 0: score = c * tanh(scale * q.k / c).  With both
//                neutral the launcher takes the kWin == false kernel, which is the code it was before this form existed.
#pragma once
#include <type_traits>

#include "common.h"
#include "gqa_kv_fp8.h"

namespace chitu {

constexpr int kHd = 128;
constexpr int kVRowB = 272;  // LDS row stride of the V slab (256 B + 16 pad)
constexpr float kGqaDefer = 6.0f;

typedef short s16x4g __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4g;

// grid (num_splits, batch * kv_heads); block 64.
template <bool kFp8, bool kWin = false>
__global__ __launch_bounds__(64) void gqa_decode_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh, const std::conditional_t<kFp8, uint8_t, bf16_t>* __restrict__ kc,
    const std::conditional_t<kFp8, uint8_t, bf16_t>* __restrict__ vc, int64_t num_pages, int page_size, int Hkv,
    const int32_t* __restrict__ table, int table_stride, const int32_t* __restrict__ seqlens, float scale,
    float* __restrict__ part_o, float* __restrict__ part_lse, bf16_t* __restrict__ out, int Hq, int num_splits, int window_left,
    float softcap) {
    constexpr int kRow = kFp8 ? kGqaKvFp8Row : kHd;  // elements (fp8: bytes) of one (token, kv head) row
    __shared__ __attribute__((aligned(16))) uint8_t vlds[16 * kVRowB];
    const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
    const int split = blockIdx.x, b = blockIdx.y / Hkv, kvh = blockIdx.y % Hkv;
    const int G = Hq / Hkv;  // q heads per kv head (<= 16)
    const int L = max(seqlens[b], 0);  // a corrupt negative length is an empty sequence, not a huge unsigned range
    const int n16 = (L + 15) >> 4;
    // 32-bit unsigned quotients: a 64-bit division is a software loop on the kernel's critical chain (the launcher bounds
    // 16-token steps x splits below 2^31)
    // kWin: the first visible key and its step (L - 1 - W cannot wrap: L >= 0, W <= 2^31 - 1); 0 without a window
    const int w0 = kWin && window_left >= 0 ? max(L - 1 - window_left, 0) : 0;
    const int f16 = w0 >> 4;
    int s0i = (int)((unsigned)(n16 - f16) * (unsigned)split / (unsigned)num_splits);
    int s1i = (int)((unsigned)(n16 - f16) * (unsigned)(split + 1) / (unsigned)num_splits);
    if constexpr (kWin) s0i += f16, s1i += f16;
    const float cap_inv = kWin && softcap > 0.f ? 1.0f / softcap : 0.f;
    const int32_t* tbl = table + (int64_t)b * table_stride;
    const int64_t tok_stride = (int64_t)Hkv * kRow;

    // Q^T fragments (B operand): lane holds q[head j][kk*32 + g*8 ..], zero for j >= G
    s16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        qf[kk] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (j < G) qf[kk] = *reinterpret_cast<const s16x8*>(q + b * q_sb + (kvh * G + j) * q_sh + kk * 32 + g * 8);
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
        // rows past the end re-read the last valid row, kWin: rows before the window its first row, w0 <= L - 1 (masked below)
        const int tk = kWin ? max(min(j, L - 1 - t0), w0 - t0) : min(j, L - 1 - t0);
        if constexpr (kFp8) {
            const uint8_t* krow = kc + base + (int64_t)max(tk, 0) * tok_stride;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) kf[kk] = *reinterpret_cast<const i32x2*>(krow + kk * 32 + g * 8);
            ks = *reinterpret_cast<const float*>(krow + kGqaKvFp8ScaleOff);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + i * 64, row = c >> 4, col = c & 15;
                // V rows past the end are staged as zeros (0 * garbage must stay 0): code 0 x scale 1, whatever the bytes hold
                vr[i] = i32x2{0, 0};
                vs[i] = 1.f;
                if (t0 + row < L && (!kWin || t0 + row >= w0)) {  // nor the rows before the window
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
                vr[i] = i32x4{0, 0, 0, 0};  // V rows past the end are staged as zeros (0 * garbage must stay 0)
                if (t0 + row < L && (!kWin || t0 + row >= w0))  // nor the rows before the window
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
        // ---- S^T = K Q^T : lane holds S[token t0 + 4g + r][head j]
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kcur[kk], qf[kk], s, 0, 0, 0);
        float sv[4], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if constexpr (kWin) {
                float x = s[r] * scale;
                if (softcap > 0.f) {  // c * tanh(x / c), tanh(y) = 1 - 2 / (1 + e^2y); |y| <= 15 keeps e^2y finite, tanh(15) rounds to 1
                    const float y = __builtin_fminf(__builtin_fmaxf(x * cap_inv, -15.f), 15.f);
                    x = softcap * (1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * y)));
                }
                const int t = t0 + g * 4 + r;
                sv[r] = t >= w0 && t < L ? x : -INFINITY;
            } else {
                sv[r] = (t0 + g * 4 + r) < L ? s[r] * scale : -INFINITY;
            }
            mx = __builtin_fmaxf(mx, sv[r]);
        }
        float al[4] = {1.f, 1.f, 1.f, 1.f};
        const bool rescale = __any(mx > m_run + kGqaDefer);
        if (rescale) {
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = __builtin_fmaxf(m_run, mx);
            const float alpha = m_new == -INFINITY ? 1.f : __expf(m_run - m_new);
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
    // lane holds O[head 4g+r][dim c*16 + j]; its (m, l) are for head j -> fetch those of heads 4g+r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int hh = g * 4 + r;
        const float l = __shfl(l_run, hh, 64), m = __shfl(m_run, hh, 64);
        if (hh >= G) continue;
        const int h = kvh * G + hh;
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        if (num_splits == 1) {
#pragma unroll
            for (int c = 0; c < 8; ++c) out[((int64_t)b * Hq + h) * kHd + c * 16 + j] = f32_to_bf16(o[c][r] * inv);
        } else {
            float* dst = part_o + (((int64_t)b * Hq + h) * num_splits + split) * kHd;
#pragma unroll
            for (int c = 0; c < 8; ++c) dst[c * 16 + j] = o[c][r] * inv;
            if (j == 0) part_lse[((int64_t)b * Hq + h) * num_splits + split] = l > 0.f ? m + __logf(l) : -INFINITY;
        }
    }
}

// gqa_merge_kernel over `bh` (batch x q head) rows of `num_splits` partials (gqa_decode.hip)
void launch_gqa_merge(const float* part_o, const float* part_lse, bf16_t* out, int64_t bh, int num_splits, hipStream_t st);

// The argument checks, the workspace carve-up and the two launches of chitu_hip_gqa_decode / chitu_hip_gqa_decode_kv_fp8.
// window_left = -1 and softcap = 0 (what the two plain entries pass): the kernel without the window / cap code.
template <bool kFp8>
static inline int gqa_decode_launch(const void* q_bf16, int64_t q_stride_b, int64_t q_stride_h, const void* k_cache,
                                    const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                                    const int32_t* block_table, int32_t table_stride, const int32_t* seqlens,
                                    float softmax_scale, void* out_bf16, int32_t batch, int32_t q_heads, int32_t head_dim,
                                    int32_t num_splits, void* workspace, int64_t workspace_bytes, int32_t window_left,
                                    float softcap, void* stream) {
    using cache_t = std::conditional_t<kFp8, uint8_t, bf16_t>;
    CHITU_REQUIRE(q_bf16 && k_cache && v_cache && block_table && seqlens && out_bf16);
    CHITU_REQUIRE(batch >= 0 && q_heads >= 1 && kv_heads >= 1 && num_pages >= 1 && table_stride >= 1);
    CHITU_REQUIRE(q_heads % kv_heads == 0 && num_splits >= 1 && num_splits <= 256);
    CHITU_REQUIRE(window_left >= -1 && softcap >= 0.f);  // (a NaN cap fails the comparison)
    if (head_dim != kHd || q_heads / kv_heads > 16) return CHITU_ERR_UNSUPPORTED;
    if (page_size < 16 || page_size % 16 != 0) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(q_stride_b % 8 == 0 && q_stride_h % 8 == 0);
    // 16-byte fragment loads of q, K and V (fp8: 8-byte code loads; its rows are 9 x 16 bytes, so every row stays aligned)
    CHITU_REQUIRE((((uintptr_t)q_bf16 | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0);
    CHITU_REQUIRE((int64_t)table_stride * (page_size / 16) * (num_splits + 1) < (1ll << 31));  // 32-bit split arithmetic
    if (batch == 0) return CHITU_OK;
    float* part_o = nullptr;
    float* part_lse = nullptr;
    if (num_splits > 1) {
        const int64_t need = (int64_t)batch * q_heads * num_splits * (kHd + 1) * 4;
        CHITU_REQUIRE(workspace && workspace_bytes >= need);
        part_o = (float*)workspace;
        part_lse = part_o + (int64_t)batch * q_heads * num_splits * kHd;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)num_splits, (unsigned)(batch * kv_heads));
#define CHITU_GQA_DECODE_LAUNCH(WIN)                                                                                          \
    hipLaunchKernelGGL((gqa_decode_kernel<kFp8, WIN>), grid, dim3(64), 0, st, (const bf16_t*)q_bf16, q_stride_b, q_stride_h,   \
                       (const cache_t*)k_cache, (const cache_t*)v_cache, num_pages, (int)page_size, (int)kv_heads, block_table, \
                       (int)table_stride, seqlens, softmax_scale, part_o, part_lse, (bf16_t*)out_bf16, (int)q_heads,           \
                       (int)num_splits, (int)window_left, softcap)
    if (window_left < 0 && softcap == 0.f) CHITU_GQA_DECODE_LAUNCH(false);
    else CHITU_GQA_DECODE_LAUNCH(true);
#undef CHITU_GQA_DECODE_LAUNCH
    if (num_splits > 1) launch_gqa_merge(part_o, part_lse, (bf16_t*)out_bf16, (int64_t)batch * q_heads, (int)num_splits, st);
    CHITU_RETURN_LAUNCH_STATUS();
}

}  // namespace chitu
