// The "QKV post" launches that do something to every head before the rotation, gfx950, head_dim 128 (new: no reference
// counterpart): RoPE on q in place and on k, the rotated k and v written into the token's page row (bf16 or fp8 cache), with
//   HeadNorm  Qwen3's per-head RMSNorm of the q and k heads (chitu_ext_*), or
//   HeadBias  Qwen2's q / k / v projection bias (chitu_ext5_*; the reference adds it inside torch's linear)
// in front.  One decode kernel and one launcher take the policy as a template argument; the two prefill kernels (no cache,
// different argument lists) call the same head functions, so decode and prefill agree bit for bit.
//
// The arithmetic of one head x (128 bf16 channels), each stated in one place:
//   qk_norm_rope_head   weight w (bf16), eps:
//     ss  = sum x_i^2 in fp32 (any order)           rr = rsqrtf(ss / 128.0f + eps)
//     n_i = bf16((x_i * rr) * w_i)                  norm.hip's order and single rounding; then RoPE on n
//   qkv_bias_head       bias chunk b: y_i = bf16_rne(float(x_i) + float(b_i)) -- one fp32 add, one rounding: a bf16 torch.add;
//     q and k heads: RoPE on y; v heads: y itself.  bias is one bf16 row [(hq + 2 hkv) * 128], laid out like a row of qkv.
//     So the decode entries are, bit for bit, chitu_hip_gqa_qkv_post / chitu_hip_gqa_qkv_post_kv_fp8 applied to qkv + bias.
//     This is NOT Hugging Face's single rounding of acc_fp32 + bias: the GEMM in front has already rounded x to bf16.  The
//     second rounding moves a value by at most one bf16 ulp of the sum, inside the model-level bar (2e-2 of the logits' peak)
//     that tests/test_gpu_qwen2.py holds against Hugging Face's fp32 run.
//   rope_head_row16     RoPE on bf16 numbers widened to fp32, as rope_kernel (kv.hip) states it: products rounded separately,
//     r0 = n0 c - n1 s, r1 = n1 c + n0 s, one rounding to bf16.  layout 0: interleaved pairs, 1: half split.
//     With a rotary width R < 128 (chitu_ext7_*, GLM-4: R = 64, layout 0 only) the pairs (2 i, 2 i + 1), i < R / 2, rotate over
//     a cos / sin row of R / 2 floats and the channels R .. 127 are n itself, bit for bit: Hugging Face's
//     modeling_glm.apply_rotary_pos_emb.  Every other entry passes R = 128.
//   fp8 cache: the rotated, bf16-rounded k head and the v head go through gqa_kv_fp8_quant_head (12 zero bytes written).
//
// The lane mapping is gqa_kv_fp8.hip's: one 16-lane DPP row per head, 8 channels per lane, reductions as four row rotations
// on the VALU; a wave takes four heads.  With the half-split layout lane l's rotation partner is lane (l ^ 8)'s prepared
// chunk, fetched by one more row rotation (row_ror:8) per channel instead of a second load and a second norm or add.
#include "gqa_kv_fp8.h"
#include "chitu_hip_ext.h"
#include "chitu_hip_ext5.h"
#include "chitu_hip_ext7.h"

namespace chitu {

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ i32x4 ld_chunk(const bf16_t* p) { return *reinterpret_cast<const i32x4*>(p); }

__device__ __forceinline__ i32x4 f32x8_to_bf16x8(const float (&y)[8]) {  // exact where y holds bf16 numbers
    i32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (int)f32x2_to_bf16x2(y[2 * k], y[2 * k + 1]);
    return o;
}

// The cos / sin values of one lane's channels.  layout 0: lane l owns the pairs 4 l .. 4 l + 3 (c[0..3]); layout 1: its
// channels 8 l + k rotate by entry 8 (l & 7) + k (c[0..7]).  R is the rotary width: the first R channels of a head rotate
// over a cos / sin row of R / 2 floats (cb, sb point at that row), the rest pass through.  R < 128 exists for layout 0 only
// (the entries refuse it otherwise): lane l rotates iff 8 l < R, and a lane that does not loads nothing.
struct QkRot {
    float c[8], s[8];
};

__device__ __forceinline__ QkRot qk_load_rot(int l, const float* __restrict__ cb, const float* __restrict__ sb, int layout, int R) {
    QkRot t;
    const int at = layout == 0 ? 4 * l : 8 * (l & 7);
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, s0 = {0.f, 0.f, 0.f, 0.f};
    if (layout != 0 || 8 * l < R) {
        c0 = *reinterpret_cast<const f32x4*>(cb + at);
        s0 = *reinterpret_cast<const f32x4*>(sb + at);
    }
    f32x4 c1 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    if (layout != 0) {
        c1 = *reinterpret_cast<const f32x4*>(cb + at + 4);
        s1 = *reinterpret_cast<const f32x4*>(sb + at + 4);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) t.c[k] = c0[k], t.s[k] = s0[k], t.c[4 + k] = c1[k], t.s[4 + k] = s1[k];
    return t;
}

// One head = one 16-lane DPP row, all 16 lanes active; n: lane l's channels 8 l .. 8 l + 7 as fp32 values of bf16 numbers.
// Returns the lane's 8 channels as bf16 bits: rotated where 8 l < R, else n itself (layout 0; layout 1 has R = 128, so the
// row rotation below always runs with all 16 lanes).
__device__ __forceinline__ i32x4 rope_head_row16(int l, const float (&n)[8], const QkRot& t, int layout, int R) {
#pragma clang fp contract(off)  // products rounded separately, like rope_kernel / gqa_qkv_post_kernel
    if (layout == 0) {
        if (8 * l >= R) return f32x8_to_bf16x8(n);
        i32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[k] = (int)f32x2_to_bf16x2(n[2 * k] * t.c[k] - n[2 * k + 1] * t.s[k], n[2 * k + 1] * t.c[k] + n[2 * k] * t.s[k]);
        return o;
    }
    float r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float y = dpp_row<0x128>(n[k]);  // row_ror:8 = lane l ^ 8
        // l < 8: n is x0 (channel i), y is x1 (channel i + 64); else the other way round
        r[k] = l < 8 ? n[k] * t.c[k] - y * t.s[k] : n[k] * t.c[k] + y * t.s[k];
    }
    return f32x8_to_bf16x8(r);
}

// lane l's chunk xraw of one head and the same chunk wraw of the weight -> its 8 normalised and rotated channels
__device__ __forceinline__ i32x4 qk_norm_rope_head(int l, const i32x4 xraw, const i32x4 wraw, float eps, const QkRot& t, int layout) {
    // the head norm has no partial width: its entries pass R = 128
#pragma clang fp contract(off)
    float x[8], w[8], n[8];
    bf16x8_to_f32(xraw, x);
    bf16x8_to_f32(wraw, w);
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) ss += x[k] * x[k];
    ss = row16_reduce_sum(ss);  // the same bits in all 16 lanes: every step adds the same two numbers in both of a pair's lanes
    const float rr = rsqrtf(ss / 128.0f + eps);
#pragma unroll
    for (int k = 0; k < 8; ++k) n[k] = round_bf16((x[k] * rr) * w[k]);
    return rope_head_row16(l, n, t, layout, 128);
}

// lane l's 8 channels of one head plus their bias, as fp32 values of bf16 numbers
__device__ __forceinline__ void qkv_bias_head(const i32x4 xraw, const i32x4 braw, float (&y)[8]) {
    float x[8], b[8];
    bf16x8_to_f32(xraw, x);
    bf16x8_to_f32(braw, b);
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = round_bf16(x[k] + b[k]);
}

// What the decode kernel does to a head before the rotation.  A policy is passed to the kernel by value and gives
//   Lane     what a lane holds besides the head's channels; start(l) issues the loads that do not depend on the head,
//            fetch(lane, l, u) those of head u -- called where the loop requests head u's channels, one pass ahead
//   Head     a head prepared ONCE per pass (prepare), from which the loop takes either rotated() bits (q and k heads; the last
//            argument is the rotary width R) or plain() bits (v heads): the bias form computes its sum once, not once per branch
//   operands_nonnull / operands_aligned16: the launcher's checks of the policy's own operands.

// Qwen3's head norm: q and k heads normalised with their own weight [128], v heads copied.  Both weight chunks are loaded
// once per lane, before anything waits.
struct HeadNorm {
    const bf16_t *q_w, *k_w;
    float eps;
    struct Lane {
        i32x4 qw, kw;
    };
    typedef i32x4 Head;
    static constexpr bool kHasWidth = false;  // no entry of this policy takes a rotary width: the full width alone is built
    bool operands_nonnull() const { return q_w && k_w; }
    bool operands_aligned16() const { return aligned16(q_w) && aligned16(k_w); }
    __device__ __forceinline__ Lane start(int l) const { return Lane{ld_chunk(q_w + l * 8), ld_chunk(k_w + l * 8)}; }
    __device__ __forceinline__ void fetch(Lane&, int, int) const {}
    __device__ __forceinline__ void prepare(const Lane&, const i32x4 xraw, Head& h) const { h = xraw; }
    __device__ __forceinline__ i32x4 rotated(int l, const Lane& s, const Head& h, bool is_q, const QkRot& t, int layout, int) const {
        return qk_norm_rope_head(l, h, is_q ? s.qw : s.kw, eps, t, layout);
    }
    __device__ __forceinline__ i32x4 plain(const Head& h) const { return h; }
};

// Qwen2's projection bias: added to q, k and v heads.  One bias chunk per head, requested together with the head's channels.
struct HeadBias {
    const bf16_t* bias;
    struct Lane {
        i32x4 b = {0, 0, 0, 0};
    };
    struct Head {
        float y[8];
    };
    static constexpr bool kHasWidth = true;  // chitu_ext7_*: the partial-width instantiation is built as well
    bool operands_nonnull() const { return bias; }
    bool operands_aligned16() const { return aligned16(bias); }
    __device__ __forceinline__ Lane start(int) const { return Lane{}; }
    __device__ __forceinline__ void fetch(Lane& s, int l, int u) const { s.b = ld_chunk(bias + u * 128 + l * 8); }
    __device__ __forceinline__ void prepare(const Lane& s, const i32x4 xraw, Head& h) const { qkv_bias_head(xraw, s.b, h.y); }
    __device__ __forceinline__ i32x4 rotated(int l, const Lane&, const Head& h, bool, const QkRot& t, int layout, int R) const {
        return rope_head_row16(l, h.y, t, layout, R);
    }
    __device__ __forceinline__ i32x4 plain(const Head& h) const { return f32x8_to_bf16x8(h.y); }
};

// gqa_qkv_post_kernel (kv.hip) / gqa_qkv_post_kv_fp8_kernel (gqa_kv_fp8.hip) with Pre in front of the rotation.
// grid (batch), block 256; qkv row = [hq | hkv | hkv] heads of 128 bf16.  q heads in place; k heads into the token's page row
// (FP8: rounded to bf16 first, then gqa_kv_fp8_quant_head); v heads stored (FP8: quantised).  The range rules are
// paged_token_row's (common.h): where it refuses, nothing is written to the caches and q is still produced.  The length, the
// rotary row, the policy's own loads and the first head's channels are requested before anything waits; the table entry
// needs the length.  Each pass requests the next pass's head (u + 16) before it works on its own.  R: the rotary width; cos /
// sin are [batch, R / 2].  kPartial = false is the full width as a compile-time constant -- every entry but chitu_ext7_*, and
// those at rotary_dim 128: the code the kernel had before it knew a width.  With the width read at run time the full-width
// bias launch measured 0.08 - 0.11 us (3 - 4 %) slower at bs 16 than the build before (profiles/glm4_rope_ab.json);
// the partial instantiation pays that price: 2.87 us at R = 64 against 2.81 us at the full width.
template <class Pre, bool FP8, bool kPartial>
__global__ __launch_bounds__(256) void gqa_qkv_post_row16_kernel(
    bf16_t* __restrict__ qkv, int64_t row_stride, int hq, int hkv, const float* __restrict__ cos, const float* __restrict__ sin,
    int layout, int rotary_dim, const Pre pre, uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache, int64_t num_pages,
    int page_size, const int32_t* __restrict__ table, int pages_per_seq, const int32_t* __restrict__ old_lens) {
    constexpr int64_t kHeadBytes = FP8 ? kGqaKvFp8Row : 256;
    const int R = kPartial ? rotary_dim : 128;
    const int b = blockIdx.x, l = threadIdx.x & 15, nh = hq + 2 * hkv;
    bf16_t* row = qkv + (int64_t)b * row_stride;
    int u = threadIdx.x >> 4;  // uniform per 16-lane row
    const int L = old_lens[b];
    const QkRot rot = qk_load_rot(l, cos + (int64_t)b * (R >> 1), sin + (int64_t)b * (R >> 1), layout, R);
    typename Pre::Lane next_lane = pre.start(l);
    i32x4 next = {0, 0, 0, 0};
    if (u < nh) {
        next = ld_chunk(row + u * 128 + l * 8);
        pre.fetch(next_lane, l, u);
    }
    int64_t off = -1, trow;  // byte offset of the token's row in either cache
    if (paged_token_row(b, L, num_pages, page_size, table, pages_per_seq, trow)) off = trow * (int64_t)hkv * kHeadBytes;
    for (; u < nh; u += 16) {
        const i32x4 xraw = next;
        const typename Pre::Lane lane = next_lane;
        if (u + 16 < nh) {
            next = ld_chunk(row + (u + 16) * 128 + l * 8);
            pre.fetch(next_lane, l, u + 16);
        }
        typename Pre::Head head;
        pre.prepare(lane, xraw, head);
        if (u < hq) {
            *reinterpret_cast<i32x4*>(row + u * 128 + l * 8) = pre.rotated(l, lane, head, true, rot, layout, R);
            continue;
        }
        if (off < 0) continue;
        const bool is_k = u < hq + hkv;
        const i32x4 o = is_k ? pre.rotated(l, lane, head, false, rot, layout, R) : pre.plain(head);
        uint8_t* dst = (is_k ? k_cache : v_cache) + off + (int64_t)(is_k ? u - hq : u - hq - hkv) * kHeadBytes;
        if (FP8) {
            float r[8];
            bf16x8_to_f32(o, r);
            gqa_kv_fp8_quant_head(l, r, dst);
        } else {
            *reinterpret_cast<i32x4*>(dst + l * 16) = o;
        }
    }
}

// The prefill forms: no cache, the whole prompt in one launch.  grid ceil(heads / 16), block 256: 16-lane row r of block i
// takes head 16 i + r.  Head norm: the [rows, hq + hkv] heads of two strided inputs into two strided outputs.
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh, const bf16_t* __restrict__ k, int64_t k_sb, int64_t k_sh,
    bf16_t* __restrict__ oq, int64_t oq_sb, int64_t oq_sh, bf16_t* __restrict__ ok, int64_t ok_sb, int64_t ok_sh,
    const float* __restrict__ cos, const float* __restrict__ sin, int layout, const bf16_t* __restrict__ q_w,
    const bf16_t* __restrict__ k_w, float eps, int64_t heads, int hq, int hkv) {
    const int l = threadIdx.x & 15;
    const int64_t u = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (u >= heads) return;
    const int64_t t = u / (hq + hkv);
    const int h = (int)(u % (hq + hkv));
    const bool is_q = h < hq;
    const bf16_t* src = is_q ? q + t * q_sb + h * q_sh : k + t * k_sb + (h - hq) * k_sh;
    bf16_t* dst = is_q ? oq + t * oq_sb + h * oq_sh : ok + t * ok_sb + (h - hq) * ok_sh;
    const i32x4 xraw = ld_chunk(src + l * 8);
    const i32x4 wraw = ld_chunk((is_q ? q_w : k_w) + l * 8);
    const QkRot rot = qk_load_rot(l, cos + t * 64, sin + t * 64, layout, 128);
    *reinterpret_cast<i32x4*>(dst + l * 8) = qk_norm_rope_head(l, xraw, wraw, eps, rot, layout);
}

// Bias: the [rows, hq + 2 hkv] heads of one merged input -- q, k and v into three contiguous outputs.  cos / sin [rows, R / 2].
template <bool kPartial>
__global__ __launch_bounds__(256) void qkv_bias_rope_kernel(
    const bf16_t* __restrict__ qkv, int64_t sb, int64_t sh, const bf16_t* __restrict__ bias, const float* __restrict__ cos,
    const float* __restrict__ sin, bf16_t* __restrict__ oq, bf16_t* __restrict__ ok, bf16_t* __restrict__ ov, int layout,
    int rotary_dim, int64_t heads, int hq, int hkv) {
    const int R = kPartial ? rotary_dim : 128;
    const int l = threadIdx.x & 15, nh = hq + 2 * hkv;
    const int64_t u = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (u >= heads) return;
    const int64_t t = u / nh;
    const int h = (int)(u % nh);
    const i32x4 xraw = ld_chunk(qkv + t * sb + h * sh + l * 8);
    const i32x4 braw = ld_chunk(bias + h * 128 + l * 8);
    const QkRot rot = qk_load_rot(l, cos + t * (R >> 1), sin + t * (R >> 1), layout, R);
    float y[8];
    qkv_bias_head(xraw, braw, y);
    bf16_t* dst = h < hq         ? oq + (t * hq + h) * 128
                  : h < hq + hkv ? ok + (t * hkv + (h - hq)) * 128
                                 : ov + (t * hkv + (h - hq - hkv)) * 128;
    *reinterpret_cast<i32x4*>(dst + l * 8) = h < hq + hkv ? rope_head_row16(l, y, rot, layout, R) : f32x8_to_bf16x8(y);
}

// RoPE alone (chitu_ext7_rope): the [rows, qh + kh] heads of two strided inputs into two strided outputs, as
// qk_norm_rope_kernel walks them; the first R channels of every head rotate, the rest are copied.
__global__ __launch_bounds__(256) void rope_row16_kernel(
    const bf16_t* __restrict__ q, int64_t q_sb, int64_t q_sh, const bf16_t* __restrict__ k, int64_t k_sb, int64_t k_sh,
    bf16_t* __restrict__ oq, int64_t oq_sb, int64_t oq_sh, bf16_t* __restrict__ ok, int64_t ok_sb, int64_t ok_sh,
    const float* __restrict__ cos, const float* __restrict__ sin, int layout, int R, int64_t heads, int qh, int kh) {
    const int l = threadIdx.x & 15;
    const int64_t u = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (u >= heads) return;
    const int64_t t = u / (qh + kh);
    const int h = (int)(u % (qh + kh));
    const bool is_q = h < qh;
    const bf16_t* src = is_q ? q + t * q_sb + h * q_sh : k + t * k_sb + (h - qh) * k_sh;
    bf16_t* dst = is_q ? oq + t * oq_sb + h * oq_sh : ok + t * ok_sb + (h - qh) * ok_sh;
    const i32x4 xraw = ld_chunk(src + l * 8);
    const QkRot rot = qk_load_rot(l, cos + t * (R >> 1), sin + t * (R >> 1), layout, R);
    float x[8];
    bf16x8_to_f32(xraw, x);
    *reinterpret_cast<i32x4*>(dst + l * 8) = rope_head_row16(l, x, rot, layout, R);
}

// The rotary width of the chitu_ext7_ entries: whole 8-channel lanes and 16-byte aligned rows of R / 2 floats.
static inline bool rotary_dim_ok(int32_t R) { return R >= 8 && R <= 128 && R % 8 == 0; }

// The decode entries: the shared checks in the order every one of them has always made them, the policy's own
// operands checked where the entry's extra pointers used to be.  rotary_dim is 128 for every entry that has no such argument.
template <class Pre, bool FP8>
static int launch_gqa_qkv_post_row16(const Pre pre, void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                     int32_t head_dim, const float* cos, const float* sin, int32_t layout, int32_t rotary_dim,
                                     void* k_cache, void* v_cache, int64_t num_pages, int32_t page_size,
                                     const int32_t* page_table, int32_t pages_per_seq, const int32_t* old_seq_lens, int32_t batch,
                                     void* stream) {
    CHITU_REQUIRE(qkv_bf16 && cos && sin && pre.operands_nonnull() && k_cache && v_cache && page_table && old_seq_lens);
    CHITU_REQUIRE(batch >= 0 && q_heads >= 1 && kv_heads >= 1 && num_pages >= 1 && page_size >= 1);
    CHITU_REQUIRE(pages_per_seq >= 1 && (layout == 0 || layout == 1) && rotary_dim_ok(rotary_dim));
    if (head_dim != 128 || row_stride % 8 != 0 || row_stride < (int64_t)(q_heads + 2 * kv_heads) * head_dim)
        return CHITU_ERR_UNSUPPORTED;
    if (layout == 1 && rotary_dim != 128) return CHITU_ERR_UNSUPPORTED;  // a partial half split has another lane partner
    CHITU_REQUIRE(aligned16(qkv_bf16) && aligned16(k_cache) && aligned16(v_cache));  // 16-byte loads and stores
    CHITU_REQUIRE(aligned16(cos) && aligned16(sin) && pre.operands_aligned16());
    if (batch == 0) return CHITU_OK;
    auto kernel = gqa_qkv_post_row16_kernel<Pre, FP8, false>;
    if constexpr (Pre::kHasWidth) {  // only the bias policy has entries with a width
        if (rotary_dim != 128) kernel = gqa_qkv_post_row16_kernel<Pre, FP8, true>;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv_bf16, row_stride, (int)q_heads,
                       (int)kv_heads, cos, sin, (int)layout, (int)rotary_dim, pre, (uint8_t*)k_cache, (uint8_t*)v_cache, num_pages,
                       (int)page_size, page_table, (int)pages_per_seq, old_seq_lens);
    CHITU_RETURN_LAUNCH_STATUS();
}

// The prefill form of the bias entries (chitu_ext5_qkv_bias_rope: rotary_dim 128; chitu_ext7_qkv_bias_rope).
static int launch_qkv_bias_rope(const void* qkv_bf16, int64_t row_stride, int64_t head_stride, const void* bias_bf16,
                                const float* cos, const float* sin, void* out_q_bf16, void* out_k_bf16, void* out_v_bf16,
                                int64_t rows, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t layout,
                                int32_t rotary_dim, void* stream) {
    CHITU_REQUIRE(qkv_bf16 && bias_bf16 && cos && sin && out_q_bf16 && out_k_bf16 && out_v_bf16);
    CHITU_REQUIRE(rows >= 0 && q_heads >= 1 && kv_heads >= 1 && (layout == 0 || layout == 1) && rotary_dim_ok(rotary_dim));
    if (head_dim != 128) return CHITU_ERR_UNSUPPORTED;
    if (layout == 1 && rotary_dim != 128) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(((row_stride | head_stride) & 7) == 0 && row_stride >= 0 && head_stride >= 0);  // every head 16-byte aligned
    CHITU_REQUIRE(aligned16(qkv_bf16) && aligned16(bias_bf16) && aligned16(cos) && aligned16(sin));
    CHITU_REQUIRE(aligned16(out_q_bf16) && aligned16(out_k_bf16) && aligned16(out_v_bf16));
    const int64_t heads = rows * ((int64_t)q_heads + 2 * (int64_t)kv_heads);
    CHITU_REQUIRE(heads < (1ll << 34));
    if (rows == 0) return CHITU_OK;
    const auto kernel = rotary_dim != 128 ? qkv_bias_rope_kernel<true> : qkv_bias_rope_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((heads + 15) / 16)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv_bf16,
                       row_stride, head_stride, (const bf16_t*)bias_bf16, cos, sin, (bf16_t*)out_q_bf16, (bf16_t*)out_k_bf16,
                       (bf16_t*)out_v_bf16, (int)layout, (int)rotary_dim, heads, (int)q_heads, (int)kv_heads);
    CHITU_RETURN_LAUNCH_STATUS();
}

}  // namespace chitu

extern "C" int chitu_ext_gqa_qkv_norm_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                           int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                           void* k_cache, void* v_cache, int64_t num_pages, int32_t page_size,
                                           const int32_t* page_table, int32_t pages_per_seq, const int32_t* old_seq_lens,
                                           int32_t batch, const void* q_norm_weight_bf16, const void* k_norm_weight_bf16,
                                           float eps, void* stream) {
    using namespace chitu;
    return launch_gqa_qkv_post_row16<HeadNorm, false>(
        HeadNorm{(const bf16_t*)q_norm_weight_bf16, (const bf16_t*)k_norm_weight_bf16, eps}, qkv_bf16, row_stride, q_heads, kv_heads,
        head_dim, cos, sin, layout, 128, k_cache, v_cache, num_pages, page_size, page_table, pages_per_seq, old_seq_lens, batch,
        stream);
}

extern "C" int chitu_ext_gqa_qkv_norm_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                                  int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                                  void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                                  const int32_t* page_table, int32_t pages_per_seq,
                                                  const int32_t* old_seq_lens, int32_t batch, const void* q_norm_weight_bf16,
                                                  const void* k_norm_weight_bf16, float eps, void* stream) {
    using namespace chitu;
    return launch_gqa_qkv_post_row16<HeadNorm, true>(
        HeadNorm{(const bf16_t*)q_norm_weight_bf16, (const bf16_t*)k_norm_weight_bf16, eps}, qkv_bf16, row_stride, q_heads, kv_heads,
        head_dim, cos, sin, layout, 128, k_cache_u8, v_cache_u8, num_pages, page_size, page_table, pages_per_seq, old_seq_lens,
        batch, stream);
}

extern "C" int chitu_ext5_gqa_qkv_bias_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                            int32_t head_dim, const float* cos, const float* sin, int32_t layout, void* k_cache,
                                            void* v_cache, int64_t num_pages, int32_t page_size, const int32_t* page_table,
                                            int32_t pages_per_seq, const int32_t* old_seq_lens, int32_t batch,
                                            const void* bias_bf16, void* stream) {
    using namespace chitu;
    return launch_gqa_qkv_post_row16<HeadBias, false>(HeadBias{(const bf16_t*)bias_bf16}, qkv_bf16, row_stride, q_heads, kv_heads,
                                                      head_dim, cos, sin, layout, 128, k_cache, v_cache, num_pages, page_size,
                                                      page_table, pages_per_seq, old_seq_lens, batch, stream);
}

extern "C" int chitu_ext5_gqa_qkv_bias_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                                   int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                                   void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                                   const int32_t* page_table, int32_t pages_per_seq,
                                                   const int32_t* old_seq_lens, int32_t batch, const void* bias_bf16,
                                                   void* stream) {
    using namespace chitu;
    return launch_gqa_qkv_post_row16<HeadBias, true>(HeadBias{(const bf16_t*)bias_bf16}, qkv_bf16, row_stride, q_heads, kv_heads,
                                                     head_dim, cos, sin, layout, 128, k_cache_u8, v_cache_u8, num_pages, page_size,
                                                     page_table, pages_per_seq, old_seq_lens, batch, stream);
}

extern "C" int chitu_ext_qk_norm_rope(const void* q_bf16, const void* k_bf16, void* out_q_bf16, void* out_k_bf16,
                                      const float* cos, const float* sin, const void* q_norm_weight_bf16,
                                      const void* k_norm_weight_bf16, float eps, int64_t rows, int32_t q_heads, int32_t k_heads,
                                      int32_t head_dim, int64_t q_sb, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t oq_sb,
                                      int64_t oq_sh, int64_t ok_sb, int64_t ok_sh, int32_t layout, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(q_bf16 && k_bf16 && out_q_bf16 && out_k_bf16 && cos && sin && q_norm_weight_bf16 && k_norm_weight_bf16);
    CHITU_REQUIRE(rows >= 0 && q_heads >= 1 && k_heads >= 1 && (layout == 0 || layout == 1));
    if (head_dim != 128) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(((q_sb | q_sh | k_sb | k_sh | oq_sb | oq_sh | ok_sb | ok_sh) & 7) == 0);  // elements: every head 16-byte aligned
    CHITU_REQUIRE(aligned16(q_bf16) && aligned16(k_bf16) && aligned16(out_q_bf16) && aligned16(out_k_bf16));
    CHITU_REQUIRE(aligned16(cos) && aligned16(sin) && aligned16(q_norm_weight_bf16) && aligned16(k_norm_weight_bf16));
    const int64_t heads = rows * (q_heads + k_heads);
    CHITU_REQUIRE(heads < (1ll << 34));
    if (rows == 0) return CHITU_OK;
    hipLaunchKernelGGL(qk_norm_rope_kernel, dim3((unsigned)((heads + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)q_bf16, q_sb, q_sh, (const bf16_t*)k_bf16, k_sb, k_sh, (bf16_t*)out_q_bf16, oq_sb, oq_sh,
                       (bf16_t*)out_k_bf16, ok_sb, ok_sh, cos, sin, (int)layout, (const bf16_t*)q_norm_weight_bf16,
                       (const bf16_t*)k_norm_weight_bf16, eps, heads, (int)q_heads, (int)k_heads);
    CHITU_RETURN_LAUNCH_STATUS();
}

extern "C" int chitu_ext5_qkv_bias_rope(const void* qkv_bf16, int64_t row_stride, int64_t head_stride, const void* bias_bf16,
                                        const float* cos, const float* sin, void* out_q_bf16, void* out_k_bf16, void* out_v_bf16,
                                        int64_t rows, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t layout,
                                        void* stream) {
    return chitu::launch_qkv_bias_rope(qkv_bf16, row_stride, head_stride, bias_bf16, cos, sin, out_q_bf16, out_k_bf16, out_v_bf16, rows,
                                       q_heads, kv_heads, head_dim, layout, 128, stream);
}

// ---- include/chitu_hip_ext7.h: the same launches with a rotary width
extern "C" int chitu_ext7_gqa_qkv_bias_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                            int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                            int32_t rotary_dim, void* k_cache, void* v_cache, int64_t num_pages, int32_t page_size,
                                            const int32_t* page_table, int32_t pages_per_seq, const int32_t* old_seq_lens,
                                            int32_t batch, const void* bias_bf16, void* stream) {
    using namespace chitu;
    return launch_gqa_qkv_post_row16<HeadBias, false>(HeadBias{(const bf16_t*)bias_bf16}, qkv_bf16, row_stride, q_heads, kv_heads,
                                                      head_dim, cos, sin, layout, rotary_dim, k_cache, v_cache, num_pages, page_size,
                                                      page_table, pages_per_seq, old_seq_lens, batch, stream);
}

extern "C" int chitu_ext7_gqa_qkv_bias_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                                   int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                                   int32_t rotary_dim, void* k_cache_u8, void* v_cache_u8, int64_t num_pages,
                                                   int32_t page_size, const int32_t* page_table, int32_t pages_per_seq,
                                                   const int32_t* old_seq_lens, int32_t batch, const void* bias_bf16,
                                                   void* stream) {
    using namespace chitu;
    return launch_gqa_qkv_post_row16<HeadBias, true>(HeadBias{(const bf16_t*)bias_bf16}, qkv_bf16, row_stride, q_heads, kv_heads,
                                                     head_dim, cos, sin, layout, rotary_dim, k_cache_u8, v_cache_u8, num_pages,
                                                     page_size, page_table, pages_per_seq, old_seq_lens, batch, stream);
}

extern "C" int chitu_ext7_qkv_bias_rope(const void* qkv_bf16, int64_t row_stride, int64_t head_stride, const void* bias_bf16,
                                        const float* cos, const float* sin, void* out_q_bf16, void* out_k_bf16, void* out_v_bf16,
                                        int64_t rows, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t layout,
                                        int32_t rotary_dim, void* stream) {
    return chitu::launch_qkv_bias_rope(qkv_bf16, row_stride, head_stride, bias_bf16, cos, sin, out_q_bf16, out_k_bf16, out_v_bf16, rows,
                                       q_heads, kv_heads, head_dim, layout, rotary_dim, stream);
}

extern "C" int chitu_ext7_rope(const void* q, const void* k, void* out_q, void* out_k, const float* cos, const float* sin,
                               int act_dtype, int32_t batch, int32_t q_heads, int32_t k_heads, int32_t head_dim, int64_t q_sb,
                               int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t oq_sb, int64_t oq_sh, int64_t ok_sb, int64_t ok_sh,
                               int32_t layout, int32_t rotary_dim, void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(q && k && out_q && out_k && cos && sin);
    CHITU_REQUIRE(batch >= 0 && q_heads >= 0 && k_heads >= 0 && (layout == 0 || layout == 1) && rotary_dim_ok(rotary_dim));
    if (act_dtype != 0 || head_dim != 128) return CHITU_ERR_UNSUPPORTED;
    if (layout == 1 && rotary_dim != 128) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(((q_sb | q_sh | k_sb | k_sh | oq_sb | oq_sh | ok_sb | ok_sh) & 7) == 0);  // elements: every head 16-byte aligned
    CHITU_REQUIRE(aligned16(q) && aligned16(k) && aligned16(out_q) && aligned16(out_k) && aligned16(cos) && aligned16(sin));
    const int64_t heads = (int64_t)batch * ((int64_t)q_heads + (int64_t)k_heads);
    CHITU_REQUIRE(heads < (1ll << 34));
    if (heads == 0) return CHITU_OK;
    hipLaunchKernelGGL(rope_row16_kernel, dim3((unsigned)((heads + 15) / 16)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q,
                       q_sb, q_sh, (const bf16_t*)k, k_sb, k_sh, (bf16_t*)out_q, oq_sb, oq_sh, (bf16_t*)out_k, ok_sb, ok_sh, cos, sin,
                       (int)layout, (int)rotary_dim, heads, (int)q_heads, (int)k_heads);
    CHITU_RETURN_LAUNCH_STATUS();
}
