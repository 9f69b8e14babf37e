// Per-head QK-norm (Qwen3) fused with RoPE and the paged K / V append, gfx950, head_dim 128 (new: no reference counterpart).
//
// Qwen3 applies an RMSNorm with a learned [128] weight to every q head and every k head, after the projection and before
// RoPE.  The arithmetic of one head x (128 bf16 channels), weight w (bf16), eps -- qk_norm_rope_head below, the one place
// that states it, so every kernel of this file agrees bit for bit:
//   ss  = sum x_i^2 in fp32 (any order)           rr = rsqrtf(ss / 128.0f + eps)
//   n_i = bf16((x_i * rr) * w_i)                  norm.hip's order and single rounding
//   RoPE on n widened back to fp32, as rope_kernel (kv.hip) states it: products rounded separately,
//   r0 = n0 c - n1 s, r1 = n1 c + n0 s, one rounding to bf16.  layout 0: interleaved pairs, 1: half split.
//
// The lane mapping is gqa_kv_fp8.hip's: one 16-lane DPP row per head, 8 channels per lane, the sum of squares as four row
// rotations on the VALU; a wave takes four heads.  With the half-split layout lane l's rotation partner is lane (l ^ 8)'s
// normalised chunk, fetched by one more row rotation (row_ror:8) per channel instead of a second load and a second norm.
#include "head_rope.h"
#include "chitu_hip_ext.h"

namespace chitu {

// One head = one 16-lane DPP row, all 16 lanes active: lane l holds channels 8 l .. 8 l + 7 (xraw) and their weights (wraw).
// Returns the lane's 8 normalised and rotated channels as bf16 bits.
__device__ __forceinline__ i32x4 qk_norm_rope_head(int l, const i32x4 xraw, const i32x4 wraw, float eps, const QkRot& t, int layout) {
#pragma clang fp contract(off)  // products rounded separately, like rope_kernel / gqa_qkv_post_kernel
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
    return rope_head_row16(l, n, t, layout);
}

// gqa_qkv_post_kernel (kv.hip) / gqa_qkv_post_kv_fp8_kernel (gqa_kv_fp8.hip) with the head norm in front of the rotation.
// grid (batch), block 256; qkv row = [hq | hkv | hkv] heads of 128 bf16.  q heads in place; k heads into the token's page row
// (FP8: rounded to bf16 first, then gqa_kv_fp8_quant_head); v heads copied (FP8: quantised).  The range rules are
// gqa_qkv_post_kernel's: a negative length, a position beyond the table or a table entry outside [0, num_pages) writes
// nothing to the caches, q is still produced.  The length, the rotary row, both weights and the first head's channels are
// requested before anything waits; the table entry needs the length.
template <bool FP8>
__global__ __launch_bounds__(256) void gqa_qkv_norm_post_kernel(
    bf16_t* __restrict__ qkv, int64_t row_stride, int hq, int hkv, const float* __restrict__ cos, const float* __restrict__ sin,
    int layout, const bf16_t* __restrict__ q_w, const bf16_t* __restrict__ k_w, float eps, uint8_t* __restrict__ k_cache,
    uint8_t* __restrict__ v_cache, int64_t num_pages, int page_size, const int32_t* __restrict__ table, int pages_per_seq,
    const int32_t* __restrict__ old_lens) {
    constexpr int64_t kHeadBytes = FP8 ? kGqaKvFp8Row : 256;
    const int b = blockIdx.x, l = threadIdx.x & 15, nh = hq + 2 * hkv;
    bf16_t* row = qkv + (int64_t)b * row_stride;
    int u = threadIdx.x >> 4;  // uniform per 16-lane row
    const int L = old_lens[b];
    const QkRot rot = qk_load_rot(l, cos + (int64_t)b * 64, sin + (int64_t)b * 64, layout);
    const i32x4 qw = *reinterpret_cast<const i32x4*>(q_w + l * 8), kw = *reinterpret_cast<const i32x4*>(k_w + l * 8);
    i32x4 next = {0, 0, 0, 0};
    if (u < nh) next = *reinterpret_cast<const i32x4*>(row + u * 128 + l * 8);
    int64_t off = -1;  // byte offset of the token's row in either cache
    {
        const int pidx = L / page_size;
        if (L >= 0 && pidx < pages_per_seq) {
            const int64_t page = table[(int64_t)b * pages_per_seq + pidx];
            if (page >= 0 && page < num_pages) off = (page * page_size + (L % page_size)) * (int64_t)hkv * kHeadBytes;
        }
    }
    for (; u < nh; u += 16) {
        const i32x4 xraw = next;
        if (u + 16 < nh) next = *reinterpret_cast<const i32x4*>(row + (u + 16) * 128 + l * 8);
        if (u < hq) {
            *reinterpret_cast<i32x4*>(row + u * 128 + l * 8) = qk_norm_rope_head(l, xraw, qw, eps, rot, layout);
            continue;
        }
        if (off < 0) continue;
        const bool is_k = u < hq + hkv;
        const i32x4 o = is_k ? qk_norm_rope_head(l, xraw, kw, eps, rot, layout) : xraw;
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

// The prefill form: no cache.  grid ceil(rows * (hq + hkv) / 16), block 256: 16-lane row r of block i takes head 16 i + r of
// the [rows, hq + hkv] heads -- the whole prompt in one launch.
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
    const i32x4 xraw = *reinterpret_cast<const i32x4*>(src + l * 8);
    const i32x4 wraw = *reinterpret_cast<const i32x4*>((is_q ? q_w : k_w) + l * 8);
    const QkRot rot = qk_load_rot(l, cos + t * 64, sin + t * 64, layout);
    *reinterpret_cast<i32x4*>(dst + l * 8) = qk_norm_rope_head(l, xraw, wraw, eps, rot, layout);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool FP8>
static int launch_gqa_qkv_norm_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                                    const float* cos, const float* sin, int32_t layout, const void* q_norm_w, const void* k_norm_w,
                                    float eps, void* k_cache, void* v_cache, int64_t num_pages, int32_t page_size,
                                    const int32_t* page_table, int32_t pages_per_seq, const int32_t* old_seq_lens, int32_t batch,
                                    void* stream) {
    CHITU_REQUIRE(qkv_bf16 && cos && sin && q_norm_w && k_norm_w && k_cache && v_cache && page_table && old_seq_lens);
    CHITU_REQUIRE(batch >= 0 && q_heads >= 1 && kv_heads >= 1 && num_pages >= 1 && page_size >= 1);
    CHITU_REQUIRE(pages_per_seq >= 1 && (layout == 0 || layout == 1));
    if (head_dim != 128 || row_stride % 8 != 0 || row_stride < (int64_t)(q_heads + 2 * kv_heads) * head_dim)
        return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(aligned16(qkv_bf16) && aligned16(k_cache) && aligned16(v_cache));  // 16-byte loads and stores
    CHITU_REQUIRE(aligned16(cos) && aligned16(sin) && aligned16(q_norm_w) && aligned16(k_norm_w));
    if (batch == 0) return CHITU_OK;
    hipLaunchKernelGGL(gqa_qkv_norm_post_kernel<FP8>, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv_bf16,
                       row_stride, (int)q_heads, (int)kv_heads, cos, sin, (int)layout, (const bf16_t*)q_norm_w,
                       (const bf16_t*)k_norm_w, eps, (uint8_t*)k_cache, (uint8_t*)v_cache, num_pages, (int)page_size, page_table,
                       (int)pages_per_seq, old_seq_lens);
    CHITU_RETURN_LAUNCH_STATUS();
}

}  // namespace chitu

extern "C" int chitu_ext_gqa_qkv_norm_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                           int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                           void* k_cache, void* v_cache, int64_t num_pages, int32_t page_size,
                                           const int32_t* page_table, int32_t pages_per_seq, const int32_t* old_seq_lens,
                                           int32_t batch, const void* q_norm_weight_bf16, const void* k_norm_weight_bf16,
                                           float eps, void* stream) {
    return chitu::launch_gqa_qkv_norm_post<false>(qkv_bf16, row_stride, q_heads, kv_heads, head_dim, cos, sin, layout,
                                                  q_norm_weight_bf16, k_norm_weight_bf16, eps, k_cache, v_cache, num_pages, page_size,
                                                  page_table, pages_per_seq, old_seq_lens, batch, stream);
}

extern "C" int chitu_ext_gqa_qkv_norm_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                                  int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                                  void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                                  const int32_t* page_table, int32_t pages_per_seq,
                                                  const int32_t* old_seq_lens, int32_t batch, const void* q_norm_weight_bf16,
                                                  const void* k_norm_weight_bf16, float eps, void* stream) {
    return chitu::launch_gqa_qkv_norm_post<true>(qkv_bf16, row_stride, q_heads, kv_heads, head_dim, cos, sin, layout,
                                                 q_norm_weight_bf16, k_norm_weight_bf16, eps, k_cache_u8, v_cache_u8, num_pages,
                                                 page_size, page_table, pages_per_seq, old_seq_lens, batch, stream);
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
