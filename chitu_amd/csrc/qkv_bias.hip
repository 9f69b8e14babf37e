// The q / k / v projection bias (Qwen2, Qwen2.5, R1-Distill-Qwen) fused with RoPE and the paged K / V append, gfx950,
// head_dim 128 (new: no reference counterpart -- the reference adds the bias inside torch's linear).
//
// bias is one bf16 row [(hq + 2 hkv) * 128], laid out like a row of qkv: this rank's q heads, then k heads, then v heads.
// The arithmetic of one head x (128 bf16 channels) and its bias chunk b -- qkv_bias_head below, the one place that states
// it, so every kernel of this file agrees bit for bit:
//   y_i = bf16_rne(float(x_i) + float(b_i))          one fp32 add, one rounding: a bf16 torch.add
//   q and k heads: RoPE on y widened back to fp32, as rope_kernel (kv.hip) states it (head_rope.h): products rounded
//   separately, one rounding to bf16.  layout 0: interleaved pairs, 1: half split.      v heads: y itself.
//   fp8 cache: the rotated, bf16-rounded k head and the v head y go through gqa_kv_fp8_quant_head (12 zero bytes written).
// So the decode entries are, bit for bit, chitu_hip_gqa_qkv_post / chitu_hip_gqa_qkv_post_kv_fp8 applied to qkv + bias.
// This is NOT Hugging Face's single rounding of acc_fp32 + bias: the GEMM in front has already rounded x to bf16.  The
// second rounding moves a value by at most one bf16 ulp of the sum, inside the model-level bar (2e-2 of the logits' peak)
// that tests/test_gpu_qwen2.py holds against Hugging Face's fp32 run.
//
// The lane mapping is qk_norm.hip's and gqa_kv_fp8.hip's: one 16-lane DPP row per head, 8 channels per lane, a wave takes
// four heads.  With the half-split layout lane l's rotation partner is lane (l ^ 8)'s already biased chunk, fetched by one
// row rotation (row_ror:8) per channel instead of a second load and a second add.
#include "head_rope.h"
#include "chitu_hip_ext5.h"

namespace chitu {

// lane l's 8 channels of one head plus their bias, as fp32 values of bf16 numbers
__device__ __forceinline__ void qkv_bias_head(const i32x4 xraw, const i32x4 braw, float (&y)[8]) {
    float x[8], b[8];
    bf16x8_to_f32(xraw, x);
    bf16x8_to_f32(braw, b);
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = round_bf16(x[k] + b[k]);
}

__device__ __forceinline__ i32x4 f32x8_to_bf16x8(const float (&y)[8]) {  // exact: y holds bf16 numbers
    i32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (int)f32x2_to_bf16x2(y[2 * k], y[2 * k + 1]);
    return o;
}

// gqa_qkv_post_kernel (kv.hip) / gqa_qkv_post_kv_fp8_kernel (gqa_kv_fp8.hip) with the bias in front of the rotation.
// grid (batch), block 256; qkv row = [hq | hkv | hkv] heads of 128 bf16.  q heads in place; k heads into the token's page row
// (FP8: rounded to bf16 first, then gqa_kv_fp8_quant_head); biased v heads stored (FP8: quantised).  The range rules are
// gqa_qkv_post_kernel's: a negative length, a position beyond the table or a table entry outside [0, num_pages) writes
// nothing to the caches, q is still produced.  The length, the rotary row and the first head's channels and bias chunk are
// requested before anything waits; the table entry needs the length.
template <bool FP8>
__global__ __launch_bounds__(256) void gqa_qkv_bias_post_kernel(
    bf16_t* __restrict__ qkv, int64_t row_stride, int hq, int hkv, const float* __restrict__ cos, const float* __restrict__ sin,
    int layout, const bf16_t* __restrict__ bias, uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache, int64_t num_pages,
    int page_size, const int32_t* __restrict__ table, int pages_per_seq, const int32_t* __restrict__ old_lens) {
    constexpr int64_t kHeadBytes = FP8 ? kGqaKvFp8Row : 256;
    const int b = blockIdx.x, l = threadIdx.x & 15, nh = hq + 2 * hkv;
    bf16_t* row = qkv + (int64_t)b * row_stride;
    int u = threadIdx.x >> 4;  // uniform per 16-lane row
    const int L = old_lens[b];
    const QkRot rot = qk_load_rot(l, cos + (int64_t)b * 64, sin + (int64_t)b * 64, layout);
    i32x4 next = {0, 0, 0, 0}, next_b = {0, 0, 0, 0};
    if (u < nh) {
        next = *reinterpret_cast<const i32x4*>(row + u * 128 + l * 8);
        next_b = *reinterpret_cast<const i32x4*>(bias + u * 128 + l * 8);
    }
    int64_t off = -1;  // byte offset of the token's row in either cache
    {
        const int pidx = L / page_size;
        if (L >= 0 && pidx < pages_per_seq) {
            const int64_t page = table[(int64_t)b * pages_per_seq + pidx];
            if (page >= 0 && page < num_pages) off = (page * page_size + (L % page_size)) * (int64_t)hkv * kHeadBytes;
        }
    }
    for (; u < nh; u += 16) {
        const i32x4 xraw = next, braw = next_b;
        if (u + 16 < nh) {
            next = *reinterpret_cast<const i32x4*>(row + (u + 16) * 128 + l * 8);
            next_b = *reinterpret_cast<const i32x4*>(bias + (u + 16) * 128 + l * 8);
        }
        float y[8];
        qkv_bias_head(xraw, braw, y);
        if (u < hq) {
            *reinterpret_cast<i32x4*>(row + u * 128 + l * 8) = rope_head_row16(l, y, rot, layout);
            continue;
        }
        if (off < 0) continue;
        const bool is_k = u < hq + hkv;
        const i32x4 o = is_k ? rope_head_row16(l, y, rot, layout) : f32x8_to_bf16x8(y);
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

// The prefill form: no cache.  grid ceil(rows * (hq + 2 hkv) / 16), block 256: 16-lane row r of block i takes head 16 i + r
// of the [rows, hq + 2 hkv] heads -- the whole prompt in one launch, q, k and v into three contiguous outputs.
__global__ __launch_bounds__(256) void qkv_bias_rope_kernel(
    const bf16_t* __restrict__ qkv, int64_t sb, int64_t sh, const bf16_t* __restrict__ bias, const float* __restrict__ cos,
    const float* __restrict__ sin, bf16_t* __restrict__ oq, bf16_t* __restrict__ ok, bf16_t* __restrict__ ov, int layout,
    int64_t heads, int hq, int hkv) {
    const int l = threadIdx.x & 15, nh = hq + 2 * hkv;
    const int64_t u = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (u >= heads) return;
    const int64_t t = u / nh;
    const int h = (int)(u % nh);
    const i32x4 xraw = *reinterpret_cast<const i32x4*>(qkv + t * sb + h * sh + l * 8);
    const i32x4 braw = *reinterpret_cast<const i32x4*>(bias + h * 128 + l * 8);
    const QkRot rot = qk_load_rot(l, cos + t * 64, sin + t * 64, layout);
    float y[8];
    qkv_bias_head(xraw, braw, y);
    bf16_t* dst = h < hq         ? oq + (t * hq + h) * 128
                  : h < hq + hkv ? ok + (t * hkv + (h - hq)) * 128
                                 : ov + (t * hkv + (h - hq - hkv)) * 128;
    *reinterpret_cast<i32x4*>(dst + l * 8) = h < hq + hkv ? rope_head_row16(l, y, rot, layout) : f32x8_to_bf16x8(y);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool FP8>
static int launch_gqa_qkv_bias_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                                    const float* cos, const float* sin, int32_t layout, const void* bias_bf16, void* k_cache,
                                    void* v_cache, int64_t num_pages, int32_t page_size, const int32_t* page_table,
                                    int32_t pages_per_seq, const int32_t* old_seq_lens, int32_t batch, void* stream) {
    CHITU_REQUIRE(qkv_bf16 && cos && sin && bias_bf16 && k_cache && v_cache && page_table && old_seq_lens);
    CHITU_REQUIRE(batch >= 0 && q_heads >= 1 && kv_heads >= 1 && num_pages >= 1 && page_size >= 1);
    CHITU_REQUIRE(pages_per_seq >= 1 && (layout == 0 || layout == 1));
    if (head_dim != 128 || row_stride % 8 != 0 || row_stride < (int64_t)(q_heads + 2 * kv_heads) * head_dim)
        return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(aligned16(qkv_bf16) && aligned16(k_cache) && aligned16(v_cache));  // 16-byte loads and stores
    CHITU_REQUIRE(aligned16(cos) && aligned16(sin) && aligned16(bias_bf16));
    if (batch == 0) return CHITU_OK;
    hipLaunchKernelGGL(gqa_qkv_bias_post_kernel<FP8>, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv_bf16,
                       row_stride, (int)q_heads, (int)kv_heads, cos, sin, (int)layout, (const bf16_t*)bias_bf16, (uint8_t*)k_cache,
                       (uint8_t*)v_cache, num_pages, (int)page_size, page_table, (int)pages_per_seq, old_seq_lens);
    CHITU_RETURN_LAUNCH_STATUS();
}

}  // namespace chitu

extern "C" int chitu_ext5_gqa_qkv_bias_post(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                            int32_t head_dim, const float* cos, const float* sin, int32_t layout, void* k_cache,
                                            void* v_cache, int64_t num_pages, int32_t page_size, const int32_t* page_table,
                                            int32_t pages_per_seq, const int32_t* old_seq_lens, int32_t batch,
                                            const void* bias_bf16, void* stream) {
    return chitu::launch_gqa_qkv_bias_post<false>(qkv_bf16, row_stride, q_heads, kv_heads, head_dim, cos, sin, layout, bias_bf16,
                                                  k_cache, v_cache, num_pages, page_size, page_table, pages_per_seq, old_seq_lens,
                                                  batch, stream);
}

extern "C" int chitu_ext5_gqa_qkv_bias_post_kv_fp8(void* qkv_bf16, int64_t row_stride, int32_t q_heads, int32_t kv_heads,
                                                   int32_t head_dim, const float* cos, const float* sin, int32_t layout,
                                                   void* k_cache_u8, void* v_cache_u8, int64_t num_pages, int32_t page_size,
                                                   const int32_t* page_table, int32_t pages_per_seq,
                                                   const int32_t* old_seq_lens, int32_t batch, const void* bias_bf16,
                                                   void* stream) {
    return chitu::launch_gqa_qkv_bias_post<true>(qkv_bf16, row_stride, q_heads, kv_heads, head_dim, cos, sin, layout, bias_bf16,
                                                 k_cache_u8, v_cache_u8, num_pages, page_size, page_table, pages_per_seq,
                                                 old_seq_lens, batch, stream);
}

extern "C" int chitu_ext5_qkv_bias_rope(const void* qkv_bf16, int64_t row_stride, int64_t head_stride, const void* bias_bf16,
                                        const float* cos, const float* sin, void* out_q_bf16, void* out_k_bf16, void* out_v_bf16,
                                        int64_t rows, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t layout,
                                        void* stream) {
    using namespace chitu;
    CHITU_REQUIRE(qkv_bf16 && bias_bf16 && cos && sin && out_q_bf16 && out_k_bf16 && out_v_bf16);
    CHITU_REQUIRE(rows >= 0 && q_heads >= 1 && kv_heads >= 1 && (layout == 0 || layout == 1));
    if (head_dim != 128) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(((row_stride | head_stride) & 7) == 0 && row_stride >= 0 && head_stride >= 0);  // every head 16-byte aligned
    CHITU_REQUIRE(aligned16(qkv_bf16) && aligned16(bias_bf16) && aligned16(cos) && aligned16(sin));
    CHITU_REQUIRE(aligned16(out_q_bf16) && aligned16(out_k_bf16) && aligned16(out_v_bf16));
    const int64_t heads = rows * ((int64_t)q_heads + 2 * (int64_t)kv_heads);
    CHITU_REQUIRE(heads < (1ll << 34));
    if (rows == 0) return CHITU_OK;
    hipLaunchKernelGGL(qkv_bias_rope_kernel, dim3((unsigned)((heads + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)qkv_bf16, row_stride, head_stride, (const bf16_t*)bias_bf16, cos, sin, (bf16_t*)out_q_bf16,
                       (bf16_t*)out_k_bf16, (bf16_t*)out_v_bf16, (int)layout, heads, (int)q_heads, (int)kv_heads);
    CHITU_RETURN_LAUNCH_STATUS();
}
