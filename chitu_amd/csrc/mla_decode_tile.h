// What the MLA paged decode kernels share (mla_decode.hip: bf16 cache, mla_decode_kv_fp8.hip: fp8 latent cache; each one kernel
// template over kTok = 1 or 2 query tokens per workgroup): the bf16 tile image and its fragment addressing, the tile step (QK^T,
// online softmax, P -> bf16, PV), the split range, the page lookup, Q's addressing, the LDS carve-up, the empty-split publication,
// the epilogue, and the host side (argument checks, workspace, launch).  The two formats differ in how a tile's bytes reach the
// image, and in nothing behind that: the fp8 kernel's output is bit-identical to the bf16 kernel's on the dequantised cache
// because both run this text.
#pragma once
#include "common.h"

namespace chitu {

constexpr int kC = 512;        // kv_lora_rank (latent / V width)
constexpr int kR = 64;         // qk_rope_head_dim
constexpr int kD = kC + kR;    // cached row width (576)
constexpr int kTile = 64;      // KV tokens per tile
constexpr int kPStride = 72;   // P row stride in bf16 elements (64 + 8 pad)
constexpr int kMaxTilesLds = 512;  // page ids cached in LDS per split (32k tokens)

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// LDS image of a tile: [64 rows][1152 B] unpadded, the 16-byte chunk c of row r stored at c ^ swz(r),
// swz(r) = 5 * bit3(r) + 2 * bit1(r).  A DMA piece is 1 KiB of the image, lane-linear (lds_dma.h): image chunk q = 64 n + lane
// -> row q / 72, position q % 72, source chunk (q % 72) ^ swz(row).  Readers: K fragments (ds_read_b128, lane groups
// {0-3,12-15,20-27},...: 16 rows with chunk g or g ^ 1) and V^T fragments (ds_read_b64_tr_b16, 32 lanes = 8 rows x 32 B)
// both land on 16 distinct 16-byte slots of the 256-byte bank row (checked exhaustively for every wave / k step;
// the padded 1184-byte rows of rounds 2-4 left the transpose reads 2-way conflicted).
constexpr int kRowU = kD * 2;            // 1152
constexpr int kTileU = kTile * kRowU;    // 73728
__device__ __forceinline__ int kv_swz(int r) { return ((r >> 3) & 1) * 5 + ((r >> 1) & 1) * 2; }

__device__ __forceinline__ void store16_sc1(void* dst, i32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
}

// fragment addressing inside a tile image (see the layout note above) of lane (j = lane & 15, g = lane >> 4) of a wave
struct MlaFrag {
    int ksw, koff0, koff1, vrow_off, vx[4];
};
__device__ __forceinline__ MlaFrag mla_frag(int wave, int j, int g) {
    MlaFrag f;
    f.ksw = kv_swz(j);                                             // row wave*16 + j: bits 1 and 3 are j's
    f.koff0 = (wave * 16 + j) * kRowU + ((g ^ f.ksw) << 4);        // even k steps; odd ones: chunk ^ 4
    f.koff1 = (wave * 16 + j) * kRowU + (((g ^ f.ksw) ^ 4) << 4);
    const int vsw = (g & 1) * 5 + ((j >> 3) & 1) * 2;              // rows ks*32 + g*8 + (j>>2) (+4): bit 3 = g & 1, bit 1 = j >> 3
    f.vrow_off = (g * 8 + (j >> 2)) * kRowU + wave * 256 + ((((j >> 1) & 1) ^ (vsw & 1)) << 4) + (j & 1) * 8;
#pragma unroll
    for (int k = 0; k < 4; ++k) f.vx[k] = ((2 * k) ^ (vsw & 6)) << 4;
    return f;
}

// Q (16 heads x 576 = 1152 chunks of 16 B) in the tile image's own layout (row = head, chunk c at c ^ swz(row)): chunk c < 1152
__device__ __forceinline__ void mla_q_store(uint8_t* img, int c, i32x4 v) {
    *reinterpret_cast<i32x4*>(img + (c / 72) * kRowU + (((c % 72) ^ kv_swz(c / 72)) << 4)) = v;
}
// ... read back like a K fragment, into the registers of every wave (the A operand never changes).
// lane (j, g): qf[kk] = elements [32 kk + 8 g, +8) of head j
__device__ __forceinline__ void mla_q_frags(s16x8 (&qf)[18], const uint8_t* img, int j, int g) {
    const int ksw0 = kv_swz(j);
#pragma unroll
    for (int kk = 0; kk < 18; ++kk)
        qf[kk] = *reinterpret_cast<const s16x8*>(img + j * kRowU + (kk >> 1) * 128 + (((g + 4 * (kk & 1)) ^ ksw0) << 4));
}

// ---- what a workgroup works on.  kTok = 1: one query token per sequence (q_len 1, row b); kTok = 2: q_len = T <= kMlaMultiMaxQ
// tokens per sequence, two per workgroup.  Q's strides and the query length reach the kernels as structs templated on kTok: the
// one-token forms hold no token stride and no T.
constexpr int kMlaMultiMaxQ = 8;  // cache_manager.MAX_DECODE_Q
template <int kTok>
struct MlaQStride {
    int64_t b, t, h;
};
template <>
struct MlaQStride<1> {
    int64_t b, h;
};
template <int kTok>
struct MlaQLen {
    int T;
};
template <>
struct MlaQLen<1> {};
template <int kTok>
__device__ __forceinline__ int mla_q_len(const MlaQLen<kTok>& ql) {
    if constexpr (kTok == 1) return 1;
    else return ql.T;
}

// blockIdx.z -> (head block, the pair's tokens t0, t1); an odd T's last pair has one token (two == false, t1 == t0)
struct MlaPair {
    int hb, t0, t1;
    bool two;
};
template <int kTok>
__device__ __forceinline__ MlaPair mla_pair_of_block(int z, int T) {
    if constexpr (kTok == 1) return MlaPair{z, 0, 0, false};
    const int pairs = (T + 1) >> 1;
    MlaPair p;
    p.hb = z / pairs;
    p.t0 = 2 * (z % pairs);
    p.two = p.t0 + 1 < T;
    p.t1 = p.two ? p.t0 + 1 : p.t0;
    return p;
}

// Chunk c < 1152 of the Q block (16 heads x 576 = 72 chunks of 16 B per head) of query token t of sequence b; heads past H
// re-read head H - 1
template <int kTok>
__device__ __forceinline__ const bf16_t* mla_q_chunk_src(const bf16_t* q_nope, const MlaQStride<kTok>& qn, const bf16_t* q_pe,
                                                         const MlaQStride<kTok>& qp, int b, int t, int h0, int H, int c) {
    const int row = c / 72, col = c % 72;
    const int h = min(h0 + row, H - 1);
    if constexpr (kTok == 1)
        return col < 64 ? q_nope + b * qn.b + h * qn.h + col * 8 : q_pe + b * qp.b + h * qp.h + (col - 64) * 8;
    else
        return col < 64 ? q_nope + b * qn.b + t * qn.t + h * qn.h + col * 8 : q_pe + b * qp.b + t * qp.t + h * qp.h + (col - 64) * 8;
}

// The tiles [tile0, tile1) of split `split` of a sequence of L keys (32-bit unsigned quotients: the host bounds tiles x splits)
struct MlaSplit {
    int tile0, tile1;
    bool pages_in_lds;  // the split's page ids fit the LDS list
};
__device__ __forceinline__ MlaSplit mla_split_range(int L, int split, int num_splits) {
    const int n_tiles = (L + kTile - 1) / kTile;
    MlaSplit sp;
    sp.tile0 = (int)((unsigned)n_tiles * (unsigned)split / (unsigned)num_splits);
    sp.tile1 = (int)((unsigned)n_tiles * (unsigned)(split + 1) / (unsigned)num_splits);
    sp.pages_in_lds = (sp.tile1 - sp.tile0) <= kMaxTilesLds;
    return sp;
}

// Where the rows of the tile that starts at token t0 lie, given its page id; row_bytes: 1152 (bf16) or 656 (fp8).  (The range test
// is made on the 32-bit id, before it is widened: tested as a 64-bit value it compiles to 64-bit vector compares on the
// seqlens -> table -> page -> request chain.)
__device__ __forceinline__ const uint8_t* mla_page_src(const uint8_t* cache, int row_bytes, int64_t num_pages, int page_size,
                                                       int page_id, int t0) {
    const int64_t page = page_id >= 0 && page_id < num_pages ? page_id : 0;  // corrupt table: stay in bounds
    return cache + (page * page_size + (t0 % page_size)) * (int64_t)row_bytes;
}
// ... of tile `tile` of the split: its page id from the LDS list (from_lds: the caller's rule for when that list may be read)
// or from the table
__device__ __forceinline__ const uint8_t* mla_tile_src(const uint8_t* cache, int row_bytes, int64_t num_pages, int page_size,
                                                       const int32_t* tbl, int max_page_idx, const int* pages_lds, bool from_lds,
                                                       int tile, int tile0) {
    const int t0 = tile * kTile;
    const int page_id = from_lds ? pages_lds[tile - tile0] : tbl[min(t0 / page_size, max_page_idx)];
    return mla_page_src(cache, row_bytes, num_pages, page_size, page_id, t0);
}
// The LDS list: page ids of the split's tiles (none at one tile per split, the short-context shape: no table load, and no wait
// of the compiler's for one -- which, counting in order, would also wait for the tile requested before)
__device__ __forceinline__ void mla_fill_page_list(int* pages_lds, const int32_t* tbl, int max_page_idx, int page_size,
                                                   const MlaSplit& sp, int tid) {
    if (sp.pages_in_lds && sp.tile1 - sp.tile0 > 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (tid + i * 256 < sp.tile1 - sp.tile0)
                pages_lds[tid + i * 256] = tbl[min(((sp.tile0 + tid + i * 256) * kTile) / page_size, max_page_idx)];
    }
}

// Dynamic LDS of a decode workgroup: kTiles bytes of tile images and staging (bf16: two images; fp8: one image and the staging
// buffers), then P [16][kPStride] bf16, the softmax exchange red_max / red_sum [4][16] fp32 and the page list [kMaxTilesLds].
// The kernels' pointers and the host's byte count both come from these offsets.  (Offsets, not pointer members, and the tokens'
// state as plain arrays, not structs: either struct form changed the compiler's register allocation or its schedule of the PV
// reads.)
template <int kTiles>
struct MlaLds {
    static constexpr int kP = kTiles, kRedMax = kP + 16 * kPStride * 2, kRedSum = kRedMax + 64 * 4, kPages = kRedSum + 64 * 4;
    static constexpr int kBytes = kPages + kMaxTilesLds * 4;
};

// One 64-token tile whose image is complete at `kv` and visible to the workgroup: the caller has waited, met and issued what
// it issues.  p_lds [16][kPStride], red_max / red_sum [4][16]: free on entry, in use until the caller's next barrier.
__device__ __forceinline__ void mla_tile_step(const uint8_t* kv, const s16x8 (&qf)[18], const MlaFrag& f, int valid, float scale,
                                              bf16_t* p_lds, float* red_max, float* red_sum, f32x4 (&o)[8], float (&m_run)[4],
                                              float (&l_run)[4], int wave, int j, int g) {
    // ---- S = Q K^T for this wave's 16 tokens (two accumulators: no 18-deep dependent chain)
    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 18; kk += 2) {
        const s16x8 k0 = *reinterpret_cast<const s16x8*>(kv + f.koff0 + (kk >> 1) * 128);
        const s16x8 k1 = *reinterpret_cast<const s16x8*>(kv + f.koff1 + (kk >> 1) * 128);
        s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[kk], k0, s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[kk + 1], k1, s1, 0, 0, 0);
    }
    // lane holds S[head 4g+r][token wave*16+j]
    CHITU_PROBE_MARK(11);
    const bool tok_ok = (wave * 16 + j) < valid;
    float sv[4], mx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sv[r] = tok_ok ? (s0[r] + s1[r]) * scale : -INFINITY;
        mx[r] = row16_reduce_max(sv[r]);
    }
    if (j == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red_max[wave * 16 + g * 4 + r] = mx[r];
    }
    __syncthreads();
    float alpha[4], psum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int hh = g * 4 + r;
        const float mt = __builtin_fmaxf(__builtin_fmaxf(red_max[hh], red_max[16 + hh]),
                                         __builtin_fmaxf(red_max[32 + hh], red_max[48 + hh]));
        const float m_new = __builtin_fmaxf(m_run[r], mt);  // finite: the tile's first token is valid
        alpha[r] = __expf(m_run[r] - m_new);
        m_run[r] = m_new;
        const float p = __expf(sv[r] - m_new);
        psum[r] = row16_reduce_sum(p);
        p_lds[hh * kPStride + wave * 16 + j] = f32_to_bf16(p);
    }
    if (j == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red_sum[wave * 16 + g * 4 + r] = psum[r];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[c][r] *= alpha[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int hh = g * 4 + r;
        l_run[r] = l_run[r] * alpha[r] + (red_sum[hh] + red_sum[16 + hh] + red_sum[32 + hh] + red_sum[48 + hh]);
    }

    // ---- O += P V : this wave owns latent columns [wave*128, wave*128+128)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const s16x8 pfrag = *reinterpret_cast<const s16x8*>(p_lds + j * kPStride + ks * 32 + g * 8);
        const uint8_t* vbase = kv + f.vrow_off + ks * 32 * kRowU;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint8_t* va = vbase + f.vx[c & 3] + (c >> 2) * 128;
            const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va));
            const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(va + 4 * kRowU));
            s16x8 vf;
            vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
            vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
            o[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pfrag, vf, o[c], 0, 0, 0);
        }
    }
}

// an empty split publishes LSE = -inf and zero rows (nothing of it is read by the merge); one split: the output rows are zero
__device__ __forceinline__ void mla_publish_empty_split(bf16_t* part_o, float* part_lse, bf16_t* out, int b, int H, int h0, int split,
                                                        int num_splits, int tid) {
    if (num_splits > 1) {
        if (tid < 16 && h0 + tid < H) part_lse[((int64_t)b * H + h0 + tid) * num_splits + split] = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int chunk = tid + i * 256, hr = chunk >> 6, c8 = chunk & 63;
            if (h0 + hr < H)
                *reinterpret_cast<i32x4*>(part_o + (((int64_t)b * H + h0 + hr) * num_splits + split) * kC + c8 * 8) = i32x4{0, 0, 0, 0};
        }
    } else {
        for (int i = tid; i < 16 * kC / 8; i += 256)
            if (h0 + (i >> 6) < H) *reinterpret_cast<i32x4*>(out + ((int64_t)b * H + h0 + (i >> 6)) * kC + (i & 63) * 8) = i32x4{0, 0, 0, 0};
    }
}

// ---- epilogue: lane holds O[head 4g+r][col wave*128 + c*16 + j]; inv[r]: what row r is normalised by.  One split: the rows of out
__device__ __forceinline__ void mla_store_out_rows(bf16_t* out, const f32x4 (&o)[8], const float (&inv)[4], int b, int H, int h0,
                                                   int wave, int j, int g) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int h = h0 + g * 4 + r;
        if (h >= H) continue;
        bf16_t* dst = out + ((int64_t)b * H + h) * kC + wave * 128 + j;
#pragma unroll
        for (int c = 0; c < 8; ++c) dst[c * 16] = f32_to_bf16(o[c][r] * inv[r]);
    }
}
// split partials: transposed through o_lds ([16][512] bf16 = 16 KB of the dead tile image) so every thread stores 16-B pieces
// of whole rows; they leave as BF16 (the normalised o of a split is an attention output: the merge's convex combination keeps
// the 2^-9 rounding below the final output's own) in the workspace layout mla_merge_kernel and mla_merge_uv_quant_kernel read
__device__ __forceinline__ void mla_store_partial_rows(bf16_t* part_o, bf16_t* o_lds, const f32x4 (&o)[8], const float (&inv)[4], int b,
                                                       int H, int h0, int split, int num_splits, int tid, int wave, int j, int g) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) o_lds[(g * 4 + r) * kC + wave * 128 + c * 16 + j] = f32_to_bf16(o[c][r] * inv[r]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int chunk = tid + i * 256;
        const int hr = chunk >> 6, c8 = chunk & 63;
        if (h0 + hr < H) {
            const i32x4 v = *reinterpret_cast<const i32x4*>(o_lds + hr * kC + c8 * 8);
            // write-through (sc1): partials left DIRTY in the L2s would be flushed by the end-of-kernel release, in
            // front of the launch that reads them back; streamed out here they overlap the other workgroups
            store16_sc1(part_o + (((int64_t)b * H + h0 + hr) * num_splits + split) * kC + c8 * 8, v);
        }
    }
}

// ---- kTok = 2: everything above is used as it is -- a staged tile is multiplied once per token of the pair by mla_tile_step with
// that token's own state, so a token's arithmetic and its order are the one-token kernels'.

// What a query token keeps across the tiles -- its Q fragments qf[18] (the A operand), accumulators o[8] and running max / sum
// m_run[4], l_run[4] -- lives in the kernels as arrays over the workgroup's kTok tokens.
//
// One staged tile, once per token of the pair: token k sees L_k keys, valid_k = min(64, L_k - tile * 64) of this tile's; a token
// with none skips the step (the condition is workgroup-uniform: the barriers inside the step stay matched).  The exchange areas
// are in use until a barrier, hence the one between the two steps.
__device__ __forceinline__ void mla_pair_tile_steps(const uint8_t* kv, const MlaFrag& f, int tile, int L0, int L1, float scale,
                                                    bf16_t* p_lds, float* red_max, float* red_sum, const s16x8 (&qf)[2][18],
                                                    f32x4 (&o)[2][8], float (&m_run)[2][4], float (&l_run)[2][4], int wave, int j,
                                                    int g) {
    const int valid0 = min(kTile, L0 - tile * kTile), valid1 = min(kTile, L1 - tile * kTile);
    if (valid0 > 0) mla_tile_step(kv, qf[0], f, valid0, scale, p_lds, red_max, red_sum, o[0], m_run[0], l_run[0], wave, j, g);
    if (valid1 > 0) {
        if (valid0 > 0) __syncthreads();
        mla_tile_step(kv, qf[1], f, valid1, scale, p_lds, red_max, red_sum, o[1], m_run[1], l_run[1], wave, j, g);
    }
}

// A token's epilogue, `row` = b * T + t: the single-token kernels' (1 / l_run, LSE = m_run + log l_run) where the token saw a
// key in this split; where it saw none (l_run == 0), zero rows and LSE = -inf, what mla_publish_empty_split writes.
__device__ __forceinline__ void mla_token_epilogue(const f32x4 (&o)[8], const float (&m_run)[4], const float (&l_run)[4], bf16_t* part_o,
                                                   float* part_lse, bf16_t* out, bf16_t* o_lds, int row, int H, int h0, int split,
                                                   int num_splits, int tid, int wave, int j, int g) {
    float inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) inv[r] = l_run[r] > 0.f ? 1.0f / l_run[r] : 0.f;
    if (num_splits == 1) {
        mla_store_out_rows(out, o, inv, row, H, h0, wave, j, g);
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int h = h0 + g * 4 + r;
        if (wave == 0 && j == 0 && h < H)
            part_lse[((int64_t)row * H + h) * num_splits + split] = l_run[r] > 0.f ? m_run[r] + __logf(l_run[r]) : -INFINITY;
    }
    mla_store_partial_rows(part_o, o_lds, o, inv, row, H, h0, split, num_splits, tid, wave, j, g);
}

// ---- host side of the five decode entries (chitu_hip_mla_decode, _merge_uv_quant_fp8, _multi: mla_decode.hip; _kv_fp8, _multi_kv_fp8:
// mla_decode_kv_fp8.hip)
// Stage 2 (mla_decode.hip: a kernel is launched from the translation unit that defines it)
void launch_mla_merge(const bf16_t* part_o, const float* part_lse, bf16_t* out, int64_t rows, int num_splits, hipStream_t st);

// The argument checks the entries share, in the order their return codes depend on; min_splits: 1, or 2 where one split is
// another entry's business.  An entry's own BAD_ARG checks come before this call, what it refuses as UNSUPPORTED behind it.
static inline int mla_decode_check_args(const void* q_nope, const void* q_pe, const void* kv_cache, const int32_t* block_table,
                                        const int32_t* seqlens, int32_t batch, int32_t heads, int64_t num_pages, int32_t page_size,
                                        int32_t table_stride, int32_t kv_lora_rank, int32_t rope_dim, int32_t num_splits,
                                        int32_t min_splits) {
    CHITU_REQUIRE(q_nope && q_pe && kv_cache && block_table && seqlens);
    CHITU_REQUIRE(batch >= 0 && heads >= 1 && num_pages >= 1 && table_stride >= 1);
    CHITU_REQUIRE(((uintptr_t)kv_cache & 15) == 0 && ((uintptr_t)q_nope & 15) == 0 && ((uintptr_t)q_pe & 15) == 0);  // 16-byte loads
    if (kv_lora_rank != kC || rope_dim != kR) return CHITU_ERR_UNSUPPORTED;
    if (page_size < kTile || page_size % kTile != 0) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE(num_splits >= min_splits && num_splits <= 256);
    // the kernel's split arithmetic is 32-bit: tiles the table can address x (splits + 1) must stay below 2^31
    CHITU_REQUIRE((int64_t)table_stride * (page_size / kTile) * (num_splits + 1) < (1ll << 31));
    return CHITU_OK;
}
// workspace (num_splits > 1, batch > 0): bf16 partial rows [batch, heads, splits, 512] | fp32 LSE [batch, heads, splits]
static inline int mla_decode_carve_workspace(void* workspace, int64_t workspace_bytes, int32_t rows, int32_t heads, int32_t num_splits,
                                             bf16_t** part_o, float** part_lse) {
    const int64_t need = (int64_t)rows * heads * num_splits * (kC * 2 + 4);
    CHITU_REQUIRE(workspace && workspace_bytes >= need);
    *part_o = (bf16_t*)workspace;
    *part_lse = (float*)(*part_o + (int64_t)rows * heads * num_splits * kC);
    return CHITU_OK;
}

// the multi-token entries' argument checks: their own BAD_ARG checks, then the shared ones
static inline int mla_decode_multi_check_args(const void* q_nope, const void* q_pe, const void* kv_cache, const int32_t* block_table,
                                              const int32_t* seqlens, int32_t batch, int32_t q_len, int32_t heads, int64_t num_pages,
                                              int32_t page_size, int32_t table_stride, int32_t kv_lora_rank, int32_t rope_dim,
                                              int32_t num_splits, int64_t qn_sb, int64_t qn_st, int64_t qn_sh, int64_t qp_sb,
                                              int64_t qp_st, int64_t qp_sh) {
    CHITU_REQUIRE(q_len >= 1 && q_len <= kMlaMultiMaxQ);
    CHITU_REQUIRE(batch <= INT32_MAX / kMlaMultiMaxQ);  // batch * q_len rows
    CHITU_REQUIRE(((qn_sb | qn_st | qn_sh | qp_sb | qp_st | qp_sh) & 7) == 0);  // 16-byte loads of q
    return mla_decode_check_args(q_nope, q_pe, kv_cache, block_table, seqlens, batch, heads, num_pages, page_size, table_stride,
                                 kv_lora_rank, rope_dim, num_splits, 1);
}

// What every entry does behind its argument checks: nothing at batch 0; the workspace carve (num_splits > 1); the opt-in above
// 64 KB of dynamic LDS, set on every call (it is per device and cheap; a process-wide "done" flag would leave the second GPU of a
// multi-device process without it); the launch on grid (num_splits, batch, grid_z) -- `launch(kernel, grid, lds_bytes, part_o,
// part_lse)` is the entry's own hipLaunchKernelGGL, which adds the kernel's arguments -- and stage 2 over `rows` = batch * q_len
// query rows where there is an `out` to merge into (no out: the split partials are left for a fused consumer).
template <typename Kernel, typename Launch>
static inline int mla_decode_launch(Kernel kernel, int lds_bytes, unsigned grid_z, int32_t rows, int32_t batch, int32_t heads,
                                    int32_t num_splits, void* workspace, int64_t workspace_bytes, void* out_bf16, hipStream_t st,
                                    Launch launch) {
    if (batch == 0) return CHITU_OK;
    bf16_t* part_o = nullptr;
    float* part_lse = nullptr;
    if (num_splits > 1)
        if (int rc = mla_decode_carve_workspace(workspace, workspace_bytes, rows, heads, num_splits, &part_o, &part_lse)) return rc;
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    launch(kernel, dim3((unsigned)num_splits, (unsigned)batch, grid_z), lds_bytes, part_o, part_lse);
    if (num_splits > 1 && out_bf16) launch_mla_merge(part_o, part_lse, (bf16_t*)out_bf16, (int64_t)rows * heads, (int)num_splits, st);
    CHITU_RETURN_LAUNCH_STATUS();
}

}  // namespace chitu
