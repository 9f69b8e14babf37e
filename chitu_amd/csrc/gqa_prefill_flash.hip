// Causal GQA / MHA prefill attention for gfx950, head_dim 128, flash form -- the attn_varlen_func call of
// Attention.prefill_forward (chitu/models/model.py:104-132; interface chitu/attn_backend.py:39-90; the reference runs it on
// third-party flash_attn, attn_backend.py:167-206, or on RefAttnBackend's O(L^2)-memory torch path, :394-455).
//
//   out[t,h,:] = softmax_{s <= t, same sequence}( scale * q[t,h,:] . k[s,h / G,:] ) . v[s,h / G,:]        G = Hq / Hkv
//
// The structure of mla_prefill_flash.hip at head_dim 128: the G query heads of a KV head are rows of one Q matrix, a
// workgroup owns 128 Q rows (128 / G consecutive tokens x G heads; any G <= 32, see kEven) of one KV head, each of its 4 waves 32;
//   * Q fragments in registers (8 x 4 VGPRs), S^T = K Q^T by v_mfma_f32_32x32x16_bf16 so a Q row's scores of a 32-key block
//     sit in one lane pair: in-lane softmax, running maximum moved only when a block outgrows it by 2^8 (deferred rescale);
//   * O^T = V^T P^T: bf16 P is already the B fragment, V^T fragments by ds_read_b64_tr_b16, the 32 x 128 accumulator (64
//     registers) per Q row in-lane;
//   * 64-key K and V tiles by LDS-DMA (lds_dma.h) into a 2-deep ring, one barrier per tile; K rows [64][256 B] with chunk c of
//     key r at c ^ (r & 15) (ds_read_b128 of 16 keys x one chunk column: 16 bank groups), V rows with chunk c at
//     c ^ ((r & 3) << 2) (four consecutive keys of a transposed read: four 64-byte bank quarters);
//   * 64 KB of LDS and <= 256 registers: two workgroups per CU, so one workgroup's softmax runs beside the other's MFMAs.
// KV is read once per 128 / G query tokens (the composition this replaces -- one decode launch row per query token over
// staged pages, attn_backend._gqa_varlen_causal of rounds 2-4 -- read it once per token).  Causal work grows with the block
// index: blocks are issued heaviest first.
//
// kWin (chitu_hip_gqa_prefill_window): window_size = (W, 0) and softcap of the same call (attn_backend.py:55-69; the arithmetic of
// RefAttnBackend._attention, :294-392).  W >= 0: query position p sees the keys p - W .. p.  A workgroup's first tile is the one
// that holds key max(0, p0 - W) instead of tile 0 (the ring starts there), half tiles wholly below that key are skipped
// (workgroup-uniform), and the tiles that reach below p0 - W + BQ mask per lane (key < pq - W).  A query row's first half tiles
// can then be empty for that row: its running maximum stays -inf, which the kWin arithmetic allows for.  softcap = c > 0: the
// score is c * tanh(scale * q.k / c), folded into log2 units after the cap.
//
// kPaged (chitu_hip_gqa_prefill_paged): the same kernel with its keys read through a block table -- continued / chunked prefill, the
// seqlen_q != seqlen_k, bottom-right aligned causal case of attn_varlen_func / attn_with_kvcache (attn_backend.py:39-90, :92-164).
// Sequence s has L = seqlens_k[s] keys in its pages, the n = cu_seqlens[s + 1] - cu_seqlens[s] rows of this call (appended before
// it) included; P = L - n is the prefix.  Three things change and nothing else:
//   * positions: blocks of BQ query tokens start at the first NEW token (p0 is local to them; Q rows and output rows are
//     cu_seqlens[s] + local), every position compared against a key is P + local; 64-key tiles still start at key 0.  At P = 0 this
//     is the contiguous kernel block for block, at P % 128 == 0 (P % BQ == 0) it is the contiguous kernel's blocks P / BQ ..: bit-identical
//     outputs (the wave-wide rescale vote sees the same rows).  A query at a negative position (L < n) stores zeros.
//   * issue(): key position t lives at cache row table[s][t / page_size] * page_size + t % page_size.  Positions are clamped to
//     [lo, L - 1] first (lo: the block's lowest visible key, 0 without a window), so no byte of a row >= L or before the window
//     reaches LDS -- a masked key's V row is still multiplied (by 0), so it has to be finite.  A wave brings 16 keys that start at a
//     multiple of 16; page_size % 16 == 0 puts them in one page, and the clamp keeps them there or collapses all 16 onto key lo or
//     key L - 1: ONE table entry per wave and tile, table[s][clamp(t0 + 16 wave) / page_size], always of a page that holds a visible key.
//   * that entry is loaded wave-uniformly, i.e. by a SCALAR load (the index is readfirstlane'd, the table is read through the
//     constant address space): scalar loads count on lgkmcnt, so the compiler's wait for the entry is not a vmcnt wait and cannot
//     drain the LDS-DMA in flight (the rule of tools/check_flash_asm.audit_dma_loops).  This was chosen over requesting a VECTOR load
//     one tile early behind the loop's own vmcnt(0): that keeps a compiler-counted vector load in the DMA-fed loop and stays correct
//     only as long as hipcc places its wait where we hope; a scalar load is right wherever the wait lands.  Its latency is still
//     taken off the path: the entry of tile t + 2 is requested right after issue(t + 1) and first used one iteration later.
#include <type_traits>

#include "common.h"
#include "chitu_hip_ext4.h"
#include "lds_dma.h"

namespace chitu {

namespace gpf {
constexpr int kD = 128;                // head_dim
constexpr int kTile = 64;              // keys per staged tile
constexpr int kRow = kD * 2;           // bytes per K / V row
constexpr int kTileB = kTile * kRow;   // 16 KB
constexpr int kBuf = 2 * kTileB;       // K + V of one ring slot
constexpr float kDefer = 8.0f;
}  // namespace gpf

typedef float f32x16g __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4_gp;

// GT: query heads per KV head, 1 .. 32; 0: taken at run time from the launch (Hq / gridDim.z).  G is used in the set-up and the
// epilogue only, never in the tile loop.
template <int GT, bool kWin = false, bool kPaged = false>
__global__ __launch_bounds__(256, 2) void gqa_prefill_flash_kernel(
    const bf16_t* __restrict__ q, int64_t q_st, int64_t q_sh, const bf16_t* __restrict__ k, int64_t k_st, int64_t k_sh,
    const bf16_t* __restrict__ v, int64_t v_st, int64_t v_sh, const int32_t* __restrict__ cu_seqlens, float scale,
    bf16_t* __restrict__ out, int Hq, int window_left, float softcap, const int32_t* __restrict__ seqlens_k,
    const int32_t* __restrict__ block_table, int table_stride, int page_size) {
    // kPaged: k / v are the caches, k_st / v_st = kv_heads * 128, k_sh / v_sh = 128, cu_seqlens = cu_seqlens_q
    using namespace gpf;
    // kEven (G divides 32): a wave holds 32 / G whole tokens and all 128 rows are live.  Otherwise Q row R = 32 wave + row is
    // head R % G of token R / G -- a token's heads may lie in two waves, which nothing minds: a row is one MFMA column with its
    // own in-lane softmax -- and the 128 - BQ * G rows after the last live one duplicate it (the same position: the same mask,
    // the same vote in the rescale ballot, a finite running maximum) and store nothing.
    constexpr bool kEven = GT > 0 && 32 % GT == 0;
    constexpr int GE = kEven ? GT : 1;  // (the divisor of the kEven arms below, so that they compile at GT = 0)
    const int G = GT > 0 ? GT : Hq / (int)gridDim.z;
    const int BQ = 128 / G;  // query tokens per workgroup
    __shared__ __attribute__((aligned(16))) uint8_t smem[2 * kBuf];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane & 31, hi = lane >> 5;
    const int seq = blockIdx.y, kvh = blockIdx.z;
    const int s0 = cu_seqlens[seq], n = cu_seqlens[seq + 1] - s0;  // first Q / output row, query tokens
    const int L = kPaged ? seqlens_k[seq] : n;                     // keys
    const int P = kPaged ? L - n : 0;                              // position of the first query token
    const int p0 = ((int)gridDim.x - 1 - (int)blockIdx.x) * BQ;  // heaviest (latest) block first; local to the query tokens
    if (p0 >= n) return;
    const int nq = min(BQ, n - p0);
    const int n_keys = P + p0 + nq;
    const int R = kEven ? 0 : min(wave * 32 + row, BQ * G - 1);     // !kEven: this lane's Q row, a padding row taking the last live one
    auto live = [&] { return kEven || wave * 32 + row < BQ * G; };  // not a padding row
    // this lane's head within the group and its query token within the block (one past the end repeats the last, stores nothing).
    // The kEven arms divide unsigned, which is what keeps those kernels' code what it was before GT = 0 and !kEven existed.
    auto hq = [&] { return kEven ? (int)((unsigned)row % (unsigned)GE) : R % G; };
    const int tq = kEven ? wave * (32 / GE) + (int)((unsigned)row / (unsigned)GE) : R / G;
    const int tl = p0 + min(tq, nq - 1);    // its index among the sequence's query tokens
    if (kPaged && n_keys <= 0) {            // every query of the block sits before key 0 (L < n): zeros, no key is touched
        if (live() && tq < nq && kvh * G + hq() < Hq) {
            bf16_t* dst = out + ((int64_t)(s0 + p0 + tq) * Hq + kvh * G + hq()) * kD + 64 * hi;
            for (int i = 0; i < 8; ++i) *reinterpret_cast<i32x4*>(dst + 8 * i) = i32x4{0, 0, 0, 0};
        }
        return;
    }
    const int n_tiles = (n_keys + kTile - 1) / kTile;
    const bool win = kWin && window_left >= 0;
    const int lo = win ? max(P + p0 - window_left, 0) : 0;  // the block's lowest visible key
    const int tile0 = lo / kTile;
    // its position: keys 0 .. pq (kWin: klo .. pq).  kPaged: a row before key 0 computes as position 0 and stores zeros
    const int pq = kPaged ? max(P + tl, 0) : tl;
    const int klo = win ? pq - window_left : 0;
    const int head = kvh * G + hq();
    const bf16_t* kbase = k + (kPaged ? 0 : (int64_t)s0 * k_st) + (int64_t)kvh * k_sh;  // kPaged: cache rows, not rows of this call
    const bf16_t* vbase = v + (kPaged ? 0 : (int64_t)s0 * v_st) + (int64_t)kvh * v_sh;
    const uint32_t lds0 = lds_offset_of(&smem[0]);

    // ---- tile DMA: wave w brings keys 16 w .. 16 w + 15 of K and of V, four 4-row pieces each
    const int dr = lane >> 4, dp = lane & 15;  // row inside a piece, chunk position
    // kPaged: the wave's 16 keys of a tile, clamped to [lo, L - 1], lie in one page (header); its first key's position in the
    // sequence and its table entry, both wave-uniform, the entry by a scalar load
    const __attribute__((address_space(4))) int32_t* trow =
        (const __attribute__((address_space(4))) int32_t*)(block_table + (int64_t)seq * table_stride);
    auto page_first = [&](int tile) {
        const int a = min(max(tile * kTile + wave * 16, lo), L - 1);
        return __builtin_amdgcn_readfirstlane(a / page_size);
    };
    int pidx = 0, pentry = 0;  // of the tile issue() is called for next
    if constexpr (kPaged) {
        pidx = page_first(tile0);
        pentry = trow[pidx];
    }
    auto issue = [&](int tile) {
        const int t0 = tile * kTile;
        const uint32_t dst = lds0 + (uint32_t)((tile & 1) * kBuf);
        // kPaged: cache row of key position x is prow + x
        const int64_t prow = kPaged ? ((int64_t)pentry - pidx) * page_size : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = wave * 16 + i * 4 + dr;
            // rows past the sequence repeat its last key (finite, masked by causality); kPaged: rows before the window repeat key lo
            const int64_t grow = kPaged ? prow + min(max(t0 + r, lo), L - 1) : min(t0 + r, L - 1);
            glds16_vaddr(kbase + grow * k_st + ((dp ^ (r & 15)) << 3), dst + (uint32_t)((wave * 4 + i) * 1024));
            glds16_vaddr(vbase + grow * v_st + ((dp ^ ((r & 3) << 2)) << 3), dst + (uint32_t)(kTileB + (wave * 4 + i) * 1024));
        }
    };
    issue(tile0);
    if constexpr (kPaged) {
        pidx = page_first(tile0 + 1);
        pentry = trow[pidx];
    }

    // ---- Q fragments (B operand of S^T = K Q^T): lane (row, hi) holds q[token][head][16 kk + 8 hi .. + 8]
    s16x8 qf[8];
    {
        const bf16_t* qp = q + (int64_t)(s0 + tl) * q_st + (int64_t)head * q_sh + hi * 8;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) qf[kk] = *reinterpret_cast<const s16x8*>(qp + kk * 16);
        // hipcc must wait for these loads HERE, not inside the tile loop (its vmcnt ladder would drain the LDS-DMA it cannot see)
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) asm volatile("" : "+v"(qf[kk]));
    }
    f32x16g o[4];  // O^T[dim 32 cb + crow(reg, hi)][this lane's Q row]
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const float c2 = scale * 1.4426950408889634f;
    const bool cap = kWin && softcap > 0.f;
    const float cap_in = cap ? scale / softcap : 0.f, cap_out = softcap * 1.4426950408889634f;

    // lane-constant LDS offsets
    int koff[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) koff[kk] = row * kRow + (((2 * kk + hi) ^ (lane & 15)) << 4);
    const int rr = (lane & 15) >> 2, cl = 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1);
    int voff[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) voff[cb] = (4 * hi + rr) * kRow + ((cb ^ rr) << 6) + (cl << 4) + ((lane & 1) << 3);

    for (int tile = tile0; tile < n_tiles; ++tile) {
        const int t0 = tile * kTile;
        glds_wait_all();   // this wave's pieces of the tile have landed
        __syncthreads();   // everyone's have; the other ring slot is no longer being read
        if (tile + 1 < n_tiles) issue(tile + 1);
        if constexpr (kPaged) {  // the entry of tile + 2 (clamped: always a page with a visible key), used one iteration later
            pidx = page_first(tile + 2);
            pentry = trow[pidx];
        }
        const uint8_t* bufK = smem + (tile & 1) * kBuf;
        const uint8_t* bufV = bufK + kTileB;
        // the tile reaches into the block's own token range (two tiles at G = 1) or, kWin, below some row's window: mask by position
        const bool last = t0 + kTile > P + p0 || (win && t0 < P + p0 - window_left + BQ);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (t0 + kb * 32 >= n_keys) break;  // the block's last key is before this half tile (workgroup-uniform)
            if (kWin && t0 + kb * 32 + 32 <= lo) continue;  // the block's lowest visible key is behind it (workgroup-uniform)
            // ---- S^T[key 32 kb + crow(reg, hi)][Q row]
            f32x16g s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const s16x8 kf = *reinterpret_cast<const s16x8*>(bufK + kb * 32 * kRow + koff[kk]);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], s, 0, 0, 0);
            }
            float pmax = -INFINITY;
            if (kWin && cap) {  // c * tanh(x / c) in log2 units; tanh(y) = 1 - 2 / (1 + e^2y), |y| <= 15 keeps e^2y finite
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const float y = __builtin_fminf(__builtin_fmaxf(s[r] * cap_in, -15.f), 15.f);
                    const float x = cap_out * (1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * y)));
                    s[r] = !last || (key <= pq && key >= klo) ? x : -INFINITY;
                    pmax = __builtin_fmaxf(pmax, s[r]);
                }
            } else if (last) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    s[r] = key <= pq && (!kWin || key >= klo) ? s[r] * c2 : -INFINITY;
                    pmax = __builtin_fmaxf(pmax, s[r]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] *= c2;
                    pmax = __builtin_fmaxf(pmax, s[r]);
                }
            }
            if (__builtin_amdgcn_ballot_w64(pmax > m + kDefer) != 0) {  // m = -inf (first block): every lane votes
                const float mx = __builtin_fmaxf(pmax, __shfl_xor(pmax, 32, 64));
                const float m_new = __builtin_fmaxf(m, mx);  // finite: key 0 is visible to every row (kWin: -inf until the row's window)
                const float alpha = kWin && m_new == -INFINITY ? 1.f : __builtin_amdgcn_exp2f(m - m_new);
                m = m_new;
                l *= alpha;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[cb][r] *= alpha;
            }
            s16x8 pb[2];
            float psum = 0.f;
            const float ms = kWin && m == -INFINITY ? 0.f : m;  // a row with no visible key yet: every p is 2^-inf = 0
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float a = __builtin_amdgcn_exp2f(s[r] - ms);
                const float b = __builtin_amdgcn_exp2f(s[r + 1] - ms);
                psum += a + b;
                const uint32_t pk = f32x2_to_bf16x2(a, b);
                pb[r >> 3][r & 7] = (short)(pk & 0xffffu);
                pb[r >> 3][(r & 7) + 1] = (short)(pk >> 16);
            }
            l += psum;
            // ---- O^T += V^T P^T: k-slot 8 hi + e of step t <-> key 32 kb + 16 t + 8 (e >> 2) + 4 hi + (e & 3)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const uint8_t* vb = bufV + (kb * 32 + t * 16) * kRow;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_gp*)(vb + voff[cb]));
                    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_gp*)(vb + 8 * kRow + voff[cb]));
                    s16x8 vf;
                    vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
                    vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
                    o[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pb[t], o[cb], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: lane holds dims 32 cb + 8 rq + 4 hi + {0..3} of its row: 8-byte stores (l and l ^ 32 fill 16 bytes)
    const float inv = kPaged && P + tl < 0 ? 0.f : 1.0f / (l + __shfl_xor(l, 32, 64));
    if (!live() || tq >= nq || head >= Hq) return;
    bf16_t* dst = out + ((int64_t)(s0 + p0 + tq) * Hq + head) * kD + 4 * hi;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            i32x2 pk;
            pk[0] = (int)f32x2_to_bf16x2(o[cb][4 * rq] * inv, o[cb][4 * rq + 1] * inv);
            pk[1] = (int)f32x2_to_bf16x2(o[cb][4 * rq + 2] * inv, o[cb][4 * rq + 3] * inv);
            *reinterpret_cast<i32x2*>(dst + 32 * cb + 8 * rq) = pk;
        }
    }
}

}  // namespace chitu

namespace chitu {

// window_left = -1 and softcap = 0 (chitu_hip_gqa_prefill): the kernels without the window / cap code.  any_group
// (chitu_hip_ext4.h): every G <= 32 instead of the powers of two; at a power of two the launch is the same either way.
static int gqa_prefill_launch(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_bf16, int64_t k_stride_t,
                              int64_t k_stride_h, const void* v_bf16, int64_t v_stride_t, int64_t v_stride_h,
                              const int32_t* cu_seqlens, int32_t n_seq, int32_t max_seqlen, float softmax_scale, void* out_bf16,
                              int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t window_left, float softcap,
                              void* stream, bool any_group = false) {
    CHITU_REQUIRE(q_bf16 && k_bf16 && v_bf16 && cu_seqlens && out_bf16 && n_seq >= 0 && max_seqlen >= 0);
    CHITU_REQUIRE(q_heads >= 1 && kv_heads >= 1 && q_heads % kv_heads == 0);
    CHITU_REQUIRE(window_left >= -1 && softcap >= 0.f);  // (a NaN cap fails the comparison)
    if (head_dim != gpf::kD) return CHITU_ERR_UNSUPPORTED;
    const int G = q_heads / kv_heads;
    if (G > 32 || (!any_group && (G & (G - 1)) != 0)) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE((q_stride_t | q_stride_h | k_stride_t | k_stride_h | v_stride_t | v_stride_h) % 8 == 0);
    CHITU_REQUIRE(((uintptr_t)q_bf16 | (uintptr_t)k_bf16 | (uintptr_t)v_bf16 | (uintptr_t)out_bf16) % 16 == 0);
    if (n_seq == 0 || max_seqlen == 0) return CHITU_OK;
    const int BQ = 128 / G;
    const dim3 grid((unsigned)((max_seqlen + BQ - 1) / BQ), (unsigned)n_seq, (unsigned)kv_heads);
#define LAUNCH_GW(GV, WIN)                                                                                                   \
    hipLaunchKernelGGL((gqa_prefill_flash_kernel<GV, WIN>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q_bf16,    \
                       q_stride_t, q_stride_h, (const bf16_t*)k_bf16, k_stride_t, k_stride_h, (const bf16_t*)v_bf16, v_stride_t, \
                       v_stride_h, cu_seqlens, softmax_scale, (bf16_t*)out_bf16, (int)q_heads, (int)window_left, softcap,            \
                       (const int32_t*)nullptr, (const int32_t*)nullptr, 0, 0)
#define LAUNCH_G(GV)                                                 \
    do {                                                             \
        if (window_left < 0 && softcap == 0.f) LAUNCH_GW(GV, false); \
        else LAUNCH_GW(GV, true);                                    \
    } while (0)
    switch (G) {
        case 1: LAUNCH_G(1); break;
        case 2: LAUNCH_G(2); break;
        case 4: LAUNCH_G(4); break;
        case 8: LAUNCH_G(8); break;
        case 16: LAUNCH_G(16); break;
        case 32: LAUNCH_G(32); break;
        case 3: LAUNCH_G(3); break;   // the group sizes of published models that do not divide 32 ...
        case 5: LAUNCH_G(5); break;
        case 6: LAUNCH_G(6); break;
        case 7: LAUNCH_G(7); break;
        case 12: LAUNCH_G(12); break;
        default: LAUNCH_G(0); break;  // ... and every other one: G at run time
    }
#undef LAUNCH_G
#undef LAUNCH_GW
    CHITU_RETURN_LAUNCH_STATUS();
}

// the kPaged kernels: K / V rows through the block table, query positions aligned to the end of each sequence's keys
static int gqa_prefill_paged_launch(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_cache,
                                    const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                                    const int32_t* block_table, int32_t table_stride, const int32_t* cu_seqlens_q,
                                    const int32_t* seqlens_k, int32_t n_seq, int32_t max_seqlen_q, float softmax_scale,
                                    void* out_bf16, int32_t q_heads, int32_t head_dim, int32_t window_left, float softcap,
                                    void* stream, bool any_group = false) {
    CHITU_REQUIRE(q_bf16 && k_cache && v_cache && block_table && cu_seqlens_q && seqlens_k && out_bf16);
    CHITU_REQUIRE(n_seq >= 0 && max_seqlen_q >= 0 && num_pages >= 1 && table_stride >= 1);
    CHITU_REQUIRE(q_heads >= 1 && kv_heads >= 1 && q_heads % kv_heads == 0);
    CHITU_REQUIRE(window_left >= -1 && softcap >= 0.f);  // (a NaN cap fails the comparison)
    if (head_dim != gpf::kD) return CHITU_ERR_UNSUPPORTED;
    const int G = q_heads / kv_heads;
    if (G > 32 || (!any_group && (G & (G - 1)) != 0)) return CHITU_ERR_UNSUPPORTED;
    if (page_size < 16 || page_size % 16 != 0) return CHITU_ERR_UNSUPPORTED;
    CHITU_REQUIRE((q_stride_t | q_stride_h) % 8 == 0);
    CHITU_REQUIRE(((uintptr_t)q_bf16 | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)out_bf16) % 16 == 0);
    if (n_seq == 0 || max_seqlen_q == 0) return CHITU_OK;
    const int BQ = 128 / G;
    const dim3 grid((unsigned)((max_seqlen_q + BQ - 1) / BQ), (unsigned)n_seq, (unsigned)kv_heads);
    const int64_t row = (int64_t)kv_heads * gpf::kD;
#define LAUNCH_GW(GV, WIN)                                                                                                  \
    hipLaunchKernelGGL((gqa_prefill_flash_kernel<GV, WIN, true>), grid, dim3(256), 0, (hipStream_t)stream,                    \
                       (const bf16_t*)q_bf16, q_stride_t, q_stride_h, (const bf16_t*)k_cache, row, (int64_t)gpf::kD,          \
                       (const bf16_t*)v_cache, row, (int64_t)gpf::kD, cu_seqlens_q, softmax_scale, (bf16_t*)out_bf16,         \
                       (int)q_heads, (int)window_left, softcap, seqlens_k, block_table, (int)table_stride, (int)page_size)
#define LAUNCH_G(GV)                                                 \
    do {                                                             \
        if (window_left < 0 && softcap == 0.f) LAUNCH_GW(GV, false); \
        else LAUNCH_GW(GV, true);                                    \
    } while (0)
    switch (G) {
        case 1: LAUNCH_G(1); break;
        case 2: LAUNCH_G(2); break;
        case 4: LAUNCH_G(4); break;
        case 8: LAUNCH_G(8); break;
        case 16: LAUNCH_G(16); break;
        case 32: LAUNCH_G(32); break;
        case 3: LAUNCH_G(3); break;   // the group sizes of published models that do not divide 32 ...
        case 5: LAUNCH_G(5); break;
        case 6: LAUNCH_G(6); break;
        case 7: LAUNCH_G(7); break;
        case 12: LAUNCH_G(12); break;
        default: LAUNCH_G(0); break;  // ... and every other one: G at run time
    }
#undef LAUNCH_G
#undef LAUNCH_GW
    CHITU_RETURN_LAUNCH_STATUS();
}

}  // namespace chitu

extern "C" int chitu_hip_gqa_prefill_paged(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_cache,
                                           const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                                           const int32_t* block_table, int32_t table_stride, const int32_t* cu_seqlens_q,
                                           const int32_t* seqlens_k, int32_t n_seq, int32_t max_seqlen_q, float softmax_scale,
                                           void* out_bf16, int32_t q_heads, int32_t head_dim, int32_t window_left, float softcap,
                                           void* stream) {
    return chitu::gqa_prefill_paged_launch(q_bf16, q_stride_t, q_stride_h, k_cache, v_cache, num_pages, page_size, kv_heads,
                                           block_table, table_stride, cu_seqlens_q, seqlens_k, n_seq, max_seqlen_q, softmax_scale,
                                           out_bf16, q_heads, head_dim, window_left, softcap, stream);
}

extern "C" int chitu_hip_gqa_prefill(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_bf16,
                                     int64_t k_stride_t, int64_t k_stride_h, const void* v_bf16, int64_t v_stride_t,
                                     int64_t v_stride_h, const int32_t* cu_seqlens, int32_t n_seq, int32_t max_seqlen,
                                     float softmax_scale, void* out_bf16, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                                     void* stream) {
    return chitu::gqa_prefill_launch(q_bf16, q_stride_t, q_stride_h, k_bf16, k_stride_t, k_stride_h, v_bf16, v_stride_t, v_stride_h,
                                     cu_seqlens, n_seq, max_seqlen, softmax_scale, out_bf16, q_heads, kv_heads, head_dim, -1, 0.0f,
                                     stream);
}

extern "C" int chitu_hip_gqa_prefill_window(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_bf16,
                                            int64_t k_stride_t, int64_t k_stride_h, const void* v_bf16, int64_t v_stride_t,
                                            int64_t v_stride_h, const int32_t* cu_seqlens, int32_t n_seq, int32_t max_seqlen,
                                            float softmax_scale, void* out_bf16, int32_t q_heads, int32_t kv_heads,
                                            int32_t head_dim, int32_t window_left, float softcap, void* stream) {
    return chitu::gqa_prefill_launch(q_bf16, q_stride_t, q_stride_h, k_bf16, k_stride_t, k_stride_h, v_bf16, v_stride_t, v_stride_h,
                                     cu_seqlens, n_seq, max_seqlen, softmax_scale, out_bf16, q_heads, kv_heads, head_dim, window_left,
                                     softcap, stream);
}

// ---- chitu_hip_ext4.h: the same launchers at any group size
extern "C" int chitu_ext4_gqa_prefill(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_bf16,
                                      int64_t k_stride_t, int64_t k_stride_h, const void* v_bf16, int64_t v_stride_t,
                                      int64_t v_stride_h, const int32_t* cu_seqlens, int32_t n_seq, int32_t max_seqlen,
                                      float softmax_scale, void* out_bf16, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                                      int32_t window_left, float softcap, void* stream) {
    return chitu::gqa_prefill_launch(q_bf16, q_stride_t, q_stride_h, k_bf16, k_stride_t, k_stride_h, v_bf16, v_stride_t, v_stride_h,
                                     cu_seqlens, n_seq, max_seqlen, softmax_scale, out_bf16, q_heads, kv_heads, head_dim, window_left,
                                     softcap, stream, true);
}

extern "C" int chitu_ext4_gqa_prefill_paged(const void* q_bf16, int64_t q_stride_t, int64_t q_stride_h, const void* k_cache,
                                            const void* v_cache, int64_t num_pages, int32_t page_size, int32_t kv_heads,
                                            const int32_t* block_table, int32_t table_stride, const int32_t* cu_seqlens_q,
                                            const int32_t* seqlens_k, int32_t n_seq, int32_t max_seqlen_q, float softmax_scale,
                                            void* out_bf16, int32_t q_heads, int32_t head_dim, int32_t window_left, float softcap,
                                            void* stream) {
    return chitu::gqa_prefill_paged_launch(q_bf16, q_stride_t, q_stride_h, k_cache, v_cache, num_pages, page_size, kv_heads,
                                           block_table, table_stride, cu_seqlens_q, seqlens_k, n_seq, max_seqlen_q, softmax_scale,
                                           out_bf16, q_heads, head_dim, window_left, softcap, stream, true);
}
