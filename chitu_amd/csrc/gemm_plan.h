// Every launch rule of the weight-streaming dense GEMMs, as plain C++: no HIP include and nothing device-side, so a host
// compiler alone compiles it (tests/test_dense_exact_host.py does, and checks each rule against the tests' own mirrors).
//
// A launch is a grid of (N + 15) / 16 tiles x S, workgroups of WK waves that split K between them, and one pass per 32 or 64
// token rows.  The fp8 / soft-fp8 launchers (fp8_gemm.hip), the fused norm + fp8 GEMM (fp8_norm_gemm.hip), the int8 W8A8
// launcher (w8a8_int8.hip) and, through stream_gemm.h, the bf16 and W8A16 ones take their plans from here.  Options
// (common.h::debug_option) come in as values: < 0 = none.
#pragma once
#include <cstdint>
#include <type_traits>

namespace chitu {

struct SplitPlan {
    int WK, S;  // waves per workgroup that split K; workgroups per tile that split K (S > 1: fp32 planes + a reduce)
};

// ---------------------------------------------------------------- fp8 weights, 128-wide K blocks
// WK: the widest power of two <= 8 within T = min(KB, ceil(1536 / tiles)) waves per tile.
inline SplitPlan fp8_split_plan(int64_t N, int64_t K) {
    const int tiles = (int)((N + 15) / 16);
    const int KB = (int)((K + 127) / 128);
    int T = (1536 + tiles - 1) / tiles;
    if (T > KB) T = KB;
    if (T < 1) T = 1;
    int WK = 1;
    while (WK * 2 <= T && WK < 8) WK *= 2;
    // A cross-workgroup split costs a second (reduce) launch: measured ~5 us inside the decode
    // graph, more than the few us it saves on <= 16 MB of weights.  Only use it when N alone
    // leaves most of the chip idle AND the matrix is big enough to matter.
    int S = 1;
    if (tiles * WK < 256 && N * K >= (int64_t)(24 << 20)) {
        S = (T + WK - 1) / WK;
        if (S > 8) S = 8;
        if (S * WK > KB) S = KB / WK > 0 ? KB / WK : 1;
    }
    return {WK, S};
}

// chitu_hip_soft_fp8_gemm: the plan, without the cross-workgroup split when its S planes of M x N fp32 do not fit the
// caller's workspace (workspace_bytes: 0 for none).
inline SplitPlan fp8_plan_in_workspace(int64_t M, int64_t N, int64_t K, int64_t workspace_bytes) {
    SplitPlan plan = fp8_split_plan(N, K);
    if (plan.S > 1 && workspace_bytes < (int64_t)plan.S * M * N * 4) plan.S = 1;
    return plan;
}

// chitu_hip_fp8_gemm_blockscale[_tm], in this order: the plan in the workspace, the fp8_gemm_wk option in place of its WK,
// then WK halved until every wave of every split has a K block.
inline SplitPlan fp8_stream_plan(int64_t M, int64_t N, int64_t K, int64_t workspace_bytes, int forced_wk) {
    SplitPlan plan = fp8_plan_in_workspace(M, N, K, workspace_bytes);
    if (forced_wk >= 0) plan.WK = forced_wk;
    while (plan.WK > 1 && plan.WK * plan.S > (int)(K / 128)) plan.WK >>= 1;
    return plan;
}

// chitu_hip_fp8_gemm_blockscale_partials: the caller sets S; WK doubles while every wave keeps a K block, up to 8.
inline SplitPlan fp8_partials_plan(int64_t K, int num_splits) {
    SplitPlan plan{1, num_splits};
    while (plan.WK < 8 && plan.WK * 2 * plan.S <= (int)(K / 128)) plan.WK *= 2;
    return plan;
}

// DEEP (a pass of at most 16 rows): 8 waves with 5 to 8 K blocks each request their whole K range at once, one HBM round
// trip instead of two.  deep_option: the fp8_gemm_deep option, 0 = never.
inline bool fp8_deep(SplitPlan plan, int64_t K, int deep_option) {
    const int per_wave = (int)(K / 128) / (plan.WK * plan.S);
    return plan.WK == 8 && per_wave > 4 && per_wave <= 8 && deep_option != 0;
}

// chitu_hip_fp8_gemm_add_norm (K % 128 == 0, K <= 8192): the K split chitu_hip_fp8_gemm_blockscale picks for the shape, so
// that the fused and the unfused launches accumulate in the same order; 0 = a cross-workgroup split or < 4 waves: not served.
inline int fp8_norm_gemm_wk(int64_t N, int64_t K) {
    const SplitPlan plan = fp8_split_plan(N, K);
    if (plan.S > 1) return 0;
    int WK = plan.WK;
    while (WK > 1 && WK > (int)(K / 128)) WK >>= 1;
    return WK >= 4 ? WK : 0;
}

// ---------------------------------------------------------------- int8 W8A8: by the tile count alone, no grid split
inline int w8a8_int8_wk(int64_t N, int64_t K) {
    const int tiles = (int)((N + 15) / 16);
    int WK = tiles >= 1024 ? 2 : tiles >= 384 ? 4 : 8;
    while (WK > 1 && WK > (int)(K / 128)) WK >>= 1;
    return WK;
}

// ---------------------------------------------------------------- bf16 and W8A16 (stream_gemm.h)
// K-split width: the widest power of two <= 8 that leaves every wave (of each of the S grid splits) a K step and the launch
// at most 4096 waves.  Mirrored by chitu_amd.ops.w8a16_plan and tests/dense_exact.py::bf16_wk.
inline int stream_wk(int64_t tiles, int64_t steps, int64_t S = 1) {
    int WK = 8;
    while (WK > 1 && (WK * S > steps || tiles * S * WK > 4096)) WK >>= 1;
    return WK;
}

// ---------------------------------------------------------------- the M walk of all of them
// ROWS-row passes, launch(m_base, MT, WK) with MT = the 16-row token tiles of a pass -- 1 when at most 16 rows are left, 2
// when at most 32 (or ROWS is 32), else 4 -- and WK one of 8, 4, 2, 1: both as std::integral_constant, for the kernel's
// template arguments.
template <int ROWS = 32, class F>
inline void stream_walk_m(int64_t M, int WK, F&& launch) {
    static_assert(ROWS == 32 || ROWS == 64, "a pass is two or four token tiles");
    auto with_wk = [&](int m_base, auto mt) {
        switch (WK) {
            case 8: launch(m_base, mt, std::integral_constant<int, 8>{}); break;
            case 4: launch(m_base, mt, std::integral_constant<int, 4>{}); break;
            case 2: launch(m_base, mt, std::integral_constant<int, 2>{}); break;
            default: launch(m_base, mt, std::integral_constant<int, 1>{}); break;
        }
    };
    for (int64_t mb = 0; mb < M; mb += ROWS) {
        if (M - mb <= 16) with_wk((int)mb, std::integral_constant<int, 1>{});
        else if (ROWS == 32 || M - mb <= 32) with_wk((int)mb, std::integral_constant<int, 2>{});
        else if constexpr (ROWS == 64) with_wk((int)mb, std::integral_constant<int, 4>{});
    }
}

}  // namespace chitu
