"""Multi-token MLA paged decode on the GPU (chitu_hip_mla_decode_multi / _kv_fp8, the kTok = 2 kernels of csrc/mla_decode.hip and
csrc/mla_decode_kv_fp8.hip, through HipAttnBackend.mla_decode_multi): the bit-identity table of the kernel's header against chitu_hip_mla_decode on the expanded
problem, the attention bar and the counting construction where no bit claim is made, the causality probe, the fp8 entry
against the bf16 entry on the dequantised cache, strided q and the argument errors.  Page size 64; wherever no key lives the
caches hold NaN (tests/mla_multi_ref.py)."""
import ctypes

import pytest
import torch

from tests import attn_exact as ax
from tests import mla_multi_ref as mr
from tests.test_gpu_mla import REL_TOL
from tests.util import assert_close

pytestmark = pytest.mark.gpu

SCALE = mr.SCALE


def backend(H):
    from chitu_amd.attn_backend import HipAttnBackend

    return HipAttnBackend(local_n_heads=H, max_seq_len=8192)


def device_cache(case, fp8, want_bf16_twin=False):
    """(cache on the device, table); fp8 with want_bf16_twin: also the dequantised bf16 cache"""
    from chitu_amd import ops

    cache, table = mr.paged(case["rows"], case["lens"].tolist(), seed=case["seed"], fp8=fp8)
    cache = cache.cuda()
    if want_bf16_twin:
        return cache, ops.mla_kv_dequant_fp8(cache), table
    return cache, table


def ws_bytes(part, rows, H):
    """the live bytes of a returned workspace: bf16 partial rows [rows, H, S, 512] | fp32 LSE [rows, H, S]"""
    ws, S = part
    return ws.view(torch.uint8)[: rows * H * S * (512 * 2 + 4)].clone().cpu()


def run_multi(case, cache, table, splits, partials=False, q=None, kernel="multi"):
    """the multi-token launch itself (kernel="multi": never the host's routing rule)"""
    H = case["q_nope"].shape[2]
    qn, qp = q if q is not None else (case["q_nope"].cuda(), case["q_pe"].cuda())
    res = backend(H).mla_decode_multi(qn, qp, cache, case["lens"].cuda(), table.cuda(), SCALE, num_splits=splits, return_partials=partials,
                                      kernel=kernel)
    if partials:
        bs, T = case["q_nope"].shape[:2]
        return ws_bytes(res, bs * T, H)
    return res.cpu()


def run_expanded(case, cache, table, splits, partials=False):
    """chitu_hip_mla_decode on batch * T rows, each table row repeated T times, lengths L_t"""
    bs, T, H, _ = case["q_nope"].shape
    qn, qp, tab, exp = mr.expand(case, table)
    res = backend(H).mla_decode(qn.cuda(), qp.cuda(), cache, exp.cuda(), tab.cuda(), SCALE, num_splits=splits, return_partials=partials)
    if partials:
        return ws_bytes(res, bs * T, H)
    return res.view(bs, T, H, 512).cpu()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def zero_rows_where_no_key(out, lens, T):
    for b, L in enumerate(lens):
        for t in range(T):
            if L - T + t < 0:
                assert bool((out[b, t] == 0).all()), (b, t)


# ---------------------------------------------------------------- q_len == 1: the single-token entries' bits
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("H", [16, 20])
def test_one_token_is_bit_identical_to_the_single_token_entry(H, splits, fp8):
    case = mr.random_case(H, 1, [130, 0, 65], seed=7 + H)
    cache, table = device_cache(case, fp8)
    got, want = run_multi(case, cache, table, splits), run_expanded(case, cache, table, splits)
    assert not torch.isnan(want.float()).any() and same_bits(got, want)
    if splits > 1:
        assert torch.equal(run_multi(case, cache, table, splits, partials=True), run_expanded(case, cache, table, splits, partials=True))


# ---------------------------------------------------------------- one split: every row is the expanded call's
# together: L = T (the first token sees one key), L < T (queries without a key: zeros), 65 / T = 2 and 67 / T = 5 (tokens on both
# sides of a tile and page edge), 64 exactly, 200 (four tiles), 0
ONE_SPLIT = [(2, 16, [2, 65, 0]), (2, 20, [1, 64, 200]), (3, 20, [3, 2, 200]), (5, 16, [67, 4, 64]), (5, 20, [5, 0, 200]),
             (8, 16, [8, 5, 200]), (8, 20, [64, 67, 0])]


@pytest.mark.parametrize("T,H,lens", ONE_SPLIT)
def test_one_split_rows_are_bit_identical_to_the_expanded_single_token_call(T, H, lens):
    case = mr.random_case(H, T, lens, seed=T * 100 + H)
    cache, table = device_cache(case, False)
    got, want = run_multi(case, cache, table, 1), run_expanded(case, cache, table, 1)
    assert not torch.isnan(got.float()).any()
    for b in range(len(lens)):
        for t in range(T):
            assert same_bits(got[b, t], want[b, t]), (b, t)
    zero_rows_where_no_key(got, lens, T)
    assert_close(got, mr.multi64(case["q_nope"].float(), case["q_pe"].float(), case["rows"], lens), REL_TOL, what=(T, H, lens))


# ---------------------------------------------------------------- several splits, every sequence's tokens inside one tile
SAME_TILE = [(2, 16, [64, 130, 10]), (4, 20, [200, 68, 128]), (8, 20, [72, 200, 8]), (5, 16, [197, 5, 0])]


@pytest.mark.parametrize("splits", [2, 3, 7])
@pytest.mark.parametrize("T,H,lens", SAME_TILE)
def test_splits_with_tokens_in_one_tile_are_bit_identical_output_and_workspace(T, H, lens, splits):
    assert mr.same_tile(lens, T)
    case = mr.random_case(H, T, lens, seed=T * 10 + splits)
    cache, table = device_cache(case, False)
    got, want = run_multi(case, cache, table, splits), run_expanded(case, cache, table, splits)
    assert not torch.isnan(got.float()).any() and same_bits(got, want)
    assert torch.equal(run_multi(case, cache, table, splits, partials=True), run_expanded(case, cache, table, splits, partials=True))


# ---------------------------------------------------------------- several splits, tokens on both sides of a tile edge: the bar
STRADDLE = [(2, 16, [65, 65, 0]), (4, 20, [130, 65, 129])]


@pytest.mark.parametrize("splits", [2, 3, 7])
@pytest.mark.parametrize("T,H,lens", STRADDLE)
def test_splits_with_straddling_tokens_meet_the_attention_bar_and_count_every_key(T, H, lens, splits):
    """the earlier tokens' split ranges are not those of their own single-token launch: no torch.equal claim"""
    assert not mr.same_tile(lens, T)
    case = mr.random_case(H, T, lens, seed=T + splits)
    cache, table = device_cache(case, False)
    got = run_multi(case, cache, table, splits)
    err = assert_close(got, mr.multi64(case["q_nope"].float(), case["q_pe"].float(), case["rows"], lens), REL_TOL, what=(T, H, lens, splits))
    count = mr.count_case(H, T, lens, salt=splits)
    cache, table = device_cache(count, False)
    worst = ax.check_count(run_multi(count, cache, table, splits), count["want"])
    print(f"straddling T={T} lens={lens} splits={splits}: max_rel_to_peak {err:.2e}, counting {worst:.2e} (bar {ax.REL_COUNT:.2e})")


@pytest.mark.parametrize("splits", [1, 3])
def test_counting_at_lengths_across_two_tiles(splits):
    """T = 3 at fifteen lengths in 0 .. 131, three per launch: one lost or wrongly admitted key moves a channel by >= 1/17"""
    for L0 in range(0, 132, 33):
        count = mr.count_case(16, 3, [L0, L0 + 1, min(L0 + 32, 131)], salt=1)
        cache, table = device_cache(count, False)
        ax.check_count(run_multi(count, cache, table, splits), count["want"])


# ---------------------------------------------------------------- causality
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("T,L", mr.CAUSAL)
def test_a_key_one_past_a_tokens_horizon_is_not_seen_by_it_and_is_seen_by_the_next(T, L, splits, fp8):
    """fails for a kernel that masks by L instead of L_t (three probes, i.e. sequences, per launch)"""
    H = 16
    for first in range(0, T - 1, 3):
        case = mr.causal_probe_case(H, T, L, probes=range(first, min(first + 3, T - 1)))
        cache, table = device_cache(case, fp8)
        got = run_multi(case, cache, table, splits).double()
        ref = mr.multi64(case["q_nope"].float(), case["q_pe"].float(), case["rows"], case["lens"])
        for n, (i, pos) in enumerate(zip(case["probes"], case["pos"])):
            key_row = case["rows"][n][pos, :512].double().expand(H, 512)
            for t in range(T):
                if t > i:
                    ax.check_dominant(got[n, t], key_row)
                else:  # the key is invisible: the mean of the visible rows, >= 1 away from the key's row in some channel
                    assert float((got[n, t] - key_row).abs().max()) >= 0.5, (i, t)
                    assert_close(got[n, t], ref[n, t], REL_TOL, what=("unseen", i, t))


# ---------------------------------------------------------------- the fp8 entry
@pytest.mark.parametrize("T,H,lens,splits", [(1, 20, [130, 0, 65], 3), (5, 16, [67, 4, 64], 1), (8, 20, [64, 67, 0], 1),
                                             (4, 20, [200, 68, 128], 3), (8, 20, [72, 200, 8], 7), (4, 20, [130, 65, 129], 2),
                                             (2, 16, [65, 65, 0], 7)])
def test_fp8_entry_is_bit_identical_to_the_bf16_entry_on_the_dequantised_cache(T, H, lens, splits):
    case = mr.random_case(H, T, lens, seed=T + H + splits)
    c8, c16, table = device_cache(case, True, want_bf16_twin=True)
    got, want = run_multi(case, c8, table, splits), run_multi(case, c16, table, splits)
    assert not torch.isnan(want.float()).any() and same_bits(got, want)
    zero_rows_where_no_key(got, lens, T)
    if splits > 1:
        assert torch.equal(run_multi(case, c8, table, splits, partials=True), run_multi(case, c16, table, splits, partials=True))


# ---------------------------------------------------------------- strided q
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_strided_q_gives_the_contiguous_result(fp8):
    """q_nope and q_pe as slices of one wider buffer, with token and head strides that are not those of a contiguous tensor"""
    T, H, lens = 3, 20, [67, 2, 130]
    case = mr.random_case(H, T, lens, seed=5)
    cache, table = device_cache(case, fp8)
    wide = torch.full((3, T + 1, H + 2, 32 + 576 + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    wide[:, :T, 1 : H + 1, 32 : 32 + 512] = case["q_nope"].cuda()
    wide[:, :T, 1 : H + 1, 32 + 512 : 32 + 576] = case["q_pe"].cuda()
    qn, qp = wide[:, :T, 1 : H + 1, 32 : 32 + 512], wide[:, :T, 1 : H + 1, 32 + 512 : 32 + 576]
    assert not qn.is_contiguous() and qn.stride(1) != H * qn.stride(2) and qn.data_ptr() % 16 == 0 and qp.data_ptr() % 16 == 0
    for splits in (1, 3):
        assert same_bits(run_multi(case, cache, table, splits, q=(qn, qp)), run_multi(case, cache, table, splits))


# ---------------------------------------------------------------- the host's routing to the composition
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_routed_to_the_composition_it_is_the_expanded_single_token_call(fp8):
    """kernel="composed" (what the measured rule picks for small launches): mla_decode on the expanded rows, built by the
    backend or handed in, output and workspace; and the rule itself takes that path for this small shape"""
    T, H, lens = 4, 20, [130, 3, 65]
    case = mr.random_case(H, T, lens, seed=17)
    cache, table = device_cache(case, fp8)
    for splits in (1, 3):
        want = run_expanded(case, cache, table, splits)
        assert same_bits(run_multi(case, cache, table, splits, kernel="composed"), want)
        if splits > 1:
            assert torch.equal(run_multi(case, cache, table, splits, partials=True, kernel="composed"),
                               run_expanded(case, cache, table, splits, partials=True))
    _, _, tab, exp = mr.expand(case, table)
    be = backend(H)
    args = (case["q_nope"].cuda(), case["q_pe"].cuda(), cache, case["lens"].cuda(), table.cuda(), SCALE)
    got = be.mla_decode_multi(*args, num_splits=1, kernel="composed", expanded=(tab.cuda(), exp.cuda())).cpu()
    assert same_bits(got, run_expanded(case, cache, table, 1))
    from chitu_amd import _lib, attn_backend

    assert not attn_backend.mla_multi_beats_composition(len(lens), T, H, table.shape[1])
    _lib.call_log = []
    try:
        by_rule = be.mla_decode_multi(*args).cpu()
        names = [n for n, _ in _lib.call_log]
    finally:
        _lib.call_log = None
    assert names == ["chitu_hip_mla_decode_kv_fp8" if fp8 else "chitu_hip_mla_decode"], names
    assert same_bits(by_rule, run_expanded(case, cache, table, None))  # (the same default split count: sized for bs * T rows)


# ---------------------------------------------------------------- errors
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_argument_errors(fp8):
    from chitu_amd import _lib
    from chitu_amd._lib import f32, i32, i64, ptr, stream_ptr

    H, T = 16, 2
    case = mr.random_case(H, T, [10], seed=1)
    cache, table = device_cache(case, fp8)
    qn, qp, lens, tab = case["q_nope"].cuda(), case["q_pe"].cuda(), case["lens"].cuda(), table.cuda()
    out = torch.zeros(1, T, H, 512, dtype=torch.bfloat16, device="cuda")
    entry = getattr(_lib.lib(), "chitu_hip_mla_decode_multi_kv_fp8" if fp8 else "chitu_hip_mla_decode_multi")

    def call(q_len=T, page=64):
        return entry(ptr(qn), i64(qn.stride(0)), i64(qn.stride(1)), i64(qn.stride(2)), ptr(qp), i64(qp.stride(0)), i64(qp.stride(1)),
                     i64(qp.stride(2)), ptr(cache), i64(cache.shape[0]), i32(page), ptr(tab), i32(tab.stride(0)), ptr(lens), f32(SCALE),
                     ptr(out), i32(1), i32(q_len), i32(H), i32(512), i32(64), i32(1), ctypes.c_void_p(0), i64(0), stream_ptr())

    assert call(q_len=0) == -1 and call(q_len=9) == -1     # CHITU_ERR_BAD_ARG
    assert call(page=96) == -2 and call(page=32) == -2     # CHITU_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(out.any())                             # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(out.any())
    with pytest.raises(ValueError):
        backend(H).mla_decode_multi(torch.zeros(1, 9, H, 512, dtype=torch.bfloat16, device="cuda"),
                                    torch.zeros(1, 9, H, 64, dtype=torch.bfloat16, device="cuda"), cache, lens, tab, SCALE)
