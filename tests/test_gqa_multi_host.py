"""Multi-token GQA decode, the host side (no GPU): the equivalence the GPU tests rest on against the reference's own outputs
(tests/golden/attn_multi.npz), the case builders of tests/attn_multi_ref.py against the fp64 attention, the two C entries'
declarations and argument checks, the cache manager's page accounting for multi-token steps, and NgramDrafter."""
import ctypes
import os
import re

import pytest
import torch

from tests import attn_exact as ax
from tests import attn_multi_ref as mr
from tests import attn_window_ref as wr
from tests.util import assert_close, bf16, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("chitu_hip_gqa_decode_multi", "chitu_hip_gqa_decode_multi_kv_fp8")


# ---------------------------------------------------------------- the equivalence, pinned to the reference
@pytest.mark.parametrize("T", mr.FIXM_T)
def test_single_token_attention_on_expanded_rows_is_the_reference_multi_token_attention(T):
    """RefAttnBackend._attention(causal=True, seqlen_q = T) stored in the fixture == the fp64 single-token attention of
    tests/attn_window_ref.py on the rows (b, t) with lengths L - T + t + 1.  The fixture is the reference's fp32 result rounded
    to bf16 (half an ulp, 2^-9 of the value); the bar is twice that, of the peak."""
    g = golden("attn_multi")
    inp = mr.fixture_multi_inputs(T)
    B = inp["q"].shape[0]
    exp = mr.expanded_lengths(inp["lens"].tolist(), T)
    for W in mr.FIXM_WINDOWS:
        for c in mr.FIXM_CAPS:
            ref = bf16(g[mr.fixture_multi_key(T, W, c)]).view(B * T, mr.FIXM_HQ, 128)
            for b in range(B):  # every sequence has its own rows
                rows = slice(b * T, (b + 1) * T)
                got = wr.decode64_window(inp["q"][b].float(), inp["K"][b].float(), inp["V"][b].float(), exp[rows], ax.GQA_SCALE, W, c)
                assert_close(got, ref[rows], 2.0 ** -8, what=("equivalence", T, W, c, b))


def test_fixture_holds_a_query_that_sees_only_the_new_rows():
    """attended length == T: query t sees t + 1 keys, query 0 only its own"""
    for T in mr.FIXM_T:
        assert mr.expanded_lengths(mr.fixture_multi_lengths(T), T)[:T] == list(range(1, T + 1))
    assert mr.expanded_lengths([0, 1, 5], 3) == [0, 0, 0, 0, 0, 1, 3, 4, 5]


# ---------------------------------------------------------------- the builders
@pytest.mark.parametrize("W", [-1, 1, 17])
def test_dominant_case_expects_what_the_fp64_attention_gives(W):
    for (Hq, Hkv), (n, T, page) in zip(mr.MULTI_HEADS[:3], ((70, 4, 16), (130, 5, 48), (67, 8, 16))):
        c = mr.multi_dominant_case(n, T, Hq, Hkv, page, mr.MULTI_SPLITS, W)
        bs = c["q"].shape[0]
        got = wr.decode64_window(c["q"].float().view(bs * T, Hq, 128), c["K"], c["V"], mr.expanded_lengths([n] * bs, T), ax.GQA_SCALE, W)
        ax.check_dominant(got, c["want"])
        # and admitting one key past a query's range (the next draft token's) would be seen
        wrong = wr.decode64_window(c["q"].float().view(bs * T, Hq, 128), c["K"], c["V"],
                                   [min(x + 1, n) for x in mr.expanded_lengths([n] * bs, T)], ax.GQA_SCALE, -1)
        assert float((wrong - c["want"]).abs().max()) >= 1.0


def test_counting_precondition_holds_on_expanded_lengths():
    """REL_COUNT needs <= 16 keys in any position channel (tests/attn_exact.py); the expanded lengths stay within the builders' range"""
    for Hq, Hkv in mr.MULTI_HEADS:
        c = ax.gqa_count_case(mr.COUNT_N, Hq, Hkv, lengths=mr.expanded_lengths(range(mr.COUNT_N + 1), 8))
        assert ax.max_keys_per_position_channel(c["V"], ax.P_GQA) <= 16 and int(c["lens"].max()) == mr.COUNT_N
        assert int((c["lens"] == 0).sum()) == sum(min(8, 8 - L) for L in range(8))  # the queries before the first key


def test_graded_case_straddles_the_deferral_constant():
    defer = ax.source_constant("gqa_decode_tile.h", "kGqaDefer")
    ks, leads = ax.graded_amplitudes(defer, ax.GQA_SCALE)
    assert leads[0] < defer < leads[1]
    c = mr.multi_graded_case(130, 4, 8, 2, ks, tokens=[5, 120], probing_t=1)
    assert c["want"].shape == (4 * 4, 8, 128) and bool(torch.isfinite(c["want"]).all())


# ---------------------------------------------------------------- the C entries
def _header():
    return open(os.path.join(ROOT, "include", "chitu_hip.h")).read()


def test_entries_are_in_the_header_with_their_note_and_abi_version_9():
    text = _header()
    assert int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)) >= 9
    notes = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M)
        assert [n for n in notes if name in n and "attn_backend.py:92-164" in n and "q_len" in n and "L - T + t" in n], name
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in integ.splitlines() if l.startswith("| 8 → 9 |")]
    assert len(row) == 1 and all(name in row[0] for name in ENTRIES)


def _cdll():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_entries_check_their_arguments_on_the_host():
    """Nothing is launched (batch 0; the pointers are never dereferenced), so this needs no GPU."""
    lib = _cdll()
    buf = ctypes.create_string_buffer(128)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    BAD_ARG, UNSUPPORTED = -1, -2
    for name in ENTRIES:
        entry = getattr(lib, name)

        def call(T=4, W=-1, c=0.0, hd=128, splits=1, hq=32, hkv=8, st=4096, page=16):
            return entry(p, i64(4 * 4096), i64(st), i64(128), p, p, i64(4), i32(page), i32(hkv), p, i32(4), p, f32(0.1), p, i32(0), i32(T),
                         i32(hq), i32(hd), i32(splits), p, i64(0), i32(W), f32(c), None)

        assert all(call(T=T) == 0 for T in range(1, 9)) and call(W=0, c=5.0) == 0 and call(W=2 ** 31 - 1) == 0
        assert call(T=0) == BAD_ARG and call(T=9) == BAD_ARG and call(T=-1) == BAD_ARG
        assert call(W=-2) == BAD_ARG and call(c=-1.0) == BAD_ARG and call(c=float("nan")) == BAD_ARG
        assert call(st=4100) == BAD_ARG and call(splits=0) == BAD_ARG and call(splits=257) == BAD_ARG and call(hq=30) == BAD_ARG
        assert call(hd=64) == UNSUPPORTED and call(hq=32, hkv=1) == UNSUPPORTED and call(page=24) == UNSUPPORTED


# ---------------------------------------------------------------- the cache manager
def _manager(page=4, max_reqs=3, max_seq_len=40):
    from chitu_amd.cache_manager import PagedKVCacheManager

    return PagedKVCacheManager(0, 1, num_hot_req=max_reqs, block_size=page, max_seq_len=max_seq_len, device="cpu",
                               kv_shape_per_sample=(8,), dtype=torch.bfloat16)


def _pages_ok(mgr, reqs):
    held = [b for r in reqs for b in mgr.block_table[r]]
    assert len(set(held)) == len(held) and not set(held) & set(mgr.free_blocks)
    assert len(held) + len(mgr.free_blocks) == mgr.num_blocks and len(set(mgr.free_blocks)) == len(mgr.free_blocks)
    for r in reqs:
        assert len(mgr.block_table[r]) == -(-mgr.seq_lens[r] // mgr.block_size), (r, mgr.seq_lens[r], mgr.block_table[r])


def test_multi_token_steps_keep_the_page_accounting():
    mgr = _manager()
    reqs = ["a", "b", "c"]
    for r, n in zip(reqs, (3, 4, 9)):
        mgr.register_sequence(r, n)
    _pages_ok(mgr, reqs)
    lens = dict(mgr.seq_lens)
    for T, accepted in ((4, [1, 4, 2]), (8, [8, 1, 1]), (2, [2, 2, 1]), (5, [1, 1, 5])):
        mgr.prepare_block_table_for_decode_multi(reqs, T)
        for r in reqs:  # room for all T rows while the step runs
            assert len(mgr.block_table[r]) == -(-(lens[r] + T) // mgr.block_size)
        rows, incl, table = mgr.get_gpu_multi_row_lens(), mgr.get_gpu_multi_seq_lens_incl(), mgr.get_gpu_multi_block_table()
        assert rows.tolist() == [lens[r] + t for r in reqs for t in range(T)] and incl.tolist() == [lens[r] + T for r in reqs]
        assert tuple(table.shape) == (len(reqs) * T, mgr.max_blocks_per_req)
        for b, r in enumerate(reqs):
            ids = mgr.block_table[r]
            for t in range(T):
                assert table[b * T + t, : len(ids)].tolist() == ids and not bool(table[b * T + t, len(ids) :].any())
        assert table[::T].stride(0) == T * mgr.max_blocks_per_req  # what the attention reads: one row per sequence, no copy
        mgr.finalize_cache_multi_decode(reqs, accepted)
        for r, a in zip(reqs, accepted):
            lens[r] += a
        assert dict(mgr.seq_lens) == lens
        _pages_ok(mgr, reqs)
    # the single-token step goes on from there: its invariant held
    mgr.prepare_cache_decode(reqs)
    mgr.prepare_block_table_for_decode(reqs)
    assert mgr.get_gpu_block_table().tolist() == [mgr.block_table[r] + [0] * (mgr.max_blocks_per_req - len(mgr.block_table[r])) for r in reqs]
    mgr.finalize_cache_single_decode(reqs)
    _pages_ok(mgr, reqs)
    for r in reqs:
        mgr.finalize_cache_all_decode(r)
    assert sorted(mgr.free_blocks) == list(range(mgr.num_blocks))


def test_multi_token_buffers_are_persistent_and_the_arguments_are_checked():
    mgr = _manager()
    mgr.register_sequence("a", 5)
    mgr.prepare_block_table_for_decode_multi(["a"], 4)
    ptrs = (mgr.get_gpu_multi_row_lens().data_ptr(), mgr.get_gpu_multi_block_table().data_ptr())
    mgr.finalize_cache_multi_decode(["a"], [3])
    mgr.prepare_block_table_for_decode_multi(["a"], 4)
    assert ptrs == (mgr.get_gpu_multi_row_lens().data_ptr(), mgr.get_gpu_multi_block_table().data_ptr())  # a captured step replays on them
    assert mgr.get_gpu_multi_row_lens().tolist() == [8, 9, 10, 11]
    for bad in ([0], [5]):
        with pytest.raises(AssertionError):
            mgr.finalize_cache_multi_decode(["a"], bad)
    with pytest.raises(AssertionError):
        mgr.prepare_block_table_for_decode_multi(["a"], 9)
    mgr.finalize_cache_multi_decode(["a"], [4])
    mgr.seq_lens["a"] = mgr.max_blocks_per_req * mgr.block_size - 2
    with pytest.raises(Exception, match="do not fit"):
        mgr.prepare_block_table_for_decode_multi(["a"], 4)
    # a step that one request cannot take takes no page from any: the others keep ceil(len / block) pages
    mgr.register_sequence("b", 4)
    held, free = list(mgr.block_table["b"]), len(mgr.free_blocks)
    with pytest.raises(Exception, match="do not fit"):
        mgr.prepare_block_table_for_decode_multi(["b", "a"], 4)
    assert mgr.block_table["b"] == held and len(mgr.free_blocks) == free


# ---------------------------------------------------------------- the drafter
def test_ngram_drafter_continues_the_latest_earlier_occurrence():
    from chitu_amd.sampling import NgramDrafter

    d = NgramDrafter(2)
    assert d.propose([1, 2, 3, 4, 1, 2], 3) == [3, 4, 1]
    assert d.propose([1, 2, 9, 1, 2, 8, 1, 2], 2) == [8, 1]          # the latest occurrence, not the first
    assert d.propose([1, 2, 3, 1, 2], 4) == [3, 1, 2, 2]             # the continuation ends with the history: its last token repeats
    assert d.propose([1, 2, 3], 2) == [3, 3] and d.propose([7], 3) == [7, 7, 7]  # no earlier occurrence / too short
    assert d.propose([5, 5, 5, 5], 3) == [5, 5, 5] and d.propose([1, 2, 3], 0) == []
    assert NgramDrafter(1).propose([4, 6, 4], 2) == [6, 4] and NgramDrafter(3).propose([1, 2, 3, 9, 1, 2, 3], 1) == [9]
    assert all(isinstance(t, int) for t in d.propose(torch.tensor([1, 2, 3, 1, 2]).tolist(), 3))
    with pytest.raises(ValueError):
        NgramDrafter(0)
