"""Continued prefill over the paged K / V cache, the host side (no GPU): the case builders of tests/attn_paged_prefill_ref.py
against the fp64 causal attention, the counting precondition, the cache manager's page accounting for continued prefill, the C
entry's declaration, export and argument checks, and the documents' agreement with the header."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests import attn_exact as ax
from tests import attn_paged_prefill_ref as pp
from tests import attn_window_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "chitu_hip_gqa_prefill_paged"


# ---------------------------------------------------------------- the builders
def _whole(case, s):
    """sequence s as one contiguous prefill over all its L rows: the new rows' queries behind zero queries for the prefix"""
    P, n = case["prefixes"][s], case["news"][s]
    cu = pp.cu_q(case)
    q = torch.cat([torch.zeros(P, *case["q"].shape[1:]), case["q"][cu[s] : cu[s + 1]].float()])
    return q, case["K"][s], case["V"][s]


@pytest.mark.parametrize("W,c", [(-1, 0.0), (5, 0.0), (64, 5.0)])
def test_expectation_is_the_causal_prefill_of_the_whole_sequence(W, c):
    """expected64 (decode64 over the first P + i + 1 keys) == prefill64 at P = 0 and rows [P:] of prefill64 on the whole sequence"""
    case = pp.random_case([(0, 33), (0, 1), (17, 31), (64, 2), (130, 5)], 8, 2, seed=1)
    got, cu = pp.expected64(case, W=W, c=c), pp.cu_q(case)
    for s, (P, n) in enumerate(zip(case["prefixes"], case["news"])):
        q, k, v = _whole(case, s)
        if W < 0 and c == 0.0:
            ref = ax.prefill64(q, k, v, [0, P + n], ax.GQA_SCALE)
        else:
            ref = wr.prefill64_window(q, k, v, [0, P + n], ax.GQA_SCALE, W, c)
        assert float((got[cu[s] : cu[s + 1]] - ref[P:]).abs().max()) < 1e-12, (s, P, n)


def test_queries_before_the_first_key_expect_zeros():
    case = pp.random_case([(-3, 5), (-1, 1)], 4, 4, seed=2)  # L = 2 and 0 keys
    want = pp.expected64(case)
    assert not bool(want[:3].any()) and bool(want[3].any()) and bool(want[4].any()) and not bool(want[5].any())


@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (8, 2), (8, 1)])
def test_counting_case_is_the_closed_form_and_keeps_its_precondition(Hq, Hkv):
    """REL_COUNT needs <= 16 keys in any position channel (tests/attn_exact.py)"""
    case = pp.count_case(pp.pairs(), Hq, Hkv)
    assert pp.max_keys_per_position_channel(case) <= 16
    assert float((pp.expected64(case) - case["want"]).abs().max()) < 1e-12
    for W in (0, 5, 64, 100):
        assert pp.max_keys_per_position_channel(case, W) <= 16
        want = pp.count_want_window(case, Hq, W)
        assert float((pp.expected64(case, W=W) - want).abs().max()) < 1e-12
        if W < ax.P_GQA:  # exactly min(W + 1, P + i + 1) keys, one per position channel: each weighs 1 / count
            lens = torch.tensor([L for P, n in zip(case["prefixes"], case["news"]) for L in pp.query_lengths(P, n)])
            count = torch.minimum(lens, torch.tensor(W + 1))
            assert torch.equal((want[:, 0, : ax.P_GQA] != 0).sum(-1), count)
            assert torch.allclose(want[:, 0, : ax.P_GQA].max(-1).values, 1.0 / count.double())


@pytest.mark.parametrize("page", pp.PAGES)
@pytest.mark.parametrize("W", [-1, 5])
def test_dominant_case_expects_what_the_fp64_attention_gives(page, W):
    case = pp.dominant_case(pp.pairs(), 8, 2, page, W)
    ax.check_dominant(pp.expected64(case, W=W), case["want"])
    # and admitting one key past a query's causal edge would be seen
    wrong = dict(case, prefixes=[P + 1 for P in case["prefixes"]], K=[torch.cat([k, k[-1:]]) for k in case["K"]],
                 V=[torch.cat([v, v[-1:]]) for v in case["V"]])
    assert float((pp.expected64(wrong) - case["want"]).abs().max()) >= 1.0
    # the probes name what the issue lists: keys 0, P - 1, P, P + i and both sides of every page and tile edge
    got = {x for x, out in pp.probes_of(200, 33, 32, page) if out is None}
    assert {0, 199, 200, 232} <= got and {e for s in (page, 64) for b in range(s, 233, s) for e in (b - 1, b)} <= got


@pytest.mark.parametrize("page", pp.PAGES)
def test_paginate_scatters_every_row_under_its_table_and_fills_the_rest(page):
    case = pp.random_case([(0, 33), (17, 31), (200, 5)], 4, 2, seed=3)
    nan = float("nan")
    kc, vc, table, lens = pp.paginate(case, page, seed=5, poison_fill=nan)
    assert lens.tolist() == [33, 48, 205]
    used = set()
    for s, L in enumerate(lens.tolist()):
        need = -(-L // page)
        ids = table[s, :need].tolist()
        assert not used & set(ids)
        used |= set(ids)
        rows_k = kc[table[s, :need].long()].flatten(0, 1)
        assert torch.equal(rows_k[:L].float(), case["K"][s]) and bool(rows_k[L:].isnan().all())
        assert torch.equal(vc[table[s, :need].long()].flatten(0, 1)[:L].float(), case["V"][s])
        assert not set(table[s, need:].tolist()) & used and bool(kc[table[s, need:].long()].isnan().all())  # valid spare pages
    spare = set(range(kc.shape[0])) - used
    assert len(spare) == 2 and bool(vc[sorted(spare)].isnan().all())
    # pages wholly before a sequence's lowest visible key keep the fill
    kc, vc, table, _ = pp.paginate(case, page, seed=5, dead_before=pp.lowest_visible(case, 5), poison_fill=nan)
    first = max(0, 200 - 5) // page
    assert bool(kc[table[2, :first].long()].isnan().all()) and not bool(kc[table[2, first].long()][: min(page, 205 - first * page)].isnan().any())


# ---------------------------------------------------------------- the cache manager
def _manager(page=4, max_reqs=3, max_seq_len=40):
    from chitu_amd.cache_manager import PagedKVCacheManager

    return PagedKVCacheManager(0, 2, num_hot_req=max_reqs, block_size=page, max_seq_len=max_seq_len, device="cpu",
                               kv_shape_per_sample=(8,), dtype=torch.bfloat16)


def _varlen(counts):
    return SimpleNamespace(cpu_lens=list(counts))


def _pages_ok(mgr, reqs):
    held = [b for r in reqs for b in mgr.block_table[r]]
    assert len(set(held)) == len(held) and not set(held) & set(mgr.free_blocks)
    assert len(held) + len(mgr.free_blocks) == mgr.num_blocks
    for r in reqs:
        assert len(mgr.block_table[r]) == -(-mgr.seq_lens[r] // mgr.block_size), (r, mgr.seq_lens[r], mgr.block_table[r])


def test_continue_takes_pages_only_up_to_the_new_length_and_rows_cross_page_boundaries():
    mgr = _manager()
    reqs = ["a", "b", "c"]
    for r, n in zip(reqs, (3, 4, 9)):
        mgr.register_sequence(r, n)
    mgr._table_rows = list(reqs)
    free0 = len(mgr.free_blocks)
    news = [6, 1, 3]  # a: 3 -> 9 rows (pages 1 -> 3); b: 4 -> 5 (opens a page); c: 9 -> 12 (stays inside its third page)
    mgr.prepare_cache_prefill_continue(reqs, _varlen(news))
    assert mgr._table_rows is None  # a table grew: the single-token step's device table is stale
    assert [len(mgr.block_table[r]) for r in reqs] == [3, 2, 3] and len(mgr.free_blocks) == free0 - 3
    assert dict(mgr.seq_lens) == {"a": 3, "b": 4, "c": 9}  # the lengths advance at finalize
    assert mgr.get_gpu_continue_seq_lens_incl().tolist() == [9, 5, 12] and mgr.get_gpu_continue_seq_lens_incl().dtype == torch.int32
    assert mgr.get_continue_position_ids().tolist() == [3, 4, 5, 6, 7, 8, 4, 9, 10, 11]
    table = mgr.get_gpu_continue_block_table()
    assert tuple(table.shape) == (3, mgr.max_blocks_per_req) and table.dtype == torch.int32
    for b, r in enumerate(reqs):
        ids = mgr.block_table[r]
        assert table[b, : len(ids)].tolist() == ids and not bool(table[b, len(ids) :].any())
    a, bb, c = (mgr.block_table[r] for r in reqs)
    want_rows = [a[0] * 4 + 3, a[1] * 4, a[1] * 4 + 1, a[1] * 4 + 2, a[1] * 4 + 3, a[2] * 4, bb[1] * 4, c[2] * 4 + 1, c[2] * 4 + 2, c[2] * 4 + 3]
    assert mgr._continue["rows"].tolist() == want_rows
    # the scatter writes exactly those rows, in both layers
    xk = torch.arange(10, dtype=torch.float32).view(10, 1).expand(10, 8).to(torch.bfloat16) + 1
    for layer in (0, 1):
        mgr.finalize_cache_bylayer_prefill_continue(xk, None, layer)
        flat = mgr.paged_kv_cache[layer].view(-1, 8)
        assert flat[want_rows, 0].tolist() == list(range(1, 11)) and int((flat[:, 0] != 0).sum()) == 10
    mgr.finalize_cache_all_prefill_continue(reqs)
    assert dict(mgr.seq_lens) == {"a": 9, "b": 5, "c": 12}
    _pages_ok(mgr, reqs)
    # rollback after a continue restores the page counts
    mgr.rollback(reqs, news)
    assert dict(mgr.seq_lens) == {"a": 3, "b": 4, "c": 9} and len(mgr.free_blocks) == free0
    _pages_ok(mgr, reqs)
    # the single-token step goes on from there
    mgr.prepare_cache_decode(reqs)
    mgr.prepare_block_table_for_decode(reqs)
    mgr.finalize_cache_single_decode(reqs)
    _pages_ok(mgr, reqs)


def test_a_batch_in_which_one_request_does_not_fit_takes_no_page_from_any():
    mgr = _manager()
    mgr.register_sequence("a", 5)
    mgr.register_sequence("b", 4)
    mgr.seq_lens["a"] = mgr.max_blocks_per_req * mgr.block_size - 2
    held, free = {r: list(mgr.block_table[r]) for r in "ab"}, len(mgr.free_blocks)
    with pytest.raises(Exception, match="do not fit"):
        mgr.prepare_cache_prefill_continue(["b", "a"], _varlen([9, 3]))
    assert {r: mgr.block_table[r] for r in "ab"} == held and len(mgr.free_blocks) == free
    # the free list, not a table, is what runs out
    mgr.seq_lens["a"] = 5
    mgr.free_blocks = type(mgr.free_blocks)(list(mgr.free_blocks)[:3])
    with pytest.raises(Exception, match="do not fit"):
        mgr.prepare_cache_prefill_continue(["b", "a"], _varlen([9, 8]))  # 3 + 2 pages
    assert {r: mgr.block_table[r] for r in "ab"} == held and len(mgr.free_blocks) == 3
    mgr.prepare_cache_prefill_continue(["b", "a"], _varlen([9, 3]))  # 3 + 0 pages
    assert len(mgr.free_blocks) == 0
    with pytest.raises(KeyError):
        mgr.prepare_cache_prefill_continue(["nobody"], _varlen([1]))


# ---------------------------------------------------------------- the C entry
def _header():
    return open(os.path.join(ROOT, "include", "chitu_hip.h")).read()


def test_entry_is_in_the_header_with_its_note():
    text = _header()
    assert int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)) >= 13
    assert re.search(r"^int " + ENTRY + r"\s*\(", text, flags=re.M)
    notes = re.findall(r"/\*.*?\*/", text, flags=re.S)
    assert [n for n in notes if ENTRY in n and "attn_backend.py:39-90" in n and "attn_backend.py:92-164" in n and ":294-392" in n
            and "L_s - n_s + i" in n and "bit-identical" in n]
    params = re.search(r"^int " + ENTRY + r"\s*\((.*?)\);", text, flags=re.M | re.S).group(1)
    names = [p.split()[-1].lstrip("*") for p in params.replace("\n", " ").split(",")]
    assert names == ["q_bf16", "q_stride_t", "q_stride_h", "k_cache", "v_cache", "num_pages", "page_size", "kv_heads", "block_table",
                     "table_stride", "cu_seqlens_q", "seqlens_k", "n_seq", "max_seqlen_q", "softmax_scale", "out_bf16", "q_heads",
                     "head_dim", "window_left", "softcap", "stream"]


def test_docs_agree_with_the_header():
    text = _header()
    n = len(re.findall(r"^int chitu_hip_\w+\s*\(", text, flags=re.M))
    version = re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)
    assert (n, version) == (94, "13")
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{n} entry points, ABI version {version}" in readme and "prefill_continue" in readme and ENTRY in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in integ.splitlines() if l.startswith("| 12 → 13 |")]
    assert len(row) == 1 and ENTRY in row[0]
    assert "3.11" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert ENTRY in open(os.path.join(ROOT, "chitu_amd", "attn_backend.py")).read()


def _cdll():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_the_entry():
    assert hasattr(_cdll(), ENTRY)


def test_entry_checks_its_arguments_on_the_host():
    """Nothing is launched (n_seq 0, or refused before the launch; the pointers are never dereferenced), so this needs no GPU."""
    entry = getattr(_cdll(), ENTRY)
    buf = ctypes.create_string_buffer(128)
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    BAD_ARG, UNSUPPORTED = -1, -2

    def call(W=-1, c=0.0, hd=128, hq=32, hkv=8, st=4096, sh=128, page=16, ts=4, n_seq=0, q=p, kc=p, vc=p, out=p, pages=4):
        return entry(q, i64(st), i64(sh), kc, vc, i64(pages), i32(page), i32(hkv), p, i32(ts), p, p, i32(n_seq), i32(64), f32(0.1), out,
                     i32(hq), i32(hd), i32(W), f32(c), None)

    assert call() == 0 and call(W=0, c=5.0) == 0 and call(W=2 ** 31 - 1) == 0 and call(page=48) == 0
    assert all(call(hq=g, hkv=1) == 0 for g in (1, 2, 4, 8, 16, 32))
    # every refusal comes before the launch: n_seq = 3 with pointers that must not be dereferenced
    for n_seq in (0, 3):
        assert call(W=-2, n_seq=n_seq) == BAD_ARG and call(c=-1.0, n_seq=n_seq) == BAD_ARG and call(c=float("nan"), n_seq=n_seq) == BAD_ARG
        assert call(st=4100, n_seq=n_seq) == BAD_ARG and call(sh=132, n_seq=n_seq) == BAD_ARG
        assert call(ts=0, n_seq=n_seq) == BAD_ARG and call(hq=30, n_seq=n_seq) == BAD_ARG and call(pages=0, n_seq=n_seq) == BAD_ARG
        off = ctypes.c_void_p(base + 8)
        assert all(call(n_seq=n_seq, **{name: off}) == BAD_ARG for name in ("q", "kc", "vc", "out"))
        assert call(q=None, n_seq=n_seq) == BAD_ARG
        assert call(hd=64, n_seq=n_seq) == UNSUPPORTED and call(page=24, n_seq=n_seq) == UNSUPPORTED and call(page=0, n_seq=n_seq) == UNSUPPORTED
        assert call(hq=64, hkv=1, n_seq=n_seq) == UNSUPPORTED and call(hq=24, hkv=8, n_seq=n_seq) == UNSUPPORTED  # G = 64, G = 3


# ---------------------------------------------------------------- the Python layers
def test_backend_and_decoder_have_the_new_methods():
    import inspect

    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.llama import LlamaAttention, LlamaDecoder
    from chitu_amd.mixtral import MixtralDecoder

    sig = inspect.signature(HipAttnBackend.attn_varlen_with_kvcache)
    assert list(sig.parameters) == ["self", "q", "k_cache", "v_cache", "cu_seqlens_q", "cache_seqlens", "block_table", "max_seqlen_q",
                                    "causal", "window_size", "softcap", "softmax_scale"]
    assert sig.parameters["causal"].default is True and sig.parameters["window_size"].default == (-1, -1)
    assert callable(LlamaAttention.prefill_forward_paged) and callable(LlamaDecoder.prefill_continue)
    assert MixtralDecoder.prefill_continue is LlamaDecoder.prefill_continue
    assert inspect.signature(LlamaDecoder.prefill).parameters["chunk_size"].default is None
    assert inspect.signature(LlamaDecoder.generate).parameters["prefill_chunk_size"].default is None
