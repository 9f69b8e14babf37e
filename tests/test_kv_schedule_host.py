"""chitu_amd.cache_manager.PagedKVCacheManager over whole schedules on the CPU (device="cpu"), against tests/kv_schedule.py's
PlainCache: after EVERY manager call the page accounting, after every prepare call every device-visible buffer, after every step
the cached rows (torch.equal), for both families and both cache formats.  Appends are plain indexing through the manager's own
tables and lengths (ops.append_to_paged_kv_cache's contract); prefill and continued prefill go through the manager's scatters.
Each test prints what it covered ("KV_SCHEDULE ...", pytest -s).

Mutation table: each line is one edit of a scratch copy of cache_manager.py, the first test of this file that then fails and its
message.  Every edit is caught.
  `_table_rows = None` removed in ...
    __init__                              test_every_call_...[gqa]: "a fresh manager's device table is not marked stale" (AttributeError; no schedule
                                          sees it: every life starts with a prefill or a register, which set the field)
    finalize_cache_bylayer_prefill        test_every_call_...[gqa]: "finalize_cache_bylayer_prefill left _table_rows = ['stale']"
    register_sequence                     test_every_call_...[gqa]: "register_sequence left _table_rows = ['stale']"
    free_req_cache_blocks                 test_every_call_...[gqa]: "finalize_cache_all_decode left _table_rows = ['stale']"
      (through the public methods these three cannot go wrong alone: a request enters `_table_rows` only by a decode step and leaves the
       manager only through free_req_cache_blocks, so a prefill or register of its name follows a free of it and the other of the pair
       still invalidates; the white-box test holds each line by itself)
    prepare_block_table_for_decode_multi  test_schedule[gqa-bf16-random-1]: "single-token step: get_gpu_block_table (step 47): device [[6, 0, 0, 0, 0],
                                          [1, 2, 5, 9, 0]] != oracle [[6, 7, 0, 0, 0], [1, 2, 5, 9, 0]]" (the kept page is missing)
    finalize_cache_multi_decode           test_every_call_...[gqa]: "finalize_cache_multi_decode left _table_rows = ['stale']" (in a schedule the growth of
                                          the same step has invalidated already)
    rollback                              test_schedule[gqa-bf16-random-1]: "single-token step: get_gpu_block_table (step 63): device [[6, 12, 0, 0, 0],
                                          [1, 2, 5, 9, 0]] != oracle [[6, 0, 0, 0, 0], [1, 2, 5, 9, 0]]" (the returned page still shows)
    prepare_cache_prefill_continue        test_schedule[gqa-bf16-random-1]: "single-token step: get_gpu_block_table (step 80): device [[22, 0, 0, 0, 0]] !=
                                          oracle [[22, 25, 18, 0, 0]]"
  `changed = True` removed (the page-boundary append of the single-token step: that path carries no `_table_rows = None`)
                                          test_schedule[gqa-bf16-random-1]: "single-token step: get_gpu_block_table (step 3): device [[0, 0, 0, 0, 0], ...
                                          != oracle [[0, 7, 0, 0, 0], ..."
  `h[:n] = 0` removed in prepare_block_table_for_decode
                                          test_schedule[gqa-bf16-random-1]: "single-token step: get_gpu_block_table (step 17): device [.., [0, 7, 5, 0, 0], ..]
                                          != oracle [.., [0, 7, 0, 0, 0], ..]" (a ring slot's older, longer row shows behind a shorter one)
  `keep` with floor in finalize_cache_multi_decode
                                          test_schedule[gqa-bf16-random-1]: "finalize_cache_multi_decode: request 'd' owns 1 pages for 27 + 0 rows, not 2"
  `keep` with floor in rollback           test_schedule[gqa-bf16-random-1]: "rollback: request 'a' owns 4 pages for 65 + 0 rows, not 5"
  the pre-check of prepare_block_table_for_decode_multi moved behind the page grab
                                          test_a_refused_call_changes_nothing[gqa]: "capacity overrun (multi-token step) changed block_table: {'a': [0],
                                          'b': [1, 2, 3, 4, 5]} -> {'a': [0, 6], 'b': [1, 2, 3, 4, 5, 7]}"
(every schedule of a family catches the same edits; the table names the first case.)

Found by test_a_refused_call_changes_nothing: a multi-token step refused for lack of free pages ("No more free blocks" in the middle
of the grab) kept the pages it had already given to the requests in front -- they then owned more than ceil(len / page) pages for
good.  The single-token step had the same shape ("too few free pages (single-token step) changed block_table", two requests at a
page multiple and one free page), and at a full block table it took a page beyond max_blocks_per_req before numpy refused the
row ("capacity overrun (single-token step) changed block_table").  prepare_block_table_for_decode and
prepare_block_table_for_decode_multi now check every request's capacity and count the pages they need before they take one, as
the continued prefill does."""
import copy

import pytest
import torch

from tests import kv_schedule as ks

CASES = [(f, fmt, n) for f in ks.FAMILIES for fmt in ks.FORMATS for n in ks.SCHEDULE_NAMES]


def test_the_ring_length_is_the_managers():
    from chitu_amd import cache_manager as cm

    assert ks.STAGE_RING == cm._STAGE_RING and max(ks.MULTI_T) == cm.MAX_DECODE_Q


@pytest.mark.parametrize("family,fmt,name", CASES, ids=["-".join(c) for c in CASES])
def test_schedule(family, fmt, name):
    fam = ks.FAMILIES[family]
    d = ks.Driver(fam, fmt)
    d.run(ks.SCHEDULES[family, name])
    assert d.reused, "no page went from a dead request to another one while others stayed live"
    assert d.skipped_copies > 0, "prepare_block_table_for_decode never skipped the table copy"
    print(f"KV_SCHEDULE host {family} {fmt} {name}: {d.step_no} steps, {d.skipped_copies} single-token steps without a table copy, "
          f"every buffer and row equal")


def _state(mgr):
    return dict(seq_lens=dict(mgr.seq_lens), block_table=copy.deepcopy(mgr.block_table), free_blocks=list(mgr.free_blocks),
                table_rows=copy.copy(mgr._table_rows), lens_dev=mgr._lens_dev.clone(), table_dev=mgr.gpu_block_table_buffer.clone())


def _same_state(a, b, what):
    for k in a:
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        assert same, f"{what} changed {k}: {a[k]} -> {b[k]}"


@pytest.mark.parametrize("family", list(ks.FAMILIES))
def test_a_refused_call_changes_nothing(family):
    fam = ks.FAMILIES[family]
    P, cap = fam.page, fam.capacity
    d = ks.Driver(fam, "bf16")
    d.run([("prefill", ["a", "b"], [P - 1, cap - 2]), ("decode", ["a", "b"])])  # a: P, b: cap - 1
    mgr = d.mgr

    def refused(what, exc, call):
        before = _state(mgr)
        with pytest.raises(exc):
            call()
        _same_state(before, _state(mgr), what)
        d.check_pages(what)

    # a needs a page for its 2 tokens, b behind it overruns its table
    refused("capacity overrun (multi-token step)", Exception, lambda: mgr.prepare_block_table_for_decode_multi(["a", "b"], 2))
    refused("capacity overrun (continued prefill)", Exception, lambda: mgr.prepare_cache_prefill_continue(["a", "b"], ks.Lens([P + 1, 2])))
    refused("unknown request (continued prefill)", KeyError, lambda: mgr.prepare_cache_prefill_continue(["a", "zz"], ks.Lens([P + 1, 1])))
    refused("unknown request (rollback)", KeyError, lambda: mgr.rollback(["a", "zz"], [1, 1]))
    refused("unknown request (single-token step)", KeyError, lambda: mgr.prepare_cache_decode(["a", "zz"]))
    refused("unknown request (multi-token step)", KeyError, lambda: mgr.prepare_block_table_for_decode_multi(["a", "zz"], 2))
    refused("rollback below zero", ValueError, lambda: mgr.rollback(["a", "b"], [1, cap]))
    d.run([("decode", ["b"])])  # b: cap, its table is full; a in front of it would take a page
    refused("capacity overrun (single-token step)", Exception, lambda: mgr.prepare_block_table_for_decode(["a", "b"]))
    # too few free pages: more live requests than num_hot_req until one page is left, then a step that needs two
    d.run([("rollback", ["b"], [cap - P])])
    names = []
    while len(mgr.free_blocks) > 1:
        names.append(f"x{len(names)}")
        mgr.register_sequence(names[-1], min(len(mgr.free_blocks) - 1, fam.max_blocks) * P)
    assert len(mgr.free_blocks) == 1
    before = _state(mgr)
    with pytest.raises(Exception, match="free pages"):
        mgr.prepare_cache_prefill_continue(["a", "b"], ks.Lens([1, 1]))
    _same_state(before, _state(mgr), "too few free pages (continued prefill)")
    with pytest.raises(Exception, match="free"):
        mgr.prepare_block_table_for_decode_multi(["a", "b"], 2)
    _same_state(before, _state(mgr), "too few free pages (multi-token step)")
    with pytest.raises(Exception, match="free pages"):
        mgr.prepare_block_table_for_decode(["a", "b"])
    _same_state(before, _state(mgr), "too few free pages (single-token step)")


@pytest.mark.parametrize("family", list(ks.FAMILIES))
def test_every_call_that_changes_a_page_list_marks_the_device_table_stale(family):
    """`_table_rows` names the requests whose rows the device table holds; every call that changes a page list has to reset it,
    each by itself (in a schedule two of them often fall into the same step and hide each other)."""
    fam = ks.FAMILIES[family]
    P = fam.page
    d = ks.Driver(fam, "bf16")
    mgr = d.mgr
    assert getattr(mgr, "_table_rows", "missing") is None, "a fresh manager's device table is not marked stale"
    marks = []
    for st, what, stale in [
        (("prefill", ["a", "b"], [P - 1, P + 3]), "finalize_cache_bylayer_prefill", True),
        (("register", "c", 0), "register_sequence", True),
        (("decode", ["a", "b", "c"]), None, False),                      # a: P, fills its page
        (("rollback", ["a", "b"], [1, 0]), "rollback without a page", False),
        (("rollback", ["b"], [4]), "rollback", True),                     # b: P + 4 -> P
        (("continue", ["c"], [2]), "prepare_cache_prefill_continue inside the page", False),
        (("continue", ["c"], [P]), "prepare_cache_prefill_continue", True),
        (("free", "c"), "finalize_cache_all_decode", True),
    ]:
        mgr._table_rows = ["stale"]
        d.step(st)
        if what is not None:
            assert (mgr._table_rows is None) == stale, f"{what} left _table_rows = {mgr._table_rows}"
            marks.append(what)
    # the multi-token step: its growth and its give-back, one at a time.  a: P - 1, b: P
    mgr._table_rows = ["stale"]
    mgr.prepare_block_table_for_decode_multi(["a"], 2)
    assert mgr._table_rows is None, f"prepare_block_table_for_decode_multi left _table_rows = {mgr._table_rows}"
    mgr._table_rows = ["stale"]
    mgr.finalize_cache_multi_decode(["a"], [1])
    assert mgr._table_rows is None, f"finalize_cache_multi_decode left _table_rows = {mgr._table_rows}"
    print(f"KV_SCHEDULE host {family}: _table_rows reset by {len(marks)} calls where a page list changed, kept where none did")


@pytest.mark.parametrize("family", list(ks.FAMILIES))
def test_a_stale_row_of_a_ring_slot_does_not_show_behind_a_shorter_one(family):
    """_STAGE_RING table copies after a row of three pages the same slot carries a row of one page: the columns behind it are 0"""
    fam = ks.FAMILIES[family]
    P = fam.page
    d = ks.Driver(fam, "bf16")
    d.run([("prefill", ["a", "b"], [2 * P + 1, 3])])
    for i in range(2 * ks.STAGE_RING):  # every step changes the rows, so every step copies: [a, b], [b, a], ...
        d.step(("decode", ["a", "b"] if i % 2 == 0 else ["b", "a"]))
    assert d.skipped_copies == 0


@pytest.mark.parametrize("family", list(ks.FAMILIES))
def test_the_captured_stretch_holds_its_three_events(family):
    """tests/test_gpu_kv_schedule.py replays one captured step over kv_schedule.captured_stretch: here, that it is what it says"""
    fam = ks.FAMILIES[family]
    steps, free_b, admit_d = ks.captured_stretch(fam)
    d = ks.Driver(fam, "fp8")
    crossings, batches = 0, []
    for i, st in enumerate(steps):
        if i == free_b:
            freed = set(d.mgr.block_table["b"])
        if st[0] == "decode":
            assert len(st[1]) == 2
            crossings += any(d.plain.length(r) % fam.page == 0 for r in st[1])
            batches.append(st[1])
        d.step(st)
        if i == admit_d:
            assert freed & set(d.mgr.block_table["d"]), "the newcomer holds none of the pages the leaver freed"
    assert crossings >= 1 and ["a", "b"] in batches and ["a", "d"] in batches and ["d", "a"] in batches
