"""The beyond-4-GiB cases of tests/big_cache.py on the CPU: every reader case of tests/test_gpu_big_cache.py holds its closed
form through the fp64 oracle at low page ids; the high-page layout puts every named row in (2^32, 2^32 + 2^31) bytes with its
32-bit alias in the guard set; and a table whose ids are replaced by their alias pages -- a kernel that wrapped -- fails every
reader case and leaves every writer's named row unchanged.  Prints each oracle error ("BIG_CACHE oracle ...", pytest -s)."""
import pytest
import torch

from tests import attn_exact as ax
from tests import big_cache as bc
from tests import test_gqa_kv_fp8_host as g8
from tests import test_mla_kv_fp8_host as m8

GEOMETRIES = {  # name -> (page, page bytes)
    "gqa bf16": (bc.GQA_PAGE, bc.GQA_PAGE * bc.GQA_HKV * 128 * 2),
    "gqa fp8": (bc.GQA_PAGE, bc.GQA_PAGE * bc.GQA_HKV * g8.ROW),
    "gqa bf16, 2 KV heads": (bc.GQA_PAGE, bc.GQA_PAGE * bc.ANY_HKV * 128 * 2),
    "mla bf16": (bc.MLA_PAGE, bc.MLA_PAGE * 576 * 2),
    "mla fp8": (bc.MLA_PAGE, bc.MLA_PAGE * m8.ROW),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_every_named_row_lies_past_4gib_and_its_alias_in_the_guard_set(name):
    page, pb = GEOMETRIES[name]
    n = 48
    named, alias, guard = bc.high_layout(pb, n)
    low = bc.low_pages(pb, n)
    offs = bc.row_offsets(named, page, pb)
    assert min(offs) > 2 ** 32 and max(offs) + pb // page < 2 ** 32 + 2 ** 31
    for p, a in zip(named, alias):
        assert a == ((p * pb) % 2 ** 32) // pb and a in guard and a not in named and a < named[0]
    for off in offs:  # a row's cut offset, its first and last byte, lands in a guard page
        assert (off % 2 ** 32) // pb in guard and ((off + pb // page - 1) % 2 ** 32) // pb in guard
    assert 0 in guard and not set(low) & set(guard) and not set(low) & set(named) and max(low) < named[0]
    assert max(named) * pb > 2 ** 32  # the thresholds of the older tests' docstrings
    if name == "gqa bf16":
        assert named[0] == 8193
    if name == "mla bf16":
        assert named[0] == 58255


def small_scene(fam, fp8, cases):
    """CPU caches just large enough for the guard set and the low pages; (caches, low ids, alias ids, guard)"""
    page = bc.GQA_PAGE if fam == "gqa" else bc.MLA_PAGE
    fills = bc.FILLS_GQA if fam == "gqa" else bc.FILLS_MLA
    hkv = cases[0]["seqs"][0][0].shape[1] if fam == "gqa" else None
    sentinels = [bc.sentinel_page(fam, fp8, page, f, hkv) for f in fills]
    n = bc.assign_slots(cases, page)
    pb = sentinels[0].numel() * sentinels[0].element_size()
    _, alias, guard = bc.high_layout(pb, n)
    low = bc.low_pages(pb, n)
    caches = [s.unsqueeze(0).repeat(max(low) + 1, *[1] * s.dim()) for s in sentinels]  # decoys everywhere
    for c in cases:
        bc.place_case(caches, c, low, bc.quant_of(fam, fp8))
    return caches, low, alias, guard


def run_cases(fam, fp8, cases):
    caches, low, alias, guard = small_scene(fam, fp8, cases)
    num_pages = caches[0].shape[0]
    for c in cases:
        def table(ids):
            return bc.gather_table(c, ids, num_pages) if c["entry"] == "gather" else bc.table_of(c, ids)

        err = bc.check(c, bc.oracle_run(c, caches, table(low)), fp8)
        print(f"BIG_CACHE oracle {fam} {'fp8 ' if fp8 else ''}{c['name']}: {err:.3e}")
        with pytest.raises(AssertionError):  # the table of a kernel that cut its offsets to 32 bits: decoy rows
            bc.check(c, bc.oracle_run(c, caches, table(alias)), fp8)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_gqa_reader_cases_hold_at_low_pages_and_fail_through_the_alias_table(fp8):
    run_cases("gqa", fp8, [c for c in bc.gqa_reader_cases() if not (fp8 and c["entry"] == "prefill")])


def test_gqa_any_group_prefill_cases_hold_and_fail_through_the_alias_table():
    run_cases("gqa", False, bc.gqa_reader_cases(bc.ANY_HQ, bc.ANY_HKV, prefill_only=True))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_mla_reader_cases_hold_at_low_pages_and_fail_through_the_alias_table(fp8):
    run_cases("mla", fp8, bc.mla_reader_cases())


def test_counting_bars_precondition():
    """REL_COUNT needs <= 16 permitted keys in any position channel of every counting case"""
    for c in bc.gqa_reader_cases():
        if c["kind"] == "count":
            assert max(ax.max_keys_per_position_channel(v, ax.P_GQA) for _, v in c["seqs"]) <= 16
    for c in bc.mla_reader_cases():
        if c["kind"] == "count":
            assert ax.max_keys_per_position_channel(c["seqs"][0][0][:, :512].unsqueeze(1), ax.P_MLA) <= 16


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
@pytest.mark.parametrize("T", [1, 3])
def test_a_writer_that_wraps_misses_its_named_row_and_changes_a_guard_page(name, T):
    """the append stated on the CPU (big_cache.write_oracle) through the alias table: the named rows keep their decoys, and what
    the GPU tests compare after every writer -- the guard set -- differs"""
    page, pb = GEOMETRIES[name]
    row = pb // page
    _, alias, guard = bc.high_layout(pb, 6)
    low = bc.low_pages(pb, 6)
    cache = torch.full((max(low) + 1, page, row), 7, dtype=torch.uint8)
    old, positions = bc.writer_positions(page, T)
    assert {pos // page for _, pos in positions} == {0, 1}  # both pages of a sequence, and (T = 3) one sequence across the edge
    new = torch.arange(len(positions) * row, dtype=torch.int64).view(len(positions), row).remainder(200).to(torch.uint8) + 8
    before = cache.clone()
    bc.write_oracle(cache, bc.writer_table(alias), positions, new)
    assert torch.equal(cache[low], before[low]), "the wrapped writer reached its named rows"
    assert not torch.equal(cache[guard], before[guard])
    bc.write_oracle(cache.copy_(before), bc.writer_table(low), positions, new)
    assert torch.equal(cache[guard], before[guard]) and not torch.equal(cache[low], before[low])


def writer_cases():
    out = [("gqa", False, c) for c in bc.gqa_writer_cases(False)] + [("gqa", True, c) for c in bc.gqa_writer_cases(True)]
    return out + [("mla", False, c) for c in bc.mla_writer_cases()]


@pytest.mark.parametrize("fam,fp8,case", writer_cases(), ids=lambda v: v["name"].replace(" ", "-") if isinstance(v, dict) else str(v))
def test_every_writer_cases_rows_land_in_the_named_pages_and_a_wrapped_writer_shows(fam, fp8, case):
    """Each writer case's expected rows (the central candidate where the builder gives rsqrtf candidates) through the append stated
    on the CPU, on a small cache of decoys: through the low table exactly the named rows hold them, bit for bit, and no guard page
    changes; through the alias table -- the writer that wrapped -- the named rows keep their decoys, which differ from every
    expected row, and a guard page changes: assertions (a) and (c) of the GPU test both fail."""
    page = bc.GQA_PAGE if fam == "gqa" else bc.MLA_PAGE
    sentinels = [bc.sentinel_page(fam, fp8, page, f) for f in (bc.FILLS_GQA if fam == "gqa" else bc.FILLS_MLA)]
    pb = sentinels[0].numel() * sentinels[0].element_size()
    _, alias, guard = bc.high_layout(pb, 6)
    low = bc.low_pages(pb, 6)
    _, positions = bc.writer_positions(page, 1)
    for s, want in zip(sentinels, case["want_rows"]):
        rows = bc._first(want)
        assert rows.dtype == s.dtype and tuple(rows.shape[1:]) == tuple(s.shape[1:])
        fresh = s.unsqueeze(0).repeat(max(low) + 1, *[1] * s.dim())
        named_rows = lambda c: torch.stack([c[low[bc.WRITER_SLOTS[b][pos // page]], pos % page] for b, pos in positions])
        good = bc.write_oracle(fresh.clone(), bc.writer_table(low), positions, rows)
        assert torch.equal(named_rows(good).view(torch.uint8), rows.view(torch.uint8)) and torch.equal(good[guard], fresh[guard])
        keep = torch.ones(good.shape[:2], dtype=torch.bool)
        for b, pos in positions:
            keep[low[bc.WRITER_SLOTS[b][pos // page]], pos % page] = False
        assert torch.equal(good[keep], fresh[keep]), "the oracle changed a row that is not addressed"
        wrapped = bc.write_oracle(fresh.clone(), bc.writer_table(alias), positions, rows)
        assert torch.equal(wrapped[low], fresh[low]) and not torch.equal(wrapped[guard], fresh[guard])
        for got, r in zip(named_rows(wrapped), rows):  # the decoy a wrapped writer leaves is no expected row
            assert not torch.equal(got.view(torch.uint8), r.view(torch.uint8))
