"""tests/sample_exact.py against the specification, on the CPU: every builder's expected values through
oracle.sampling.sample_fixed_point, every "reach" record through the two path models (sample_candidate_model, None = falls back,
and sample_radix_model) and the numpy traces that expose their intermediates, the closed forms, the margin condition of the
logits-space cases and the special-value rows.  A case that no longer reaches its recorded path, level, clause, bin or segment
fails here, without a GPU."""

import numpy as np
import pytest
import torch

from oracle import sampling as osmp
from tests import sample_exact as se
from tests import spec_verify_ref as sv


def _traces(case):
    """per draw: cand_trace and radix_trace merged (the list's own n_kept under n_kept_list)"""
    out, cache = [], {}
    for k, p, u in case.draws:
        if (k, p) not in cache:
            cache[(k, p)] = se.cand_trace(case.row, k, p)
        t = dict(se.radix_trace(case.row, k, p, u))
        t.update(cache[(k, p)])
        out.append(t)
    return out


@pytest.mark.parametrize("name", list(se.GROUPS))
def test_expected_values_are_the_specifications(name):
    for case in se.group(name):
        want = case.expected()
        for i, (k, p, u) in enumerate(case.draws):
            tok, n, mass = osmp.sample_fixed_point(case.row, 1.0, k, p, u, probs_mode=True)
            assert (tok, n) == want[i][:2], (case.name, i, case.draws[i])
            assert mass == want[i][2] / want[i][3]
            if case.closed is not None and case.closed[i] is not None:
                c_tok, c_n = case.closed[i]
                assert c_tok is None or c_tok == tok, (case.name, i, c_tok, tok)
                assert c_n is None or c_n == n, (case.name, i, c_n, n)


@pytest.mark.parametrize("name", list(se.GROUPS))
def test_every_draw_reaches_what_it_records(name):
    for case in se.group(name):
        want = case.expected()
        traces = _traces(case)
        # thin the largest vocabulary's model runs: the models are Python loops over the row (every draw still has its trace)
        step = 1 if case.row.size <= 8191 else 3
        for i, (k, p, u) in enumerate(case.draws):
            t = traces[i]
            for field, value in case.reach[i].items():
                assert t.get(field) == value, (case.name, i, case.draws[i], field, t.get(field), value)
            assert (t["token"], t["n_kept"]) == want[i][:2], (case.name, i)
            if i % step:
                continue
            model = osmp.sample_candidate_model(case.row, 1.0, k, p, u, probs_mode=True)
            assert (model is None) == (t["path"] == "radix"), (case.name, i, case.draws[i], t["path"])
            if model is not None:
                assert model == want[i][:2]
            assert osmp.sample_radix_model(case.row, 1.0, k, p, u, probs_mode=True) == want[i][:2], (case.name, i)


def test_capacity_edges_fall_where_the_kernel_text_says():
    """counts[j] <= kCandCap, key >= threshold: 1024 at the threshold with top_k 1024 stays on the list; top_k 1025, 1023 entries
    with top_k 1024 and 1025 entries fall back; one ulp below the threshold the entries count for the next level only"""
    by = {c.name: c for c in se.group("A1")}

    def path(name, k, p):
        return se.cand_trace(by[name].row, k, p)["path"]

    assert path("A1-at-1024", 1024, 1.0) == "list" and path("A1-at-1024", 1025, 1.0) == "radix"
    assert path("A1-at-1023", 1024, 1.0) == "radix" and path("A1-at-1023", 10, 1.0) == "list"
    assert all(path("A1-at-1025", k, p) == "radix" for k, p in ((10, 1.0), (1024, 1.0), (1025, 1.0), (-1, 0.5)))
    assert se.cand_trace(by["A1-at-1024"].row, 10, 1.0)["counts"] == [1024] * 5
    assert se.cand_trace(by["A1-below-1024"].row, 10, 1.0)["counts"] == [1, 1024, 1024, 1024, 1024]
    assert se.cand_trace(by["A1-below-1025"].row, 10, 1.0)["level"] == 0


def test_the_case_list_covers_every_edge():
    levels, alone, lengths, npows = set(), set(), set(), set()
    for name in ("A1", "A2", "A3", "A4", "A5", "A6"):
        for case in se.group(name):
            for t in _traces(case):
                if t["path"] == "list":
                    levels.add(t["level"])
                    lengths.add(t["n_cand"])
                    npows.add(max(64, 1 << (t["n_cand"] - 1).bit_length()))
                if t.get("clauses") is not None:
                    alone.add(t["clauses"])
    assert levels == {0, 1, 2, 3, 4}
    assert {(False, True, False, False), (False, False, True, False), (False, False, False, True), (False,) * 4,
            (True, True, False, False), (True, False, True, False)} <= alone
    assert not any(c[0] and not (c[1] or c[2]) for c in alone)  # clause 1 is never true alone
    assert {1, 2, 63, 64, 65, 128, 129, 1024} <= lengths and npows == {64, 128, 256, 1024}
    # radix: every level resolves a pair, segments / chunks / lanes / slots of the rescan
    taus = [r["tau"] for r in se.group("B1")[0].reach]
    assert {0x3E9003FF ^ 0x3E900400} == {0x7FF} and 0x3E900400 in taus  # bin 1023 of one level-3 histogram, bin 0 of the next
    for case in se.group("B2"):
        sl = se.seg_len_of(case.row.size)
        tr = _traces(case)
        toks = {t["token"] for t in tr}
        ks = {d[0] for d in case.draws}
        assert ks == {k for k in (sl, sl + 1, sl + 2, 2 * sl + 1, case.row.size) if 1 < k <= case.row.size}
        edges = {e for e in range(256, max(ks), 256)}
        assert all(e - 1 in toks and e in toks for e in edges)
        assert {(t["lane"], t["slot"]) for t in tr} >= {(l, s) for l in (0, 63) for s in range(4)}
        if case.row.size > 256:
            assert {t["seg"] for t in tr} >= {0, 1} and any(t["ties_before_seg"] for t in tr)
    for name in ("B3", "B6"):
        case = se.group(name)[0]
        tr = _traces(case)
        n_seg = -(-case.row.size // se.seg_len_of(case.row.size))
        assert {t["seg"] for t in tr} >= {0, 3, 4, n_seg - 2, n_seg - 1}
        assert any(t["seg"] > 3 and t["ties_before_seg"] > t["c_keep"] for t in tr)  # a draw behind the exhausted tie quota
    assert {t["keep_all"] for t in _traces(se.group("B4")[0])} == {True, False}
    assert {t["tau"] for t in _traces(se.group("B5")[0])} == {0, se.key_of(se.p2(41))}
    assert se.group("B6")[0].row.size == 32773 and any(t["token"] >= 32768 for c in se.group("B6") for t in _traces(c))


@pytest.mark.parametrize("name", se.VERIFY_GROUPS)
def test_verification_rows(name):
    for case in se.group(name):
        v = se.verify_rows(case)
        rows = len(v["drafts"])
        assert rows % 2 == 0 and v["drafts"][1::2] == [-1] * (rows // 2) and all(d >= 0 for d in v["drafts"][0::2])
        assert v["tokens"][1::2] == v["bonus_want"] and not any(v["accepted"][1::2])
        assert 0 < sum(v["accepted"]) < rows // 2  # both branches
        if case.row.size <= 4099:  # the rule from scratch, row by row
            acc, tok, out = sv.verify([case.row] * rows, 2, [1.0] * rows, v["top_ks"], v["top_ps"], v["drafts"], v["uniforms"], True)
            assert [int(a) for a in acc] == v["accepted"] and tok == v["tokens"] and np.array_equal(out, v["out"])
        # the draft kinds: a kept tie, a dropped tie of the same weight (B2 / B3 / A5 below the 40th), a token outside
        kinds = set()
        for k, p, d in zip(v["top_ks"][0::2], v["top_ps"][0::2], v["drafts"][0::2]):
            kw = case.kw(k, p)
            kinds.add("kept" if kw["mask"][d] else ("tie-dropped" if case.row[d] == case.row[kw["mask"]].min() else "outside"))
        assert "kept" in kinds and (case.name == "B2-equal-256" or "tie-dropped" in kinds)


def test_logits_cases_keep_their_margins():
    cases = se.logits_cases()
    assert {(c.x.size, c.temperature) for c in cases} == {(v, t) for v in se.LOGIT_VOCABS for t in se.TEMPERATURES}
    admitted = 0
    for c in cases:
        assert np.array_equal(c.x * 8, np.round(c.x * 8)) and float(np.abs(c.x).max()) <= 16
        assert np.array_equal(c.x.astype(np.float16).astype(np.float32), c.x)
        assert np.array_equal(se.from_bits(se.to_bits(c.x, "bfloat16"), "bfloat16"), c.x)
        assert len(c.draws) >= 2, c.name
        x_t = (c.x / np.float32(c.temperature)).astype(np.float32)
        gaps = np.diff(np.unique(x_t))
        assert gaps.size == 0 or float(gaps.min()) >= 1 / 16 - 1e-6  # distinct logits: >= 1/16 nat apart
        twin = c.twin()
        assert float(twin.max()) == 1.0
        for (k, p, u), want in zip(c.draws, c.expected):
            cut, draw = se.logits_margins(c.x, c.temperature, k, p, u)
            assert cut >= se.MARGIN and draw >= se.MARGIN, (c.name, k, p, u, cut, draw)
            assert osmp.sample_fixed_point(twin, 1.0, k, p, u, probs_mode=True)[:2] == want
            admitted += 1
    assert admitted >= 150


@pytest.mark.parametrize("fmt", list(se.FORMATS))
def test_special_value_rows(fmt):
    dtype = getattr(torch, fmt)
    rows = {r.name: r for r in se.special_rows(fmt)}
    for r in rows.values():
        x = se.from_bits(r.bits, fmt)
        stored = torch.from_numpy(r.bits.astype(np.int32 if fmt == "float32" else np.int16)).view(dtype)
        assert np.array_equal(stored.float().numpy().view(np.uint32) & 0x7F800000, x.view(np.uint32) & 0x7F800000)
        greedy = int(torch.argmax(stored))
        with np.errstate(all="ignore"):
            assert osmp._argmax(x) == greedy, r.name
        for t, k, p, u, tok, n in se.special_expected(r, fmt):
            assert 0 <= tok < x.size and (k != 1 or tok == greedy)
            if np.isnan(x).any() or np.isposinf(x).any():
                assert tok == greedy  # no positive weight: the arg-max
    nan_at = {name: int(name.rsplit("-", 1)[1]) for name in rows if name.startswith(("nan-", "neg-nan-")) and name[-1].isdigit()}
    assert len(nan_at) == 6
    for name, at in nan_at.items():
        assert se.special_expected(rows[name], fmt)[0][4] == at
    assert se.special_expected(rows["neg-nan-beside-pinf"], fmt)[0][4] == 50
    last = se.special_expected(rows["ninf-tail"], fmt)
    assert last[1][4] == 999 and last[1][5] == 1024  # the largest u draws the last finite token; -inf tokens count as kept
    assert se.special_expected(rows["all-ninf"], fmt)[0][4:] == (0, 1027)
    assert se.special_expected(rows["one-finite"], fmt)[1][4] == 777
    assert se.special_expected(rows["two-pinf"], fmt)[0][4] == 300
