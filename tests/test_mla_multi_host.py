"""Multi-token MLA decode, the host side (no GPU): the fp64 reference of tests/mla_multi_ref.py against oracle/mla.py on the
expanded rows, its builders' closed forms, and the two C entries' export, declaration and argument checks."""
import ctypes
import os
import re

import pytest
import torch

from oracle import mla as omla
from tests import attn_exact as ax
from tests import mla_multi_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("chitu_hip_mla_decode_multi", "chitu_hip_mla_decode_multi_kv_fp8")


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("T,lens", [(1, [1, 65]), (2, [1, 2, 65]), (3, [2, 3, 0]), (5, [3, 5, 67]), (8, [8, 7, 130])])
def test_fp64_reference_is_the_oracle_on_the_expanded_rows(T, lens):
    """L < T (queries with no key: zeros), L = T (the first token sees one key) and tokens on both sides of a page edge.  The
    oracle works in fp32: 2^-20 of the peak is ample for sums of <= 130 terms."""
    H = 3
    case = mr.random_case(H, T, lens, seed=T)
    cache, table = mr.paged(case["rows"], lens, seed=T)
    qn, qp, tab, exp = mr.expand(case, table)
    assert exp.tolist() == [max(0, L - T + t + 1) for L in lens for t in range(T)]
    want = omla.mla_decode(qn.float(), qp.float(), cache.float(), tab, exp, mr.SCALE)
    got = mr.multi64(case["q_nope"].float(), case["q_pe"].float(), case["rows"], lens).view(-1, H, 512)
    assert float((got - want.double()).abs().max()) <= 2.0 ** -20 * float(want.abs().max())
    for i, n in enumerate(exp.tolist()):
        assert n > 0 or not bool(got[i].any())


def test_builders_expect_what_the_fp64_reference_gives():
    c = mr.count_case(2, 4, [3, 4, 67, 130])
    got = mr.multi64(c["q_nope"].float(), c["q_pe"].float(), c["rows"], c["lens"])
    assert float((got - c["want"]).abs().max()) <= 1e-12
    assert not bool(c["want"][0, 0].any()) and bool(c["want"][0, 1].any())  # L = 3, T = 4: token 0 has no key, token 1 has one
    for T, L in mr.CAUSAL:
        p = mr.causal_probe_case(2, T, L)
        got = mr.multi64(p["q_nope"].float(), p["q_pe"].float(), p["rows"], p["lens"])
        for n, (i, pos) in enumerate(zip(p["probes"], p["pos"])):
            assert pos == L - T + i + 1
            key_row = p["rows"][n][pos, :512].double()
            for t in range(T):
                d = float((got[n, t] - key_row).abs().max())
                assert (d <= ax.ABS_DOMINANT) if t > i else (d >= 1.0), (T, L, i, t, d)


def test_same_tile_predicate():
    assert mr.same_tile([64, 10, 128], 4) and not mr.same_tile([65], 2) and not mr.same_tile([130], 4) and mr.same_tile([70], 5)


# ---------------------------------------------------------------- the C entries
def _cdll():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def _params(text, name):
    body = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1)
    return [" ".join(p.split()) for p in body.split(",")]


def test_library_exports_the_entries_and_the_header_declares_them():
    lib = _cdll()
    assert all(hasattr(lib, name) for name in ENTRIES)
    text = open(os.path.join(ROOT, "include", "chitu_hip.h")).read()
    assert int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)) >= 10
    notes = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name, plain in zip(ENTRIES, ("chitu_hip_mla_decode", "chitu_hip_mla_decode_kv_fp8")):
        assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M)
        # the single-token entry's list with the token strides behind the batch strides and q_len behind batch
        want = _params(text, plain)
        for after, new in (("int64_t qn_stride_b", "int64_t qn_stride_t"), ("int64_t qp_stride_b", "int64_t qp_stride_t"),
                           ("int32_t batch", "int32_t q_len")):
            want.insert(want.index(after) + 1, new)
        assert _params(text, name) == want, name
        assert [n for n in notes if name in n and "q_len" in n and "L - T + t" in n and "attn_backend.py:523-527" in n], name
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in integ.splitlines() if l.startswith("| 9 → 10 |")]
    assert len(row) == 1 and all(name in row[0] for name in ENTRIES)


def test_entries_check_their_arguments_on_the_host():
    """Nothing is launched (batch 0; the pointers are never dereferenced), so this needs no GPU."""
    lib = _cdll()
    buf = ctypes.create_string_buffer(128)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 8)
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    BAD_ARG, UNSUPPORTED = -1, -2
    for name in ENTRIES:
        entry = getattr(lib, name)

        def call(T=4, st=16 * 512, sh=512, page=64, splits=1, C=512, R=64, q=p, out=p):
            return entry(q, i64(4 * 16 * 512), i64(st), i64(sh), p, i64(4 * 16 * 64), i64(16 * 64), i64(64), p, i64(4), i32(page), p,
                         i32(4), p, f32(0.1), out, i32(0), i32(T), i32(16), i32(C), i32(R), i32(splits), p, i64(0), None)

        assert all(call(T=T) == 0 for T in range(1, 9)) and call(page=128) == 0 and call(splits=256) == 0
        assert call(T=0) == BAD_ARG and call(T=9) == BAD_ARG and call(T=-1) == BAD_ARG
        assert call(st=16 * 512 + 4) == BAD_ARG and call(sh=516) == BAD_ARG and call(q=odd) == BAD_ARG
        assert call(splits=0) == BAD_ARG and call(splits=257) == BAD_ARG and call(out=None) == BAD_ARG and call(out=None, splits=2) == 0
        assert call(page=96) == UNSUPPORTED and call(page=32) == UNSUPPORTED and call(C=256) == UNSUPPORTED and call(R=32) == UNSUPPORTED


# ---------------------------------------------------------------- the routing rule
def test_routing_rule_separates_the_measured_shapes(monkeypatch):
    """profiles/mla_multi_sweep.json (16 heads, 64-token pages, table width ctx / 64 + 1, 256 CUs): the multi launch is faster at
    bs 16 / ctx 8192, ties at bs 16 / ctx 1024 / T 4 and is slower at bs 1 and at bs 16 / ctx 1024 / T 2"""
    import json

    from chitu_amd import attn_backend as ab

    monkeypatch.setattr(ab, "_num_cus", lambda: 256)
    doc = json.load(open(os.path.join(ROOT, "profiles", "mla_multi_sweep.json")))
    assert len(doc["multi_sweep"]) == 8
    for row in doc["multi_sweep"]:
        worst = max(row[f]["multi_over_composed"] for f in ("bf16", "fp8"))
        best = min(row[f]["multi_over_composed"] for f in ("bf16", "fp8"))
        takes_multi = ab.mla_multi_beats_composition(row["bs"], row["T"], 16, row["ctx"] // 64 + 1)
        assert takes_multi == (worst < 1.0), (row["bs"], row["ctx"], row["T"], best, worst)
        assert all(row[f]["equal_at_one_split"] for f in ("bf16", "fp8"))


# ---------------------------------------------------------------- tensor parallelism: the collectives' row capacity
def test_a_multi_token_step_beyond_the_communicators_rows_raises(monkeypatch):
    from chitu_amd import deepseek_v3
    from chitu_amd import tensor_parallel as tp

    class Comm:
        max_rows = 64

    monkeypatch.setattr(tp, "xgmi_comm", lambda: None)
    deepseek_v3._check_multi_step_rows(10 ** 6)  # one rank: no communicator, nothing to exceed
    monkeypatch.setattr(tp, "xgmi_comm", lambda: Comm())
    deepseek_v3._check_multi_step_rows(64)
    with pytest.raises(ValueError, match=r"72 rows .* 64 rows.*max_rows >= 72"):
        deepseek_v3._check_multi_step_rows(9 * 8)

