"""Draft verification of speculative decoding with sampling, the host side (no GPU): the integer rule of tests/spec_verify_ref.py
against brute force, and chitu_hip_speculative_verify's declaration, export, argument checks and documents."""
import ctypes
import os
import re

import numpy as np

from oracle import sampling as osmp
from tests import spec_verify_ref as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "chitu_hip_speculative_verify"


# ---------------------------------------------------------------- the rule
def test_emitted_tokens_follow_p_for_every_draft_by_brute_force():
    """A 6-token probability row, no top-k / top-p cut: u_acc and u_alt sweep the midpoints of an N x N grid, so the share of grid
    points that emit token x is P(emit x) to the grid's resolution.  Per draft the acceptance share is p(d) within one grid line
    (1 / N); the share of an emitted x != d is the product of the rejected share and the replacement sweep's share of x, each
    within 1 / N of its value and both <= 1, so the emitted share is p within 3 / N -- for every draft in {each token, out of
    range}."""
    p = np.array([0.4, 0.05, 0.25, 0.0, 0.2, 0.1], dtype=np.float32)
    N = 200
    grid = (np.arange(N) + 0.5) / N
    kw = sv.kept_weights(p, 1.0, -1, 1.0, probs_mode=True)
    dist = kw["w"].astype(np.float64) / kw["S"]
    assert np.abs(dist - p / p.sum()).max() < 1e-6
    for d in list(range(6)) + [6, 11]:
        counts = np.zeros(6)
        n_acc = 0
        alt = [sv.verify_row_from(kw, d, 1.0, u)[1] for u in grid]  # u_acc = 1 rejects whenever anything else has mass
        for ua in grid:
            a, t = sv.verify_row_from(kw, d, ua, 0.0)
            if a:
                assert t == d
                n_acc += 1
                counts[d] += N
            else:
                for t in alt:
                    counts[t] += 1
        p_d = dist[d] if d < 6 else 0.0
        assert abs(n_acc / N - p_d) <= 1.0 / N, (d, n_acc)
        assert np.abs(counts / (N * N) - dist).max() <= 3.0 / N, (d, counts / (N * N), dist)
        assert counts[3] == 0  # a zero-probability token is never emitted
        if d < 6 and d != 3:
            assert all(t != d for t in alt)  # the replacement never is the rejected draft


def test_rows_without_a_draft_greedy_rows_and_degenerate_rows():
    rng = np.random.default_rng(0)
    row = rng.normal(0, 3, 300).astype(np.float32)
    for u in (0.0, 0.3, 0.99999994):
        assert sv.verify_row(row, 0.9, 12, 0.95, -1, 0.0, u) == (False, osmp.sample_fixed_point(row, 0.9, 12, 0.95, u)[0])
    best = int(np.argmax(row))
    assert sv.verify_row(row, 0.9, 1, 0.95, best, 0.99, 0.5) == (True, best)
    assert sv.verify_row(row, 0.9, 1, 0.95, best + 1, 0.0, 0.5) == (False, best)
    assert sv.verify_row(row, 0.9, 1, 0.95, -1, 0.0, 0.5) == (False, best)
    zeros = np.zeros(7, dtype=np.float32)  # all-zero probabilities: S == 0
    assert sv.verify_row(zeros, 1.0, -1, 1.0, 0, 0.5, 0.5, probs_mode=True) == (True, 0)
    assert sv.verify_row(zeros, 1.0, -1, 1.0, 2, 0.0, 0.5, probs_mode=True) == (False, 0)
    # the whole mass on the draft: accepted for every u_acc
    one = np.array([0, 0, 1, 0], dtype=np.float32)
    assert sv.verify_row(one, 1.0, -1, 1.0, 2, 0.99999994, 0.5, probs_mode=True) == (True, 2)
    # ties at the cut: equal weights, top_k 3 keeps indices 0 .. 2 -- index 2 is the last kept tie, index 3 the first dropped one
    eq = np.full(8, 0.125, dtype=np.float32)
    assert sv.verify_row(eq, 1.0, 3, 1.0, 2, 0.3, 0.0, probs_mode=True) == (True, 2)
    assert sv.verify_row(eq, 1.0, 3, 1.0, 2, 0.34, 0.99, probs_mode=True) == (False, 1)
    assert sv.verify_row(eq, 1.0, 3, 1.0, 3, 0.0, 0.99, probs_mode=True) == (False, 2)


def test_sequences_and_threshold_uniforms():
    out = sv.sequences([1, 1, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1], [5, 6, 7, 8, 1, 2, 3, 4, 9, 9, 9, 9], 4)
    assert out.tolist() == [[3, 5, 6, 7, -1], [1, 1, -1, -1, -1], [4, 9, 9, 9, 9]]  # an accept in the last row does not count
    for w_d, S in ((1, 3), (12345678901, 98765432109876), (1 << 39, (1 << 40) + 1), (5, 1 << 50)):
        below, above = sv.u_around(w_d, S)
        assert sv.target(below, S) < w_d <= sv.target(above, S)
        assert np.nextafter(np.float32(below), np.float32(1)) == np.float32(above)
    assert sv.u_around(0, 100) == (None, 0.0)
    assert sv.u_around(100, 100)[1] is None


# ---------------------------------------------------------------- the C entry
def _header():
    return open(os.path.join(ROOT, "include", "chitu_hip.h")).read()


def _cdll():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_declares_the_entry_with_its_note():
    text = _header()
    assert int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)) >= 11
    assert re.search(r"^int " + ENTRY + r"\s*\(", text, flags=re.M)
    assert re.search(ENTRY + r"\s+new: no reference counterpart", text)
    note = [n for n in re.findall(r"/\*.*?\*/", text, flags=re.S) if ENTRY in n and "target(u_acc, S) < w_d" in n and "u_alt" in n]
    assert note, "no header note that states the rule"


def test_library_exports_the_entry():
    assert hasattr(_cdll(), ENTRY)


def test_docs_agree_with_the_header():
    text = _header()
    n = len(re.findall(r"^int chitu_hip_\w+\s*\(", text, flags=re.M))
    version = re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)
    assert f"{n} entry points, ABI version {version}" in open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in integ.splitlines() if l.startswith("| 10 → 11 |")]
    assert len(row) == 1 and ENTRY in row[0]
    assert ENTRY in open(os.path.join(ROOT, "chitu_amd", "sampling.py")).read()


def test_entry_refuses_bad_arguments_on_the_host():
    """Nothing is launched (no rows, or refused before the launch; the pointers are never dereferenced), so this needs no GPU."""
    lib = _cdll()
    buf = ctypes.create_string_buffer(128)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    BAD_ARG = -1

    def call(T=4, rows=0, dtype=2, probs=0, temps=p, ks=p, ps=p, drafts=p, us=p, out=p, vocab=100, stride=100):
        return lib.chitu_hip_speculative_verify(p, dtype, i64(stride), i64(rows), i32(vocab), temps, ks, ps, drafts, us, i32(T), i32(probs),
                                                out, None, None, None)

    assert all(call(T=T) == 0 for T in range(2, 9)) and call(probs=1, temps=None) == 0
    assert call(T=1) == BAD_ARG and call(T=9) == BAD_ARG and call(T=0) == BAD_ARG and call(T=-4) == BAD_ARG
    assert call(T=4, rows=5) == BAD_ARG and call(T=3, rows=4) == BAD_ARG and call(rows=-4) == BAD_ARG
    for missing in ("ks", "ps", "drafts", "us", "out", "temps"):
        assert call(**{missing: None}) == BAD_ARG, missing
    assert call(dtype=3) == BAD_ARG and call(probs=2) == BAD_ARG and call(vocab=0) == BAD_ARG and call(stride=99) == BAD_ARG
