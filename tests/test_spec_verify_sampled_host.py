"""Verification of a sampled draft, the host side (no GPU): the integer rule of tests/spec_verify_sampled_ref.py -- its reduction to
the merged point-mass rule, its losslessness counted exactly over the whole 2^-24 grid, its two fixed points -- then
PagedKVCacheManager.rollback, and chitu_hip_speculative_verify_sampled's declaration, export, argument checks and documents."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import spec_verify_ref as sv
from tests import spec_verify_sampled_ref as svs
from tests import test_gpu_spec_verify as base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "chitu_hip_speculative_verify_sampled"
GRID = svs.GRID


# ---------------------------------------------------------------- the rule
@pytest.mark.parametrize("kind,top_k,top_p", [("peaked", 50, 0.9), ("ties", -1, 0.6), ("equal", 7, 1.0), ("peaked", -1, 1.0),
                                              ("underflow", -1, 1.0), ("peaked", 1, 0.9), ("peaked", 2, 0.0)])
def test_a_one_hot_draft_row_reduces_to_the_point_mass_rule(kind, top_k, top_p):
    """q one-hot at d (probs_mode: v_d = S_q = 2^40, every other v_i = 0) and uniforms on the 2^-24 grid: the acceptance test
    U * 2^40 * S_p < 2^24 * w_d * 2^40 is u * S_p < w_d, the residual is 2^40 * (w without d) and its position floor(u * 2^40 *
    (S_p - w_d)) selects what floor(u * (S_p - w_d)) selects among w -- so (accepted, token) is spec_verify_ref.verify_row's, for
    every draft kind of tests/test_gpu_spec_verify.py that a row can be one-hot at (vocab + 5 has no such row), u_acc at 0, on both
    sides of the threshold and at 1 - 2^-24, and a spread of u_alt."""
    vocab = 300
    p = torch.softmax(base._rows(kind, 1, vocab, 7) / 0.8, dim=-1)[0].numpy()
    kw_p, kinds = base._drafts_of(p, 1.0, top_k, top_p, True)
    u_alts = [0.0, 0.5, 1 - 2.0**-24, 12345 / GRID, 9999999 / GRID, 0.75]
    checked = accepted = 0
    for d in [k for k in kinds if k < vocab]:
        q = np.zeros(vocab, dtype=np.float32)
        q[d] = 1.0
        kw_q = svs.kept_weights(q, 1.0, top_k, top_p, True)
        u_accs = [0, GRID - 1]
        if kw_p["w"] is not None and kw_p["S"] > 0:
            assert kw_q["S"] == 1 << 40 and int(kw_q["w"][d]) == 1 << 40
            thr = -(-(GRID * int(kw_p["w"][d])) // kw_p["S"])  # the smallest U that rejects
            u_accs += [U for U in (thr - 1, thr) if 0 <= U < GRID]
        for U in u_accs:
            for u_alt in u_alts:
                got = svs.verify_row_from(kw_p, kw_q, d, U / GRID, u_alt)
                assert got == sv.verify_row_from(kw_p, d, U / GRID, u_alt), (d, U, u_alt, got)
                checked += 1
                accepted += bool(got[0])
    assert checked >= (24 if top_k == 1 else 36) and 0 < accepted < checked


def _pairs():
    """(p, q) probability rows of 2 .. 8 tokens: ties, zeros, disjoint supports, p == q, one-hot rows"""
    rng = np.random.default_rng(5)
    out = [([0.5, 0.5], [0.25, 0.75]), ([1.0, 0.0], [0.0, 1.0]), ([0.2, 0.3, 0.5], [0.2, 0.3, 0.5]),
           ([0.25, 0.25, 0.25, 0.25], [0.1, 0.4, 0.4, 0.1]), ([0.5, 0.0, 0.5, 0.0, 0.0], [0.0, 0.3, 0.0, 0.3, 0.4]),
           ([0.4, 0.05, 0.25, 0.0, 0.2, 0.1], [0.05, 0.4, 0.0, 0.25, 0.1, 0.2]), ([0.0, 0.0, 1.0], [0.3, 0.3, 0.4]),
           ([0.3, 0.3, 0.4], [0.0, 0.0, 1.0])]
    for n in (2, 3, 5, 7, 8):
        out.append((rng.random(n), rng.random(n)))
        out.append((np.round(rng.random(n) * 4) + (np.arange(n) == 0), np.round(rng.random(n) * 4) + (np.arange(n) == n - 1)))  # ties and zeros
    return [(np.asarray(p, dtype=np.float32), np.asarray(q, dtype=np.float32)) for p, q in out]


def _ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("top_k,top_p", [(-1, 1.0), (3, 1.0), (-1, 0.7)])
def test_the_integer_rule_is_lossless_on_the_grid(top_k, top_p):
    """Counted exactly over all 2^24 values of each uniform, by intervals and not by enumeration.  With p_i = w_i / S_p and
    q_i = v_i / S_q the kept distributions, a draft d ~ q is accepted for the U below ceil(2^24 w_d S_q / (v_d S_p)) (capped at 2^24),
    so P_acc(d) is min(1, p_d / q_d) rounded UP to the grid: off by less than one step g = 2^-24.  A rejected row emits x for the U
    with floor(U R / 2^24) in [C_{x-1}, C_x) (C the cumulative residual): ceil(2^24 C_x / R) - ceil(2^24 C_{x-1} / R) grid points,
    r_x / R to within less than one step.  Then
        P(emit x) = q_x P_acc(x) + [sum_d q_d (1 - P_acc(d))] P_res(x),
    where the exact values of the three factors give min(p_x, q_x) + rho * (r_x / R) = p_x (rho = R / (S_p S_q) = sum_d max(q_d - p_d, 0)
    = sum_d max(p_d - q_d, 0)).  Errors: q_x * g <= g in the first term; the bracket is off by at most sum_d q_d g = g and multiplies
    P_res <= 1; P_res is off by at most g and multiplies rho <= 1.  So |P(emit x) - p_x| < 3 * 2^-24 for every x: one grid step per
    accept decision (twice: in the accepted mass of x and in the rejected mass) and one per residual interval."""
    g = Fraction(1, GRID)
    for p, q in _pairs():
        kw_p, kw_q = svs.kept_weights(p, 1.0, top_k, top_p, True), svs.kept_weights(q, 1.0, top_k, top_p, True)
        S_p, S_q = kw_p["S"], kw_q["S"]
        assert S_p > 0 and S_q > 0
        w, v = [int(x) for x in kw_p["w"]], [int(x) for x in kw_q["w"]]
        n = len(w)
        r, R = svs.residual(kw_p, kw_q)
        # P_acc(d) by the threshold, cross-checked against the rule at the threshold's two neighbours
        p_acc = []
        for d in range(n):
            if v[d] == 0:
                p_acc.append(None)  # never drafted
                continue
            thr = min(GRID, _ceil_div(GRID * w[d] * S_q, v[d] * S_p))
            for U in (thr - 1, thr):
                if 0 <= U < GRID:
                    assert svs.accepts(w[d], v[d], S_p, S_q, U) == (U < thr)
                    assert svs.verify_row_from(kw_p, kw_q, d, U / GRID, 0.0)[0] == (U < thr)
            p_acc.append(Fraction(thr, GRID))
        reject_mass = sum(Fraction(v[d], S_q) * (1 - p_acc[d]) for d in range(n) if v[d])
        if R == 0:
            assert reject_mass == 0  # p == q: nothing is ever rejected
            p_res = [Fraction(0)] * n
        else:
            cum, bounds = 0, [0]
            for x in range(n):
                cum += r[x]
                bounds.append(min(GRID, _ceil_div(cum * GRID, R)))
            assert bounds[-1] == GRID
            p_res = [Fraction(bounds[x + 1] - bounds[x], GRID) for x in range(n)]
            some_rejected = next(d for d in range(n) if v[d] and p_acc[d] < 1)
            for x in range(n):  # the intervals are the rule's: their first and last grid point emit x
                for U in (bounds[x], bounds[x + 1] - 1):
                    if bounds[x] < bounds[x + 1]:
                        assert svs.verify_row_from(kw_p, kw_q, some_rejected, 1.0, U / GRID) == (False, x), (x, U)
        for x in range(n):
            emitted = (Fraction(v[x], S_q) * p_acc[x] if v[x] else 0) + reject_mass * p_res[x]
            assert abs(emitted - Fraction(w[x], S_p)) < 3 * g, (p, q, x, float(emitted), w[x] / S_p)
            if w[x] == 0:
                assert emitted == 0  # a token the target does not keep is never emitted


def test_fixed_points_of_the_rule():
    p = np.array([0.4, 0.05, 0.25, 0.0, 0.2, 0.1], dtype=np.float32)
    kw = svs.kept_weights(p, 1.0, -1, 1.0, True)
    for d in (0, 1, 2, 4, 5):  # p == q bit for bit: accepted at every U
        for U in (0, 1, GRID // 2, GRID - 1):
            assert svs.verify_row_from(kw, dict(kw), d, U / GRID, 0.3) == (True, d)
        assert svs.verify_row_from(kw, dict(kw), d, 1.0, 0.3) == (True, d)  # u = 1 clamps to the last grid point
    # w_d == 0: rejected at U = 0; with p == q the residual is empty and the row emits the arg-max
    assert svs.verify_row_from(kw, dict(kw), 3, 0.0, 0.3) == (False, 0)
    assert svs.verify_row_from(kw, dict(kw), 11, 0.0, 0.3) == (False, 0)
    q = np.array([0.1, 0.1, 0.1, 0.5, 0.1, 0.1], dtype=np.float32)
    kw_q = svs.kept_weights(q, 1.0, -1, 1.0, True)
    acc, tok = svs.verify_row_from(kw, kw_q, 3, 0.0, 0.0)
    assert not acc and tok == 0
    # v_d == 0 < w_d always accepts
    q0 = np.array([0.5, 0.0, 0.5, 0.0, 0.0, 0.0], dtype=np.float32)
    assert svs.verify_row_from(kw, svs.kept_weights(q0, 1.0, -1, 1.0, True), 1, 0.99999994, 0.0) == (True, 1)
    # greedy rows, degenerate rows and rows without a draft are the merged rule's
    row = np.random.default_rng(0).normal(0, 3, 300).astype(np.float32)
    best = int(np.argmax(row))
    assert svs.verify_row(row, row[::-1].copy(), 0.9, 1, 0.95, best, 0.99, 0.5) == (True, best)
    assert svs.verify_row(row, row[::-1].copy(), 0.9, 1, 0.95, best + 1, 0.0, 0.5) == (False, best)
    for u in (0.0, 0.3, 0.99999994):
        assert svs.verify_row(row, None, 0.9, 12, 0.95, -1, 0.0, u) == sv.verify_row(row, 0.9, 12, 0.95, -1, 0.0, u)
    zeros = np.zeros(7, dtype=np.float32)
    assert svs.verify_row(zeros, p[:6].repeat(2)[:7], 1.0, -1, 1.0, 0, 0.5, 0.5, probs_mode=True) == (True, 0)
    assert svs.verify_row(p, np.zeros(6, dtype=np.float32), 1.0, -1, 1.0, 2, 0.0, 0.5, probs_mode=True) == (False, 0)  # S_q == 0
    assert svs.grid(float("nan")) == 0 and svs.grid(-1.0) == 0 and svs.grid(2.0) == GRID - 1 and svs.grid(0.5) == GRID // 2
    for R, U in ((0, 5), (1, GRID - 1), ((1 << 114) - 12345, GRID - 1), ((1 << 100) + 77, 1234567)):
        assert svs.position(R, U) == (U * R) >> 24


# ---------------------------------------------------------------- the cache manager
def _cache():
    from chitu_amd.cache_manager import PagedKVCacheManager

    return PagedKVCacheManager(0, 1, num_hot_req=4, block_size=4, max_seq_len=16, device="cpu", kv_shape_per_sample=(2,), dtype=torch.float32)


def test_rollback_gives_rows_and_pages_back():
    c = _cache()
    free = len(c.free_blocks)
    c.register_sequence("a", 9)  # three pages
    c.register_sequence("b", 4)  # one full page
    pages_a = list(c.block_table["a"])
    assert len(pages_a) == 3 and len(c.free_blocks) == free - 4
    c._table_rows = ["a", "b"]
    c.rollback(["a", "b"], [0, 0])  # nothing dropped: nothing changes
    assert c.seq_lens == {"a": 9, "b": 4} and c.block_table["a"] == pages_a and c._table_rows == ["a", "b"]
    c.rollback(["a"], [1])  # 9 -> 8: the third page holds no row any more
    assert c.seq_lens["a"] == 8 and c.block_table["a"] == pages_a[:2] and c._table_rows is None
    assert c.free_blocks[-1] == pages_a[2] and len(c.free_blocks) == free - 3
    c._table_rows = ["a", "b"]
    c.rollback(["a", "b"], [3, 1])  # inside a page: lengths only
    assert c.seq_lens == {"a": 5, "b": 3} and len(c.block_table["a"]) == 2 and len(c.block_table["b"]) == 1 and c._table_rows == ["a", "b"]
    c.rollback(["a", "b"], [5, 3])  # more than any decode appended: down to nothing
    assert c.seq_lens == {"a": 0, "b": 0} and c.block_table["a"] == [] and c.block_table["b"] == [] and c._table_rows is None
    assert len(c.free_blocks) == free and sorted(c.free_blocks) == list(range(c.num_blocks))
    c.prepare_block_table_for_decode(["a"])  # the single-token step takes a page again at length 0
    assert len(c.block_table["a"]) == 1


def test_rollback_refuses_to_drop_below_zero():
    c = _cache()
    c.register_sequence("a", 6)
    c.register_sequence("b", 2)
    before = (dict(c.seq_lens), {k: list(v) for k, v in c.block_table.items()}, list(c.free_blocks))
    with pytest.raises(ValueError):
        c.rollback(["a", "b"], [1, 3])  # b is refused: a keeps its row too
    with pytest.raises(ValueError):
        c.rollback(["a"], [-1])
    assert (dict(c.seq_lens), {k: list(v) for k, v in c.block_table.items()}, list(c.free_blocks)) == before


def test_rollback_after_a_multi_token_step_matches_finalize():
    """a step of 4 rows of which 2 are kept, then 1 given back, is a step of which 1 was kept"""
    a, b = _cache(), _cache()
    for c, keep in ((a, 2), (b, 1)):
        c.register_sequence("r", 7)
        c.prepare_block_table_for_decode_multi(["r"], 4)
        c.finalize_cache_multi_decode(["r"], [keep])
    a.rollback(["r"], [1])
    assert a.seq_lens == b.seq_lens and len(a.block_table["r"]) == len(b.block_table["r"]) == 2 and len(a.free_blocks) == len(b.free_blocks)


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
    assert int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)) >= 12
    assert re.search(r"^int " + ENTRY + r"\s*\(", text, flags=re.M)
    assert re.search(ENTRY + r"\s+new: no reference counterpart", text)
    note = [n for n in re.findall(r"/\*.*?\*/", text, flags=re.S)
            if ENTRY in n and "U(u_acc) * v_d * S_p < 2^24 * w_d * S_q" in n and "max(0, w_i * S_q - v_i * S_p)" in n]
    assert note, "no header note that states the rule"


def test_library_exports_the_entry_and_python_binds_it():
    assert hasattr(_cdll(), ENTRY)
    from chitu_amd import sampling

    assert callable(sampling.speculative_verify_sampled) and callable(sampling.ModelDrafter)
    for name in ("check_target", "start", "draft", "settle", "retire"):
        assert callable(getattr(sampling.ModelDrafter, name))


def test_docs_agree_with_the_header():
    text = _header()
    n = len(re.findall(r"^int chitu_hip_\w+\s*\(", text, flags=re.M))
    version = re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{n} entry points, ABI version {version}" in readme and "ModelDrafter" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in integ.splitlines() if l.startswith("| 11 → 12 |")]
    assert len(row) == 1 and ENTRY in row[0]
    assert ENTRY in open(os.path.join(ROOT, "chitu_amd", "sampling.py")).read()
    assert "3.10" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("llama.py", "deepseek_v3.py", "mixtral.py"):
        path = os.path.join(ROOT, "chitu_amd", name)
        if os.path.exists(path):
            assert "out of scope here" not in open(path).read(), name


def test_entry_refuses_bad_arguments_on_the_host():
    """Nothing is launched (no rows, or refused before the launch; the pointers are never dereferenced), so this needs no GPU."""
    lib = _cdll()
    buf = ctypes.create_string_buffer(128)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    BAD_ARG = -1

    def call(T=4, rows=0, dtype=2, qdtype=0, probs=0, x=p, q=p, temps=p, ks=p, ps=p, drafts=p, us=p, out=p, vocab=100, stride=100, qstride=100):
        return getattr(lib, ENTRY)(x, dtype, i64(stride), q, qdtype, i64(qstride), i64(rows), i32(vocab), temps, ks, ps, drafts, us, i32(T),
                                   i32(probs), out, None, None, None)

    assert all(call(T=T) == 0 for T in range(2, 9)) and call(probs=1, temps=None) == 0
    assert all(call(dtype=a, qdtype=b) == 0 for a in range(3) for b in range(3))
    assert call(T=1) == BAD_ARG and call(T=9) == BAD_ARG and call(T=0) == BAD_ARG
    assert call(T=4, rows=5) == BAD_ARG and call(rows=-4) == BAD_ARG
    for missing in ("x", "q", "ks", "ps", "drafts", "us", "out", "temps"):
        assert call(**{missing: None}) == BAD_ARG, missing
    assert call(dtype=3) == BAD_ARG and call(qdtype=3) == BAD_ARG and call(qdtype=-1) == BAD_ARG and call(probs=2) == BAD_ARG
    assert call(vocab=0) == BAD_ARG and call(stride=99) == BAD_ARG and call(qstride=99) == BAD_ARG
    assert call(vocab=(1 << 21) + 1, stride=1 << 22, qstride=1 << 22) == BAD_ARG  # the rule's products stay below 2^128
