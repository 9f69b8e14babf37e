"""The fused launches on exact data: the norm-prologue GEMMs, mla_q_proj and merge + W_UV against CPU expectations.

Builders and CPU expectations: tests/fused_exact.py; their CPU checks: tests/test_fused_exact_host.py.  Every entry is called
through the C ABI with each output between G guard rows (and guard columns where a row stride allows them) of the NaN sentinels
of tests/dense_exact.py, the output itself pre-filled with the sentinel; after each launch the guards are untouched, no live
element still holds the sentinel and the result equals the expectation bit for bit -- a CPU expectation, never another kernel's
output, and no tolerance anywhere.  Where rsqrtf or expf could show, the comparison is whole-row / per-element equality with one
candidate of tests/row_exact.py's sets (radii RSQRT_RADIUS, EXPF_RADIUS: the project's, no new number).

  A  chitu_hip_bf16_gemm_add_norm: M 1..4 (MR 1 / 2 / 4, M = 3 with a dead row), K 512..8192, N 1..8208 (both WK, both ring
     depths by the launcher's rule and through the bf16_gemm_deep option), 1 and 2 terms at a term stride wider than K, x a
     strided view at an offset base, three output types; sum_out on its own -- a sum_out that overlaps x or add is refused
  B  chitu_hip_bf16_gemm_silu_add_norm: the same M and K, inter 8..4112, per-element expf candidates
  D  chitu_hip_fp8_gemm_add_norm: 1 / 2 / 9 / 10 / 11 / 16 terms (the three register variants), M = 2, WK 4 and 8 (by K and
     by the tile rule), strided terms and rows with NaN in the gaps; return codes with outputs untouched
  E  chitu_hip_mla_q_proj: MT 1 and 2, q_lora_rank with 0 / 1 / 2 K blocks per wave, N 1..1536, a row stride with NaN filler,
     the KV rider on valid and out-of-table batches; return codes
  C  chitu_hip_bf16_gemm_add_norm_qkv_post: three head layouts, quarter-turn rotations, pages 16 and 48, out-of-table batches
     between guard pages; the k / v columns of qkv_out stay untouched, as the header says
  F  chitu_hip_absorb_bmm_rope_kv_fp8: the exact bmm under all three scale stride sets, q_pe in place, the KV rider
  G  chitu_hip_mla_merge_absorb_uv_quant_fp8 and _tm on a hand-built workspace: live / empty / negligible splits, S 2..130,
     a (b, h) with no live split, tile-major padding
  H  the ops wrappers inside tests.util.poisoned_allocations() == outside it == the expectation
  I  the full-mantissa family: row_exact.rms_case rows in front of an identity GEMM weight (A, D, E)

The header's promises that are tested as stated: chitu_hip_mla_q_proj "can differ in the last bf16 bit" from mla_qkv_post stays
true for general data (the identity family matches one rsqrt candidate row per token, not the other kernel).

Bugs these tests exposed:
  - include/chitu_hip.h promised that sum_out of the three bf16 norm-prologue entries "may alias x or add".  It cannot: EVERY
    workgroup of the GEMM re-reads x and add for its own copy of the prologue while workgroup 0 writes sum_out, so a workgroup
    that starts after that store (any grid that is not resident at once, e.g. 1024 tiles at WK = 4 with 48 KB of LDS each)
    normalises x + 2 add.  Found by reading the kernel while the aliased cases of section A were written, not by a failing
    run (whether it shows depends on workgroup scheduling, so a passing run proves nothing).  The launchers now refuse an
    overlapping sum_out with CHITU_ERR_BAD_ARG, the header says so, and section A tests the refusal (the ops wrappers always
    allocated sum_out, so no model path changes).  chitu_hip_rmsnorm, where one workgroup owns a row, still runs in place.
No kernel computed a wrong value on these cases.

The (b, h) without a live split (section G): every LSE is -inf, so wsum = 0, inv = 0, the merged row is zeros, the projection is
zeros, amax = 0 and the scale is 0; the codes are 0 / 0 = NaN (the kernel's `v / sc` path, group_div_fast(0) being false).
oracle/fp8.py::act_quant_deepseek_v3 of a zero group gives the same: scale 0, NaN codes (compared NaN as NaN).

Measured on the MI355X: 219 tests, 4.2 s for the module.  rsqrtf: the exact normalised row has ONE expectation; of the 88 rows of
the full-mantissa family (section I) 0 took a non-central candidate.  expf: 0 of the 19 056 SiLU elements of section B did.

Mutations tried by hand on the MI355X (other builds of the library, never committed; each run once against this module only;
all of them change only computed values or move a store inside a guarded buffer) and what caught them:
  - fp8_norm_gemm.hip, K loop: the activation scale of the neighbouring group (`xs[kb + d - 1]`): all 46 cases of section D, its
    4 identity cases and ops.fp8_linear_add_norm, e.g. "chitu_hip_fp8_gemm_add_norm 1-1-16-512-bf16 out f32 (WK, term
    registers, MR) = (4, 1, 1): 16 of 16 elements differ in 1 rows; first (row, col, got, want): [(0, 0, 409.5, -630.0), ...".
  - fp8_norm_gemm.hip: `kb1 - 1` in wave 1: the same 51, "... [(0, 0, -726.0, -630.0), (0, 1, 310.0, 270.0), ...".
  - bf16_norm_gemm.hip, add_norm_issue: the second term's offset dropped: the 9 two-term cases of section A and
    ops.bf16_linear_add_norm, "chitu_hip_bf16_gemm_add_norm 1-16-576-2--1-own-f16 ... sum_out: 576 of 576 elements differ";
    no one-term case, rightly.
  - mla_q_proj.hip: the wave -> K-range map `t` replaced by `wave`: NOTHING, rightly -- the eight ranges are the same set, each
    still summed by one wave, and on exact data the order of the cross-wave sum cannot show.  No comparison can see it.
  - mla_q_proj.hip: `ws[i]` taken from block 0: all 30 cases of section E with more than one K block and ops.mla_q_proj,
    "chitu_hip_mla_q_proj 1-384-16-f16-False out f32 blocks per wave [0, 1, 0, 0, 0, 0, 1, 1] {}: 16 of 16 elements differ";
    not the 5 cases of q_lora_rank 128 (block 0 is their only block) nor the identity family (all its scales are 1), rightly.
  - absorb.hip, mla_merge_uv_quant_kernel: `i < S - 1` in the S <= 16 path: 14 of the 15 cases with S <= 16, "... 1-1-2-w_uv
    (live splits per (b, h): [1], dead (b, h) -1) scales: 1 of 1 elements differ ... [(0, 0, 0.0, 2.2232143878936768)]".  The
    one it missed, (1, 1, 16), had its single live split elsewhere than on the last split: a gap, closed -- merge_case now puts
    one live split of every (b, h) on the last split or the first.  (The `S > 16` loop was not mutated.)
  - mla_merge_uv_quant_kernel: the tile-major row `m + 1` for `b & 15 < 15`: all 34 cases of section G and the tile-major
    ops wrapper, "tile-major codes (padding rows = sentinel): 256 of 2048 elements differ in 8 rows"; no row-major comparison.
  - gemm_common.h, gemm_epilogue_v2: `m >= M + 1` (run without section H, whose outputs have no guard row): every case whose
    tile has a row M -- 27 of A, 46 of D, their 8 identity cases, the 21 cases of E with batch 1 / 5 / 17 and 3 of its identity
    cases, "stored outside the output, first (buffer row - G, col): [(1, 0)]"; batch 16 and 32 fill their tiles, rightly not.
"""

import contextlib

import pytest
import torch

from tests import dense_exact as dx
from tests import fused_exact as fx
from tests import row_exact as rx
from tests import test_gpu_dense_exact as td  # (its _absorb_args ...
from tests import test_gpu_row_exact as tr    # ... and this one's _call, _Pages, _mla_inputs, _check_mla_cache: nothing is copied)
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -2
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
i32, i64, f32, _call = tr.i32, tr.i64, tr.f32, tr._call


def _L():
    from chitu_amd import _lib

    return _lib


def _id(case):
    return "-".join(str(v).replace(" ", "") for v in case if not isinstance(v, tuple))


def _ok(entry, case, n, extra=""):
    print(f"FUSEDEXACT {entry} {_id(case)}: ok, {n} elements{extra}")


def _types(dt):
    return ["f32"] if dt == "f32" else ["f32", dt]


class _Inputs:
    """x as a strided view at an offset base, add [rows, terms, dim] with row and term strides wider than the data; both inside
    guarded sentinel buffers, so every gap holds a NaN and a store into an input is seen."""

    def __init__(self, c):
        rows, dim, terms = c["rows"], c["dim"], max(c["terms"], 1)
        self.xb = rx.Guarded(rows, dim, BF16, stride=dim + 24)
        self.xb.view.copy_(rx.bits(c["x"]).cuda())
        self.tstride = dim + 16 if terms > 1 else 0
        cols = (terms - 1) * self.tstride + dim
        self.ab = rx.Guarded(rows, cols, BF16, stride=cols + 8)
        for k in range(terms):
            self.ab.view[:, k * self.tstride: k * self.tstride + dim].copy_(rx.bits(c["add"][:, k]).cuda())
        self.x, self.add = self.xb.view, self.ab.view
        self.want_x, self.want_add = self.xb.full.clone(), self.ab.full.clone()

    def unchanged(self, what):
        assert torch.equal(self.xb.full, self.want_x) and torch.equal(self.ab.full, self.want_add), f"{what}: an input buffer was written"


# ---------------------------------------------------------------- A: bf16 GEMM behind add + norm
def _bf16_add_norm(inp, c, w_dev, sum_view, sum_stride, out, dt, M, N, K, rc=0):
    _call("chitu_hip_bf16_gemm_add_norm", inp.x, i64(inp.xb.stride), inp.add, i64(inp.ab.stride), i32(max(c["terms"], 1)), i64(inp.tstride),
          sum_view, i64(sum_stride), c["w"].cuda(), f32(c["eps"]), w_dev, out, i32(dx.DT_CODE[dt]), i64(M), i64(N), i64(K), rc=rc)


@pytest.mark.parametrize("case", fx.A_CASES, ids=_id)
def test_bf16_gemm_add_norm_every_form(case):
    M, N, K, terms, deep, place, dt, form = case
    assert fx.bf16_norm_form(M, N, K, deep) == form
    c, w = fx.norm_case(M, K, terms), fx.bf16_weight(N, K)
    exact = fx.bf16_exact(c, w)
    w_dev, inp = w["w_q"].cuda(), _Inputs(c)
    n = 0
    for t in _types(dt):
        dtype = dx.DTYPES[t]
        what = f"chitu_hip_bf16_gemm_add_norm {_id(case)} out {t} (WK, ring, MR) = {form}"
        out, s_out = rx.Guarded(M, N, dtype), rx.Guarded(M, K, BF16, stride=K + 8)
        with _L().debug_option("bf16_gemm_deep", deep) if deep >= 0 else contextlib.nullcontext():
            _bf16_add_norm(inp, c, w_dev, s_out.view, K + 8, out.view, t, M, N, K)
        rx.assert_same(s_out.check(what + " sum_out"), c["v"], what + " sum_out")
        rx.assert_same(out.check(what), dx.expect(exact, dtype), what)
        inp.unchanged(what)
        n += M * N + M * K
    # a sum_out inside x or add is refused before anything is launched (see "Bugs these tests exposed")
    if place != "own":
        out = rx.Guarded(M, N, F32)
        src = inp.xb if place == "x" else inp.ab
        _bf16_add_norm(inp, c, w_dev, src.view[:, :K], src.stride, out.view, "f32", M, N, K, rc=ERR_BAD_ARG)
        out.untouched(f"chitu_hip_bf16_gemm_add_norm {_id(case)} with sum_out = {place}")
        inp.unchanged(f"refused sum_out = {place}")
    _ok("chitu_hip_bf16_gemm_add_norm", case, n)


# ---------------------------------------------------------------- B: SiLU epilogue
@pytest.mark.parametrize("case", fx.B_CASES, ids=_id)
def test_bf16_gemm_silu_add_norm(case):
    M, inter, K, place, form = case
    c, w = fx.norm_case(M, K, 1), fx.silu_weight(inter, K)
    cand, gate = fx.silu_expect(c, w, inter)
    inp = _Inputs(c)
    what = f"chitu_hip_bf16_gemm_silu_add_norm {_id(case)}"
    out, s_out = rx.Guarded(M, inter, BF16), rx.Guarded(M, K, BF16, stride=K + 8)
    args = lambda sv, ss, o: (inp.x, i64(inp.xb.stride), inp.add, i64(inp.ab.stride), sv, i64(ss), c["w"].cuda(), f32(c["eps"]), w["w_q"].cuda(),
                              o, i64(M), i64(inter), i64(K))
    _call("chitu_hip_bf16_gemm_silu_add_norm", *args(s_out.view, K + 8, out.view))
    rx.assert_same(s_out.check(what + " sum_out"), c["v"], what + " sum_out")
    got = out.check(what)
    idx = rx.silu_match(got.reshape(-1, 1), cand, what + " (one row per output element)")
    inp.unchanged(what)
    if place != "own":
        out2 = rx.Guarded(M, inter, BF16)
        src = inp.xb if place == "x" else inp.ab
        _call("chitu_hip_bf16_gemm_silu_add_norm", *args(src.view[:, :K], src.stride, out2.view), rc=ERR_BAD_ARG)
        out2.untouched(what + f" with sum_out = {place}")
        inp.unchanged(what + f" refused sum_out = {place}")
    _ok("chitu_hip_bf16_gemm_silu_add_norm", case, M * inter + M * K, f", {int((idx != 0).sum())} of {idx.numel()} took a non-central expf candidate")


# ---------------------------------------------------------------- C: RoPE + paged K/V append epilogue
def _quarter_turns(M, half, seed):
    """cos / sin [M, half] drawn from the four exact rotations, as dense_exact.rope_case draws them."""
    pick = torch.randint(0, 4, (M, half), generator=torch.Generator().manual_seed(seed))
    return torch.tensor([1.0, 0.0, -1.0, 0.0])[pick].contiguous(), torch.tensor([0.0, 1.0, 0.0, -1.0])[pick].contiguous()


def _qkv_case(case):
    hq, hkv, d, K, M, page, variant = case
    N = (hq + 2 * hkv) * d
    c, w = fx.norm_case(M, K, 1), fx.bf16_weight(N, K)
    heads = dx.expect(fx.bf16_exact(c, w), BF16).view(M, hq + 2 * hkv, d)  # the projection's bf16 output: exact, rounded once
    cos, sin = _quarter_turns(M, d // 2, seed=K + d + M)
    rot = rx.rope_oracle(heads[:, : hq + hkv], cos, sin, 0)
    a, b = rot.float().abs().view(-1, d // 2, 2).sort(-1).values, heads[:, : hq + hkv].float().abs().view(-1, d // 2, 2).sort(-1).values
    assert torch.equal(a, b)  # a signed permutation of every pair
    bad = variant != "valid"
    lens, table, num_pages, _, kinds = rx.paged_batch(M, page, seed=int(variant[-1]) if bad else 2, bad=bad)
    return N, c, w, heads, cos, sin, rot, lens, table, num_pages, kinds


@pytest.mark.parametrize("case", fx.C_CASES, ids=_id)
def test_bf16_gemm_add_norm_qkv_post(case):
    """include/chitu_hip.h: qkv_out "receives the ROTATED q heads only" -- its k / v columns are left untouched (they keep the
    sentinel), the rotated k heads and the v heads are in their page rows and every other cache row is as it was."""
    hq, hkv, d, K, M, page, variant = case
    N, c, w, heads, cos, sin, rot, lens, table, num_pages, kinds = _qkv_case(case)
    assert fx.bf16_norm_form(M, N, K) is not None
    inp = _Inputs(c)
    out, s_out = rx.Guarded(M, N, BF16), rx.Guarded(M, K, BF16, stride=K + 8)
    kc, vc = tr._Pages(num_pages, page, (hkv, d), BF16, seed=7), tr._Pages(num_pages, page, (hkv, d), BF16, seed=8)
    _call("chitu_hip_bf16_gemm_add_norm_qkv_post", inp.x, i64(inp.xb.stride), inp.add, i64(inp.ab.stride), s_out.view, i64(K + 8), c["w"].cuda(),
          f32(c["eps"]), w["w_q"].cuda(), out.view, i64(M), i64(K), i32(hq), i32(hkv), i32(d), cos.cuda(), sin.cuda(), kc.inner, vc.inner,
          i64(num_pages), i32(page), table.cuda(), i32(table.shape[1]), lens.cuda())
    what = f"chitu_hip_bf16_gemm_add_norm_qkv_post {_id(case)} {kinds}"
    rx.assert_same(s_out.check(what + " sum_out"), c["v"], what + " sum_out")
    got = out.check(what + " qkv_out", written=False)
    rx.assert_same(got[:, : hq * d], rot[:, :hq].reshape(M, hq * d), what + " q heads of qkv_out")
    assert bool((rx.bits(got[:, hq * d:]) == dx.SENTINEL16).all()), f"{what}: the k / v columns of qkv_out were written"
    kc.check(rx.append_oracle(kc.inner_init(), rot[:, hq:], lens, table, page, num_pages), what + " k cache")
    vc.check(rx.append_oracle(vc.inner_init(), heads[:, hq + hkv:], lens, table, page, num_pages), what + " v cache")
    inp.unchanged(what)
    _ok("chitu_hip_bf16_gemm_add_norm_qkv_post", case, M * hq * d + M * K + 2 * M * hkv * d)


# ---------------------------------------------------------------- D: block-fp8 GEMM behind [sum +] add + norm + act_quant
def _fp8_add_norm(inp, c, wq, ws, s_out, out, dt, M, N, K, rc=0, terms=None):
    _call("chitu_hip_fp8_gemm_add_norm", inp.x, i64(inp.xb.stride), inp.add, i64(inp.ab.stride), i32(terms or max(c["terms"], 1)), i64(inp.tstride),
          s_out.view, i64(s_out.stride), c["w"].cuda(), f32(c["eps"]), wq, ws, out.view, i32(dx.DT_CODE[dt]), i64(M), i64(N), i64(K), rc=rc)


@pytest.mark.parametrize("case", fx.D_CASES, ids=_id)
def test_fp8_gemm_add_norm_every_form(case):
    M, terms, N, K, dt, form = case
    assert fx.fp8_norm_form(M, terms, N, K) == form
    c, w = fx.norm_case(M, K, terms), fx.fp8_weight(N, K)
    exact = fx.fp8_exact(c, w)
    wq, ws, inp = w["w_q"].cuda(), w["w_s"].cuda(), _Inputs(c)
    n = 0
    for t in _types(dt):
        dtype = dx.DTYPES[t]
        what = f"chitu_hip_fp8_gemm_add_norm {_id(case)} out {t} (WK, term registers, MR) = {form}"
        out, s_out = rx.Guarded(M, N, dtype), rx.Guarded(M, K, BF16, stride=K + 8)
        _fp8_add_norm(inp, c, wq, ws, s_out, out, t, M, N, K)
        rx.assert_same(s_out.check(what + " sum_out"), c["v"], what + " sum_out")
        rx.assert_same(out.check(what), dx.expect(exact, dtype), what)
        inp.unchanged(what)
        n += M * N + M * K
    _ok("chitu_hip_fp8_gemm_add_norm", case, n)


@pytest.mark.parametrize("case", fx.D_REFUSED, ids=_id)
def test_fp8_gemm_add_norm_refuses_what_it_does_not_serve(case):
    M, terms, N, K = case
    assert fx.fp8_norm_form(M, terms, N, K) is None
    # (operands of the full size all the same: nothing may be read, but nothing could be read out of bounds either)
    x, add, nw = torch.zeros(M, K, dtype=BF16).cuda(), torch.zeros(M, terms, K, dtype=BF16).cuda(), torch.ones(K, dtype=BF16).cuda()
    wq, ws = torch.zeros(N, K, dtype=U8).cuda(), torch.ones((N + 127) // 128, (K + 127) // 128).cuda()
    out, s_out = rx.Guarded(M, N, BF16), rx.Guarded(M, K, BF16)
    _call("chitu_hip_fp8_gemm_add_norm", x, i64(K), add, i64(terms * K), i32(terms), i64(K), s_out.view, i64(K), nw, f32(1e-6), wq, ws, out.view,
          i32(0), i64(M), i64(N), i64(K), rc=ERR_UNSUPPORTED)
    out.untouched(f"refused {case} out")
    s_out.untouched(f"refused {case} sum_out")
    _ok("chitu_hip_fp8_gemm_add_norm", case, 0, " (CHITU_ERR_UNSUPPORTED, outputs untouched)")


# ---------------------------------------------------------------- E: mla_q_proj
def _q_proj(row_dev, stride, rank, qw, eps, wq, ws, out, dt, N, c_kv, cos, sin, pages, num_pages, page, table, lens, batch, rc=0):
    _call("chitu_hip_mla_q_proj", row_dev, i64(stride), i32(rank), qw.cuda(), f32(eps), wq, ws, out.view, i32(dx.DT_CODE[dt]), i64(N),
          c_kv["w"].cuda(), f32(rx.EPS), cos.cuda(), sin.cuda(), pages.inner, i64(num_pages), i32(page), table.cuda(), i32(table.shape[1]),
          lens.cuda(), i32(batch), i32(512), i32(64), rc=rc)


def _q_proj_rows(q_x, batch, seed):
    """[q_a | kv_c | k_pe] rows at a row stride with NaN filler columns."""
    kv_row, _, c_kv, k_pe, cos, sin = tr._mla_inputs(batch, 0, seed=seed)
    row = torch.cat([q_x, kv_row], 1)
    keep, view = tr._strided(row, row.shape[1] + 24)
    return keep, view, row.shape[1] + 24, c_kv, k_pe, cos, sin


@pytest.mark.parametrize("case", fx.E_CASES, ids=_id)
def test_mla_q_proj_every_tile_form_and_rank(case):
    batch, rank, N, dt, bad = case
    eps = fx.EPS_LIST[batch % 2]
    c, w = fx.norm_case(batch, rank, 0, eps, seed=1), fx.fp8_weight(N, rank)
    exact = fx.fp8_exact(c, w)
    page = [16, 48][batch % 2]
    lens, table, num_pages, _, kinds = rx.paged_batch(batch, page, seed=rank // 128 + batch, bad=bad and batch >= 4)
    keep, rows, stride, c_kv, k_pe, cos, sin = _q_proj_rows(c["x"], batch, seed=50 + batch)
    wq, ws = w["w_q"].cuda(), w["w_s"].cuda()
    n = 0
    for t in _types(dt):
        dtype = dx.DTYPES[t]
        what = f"chitu_hip_mla_q_proj {_id(case)} out {t} blocks per wave {fx.qproj_blocks(rank)} {kinds}"
        out = rx.Guarded(batch, N, dtype)
        pages = tr._Pages(num_pages, page, (576,), BF16, seed=6)
        _q_proj(rows, stride, rank, c["w"], eps, wq, ws, out, t, N, c_kv, cos, sin, pages, num_pages, page, table, lens, batch)
        rx.assert_same(out.check(what), dx.expect(exact, dtype), what)
        tr._check_mla_cache(pages, c_kv, k_pe, cos, sin, lens, table, num_pages, what)
        n += batch * N
    _ok("chitu_hip_mla_q_proj", case, n)


@pytest.mark.parametrize("case", fx.E_REFUSED, ids=_id)
def test_mla_q_proj_refuses_what_it_does_not_serve(case):
    batch, rank = case
    lens, table, num_pages, _, _ = rx.paged_batch(batch, 16, seed=1)
    kv_row, _, c_kv, k_pe, cos, sin = tr._mla_inputs(batch, 0, seed=3)
    stride = (rank + 576 + 7) // 8 * 8 + 8
    rows = torch.zeros(batch, stride, dtype=BF16).cuda()
    out = rx.Guarded(batch, 40, BF16)
    pages = tr._Pages(num_pages, 16, (576,), BF16, seed=6)
    qw = torch.ones(rank, dtype=BF16)
    wq, ws = torch.zeros(40, rank, dtype=U8).cuda(), torch.ones(1, (rank + 127) // 128).cuda()
    _q_proj(rows, stride, rank, qw, 1e-6, wq, ws, out, "bf16", 40, c_kv, cos, sin, pages, num_pages, 16, table, lens, batch, rc=ERR_UNSUPPORTED)
    out.untouched(f"refused {case}")
    pages.check(pages.inner_init(), f"refused {case}")
    _ok("chitu_hip_mla_q_proj", case, 0, " (CHITU_ERR_UNSUPPORTED, output and cache untouched)")


# ---------------------------------------------------------------- F: W_UK bmm + RoPE(q_pe) + the KV rider
def _absorb_kv_case(case):
    B, H, N, K, st, bad = case
    c = dx.absorb_case(B, H, N, K, st)
    q, cos, sin, q_want = dx.rope_case(B, H, seed=B + H + N + K)
    kv_row, _, c_kv, k_pe, _, _ = tr._mla_inputs(B, 0, seed=80 + B + H)   # (the launch has ONE cos / sin: the quarter turns)
    page = [16, 48][(B + H) % 2]
    lens, table, num_pages, _, kinds = rx.paged_batch(B, page, seed=N // 16 + K, bad=bad)
    return c, q, cos, sin, q_want, kv_row, c_kv, k_pe, page, lens, table, num_pages, kinds


@pytest.mark.parametrize("case", fx.F_CASES, ids=_id)
def test_absorb_bmm_rope_kv(case):
    B, H, N, K, st, bad = case
    c, q, cos, sin, q_want, kv_row, c_kv, k_pe, page, lens, table, num_pages, kinds = _absorb_kv_case(case)
    keep, head, (sh, sn, sk) = td._absorb_args(c, B, H, N, K)
    _, kv_in = tr._strided(kv_row, 576 + 64)
    out = rx.Guarded(B * H, N, BF16)
    q_dev = q.cuda()
    pages = tr._Pages(num_pages, page, (576,), BF16, seed=9)
    x, x_sb, x_sh, w, w_sh, scale, off = head   # (pointers of tensors that `keep` holds)
    _call("chitu_hip_absorb_bmm_rope_kv_fp8", x, x_sb, x_sh, w, w_sh, scale, off, i64(sh), i64(sn), i64(sk), out.view, i64(H * N), i64(N), i32(B),
          i32(H), i32(N), i32(K), q_dev[dx.G:], i64(H * 64), i64(64), cos.cuda(), sin.cuda(), i32(64), kv_in, i64(640), c_kv["w"].cuda(), f32(rx.EPS),
          pages.inner, i64(num_pages), i32(page), table.cuda(), i32(table.shape[1]), lens.cuda(), i32(512))
    what = f"chitu_hip_absorb_bmm_rope_kv_fp8 {_id(case)} {kinds}"
    rx.assert_same(out.check(what), dx.expect(c["exact"], BF16).reshape(B * H, N), what + " out")
    rx.assert_same(q_dev.cpu().view(-1, 64), q_want.view(-1, 64), what + " q_pe in place (guard tokens untouched)")
    tr._check_mla_cache(pages, c_kv, k_pe, cos, sin, lens, table, num_pages, what)
    del keep
    _ok("chitu_hip_absorb_bmm_rope_kv_fp8", case, B * H * (N + 64))


# ---------------------------------------------------------------- G: merge + W_UV + act_quant on a hand-built workspace
@pytest.mark.parametrize("case", fx.G_CASES, ids=_id)
def test_mla_merge_absorb_uv_quant_row_and_tile_major(case):
    B, H, S, st = case
    mc, ac = fx.merge_case(B, H, S), dx.absorb_case(B, H, 128, 512, st)
    q_want, s_want = fx.merge_expect(mc, ac)
    sh, sn, sk = ac["strides"]
    wsb, w, scale = fx.merge_workspace(mc).cuda(), ac["w_store"].cuda(), ac["scale"].cuda()
    head = (wsb, i32(S), w, i64(w.stride(0)), scale, i64(dx.ABSORB_OFFSET), i64(sh), i64(sk))
    what = f"chitu_hip_mla_merge_absorb_uv_quant_fp8 {_id(case)} (live splits per (b, h): {sorted(set(mc['live'].tolist()))}, dead (b, h) {mc['dead']})"
    q, qs = rx.Guarded(B, H * 128, U8), rx.Guarded(B, H, F32)
    _call("chitu_hip_mla_merge_absorb_uv_quant_fp8", *head, q.view, qs.view, i32(B), i32(H), i32(512))
    rx.assert_same(qs.check(what + " scales"), s_want, what + " scales")
    rx.assert_same(q.check(what + " codes", written=False), q_want.view(U8), what + " codes", nan_ok=True)
    # tile-major: the padding rows and scales of the last tile keep the sentinel
    T = (B + 15) // 16
    qt_want, st_want = rx.to_tile_major(q_want.view(U8), s_want)
    qt, qst = rx.Guarded(T * 16, H * 128, U8), rx.Guarded(T * H, 16, F32)
    _call("chitu_hip_mla_merge_absorb_uv_quant_fp8_tm", *head, qt.view, qst.view, i32(B), i32(H), i32(512))
    rx.assert_same(qt.check(what + " tile-major codes", written=False), qt_want, what + " tile-major codes (padding rows = sentinel)", nan_ok=True)
    got_s = qst.check(what + " tile-major scales", written=False)
    rx.assert_same(rx.bits(got_s), st_want.reshape(T * H, 16), what + " tile-major scales (padding rows = sentinel)")
    _ok("chitu_hip_mla_merge_absorb_uv_quant_fp8[_tm]", case, 2 * (B * H * 128 + B * H))


# ---------------------------------------------------------------- I: the full-mantissa family behind an identity weight
@pytest.mark.parametrize("case", fx.D_IDENT, ids=_id)
def test_fp8_gemm_add_norm_full_mantissa_rows_behind_an_identity(case):
    M, K, terms = case
    ic = fx.ident_case(M, K, terms)
    c = dict(ic["c"], rows=M, dim=K, terms=terms, eps=rx.EPS)
    c["add"] = c["add"].reshape(M, terms, K)
    inp = _Inputs(c)
    wq, ws = fx.ident_fp8_weight(K)
    out, s_out = rx.Guarded(M, K, F32), rx.Guarded(M, K, BF16, stride=K + 8)
    what = f"chitu_hip_fp8_gemm_add_norm identity {_id(case)}"
    _fp8_add_norm(inp, c, wq.cuda(), ws.cuda(), s_out, out, "f32", M, K, K)
    rx.assert_same(s_out.check(what + " sum_out"), c["v"], what + " sum_out")
    idx = rx.match_rows(out.check(what), ic["t"], ic["rr"], ic["fp8_out"], what + " (codes x scale of act_quant(candidate row))")
    _ok("chitu_hip_fp8_gemm_add_norm identity", case, M * K, f", {int((idx != 0).sum())} of {M} rows took a non-central rsqrt candidate")


@pytest.mark.parametrize("case", fx.A_IDENT, ids=_id)
def test_bf16_gemm_add_norm_full_mantissa_rows_behind_an_identity(case):
    M, K, terms = case
    ic = fx.ident_case(M, K, terms)
    c = dict(ic["c"], rows=M, dim=K, terms=terms, eps=rx.EPS)
    c["add"] = c["add"].reshape(M, terms, K)
    inp = _Inputs(c)
    out, s_out = rx.Guarded(M, K, F32), rx.Guarded(M, K, BF16, stride=K + 8)
    what = f"chitu_hip_bf16_gemm_add_norm identity {_id(case)}"
    _bf16_add_norm(inp, c, torch.eye(K, dtype=BF16).cuda(), s_out.view, K + 8, out.view, "f32", M, K, K)
    rx.assert_same(s_out.check(what + " sum_out"), c["v"], what + " sum_out")
    idx = rx.match_rows(out.check(what), ic["t"], ic["rr"], ic["bf16_out"], what + " (the candidate row itself)")
    _ok("chitu_hip_bf16_gemm_add_norm identity", case, M * K, f", {int((idx != 0).sum())} of {M} rows took a non-central rsqrt candidate")


@pytest.mark.parametrize("case", fx.E_IDENT, ids=_id)
def test_mla_q_proj_full_mantissa_rows_behind_an_identity(case):
    batch, rank = case
    ic = fx.ident_case(batch, rank, 0, seed=2)
    lens, table, num_pages, _, kinds = rx.paged_batch(batch, 16, seed=rank // 128)
    keep, rows, stride, c_kv, k_pe, cos, sin = _q_proj_rows(ic["c"]["x"], batch, seed=70 + batch)
    wq, ws = fx.ident_fp8_weight(rank)
    out = rx.Guarded(batch, rank, F32)
    pages = tr._Pages(num_pages, 16, (576,), BF16, seed=6)
    what = f"chitu_hip_mla_q_proj identity {_id(case)}"
    _q_proj(rows, stride, rank, ic["c"]["w"], rx.EPS, wq.cuda(), ws.cuda(), out, "f32", rank, c_kv, cos, sin, pages, num_pages, 16, table, lens, batch)
    idx = rx.match_rows(out.check(what), ic["t"], ic["rr"], ic["fp8_out"], what + " (codes x scale of act_quant(candidate row))")
    tr._check_mla_cache(pages, c_kv, k_pe, cos, sin, lens, table, num_pages, what)
    _ok("chitu_hip_mla_q_proj identity", case, batch * rank, f", {int((idx != 0).sum())} of {batch} rows took a non-central rsqrt candidate")


# ---------------------------------------------------------------- H: the ops wrappers
def _twice(fn, want, what):
    """fn() -> tuple of tensors, outside and inside poisoned_allocations(): equal to each other and to the expectation."""
    plain = [t.cpu() for t in fn()]
    with poisoned_allocations():
        foul = [t.cpu() for t in fn()]
    for i, (a, b, w) in enumerate(zip(plain, foul, want)):
        rx.assert_same(a, b, f"{what} output {i}: poisoned allocations change it", nan_ok=True)
        if w is not None:
            rx.assert_same(a, w, f"{what} output {i}", nan_ok=True)
    _ok("ops." + what, (), sum(t.numel() for t in plain), " (inside poisoned_allocations() == outside == the expectation)")


def test_ops_bf16_linear_add_norm_wrappers():
    from chitu_amd import ops

    M, N, K = 3, 136, 1024
    c, w = fx.norm_case(M, K, 2), fx.bf16_weight(N, K)
    x, add, nw, wd = c["x"].cuda(), c["add"].cuda().contiguous(), c["w"].cuda(), w["w_q"].cuda()
    _twice(lambda: ops.bf16_linear_add_norm(x, add, nw, c["eps"], wd, out_dtype=F32), [c["v"], dx.expect(fx.bf16_exact(c, w), F32)],
           "bf16_linear_add_norm")
    c, w = fx.norm_case(M, K, 1), fx.silu_weight(N, K)
    cand, _ = fx.silu_expect(c, w, N)
    x, add = c["x"].cuda(), c["add"][:, 0].contiguous().cuda()
    got = ops.bf16_linear_silu_add_norm(x, add, c["w"].cuda(), c["eps"], w["w_q"].cuda())[1].cpu()
    rx.silu_match(got.reshape(-1, 1), cand, "ops.bf16_linear_silu_add_norm")
    _twice(lambda: ops.bf16_linear_silu_add_norm(x, add, c["w"].cuda(), c["eps"], w["w_q"].cuda()), [c["v"], got], "bf16_linear_silu_add_norm")


def test_ops_bf16_linear_add_norm_qkv_post_wrapper():
    from chitu_amd import ops

    case = (4, 4, 64, 1024, 4, 16, "valid")
    hq, hkv, d, K, M, page, _ = case
    N, c, w, heads, cos, sin, rot, lens, table, num_pages, kinds = _qkv_case(case)

    def run():
        kc, vc = tr._Pages(num_pages, page, (hkv, d), BF16, seed=7), tr._Pages(num_pages, page, (hkv, d), BF16, seed=8)
        k4, v4 = (p.inner[: num_pages * page].view(num_pages, page, hkv, d) for p in (kc, vc))
        x_new, qkv = ops.bf16_linear_add_norm_qkv_post(c["x"].cuda(), c["add"][:, 0].contiguous().cuda(), c["w"].cuda(), c["eps"], w["w_q"].cuda(),
                                                       hq, hkv, cos.cuda(), sin.cuda(), k4, v4, table.cuda(), lens.cuda())
        return x_new, qkv[:, :hq].contiguous(), k4.clone(), v4.clone()

    kc0, vc0 = tr._Pages(num_pages, page, (hkv, d), BF16, seed=7), tr._Pages(num_pages, page, (hkv, d), BF16, seed=8)
    want = [c["v"], rot[:, :hq].contiguous(),
            rx.append_oracle(kc0.inner_init(), rot[:, hq:], lens, table, page, num_pages).view(num_pages, page, hkv, d),
            rx.append_oracle(vc0.inner_init(), heads[:, hq + hkv:], lens, table, page, num_pages).view(num_pages, page, hkv, d)]
    _twice(run, want, "bf16_linear_add_norm_qkv_post")


def test_ops_fp8_linear_add_norm_and_mla_q_proj_wrappers():
    from chitu_amd import ops

    M, terms, N, K = 1, 9, 136, 2048
    c, w = fx.norm_case(M, K, terms), fx.fp8_weight(N, K)
    x, add = c["x"].cuda(), c["add"].contiguous().cuda()
    _twice(lambda: ops.fp8_linear_add_norm(x, add, c["w"].cuda(), c["eps"], w["w_q"].cuda(), w["w_s"].cuda(), out_dtype=F32),
           [c["v"], dx.expect(fx.fp8_exact(c, w), F32)], "fp8_linear_add_norm")
    batch, rank, N = 17, 1536, 200
    c, w = fx.norm_case(batch, rank, 0, seed=1), fx.fp8_weight(N, rank)
    kv_row, _, c_kv, k_pe, cos, sin = tr._mla_inputs(batch, 0, seed=67)
    rows = torch.cat([c["x"], kv_row], 1).cuda()
    lens, table, num_pages, _, kinds = rx.paged_batch(batch, 16, seed=5)
    seen = []

    def run():
        pages = tr._Pages(num_pages, 16, (576,), BF16, seed=6)
        cache = pages.inner[: num_pages * 16].view(num_pages, 16, 576)
        out = ops.mla_q_proj(rows, rank, c["w"].cuda(), c["eps"], w["w_q"].cuda(), w["w_s"].cuda(), c_kv["w"].cuda(), rx.EPS, cos.cuda(), sin.cuda(),
                             cache, table.cuda(), lens.cuda(), out_dtype=F32)
        torch.cuda.synchronize()
        tr._check_mla_cache(pages, c_kv, k_pe, cos, sin, lens, table, num_pages, "ops.mla_q_proj")
        seen.append(pages.dev.cpu())
        return (out,)

    _twice(run, [dx.expect(fx.fp8_exact(c, w), F32)], "mla_q_proj")
    assert torch.equal(rx.bits(seen[0]), rx.bits(seen[1])), "ops.mla_q_proj: poisoned allocations change the cache"


def test_ops_absorb_bmm_rope_kv_and_merge_wrappers():
    from chitu_amd import ops

    case = (17, 5, 128, 192, "w_uk", False)
    B, H, N, K, st, _ = case
    c, q, cos, sin, q_want, kv_row, c_kv, k_pe, page, lens, table, num_pages, kinds = _absorb_kv_case(case)
    sh, sn, sk = c["strides"]
    wide = torch.zeros(B, H, K + 64, dtype=BF16)
    wide[..., :K] = c["x"]
    x = wide.cuda()[..., :K]
    w_dev, scale = c["w_store"].cuda(), c["scale"].cuda()
    w3 = torch.as_strided(w_dev, (H, N, K), (w_dev.stride(0), K, 1))
    seen = []

    def run():
        q_dev = q.cuda()
        pages = tr._Pages(num_pages, page, (576,), BF16, seed=9)
        cache = pages.inner[: num_pages * page].view(num_pages, page, 576)
        out = ops.absorb_bmm_rope_kv_fp8(x, w3, scale, dx.ABSORB_OFFSET, sh, sn, sk, q_dev[dx.G:dx.G + B], cos.cuda(), sin.cuda(), kv_row.cuda(),
                                         c_kv["w"].cuda(), rx.EPS, cache, table.cuda(), lens.cuda())
        torch.cuda.synchronize()
        tr._check_mla_cache(pages, c_kv, k_pe, cos, sin, lens, table, num_pages, "ops.absorb_bmm_rope_kv_fp8")
        seen.append(pages.dev.cpu())
        return out, q_dev

    _twice(run, [dx.expect(c["exact"], BF16), q_want], "absorb_bmm_rope_kv_fp8")
    assert torch.equal(rx.bits(seen[0]), rx.bits(seen[1])), "ops.absorb_bmm_rope_kv_fp8: poisoned allocations change the cache"
    B, H, S = 17, 5, 17
    mc, ac = fx.merge_case(B, H, S), dx.absorb_case(B, H, 128, 512, "w_uv")
    q_want, s_want = fx.merge_expect(mc, ac)
    sh, sn, sk = ac["strides"]
    w_dev, scale, wsb = ac["w_store"].cuda(), ac["scale"].cuda(), fx.merge_workspace(mc).cuda()
    w3 = torch.as_strided(w_dev, (H, 128, 512), (w_dev.stride(0), 512, 1))
    _twice(lambda: ops.mla_merge_absorb_uv_quant_fp8(wsb, S, B, w3, scale, dx.ABSORB_OFFSET, sh, sk), [q_want, s_want], "mla_merge_absorb_uv_quant_fp8")

    def run_tm():
        tq, _ = ops.mla_merge_absorb_uv_quant_fp8(wsb, S, B, w3, scale, dx.ABSORB_OFFSET, sh, sk, tile_major=True)
        return tq.to_row_major()

    _twice(run_tm, [q_want, s_want], "mla_merge_absorb_uv_quant_fp8(tile_major)")
