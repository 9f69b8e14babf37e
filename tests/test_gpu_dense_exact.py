"""The dense GEMM family on exact integer data: every launch variant, every store edge, guarded outputs.

The other dense-GEMM tests feed randn data and compare against the tensor's peak; here (builders: tests/dense_exact.py, their
CPU checks: tests/test_dense_exact_host.py) the operands are small integers with power-of-two scales that differ between
neighbouring tokens and blocks, every partial sum is exact in fp32 in any order, and the assertion is torch.equal against the
float64 matmul rounded once.  Every entry is called through the C ABI with its output between G guard rows of a NaN sentinel,
the output itself pre-filled with the sentinel: after each launch the guards are untouched and no output element still holds
it.  Every case is run with an fp32 output (the exact value itself) and, where it names another type, in that type too.

  A  chitu_hip_fp8_gemm_blockscale, streaming: token-tile forms 1 / 2 / 4 and a second 64-row pass x fp8_gemm_wk, the DEEP ring
  B  chitu_hip_fp8_gemm_blockscale_tm on the permuted operands
  C  chitu_hip_fp8_gemm_blockscale_partials: every plane is the contraction over its own K range
  D  the in-library split (plan S > 1: fp32 planes in the workspace + the reduce launch) and its small-workspace fallback
  E  the tiled fp8 GEMM (M >= 128) at both tile heights, and the streaming kernel on the same inputs
  F  chitu_hip_bf16_gemm: streaming x bf16_gemm_wk, DEEP ring, split-K planes; tiled at both heights, split-K, the empty share
  G  chitu_hip_bf16_gemm_silu x bf16_silu_wk
  H  chitu_hip_soft_fp8_gemm
  I  absorb.hip: bmm, bmm + RoPE, W_UV + act_quant, with a NaN-filled scale tensor under three stride sets
  J  chitu_hip_w8a8_int8_gemm
  K  the ops wrappers inside tests.util.poisoned_allocations() == outside it

Mutations tried by hand on the MI355X (other builds of the library, never committed; each run once; all of them change only
computed values or move a store inside the guarded buffer) and what caught them here:
  - fp8_gemm.hip, fp8_gemm_kernel: the weight scale of K block kb read from kb + 1 (`wsp[min(kb + 1, KB - 1)]`): 72 cases of
    sections A to E and K, every one with K > 128, e.g. test_fp8_gemm_partial_planes...[70-136-384-2] "18949 of 19040 elements
    differ from the exact result in 140 rows ... (0, 0, -424.0, -848.0)" (a factor of two: the neighbour's power of two).
  - fp8_gemm.hip, `kb1 - 1` for kb1 in wave 1: 60 cases of A to E and K (all with WK >= 2 and more than one block in wave 1),
    e.g. test_fp8_gemm_partial_planes...[70-136-2048-2] "18961 of 19040 elements differ".
  - gemm_common.h, gemm_epilogue_v2: the wave-order reduce stops before the last wave (`w < WK - 1`): 60 cases of A to E and K again.
  - gemm_common.h, gemm_epilogue_v2: `if (m >= M + 1) return` on the S = 1 paths (a store to row M; run against sections A
    and B only, where that row is a guard row): 22 cases, every M that is no multiple of 16 -- "chitu_hip_fp8_gemm_blockscale_tm
    M=17 N=136 K=128 fp8_gemm_wk=-1 out f32: stored into the guard rows after the output, first (row, col): [[0, 0], [0, 1], ..."
  - fp8_gemm.hip, tile-major scale address `(m + 1) & 15` for `m & 15` (the neighbouring token's scale): every M (six then) of
    test_fp8_gemm_tile_major_every..., the tile-major DEEP cases and ops.fp8_gemm_deepseek_v3 (tile-major) of section K;
    no row-major case.
  - bf16_gemm_tiled.hip: the empty K share returns without zeroing its plane: the four K = 320, S = 4 cases of
    test_bf16_gemm_tiled_at_both_heights_split_k_and_streamed, "2400 output elements never written, first (row, col): [[900, 0], ..."
    (plane 3 of 300 rows); test_bf16_gemm_tiled_split_k_planes_sum_to_the_gemm has no empty share.
  - absorb.hip, absorb_bmm_kernel: the scale of K block 0 for every K block: every case of section I with K >= 192 and a
    non-zero K stride (16 of 24) and ops.absorb_bmm_fp8 of section K; the w_uk stride set (K stride 0) rightly not.
  - fp8_gemm.hip, splitk_reduce_kernel: `s < S - 1`: all eight cases of section D, fp8 and soft, in the run with the full
    workspace ("workspace 236096 B (S=7) out f32: 8431 of 8432 elements differ"); nothing else reaches that kernel.
  - bf16_gemm_kernel (then in gate.hip, now stream_gemm.h through bf16_gemm.hip): `kb1 - 1` in wave 0 where it has more than one block: 37 cases of section F (streaming, DEEP
    ring, split-K planes, and the tiled shapes streamed with bf16_gemm_tiled = 0).
  - w8a8_int8.hip: the channel scale of n + 1 for n: all five M of section J, "1555 of 1600 elements differ ... in 40 rows;
    worst row 0 (39 elements)" (the last channel reads its own scale).
Not tried: dropping the `(N & 1) == 0` test of the packed 16-bit store alone.  With `n + 1 < N` still in place the pair stays
inside its row, so the only effect is a misaligned 4-byte store -- nothing a comparison can see, and not something to run.
"""

import contextlib
import ctypes

import pytest
import torch

from oracle import fp8 as ofp8
from tests import dense_exact as dx
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -2
F32, BF16 = torch.float32, torch.bfloat16


def _id(case):
    return "-".join(str(v) for v in case)


def _abi():
    from chitu_amd import _lib

    return _lib


@contextlib.contextmanager
def _options(**opts):
    """debug options forced for the block (-1 = the launcher's own heuristic)."""
    from chitu_amd._lib import debug_option

    with contextlib.ExitStack() as stack:
        for name, value in opts.items():
            stack.enter_context(debug_option(name, value))
        yield


def _nan_workspace(nbytes):
    """A workspace of exactly nbytes bytes (rounded up to whole floats), every float a NaN."""
    return torch.full(((nbytes + 3) // 4,), float("nan"), dtype=F32, device="cuda")


def _types(dt):
    return ["f32"] if dt == "f32" else ["f32", dt]


def _finish(rc, entry, full, dtype, want, what, planes=None):
    from chitu_amd._lib import check

    check(rc, entry)
    torch.cuda.synchronize()
    got = dx.check_guarded(full, dtype, what, planes)
    dx.assert_equal(got, want, what)  # (torch.equal, with the worst row and the first positions in the message)
    return got


# ---------------------------------------------------------------- A, B, D, E: the W8A8 block-scaled GEMM
def _fp8_gemm(c, M, N, K, dt, what, tile_major=False, ws_bytes=None, expect_rc=0):
    """One launch of chitu_hip_fp8_gemm_blockscale[_tm] with a guarded output of type dt and a NaN-filled workspace (of
    8 M N floats, or of exactly ws_bytes bytes): guards, sentinels, torch.equal."""
    lib = _abi()
    from chitu_amd._lib import i64, ptr, stream_ptr

    dtype = dx.DTYPES[dt]
    a_q, a_s = dx.to_tile_major(c["a_q"], c["a_s"]) if tile_major else (c["a_q"], c["a_s"])
    dev = [a_q.cuda(), a_s.float().cuda(), c["w_q"].cuda(), c["w_s"].float().cuda()]
    full, out = dx.guarded(M, N, dtype)
    nbytes = 8 * M * N * 4 if ws_bytes is None else ws_bytes
    ws = _nan_workspace(nbytes)
    entry = "chitu_hip_fp8_gemm_blockscale_tm" if tile_major else "chitu_hip_fp8_gemm_blockscale"
    rc = getattr(lib.lib(), entry)(*(ptr(t) for t in dev), ptr(out), ctypes.c_int(dx.DT_CODE[dt]), i64(M), i64(N), i64(K),
                                   ptr(ws), i64(nbytes), stream_ptr())
    if expect_rc:
        assert rc == expect_rc, (what, rc)
        return None
    _finish(rc, entry, full, dtype, dx.expect(c["exact"], dtype), f"{entry} {what} out {dt}")
    return ws


@pytest.mark.parametrize("M", dx.A_M)
def test_fp8_gemm_streaming_every_token_tile_form_and_wave_split(M):
    """Section A: the row-major streaming kernel at this M under fp8_gemm_wk = heuristic, 1, 2, 4, 8, each at a K with at least
    that many blocks so that it is launched as forced (N, K and the output type cycle through 8 / 129 / 136 / 272,
    128 / 384 / 1024 / 5120 and fp32 / bf16 / f16).  tests/test_dense_exact_host.py shows from the launcher's mirror that
    every (token-tile form, launched WK) pair occurs."""
    for m, N, K, wk, dt in [c for c in dx.A_CASES if c[0] == M]:
        assert wk < 0 or dx.fp8_wk(N, K, wk) == wk  # K has at least wk blocks: the forced split is the launched one
        c = dx.fp8_case(M, N, K)
        for t in _types(dt):
            with _options(fp8_gemm_wk=wk):
                _fp8_gemm(c, M, N, K, t, f"M={M} N={N} K={K} fp8_gemm_wk={wk} (launches WK {dx.fp8_wk(N, K, wk)})")


@pytest.mark.parametrize("case", dx.A_DEEP, ids=_id)
def test_fp8_gemm_streaming_deep_ring_on_and_off(case):
    """K = 5120 at M <= 16 is 5 K blocks per wave at WK = 8: the DEEP ring (fp8_gemm_deep 1) and the 4-deep ring (0)."""
    M, N, K, wk, deep, dt = case
    assert dx.fp8_wk(N, K, wk) == 8 and 4 < (K // 128) // 8 <= 8
    c = dx.fp8_case(M, N, K)
    for t in _types(dt):
        with _options(fp8_gemm_wk=wk, fp8_gemm_deep=deep):
            _fp8_gemm(c, M, N, K, t, f"M={M} N={N} K={K} fp8_gemm_wk={wk} fp8_gemm_deep={deep}")


@pytest.mark.parametrize("M", dx.B_M)
def test_fp8_gemm_tile_major_every_token_tile_form_and_wave_split(M):
    """Section B: the same matrix through chitu_hip_fp8_gemm_blockscale_tm on the permuted operands (the rows padding the last
    tile hold NaN codes and scales).  Equal to the expectation, hence to the row-major entry's bits."""
    for m, N, K, wk, dt in [c for c in dx.B_CASES if c[0] == M]:
        assert wk < 0 or dx.fp8_wk(N, K, wk) == wk
        c = dx.fp8_case(M, N, K)
        for t in _types(dt):
            with _options(fp8_gemm_wk=wk):
                _fp8_gemm(c, M, N, K, t, f"M={M} N={N} K={K} fp8_gemm_wk={wk}", tile_major=True)


@pytest.mark.parametrize("case", dx.B_DEEP, ids=_id)
def test_fp8_gemm_tile_major_deep_ring_on_and_off(case):
    M, N, K, wk, deep, dt = case
    c = dx.fp8_case(M, N, K)
    for t in _types(dt):
        with _options(fp8_gemm_wk=wk, fp8_gemm_deep=deep):
            _fp8_gemm(c, M, N, K, t, f"M={M} N={N} K={K} fp8_gemm_wk={wk} fp8_gemm_deep={deep}", tile_major=True)


def test_fp8_gemm_tile_major_round_trip_and_the_tiled_threshold():
    """The host permutation is what ops.TiledQuant.to_row_major inverts, on the device too; 128 rows are refused."""
    from chitu_amd import ops

    c = dx.fp8_case(33, 136, 384)
    qt, st = dx.to_tile_major(c["a_q"], c["a_s"])
    q, s = ops.TiledQuant(qt.cuda(), st.cuda(), 33, 384).to_row_major()
    assert torch.equal(q.cpu().view(torch.uint8), c["a_q"].view(torch.uint8)) and torch.equal(s.cpu(), c["a_s"])
    _fp8_gemm(dx.fp8_case(128, 8, 128), 128, 8, 128, "f32", "M=128", tile_major=True, expect_rc=ERR_UNSUPPORTED)


@pytest.mark.parametrize("case", dx.C_CASES, ids=_id)
def test_fp8_gemm_partial_planes_are_the_contraction_over_their_own_k_range(case):
    """Section C: chitu_hip_fp8_gemm_blockscale_partials, guards around the plane stack."""
    lib = _abi()
    from chitu_amd._lib import i32, i64, ptr, stream_ptr

    M, N, K, S = case
    c = dx.fp8_case(M, N, K)
    want = torch.stack([dx.expect(c["a_deq"][:, k0:k1] @ c["w_deq"][:, k0:k1].T, F32) for k0, k1 in dx.partials_ranges(K, S)])
    dev = [c["a_q"].cuda(), c["a_s"].float().cuda(), c["w_q"].cuda(), c["w_s"].float().cuda()]
    full, planes = dx.guarded(M, N, F32, planes=S)
    rc = lib.lib().chitu_hip_fp8_gemm_blockscale_partials(*(ptr(t) for t in dev), ptr(planes), i64(M), i64(N), i64(K), i32(S), stream_ptr())
    _finish(rc, "chitu_hip_fp8_gemm_blockscale_partials", full, F32, want, f"partials M={M} N={N} K={K} S={S}", planes=S)


def _soft_gemm(c, M, N, K, dt, what, ws_bytes=None):
    lib = _abi()
    from chitu_amd._lib import i64, ptr, stream_ptr

    dtype = dx.DTYPES[dt]
    dev = [c["a_q"].cuda(), c["w_q"].cuda(), c["w_s"].float().cuda()]
    full, out = dx.guarded(M, N, dtype)
    nbytes = 8 * M * N * 4 if ws_bytes is None else ws_bytes
    ws = _nan_workspace(nbytes)
    rc = lib.lib().chitu_hip_soft_fp8_gemm(*(ptr(t) for t in dev), ptr(out), ctypes.c_int(dx.DT_CODE[dt]), i64(M), i64(N), i64(K),
                                           ptr(ws), i64(nbytes), stream_ptr())
    _finish(rc, "chitu_hip_soft_fp8_gemm", full, dtype, dx.expect(c["exact"], dtype), f"chitu_hip_soft_fp8_gemm {what} out {dt}")
    return ws


@pytest.mark.parametrize("entry", ["fp8", "soft"])
@pytest.mark.parametrize("case", dx.D_CASES, ids=_id)
def test_in_library_split_with_its_reduce_launch_and_the_small_workspace_fallback(case, entry):
    """Section D: (N, K) = (496, 50816) and (24, 2^20) are the shapes at which plan_split cuts K over S = 7 and S = 8 workgroups
    per tile (WK 8): fp32 planes in the workspace, then splitk_reduce_kernel.  With a NaN-filled workspace of exactly
    S M N 4 bytes the split runs; with one byte less the launcher falls back to S = 1.  Both return the same exact result.
    The run itself shows which path was taken: after the split every one of the S M N floats of the workspace is finite (the
    planes were written), after the fallback every one is still NaN (nothing was).
    (The 2^20-long contraction draws its integers from -1..1 so that the 2^24 bound holds.)"""
    M, N, K, lim, dt = case
    wk, S = dx.plan_split(N, K)
    assert (wk, S) == {(496, 50816): (8, 7), (24, 1048576): (8, 8)}[N, K]
    c = (dx.fp8_case if entry == "fp8" else dx.soft_case)(M, N, K, lim)
    run = _fp8_gemm if entry == "fp8" else _soft_gemm
    for nbytes, plan in ((S * M * N * 4, f"S={S}"), (S * M * N * 4 - 1, "the S=1 fallback")):
        for t in _types(dt):
            ws = run(c, M, N, K, t, f"M={M} N={N} K={K} workspace {nbytes} B ({plan})", ws_bytes=nbytes).cpu()
            assert ws.numel() == S * M * N
            if nbytes == S * M * N * 4:
                assert bool(torch.isfinite(ws).all()), f"{entry} {case}: {int((~torch.isfinite(ws)).sum())} plane elements unwritten: the split did not run"
            else:
                assert bool(torch.isnan(ws).all()), f"{entry} {case}: the fallback wrote {int((~torch.isnan(ws)).sum())} workspace elements"


@pytest.mark.parametrize("case", dx.E_CASES, ids=_id)
def test_fp8_gemm_tiled_at_both_heights_and_streamed(case):
    """Section E: M >= 128 takes the tiled kernel (fp8_tiled_tm 64 / 128 / heuristic; 257 x 264 is a 3 x 3 grid of 128-tiles whose
    XCD-blocked order launches padding workgroups); fp8_gemm_tiled = 0 streams the same inputs in 64-row passes.  The scaled
    16x16x128 MFMA sums 128 integer products of magnitude <= 16: exact."""
    M, N, K, tm, dt = case
    c = dx.fp8_case(M, N, K)
    for t in _types(dt):
        with _options(fp8_tiled_tm=tm):
            _fp8_gemm(c, M, N, K, t, f"tiled M={M} N={N} K={K} fp8_tiled_tm={tm}")
    with _options(fp8_gemm_tiled=0):
        _fp8_gemm(c, M, N, K, dt, f"streamed (fp8_gemm_tiled=0) M={M} N={N} K={K}")


# ---------------------------------------------------------------- F, G: bf16
def _bf16_gemm(c, M, N, K, dt, what, S=1, ranges=None, expect_rc=0):
    lib = _abi()
    from chitu_amd._lib import i32, i64, ptr, stream_ptr

    dev = [c["a_q"].cuda(), c["w_q"].cuda()]
    if S == 1:
        dtype = dx.DTYPES[dt]
        full, out = dx.guarded(M, N, dtype)
        args, want, planes = (ptr(out), ctypes.c_int(dx.DT_CODE[dt]), i64(M), i64(N), i64(K), i32(1), ptr(None)), dx.expect(c["exact"], dtype), None
    else:
        dtype = F32
        full, out = dx.guarded(M, N, F32, planes=S)
        args, planes = (ptr(None), ctypes.c_int(0), i64(M), i64(N), i64(K), i32(S), ptr(out)), S
        want = None if expect_rc else torch.stack([dx.expect(c["a_deq"][:, k0:k1] @ c["w_deq"][:, k0:k1].T, F32) for k0, k1 in ranges])
    rc = lib.lib().chitu_hip_bf16_gemm(ptr(dev[0]), ptr(dev[1]), *args, stream_ptr())
    if expect_rc:
        assert rc == expect_rc, (what, rc)
        return
    _finish(rc, "chitu_hip_bf16_gemm", full, dtype, want, f"chitu_hip_bf16_gemm {what} out {dt if S == 1 else 'planes'}", planes=planes)


@pytest.mark.parametrize("M", dx.F_M)
def test_bf16_gemm_streaming_every_token_tile_form_and_wave_split(M):
    """Section F, streaming (M < 256 with N < 1024): 32-row passes, bf16_gemm_wk = heuristic, 1, 2, 4, 8; N = 130 is even but no
    multiple of 4, 129 is odd."""
    for m, N, K, wk, dt in [c for c in dx.F_STREAM if c[0] == M]:
        assert wk < 0 or dx.bf16_wk(N, K, wk) == wk
        c = dx.bf16_case(M, N, K)
        for t in _types(dt):
            with _options(bf16_gemm_wk=wk):
                _bf16_gemm(c, M, N, K, t, f"M={M} N={N} K={K} bf16_gemm_wk={wk}")


@pytest.mark.parametrize("case", dx.F_DEEP, ids=_id)
def test_bf16_gemm_streaming_deep_ring_on_and_off(case):
    M, N, K, wk, deep, dt = case
    c = dx.bf16_case(M, N, K)
    for t in _types(dt):
        with _options(bf16_gemm_wk=wk, bf16_gemm_deep=deep):
            _bf16_gemm(c, M, N, K, t, f"M={M} N={N} K={K} bf16_gemm_wk={wk} bf16_gemm_deep={deep}")
    with _options(bf16_gemm_wk=wk):  # deep -1: the launcher's own rule
        _bf16_gemm(c, M, N, K, dt, f"M={M} N={N} K={K} bf16_gemm_wk={wk} bf16_gemm_deep=-1")


@pytest.mark.parametrize("case", dx.F_SPLIT, ids=_id)
def test_bf16_gemm_streaming_split_k_planes(case):
    """num_splits 3 and 8 at launched WK 2, 4 and 8 (K is long enough for S WK waves) and under the heuristic: the planes are
    the output, each the contraction over its own K range.  K = 7680, S = 3 at M <= 16 is 5 blocks per wave: the DEEP ring
    writing planes."""
    M, N, K, S, wk = case
    assert wk < 0 or dx.bf16_wk(N, K, wk, S) == wk
    c = dx.bf16_case(M, N, K)
    with _options(bf16_gemm_wk=wk):
        _bf16_gemm(c, M, N, K, "f32", f"M={M} N={N} K={K} S={S} bf16_gemm_wk={wk}", S=S, ranges=dx.bf16_stream_ranges(K, S))


@pytest.mark.parametrize("case", dx.F_TILED, ids=_id)
def test_bf16_gemm_tiled_at_both_heights_split_k_and_streamed(case):
    """Section F, tiled (M >= 256, or M >= 128 with N >= 1024) at tile heights 64 and 128, num_splits 1, 3, 4: at K = 320, S = 4
    the shares are 2, 2, 1, 0 blocks and the empty share writes zeros.  bf16_gemm_tiled = 0 streams the same inputs."""
    M, N, K, S, tm, dt = case
    c = dx.bf16_case(M, N, K)
    for t in _types(dt) if S == 1 else ["f32"]:
        with _options(fp8_tiled_tm=tm):
            _bf16_gemm(c, M, N, K, t, f"tiled M={M} N={N} K={K} S={S} fp8_tiled_tm={tm}", S=S, ranges=dx.bf16_tiled_ranges(K, S))
    if tm == 64:
        with _options(fp8_tiled_tm=-1):
            _bf16_gemm(c, M, N, K, dt, f"tiled M={M} N={N} K={K} S={S} heuristic height", S=S, ranges=dx.bf16_tiled_ranges(K, S))
        with _options(bf16_gemm_tiled=0):
            _bf16_gemm(c, M, N, K, dt, f"streamed (bf16_gemm_tiled=0) M={M} N={N} K={K} S={S}", S=S, ranges=dx.bf16_stream_ranges(K, S))


def test_bf16_gemm_refuses_more_splits_than_k_blocks():
    _bf16_gemm(dx.bf16_case(17, 136, 192), 17, 136, 192, "f32", "S=4 at K=192", S=4, expect_rc=ERR_BAD_ARG)
    _bf16_gemm(dx.bf16_case(256, 136, 64), 256, 136, 64, "f32", "S=2 at K=64", S=2, expect_rc=ERR_BAD_ARG)


@pytest.mark.parametrize("M", dx.G_M)
def test_bf16_gemm_silu_every_wave_split(M):
    """Section G: h = x w13^T is exact, so the entry's output must be ops.silu_and_mul of bf16(h) bit for bit (the same device
    SiLU on the same bf16 inputs: the "different summation order" of the randn test is gone), and within the bar of
    test_silu_and_mul_bit_exact against torch on the CPU: at most one bf16 ulp, under 1 % of the elements differing."""
    from chitu_amd import ops
    from chitu_amd._lib import i64, ptr, stream_ptr

    for m, inter, K, wk in [c for c in dx.G_CASES if c[0] == M]:
        assert wk < 0 or dx.bf16_wk(inter, K, wk) == wk
        c = dx.silu_case(M, inter, K)
        h = dx.expect(c["exact"], BF16)
        dev = [c["a_q"].cuda(), c["w_q"].cuda()]
        full, out = dx.guarded(M, inter, BF16)
        with _options(bf16_silu_wk=wk):
            rc = _abi().lib().chitu_hip_bf16_gemm_silu(ptr(dev[0]), ptr(dev[1]), ptr(out), i64(M), i64(inter), i64(K), stream_ptr())
        what = f"chitu_hip_bf16_gemm_silu M={M} inter={inter} K={K} bf16_silu_wk={wk}"
        got = _finish(rc, "chitu_hip_bf16_gemm_silu", full, BF16, ops.silu_and_mul(h.cuda()).cpu(), what)
        ref = torch.nn.functional.silu(h[:, :inter]) * h[:, inter:]
        d = (got.view(torch.int16).int() - ref.view(torch.int16).int()).abs()
        print(f"{what}: {int((d > 0).sum())} of {d.numel()} elements differ from torch on the CPU, max {int(d.max())} ulp")
        assert d.max() <= 1 and (d > 0).float().mean() < 0.01, what


# ---------------------------------------------------------------- H: soft fp8
@pytest.mark.parametrize("M", sorted({c[0] for c in dx.H_CASES}))
def test_soft_fp8_gemm_every_plan(M):
    """Section H: 32-row passes; K = 128, 384, 640, 1024 make the plan pick WK 1, 2, 4, 8."""
    for m, N, K, dt in [c for c in dx.H_CASES if c[0] == M]:
        c = dx.soft_case(M, N, K)
        for t in _types(dt):
            _soft_gemm(c, M, N, K, t, f"M={M} N={N} K={K} (WK {dx.plan_split(N, K)[0]})")


# ---------------------------------------------------------------- I: absorb
def _absorb_args(c, B, H, N, K):
    from chitu_amd._lib import i64, ptr

    wide = torch.zeros(B, H, K + 64, dtype=BF16)
    wide[..., :K] = c["x"]
    wide[..., K:] = float("nan")
    wide = wide.cuda()
    x = wide[..., :K]
    w, scale = c["w_store"].cuda(), c["scale"].cuda()
    sh, sn, sk = c["strides"]
    keep = (wide, w, scale)
    return keep, (ptr(x), i64(x.stride(0)), i64(x.stride(1)), ptr(w), i64(w.stride(0)), ptr(scale), i64(dx.ABSORB_OFFSET)), (sh, sn, sk)


@pytest.mark.parametrize("case", dx.I_BMM, ids=_id)
def test_absorb_bmm_with_and_without_rope(case):
    """Section I: x a strided view, w with a head stride above N K, the scales at a non-zero offset of a NaN-filled tensor under
    the two stride sets of the model and one with three distinct strides; then the same product with q_pe rotated in place
    by exact quarter turns -- a signed permutation, bit for bit, the rows of the tokens before and after the batch untouched."""
    from chitu_amd._lib import i32, i64, ptr, stream_ptr

    B, H, N, K, st = case
    c = dx.absorb_case(B, H, N, K, st)
    want = dx.expect(c["exact"], BF16).reshape(B * H, N)
    keep, head, (sh, sn, sk) = _absorb_args(c, B, H, N, K)
    tail = (i64(sh), i64(sn), i64(sk))
    full, out = dx.guarded(B * H, N, BF16)
    dims = (ptr(out), i64(H * N), i64(N), i32(B), i32(H), i32(N), i32(K))
    rc = _abi().lib().chitu_hip_absorb_bmm_fp8(*head, *tail, *dims, stream_ptr())
    _finish(rc, "chitu_hip_absorb_bmm_fp8", full, BF16, want, f"chitu_hip_absorb_bmm_fp8 {case}")
    q, cos, sin, q_want = dx.rope_case(B, H, seed=B + H + N + K)
    q_dev, cos_dev, sin_dev = q.cuda(), cos.cuda(), sin.cuda()
    full, out = dx.guarded(B * H, N, BF16)
    dims = (ptr(out), i64(H * N), i64(N), i32(B), i32(H), i32(N), i32(K))
    rc = _abi().lib().chitu_hip_absorb_bmm_rope_fp8(*head, *tail, *dims, ptr(q_dev[dx.G:]), i64(H * 64), i64(64), ptr(cos_dev), ptr(sin_dev),
                                                    i32(64), stream_ptr())
    _finish(rc, "chitu_hip_absorb_bmm_rope_fp8", full, BF16, want, f"chitu_hip_absorb_bmm_rope_fp8 {case}")
    dx.assert_equal(q_dev.cpu().float().view(-1, 64), q_want.float().view(-1, 64), f"q_pe after chitu_hip_absorb_bmm_rope_fp8 {case}")
    del keep


@pytest.mark.parametrize("case", dx.I_UV, ids=_id)
def test_absorb_uv_quant_codes_and_scales(case):
    """K = 512 is the compile-time form, 256 the runtime loop: codes and scales equal act_quant_deepseek_v3 (the CPU oracle) of
    the exact product rounded to bf16, bit for bit; both outputs between guards."""
    from chitu_amd._lib import i32, i64, ptr, stream_ptr

    B, H, K, st = case
    c = dx.absorb_case(B, H, 128, K, st)
    sh, sn, sk = c["strides"]
    q_want, s_want = ofp8.act_quant_deepseek_v3(dx.expect(c["exact"], BF16).reshape(B, H * 128).contiguous())
    keep, head, _ = _absorb_args(c, B, H, 128, K)
    codes = torch.full((B + 2 * dx.G, H * 128), 0x7F, dtype=torch.uint8, device="cuda")  # (0x7F: the e4m3fn NaN, no code of finite data)
    full_s, s_out = dx.guarded(B, H, F32)
    rc = _abi().lib().chitu_hip_absorb_uv_quant_fp8(*head, i64(sh), i64(sk), ptr(codes[dx.G:]), ptr(s_out), i32(B), i32(H), i32(K), stream_ptr())
    _finish(rc, "chitu_hip_absorb_uv_quant_fp8", full_s, F32, s_want, f"scales of chitu_hip_absorb_uv_quant_fp8 {case}")
    got = codes.cpu()
    assert bool((got[: dx.G] == 0x7F).all()) and bool((got[dx.G + B:] == 0x7F).all()), f"{case}: codes stored into the guard rows"
    assert not bool((got[dx.G:dx.G + B] == 0x7F).any()), f"{case}: codes never written"
    dx.assert_equal(got[dx.G:dx.G + B].int(), q_want.view(torch.uint8).int(), f"codes of chitu_hip_absorb_uv_quant_fp8 {case}")
    del keep


# ---------------------------------------------------------------- J: int8
@pytest.mark.parametrize("M", sorted({c[0] for c in dx.J_CASES}))
def test_w8a8_int8_gemm_every_plan_bias_and_output_type(M):
    """Section J: WK 1, 4, 2, 1, 2 over the (N, K) list, a ragged last tile, the bias absent or present in each of its types with
    integer values; fp32 (the exact value) and the case's own output type."""
    from chitu_amd._lib import i64, ptr, stream_ptr

    for m, N, K, bias, dt in [c for c in dx.J_CASES if c[0] == M]:
        c = dx.int8_case(M, N, K)
        exact = c["exact"] + (0 if bias is None else c["bias"][None, :])
        dev = [c["a_q"].cuda(), c["a_s"].float().cuda(), c["w_q"].cuda(), c["w_s"].float().cuda(),
               None if bias is None else c["bias"].to(dx.DTYPES[bias]).cuda()]
        for t in _types(dt):
            dtype = dx.DTYPES[t]
            full, out = dx.guarded(M, N, dtype)
            rc = _abi().lib().chitu_hip_w8a8_int8_gemm(*(ptr(x) for x in dev), ctypes.c_int(dx.DT_CODE[bias or "bf16"]), ptr(out),
                                                       ctypes.c_int(dx.DT_CODE[t]), i64(M), i64(N), i64(K), stream_ptr())
            _finish(rc, "chitu_hip_w8a8_int8_gemm", full, dtype, dx.expect(exact, dtype),
                    f"chitu_hip_w8a8_int8_gemm M={M} N={N} K={K} bias {bias} out {t}")


# ---------------------------------------------------------------- K: warm-state independence of the wrappers
def test_ops_wrappers_do_not_depend_on_what_their_buffers_held():
    """One ragged shape per wrapper: the result inside poisoned_allocations() (torch.empty and the workspace filled with 0xFF
    bytes) equals the result outside it, and both equal the expectation."""
    from chitu_amd import ops

    M, N, K = 33, 129, 384
    c = dx.fp8_case(M, N, K)
    dev = [c["a_q"].cuda(), c["a_s"].float().cuda(), c["w_q"].cuda(), c["w_s"].float().cuda()]
    qt, st = dx.to_tile_major(c["a_q"], c["a_s"])
    tq = ops.TiledQuant(qt.cuda(), st.cuda(), M, K)
    s = dx.soft_case(M, N, K)
    b = dx.bf16_case(33, 130, 192)
    g = dx.silu_case(33, 136, 512)
    a = dx.absorb_case(17, 3, 136, 192, "distinct")
    keep, _, (sh, sn, sk) = _absorb_args(a, 17, 3, 136, 192)
    x_view = keep[0][..., :192]
    w_view = keep[1][:, : 136 * 192].view(3, 136, 192).view(torch.float8_e4m3fn)
    calls = {
        "fp8_gemm_deepseek_v3": (lambda: ops.fp8_gemm_deepseek_v3(*dev, out_dtype=F32), dx.expect(c["exact"], F32)),
        "fp8_gemm_deepseek_v3 (tile-major)": (lambda: ops.fp8_gemm_deepseek_v3(tq, None, dev[2], dev[3], out_dtype=BF16), dx.expect(c["exact"], BF16)),
        "soft_fp8_gemm_deepseek_v3": (lambda: ops.soft_fp8_gemm_deepseek_v3(s["a_q"].cuda(), s["w_q"].cuda(), s["w_s"].float().cuda()),
                                      dx.expect(s["exact"], torch.get_default_dtype())),
        "bf16_linear": (lambda: ops.bf16_linear(b["a_q"].cuda(), b["w_q"].cuda(), out_dtype=F32), dx.expect(b["exact"], F32)),
        "bf16_linear_silu": (lambda: ops.bf16_linear_silu(g["a_q"].cuda(), g["w_q"].cuda()), None),
        "absorb_bmm_fp8": (lambda: ops.absorb_bmm_fp8(x_view, w_view, keep[2], dx.ABSORB_OFFSET, sh, sn, sk), dx.expect(a["exact"], BF16)),
    }
    for name, (call, want) in calls.items():
        plain = call().cpu()
        with poisoned_allocations():
            foul = call().cpu()
        if want is None:
            want = ops.silu_and_mul(dx.expect(g["exact"], BF16).cuda()).cpu()
        dx.assert_equal(plain, want, f"ops.{name}")
        dx.assert_equal(foul, plain, f"ops.{name} inside poisoned_allocations()")
