"""W4A16 g128 kernels (include/chitu_hip_ext9.h) against the CPU references of tests/w4a16_ref.py over GRID + RING: every
(MT, WK) instantiation of both streaming kernels (asserted through ops.w4a16_plan), odd N and odd inter (the phantom row of
a scale pair, single bf16 stores), the half-line K tail on every position of a wave's share, the ring wrap, the second 32-row
launch -- plus widen, one prefill-sized case through the tiled form and the Python entries.

pow2 scales: bit for bit.  quantiser scales: between the roundings of the accumulator interval's ends (w4a16_ref's rho).
SiLU: tests/silu_ref.py's candidate rule.  The count of elements with two admissible values is printed per (entry, kind).

Every streaming launch goes through the C entry on over-allocated, poisoned buffers: NaN in the output rows beyond M, in the
activation rows beyond M and in the scale pairs beyond the last one (for w13: behind the pairs of w3), POISON in the packed
rows beyond N (2 inter).  Afterwards all poison is intact and no NaN is inside [M, N]."""
import pytest
import torch

from tests import w4a16_ref as w4
from tests.silu_ref import check_silu

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
POISON = 0x5A  # codes 2 and 13 as stored: nothing the kernels could mistake for zero
PAD_W, PAD_S, PAD_X, PAD_OUT = 16, 16, 3, 2  # weight rows, scale pairs, activation rows, output rows


def _guarded(t, pad, poison=None):
    """t [rows, ...] on the CPU -> device buffer with `pad` more rows of NaN (or `poison`) behind it"""
    whole = torch.empty(t.shape[0] + pad, *t.shape[1:], dtype=t.dtype, device="cuda")
    whole[: t.shape[0]] = t.cuda()
    whole[t.shape[0]:] = float("nan") if poison is None else poison
    return whole


def _intact(whole, rows, poison=None):
    tail = whole[rows:]
    return bool(torch.isnan(tail.float()).all()) if poison is None else bool((tail == poison).all())


def _run_stream(entry, x, packed, scales, M, N, K, out_dtype=BF16):
    """the C entry on poisoned, over-allocated buffers; returns the [M, N] result (CPU) after checking the poison"""
    from chitu_amd import _lib
    from chitu_amd._lib import check, float_dtype_code, i32, i64, ptr, stream_ptr

    rows = 2 * N if entry == "silu" else N
    assert tuple(x.shape) == (M, K) and tuple(packed.shape) == (rows, K // 2)
    assert tuple(scales.shape) == ((2 if entry == "silu" else 1) * ((N + 1) // 2), (K + 255) // 256, 4)
    xw, pw, sw = _guarded(x, PAD_X), _guarded(packed, PAD_W, POISON), _guarded(scales, PAD_S)
    out = torch.full((M + PAD_OUT, N), float("nan"), dtype=out_dtype, device="cuda")
    lib = _lib.lib()
    if entry == "silu":
        assert out_dtype == BF16
        rc = lib.chitu_ext9_w4a16_gemm_silu(ptr(xw), ptr(pw), ptr(sw), ptr(out), i64(M), i64(N), i64(K), stream_ptr())
    else:
        rc = lib.chitu_ext9_w4a16_gemm(ptr(xw), ptr(pw), ptr(sw), ptr(out), i32(float_dtype_code(out_dtype)), i64(M), i64(N), i64(K),
                                       stream_ptr())
    check(rc, entry)
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool(torch.isnan(host[M:].float()).all()), "the output rows beyond M were written"
    assert _intact(xw, M) and _intact(pw, rows, POISON) and _intact(sw, scales.shape[0]), "an input guard changed"
    assert torch.equal(xw[:M].cpu(), x) and torch.equal(pw[:rows].cpu(), packed), "an input changed"
    return host[:M]


def _assert_bits(got, want, what):
    it = torch.int16 if got.element_size() == 2 else torch.int32
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = (got.contiguous().view(it) != want.contiguous().view(it)).nonzero()
    assert bad.numel() == 0, (what, bad.shape[0], bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _assert_between(got, lo, hi, what):
    """lo <= got <= hi, and bit for bit where the ends agree; returns the count of elements where they do not"""
    assert not bool(torch.isnan(got.float()).any()), (what, "NaN inside [M, N]")
    free = lo != hi
    ok = (got.float() >= lo.float()) & (got.float() <= hi.float())
    assert bool(ok.all()), (what, (~ok).nonzero()[:4].tolist(), got[~ok][:4], lo[~ok][:4], hi[~ok][:4])
    it = torch.int16 if got.element_size() == 2 else torch.int32
    same = got.contiguous().view(it) == lo.contiguous().view(it)
    assert bool((same | free | ((got == 0) & (lo == 0))).all()), what
    return int(free.sum())


def _check_case(c, got, dt, what):
    if c.entry == "silu":
        want, g, u, gh, uh = c.silu_args()
        assert not bool(torch.isnan(got.float()).any()), (what, "NaN inside [M, inter]")
        return check_silu(got, want, g, u, what, gh, uh)
    lo, hi = c.linear_ends(dt)
    if c.kind == "pow2":
        _assert_bits(got, lo, what)
        return 0
    return _assert_between(got, lo, hi, what)


@pytest.mark.parametrize("kind", ["pow2", "quantiser"])
@pytest.mark.parametrize("entry", ["linear", "silu"])
def test_streaming_entries_over_the_grid(entry, kind):
    from chitu_amd import ops

    silu = entry == "silu"
    seen, free = set(), {BF16: [0, 0], F16: [0, 0]}
    for (M, N, K) in w4.GRID + w4.RING:
        plan = ops.w4a16_plan(M, N, K, silu=silu)
        assert plan["form"] == "stream" and len(plan["launches"]) == -(-M // 32)
        seen.update(plan["launches"])
        c = w4.case(entry, kind, M, N, K)
        packed, scales = c.packed()
        types = (BF16,) if silu else (BF16, F32) + ((F16,) if (M, N, K) in w4.F16_SHAPES else ())
        for dt in types:
            got = _run_stream(entry, c.x, packed, scales, M, N, K, dt)
            n = _check_case(c, got, dt, f"{entry} {kind} {dt} M={M} N={N} K={K}")
            if dt != F32:
                free[dt][0] += n
                free[dt][1] += got.numel()
        print(f"W4A16EXACT {entry} {kind} M={M} N={N} K={K} plan={sorted(set(plan['launches']))}: ok, {M * N} elements x {len(types)} types")
    assert seen == (w4.ALL_SILU if silu else w4.ALL_LINEAR), seen  # every kernel instantiation was launched
    for dt, (n, total) in free.items():
        if total:
            print(f"W4A16EXACT {entry} {kind} {dt}: {n} of {total} elements with two admissible values")
            assert n <= w4.CAP * total


@pytest.mark.parametrize("M,N,K", [(17, 23, 384), (33, 1, 1152), (1, 23, 1152)])
def test_phantom_scale_slots_never_reach_a_result(M, N, K):
    """Odd N / odd inter and K % 256 == 128: the scale slots of the row and of the group that do not exist hold NaN in the
    device copy (pack_w4a16 writes zero there); the results must be those of the zero-filled copy, bit for bit."""
    for entry in ("linear", "silu"):
        c = w4.case(entry, "quantiser", M, N, K)
        packed, scales = c.packed()
        P, T = (N + 1) // 2, (K + 255) // 256
        poisoned = scales.clone().view(c.halves, P, T, 2, 2)
        assert N % 2 == 1 and K % 256 == 128
        assert bool((poisoned[:, P - 1, :, 1, :] == 0).all()) and bool((poisoned[:, :, T - 1, :, 1] == 0).all())
        poisoned[:, P - 1, :, 1, :] = float("nan")  # row N of the last pair
        poisoned[:, :, T - 1, :, 1] = float("nan")  # group K / 128 of the last step
        poisoned = poisoned.view_as(scales)
        for dt in (BF16,) if entry == "silu" else (BF16, F32):
            clean = _run_stream(entry, c.x, packed, scales, M, N, K, dt)
            got = _run_stream(entry, c.x, packed, poisoned, M, N, K, dt)
            _assert_bits(got, clean, f"phantom {entry} {dt} M={M} N={N} K={K}")
        print(f"W4A16EXACT phantom {entry} M={M} N={N} K={K}: ok, {int(torch.isnan(poisoned).sum())} NaN slots")


@pytest.mark.parametrize("M,N,K", [(17, 24, 384), (33, 40, 1152)])
def test_int4_stream_equals_bf16_stream_over_the_widened_weights(M, N, K):
    """The two line policies of stream_gemm.h against each other.  pow2 scales: W' = bf16((u - 8) s) is exact and both
    accumulators are the real product, so the plain pair into fp32 and the SiLU pair into bf16 must be torch.equal."""
    from chitu_amd import _lib, ops
    from chitu_amd._lib import check, i32, i64, ptr, stream_ptr

    lib = _lib.lib()
    for silu in (False, True):
        c = w4.case("silu" if silu else "linear", "pow2", M, N, K)
        packed, scales = c.packed()
        assert torch.equal(w4.widened(c.u, c.s).to(torch.float64), w4.dequantised(c.u, c.s))
        P = scales.shape[0] // c.halves
        wide = torch.cat([ops.w4a16_widen(packed[h * N:(h + 1) * N].cuda(), scales[h * P:(h + 1) * P].cuda()) for h in range(c.halves)])
        assert torch.equal(wide.cpu(), w4.widened(c.u, c.s))
        got = _run_stream(c.entry, c.x, packed, scales, M, N, K, BF16 if silu else F32)
        xd = c.x.cuda()
        ref = torch.full((M, N), float("nan"), dtype=got.dtype, device="cuda")
        if silu:
            rc = lib.chitu_hip_bf16_gemm_silu(ptr(xd), ptr(wide), ptr(ref), i64(M), i64(N), i64(K), stream_ptr())
        else:
            rc = lib.chitu_hip_bf16_gemm(ptr(xd), ptr(wide), ptr(ref), i32(2), i64(M), i64(N), i64(K), i32(1), ptr(None), stream_ptr())
        check(rc, "chitu_hip_bf16_gemm" + ("_silu" if silu else ""))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(got.float()).any()) and torch.equal(got, ref.cpu()), (silu, M, N, K)
        print(f"W4A16EXACT int4 == bf16 {'silu' if silu else 'linear'} M={M} N={N} K={K}: ok, {got.numel()} elements")


@pytest.mark.parametrize("K", [128, 384, 1152])
@pytest.mark.parametrize("N", [1, 5, 16])
def test_widen_over_odd_rows_and_every_group_parity(N, K):
    from chitu_amd import _lib
    from chitu_amd._lib import check, i64, ptr, stream_ptr
    from chitu_amd.quantize.w4a16 import pack_w4a16

    u, s = w4.make_u(N, K, 100 * N + K), w4.quantiser_scales(N, K, 200 * N + K)
    packed, scales = pack_w4a16(u, s)
    pw, sw = _guarded(packed, PAD_W, POISON), _guarded(scales, PAD_S)
    out = torch.full((N + PAD_OUT, K), float("nan"), dtype=BF16, device="cuda")
    check(_lib.lib().chitu_ext9_w4a16_widen(ptr(pw), ptr(sw), ptr(out), i64(N), i64(K), stream_ptr()), "widen")
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool(torch.isnan(host[N:].float()).all()) and _intact(pw, N, POISON) and _intact(sw, scales.shape[0])
    _assert_bits(host[:N], w4.widened(u, s), f"widen N={N} K={K}")
    print(f"W4A16EXACT widen N={N} K={K}: ok, {N * K} elements")


@pytest.mark.parametrize("kind", ["pow2", "quantiser"])
def test_prefill_sized_case_through_the_tiled_form(kind):
    """M = 256: widen + the tiled bf16 GEMM.  pow2: W' is exact and the accumulator the real product, so the streaming
    expectation holds bit for bit.  quantiser: the fp64 product over W' as rounded on the CPU, within
    tests/test_gpu_w4a16.py::test_random_inputs_within_the_derived_bound's bound."""
    from chitu_amd import ops

    M, N, K = w4.TILED
    inter = N // 2
    assert ops.w4a16_plan(M, N, K)["form"] == "tiled" and ops.w4a16_plan(M, inter, K, silu=True)["form"] == "tiled"
    lin, sil = w4.case("linear", kind, M, N, K), w4.case("silu", kind, M, inter, K)
    for c in (lin, sil):
        packed, scales = c.packed()
        xd, pd, sd = c.x.cuda(), packed.cuda(), scales.cuda()
        if c.entry == "silu":
            got = ops.w4a16_linear_silu(xd, pd, sd).cpu()
            assert got.dtype == BF16 and tuple(got.shape) == (M, inter)
            if kind == "pow2":
                n = _check_case(c, got, BF16, f"tiled silu {kind}")
                print(f"W4A16EXACT silu-tiled {kind} M={M} inter={inter} K={K}: ok, {got.numel()} elements, {n} on a rounding boundary")
            else:  # the chain over the GEMM's own accumulators: the bf16 launch over W', bit for bit
                wide = torch.cat([ops.w4a16_widen(pd[:inter], sd[: inter // 2]), ops.w4a16_widen(pd[inter:], sd[inter // 2:])])
                assert torch.equal(wide.cpu(), w4.widened(c.u, c.s))
                _assert_bits(got, ops.bf16_linear_silu(xd, wide).cpu(), f"tiled silu {kind}")
                print(f"W4A16EXACT silu-tiled {kind} M={M} inter={inter} K={K}: ok, {got.numel()} elements")
            continue
        for dt in (BF16, F32):
            got = ops.w4a16_linear(xd, pd, sd, out_dtype=dt).cpu()
            assert got.dtype == dt and tuple(got.shape) == (M, N)
            if kind == "pow2":
                _check_case(c, got, dt, f"tiled linear {kind} {dt}")
            else:
                W = w4.widened(c.u, c.s).to(torch.float64)
                xf = c.x.to(torch.float64)
                ref, mag = xf @ W.t(), xf.abs() @ W.abs().t()
                bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
                err = (got.to(torch.float64) - ref).abs()
                print(f"W4A16EXACT linear-tiled {kind} {dt}: max err / bound {float((err / bound).max()):.3e}")
                assert bool((err <= bound).all())
            print(f"W4A16EXACT linear-tiled {kind} {dt} M={M} N={N} K={K}: ok, {got.numel()} elements")


def test_python_entries_match_the_c_entries_and_take_leading_dims():
    from chitu_amd import ops

    M, N, K = 6, 23, 384
    lin, sil = w4.case("linear", "quantiser", M, N, K), w4.case("silu", "quantiser", M, N, K)
    packed, scales = lin.packed()
    xd = lin.x.view(2, 3, K).cuda()
    for dt in (None, F16, F32):
        got = ops.w4a16_linear(xd, packed.cuda(), scales.cuda(), out_dtype=dt)
        assert tuple(got.shape) == (2, 3, N) and got.dtype == (dt or BF16)
        _assert_bits(got.cpu().view(M, N), _run_stream("linear", lin.x, packed, scales, M, N, K, dt or BF16), f"ops.w4a16_linear {dt}")
        _assert_between(got.cpu().view(M, N), *lin.linear_ends(dt or BF16), f"ops.w4a16_linear {dt}")
    packed, scales = sil.packed()
    gs = ops.w4a16_linear_silu(sil.x.view(2, 3, K).cuda(), packed.cuda(), scales.cuda())
    assert tuple(gs.shape) == (2, 3, N) and gs.dtype == BF16
    _assert_bits(gs.cpu().view(M, N), _run_stream("silu", sil.x, packed, scales, M, N, K), "ops.w4a16_linear_silu")
    _check_case(sil, gs.cpu().view(M, N), BF16, "ops.w4a16_linear_silu")
    print(f"W4A16EXACT ops M={M} N={N} K={K}: ok, {4 * M * N} elements")
