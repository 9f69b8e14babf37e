"""W8A16 kernels (include/chitu_hip_ext6.h) against the integer specification of tests/w8a16_ref.py, bit for bit, over
M x N x K = tests.w8a16_ref.GRID -- every (MT, WK) instantiation of both streaming kernels (asserted through
ops.w8a16_plan), the ring tail, the half-line K tail, partial row tiles and the second 32-row launch -- plus one
prefill-sized case through the widen + tiled GEMM + scale_round form.  Every buffer is over-allocated and poisoned: NaN in
the output beyond [M, N], in the activations beyond M rows and in the scales beyond N, -128 in the weight rows beyond N.
Nothing outside the extents may reach a result or be written.

The SiLU entry's expectation restates the rounding chain on the CPU in fp32.  One step of it is not exactly specified on
either side: exp(-g) goes through the device's expf and through the CPU's, each at most 1 ulp off (HIP's and glibc's
documented bounds), so the two differ by at most 2 fp32 ulps = a factor within 1 -+ 2^-22.  The add and the divide behind it
are correctly rounded and monotone on both sides, so the device's silu lies between the CPU chain evaluated at
exp * (1 - 2^-22) and at exp * (1 + 2^-22).  Where those two round to one bf16 number the output is checked bit for bit
against it; where they differ (silu sits on a bf16 rounding boundary: a few elements in ten thousand) either end is
accepted.  The count of such elements is printed.
"""
import pytest
import torch

from tests import w8a16_ref as wr

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC0


def _abi():
    from chitu_amd import _lib

    return _lib


def _poisoned(t, pad_rows, poison):
    """t [rows, cols] -> device buffer [rows + pad_rows, cols] whose tail holds `poison`; returns (whole, view of the head)"""
    whole = torch.empty(t.shape[0] + pad_rows, t.shape[1], dtype=t.dtype, device="cuda")
    whole[: t.shape[0]] = t.cuda()
    if t.dtype == torch.int8:
        whole[t.shape[0]:] = poison
    else:
        whole[t.shape[0]:] = float("nan")
    return whole, whole[: t.shape[0]]


def _scales(kind, rows, seed):
    return wr.pow2_scales(rows) if kind == "pow2" else wr.quantiser_scales(rows, seed)


def _run_stream(entry, x, q, s, M, N, K, out_dtype=torch.bfloat16):
    """the C entry on poisoned, over-allocated buffers; returns the [M, N] result after checking that the poison is intact"""
    from chitu_amd._lib import check, float_dtype_code, i32, i64, ptr, stream_ptr

    xw, _ = _poisoned(x, 3, None)
    qw, _ = _poisoned(q, 16, -128)
    sw = torch.full((q.shape[0] + 16,), float("nan"), dtype=torch.float32, device="cuda")
    sw[: q.shape[0]] = s.cuda()
    out = torch.full((M + 2, N), float("nan"), dtype=out_dtype, device="cuda")
    lib = _abi().lib()
    if entry == "silu":
        # w13 = [w1; w3]: the up rows follow the gate rows directly, so the padding sits behind row 2 * inter
        rc = lib.chitu_ext6_w8a16_gemm_silu(ptr(xw), ptr(qw), ptr(sw), ptr(out), i64(M), i64(N), i64(K), stream_ptr())
    else:
        rc = lib.chitu_ext6_w8a16_gemm(ptr(xw), ptr(qw), ptr(sw), ptr(out), i32(float_dtype_code(out_dtype)), i64(M), i64(N), i64(K),
                                       stream_ptr())
    check(rc, entry)
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool(torch.isnan(host[M:]).all()), "the output rows beyond M were written"
    assert bool(torch.isnan(xw[M:].float()).all()) and bool(torch.isnan(sw[q.shape[0]:]).all()) and bool((qw[q.shape[0]:] == -128).all())
    return host[:M]


def _assert_bits(got, want, what):
    a, b = got.contiguous().view(torch.int16 if got.element_size() == 2 else torch.int32), want.contiguous().view(
        torch.int16 if want.element_size() == 2 else torch.int32)
    bad = (a != b).nonzero()
    assert bad.numel() == 0, (what, bad[:4].tolist(), got.flatten()[:4], want.flatten()[:4])


def _silu_candidates(x, q13, s):
    """(lo, hi): the two ends of the admissible bf16 outputs per element (equal except on a rounding boundary of silu's bf16
    rounding): the fp32 chain of wr.expected_silu with exp(-g) moved by 2 fp32 ulps either way"""
    inter = q13.shape[0] // 2
    a = wr.acc_int(x, q13).to(torch.float32) * s.view(1, -1)
    g, u = a[:, :inter].to(torch.bfloat16).float(), a[:, inter:].to(torch.bfloat16).float()
    e = torch.exp(-g)
    outs = []
    for f in (1.0 - 2.0 ** -22, 1.0 + 2.0 ** -22):
        sg = (g / (1.0 + e * torch.tensor(f, dtype=torch.float32))).to(torch.bfloat16).float()
        outs.append((sg * u).to(torch.bfloat16))
    return outs[0], outs[1]


def _check_silu(got, x, q13, s, what):
    lo, hi = _silu_candidates(x, q13, s)
    want = wr.expected_silu(x, q13, s)
    gb, lb, hb, wb = (t.contiguous().view(torch.int16) for t in (got, lo, hi, want))
    free = lb != hb
    assert bool(((gb == lb) | (gb == hb)).all()), (what, ((gb != lb) & (gb != hb)).nonzero()[:4].tolist())
    assert bool((gb == wb)[~free].all()), what  # off a boundary the CPU's fp32 chain is the answer, bit for bit
    return int(free.sum())


@pytest.mark.parametrize("kind", ["pow2", "quantiser"])
@pytest.mark.parametrize("entry", ["linear", "silu"])
def test_streaming_entries_are_bit_exact_over_the_grid(entry, kind):
    from chitu_amd import ops

    silu = entry == "silu"
    seen, boundary = set(), 0
    for idx, (M, N, K) in enumerate(wr.GRID):
        plan = ops.w8a16_plan(M, N, K, silu=silu)
        assert plan["form"] == "stream" and len(plan["launches"]) == -(-M // 32)
        seen.update(plan["launches"])
        rows = 2 * N if silu else N
        x, q, s = wr.make_x(M, K, 1000 + idx), wr.make_q(rows, K, 2000 + idx), _scales(kind, rows, 3000 + idx)
        got = _run_stream(entry, x, q, s, M, N, K)
        what = f"{entry} {kind} M={M} N={N} K={K}"
        if silu:
            boundary += _check_silu(got, x, q, s, what)
        else:
            _assert_bits(got, wr.expected_linear(x, q, s), what)
        print(f"W8A16EXACT {entry} {kind} M={M} N={N} K={K} plan={sorted(set(plan['launches']))}: ok, {got.numel()} elements")
    assert seen == (wr.ALL_SILU if silu else wr.ALL_LINEAR), seen  # every kernel instantiation was launched
    if silu:
        print(f"W8A16EXACT {entry} {kind}: {boundary} elements on a bf16 rounding boundary of silu (either neighbour accepted)")


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16])
def test_linear_entry_other_output_types(out_dtype):
    for idx, (M, N, K) in enumerate([(1, 24, 192), (17, 40, 512), (33, 16, 1088)]):
        x, q, s = wr.make_x(M, K, 40 + idx), wr.make_q(N, K, 50 + idx), wr.quantiser_scales(N, 60 + idx)
        got = _run_stream("linear", x, q, s, M, N, K, out_dtype)
        _assert_bits(got, wr.expected_linear(x, q, s, out_dtype), f"{out_dtype} M={M} N={N} K={K}")
        print(f"W8A16EXACT linear {out_dtype} M={M} N={N} K={K}: ok, {got.numel()} elements")


@pytest.mark.parametrize("M,N,K", [(17, 24, 192), (33, 40, 512)])
def test_int8_stream_equals_bf16_stream_over_the_widened_weights(M, N, K):
    """The two line policies of stream_gemm.h against each other: with every scale 1.0 the int8 launch must equal the bf16
    launch over ops.w8a16_widen(q), torch.equal -- the plain pair into fp32 (both accumulators are exact integers below 2^24,
    wr.acc_int's own assertion), the SiLU pair into bf16 (the same device chain on the same exact accumulators)."""
    from chitu_amd import ops
    from chitu_amd._lib import check, i32, i64, ptr, stream_ptr

    lib = _abi().lib()
    for silu in (False, True):
        rows = 2 * N if silu else N
        x, q = wr.make_x(M, K, 70 + M), wr.make_q(rows, K, 80 + M)
        wr.acc_int(x, q)
        ones = torch.ones(rows, dtype=torch.float32)
        xd, wide = x.cuda(), ops.w8a16_widen(q.cuda())
        got = _run_stream("silu" if silu else "linear", x, q, ones, M, N, K, torch.bfloat16 if silu else torch.float32)
        ref = torch.full((M, N), float("nan"), dtype=got.dtype, device="cuda")
        if silu:
            rc = lib.chitu_hip_bf16_gemm_silu(ptr(xd), ptr(wide), ptr(ref), i64(M), i64(N), i64(K), stream_ptr())
        else:
            rc = lib.chitu_hip_bf16_gemm(ptr(xd), ptr(wide), ptr(ref), i32(2), i64(M), i64(N), i64(K), i32(1), ptr(None), stream_ptr())
        check(rc, "chitu_hip_bf16_gemm" + ("_silu" if silu else ""))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(got.float()).any()) and torch.equal(got, ref.cpu()), (silu, M, N, K)
        print(f"W8A16EXACT int8 == bf16 {'silu' if silu else 'linear'} M={M} N={N} K={K}: ok, {got.numel()} elements")


@pytest.mark.parametrize("kind", ["pow2", "quantiser"])
def test_prefill_sized_case_through_the_tiled_form(kind):
    """M = 256: widen (exact) + the tiled bf16 GEMM into fp32 + scale_round obey the same contract, so: bit-exact."""
    from chitu_amd import ops

    M, N, K = wr.TILED_CASE
    assert ops.w8a16_plan(M, N, K)["form"] == "tiled" and ops.w8a16_plan(M, N // 2, K, silu=True)["form"] == "tiled"
    x, q, s = wr.make_x(M, K, 7), wr.make_q(N, K, 8), _scales(kind, N, 9)
    wide = ops.w8a16_widen(q.cuda()).cpu()
    assert wide.dtype == torch.bfloat16 and torch.equal(wide.float(), q.float())
    print(f"W8A16EXACT widen N={N} K={K}: ok, {wide.numel()} elements")
    got = ops.w8a16_linear(x.cuda(), q.cuda(), s.cuda()).cpu()
    _assert_bits(got, wr.expected_linear(x, q, s), f"tiled linear {kind}")
    print(f"W8A16EXACT linear-tiled {kind} M={M} N={N} K={K}: ok, {got.numel()} elements")
    got32 = ops.w8a16_linear(x.cuda(), q.cuda(), s.cuda(), out_dtype=torch.float32).cpu()
    _assert_bits(got32, wr.expected_linear(x, q, s, torch.float32), f"tiled linear fp32 {kind}")
    gs = ops.w8a16_linear_silu(x.cuda(), q.cuda(), s.cuda()).cpu()  # the same rows read as [w1; w3], inter = N / 2
    n_free = _check_silu(gs, x, q, s, f"tiled silu {kind}")
    print(f"W8A16EXACT silu-tiled {kind} M={M} inter={N // 2} K={K}: ok, {gs.numel()} elements, {n_free} on a rounding boundary")


def test_python_entries_match_the_c_entries_and_take_leading_dims():
    from chitu_amd import ops

    M, N, K = 6, 40, 192
    x, q, s = wr.make_x(M, K, 1), wr.make_q(2 * N, K, 2), wr.quantiser_scales(2 * N, 3)
    got = ops.w8a16_linear(x.view(2, 3, K).cuda(), q.cuda(), s.cuda())
    assert tuple(got.shape) == (2, 3, 2 * N) and got.dtype == torch.bfloat16
    _assert_bits(got.cpu().view(M, 2 * N), wr.expected_linear(x, q, s), "ops.w8a16_linear")
    gs = ops.w8a16_linear_silu(x.view(2, 3, K).cuda(), q.cuda(), s.cuda())
    assert tuple(gs.shape) == (2, 3, N)
    _check_silu(gs.cpu().view(M, N), x, q, s, "ops.w8a16_linear_silu")
    print(f"W8A16EXACT ops M={M} N={2 * N} K={K}: ok, {got.numel() + gs.numel()} elements")
