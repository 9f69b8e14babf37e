"""The row kernels between the GEMMs on exact data: norms, quantisers, RoPE, paged appends, gather, moe_sum, SiLU.

Builders and CPU oracles: tests/row_exact.py; their CPU checks: tests/test_row_exact_host.py.  Every entry is called through the
C ABI with each output between G guard rows (and guard columns where a row stride allows them) of the NaN sentinels of
tests/dense_exact.py, the output itself pre-filled with the sentinel; after each launch the guards are untouched, no element
that should have been written still holds the sentinel, and the result equals the oracle bit for bit (every difference is
reported with its row and column).

  A  chitu_hip_rmsnorm without add (256-thread form): 16 dims around every per-pass boundary, strided x and y, fused fp8 modes, y = NULL
  B  chitu_hip_rmsnorm with add (wide form): residual, 1..16 terms, aliased sum_out, tile-major output and its padding, int8 mode
  C  return codes of chitu_hip_rmsnorm, outputs untouched
  D  chitu_hip_act_quant_fp8: three input types x two modes on the adversarial table, and a second stride iteration
  E  chitu_hip_quant_act_int8: vector and scalar kernel, exact ties, the zero row, NaN
  F  chitu_hip_weight_dequant_fp8: all 256 codes to f16 / fp32, an f16 overflow, a second stride iteration
  G  chitu_hip_rope: three types x both layouts, head_dim 2, no q heads / no k heads, strided views, a second stride iteration
  H  the bf16 append entries against the oracle, valid batches and out-of-table batches between guard pages
  I  chitu_hip_embed_rope_gather: clamped positions, half > 256, foreign tokens
  J  chitu_hip_moe_sum: top-k 1, 2, 9, 16 and a second stride iteration
  K  chitu_hip_silu_and_mul: all 65 536 gates
  L  the ops wrappers inside tests.util.poisoned_allocations() == outside it

Candidate sets (tests/row_exact.py): rsqrtf and expf are not correctly rounded on the device, so the oracle gives one expected
row per candidate value: the correctly rounded one and its neighbours within RSQRT_RADIUS = 1 and EXPF_RADIUS = 1 fp32 ulp.
Source of both radii: no accuracy table of the device library comes with the toolchain (neither the ISA text nor the
device-library documentation is installed beside the compiler), so both are the +-1 ulp starting value, which is also the
figure the HIP programming guide's table of device math functions gives for rsqrtf and expf.  Measured on the MI355X (every
test prints its count, `ROWEXACT ... non-central`):
  - rsqrtf: 0 of the 1175 rows checked by this module took a non-central candidate (sections A, B, H);
  - expf:   0 of the 65 536 gates of section K took a non-central candidate.
No row and no gate needed more than the radius.

Bugs these tests exposed, fixed with them:
  - common.h, group_div (the reciprocal-and-correction division of every fp8 quantiser): x = -0 gave +0 (the residual of -0
    is +0), so a -0 input had code 0x00 where IEEE division and the reference give 0x80.  Shown by every fused-quant case of
    sections A and B and by mla_qkv_post ("(0, 35, 0.0, 128.0)": got code 0x00, want 0x80): a zero input times a negative
    norm weight is -0.  The quotient now takes x's sign.
  - quant.hip, weight_dequant_kernel to f16: the compiler folded the multiply and the conversion into v_fma_mixlo_f16 x, s, 0,
    which rounds once instead of twice and turns code 0x80 (-0) into +0; shown by test_weight_dequant_every_code[f16] and the
    stride case ("(1, 185, 0.0, -0.0)").  The fp32 product is now kept as a value of its own.
  - oracle/fp8.py: NaN and Inf inputs (section D) -- the reference's kernels drop NaN in the maximum and clamp a NaN quotient
    to -448 (tl.max / tl.maximum / tl.clamp with propagate_nan NONE); the kernel already did, the oracle (torch.clamp, amax)
    did not and was corrected.

Mutations tried by hand on the MI355X (other builds of the library, never committed; each run once against this whole module;
all of them change only computed values or move a store inside a guarded buffer) and what caught them:
  - norm_common.h, rmsnorm_row: `n_chunks - 2` in the clamp of the x loads: 45 cases -- every dim but 8 of section A plain
    (15; one chunk has nothing to clamp), all 18 fused-quant cases of A, all 12 mla_qkv_post cases (q_norm).
  - rmsnorm_row: `dim + 8` in the mean: 46 cases, all 16 dims of A plain, the 18 fused-quant cases, the 12 mla_qkv_post cases.
  - rmsnorm_wide_finish: `dim + 8` in the mean: 48 cases, every test of section B.
  - quant.hip, act_quant_kernel: the neighbouring group's scale (`__shfl_xor(sc, 16)`): all 12 cases of section D, e.g.
    "bf16 mode 0 (1, 128) codes: 128 of 128 elements differ".
  - rmsnorm_wide_finish: `tid >> 5` for `tid >> 4` in the tile-major scale address: all 10 cases of
    test_rmsnorm_add_row_major_and_tile_major_quant ("tile-major scales (padding rows = sentinel): 2 of 32 elements differ")
    and ops.rms_norm(tile_major) of section L; no row-major case.
  - sum_terms_bf16x8: `k < terms - 1`: 26 cases -- terms 2..16 of test_rmsnorm_add_sums_every_term_count_in_order (terms = 1
    does not sum), the 10 tile-major cases (their second shape has 3 terms), the 5-term aliased case.
  - moe.hip, moe_sum_kernel: the stride of the grid-stride loop DOUBLED: test_moe_sum_second_stride_iteration alone ("output
    elements never written").  A HALVED stride only computes the same elements twice; no comparison can see it.
  - quant.hip, act_quant_kernel and silu_and_mul_kernel: the stride doubled: the 6 cases of
    test_act_quant_second_stride_iteration, and test_silu_and_mul_every_gate_bit_pattern.
  - kv.hip, gqa_qkv_post_kernel: `page < num_pages` removed: the two out-of-table cases of section H for that entry, "k cache:
    the guard pages after the cache: 2176 of 34816 elements differ in 1 rows" -- a changed guard page, no fault.
  - the same test removed from append_paged_kv_kernel (5 out-of-table cases, one per row size), mla_kv_prep_kernel (1),
    mla_kv_row_ptr (the 6 out-of-table cases of mla_qkv_post) and the append epilogue of bf16_gemm_add_norm_kernel
    (out-of-table-0, the launch that carries the page id == num_pages): each only by its own out-of-table case.
  - kv.hip, rope_kernel: `2 * i` for `i` in the half-split layout: the three layout-1 cases of test_rope_every_type_and_layout,
    test_rope_second_stride_iteration[1] and ops.apply_rotary_pos_emb of section L; no layout-0 case.
  - w8a8_int8.hip, quant_act_int8_vec_kernel: roundf for rintf (half away from zero): all 8 vector-kernel cases of section E
    ("K=8 bf16 codes: ... (0, 1, 91.0, 90.0)"); the scalar kernel, not mutated, rightly not.
"""

import ctypes

import pytest
import torch

from tests import dense_exact as dx
from tests import row_exact as rx
from tests.util import poisoned_allocations

pytestmark = pytest.mark.gpu

ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -2
BF16, F16, F32, U8, I8 = torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.int8
G = dx.G
NULL = None


def _L():
    from chitu_amd import _lib

    return _lib


def _call(entry, *args, rc=0):
    """One launch on torch's current stream; the return code is asserted."""
    L = _L()
    conv = []
    for a in args:
        if a is None or isinstance(a, torch.Tensor):
            conv.append(L.ptr(a))
        else:
            conv.append(a)
    got = getattr(L.lib(), entry)(*conv, L.stream_ptr())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a GPU fault: nothing more is started on the card by this session
        pytest.exit(f"{entry}: {e}", returncode=3)
    assert got == rc, f"{entry} returned {got}, expected {rc}"


def i32(v):
    return ctypes.c_int32(int(v))


def i64(v):
    return ctypes.c_int64(int(v))


def f32(v):
    return ctypes.c_float(float(v))


def _strided(t, stride, fill=float("nan")):
    """t [rows, cols] on the GPU as a view of a [rows, stride] buffer whose other columns hold `fill`."""
    rows, cols = t.shape
    wide = torch.full((rows, stride), fill, dtype=t.dtype) if t.is_floating_point() else torch.full((rows, stride), int(fill), dtype=t.dtype)
    wide[:, :cols] = t
    wide = wide.cuda()
    return wide, wide[:, :cols]


def _rmsnorm(x, x_stride, add, add_stride, terms, term_stride, sum_out, sum_stride, w, y, y_stride, rows, dim, q, qs, mode,
             rc=0, eps=rx.EPS):
    _call("chitu_hip_rmsnorm", x, i64(x_stride), add, i64(add_stride), i32(terms), i64(term_stride), sum_out, i64(sum_stride), w, y,
          i64(y_stride), i64(rows), i32(dim), f32(eps), q, qs, i32(mode), f32(1e-10), rc=rc)


def _report(kind, idx, what):
    n = int((idx != 0).sum())
    print(f"ROWEXACT {kind} non-central: {n} of {len(idx)} ({what})")
    return n


def _check_fused_quant(y_got, q_buf, qs_buf, mode, what):
    """Codes and scales == the quantiser oracle applied to the bf16 row the kernel wrote."""
    q_want, s_want = rx.quant_fp8(y_got, mode - 1)
    rx.assert_same(qs_buf.check(f"{what} scales"), s_want, f"{what} scales")
    rx.assert_same(q_buf.check(f"{what} codes", written=False), q_want.view(U8), f"{what} codes", nan_ok=True)


# ---------------------------------------------------------------- A: the 256-thread form
@pytest.mark.parametrize("dim", rx.A_DIMS)
def test_rmsnorm_plain_every_pass_boundary_strided(dim):
    """x at a row stride of dim + 576 (NaN between the rows), y at dim + 8 with sentinel columns, rows 1 and 3."""
    for rows in rx.A_ROWS:
        c = rx.rms_case(rows, dim)
        keep, x = _strided(c["x"], dim + 576)
        y = rx.Guarded(rows, dim, BF16, stride=dim + 8)
        _rmsnorm(x, dim + 576, NULL, 0, 1, 0, NULL, 0, c["w"].cuda(), y.view, dim + 8, rows, dim, NULL, NULL, 0)
        what = f"chitu_hip_rmsnorm rows={rows} dim={dim}"
        t, rr, want = rx.rms_oracle(c["v"], c["w"])
        _report("rsqrtf", rx.match_rows(y.check(what), t, rr, want, what), what)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dim", rx.A_QDIMS)
def test_rmsnorm_plain_fused_quant_and_null_y(dim, mode):
    for rows in rx.A_ROWS:
        c = rx.rms_case(rows, dim, seed=mode)
        keep, x = _strided(c["x"], dim + 576)
        w = c["w"].cuda()
        y = rx.Guarded(rows, dim, BF16, stride=dim + 8)
        q, qs = rx.Guarded(rows, dim, U8), rx.Guarded(rows, dim // 128, F32)
        _rmsnorm(x, dim + 576, NULL, 0, 1, 0, NULL, 0, w, y.view, dim + 8, rows, dim, q.view, qs.view, mode)
        what = f"chitu_hip_rmsnorm rows={rows} dim={dim} quant_mode={mode}"
        t, rr, want = rx.rms_oracle(c["v"], c["w"])
        y_got = y.check(what)
        _report("rsqrtf", rx.match_rows(y_got, t, rr, want, what), what)
        _check_fused_quant(y_got, q, qs, mode, what)
        q2, qs2 = rx.Guarded(rows, dim, U8), rx.Guarded(rows, dim // 128, F32)
        _rmsnorm(x, dim + 576, NULL, 0, 1, 0, NULL, 0, w, NULL, 0, rows, dim, q2.view, qs2.view, mode)
        _check_fused_quant(y_got, q2, qs2, mode, what + " y=NULL")


# ---------------------------------------------------------------- B: the wide form
def _wide(c, rows, dim, terms, mode=0, alias=None, tile_major=False):
    """One launch of the residual form.  add rows at a non-contiguous stride; alias: None | "x" | "add" (sum_out = that buffer).
    Returns (y, q buffer, qs buffer)."""
    w = c["w"].cuda()
    x = c["x"].cuda().contiguous()
    add_stride = terms * dim + 64
    keep, add = _strided(c["add"].reshape(rows, terms * dim), add_stride)
    what = f"chitu_hip_rmsnorm(add) rows={rows} dim={dim} terms={terms} mode={mode} alias={alias} tile_major={tile_major}"
    y = rx.Guarded(rows, dim, BF16, stride=dim + 8)
    if alias == "x":
        s_ptr, s_stride, s_buf = x, dim, None
    elif alias == "add":
        assert terms == 1
        s_ptr, s_stride, s_buf = add, add_stride, None
    else:
        s_buf = rx.Guarded(rows, dim, BF16, stride=dim + 8)
        s_ptr, s_stride = s_buf.view, dim + 8
    q = qs = None
    if mode == 3:
        q, qs = rx.Guarded(rows, dim, I8, sentinel=rx.INT8_SENTINEL), rx.Guarded(rows, 1, F32)
    elif mode and tile_major:
        t = (rows + 15) // 16
        q, qs = rx.Guarded(t * 16, dim, U8), rx.Guarded(t * (dim // 128), 16, F32)
    elif mode:
        q, qs = rx.Guarded(rows, dim, U8), rx.Guarded(rows, dim // 128, F32)
    _rmsnorm(x, dim, add, add_stride, terms, dim, s_ptr, s_stride, w, y.view, dim + 8, rows, dim, q and q.view, qs and qs.view,
             mode + (4 if tile_major else 0))
    if alias == "x":
        s_got = x.cpu()
    elif alias == "add":
        s_got = add.cpu()
        assert bool(torch.isnan(keep.cpu()[:, dim:]).all()), f"{what}: stored between the add rows"
    else:
        s_got = s_buf.check(what + " sum_out")
    rx.assert_same(s_got, rx.residual_oracle(c["x"], rx.sum_terms_oracle(c["add"])), what + " sum_out")
    t_, rr, want = rx.rms_oracle(c["v"], c["w"])
    y_got = y.check(what)
    _report("rsqrtf", rx.match_rows(y_got, t_, rr, want, what), what)
    return y_got, q, qs, what


@pytest.mark.parametrize("dim", [d for d in rx.A_DIMS if d % 8 == 0])
def test_rmsnorm_add_every_dim(dim):
    for rows in rx.A_ROWS:
        _wide(rx.rms_case(rows, dim, 1), rows, dim, 1)


@pytest.mark.parametrize("terms", list(range(1, 17)))
def test_rmsnorm_add_sums_every_term_count_in_order(terms):
    for dim in rx.B_TERM_DIMS:
        _wide(rx.rms_case(3, dim, terms), 3, dim, terms)


@pytest.mark.parametrize("alias", ["x", "add"])
def test_rmsnorm_add_sum_out_may_be_an_input(alias):
    for dim in (136, 8192):
        _wide(rx.rms_case(3, dim, 1, seed=7), 3, dim, 1, alias=alias)
    if alias == "x":
        _wide(rx.rms_case(3, 2048, 5, seed=7), 3, 2048, 5, alias=alias)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("rows", rx.B_TILE_ROWS)
def test_rmsnorm_add_row_major_and_tile_major_quant(rows, mode):
    """The tile-major output is the row-major codes and scales, permuted; the padding rows of the last tile keep the sentinel."""
    for dim, terms in ((256, 1), (2176, 3)):
        c = rx.rms_case(rows, dim, terms, seed=rows)
        y_got, q, qs, what = _wide(c, rows, dim, terms, mode)
        _check_fused_quant(y_got, q, qs, mode, what)
        y_tm, qt, qst, what = _wide(c, rows, dim, terms, mode, tile_major=True)
        rx.assert_same(y_tm, y_got, what + " y")
        q_want, s_want = rx.quant_fp8(y_got, mode - 1)
        qt_want, st_want = rx.to_tile_major(q_want.view(U8), s_want)
        rx.assert_same(qt.check(what + " codes", written=False), qt_want, what + " tile-major codes (padding rows = sentinel)")
        got_s = rx.bits(qst.check(what + " scales", written=False))
        rx.assert_same(got_s, st_want.reshape(got_s.shape), what + " tile-major scales (padding rows = sentinel)")


@pytest.mark.parametrize("dim", rx.B_INT8_DIMS)
def test_rmsnorm_add_int8_mode(dim):
    for rows in rx.A_ROWS:
        y_got, q, qs, what = _wide(rx.rms_case(rows, dim, 1, seed=3), rows, dim, 1, mode=3)
        q_want, s_want = rx.quant_int8(y_got)
        rx.assert_same(qs.check(what + " scales"), s_want[:, None], what + " int8 scales")
        rx.assert_same(q.check(what + " codes", written=False), q_want, what + " int8 codes")


# ---------------------------------------------------------------- C: return codes
def test_rmsnorm_return_codes_leave_the_output_alone():
    c = rx.rms_case(3, 136, 1)
    x, w, add = c["x"].cuda(), c["w"].cuda(), c["add"].reshape(3, 136).cuda()
    big = torch.zeros(3, 17 * 136, dtype=BF16, device="cuda")
    y, s = rx.Guarded(3, 8200, BF16), rx.Guarded(3, 136, BF16)
    _rmsnorm(x, 136, NULL, 0, 1, 0, NULL, 0, w, y.view, 8200, 3, 12, NULL, NULL, 0, rc=ERR_UNSUPPORTED)       # dim % 8 != 0
    _rmsnorm(x, 8200, NULL, 0, 1, 0, NULL, 0, w, y.view, 8200, 3, 8200, NULL, NULL, 0, rc=ERR_UNSUPPORTED)    # dim > 8192
    _rmsnorm(x, 136, big, 17 * 136, 17, 136, s.view, 136, w, y.view, 8200, 3, 136, NULL, NULL, 0, rc=ERR_UNSUPPORTED)  # 17 terms
    _rmsnorm(x, 136, add, 136, 1, 0, s.view, 136, w, y.view, 8200, 0, 136, NULL, NULL, 0, rc=0)               # no rows
    _rmsnorm(x, 136, NULL, 0, 1, 0, NULL, 0, w, y.view, 8200, 0, 136, NULL, NULL, 0, rc=0)
    y.untouched("y after four refused / empty calls")
    s.untouched("sum_out after four refused / empty calls")


# ---------------------------------------------------------------- D: act_quant
def _act_quant(x, dt, mode, what):
    rows, cols = x.numel() // x.shape[-1], x.shape[-1]
    q, s = rx.Guarded(rows, cols, U8), rx.Guarded(rows, cols // 128, F32)
    _call("chitu_hip_act_quant_fp8", x.cuda(), ctypes.c_int(rx.DT_CODE[dt]), i64(rows), i64(cols), i32(128), i32(mode), f32(1e-10),
          q.view, s.view)
    q_want, s_want = rx.quant_fp8(x.reshape(rows, cols), mode)
    rx.assert_same(s.check(what + " scales"), s_want, what + " scales")
    rx.assert_same(q.check(what + " codes", written=False), q_want.view(U8), what + " codes", nan_ok=True)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_act_quant_adversarial_table(dt, mode):
    """Ties at every e4m3 midpoint in both signs, the zero group, scales outside the fast-division range beside normal groups
    in one wave, a quotient above 448, NaN and +-Inf among finite values (the NaN rule: oracle/fp8.py)."""
    x, kinds = rx.quant_table(dt)
    what = f"chitu_hip_act_quant_fp8 {dt} mode {mode}"
    _act_quant(x[:1].contiguous(), dt, mode, what + " (1, 128)")
    _act_quant(x[:12].reshape(3, 2, 256).contiguous(), dt, mode, what + " (3, 2, 256)")
    _act_quant(x.reshape(5, 512).contiguous(), dt, mode, what + " the whole table (5, 512)")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_act_quant_second_stride_iteration(dt, mode):
    _act_quant(rx.quant_big(dt), dt, mode, f"chitu_hip_act_quant_fp8 {dt} mode {mode} 4104 x 1024 (32 832 groups)")


# ---------------------------------------------------------------- E: int8 activations
def _quant_int8(x, dt, what):
    rows, K = x.shape
    q, s = rx.Guarded(rows, K, I8, sentinel=rx.INT8_SENTINEL), rx.Guarded(rows, 1, F32)
    _call("chitu_hip_quant_act_int8", x.cuda(), ctypes.c_int(rx.DT_CODE[dt]), i64(rows), i64(K), q.view, s.view)
    q_want, s_want = rx.quant_int8(x)
    rx.assert_same(s.check(what + " scales"), s_want[:, None], what + " scales")
    rx.assert_same(q.check(what + " codes", written=False), q_want, what + " codes")


def _int8_rows(K, dt):
    return torch.stack([rx.int8_row(K, dt, 0, 1), rx.int8_row(K, dt, -3, 2), torch.zeros(K, dtype=rx.DTYPES[dt]), rx.int8_row(K, dt, 4, 3, special=False)])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K", rx.E_VEC_K)
def test_quant_act_int8_vector_kernel(K, dt):
    _quant_int8(_int8_rows(K, dt), dt, f"chitu_hip_quant_act_int8 (vector) K={K} {dt}")


@pytest.mark.parametrize("K,dt", [(K, dt) for K in rx.E_SCALAR_K for dt in ("bf16", "f16", "f32")] + [(2048, "f32")])
def test_quant_act_int8_scalar_kernel(K, dt):
    """K = 1, 7, 1001 (K % 8 != 0) and 16 392 (> 16 384) reach the scalar kernel in every type, K = 2048 with fp32 input only."""
    _quant_int8(_int8_rows(K, dt), dt, f"chitu_hip_quant_act_int8 (scalar) K={K} {dt}")


# ---------------------------------------------------------------- F: weight dequant
def _dequant(codes, scales, dt, what):
    B, M, N = codes.shape
    y = rx.Guarded(B * M, N, rx.DTYPES[dt])
    _call("chitu_hip_weight_dequant_fp8", codes.cuda(), scales.cuda(), i64(B), i64(M), i64(N), i32(128), i32(0), ctypes.c_int(rx.DT_CODE[dt]), y.view)
    want = rx.dequant_oracle(codes, scales, rx.DTYPES[dt]).reshape(B * M, N)
    got = y.check(what, written=False)
    rx.assert_same(got, want, what, nan_ok=True)
    live = ~torch.isnan(want)
    assert not bool((rx.bits(got)[live] == y.sentinel).any()), f"{what}: elements never written"


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_weight_dequant_every_code(dt):
    """N = 272 takes the 16-byte path, N = 250 the ragged one; the block scales differ and one overflows f16 (448 x 4096)."""
    for N in (272, 250):
        g = torch.Generator().manual_seed(N)
        codes = ((torch.arange(2 * 130 * N) * 7 + torch.randint(0, 3, (2 * 130 * N,), generator=g)) % 256).to(U8).view(2, 130, N)
        assert len(set(codes.flatten().tolist())) == 256
        scales = torch.tensor([[[0.5, 4096.0, 3.0], [0.001953125, 2.0 ** -20, 1.5]], [[2.0, 0.75, 1.0], [4096.0, 2.0 ** 10, 5.0]]])
        scales = scales[:, :, : (N + 127) // 128].contiguous()  # [batch, ceil(130 / 128), ceil(N / 128)]
        _dequant(codes, scales, dt, f"chitu_hip_weight_dequant_fp8 N={N} out {dt}")


def test_weight_dequant_second_stride_iteration():
    M, N = 2100, 4096
    assert M * (N // 16) > 2048 * 256
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 256, (1, M, N), generator=g, dtype=U8)
    scales = torch.ldexp(torch.ones(1, 17, 32), torch.randint(-6, 5, (1, 17, 32), generator=g).int())
    _dequant(codes, scales, "f16", f"chitu_hip_weight_dequant_fp8 {M} x {N} out f16")


# ---------------------------------------------------------------- G: RoPE
def _rope(bs, qh, kh, d, dt, layout, what):
    dtype = rx.DTYPES[dt]
    q, cos, sin = rx.rope_inputs(bs, max(qh, 1), d, dtype, seed=bs + qh + d)
    k, _, _ = rx.rope_inputs(bs, max(kh, 1), d, dtype, seed=bs + kh + d + 1)
    pad = 16
    keep_q, qv = _strided(q.reshape(bs * max(qh, 1), d), d + pad)
    keep_k, kv = _strided(k.reshape(bs * max(kh, 1), d), d + pad)
    oq, ok = rx.Guarded(bs * max(qh, 1), d, dtype, stride=d + 8), rx.Guarded(bs * max(kh, 1), d, dtype, stride=d + 8)
    _call("chitu_hip_rope", qv, kv, oq.view, ok.view, cos.cuda(), sin.cuda(), ctypes.c_int(rx.DT_CODE[dt]), i32(bs), i32(qh), i32(kh), i32(d),
          i64(max(qh, 1) * (d + pad)), i64(d + pad), i64(max(kh, 1) * (d + pad)), i64(d + pad),
          i64(max(qh, 1) * (d + 8)), i64(d + 8), i64(max(kh, 1) * (d + 8)), i64(d + 8), i32(layout))
    for name, heads, x, out in (("q", qh, q, oq), ("k", kh, k, ok)):
        if heads == 0:
            out.untouched(f"{what}: out_{name} with no {name} heads")
        else:
            rx.assert_same(out.check(f"{what} out_{name}"), rx.rope_oracle(x, cos, sin, layout).reshape(bs * heads, d), f"{what} out_{name}")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_rope_every_type_and_layout(dt, layout):
    for d in (2, 128):
        for qh, kh in ((3, 2), (0, 2), (3, 0)):
            _rope(5, qh, kh, d, dt, layout, f"chitu_hip_rope {dt} layout {layout} d={d} heads {qh}+{kh}")


@pytest.mark.parametrize("layout", [0, 1])
def test_rope_second_stride_iteration(layout):
    assert 129 * 66 * 64 > 2048 * 256
    _rope(129, 33, 33, 128, "bf16", layout, f"chitu_hip_rope bf16 layout {layout} 129 x (33 + 33) heads x 128")


# ---------------------------------------------------------------- H: appends
class _Pages:
    """A paged cache [G + num_pages + G pages, page, *row] on the GPU filled with a pattern; the kernel is given the pointer
    G pages in and `num_pages`: whatever a kernel without the out-of-table guard writes lands in a guard page."""

    def __init__(self, num_pages, page, row_shape, dtype, seed):
        g = torch.Generator().manual_seed(seed)
        n = (num_pages + 2 * G) * page
        if dtype == U8:
            init = torch.randint(0, 256, (n, *row_shape), generator=g, dtype=U8)
        else:
            init = (torch.randn(n, *row_shape, generator=g) * 100.0).to(dtype)
        self.init, self.page, self.num_pages = init, page, num_pages
        self.dev = init.cuda()
        self.inner = self.dev[G * page:]

    def rows(self):
        """(guard rows before, interior rows, guard rows after) after the launch, on the CPU."""
        got = self.dev.cpu()
        a, b = G * self.page, (G + self.num_pages) * self.page
        return got, a, b

    def check(self, want_inner, what):
        got, a, b = self.rows()
        rx.assert_same(got[:a].reshape(a, -1), self.init[:a].reshape(a, -1), what + ": the guard pages before the cache")
        rx.assert_same(got[b:].reshape(a, -1), self.init[b:].reshape(a, -1), what + ": the guard pages after the cache")
        rx.assert_same(got[a:b].reshape(b - a, -1), want_inner.reshape(b - a, -1), what + ": the cache")

    def inner_init(self):
        a, b = G * self.page, (G + self.num_pages) * self.page
        return self.init[a:b]


@pytest.mark.parametrize("bad", [False, True], ids=["valid", "out-of-table"])
@pytest.mark.parametrize("row_bytes", rx.APPEND_ROW_BYTES + [4112])
def test_append_paged_kv_both_copy_paths(row_bytes, bad):
    B, page = 8, 4
    lens, table, num_pages, _, kinds = rx.paged_batch(B, page, seed=row_bytes, bad=bad)
    pages = _Pages(num_pages, page, (row_bytes,), U8, seed=row_bytes)
    new = torch.randint(0, 256, (B, row_bytes), generator=torch.Generator().manual_seed(1), dtype=U8)
    _call("chitu_hip_append_paged_kv", pages.inner, i64(num_pages), i32(page), i64(row_bytes), table.cuda(), i32(table.shape[1]),
          new.cuda(), lens.cuda(), i32(B))
    pages.check(rx.append_oracle(pages.inner_init(), new, lens, table, page, num_pages), f"chitu_hip_append_paged_kv row_bytes={row_bytes} {kinds}")


def _mla_inputs(B, q_lora, seed):
    """[q_a (q_lora, if any) | kv_c (512) | k_pe (64)] rows on integer data, the norm weights, cos / sin."""
    c_kv = rx.rms_case(B, 512, seed=seed)
    g = torch.Generator().manual_seed(seed + 99)
    k_pe = (dx.ints(g, 40, B, 64).float() * 0.125).to(BF16)
    ang = torch.rand(B, 32, generator=g) * 6.2831853
    parts = [c_kv["x"], k_pe]
    c_q = None
    if q_lora:
        c_q = rx.rms_case(B, q_lora, seed=seed + 1)
        parts = [c_q["x"]] + parts
    return torch.cat(parts, 1), c_q, c_kv, k_pe, torch.cos(ang).contiguous(), torch.sin(ang).contiguous()


def _mla_quantum(B, c_q, c_kv):
    """The power of two every element of an _mla_inputs row is an integer multiple of."""
    two = lambda e, n: torch.ldexp(torch.ones(B, 1), e.int()[:, None]).expand(B, n)
    return torch.cat([two(c_q["e"], c_q["x"].shape[1]), two(c_kv["e"], 512), torch.full((B, 64), 0.125)], 1)


def _check_mla_cache(pages, c_kv, k_pe, cos, sin, lens, table, num_pages, what):
    """Every live row is [one kv_norm candidate, whole | RoPE(k_pe)], everything else as it was."""
    page = pages.page
    got, a, b = pages.rows()
    t, rr, want = rx.rms_oracle(c_kv["v"], c_kv["w"])
    pe = rx.rope_oracle(k_pe[:, None, :], cos, sin, 0)[:, 0]
    live = [(i, rx.live_row(i, lens, table, page, table.shape[1], num_pages)) for i in range(len(lens))]
    live = [(i, r) for i, r in live if r is not None]
    ids = torch.tensor([i for i, _ in live])
    got_rows = torch.stack([got[a + r] for _, r in live])
    idx = rx.match_rows(got_rows[:, :512].contiguous(), t[ids], rr[:, ids], want[:, ids], what + " kv_norm rows (live sequences)")
    _report("rsqrtf", idx, what)
    new = torch.cat([got_rows[:, :512], pe[ids]], 1)
    full_new = torch.zeros(len(lens), 576, dtype=BF16)
    full_new[ids] = new
    pages.check(rx.append_oracle(pages.inner_init(), full_new, lens, table, page, num_pages), what)


@pytest.mark.parametrize("bad", [False, True], ids=["valid", "out-of-table"])
def test_mla_kv_prep_against_the_oracle(bad):
    B, page, H = 8, 4, 5
    lens, table, num_pages, _, kinds = rx.paged_batch(B, page, seed=11, bad=bad)
    row, _, c_kv, k_pe, cos, sin = _mla_inputs(B, 0, seed=21)
    keep, kv_in = _strided(row, 576 + 64)
    g = torch.Generator().manual_seed(5)
    q = (dx.ints(g, 40, B, H, 64).float() * 0.25).to(BF16)
    qb = rx.Guarded(B * H, 64, BF16, stride=72)
    qb.view.copy_(rx.bits(q.reshape(B * H, 64)).cuda())
    pages = _Pages(num_pages, page, (576,), BF16, seed=2)
    _call("chitu_hip_mla_kv_prep", kv_in, i64(640), qb.view, i64(H * 72), i64(72), i32(H), cos.cuda(), sin.cuda(), c_kv["w"].cuda(), f32(rx.EPS),
          pages.inner, i64(num_pages), i32(page), table.cuda(), i32(table.shape[1]), lens.cuda(), i32(B), i32(512), i32(64))
    what = f"chitu_hip_mla_kv_prep {kinds}"
    _check_mla_cache(pages, c_kv, k_pe, cos, sin, lens, table, num_pages, what)
    rx.assert_same(qb.check(what + " q_pe"), rx.rope_oracle(q, cos, sin, 0).reshape(B * H, 64), what + " q_pe (every sequence is rotated)")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("bad", [False, True], ids=["valid", "out-of-table"])
def test_gqa_qkv_post_against_the_oracle(bad, layout):
    B, page, hq, hkv, d = 8, 4, 3, 17, 128
    assert (hq + hkv) * d // 2 > 256 and hkv * d // 8 > 256  # both loops repeat
    lens, table, num_pages, _, kinds = rx.paged_batch(B, page, seed=13 + layout, bad=bad)
    x, cos, sin = rx.rope_inputs(B, hq + 2 * hkv, d, BF16, seed=31)
    N = (hq + 2 * hkv) * d
    qkv = rx.Guarded(B, N, BF16, stride=N + 8)
    qkv.view.copy_(rx.bits(x.reshape(B, N)).cuda())
    kc, vc = _Pages(num_pages, page, (hkv, d), BF16, seed=3), _Pages(num_pages, page, (hkv, d), BF16, seed=4)
    _call("chitu_hip_gqa_qkv_post", qkv.view, i64(N + 8), i32(hq), i32(hkv), i32(d), cos.cuda(), sin.cuda(), i32(layout), kc.inner, vc.inner,
          i64(num_pages), i32(page), table.cuda(), i32(table.shape[1]), lens.cuda(), i32(B))
    what = f"chitu_hip_gqa_qkv_post layout {layout} {kinds}"
    rot = rx.rope_oracle(x[:, :hq + hkv], cos, sin, layout)
    want_row = x.clone()
    want_row[:, :hq] = rot[:, :hq]
    rx.assert_same(qkv.check(what + " qkv"), want_row.reshape(B, N), what + " qkv row (q rotated in place, k and v as they were)")
    kc.check(rx.append_oracle(kc.inner_init(), rot[:, hq:], lens, table, page, num_pages), what + " k cache")
    vc.check(rx.append_oracle(vc.inner_init(), x[:, hq + hkv:], lens, table, page, num_pages), what + " v cache")


def _split_planes(row, quantum, P, seed):
    """fp32 planes [P, B, n], every value an integer multiple of its element's quantum (the power of two of its part of the
    row), that sum to the bf16 row: every partial sum is an integer below 2^24 times the quantum, exact in any order."""
    g = torch.Generator().manual_seed(seed)
    planes = [dx.ints(g, 30, *row.shape).float() * quantum for _ in range(P - 1)]
    last = row.float() - sum(planes) if planes else row.float()
    out = torch.stack(planes + [last])
    assert torch.equal(out.double().sum(0), row.double()) and torch.equal((out / quantum).round(), out / quantum)
    assert float((out / quantum).abs().sum(0).max()) < 2 ** 24
    return out.contiguous()


@pytest.mark.parametrize("bad", [False, True], ids=["valid", "out-of-table"])
@pytest.mark.parametrize("q_lora", [128, 2048])
@pytest.mark.parametrize("planes", [0, 1, 16])
def test_mla_qkv_post_against_the_oracle(planes, q_lora, bad):
    B, page = 8, 4
    lens, table, num_pages, _, kinds = rx.paged_batch(B, page, seed=17 + planes, bad=bad)
    row, c_q, c_kv, k_pe, cos, sin = _mla_inputs(B, q_lora, seed=41 + planes)
    stride = q_lora + 576 + 8
    if planes == 0:
        keep, src = _strided(row, stride)
    else:
        pl = _split_planes(row, _mla_quantum(B, c_q, c_kv), planes, seed=planes)
        wide = torch.full((planes, B, stride), float("nan"))
        wide[:, :, : q_lora + 576] = pl
        src = wide.cuda()
    q, qs = rx.Guarded(B, q_lora, U8), rx.Guarded(B, q_lora // 128, F32)
    pages = _Pages(num_pages, page, (576,), BF16, seed=6)
    _call("chitu_hip_mla_qkv_post", src, i32(planes), i64(stride), i32(q_lora), c_q["w"].cuda(), f32(rx.EPS), q.view, qs.view, c_kv["w"].cuda(),
          f32(rx.EPS), cos.cuda(), sin.cuda(), pages.inner, i64(num_pages), i32(page), table.cuda(), i32(table.shape[1]), lens.cuda(), i32(B),
          i32(512), i32(64))
    what = f"chitu_hip_mla_qkv_post planes={planes} q_lora={q_lora} {kinds}"
    _check_mla_cache(pages, c_kv, k_pe, cos, sin, lens, table, num_pages, what)
    # q_norm + act_quant: y is not written, so the codes and scales of a row are those of ONE candidate row
    t, rr, want = rx.rms_oracle(c_q["v"], c_q["w"])
    got_q, got_s = q.check(what + " codes", written=False), qs.check(what + " scales")
    cand = [rx.quant_fp8(w_, 0) for w_ in want]
    both = torch.cat([rx.canon_nan(got_q).int(), rx.bits(got_s).int()], 1)
    cand_both = torch.stack([torch.cat([rx.canon_nan(cq.view(U8)).int(), rx.bits(cs).int()], 1) for cq, cs in cand])
    hit = (both[None] == cand_both).all(-1)
    assert bool(hit.any(0).all()), (f"{what}: q rows {(~hit.any(0)).nonzero().flatten().tolist()} equal the quantised form of no candidate row; "
                                    f"first differences from the central one (row, col): {(both != cand_both[0]).nonzero()[:6].tolist()}")
    _report("rsqrtf", torch.where(hit[0], 0, 1), what + " q_norm")


QP = dict(M=4, K=512, hq=2, hkv=1, d=64)


@pytest.mark.parametrize("variant", ["valid", "out-of-table-0", "out-of-table-1"])
def test_bf16_gemm_add_norm_qkv_post_append_epilogue(variant):
    """The projection is a signed selection (every weight row holds one power of two), so the GEMM output is one exact
    product per element whatever the summation order, and the epilogue's RoPE and append are compared with the oracle
    directly.  Four tokens per launch: the four out-of-table kinds take two launches."""
    from chitu_amd import ops

    M, K, hq, hkv, d = QP["M"], QP["K"], QP["hq"], QP["hkv"], QP["d"]
    N = (hq + 2 * hkv) * d
    assert ops.bf16_add_norm_fits(M, N, K)
    bad = variant != "valid"
    page = 4
    lens, table, num_pages, _, kinds = rx.paged_batch(M, page, seed=int(variant[-1]) if bad else 2, bad=bad)
    c = rx.rms_case(M, K, 1, seed=9)
    g = torch.Generator().manual_seed(8)
    col = (torch.arange(N) * 37 + 5) % K
    W = torch.zeros(N, K)
    W[torch.arange(N), col] = torch.ldexp(torch.ones(N), torch.randint(-1, 2, (N,), generator=g).int()) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)
    ang = torch.rand(M, d // 2, generator=g) * 6.2831853
    cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    out, s_out = rx.Guarded(M, N, BF16), rx.Guarded(M, K, BF16)
    kc, vc = _Pages(num_pages, page, (hkv, d), BF16, seed=7), _Pages(num_pages, page, (hkv, d), BF16, seed=8)
    _call("chitu_hip_bf16_gemm_add_norm_qkv_post", c["x"].cuda(), i64(K), c["add"].reshape(M, K).cuda(), i64(K), s_out.view, i64(K), c["w"].cuda(),
          f32(rx.EPS), W.to(BF16).cuda(), out.view, i64(M), i64(K), i32(hq), i32(hkv), i32(d), cos.cuda(), sin.cuda(), kc.inner, vc.inner,
          i64(num_pages), i32(page), table.cuda(), i32(table.shape[1]), lens.cuda())
    what = f"chitu_hip_bf16_gemm_add_norm_qkv_post {kinds}"
    rx.assert_same(s_out.check(what + " sum_out"), c["v"], what + " sum_out")
    t, rr, y = rx.rms_oracle(c["v"], c["w"])
    got_out = out.check(what + " qkv_out", written=False)
    sent = rx.bits(got_out) == dx.SENTINEL16
    assert not bool(sent[:, : hq * d].any()) and bool(sent[:, hq * d:].all()), f"{what}: qkv_out holds the rotated q heads and nothing else"
    cand_q, cand_k, cand_v = [], [], []
    for yc in y:
        proj = (yc.float() @ W.T).to(BF16)  # one product per element: exact
        assert torch.equal(proj.double(), yc.double() @ W.double().T)
        heads = proj.view(M, hq + 2 * hkv, d)
        rot = rx.rope_oracle(heads[:, : hq + hkv], cos, sin, 0)
        cand_q.append(rot[:, :hq].reshape(M, hq * d)), cand_k.append(rot[:, hq:].reshape(M, hkv * d)), cand_v.append(heads[:, hq + hkv:].reshape(M, hkv * d))
    gk, a, b = kc.rows()
    gv, _, _ = vc.rows()
    new_k, new_v = torch.zeros(M, hkv, d, dtype=BF16), torch.zeros(M, hkv, d, dtype=BF16)
    picks = []
    for m in range(M):
        r = rx.live_row(m, lens, table, page, table.shape[1], num_pages)
        got_row = [got_out[m, : hq * d]] + ([gk[a + r].reshape(-1), gv[a + r].reshape(-1)] if r is not None else [])
        ok = [all(torch.equal(rx.bits(gr), rx.bits(cd[ci][m])) for gr, cd in zip(got_row, (cand_q, cand_k, cand_v))) for ci in range(len(y))]
        assert any(ok), f"{what}: token {m} (t = {float(t[m])!r}) equals the epilogue of no candidate row"
        picks.append(ok.index(True))
        if r is not None:
            new_k[m], new_v[m] = gk[a + r], gv[a + r]
    _report("rsqrtf", torch.tensor(picks), what)
    kc.check(rx.append_oracle(kc.inner_init(), new_k, lens, table, page, num_pages), what + " k cache")
    vc.check(rx.append_oracle(vc.inner_init(), new_v, lens, table, page, num_pages), what + " v cache")


# ---------------------------------------------------------------- I: the decode prologue
def test_embed_rope_gather_clamps_positions():
    B, dim, half, V, T = 7, 136, 300, 9, 6
    g = torch.Generator().manual_seed(2)
    table = (torch.randn(V, dim, generator=g)).to(BF16)
    cos_t, sin_t = torch.randn(T, half, generator=g), torch.randn(T, half, generator=g)
    tokens = torch.tensor([100, 108, 99, 109, 104, 100, 107])
    pos = torch.tensor([-1, T, 0, T - 1, 3, -7, T + 5], dtype=torch.int32)
    h, co, so = rx.Guarded(B, dim, BF16), rx.Guarded(B, half, F32), rx.Guarded(B, half, F32)
    _call("chitu_hip_embed_rope_gather", tokens.cuda(), table.cuda(), i64(100), i64(V), i32(dim), h.view, pos.cuda(), cos_t.cuda(), sin_t.cuda(),
          i64(T), i32(half), co.view, so.view, i32(B))
    wh, wc, ws = rx.embed_gather_oracle(tokens, table, 100, pos, cos_t, sin_t)
    rx.assert_same(h.check("embed rows"), wh, "chitu_hip_embed_rope_gather h")
    rx.assert_same(co.check("cos"), wc, "chitu_hip_embed_rope_gather cos (positions -1 and table_rows clamp)")
    rx.assert_same(so.check("sin"), ws, "chitu_hip_embed_rope_gather sin")


# ---------------------------------------------------------------- J: moe_sum
def _moe_sum(tokens, topk, N, seed):
    g = torch.Generator().manual_seed(seed)
    c3 = (dx.ints(g, 7, tokens, topk, N).float() * 0.25).to(BF16)
    out = rx.Guarded(tokens, N, BF16)
    _call("chitu_hip_moe_sum", c3.cuda(), out.view, i64(tokens), i32(topk), i64(N))
    what = f"chitu_hip_moe_sum tokens={tokens} topk={topk} N={N}"
    rx.assert_same(out.check(what), rx.moe_sum_oracle(c3), what)


@pytest.mark.parametrize("topk", rx.J_TOPK)
def test_moe_sum_every_topk(topk):
    _moe_sum(5, topk, 136, topk)


def test_moe_sum_second_stride_iteration():
    assert 4100 * (1032 // 8) > 2048 * 256
    _moe_sum(4100, 2, 1032, 0)


# ---------------------------------------------------------------- K: SiLU
def test_silu_and_mul_every_gate_bit_pattern():
    """65 536 rows x d = 136: row r's gates are the bf16 bit pattern r, against +-0, subnormals, +-the largest finite value
    and full-mantissa up values; 1 114 112 chunks, so the stride loop (4096 x 256 threads) runs twice."""
    gate, up, x = rx.silu_case()
    out = rx.Guarded(65536, 136, BF16)
    _call("chitu_hip_silu_and_mul", x.cuda(), out.view, i64(65536), i64(136))
    got = out.check("silu", written=False)
    want = rx.silu_oracle(gate, up)
    idx = rx.silu_match(got, want, "chitu_hip_silu_and_mul 65536 x 136")
    live = ~torch.isnan(want[0])
    assert not bool((rx.bits(got)[live] == dx.SENTINEL16).any()), "chitu_hip_silu_and_mul: elements never written"
    _report("expf", idx, "gates of chitu_hip_silu_and_mul")
    # d = 8: one chunk per row
    x8 = torch.cat([x[:, :8], up[:, :8]], 1).contiguous()
    out8 = rx.Guarded(65536, 8, BF16)
    _call("chitu_hip_silu_and_mul", x8.cuda(), out8.view, i64(65536), i64(8))
    rx.silu_match(out8.check("silu d=8", written=False), want[:, :, :8].contiguous(), "chitu_hip_silu_and_mul 65536 x 8")


# ---------------------------------------------------------------- L: the wrappers do not depend on what their buffers held
def test_ops_wrappers_do_not_depend_on_what_their_buffers_held():
    from chitu_amd import fused_moe, ops
    from chitu_amd.quantize import w8a8

    c = rx.rms_case(17, 2176, 3, seed=1)
    x, w, add = c["x"].cuda(), c["w"].cuda(), c["add"].cuda()
    tab, _ = rx.quant_table("bf16")
    tab = tab.reshape(5, 512).cuda()
    rq, rcos, rsin = rx.rope_inputs(5, 3, 128, BF16, seed=1)
    rk = rx.rope_inputs(5, 2, 128, BF16, seed=2)[0]
    _, _, sx = rx.silu_case()
    sx = sx[::97, : 2 * 128].contiguous().cuda()
    lens, table, num_pages, _, _ = rx.paged_batch(8, 4, seed=1)
    row, c_q, c_kv, k_pe, cos, sin = _mla_inputs(8, 128, seed=3)
    gx = rx.rope_inputs(8, 3 + 2 * 2, 128, BF16, seed=4)
    i8 = _int8_rows(2056, "bf16").cuda()

    def flat(r):
        return [t for t in (r if isinstance(r, (tuple, list)) else [r]) if t is not None]

    def tiled():
        _, y, tq, _ = ops.rms_norm(x, w, rx.EPS, quant="act", add=add, tile_major=True)
        return (y,) + tuple(tq.to_row_major())

    def kv_prep():
        cache = torch.zeros(num_pages, 4, 576, dtype=BF16, device="cuda")
        q_pe = rq[:, :, :64].contiguous().cuda().repeat(2, 1, 1)[:8]
        ops.mla_kv_prep(row[:, 128:].cuda(), q_pe, cos.cuda(), sin.cuda(), c_kv["w"].cuda(), rx.EPS, cache, table[:8].contiguous().cuda(), lens.cuda())
        return cache, q_pe

    def qkv_post():
        cache = torch.zeros(num_pages, 4, 576, dtype=BF16, device="cuda")
        q, s = ops.mla_qkv_post(row.cuda(), 128, c_q["w"].cuda(), rx.EPS, c_kv["w"].cuda(), rx.EPS, cos.cuda(), sin.cuda(), cache,
                                table[:8].contiguous().cuda(), lens.cuda())
        return cache, q.view(U8), s

    def gqa_post():
        kc = torch.zeros(num_pages, 4, 2, 128, dtype=BF16, device="cuda")
        vc = torch.zeros_like(kc)
        qkv = gx[0].clone().cuda()
        ops.gqa_qkv_post(qkv, 3, 2, gx[1].cuda(), gx[2].cuda(), kc, vc, table[:8].contiguous().cuda(), lens.cuda())
        return qkv, kc, vc

    def append():
        cache = torch.zeros(num_pages, 4, 30, dtype=BF16, device="cuda")
        ops.append_to_paged_kv_cache(cache, table[:8].contiguous().cuda(), gx[0][:, 0, :30].contiguous().cuda(), lens.cuda())
        return cache

    calls = {
        "rms_norm": lambda: ops.rms_norm(x, w, rx.EPS),
        "rms_norm(quant=group)": lambda: ops.rms_norm(x, w, rx.EPS, quant="group"),
        "rms_norm(add=terms, quant=act)": lambda: ops.rms_norm(x, w, rx.EPS, quant="act", add=add),
        "rms_norm(add, tile_major)": tiled,
        "rms_norm(add, int8)": lambda: ops.rms_norm(x, w, rx.EPS, quant="int8", add=add[:, 0].contiguous()),
        "act_quant_deepseek_v3": lambda: ops.act_quant_deepseek_v3(tab),
        "per_token_group_quant_fp8": lambda: fused_moe.per_token_group_quant_fp8(tab, 128),
        "quant_act": lambda: w8a8.quant_act(i8),
        "silu_and_mul": lambda: ops.silu_and_mul(sx),
        "apply_rotary_pos_emb": lambda: ops.apply_rotary_pos_emb(rq.cuda(), rk.cuda(), rcos.cuda(), rsin.cuda(), "hf-llama"),
        "append_to_paged_kv_cache": append,
        "mla_kv_prep": kv_prep,
        "mla_qkv_post": qkv_post,
        "gqa_qkv_post": gqa_post,
        "embed_rope_gather": lambda: ops.embed_rope_gather(torch.tensor([3, 0, 11, 5]).cuda(), x[:9].contiguous(), 2, torch.tensor([0, 9, 2, -1], dtype=torch.int32).cuda(),
                                                           rcos.cuda(), rsin.cuda()),
    }
    for name, call in calls.items():
        plain = [t.cpu() for t in flat(call())]
        with poisoned_allocations():
            foul = [t.cpu() for t in flat(call())]
        assert len(plain) == len(foul)
        for k, (p, f) in enumerate(zip(plain, foul)):
            p2, f2 = (p.view(U8), f.view(U8)) if p.dtype == torch.float8_e4m3fn else (p, f)
            rx.assert_same(f2.reshape(-1, f2.shape[-1]), p2.reshape(-1, p2.shape[-1]), f"ops.{name} output {k} inside poisoned_allocations()", nan_ok=True)
