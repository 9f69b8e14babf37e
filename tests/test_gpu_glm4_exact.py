"""The partial-rotary entries (include/chitu_hip_ext7.h, csrc/qkv_post_row16.hip) on the GPU against the CPU oracle of
tests/glm4_exact.py: the decode form over bf16 and over fp8 page rows, the prefill form and the plain RoPE entry.  Every comparison
is on bit patterns: q and every cache byte against the oracle (poisoned caches between guard pages: exactly one row per live
sequence changes), the full width against the chitu_ext5_ entries and chitu_hip_rope, the forms against each other.  The shapes
are the smallest that reach every lane class -- rotating, passing, and the boundary lane at R = 8 and R = 120 -- and every pass
of the decode loop; one line `GLM4EXACT <entry> <case>: ok, <n> elements` per case."""

import pytest
import torch

from tests import glm4_exact as gx
from tests import row_exact as rx
from tests.test_gpu_row_exact import _Pages, _call, i32, i64

pytestmark = pytest.mark.gpu

BF16, U8, F32, D, PAGE = torch.bfloat16, torch.uint8, torch.float32, 128, gx.PAGE
ENTRY = {"bf16": "chitu_ext7_gqa_qkv_bias_post", "fp8": "chitu_ext7_gqa_qkv_bias_post_kv_fp8"}
EXT5_ENTRY = {"bf16": "chitu_ext5_gqa_qkv_bias_post", "fp8": "chitu_ext5_gqa_qkv_bias_post_kv_fp8"}
BAD_ARG, UNSUPPORTED = -1, -2


def _caches(fmt, num_pages, hkv):
    row_shape, dt = ((hkv, 144), U8) if fmt == "fp8" else ((hkv, D), BF16)
    return _Pages(num_pages, PAGE, row_shape, dt, seed=3), _Pages(num_pages, PAGE, row_shape, dt, seed=4)


def _decode_exact(fmt, hq, hkv, bs, R, bad, seed):
    c = gx.glm4_case(bs, hq, hkv, R, seed=seed)
    x, bias = c["x"], c["bias"]
    lens, table, num_pages, kinds = gx.paged(bs, seed=seed, bad=bad)
    nh = hq + 2 * hkv
    N = nh * D
    cos, sin, table_d, lens_d, bias_d = c["cos"].cuda(), c["sin"].cuda(), table.cuda(), lens.cuda(), bias.cuda()
    qkv = rx.Guarded(bs, N, BF16, stride=N + 8)
    qkv.view.copy_(rx.bits(x.reshape(bs, N)).cuda())
    kc, vc = _caches(fmt, num_pages, hkv)
    _call(ENTRY[fmt], qkv.view, i64(N + 8), i32(hq), i32(hkv), i32(D), cos, sin, i32(0), i32(R), kc.inner, vc.inner, i64(num_pages),
          i32(PAGE), table_d, i32(table.shape[1]), lens_d, i32(bs), bias_d)
    case = f"hq={hq} hkv={hkv} bs={bs} R={R} lens={lens.tolist()} {kinds}"
    what = f"{ENTRY[fmt]} {case}"
    y, q, k, v = gx.glm4_oracle(c)
    row = qkv.check(what + " qkv", written=False).view(bs, nh, D)
    rx.assert_same(row[:, :hq], q, what + " q heads (every sequence, in place)")
    rx.assert_same(row[:, :hq, R:], y[:, :hq, R:], what + " q channels behind the width == the biased input")
    rx.assert_same(row[:, hq:], x[:, hq:], what + " k and v heads of the qkv row (as they were)")
    # the caches: exactly one row per live sequence (fp8: codes, scale and the 12 zero bytes), every other byte as it was
    live = [b for b in range(bs) if rx.live_row(b, lens, table, PAGE, table.shape[1], num_pages) is not None]
    assert len(live) == bs - len(kinds) and (bad or len(live) == bs)
    new_k, new_v = (gx.fp8_rows(k), gx.fp8_rows(v)) if fmt == "fp8" else (k, v)
    kc.check(rx.append_oracle(kc.inner_init(), new_k, lens, table, PAGE, num_pages), what + " k cache")
    vc.check(rx.append_oracle(vc.inner_init(), new_v, lens, table, PAGE, num_pages), what + " v cache")
    if fmt == "bf16":  # the pass-through channels of the stored k rows are the biased input's bits
        got_k = kc.dev[rx.G * PAGE:].cpu().view(-1, hkv, D)
        for b in live:
            r = rx.live_row(b, lens, table, PAGE, table.shape[1], num_pages)
            rx.assert_same(got_k[r][:, R:], y[b, hq:hq + hkv, R:], what + f" k page row of sequence {b} behind the width")
    print(f"GLM4EXACT {ENTRY[fmt]} {case}: ok, {bs * hq * D + 2 * len(live) * hkv * (144 if fmt == 'fp8' else D)} elements")


@pytest.mark.parametrize("R", gx.WIDTHS)
@pytest.mark.parametrize("bs", gx.BATCHES)
@pytest.mark.parametrize("hq,hkv", gx.SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_decode_form_exact(fmt, hq, hkv, bs, R):
    """Old lengths 0, 15, 16 and 17 at page 16 spread over the rows, as tests/test_gpu_qkv_bias.py spreads them."""
    _decode_exact(fmt, hq, hkv, bs, R, False, seed=hq + hkv + bs)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("hq,hkv", gx.SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_decode_form_out_of_table_rows_write_no_cache_byte_and_still_produce_q(fmt, hq, hkv, seed):
    """Seed 0: a negative length and a table entry of num_pages; seed 1: a length past the table and an entry of -1 -- among
    three valid rows."""
    _decode_exact(fmt, hq, hkv, 5, 64, True, seed=seed)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("hq,hkv", [(32, 2), (4, 2)])
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_full_width_is_the_ext5_entry_byte_for_byte(fmt, hq, hkv, layout):
    bs = 3
    c = gx.glm4_case(bs, hq, hkv, 128, seed=layout)
    lens, table, num_pages, _ = gx.paged(bs, seed=layout)
    nh = hq + 2 * hkv
    N = nh * D
    cos, sin, table_d, lens_d, bias_d = c["cos"].cuda(), c["sin"].cuda(), table.cuda(), lens.cuda(), c["bias"].cuda()
    got = []
    for entry, width in ((ENTRY[fmt], (i32(128),)), (EXT5_ENTRY[fmt], ())):
        qkv = c["x"].reshape(bs, N).cuda()
        kc, vc = _caches(fmt, num_pages, hkv)
        _call(entry, qkv, i64(N), i32(hq), i32(hkv), i32(D), cos, sin, i32(layout), *width, kc.inner, vc.inner, i64(num_pages), i32(PAGE),
              table_d, i32(table.shape[1]), lens_d, i32(bs), bias_d)
        got.append((qkv, kc.dev, vc.dev))
    for a, b, name in zip(got[0], got[1], ("qkv row", "k cache", "v cache")):
        assert torch.equal(rx.bits(a), rx.bits(b)), (fmt, hq, hkv, layout, name)
    assert not torch.equal(rx.bits(got[0][0]), rx.bits(c["x"].reshape(bs, N).cuda()))
    print(f"GLM4EXACT {ENTRY[fmt]} hq={hq} hkv={hkv} bs={bs} R=128 layout={layout} == {EXT5_ENTRY[fmt]}: ok, "
          f"{sum(t.numel() for t in got[0])} elements")


@pytest.mark.parametrize("R", gx.WIDTHS + [128])
@pytest.mark.parametrize("rows", gx.PREFILL_ROWS)
@pytest.mark.parametrize("hq,hkv", gx.SHAPES)
def test_prefill_form_is_the_oracle_and_the_decode_forms_rows(hq, hkv, rows, R):
    """One launch over `rows` strided rows (37 rows of 36 heads: 84 workgroups, the last partly empty) -> three contiguous outputs
    between guard rows: the oracle's bits, and the bits the decode form leaves in q and in the page rows."""
    c = gx.glm4_case(rows, hq, hkv, R, seed=R)
    nh = hq + 2 * hkv
    N = nh * D
    src = torch.full((rows, N + 8), float("nan"), dtype=BF16)
    src[:, :N] = c["x"].reshape(rows, N)
    src = src.cuda()
    cos, sin, bias_d = c["cos"].cuda(), c["sin"].cuda(), c["bias"].cuda()
    oq, ok, ov = rx.Guarded(rows, hq * D, BF16), rx.Guarded(rows, hkv * D, BF16), rx.Guarded(rows, hkv * D, BF16)
    _call("chitu_ext7_qkv_bias_rope", src, i64(N + 8), i64(D), bias_d, cos, sin, oq.view, ok.view, ov.view, i64(rows), i32(hq), i32(hkv),
          i32(D), i32(0), i32(R))
    case = f"hq={hq} hkv={hkv} rows={rows} R={R}"
    what = f"chitu_ext7_qkv_bias_rope {case}"
    _, q, k, v = gx.glm4_oracle(c)
    got_q, got_k, got_v = (o.check(what + n).view(rows, h, D) for o, n, h in ((oq, " out_q", hq), (ok, " out_k", hkv), (ov, " out_v", hkv)))
    rx.assert_same(got_q, q, what + " q heads")
    rx.assert_same(got_k, k, what + " k heads")
    rx.assert_same(got_v, v, what + " v heads")
    assert torch.equal(rx.bits(src.cpu()[:, :N]), rx.bits(c["x"].reshape(rows, N)))  # the inputs are read only
    # the decode form on the same rows: row b appends at a position of a sequence of its own
    lens = torch.tensor([gx.OLD_LENS[b % 4] for b in range(rows)], dtype=torch.int32)
    table = torch.arange(2 * rows, dtype=torch.int32).view(rows, 2)
    work = c["x"].cuda()
    kc, vc = (torch.zeros(2 * rows, PAGE, hkv, D, dtype=BF16, device="cuda") for _ in range(2))
    _call(ENTRY["bf16"], work, i64(N), i32(hq), i32(hkv), i32(D), cos, sin, i32(0), i32(R), kc, vc, i64(2 * rows), i32(PAGE), table.cuda(),
          i32(2), lens.cuda(), i32(rows), bias_d)
    at = (table[torch.arange(rows), (lens // PAGE).long()].long() * PAGE + (lens % PAGE).long()).cuda()
    assert torch.equal(work[:, :hq].cpu(), got_q), what + ": q of the decode form == out_q"
    assert torch.equal(kc.view(-1, hkv, D)[at].cpu(), got_k) and torch.equal(vc.view(-1, hkv, D)[at].cpu(), got_v), what + ": page rows == out_k, out_v"
    print(f"GLM4EXACT chitu_ext7_qkv_bias_rope {case}: ok, {rows * nh * D} elements")


def _rope_call(q, k, cos, sin, layout, R, entry="chitu_ext7_rope", rc=0):
    """q [bs, qh, 128], k [bs, kh, 128] or [bs, 128] (views allowed) -> (out_q, out_k) contiguous, pre-filled with NaN."""
    oq = torch.full(q.shape, float("nan"), dtype=BF16, device="cuda")
    ok = torch.full(k.shape, float("nan"), dtype=BF16, device="cuda")
    kh, k_sh, ok_sh = (1, 0, 0) if k.dim() == 2 else (k.shape[1], k.stride(1), ok.stride(1))
    width = (i32(R),) if entry == "chitu_ext7_rope" else ()
    _call(entry, q, k, oq, ok, cos, sin, i32(0), i32(q.shape[0]), i32(q.shape[1]), i32(kh), i32(D), i64(q.stride(0)), i64(q.stride(1)),
          i64(k.stride(0)), i64(k_sh), i64(oq.stride(0)), i64(oq.stride(1)), i64(ok.stride(0)), i64(ok_sh), i32(layout), *width, rc=rc)
    return oq, ok


@pytest.mark.parametrize("R", gx.WIDTHS + [128])
@pytest.mark.parametrize("k_dims", [3, 2])
def test_rope_entry_is_the_oracle_over_strided_views_and_a_2d_k(R, k_dims):
    """q and k as strided views of one merged [bs, 9, 128] projection (the prefill path's call), or k as a [bs, 128] row; 37 rows:
    more than one workgroup, the last partly empty."""
    bs, hq, hkv = 37, 5, 2
    c = gx.glm4_case(bs, hq, hkv, R, seed=R + k_dims)
    x = c["x"].cuda()
    cos, sin = c["cos"].cuda(), c["sin"].cuda()
    q = x[:, :hq]
    k = x[:, hq:hq + hkv] if k_dims == 3 else x[:, hq]
    oq, ok = _rope_call(q, k, cos, sin, 0, R)
    want_q = gx.rotate_partial(c["x"][:, :hq].contiguous(), c["cos"], c["sin"])
    want_k = gx.rotate_partial(c["x"][:, hq:hq + hkv].contiguous(), c["cos"], c["sin"])
    rx.assert_same(oq.cpu(), want_q, f"chitu_ext7_rope R={R} q")
    rx.assert_same(ok.cpu(), want_k if k_dims == 3 else want_k[:, 0], f"chitu_ext7_rope R={R} k ({k_dims}-D)")
    assert torch.equal(rx.bits(x.cpu()), rx.bits(c["x"]))  # the inputs are read only
    if R == 128:  # the frozen entry on the same views, both layouts
        for layout in (0, 1):
            a = _rope_call(q, k, cos, sin, layout, 128)
            b = _rope_call(q, k, cos, sin, layout, 128, entry="chitu_hip_rope")
            assert torch.equal(rx.bits(a[0]), rx.bits(b[0])) and torch.equal(rx.bits(a[1]), rx.bits(b[1])), layout
    print(f"GLM4EXACT chitu_ext7_rope bs={bs} qh={hq} kh={hkv if k_dims == 3 else '2-D'} R={R}: ok, {oq.numel() + ok.numel()} elements")


def _full_width_rows(bs):
    """cos / sin [bs, 64] rows for a call of the full-width entries."""
    cos_t, sin_t = gx.rope_table(128)
    return cos_t[:bs].contiguous().cuda(), sin_t[:bs].contiguous().cuda()


def test_ops_wrappers_take_glm4_and_agree_with_each_other_and_with_the_quantiser():
    """ops.gqa_qkv_bias_post, its fp8 form, ops.qkv_bias_rope and ops.apply_rotary_pos_emb[_torch] with rotary_type "glm4": the same
    q, the fp8 rows are the quantiser's image of the bf16 rows, the width comes from cos.shape[-1]."""
    from chitu_amd import _lib, ops

    hq, hkv, bs = 32, 2, 5
    c = gx.glm4_case(bs, hq, hkv, 64, seed=9)
    x, bias, cos, sin = c["x"].cuda(), c["bias"].cuda(), c["cos"].cuda(), c["sin"].cuda()
    lens, table, num_pages, _ = gx.paged(bs, seed=1)
    kc, vc = (torch.zeros(num_pages, PAGE, hkv, D, dtype=BF16, device="cuda") for _ in range(2))
    k8, v8 = (torch.full((num_pages, PAGE, hkv, 144), 0x55, dtype=U8, device="cuda") for _ in range(2))
    _lib.call_log = []
    try:
        q16 = ops.gqa_qkv_bias_post(x.clone(), hq, hkv, cos, sin, kc, vc, table.cuda(), lens.cuda(), bias, rotary_type="glm4")
        q8 = ops.gqa_qkv_bias_post_kv_fp8(x.clone(), hq, hkv, cos, sin, k8, v8, table.cuda(), lens.cuda(), bias, rotary_type="glm4")
        oq, ok, ov = ops.qkv_bias_rope(x, hq, hkv, bias, cos, sin, rotary_type="glm4")
        summed = x + bias.view(-1, D)
        rq, rk = ops.apply_rotary_pos_emb_torch(summed[:, :hq], summed[:, hq:hq + hkv], cos, sin, rotary_type="glm4")
        ops.qkv_bias_rope(x, hq, hkv, bias, *_full_width_rows(bs), rotary_type="hf-llama")  # the other types keep their entry
        names = [n for n, _ in _lib.call_log]
    finally:
        _lib.call_log = None
    assert names == ["chitu_ext7_gqa_qkv_bias_post", "chitu_ext7_gqa_qkv_bias_post_kv_fp8", "chitu_ext7_qkv_bias_rope", "chitu_ext7_rope",
                     "chitu_ext5_qkv_bias_rope"], names
    _, q, k, v = gx.glm4_oracle(c)
    rx.assert_same(oq.cpu(), q, "ops.qkv_bias_rope glm4 q")
    at = torch.tensor([int(table[b, int(lens[b]) // PAGE]) * PAGE + int(lens[b]) % PAGE for b in range(bs)]).cuda()
    assert torch.equal(q16, oq) and torch.equal(q8, oq) and torch.equal(rq, oq) and torch.equal(rk, ok)
    assert torch.equal(kc.view(-1, hkv, D)[at], ok) and torch.equal(vc.view(-1, hkv, D)[at], ov) and torch.equal(ov.cpu(), v)
    assert torch.equal(k8.view(-1, hkv, 144)[at], ops.gqa_kv_quant_fp8(ok)) and torch.equal(v8.view(-1, hkv, 144)[at], ops.gqa_kv_quant_fp8(ov))
    print(f"GLM4EXACT ops wrappers hq={hq} hkv={hkv} bs={bs} R=64: ok, {4 * oq.numel()} elements")


def test_refused_arguments_return_their_codes_and_launch_nothing():
    """R = 12, 0 or 136: CHITU_ERR_BAD_ARG; the half-split layout with R = 64: CHITU_ERR_UNSUPPORTED; a cos base off 16 bytes:
    CHITU_ERR_BAD_ARG -- on device buffers that stay as they were: q, both caches, the outputs."""
    hq, hkv, bs = 4, 2, 3
    c = gx.glm4_case(bs, hq, hkv, 64)
    nh = hq + 2 * hkv
    N = nh * D
    lens, table, num_pages, _ = gx.paged(bs, seed=0)
    wide = torch.zeros(bs * 32 + 8, dtype=F32, device="cuda")
    cos, sin = c["cos"].cuda(), c["sin"].cuda()
    cos_off = wide[2:2 + bs * 32].view(bs, 32)  # 8 bytes past a 16-byte boundary
    assert cos_off.data_ptr() % 16 == 8
    bias_d, table_d, lens_d = c["bias"].cuda(), table.cuda(), lens.cuda()
    refusals = [(12, 0, cos, BAD_ARG), (0, 0, cos, BAD_ARG), (136, 0, cos, BAD_ARG), (64, 1, cos, UNSUPPORTED), (64, 0, cos_off, BAD_ARG)]
    n = 0
    for fmt in ("bf16", "fp8"):
        for R, layout, cs, rc in refusals:
            qkv = c["x"].reshape(bs, N).cuda()
            kc, vc = _caches(fmt, num_pages, hkv)
            _call(ENTRY[fmt], qkv, i64(N), i32(hq), i32(hkv), i32(D), cs, sin, i32(layout), i32(R), kc.inner, vc.inner, i64(num_pages), i32(PAGE),
                  table_d, i32(table.shape[1]), lens_d, i32(bs), bias_d, rc=rc)
            assert torch.equal(rx.bits(qkv.cpu()), rx.bits(c["x"].reshape(bs, N))), (fmt, R, layout)
            assert torch.equal(kc.dev.cpu(), kc.init) and torch.equal(vc.dev.cpu(), vc.init), (fmt, R, layout)
            n += 1
    for R, layout, cs, rc in refusals:
        src = c["x"].reshape(bs, N).cuda()
        oq, ok, ov = rx.Guarded(bs, hq * D, BF16), rx.Guarded(bs, hkv * D, BF16), rx.Guarded(bs, hkv * D, BF16)
        _call("chitu_ext7_qkv_bias_rope", src, i64(N), i64(D), bias_d, cs, sin, oq.view, ok.view, ov.view, i64(bs), i32(hq), i32(hkv), i32(D),
              i32(layout), i32(R), rc=rc)
        for o in (oq, ok, ov):
            o.untouched(f"chitu_ext7_qkv_bias_rope R={R} layout={layout}")
        x3 = c["x"].cuda()
        a, b = _rope_call(x3[:, :hq], x3[:, hq:hq + hkv], cs, sin, layout, R, rc=rc)
        assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()), ("chitu_ext7_rope", R, layout)
        n += 2
    print(f"GLM4EXACT return codes: ok, {n} refused calls left q, the caches and the outputs as they were")
