"""The q / k / v bias kernels (csrc/qkv_post_row16.hip) on the GPU against the CPU oracle of tests/qkv_bias_exact.py: the decode form
over bf16 and over fp8 page rows and the prefill form.  Every comparison is bit for bit: q and every cache byte against the
oracle (poisoned caches between guard pages: exactly one row per live sequence changes), against the existing entry run on the
bf16 sum qkv + bias, and the three forms against each other."""

import pytest
import torch

from tests import qkv_bias_exact as bx
from tests import row_exact as rx
from tests.test_gpu_row_exact import _Pages, _call, i32, i64

pytestmark = pytest.mark.gpu

BF16, U8, D, PAGE = torch.bfloat16, torch.uint8, 128, bx.PAGE
ENTRY = {"bf16": "chitu_ext5_gqa_qkv_bias_post", "fp8": "chitu_ext5_gqa_qkv_bias_post_kv_fp8"}
OLD_ENTRY = {"bf16": "chitu_hip_gqa_qkv_post", "fp8": "chitu_hip_gqa_qkv_post_kv_fp8"}


def _caches(fmt, num_pages, hkv):
    row_shape, dt = ((hkv, 144), U8) if fmt == "fp8" else ((hkv, D), BF16)
    return _Pages(num_pages, PAGE, row_shape, dt, seed=3), _Pages(num_pages, PAGE, row_shape, dt, seed=4)


def _decode_exact(fmt, hq, hkv, bs, layout, bad, seed):
    c = bx.bias_case(bs, hq, hkv, seed=seed)
    x, bias = c["x"], c["bias"]
    lens, table, num_pages, kinds = bx.paged(bs, seed=seed, bad=bad)
    nh = hq + 2 * hkv
    N = nh * D
    cos, sin, table_d, lens_d, bias_d = c["cos"].cuda(), c["sin"].cuda(), table.cuda(), lens.cuda(), bias.cuda()
    qkv = rx.Guarded(bs, N, BF16, stride=N + 8)
    qkv.view.copy_(rx.bits(x.reshape(bs, N)).cuda())
    kc, vc = _caches(fmt, num_pages, hkv)
    _call(ENTRY[fmt], qkv.view, i64(N + 8), i32(hq), i32(hkv), i32(D), cos, sin, i32(layout), kc.inner, vc.inner, i64(num_pages), i32(PAGE),
          table_d, i32(table.shape[1]), lens_d, i32(bs), bias_d)
    what = f"{ENTRY[fmt]} hq={hq} hkv={hkv} bs={bs} layout={layout} lens={lens.tolist()} {kinds}"
    _, q, k, v = bx.bias_oracle(c, layout)
    row = qkv.check(what + " qkv", written=False).view(bs, nh, D)
    rx.assert_same(row[:, :hq], q, what + " q heads (every sequence, in place)")
    rx.assert_same(row[:, hq:], x[:, hq:], what + " k and v heads of the qkv row (as they were)")
    # the caches: exactly one row per live sequence (fp8: codes, scale and the 12 zero bytes), every other byte as it was
    live = [b for b in range(bs) if rx.live_row(b, lens, table, PAGE, table.shape[1], num_pages) is not None]
    assert len(live) == bs - len(kinds) and (bad or len(live) == bs)
    new_k, new_v = (bx.fp8_rows(k), bx.fp8_rows(v)) if fmt == "fp8" else (k, v)
    kc.check(rx.append_oracle(kc.inner_init(), new_k, lens, table, PAGE, num_pages), what + " k cache")
    vc.check(rx.append_oracle(vc.inner_init(), new_v, lens, table, PAGE, num_pages), what + " v cache")
    # the existing entry on the bf16 sum (a torch add on the device): the same q and the same cache bytes
    summed = (x.cuda() + bias_d.view(nh, D)).contiguous()
    kc2, vc2 = _caches(fmt, num_pages, hkv)
    _call(OLD_ENTRY[fmt], summed, i64(N), i32(hq), i32(hkv), i32(D), cos, sin, i32(layout), kc2.inner, vc2.inner, i64(num_pages), i32(PAGE),
          table_d, i32(table.shape[1]), lens_d, i32(bs))
    rx.assert_same(row[:, :hq], summed.cpu()[:, :hq], what + f" q == {OLD_ENTRY[fmt]} on qkv + bias")
    assert torch.equal(kc.dev, kc2.dev) and torch.equal(vc.dev, vc2.dev), what + f": cache bytes == {OLD_ENTRY[fmt]} on qkv + bias"
    print(f"QKVBIAS {what}: q, {len(live)} k rows and {len(live)} v rows exact, == {OLD_ENTRY[fmt]}(qkv + bias)")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("bs", bx.BATCHES)
@pytest.mark.parametrize("hq,hkv", bx.SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_decode_form_exact(fmt, hq, hkv, bs, layout):
    """Old lengths 0, 15, 16 and 17 at page 16 spread over the rows (tests/test_qkv_bias_exact_host.py checks the spread)."""
    _decode_exact(fmt, hq, hkv, bs, layout, False, seed=hq + hkv + layout + bs)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("hq,hkv", bx.SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_decode_form_out_of_table_rows_write_no_cache_byte_and_still_produce_q(fmt, hq, hkv, layout, seed):
    """Seed 0: a negative length and a table entry of num_pages; seed 1: a length past the table and an entry of -1 -- among
    three valid rows."""
    _decode_exact(fmt, hq, hkv, 5, layout, True, seed=seed)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("rows", bx.PREFILL_ROWS)
@pytest.mark.parametrize("hq,hkv", bx.SHAPES)
def test_prefill_form_is_the_oracle_and_the_decode_forms_rows(hq, hkv, rows, layout):
    """One launch over `rows` strided rows (37 rows of 9 heads: 21 workgroups, the last partly empty) -> three contiguous
    outputs between guard rows: the oracle's bits, and the bits the decode form leaves in q and in the page rows."""
    c = bx.bias_case(rows, hq, hkv, seed=layout)
    nh = hq + 2 * hkv
    N = nh * D
    src = torch.full((rows, N + 8), float("nan"), dtype=BF16)
    src[:, :N] = c["x"].reshape(rows, N)
    src = src.cuda()
    cos, sin, bias_d = c["cos"].cuda(), c["sin"].cuda(), c["bias"].cuda()
    oq, ok, ov = rx.Guarded(rows, hq * D, BF16), rx.Guarded(rows, hkv * D, BF16), rx.Guarded(rows, hkv * D, BF16)
    _call("chitu_ext5_qkv_bias_rope", src, i64(N + 8), i64(D), bias_d, cos, sin, oq.view, ok.view, ov.view, i64(rows), i32(hq), i32(hkv),
          i32(D), i32(layout))
    what = f"chitu_ext5_qkv_bias_rope hq={hq} hkv={hkv} rows={rows} layout={layout}"
    _, q, k, v = bx.bias_oracle(c, layout)
    got_q, got_k, got_v = oq.check(what + " out_q").view(rows, hq, D), ok.check(what + " out_k").view(rows, hkv, D), ov.check(what + " out_v").view(rows, hkv, D)
    rx.assert_same(got_q, q, what + " q heads")
    rx.assert_same(got_k, k, what + " k heads")
    rx.assert_same(got_v, v, what + " v heads")
    assert torch.equal(rx.bits(src.cpu()[:, :N]), rx.bits(c["x"].reshape(rows, N)))  # the inputs are read only
    # the decode form on the same rows: row b appends at position b of a sequence of its own
    lens = torch.tensor([bx.OLD_LENS[b % 4] for b in range(rows)], dtype=torch.int32)
    table = torch.arange(2 * rows, dtype=torch.int32).view(rows, 2)
    work = c["x"].cuda()
    kc, vc = (torch.zeros(2 * rows, PAGE, hkv, D, dtype=BF16, device="cuda") for _ in range(2))
    _call(ENTRY["bf16"], work, i64(N), i32(hq), i32(hkv), i32(D), cos, sin, i32(layout), kc, vc, i64(2 * rows), i32(PAGE), table.cuda(), i32(2),
          lens.cuda(), i32(rows), bias_d)
    at = (table[torch.arange(rows), (lens // PAGE).long()].long() * PAGE + (lens % PAGE).long()).cuda()
    assert torch.equal(work[:, :hq].cpu(), got_q), what + ": q of the decode form == out_q"
    assert torch.equal(kc.view(-1, hkv, D)[at].cpu(), got_k) and torch.equal(vc.view(-1, hkv, D)[at].cpu(), got_v), what + ": page rows == out_k, out_v"
    print(f"QKVBIAS {what}: {rows * nh} heads exact, == the decode form's q and page rows")


def test_ops_wrappers_agree_with_each_other_and_with_the_quantiser():
    """ops.gqa_qkv_bias_post, its fp8 form and ops.qkv_bias_rope on random data with both rotary types: the same q, the fp8
    rows are the quantiser's image of the bf16 rows."""
    from chitu_amd import ops

    hq, hkv, bs = 7, 1, 5
    for rotary in ("llama", "hf-llama"):
        g = torch.Generator().manual_seed(5)
        x = (torch.randn(bs, hq + 2 * hkv, D, generator=g) * 2).to(BF16).cuda()
        bias = (torch.randn((hq + 2 * hkv) * D, generator=g) * 0.5).to(BF16).cuda()
        lens, table, num_pages, _ = bx.paged(bs, seed=1)
        cos_t, sin_t = bx.rope_table()
        cos, sin = cos_t[lens.long() + 3].contiguous().cuda(), sin_t[lens.long() + 3].contiguous().cuda()
        kc, vc = (torch.zeros(num_pages, PAGE, hkv, D, dtype=BF16, device="cuda") for _ in range(2))
        k8, v8 = (torch.full((num_pages, PAGE, hkv, 144), 0x55, dtype=U8, device="cuda") for _ in range(2))
        q16 = ops.gqa_qkv_bias_post(x.clone(), hq, hkv, cos, sin, kc, vc, table.cuda(), lens.cuda(), bias, rotary_type=rotary)
        q8 = ops.gqa_qkv_bias_post_kv_fp8(x.clone(), hq, hkv, cos, sin, k8, v8, table.cuda(), lens.cuda(), bias, rotary_type=rotary)
        oq, ok, ov = ops.qkv_bias_rope(x, hq, hkv, bias, cos, sin, rotary_type=rotary)
        at = torch.tensor([int(table[b, int(lens[b]) // PAGE]) * PAGE + int(lens[b]) % PAGE for b in range(bs)]).cuda()
        assert torch.equal(q16, oq) and torch.equal(q8, oq) and oq.is_contiguous() and ok.is_contiguous() and ov.is_contiguous()
        assert torch.equal(kc.view(-1, hkv, D)[at], ok) and torch.equal(vc.view(-1, hkv, D)[at], ov)
        assert torch.equal(ov, x[:, hq + hkv:] + bias.view(-1, D)[hq + hkv:])
        assert torch.equal(k8.view(-1, hkv, 144)[at], ops.gqa_kv_quant_fp8(ok)) and torch.equal(v8.view(-1, hkv, 144)[at], ops.gqa_kv_quant_fp8(ov))
        want_q, want_k = ops.apply_rotary_pos_emb(*(t.contiguous() for t in (x + bias.view(-1, D)).split([hq, hkv, hkv], 1)[:2]), cos, sin, rotary_type=rotary)
        assert torch.equal(oq, want_q) and torch.equal(ok, want_k), "== chitu_hip_rope on the bf16 sum"
    print("QKVBIAS ops wrappers: decode bf16 == decode fp8 == prefill == rope(qkv + bias), both rotary types")


def test_decode_form_takes_the_multi_token_row_tables():
    """T = 3 rows per sequence from the cache manager's decode_multi buffers, two sequences whose rows cross a page edge: the
    rows land at consecutive positions of each sequence and equal the prefill form on the same rows."""
    from chitu_amd import ops
    from chitu_amd.cache_manager import PagedKVCacheManager

    hq, hkv, T = 4, 2, 3
    cache = PagedKVCacheManager(0, 1, num_hot_req=4, block_size=PAGE, max_seq_len=64, device="cuda", n_local_kv_heads=hkv, head_dim=D,
                                dtype=BF16)
    reqs, olds = ["a", "b"], [15, 30]
    for r, n in zip(reqs, olds):
        cache.register_sequence(r, n)
    cache.prepare_block_table_for_decode_multi(reqs, T)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(len(reqs) * T, hq + 2 * hkv, D, generator=g).to(BF16).cuda()
    bias = bx.bias_row(hq, hkv).cuda()
    row_lens = cache.get_gpu_multi_row_lens()
    assert row_lens.tolist() == [15, 16, 17, 30, 31, 32]
    cos_t, sin_t = bx.rope_table()
    cos, sin = cos_t.cuda()[row_lens.long()].contiguous(), sin_t.cuda()[row_lens.long()].contiguous()
    k_cache, v_cache = cache.get_paged_kv_cache(0)
    k_cache.zero_(), v_cache.zero_()
    q = ops.gqa_qkv_bias_post(x.clone(), hq, hkv, cos, sin, k_cache, v_cache, cache.get_gpu_multi_block_table(), row_lens, bias,
                              rotary_type="hf-llama")
    oq, ok, ov = ops.qkv_bias_rope(x, hq, hkv, bias, cos, sin, rotary_type="hf-llama")
    assert torch.equal(q, oq)
    for i, (r, n) in enumerate(zip(reqs, olds)):
        pages = torch.tensor(cache.block_table[r], device="cuda")
        assert len(pages) == (n + T + PAGE - 1) // PAGE
        seq_k, seq_v = k_cache[pages].flatten(0, 1), v_cache[pages].flatten(0, 1)
        assert torch.equal(seq_k[n:n + T], ok[i * T:(i + 1) * T]) and torch.equal(seq_v[n:n + T], ov[i * T:(i + 1) * T])
        assert not bool(seq_k[:n].any()) and not bool(seq_k[n + T:].any())  # nothing but the T rows
    assert int((k_cache != 0).any(-1).any(-1).sum()) == len(reqs) * T
    print("QKVBIAS decode form on decode_multi's row tables: 6 rows at positions 15..17 and 30..32 == the prefill form")
