"""The per-head QK-norm kernels (csrc/qkv_post_row16.hip) on the GPU against the CPU oracle of tests/qk_norm_exact.py: the decode form
over bf16 and over fp8 page rows and the prefill form, exact on integer data (every head equals one rr candidate as a whole,
exactly one page row per live sequence changes, nothing else does), bit-identical to each other on random data, and within
the project's bar of a float64 norm + RoPE."""

import pytest
import torch

from tests import qk_norm_exact as qx
from tests import row_exact as rx
from tests.test_gpu_row_exact import _Pages, _call, f32, i32, i64
from tests.util import assert_close

pytestmark = pytest.mark.gpu

BF16, U8, D = torch.bfloat16, torch.uint8, 128
ENTRY = {"bf16": "chitu_ext_gqa_qkv_norm_post", "fp8": "chitu_ext_gqa_qkv_norm_post_kv_fp8"}


def _whole_head_hits(got, cands, what):
    """got [heads, W], cands [C, heads, W] (any integer dtype): every head equals one candidate as a whole."""
    hit = (got[None] == cands).all(-1).any(0)
    assert bool(hit.all()), f"{what}: heads {(~hit).nonzero().flatten().tolist()[:8]} equal no candidate"


def _decode_exact(fmt, hq, hkv, bs, layout, page, bad, seed):
    c = qx.qk_case(bs, hq, hkv, seed=seed)
    x = c["x"]
    lens, table, num_pages, _, kinds = rx.paged_batch(bs, page, seed=seed, bad=bad)
    N = (hq + 2 * hkv) * D
    qkv = rx.Guarded(bs, N, BF16, stride=N + 8)
    qkv.view.copy_(rx.bits(x.reshape(bs, N)).cuda())
    row_shape, dt = ((hkv, 144), U8) if fmt == "fp8" else ((hkv, D), BF16)
    kc, vc = _Pages(num_pages, page, row_shape, dt, seed=3), _Pages(num_pages, page, row_shape, dt, seed=4)
    _call(ENTRY[fmt], qkv.view, i64(N + 8), i32(hq), i32(hkv), i32(D), c["cos"].cuda(), c["sin"].cuda(), i32(layout), kc.inner, vc.inner,
          i64(num_pages), i32(page), table.cuda(), i32(table.shape[1]), lens.cuda(), i32(bs), c["q_w"].cuda(), c["k_w"].cuda(), f32(qx.EPS))
    what = f"{ENTRY[fmt]} hq={hq} hkv={hkv} bs={bs} layout={layout} page={page} {kinds}"
    cand_q, cand_k = qx.qk_oracle(c, layout)
    row = qkv.check(what + " qkv", written=False).view(bs, hq + 2 * hkv, D)
    idx = qx.match_heads(row[:, :hq].contiguous(), cand_q, what + " q heads (every sequence, in place)")
    rx.assert_same(row[:, hq:], x[:, hq:], what + " k and v heads of the qkv row (as they were)")
    # the caches: exactly one row per live sequence, k = one candidate (fp8: its codes, scale and 12 zero bytes), v = the input
    live = [(b, rx.live_row(b, lens, table, page, table.shape[1], num_pages)) for b in range(bs)]
    live = [(b, r) for b, r in live if r is not None]
    assert len(live) == bs - len(kinds) and (bad or len(live) == bs)
    got, a, _ = kc.rows()
    new_k = torch.zeros(bs, *row_shape, dtype=dt)
    yk = cand_k[2]  # [C, bs, hkv, 128]
    for b, r in live:
        new_k[b] = got[a + r]
        cands = qx.fp8_rows(yk[:, b]) if fmt == "fp8" else rx.bits(yk[:, b])
        _whole_head_hits(new_k[b] if fmt == "fp8" else rx.bits(new_k[b]), cands, what + f" k page row of sequence {b}")
    new_v = qx.fp8_rows(x[:, hq + hkv:]) if fmt == "fp8" else x[:, hq + hkv:]
    kc.check(rx.append_oracle(kc.inner_init(), new_k, lens, table, page, num_pages), what + " k cache")
    vc.check(rx.append_oracle(vc.inner_init(), new_v, lens, table, page, num_pages), what + " v cache")
    return idx


@pytest.mark.parametrize("page", qx.PAGES)
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("bs", qx.BATCHES)
@pytest.mark.parametrize("hq,hkv", qx.SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_decode_form_exact(fmt, hq, hkv, bs, layout, page):
    """Old lengths at 0, page - 1, page, the last position the table covers and more (row_exact.paged_batch's slots; the seed
    walks a batch of one through them)."""
    _decode_exact(fmt, hq, hkv, bs, layout, page, False, seed=hq + hkv + layout + page)


def test_the_valid_cases_cover_the_four_named_lengths():
    seen = set()
    for hq, hkv in qx.SHAPES:
        for bs in qx.BATCHES:
            for layout in (0, 1):
                for page in qx.PAGES:
                    lens = rx.paged_batch(bs, page, seed=hq + hkv + layout + page)[0].tolist()
                    seen |= {("0", "page-1", "page", "last")[i] for i, v in enumerate((0, page - 1, page, 3 * page - 1)) if v in lens}
    assert seen == {"0", "page-1", "page", "last"}


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("hq,hkv", qx.SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_decode_form_out_of_table_rows_write_no_cache_byte_and_still_produce_q(fmt, hq, hkv, layout):
    """A negative length, a length past the table, a table entry of -1 and one of num_pages, among 13 valid rows."""
    _decode_exact(fmt, hq, hkv, 17, layout, 16, True, seed=3 + layout)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("bs", qx.BATCHES)
@pytest.mark.parametrize("hq,hkv", qx.SHAPES)
def test_prefill_form_exact(hq, hkv, bs, layout):
    c = qx.qk_case(bs, hq, hkv, seed=layout)
    N = (hq + 2 * hkv) * D
    src = torch.full((bs, N + 8), float("nan"), dtype=BF16)
    src[:, :N] = c["x"].reshape(bs, N)
    src = src.cuda()
    oq, ok = rx.Guarded(bs, hq * D, BF16, stride=hq * D + 8), rx.Guarded(bs, hkv * D, BF16, stride=hkv * D + 16)
    _call("chitu_ext_qk_norm_rope", src, src[:, hq * D:], oq.view, ok.view, c["cos"].cuda(), c["sin"].cuda(), c["q_w"].cuda(), c["k_w"].cuda(),
          f32(qx.EPS), i64(bs), i32(hq), i32(hkv), i32(D), i64(N + 8), i64(D), i64(N + 8), i64(D), i64(hq * D + 8), i64(D),
          i64(hkv * D + 16), i64(D), i32(layout))
    what = f"chitu_ext_qk_norm_rope hq={hq} hkv={hkv} bs={bs} layout={layout}"
    cand_q, cand_k = qx.qk_oracle(c, layout)
    qx.match_heads(oq.check(what + " out_q").view(bs, hq, D), cand_q, what + " q heads")
    qx.match_heads(ok.check(what + " out_k").view(bs, hkv, D), cand_k, what + " k heads")
    assert torch.equal(rx.bits(src.cpu()[:, :N]), rx.bits(c["x"].reshape(bs, N)))  # the inputs are read only


# ---------------------------------------------------------------- random data: the three forms against each other and float64
def _random_case(bs, hq, hkv, page, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(bs, hq + 2 * hkv, D, generator=g) * torch.rand(bs, hq + 2 * hkv, 1, generator=g) * 4).to(BF16)
    q_w, k_w = ((1 + 0.2 * torch.randn(D, generator=g)).to(BF16) for _ in range(2))
    lens, table, num_pages, _, _ = rx.paged_batch(bs, page, seed=seed)
    pos = lens.long() + 5
    cos_t, sin_t = qx.rope_table()
    return x, q_w, k_w, lens, table[:bs].contiguous(), num_pages, cos_t[pos].contiguous(), sin_t[pos].contiguous()


def _row_index(lens, table, page):
    return torch.tensor([int(table[b, int(lens[b]) // page]) * page + int(lens[b]) % page for b in range(len(lens))])


@pytest.mark.parametrize("rotary", ["llama", "hf-llama"])
@pytest.mark.parametrize("hq,hkv,bs", [(8, 2, 17), (5, 1, 3), (8, 8, 1)])
def test_the_three_forms_agree_bit_for_bit_and_with_float64(hq, hkv, bs, rotary):
    from chitu_amd import ops

    page, eps, layout = 16, 1e-6, 0 if rotary == "llama" else 1
    x, q_w, k_w, lens, table, num_pages, cos, sin = _random_case(bs, hq, hkv, page, seed=11 * hq + bs)
    dev = lambda *ts: [t.cuda() for t in ts]
    qw_d, kw_d, cos_d, sin_d, table_d, lens_d = dev(q_w, k_w, cos, sin, table, lens)
    kc, vc = (torch.zeros(num_pages, page, hkv, D, dtype=BF16, device="cuda") for _ in range(2))
    k8, v8 = (torch.full((num_pages, page, hkv, 144), 0x55, dtype=U8, device="cuda") for _ in range(2))
    w16, w8 = x.cuda(), x.cuda()
    q16 = ops.gqa_qkv_norm_post(w16, hq, hkv, cos_d, sin_d, kc, vc, table_d, lens_d, qw_d, kw_d, eps, rotary_type=rotary)
    q8 = ops.gqa_qkv_norm_post_kv_fp8(w8, hq, hkv, cos_d, sin_d, k8, v8, table_d, lens_d, qw_d, kw_d, eps, rotary_type=rotary)
    xd = x.cuda()
    oq, ok = ops.qk_norm_rope(xd[:, :hq], xd[:, hq:hq + hkv], qw_d, kw_d, eps, cos_d, sin_d, rotary_type=rotary)
    torch.cuda.synchronize()
    rows = _row_index(lens, table, page)
    k_rows, v_rows = kc.view(-1, hkv, D)[rows.cuda()], vc.view(-1, hkv, D)[rows.cuda()]
    assert torch.equal(q16, oq) and torch.equal(q8, oq), "q of the decode forms == out_q of the prefill form"
    assert torch.equal(k_rows, ok), "page rows of the decode form == out_k of the prefill form"
    assert torch.equal(v_rows, xd[:, hq + hkv:]), "v rows are the input"
    assert torch.equal(k8.view(-1, hkv, 144)[rows.cuda()], ops.gqa_kv_quant_fp8(k_rows)), "fp8 k rows == the quantiser on the bf16 rows"
    assert torch.equal(v8.view(-1, hkv, 144)[rows.cuda()], ops.gqa_kv_quant_fp8(v_rows)), "fp8 v rows == the quantiser on the bf16 rows"
    # float64 norm, then float64 RoPE (no intermediate rounding at all)
    xq = x.double()
    n = torch.cat([xq[:, :hq] * q_w.double(), xq[:, hq:hq + hkv] * k_w.double()], 1)
    n = n / ((xq[:, :hq + hkv] ** 2).mean(-1, keepdim=True) + eps).sqrt()
    c, s = cos.double()[:, None], sin.double()[:, None]
    n0, n1 = (n[..., 0::2], n[..., 1::2]) if layout == 0 else (n[..., :64], n[..., 64:])
    want = torch.empty_like(n)
    if layout == 0:
        want[..., 0::2], want[..., 1::2] = n0 * c - n1 * s, n1 * c + n0 * s
    else:
        want[..., :64], want[..., 64:] = n0 * c - n1 * s, n1 * c + n0 * s
    print("QKNORM q vs float64:", assert_close(oq.cpu().float(), want[:, :hq].float(), 1e-2, what="q"))
    print("QKNORM k vs float64:", assert_close(ok.cpu().float(), want[:, hq:].float(), 1e-2, what="k"))


def test_decode_form_takes_the_multi_token_row_tables():
    """T = 3 rows per sequence from the cache manager's decode_multi buffers, two sequences whose rows cross a page edge: the
    rows land at consecutive positions of each sequence and equal the prefill form on the same rows."""
    from chitu_amd import ops
    from chitu_amd.cache_manager import PagedKVCacheManager

    hq, hkv, T, page, eps = 4, 2, 3, 16, 1e-6
    cache = PagedKVCacheManager(0, 1, num_hot_req=4, block_size=page, max_seq_len=64, device="cuda", n_local_kv_heads=hkv, head_dim=D,
                                dtype=BF16)
    reqs, olds = ["a", "b"], [15, 30]
    for r, n in zip(reqs, olds):
        cache.register_sequence(r, n)
    cache.prepare_block_table_for_decode_multi(reqs, T)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(len(reqs) * T, hq + 2 * hkv, D, generator=g).to(BF16).cuda()
    q_w, k_w = ((1 + 0.2 * torch.randn(D, generator=g)).to(BF16).cuda() for _ in range(2))
    row_lens = cache.get_gpu_multi_row_lens()
    assert row_lens.tolist() == [15, 16, 17, 30, 31, 32]
    cos_t, sin_t = qx.rope_table()
    cos, sin = cos_t.cuda()[row_lens.long()].contiguous(), sin_t.cuda()[row_lens.long()].contiguous()
    k_cache, v_cache = cache.get_paged_kv_cache(0)
    k_cache.zero_(), v_cache.zero_()
    work = x.clone()
    q = ops.gqa_qkv_norm_post(work, hq, hkv, cos, sin, k_cache, v_cache, cache.get_gpu_multi_block_table(), row_lens, q_w, k_w, eps,
                              rotary_type="hf-llama")
    oq, ok = ops.qk_norm_rope(x[:, :hq], x[:, hq:hq + hkv], q_w, k_w, eps, cos, sin, rotary_type="hf-llama")
    assert torch.equal(q, oq)
    for i, (r, n) in enumerate(zip(reqs, olds)):
        pages = torch.tensor(cache.block_table[r], device="cuda")
        assert len(pages) == (n + T + page - 1) // page
        seq_k, seq_v = k_cache[pages].flatten(0, 1), v_cache[pages].flatten(0, 1)
        assert torch.equal(seq_k[n:n + T], ok[i * T:(i + 1) * T]) and torch.equal(seq_v[n:n + T], x[i * T:(i + 1) * T, hq + hkv:])
        assert not bool(seq_k[:n].any()) and not bool(seq_k[n + T:].any())  # nothing but the T rows
    assert int((k_cache != 0).any(-1).any(-1).sum()) == len(reqs) * T
