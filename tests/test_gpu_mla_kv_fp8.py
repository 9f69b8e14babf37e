"""FP8 latent KV cache of the MLA paged decode on the GPU: the quantiser / dequantiser / append kernels against the CPU
statement of the format (tests/test_mla_kv_fp8_host.py), the fp8 decode kernel against chitu_hip_mla_decode on the dequantised
cache (bit for bit: dequantisation is exact and the arithmetic behind it is the bf16 kernel's), one direct comparison with an
fp32 CPU attention, the backend operator, and DeepSeekV3Args(kv_cache_dtype="fp8") end to end."""
import pytest
import torch

from tests.test_mla_kv_fp8_host import ROW, dequant_ref, edge_rows, quant_ref, sample_rows
from tests.util import assert_close, max_rel_to_peak

pytestmark = pytest.mark.gpu

SCALE = 0.1352


def rows_with_edges(T, seed=0):
    return torch.cat([edge_rows(), sample_rows(T, seed)])[:T].contiguous()


# ---------------------------------------------------------------- 1. + 2. quantiser, dequantiser
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("T", [1, 3, 67])
def test_quantiser_writes_the_reference_bytes_and_nothing_else(T, strided):
    from chitu_amd import ops

    x = rows_with_edges(T, seed=T)
    if strided:  # a [:, q:q+576] view of a wider projection output
        wide = torch.randn(T, 24 + 576 + 8).to(torch.bfloat16)
        wide[:, 24:600] = x
        src = wide.cuda()[:, 24:600]
        assert not src.is_contiguous() or T == 1
    else:
        src = x.cuda()
    want = quant_ref(x)
    dst = torch.full((T + 2, 704), 0xA5, dtype=torch.uint8, device="cuda")
    ops.mla_kv_quant_fp8(src, out=dst[1 : T + 1])
    got = dst.cpu()
    assert torch.equal(got[1 : T + 1, :ROW], want)
    assert torch.equal(got[1 : T + 1, 528:ROW].contiguous().view(torch.int16), x[:, 512:].contiguous().view(torch.int16))  # the rope bytes
    guard = got.clone()
    guard[1 : T + 1, :ROW] = 0xA5
    assert bool((guard == 0xA5).all())
    assert torch.equal(ops.mla_kv_quant_fp8(src).cpu(), want)  # the allocating form


def test_dequantiser_is_the_reference_and_the_round_trip_stays_within_the_format():
    from chitu_amd import ops

    x = rows_with_edges(67, seed=9)
    rows = quant_ref(x)
    got = ops.mla_kv_dequant_fp8(rows.cuda()).cpu()
    assert torch.equal(got.view(torch.int16), dequant_ref(rows).view(torch.int16))
    rt = ops.mla_kv_dequant_fp8(ops.mla_kv_quant_fp8(x.cuda())).cpu()
    assert torch.equal(rt.view(torch.int16), got.view(torch.int16))
    lat = x[:, :512].float().view(-1, 4, 128)
    peak = lat.abs().amax(-1)
    err = (rt[:, :512].float().view(-1, 4, 128) - lat).abs().amax(-1)
    live = peak > 448.0 * 2.0 ** -64  # (a group below the scale floor flushes towards zero: the 1e-30 edge)
    assert bool((err[live] <= peak[live] * 2.0 ** -4).all()) and bool((err[~live] <= peak[~live]).all())
    assert torch.equal(rt[:, 512:].contiguous().view(torch.int16), x[:, 512:].contiguous().view(torch.int16))
    # a whole cache: leading dimensions are kept
    assert tuple(ops.mla_kv_dequant_fp8(rows[:64].view(4, 16, ROW).cuda()).shape) == (4, 16, 576)


# ---------------------------------------------------------------- 3. append
@pytest.mark.parametrize("page", [4, 64])
def test_append_changes_exactly_the_addressed_rows(page):
    from chitu_amd import ops

    lens = [0, 3, 4, 63, 64]  # first slot, last slot of a page (page 4), first of the next, and the same for page 64
    B = len(lens)
    per = 64 // page + 1
    num_pages = B * per + 3
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(page))
    table = perm[: B * per].view(B, per).to(torch.int32)
    x = rows_with_edges(B, seed=page)
    want = quant_ref(x)

    def run(table_, lens_):
        cache = torch.full((num_pages, page, ROW), 0xA5, dtype=torch.uint8, device="cuda")
        ops.append_mla_kv_fp8(cache, table_.cuda(), x.cuda().view(B, 1, 576), torch.tensor(lens_, dtype=torch.int32).cuda())
        return cache.cpu()

    def expect(table_, lens_, live):
        cache = torch.full((num_pages, page, ROW), 0xA5, dtype=torch.uint8)
        for b in live:
            cache[int(table_[b, lens_[b] // page]), lens_[b] % page] = want[b]
        return cache

    assert torch.equal(run(table, lens), expect(table, lens, range(B)))
    # an out-of-range table entry (sequence 1), a negative length (3) and a position beyond the table (0) write nothing
    bad_table = table.clone()
    bad_table[1, lens[1] // page] = num_pages
    bad_lens = list(lens)
    bad_lens[3] = -1
    bad_lens[0] = per * page
    assert torch.equal(run(bad_table, bad_lens), expect(table, lens, [2, 4]))
    bad_table[1, lens[1] // page] = -1
    assert torch.equal(run(bad_table, bad_lens), expect(table, lens, [2, 4]))


# ---------------------------------------------------------------- 4. - 6. decode
def backend(H):
    from chitu_amd.attn_backend import HipAttnBackend

    return HipAttnBackend(local_n_heads=H, max_seq_len=8192)


def garbage_cache(num_pages, page, kind):
    """Finite garbage a correct kernel never reads: kind 0 = codes 0x7e (448) with scale 2^20 and a large rope part,
    kind 1 = 0xA5 bytes everywhere."""
    if kind:
        return torch.full((num_pages, page, ROW), 0xA5, dtype=torch.uint8)
    row = torch.empty(ROW, dtype=torch.uint8)
    row[:512] = 0x7E
    row[512:528] = torch.full((4,), 2.0 ** 20).view(torch.uint8)
    row[528:] = torch.full((64,), 3.0e38).to(torch.bfloat16).view(torch.uint8)
    return row.repeat(num_pages, page, 1)


def make_case(bs, H, lens, page=64, seed=0, garbage=0):
    """q as non-contiguous views, the fp8 cache in permuted pages with garbage wherever no token lives, the table (its unused
    entries point at whole unwritten pages), the lengths."""
    g = torch.Generator().manual_seed(seed)
    per = max(1, max((l + page - 1) // page for l in lens)) + 1
    num_pages = bs * per + 2
    perm = torch.randperm(num_pages, generator=g)
    table = perm[: bs * per].view(bs, per).to(torch.int32)
    cache = garbage_cache(num_pages, page, garbage)
    for b, n in enumerate(lens):
        if n:
            rows = quant_ref(torch.cat([torch.randn(n, 512, generator=g) * (0.5 + b), torch.randn(n, 64, generator=g)], -1).to(torch.bfloat16))
            for p in range((n + page - 1) // page):
                k = min(page, n - p * page)
                cache[int(table[b, p]), :k] = rows[p * page : p * page + k]
    qw = (torch.randn(bs, H, 32 + 576 + 8, generator=g) * 0.3).to(torch.bfloat16)
    return qw, cache, table, torch.tensor(lens, dtype=torch.int32)


def split_q(qw):
    """(q_nope, q_pe) as views into a wider tensor: neither is contiguous"""
    q_nope, q_pe = qw[..., 32 : 32 + 512], qw[..., 32 + 512 : 32 + 576]
    assert not q_nope.is_contiguous() and not q_pe.is_contiguous()
    return q_nope, q_pe


def run_pair(bs, H, lens, splits, page=64, seed=0, partials=False):
    """(fp8 kernel on the cache, bf16 kernel on the dequantised cache) at the same num_splits"""
    from chitu_amd import ops

    qw, cache, table, sl = make_case(bs, H, lens, page, seed)
    be = backend(H)
    (qn, qp), c8, t, s = split_q(qw.cuda()), cache.cuda(), table.cuda(), sl.cuda()
    c16 = ops.mla_kv_dequant_fp8(c8)
    assert torch.equal(c16.cpu().view(-1, 576).view(torch.int16), dequant_ref(cache.view(-1, ROW)).view(torch.int16))
    if not partials:
        got = be.mla_decode(qn, qp, c8, s, t, SCALE, num_splits=splits).cpu()
        want = be.mla_decode(qn, qp, c16, s, t, SCALE, num_splits=splits).cpu()
        return got, want
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(H, 256, 512, generator=g) * 0.5).to(torch.float8_e4m3fn).cuda()
    sc = (torch.rand(H * 2, 4, generator=g) * 0.02 + 0.01).cuda()
    res = []
    for c in (c8, c16):  # (the partials live in one shared workspace: merged before the other arm runs)
        part = be.mla_decode(qn, qp, c, s, t, SCALE, num_splits=splits, return_partials=True)
        assert isinstance(part, tuple) and part[1] == splits
        q, s_ = ops.mla_merge_absorb_uv_quant_fp8(part[0], part[1], bs, w[:, 128:], sc, 4, 8, 1)
        res.append((q.view(torch.uint8).cpu(), s_.cpu()))
    return res


CASES = [(1, 16, [1]), (3, 5, [63, 64, 65]), (3, 5, [130, 0, 257]), (2, 32, [130, 0]), (2, 32, [257, 65])]


@pytest.mark.parametrize("splits", [1, 3, None, 7], ids=["s1", "s3", "default", "more_than_tiles"])
@pytest.mark.parametrize("bs,H,lens", CASES)
def test_decode_is_bit_identical_to_the_bf16_kernel_on_the_dequantised_cache(bs, H, lens, splits):
    got, want = run_pair(bs, H, lens, splits, seed=sum(lens) + H)
    assert not torch.isnan(want.float()).any()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    for b, n in enumerate(lens):  # an empty sequence attends to nothing: zeros, as from the bf16 kernel
        if n == 0:
            assert bool((got[b] == 0).all())


@pytest.mark.parametrize("bs,H,lens,splits", [(3, 16, [63, 64, 65], 3), (2, 32, [130, 257], 2), (3, 5, [130, 0, 257], 7)])
def test_decode_partials_merge_to_the_same_codes(bs, H, lens, splits):
    (q8, s8), (q16, s16) = run_pair(bs, H, lens, splits, seed=H, partials=True)
    assert torch.equal(q8, q16) and torch.equal(s8, s16)


@pytest.mark.parametrize("splits", [1, 2])
def test_decode_page_size_128(splits):
    got, want = run_pair(2, 16, [200, 129], splits, page=128, seed=11)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("splits", [1, 2, None])
def test_decode_many_tiles_per_split(splits):
    """ctx 4160 = 65 tiles: dozens of tiles per split, the page ids of a split cached in LDS"""
    got, want = run_pair(1, 16, [4160], splits, seed=13)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_decode_does_not_depend_on_bytes_past_the_length():
    outs = []
    for garbage in (0, 1):
        qw, cache, table, sl = make_case(3, 16, [130, 0, 257], seed=21, garbage=garbage)
        be = backend(16)
        (qn, qp), c8, t, s = split_q(qw.cuda()), cache.cuda(), table.cuda(), sl.cuda()
        outs.append([be.mla_decode(qn, qp, c8, s, t, SCALE, num_splits=n).cpu() for n in (1, 4)])
    for a, b in zip(*outs):
        assert not torch.isnan(a.float()).any() and torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert bool((outs[0][0][1] == 0).all()) and bool((outs[0][1][1] == 0).all())  # length 0


def test_decode_against_fp32_attention_over_the_dequantised_rows():
    """The chain of equalities above rests on the bf16 kernel; this one does not: softmax(scale * q . c) . c[:512] in fp32 on
    the CPU over the rows the cache holds, at the project's attention bar."""
    bs, H, lens = 2, 16, [130, 257]
    qw, cache, table, sl = make_case(bs, H, lens, seed=31)
    q_nope, q_pe = split_q(qw)
    be = backend(H)
    ref = torch.zeros(bs, H, 512)
    for b, n in enumerate(lens):
        rows = torch.cat([cache[int(table[b, p])] for p in range((n + 63) // 64)])[:n]
        c = dequant_ref(rows).float()
        q = torch.cat([q_nope[b], q_pe[b]], -1).float()
        ref[b] = torch.softmax(q @ c.T * SCALE, dim=-1) @ c[:, :512]
    for splits in (1, 3):
        out = be.mla_decode(*split_q(qw.cuda()), cache.cuda(), sl.cuda(), table.cuda(), SCALE, num_splits=splits)
        assert_close(out, ref, 1e-2, what=f"fp8 KV decode vs fp32 attention, splits={splits}")


# ---------------------------------------------------------------- 7. the backend operator
def test_mla_attn_with_kvcache_appends_quantised_rows_and_attends_over_them():
    from chitu_amd import ops

    bs, H, lens = 3, 16, [63, 64, 130]
    qw, cache, table, sl = make_case(bs, H, lens, seed=41)
    q_nope, q_pe = split_q(qw.cuda())
    kv = rows_with_edges(bs, seed=43)
    be = backend(H)
    c8 = cache.cuda()
    out = be.mla_attn_with_kvcache(q_nope, q_pe, c8, kv.cuda().view(bs, 1, 576), sl.cuda(), (sl + 1).cuda(),
                                   table.cuda(), softmax_scale=SCALE)
    assert tuple(out.shape) == (bs, 1, H, 512)
    want_cache = cache.clone()
    new = quant_ref(kv)
    for b, n in enumerate(lens):
        want_cache[int(table[b, n // 64]), n % 64] = new[b]
    assert torch.equal(c8.cpu(), want_cache)
    want = be.mla_decode(q_nope, q_pe, ops.mla_kv_dequant_fp8(want_cache.cuda()), (sl + 1).cuda(), table.cuda(), SCALE)
    assert torch.equal(out.view(bs, H, 512).cpu().view(torch.int16), want.cpu().view(torch.int16))
    # the fused decode + merge launch reads bf16 rows only: an fp8 cache takes the two-launch form
    assert be.mla_decode_merge_uv_quant(q_nope, q_pe, c8, (sl + 1).cuda(), table.cuda(), SCALE,
                                        torch.zeros(H, 128, 512, dtype=torch.uint8, device="cuda"),
                                        torch.ones(H * 2, 4, device="cuda"), 4, 8, 1) is None


# ---------------------------------------------------------------- 8. the model
def model_args(q_lora, **kw):
    from chitu_amd.deepseek_v3 import DeepSeekV3Args

    if q_lora:  # tests/test_gpu_deepseek.py::tiny_args / v2lite_like_args at two layers
        return DeepSeekV3Args(vocab_size=1024, dim=512, inter_dim=1024, moe_inter_dim=256, n_layers=2, n_dense_layers=1, n_heads=16,
                              n_routed_experts=16, n_shared_experts=1, n_activated_experts=4, n_expert_groups=4, n_limited_groups=2,
                              q_lora_rank=256, gate_bias=True, **kw)
    return DeepSeekV3Args(vocab_size=1024, dim=512, inter_dim=1024, moe_inter_dim=640, n_layers=2, n_dense_layers=1, n_heads=16,
                          n_routed_experts=16, n_shared_experts=2, n_activated_experts=6, n_expert_groups=1, n_limited_groups=1,
                          q_lora_rank=0, gate_bias=False, score_func="softmax", route_scale=1.0, **kw)


def build(args, cache_format=None, max_reqs=4, max_seq=512):
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, mla_kv_layout
    from chitu_amd.deepseek_v3 import DeepSeekV3Decoder, init_synthetic_

    shape, dtype = mla_kv_layout(cache_format or args.kv_cache_dtype)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=max_reqs, block_size=64, max_seq_len=max_seq, device="cuda",
                                kv_shape_per_sample=shape, dtype=dtype)
    model = DeepSeekV3Decoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=max_seq),
                              max_position_embeddings=max_seq, device="cuda")
    init_synthetic_(model, seed=0)
    return model, cache


PROMPTS = [[(7 * i + 3) % 1024 for i in range(5)], [(13 * i + 1) % 1024 for i in range(70)], [(29 * i + 11) % 1024 for i in range(33)]]
STEP_TOKENS = [[5, 900, 17], [321, 4, 77], [1000, 1001, 2], [64, 65, 66]]
REQS = ["a", "b", "c"]


def run_model(q_lora, fmt):
    """ragged prefill of three prompts, then four decode steps with fixed input tokens; every step eagerly AND through its
    verified graph (the graph's append rewrites the eager step's rows with the same bytes)"""
    from chitu_amd import graphs

    model, cache = build(model_args(q_lora, kv_cache_dtype=fmt))
    n0 = len(graphs.capture_log)
    logits = [model.prefill(PROMPTS, REQS).cpu()]
    graph_equal = []
    for toks in STEP_TOKENS:
        tok = torch.tensor(toks, dtype=torch.int64, device="cuda")
        cache.prepare_cache_decode(REQS)
        cache.prepare_block_table_for_decode(REQS)
        eager = model.decode(tok, use_graph=False).clone()
        replay = model.decode(tok, use_graph=True)
        graph_equal.append(torch.equal(eager, replay))
        cache.finalize_cache_single_decode(REQS)
        logits.append(eager.cpu())
    rows = []
    for r in REQS:  # layer 0's cached rows of every request, in token order
        n = cache.seq_lens[r]
        c = cache.get_paged_kv_cache(0)
        rows.append(torch.cat([c[blk] for blk in cache.block_table[r]])[:n].cpu())
    captures = graphs.capture_log[n0:]
    return dict(logits=torch.stack(logits), graph_equal=graph_equal, rows=torch.cat(rows), captures=captures)


@pytest.fixture(scope="module", params=[256, 0], ids=["q_lora", "no_q_lora"])
def model_runs(request):
    return {fmt: run_model(request.param, fmt) for fmt in ("bf16", "fp8")}


def test_model_graph_step_equals_eager_step_in_fp8_mode(model_runs):
    r = model_runs["fp8"]
    assert all(r["graph_equal"]), r["graph_equal"]
    assert r["captures"] and all(c["attempts"] == 1 and not c["mismatches"] for c in r["captures"]), r["captures"]


def test_model_layer0_rows_are_the_quantised_rows_of_the_bf16_cache_model(model_runs):
    """layer 0's rows depend on the tokens only: prefill rows (quantised on their way into the pages) and the rows of the four
    decode steps (every producer path -> stage -> quantising append) hold the quantiser's bytes of what a bf16 cache holds"""
    want = quant_ref(model_runs["bf16"]["rows"])
    got = model_runs["fp8"]["rows"]
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5 + 70 + 33 + 3 * 4, ROW)
    assert torch.equal(got, want)


# max_rel_to_peak of the fp8-cache model's logits against the bf16-cache model's over prefill + 4 decode steps, measured on an
# MI355X; the bar is twice the measurement: one flipped fp8 code in a latent row moves this tiny random model visibly
MEASURED_LOGIT_ERR = {"q_lora": 0.034821, "no_q_lora": 0.030822}


def test_model_logits_stay_close_to_the_bf16_cache_model(model_runs, request):
    a, b = model_runs["fp8"]["logits"], model_runs["bf16"]["logits"]
    assert torch.equal(a[0], b[0])  # the prompt's own attention reads the unquantised rows
    err = max_rel_to_peak(a[1:], b[1:])
    key = request.node.callspec.id
    print(f"fp8 KV cache vs bf16 KV cache, logits max_rel_to_peak [{key}]: {err:.6f}")
    assert err > 0  # the quantised cache is really read
    assert err < 2 * MEASURED_LOGIT_ERR[key], err


def test_model_cache_and_args_must_agree():
    with pytest.raises(AssertionError):
        build(model_args(256, kv_cache_dtype="fp8"), cache_format="bf16")
    with pytest.raises(AssertionError):
        build(model_args(256), cache_format="fp8")
    with pytest.raises(ValueError):
        build(model_args(256, kv_cache_dtype="fp4"), cache_format="bf16")


def test_model_generate_in_fp8_mode():
    model, cache = build(model_args(256, kv_cache_dtype="fp8"))
    free = len(cache.free_blocks)
    out = model.generate(PROMPTS[:2], 5)
    assert tuple(out.shape) == (2, 5) and out.dtype == torch.int64 and int(out.min()) >= 0 and int(out.max()) < 1024
    assert len(cache.free_blocks) == free
