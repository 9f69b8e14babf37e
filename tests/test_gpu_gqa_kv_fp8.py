"""FP8 K / V cache of the GQA / MHA paged decode on the GPU: quantiser / dequantiser / append / qkv_post against the CPU statement of
the format (tests/test_gqa_kv_fp8_host.py), the decode kernel bit for bit against the bf16 kernel on the dequantised cache, and
LlamaDecoder / MixtralDecoder with kv_cache_dtype="fp8"."""
import functools

import pytest
import torch

from oracle import gqa as ogqa
from tests.test_gqa_kv_fp8_host import ROW, dequant_ref, edge_rows, quant_ref, sample_rows
from tests.util import assert_close, max_rel_to_peak

pytestmark = pytest.mark.gpu


def rows_with_edges(T, H, seed=0):
    """[T, H, 128] bf16 over ten decades of magnitude, its first heads the format's edge heads (peaks 448, 450, 896, 0, 1e-30)"""
    x = sample_rows(T, H, seed).reshape(T * H, 128)
    e = edge_rows().reshape(-1, 128)
    n = min(len(e), T * H)
    x[:n] = e[:n]
    return x.reshape(T, H, 128)


# ---------------------------------------------------------------- 1. quantiser, dequantiser
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("T", [1, 3, 67])
def test_quantiser_writes_the_reference_bytes_and_nothing_else(T, H, strided):
    from chitu_amd import ops

    x = rows_with_edges(T, H, seed=T + H)
    if strided:  # the k slice of a merged qkv projection's output
        wide = torch.randn(T, 4 + 2 * H, 128).to(torch.bfloat16)
        wide[:, 4 : 4 + H] = x
        src = wide.cuda()[:, 4 : 4 + H]
        assert not src.is_contiguous() or T == 1
    else:
        src = x.cuda()
    want = quant_ref(x)
    assert torch.equal(ops.gqa_kv_quant_fp8(src).cpu(), want)
    # into a destination with sentinel bytes before, after and between its rows
    big = torch.full((T + 2, H * ROW + 16), 0xA5, dtype=torch.uint8, device="cuda")
    out = big[1 : T + 1, : H * ROW].unflatten(1, (H, ROW))
    ops.gqa_kv_quant_fp8(src, out=out)
    got = big.cpu()
    assert torch.equal(got[1 : T + 1, : H * ROW].reshape(T, H, ROW), want)
    assert bool((got[0] == 0xA5).all()) and bool((got[T + 1] == 0xA5).all()) and bool((got[:, H * ROW :] == 0xA5).all())


def test_dequantiser_is_the_reference():
    from chitu_amd import ops

    rows = quant_ref(rows_with_edges(67, 8, seed=3))
    want = dequant_ref(rows)
    got = ops.gqa_kv_dequant_fp8(rows.cuda()).cpu()
    assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16))
    # a whole cache [pages, page, Hkv, 144] in one call
    got4 = ops.gqa_kv_dequant_fp8(rows[:64].reshape(4, 16, 8, ROW).cuda()).cpu()
    assert torch.equal(got4.view(torch.int16), want[:64].reshape(4, 16, 8, 128).view(torch.int16))


# ---------------------------------------------------------------- 2. append
@pytest.mark.parametrize("page", [16, 256])
def test_append_changes_exactly_the_addressed_rows(page):
    from chitu_amd import ops

    g = torch.Generator().manual_seed(page)
    H, lens = 2, [15, 16, 255, 256, -1, 40]
    bs, per = len(lens), 256 // page + 1
    num_pages = bs * per + 1
    table = torch.randperm(num_pages, generator=g)[: bs * per].view(bs, per).to(torch.int32)
    table[5, 40 // page] = num_pages + 3  # an entry outside [0, num_pages): that sequence writes nothing
    k, v = rows_with_edges(bs, H, seed=1), rows_with_edges(bs, H, seed=2)
    kc = torch.randint(0, 256, (num_pages, page, H, ROW), generator=g, dtype=torch.uint8)
    vc = torch.randint(0, 256, (num_pages, page, H, ROW), generator=g, dtype=torch.uint8)
    want_k, want_v = kc.clone(), vc.clone()
    qk, qv = quant_ref(k), quant_ref(v)
    for b, L in enumerate(lens[:4]):
        want_k[int(table[b, L // page]), L % page] = qk[b]
        want_v[int(table[b, L // page]), L % page] = qv[b]
    kd, vd = kc.cuda(), vc.cuda()
    ops.append_gqa_kv_fp8(kd, vd, table.cuda(), k.cuda().unsqueeze(1), v.cuda(), torch.tensor(lens, dtype=torch.int32).cuda())
    assert torch.equal(kd.cpu(), want_k) and torch.equal(vd.cpu(), want_v)
    assert not torch.equal(want_k, kc)


# ---------------------------------------------------------------- 3. RoPE + append with quantising stores
@pytest.mark.parametrize("rotary", ["llama", "hf-llama"])
def test_qkv_post_writes_the_quantised_rows_of_the_bf16_entry(rotary):
    from chitu_amd import ops

    g = torch.Generator().manual_seed(2)
    bs, hq, hkv, hd, pages = 5, 8, 2, 128, 12
    qkv = torch.randn(bs, hq + 2 * hkv, hd, generator=g).to(torch.bfloat16)
    qkv[0, hq] *= 300.0  # heads of very different magnitude
    qkv[1, hq + hkv] *= 1e-3
    qkv = qkv.cuda()
    cos, sin = torch.randn(bs, hd // 2, generator=g).cuda(), torch.randn(bs, hd // 2, generator=g).cuda()
    table = torch.stack([torch.randperm(pages, generator=g)[:2] for _ in range(bs)]).to(torch.int32)
    lens = [0, 255, 256, 300, 511]
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    kc16 = torch.zeros(pages, 256, hkv, hd, dtype=torch.bfloat16, device="cuda")
    vc16 = torch.zeros_like(kc16)
    work16 = qkv.clone()
    q16 = ops.gqa_qkv_post(work16, hq, hkv, cos, sin, kc16, vc16, table.cuda(), lens_d, rotary_type=rotary)
    kc8 = torch.randint(0, 256, (pages, 256, hkv, ROW), generator=g, dtype=torch.uint8)
    vc8 = torch.randint(0, 256, (pages, 256, hkv, ROW), generator=g, dtype=torch.uint8)
    want_k, want_v = kc8.clone(), vc8.clone()
    for b, L in enumerate(lens):
        p, o = int(table[b, L // 256]), L % 256
        want_k[p, o] = quant_ref(kc16[p, o].cpu().unsqueeze(0))[0]
        want_v[p, o] = quant_ref(vc16[p, o].cpu().unsqueeze(0))[0]
    kd, vd, work8 = kc8.cuda(), vc8.cuda(), qkv.clone()
    q8 = ops.gqa_qkv_post_kv_fp8(work8, hq, hkv, cos, sin, kd, vd, table.cuda(), lens_d, rotary_type=rotary)
    assert torch.equal(q8, q16) and not torch.equal(q8, qkv[:, :hq])
    assert torch.equal(work8[:, hq:], qkv[:, hq:])  # k / v parts of the row untouched
    assert torch.equal(kd.cpu(), want_k) and torch.equal(vd.cpu(), want_v)


# ---------------------------------------------------------------- 4. decode
@functools.lru_cache(maxsize=None)
def decode_case(bs, Hq, Hkv, lens, page, seed=0):
    """(q, fp8 K, fp8 V, their dequantised bf16 images, lengths incl., table), all on the GPU.  Pages hold heads of mixed magnitude;
    the table is a shuffle and one page is left unused."""
    g = torch.Generator().manual_seed(seed + bs + Hq + len(lens))
    per = [(l + page - 1) // page for l in lens]
    pages = sum(per) + 2
    mag = 10.0 ** (torch.rand(pages, page, Hkv, 1, generator=g) * 2 - 1)
    k8 = quant_ref((torch.randn(pages, page, Hkv, 128, generator=g) * mag).to(torch.bfloat16).view(-1, Hkv, 128)).view(pages, page, Hkv, ROW)
    v8 = quant_ref((torch.randn(pages, page, Hkv, 128, generator=g) * mag).to(torch.bfloat16).view(-1, Hkv, 128)).view(pages, page, Hkv, ROW)
    perm = torch.randperm(pages, generator=g)
    table = torch.zeros(bs, max(per) + 1, dtype=torch.int32)
    o = 0
    for b in range(bs):
        table[b, : per[b]] = perm[o : o + per[b]].to(torch.int32)
        o += per[b]
    q = (torch.randn(bs, 1, Hq, 128, generator=g) * 0.5).to(torch.bfloat16)
    return dict(q=q.cuda(), k8=k8.cuda(), v8=v8.cuda(), k16=dequant_ref(k8).cuda(), v16=dequant_ref(v8).cuda(),
                lens=torch.tensor(lens, dtype=torch.int32).cuda(), table=table.cuda(), cpu=dict(q=q, k8=k8, v8=v8, table=table))


def run(c, fmt, splits, k8=None, v8=None, partials=False):
    from chitu_amd import workspace
    from chitu_amd.attn_backend import HipAttnBackend

    bs, _, Hq, _ = c["q"].shape
    kc, vc = (c["k8"] if k8 is None else k8, c["v8"] if v8 is None else v8) if fmt == "fp8" else (c["k16"], c["v16"])
    if partials:
        workspace.get(bs * Hq * splits * 129 * 4, "cuda", "gqa").zero_()
    out = HipAttnBackend(local_n_heads=Hq).attn_with_kvcache(c["q"], kc, vc, cache_seqlens=c["lens"], block_table=c["table"],
                                                             num_splits=splits)
    if partials:
        return out, workspace.get(bs * Hq * splits * 129 * 4, "cuda", "gqa")[: bs * Hq * splits * 129 * 4].clone()
    return out


CASES = [
    (1, 32, 8, (1,), 256),
    (3, 32, 8, (15, 16, 17), 16),
    (3, 32, 8, (255, 256, 257), 256),
    (4, 32, 8, (6, 301, 0, 1001), 64),  # one empty sequence
    (2, 8, 8, (100, 17), 64),  # MHA
    (3, 16, 1, (40, 41, 700), 64),  # group 16
]


@pytest.mark.parametrize("splits", [1, 3, None, "more"])
@pytest.mark.parametrize("bs,Hq,Hkv,lens,page", CASES)
def test_decode_is_bit_identical_to_the_bf16_kernel_on_the_dequantised_cache(bs, Hq, Hkv, lens, page, splits):
    c = decode_case(bs, Hq, Hkv, lens, page)
    if splits == "more":  # more splits than the longest sequence has 16-token steps: empty splits everywhere
        splits = (max(lens) + 15) // 16 + 3
    a, b = run(c, "fp8", splits), run(c, "bf16", splits)
    assert tuple(a.shape) == (bs, 1, Hq, 128) and torch.isfinite(a.float()).all()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert bool((a[[i for i, l in enumerate(lens) if l == 0]] == 0).all())


@pytest.mark.parametrize("splits", [17, 33])
def test_decode_merges_16k_plus_1_splits(splits):
    c = decode_case(4, 32, 8, (6, 301, 0, 1001), 64)
    assert torch.equal(run(c, "fp8", splits).view(torch.int16), run(c, "bf16", splits).view(torch.int16))


def test_decode_partials_are_bit_identical_too():
    bs, Hq, S = 4, 32, 5
    c = decode_case(bs, Hq, 8, (6, 301, 0, 1001), 64)
    (a, wa), (b, wb) = run(c, "fp8", S, partials=True), run(c, "bf16", S, partials=True)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(wa, wb)  # part_o and part_lse, byte for byte (rows of empty splits are not written: zeroed above)
    lse = wa.view(torch.float32)[bs * Hq * S * 128 :].view(bs, Hq, S)
    # the empty sequence: -inf everywhere; the 6-token one: one live split of five; the 1001-token one: all five live
    assert bool(torch.isinf(lse[2]).all()) and bool((torch.isfinite(lse[0]).sum(-1) == 1).all()) and bool(torch.isfinite(lse[3]).all())
    assert float(wa.view(torch.float32)[: bs * Hq * S * 128].abs().max()) > 0


def test_decode_does_not_depend_on_bytes_past_the_length():
    """every byte past each sequence's length, unused pages included, set to 0xFF: NaN codes, NaN scales, pad bytes"""
    bs, Hq, Hkv, lens, page = 4, 32, 8, (6, 301, 0, 1001), 64
    c = decode_case(bs, Hq, Hkv, lens, page)
    table = c["cpu"]["table"]
    dead = torch.ones(c["cpu"]["k8"].shape[:2], dtype=torch.bool)
    for b, L in enumerate(lens):
        for t in range(L):
            dead[int(table[b, t // page]), t % page] = False
    assert int(dead.sum()) > 0
    k8, v8 = c["cpu"]["k8"].clone(), c["cpu"]["v8"].clone()
    k8[dead], v8[dead] = 0xFF, 0xFF
    for splits in (1, 4, None):
        a = run(c, "fp8", splits, k8=k8.cuda(), v8=v8.cuda())
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a.view(torch.int16), run(c, "fp8", splits).view(torch.int16))


def test_decode_against_fp32_attention_over_the_dequantised_rows():
    """the one absolute anchor: everything above compares two GPU kernels"""
    bs, Hq, Hkv, lens, page = 3, 16, 8, (40, 129, 300), 64
    c = decode_case(bs, Hq, Hkv, lens, page, seed=9)
    cpu = c["cpu"]
    ref, _, _ = ogqa.attn_with_kvcache(cpu["q"], dequant_ref(cpu["k8"]), dequant_ref(cpu["v8"]), None, None, list(lens), cpu["table"])
    for splits in (1, None):
        assert_close(run(c, "fp8", splits).cpu(), ref, 1e-2, what=splits)


def test_attn_with_kvcache_appends_quantised_rows_and_attends_over_them():
    from chitu_amd import ops
    from chitu_amd.attn_backend import HipAttnBackend

    bs, Hq, Hkv, lens, page = 3, 32, 8, (15, 16, 300), 16
    c = decode_case(bs, Hq, Hkv, tuple(l + 1 for l in lens), page, seed=4)  # pages for the appended token too
    g = torch.Generator().manual_seed(11)
    k, v = rows_with_edges(bs, Hkv, seed=5), (torch.randn(bs, Hkv, 128, generator=g) * 3).to(torch.bfloat16)
    sl = torch.tensor(lens, dtype=torch.int32).cuda()
    k8, v8 = c["k8"].clone(), c["v8"].clone()
    be = HipAttnBackend(local_n_heads=Hq)
    out = be.attn_with_kvcache(c["q"], k8, v8, k.cuda().unsqueeze(1), v.cuda().unsqueeze(1), cache_seqlens=sl, block_table=c["table"])
    want_k, want_v = c["cpu"]["k8"].clone(), c["cpu"]["v8"].clone()
    for b, L in enumerate(lens):
        p = int(c["cpu"]["table"][b, L // page])
        want_k[p, L % page], want_v[p, L % page] = quant_ref(k)[b], quant_ref(v)[b]
    assert torch.equal(k8.cpu(), want_k) and torch.equal(v8.cpu(), want_v)
    ref = be.attn_with_kvcache(c["q"], ops.gqa_kv_dequant_fp8(k8), ops.gqa_kv_dequant_fp8(v8), cache_seqlens=sl + 1, block_table=c["table"])
    assert tuple(out.shape) == (bs, 1, Hq, 128) and torch.equal(out.view(torch.int16), ref.view(torch.int16))


# ---------------------------------------------------------------- 5. the models
def llama_args(n_kv_heads, **kw):
    from chitu_amd.llama import LlamaArgs

    return LlamaArgs(dim=1024, n_layers=3, n_heads=8, n_kv_heads=n_kv_heads, vocab_size=2048, ffn_dim=2048, **kw)  # test_gpu_llama.py::tiny_args


def mixtral_args(**kw):
    from chitu_amd.mixtral import MixtralArgs

    return MixtralArgs(dim=1024, n_layers=2, n_heads=8, n_kv_heads=2, vocab_size=2048, ffn_dim=512, num_local_experts=8,
                       num_experts_per_tok=2, **kw)  # test_gpu_mixtral.py::build


def build(args, cache_format=None, max_reqs=4, max_seq=1024, page=256):
    from chitu_amd import llama, mixtral
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, gqa_kv_layout

    mod = mixtral if isinstance(args, mixtral.MixtralArgs) else llama
    shape, dtype = gqa_kv_layout(cache_format or args.kv_cache_dtype, args.n_kv_heads)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=max_reqs, block_size=page, max_seq_len=max_seq, device="cuda",
                                k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype)
    decoder = mod.MixtralDecoder if mod is mixtral else mod.LlamaDecoder
    model = decoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=max_seq), max_position_embeddings=max_seq,
                    device="cuda")
    mod.init_synthetic_(model, seed=0)
    return model, cache


PROMPTS = [[(13 * i + 1) % 2048 for i in range(70)], [(7 * i + 3) % 2048 for i in range(5)], [(29 * i + 11) % 2048 for i in range(255)]]
STEP_TOKENS = [[5, 900, 17], [321, 4, 77], [1000, 1001, 2], [64, 65, 66]]
REQS = ["a", "b", "c"]


def run_model(args, bs):
    """ragged prefill of `bs` prompts (the third one ends one row short of its page: the decode steps fill it and open the next), then four decode
    steps with fixed input tokens, every step eagerly AND through its verified graph from the same cache bytes"""
    model, cache = build(args)
    reqs = REQS[:bs]
    logits = [model.prefill(PROMPTS[:bs], reqs).cpu()]
    graph_equal = []
    for toks in STEP_TOKENS:
        tok = torch.tensor(toks[:bs], dtype=torch.int64, device="cuda")
        cache.prepare_cache_decode(reqs)
        cache.prepare_block_table_for_decode(reqs)
        snap_k, snap_v = cache.paged_k_cache.clone(), cache.paged_v_cache.clone()
        eager = model.decode(tok, use_graph=False).clone()
        kv_eager = cache.paged_k_cache.clone(), cache.paged_v_cache.clone()
        cache.paged_k_cache.copy_(snap_k)
        cache.paged_v_cache.copy_(snap_v)
        replay = model.decode(tok, use_graph=True)
        graph_equal.append(torch.equal(eager, replay) and torch.equal(kv_eager[0], cache.paged_k_cache)
                           and torch.equal(kv_eager[1], cache.paged_v_cache) and not torch.equal(snap_k, cache.paged_k_cache))
        cache.finalize_cache_single_decode(reqs)
        logits.append(eager.cpu())
    rows = []
    for c in cache.get_paged_kv_cache(0):  # layer 0's cached K and V rows of every request, in token order
        rows.append(torch.cat([torch.cat([c[blk] for blk in cache.block_table[r]])[: cache.seq_lens[r]].cpu() for r in reqs]))
    return dict(logits=torch.stack(logits), graph_equal=graph_equal, rows=rows)


# (n_kv_heads, batch): LlamaDecoder rotates interleaved pairs ("llama").  Batch 3 is above llama.FUSE_NORM_MAX_BS: the unfused
# layer (add + norm, projection, gqa_qkv_post_kv_fp8).  Batch 1 is where a bf16 cache takes bf16_linear_add_norm_qkv_post, whose
# epilogue writes bf16 rows: the fp8 model must take bf16_linear_add_norm + gqa_qkv_post_kv_fp8 there (the bf16 twin does fuse).
@pytest.fixture(scope="module", params=[(2, 3), (8, 1)], ids=["gqa4_bs3", "mha_bs1"])
def llama_runs(request):
    n_kv, bs = request.param
    return {fmt: run_model(llama_args(n_kv, kv_cache_dtype=fmt), bs) for fmt in ("bf16", "fp8")}, bs


def test_llama_graph_step_equals_eager_step_in_fp8_mode(llama_runs):
    runs, _ = llama_runs
    assert all(runs["fp8"]["graph_equal"]) and len(runs["fp8"]["graph_equal"]) >= 3, runs["fp8"]["graph_equal"]


def test_llama_layer0_rows_are_the_quantised_rows_of_the_bf16_cache_model(llama_runs):
    """layer 0's rows depend on the tokens only: prefill rows (quantised on their way into the pages) and the rows of the four
    decode steps (RoPE + append with quantising stores) hold the quantiser's bytes of what a bf16 cache holds"""
    runs, bs = llama_runs
    n = sum(len(p) for p in PROMPTS[:bs]) + bs * len(STEP_TOKENS)
    for got, twin in zip(runs["fp8"]["rows"], runs["bf16"]["rows"]):
        assert got.dtype == torch.uint8 and tuple(got.shape[::2]) == (n, ROW) and twin.dtype == torch.bfloat16
        assert torch.equal(got, quant_ref(twin))


# max_rel_to_peak of the fp8-cache model's logits against the bf16-cache model's over 4 decode steps, measured on an MI355X.  The bar is
# twice the measurement (the margin of tests/test_gpu_mla_kv_fp8.py, for its reason: one flipped fp8 code in a cached row moves this
# tiny random model visibly).
MEASURED_LOGIT_ERR = {"gqa4_bs3": 0.023682, "mha_bs1": 0.013327}


def test_llama_logits_stay_close_to_the_bf16_cache_model(llama_runs, request):
    runs, _ = llama_runs
    a, b = runs["fp8"]["logits"], runs["bf16"]["logits"]
    assert torch.equal(a[0], b[0])  # the prompt's own attention reads the unquantised rows
    err = max_rel_to_peak(a[1:], b[1:])
    key = request.node.callspec.id
    print(f"fp8 KV cache vs bf16 KV cache, logits max_rel_to_peak [{key}]: {err:.6f}")
    assert err > 0  # the quantised cache is really read
    assert torch.isfinite(a).all()
    assert err < 2 * MEASURED_LOGIT_ERR[key], err


def test_model_cache_and_args_must_agree():
    with pytest.raises(ValueError, match="gqa_kv_layout"):
        build(llama_args(2, kv_cache_dtype="fp8"), cache_format="bf16")
    with pytest.raises(ValueError, match="gqa_kv_layout"):
        build(llama_args(2), cache_format="fp8")
    with pytest.raises(ValueError):
        build(llama_args(2, kv_cache_dtype="fp4"), cache_format="bf16")


def test_llama_generate_in_fp8_mode():
    model, cache = build(llama_args(2, kv_cache_dtype="fp8"))
    free = len(cache.free_blocks)
    out = model.generate(PROMPTS[:2], 5)
    assert tuple(out.shape) == (2, 5) and out.dtype == torch.int64 and int(out.min()) >= 0 and int(out.max()) < 2048
    assert len(cache.free_blocks) == free


def test_mixtral_graph_step_equals_eager_step_in_fp8_mode():
    """MixtralBlock rotates half-split pairs ("hf-llama") and reaches LlamaAttention.decode_from_residual at batch 2"""
    r = run_model(mixtral_args(kv_cache_dtype="fp8"), 2)
    assert all(r["graph_equal"]), r["graph_equal"]
    assert torch.isfinite(r["logits"]).all() and r["rows"][0].dtype == torch.uint8
