"""The page-addressing launches listed in the test names below, at pages more than 2^32 bytes into their allocation, and the two
step drivers (tiny Llama, tiny DeepSeek-V3) on a manager that hands out such pages (tests/big_cache.py: the layout, the
cases, the CPU oracles; tests/test_big_cache_host.py shows on the CPU that a kernel which cut an offset to 32 bits fails these
assertions).  One allocation per cache format and module; only the named, low and guard pages are ever written.  Every test
asserts (a) the closed-form or bit-exact expectation at the existing bars, (b) bit identity with the same call on the same rows at
low page ids of the same allocation, (c) that the guard pages -- page 0 and the 32-bit alias of every named page -- and every row
the call does not address are unchanged.  The embedding gather and the LM-head GEMM read a 4 GiB table on both sides of 2^31 and
2^32 bytes.  Each test prints its worst error and the highest byte offset it addressed ("BIG_CACHE ...", pytest -s)."""
import pytest
import torch

from tests import attn_exact as ax
from tests import big_cache as bc
from tests import dense_exact as dx
from tests import row_exact as rx
from tests import test_gqa_kv_fp8_host as g8
from tests import test_mla_kv_fp8_host as m8

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SLOTS = {"gqa": 48, "mla": 24}


def report(what, err, top):
    print(f"BIG_CACHE kernel {what}: {err:.3e}; highest byte offset addressed 2^32 + {top - 2 ** 32}")


def same(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---------------------------------------------------------------- one allocation per cache format
def allocation(fam, fp8):
    if fam == "gqa":
        shape, n_caches = (bc.GQA_PAGE, bc.GQA_HKV, g8.ROW if fp8 else 128), 2
    else:
        shape, n_caches = (bc.MLA_PAGE, m8.ROW if fp8 else 576), 1
    pb = (1 if fp8 else 2) * int(torch.tensor(shape).prod())
    named, _, _ = bc.high_layout(pb, SLOTS[fam])
    pages = named[-1] + 1
    bc.need_free(n_caches * pages * pb)
    caches = None
    try:
        caches = [torch.empty(pages, *shape, dtype=torch.uint8 if fp8 else BF16, device="cuda") for _ in range(n_caches)]
        assert named[0] * pb > 2 ** 32
        yield caches
    finally:
        del caches
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def gqa_bf16():
    yield from allocation("gqa", False)


@pytest.fixture(scope="module")
def gqa_fp8():
    yield from allocation("gqa", True)


@pytest.fixture(scope="module")
def mla_bf16():
    yield from allocation("mla", False)


@pytest.fixture(scope="module")
def mla_fp8():
    yield from allocation("mla", True)


def sentinels_of(fam, caches):
    fp8 = caches[0].dtype == torch.uint8
    hkv = caches[0].shape[2] if fam == "gqa" else None
    return [bc.sentinel_page(fam, fp8, caches[0].shape[1], f, hkv) for f in (bc.FILLS_GQA if fam == "gqa" else bc.FILLS_MLA)]


# ---------------------------------------------------------------- readers
def backend(H):
    from chitu_amd.attn_backend import HipAttnBackend

    return HipAttnBackend(local_n_heads=H)


def i32(values):
    return torch.tensor(list(values), dtype=torch.int32).cuda()


def gpu_run(case, caches, table, splits):
    """the case through the project's entry; the rows in the order of big_cache.oracle_run"""
    from chitu_amd import ops

    table = table.cuda()
    if case["entry"] == "decode":
        q = case["q"].cuda()
        out = backend(q.shape[2]).attn_with_kvcache(q, caches[0], caches[1], cache_seqlens=i32(case["totals"]), block_table=table,
                                                    softmax_scale=ax.GQA_SCALE, causal=True, window_size=(case["W"], 0), num_splits=splits)
        return out.reshape(-1, *q.shape[2:])
    if case["entry"] == "prefill":
        q = case["q"].to(BF16).cuda()
        window = (case["W"], 0) if case["W"] >= 0 else (-1, -1)
        return backend(q.shape[1]).attn_varlen_with_kvcache(q, caches[0], caches[1], i32(ax.cu_of(case["news"])), i32(case["totals"]), table,
                                                            max(case["news"]), causal=True, window_size=window, softmax_scale=ax.GQA_SCALE)
    if case["entry"] == "mla_multi":
        qn, qp = case["q_nope"].cuda(), case["q_pe"].cuda()
        out = backend(qn.shape[2]).mla_decode_multi(qn, qp, caches[0], i32(case["totals"]), table, ax.MLA_SCALE, num_splits=splits, kernel="multi")
        return out.reshape(-1, *qn.shape[2:])
    assert case["entry"] == "gather"
    cu = ax.cu_of(case["totals"])
    return ops.mla_kv_gather(caches[0], table, i32(cu), cu[-1])


def readers(fam, caches, cases, tag):
    """(a), (b) and (c) for every case at splits 1 and 3 (where the entry takes splits)"""
    fp8 = caches[0].dtype == torch.uint8
    page, pb = caches[0].shape[1], bc.page_bytes_of(caches[0])
    n = bc.assign_slots(cases, page)
    assert n <= SLOTS[fam]
    named, _, guard = bc.high_layout(pb, n)
    low = bc.low_pages(pb, n)
    assert named[-1] < caches[0].shape[0]
    touch = sorted(set(named) | set(low) | set(guard))
    bc.fill_pages(caches, sentinels_of(fam, caches), touch)
    for c in cases:
        for ids in (named, low):
            bc.place_case(caches, c, ids, bc.quant_of(fam, fp8))
    before = [c[touch].clone() for c in caches]
    for c in cases:
        def table(ids):
            return bc.gather_table(c, ids, caches[0].shape[0]) if c["entry"] == "gather" else bc.table_of(c, ids)

        top = max(int(p) for p in table(named).flatten() if p < caches[0].shape[0]) * pb + pb
        assert top > 2 ** 32
        for s in (bc.SPLITS if c["entry"] in ("decode", "mla_multi") else [None]):
            high, lo = gpu_run(c, caches, table(named), s), gpu_run(c, caches, table(low), s)
            report(f"{tag} {c['name']} splits={s}", bc.check(c, high, fp8), top)
            assert same(high, lo), f"{tag} {c['name']} splits={s}: the result depends on the page ids"
    for c, b in zip(caches, before):
        assert torch.equal(c[touch], b), f"{tag}: a reader changed a page"


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_gqa_multi_token_and_window_decode_beyond_4gib(fmt, request):
    """gqa_decode_multi / _kv_fp8 at T in {2, 8} and gqa_decode_window / _kv_fp8_window (through attn_with_kvcache)"""
    caches = request.getfixturevalue("gqa_" + fmt)
    readers("gqa", caches, [c for c in bc.gqa_reader_cases() if c["entry"] == "decode"], f"gqa decode {fmt}")


def test_gqa_paged_prefill_beyond_4gib(gqa_bf16):
    """gqa_prefill_paged: counting, windowed counting and dominant keys behind prefixes in high pages"""
    readers("gqa", gqa_bf16, [c for c in bc.gqa_reader_cases() if c["entry"] == "prefill"], "gqa prefill paged")


def test_gqa_paged_prefill_any_group_beyond_4gib(gqa_bf16):
    """the any-group entry (Hq, Hkv = 6, 2): the same allocation seen as pages of two KV heads"""
    views = [c.view(-1, bc.GQA_PAGE, bc.ANY_HKV, 128) for c in gqa_bf16]
    readers("gqa", views, bc.gqa_reader_cases(bc.ANY_HQ, bc.ANY_HKV, prefill_only=True), "gqa prefill paged any group")


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_mla_multi_token_decode_and_gather_beyond_4gib(fmt, request):
    """mla_decode_multi / _kv_fp8 at T in {2, 8}; mla_kv_gather against the indexed rows, one table entry >= num_pages"""
    readers("mla", request.getfixturevalue("mla_" + fmt), bc.mla_reader_cases(), f"mla {fmt}")


# ---------------------------------------------------------------- writers
def match(got, want, what):
    """got equals want bit for bit; want = big_cache.cand([C, ...]): every head (the last-but-one dimension; a row of the MLA
    cache, or of a 2-d output, counts as one head) equals one of the C candidates as a whole"""
    if not isinstance(want, tuple):
        assert same(got, want), what
        return
    want = want[1]
    g = got.cpu().contiguous().view(torch.uint8).flatten(0, -2)
    w = want.contiguous().view(torch.uint8).flatten(1, -2)
    hit = (g[None] == w).all(-1).any(0)
    assert bool(hit.all()), f"{what}: {int((~hit).sum())} heads equal no candidate"


def writer(fam, caches, name, T, call, want_rows, want_aux):
    """call(caches, table [bs, 2], old lengths [3]) -> aux tensors.  (c) exactly the addressed rows of the named pages changed and
    no guard page; (b) those rows and the aux outputs are the same bits at high and at low pages; (a) they are want_*."""
    page, pb = caches[0].shape[1], bc.page_bytes_of(caches[0])
    named, _, guard = bc.high_layout(pb, 6)
    sentinels = sentinels_of(fam, caches)
    old, positions = bc.writer_positions(page, T)
    got = {}
    for tag, ids in (("high", named), ("low", bc.low_pages(pb, 6))):
        touch = sorted(set(ids) | set(guard))
        bc.fill_pages(caches, sentinels, touch)
        aux = call(caches, bc.writer_table(ids).cuda(), i32(old))
        torch.cuda.synchronize()
        rows = []
        for cache, s in zip(caches, sentinels):
            g = cache[touch].cpu()
            w = s.unsqueeze(0).repeat(len(touch), *[1] * s.dim())
            new = []
            for b, pos in positions:
                at = touch.index(ids[bc.WRITER_SLOTS[b][pos // page]]), pos % page
                assert not torch.equal(g[at], s[pos % page]), f"{name} at {tag} pages: an addressed row still holds the decoy"
                new.append(g[at].clone())
                w[at] = g[at]
            assert torch.equal(g, w), f"{name} at {tag} pages: a guard page or a row that is not addressed changed"
            rows.append(torch.stack(new))
        got[tag] = rows + [a.cpu() for a in aux]
    for h, lo in zip(got["high"], got["low"]):
        assert same(h, lo), f"{name}: the rows written depend on the page ids"
    for g, w in zip(got["high"], list(want_rows) + list(want_aux)):
        match(g, w, name)
    top = max(named[k] for row in bc.WRITER_SLOTS for k in row) * pb + pb
    assert top > 2 ** 32
    report(name, 0.0, top)


def dev(v):
    return v.cuda() if isinstance(v, torch.Tensor) else v


def gqa_call(c, fp8):
    """the launch of a big_cache.gqa_writer_cases entry: -> the outputs that want_aux names"""
    from chitu_amd import ops

    if c["entry"] == "bf16_linear_add_norm_qkv_post":
        def call(caches, table, lens):
            x_new, qkv = ops.bf16_linear_add_norm_qkv_post(dev(c["x"]), dev(c["add"]), dev(c["w"]), c["eps"], dev(c["wqkv"]), bc.GQA_HQ, bc.GQA_HKV,
                                                           dev(c["cos"]), dev(c["sin"]), caches[0], caches[1], table, lens)
            return [x_new, qkv[:, : bc.GQA_HQ].clone()]
        return call

    def call(caches, table, lens):
        f = getattr(ops, c["entry"] + ("_kv_fp8" if fp8 else ""))
        return [f(dev(c["x"]), bc.GQA_HQ, bc.GQA_HKV, dev(c["cos"]), dev(c["sin"]), caches[0], caches[1], table, lens,
                  *[dev(e) for e in c["extra"]], **c["kw"]).clone()]
    return call


def mla_call(c):
    """the launch of a big_cache.mla_writer_cases entry"""
    from chitu_amd import ops

    def call(caches, table, lens):
        cos, sin, kv_w, cache = dev(c["cos"]), dev(c["sin"]), dev(c["kv_w"]), caches[0]
        if c["kind"] == "kv_prep":
            q = dev(c["q_pe"])
            ops.mla_kv_prep(dev(c["row"]), q, cos, sin, kv_w, rx.EPS, cache, table, lens)
            return [q]
        if c["kind"] == "qkv_post":
            q, s = ops.mla_qkv_post(dev(c["row"]), c["q_lora"], dev(c["q_w"]), rx.EPS, kv_w, rx.EPS, cos, sin, cache, table, lens)
            return [torch.cat([q.view(torch.uint8), s.contiguous().view(torch.uint8).view(q.shape[0], -1)], 1)]
        if c["kind"] == "q_proj":
            assert ops.mla_q_proj_fits(c["row"].shape[0], c["rank"])
            return [ops.mla_q_proj(dev(c["row"]), c["rank"], dev(c["q_w"]), c["q_eps"], dev(c["wq"]), dev(c["ws"]), kv_w, rx.EPS, cos, sin, cache,
                                   table, lens, out_dtype=torch.float32)]
        assert c["kind"] == "absorb"
        a, B = c["c"], c["row"].shape[0]
        sh, sn, sk = a["strides"]
        w_dev = dev(a["w_store"])
        w3 = torch.as_strided(w_dev, (c["H"], c["N"], c["K"]), (w_dev.stride(0), c["K"], 1))
        q = dev(c["q"])
        out = ops.absorb_bmm_rope_kv_fp8(dev(a["x"]), w3, dev(a["scale"]), dx.ABSORB_OFFSET, sh, sn, sk, q[dx.G : dx.G + B], cos, sin, dev(c["row"]),
                                         kv_w, rx.EPS, cache, table, lens)
        return [out, q]
    return call


def expanded(table, lens, T):
    """the table rows and positions of T new rows per sequence, (b, t) order: what attn_with_kvcache hands the append kernels"""
    return table.repeat_interleave(T, dim=0).contiguous(), (lens.view(-1, 1) + torch.arange(T, dtype=torch.int32, device=lens.device)).view(-1)


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_gqa_writers_beyond_4gib(fmt, request):
    """gqa_qkv_post (both rotary layouts), gqa_qkv_norm_post, gqa_qkv_bias_post, the GLM-4 rotary type, bf16 pages only:
    bf16_linear_add_norm_qkv_post; and three new rows per sequence through the append kernels (one sequence's rows across a
    page edge) -- into bf16 and fp8 pages"""
    from chitu_amd import ops

    caches, fp8 = request.getfixturevalue("gqa_" + fmt), fmt == "fp8"
    for c in bc.gqa_writer_cases(fp8):
        writer("gqa", caches, c["name"], 1, gqa_call(c, fp8), c["want_rows"], c["want_aux"])
    T = 3
    g = torch.Generator().manual_seed(9)
    new = [(torch.randn(3 * T, bc.GQA_HKV, 128, generator=g) * 3).to(BF16) for _ in range(2)]

    def append(caches, table, lens):
        t, pos = expanded(table, lens, T)
        if fp8:
            ops.append_gqa_kv_fp8(caches[0], caches[1], t, new[0].cuda(), new[1].cuda(), pos)
        else:
            for cache, rows in zip(caches, new):
                ops.append_to_paged_kv_cache(cache, t, rows.cuda(), pos)
        return []

    writer("gqa", caches, f"append, 3 rows per sequence, {fmt}", T, append, [g8.quant_ref(r) if fp8 else r for r in new], [])


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_mla_appends_beyond_4gib(fmt, request):
    """three new rows per sequence through append_to_paged_kv_cache / append_mla_kv_fp8"""
    from chitu_amd import ops

    caches, fp8 = request.getfixturevalue("mla_" + fmt), fmt == "fp8"
    T = 3
    new = torch.randn(3 * T, 576, generator=torch.Generator().manual_seed(4)).to(BF16)

    def append(caches, table, lens):
        t, pos = expanded(table, lens, T)
        if fp8:
            ops.append_mla_kv_fp8(caches[0], t, new.cuda().view(-1, 1, 576), pos)
        else:
            ops.append_to_paged_kv_cache(caches[0], t, new.cuda().view(-1, 1, 576), pos)
        return []

    writer("mla", caches, f"mla append, 3 rows per sequence, {fmt}", T, append, [m8.quant_ref(new) if fp8 else new], [])


def test_mla_single_token_writers_beyond_4gib(mla_bf16):
    """mla_kv_prep, mla_qkv_post, mla_q_proj and absorb_bmm_rope_kv_fp8 append into pages past 2^32 bytes"""
    for c in bc.mla_writer_cases():
        writer("mla", mla_bf16, c["name"], 1, mla_call(c), c["want_rows"], c["want_aux"])


# ---------------------------------------------------------------- the step drivers on a manager that hands out high pages
def driver_logits(model, cache, prompts, first_page):
    """prefill, two decode steps, one two-token step and one continued prefill, eagerly, with the manager's free list
    starting at first_page; -> (every step's logits, the page ids the requests held at the end).  Leaves the cache empty."""
    from collections import deque

    reqs = [f"r{i}" for i in range(len(prompts))]
    cache.free_blocks = deque(range(cache.num_blocks))
    cache.free_blocks.rotate(-first_page)
    vocab = model.args.vocab_size
    g = torch.Generator().manual_seed(11)
    out = [model.prefill(prompts, reqs).clone()]
    for _ in range(2):
        cache.prepare_cache_decode(reqs)
        cache.prepare_block_table_for_decode(reqs)
        out.append(model.decode(torch.randint(0, vocab, (len(reqs),), generator=g).cuda(), use_graph=False).clone())
        cache.finalize_cache_single_decode(reqs)
    cache.prepare_block_table_for_decode_multi(reqs, 2)
    out.append(model.decode_multi(torch.randint(0, vocab, (len(reqs), 2), generator=g).cuda(), use_graph=False).clone())
    cache.finalize_cache_multi_decode(reqs, [2] * len(reqs))
    out.append(model.prefill_continue([torch.randint(0, vocab, (n,), generator=g).tolist() for n in (3, 1, 7)], reqs).clone())
    pages = sorted(p for r in reqs for p in cache.block_table[r])
    for r in reqs:
        cache.finalize_cache_all_decode(r)
    return out, pages


def driver_check(model, cache, layer_cache, prompts, what):
    pb = layer_cache[0].numel() * layer_cache.element_size()
    first = bc.first_page_beyond_4gib(pb)
    assert first + 64 < cache.num_blocks
    high, pages = driver_logits(model, cache, prompts, first)
    assert min(pages) >= first and min(pages) * pb > 2 ** 32, "the manager did not hand out pages past 2^32 bytes"
    low, low_pages = driver_logits(model, cache, prompts, 0)
    assert max(low_pages) < 64 and len(low_pages) == len(pages)
    for step, (h, lo) in enumerate(zip(high, low)):
        assert bool(torch.isfinite(h).all()) and same(h, lo), f"{what}: the logits of step {step} depend on the page ids"
    report(f"{what} driver: prefill, 2 decodes, a 2-token step, a continued prefill", 0.0, (max(pages) + 1) * pb)


def test_llama_step_driver_on_pages_beyond_4gib():
    """tests/test_gpu_llama_multi.py's tiny Llama (bf16 cache) with enough pages for ids past 4 GiB per layer tensor: every
    step's logits are bit-identical to the same schedule on low pages -- the driver against itself, so that a page-touching
    launch no test above lists is covered too"""
    from tests.test_gpu_llama import build, tiny_args
    from tests.test_gpu_llama_multi import prompts_of

    args = tiny_args()
    pb = 256 * args.n_kv_heads * args.head_dim * 2
    reqs = -(-(bc.first_page_beyond_4gib(pb) + 80) // 5)  # five pages per request slot at max_seq 1024
    bc.need_free(2 * args.n_layers * reqs * 5 * pb)
    model = cache = None
    try:
        model, cache = build(args, max_reqs=reqs)
        driver_check(model, cache, cache.paged_k_cache[0], prompts_of(args.vocab_size), "llama")
    finally:
        del model, cache
        torch.cuda.empty_cache()


def test_deepseek_v3_step_driver_on_pages_beyond_4gib():
    """tests/test_gpu_deepseek_multi.py's tiny DeepSeek-V3 with a bf16 latent cache, as above"""
    from tests.test_gpu_deepseek_multi import build_variant, prompts_of

    pb = 64 * 576 * 2
    reqs = -(-(bc.first_page_beyond_4gib(pb) + 80) // 9)  # nine pages per request slot at max_seq 512
    model = cache = None
    try:
        from tests.test_gpu_deepseek import tiny_args

        bc.need_free(tiny_args().n_layers * reqs * 9 * pb)
        model, cache = build_variant("v3_like", "bf16", max_reqs=reqs)
        driver_check(model, cache, cache.paged_kv_cache[0], prompts_of(model.args.vocab_size), "deepseek-v3")
    finally:
        del model, cache
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- embedding gather and LM head past 2^31 and 2^32 bytes
def test_embedding_gather_and_lm_head_on_both_sides_of_2gib_and_4gib():
    """a bf16 table of 262 400 rows of 8192 (row 131 072 starts at 2^31 bytes, row 262 144 at 2^32): embed_rope_gather returns the
    indexed rows bit for bit, an id outside the shard a zero row; as a bf16_linear weight the probed rows' output columns are
    the exact integer products and every other column is exactly 0"""
    from chitu_amd import ops

    rows, dim = 262400, 8192
    bc.need_free(rows * dim * 2)
    table = None
    try:
        table = torch.empty(rows, dim, dtype=BF16, device="cuda")
        probed = [131071, 131072, 262143, 262144, rows - 1]
        assert probed[1] * dim * 2 == 2 ** 31 and probed[3] * dim * 2 == 2 ** 32
        alias = sorted({(r * dim * 2 % 2 ** 32) // (dim * 2) for r in probed if r * dim * 2 >= 2 ** 32} | {0})
        g = torch.Generator().manual_seed(1)
        want = torch.randn(len(probed), dim, generator=g).to(BF16)
        table[alias] = torch.full((len(alias), dim), ax.K_AMP, dtype=BF16).cuda()  # what a cut offset would read
        table[probed] = want.cuda()
        start = 1000
        ids = torch.tensor([start + r for r in probed] + [start - 1, start + rows], dtype=torch.int64)
        h, _, _ = ops.embed_rope_gather(ids.cuda(), table, start)
        assert same(h[: len(probed)], want), "embed_rope_gather: not the indexed rows"
        assert not bool(h[len(probed) :].any()), "embed_rope_gather: an id outside the shard gives a zero row"
        table.zero_()
        w = dx.ints(g, 4, len(probed), dim)
        table[probed] = w.to(BF16).cuda()
        for M in (1, 3):
            x = dx.ints(g, 4, M, dim)
            exact = x.double() @ w.double().T
            assert float(exact.abs().max()) < 2 ** 24
            out = ops.bf16_linear(x.to(BF16).cuda(), table)
            assert same(out[:, probed], dx.expect(exact, BF16)), f"bf16_linear M={M}: the probed rows' columns"
            out[:, probed] = 0
            assert not bool(out.any()), f"bf16_linear M={M}: a column of a zero weight row is not 0"
        report("embedding gather and LM head", 0.0, rows * dim * 2)
    finally:
        del table
        torch.cuda.empty_cache()
