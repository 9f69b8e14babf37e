"""Exact per-key tests of the six attention kernels (GQA decode, MLA decode, their fp8-cache twins, GQA and MLA flash prefill)
over every length, split count and page size: the constructions of tests/attn_exact.py, whose expected values are closed forms
(and the fp64 attention there), never a kernel's output.  tests/test_attn_exact_host.py shows on the CPU that the oracles meet
every bound asserted here.  Each test prints its worst error ("ATTN_EXACT ...", pytest -s).

Decode reads only: all batch rows of a launch use the same block-table row over one small cache of shuffled pages and differ
in cache_seqlens (counting: batch row = length, one launch is a whole length sweep) or in q (probes)."""
import math

import pytest
import torch

from oracle import mla as omla
from tests import attn_exact as ax
from tests import test_gqa_kv_fp8_host as g8
from tests import test_mla_kv_fp8_host as m8
from tests.util import assert_close

pytestmark = pytest.mark.gpu

GQA_HEADS = [(4, 4), (8, 2), (16, 1)]
GQA_PAGES = [16, 48, 256]            # a new page on every step; not a power of two; the usual one
GQA_SPLITS = [1, 2, 3, 5, 8, 17, None]  # 17: more splits than steps at 130 keys, and the merge kernel's 16 k + 1 case
MLA_PAGES = [64, 128, 192]           # mla_decode_check_args takes every multiple of the 64-key tile
MLA_SPLITS = [1, 2, 3, 4, 5, 7, None]
MLA_HEADS = [16, 32, 5]


def report(what, err):
    print(f"ATTN_EXACT kernel {what}: {err:.3e}")


def backend(H):
    from chitu_amd.attn_backend import HipAttnBackend

    return HipAttnBackend(local_n_heads=H)


def real(splits):
    return [s for s in splits if s is not None]


# ---------------------------------------------------------------- GQA decode
def gqa_device(case, page, fp8=False):
    """(q, k_cache, v_cache, lens, table) on the GPU; fp8: the caches quantised by the project's quantiser, which must give the rows back"""
    from chitu_amd import ops

    kc, vc, table = ax.gqa_pages(case, page, seed=page)
    kd, vd = kc.cuda(), vc.cuda()
    if fp8:
        shape = kc.shape
        k8, v8 = (ops.gqa_kv_quant_fp8(c.view(-1, shape[2], 128)).view(*shape[:3], g8.ROW) for c in (kd, vd))
        for c8, c in ((k8, kd), (v8, vd)):
            assert torch.equal(ops.gqa_kv_dequant_fp8(c8).view(torch.int16), c.view(torch.int16))
        assert torch.equal(k8.cpu().view(-1, shape[2], g8.ROW), g8.quant_ref(kc.view(-1, shape[2], 128)))
        kd, vd = k8, v8
    return case["q"].cuda(), kd, vd, case["lens"].cuda(), table.cuda()


def gqa_run(dev, splits):
    q, kd, vd, lens, table = dev
    out = backend(q.shape[2]).attn_with_kvcache(q, kd, vd, cache_seqlens=lens, block_table=table, softmax_scale=ax.GQA_SCALE, num_splits=splits)
    return out[:, 0]


@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
@pytest.mark.parametrize("page", GQA_PAGES)
def test_gqa_decode_counts_every_key_once_at_every_length(page, Hq, Hkv):
    """lengths 0 .. 130 (eight 16-key steps plus 2) in one launch per split count"""
    c = ax.gqa_count_case(130, Hq, Hkv)
    dev = gqa_device(c, page)
    worst = max(ax.check_count(gqa_run(dev, s), c["want"]) for s in GQA_SPLITS)
    report(f"gqa decode counting page={page} Hq={Hq} Hkv={Hkv}, relative", worst)


@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
@pytest.mark.parametrize("n", [17, 64, 130])
def test_gqa_decode_returns_the_probed_keys_row(n, Hq, Hkv):
    """keys 0 and n - 1 and both sides of every step, page and split edge, one probe per head of a group"""
    worst = 0.0
    for page in GQA_PAGES:
        c = ax.gqa_dominant_case(n, Hq, Hkv, ax.probe_tokens(n, ax.STEP_GQA, page, real(GQA_SPLITS)))
        dev = gqa_device(c, page)
        worst = max([worst] + [ax.check_dominant(gqa_run(dev, s), c["want"]) for s in GQA_SPLITS])
    report(f"gqa decode dominant key n={n} Hq={Hq} Hkv={Hkv}, absolute", worst)


def test_gqa_decode_on_both_sides_of_the_deferral_constant():
    """A key that leads by just under kGqaDefer nats (large p, no rescale) and by just over it (rescale), in the first step and
    in a later one; random V; against the fp64 oracle at the arithmetic bar.  Key 120 is in step 7 of 9: with 1 and 3 splits
    (steps 0-8 and 6-8) a step with a finite maximum of 0 precedes it, so the deferral comparison decides; the default split
    count gives every step its own split, where the first step of a split always rescales."""
    ks, leads = ax.graded_amplitudes(ax.source_constant("gqa_decode_tile.h", "kGqaDefer"), ax.GQA_SCALE)
    for Hq, Hkv in ((8, 2), (16, 1)):
        c = ax.gqa_graded_case(130, Hq, Hkv, ks, tokens=[5, 120])
        for page in (16, 256):
            dev = gqa_device(c, page)
            for s in (1, 3, None):
                assert_close(gqa_run(dev, s), c["want"], 1e-2, what=("gqa decode graded", leads, page, s))


@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
def test_gqa_decode_kv_fp8_counts_and_probes(Hq, Hkv):
    """the fp8 K / V cache against the closed forms (the shared tile code cannot fake those): page 48, splits 1, 3 and more than steps"""
    page, splits = 48, [1, 3, 17]
    c = ax.gqa_count_case(130, Hq, Hkv)
    dev = gqa_device(c, page, fp8=True)
    report(f"gqa decode kv fp8 counting Hq={Hq} Hkv={Hkv}, relative", max(ax.check_count(gqa_run(dev, s), c["want"]) for s in splits))
    worst = 0.0
    for n in (17, 64, 130):
        c = ax.gqa_dominant_case(n, Hq, Hkv, ax.probe_tokens(n, ax.STEP_GQA, page, splits))
        dev = gqa_device(c, page, fp8=True)
        worst = max([worst] + [ax.check_dominant(gqa_run(dev, s), c["want"]) for s in splits])
    report(f"gqa decode kv fp8 dominant key Hq={Hq} Hkv={Hkv}, absolute", worst)


# ---------------------------------------------------------------- MLA decode
def mla_device(case, page, fp8=False):
    from chitu_amd import ops

    cache, table = ax.mla_pages(case, page, seed=page)
    cd = cache.cuda()
    if fp8:
        c8 = ops.mla_kv_quant_fp8(cd.view(-1, 576)).view(cache.shape[0], page, m8.ROW)
        assert torch.equal(ops.mla_kv_dequant_fp8(c8).view(torch.int16), cd.view(torch.int16))
        cd = c8
    return case["q_nope"].cuda(), case["q_pe"].cuda(), cd, case["lens"].cuda(), table.cuda()


def mla_run(dev, splits):
    qn, qp, cd, lens, table = dev
    return backend(qn.shape[1]).mla_decode(qn, qp, cd, lens, table, ax.MLA_SCALE, num_splits=splits)


@pytest.mark.parametrize("H", MLA_HEADS)
@pytest.mark.parametrize("page", MLA_PAGES)
def test_mla_decode_counts_every_key_once_at_every_length(page, H):
    """lengths 0 .. 258 (four 64-key tiles plus 2) in one launch per split count"""
    c = ax.mla_count_case(258, H)
    dev = mla_device(c, page)
    worst = max(ax.check_count(mla_run(dev, s), c["want"]) for s in MLA_SPLITS)
    report(f"mla decode counting page={page} H={H}, relative", worst)


@pytest.mark.parametrize("H", MLA_HEADS)
@pytest.mark.parametrize("n", [17, 64, 130, 258])
def test_mla_decode_returns_the_probed_keys_row(n, H):
    worst = 0.0
    for page in MLA_PAGES:
        c = ax.mla_dominant_case(n, H, ax.probe_tokens(n, ax.TILE, page, real(MLA_SPLITS)))
        dev = mla_device(c, page)
        worst = max([worst] + [ax.check_dominant(mla_run(dev, s), c["want"]) for s in MLA_SPLITS])
    report(f"mla decode dominant key n={n} H={H}, absolute", worst)


def test_mla_decode_graded_margin():
    """mla_decode_tile.h's tile step has no deferral constant (it rescales on every tile); the margins of the MLA prefill kernel's
    constant, key in the first tile and in a later one, random latent rows, against the fp64 oracle at the arithmetic bar."""
    ks, leads = ax.graded_amplitudes(ax.source_constant("mla_prefill_flash.hip", "kDefer") * math.log(2), ax.MLA_SCALE)
    c = ax.mla_graded_case(258, 16, ks, tokens=[5, 200])
    dev = mla_device(c, 64)
    for s in (1, 3, None):
        assert_close(mla_run(dev, s), c["want"], 1e-2, what=("mla decode graded", leads, s))


@pytest.mark.parametrize("H", [16, 5])
def test_mla_decode_kv_fp8_counts_and_probes(H):
    page, splits = 64, [1, 3, 7]
    c = ax.mla_count_case(258, H)
    dev = mla_device(c, page, fp8=True)
    report(f"mla decode kv fp8 counting H={H}, relative", max(ax.check_count(mla_run(dev, s), c["want"]) for s in splits))
    worst = 0.0
    for n in (17, 64, 130, 258):
        c = ax.mla_dominant_case(n, H, ax.probe_tokens(n, ax.TILE, page, splits))
        dev = mla_device(c, page, fp8=True)
        worst = max([worst] + [ax.check_dominant(mla_run(dev, s), c["want"]) for s in splits])
    report(f"mla decode kv fp8 dominant key H={H}, absolute", worst)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_mla_decode_one_split_of_more_than_512_tiles(fp8):
    """33000 keys in ONE split are 516 tiles: more than kMaxTilesLds page ids, so the kernel reads the table per tile
    (pages_in_lds == false); with two splits it is back on the LDS list.  Both runs must return the probed keys' rows, and both
    must agree with the oracle on random data at the existing bar."""
    from chitu_amd import ops

    assert ax.LONG_N > ax.TILE * ax.source_constant("mla_decode_tile.h", "kMaxTilesLds")
    c = ax.mla_dominant_case(ax.LONG_N, 16, ax.LONG_PROBES)
    dev = mla_device(c, 64, fp8=fp8)
    for s in (1, 2):
        report(f"mla decode {'kv fp8 ' if fp8 else ''}dominant key n={ax.LONG_N} splits={s}, absolute", ax.check_dominant(mla_run(dev, s), c["want"]))
    g = torch.Generator().manual_seed(33)
    rows = torch.randn(ax.LONG_N, 576, generator=g).to(torch.bfloat16)
    if fp8:  # the rows the cache will hold
        rows = m8.dequant_ref(m8.quant_ref(rows))
    r = dict(q_nope=(torch.randn(2, 16, 512, generator=g) * 0.3).to(torch.bfloat16), q_pe=(torch.randn(2, 16, 64, generator=g) * 0.3).to(torch.bfloat16),
             rows=rows.float(), lens=torch.tensor([ax.LONG_N, ax.LONG_N - 65], dtype=torch.int32), fill=0.0)
    cache, table = ax.mla_pages(r, 64, seed=7)
    ref = omla.mla_decode(r["q_nope"], r["q_pe"], cache, table, r["lens"], ax.MLA_SCALE)
    cd = cache.cuda()
    if fp8:
        cd = ops.mla_kv_quant_fp8(cd.view(-1, 576)).view(cache.shape[0], 64, m8.ROW)
        assert torch.equal(ops.mla_kv_dequant_fp8(cd).cpu().view(torch.int16), cache.view(torch.int16))
    for s in (1, 2):
        out = mla_run((r["q_nope"].cuda(), r["q_pe"].cuda(), cd, r["lens"].cuda(), table.cuda()), s)
        assert_close(out, ref, 1e-2, what=("mla decode, 516 tiles, random data", fp8, s))


# ---------------------------------------------------------------- prefill
def cu_dev(case):
    return torch.tensor(case["cu"], dtype=torch.int32).cuda()


def gqa_prefill(case, Hq, strided=False):
    q, k, v = (case[n].to(torch.bfloat16).cuda() for n in ("q", "k", "v"))
    if strided:  # the slices of one merged qkv projection output
        Hkv = k.shape[1]
        qkv = torch.cat([q, k, v], dim=1)
        q, k, v = qkv[:, :Hq], qkv[:, Hq : Hq + Hkv], qkv[:, Hq + Hkv :]
        assert not q.is_contiguous()
    cu, m = cu_dev(case), max(b - a for a, b in zip(case["cu"][:-1], case["cu"][1:]))
    return backend(Hq).attn_varlen_func(q, k, v, cu, cu, m, m, causal=True, softmax_scale=ax.GQA_SCALE)


@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (8, 2), (32, 1)])  # 128, 32 and 4 query tokens in a workgroup
def test_gqa_prefill_every_query_row_is_its_own_length_sweep(Hq, Hkv, monkeypatch):
    """Counting, tied dominant keys and the graded margin through the flash kernel (contiguous and strided) and, where the decode
    kernel's group limit allows, through the composition from the decode kernel."""
    count = ax.prefill_count_case(ax.PREFILL_SEQS, Hq, Hkv, 128, ax.P_GQA)
    tied = ax.prefill_dominant_case(ax.PREFILL_SEQS, Hq, Hkv, 128)
    ks, leads = ax.graded_amplitudes(ax.source_constant("gqa_prefill_flash.hip", "kDefer") * math.log(2), ax.GQA_SCALE)
    graded = ax.prefill_graded_case(200, Hq, Hkv, 128, ks, tokens=[5, 150])
    modes = [("flash", False), ("flash", True)] + ([("compose", False)] if Hq // Hkv <= 16 else [])
    for mode, strided in modes:
        monkeypatch.setenv("CHITU_GQA_PREFILL", mode)
        tag = f"gqa prefill {mode}{' strided' if strided else ''} Hq={Hq} Hkv={Hkv}"
        report(f"{tag} counting, relative", ax.check_count(gqa_prefill(count, Hq, strided), count["want"]))
        report(f"{tag} tied dominant keys, relative", ax.check_tied(gqa_prefill(tied, Hq, strided), tied["want"]))
        assert_close(gqa_prefill(graded, Hq, strided), graded["want"], 1e-2, what=(tag, "graded", leads))


def mla_prefill(case, H):
    q, kv = case["q"].to(torch.bfloat16).cuda(), case["k"].to(torch.bfloat16).cuda()
    cu, m = cu_dev(case), max(b - a for a, b in zip(case["cu"][:-1], case["cu"][1:]))
    return backend(H).attn_varlen_func(q, kv, kv[..., :512].contiguous(), cu, cu, m, m, causal=True, softmax_scale=ax.MLA_SCALE)


@pytest.mark.parametrize("mode", ["flash", "exact"])
@pytest.mark.parametrize("H", [16, 5])
def test_mla_prefill_every_query_row_is_its_own_length_sweep(H, mode, monkeypatch):
    monkeypatch.setenv("CHITU_MLA_PREFILL", mode)
    count = ax.prefill_count_case(ax.PREFILL_SEQS, H, 1, 512, ax.P_MLA)
    report(f"mla prefill {mode} H={H} counting, relative", ax.check_count(mla_prefill(count, H), count["want"]))
    tied = ax.prefill_dominant_case(ax.PREFILL_SEQS, H, 1, 512)
    report(f"mla prefill {mode} H={H} tied dominant keys, relative", ax.check_tied(mla_prefill(tied, H), tied["want"]))
    ks, leads = ax.graded_amplitudes(ax.source_constant("mla_prefill_flash.hip", "kDefer") * math.log(2), ax.MLA_SCALE)
    graded = ax.prefill_graded_case(200, H, 1, 512, ks, tokens=[5, 150])
    assert_close(mla_prefill(graded, H), graded["want"], 1e-2, what=("mla prefill graded", mode, H, leads))


# ---------------------------------------------------------------- byte offsets beyond 4 GiB
def first_page_beyond_4gib(page_bytes):
    return 2 ** 32 // page_bytes + 1


def need_free(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * nbytes:
        pytest.skip(f"{nbytes / 2**30:.1f} GiB cache: needs {3 * nbytes / 2**30:.0f} GiB free, {free / 2**30:.0f} GiB are")


def place_and_append(caches, rows, fills, tables, lens, quant, append):
    """Write every sequence's rows but its last into its pages (the pages' other rows and page 0 hold fills[c] everywhere: what a
    wrongly admitted key would show), append the last row through the project's append op, and assert that exactly the addressed
    rows of the named pages changed, page 0 not at all.  caches / rows / fills: one entry per cache (K and V, or the one MLA
    cache); rows[c][s]: [n_s, ...] bf16 logical rows of sequence s."""
    page = caches[0].shape[1]
    ids = sorted({int(p) for t in tables for p in t})
    want = []
    for cache, seq_rows, fill in zip(caches, rows, fills):
        sentinel = quant(torch.full((page,) + tuple(seq_rows[0].shape[1:]), fill, dtype=torch.bfloat16))
        cache[0] = sentinel.cuda()
        for i in ids:
            cache[i] = sentinel.cuda()
        for r, t, n in zip(seq_rows, tables, lens):
            for p in range((n + page - 1) // page):
                stop = min(n - 1, (p + 1) * page)
                if stop > p * page:
                    cache[int(t[p]), : stop - p * page] = quant(r[p * page : stop]).cuda()
        w = cache[ids].cpu()
        for r, t, n in zip(seq_rows, tables, lens):
            w[ids.index(int(t[(n - 1) // page])), (n - 1) % page] = quant(r[n - 1 : n])[0]
        want.append((w, sentinel))
    width = max(len(t) for t in tables)
    table = torch.tensor([list(t) + [t[-1]] * (width - len(t)) for t in tables], dtype=torch.int32).cuda()
    old = torch.tensor([n - 1 for n in lens], dtype=torch.int32).cuda()
    append(table, [torch.stack([r[n - 1] for r, n in zip(seq_rows, lens)]).cuda() for seq_rows in rows], old)
    for cache, (w, sentinel) in zip(caches, want):
        assert torch.equal(cache[ids].cpu(), w), "the append changed another row of the named pages, or not the addressed one"
        assert torch.equal(cache[0].cpu(), sentinel), "the append wrote into page 0"
    return table


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_gqa_caches_beyond_4gib(fp8):
    """K / V caches whose every named page lies more than 2^32 bytes into the allocation (page 256, 8 KV heads: page ids above 8192;
    fp8 rows: above 14563): the append writes exactly the addressed rows, and constructions 1 and 2 hold at 17 and 130 keys
    (ax.big_gqa_cases; the rest of every named page holds 16 in K and 1 in V)."""
    from chitu_amd import ops

    Hq, Hkv, page = 32, 8, 256
    row = g8.ROW if fp8 else 128
    first = first_page_beyond_4gib(page * Hkv * row * (1 if fp8 else 2))
    pages = first + 6
    need_free(2 * pages * page * Hkv * row * (1 if fp8 else 2))
    kc = vc = None
    try:
        kc, vc = (torch.empty(pages, page, Hkv, row, dtype=torch.uint8 if fp8 else torch.bfloat16, device="cuda") for _ in range(2))
        assert (first * page * Hkv * row) * kc.element_size() > 2 ** 32
        tables = [[first + 3], [first + 1], [first + 4], [first]]  # each sequence in its own page, in no order
        cases = ax.big_gqa_cases(Hq, Hkv, page)
        lens = [int(c["lens"][0]) for c in cases]
        quant = (lambda r: g8.quant_ref(r.to(torch.bfloat16))) if fp8 else (lambda r: r.to(torch.bfloat16))

        def append(table, new, old):
            if fp8:
                ops.append_gqa_kv_fp8(kc, vc, table, new[0], new[1], old)
            else:
                ops.append_to_paged_kv_cache(kc, table, new[0].contiguous(), old)
                ops.append_to_paged_kv_cache(vc, table, new[1].contiguous(), old)

        rows = [[c["K"].to(torch.bfloat16) for c in cases], [c["V"].to(torch.bfloat16) for c in cases]]
        table = place_and_append([kc, vc], rows, [ax.K_AMP, 1.0], tables, lens, quant, append)
        be = backend(Hq)
        tag = f"gqa decode {'kv fp8 ' if fp8 else ''}beyond 4 GiB"
        for splits in (1, 3):
            for s, c in enumerate(cases):
                bs = c["q"].shape[0]
                out = be.attn_with_kvcache(c["q"].cuda(), kc, vc, cache_seqlens=c["lens"].cuda(), block_table=table[s : s + 1].repeat(bs, 1).contiguous(),
                                           softmax_scale=ax.GQA_SCALE, num_splits=splits)[:, 0]
                if s < 2:
                    report(f"{tag} counting n={lens[s]} splits={splits}, relative", ax.check_count(out, c["want"]))
                else:
                    report(f"{tag} dominant key n={lens[s]} splits={splits}, absolute", ax.check_dominant(out, c["want"]))
    finally:
        del kc, vc
        torch.cuda.empty_cache()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_mla_cache_beyond_4gib(fp8):
    """The latent cache with every named page more than 2^32 bytes in (bf16 rows: page ids above 58255; fp8 rows: above 102300);
    ax.big_mla_cases, the rest of every named page holds 16 everywhere."""
    from chitu_amd import ops

    H, page = 16, 64
    row_bytes = m8.ROW if fp8 else 1152
    first = first_page_beyond_4gib(page * row_bytes)
    pages = first + 10
    need_free(pages * page * row_bytes)
    cache = None
    try:
        cache = torch.empty(pages, page, m8.ROW if fp8 else 576, dtype=torch.uint8 if fp8 else torch.bfloat16, device="cuda")
        assert first * page * row_bytes > 2 ** 32
        tables = [[first + 8], [first + 2, first + 7, first + 1], [first + 5], [first + 4, first, first + 6]]
        cases = ax.big_mla_cases(H, page)
        lens = [int(c["lens"][0]) for c in cases]
        quant = (lambda r: m8.quant_ref(r.to(torch.bfloat16))) if fp8 else (lambda r: r.to(torch.bfloat16))

        def append(table, new, old):
            if fp8:
                ops.append_mla_kv_fp8(cache, table, new[0].view(-1, 1, 576), old)
            else:
                ops.append_to_paged_kv_cache(cache, table, new[0].view(-1, 1, 576).contiguous(), old)

        table = place_and_append([cache], [[c["rows"].to(torch.bfloat16) for c in cases]], [ax.K_AMP], tables, lens, quant, append)
        be = backend(H)
        tag = f"mla decode {'kv fp8 ' if fp8 else ''}beyond 4 GiB"
        for splits in (1, 3):
            for s, c in enumerate(cases):
                bs = c["q_nope"].shape[0]
                out = be.mla_decode(c["q_nope"].cuda(), c["q_pe"].cuda(), cache, c["lens"].cuda(), table[s : s + 1].repeat(bs, 1).contiguous(),
                                    ax.MLA_SCALE, num_splits=splits)
                if s < 2:
                    report(f"{tag} counting n={lens[s]} splits={splits}, relative", ax.check_count(out, c["want"]))
                else:
                    report(f"{tag} dominant key n={lens[s]} splits={splits}, absolute", ax.check_dominant(out, c["want"]))
    finally:
        del cache
        torch.cuda.empty_cache()
