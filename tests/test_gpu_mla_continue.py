"""Continued and chunked prefill over the MLA latent cache on the GPU (DeepSeek-V3): the gather out of the pages
(chitu_ext2_mla_kv_gather, bf16 and fp8 pages), the flash prefill kernel with separate query and key extents
(chitu_ext2_mla_prefill_flash_continue) against the whole-sequence kernel bit for bit, against fp64, against exact constructions
and against the multi-token decode kernel, and DeepSeekV3Decoder.prefill_continue / prefill(chunk_size=) / generate(
prefill_chunk_size=) against the one-shot prefill and the decode steps.  Builders: tests/mla_continue_ref.py."""
import functools

import pytest
import torch

from tests import attn_exact as ax
from tests import mla_continue_ref as mc
from tests import row_exact as rx
from tests.test_gpu_deepseek_multi import LOGITS_BAR, MAKE_ARGS, ROWS_BAR, build_variant, cached_rows
from tests.util import assert_close, max_rel_to_peak

pytestmark = pytest.mark.gpu

ATTN_BAR = 1e-2  # the project's attention bar: of the peak of the fp64 attention
HEADS = [16, 5]  # one full head group; a partial one


def report(what, value):
    print(f"MLA_CONTINUE {what}: {value:.3e}" if isinstance(value, float) else f"MLA_CONTINUE {what}: {value}")


# ================================================================ the gather
GATHER_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 200]
NAN_BYTE = 0xFF  # 0xFF.. is NaN as bf16, as e4m3fn and as the fp32 scale


@functools.lru_cache(maxsize=None)
def gather_case(page, fmt):
    """Shuffled pages holding the sequences of GATHER_LENS; returns the clean cache, the poisoned one (NaN in every unreferenced
    page, in every row >= L of a last page and in the pages the table's entries beyond ceil(L / page) point at), the table
    (two such entries behind every sequence's pages), cu_seqlens_k and the expected rows (bf16 [T, 576]) -- CPU tensors."""
    from chitu_amd import ops

    g = torch.Generator().manual_seed(page + (1 if fmt == "fp8" else 0))
    need = [-(-L // page) for L in GATHER_LENS]
    n_pages = sum(need) + 5
    perm = torch.randperm(n_pages, generator=g).tolist()
    rows = (torch.randn(n_pages, page, 576, generator=g) * 2).to(torch.bfloat16)
    if fmt == "fp8":
        cache = ops.mla_kv_quant_fp8(rows.view(-1, 576).cuda()).cpu().view(n_pages, page, 656)
    else:
        cache = rows
    width = max(need) + 2
    spare = perm[sum(need):]
    table = torch.zeros(len(GATHER_LENS), width, dtype=torch.int32)
    live = torch.zeros(n_pages, page, dtype=torch.bool)
    want, used = [], 0
    for s, (L, k) in enumerate(zip(GATHER_LENS, need)):
        pages = perm[used:used + k]
        used += k
        table[s, :k] = torch.tensor(pages, dtype=torch.int32)
        table[s, k:] = torch.tensor([spare[(s + j) % len(spare)] for j in range(width - k)], dtype=torch.int32)
        for t in range(L):
            live[pages[t // page], t % page] = True
            want.append(cache[pages[t // page], t % page])
    want = torch.stack(want)
    if fmt == "fp8":
        want = ops.mla_kv_dequant_fp8(want.contiguous().cuda()).cpu()
    poisoned = cache.clone()
    poisoned.view(torch.uint8).view(n_pages, page, -1)[~live] = NAN_BYTE
    return dict(cache=cache, poisoned=poisoned, table=table, cu=torch.tensor(ax.cu_of(GATHER_LENS), dtype=torch.int32), want=want)


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("page", [16, 48, 64])
def test_gather_is_the_indexed_rows_and_reads_no_row_it_does_not_own(page, fmt):
    from chitu_amd import ops

    c = gather_case(page, fmt)
    T = int(c["cu"][-1])
    assert T == sum(GATHER_LENS) and bool(torch.isfinite(c["want"].float()).all())
    got = {}
    for name in ("cache", "poisoned"):
        out = rx.Guarded(T, 576, torch.bfloat16, stride=592)
        res = ops.mla_kv_gather(c[name].cuda(), c["table"].cuda(), c["cu"].cuda(), T, out=out.view.view(torch.bfloat16))
        assert res.data_ptr() == out.view.data_ptr()
        got[name] = out.check(f"gather page={page} {fmt} {name}", written=False)  # guard rows and columns untouched
        assert torch.equal(got[name].view(torch.int16), c["want"].view(torch.int16)), (page, fmt, name)
    assert bool(torch.isfinite(got["poisoned"].float()).all())
    fresh = ops.mla_kv_gather(c["cache"].cuda(), c["table"].cuda(), c["cu"].cuda(), T)  # out=None: allocated, contiguous
    assert tuple(fresh.shape) == (T, 576) and torch.equal(fresh.cpu().view(torch.int16), c["want"].view(torch.int16))


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_gather_writes_zeros_for_a_table_entry_out_of_range(fmt):
    from chitu_amd import ops

    page = 16
    c = gather_case(page, fmt)
    table = c["table"].clone()
    n_pages = c["cache"].shape[0]
    table[4, 1] = -1        # sequence of 17 rows: its second page (row 16)
    table[8, 3] = n_pages   # sequence of 200 rows: rows 48 .. 63
    cu = c["cu"].tolist()
    want = c["want"].clone()
    want[cu[4] + 16] = 0
    want[cu[8] + 48:cu[8] + 64] = 0
    T = cu[-1]
    out = rx.Guarded(T, 576, torch.bfloat16)
    ops.mla_kv_gather(c["poisoned"].cuda(), table.cuda(), c["cu"].cuda(), T, out=out.view.view(torch.bfloat16))
    assert torch.equal(out.check("gather out-of-range entries", written=False).view(torch.int16), want.view(torch.int16))


# ================================================================ the flash kernel with separate extents
def random_case(seqs, H, seed):
    g = torch.Generator().manual_seed(seed)
    T = sum(seqs)
    q = (torch.randn(T, H, 576, generator=g) * 0.3).to(torch.bfloat16)
    kv = torch.randn(T, 576, generator=g).to(torch.bfloat16)
    return q, kv, ax.cu_of(seqs)


@pytest.mark.parametrize("H", HEADS)
def test_no_prefix_is_the_whole_sequence_kernel_bit_for_bit(H):
    q, kv, cu = random_case(ax.PREFILL_SEQS, H, seed=H)
    whole = mc.flash_whole(q, kv, cu, ax.MLA_SCALE)
    got = mc.flash_continue(q, kv, cu, cu, max(ax.PREFILL_SEQS), ax.MLA_SCALE)
    assert torch.equal(got.view(torch.int16), whole.view(torch.int16))


PREFIXES = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 200]
NEW = [1, 2, 7, 8, 9, 33, 129]


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("n", NEW)
def test_rows_of_whole_blocks_equal_the_whole_sequence_call_and_all_rows_meet_the_bar(n, H):
    """One ragged launch per n: the eleven prefixes as eleven sequences.  Rows at an absolute position >= 8 * ceil(P / 8) sit in
    workgroups that hold the same eight rows as in the whole-sequence call (same votes, same arithmetic): torch.equal.  The up
    to 7 rows in front share their workgroup with dead rows: the attention bar against fp64, as every live row."""
    seqs = [P + n for P in PREFIXES]
    q, kv, cu = random_case(seqs, H, seed=100 * n + H)
    whole = mc.flash_whole(q, kv, cu, ax.MLA_SCALE).cpu()
    qt, cu_q, idx = mc.tails(q, cu, [n] * len(PREFIXES))
    got = mc.flash_continue(qt, kv, cu_q, cu, n, ax.MLA_SCALE).cpu()
    ref = mc.prefill64_offset(qt.float(), kv.float(), cu_q, cu, ax.MLA_SCALE)
    err = max_rel_to_peak(got, ref)
    report(f"n={n} H={H} all live rows vs fp64, of the peak", err)
    assert err < ATTN_BAR
    n_equal = 0
    for s, P in enumerate(PREFIXES):
        first = max(8 * -(-P // 8) - P, 0)  # the first query whose block has no dead row
        rows = slice(cu_q[s] + first, cu_q[s + 1])
        if first < n:
            assert torch.equal(got[rows].view(torch.int16), whole[idx[rows]].view(torch.int16)), (P, n, H)
            n_equal += n - first
    assert n_equal > 0 or n < 8


@pytest.mark.parametrize("H", HEADS)
def test_zero_queries_count_exactly_the_first_P_plus_i_plus_1_rows(H):
    """q = 0: the output is the mean of the indicator rows of exactly the permitted keys; one key more or less (an unmasked block,
    a prefix row dropped) moves a channel by >= 1/17 of its value, or sets a channel no permitted key sets."""
    c = mc.count_case([(P, n) for P in PREFIXES for n in NEW], H)
    got = mc.flash_continue(c["q"], c["kv"], c["cu_q"], c["cu_k"], c["max_q"], ax.MLA_SCALE)
    report(f"counting H={H}: worst relative error of n_d / n", ax.check_count(got, c["want"]))


DOMINANT_PAIRS = [(1, 2), (7, 9), (8, 3), (31, 3), (32, 2), (33, 8), (63, 2), (65, 7)]


@pytest.mark.parametrize("P,n", DOMINANT_PAIRS)
def test_a_dominant_key_returns_its_row_and_one_past_the_causal_edge_does_not_appear(P, n):
    """Keys 0, P - 1, P, P + i and both sides of every 32-key block edge, each probed by query i of its own sequence: the output
    is that key's row.  Then the key at P + i + 1, one past query i's causal edge, carries the amplitude: an unmasked block would
    return its row; the masked kernel returns the mean of the permitted rows."""
    H = 5
    c = mc.dominant_case(P, n, H)
    got = mc.flash_continue(c["q"], c["kv"], c["cu_q"], c["cu_k"], c["max_q"], ax.MLA_SCALE).cpu()
    report(f"dominant P={P} n={n}: worst absolute error", ax.check_dominant(got[c["probed"]], c["want"][c["probed"]]))
    rest = torch.ones(got.shape[0], dtype=torch.bool)
    rest[c["probed"]] = False
    ax.check_tied(got[rest], c["want"][rest])
    if n > 1:
        b = mc.dominant_case(P, n, H, beyond=True)
        got = mc.flash_continue(b["q"], b["kv"], b["cu_q"], b["cu_k"], b["max_q"], ax.MLA_SCALE).cpu()
        report(f"beyond the edge P={P} n={n}: worst relative error of the mean", ax.check_tied(got, b["want"]))


def test_more_queries_than_keys_stays_inside_the_sequence():
    """(L, n) = (3, 5), outside the contract, between two ordinary sequences: its last 3 rows are the attention of 3 queries over
    3 keys, its first 2 rows keep the sentinel, the guards and the neighbours' rows are as without it."""
    H = 5
    ns, Ls = [4, 5, 6], [10, 3, 6]
    g = torch.Generator().manual_seed(5)
    q = (torch.randn(sum(ns), H, 576, generator=g) * 0.3).to(torch.bfloat16)
    kv = torch.randn(sum(Ls), 576, generator=g).to(torch.bfloat16)
    cu_q, cu_k = ax.cu_of(ns), ax.cu_of(Ls)
    out = rx.Guarded(sum(ns) * H, 512, torch.bfloat16)
    mc.flash_continue(q, kv, cu_q, cu_k, max(ns), ax.MLA_SCALE, out=out.view.view(torch.bfloat16).view(sum(ns), H, 512))
    got = out.check("L < n", written=False).view(sum(ns), H, 512)
    skipped = got[cu_q[1]:cu_q[1] + 2].view(torch.int16)
    assert bool((skipped == rx.SENTINEL16).all())
    ref = mc.prefill64_offset(q.float(), kv.float(), cu_q, cu_k, ax.MLA_SCALE)
    live = torch.ones(sum(ns), dtype=torch.bool)
    live[cu_q[1]:cu_q[1] + 2] = False
    assert max_rel_to_peak(got[live], ref[live]) < ATTN_BAR


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_up_to_eight_queries_agree_with_the_multi_token_decode_kernel(T, fmt):
    """The other implementation of this mask, on the same pages: HipAttnBackend.mla_attn_varlen_with_kvcache (gather + flash)
    against mla_decode_multi, both reading a bf16 or an fp8 cache."""
    from chitu_amd import ops
    from chitu_amd.attn_backend import HipAttnBackend

    H, page = 16, 64
    lens = [T, 17, 64, 65, 200]
    g = torch.Generator().manual_seed(T)
    need = [-(-L // page) for L in lens]
    n_pages = sum(need) + 2
    perm = torch.randperm(n_pages, generator=g)
    rows = torch.randn(n_pages, page, 576, generator=g).to(torch.bfloat16).cuda()
    cache = ops.mla_kv_quant_fp8(rows.view(-1, 576)).view(n_pages, page, 656) if fmt == "fp8" else rows
    table = torch.zeros(len(lens), max(need), dtype=torch.int32)
    used = 0
    for s, k in enumerate(need):
        table[s, :k] = perm[used:used + k].to(torch.int32)
        used += k
    q = (torch.randn(len(lens), T, H, 576, generator=g) * 0.3).to(torch.bfloat16).cuda()
    be = HipAttnBackend(local_n_heads=H)
    seqlens = torch.tensor(lens, dtype=torch.int32).cuda()
    want = be.mla_decode_multi(q[..., :512], q[..., 512:], cache, seqlens, table.cuda(), ax.MLA_SCALE, kernel="multi")
    cu_q = torch.arange(0, (len(lens) + 1) * T, T, dtype=torch.int32).cuda()
    got = be.mla_attn_varlen_with_kvcache(q.view(-1, H, 576), cache, cu_q, seqlens, table.cuda(), T, sum(lens), ax.MLA_SCALE)
    assert tuple(got.shape) == (len(lens) * T, H, 512)
    err = max_rel_to_peak(got, want.view(-1, H, 512))
    report(f"T={T} {fmt} vs mla_decode_multi, of the peak", err)
    assert err < ATTN_BAR


# ================================================================ the model
PROMPT_LENS, HEAD_LENS = (21, 70, 45), (5, 33, 17)
A, B, C = ["a0", "a1", "a2"], ["b0", "b1", "b2"], ["c0", "c1", "c2"]


def prompts_of(vocab, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in PROMPT_LENS]


def decode_tail(model, cache, prompts, reqs, step=1):
    """prefill of the heads, then the tails through decode steps (requests leave as their prompts end): token by token through
    the single-token step, or with step = 8 through decode_multi, T = min(8, the shortest remaining tail) tokens at a time (one
    token: the single-token step).  Returns the logits of every prompt's last token.  Every path here exists without
    prefill_continue."""
    logits = model.prefill([p[:h] for p, h in zip(prompts, HEAD_LENS)], reqs).clone()
    done = list(HEAD_LENS)
    while True:
        live = [i for i, p in enumerate(prompts) if len(p) > done[i]]
        if not live:
            return logits
        ids = [reqs[i] for i in live]
        T = min(step, min(len(prompts[i]) - done[i] for i in live))
        tok = torch.tensor([prompts[i][done[i]:done[i] + T] for i in live], dtype=torch.int64, device="cuda")
        if T == 1:
            cache.prepare_cache_decode(ids)
            cache.prepare_block_table_for_decode(ids)
            out = model.decode(tok[:, 0].contiguous(), use_graph=False)
            cache.finalize_cache_single_decode(ids)
        else:
            cache.prepare_block_table_for_decode_multi(ids, T)
            out = model.decode_multi(tok, use_graph=False)[:, -1]
            cache.finalize_cache_multi_decode(ids, [T] * len(ids))
        logits[torch.tensor(live, device="cuda")] = out
        for i in live:
            done[i] += T


def spread(cache, prompts, got_logits, want_logits, reqs_got, reqs_want):
    """(logits error, worst cached-row error over requests and layers), both of the peak"""
    rows = 0.0
    for a, b, p in zip(reqs_want, reqs_got, prompts):
        assert cache.seq_lens[a] == cache.seq_lens[b] == len(p)
        assert len(cache.block_table[a]) == len(cache.block_table[b]) == -(-len(p) // cache.block_size)
        ra, rb = cached_rows(cache, a, 0, len(p)), cached_rows(cache, b, 0, len(p))
        rows = max(rows, max(max_rel_to_peak(rb[layer], ra[layer]) for layer in range(ra.shape[0])))
    return max_rel_to_peak(got_logits, want_logits), rows


@functools.lru_cache(maxsize=None)
def bars_of(arch):
    """(logits bar, rows bar) of the model comparisons: tests/test_gpu_prefill_paged.py's 3e-2 and 1e-2 of the peak, or twice the
    PARENT's own spread where that is larger.  The fp8-weight stack re-quantises activations per row group, so two paths whose
    GEMMs run at other row counts or through other launches may flip a code; the spread is measured between two such paths that
    exist without prefill_continue -- one-shot prefill against prefill(head) + token-by-token decode of the tail, bf16 cache --
    once per architecture."""
    model, cache = build_variant(arch, "bf16")
    prompts = prompts_of(model.args.vocab_size)
    whole = model.prefill(prompts, A).clone()
    parent = spread(cache, prompts, decode_tail(model, cache, prompts, B), whole, B, A)
    report(f"{arch} parent spread (one-shot vs head + decode, bf16 cache): logits, rows", f"{parent[0]:.3e} {parent[1]:.3e}")
    return max(LOGITS_BAR, 2 * parent[0]), max(ROWS_BAR, 2 * parent[1])


@pytest.mark.parametrize("arch", list(MAKE_ARGS))
def test_bf16_split_and_chunked_prefill_are_the_one_shot_prefill(arch):
    """prefill(head) + prefill_continue(tail), and prefill(chunk_size = c) for four chunk sizes, against one-shot prefill: the
    last-token logits and every layer's cached rows at the bars of bars_of (3e-2 and 1e-2 of the peak, or twice the parent's
    own spread)."""
    model, cache = build_variant(arch, "bf16", max_reqs=24)
    vocab = model.args.vocab_size
    prompts = prompts_of(vocab)
    whole = model.prefill(prompts, A).clone()
    bars = bars_of(arch)
    model.prefill([p[:h] for p, h in zip(prompts, HEAD_LENS)], C)
    got = model.prefill_continue([p[h:] for p, h in zip(prompts, HEAD_LENS)], C)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, vocab) and bool(torch.isfinite(got).all())
    runs = {"split": (got, C)}
    for c in (7, 16, 64, 100):
        reqs = [f"k{c}_{i}" for i in range(3)]
        runs[f"chunk_size={c}"] = (model.prefill(prompts, reqs, chunk_size=c), reqs)
    for name, (logits, reqs) in runs.items():
        e = spread(cache, prompts, logits, whole, reqs, A)
        report(f"{arch} bf16 {name} vs one-shot: logits, rows (bars {bars[0]:.3e} {bars[1]:.3e})", f"{e[0]:.3e} {e[1]:.3e}")
        assert e[0] < bars[0] and e[1] < bars[1], (arch, name, e, bars)


@pytest.mark.parametrize("arch", list(MAKE_ARGS))
def test_fp8_split_prefill_is_prefill_plus_single_token_decode(arch):
    """With an fp8 cache prefill_continue attends over quantised rows, as the decode step does and one-shot prefill does not: the
    comparison is prefill(head) + decode of the tail, token by token -- the prefill stack against the decode stack, the pair of
    paths bars_of measures.  Logits at the same bar as the bf16 test (bars_of: 3e-2, or twice the parent's spread).  Lengths and
    table sizes equal (spread asserts them).  The rows are printed, not asserted: one e4m3 code that the other stack flips moves
    a dequantised element by 1/16 of its value, up to 7 % of the peak, while both rows are right.  Also printed: the spread of
    head + decode_multi (up to 8 tokens a step) against head + decode, two decode-stack paths: 0 on an MI355X.
    Measured on an MI355X: v3_like 1.99e-2 (bar 4.10e-2), v2lite_like 3.21e-2 (bar 4.03e-2; above the plain 3e-2)."""
    model, cache = build_variant(arch, "fp8", max_reqs=12)
    vocab = model.args.vocab_size
    prompts = prompts_of(vocab)
    bar = bars_of(arch)[0]
    want = decode_tail(model, cache, prompts, A)
    parent = spread(cache, prompts, decode_tail(model, cache, prompts, C, step=8), want, C, A)
    report(f"{arch} fp8 head + decode_multi vs head + decode: logits, rows", f"{parent[0]:.3e} {parent[1]:.3e}")
    model.prefill([p[:h] for p, h in zip(prompts, HEAD_LENS)], B)
    got = model.prefill_continue([p[h:] for p, h in zip(prompts, HEAD_LENS)], B)
    e = spread(cache, prompts, got, want, B, A)
    report(f"{arch} fp8 split vs head + decode: logits, rows (logits bar {bar:.3e})", f"{e[0]:.3e} {e[1]:.3e}")
    assert e[0] < bar, (e, bar)


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("arch", list(MAKE_ARGS))
def test_prefill_continue_of_three_tokens_is_one_multi_token_step(arch, fmt):
    """The same three tokens behind the same prompts through the prefill stack (prefill_continue) and through the decode stack
    (decode_multi): bars_of's bars, the spread of exactly such a pair of paths."""
    logits_bar, rows_bar = bars_of(arch)
    model, cache = build_variant(arch, fmt)
    vocab = model.args.vocab_size
    prompts = prompts_of(vocab)
    model.prefill(prompts, A)
    model.prefill(prompts, B)
    tokens = torch.randint(0, vocab, (3, 3), generator=torch.Generator().manual_seed(2))
    cache.prepare_block_table_for_decode_multi(A, 3)
    multi = model.decode_multi(tokens.cuda(), use_graph=False).clone()
    cache.finalize_cache_multi_decode(A, [3] * 3)
    got = model.prefill_continue(tokens.tolist(), B)
    report(f"{arch} {fmt} prefill_continue(3) vs decode_multi: logits of the peak", max_rel_to_peak(got, multi[:, -1]))
    assert_close(got, multi[:, -1], logits_bar, what=(arch, fmt))
    for a, b, n in zip(A, B, PROMPT_LENS):
        assert cache.seq_lens[a] == cache.seq_lens[b] == n + 3
        ra, rb = cached_rows(cache, a, n, 3), cached_rows(cache, b, n, 3)
        report(f"{arch} {fmt} {b} appended rows, of the peak", max_rel_to_peak(rb, ra))
        if fmt == "bf16":  # (fp8 rows: one flipped e4m3 code is 1/16 of an element; the logits above are the check)
            assert max_rel_to_peak(rb, ra) < rows_bar, (arch, fmt, b)


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_generate_with_a_prefill_chunk_size_returns_its_pages(fmt):
    model, cache = build_variant("v3_like", fmt)
    prompts = prompts_of(model.args.vocab_size)
    free = len(cache.free_blocks)
    out = model.generate(prompts, 4, prefill_chunk_size=7)
    assert tuple(out.shape) == (3, 4) and out.dtype == torch.int64 and len(cache.free_blocks) == free and not cache.seq_lens
    with pytest.raises(ValueError):
        model.prefill(prompts, A, chunk_size=0)
    assert len(cache.free_blocks) == free and not cache.seq_lens


def test_an_unknown_request_or_an_overflow_raises_before_any_cache_state_changes():
    model, cache = build_variant("v3_like", "bf16", max_reqs=2)  # 2 x 9 pages of 64 rows; max_seq 512
    vocab = model.args.vocab_size
    prompts = prompts_of(vocab)[:2]
    model.prefill(prompts, A[:2])

    def state():
        return (dict(cache.seq_lens), list(cache.free_blocks), {r: list(t) for r, t in cache.block_table.items()},
                cache.paged_kv_cache.clone())

    before = state()

    def unchanged():
        now = state()
        return now[:3] == before[:3] and torch.equal(now[3], before[3])

    with pytest.raises(KeyError):
        model.prefill_continue([[1, 2], [3]], [A[0], "nobody"])
    assert unchanged()
    with pytest.raises(AssertionError):  # past the rotary table (max_position_embeddings = 512)
        model.prefill_continue([[1] * 3, [2] * (512 - PROMPT_LENS[1] + 1)], A[:2])
    assert unchanged()
    with pytest.raises(AssertionError):
        model.prefill_continue([[1], []], A[:2])
    assert unchanged()
    taken = [cache.get_free_block() for _ in range(len(cache.free_blocks) - 1)]  # one free page left
    before = state()
    with pytest.raises(Exception, match="free pages"):  # each request needs one page more
        model.prefill_continue([[1] * 60, [2] * 100], A[:2])
    assert unchanged()
    cache.free_blocks.extend(taken)
    before = state()
    got = model.prefill_continue([[1] * 60, [2] * 100], A[:2])  # and with the pages back it runs
    assert bool(torch.isfinite(got).all()) and cache.seq_lens[A[0]] == PROMPT_LENS[0] + 60 and cache.seq_lens[A[1]] == PROMPT_LENS[1] + 100
