"""Continued and chunked prefill over the paged K / V cache on the GPU: chitu_hip_gqa_prefill_paged (through
HipAttnBackend.attn_varlen_with_kvcache) against the contiguous flash kernel bit for bit where the two must agree, against the closed
forms and the fp64 attention of tests/attn_paged_prefill_ref.py, with every byte it must not use poisoned, against the multi-token
decode kernel; then LlamaDecoder / MixtralDecoder.prefill_continue, prefill(chunk_size=) and generate(prefill_chunk_size=) against
the one-shot prefill."""
import functools

import pytest
import torch

from tests import attn_exact as ax
from tests import attn_paged_prefill_ref as pp
from tests.util import assert_close, max_rel_to_peak

pytestmark = pytest.mark.gpu

HEADS = [(8, 8), (8, 2), (8, 1)]  # 128, 32 and 16 query tokens in a workgroup


def backend(Hq):
    from chitu_amd.attn_backend import HipAttnBackend

    return HipAttnBackend(local_n_heads=Hq)


def report(what, err):
    print(f"PREFILL_PAGED {what}: {err:.3e}")


def run_paged(case, pages, Hq, W=-1, c=0.0):
    """the kernel under test on a case of tests/attn_paged_prefill_ref.py and its pages (k_cache, v_cache, table, lens)"""
    kc, vc, table, lens = pages
    cu = torch.tensor(pp.cu_q(case), dtype=torch.int32).cuda()
    return backend(Hq).attn_varlen_with_kvcache(
        case["q"].to(torch.bfloat16).cuda(), kc.cuda(), vc.cuda(), cu, lens.cuda(), table.cuda(), max(case["news"]), causal=True,
        window_size=(W, 0) if W >= 0 else (-1, -1), softcap=c, softmax_scale=ax.GQA_SCALE)


def run_contiguous(case, Hq):
    """chitu_hip_gqa_prefill on every sequence's rows laid out contiguously, a query for EVERY row (case['q_all'])"""
    Ls = [int(k.shape[0]) for k in case["K"]]
    cu = torch.tensor(ax.cu_of(Ls), dtype=torch.int32).cuda()
    q, k, v = (torch.cat(x).to(torch.bfloat16).cuda() for x in (case["q_all"], case["K"], case["V"]))
    return backend(Hq).attn_varlen_func(q, k, v, cu, cu, max(Ls), max(Ls), causal=True, softmax_scale=ax.GQA_SCALE)


def whole_case(seq_pairs, Hq, Hkv, seed):
    """random rows with a query for every key; case['q'] holds the queries of the new rows only"""
    g = torch.Generator().manual_seed(seed)
    q_all = [(torch.randn(P + n, Hq, 128, generator=g) * 0.5).to(torch.bfloat16).float() for P, n in seq_pairs]
    K = [torch.randn(P + n, Hkv, 128, generator=g).to(torch.bfloat16).float() for P, n in seq_pairs]
    V = [torch.randn(P + n, Hkv, 128, generator=g).to(torch.bfloat16).float() for P, n in seq_pairs]
    return dict(q=torch.cat([q[P:] for q, (P, _) in zip(q_all, seq_pairs)]), q_all=q_all, K=K, V=V,
                prefixes=[P for P, _ in seq_pairs], news=[n for _, n in seq_pairs])


# ---------------------------------------------------------------- the two bit identities
@pytest.mark.parametrize("page", pp.PAGES)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_prefix_0_is_the_contiguous_kernel_bit_for_bit_under_any_block_table(Hq, Hkv, page):
    """(a): n = L.  One launch over ax.PREFILL_SEQS, each sequence's pages a random permutation."""
    case = whole_case([(0, L) for L in ax.PREFILL_SEQS], Hq, Hkv, seed=page + Hq)
    want = run_contiguous(case, Hq)
    for seed in (0, 1):
        got = run_paged(case, pp.paginate(case, page, seed=seed), Hq)
        assert torch.equal(got, want), (seed, max_rel_to_peak(got, want))
    assert_close(want, pp.expected64(case), 1e-2, what="the contiguous kernel itself")


@pytest.mark.parametrize("page", [16, 256])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_prefix_multiple_of_128_is_rows_of_the_whole_sequence_call_bit_for_bit(Hq, Hkv, page):
    """(b): P in {128, 256} x n in {1, 33, 129} as six sequences of one ragged launch against rows [P:] of chitu_hip_gqa_prefill
    on the whole sequences."""
    seq_pairs = [(P, n) for P in (128, 256) for n in (1, 33, 129)]
    case = whole_case(seq_pairs, Hq, Hkv, seed=7 + page)
    whole = run_contiguous(case, Hq)
    cu = ax.cu_of([P + n for P, n in seq_pairs])
    want = torch.cat([whole[cu[s] + P : cu[s + 1]] for s, (P, _) in enumerate(seq_pairs)])
    got = run_paged(case, pp.paginate(case, page, seed=3), Hq)
    assert torch.equal(got, want), max_rel_to_peak(got, want)


# ---------------------------------------------------------------- exact constructions
@pytest.mark.parametrize("page", pp.PAGES)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_every_query_counts_exactly_its_keys_and_returns_the_probed_keys_row(Hq, Hkv, page):
    """Prefixes {0, 1, 15, 16, 17, 63, 64, 65, 200} paired with new lengths {1, 2, 31, 33, 129} in one ragged launch.  Counting:
    q = 0, the output is the mean of exactly the first P + i + 1 V rows.  Dominant keys: 0, P - 1, P, P + i and both sides of every
    page and tile edge return their own row; a key one past the causal edge with the dominant score does not appear."""
    count = pp.count_case(pp.pairs(), Hq, Hkv)
    report(f"counting Hq={Hq} Hkv={Hkv} page={page}, relative",
           ax.check_count(run_paged(count, pp.paginate(count, page, seed=1), Hq), count["want"]))
    dom = pp.dominant_case(pp.pairs(), Hq, Hkv, page)
    report(f"dominant keys Hq={Hq} Hkv={Hkv} page={page}, absolute",
           ax.check_dominant(run_paged(dom, pp.paginate(dom, page, seed=2, v_fill=15.0), Hq), dom["want"]))


def test_queries_before_the_first_key_give_zeros():
    """L < n: the first n - L queries sit at negative positions (and a sequence of 0 keys has only such queries)"""
    case = pp.random_case([(-3, 5), (0, 4), (-1, 1), (-140, 200)], 8, 2, seed=4)
    got = run_paged(case, pp.paginate(case, 16, seed=4, poison_fill=float("nan")), 8).float().cpu()
    want = pp.expected64(case)
    dead = torch.tensor([P + i < 0 for P, n in zip(case["prefixes"], case["news"]) for i in range(n)])
    assert int(dead.sum()) == 3 + 1 + 140 and not bool(got[dead].any()) and not bool(want[dead].any())
    assert_close(got[~dead], want[~dead], 1e-2, what="rows behind the queries at negative positions")


# ---------------------------------------------------------------- poison
@pytest.mark.parametrize("page", pp.PAGES)
@pytest.mark.parametrize("W", [-1, 5, 100])
def test_no_byte_outside_the_visible_keys_is_used(page, W):
    """NaN in every page no sequence needs, in the pages every table entry beyond ceil(L / page) points at (valid indices), in the
    rows >= L of the last pages and (W >= 0) in the pages wholly before a sequence's lowest visible key: the outputs are finite
    and bit-identical to the run over finite fills."""
    Hq, Hkv = 8, 2
    case = pp.random_case(pp.pairs(), Hq, Hkv, seed=5)
    dead = pp.lowest_visible(case, W)
    clean = run_paged(case, pp.paginate(case, page, seed=6), Hq, W)
    pages = pp.paginate(case, page, seed=6, dead_before=dead, poison_fill=float("nan"))
    assert bool(pages[0].isnan().any()) and bool(pages[1].isnan().any())
    got = run_paged(case, pages, Hq, W)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)
    assert_close(got, pp.expected64(case, W=W), 1e-2, what=("poisoned", page, W))


# ---------------------------------------------------------------- window and cap
@pytest.mark.parametrize("c", [0.0, 5.0])
@pytest.mark.parametrize("W", [0, 5, 64, 100])
def test_window_and_cap_against_the_fp64_attention(W, c):
    Hq, Hkv, page = 8, 2, 16
    case = pp.random_case(pp.pairs(), Hq, Hkv, seed=8)
    for x in case["K"]:
        x *= 4.0  # scores of several nats: the cap matters
    want = pp.expected64(case, W=W, c=c)
    got = run_paged(case, pp.paginate(case, page, seed=9), Hq, W, c)
    report(f"window W={W} cap={c}, of the peak", assert_close(got, want, 1e-2, what=("window", W, c)))
    if c > 0 and W > 0:  # (one visible key: any cap gives its V row)
        assert max_rel_to_peak(pp.expected64(case, W=W), want) > 3e-2  # the cap is not a no-op on this data


@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("W", [0, 5, 64, 100])
def test_window_counts_exactly_its_keys_over_poisoned_pages(W, Hq, Hkv):
    """q = 0 under a window: the mean of exactly the last min(W + 1, P + i + 1) V rows; the pages wholly before a sequence's
    window hold NaN.  Dominant keys under the window: the first visible key returns its row, the one before it does not appear."""
    count = pp.count_case(pp.pairs(), Hq, Hkv)
    nan = float("nan")
    for page in pp.PAGES:
        pages = pp.paginate(count, page, seed=page, dead_before=pp.lowest_visible(count, W), poison_fill=nan)
        report(f"window counting W={W} Hq={Hq} Hkv={Hkv} page={page}, relative",
               ax.check_count(run_paged(count, pages, Hq, W), pp.count_want_window(count, Hq, W)))
    dom = pp.dominant_case(pp.pairs(), Hq, Hkv, 16, W)
    pages = pp.paginate(dom, 16, seed=W, dead_before=pp.lowest_visible(dom, W), poison_fill=nan)
    report(f"window dominant keys W={W} Hq={Hq} Hkv={Hkv}, absolute", ax.check_dominant(run_paged(dom, pages, Hq, W), dom["want"]))


# ---------------------------------------------------------------- against the other kernels, random data
@pytest.mark.parametrize("n", range(1, 9))
def test_against_the_multi_token_decode_kernel(n):
    """n = 1 .. 8 new rows per sequence over the same cache: chitu_hip_gqa_decode_multi is the other implementation of this mask"""
    Hq, Hkv, page = 8, 2, 16
    case = pp.random_case([(P, n) for P in (0, 5, 16, 63, 130)], Hq, Hkv, seed=20 + n)
    kc, vc, table, lens = (t.cuda() for t in pp.paginate(case, page, seed=n))
    got = run_paged(case, (kc, vc, table, lens), Hq)
    q = case["q"].to(torch.bfloat16).cuda().view(len(case["news"]), n, Hq, 128)
    multi = backend(Hq).attn_with_kvcache(q, kc, vc, None, None, cache_seqlens=lens, block_table=table, causal=True,
                                          softmax_scale=ax.GQA_SCALE)
    report(f"against gqa_decode_multi n={n}, of the peak", assert_close(got, multi.view(-1, Hq, 128), 1e-2, what=("decode_multi", n)))
    assert_close(got, pp.expected64(case), 1e-2, what=("fp64", n))


def test_random_data_long_prefix():
    """P = 1000, n = 300, G = 4: 21 tiles, 10 query blocks, a prefix that is no multiple of anything"""
    Hq, Hkv = 8, 2
    case = pp.random_case([(1000, 300)], Hq, Hkv, seed=30)
    for page in (16, 256):
        got = run_paged(case, pp.paginate(case, page, seed=31), Hq)
        report(f"random data P=1000 n=300 page={page}, of the peak", assert_close(got, pp.expected64(case), 1e-2, what=("random", page)))


def test_backend_refuses_what_is_not_implemented():
    from chitu_amd.ops import GQA_KV_FP8_ROW

    be = backend(8)
    q = torch.zeros(4, 8, 128, dtype=torch.bfloat16, device="cuda")
    cu = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    lens = torch.tensor([4], dtype=torch.int32, device="cuda")
    table = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    fp8 = torch.zeros(2, 16, 2, GQA_KV_FP8_ROW, dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError):
        be.attn_varlen_with_kvcache(q, fp8, fp8, cu, lens, table, 4)
    bf = torch.zeros(2, 16, 2, 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(NotImplementedError):
        be.attn_varlen_with_kvcache(q, bf, bf, cu, lens, table, 4, causal=False)
    with pytest.raises(NotImplementedError):
        be.attn_varlen_with_kvcache(q, bf, bf, cu, lens, table, 4, causal=False, window_size=(3, 2))
    with pytest.raises(ValueError):
        be.attn_varlen_with_kvcache(q, bf, bf, cu, lens, table, 4, softcap=-1.0)
    assert not bool(be.attn_varlen_with_kvcache(q, bf, bf, cu, lens, table, 4, causal=False, window_size=(3, 0)).any())


# ---------------------------------------------------------------- the model
PROMPT_LENS = (21, 70, 45)
HEAD_LENS = (5, 33, 17)  # the split points: inside a page, one past a page boundary, one past another
PAGE = 16


def tiny(Hq, Hkv, sliding_window=None):
    """(model, cache), built once per shape; whatever an earlier test left in the cache is released"""
    model, cache = _tiny(Hq, Hkv, sliding_window)
    release(cache)
    return model, cache


@functools.lru_cache(maxsize=None)
def _tiny(Hq, Hkv, sliding_window):
    """2 layers, head_dim 128 (dim = 128 Hq), vocab 512, block size 16"""
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.llama import LlamaArgs, LlamaDecoder, init_synthetic_

    args = LlamaArgs(dim=128 * Hq, n_layers=2, n_heads=Hq, n_kv_heads=Hkv, vocab_size=512, ffn_dim=512, sliding_window=sliding_window)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=8, block_size=PAGE, max_seq_len=256, device="cuda",
                                n_local_kv_heads=Hkv, head_dim=128, dtype=torch.bfloat16)
    model = LlamaDecoder(args, cache, HipAttnBackend(local_n_heads=Hq, max_seq_len=256), max_position_embeddings=256, device="cuda")
    init_synthetic_(model, seed=0)
    return model, cache


def prompts_of(vocab, lens=PROMPT_LENS, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lens]


def rows_of(cache, req, count):
    """[2, layers, count, Hkv, 128]: the first `count` K and V rows of a request, in token order"""
    out = []
    for c in (cache.paged_k_cache, cache.paged_v_cache):
        pages = torch.tensor(cache.block_table[req], device=c.device)
        out.append(c[:, pages].flatten(1, 2)[:, :count])
    return torch.stack(out)


def release(cache):
    for r in list(cache.seq_lens):
        cache.finalize_cache_all_decode(r)
    assert len(cache.free_blocks) == cache.num_blocks


def compare_with_whole(model, cache, prompts, whole_logits, reqs_whole, got_logits, reqs_got, tag, elementwise=True):
    """logits within 3e-2 and every layer's K / V rows within 1e-2 of the peak.  elementwise: also tests.util.assert_close's
    per-element form (1 % of the element + 0.5 % of the peak), which the bf16 Llama stack meets.  Mixtral's experts quantise their
    input to int8 per token: a bf16 value that the GEMMs' other row count rounds the other way can flip a code, which moves single
    elements of the next layer's rows by more than their own 1 % while staying inside 1 % of the peak -- the case
    assert_close_elementwise's outlier_frac describes; there the bar is the peak norm alone, as in tests/test_gpu_mixtral.py."""
    report(f"{tag}: last-token logits, of the peak", assert_close(got_logits, whole_logits, 3e-2, what=(tag, "logits")))
    for a, b, p in zip(reqs_whole, reqs_got, prompts):
        assert cache.seq_lens[a] == cache.seq_lens[b] == len(p) and len(cache.block_table[a]) == len(cache.block_table[b]) == -(-len(p) // cache.block_size)
        ra, rb = rows_of(cache, a, len(p)), rows_of(cache, b, len(p))
        for layer in range(ra.shape[1]):
            for i, name in enumerate("KV"):
                if elementwise:
                    assert_close(rb[i, layer], ra[i, layer], 1e-2, what=(tag, b, name, layer))
                else:
                    err = max_rel_to_peak(rb[i, layer], ra[i, layer])
                    print(f"PREFILL_PAGED {tag} {b} {name} layer {layer}: max_rel_to_peak {err:.3e}")
                    assert err < 1e-2, (tag, b, name, layer, err)


def split_test(model, cache, tag):
    vocab = model.args.vocab_size
    prompts = prompts_of(vocab)
    A, B = ["a0", "a1", "a2"], ["b0", "b1", "b2"]
    whole = model.prefill(prompts, A).clone()
    model.prefill([p[:h] for p, h in zip(prompts, HEAD_LENS)], B)
    got = model.prefill_continue([p[h:] for p, h in zip(prompts, HEAD_LENS)], B)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, vocab) and bool(torch.isfinite(got).all())
    compare_with_whole(model, cache, prompts, whole, A, got, B, tag)
    release(cache)


@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (4, 4)])
def test_prefill_of_a_head_then_prefill_continue_of_the_tail_is_the_whole_prefill(Hq, Hkv):
    split_test(*tiny(Hq, Hkv), f"split Hq={Hq} Hkv={Hkv}")


def test_split_prefill_under_a_sliding_window():
    split_test(*tiny(2, 1, 24), "split sliding_window=24")


@pytest.mark.parametrize("chunk", [7, 16, 64, 100])
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (4, 4)])
def test_chunked_prefill_is_the_whole_prefill(Hq, Hkv, chunk):
    """chunk sizes below, at and above the block size and longer than every prompt; requests leave the rounds as they run out"""
    model, cache = tiny(Hq, Hkv)
    prompts = prompts_of(model.args.vocab_size)
    A, C = ["a0", "a1", "a2"], ["c0", "c1", "c2"]
    whole = model.prefill(prompts, A).clone()
    got = model.prefill(prompts, C, chunk_size=chunk)
    compare_with_whole(model, cache, prompts, whole, A, got, C, f"chunk_size={chunk} Hq={Hq} Hkv={Hkv}")
    release(cache)


def test_generate_with_chunked_prefill_returns_its_pages():
    model, cache = tiny(2, 1)
    prompts = prompts_of(model.args.vocab_size)
    free = len(cache.free_blocks)
    out = model.generate(prompts, 4, use_graph=False, prefill_chunk_size=7)
    assert tuple(out.shape) == (3, 4) and out.dtype == torch.int64 and len(cache.free_blocks) == free and not cache.seq_lens


def test_prefill_continue_of_three_tokens_against_decode_multi():
    model, cache = tiny(2, 1)
    vocab = model.args.vocab_size
    prompts = prompts_of(vocab)
    A, B = ["a0", "a1", "a2"], ["b0", "b1", "b2"]
    model.prefill(prompts, A)
    model.prefill(prompts, B)
    tokens = torch.randint(0, vocab, (3, 3), generator=torch.Generator().manual_seed(9))
    got = model.prefill_continue(tokens.tolist(), A)
    cache.prepare_block_table_for_decode_multi(B, 3)
    multi = model.decode_multi(tokens.cuda(), use_graph=False)[:, -1]
    cache.finalize_cache_multi_decode(B, [3, 3, 3])
    report("prefill_continue of 3 tokens against decode_multi, of the peak", assert_close(got, multi, 3e-2, what="decode_multi"))
    for a, b, p in zip(A, B, prompts):
        assert cache.seq_lens[a] == cache.seq_lens[b] == len(p) + 3 and len(cache.block_table[a]) == len(cache.block_table[b])
        assert_close(rows_of(cache, a, len(p) + 3), rows_of(cache, b, len(p) + 3), 1e-2, what=("rows", a))
    release(cache)


def test_prefill_continue_checks_its_requests_before_it_changes_anything():
    model, cache = tiny(2, 1)
    prompts = prompts_of(model.args.vocab_size)
    model.prefill(prompts, ["a0", "a1", "a2"])
    state = (dict(cache.seq_lens), len(cache.free_blocks))
    with pytest.raises(AssertionError, match="max_position_embeddings"):
        model.prefill_continue([[1] * 4, [1] * 200], ["a0", "a1"])  # 70 + 200 > 256
    with pytest.raises(KeyError):
        model.prefill_continue([[1, 2]], ["nobody"])
    assert (dict(cache.seq_lens), len(cache.free_blocks)) == state
    release(cache)


def test_mixtral_split_prefill():
    from tests.test_gpu_mixtral import build

    args, model, cache = build()
    prompts = prompts_of(args.vocab_size, lens=(21, 300, 45))
    heads = (5, 257, 17)
    A, B = ["a0", "a1", "a2"], ["b0", "b1", "b2"]
    whole = model.prefill(prompts, A).clone()
    model.prefill([p[:h] for p, h in zip(prompts, heads)], B)
    got = model.prefill_continue([p[h:] for p, h in zip(prompts, heads)], B)
    compare_with_whole(model, cache, prompts, whole, A, got, B, "mixtral split", elementwise=False)


def test_fp8_cache_is_refused_before_any_cache_state_changes():
    from tests.test_gpu_llama_multi import build_variant

    model, cache = build_variant("fp8")
    prompts = prompts_of(model.args.vocab_size)
    model.prefill(prompts, ["a0", "a1", "a2"])
    state = (dict(cache.seq_lens), len(cache.free_blocks), {r: list(b) for r, b in cache.block_table.items()})
    with pytest.raises(NotImplementedError):
        model.prefill_continue([[1, 2, 3]], ["a0"])
    with pytest.raises(NotImplementedError):
        model.prefill(prompts, ["c0", "c1", "c2"], chunk_size=16)
    with pytest.raises(NotImplementedError):
        model.generate(prompts, 2, prefill_chunk_size=16)
    assert (dict(cache.seq_lens), len(cache.free_blocks), {r: list(b) for r, b in cache.block_table.items()}) == state
