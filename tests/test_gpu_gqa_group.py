"""The flash GQA prefill at group sizes that do not divide 32 (chitu_ext4_gqa_prefill / chitu_ext4_gqa_prefill_paged through
HipAttnBackend) on the GPU: G = 3, 5, 7 and 12 (and 24, the run-time-G instantiation) against the closed forms of
tests/attn_exact.py, tests/attn_paged_prefill_ref.py and tests/attn_group_ref.py, against the old entries and the contiguous
kernel bit for bit where they must agree, against the fp64 attention under a window and a cap and on random data, against the
composition from the decode kernel; then LlamaDecoder at 6 / 2 and 5 / 1 heads and a G = 5 Qwen3 from Hugging Face's fp32 run
(tests/golden/qwen3_g5_hf.npz)."""
import gc

import numpy as np
import pytest
import torch

from tests import attn_exact as ax
from tests import attn_group_ref as gr
from tests import attn_paged_prefill_ref as pp
from tests import attn_window_ref as wr
from tests import qwen3_ref as qr
from tests.test_gpu_prefill_paged import (HEAD_LENS, compare_with_whole, prompts_of, release, rows_of, run_contiguous, run_paged,
                                          split_test, tiny, whole_case)
from tests.util import assert_close, max_rel_to_peak

pytestmark = pytest.mark.gpu

GROUPS = gr.GROUPS


def backend(Hq):
    from chitu_amd.attn_backend import HipAttnBackend

    return HipAttnBackend(local_n_heads=Hq)


def report(what, err):
    print(f"GQA_GROUP {what}: {err:.3e}")


def contiguous(case, Hq, W=-1, c=0.0, strided=False):
    """the contiguous kernel on a case of tests/attn_exact.py (q, k, v, cu)"""
    q, k, v = (case[n].to(torch.bfloat16).cuda() for n in ("q", "k", "v"))
    if strided:  # the slices of one merged qkv projection output
        Hkv = k.shape[1]
        qkv = torch.cat([q, k, v], dim=1)
        q, k, v = qkv[:, :Hq], qkv[:, Hq : Hq + Hkv], qkv[:, Hq + Hkv :]
        assert not q.is_contiguous()
    cu = torch.tensor(case["cu"], dtype=torch.int32).cuda()
    m = max(b - a for a, b in zip(case["cu"][:-1], case["cu"][1:]))
    return backend(Hq).attn_varlen_func(q, k, v, cu, cu, m, m, causal=True, window_size=(W, 0) if W >= 0 else (-1, -1), softcap=c,
                                        softmax_scale=case.get("scale", ax.GQA_SCALE))


def behind_a_prefix(case, prefix_of):
    """a case of tests/attn_exact.py as one of tests/attn_paged_prefill_ref.py: sequence s keeps the queries (and expected rows)
    behind its first prefix_of(L) keys"""
    cu = case["cu"]
    prefixes = [prefix_of(s1 - s0) for s0, s1 in zip(cu[:-1], cu[1:])]
    rows = torch.cat([torch.arange(s0 + P, s1) for (s0, s1), P in zip(zip(cu[:-1], cu[1:]), prefixes)])
    return dict(q=case["q"][rows], K=[case["k"][s0:s1] for s0, s1 in zip(cu[:-1], cu[1:])],
                V=[case["v"][s0:s1] for s0, s1 in zip(cu[:-1], cu[1:])], prefixes=prefixes,
                news=[s1 - s0 - P for (s0, s1), P in zip(zip(cu[:-1], cu[1:]), prefixes)], want=case["want"][rows])


# ---------------------------------------------------------------- 1. counting and dominant keys
@pytest.mark.parametrize("Hq,Hkv", GROUPS)
def test_contiguous_kernel_counts_its_keys_and_keeps_every_head_with_its_token(Hq, Hkv):
    """Sequence lengths of attn_exact.PREFILL_SEQS and around one and two workgroups' 128 // G tokens.  Counting: row i is the
    mean of exactly i + 1 V rows.  Dominant keys, one query per token and one per (token, head): the tied keys' rows."""
    seqs = gr.seqs_for(Hq // Hkv)
    count = ax.prefill_count_case(seqs, Hq, Hkv, 128, ax.P_GQA)
    tied = ax.prefill_dominant_case(seqs, Hq, Hkv, 128)
    heads = gr.group_dominant_case(seqs, Hq, Hkv)
    for strided in (False, True):
        tag = f"contiguous{' strided' if strided else ''} Hq={Hq} Hkv={Hkv}"
        report(f"{tag} counting, relative", ax.check_count(contiguous(count, Hq, strided=strided), count["want"]))
        report(f"{tag} tied dominant keys, relative", ax.check_tied(contiguous(tied, Hq, strided=strided), tied["want"]))
        report(f"{tag} a key per head, relative", ax.check_tied(contiguous(heads, Hq, strided=strided), heads["want"]))


@pytest.mark.parametrize("page", [16, 48])
@pytest.mark.parametrize("Hq,Hkv", GROUPS)
def test_paged_kernel_counts_its_keys_and_returns_the_probed_keys_row(Hq, Hkv, page):
    """tests/test_gpu_prefill_paged.py's ragged launch (9 prefixes x 5 new lengths) at these group sizes, and a key per head
    behind prefixes of 0 and of a third of each sequence."""
    count = pp.count_case(pp.pairs(), Hq, Hkv)
    report(f"paged counting Hq={Hq} Hkv={Hkv} page={page}, relative",
           ax.check_count(run_paged(count, pp.paginate(count, page, seed=1), Hq), count["want"]))
    dom = pp.dominant_case(pp.pairs(), Hq, Hkv, page)
    report(f"paged dominant keys Hq={Hq} Hkv={Hkv} page={page}, absolute",
           ax.check_dominant(run_paged(dom, pp.paginate(dom, page, seed=2, v_fill=15.0), Hq), dom["want"]))
    heads = gr.group_dominant_case(gr.seqs_for(Hq // Hkv), Hq, Hkv)
    for name, prefix_of in (("prefix 0", lambda L: 0), ("prefix L // 3", lambda L: L // 3)):
        case = behind_a_prefix(heads, prefix_of)
        got = run_paged(case, pp.paginate(case, page, seed=3, v_fill=15.0), Hq)
        report(f"paged a key per head, {name} Hq={Hq} Hkv={Hkv} page={page}, relative", ax.check_tied(got, case["want"]))


# ---------------------------------------------------------------- 2. bit identities
def _contig_args(q, k, v, cu, m, Hq, Hkv):
    from chitu_amd._lib import f32, i32, i64, ptr

    out = torch.empty_like(q)
    return out, (ptr(q), i64(q.stride(0)), i64(q.stride(1)), ptr(k), i64(k.stride(0)), i64(k.stride(1)), ptr(v), i64(v.stride(0)),
                 i64(v.stride(1)), ptr(cu), i32(cu.numel() - 1), i32(m), f32(ax.GQA_SCALE), ptr(out), i32(Hq), i32(Hkv), i32(128))


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (8, 1)])
def test_at_a_power_of_two_the_new_entries_are_the_old_ones_bit_for_bit(Hq, Hkv):
    from chitu_amd import _lib
    from chitu_amd._lib import check, f32, i32, i64, ptr, stream_ptr

    lib = _lib.lib()
    seqs = ax.PREFILL_SEQS
    g = torch.Generator().manual_seed(Hq + Hkv)
    T = sum(seqs)
    q = (torch.randn(T, Hq, 128, generator=g) * 0.5).to(torch.bfloat16).cuda()
    k, v = (torch.randn(T, Hkv, 128, generator=g).to(torch.bfloat16).cuda() for _ in range(2))
    cu = torch.tensor(ax.cu_of(seqs), dtype=torch.int32).cuda()
    for W, c in ((-1, 0.0), (5, 0.0), (64, 5.0), (-1, 5.0)):
        old, a = _contig_args(q, k, v, cu, max(seqs), Hq, Hkv)
        if W < 0 and c == 0.0:
            check(lib.chitu_hip_gqa_prefill(*a, stream_ptr()), "old")
        else:
            check(lib.chitu_hip_gqa_prefill_window(*a, i32(W), f32(c), stream_ptr()), "old")
        new, a = _contig_args(q, k, v, cu, max(seqs), Hq, Hkv)
        check(lib.chitu_ext4_gqa_prefill(*a, i32(W), f32(c), stream_ptr()), "new")
        assert torch.equal(new, old) and bool(torch.isfinite(new).all()), (W, c)
    case = pp.random_case(pp.pairs(), Hq, Hkv, seed=11)
    kc, vc, table, lens = (t.cuda() for t in pp.paginate(case, 16, seed=12))
    qq = case["q"].to(torch.bfloat16).cuda()
    cuq = torch.tensor(pp.cu_q(case), dtype=torch.int32).cuda()
    for W, c in ((-1, 0.0), (5, 5.0)):
        outs = []
        for entry in (lib.chitu_hip_gqa_prefill_paged, lib.chitu_ext4_gqa_prefill_paged):
            out = torch.empty_like(qq)
            check(entry(ptr(qq), i64(qq.stride(0)), i64(qq.stride(1)), ptr(kc), ptr(vc), i64(kc.shape[0]), i32(kc.shape[1]), i32(Hkv),
                        ptr(table), i32(table.stride(0)), ptr(cuq), ptr(lens), i32(lens.numel()), i32(max(case["news"])),
                        f32(ax.GQA_SCALE), ptr(out), i32(Hq), i32(128), i32(W), f32(c), stream_ptr()), "paged")
            outs.append(out)
        assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all()), (W, c)
        assert_close(outs[1], pp.expected64(case, W=W, c=c), 1e-2, what=("paged", W, c))


@pytest.mark.parametrize("Hq,Hkv", GROUPS)
def test_prefix_0_is_the_contiguous_kernel_bit_for_bit_under_any_block_table(Hq, Hkv):
    case = whole_case([(0, L) for L in gr.seqs_for(Hq // Hkv)], Hq, Hkv, seed=Hq)
    want = run_contiguous(case, Hq)
    for seed, page in ((0, 16), (1, 48)):
        got = run_paged(case, pp.paginate(case, page, seed=seed), Hq)
        assert torch.equal(got, want), (seed, max_rel_to_peak(got, want))
    assert_close(want, pp.expected64(case), 1e-2, what="the contiguous kernel itself")


@pytest.mark.parametrize("Hq,Hkv,prefixes", [(6, 2, (42, 126)), (5, 1, (25, 100)), (7, 1, (18, 126))])
def test_prefix_multiple_of_the_token_block_is_rows_of_the_whole_sequence_call_bit_for_bit(Hq, Hkv, prefixes):
    """P a multiple of 128 // G: the paged kernel's workgroups hold the rows of the contiguous kernel's workgroups P / BQ ..,
    padding rows included, so the wave-wide rescale vote sees the same rows."""
    assert all(P % gr.block_tokens(Hq // Hkv) == 0 for P in prefixes)
    seq_pairs = [(P, n) for P in prefixes for n in (1, 33, 129)]
    case = whole_case(seq_pairs, Hq, Hkv, seed=7 + Hq)
    whole = run_contiguous(case, Hq)
    cu = ax.cu_of([P + n for P, n in seq_pairs])
    want = torch.cat([whole[cu[s] + P : cu[s + 1]] for s, (P, _) in enumerate(seq_pairs)])
    for page in (16, 256):
        got = run_paged(case, pp.paginate(case, page, seed=3), Hq)
        assert torch.equal(got, want), (page, max_rel_to_peak(got, want))


# ---------------------------------------------------------------- 3. window and cap
@pytest.mark.parametrize("c", [0.0, 5.0])
@pytest.mark.parametrize("W", [0, 5, 64, 100])
@pytest.mark.parametrize("Hq,Hkv", [(6, 2), (5, 1)])
def test_window_and_cap_against_the_fp64_attention(Hq, Hkv, W, c):
    seqs = gr.seqs_for(Hq // Hkv)
    g = torch.Generator().manual_seed(W + Hq)
    T = sum(seqs)
    case = dict(q=(torch.randn(T, Hq, 128, generator=g) * 0.5).to(torch.bfloat16).float(),
                k=(torch.randn(T, Hkv, 128, generator=g) * 4.0).to(torch.bfloat16).float(),  # scores of several nats: the cap matters
                v=torch.randn(T, Hkv, 128, generator=g).to(torch.bfloat16).float(), cu=ax.cu_of(seqs))
    want = wr.prefill64_window(case["q"], case["k"], case["v"], case["cu"], ax.GQA_SCALE, W, c)
    report(f"contiguous window W={W} cap={c} Hq={Hq}, of the peak", assert_close(contiguous(case, Hq, W, c), want, 1e-2, what=(W, c)))
    paged = pp.random_case(pp.pairs(), Hq, Hkv, seed=8)
    for x in paged["K"]:
        x *= 4.0
    got = run_paged(paged, pp.paginate(paged, 16, seed=9), Hq, W, c)
    report(f"paged window W={W} cap={c} Hq={Hq}, of the peak", assert_close(got, pp.expected64(paged, W=W, c=c), 1e-2, what=("paged", W, c)))


@pytest.mark.parametrize("W", [0, 5, 64, 100])
def test_window_counts_exactly_its_keys_over_poisoned_pages(W):
    Hq, Hkv = 5, 1
    count = pp.count_case(pp.pairs(), Hq, Hkv)
    for page in (16, 48):
        pages = pp.paginate(count, page, seed=page, dead_before=pp.lowest_visible(count, W), poison_fill=float("nan"))
        report(f"window counting W={W} page={page}, relative",
               ax.check_count(run_paged(count, pages, Hq, W), pp.count_want_window(count, Hq, W)))
    flat = ax.prefill_count_case(gr.seqs_for(5), Hq, Hkv, 128, ax.P_GQA)
    report(f"contiguous window counting W={W}, relative", ax.check_count(contiguous(flat, Hq, W), wr.prefill_count_want(flat, Hq, W)))


@pytest.mark.parametrize("Hq,Hkv", GROUPS)
def test_queries_before_the_first_key_give_zeros(Hq, Hkv):
    """L < n: the first n - L queries sit at negative positions (and a sequence of 0 keys has only such queries)"""
    case = pp.random_case([(-3, 5), (0, 4), (-1, 1), (-140, 200)], Hq, Hkv, seed=4)
    got = run_paged(case, pp.paginate(case, 16, seed=4, poison_fill=float("nan")), Hq).float().cpu()
    want = pp.expected64(case)
    dead = torch.tensor([P + i < 0 for P, n in zip(case["prefixes"], case["news"]) for i in range(n)])
    assert int(dead.sum()) == 3 + 1 + 140 and not bool(got[dead].any()) and not bool(want[dead].any())
    assert_close(got[~dead], want[~dead], 1e-2, what="rows behind the queries at negative positions")


# ---------------------------------------------------------------- 4. random data
RANDOM_SEQS = [1, 2, 31, 33, 127, 129, 300, 700]


def random_flat(Hq, Hkv):
    """tests/test_gpu_gqa.py's data: a spiked key that forces the rescale branch late in the last sequence"""
    g = torch.Generator().manual_seed(Hq * 7 + Hkv)
    T = sum(RANDOM_SEQS)
    q = (torch.randn(T, Hq, 128, generator=g) * 0.5).to(torch.bfloat16)
    k = torch.randn(T, Hkv, 128, generator=g).to(torch.bfloat16)
    v = torch.randn(T, Hkv, 128, generator=g).to(torch.bfloat16)
    k[T - 40, 0] = (q[T - 3, 0].float() * 4).to(torch.bfloat16)  # q . k ~ 4 |q|^2 = 128: towers over the row's other scores
    return q, k, v, torch.tensor([0] + list(np.cumsum(RANDOM_SEQS)), dtype=torch.int32)


@pytest.mark.parametrize("Hq,Hkv", GROUPS)
def test_random_data_against_the_oracle_the_composition_and_strided_views(Hq, Hkv, monkeypatch):
    from oracle import gqa as ogqa

    q, k, v, cu = random_flat(Hq, Hkv)
    be, m = backend(Hq), max(RANDOM_SEQS)
    outs = {}
    for mode in ("flash", "compose"):
        monkeypatch.setenv("CHITU_GQA_PREFILL", mode)
        outs[mode] = be.attn_varlen_func(q.cuda(), k.cuda(), v.cuda(), cu.cuda(), cu.cuda(), m, m, causal=True).cpu()
    assert bool(torch.isfinite(outs["flash"]).all())
    report(f"flash vs oracle Hq={Hq} Hkv={Hkv}, of the peak",
           assert_close(outs["flash"], ogqa.attn_varlen_causal(q, k, v, cu), 1e-2, what=("flash vs oracle", Hq, Hkv)))
    report(f"flash vs composition Hq={Hq} Hkv={Hkv}, of the peak",
           assert_close(outs["flash"], outs["compose"], 1e-2, what=("flash vs composition", Hq, Hkv)))
    monkeypatch.setenv("CHITU_GQA_PREFILL", "flash")
    qkv = torch.cat([q, k, v], dim=1).cuda()
    qs, ks, vs = qkv[:, :Hq], qkv[:, Hq : Hq + Hkv], qkv[:, Hq + Hkv :]
    assert not qs.is_contiguous()
    assert torch.equal(be.attn_varlen_func(qs, ks, vs, cu.cuda(), cu.cuda(), m, m, causal=True).cpu(), outs["flash"])


@pytest.mark.parametrize("Hq,Hkv", [(24, 1), (12, 2), (11, 1)])
def test_group_sizes_beside_the_swept_ones(Hq, Hkv):
    """G = 24 has no instantiation of its own (the run-time-G kernel; 5 query tokens and 8 padding rows in a workgroup), and the
    composition cannot run it (the decode kernels stop at G = 16): fp64 only.  G = 6 is the compiled size GROUPS leaves out, G = 11
    the run-time-G kernel with a token's heads across two waves and 7 padding rows."""
    q, k, v, cu = random_flat(Hq, Hkv)
    m = max(RANDOM_SEQS)
    got = backend(Hq).attn_varlen_func(q.cuda(), k.cuda(), v.cuda(), cu.cuda(), cu.cuda(), m, m, causal=True).cpu()
    want = ax.prefill64(q.float(), k.float(), v.float(), cu.tolist(), ax.GQA_SCALE)
    G = Hq // Hkv
    report(f"G={G} flash vs fp64, of the peak", assert_close(got, want, 1e-2, what=("flash", G)))
    heads = gr.group_dominant_case(gr.seqs_for(G), Hq, Hkv)
    report(f"G={G} a key per head, relative", ax.check_tied(contiguous(heads, Hq), heads["want"]))
    count = pp.count_case(pp.pairs(), Hq, Hkv)
    report(f"G={G} paged counting, relative", ax.check_count(run_paged(count, pp.paginate(count, 16, seed=1), Hq), count["want"]))
    case = pp.random_case(pp.pairs(), Hq, Hkv, seed=24)
    got = run_paged(case, pp.paginate(case, 16, seed=24), Hq)
    report(f"G={G} paged vs fp64, of the peak", assert_close(got, pp.expected64(case), 1e-2, what=("paged", G)))


# ---------------------------------------------------------------- 5. models
@pytest.fixture(autouse=True)
def models_are_gone_after_each_test():
    yield
    gc.collect()


@pytest.mark.parametrize("Hq,Hkv,window", [(6, 2, None), (5, 1, None), (6, 2, 24)])
def test_prefill_of_a_head_then_prefill_continue_of_the_tail_is_the_whole_prefill(Hq, Hkv, window):
    split_test(*tiny(Hq, Hkv, window), f"split Hq={Hq} Hkv={Hkv} sliding_window={window}")


@pytest.mark.parametrize("chunk", [7, 64])
@pytest.mark.parametrize("Hq,Hkv", [(6, 2), (5, 1)])
def test_chunked_prefill_is_the_whole_prefill(Hq, Hkv, chunk):
    model, cache = tiny(Hq, Hkv)
    prompts = prompts_of(model.args.vocab_size)
    A, C = ["a0", "a1", "a2"], ["c0", "c1", "c2"]
    whole = model.prefill(prompts, A).clone()
    got = model.prefill(prompts, C, chunk_size=chunk)
    compare_with_whole(model, cache, prompts, whole, A, got, C, f"chunk_size={chunk} Hq={Hq} Hkv={Hkv}")
    release(cache)


@pytest.mark.parametrize("Hq,Hkv", [(6, 2), (5, 1)])
def test_prefill_continue_of_three_tokens_against_decode_multi(Hq, Hkv):
    model, cache = tiny(Hq, Hkv)
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
    report(f"prefill_continue of 3 tokens against decode_multi Hq={Hq}, of the peak", assert_close(got, multi, 3e-2, what="decode_multi"))
    for a, b, p in zip(A, B, prompts):
        assert cache.seq_lens[a] == cache.seq_lens[b] == len(p) + 3 and len(cache.block_table[a]) == len(cache.block_table[b])
        assert_close(rows_of(cache, a, len(p) + 3), rows_of(cache, b, len(p) + 3), 1e-2, what=("rows", a))
    release(cache)


PAGE = 16


def g5_model(tmp_path, max_reqs=8):
    """A Qwen3Decoder of the G = 5 fixture's shape (hidden 256, 5 / 1 heads of 128), its parameters regenerated from the seed,
    written as an HF-named safetensors directory and loaded by load_checkpoint_hf_llama"""
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.checkpoint import load_checkpoint_hf_llama
    from chitu_amd.qwen3 import Qwen3Decoder

    g, cfg, hf = gr.qwen3_g5_fixture()
    args = qr.qwen3_args(cfg)
    assert args.n_heads // args.n_kv_heads == 5
    path = qr.write_hf_dir(hf, str(tmp_path / "qwen3_g5"))
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=max_reqs, block_size=PAGE, max_seq_len=256, device="cuda",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=torch.bfloat16)
    model = Qwen3Decoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=256), max_position_embeddings=256, device="cuda")
    load_checkpoint_hf_llama(model, path)
    return g, model, cache


def test_g5_qwen3_hf_checkpoint_reproduces_the_hf_fp32_run(tmp_path):
    """Prefill of the prompt (chitu_ext4_gqa_prefill), then 32 decode steps fed the fixture's tokens, as one hipGraph replay per
    step and as eager launches."""
    g, model, cache = g5_model(tmp_path, max_reqs=2)
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    k0 = torch.from_numpy(g["k0_fp32"])

    def run(req, use_graph):
        rows = [model.prefill([prompt], [req]).float().cpu()]
        for step in range(32):
            cache.prepare_cache_decode([req])
            cache.prepare_block_table_for_decode([req])
            tok = torch.tensor([toks[step]], dtype=torch.int64, device="cuda")
            rows.append(model.decode(tok, use_graph=use_graph).float().cpu())
            cache.finalize_cache_single_decode([req])
        assert cache.seq_lens[req] == len(prompt) + 32 == k0.shape[0]
        k_rows = rows_of(cache, req, k0.shape[0])[0, 0].float().cpu()  # K, layer 0
        cache.finalize_cache_all_decode(req)
        return torch.cat(rows), k_rows

    (graph, k_graph), (eager, k_eager) = run("g", True), run("e", False)
    qr.check_logits(eager, g, "G = 5 HIP eager vs HF fp32")
    qr.check_logits(graph, g, "G = 5 HIP graph vs HF fp32")
    assert torch.equal(graph, eager) and torch.equal(k_graph, k_eager)
    report("G = 5 Qwen3 layer-0 K page rows vs HF fp32", assert_close(k_eager, k0, 1e-2, what="layer 0 K page rows"))


def test_g5_qwen3_continued_and_chunked_prefill_are_the_whole_prefill(tmp_path):
    g, model, cache = g5_model(tmp_path)
    prompts = prompts_of(model.args.vocab_size)
    A, B, C = ["a0", "a1", "a2"], ["b0", "b1", "b2"], ["c0", "c1", "c2"]
    whole = model.prefill(prompts, A).clone()
    model.prefill([p[:h] for p, h in zip(prompts, HEAD_LENS)], B)
    got = model.prefill_continue([p[h:] for p, h in zip(prompts, HEAD_LENS)], B)
    compare_with_whole(model, cache, prompts, whole, A, got, B, "G = 5 qwen3 split")
    got = model.prefill(prompts, C, chunk_size=7)
    compare_with_whole(model, cache, prompts, whole, A, got, C, "G = 5 qwen3 chunk_size=7")
    release(cache)
