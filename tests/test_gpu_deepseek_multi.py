"""DeepSeekV3Decoder.decode_multi (T tokens per sequence in one step over the MLA latent cache, the verify step of speculative
decoding) and DeepSeekV3Decoder.generate_speculative on the GPU, mirroring tests/test_gpu_llama_multi.py: the multi-token step
against T sequential single-token steps, graph replay against the eager step, the fused small-batch launches at bs = 1, and greedy
draft-and-verify generation against plain greedy generation.  Models: the two tiny configurations of tests/test_gpu_deepseek.py
(with and without a q low-rank path), each with a bf16 and an fp8 latent cache."""
import dataclasses

import pytest
import torch

from tests.test_gpu_deepseek import tiny_args, v2lite_like_args
from tests.test_gpu_llama_multi import ReplayDrafter, plain_greedy_with_gaps
from tests.test_gpu_mla_kv_fp8 import build
from tests.util import assert_close, max_rel_to_peak

pytestmark = pytest.mark.gpu

PROMPT_LENS = (5, 63, 33)  # the second one ends one row short of its page: the step's rows fill it and open the next
REQS_A, REQS_B = ["a0", "a1", "a2"], ["b0", "b1", "b2"]
MAKE_ARGS = {"v3_like": tiny_args, "v2lite_like": v2lite_like_args}
LOGITS_BAR, ROWS_BAR = 3e-2, 1e-2  # tests/test_gpu_llama_multi.py's bars


def build_variant(arch, fmt, max_reqs=8):
    return build(dataclasses.replace(MAKE_ARGS[arch](), kv_cache_dtype=fmt), max_reqs=max_reqs)


def prompts_of(vocab, seed=3, lens=PROMPT_LENS):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lens]


def cached_rows(cache, req, first, count):
    """[layers, count, 576] bf16: the rows first .. first + count - 1 of a request in token order (an fp8 cache: dequantised)"""
    from chitu_amd import ops

    out = []
    for layer in range(cache.paged_kv_cache.shape[0]):
        c = cache.get_paged_kv_cache(layer)
        rows = torch.cat([c[blk] for blk in cache.block_table[req]])[first : first + count].contiguous()
        out.append(ops.mla_kv_dequant_fp8(rows) if rows.dtype == torch.uint8 else rows)
    return torch.stack(out)


@pytest.fixture(params=["multi", "rule"])
def route(request, monkeypatch):
    """"multi": the attention of a multi-token step is always the pair kernel (the routing threshold set to 0); "rule": the
    backend's measured rule decides, which for models this small means the single-token kernel on the expanded rows"""
    from chitu_amd import attn_backend

    if request.param == "multi":
        monkeypatch.setattr(attn_backend, "MLA_MULTI_MIN_TILE_STEPS_PER_CU", 0.0)
    return request.param


def attention_entry(route, fmt):
    return "chitu_hip_mla_decode" + ("_multi" if route == "multi" else "") + ("_kv_fp8" if fmt == "fp8" else "")


def snapshot(cache):
    return cache.paged_kv_cache.clone()


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("arch", list(MAKE_ARGS))
@pytest.mark.parametrize("T", [2, 4])
def test_one_multi_token_step_is_T_single_token_steps(T, arch, fmt, route):
    """after a ragged prefill: decode_multi over tokens [bs, T] on one set of requests against T sequential decode steps on a
    second, identically prepared set.  Logits per position at 3e-2 of the peak, the T appended rows of every layer at 1e-2."""
    model, cache = build_variant(arch, fmt)
    vocab = model.args.vocab_size
    prompts = prompts_of(vocab)
    model.prefill(prompts, REQS_A)
    model.prefill(prompts, REQS_B)
    tokens = torch.randint(0, vocab, (len(prompts), T), generator=torch.Generator().manual_seed(T)).cuda()
    cache.prepare_block_table_for_decode_multi(REQS_A, T)
    multi = model.decode_multi(tokens, use_graph=False).clone()
    cache.finalize_cache_multi_decode(REQS_A, [T] * len(prompts))
    assert multi.dtype == torch.float32 and tuple(multi.shape) == (len(prompts), T, vocab) and bool(torch.isfinite(multi).all())
    for t in range(T):
        cache.prepare_cache_decode(REQS_B)
        cache.prepare_block_table_for_decode(REQS_B)
        single = model.decode(tokens[:, t].contiguous(), use_graph=False)
        cache.finalize_cache_single_decode(REQS_B)
        print(f"DEEPSEEK_MULTI {arch} {fmt} T={T} position {t}: logits max_rel_to_peak {max_rel_to_peak(multi[:, t], single):.3e}")
        assert_close(multi[:, t], single, LOGITS_BAR, what=(arch, fmt, T, t))
    for a, b, n in zip(REQS_A, REQS_B, PROMPT_LENS):
        assert cache.seq_lens[a] == cache.seq_lens[b] == n + T and len(cache.block_table[a]) == len(cache.block_table[b])
        ra, rb = cached_rows(cache, a, n, T), cached_rows(cache, b, n, T)
        print(f"DEEPSEEK_MULTI {arch} {fmt} T={T} {a} rows: max_rel_to_peak {max_rel_to_peak(ra, rb):.3e}")
        assert_close(ra, rb, ROWS_BAR, what=(arch, fmt, T, a))


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("arch", list(MAKE_ARGS))
def test_graph_replay_is_the_eager_step_also_after_partial_acceptance(arch, fmt, route):
    """capture_verified checks the first replay against the eager step itself; here the cache and logits of a replay equal those
    of the eager step from the same cache bytes, twice: the second time after finalize kept 1, 3 and 2 of the 4 rows"""
    from chitu_amd import graphs

    model, cache = build_variant(arch, fmt)
    vocab, T = model.args.vocab_size, 4
    model.prefill(prompts_of(vocab), REQS_A)
    g = torch.Generator().manual_seed(11)
    n0 = len(graphs.capture_log)
    for kept in ([1, 3, 2], [4, 4, 4]):
        tokens = torch.randint(0, vocab, (3, T), generator=g).cuda()
        cache.prepare_block_table_for_decode_multi(REQS_A, T)
        snap = snapshot(cache)
        eager = model.decode_multi(tokens, use_graph=False).clone()
        kv_eager = snapshot(cache)
        cache.paged_kv_cache.copy_(snap)
        replay = model.decode_multi(tokens, use_graph=True)
        assert torch.equal(eager, replay) and not torch.equal(snap, cache.paged_kv_cache)
        assert torch.equal(kv_eager, cache.paged_kv_cache)
        cache.paged_kv_cache.copy_(snap)
        assert torch.equal(eager, model.decode_multi(tokens, use_graph=True)) and torch.equal(kv_eager, cache.paged_kv_cache)  # a second replay
        cache.finalize_cache_multi_decode(REQS_A, kept)
    assert [k for k in model.graphs if len(k) == 3] == [(3, T, graphs.graph_mode(True))]  # one capture, replayed on new lengths
    captures = graphs.capture_log[n0:]
    assert captures and all(c["attempts"] == 1 and not c["mismatches"] for c in captures), captures


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("arch", list(MAKE_ARGS))
def test_batch_one_takes_the_fused_small_batch_launches_with_two_tokens(arch, fmt, route):
    """bs = 1, T = 2: two rows, within the row limits of the fused small-batch launches -- with a q low-rank path q_norm + quant +
    wq_b + the KV rows in ONE launch (mla_q_proj) on the multi-token tables, without one the absorb + RoPE + KV launch -- and the
    split merge inside the W_UV projection; the attention is ONE launch per layer: chitu_hip_mla_decode_multi, or under the
    backend's rule (a launch this small) chitu_hip_mla_decode on the two expanded rows.  Eager and graph against
    two sequential single-token steps: the bars of the test above."""
    from chitu_amd import _lib, deepseek_v3

    model, cache = build_variant(arch, fmt)
    vocab, T = model.args.vocab_size, 2
    prompt = prompts_of(vocab)[1:2]  # 63 tokens: the step fills the page and opens the next
    model.prefill(prompt, ["a0"])
    model.prefill(prompt, ["b0"])
    tokens = torch.randint(0, vocab, (1, T), generator=torch.Generator().manual_seed(9)).cuda()
    cache.prepare_block_table_for_decode_multi(["a0"], T)
    snap = snapshot(cache)
    _lib.call_log = []
    try:
        multi = model.decode_multi(tokens, use_graph=False).clone()
        names = [name for name, _ in _lib.call_log]
    finally:
        _lib.call_log = None
    n_layers = model.args.n_layers
    assert [n for n in names if n.startswith("chitu_hip_mla_decode")] == [attention_entry(route, fmt)] * n_layers, names
    assert names.count("chitu_hip_mla_merge_absorb_uv_quant_fp8") + names.count("chitu_hip_mla_merge_absorb_uv_quant_fp8_tm") == n_layers, names
    if arch == "v3_like":
        assert deepseek_v3.FUSE_Q_PROJ and names.count("chitu_hip_mla_q_proj") == n_layers, names
    else:
        assert names.count("chitu_hip_absorb_bmm_rope_kv_fp8") == n_layers, names
    assert names.count("chitu_hip_mla_kv_append_fp8") == (n_layers if fmt == "fp8" else 0), names
    kv_eager = snapshot(cache)
    cache.paged_kv_cache.copy_(snap)
    assert torch.equal(multi, model.decode_multi(tokens, use_graph=True)) and torch.equal(kv_eager, cache.paged_kv_cache)
    cache.finalize_cache_multi_decode(["a0"], [T])
    for t in range(T):
        cache.prepare_cache_decode(["b0"])
        cache.prepare_block_table_for_decode(["b0"])
        single = model.decode(tokens[:, t].contiguous(), use_graph=False)
        cache.finalize_cache_single_decode(["b0"])
        print(f"DEEPSEEK_MULTI fused {arch} {fmt} bs=1 T={T} position {t}: logits max_rel_to_peak {max_rel_to_peak(multi[:, t], single):.3e}")
        assert_close(multi[:, t], single, LOGITS_BAR, what=("fused", arch, fmt, t))
    n = len(prompt[0])
    assert_close(cached_rows(cache, "a0", n, T), cached_rows(cache, "b0", n, T), ROWS_BAR, what=("fused", arch, fmt))


SPEC_SEED, SPEC_NEW, SPEC_DRAFT = 165, 5, 3


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_speculative_generation_gives_the_plain_greedy_tokens(fmt, route):
    """generate_speculative against plain greedy generation, tests/test_gpu_llama_multi.py's scheme, with four drafters: one that
    is always wrong (plain's token + 1: nothing accepted, one token per step), one that proposes the plain run's continuation, one
    that replays the speculative path's OWN output, and NgramDrafter.  Every run's tokens are compared with plain's up to each
    request's first position where the plain path's top-2 logit gap is under 2 * LOGITS_BAR of the peak (there the two paths,
    whose GEMMs run at other row counts, may legitimately pick different tokens); at least half of every request's positions
    must be compared.

    The step counts are exact where they can be.  Always wrong: SPEC_NEW - 1 steps, nothing accepted.  Own output replayed: a
    verify step is deterministic and row t's logits depend on the tokens up to t alone, so every draft is accepted and the run
    takes ceil((SPEC_NEW - 1) / (SPEC_DRAFT + 1)) steps -- a path that accepts nothing fails this.  Plain's continuation: the
    same counts wherever all positions are comparable; in general at least the drafts that lie before each request's first
    narrow gap are accepted.

    SPEC_SEED was chosen on an MI355X from the PLAIN path alone (plain_greedy_with_gaps: prefill + graph-replayed decode steps,
    code the multi-token step does not touch) run over the prompt seeds 0 .. 299 with both cache formats: in this tiny random
    model no seed keeps every gap of 5 new tokens above 6 % of the peak; the seed taken compares the most positions in its worst
    request.  The assertion on the compared share re-checks the choice on every run."""
    from chitu_amd.sampling import NgramDrafter

    assert (SPEC_NEW - 1) % (SPEC_DRAFT + 1) == 0
    model, cache = build_variant("v3_like", fmt)
    vocab = model.args.vocab_size
    prompts = prompts_of(vocab, SPEC_SEED)
    n_req, free_before = len(prompts), len(cache.free_blocks)
    plain, gaps = plain_greedy_with_gaps(model, cache, prompts, SPEC_NEW, REQS_B)
    assert torch.equal(plain, model.generate(prompts, SPEC_NEW)) and len(cache.free_blocks) == free_before
    comparable = (gaps >= 2 * LOGITS_BAR).long().cumprod(dim=1).bool()  # positions before the first narrow gap of each request
    print(f"DEEPSEEK_MULTI speculative {fmt}: plain path top-2 gaps over the peak {gaps.tolist()}; compared {comparable.sum(1).tolist()} of {SPEC_NEW} each")
    assert bool((comparable.sum(1) * 2 >= SPEC_NEW).all())

    def run(drafter, what):
        out = model.generate_speculative(prompts, SPEC_NEW, drafter, SPEC_DRAFT)
        stats = dict(model.speculative_stats)
        again = model.generate_speculative(prompts, SPEC_NEW, drafter, SPEC_DRAFT)
        assert tuple(out.shape) == (n_req, SPEC_NEW) and out.dtype == torch.int64 and torch.equal(out, again)
        assert stats == model.speculative_stats and len(cache.free_blocks) == free_before and not cache.seq_lens
        assert bool((out == plain).cpu()[comparable].all()), (what, out.tolist(), plain.tolist(), gaps.tolist())
        print(f"DEEPSEEK_MULTI speculative {fmt}: {what}: {stats}, equal to plain at {int((out == plain).sum())} of {out.numel()}")
        return out, stats

    own, stats = run(ReplayDrafter(prompts, plain, vocab, wrong=True), "always wrong")
    assert stats == dict(steps=SPEC_NEW - 1, drafted=(SPEC_NEW - 1) * n_req * SPEC_DRAFT, accepted=0), stats
    full = -(-(SPEC_NEW - 1) // (SPEC_DRAFT + 1))
    out, stats = run(ReplayDrafter(prompts, own, vocab, wrong=False), "own output replayed")
    assert torch.equal(out, own) and stats == dict(steps=full, drafted=full * n_req * SPEC_DRAFT, accepted=full * n_req * SPEC_DRAFT), stats
    out, stats = run(ReplayDrafter(prompts, plain, vocab, wrong=False), "plain's continuation")
    # the first round drafts plain's tokens 1 .. SPEC_DRAFT: the path accepts those before the request's first narrow gap
    sure = int(comparable[:, 1 : 1 + SPEC_DRAFT].sum())
    assert sure >= 1 and stats["accepted"] >= sure and full <= stats["steps"] <= SPEC_NEW - 1, (stats, sure)
    if bool(comparable.all()):
        assert torch.equal(out.cpu(), plain.cpu()) and stats["steps"] == full and stats["accepted"] == stats["drafted"], stats
    _, stats = run(NgramDrafter(2), "ngram")
    assert full <= stats["steps"] <= SPEC_NEW - 1, stats


def test_speculative_generation_is_greedy_only_and_checks_the_draft_length():
    from chitu_amd.sampling import NgramDrafter

    model, cache = build_variant("v2lite_like", "fp8")
    prompts = prompts_of(model.args.vocab_size)
    for kw in (dict(top_ks=[5, 5, 5]), dict(temperatures=[0.7] * 3), dict(top_ps=[0.9] * 3), dict(frequency_penalties=[0.1] * 3)):
        with pytest.raises(NotImplementedError):
            model.generate_speculative(prompts, 4, NgramDrafter(2), 3, **kw)
    for bad in (0, 8):
        with pytest.raises(ValueError):
            model.generate_speculative(prompts, 4, NgramDrafter(2), bad)
    with pytest.raises(ValueError):
        model.decode_multi(torch.zeros(3, 1, dtype=torch.int64, device="cuda"))
    free_before = len(cache.free_blocks)
    out = model.generate_speculative(prompts, 6, NgramDrafter(2), 2)
    assert tuple(out.shape) == (3, 6) and len(cache.free_blocks) == free_before
