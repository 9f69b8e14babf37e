"""sampling.ModelDrafter (a draft MODEL with a paged cache of its own, drafting on the device) through generate_speculative and
generate_speculative_sampled, on the tiny models of tests/test_gpu_spec_sampled.py: self-drafting, a shallower drafter, the two
caches' bookkeeping, sampled drafts judged by chitu_hip_speculative_verify_sampled, a drafter the target never agrees with, and the
errors."""
import dataclasses
import gc

import numpy as np
import pytest
import torch

from oracle import sampling as osmp

pytestmark = pytest.mark.gpu

NEW, DRAFT = 10, 3  # (NEW - 1) % (DRAFT + 1) != 0: the last round drafts past the end
UNCLEAR = 2 * 3e-2  # tests/test_gpu_llama_multi.py: under this top-2 gap (over the peak) two paths may pick different tokens


@pytest.fixture(autouse=True)
def models_are_gone_after_each_test():
    """set up before monkeypatch, so torn down after its undo: the test's models (two per test, each with captured graphs made in
    inference mode) are collected here, not at some later test's capture"""
    yield
    gc.collect()


def _build(family, n_layers=None, max_reqs=8):
    """tests/test_gpu_spec_sampled.py's _build (every call: a new model with the same synthetic weights and a cache of its own),
    plus "llama_fp8" (tests/test_gpu_llama_multi.py's fp8 variant) and a layer count"""
    gc.collect()  # what earlier tests left behind goes now, not during a capture
    if family == "deepseek_v3":
        from tests.test_gpu_deepseek import tiny_args
        from tests.test_gpu_mla_kv_fp8 import build

        args = tiny_args()
        return build(args if n_layers is None else dataclasses.replace(args, n_layers=n_layers), max_reqs=max_reqs)
    from tests.test_gpu_llama import build, tiny_args

    args = tiny_args() if n_layers is None else dataclasses.replace(tiny_args(), n_layers=n_layers)
    if family == "llama":
        return build(args, max_reqs=max_reqs)
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, gqa_kv_layout
    from chitu_amd.llama import LlamaDecoder, init_synthetic_

    args = dataclasses.replace(args, kv_cache_dtype="fp8")
    shape, dtype = gqa_kv_layout("fp8", args.n_kv_heads)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=max_reqs, block_size=256, max_seq_len=1024, device="cuda",
                                k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype)
    model = LlamaDecoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=1024), max_position_embeddings=1024, device="cuda")
    init_synthetic_(model, seed=0)
    return model, cache


def _page(family):
    return 64 if family == "deepseek_v3" else 256


def _prompts(vocab, family, seed=3, n=3):
    """ragged; the second prompt ends one row short of its page, so the first round's rows cross the boundary"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (k,), generator=g).tolist() for k in (5, _page(family) - 1, 33)[:n]]


class Watch:
    """wraps the target's decode_multi (keeps every verify step's tokens and logits) and the drafter's settle (checks the
    cache-length invariant after it, for the round's requests)"""

    def __init__(self, monkeypatch, model, drafter):
        # The wrappers go on the CLASSES, through monkeypatch: anything set on an instance (monkeypatch's undo too, which puts
        # the bound method back into the instance's dict) leaves the model in a reference cycle.  Its captured graphs then live
        # until the cyclic collector runs: in the middle of a later test's stream capture, which the runtime refuses, or past a
        # later test's torch.cuda.CUDAGraph(), which then shares the generator state these graphs made in inference mode.
        self.steps, self.settled = [], 0
        inner_multi, inner_settle = type(model).decode_multi, type(drafter).settle

        def decode_multi(self_, step, use_graph=True):
            logits = inner_multi(self_, step, use_graph=use_graph)
            if self_ is model:
                self.steps.append((step.cpu().clone(), logits.detach().float().cpu().clone()))
            return logits

        def settle(self_, req_ids, kept):
            inner_settle(self_, req_ids, kept)
            if self_ is not drafter:
                return
            for r in req_ids:
                assert drafter.model.cache.seq_lens[r] == model.cache.seq_lens[r], (r, drafter.model.cache.seq_lens[r], model.cache.seq_lens[r])
                for c in (model.cache, drafter.model.cache):
                    if hasattr(c, "block_table"):  # no page beyond the length stays taken
                        assert len(c.block_table[r]) == -(-c.seq_lens[r] // c.block_size), (r, c.seq_lens[r], c.block_table[r])
            self.settled += 1

        monkeypatch.setattr(type(model), "decode_multi", decode_multi)
        monkeypatch.setattr(type(drafter), "settle", settle)


@pytest.mark.parametrize("family", ["llama", "deepseek_v3", "llama_fp8"])
def test_self_drafting_greedy(family, monkeypatch):
    """the drafter is the target's twin (same weights, its own cache): the tokens are generate_speculative's with NgramDrafter; every
    rejected draft sits on a verify row whose top-2 gap is under the margin at which the single-token path (the drafter's) and the
    multi-token path may disagree; at least one round accepts every draft of a request (settle's missing-row case); the two
    caches agree after every settle and both free lists return to their start"""
    from chitu_amd.sampling import ModelDrafter, NgramDrafter

    model, cache = _build(family)
    twin, twin_cache = _build(family)
    prompts = _prompts(model.args.vocab_size, family)
    free, twin_free = len(cache.free_blocks), len(twin_cache.free_blocks)
    want = model.generate_speculative(prompts, NEW, NgramDrafter(2), DRAFT)
    drafter = ModelDrafter(twin, sample=False)
    watch = Watch(monkeypatch, model, drafter)
    got = model.generate_speculative(prompts, NEW, drafter, DRAFT)
    stats = dict(model.speculative_stats)
    print(f"MODEL_DRAFTER {family} self-draft greedy: {stats}")
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert len(cache.free_blocks) == free and len(twin_cache.free_blocks) == twin_free and not cache.seq_lens and not twin_cache.seq_lens
    assert watch.settled == stats["steps"] == len(watch.steps)
    full = rejected = 0
    for step, logits in watch.steps:
        best = logits.argmax(dim=-1)
        for b in range(step.shape[0]):
            t = 0
            while t < DRAFT and int(step[b, 1 + t]) == int(best[b, t]):
                t += 1
            if t == DRAFT:
                full += 1
                continue
            rejected += 1
            top2 = logits[b, t].topk(2).values
            gap = float((top2[0] - top2[1]) / logits[b, t].abs().max())
            assert gap < UNCLEAR, (family, b, t, gap)
    print(f"MODEL_DRAFTER {family} self-draft greedy: {full} request-rounds accepted every draft, {rejected} rejected one")
    assert full >= 1
    assert stats["accepted"] >= full * DRAFT


@pytest.mark.parametrize("family", ["llama", "deepseek_v3"])
@pytest.mark.parametrize("bs", [1, 3])
def test_a_shallower_drafter_does_not_change_greedy_output(family, bs, monkeypatch):
    """one layer drafting for three: whatever it proposes, the greedy output is generate_speculative's"""
    from chitu_amd.sampling import ModelDrafter, NgramDrafter

    model, cache = _build(family)
    small, small_cache = _build(family, n_layers=1)
    prompts = _prompts(model.args.vocab_size, family, n=bs)
    free, small_free = len(cache.free_blocks), len(small_cache.free_blocks)
    want = model.generate_speculative(prompts, NEW, NgramDrafter(2), DRAFT)
    drafter = ModelDrafter(small, sample=False)
    watch = Watch(monkeypatch, model, drafter)
    got = model.generate_speculative(prompts, NEW, drafter, DRAFT)
    print(f"MODEL_DRAFTER {family} bs={bs} one-layer drafter, greedy: {model.speculative_stats}")
    assert torch.equal(got, want)
    assert watch.settled == model.speculative_stats["steps"]
    assert len(cache.free_blocks) == free and len(small_cache.free_blocks) == small_free and not small_cache.seq_lens


@pytest.mark.parametrize("family", ["llama", "deepseek_v3", "llama_fp8"])
def test_sampled_drafts_bookkeeping_and_possible_tokens(family, monkeypatch):
    """self-drafting under sampling parameters: the drafts are drawn from the twin's rows and judged with them
    (speculative_verify_sampled, recorded here).  Every emitted token lies in the kept set the specification gives for its
    (penalised) target row -- one row per run may emit a token at most 2 places past the edge, as tests/test_gpu_spec_sampled.py
    allows for the GPU's exp; the caches agree after every settle and end empty; the same seed gives the same tokens, with the
    captured steps and with the eager ones; all top_k <= 1 gives the greedy run's tokens."""
    from chitu_amd import sampling
    from chitu_amd.sampling import ModelDrafter

    model, cache = _build(family)
    twin, twin_cache = _build(family)
    vocab = model.args.vocab_size
    prompts = _prompts(vocab, family)
    free, twin_free = len(cache.free_blocks), len(twin_cache.free_blocks)
    drafter = ModelDrafter(twin)
    watch = Watch(monkeypatch, model, drafter)
    rounds = []
    inner = sampling.speculative_verify_sampled

    def recording(logits, draft_logits, drafts, T, temperatures, top_ks, top_ps, **kw):
        out = inner(logits, draft_logits, drafts, T, temperatures, top_ks, top_ps, **kw)
        assert tuple(draft_logits.shape) == tuple(logits.shape) and draft_logits.dtype == torch.float32
        rounds.append(dict(logits=logits.detach().float().cpu().numpy().copy(), drafts=drafts.cpu().tolist(), T=T,
                           temps=temperatures.cpu().tolist(), ks=top_ks.cpu().tolist(), ps=top_ps.cpu().tolist(), out=out.cpu().numpy().copy()))
        return out

    monkeypatch.setattr(sampling, "speculative_verify_sampled", recording)
    params = dict(temperatures=[0.8, 1.0, 1.3], top_ks=[5, -1, 20], top_ps=[0.9, 0.9, 0.9])

    def run(seed, use_graph=True, **extra):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        out = model.generate_speculative_sampled(prompts, NEW, drafter, DRAFT, generator=gen, use_graph=use_graph, **{**params, **extra})
        assert tuple(out.shape) == (3, NEW) and int(out.min()) >= 0 and int(out.max()) < vocab
        assert len(cache.free_blocks) == free and len(twin_cache.free_blocks) == twin_free and not cache.seq_lens and not twin_cache.seq_lens
        return out, dict(model.speculative_stats)

    a, stats = run(3, frequency_penalties=[0.0, 0.5, 0.0])
    print(f"MODEL_DRAFTER {family} self-draft sampled: {stats}")
    assert rounds and watch.settled == stats["steps"] == len(rounds)
    emitted = loose = 0
    for rd in rounds:
        T = rd["T"]
        for b in range(rd["out"].shape[0]):
            n = int(rd["out"][b, 0])
            assert 1 <= n <= T and (rd["out"][b, 1 + n :] == -1).all()
            for t in range(n):
                r, tok = b * T + t, int(rd["out"][b, 1 + t])
                if t < n - 1:
                    assert tok == rd["drafts"][r]  # an accepted draft
                mask, n_kept, _, _ = osmp.kept_set_fixed_point(rd["logits"][r], rd["temps"][r], rd["ks"][r], rd["ps"][r])
                emitted += 1
                if not mask[tok]:
                    order = np.argsort(-rd["logits"][r], kind="stable")
                    assert int(np.nonzero(order == tok)[0][0]) < n_kept + 2, (r, tok, n_kept)
                    loose += 1
    assert loose <= 1 and emitted >= 3 * (NEW - 1)
    b, stats_b = run(3, frequency_penalties=[0.0, 0.5, 0.0])
    assert torch.equal(a, b) and stats == stats_b
    c, _ = run(11)
    d, _ = run(11, use_graph=False)
    assert torch.equal(c, d)
    n_sampled = len(rounds)
    greedy, _ = run(5, top_ks=[1, 0, -1])
    assert len(rounds) == n_sampled  # greedy rows: the point-mass entry, no draft logits read
    assert torch.equal(greedy, model.generate_speculative(prompts, NEW, drafter, DRAFT))


class _StubCache:
    def __init__(self):
        self.seq_lens = {}

    def prepare_cache_decode(self, ids):
        pass

    def prepare_block_table_for_decode(self, ids):
        pass

    def finalize_cache_single_decode(self, ids):
        for r in ids:
            self.seq_lens[r] += 1

    def rollback(self, ids, n_drop):
        for r, d in zip(ids, n_drop):
            self.seq_lens[r] -= d

    def finalize_cache_all_decode(self, r):
        del self.seq_lens[r]


class _StubDraftModel:
    """a draft "model" whose every row favours one token by 30: sampled or not, it proposes that token"""

    def __init__(self, vocab, fav):
        self.device, self.cache, self.fav = torch.device("cuda"), _StubCache(), fav
        self.args = type("Args", (), {"vocab_size": vocab})()

    def prefill(self, prompts, req_ids):
        for p, r in zip(prompts, req_ids):
            self.cache.seq_lens[r] = len(p)
        return torch.zeros(len(prompts), self.args.vocab_size, device=self.device)

    def decode(self, tokens, use_graph=True):
        x = torch.zeros(tokens.shape[0], self.args.vocab_size, device=self.device)
        x[:, self.fav] = 30.0
        return x


@pytest.mark.parametrize("family", ["llama", "deepseek_v3"])
@pytest.mark.parametrize("sample", [True, False])
def test_a_drafter_the_target_never_agrees_with(family, sample, monkeypatch):
    """the draft model always proposes vocab - 1 (q(vocab - 1) = 1 - 2e-10) under top_k 5: where that token is not among a target
    row's five largest logits, p(d) = 0, nothing is accepted, the replacement comes from max(p - q, 0) = p and every round emits
    one token.  The precondition is checked on every verify step's logits, as tests/test_gpu_spec_sampled.py does."""
    from chitu_amd.sampling import ModelDrafter

    model, cache = _build(family)
    vocab = model.args.vocab_size
    prompts = _prompts(vocab, family)
    stub = _StubDraftModel(vocab, vocab - 1)
    drafter = ModelDrafter(stub, sample=sample)
    watch = Watch(monkeypatch, model, drafter)
    gen = torch.Generator(device="cuda").manual_seed(7)
    out = model.generate_speculative_sampled(prompts, NEW, drafter, DRAFT, temperatures=[1.0] * 3, top_ks=[5] * 3, top_ps=[1.0] * 3, generator=gen)
    assert len(watch.steps) == NEW - 1
    for step, logits in watch.steps:
        assert bool((step[:, 1:] == vocab - 1).all())
        first = logits[:, 0].numpy()
        assert (first[:, vocab - 1] < np.sort(first, axis=-1)[:, -5]).all(), "precondition: vocab - 1 is among a row's top 5; pick other prompts"
    assert model.speculative_stats == dict(steps=NEW - 1, accepted=0, drafted=(NEW - 1) * len(prompts) * DRAFT)
    assert not bool((out[:, 1:] == vocab - 1).any())
    assert not cache.seq_lens and not stub.cache.seq_lens


def test_errors():
    from chitu_amd.sampling import ModelDrafter

    model, cache = _build("llama")
    prompts = _prompts(model.args.vocab_size, "llama")
    free = len(cache.free_blocks)
    with pytest.raises(ValueError, match="vocabulary"):
        model.generate_speculative(prompts, NEW, ModelDrafter(_StubDraftModel(model.args.vocab_size + 1, 0)), DRAFT)
    with pytest.raises(ValueError, match="cache"):
        model.generate_speculative_sampled(prompts, NEW, ModelDrafter(model), DRAFT, top_ks=[5] * 3)
    twin, _ = _build("llama")
    for bad in (0, 8):
        with pytest.raises(ValueError, match="draft_len"):
            model.generate_speculative(prompts, NEW, ModelDrafter(twin), bad)
        with pytest.raises(ValueError, match="draft_len"):
            model.generate_speculative_sampled(prompts, NEW, ModelDrafter(twin), bad, top_ks=[5] * 3)
    with pytest.raises(TypeError):
        ModelDrafter(object())
    assert len(cache.free_blocks) == free and not cache.seq_lens  # every refusal came before a prefill


class _ScriptedTwin:
    """A draft model for tests that need a chosen acceptance per request: a real twin decoder does the work (prefill, graph-replayed
    decode steps, its own paged cache), but the logits handed to the drafter favour by 30 the token this script names -- for the
    requests in `right`, the token a finished greedy run of the target produced at that position (accepted), for the others
    `wrong(that token)` (rejected).  The position comes from the twin's cache: the row's length is the index of the step's input token."""

    def __init__(self, monkeypatch, twin, known, right, wrong):
        self.twin, self.cache, self.device, self.args = twin, twin.cache, twin.device, twin.args
        self.known, self.right, self.wrong, self.prompt_len, self.ids = known, set(right), wrong, {}, []
        inner = type(twin.cache).prepare_cache_decode

        def prepare_cache_decode(cache, req_ids):  # on the class (see Watch)
            if cache is twin.cache:
                self.ids = list(req_ids)
            inner(cache, req_ids)

        monkeypatch.setattr(type(twin.cache), "prepare_cache_decode", prepare_cache_decode)

    def prefill(self, prompts, req_ids):
        self.prompt_len.update({r: len(p) for p, r in zip(prompts, req_ids)})
        return self.twin.prefill(prompts, req_ids)

    def decode(self, tokens, use_graph=True):
        real = self.twin.decode(tokens, use_graph=use_graph)
        assert len(self.ids) == tokens.shape[0]
        fav = []
        for r in self.ids:
            nxt = self.cache.seq_lens[r] + 1 - self.prompt_len[r]  # index, among the generated tokens, of the token this row predicts
            tok = self.known[r][nxt] if nxt < len(self.known[r]) else 0
            fav.append(tok if r in self.right else self.wrong(tok))
        x = torch.zeros_like(real)
        x[torch.arange(len(fav), device=x.device), torch.tensor(fav, device=x.device)] = 30.0
        return x


@pytest.mark.parametrize("family", ["llama", "deepseek_v3"])
@pytest.mark.parametrize("loop", ["greedy", "sampled"])
def test_requests_retire_in_different_rounds(family, loop, monkeypatch):
    """Uneven acceptance by construction, in both loops: request 0's drafts are the target's own greedy tokens (a verify step is
    deterministic and a row's logits depend on the tokens before it alone: tests/test_gpu_llama_multi.py), so every one is accepted
    and it retires after ceil((NEW - 1) / (DRAFT + 1)) rounds; the other two requests' drafts are never accepted -- greedy loop:
    the greedy token + 1; sampled loop: vocab - 1 under top_k 5, the precondition checked on every verify step as in
    test_a_drafter_the_target_never_agrees_with -- so they emit one token per round and retire in round NEW - 1.  In the sampled
    loop request 0 has top_k 1 inside a sampling batch (greedy rows of both kernels), the other two sample.  After the partial
    retire the loop rebuilds the per-request and per-row parameters and gathers the survivors' last tokens.  Checked: the retire
    round of every request, the cache-length invariant and the page counts after every settle (Watch), request 0's tokens, the
    acceptance counts, and both caches' free lists."""
    from chitu_amd.sampling import ModelDrafter

    model, cache = _build(family)
    twin, twin_cache = _build(family)
    vocab = model.args.vocab_size
    prompts = _prompts(vocab, family)
    reqs = ["r0", "r1", "r2"]
    free, twin_free = len(cache.free_blocks), len(twin_cache.free_blocks)
    own = model.generate_speculative(prompts, NEW, ModelDrafter(twin, sample=False), DRAFT)
    known = {r: row for r, row in zip(reqs, own.tolist())}
    wrong = (lambda t: (t + 1) % vocab) if loop == "greedy" else (lambda t: vocab - 1)
    drafter = ModelDrafter(_ScriptedTwin(monkeypatch, twin, known, ["r0"], wrong), sample=(loop == "sampled"))
    watch = Watch(monkeypatch, model, drafter)
    retired = {}
    inner_retire = ModelDrafter.retire

    def retire(self_, req_id):
        if self_ is drafter:
            retired[req_id] = watch.settled
        inner_retire(self_, req_id)

    monkeypatch.setattr(ModelDrafter, "retire", retire)
    if loop == "greedy":
        out = model.generate_speculative(prompts, NEW, drafter, DRAFT, req_ids=reqs)
        assert torch.equal(out, own)
    else:
        gen = torch.Generator(device="cuda").manual_seed(7)
        out = model.generate_speculative_sampled(prompts, NEW, drafter, DRAFT, temperatures=[1.0] * 3, top_ks=[1, 5, 5], top_ps=[1.0] * 3,
                                                 generator=gen, req_ids=reqs)
        assert torch.equal(out[0], own[0])
        for step, logits in watch.steps:
            rows = slice(1, None) if step.shape[0] == 3 else slice(0, None)  # request 0 is row 0 while it lives
            first = logits[rows, 0].numpy()
            assert (first[:, vocab - 1] < np.sort(first, axis=-1)[:, -5]).all(), "precondition: vocab - 1 is among a row's top 5; pick other prompts"
        assert not bool((out[1:, 1:] == vocab - 1).any())
    fast = -(-(NEW - 1) // (DRAFT + 1))
    print(f"MODEL_DRAFTER {family} {loop}: retire rounds {retired}, {model.speculative_stats}")
    assert retired == {"r0": fast, "r1": NEW - 1, "r2": NEW - 1} and fast < NEW - 1
    assert [s.shape[0] for s, _ in watch.steps] == [3] * fast + [2] * (NEW - 1 - fast)
    # request 0: every draft of its rounds accepted, except those past the end in its last round, which may or may not be
    lo = NEW - 1 - fast
    assert lo <= model.speculative_stats["accepted"] <= fast * DRAFT
    assert model.speculative_stats["steps"] == NEW - 1 == watch.settled
    assert model.speculative_stats["drafted"] == DRAFT * (3 * fast + 2 * (NEW - 1 - fast))
    assert len(cache.free_blocks) == free and len(twin_cache.free_blocks) == twin_free and not cache.seq_lens and not twin_cache.seq_lens
