"""generate_speculative_sampled (speculative decoding with sampling: sampling.generate_speculative_sampled over decode_multi and
chitu_hip_speculative_verify) on LlamaDecoder and DeepSeekV3Decoder, with the tiny models of tests/test_gpu_llama_multi.py and
tests/test_gpu_deepseek_multi.py: greedy parameters reduce to generate_speculative, the bookkeeping under sampling parameters,
every emitted token possible under its row's parameters, and the frequency penalty across the drafts of a round."""
import numpy as np
import pytest
import torch

from oracle import sampling as osmp

pytestmark = pytest.mark.gpu

NEW, DRAFT = 9, 3


def _build(family):
    if family == "llama":
        from tests.test_gpu_llama import build, tiny_args

        return build(tiny_args())
    from tests.test_gpu_deepseek import tiny_args
    from tests.test_gpu_mla_kv_fp8 import build

    return build(tiny_args(), max_reqs=8)


@pytest.fixture(params=["llama", "deepseek_v3"])
def family(request):
    return request.param


def _prompts(vocab, seed=3, lens=(5, 63, 33)):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lens]


class PositionDrafter:
    """proposes, per prompt, the tokens a finished run produced at the positions to come (tests/test_gpu_llama_multi.py's
    ReplayDrafter without the "wrong" switch)"""

    def __init__(self, prompts, tokens):
        self.known = {tuple(p): [int(t) for t in row] for p, row in zip(prompts, tokens.tolist())}

    def propose(self, history, k):
        for p, row in self.known.items():
            if tuple(history[: len(p)]) == p:
                return (row[len(history) - len(p) :] + [0] * k)[:k]
        raise AssertionError("unknown prompt")


class ConstantDrafter:
    def __init__(self, token):
        self.token = token

    def propose(self, history, k):
        return [self.token] * k


class RepeatLastDrafter:
    def propose(self, history, k):
        return [int(history[-1])] * k


class Recorder:
    """wraps sampling.speculative_verify: keeps every round's verify logits (as the launch saw them: penalised), arguments and out"""

    def __init__(self, monkeypatch):
        from chitu_amd import sampling

        self.rounds = []
        inner = sampling.speculative_verify

        def recording(logits, drafts, T, temperatures, top_ks, top_ps, **kw):
            out = inner(logits, drafts, T, temperatures, top_ks, top_ps, **kw)
            self.rounds.append(dict(logits=logits.detach().float().cpu().numpy().copy(), drafts=list(drafts), T=T,
                                    temps=temperatures.cpu().tolist(), ks=top_ks.cpu().tolist(), ps=top_ps.cpu().tolist(),
                                    out=out.cpu().numpy().copy()))
            return out

        monkeypatch.setattr(sampling, "speculative_verify", recording)


def test_greedy_parameters_reduce_to_the_greedy_path(family):
    """every top_k = 1: the rows are greedy rows of the verify kernel (accepted iff draft == argmax), so tokens and statistics are
    generate_speculative's, drafter for drafter -- both loops replay the same captured step on the same inputs"""
    from chitu_amd.sampling import NgramDrafter

    model, cache = _build(family)
    prompts = _prompts(model.args.vocab_size)
    free_before = len(cache.free_blocks)
    plain = model.generate_speculative(prompts, NEW, NgramDrafter(2), DRAFT)
    for drafter in (NgramDrafter(2), PositionDrafter(prompts, plain), ConstantDrafter(0)):
        want = model.generate_speculative(prompts, NEW, drafter, DRAFT)
        want_stats = dict(model.speculative_stats)
        got = model.generate_speculative_sampled(prompts, NEW, drafter, DRAFT, temperatures=[0.5, 1.0, 2.0], top_ks=[1, 1, 1], top_ps=[0.9] * 3)
        assert torch.equal(got, want) and model.speculative_stats == want_stats, (type(drafter).__name__, model.speculative_stats, want_stats)
        got = model.generate_speculative_sampled(prompts, NEW, drafter, DRAFT, top_ks=[1, 0, -1])  # `is_all_greedy`: every top_k <= 1
        assert torch.equal(got, want) and model.speculative_stats == want_stats
        assert len(cache.free_blocks) == free_before and not cache.seq_lens
    with pytest.raises(ValueError):
        model.generate_speculative_sampled(prompts, NEW, NgramDrafter(2), 8, top_ks=[5] * 3)


def test_bookkeeping_with_sampling_parameters(family):
    from chitu_amd.sampling import NgramDrafter

    model, cache = _build(family)
    vocab = model.args.vocab_size
    prompts = _prompts(vocab)
    n_req, free_before = len(prompts), len(cache.free_blocks)

    def run(drafter, seed, temps, ks, ps=(0.9, 0.9, 0.9), new=NEW):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        out = model.generate_speculative_sampled(prompts, new, drafter, DRAFT, temperatures=temps, top_ks=ks, top_ps=list(ps), generator=gen)
        assert tuple(out.shape) == (n_req, new) and out.dtype == torch.int64 and out.is_cuda
        assert int(out.min()) >= 0 and int(out.max()) < vocab
        assert len(cache.free_blocks) == free_before and not cache.seq_lens
        stats = dict(model.speculative_stats)
        assert set(stats) == {"steps", "accepted", "drafted"} and stats["drafted"] % DRAFT == 0 and (new > 1) <= stats["steps"] <= new - 1
        return out, stats

    temps, ks = [0.8, 1.0, 1.3], [5, -1, 20]
    a, stats_a = run(NgramDrafter(2), 1, temps, ks)
    b, stats_b = run(NgramDrafter(2), 1, temps, ks)
    assert torch.equal(a, b) and stats_a == stats_b
    c, _ = run(NgramDrafter(2), 2, temps, ks)
    assert not torch.equal(a, c)
    one, _ = run(NgramDrafter(2), 1, temps, ks, new=1)  # the first token alone: sampled from the prefill logits
    assert torch.equal(one[:, 0], a[:, 0])

    # a drafter that replays a finished run's own tokens: its drafts are tokens the run drew from these very distributions, but one
    # rejection sends the request down another path, where the old run's tokens are as good as random drafts.  At a temperature of
    # 0.01 a logit gap of 0.05 already is a factor e^-5 in weight: the drawn tokens carry nearly all of their rows' mass, so each
    # request follows its old run, its drafts are accepted and it finishes in fewer steps than tokens.
    cold = [0.01, 0.01, 0.01]
    own, _ = run(NgramDrafter(2), 5, cold, ks)
    _, stats = run(PositionDrafter(prompts, own), 5, cold, ks)
    print(f"SPEC_SAMPLED {family}: own tokens replayed: {stats}")
    assert stats["accepted"] >= 1 and stats["steps"] < NEW - 1, stats


def test_a_draft_outside_the_top_k_is_never_accepted(family, monkeypatch):
    """the drafter always proposes vocab - 1 under top_k 5: where that token is not among a row's five largest logits its kept
    weight is 0, so nothing is accepted and every step emits one token.  The precondition is checked on every verify step's
    logits (the decode_multi step's output, as the launch saw it), in the row that judges the first draft."""
    model, cache = _build(family)
    vocab = model.args.vocab_size
    prompts = _prompts(vocab)
    rec = Recorder(monkeypatch)
    gen = torch.Generator(device="cuda").manual_seed(7)
    out = model.generate_speculative_sampled(prompts, NEW, ConstantDrafter(vocab - 1), DRAFT, temperatures=[1.0] * 3, top_ks=[5] * 3,
                                             top_ps=[1.0] * 3, generator=gen)
    assert len(rec.rounds) == NEW - 1
    for rd in rec.rounds:
        first = rd["logits"][:: rd["T"]]  # each sequence's row 0 decides: while nothing is accepted the later rows never count
        assert (first[:, vocab - 1] < np.sort(first, axis=-1)[:, -5]).all(), "precondition: vocab - 1 is among a row's top 5; pick other prompts"
        assert (rd["out"][:, 0] == 1).all() and (rd["out"][:, 2:] == -1).all()
    assert model.speculative_stats == dict(steps=NEW - 1, accepted=0, drafted=(NEW - 1) * len(prompts) * DRAFT)
    assert not bool((out[:, 1:] == vocab - 1).any())


def test_every_emitted_token_was_possible(family, monkeypatch):
    """every token a round emits lies in the kept set the specification gives for its row's logits and the request's parameters;
    the GPU's exp may move the edge of that set by elements of negligible mass (tests/test_gpu_sampler.py's logits test allows the
    kept count to differ by 2), so one row per run may emit a token at most 2 places past the edge"""
    from chitu_amd.sampling import NgramDrafter

    model, cache = _build(family)
    prompts = _prompts(model.args.vocab_size)
    rec = Recorder(monkeypatch)
    gen = torch.Generator(device="cuda").manual_seed(3)
    out = model.generate_speculative_sampled(prompts, NEW, NgramDrafter(2), DRAFT, temperatures=[0.8, 1.0, 1.3], top_ks=[5, -1, 20],
                                             top_ps=[0.9, 0.9, 0.9], frequency_penalties=[0.0, 0.5, 0.0], generator=gen)
    assert rec.rounds and tuple(out.shape) == (3, NEW)
    emitted = loose = 0
    for rd in rec.rounds:
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


def test_frequency_penalty_forbids_repeats(family):
    """a penalty of 1e4 on request 0 (top_k -1, temperature 1; request 1's top_k of 50 makes the batch a sampling batch, where -1
    means no limit): it never repeats a token, whatever the drafter proposes -- here the last token again and again"""
    model, cache = _build(family)
    prompts = _prompts(model.args.vocab_size)
    gen = torch.Generator(device="cuda").manual_seed(5)
    out = model.generate_speculative_sampled(prompts, NEW, RepeatLastDrafter(), DRAFT, temperatures=[1.0] * 3, top_ks=[-1, 50, -1], top_ps=[1.0] * 3,
                                             frequency_penalties=[1e4, 0.0, 0.0], generator=gen)
    assert len(set(out[0].tolist())) == NEW, out[0].tolist()
    assert not cache.seq_lens


class _StubCache:
    def prepare_block_table_for_decode_multi(self, ids, T):
        pass

    def finalize_cache_multi_decode(self, ids, kept):
        self.kept = getattr(self, "kept", []) + [list(kept)]

    def finalize_cache_all_decode(self, req):
        pass


class _StubModel:
    """prefill favours token `first`, every row of every verify step favours token `fav` by 30 (p = 1 - 6e-12 at temperature 1
    over 64 tokens), whatever the inputs: the loop, the penalty launch and the verify launch run as with a decoder"""

    def __init__(self, vocab, first, fav):
        self.device, self.cache, self.vocab, self.first, self.fav = torch.device("cuda"), _StubCache(), vocab, first, fav

    def prefill(self, prompts, req_ids):
        x = torch.zeros(len(prompts), self.vocab, device=self.device)
        x[:, self.first] = 30.0
        return x

    def decode_multi(self, step, use_graph=True):
        x = torch.zeros(step.shape[0], step.shape[1], self.vocab, device=self.device)
        x[:, :, self.fav] = 30.0
        return x


def test_the_penalty_of_a_row_counts_the_drafts_before_it():
    """Why row (b, t) is penalised with response[b] + drafts[b][:t]: the drafter proposes [A, A, A] and every row gives A nearly
    all the mass.  Row 0 accepts A; row 1 sees A in what would then be the response, so under a penalty of 1e4 it rejects the second
    A and emits another token -- penalised with the response alone it would accept A again.  Without a penalty it does."""
    from chitu_amd import sampling

    vocab, first, fav, new = 64, 9, 17, 8
    for penalty, repeats in ((1e4, False), (0.0, True)):
        model = _StubModel(vocab, first, fav)
        gen = torch.Generator(device="cuda").manual_seed(1)
        out = sampling.generate_speculative_sampled(model, [[1, 2, 3]], new, ConstantDrafter(fav), DRAFT, 8, [1.0], [vocab], [1.0],
                                                    frequency_penalties=[penalty], generator=gen)[0].tolist()
        assert out[:2] == [first, fav], out
        if repeats:
            assert out == [first] + [fav] * (new - 1) and model.speculative_stats == dict(steps=2, accepted=6, drafted=6)
        else:
            assert len(set(out)) == new, out
            assert model.cache.kept[0] == [2] and model.speculative_stats["accepted"] == 1  # the first A, and none after it
