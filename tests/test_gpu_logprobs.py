"""chitu_ext8_logprobs (csrc/logprobs.hip via chitu_amd.sampling.logprobs, DeviceSampler and generate) against float64 log_softmax
on the CPU, the top N from a lexsort on (-value, id).  Ids are exact.  Log-probabilities, derived for |x| <= 30: the fixed-tree
fp32 sum of <= 2^17 non-negative terms carries <= ~20 * 2^-24 relative error, expf and logf a few ulp each and x - max one
rounding, together below 1e-5 absolute in logZ, plus the rounding of the result: 2e-5 + 1e-6 |ref|.  Measured on an MI355X
(every test prints its worst error): 2.11e-6 in the sweep (vocab 129280, 3 rows, fp32), about the rounding of a result near -40
-- far below the derived bound, so the bound asserted is 4 x the measured value, BOUND = 8.5e-6 absolute."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 129280  # DeepSeek-V3's vocabulary: 16 slices, the last one short
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
BOUND = 8.5e-6


def reference(x, n):
    """(log_softmax [rows, vocab], top ids [rows, n], their log-probabilities) in float64; -1 / -inf beyond the vocabulary"""
    rows, vocab = x.shape
    lp = torch.log_softmax(x.double(), dim=-1).numpy()
    ids, top = np.full((rows, n), -1, np.int64), np.full((rows, n), -np.inf)
    for r in range(rows):
        order = np.lexsort((np.arange(vocab), -x[r].double().numpy()))[:n]
        ids[r, : len(order)], top[r, : len(order)] = order, lp[r, order]
    return lp, ids, top


@functools.lru_cache(maxsize=None)
def random_case(vocab, rows, dtype):
    g = torch.Generator().manual_seed(vocab + rows)
    x = (torch.randn(rows, vocab, generator=g) * 6).clamp_(-30, 30).to(DTYPES[dtype])
    return (x,) + reference(x.float(), 20)


def on_device(x, layout="dense"):
    """dense, or a view into a NaN-filled buffer with an odd row stride (every row has another alignment), base off by one"""
    if layout == "dense":
        return x.cuda()
    buf = torch.full((x.shape[0], x.shape[1] + 13), float("nan"), dtype=x.dtype, device="cuda")
    view = buf[:, 1 : 1 + x.shape[1]] if layout == "misaligned" else buf[:, : x.shape[1]]
    view.copy_(x)
    return view


def worst_error(got, ref, what):
    """non-finite entries equal (NaN included), finite ones within BOUND; returns the largest absolute error"""
    got, ref = got.double().cpu().numpy(), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), what
    err = np.abs(got[fin] - ref[fin])
    assert (err <= BOUND).all(), (what, err.max())
    return err.max() if err.size else 0.0


def check(xd, tokens, n, lp, ids, top, what):
    from chitu_amd import sampling

    tok = torch.as_tensor(tokens, dtype=torch.int64)
    tok_lp, top_ids, top_lp = sampling.logprobs(xd, tok.cuda(), n)
    assert torch.equal(top_ids.cpu().long(), torch.from_numpy(ids[:, :n])), what
    valid = (tok >= 0) & (tok < xd.shape[1])
    ref_tok = np.where(valid.numpy(), lp[np.arange(len(tok)), tok.clamp(0, xd.shape[1] - 1).numpy()], np.nan)
    worst = max(worst_error(tok_lp, ref_tok, (what, "token")), worst_error(top_lp, top[:, :n], (what, "top")))
    print(f"LOGPROBS {what}: worst abs error {worst:.2e}")
    return worst


@pytest.mark.parametrize("layout", ["dense", "strided", "misaligned"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("vocab", [1, 5, 1023, 8192, 8193, BIG])
def test_shape_sweep(vocab, rows, dtype, layout):
    x, lp, ids, top = random_case(vocab, rows, dtype)
    xd = on_device(x, layout)
    tokens = [(r * 7919 + 3) % vocab for r in range(rows)]
    for n in (0, 1, 20):
        check(xd, tokens, n, lp, ids, top, (vocab, rows, dtype, layout, n))


@pytest.mark.parametrize("only_at_slice_edges", [False, True])
def test_ties_go_to_the_lower_id(only_at_slice_edges):
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (2, BIG), generator=g).float()
    if only_at_slice_edges:
        x.clamp_(max=2)
        x[:, [8191, 8192, 16383, 16384, BIG - 1]] = 3
    lp, ids, top = reference(x, 20)
    assert (x[0, ids[0, :5]] == 3).all() and (np.diff(ids[0, :5]) > 0).all()
    check(x.cuda(), [0, 5], 20, lp, ids, top, "ties")


@pytest.mark.parametrize("kind", ["peak", "half_neg_inf", "all_neg_inf"])
def test_extremes(kind):
    from chitu_amd import sampling

    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, BIG, generator=g)
    if kind == "peak":
        x[:, 12345] = 80.5
    elif kind == "half_neg_inf":
        x[:, ::2] = -float("inf")
    else:
        x[1] = -float("inf")
    lp, ids, top = reference(x, 20)
    check(x.cuda(), [12345, 4], 20, lp, ids, top, kind)  # (token 4 is a -inf logit in the second and third kind)
    tok_lp, _, top_lp = sampling.logprobs(x.cuda(), torch.tensor([12345, 4]).cuda(), 20)
    if kind == "peak":
        assert (top_lp[:, 0].abs() <= 1e-6).all() and (top_lp[:, 1:] < -79).all() and (top_lp[:, 1:] > -81).all()
    if kind == "all_neg_inf":
        assert torch.isnan(top_lp[1]).all() and torch.isnan(tok_lp[1]) and torch.isfinite(top_lp[0]).all()


def test_chosen_token_at_the_slice_edges_and_out_of_range():
    x, lp, ids, top = random_case(BIG, 3, "f32")
    x6, lp6 = torch.cat([x, x]), np.concatenate([lp, lp])
    check(x6.cuda(), [0, 8191, 8192, BIG - 1, BIG, -1], 0, lp6, np.concatenate([ids, ids]), np.concatenate([top, top]), "tokens")


def test_two_launches_agree_bit_for_bit_and_leave_logits_and_tickets_alone():
    from chitu_amd import sampling

    g = torch.Generator().manual_seed(3)
    x = torch.randn(16, BIG, generator=g) * 4
    xd, tok = x.cuda(), torch.arange(16).cuda() * 8000
    a, b = sampling.logprobs(xd, tok, 20), sampling.logprobs(xd, tok, 20)
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
    assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))
    check(xd, tok.tolist(), 20, *reference(x, 20), "third launch")  # the tickets went back to zero


def test_top_n_outside_0_to_20_is_refused():
    from chitu_amd import sampling

    for n in (-1, 21):
        with pytest.raises(ValueError):
            sampling.logprobs(torch.zeros(1, 8, device="cuda"), None, n)


# ---------------------------------------------------------------- the model: DeviceSampler and generate
# (eager steps, as tests/test_gpu_prefill_paged.py runs its cached tiny model: graphs captured under inference mode and kept alive
# by that cache would leave torch's capture state unusable for the later tests that capture outside inference mode)
def test_generate_reports_the_greedy_tokens_and_the_prefill_logits_logprobs():
    from tests.test_gpu_prefill_paged import prompts_of, release, tiny

    model, cache = tiny(2, 1)
    prompts = prompts_of(model.args.vocab_size)
    plain = model.generate(prompts, 4, use_graph=False)
    tokens, lp = model.generate(prompts, 4, use_graph=False, logprobs=3)
    assert torch.equal(tokens, plain) and not lp.token_logprobs.is_cuda
    assert tuple(lp.top_ids.shape) == tuple(lp.top_logprobs.shape) == (3, 4, 3) and tuple(lp.token_logprobs.shape) == (3, 4)
    assert torch.equal(lp.top_ids[..., 0].long(), tokens.cpu()) and torch.equal(lp.token_logprobs, lp.top_logprobs[..., 0])
    logits = model.prefill(prompts, ["p0", "p1", "p2"]).float().cpu()
    release(cache)
    ref, ids, top = reference(logits, 3)
    assert np.array_equal(lp.top_ids[:, 0].numpy(), ids)
    worst = max(worst_error(lp.top_logprobs[:, 0], top, "step 0 top"),
                worst_error(lp.token_logprobs[:, 0], ref[np.arange(3), tokens[:, 0].cpu().numpy()], "step 0 token"))
    print(f"LOGPROBS generate step 0: worst abs error {worst:.2e}")


def test_logprobs_leave_a_penalised_sampled_draw_unchanged():
    from tests.test_gpu_prefill_paged import prompts_of, tiny

    model, _ = tiny(2, 1)
    prompts = prompts_of(model.args.vocab_size)
    kw = dict(temperatures=[0.8] * 3, top_ks=[50] * 3, top_ps=[0.9] * 3, frequency_penalties=[0.5] * 3)
    gen = torch.Generator(device="cuda")
    plain = model.generate(prompts, 4, use_graph=False, generator=gen.manual_seed(5), **kw)
    tokens, lp = model.generate(prompts, 4, use_graph=False, generator=gen.manual_seed(5), logprobs=2, **kw)
    assert torch.equal(tokens, plain) and bool(torch.isfinite(lp.token_logprobs).all())
    assert bool((lp.token_logprobs <= lp.top_logprobs[..., 0]).all())
