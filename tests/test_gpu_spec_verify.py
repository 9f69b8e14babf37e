"""chitu_hip_speculative_verify (csrc/sample.hip via chitu_amd.sampling.speculative_verify) against the integer rule of
tests/spec_verify_ref.py: bit-exact in probability space on both kernel paths, within the tolerance the GPU's exp allows in logits
space, the emitted distribution, and repeatability / graph replay."""

import numpy as np
import pytest
import torch

from oracle import sampling as osmp
from tests import spec_verify_ref as sv

pytestmark = pytest.mark.gpu

U_MAX = 0.99999994  # the largest float32 below 1


@pytest.fixture(params=["candidates", "radix"], autouse=True)
def sampler_path(request):
    """Every test runs twice, as tests/test_gpu_sampler.py's do: with the candidate-list path enabled (it declines where it cannot
    prove the list complete) and with the radix descent alone ("sample_radix").  Both implement the one specification."""
    from chitu_amd._lib import debug_option

    if request.param == "radix":
        with debug_option("sample_radix", 1):
            yield request.param
    else:
        yield request.param


def _rows(kind, rows, vocab, seed):
    """tests/test_gpu_sampler.py's row kinds, by value"""
    g = torch.Generator().manual_seed(seed)
    if kind == "peaked":
        return torch.randn(rows, vocab, generator=g) * 3.0
    if kind == "flat":
        return torch.randn(rows, vocab, generator=g) * 0.01
    if kind == "ties":
        return torch.round(torch.randn(rows, vocab, generator=g) * 2.0)
    if kind == "equal":
        return torch.zeros(rows, vocab)
    if kind == "underflow":
        return torch.randn(rows, vocab, generator=g) * 40.0
    raise ValueError(kind)


def _drafts_of(row, temperature, top_k, top_p, probs_mode, boundary=True):
    """(kept_weights, the drafts worth trying on this row): the arg-max, a kept token of middling weight, the last kept tie at the
    smallest kept weight, the first dropped token of that weight (the tie-rank path), a token outside K, vocab + 5
    (boundary=False: without the two at the edge of the kept set)"""
    kw = sv.kept_weights(row, temperature, top_k, top_p, probs_mode)
    vocab = len(row)
    if kw["w"] is None:
        return kw, [kw["arg_max"], (kw["arg_max"] + 1) % vocab, vocab + 5]
    _, _, fix = osmp._weights_fixed(row, temperature, probs_mode)
    mask = kw["mask"]
    kept = np.nonzero(mask)[0]
    drafts = [kw["arg_max"]]
    if kept.size:
        by_weight = kept[np.argsort(fix[kept], kind="stable")]
        drafts.append(int(by_weight[by_weight.size // 2]))
        tau_w = fix[kept].min()
        dropped_ties = np.nonzero(~mask & (fix == tau_w))[0]
        if boundary:
            drafts.append(int(kept[fix[kept] == tau_w].max()))
            if dropped_ties.size:
                drafts.append(int(dropped_ties.min()))
        outside = np.nonzero(~mask & (fix != tau_w))[0]
        if outside.size:
            drafts.append(int(outside[np.argmin(fix[outside])]))
    drafts.append(vocab + 5)
    return kw, list(dict.fromkeys(drafts))


def _u_acc_of(kw, d):
    """just below and just above the acceptance threshold w_d / S (from the reference's integers), plus 0 and the largest u"""
    us = [0.0, U_MAX]
    if kw["w"] is not None and kw["S"] > 0:
        w_d = int(kw["w"][d]) if 0 <= d < kw["w"].size else 0
        us += [u for u in sv.u_around(w_d, kw["S"]) if u is not None]
    return list(dict.fromkeys(us))


def _launch_and_compare(x, T, temps, ks, ps, drafts, us, kws, probs_mode=True):
    """one launch over x [rows, vocab] (a device tensor or view) against the rule, row by row from the kept weights kws[row]"""
    from chitu_amd import sampling

    out, acc, tok = sampling.speculative_verify(x, drafts, T, temps, ks, ps, uniforms=us, probs_mode=probs_mode, return_rows=True)
    want = [sv.verify_row_from(kws[r], drafts[r], us[r][0], us[r][1]) for r in range(len(drafts))]
    want_acc, want_tok = [int(a) for a, _ in want], [t for _, t in want]
    assert acc.dtype == torch.int32 and tok.dtype == torch.int64 and out.dtype == torch.int64
    for r in range(len(drafts)):
        assert (int(acc[r]), int(tok[r])) == (want_acc[r], want_tok[r]), (r, drafts[r], us[r], int(acc[r]), int(tok[r]), want[r])
    assert np.array_equal(out.cpu().numpy(), sv.sequences(want_acc, want_tok, T))
    return want_acc


# ---------------------------------------------------------------- bit-exact in probability space
CASES = [  # (kind, vocab, top_k, top_p): from tests/test_gpu_sampler.py's CASES
    ("peaked", 1000, 50, 0.9), ("ties", 1000, -1, 0.6), ("equal", 300, 7, 1.0), ("flat", 4099, -1, 0.9), ("underflow", 4099, -1, 1.0),
    ("peaked", 1000, 1, 0.9), ("peaked", 1000, 2, 0.0), ("peaked", 129280, 50, 0.9), ("ties", 129280, 40000, 0.6),
]


@pytest.mark.parametrize("kind,vocab,top_k,top_p", CASES)
def test_probability_space_verification_is_bit_exact(kind, vocab, top_k, top_p):
    """probs_mode: every operation of the kernel is an IEEE operation, so accepted, row_tokens and out equal the rule's.  T = 4:
    three draft rows and the bonus row (draft -1) per sequence.  Small vocabularies: every draft kind x every u_acc (0, the two
    float32 neighbours of the threshold, the largest u) x u_alt in {0, 0.5, largest}, all on one row of probabilities.  The full
    vocabulary: bs = 1, the arg-max just accepted, the middling token just rejected, the last draft kind rejected."""
    T = 4
    probs = torch.softmax(_rows(kind, 1, vocab, 7) / 0.8, dim=-1)[0]
    kw, kinds = _drafts_of(probs.numpy(), 1.0, top_k, top_p, True)
    u_alts = [0.0, 0.5, U_MAX]
    if vocab > 4099:
        picks = [kinds[0], kinds[1], kinds[min(3, len(kinds) - 1)]]
        w = [int(kw["w"][d]) if d < vocab else 0 for d in picks]
        just_accepted, just_rejected = sv.u_around(w[0], kw["S"])[0], sv.u_around(w[1], kw["S"])[1]
        assert just_accepted is not None and just_rejected is not None
        combos = list(zip(picks, [just_accepted, just_rejected, 0.0], u_alts))
    else:
        combos = [(d, ua, u) for d in kinds for ua in _u_acc_of(kw, d) for u in u_alts]
    while len(combos) % (T - 1):
        combos.append(combos[len(combos) % len(kinds)])
    drafts, us = [], []
    for s in range(len(combos) // (T - 1)):
        for d, ua, u in combos[s * (T - 1) : (s + 1) * (T - 1)]:
            drafts.append(d)
            us.append((ua, u))
        drafts.append(-1)
        us.append((0.5, u_alts[s % 3]))
    rows = len(drafts)
    x = probs.cuda().repeat(rows, 1)
    acc = _launch_and_compare(x, T, None, [top_k] * rows, [top_p] * rows, drafts, us, [kw] * rows)
    if top_k != 1 and vocab <= 4099:
        assert 0 < sum(acc) < rows - rows // T  # both branches ran


def test_mixed_parameters_per_row_odd_vocabulary_and_unaligned_rows():
    """vocab 2001 (a ragged tail) in a view whose rows start at odd element offsets (no wide loads), every row with its own
    probabilities and parameters: top_k 0 and above the vocabulary, top_p 1.5 and 0.0 among them"""
    T, rows, vocab = 4, 12, 2001
    probs = torch.softmax(_rows("peaked", rows, vocab, 11), dim=-1)
    ks = [50, 1, -1, 7, 2001, 3000, 2, 0, 100, 5, -1, 50]
    ps = [0.9, 0.5, 0.2, 1.0, 0.99, 0.8, 0.0, 0.6, 1.5, 0.0, 1.5, 0.3]
    kws, drafts, us = [], [], []
    for r in range(rows):
        kw, kinds = _drafts_of(probs[r].numpy(), 1.0, ks[r], ps[r], True)
        d = -1 if r % T == T - 1 else kinds[(r // T + r % T) % len(kinds)]
        ua = _u_acc_of(kw, d)
        kws.append(kw)
        drafts.append(d)
        us.append((ua[-1] if r % 2 else ua[-2] if len(ua) > 2 else ua[0], 0.1 * (r % 10) + 0.05))
    wide = torch.zeros(rows, vocab + 6).cuda()
    view = wide[:, 5 : 5 + vocab]
    view.copy_(probs)
    _launch_and_compare(view, T, None, ks, ps, drafts, us, kws)


# ---------------------------------------------------------------- logits space
@pytest.mark.parametrize("kind,vocab,top_k,top_p", CASES[:7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_logits_verification_within_exp_tolerance(kind, vocab, top_k, top_p, dtype):
    """The GPU's exp is an ulp off numpy's (tests/test_gpu_sampler.py's logits test), so weights move in the last bits.  The
    reference runs on the CPU first; u_acc is placed 2e-3 from the row's p(d), so `accepted` has to equal the reference's (the
    allowance |u_acc - p(d)| < 1e-4 never applies; the drafts are the arg-max, a token of middling weight, one outside the kept set
    and vocab + 5 -- whether a token AT the edge of the kept set is kept may itself move with the ulp); the token is the reference's, or its interval in the residual CDF (p without a
    rejected draft, renormalised) lies within 1e-4 of u_alt -- for one row per case at the most."""
    from chitu_amd import sampling

    T, rows = 4, 12
    temps = [0.8, 1.0, 0.5, 1.3, 0.7, 2.0] * 2
    x = _rows(kind, rows, vocab, 3).to(dtype)
    u_alts = [0.0, U_MAX, 0.5, 0.123456, 0.87654, 0.3333]
    kws, drafts, us, p_d = [], [], [], []
    for r in range(rows):
        kw, kinds = _drafts_of(x[r].float().numpy(), temps[r], top_k, top_p, False, boundary=False)
        d = -1 if r % T == T - 1 else kinds[(r // T + r % T) % len(kinds)]
        p = float(kw["w"][d]) / kw["S"] if kw["w"] is not None and kw["S"] > 0 and 0 <= d < vocab else 0.0
        ua = p - 2e-3 if (r % 2 == 0 and p > 2e-3) or p + 2e-3 >= 1.0 else p + 2e-3
        kws.append(kw)
        drafts.append(d)
        us.append((float(np.float32(ua)), u_alts[r % 6]))
        p_d.append(p)
    want = [sv.verify_row_from(kws[r], drafts[r], us[r][0], us[r][1]) for r in range(rows)]
    out, acc, tok = sampling.speculative_verify(x.cuda(), drafts, T, temps, [top_k] * rows, [top_p] * rows, uniforms=us, return_rows=True)
    acc, tok = acc.cpu().tolist(), tok.cpu().tolist()
    loose = 0
    for r in range(rows):
        assert abs(us[r][0] - p_d[r]) >= 1e-3
        assert bool(acc[r]) == bool(want[r][0]), (r, drafts[r], us[r], p_d[r], acc[r], want[r])
        if tok[r] == want[r][1]:
            continue
        assert not want[r][0] and top_k != 1, (r, tok[r], want[r])
        w = kws[r]["w"].astype(np.float64)
        if 0 <= drafts[r] < vocab:
            w[drafts[r]] = 0.0
        dist = w / w.sum()
        cdf = np.cumsum(dist)
        t = tok[r]
        assert 0 <= t < vocab and cdf[t] - dist[t] - 1e-4 <= us[r][1] <= cdf[t] + 1e-4, (r, t, want[r], cdf[t] - dist[t], cdf[t], us[r])
        loose += 1
    assert loose <= 1
    assert np.array_equal(out.cpu().numpy(), sv.sequences(acc, tok, T))


# ---------------------------------------------------------------- distribution
@pytest.mark.parametrize("which", ["most_likely", "last_kept", "outside"])
def test_emitted_tokens_follow_the_kept_distribution(which):
    """8192 sequences of T = 2 on one peaked row (vocab 300, temperature 0.9, top-k 12, top-p 0.95) with independent uniforms from
    a CUDA generator: the first emitted token's histogram within 5 sigma + 1 of the kept distribution per token (tests/
    test_gpu_sampler.py's bound), nothing outside the kept set, and the number of accepted drafts within 5 sigma of n * p(d)."""
    from chitu_amd import sampling

    n, T, vocab = 8192, 2, 300
    row = _rows("peaked", 1, vocab, 5) * 0.7
    dist = osmp.kept_distribution(row[0].numpy(), 0.9, 12, 0.95)
    kept = np.nonzero(dist)[0]
    d = {"most_likely": int(np.argmax(dist)), "last_kept": int(kept[np.argmin(dist[kept])]), "outside": int(np.argmin(dist))}[which]
    assert (dist[d] == 0) == (which == "outside")
    x = row.cuda().expand(n * T, vocab).contiguous()
    drafts = torch.tensor([d, -1] * n, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(4321)
    out, acc, _ = sampling.speculative_verify(x, drafts, T, [0.9] * (n * T), [12] * (n * T), [0.95] * (n * T), generator=gen, return_rows=True)
    out, acc = out.cpu().numpy(), acc.cpu().numpy()
    counts = np.bincount(out[:, 1], minlength=vocab).astype(np.float64)
    sigma = np.sqrt(n * dist * (1 - dist))
    worst = float(np.max(np.abs(counts - n * dist)[dist > 0] / sigma[dist > 0]))
    print(f"SPEC_VERIFY distribution, draft {which} (p = {dist[d]:.4f}): accepted {int(acc[0::2].sum())} of {n}, worst deviation {worst:.2f} sigma")
    assert counts[dist == 0].sum() == 0
    assert (np.abs(counts - n * dist) <= 5 * sigma + 1).all()
    assert abs(int(acc[0::2].sum()) - n * dist[d]) <= 5 * np.sqrt(n * dist[d] * (1 - dist[d]))
    assert np.array_equal(out[:, 0], 1 + acc[0::2]) and not acc[1::2].any()
    bonus = out[out[:, 0] == 2, 2]
    assert (dist[bonus] > 0).all() and (out[out[:, 0] == 1, 2] == -1).all()


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_two_launches_and_a_graph_replay_agree(kind):
    """Integer accumulation: two launches agree bit for bit (flat rows put every atomic of the radix path in a few bins); the
    captured launch pair replays to the same result; out's padding is -1 and column 0 is 1 + the leading accepted rows."""
    from chitu_amd import sampling

    bs, T, vocab = 8, 4, 4099
    rows = bs * T
    x = _rows(kind, rows, vocab, 9).cuda()
    temps = torch.full((rows,), 0.8, device="cuda")
    ks = torch.full((rows,), -1 if kind == "flat" else 40, dtype=torch.int32, device="cuda")
    ps = torch.full((rows,), 0.9, device="cuda")
    drafts = x.argmax(dim=-1).to(torch.int32)  # the likeliest token is always kept: u_acc = 0 accepts it, the largest u rejects it
    drafts[T - 1 :: T] = -1
    us = torch.rand(rows, 2, generator=torch.Generator().manual_seed(1))
    for s in range(bs):  # sequence s accepts its first s % T drafts
        for t in range(T):
            us[s * T + t, 0] = 0.0 if t < s % T else U_MAX
    us = us.cuda()
    a = sampling.speculative_verify(x, drafts, T, temps, ks, ps, uniforms=us, return_rows=True)
    b = sampling.speculative_verify(x, drafts, T, temps, ks, ps, uniforms=us, return_rows=True)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = sampling.speculative_verify(x, drafts, T, temps, ks, ps, uniforms=us, return_rows=True)
    graph.replay()
    torch.cuda.synchronize()
    for p, q in zip(a, c):
        assert torch.equal(p, q)
    out, acc, tok = (t.cpu().numpy() for t in a)
    acc, tok = acc.reshape(bs, T), tok.reshape(bs, T)
    for s in range(bs):
        lead = 0
        while lead < T - 1 and acc[s, lead]:
            lead += 1
        assert out[s, 0] == 1 + lead == 1 + min(s % T, T - 1)
        assert np.array_equal(out[s, 1 : 2 + lead], tok[s, : lead + 1]) and (out[s, 2 + lead :] == -1).all()
    assert acc[:, : T - 1].any() and not acc[:, : T - 1].all() and not acc[:, T - 1].any()
