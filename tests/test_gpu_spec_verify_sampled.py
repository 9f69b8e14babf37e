"""chitu_hip_speculative_verify_sampled (csrc/sample.hip via chitu_amd.sampling.speculative_verify_sampled) against the integer rule of
tests/spec_verify_sampled_ref.py: bit-exact in probability space, within the tolerance the GPU's exp allows in logits space, the
emitted distribution when the draft is drawn from the draft row, and repeatability / graph replay.  Row kinds, draft kinds and
bounds are tests/test_gpu_spec_verify.py's."""

import numpy as np
import pytest
import torch

from oracle import sampling as osmp
from tests import spec_verify_ref as sv
from tests import spec_verify_sampled_ref as svs
from tests import test_gpu_spec_verify as base

pytestmark = pytest.mark.gpu

U_MAX = base.U_MAX


@pytest.fixture(params=["candidates", "radix"], autouse=True)
def sampler_path(request):
    """Every test runs twice, as tests/test_gpu_spec_verify.py's do.  The pair passes of the new entry always take the radix cut;
    its rows without a draft are chitu_hip_sample's rows and take either path."""
    from chitu_amd._lib import debug_option

    if request.param == "radix":
        with debug_option("sample_radix", 1):
            yield request.param
    else:
        yield request.param


def _pair_drafts(p_row, q_row, temperature, top_k, top_p, probs_mode, boundary=True):
    """(kw_p, kw_q, drafts): the existing file's draft kinds on either row (arg-max, a kept token of middling weight, the last kept
    and the first dropped tie at the cut, a token outside, vocab + 5), plus a token kept by q only, one kept by p only and one
    outside both"""
    kw_p, kinds_p = base._drafts_of(p_row, temperature, top_k, top_p, probs_mode, boundary)
    kw_q, kinds_q = base._drafts_of(q_row, temperature, top_k, top_p, probs_mode, boundary)
    drafts = list(kinds_p) + list(kinds_q)
    if kw_p["w"] is not None:
        mp, mq = kw_p["mask"], kw_q["mask"]
        for sel in (mq & ~mp, mp & ~mq, ~mp & ~mq):
            idx = np.nonzero(sel)[0]
            if idx.size:
                drafts.append(int(idx[idx.size // 2]))
    return kw_p, kw_q, list(dict.fromkeys(drafts))


def _weights_of(kw_p, kw_q, d):
    n = kw_p["w"].size
    return (int(kw_p["w"][d]), int(kw_q["w"][d])) if 0 <= d < n else (0, 0)


def _u_acc_of(kw_p, kw_q, d):
    """0, the two grid neighbours of the acceptance threshold, the largest u"""
    us = [0.0, U_MAX]
    if kw_p["w"] is not None and kw_p["S"] > 0 and kw_q["S"] > 0:
        w_d, v_d = _weights_of(kw_p, kw_q, d)
        us += [u for u in svs.u_acc_around(w_d, v_d, kw_p["S"], kw_q["S"]) if u is not None]
    return list(dict.fromkeys(us))


def _nan_bonus_rows(q, drafts):
    """the draft row of a row without a draft is never read: poison it"""
    q = q.clone()
    for r, d in enumerate(drafts):
        if d < 0:
            q[r] = float("nan")
    return q


def _launch_and_compare(x, q, T, temps, ks, ps, drafts, us, kws, probs_mode=True):
    from chitu_amd import sampling

    out, acc, tok = sampling.speculative_verify_sampled(x, q, drafts, T, temps, ks, ps, uniforms=us, probs_mode=probs_mode, return_rows=True)
    want = [svs.verify_row_from(kws[r][0], kws[r][1], drafts[r], us[r][0], us[r][1]) for r in range(len(drafts))]
    want_acc, want_tok = [int(a) for a, _ in want], [t for _, t in want]
    assert acc.dtype == torch.int32 and tok.dtype == torch.int64 and out.dtype == torch.int64
    acc, tok = acc.cpu().tolist(), tok.cpu().tolist()
    for r in range(len(drafts)):
        assert (acc[r], tok[r]) == (want_acc[r], want_tok[r]), (r, drafts[r], us[r], acc[r], tok[r], want[r])
    assert np.array_equal(out.cpu().numpy(), sv.sequences(want_acc, want_tok, T))
    return want_acc


def _pack(combos, T, u_alts):
    """rows of T - 1 (draft, u_acc, u_alt) and one bonus row per sequence"""
    combos = list(combos)
    i = 0
    while len(combos) % (T - 1):
        combos.append(combos[i])
        i += 1
    drafts, us = [], []
    for s in range(len(combos) // (T - 1)):
        for d, ua, u in combos[s * (T - 1) : (s + 1) * (T - 1)]:
            drafts.append(d)
            us.append((ua, u))
        drafts.append(-1)
        us.append((0.5, u_alts[s % len(u_alts)]))
    return drafts, us


# ---------------------------------------------------------------- bit-exact in probability space
# (target kind, draft kind, vocab, T, top_k, top_p): every row kind on either side, the vocabularies around the 1024-thread,
# 1024-bin and 256-element segment steps, every T
CASES = [
    ("peaked", "peaked", 1000, 4, 50, 0.9), ("peaked", "flat", 1025, 2, -1, 0.9), ("flat", "peaked", 4099, 8, -1, 0.9),
    ("ties", "ties", 1000, 8, -1, 0.6), ("ties", "peaked", 1025, 4, 40, 0.8), ("equal", "ties", 300, 2, 7, 1.0),
    ("peaked", "equal", 300, 4, 7, 1.0), ("underflow", "peaked", 4099, 4, -1, 1.0), ("peaked", "underflow", 1025, 8, 30, 1.0),
    ("flat", "flat", 4099, 2, -1, 0.5), ("peaked", "ties", 1000, 2, 1, 0.9), ("equal", "equal", 1025, 4, 100, 0.9),
    ("peaked", "peaked", 129280, 4, 50, 0.9),
]


@pytest.mark.parametrize("kind_p,kind_q,vocab,T,top_k,top_p", CASES)
def test_probability_space_verification_is_bit_exact(kind_p, kind_q, vocab, T, top_k, top_p):
    """probs_mode: every operation of the kernel is an IEEE or an integer operation, so accepted, row_tokens and out equal the
    rule's.  Small vocabularies: every draft kind x every u_acc (0, the two grid neighbours of the threshold, the largest u) x u_alt
    in {0, 0.5, largest}, all on one pair of rows, with a bonus row (draft -1, NaN draft row) closing every sequence.  The full
    vocabulary: bs = 1, three drafts."""
    p = torch.softmax(base._rows(kind_p, 1, vocab, 7) / 0.8, dim=-1)[0]
    q = torch.softmax(base._rows(kind_q, 1, vocab, 8) / 0.9, dim=-1)[0]
    kw_p, kw_q, kinds = _pair_drafts(p.numpy(), q.numpy(), 1.0, top_k, top_p, True)
    u_alts = [0.0, 0.5, U_MAX]
    if vocab > 4099:
        picks = [kinds[0], kinds[1], int(kw_q["arg_max"])]
        ua = [_u_acc_of(kw_p, kw_q, d) for d in picks]
        combos = [(picks[0], ua[0][-1], 0.0), (picks[1], ua[1][-1], 0.5), (picks[2], U_MAX, U_MAX)]
    else:
        combos = [(d, ua, u) for d in kinds for ua in _u_acc_of(kw_p, kw_q, d) for u in u_alts]
    drafts, us = _pack(combos, T, u_alts)
    rows = len(drafts)
    x = p.cuda().repeat(rows, 1)
    qq = _nan_bonus_rows(q.repeat(rows, 1), drafts).cuda()
    acc = _launch_and_compare(x, qq, T, None, [top_k] * rows, [top_p] * rows, drafts, us, [(kw_p, kw_q)] * rows)
    if top_k != 1 and vocab <= 4099:
        assert 0 < sum(acc) < rows - rows // T  # both branches ran


def test_mixed_dtypes_strided_rows_and_parameters_per_row():
    """vocab 2001 (a ragged tail), every row pair with its own probabilities and parameters; the target rows and the draft rows in
    views whose rows start at odd element offsets (no wide loads), once f32 target with bf16 drafts and once the reverse"""
    T, rows, vocab = 4, 12, 2001
    ks = [50, 1, -1, 7, 2001, 3000, 2, 0, 100, 5, -1, 50]
    ps = [0.9, 0.5, 0.2, 1.0, 0.99, 0.8, 0.0, 0.6, 1.5, 0.0, 1.5, 0.3]
    for dt_p, dt_q in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
        p = torch.softmax(base._rows("peaked", rows, vocab, 11), dim=-1).to(dt_p)
        q = torch.softmax(base._rows("peaked", rows, vocab, 12) * 0.7, dim=-1).to(dt_q)
        kws, drafts, us = [], [], []
        for r in range(rows):
            kw_p, kw_q, kinds = _pair_drafts(p[r].float().numpy(), q[r].float().numpy(), 1.0, ks[r], ps[r], True)
            d = -1 if r % T == T - 1 else kinds[(r // T + 3 * (r % T)) % len(kinds)]
            ua = _u_acc_of(kw_p, kw_q, d)
            kws.append((kw_p, kw_q))
            drafts.append(d)
            us.append((ua[-1] if r % 2 else ua[-2] if len(ua) > 2 else ua[0], 0.1 * (r % 10) + 0.05))
        wide_p = torch.zeros(rows, vocab + 6, dtype=dt_p).cuda()
        wide_q = torch.zeros(rows, vocab + 10, dtype=dt_q).cuda()
        view_p, view_q = wide_p[:, 5 : 5 + vocab], wide_q[:, 3 : 3 + vocab]
        view_p.copy_(p)
        view_q.copy_(_nan_bonus_rows(q, drafts))
        _launch_and_compare(view_p, view_q, T, None, ks, ps, drafts, us, kws)


def test_identical_rows_always_accept_a_kept_draft():
    """p == q bit for bit: min(1, p / q) = 1, so every kept draft is accepted at every u_acc, the largest included; a draft that
    neither row keeps is rejected, and with R == 0 the row emits the arg-max"""
    from chitu_amd import sampling

    T, vocab = 4, 1025
    p = torch.softmax(base._rows("peaked", 1, vocab, 21), dim=-1)[0]
    kw, kinds = base._drafts_of(p.numpy(), 1.0, 40, 0.9, True)
    kept = [d for d in kinds if d < vocab and kw["w"][d] > 0]
    dropped = [d for d in kinds if d >= vocab or kw["w"][d] == 0]
    assert len(kept) >= 3 and len(dropped) >= 2
    combos = [(d, ua, 0.5) for d in kept + dropped for ua in (0.0, 0.5, U_MAX)]
    drafts, us = _pack(combos, T, [0.0, 0.5, U_MAX])
    rows = len(drafts)
    x = p.cuda().repeat(rows, 1)
    out, acc, tok = sampling.speculative_verify_sampled(x, x.clone(), drafts, T, None, [40] * rows, [0.9] * rows, uniforms=us,
                                                        probs_mode=True, return_rows=True)
    acc, tok = acc.cpu().tolist(), tok.cpu().tolist()
    for r, d in enumerate(drafts):
        if d in kept:
            assert (acc[r], tok[r]) == (1, d), (r, d, us[r])
        elif d >= 0:
            assert (acc[r], tok[r]) == (0, kw["arg_max"]), (r, d, us[r])
    _launch_and_compare(x, x.clone(), T, None, [40] * rows, [0.9] * rows, drafts, us, [(kw, kw)] * rows)


# ---------------------------------------------------------------- logits space
LOGIT_CASES = [("peaked", "peaked", 1000, 50, 0.9), ("ties", "peaked", 1000, -1, 0.6), ("equal", "peaked", 300, 7, 1.0),
               ("flat", "flat", 4099, -1, 0.9), ("underflow", "peaked", 4099, -1, 1.0), ("peaked", "ties", 1000, 1, 0.9),
               ("peaked", "flat", 1000, 2, 0.0)]


@pytest.mark.parametrize("kind_p,kind_q,vocab,top_k,top_p", LOGIT_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_logits_verification_within_exp_tolerance(kind_p, kind_q, vocab, top_k, top_p, dtype):
    """tests/test_gpu_spec_verify.py's logits test with the acceptance probability a = min(1, p(d) / q(d)) in the place of p(d): the
    GPU's exp is an ulp off numpy's, so u_acc is placed 2e-3 from a and `accepted` has to equal the reference's (drafts not at the
    edge of a kept set: whether such a token is kept may itself move with the ulp); the token is the reference's, or its interval
    in the residual CDF lies within 1e-4 of u_alt -- for one row per case at the most."""
    from chitu_amd import sampling

    T, rows = 4, 12
    temps = [0.8, 1.0, 0.5, 1.3, 0.7, 2.0] * 2
    x = base._rows(kind_p, rows, vocab, 3).to(dtype)
    q = base._rows(kind_q, rows, vocab, 4).to(dtype)
    u_alts = [0.0, U_MAX, 0.5, 0.123456, 0.87654, 0.3333]
    kws, drafts, us, a_d = [], [], [], []
    for r in range(rows):
        kw_p, kw_q, kinds = _pair_drafts(x[r].float().numpy(), q[r].float().numpy(), temps[r], top_k, top_p, False, boundary=False)
        d = -1 if r % T == T - 1 else kinds[(r // T + 3 * (r % T)) % len(kinds)]
        a = 0.0
        if kw_p["w"] is not None and kw_p["S"] > 0 and kw_q["S"] > 0 and d >= 0:
            w_d, v_d = _weights_of(kw_p, kw_q, d)
            a = 0.0 if w_d == 0 else 1.0 if v_d * kw_p["S"] <= w_d * kw_q["S"] else (w_d * kw_q["S"]) / (v_d * kw_p["S"])
        ua = a - 2e-3 if (r % 2 == 0 and a > 2e-3) or a + 2e-3 >= 1.0 else a + 2e-3
        kws.append((kw_p, kw_q))
        drafts.append(d)
        us.append((float(np.float32(ua)), u_alts[r % 6]))
        a_d.append(a)
    want = [svs.verify_row_from(kws[r][0], kws[r][1], drafts[r], us[r][0], us[r][1]) for r in range(rows)]
    out, acc, tok = sampling.speculative_verify_sampled(x.cuda(), _nan_bonus_rows(q, drafts).cuda(), drafts, T, temps, [top_k] * rows,
                                                        [top_p] * rows, uniforms=us, return_rows=True)
    acc, tok = acc.cpu().tolist(), tok.cpu().tolist()
    loose = 0
    for r in range(rows):
        assert abs(us[r][0] - a_d[r]) >= 1e-3
        assert bool(acc[r]) == bool(want[r][0]), (r, drafts[r], us[r], a_d[r], acc[r], want[r])
        if tok[r] == want[r][1]:
            continue
        assert not want[r][0] and top_k != 1, (r, tok[r], want[r])
        if drafts[r] < 0:
            w = kws[r][0]["w"].astype(np.float64)
        else:
            res, R = svs.residual(kws[r][0], kws[r][1])
            w = np.array([ri / R for ri in res], dtype=np.float64)
        dist = w / w.sum()
        cdf = np.cumsum(dist)
        t = tok[r]
        assert 0 <= t < vocab and cdf[t] - dist[t] - 1e-4 <= us[r][1] <= cdf[t] + 1e-4, (r, t, want[r], cdf[t] - dist[t], cdf[t], us[r])
        loose += 1
    assert loose <= 1
    assert np.array_equal(out.cpu().numpy(), sv.sequences(acc, tok, T))


# ---------------------------------------------------------------- distribution
@pytest.mark.parametrize("draft_scale", [0.7, 0.2, 2.0])
def test_emitted_tokens_follow_the_target_distribution(draft_scale):
    """8192 sequences of T = 2 on one target row (vocab 300, temperature 0.9, top-k 12, top-p 0.95): the draft is DRAWN by
    chitu_hip_sample from a draft row (another peaked row, close to, flatter than or sharper than the target) under the same
    parameters, then verified.  The first emitted token's histogram within 5 sigma + 1 of the target's kept distribution per
    token (tests/test_gpu_sampler.py's bound), nothing outside the target's kept set."""
    from chitu_amd import sampling

    n, T, vocab = 8192, 2, 300
    row = base._rows("peaked", 1, vocab, 5) * 0.7
    qrow = row * draft_scale / 0.7 + base._rows("peaked", 1, vocab, 6) * 0.1
    dist = osmp.kept_distribution(row[0].numpy(), 0.9, 12, 0.95)
    x = row.cuda().expand(n * T, vocab).contiguous()
    q = qrow.cuda().expand(n * T, vocab).contiguous()
    gen = torch.Generator(device="cuda").manual_seed(4321)
    params = ([0.9] * (n * T), [12] * (n * T), [0.95] * (n * T))
    drawn = sampling.top_k_top_p_sampling_from_logits(q, *params, generator=gen).to(torch.int32)
    drawn[1::2] = -1
    out, acc, _ = sampling.speculative_verify_sampled(x, q, drawn, T, *params, generator=gen, return_rows=True)
    out, acc = out.cpu().numpy(), acc.cpu().numpy()
    counts = np.bincount(out[:, 1], minlength=vocab).astype(np.float64)
    sigma = np.sqrt(n * dist * (1 - dist))
    worst = float(np.max(np.abs(counts - n * dist)[dist > 0] / sigma[dist > 0]))
    print(f"SPEC_VERIFY_SAMPLED distribution, draft scale {draft_scale}: accepted {int(acc[0::2].sum())} of {n}, worst deviation {worst:.2f} sigma")
    assert counts[dist == 0].sum() == 0
    assert (np.abs(counts - n * dist) <= 5 * sigma + 1).all()
    assert np.array_equal(out[:, 0], 1 + acc[0::2]) and not acc[1::2].any()
    assert 0 < acc[0::2].sum() < n
    bonus = out[out[:, 0] == 2, 2]
    assert (dist[bonus] > 0).all() and (out[out[:, 0] == 1, 2] == -1).all()


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_two_launches_and_a_graph_replay_agree(kind):
    from chitu_amd import sampling

    bs, T, vocab = 8, 4, 4099
    rows = bs * T
    x = base._rows(kind, rows, vocab, 9).cuda()
    q = base._rows(kind, rows, vocab, 10).cuda()
    temps = torch.full((rows,), 0.8, device="cuda")
    ks = torch.full((rows,), -1 if kind == "flat" else 40, dtype=torch.int32, device="cuda")
    ps = torch.full((rows,), 0.9, device="cuda")
    drafts = x.argmax(dim=-1).to(torch.int32)  # the target's likeliest token is always kept by p: u_acc = 0 accepts it
    drafts[T - 1 :: T] = -1
    us = torch.rand(rows, 2, generator=torch.Generator().manual_seed(1)).cuda()
    us[::2, 0] = 0.0
    a = sampling.speculative_verify_sampled(x, q, drafts, T, temps, ks, ps, uniforms=us, return_rows=True)
    b = sampling.speculative_verify_sampled(x, q, drafts, T, temps, ks, ps, uniforms=us, return_rows=True)
    for p_, q_ in zip(a, b):
        assert torch.equal(p_, q_)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = sampling.speculative_verify_sampled(x, q, drafts, T, temps, ks, ps, uniforms=us, return_rows=True)
    graph.replay()
    torch.cuda.synchronize()
    for p_, q_ in zip(a, c):
        assert torch.equal(p_, q_)
    out, acc, tok = (t.cpu().numpy() for t in a)
    acc, tok = acc.reshape(bs, T), tok.reshape(bs, T)
    for s in range(bs):
        lead = 0
        while lead < T - 1 and acc[s, lead]:
            lead += 1
        assert out[s, 0] == 1 + lead
        assert np.array_equal(out[s, 1 : 2 + lead], tok[s, : lead + 1]) and (out[s, 2 + lead :] == -1).all()
    assert acc[:, 0].all() and not acc[:, T - 1].any()
