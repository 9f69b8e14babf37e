"""The sampler of csrc/sample.hip (chitu_amd.sampling) at every edge of the candidate list and of the radix descent, with equality
assertions only: the cases and expected values of tests/sample_exact.py (checked on the CPU by tests/test_sample_exact_host.py),
each on both sampler paths (the `sample_radix` option) and in a dense and a column-offset view.

  probability space   token and n_kept equal the integer specification's; kept_mass is the integer ratio S / Z within the one
                      float rounding of the kernel's double -> float conversion
  verification        A5, B2 and B3 as T = 2 sequences of speculative_verify(probs_mode=True): accepted, row_tokens and out equal
                      tests/spec_verify_ref.py's, the bonus row returns the sampler's token
  logits space        grid logits admitted with a margin of 2^-12 around every decision: token and n_kept EQUAL the
                      specification's on every row, in fp32 / bf16 / fp16; the probability-space twin tells a failure of the
                      device's exp from one of the selection
  special values      -inf / +inf / NaN of either sign / fp16 subnormals and +-65504: greedy equals torch.argmax on the CPU
                      tensor, sampling equals the specification

What this file found: ordered_key() gave a NaN with the sign bit set (0xffc00000, what inf - inf yields on x86) a key below -inf,
so greedy returned the arg-max of the other elements and sampling drew as if the NaN were absent, where torch.argmax and
oracle/sampling.py return the NaN's index.  Seen on the MI355X in all three storage types and on both paths
(test_special_values: neg-nan-0 / -513 / -1026 gave 400, neg-nan-beside-pinf gave 100 for 50); fixed in csrc/sample.hip: every
NaN takes the top key.

Mutations of csrc/sample.hip tried by hand on the MI355X (other builds of the library, never committed; value-only: none can
read or write out of bounds) and what caught them here.  [c] / [r]: under the candidates / radix fixture.
  - pass 2 `key >= tkey` -> `>`: probs A2 [c] (the only cases with entries exactly at the CHOSEN level's threshold).
  - list cut `excl <= p_rem` -> `<`: probs A5 [c], verify A5 [c] (p_rem exactly the exclusive sum in front of a tie).
  - list cut `tid < k_eff` -> `<=`: probs A1 A2 A3 A5 B2 B6 [c], verify A5 B2 [c], logits and twins [c]; 23 tests.
  - the sort's index tie-break reversed: probs A1-A5 B2 [c], verify A5 B2 [c], logits and twins of vocab >= 257 [c], special
    float16 [c]; 21 tests.
  - rescan `rank < c_keep` -> `<=`: probs B3 B6 and verify B3 on both fixtures (the list declines these rows).
  - `c_p = p_rem / e_tau + 1` without the `+ 1`: probs A1 A3 B1 B4 [c] and A1-A5 B1 B4 B6 [r], verify A5 [r], every logits
    and twin test [r]; 29 tests.
  - rescan `ties_run` not carried between chunks: probs B3 B6 and verify B3 on both fixtures.
  - boundary walk `s_incl > p_rem` -> `>=` (and s_excl alike): probs A5 [r], verify A5 [r].
  - verify: `i0 + k < r.draft` -> `<=` in ties_below, and `rank < c_keep` -> `<=` for the draft: verify B2 B3 [c + r], A5 [r].
  - verify: the draft's segment keeps w_d in the segment sums: verify A5 [r].
  - verify: the rescan does not zero the rejected draft: first run NOT caught -- no replacement draw landed behind a rejected
    draft inside its segment; verify_rows() now aims one at both ends of the interval of the draft's kept neighbours and of the
    last kept token of its segment: verify B2 B3 [c + r], A5 [r].
  - verify: the list's second sort keeps the rejected draft (`in_draw = kept`): verify A5 B2 [c].
  Not caught, and not catchable by value:
  - `counts[j] <= kCandCap` -> `<`, and dropping `|| n_cand == vocab`: the row falls back to the radix descent, which evaluates
    the same specification ("which one ran cannot be told from the result").  Which path a case takes is pinned on the CPU
    (tests/test_sample_exact_host.py, against oracle.sampling.sample_candidate_model).
  - boundary walk `c_incl >= k_rem` -> `>`: the descent stops one key lower with c_keep = 0, the same kept set.
  - `seg_len` rounded up to 4 in place of 256: still a partition of the row into 16 quad-aligned segments, the same answers
    (the round-up to 256 only aligns segments with the 256-element chunks).  Dropping the round-up altogether breaks load4's
    `i0 % 4 == 0` precondition (misaligned wide loads) and was not run."""

import numpy as np
import pytest
import torch

from tests import sample_exact as se

pytestmark = pytest.mark.gpu


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


def _views(rows2d):
    """the rows on the device, dense and as a column-offset view of a wider tensor (odd row stride: no wide loads on odd rows)"""
    dense = rows2d.cuda()
    rows, vocab = dense.shape
    wide = torch.zeros(rows, vocab + 3 + vocab % 2, dtype=dense.dtype, device="cuda")
    view = wide[:, 1: 1 + vocab]
    view.copy_(dense)
    assert wide.stride(0) % 2 == 1
    return (("dense", dense), ("offset", view))


def _mass_ok(got, s, z):
    f = np.float32(s / z)
    return np.float32(got) in (f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(2)))


@pytest.mark.parametrize("name", list(se.GROUPS))
def test_probability_space_cases_equal_the_specification(name, sampler_path):
    from chitu_amd import sampling

    draws = launches = 0
    for case in se.group(name):
        want = case.expected()
        rows = len(case.draws)
        ks, ps, us = ([d[i] for d in case.draws] for i in range(3))
        for view_name, x in _views(torch.from_numpy(case.row).repeat(rows, 1)):
            tok, n_kept, mass = sampling.top_k_top_p_min_p_sampling_from_probs_torch(x, ks, ps, uniforms=us, return_stats=True)
            tok, n_kept, mass = tok.cpu().numpy(), n_kept.cpu().numpy(), mass.cpu().numpy()
            launches += 1
            for r in range(rows):
                got = (int(tok[r]), int(n_kept[r]))
                assert got == want[r][:2], (case.name, view_name, r, case.draws[r], got, want[r][:2], case.reach[r])
                assert _mass_ok(mass[r], want[r][2], want[r][3]), (case.name, view_name, r, float(mass[r]), want[r][2] / want[r][3])
                draws += 1
    print(f"SAMPLE_EXACT probs {name}/{sampler_path}: {draws} draws in {launches} launches, token / n_kept equal, kept_mass within one rounding")


@pytest.mark.parametrize("name", se.VERIFY_GROUPS)
def test_verification_rows_equal_the_rule(name, sampler_path):
    from chitu_amd import sampling

    total = accepted = 0
    for case in se.group(name):
        v = se.verify_rows(case)
        rows = len(v["drafts"])
        for view_name, x in _views(torch.from_numpy(case.row).repeat(rows, 1)):
            out, acc, tok = sampling.speculative_verify(x, v["drafts"], 2, None, v["top_ks"], v["top_ps"], uniforms=v["uniforms"],
                                                        probs_mode=True, return_rows=True)
            acc, tok = acc.cpu().numpy().tolist(), tok.cpu().numpy().tolist()
            for r in range(rows):
                assert (acc[r], tok[r]) == (v["accepted"][r], v["tokens"][r]), (
                    case.name, view_name, r, v["drafts"][r], v["top_ks"][r], v["top_ps"][r], v["uniforms"][r], acc[r], tok[r],
                    v["accepted"][r], v["tokens"][r])
            assert tok[1::2] == v["bonus_want"]  # the bonus row is the sampler's row
            assert np.array_equal(out.cpu().numpy(), v["out"])
        total += rows
        accepted += sum(v["accepted"])
    print(f"SAMPLE_EXACT verify {name}/{sampler_path}: {total} rows ({accepted} accepted) x 2 views, accepted / row_tokens / out equal")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("vocab", se.LOGIT_VOCABS)
def test_logits_space_cases_equal_the_specification(vocab, dtype, sampler_path):
    """Grid logits with a margin of 2^-12 around every decision (32 times the bound on the device's exp): token and n_kept are
    the specification's on every row.  On the MI355X all 178 admitted draws are equal in fp32, bf16 and fp16, dense and offset, on
    both paths; the probability-space twins (next test) pass too, so nothing here had to be attributed to the device's exp."""
    from chitu_amd import sampling

    cases = [c for c in se.logits_cases() if c.x.size == vocab]
    x = torch.from_numpy(np.stack([c.x for c in cases for _ in c.draws])).to(dtype)
    assert torch.equal(x.float(), torch.from_numpy(np.stack([c.x for c in cases for _ in c.draws])))  # exact in the type
    temps = [c.temperature for c in cases for _ in c.draws]
    ks, ps, us = ([d[i] for c in cases for d in c.draws] for i in range(3))
    want = [w for c in cases for w in c.expected]
    names = [c.name for c in cases for _ in c.draws]
    for view_name, xd in _views(x):
        tok, n_kept, _ = sampling.top_k_top_p_sampling_from_logits(xd, temps, ks, ps, uniforms=us, return_stats=True)
        tok, n_kept = tok.cpu().numpy(), n_kept.cpu().numpy()
        bad = [(names[r], view_name, ks[r], ps[r], us[r], int(tok[r]), int(n_kept[r]), want[r]) for r in range(len(want))
               if (int(tok[r]), int(n_kept[r])) != want[r]]
        assert not bad, bad
    print(f"SAMPLE_EXACT logits vocab {vocab} {dtype}/{sampler_path}: {len(want)} admitted draws x 2 views, token / n_kept equal")


@pytest.mark.parametrize("vocab", se.LOGIT_VOCABS)
def test_logits_space_twins_in_probability_space(vocab, sampler_path):
    """The oracle's weights of every logits case passed as probabilities: the same answers without the device's exp."""
    from chitu_amd import sampling

    cases = [c for c in se.logits_cases() if c.x.size == vocab]
    x = torch.from_numpy(np.stack([c.twin() for c in cases for _ in c.draws]))
    ks, ps, us = ([d[i] for c in cases for d in c.draws] for i in range(3))
    want = [w for c in cases for w in c.expected]
    tok, n_kept, _ = sampling.top_k_top_p_min_p_sampling_from_probs_torch(x.cuda(), ks, ps, uniforms=us, return_stats=True)
    got = list(zip(tok.cpu().numpy().tolist(), n_kept.cpu().numpy().tolist()))
    assert got == want
    print(f"SAMPLE_EXACT twins vocab {vocab}/{sampler_path}: {len(want)} draws, token / n_kept equal")


@pytest.mark.parametrize("fmt", list(se.FORMATS))
def test_special_values(fmt, sampler_path):
    """-inf padding and masks, +inf, NaN of either sign, fp16 subnormals and +-65504: greedy is torch.argmax of the CPU tensor
    (the first NaN, else the first maximum), sampling is the specification (a row without positive weight emits its arg-max)."""
    from chitu_amd import sampling

    dtype = getattr(torch, fmt)
    rows = se.special_rows(fmt)
    greedy = sampled = 0
    for vocab in sorted({r.bits.size for r in rows}):
        group = [r for r in rows if r.bits.size == vocab]
        bits = np.stack([r.bits for r in group])
        x = torch.from_numpy(bits.view(np.int32 if fmt == "float32" else np.int16)).view(dtype)
        want_greedy = torch.argmax(x, dim=-1).numpy()
        exp = [(i, e) for i, r in enumerate(group) for e in se.special_expected(r, fmt)]
        xs = x[[i for i, _ in exp]]
        temps, ks, ps, us = ([e[j] for _, e in exp] for j in range(4))
        for (view_name, xd), (_, xsd) in zip(_views(x), _views(xs)):
            assert np.array_equal(xd.cpu().view(torch.int32 if fmt == "float32" else torch.int16).numpy(),
                                  bits.view(np.int32 if fmt == "float32" else np.int16))  # the patterns arrived
            got = sampling.argmax(xd).cpu().numpy()
            bad = [(group[i].name, view_name, int(got[i]), int(want_greedy[i])) for i in range(len(group)) if got[i] != want_greedy[i]]
            assert not bad, ("greedy", bad)
            tok, n_kept, _ = sampling.top_k_top_p_sampling_from_logits(xsd, temps, ks, ps, uniforms=us, return_stats=True)
            tok, n_kept = tok.cpu().numpy(), n_kept.cpu().numpy()
            bad = [(group[i].name, view_name, e[:4], int(tok[r]), int(n_kept[r]), e[4:]) for r, (i, e) in enumerate(exp)
                   if (int(tok[r]), int(n_kept[r])) != e[4:]]
            assert not bad, ("sampling", bad)
        greedy += len(group)
        sampled += len(exp)
    print(f"SAMPLE_EXACT special {fmt}/{sampler_path}: {greedy} greedy rows, {sampled} sampling rows x 2 views, all equal")
