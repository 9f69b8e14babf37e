"""CPU self-check of the exact per-key attention tests: every builder of tests/attn_exact.py goes through oracle/gqa.py and
oracle/mla.py (fp32, rounded to bf16 like a kernel's output) and through the CPU statement of the two fp8 row formats, and every
condition the GPU assertions of tests/test_gpu_attn_exact.py rest on is asserted here.  A construction the reference cannot
pass is a bug in the test.  The reference's own error under each construction is printed (pytest -s)."""
import math

import pytest
import torch

from oracle import gqa as ogqa
from oracle import mla as omla
from tests import attn_exact as ax
from tests import test_gqa_kv_fp8_host as g8
from tests import test_mla_kv_fp8_host as m8
from tests.util import assert_close

GQA_HEADS = [(4, 4), (8, 2), (16, 1)]
GQA_PAGES = [16, 48, 256]
GQA_SPLITS = [1, 2, 3, 5, 8, 17]
MLA_SPLITS = [1, 2, 3, 4, 5, 7]


def as_bf16(x):
    return x.to(torch.bfloat16)


def report(what, err):
    print(f"ATTN_EXACT oracle {what}: {err:.3e}")


# ---------------------------------------------------------------- what the constructions promise
def test_no_position_channel_counts_more_than_16_keys():
    for n in (130, 1024):
        assert ax.max_keys_per_position_channel(ax.count_rows(n, [3, 10, 17, 24], 128, ax.P_GQA, ax.STEP_GQA), ax.P_GQA) <= 16
    for n in (258, 4096):
        assert ax.max_keys_per_position_channel(ax.count_rows(n, [3], 512, ax.P_MLA, ax.TILE), ax.P_MLA) <= 16
    assert ax.max_keys_per_position_channel(ax.count_rows(1025, [3], 128, ax.P_GQA, ax.STEP_GQA), ax.P_GQA) == 17  # the limit is tight
    for Hkv, width, P in ((8, 128, ax.P_GQA), (1, 512, ax.P_MLA)):
        c = ax.prefill_count_case(ax.PREFILL_SEQS, Hkv, Hkv, width, P)
        for s0, s1 in zip(c["cu"][:-1], c["cu"][1:]):
            assert ax.max_keys_per_position_channel(c["v"][s0:s1], P) <= 16
        # the smallest effect of one key more or less on a channel that is set: 1 / (n_d + 1) >= 1 / 17 > twice the bar
        assert 1.0 / 17 > 2 * ax.REL_COUNT
    # a head's offset moves both fields: no two KV heads (or sequences) share a row
    rows = ax.count_rows(130, [7 * h + 3 for h in range(8)], 128, ax.P_GQA, ax.STEP_GQA)
    assert len(torch.unique(rows.transpose(0, 1).reshape(8, -1), dim=0)) == 8
    assert float(rows.sum(-1).min()) == 2 and float(rows.sum(-1).max()) == 2 and float(rows.max()) == 1


def test_identity_rows_are_pairwise_distinct_by_at_least_one():
    flat = [ax.identity_rows(130, 4, 128).reshape(-1, 128), ax.identity_rows(ax.LONG_N, 1, 512).reshape(-1, 512)]
    flat.append(torch.cat([ax.identity_rows(n, 8, 128, seq=s).reshape(-1, 128) for s, n in enumerate(ax.PREFILL_SEQS)]))
    for r in flat:
        assert torch.equal(r, r.round()) and float(r.min()) >= 0 and float(r.max()) <= 15  # integers: distinct rows differ by >= 1
        assert len(torch.unique(r, dim=0)) == len(r)
        assert torch.equal(as_bf16(r).float(), r)


def test_margins_and_the_leak_of_the_other_keys():
    for scale in (ax.GQA_SCALE, ax.MLA_SCALE):
        m = ax.margin_nats(ax.Q_AMP, ax.K_AMP, scale)
        assert m >= ax.MIN_MARGIN_NATS and m >= 45.0, m
        assert ax.leak_bound(ax.LONG_N, 15.0, m) < ax.ABS_DOMINANT * 1e-6
    assert ax.leak_bound(130, 15.0, ax.margin_nats(ax.Q_AMP, ax.K_AMP, ax.GQA_SCALE)) < 4.3e-17 * 1.01


def test_graded_margins_sit_on_both_sides_of_each_kernels_deferral_constant():
    """gqa_decode_tile.h defers in nats; the two flash prefill kernels in log2 units.  mla_decode_tile.h's tile step has no deferral
    constant (it rescales on every tile): its graded cases use the MLA prefill kernel's margins and are plain arithmetic checks."""
    gd = ax.source_constant("gqa_decode_tile.h", "kGqaDefer")
    gp = ax.source_constant("gqa_prefill_flash.hip", "kDefer")
    mp = ax.source_constant("mla_prefill_flash.hip", "kDefer")
    assert (gd, gp, mp) == (6.0, 8.0, 8.0)
    for const, scale, unit in ((gd, ax.GQA_SCALE, 1.0), (gp * math.log(2), ax.GQA_SCALE, math.log(2)), (mp * math.log(2), ax.MLA_SCALE, math.log(2))):
        ks, leads = ax.graded_amplitudes(const, scale)
        for k in ks:
            assert float(as_bf16(torch.tensor(k))) == k
        lo, hi = leads[0] / unit, leads[1] / unit
        assert 0.9 * const / unit < lo < 0.99 * const / unit and 1.01 * const / unit < hi < 1.1 * const / unit, (lo, hi, const / unit)


# ---------------------------------------------------------------- GQA decode through oracle/gqa.py
def gqa_oracle(case, page, fp8=False):
    kc, vc, table = ax.gqa_pages(case, page, seed=page)
    if fp8:
        shape = kc.shape
        k8, v8 = (g8.quant_ref(c.view(-1, shape[2], 128)) for c in (kc, vc))
        for c8, c in ((k8, kc), (v8, vc)):  # the rows were chosen for this
            assert torch.equal(g8.dequant_ref(c8).view(torch.int16), c.view(-1, shape[2], 128).view(torch.int16))
        kc, vc = g8.dequant_ref(k8).view(shape), g8.dequant_ref(v8).view(shape)
    out, _, _ = ogqa.attn_with_kvcache(case["q"], kc, vc, None, None, case["lens"], table, softmax_scale=ax.GQA_SCALE)
    return out[:, 0]


@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
def test_gqa_decode_counting(Hq, Hkv):
    c = ax.gqa_count_case(130, Hq, Hkv)
    assert float((ax.decode64(c["q"][:, 0], c["K"], c["V"], c["lens"], ax.GQA_SCALE) - c["want"]).abs().max()) < 1e-14
    worst = 0.0
    for page in GQA_PAGES:
        for fp8 in (False, True):
            out = gqa_oracle(c, page, fp8)
            worst = max(worst, ax.check_count(as_bf16(out), c["want"]))
            assert ax.check_count(out, c["want"]) < 1e-6
    report(f"gqa decode counting Hq={Hq} Hkv={Hkv}, rounded to bf16, relative", worst)
    assert worst <= 2.0 ** -8


@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
@pytest.mark.parametrize("n", [17, 64, 130])
def test_gqa_decode_dominant_key(n, Hq, Hkv):
    worst = 0.0
    for page in GQA_PAGES:
        probes = ax.probe_tokens(n, ax.STEP_GQA, page, GQA_SPLITS)
        assert {0, n - 1} <= set(probes) and all(0 <= t < n for t in probes)
        c = ax.gqa_dominant_case(n, Hq, Hkv, probes)
        assert float((ax.decode64(c["q"][:, 0], c["K"], c["V"], c["lens"], ax.GQA_SCALE) - c["want"]).abs().max()) < 1e-15
        for fp8 in (False, True):
            out = gqa_oracle(c, page, fp8)
            worst = max(worst, ax.check_dominant(out, c["want"]))
    report(f"gqa decode dominant key n={n} Hq={Hq} Hkv={Hkv}, absolute", worst)
    assert worst <= ax.leak_bound(n, 15.0, ax.margin_nats(ax.Q_AMP, ax.K_AMP, ax.GQA_SCALE))


def test_probe_sets_hold_both_sides_of_every_edge():
    assert ax.split_edges(130, 16, [3]) == [48, 96] and ax.split_edges(130, 16, [17]) == [0, 16, 32, 48, 64, 80, 96, 112, 128]
    p = ax.probe_tokens(130, 16, 48, GQA_SPLITS)
    for e in (16, 48, 96, 128):
        assert e - 1 in p and e in p
    assert ax.probe_tokens(17, 16, 256, [1]) == [0, 15, 16]
    p = ax.probe_tokens(258, 64, 128, MLA_SPLITS)
    assert p == [0, 63, 64, 127, 128, 191, 192, 255, 256, 257]


def test_gqa_decode_graded_margin():
    ks, leads = ax.graded_amplitudes(ax.source_constant("gqa_decode_tile.h", "kGqaDefer"), ax.GQA_SCALE)
    c = ax.gqa_graded_case(130, 8, 2, ks, tokens=[5, 120])
    assert all(t // 16 not in (0, 6) or t < 16 for t in (5, 120))  # 120: neither in the first step of the sequence nor of a split of 3 (steps 0, 3, 6)
    out = gqa_oracle(c, 16)
    assert_close(as_bf16(out), c["want"], 1e-2)


# ---------------------------------------------------------------- MLA decode through oracle/mla.py
def mla_oracle(case, page, fp8=False):
    cache, table = ax.mla_pages(case, page, seed=page)
    if fp8:
        c8 = m8.quant_ref(cache.view(-1, 576))
        assert torch.equal(m8.dequant_ref(c8).view(torch.int16), cache.view(-1, 576).view(torch.int16))
        cache = m8.dequant_ref(c8).view(cache.shape)
    return omla.mla_decode(case["q_nope"], case["q_pe"], cache, table, case["lens"], ax.MLA_SCALE)


@pytest.mark.parametrize("H", [16, 32, 5])
def test_mla_decode_counting(H):
    c = ax.mla_count_case(258, H)
    assert float((ax.mla_decode64(c) - c["want"]).abs().max()) < 1e-14
    worst = 0.0
    for page in (64, 128, 192):
        for fp8 in (False, True):
            worst = max(worst, ax.check_count(as_bf16(mla_oracle(c, page, fp8)), c["want"]))
    report(f"mla decode counting H={H}, rounded to bf16, relative", worst)
    assert worst <= 2.0 ** -8


@pytest.mark.parametrize("n", [17, 64, 130, 258])
def test_mla_decode_dominant_key(n):
    worst = 0.0
    for page in (64, 128):
        c = ax.mla_dominant_case(n, 16, ax.probe_tokens(n, ax.TILE, page, MLA_SPLITS))
        assert float((ax.mla_decode64(c) - c["want"]).abs().max()) < 1e-15
        for fp8 in (False, True):
            out = mla_oracle(c, page, fp8)
            worst = max(worst, ax.check_dominant(out, c["want"]))
    report(f"mla decode dominant key n={n}, absolute", worst)


def test_mla_decode_long_path_probes():
    assert ax.LONG_N > ax.TILE * ax.source_constant("mla_decode_tile.h", "kMaxTilesLds") and max(ax.LONG_PROBES) < ax.LONG_N
    c = ax.mla_dominant_case(ax.LONG_N, 16, ax.LONG_PROBES)
    cache, table = ax.mla_pages(c, 64)
    assert cache.numel() * 2 < 40e6 and table.shape[1] == 517
    c8 = m8.quant_ref(cache.view(-1, 576))
    assert torch.equal(m8.dequant_ref(c8).view(torch.int16), cache.view(-1, 576).view(torch.int16))
    out = omla.mla_decode(c["q_nope"], c["q_pe"], cache, table, c["lens"], ax.MLA_SCALE)
    report("mla decode dominant key n=33000, absolute", ax.check_dominant(out, c["want"]))
    assert {int(w[0]) + 16 * int(w[1]) + 256 * int(w[2]) + 4096 * int(w[3]) for w in c["want"][0]} == set(ax.LONG_PROBES)


def test_mla_decode_graded_margin():
    ks, _ = ax.graded_amplitudes(ax.source_constant("mla_prefill_flash.hip", "kDefer") * math.log(2), ax.MLA_SCALE)
    c = ax.mla_graded_case(258, 16, ks, tokens=[5, 200])
    assert_close(as_bf16(mla_oracle(c, 64)), c["want"], 1e-2)


# ---------------------------------------------------------------- prefill through the oracles
@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (8, 2), (32, 1)])
def test_gqa_prefill_constructions(Hq, Hkv):
    c = ax.prefill_count_case(ax.PREFILL_SEQS, Hq, Hkv, 128, ax.P_GQA)
    assert float((ax.prefill64(c["q"], c["k"], c["v"], c["cu"], ax.GQA_SCALE) - c["want"]).abs().max()) < 1e-14
    out = ogqa.attn_varlen_causal(as_bf16(c["q"]), as_bf16(c["k"]), as_bf16(c["v"]), c["cu"])
    report(f"gqa prefill counting Hq={Hq} Hkv={Hkv}, rounded to bf16, relative", ax.check_count(as_bf16(out), c["want"]))
    d = ax.prefill_dominant_case(ax.PREFILL_SEQS, Hq, Hkv, 128)
    out = ogqa.attn_varlen_causal(as_bf16(d["q"]), as_bf16(d["k"]), as_bf16(d["v"]), d["cu"])
    report(f"gqa prefill tied dominant keys Hq={Hq} Hkv={Hkv}, rounded to bf16, relative", ax.check_tied(as_bf16(out), d["want"]))
    # rows with fewer than 129 keys have no tie: the expectation is the diagonal key's own row
    for s, (s0, s1) in enumerate(zip(d["cu"][:-1], d["cu"][1:])):
        m = min(s1 - s0, 128)
        assert float((d["want"][s0 : s0 + m] - d["v"][s0 : s0 + m].double().repeat_interleave(Hq // Hkv, dim=1)).abs().max()) < 1e-15
    ks, _ = ax.graded_amplitudes(ax.source_constant("gqa_prefill_flash.hip", "kDefer") * math.log(2), ax.GQA_SCALE)
    e = ax.prefill_graded_case(200, Hq, Hkv, 128, ks, tokens=[5, 150])
    assert_close(as_bf16(ogqa.attn_varlen_causal(as_bf16(e["q"]), as_bf16(e["k"]), as_bf16(e["v"]), e["cu"])), e["want"], 1e-2)


@pytest.mark.parametrize("H", [16, 5])
def test_mla_prefill_constructions(H):
    c = ax.prefill_count_case(ax.PREFILL_SEQS, H, 1, 512, ax.P_MLA)
    out = omla.mla_prefill(as_bf16(c["q"]), as_bf16(c["k"])[:, 0], c["cu"], ax.MLA_SCALE)
    report(f"mla prefill counting H={H}, rounded to bf16, relative", ax.check_count(as_bf16(out), c["want"]))
    d = ax.prefill_dominant_case(ax.PREFILL_SEQS, H, 1, 512)
    out = omla.mla_prefill(as_bf16(d["q"]), as_bf16(d["k"])[:, 0], d["cu"], ax.MLA_SCALE)
    report(f"mla prefill tied dominant keys H={H}, rounded to bf16, relative", ax.check_tied(as_bf16(out), d["want"]))
    ks, _ = ax.graded_amplitudes(ax.source_constant("mla_prefill_flash.hip", "kDefer") * math.log(2), ax.MLA_SCALE)
    e = ax.prefill_graded_case(200, H, 1, 512, ks, tokens=[5, 150])
    assert_close(as_bf16(omla.mla_prefill(as_bf16(e["q"]), as_bf16(e["k"])[:, 0], e["cu"], ax.MLA_SCALE)), e["want"], 1e-2)


def test_every_built_value_is_exact_in_bf16():
    cases = [ax.gqa_count_case(130, 8, 2), ax.gqa_dominant_case(130, 8, 2, [0, 129]), ax.mla_count_case(258, 16),
             ax.mla_dominant_case(130, 16, [0, 129]), ax.prefill_dominant_case([3, 200], 8, 2, 128), ax.prefill_count_case([3, 200], 16, 1, 512, ax.P_MLA)]
    for c in cases:
        for key in ("K", "V", "rows", "k", "v", "q"):
            if key in c and c[key].dtype == torch.float32:
                assert torch.equal(as_bf16(c[key]).float(), c[key]), key


@pytest.mark.parametrize("Hq,Hkv,width", [(8, 8, 128), (8, 2, 128), (32, 1, 128), (16, 1, 512), (5, 1, 512)])
def test_prefill_graded_case_keeps_a_wave_on_one_side_of_the_constant(Hq, Hkv, width):
    """Both flash kernels vote on the rescale per wave (32 Q rows: several tokens x the heads of a group), and a workgroup never
    spans two sequences: every head and every query row of a sequence must steer to the same channel, and only one key of that
    sequence may be set there -- else a row above the constant makes the wave of a row below it rescale too."""
    e = ax.prefill_graded_case(200, Hq, Hkv, width, [3.0, 5.0], tokens=[5, 150])
    assert len(e["combos"]) == 4 and e["cu"] == [0, 200, 400, 600, 800]
    steer = e["q"][..., e["base"] : e["base"] + 4]
    for c, (t, a) in enumerate(e["combos"]):
        s0, s1 = e["cu"][c], e["cu"][c + 1]
        assert bool((steer[s0:s1, :, c] == 8.0).all()) and float(steer[s0:s1].sum()) == 8.0 * 200 * Hq  # one channel, the same for all
        assert float(e["q"][s0:s1].abs().sum()) == 8.0 * 200 * Hq  # and nothing else in q
        col = e["k"][s0:s1, :, e["base"] : e["base"] + 4]
        assert bool((col[t, :, c] == a).all()) and float(col.abs().sum()) == a * Hkv  # one key of the sequence, in that channel only


def test_beyond_4gib_cases_through_the_oracles():
    """ax.big_gqa_cases / ax.big_mla_cases: the same bounds, bf16 and fp8 rows, with the fills the GPU test leaves in the rest of a page"""
    for c in ax.big_gqa_cases(32, 8, 256):
        assert (c["k_fill"], c["v_fill"]) in ((ax.K_AMP, 1.0), (ax.K_AMP, 15.0))
        c = dict(c, v_fill=1.0)
        for fp8 in (False, True):
            out = gqa_oracle(c, 256, fp8)
            err = ax.check_dominant(out, c["want"]) if bool(c["q"].any()) else ax.check_count(as_bf16(out), c["want"])
        report(f"gqa beyond-4-GiB case n={int(c['lens'][0])}", err)
    rows = [c["V"] for c in ax.big_gqa_cases(32, 8, 256)]
    assert not torch.equal(rows[0], rows[1][:17]) and not torch.equal(rows[2], rows[3][:17])  # a page of the other sequence shows
    for c in ax.big_mla_cases(16, 64):
        c = dict(c, fill=ax.K_AMP)
        for fp8 in (False, True):
            out = mla_oracle(c, 64, fp8)
            err = ax.check_dominant(out, c["want"]) if bool(c["q_pe"].any()) else ax.check_count(as_bf16(out), c["want"])
        report(f"mla beyond-4-GiB case n={int(c['lens'][0])}", err)
