"""Multi-token GQA paged decode on the GPU (chitu_hip_gqa_decode_multi / _kv_fp8, csrc/gqa_decode_multi.hip, through
HipAttnBackend.attn_with_kvcache with q [bs, T, Hq, 128]).  Query (b, t) of a sequence of L keys must be the single-token decode of
a row of length L - T + t + 1: the constructions of tests/attn_exact.py and tests/attn_window_ref.py on the expanded lengths
(tests/attn_multi_ref.py), whose expected values are closed forms and fp64 attention, never a kernel; bit identities with the
single-token entries at T == 1 and between the two cache formats; the reference's own outputs (tests/golden/attn_multi.npz); the
in-place append.  Each test prints its worst error ("GQA_MULTI ...", pytest -s)."""
import pytest
import torch

from tests import attn_exact as ax
from tests import attn_multi_ref as mr
from tests import attn_window_ref as wr
from tests.test_gpu_attn_window import backend, bits, gqa_device, quantise, raw_decode
from tests.util import assert_close, bf16, golden

pytestmark = pytest.mark.gpu


def report(what, err):
    print(f"GQA_MULTI kernel {what}: {err:.3e}")


def multi_device(case, T, page, fp8=False, exact=True):
    """gqa_device of a case built on expanded lengths: q as [bs, T, Hq, 128], one length and one table row per sequence"""
    q, kd, vd, lens, table = gqa_device(dict(case, q=case["q"].view(-1, 1, *case["q"].shape[-2:])), page, fp8=fp8, exact=exact)
    bs = q.shape[0] // T
    return q.view(bs, T, *q.shape[2:]), kd, vd, lens, table[:bs].contiguous()


def run(dev, totals, splits, W=-1, c=0.0):
    """-> [bs * T, Hq, 128]: the rows in the expanded order (b, t)"""
    q, kd, vd, _, table = dev
    out = backend(q.shape[2]).attn_with_kvcache(q, kd, vd, cache_seqlens=totals, block_table=table, softmax_scale=ax.GQA_SCALE, causal=True,
                                                window_size=(W, 0), softcap=c, num_splits=splits)
    assert tuple(out.shape) == tuple(q.shape)
    return out.view(-1, *q.shape[2:])


def totals_dev(totals):
    return torch.tensor(list(totals), dtype=torch.int32).cuda()


# ---------------------------------------------------------------- 1. counting
@pytest.mark.parametrize("Hq,Hkv", mr.MULTI_HEADS)
@pytest.mark.parametrize("T", mr.MULTI_T)
def test_every_query_counts_exactly_its_own_keys_at_every_length(T, Hq, Hkv):
    """q = 0: query (b, t) returns the mean of the V rows of keys 0 .. L - T + t.  Every total length L = 0 .. 70 in one launch
    (L < T: the first T - L queries see nothing and give zeros), page 16, both cache formats, splits 1, 2, 3, 5.  One key of a
    later draft token admitted one query too early moves a channel by >= 1 / 17 of its value."""
    totals = list(range(mr.COUNT_N + 1))
    c = ax.gqa_count_case(mr.COUNT_N, Hq, Hkv, lengths=mr.expanded_lengths(totals, T))
    worst = 0.0
    for fp8 in (False, True):
        dev = multi_device(c, T, 16, fp8=fp8)
        worst = max([worst] + [ax.check_count(run(dev, totals_dev(totals), s), c["want"]) for s in mr.MULTI_SPLITS])
    report(f"counting T={T} Hq={Hq} Hkv={Hkv}, relative", worst)


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (16, 1), (6, 2)])
def test_every_query_counts_exactly_the_keys_of_its_window(Hq, Hkv):
    """the same under every window of DECODE_WINDOWS, totals 0 .. 130, T = 4 and 5 (a tile's queries start at different keys)"""
    totals = list(range(wr.DECODE_N + 1))
    worst = 0.0
    for T in (4, 5):
        c = ax.gqa_count_case(wr.DECODE_N, Hq, Hkv, lengths=mr.expanded_lengths(totals, T))
        for fp8, page in ((False, 16), (True, 48)):
            dev = multi_device(c, T, page, fp8=fp8)
            for W in wr.DECODE_WINDOWS:
                want = wr.gqa_count_want(c, Hq, W)
                worst = max([worst] + [ax.check_count(run(dev, totals_dev(totals), s, W), want) for s in (1, 3, None)])
    report(f"windowed counting Hq={Hq} Hkv={Hkv}, relative", worst)


# ---------------------------------------------------------------- 2. dominant key
@pytest.mark.parametrize("Hq,Hkv", mr.MULTI_HEADS)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_every_query_finds_its_own_keys_and_none_beyond(fp8, Hq, Hkv):
    """each query's own last key, key 0 (under a window: its first visible key), both sides of every step, page and split edge; and
    the keys just outside its range -- the next draft token's key, the key before the window -- are not admitted"""
    worst = 0.0
    for n, T, page in ((70, 4, 16), (130, 5, 48), (67, 8, 16)):
        for W in (-1, 1, 17):
            c = mr.multi_dominant_case(n, T, Hq, Hkv, page, mr.MULTI_SPLITS, W)
            q, kd, vd, lens, table = gqa_device(dict(c, q=c["q"][:, :1]), page, fp8=fp8)
            dev = (c["q"].cuda(), kd, vd, lens, table)
            worst = max([worst] + [ax.check_dominant(run(dev, lens, s, W), c["want"]) for s in mr.MULTI_SPLITS + [None]])
    report(f"dominant key {'kv fp8 ' if fp8 else ''}Hq={Hq} Hkv={Hkv}, absolute", worst)


# ---------------------------------------------------------------- 3. graded margin
def test_a_rescale_voted_by_another_tokens_column_leaves_every_column_right():
    """A key that leads query token 1's column by just under / just over kGqaDefer, in the first step and in a later one (key 120 is in
    step 7: with 1 and 3 splits a step with a finite maximum precedes it); the columns of the tile's other query tokens see random
    scores of a few nats.  Every row against the fp64 attention at the arithmetic bar of the single-token graded test."""
    ks, leads = ax.graded_amplitudes(ax.source_constant("gqa_decode_tile.h", "kGqaDefer"), ax.GQA_SCALE)
    for Hq, Hkv, T in ((8, 2, 4), (8, 1, 3), (6, 2, 5)):
        c = mr.multi_graded_case(130, T, Hq, Hkv, ks, tokens=[5, 120], probing_t=1)
        for page in (16, 256):
            q, kd, vd, lens, table = gqa_device(dict(c, q=c["q"][:, :1]), page)
            for s in (1, 3, None):
                assert_close(run((c["q"].cuda(), kd, vd, lens, table), lens, s), c["want"], 1e-2, what=("gqa multi graded", leads, Hq, Hkv, T, page, s))


# ---------------------------------------------------------------- 4. soft cap
@pytest.mark.parametrize("c", sorted(wr.SOFTCAP_LEVELS))
def test_soft_cap_weighs_the_two_score_levels_per_query(c):
    """gqa_softcap_case's sequences as the LAST query of T = 3 (its lengths are then the totals); queries 0 and 1 are the same case
    one and two keys shorter: the closed form at those lengths"""
    T, worst = 3, 0.0
    for Hq, Hkv in ((8, 2), (16, 1)):
        case = wr.gqa_softcap_case(Hq, Hkv, c)
        totals = case["lens"].tolist()
        exp = mr.expanded_lengths(totals, T)
        q = case["q"].repeat_interleave(T, dim=0)  # every query of a sequence: the same one-hot row
        live = torch.tensor(exp) > 0
        want_case = dict(case, lens=torch.tensor(exp, dtype=torch.int32).clamp_(min=1))  # (the closed form divides by the key count)
        for page in (16, 256):
            for fp8 in (False, True):
                qd, kd, vd, _, table = gqa_device(case, page, fp8=fp8)
                dev = (q.view(len(totals), T, Hq, 128).cuda(), kd, vd, None, table)
                for W in (-1, 40):
                    want = wr.gqa_softcap_want(want_case, Hq, W)
                    for s in (1, 3, None):
                        got = run(dev, totals_dev(totals), s, W, c).cpu()
                        assert not bool(got[~live].any())  # a query before the sequence's first key
                        worst = max(worst, assert_close(got[live], want[live], 1e-2, what=("soft cap", c, Hq, page, fp8, W, s)))
    report(f"soft cap c={c} two-level case, relative to the peak", worst)


# ---------------------------------------------------------------- 5. random data
@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (8, 1), (6, 2)])
def test_random_data_against_the_fp64_attention_on_expanded_rows(Hq, Hkv):
    """ragged totals (two below T), both pages, windows and caps: the 1e-2 bar tests/test_gpu_gqa.py holds the single-token kernel to"""
    totals = [1, 3, 17, 70, 300, 129]
    for T in (2, 4, 8):
        c = mr.multi_random_case(totals, T, Hq, Hkv, seed=T)
        for page in (16, 256):
            kc, vc, table = ax.gqa_pages(c, page, seed=page)
            dev = (c["q"].cuda(), kc.cuda(), vc.cuda(), None, table.cuda())
            for W, cap in ((-1, 0.0), (15, 0.0), (64, 5.0), (-1, 30.0)):
                want = mr.multi_random_want(c, W, cap)
                for s in (1, 3, None):
                    assert_close(run(dev, totals_dev(totals), s, W, cap), want, 1e-2, what=("gqa multi random", Hq, Hkv, T, page, W, cap, s))


# ---------------------------------------------------------------- 6. bit identities
def raw_multi(fp8, dev, totals, T, splits, W=-1, c=0.0):
    """One C-ABI call on a zeroed workspace -> (out [bs, T, Hq, 128], the workspace's partials)"""
    from chitu_amd import _lib
    from chitu_amd._lib import check, f32, i32, i64, ptr, stream_ptr

    q, kd, vd, _, table = dev
    bs, _, Hq, D = q.shape
    assert q.shape[1] == T
    name = "chitu_hip_gqa_decode_multi_kv_fp8" if fp8 else "chitu_hip_gqa_decode_multi"
    out = torch.empty(bs, T, Hq, D, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(max(bs * T * Hq * splits * (D + 1) * 4, 16), dtype=torch.uint8, device="cuda")
    check(getattr(_lib.lib(), name)(ptr(q), i64(q.stride(0)), i64(q.stride(1)), i64(q.stride(2)), ptr(kd), ptr(vd), i64(kd.shape[0]),
                                    i32(kd.shape[1]), i32(kd.shape[2]), ptr(table), i32(table.stride(0)), ptr(totals), f32(ax.GQA_SCALE),
                                    ptr(out), i32(bs), i32(T), i32(Hq), i32(D), i32(splits), ptr(ws), i64(ws.numel()), i32(W), f32(c),
                                    stream_ptr()), name)
    return out, ws


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_one_query_token_is_the_single_token_entry_bit_for_bit(fp8):
    """T == 1: output and workspace partials of the four existing entries, lengths 0 .. 130, splits 1 and 3"""
    from chitu_amd._lib import f32, i32
    from tests.test_gpu_attn_window import random_case

    plain = "chitu_hip_gqa_decode_kv_fp8" if fp8 else "chitu_hip_gqa_decode"
    for Hq, Hkv in mr.MULTI_HEADS:
        c = random_case(list(range(wr.DECODE_N + 1)), Hq, Hkv)
        for page in (16, 256):
            dev = gqa_device(c, page, fp8=fp8, exact=False)
            for s in (1, 3):
                for W, cap in ((-1, 0.0), (17, 0.0), (40, 5.0), (-1, 30.0)):
                    if (W, cap) == (-1, 0.0):
                        want, want_ws = raw_decode(plain, dev, s)
                    else:
                        want, want_ws = raw_decode(plain + "_window", dev, s, (i32(W), f32(cap)))
                    got, got_ws = raw_multi(fp8, dev, dev[3], 1, s, W, cap)
                    assert torch.equal(bits(got[:, 0]), bits(want)) and torch.equal(got_ws, want_ws), (Hq, Hkv, page, s, W, cap)


def test_fp8_pages_give_the_bits_of_the_bf16_kernel_on_the_dequantised_cache():
    from chitu_amd import ops

    totals = list(range(wr.DECODE_N + 1))
    for Hq, Hkv in mr.MULTI_HEADS:
        for T in (2, 5):
            c = mr.multi_random_case(totals, T, Hq, Hkv, seed=3)
            kc, vc, table = ax.gqa_pages(c, 48, seed=48)
            k8, v8 = quantise(kc.cuda(), exact=False), quantise(vc.cuda(), exact=False)  # random rows: rounded here
            kq, vq = ops.gqa_kv_dequant_fp8(k8), ops.gqa_kv_dequant_fp8(v8)
            q, tb, lens = c["q"].cuda(), table.cuda(), totals_dev(totals)
            for W, cap in ((-1, 0.0), (15, 0.0), (47, 5.0)):
                for s in (1, 3):
                    got, got_ws = raw_multi(True, (q, k8, v8, None, tb), lens, T, s, W, cap)
                    want, want_ws = raw_multi(False, (q, kq, vq, None, tb), lens, T, s, W, cap)
                    assert torch.equal(bits(got), bits(want)) and torch.equal(got_ws, want_ws), (Hq, Hkv, T, W, cap, s)


# ---------------------------------------------------------------- 7. the reference's outputs
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_against_the_reference_attention_fixture(fp8):
    """tests/golden/attn_multi.npz (RefAttnBackend._attention, causal, seqlen_q = T) with every sequence in pages of its own"""
    g = golden("attn_multi")
    page, worst = 16, 0.0
    for T in mr.FIXM_T:
        inp = mr.fixture_multi_inputs(T)
        B, S = inp["K"].shape[:2]
        per = S // page
        perm = 1 + torch.randperm(B * per, generator=torch.Generator().manual_seed(T)).view(B, per)
        kc, vc = (torch.zeros(B * per + 1, page, mr.FIXM_HKV, 128, dtype=torch.bfloat16) for _ in range(2))
        kc[perm.view(-1)], vc[perm.view(-1)] = inp["K"].view(B * per, page, -1, 128), inp["V"].view(B * per, page, -1, 128)
        kd, vd = kc.cuda(), vc.cuda()
        if fp8:
            kd, vd = quantise(kd), quantise(vd)
        dev = (inp["q"].cuda(), kd, vd, None, perm.to(torch.int32).cuda())
        for W in mr.FIXM_WINDOWS:
            for c in mr.FIXM_CAPS:
                want = bf16(g[mr.fixture_multi_key(T, W, c)]).view(B * T, mr.FIXM_HQ, 128)
                for s in (1, 3, None):
                    worst = max(worst, assert_close(run(dev, inp["lens"].cuda(), s, W, c), want, wr.FIX_BAR, what=("fixture", T, W, c, s)))
    report(f"reference fixture {'kv fp8' if fp8 else 'bf16'}, of the peak", worst)


# ---------------------------------------------------------------- 8. the backend: append and refusals
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_append_puts_the_rows_where_single_token_calls_put_them(fp8):
    """k / v [bs, T, Hkv, 128] through attn_with_kvcache: the caches afterwards equal, bit for bit, the caches after T single-token
    calls that append row t at cache_seqlens + t (the same append kernels); the output is the no-append call over cache_seqlens + T"""
    Hq, Hkv, page, T = 8, 2, 16, 4
    old = [0, 5, 13, 16, 63]  # appends that cross a page edge, start a sequence, start a page
    B, per = len(old), 6
    g = torch.Generator().manual_seed(2)
    table = (1 + torch.randperm(B * per, generator=g).view(B, per)).to(torch.int32).cuda()
    kc = torch.randn(B * per + 1, page, Hkv, 128, generator=g).to(torch.bfloat16).cuda()
    vc = torch.randn(B * per + 1, page, Hkv, 128, generator=g).to(torch.bfloat16).cuda()
    if fp8:
        kc, vc = quantise(kc, exact=False), quantise(vc, exact=False)
    q = (torch.randn(B, T, Hq, 128, generator=g) * 0.5).to(torch.bfloat16).cuda()
    k = torch.randn(B, T, Hkv, 128, generator=g).to(torch.bfloat16).cuda()
    v = torch.randn(B, T, Hkv, 128, generator=g).to(torch.bfloat16).cuda()
    lens = torch.tensor(old, dtype=torch.int32).cuda()
    be = backend(Hq)
    k1, v1 = kc.clone(), vc.clone()
    for t in range(T):
        be.attn_with_kvcache(q[:, t : t + 1], k1, v1, k[:, t : t + 1].contiguous(), v[:, t : t + 1].contiguous(), cache_seqlens=lens + t,
                             block_table=table)
    k2, v2 = kc.clone(), vc.clone()
    out = be.attn_with_kvcache(q, k2, v2, k, v, cache_seqlens=lens, block_table=table, causal=True, num_splits=2)
    assert torch.equal(k2.view(torch.uint8), k1.view(torch.uint8)) and torch.equal(v2.view(torch.uint8), v1.view(torch.uint8))
    assert not torch.equal(k2.view(torch.uint8), kc.view(torch.uint8))
    again = be.attn_with_kvcache(q, k2, v2, cache_seqlens=lens + T, block_table=table, causal=True, num_splits=2)
    assert torch.equal(bits(out), bits(again)) and tuple(out.shape) == (B, T, Hq, 128)


def test_the_backend_refuses_what_the_kernel_does_not_do():
    Hq, Hkv, page = 8, 2, 16
    kc = torch.zeros(4, page, Hkv, 128, dtype=torch.bfloat16, device="cuda")
    table = torch.zeros(1, 3, dtype=torch.int32, device="cuda")
    lens = torch.full((1,), 20, dtype=torch.int32, device="cuda")
    be = backend(Hq)
    q = torch.zeros(1, 2, Hq, 128, dtype=torch.bfloat16, device="cuda")
    for kwargs in (dict(), dict(causal=False, window_size=(-1, -1)), dict(window_size=(4, -1)), dict(window_size=(4, 2))):
        with pytest.raises(NotImplementedError):
            be.attn_with_kvcache(q, kc, kc.clone(), cache_seqlens=lens, block_table=table, **kwargs)
    for kwargs in (dict(causal=True), dict(window_size=(4, 0)), dict(causal=True, window_size=(4, 7)), dict(window_size=(-1, 0))):
        assert tuple(be.attn_with_kvcache(q, kc, kc.clone(), cache_seqlens=lens, block_table=table, **kwargs).shape) == (1, 2, Hq, 128)
    with pytest.raises(AssertionError):
        be.attn_with_kvcache(torch.zeros(1, 9, Hq, 128, dtype=torch.bfloat16, device="cuda"), kc, kc.clone(), cache_seqlens=lens,
                             block_table=table, causal=True)
