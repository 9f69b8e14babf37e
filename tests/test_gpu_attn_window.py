"""Sliding-window and soft-capped GQA attention on the GPU (chitu_hip_gqa_decode_window, chitu_hip_gqa_decode_kv_fp8_window,
chitu_hip_gqa_prefill_window and the Llama args that reach them): the constructions of tests/attn_exact.py under a window, whose
expected values are the closed forms of tests/attn_window_ref.py (tests/test_attn_window_host.py shows on the CPU that they are
the fp64 attention and that the fp64 attention is the reference's), bit identities with the unwindowed kernels, and the
reference's own outputs (tests/golden/attn_window.npz).  Each test prints its worst error ("ATTN_WINDOW ...", pytest -s)."""
import dataclasses

import pytest
import torch

from tests import attn_exact as ax
from tests import attn_window_ref as wr
from tests import test_gqa_kv_fp8_host as g8
from tests.util import assert_close, bf16, golden, max_rel_to_peak

pytestmark = pytest.mark.gpu

GQA_HEADS = [(4, 4), (8, 2), (16, 1)]
GQA_PAGES = [16, 48, 256]
GQA_SPLITS = [1, 2, 3, 5, 8, 17, None]
N = wr.DECODE_N


def report(what, err):
    print(f"ATTN_WINDOW kernel {what}: {err:.3e}")


def backend(H):
    from chitu_amd.attn_backend import HipAttnBackend

    return HipAttnBackend(local_n_heads=H)


def bits(t):
    return t.contiguous().view(torch.int16)


def quantise(cache, exact=True):
    """bf16 cache [pages, page, Hkv, 128] on the GPU -> the fp8 cache of the same rows; exact: the rows must survive the round trip"""
    from chitu_amd import ops

    shape = cache.shape
    c8 = ops.gqa_kv_quant_fp8(cache.view(-1, shape[2], 128)).view(*shape[:3], g8.ROW)
    assert not exact or torch.equal(bits(ops.gqa_kv_dequant_fp8(c8)), bits(cache)), "these rows are not exact in the fp8 format"
    return c8


def gqa_device(case, page, fp8=False, exact=True):
    """(q, k_cache, v_cache, lens, table) on the GPU: every batch row over one table of shuffled pages (tests/test_gpu_attn_exact.py).
    exact=False: random rows that the fp8 cache rounds -- for comparisons of two kernels over the SAME cache"""
    kc, vc, table = ax.gqa_pages(case, page, seed=page)
    kd, vd = kc.cuda(), vc.cuda()
    if fp8:
        kd, vd = quantise(kd, exact), quantise(vd, exact)
    return case["q"].cuda(), kd, vd, case["lens"].cuda(), table.cuda()


def run(dev, splits, W=-1, c=0.0):
    q, kd, vd, lens, table = dev
    return backend(q.shape[2]).attn_with_kvcache(q, kd, vd, cache_seqlens=lens, block_table=table, softmax_scale=ax.GQA_SCALE,
                                                 window_size=(W, 0), softcap=c, num_splits=splits)[:, 0]


def random_case(lens, Hq, Hkv, seed=0):
    """small random q, small-integer K, random V (bf16 values): for the bit identities, where any data will do"""
    n = max(max(lens), 1)
    g = torch.Generator().manual_seed(seed)
    q = (torch.randint(-8, 9, (len(lens), 1, Hq, 128), generator=g).float() / 4).to(torch.bfloat16)
    V = torch.randn(n, Hkv, 128, generator=g).to(torch.bfloat16).float()
    return dict(q=q, K=ax.small_ints((n, Hkv, 128), seed + 1), V=V, lens=torch.tensor(lens, dtype=torch.int32), k_fill=ax.K_AMP, v_fill=1.0)


# ---------------------------------------------------------------- 1. counting
@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
@pytest.mark.parametrize("page", GQA_PAGES)
def test_decode_counts_exactly_the_keys_of_the_window_at_every_length(page, Hq, Hkv):
    """lengths 0 .. 130 in one launch per (window, split count): the mean of the V rows w0 .. L - 1"""
    c = ax.gqa_count_case(N, Hq, Hkv)
    dev = gqa_device(c, page)
    worst = 0.0
    for W in wr.DECODE_WINDOWS:
        want = wr.gqa_count_want(c, Hq, W)
        worst = max([worst] + [ax.check_count(run(dev, s, W), want) for s in GQA_SPLITS])
    report(f"decode counting page={page} Hq={Hq} Hkv={Hkv}, relative", worst)


@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
def test_decode_kv_fp8_counts_exactly_the_keys_of_the_window(Hq, Hkv):
    c = ax.gqa_count_case(N, Hq, Hkv)
    dev = gqa_device(c, 48, fp8=True)
    worst = 0.0
    for W in wr.DECODE_WINDOWS:
        want = wr.gqa_count_want(c, Hq, W)
        worst = max([worst] + [ax.check_count(run(dev, s, W), want) for s in GQA_SPLITS])
    report(f"decode kv fp8 counting Hq={Hq} Hkv={Hkv}, relative", worst)


# ---------------------------------------------------------------- 2. dominant key
def window_probe_case(n, W, Hq, Hkv):
    """Rows 0-2 probe the keys w0, w0 + 1 and n - 1 (lead 45 nats): their V rows.  Row 3 probes w0 - 1 with amplitude 32 and n - 1
    with 16: inside the window key n - 1 leads by 22.6 nats (the others leak n * 15 * e^-22.6 ~ 3e-7 < ABS_DOMINANT), so the answer
    is row n - 1 -- a kernel that admits w0 - 1 returns that row instead."""
    w0 = wr.first_key(n, W)
    assert 1 <= w0 and w0 + 1 <= n - 1
    targets = [w0 - 1, w0, w0 + 1, n - 1]
    K = ax.small_ints((n, Hkv, 128), 5)
    K[:, :, :4] = 0.0
    for ch, t in enumerate(targets):
        K[t, :, ch] = ax.K_AMP
    V = ax.identity_rows(n, Hkv, 128)
    q = torch.zeros(4, 1, Hq, 128)
    q[0, 0, :, 1] = q[1, 0, :, 2] = q[2, 0, :, 3] = q[3, 0, :, 0] = ax.Q_AMP
    q[3, 0, :, 3] = ax.Q_AMP / 2
    want = torch.stack([V[t].double() for t in (w0, w0 + 1, n - 1, n - 1)]).repeat_interleave(Hq // Hkv, dim=1)
    assert ax.leak_bound(n, 15.0, ax.margin_nats(ax.Q_AMP / 2, ax.K_AMP, ax.GQA_SCALE)) < ax.ABS_DOMINANT
    return dict(q=q.to(torch.bfloat16), K=K, V=V, lens=torch.full((4,), n, dtype=torch.int32), want=want, k_fill=ax.K_AMP, v_fill=15.0)


@pytest.mark.parametrize("Hq,Hkv", GQA_HEADS)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_sees_the_first_key_of_the_window_and_not_the_one_before(fp8, Hq, Hkv):
    worst = 0.0
    for W in (1, 15, 16, 17, 47, 64):
        c = window_probe_case(N, W, Hq, Hkv)
        for page in GQA_PAGES:
            dev = gqa_device(c, page, fp8=fp8)
            worst = max([worst] + [ax.check_dominant(run(dev, s, W), c["want"]) for s in GQA_SPLITS])
    report(f"decode {'kv fp8 ' if fp8 else ''}dominant key at the window edge Hq={Hq} Hkv={Hkv}, absolute", worst)


# ---------------------------------------------------------------- 3. poison
POISON_LENS = [1, 16, 17, 40, 100, 130]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_never_uses_a_row_or_a_page_outside_the_window(fp8):
    """Every sequence in its own pages (page 16).  Poisoned copy: every K and V row with t < w0 or t >= L is NaN (fp8: NaN codes
    and a NaN scale), the table entries of pages wholly before the window are -1, page 0 (nobody's) is NaN: same bits out."""
    Hq, Hkv, page, per = 8, 2, 16, 9
    B = len(POISON_LENS)
    g = torch.Generator().manual_seed(8)
    q = (torch.randint(-8, 9, (B, 1, Hq, 128), generator=g).float() / 4).to(torch.bfloat16).cuda()
    K = ax.small_ints((B, per * page, Hkv, 128), 9).to(torch.bfloat16)
    V = torch.randn(B, per * page, Hkv, 128, generator=g).to(torch.bfloat16)
    perm = 1 + torch.randperm(B * per, generator=g).view(B, per)
    kc, vc = (torch.zeros(B * per + 1, page, Hkv, 128, dtype=torch.bfloat16) for _ in range(2))
    kc[perm.view(-1)], vc[perm.view(-1)] = K.view(B * per, page, Hkv, 128), V.view(B * per, page, Hkv, 128)
    lens = torch.tensor(POISON_LENS, dtype=torch.int32).cuda()
    kd, vd = kc.cuda(), vc.cuda()
    if fp8:
        from chitu_amd import ops

        kd, vd = (ops.gqa_kv_quant_fp8(c.view(-1, Hkv, 128)).view(B * per + 1, page, Hkv, g8.ROW) for c in (kd, vd))
    be = backend(Hq)
    for W in (0, 15, 16, 40):
        table = perm.to(torch.int32)
        bad_table = table.clone()
        kp, vp = kd.clone(), vd.clone()
        for cache in (kp, vp):
            flat = cache.view(torch.uint8) if fp8 else cache.view(torch.int16)  # 0xFF bytes: NaN codes + NaN scale; 0x7FC0: a bf16 NaN
            poison = 0xFF if fp8 else 0x7FC0
            flat[0] = poison
            for b, L in enumerate(POISON_LENS):
                w0 = wr.first_key(L, W)
                for t in list(range(w0)) + list(range(L, per * page)):
                    flat[int(perm[b, t // page]), t % page] = poison
        for b, L in enumerate(POISON_LENS):
            bad_table[b, : wr.first_key(L, W) // page] = -1
        for s in (1, 3, None):
            clean = be.attn_with_kvcache(q, kd, vd, cache_seqlens=lens, block_table=table.cuda(), softmax_scale=ax.GQA_SCALE,
                                         window_size=(W, 0), num_splits=s)
            dirty = be.attn_with_kvcache(q, kp, vp, cache_seqlens=lens, block_table=bad_table.cuda(), softmax_scale=ax.GQA_SCALE,
                                         window_size=(W, 0), num_splits=s)
            assert not bool(torch.isnan(clean.float()).any())
            assert torch.equal(bits(clean), bits(dirty)), (W, s)


# ---------------------------------------------------------------- 4. identities with the existing kernel
def raw_decode(name, dev, splits, extra=()):
    """One C-ABI call on a zeroed workspace -> (out [bs, Hq, 128], the workspace's partials)"""
    from chitu_amd import _lib
    from chitu_amd._lib import check, f32, i32, i64, ptr, stream_ptr

    q, kd, vd, lens, table = dev
    bs, _, Hq, D = q.shape
    out = torch.empty(bs, Hq, D, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(max(bs * Hq * splits * (D + 1) * 4, 16), dtype=torch.uint8, device="cuda")
    q3 = q.view(bs, Hq, D)
    check(getattr(_lib.lib(), name)(ptr(q3), i64(q3.stride(0)), i64(q3.stride(1)), ptr(kd), ptr(vd), i64(kd.shape[0]), i32(kd.shape[1]),
                                    i32(kd.shape[2]), ptr(table), i32(table.stride(0)), ptr(lens), f32(ax.GQA_SCALE), ptr(out), i32(bs),
                                    i32(Hq), i32(D), i32(splits), ptr(ws), i64(ws.numel()), *extra, stream_ptr()), name)
    return out, ws


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_a_window_that_holds_the_whole_sequence_is_the_plain_kernel_bit_for_bit(fp8):
    """W >= L - 1 for every sequence (the windowed kernel, nothing to cut) and (-1, 0.0) (the launcher takes the plain kernel):
    output and workspace partials equal the plain entry's at every split count"""
    from chitu_amd._lib import f32, i32

    plain = "chitu_hip_gqa_decode_kv_fp8" if fp8 else "chitu_hip_gqa_decode"
    for Hq, Hkv in GQA_HEADS:
        c = random_case(list(range(N + 1)), Hq, Hkv)
        for page in (16, 256):
            dev = gqa_device(c, page, fp8=fp8, exact=False)
            for s in (1, 2, 3, 5, 8, 17):
                want, want_ws = raw_decode(plain, dev, s)
                for W in (-1, N - 1, 200, 2 ** 31 - 1):
                    got, got_ws = raw_decode(plain + "_window", dev, s, (i32(W), f32(0.0)))
                    assert torch.equal(bits(got), bits(want)) and torch.equal(got_ws, want_ws), (Hq, Hkv, page, s, W)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_a_window_on_a_step_edge_is_the_plain_kernel_on_the_shifted_table(fp8):
    """page 16, w0 % 16 == 0: the windowed call walks the steps [w0 / 16, n16) split exactly as the plain call splits [0, n16 - w0 / 16)
    on the table shifted left by w0 / 16 pages with length L - w0: same bits, partials included"""
    from chitu_amd._lib import f32, i32

    plain = "chitu_hip_gqa_decode_kv_fp8" if fp8 else "chitu_hip_gqa_decode"
    for W, lengths in ((15, [16, 32, 80, 128]), (17, [18, 34, 130]), (47, [48, 64, 128, 144])):
        c = random_case(lengths, 8, 2, seed=W)
        q, kd, vd, lens, table = gqa_device(c, 16, fp8=fp8, exact=False)
        shifted, short = table.clone(), lens.clone()
        for b, L in enumerate(lengths):
            w0 = wr.first_key(L, W)
            assert w0 % 16 == 0
            k = w0 // 16
            shifted[b, : table.shape[1] - k] = table[b, k:]
            short[b] = L - w0
        for s in (1, 2, 3, 5, 8, 17):
            got, got_ws = raw_decode(plain + "_window", (q, kd, vd, lens, table), s, (i32(W), f32(0.0)))
            want, want_ws = raw_decode(plain, (q, kd, vd, short, shifted), s)
            assert torch.equal(bits(got), bits(want)) and torch.equal(got_ws, want_ws), (W, s)


def test_fp8_windowed_decode_is_the_bf16_windowed_decode_on_the_dequantised_cache():
    from chitu_amd import ops

    for Hq, Hkv in GQA_HEADS:
        c = random_case(list(range(N + 1)), Hq, Hkv, seed=3)
        q, kd, vd, lens, table = gqa_device(c, 48)
        shape = kd.shape
        k8, v8 = (ops.gqa_kv_quant_fp8(x.view(-1, Hkv, 128)).view(*shape[:3], g8.ROW) for x in (kd, vd))  # random V: rounded here
        kq, vq = ops.gqa_kv_dequant_fp8(k8), ops.gqa_kv_dequant_fp8(v8)
        for W, cap in ((0, 0.0), (15, 0.0), (16, 5.0), (47, 0.0), (64, 30.0), (-1, 5.0)):
            for s in GQA_SPLITS:
                assert torch.equal(bits(run((q, k8, v8, lens, table), s, W, cap)), bits(run((q, kq, vq, lens, table), s, W, cap))), (W, cap, s)


# ---------------------------------------------------------------- 5. soft cap
@pytest.mark.parametrize("c", sorted(wr.SOFTCAP_LEVELS))
def test_decode_soft_cap_weighs_the_two_score_levels_as_tanh_says(c):
    worst = 0.0
    for Hq, Hkv in ((8, 2), (16, 1)):
        case = wr.gqa_softcap_case(Hq, Hkv, c)
        for page in (16, 256):
            for fp8 in (False, True):
                dev = gqa_device(case, page, fp8=fp8)
                for W in (-1, 40):
                    want = wr.gqa_softcap_want(case, Hq, W)
                    for s in (1, 3, None):
                        worst = max(worst, assert_close(run(dev, s, W, c), want, 1e-2, what=("soft cap", c, Hq, page, fp8, W, s)))
    report(f"decode soft cap c={c} two-level case, relative to the peak", worst)


# ---------------------------------------------------------------- 6. the reference's outputs
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_matches_the_reference_fixtures(fp8):
    """the decode cases of tests/golden/attn_window.npz paged into shuffled 16-token pages, the last row appended by the call"""
    g = golden("attn_window")
    inp = wr.fixture_decode_inputs()
    B, page = len(wr.FIX_LENGTHS), 16
    per = wr.FIX_CACHE_LEN // page
    perm = torch.randperm(B * per + 2, generator=torch.Generator().manual_seed(6))[: B * per].view(B, per)
    kc, vc = (torch.zeros(B * per + 2, page, wr.FIX_HKV, 128, dtype=torch.bfloat16) for _ in range(2))
    kc[perm.view(-1)] = inp["k_cache"].view(B * per, page, wr.FIX_HKV, 128)
    vc[perm.view(-1)] = inp["v_cache"].view(B * per, page, wr.FIX_HKV, 128)
    kd, vd = kc.cuda(), vc.cuda()
    if fp8:
        kd, vd = quantise(kd), quantise(vd)  # multiples of 1/8 up to 1: the quantiser gives them back
    be = backend(wr.FIX_HQ)
    old = inp["cache_seqlens"].to(torch.int32).cuda()
    worst = 0.0
    for W in wr.FIX_WINDOWS:
        for c in wr.FIX_CAPS:
            for s in (1, 3, None):
                out = be.attn_with_kvcache(inp["q"].cuda(), kd, vd, inp["k_new"].cuda(), inp["v_new"].cuda(), cache_seqlens=old,
                                           block_table=perm.to(torch.int32).cuda(), window_size=(W, 0) if W >= 0 else (-1, -1), softcap=c,
                                           softmax_scale=ax.GQA_SCALE, num_splits=s)[:, 0]
                worst = max(worst, assert_close(out, bf16(g[wr.fixture_key("decode", W, c)]), 1e-2, what=("fixture", fp8, W, c, s)))
    report(f"decode {'kv fp8 ' if fp8 else ''}vs the reference fixtures, relative to the peak", worst)


# ---------------------------------------------------------------- 7. prefill
def gqa_prefill(case, Hq, W=-1, c=0.0, strided=False):
    q, k, v = (case[n].to(torch.bfloat16).cuda() for n in ("q", "k", "v"))
    if strided:  # the slices of one merged qkv projection output
        Hkv = k.shape[1]
        qkv = torch.cat([q, k, v], dim=1)
        q, k, v = qkv[:, :Hq], qkv[:, Hq : Hq + Hkv], qkv[:, Hq + Hkv :]
    cu = torch.tensor(case["cu"], dtype=torch.int32).cuda()
    m = max(b - a for a, b in zip(case["cu"][:-1], case["cu"][1:]))
    return backend(Hq).attn_varlen_func(q, k, v, cu, cu, m, m, causal=True, window_size=(W, -1), softcap=c, softmax_scale=ax.GQA_SCALE)


@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (8, 2), (32, 1)])  # 128, 32 and 4 query tokens in a workgroup
def test_prefill_every_query_row_counts_exactly_the_keys_of_its_window(Hq, Hkv, monkeypatch):
    count = ax.prefill_count_case(ax.PREFILL_SEQS, Hq, Hkv, 128, ax.P_GQA)
    modes = [("flash", False), ("flash", True)] + ([("compose", False)] if Hq // Hkv <= 16 else [])
    for mode, strided in modes:
        monkeypatch.setenv("CHITU_GQA_PREFILL", mode)
        worst = max(ax.check_count(gqa_prefill(count, Hq, W, strided=strided), wr.prefill_count_want(count, Hq, W)) for W in wr.PREFILL_WINDOWS)
        report(f"prefill {mode}{' strided' if strided else ''} Hq={Hq} Hkv={Hkv} counting, relative", worst)


def test_prefill_matches_the_reference_fixtures(monkeypatch):
    g = golden("attn_window")
    pre = wr.fixture_prefill_inputs()
    rows = torch.from_numpy(g["prefill_rows"])
    for mode in ("flash", "compose"):
        monkeypatch.setenv("CHITU_GQA_PREFILL", mode)
        worst = 0.0
        for W in wr.FIX_WINDOWS:
            for c in wr.FIX_CAPS:
                out = gqa_prefill(pre, wr.FIX_HQ, W, c).cpu()[rows]
                worst = max(worst, assert_close(out, bf16(g[wr.fixture_key("prefill", W, c)]), 1e-2, what=("fixture", mode, W, c)))
        report(f"prefill {mode} vs the reference fixtures, relative to the peak", worst)


@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (8, 2), (16, 1)])
def test_prefill_flash_agrees_with_the_composition_from_the_windowed_decode(Hq, Hkv, monkeypatch):
    g = torch.Generator().manual_seed(12)
    cu = ax.cu_of(ax.PREFILL_SEQS)
    case = dict(q=torch.randn(cu[-1], Hq, 128, generator=g) * 2, k=torch.randn(cu[-1], Hkv, 128, generator=g), v=torch.randn(cu[-1], Hkv, 128, generator=g), cu=cu)
    worst = 0.0
    for W, c in ((0, 0.0), (31, 0.0), (64, 0.0), (130, 0.0), (1, 5.0), (63, 5.0), (65, 30.0), (-1, 5.0)):
        monkeypatch.setenv("CHITU_GQA_PREFILL", "flash")
        flash = gqa_prefill(case, Hq, W, c)
        monkeypatch.setenv("CHITU_GQA_PREFILL", "compose")
        worst = max(worst, assert_close(flash, gqa_prefill(case, Hq, W, c), 1e-2, what=("flash vs compose", Hq, Hkv, W, c)))
    report(f"prefill flash vs compose Hq={Hq} Hkv={Hkv}, relative to the peak", worst)


# ---------------------------------------------------------------- 8. model
def tiny_model(**kw):
    from tests.test_gpu_llama import build, tiny_args

    return build(dataclasses.replace(tiny_args(2), **kw))


def roll(model, cache, prompts, steps, use_graph, tag):
    """greedy: prefill + (steps - 1) decode steps -> (tokens [n, steps], the last step's logits)"""
    ids = [f"{tag}{i}" for i in range(len(prompts))]
    logits = model.prefill(prompts, ids)
    toks = [logits.argmax(-1)]
    for _ in range(steps - 1):
        cache.prepare_cache_decode(ids)
        cache.prepare_block_table_for_decode(ids)
        logits = model.decode(toks[-1], use_graph=use_graph).clone()
        cache.finalize_cache_single_decode(ids)
        toks.append(logits.argmax(-1))
    for r in ids:
        cache.finalize_cache_all_decode(r)
    return torch.stack(toks, dim=1), logits


def prompts_of(lengths, vocab, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lengths]


def test_a_window_wider_than_every_context_changes_no_bit_of_the_model():
    plain, cache0 = tiny_model()
    wide, cache1 = tiny_model(sliding_window=400)
    prompts = prompts_of([1, 70, 260], plain.args.vocab_size)
    for use_graph in (False, True):
        t0, l0 = roll(plain, cache0, prompts, 4, use_graph, "a")
        t1, l1 = roll(wide, cache1, prompts, 4, use_graph, "b")
        assert torch.equal(t0, t1) and torch.equal(l0, l1), use_graph
        assert torch.equal(plain.generate(prompts, 4, use_graph=use_graph), wide.generate(prompts, 4, use_graph=use_graph))
        assert torch.equal(t0, wide.generate(prompts, 4, use_graph=use_graph))


def test_windowed_model_prefill_decode_and_graph_agree_and_the_window_is_passed_down():
    model, cache = tiny_model(sliding_window=24)
    plain, cache0 = tiny_model()
    prompt = prompts_of([70], model.args.vocab_size, seed=5)[0]
    full = model.prefill([prompt], ["f"])[0].clone()
    cache.finalize_cache_all_decode("f")
    step = {}
    for use_graph in (False, True):
        rid = f"s{int(use_graph)}"
        model.prefill([prompt[:-1]], [rid])
        cache.prepare_cache_decode([rid])
        cache.prepare_block_table_for_decode([rid])
        step[use_graph] = model.decode(torch.tensor(prompt[-1:], dtype=torch.int64, device="cuda"), use_graph=use_graph)[0].clone()
        cache.finalize_cache_single_decode([rid])
        cache.finalize_cache_all_decode(rid)
    err = assert_close(full, step[False], 3e-2, what="windowed prefill vs prefill + one windowed decode step")
    assert torch.equal(step[True], step[False]), "the captured graph step is not the eager step"
    unwindowed = plain.prefill([prompt], ["u"])[0]
    gap = max_rel_to_peak(full, unwindowed)
    print(f"ATTN_WINDOW model: prefill vs prefill + decode {err:.3e}; windowed vs unwindowed logits differ by {gap:.3f} of the peak")
    assert gap > 10 * 3e-2, gap


def test_one_layer_windowed_model_sees_exactly_the_last_tokens():
    """RoPE scores depend only on relative position and, with one layer, a key / value row only on its own token: the windowed
    logits of the 70-token prompt are the unwindowed logits of its last 24 tokens alone."""
    model, _ = tiny_model(sliding_window=24, n_layers=1)
    plain, _ = tiny_model(n_layers=1)
    prompt = prompts_of([70], model.args.vocab_size, seed=7)[0]
    got = model.prefill([prompt], ["w"])[0]
    want = plain.prefill([prompt[-24:]], ["p"])[0]
    err = assert_close(got, want, 3e-2, what="windowed 70 tokens vs unwindowed last 24")
    other = plain.prefill([prompt[-25:]], ["q"])[0]
    print(f"ATTN_WINDOW model: one layer, windowed vs last 24 tokens {err:.3e} (vs last 25: {max_rel_to_peak(got, other):.3e})")
