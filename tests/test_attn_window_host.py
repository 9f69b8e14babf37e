"""Host checks (no GPU) of the sliding-window / soft-capped GQA attention: the fp64 restatements of tests/attn_window_ref.py
against the reference's own outputs (tests/golden/attn_window.npz), the closed forms the GPU tests assert against those
restatements, the preconditions of their bars, and the C ABI / documents / argument checks of the three new entries."""
import ctypes
import os
import re

import pytest
import torch

from tests import attn_exact as ax
from tests import attn_window_ref as wr
from tests.util import assert_close, bf16, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("chitu_hip_gqa_decode_window", "chitu_hip_gqa_decode_kv_fp8_window", "chitu_hip_gqa_prefill_window")
PLAIN = {"chitu_hip_gqa_decode_window": "chitu_hip_gqa_decode", "chitu_hip_gqa_decode_kv_fp8_window": "chitu_hip_gqa_decode_kv_fp8",
         "chitu_hip_gqa_prefill_window": "chitu_hip_gqa_prefill"}


# ---------------------------------------------------------------- the restatements against the reference
def test_fp64_restatements_match_the_reference_fixtures():
    g = golden("attn_window")
    dec, pre = wr.fixture_decode_inputs(), wr.fixture_prefill_inputs()
    K, V = wr.fixture_decode_rows(dec)
    rows = torch.from_numpy(g["prefill_rows"])
    assert torch.equal(rows, torch.from_numpy(wr.fixture_prefill_rows()))
    worst = 0.0
    for W in wr.FIX_WINDOWS:
        for c in wr.FIX_CAPS:
            got = torch.stack([wr.decode64_window(dec["q"][b], K[b], V[b], [L], ax.GQA_SCALE, W, c)[0] for b, L in enumerate(wr.FIX_LENGTHS)])
            worst = max(worst, assert_close(got.to(torch.bfloat16), bf16(g[wr.fixture_key("decode", W, c)]), wr.FIX_BAR, what=("decode", W, c)))
            got = wr.prefill64_window(pre["q"], pre["k"], pre["v"], pre["cu"], ax.GQA_SCALE, W, c)[rows]
            worst = max(worst, assert_close(got.to(torch.bfloat16), bf16(g[wr.fixture_key("prefill", W, c)]), wr.FIX_BAR, what=("prefill", W, c)))
    print(f"ATTN_WINDOW fp64 restatement vs the reference fixtures, worst error relative to the peak: {worst:.3e}")


def test_the_soft_cap_fixtures_cannot_be_met_without_the_cap():
    g = golden("attn_window")
    for kind in ("decode", "prefill"):
        for W in (w for w in wr.FIX_WINDOWS if w != 0):
            a, b = (bf16(g[wr.fixture_key(kind, W, c)]).float() for c in wr.FIX_CAPS)
            assert float((a - b).abs().max() / b.abs().max()) > 10 * wr.FIX_BAR, (kind, W)


def test_restatements_with_neutral_parameters_are_the_unwindowed_ones():
    c = ax.gqa_graded_case(50, 8, 2, [3.0], tokens=[5])
    assert torch.equal(wr.decode64_window(c["q"][:, 0], c["K"], c["V"], c["lens"], ax.GQA_SCALE), ax.decode64(c["q"][:, 0], c["K"], c["V"], c["lens"], ax.GQA_SCALE))
    p = ax.prefill_dominant_case([3, 40], 8, 2, 128)
    assert torch.equal(wr.prefill64_window(p["q"], p["k"], p["v"], p["cu"], ax.GQA_SCALE), ax.prefill64(p["q"], p["k"], p["v"], p["cu"], ax.GQA_SCALE))


# ---------------------------------------------------------------- the closed forms of the GPU tests
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (16, 1)])
def test_windowed_counting_mean_is_the_restatement(Hq, Hkv):
    c = ax.gqa_count_case(wr.DECODE_N, Hq, Hkv)
    for W in wr.DECODE_WINDOWS + [-1]:
        want = wr.gqa_count_want(c, Hq, W)
        ref = wr.decode64_window(c["q"][:, 0].float(), c["K"], c["V"], c["lens"], ax.GQA_SCALE, W)
        assert float((want - ref).abs().max()) < 1e-12, W
        ax.check_count(ref.to(torch.bfloat16), want)  # one bf16 rounding stays inside the bar
    assert torch.equal(wr.gqa_count_want(c, Hq, -1), c["want"]) and torch.equal(wr.gqa_count_want(c, Hq, 200), c["want"])


@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (8, 2), (32, 1)])
def test_windowed_prefill_counting_mean_is_the_restatement(Hq, Hkv):
    c = ax.prefill_count_case(ax.PREFILL_SEQS, Hq, Hkv, 128, ax.P_GQA)
    for W in wr.PREFILL_WINDOWS:
        want = wr.prefill_count_want(c, Hq, W)
        ref = wr.prefill64_window(c["q"], c["k"], c["v"], c["cu"], ax.GQA_SCALE, W)
        assert float((want - ref).abs().max()) < 1e-12, W
    assert torch.equal(wr.prefill_count_want(c, Hq, 1000), c["want"])


@pytest.mark.parametrize("c", sorted(wr.SOFTCAP_LEVELS))
def test_two_level_soft_cap_weights_are_the_restatement(c):
    case = wr.gqa_softcap_case(8, 2, c)
    for W in (-1, 40):
        want = wr.gqa_softcap_want(case, 8, W)
        ref = wr.decode64_window(case["q"][:, 0].float(), case["K"], case["V"], case["lens"], ax.GQA_SCALE, W, c)
        assert float((want - ref).abs().max()) < 1e-9, (c, W)
        # and the case tells a capped kernel from an uncapped one by far more than the bar
        off = wr.decode64_window(case["q"][:, 0].float(), case["K"], case["V"], case["lens"], ax.GQA_SCALE, W, 0.0)
        assert float((off - ref).abs().max()) > 0.3
    k_a, _ = wr.SOFTCAP_LEVELS[c]
    assert 2.5 * c <= abs(ax.Q_AMP * k_a * ax.GQA_SCALE) <= 3.5 * c


def test_no_position_channel_counts_more_than_16_permitted_keys():
    """the precondition of REL_COUNT (one key more or less moves a channel by >= 1/17), for every (L, W) the GPU tests use"""
    for Hq, Hkv in [(4, 4), (8, 2), (16, 1)]:
        c = ax.gqa_count_case(wr.DECODE_N, Hq, Hkv)
        for W in wr.DECODE_WINDOWS:
            assert wr.max_keys_per_position_channel_window(c["V"], c["lens"], W, ax.P_GQA) <= 16
    for Hq, Hkv in [(8, 8), (8, 2), (32, 1)]:
        c = ax.prefill_count_case(ax.PREFILL_SEQS, Hq, Hkv, 128, ax.P_GQA)
        for s0, s1 in zip(c["cu"][:-1], c["cu"][1:]):
            for W in wr.PREFILL_WINDOWS:
                assert wr.max_keys_per_position_channel_window(c["v"][s0:s1], range(1, s1 - s0 + 1), W, ax.P_GQA) <= 16


# ---------------------------------------------------------------- header, documents, exports
def _header():
    return open(os.path.join(ROOT, "include", "chitu_hip.h")).read()


def _params(text, name):
    body = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1)
    return [" ".join(p.split()) for p in body.split(",")]


def test_header_declares_the_entries_as_their_plain_twins_plus_two_arguments():
    text = _header()
    assert int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)) >= 8
    for name in ENTRIES:
        plain = _params(text, PLAIN[name])
        assert _params(text, name) == plain[:-1] + ["int32_t window_left", "float softcap", "void* stream"], name
        # these have a reference counterpart (window_size / softcap of the AttnBackend interface): the note cites it
        assert not re.search(name + r"\s+new: no reference counterpart", text), name
    notes = re.findall(r"/\*.*?\*/", text, flags=re.S)
    for name in ENTRIES:
        note = [n for n in notes if name in n and "attn_backend.py" in n and "window_left" in n and "softcap" in n]
        assert note, f"{name}: no header note that cites the reference and explains the two arguments"


def test_docs_agree_with_the_header_on_entry_count_and_abi_version():
    text = _header()
    n = len(re.findall(r"^int chitu_hip_\w+\s*\(", text, flags=re.M))
    version = re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{n} entry points, ABI version {version}" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in integ.splitlines() if l.startswith("| 7 → 8 |")]
    assert len(row) == 1 and all(name in row[0] for name in ENTRIES)


def _cdll():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_the_entries():
    lib = _cdll()
    assert all(hasattr(lib, name) for name in ENTRIES)


def test_entries_refuse_a_bad_window_or_cap_on_the_host():
    """Nothing is launched (batch 0 / no sequences; the pointers are never dereferenced), so this needs no GPU."""
    lib = _cdll()
    buf = ctypes.create_string_buffer(128)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    BAD_ARG, UNSUPPORTED = -1, -2

    for entry in (lib.chitu_hip_gqa_decode_window, lib.chitu_hip_gqa_decode_kv_fp8_window):

        def decode(W=-1, c=0.0, hd=128, splits=1):
            return entry(p, i64(4096), i64(128), p, p, i64(4), i32(16), i32(8), p, i32(4), p, f32(0.1), p, i32(0), i32(32), i32(hd),
                         i32(splits), p, i64(0), i32(W), f32(c), None)

        assert decode() == 0 and decode(W=0) == 0 and decode(W=2 ** 31 - 1, c=30.0) == 0 and decode(c=5.0) == 0
        assert decode(W=-2) == BAD_ARG and decode(W=-(2 ** 31)) == BAD_ARG
        assert decode(c=-1.0) == BAD_ARG and decode(c=-1e-30) == BAD_ARG and decode(c=float("nan")) == BAD_ARG
        assert decode(W=4, hd=64) == UNSUPPORTED and decode(W=4, splits=0) == BAD_ARG  # the plain entry's checks still hold

    def prefill(W=-1, c=0.0, hd=128, hq=8, hkv=2):
        return lib.chitu_hip_gqa_prefill_window(p, i64(1024), i64(128), p, i64(256), i64(128), p, i64(256), i64(128), p, i32(0), i32(0),
                                                f32(0.1), p, i32(hq), i32(hkv), i32(hd), i32(W), f32(c), None)

    assert prefill() == 0 and prefill(W=0) == 0 and prefill(W=511, c=5.0) == 0
    assert prefill(W=-2) == BAD_ARG and prefill(c=-0.5) == BAD_ARG and prefill(c=float("nan")) == BAD_ARG
    assert prefill(W=4, hd=64) == UNSUPPORTED and prefill(W=4, hq=6, hkv=2) == UNSUPPORTED


# ---------------------------------------------------------------- the Python surface
def test_backend_accepts_left_windows_and_refuses_the_rest():
    from chitu_amd.attn_backend import HipAttnBackend, window_and_cap

    assert window_and_cap((-1, -1), 0.0, False) == (-1, 0.0) and window_and_cap((-1, -1), 0.0, True) == (-1, 0.0)
    assert window_and_cap((7, 0), 0.0, False) == (7, 0.0) and window_and_cap([0, 0], 5.0, False) == (0, 5.0)
    assert window_and_cap((7, -1), 0.0, True) == (7, 0.0) and window_and_cap((7, 3), 2.5, True) == (7, 2.5)  # causal: the right side is 0
    for bad in ((7, -1), (7, 3), (-1, 3)):
        with pytest.raises(NotImplementedError):
            window_and_cap(bad, 0.0, False)
    for bad in ((-2, 0), (3, -2)):
        with pytest.raises(ValueError):
            window_and_cap(bad, 0.0, True)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            window_and_cap((-1, -1), bad, False)

    # through the public call, before anything touches a device
    be = HipAttnBackend(local_n_heads=8)
    q = torch.zeros(1, 1, 8, 128, dtype=torch.bfloat16)
    kc = torch.zeros(2, 16, 2, 128, dtype=torch.bfloat16)
    table, lens = torch.zeros(1, 2, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        be.attn_with_kvcache(q, kc, kc.clone(), cache_seqlens=lens, block_table=table, window_size=(4, 2))
    with pytest.raises(NotImplementedError):
        be.attn_with_kvcache(q, kc, kc.clone(), cache_seqlens=lens, block_table=table, window_size=(4, -1))
    with pytest.raises(ValueError):
        be.attn_with_kvcache(q, kc, kc.clone(), cache_seqlens=lens, block_table=table, softcap=-1.0)
    with pytest.raises(AssertionError):
        be.attn_with_kvcache(q, kc, kc.clone(), cache_seqlens=lens, block_table=table, cache_leftpad=lens, window_size=(4, 0))
    with pytest.raises(ValueError):
        be.attn_varlen_func(q[0], kc[0, :1], kc[0, :1], lens, lens, 1, 1, causal=True, softcap=-2.0)
    # the MLA branches keep refusing both
    with pytest.raises(AssertionError):
        be.attn_varlen_func(torch.zeros(1, 8, 576), torch.zeros(1, 1, 576), torch.zeros(1, 1, 512), lens, lens, 1, 1, causal=True, window_size=(4, 0))
    with pytest.raises(AssertionError):
        be.mla_attn_with_kvcache(None, None, None, None, 0, 1, None, window_size=(4, 0))


def test_split_count_under_a_window_follows_the_steps_the_window_overlaps():
    from chitu_amd import attn_backend as ab

    for args in ((1, 8, 128, 256), (16, 8, 16, 256), (4, 2, 1, 16), (64, 8, 4, 256)):
        assert ab.gqa_num_splits(*args, window_left=-1) == ab.gqa_num_splits(*args)
        assert ab.gqa_num_splits(*args, window_left=2 ** 31 - 1) <= ab.gqa_num_splits(*args) + 1
    assert ab.gqa_num_splits(1, 8, 128, 256, window_left=0) == 2          # (0 + 16) // 16 + 1 steps at the most
    assert ab.gqa_num_splits(1, 8, 128, 256, window_left=40) == 4         # 56 // 16 + 1
    assert ab.gqa_num_splits(1, 8, 128, 256, window_left=4095) == ab.gqa_num_splits(1, 8, 16, 256)  # the cap decides both


def test_model_args_carry_the_window_and_the_cap():
    from chitu_amd.llama import LlamaArgs, LlamaAttention
    from chitu_amd.mixtral import MixtralArgs

    for cls in (LlamaArgs, MixtralArgs):
        a = cls()
        assert a.sliding_window is None and a.attn_softcap == 0.0
    small = dict(dim=512, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=64, ffn_dim=128)
    at = LlamaAttention(LlamaArgs(**small), 0, None, None, device="cpu")
    assert at.window_size == (-1, -1) and at.softcap == 0.0
    # Hugging Face's rule: a token sees the last `sliding_window` positions, itself included -> window_left = sliding_window - 1
    at = LlamaAttention(LlamaArgs(sliding_window=4096, attn_softcap=30.0, **small), 0, None, None, device="cpu")
    assert at.window_size == (4095, 0) and at.softcap == 30.0
    assert LlamaAttention(LlamaArgs(sliding_window=1, **small), 0, None, None, device="cpu").window_size == (0, 0)
    with pytest.raises(ValueError):
        LlamaAttention(LlamaArgs(sliding_window=0, **small), 0, None, None, device="cpu")
