"""The flash GQA prefill at any group size, the parts that need no GPU: the fourth extension header against the library's exports,
the host-side argument checks of its two entries, the builders of tests/attn_group_ref.py against the fp64 attention, and the
G = 5 Qwen3 fixture (tests/golden/qwen3_g5_hf.npz, Hugging Face's fp32 run) against the CPU restatement of tests/qwen3_ref.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import attn_exact as ax
from tests import attn_group_ref as gr
from tests import qwen3_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT4_HEADER = os.path.join(ROOT, "include", "chitu_hip_ext4.h")
ENTRIES = ("chitu_ext4_gqa_prefill", "chitu_ext4_gqa_prefill_paged")


def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


# ---------------------------------------------------------------- the header
def _params(src, entry):
    text = re.search(r"\bint\s+" + entry + r"\s*\((.*?)\);", src, flags=re.S).group(1)
    return [" ".join(p.split()) for p in text.split(",")]


def test_ext4_header_declares_exactly_the_exported_ext4_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(EXT4_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(chitu_ext4_\w+)\s*\(", src)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib().LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT\s+(chitu_ext4_\w+)", out)))
    assert declared == exported == sorted(ENTRIES)
    assert re.search(r"#define\s+CHITU_HIP_EXT4_VERSION\s+1\b", src) and '#include "chitu_hip.h"' in src
    # nothing of the frozen prefixes
    assert not re.findall(r"\bint\s+(chitu_hip_\w+|chitu_ext_\w+|chitu_ext2_\w+|chitu_ext3_\w+)\s*\(", src)


def test_the_entries_have_the_argument_lists_of_the_old_ones():
    old = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chitu_hip.h")).read(), flags=re.S)
    new = re.sub(r"/\*.*?\*/", "", open(EXT4_HEADER).read(), flags=re.S)
    assert _params(new, "chitu_ext4_gqa_prefill") == _params(old, "chitu_hip_gqa_prefill_window")
    assert _params(new, "chitu_ext4_gqa_prefill_paged") == _params(old, "chitu_hip_gqa_prefill_paged")


# ---------------------------------------------------------------- host argument checks
I32, I64, F32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
PTRS = {"contig": ("q", "k", "v", "cu", "out"), "paged": ("q", "kc", "vc", "table", "cu", "lens", "out")}
ALIGNED = {"contig": ("q", "k", "v", "out"), "paged": ("q", "kc", "vc", "out")}


def _contig(p, n_seq, hq=40, hkv=8, hd=128, W=-1, c=0.0, **over):
    a = dict(q=p, q_st=I64(hq * 128), q_sh=I64(128), k=p, k_st=I64(hkv * 128), k_sh=I64(128), v=p, v_st=I64(hkv * 128), v_sh=I64(128),
             cu=p, n_seq=I32(n_seq), max_seqlen=I32(64), scale=F32(0.1), out=p, hq=I32(hq), hkv=I32(hkv), hd=I32(hd), W=I32(W),
             c=F32(c), stream=None)
    a.update(over)
    return list(a.values())


def _paged(p, n_seq, hq=40, hkv=8, hd=128, W=-1, c=0.0, page=16, **over):
    a = dict(q=p, q_st=I64(hq * 128), q_sh=I64(128), kc=p, vc=p, pages=I64(4), page=I32(page), hkv=I32(hkv), table=p, ts=I32(4), cu=p,
             lens=p, n_seq=I32(n_seq), max_seqlen=I32(64), scale=F32(0.1), out=p, hq=I32(hq), hd=I32(hd), W=I32(W), c=F32(c),
             stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("n_seq", [0, 2])
def test_entries_check_their_arguments_on_the_host(n_seq):
    """Argument checks run before anything is launched and before the zero-size return: the pointers are host memory and are
    never dereferenced (with a launch these calls would return a HIP error or fault, not -1 / -2)."""
    lib = ctypes.CDLL(_lib().LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 8)
    for kind, entry, args in (("contig", lib.chitu_ext4_gqa_prefill, _contig), ("paged", lib.chitu_ext4_gqa_prefill_paged, _paged)):
        for name in PTRS[kind]:
            assert entry(*args(p, n_seq, **{name: None})) == -1, (kind, name)
        for name in ALIGNED[kind]:
            assert entry(*args(p, n_seq, **{name: odd})) == -1, (kind, name)
        assert entry(*args(p, n_seq, q_st=I64(40 * 128 + 4))) == -1 and entry(*args(p, n_seq, q_sh=I64(132))) == -1
        assert entry(*args(p, n_seq, W=-2)) == -1 and entry(*args(p, n_seq, c=-1.0)) == -1
        assert entry(*args(p, n_seq, c=float("nan"))) == -1 and entry(*args(p, -1)) == -1
        assert entry(*args(p, n_seq, hd=64)) == -2, kind
        assert entry(*args(p, n_seq, hq=33, hkv=1)) == -2 and entry(*args(p, n_seq, hq=66, hkv=2)) == -2, kind  # G = 33
        assert entry(*args(p, n_seq, hq=7, hkv=2)) == -1 and entry(*args(p, n_seq, hq=0, hkv=1)) == -1, kind
        if n_seq == 0:  # nothing to do: 0 with nothing launched, at every group size
            for G in (3, 5, 6, 7, 12, 24) + tuple(range(1, 33)):
                assert entry(*args(p, 0, hq=G, hkv=1)) == 0 and entry(*args(p, 0, hq=2 * G, hkv=2, W=5, c=5.0)) == 0, (kind, G)
        else:  # work to do but no query row to launch for
            assert entry(*args(p, n_seq, max_seqlen=I32(0))) == 0
    assert lib.chitu_ext4_gqa_prefill_paged(*_paged(p, n_seq, page=24)) == -2
    assert lib.chitu_ext4_gqa_prefill_paged(*_paged(p, n_seq, page=0)) == -2
    assert lib.chitu_ext4_gqa_prefill_paged(*_paged(p, n_seq, ts=I32(0))) == -1
    assert lib.chitu_ext4_gqa_prefill_paged(*_paged(p, n_seq, pages=I64(0))) == -1
    # the old entries still refuse what they refused
    assert lib.chitu_hip_gqa_prefill_window(*_contig(p, n_seq, hq=24, hkv=8)) == -2
    assert lib.chitu_hip_gqa_prefill_paged(*_paged(p, n_seq, hq=24, hkv=8)) == -2


# ---------------------------------------------------------------- the builders
@pytest.mark.parametrize("Hq,Hkv", gr.GROUPS + [(24, 1)])
def test_sequence_lengths_bracket_the_workgroup_and_keep_the_counting_precondition(Hq, Hkv):
    G = Hq // Hkv
    BQ = gr.block_tokens(G)
    seqs = gr.seqs_for(G)
    assert set(ax.PREFILL_SEQS) <= set(seqs) and {BQ - 1, BQ, BQ + 1, 2 * BQ + 1} <= set(seqs) and len(set(seqs)) == len(seqs)
    assert BQ * G <= 128 < (BQ + 1) * G and (128 - BQ * G > 0) == (32 % G != 0)
    count = ax.prefill_count_case(seqs, Hq, Hkv, 128, ax.P_GQA)
    worst = max(ax.max_keys_per_position_channel(count["v"][s0:s1], ax.P_GQA) for s0, s1 in zip(count["cu"][:-1], count["cu"][1:]))
    assert worst <= 16, worst
    want = ax.prefill64(count["q"], count["k"], count["v"], count["cu"], ax.GQA_SCALE)
    ax.check_count(want.to(torch.bfloat16), count["want"])


@pytest.mark.parametrize("Hq,Hkv", gr.GROUPS)
def test_group_dominant_case_tells_the_heads_of_a_group_apart(Hq, Hkv):
    G = Hq // Hkv
    case = gr.group_dominant_case(gr.seqs_for(G), Hq, Hkv)
    got = ax.prefill64(case["q"], case["k"], case["v"], case["cu"], case["scale"])
    ax.check_tied(got.to(torch.bfloat16), case["want"])
    # the lead of the tied keys over every other one, and each head's answer: sequences under 128 tokens have no ties, so head h of
    # token i returns the identity row of key max(i - h % G, 0)
    assert ax.margin_nats(ax.Q_AMP, ax.K_AMP, ax.GQA_SCALE) >= ax.MIN_MARGIN_NATS
    s0, s1 = case["cu"][2], case["cu"][3]  # the 63-token sequence
    for h in range(Hq):
        i = torch.arange(s1 - s0)
        rows = case["v"][s0 + (i - h % G).clamp(min=0), h // G].double()
        assert float((case["want"][s0:s1, h] - rows).abs().max()) <= ax.ABS_DOMINANT, h
    # two heads of one group exchanged (and a head paired with the next KV head's group) are seen, by a whole digit
    for a, b in [(0, 1), (G - 2, G - 1), (0, G - 1)] + ([(G - 1, G)] if Hkv > 1 else []):
        wrong = gr.swap_heads(case["want"], a, b)
        assert float((wrong - case["want"]).abs().max()) >= 1.0, (a, b)
        with pytest.raises(AssertionError):
            ax.check_tied(wrong.to(torch.bfloat16), case["want"])
    # ... which attn_exact.prefill_dominant_case cannot see within a group
    plain = ax.prefill_dominant_case(gr.seqs_for(G), Hq, Hkv, 128)
    assert torch.equal(gr.swap_heads(plain["want"], 0, G - 1), plain["want"])


# ---------------------------------------------------------------- the G = 5 Qwen3 fixture
def test_g5_fixture_is_met_by_the_cpu_restatement():
    g, cfg, hf = gr.qwen3_g5_fixture()
    assert (cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["hidden_size"]) == (5, 1, 128, 256)
    assert cfg["num_hidden_layers"] == 2 and set(g.keys()) == set(qr.fixture()[0].keys())
    args = qr.qwen3_args(cfg)
    p = qr.module_params(hf, args)
    fed = g["prompt"].tolist() + g["tokens"].tolist()[:-1]
    assert g["logits_fp32"].shape == (33, cfg["vocab_size"]) and g["k0_fp32"].shape == (len(fed), 1, 128)
    logits, k0 = qr.forward(p, fed, args)
    err, agree = qr.check_logits(logits[len(g["prompt"]) - 1:], g, "G = 5 restatement vs HF fp32")
    assert agree == 33, agree
    ref = torch.from_numpy(g["logits_fp32"])  # the generator's condition on its seed: 31 steps whose top-2 gap is clear of 2 * err
    top2 = ref.topk(2, -1).values
    assert int(((top2[:, 0] - top2[:, 1]) > 2 * err * ref.abs().amax(-1)).sum()) >= 31
    k_err = float((k0.float() - torch.from_numpy(g["k0_fp32"])).abs().max() / torch.from_numpy(g["k0_fp32"]).abs().max())
    assert k_err < 1e-2, k_err
