"""The flash GQA prefill at a group size that does not divide 32 (chitu_ext4_gqa_prefill[_paged], include/chitu_hip_ext4.h): the
builders shared by tests/test_gqa_group_host.py (CPU) and tests/test_gpu_gqa_group.py (GPU).  Builds on tests/attn_exact.py and
leaves it alone.

What is new at such a G is the row mapping: Q row R = 32 wave + lane of a workgroup is head R % G of token R / G, a token's heads
can lie in two waves, and the last 128 - (128 // G) * G rows are padding.  attn_exact.prefill_dominant_case gives every head of a
token the same query and the counting case has q = 0: two heads of a group exchanged, or a head paired with the neighbouring
token, is invisible to both.  group_dominant_case makes every (token, head) pair ask for a key of its own."""
import ast

import torch

from tests import attn_exact as ax
from tests.util import golden

GROUPS = [(6, 2), (5, 1), (7, 1), (12, 1)]  # G = 3, 5, 7, 12: 42, 25, 18 and 10 query tokens in a workgroup


def block_tokens(G):
    """BQ: the query tokens of one workgroup"""
    return 128 // G


def seqs_for(G):
    """attn_exact.PREFILL_SEQS and the lengths around one and two workgroups' tokens"""
    BQ = block_tokens(G)
    out = list(ax.PREFILL_SEQS)
    for n in (BQ - 1, BQ, BQ + 1, 2 * BQ + 1):
        if n >= 1 and n not in out:
            out.append(n)
    return out


def group_dominant_case(seqs, Hq, Hkv):
    """attn_exact.prefill_dominant_case with a query per HEAD: head h of query i steers to the channel of key max(i - h % G, 0)
    (key s has 16 in channel s mod 128, identity V rows), so the heads of a group look 0, 1, .. G - 1 tokens back.  The permitted
    keys congruent to that key tie; want: prefill64, the mean of the tied keys' identity rows (attn_exact.check_tied)."""
    G = Hq // Hkv
    cu = ax.cu_of(seqs)
    T = cu[-1]
    q, k, v = torch.zeros(T, Hq, 128), torch.zeros(T, Hkv, 128), torch.zeros(T, Hkv, 128)
    for s, (s0, s1) in enumerate(zip(cu[:-1], cu[1:])):
        i = torch.arange(s1 - s0)
        k[s0 + i, :, i % 128] = ax.K_AMP
        for h in range(Hq):
            q[s0 + i, h, (i - h % G).clamp(min=0) % 128] = ax.Q_AMP
        v[s0:s1] = ax.identity_rows(s1 - s0, Hkv, 128, seq=s)
    return dict(q=q, k=k, v=v, cu=cu, want=ax.prefill64(q, k, v, cu, ax.GQA_SCALE), scale=ax.GQA_SCALE)


def swap_heads(x, a, b):
    """x [T, Hq, 128] with heads a and b exchanged: what a kernel that mixes up two heads of a group would return"""
    y = x.clone()
    y[:, a], y[:, b] = x[:, b], x[:, a]
    return y


QWEN3_G5_SEED = 116  # tests/golden/gen_qwen3_g5_hf.py::SEED


def qwen3_g5_fixture():
    """(npz, config, HF name -> bf16 tensor) of tests/golden/qwen3_g5_hf.npz: tests.qwen3_ref.qwen3_hf_params under this
    fixture's seed"""
    from tests import qwen3_ref as qr

    g = golden("qwen3_g5_hf")
    seed, qr.SEED = qr.SEED, QWEN3_G5_SEED
    try:
        hf = qr.qwen3_hf_params(g)
    finally:
        qr.SEED = seed
    return g, ast.literal_eval(str(g["cfg"][0])), hf
