"""Sliding-window and soft-capped attention: the fp64 restatements, closed forms and fixture inputs shared by
tests/test_attn_window_host.py (CPU), tests/test_gpu_attn_window.py (GPU) and tests/golden/gen_attn_window.py (the generator of
tests/golden/attn_window.npz, which runs the reference's RefAttnBackend).  Builds on tests/attn_exact.py and leaves it alone.

Semantics (the reference's, chitu/attn_backend.py:55-69 and RefAttnBackend._attention): window_left = W >= 0: the query at
position p sees key t iff p - W <= t <= p (decode: p = L - 1; prefill: p = the token's index inside its sequence); -1: no
window.  softcap = c > 0: the score is c * tanh(scale * q.k / c), before the mask and the softmax; 0: off."""
import math

import numpy as np
import torch

from tests import attn_exact as ax
from tests.util import lattice

# ---- what the GPU tests sweep (the host test checks REL_COUNT's precondition for every pair of these)
DECODE_N = 130
DECODE_WINDOWS = [0, 1, 15, 16, 17, 47, 64, 200]
PREFILL_WINDOWS = [0, 1, 31, 32, 63, 64, 65, 130]


def first_key(L, W):
    """w0: the first key the decode query of a sequence of L keys sees"""
    return 0 if W < 0 else max(0, L - 1 - W)


# ---------------------------------------------------------------- fp64 attention (attn_exact.decode64 / prefill64 + the two parameters)
def _cap(s, softcap):
    return softcap * torch.tanh(s / softcap) if softcap > 0 else s


def decode64_window(q, K, V, lens, scale, window_left=-1, softcap=0.0):
    """attn_exact.decode64 over the keys max(0, lens[b] - 1 - window_left) .. lens[b] - 1, soft-capped scores"""
    bs, Hq, _ = q.shape
    n, Hkv, _ = K.shape
    g = Hq // Hkv
    Kd, Vd = K.double().repeat_interleave(g, dim=1), V.double().repeat_interleave(g, dim=1)
    s = _cap(torch.einsum("bhd,nhd->bhn", q.double(), Kd) * scale, softcap)
    t, L = torch.arange(n).view(1, 1, n), torch.as_tensor(lens).view(bs, 1, 1)
    dead = t >= L
    if window_left >= 0:
        dead = dead | (t < L - 1 - window_left)
    p = torch.softmax(s.masked_fill(dead, float("-inf")), dim=-1)
    return torch.einsum("bhn,nhc->bhc", torch.nan_to_num(p, nan=0.0), Vd)


def prefill64_window(q, k, v, cu, scale, window_left=-1, softcap=0.0):
    """attn_exact.prefill64 where row t of a sequence sees its keys t - window_left .. t, soft-capped scores"""
    T, Hq, _ = q.shape
    g = Hq // k.shape[1]
    out = torch.zeros(T, Hq, v.shape[-1], dtype=torch.float64)
    for s0, s1 in zip(cu[:-1], cu[1:]):
        n = s1 - s0
        kk, vv = k[s0:s1].double().repeat_interleave(g, dim=1), v[s0:s1].double().repeat_interleave(g, dim=1)
        sc = _cap(torch.einsum("thd,shd->hts", q[s0:s1].double() * scale, kk), softcap)
        dead = torch.triu(torch.ones(n, n, dtype=torch.bool), diagonal=1)
        if window_left >= 0:
            dead = dead | torch.tril(torch.ones(n, n, dtype=torch.bool), diagonal=-(window_left + 1))
        out[s0:s1] = torch.einsum("hts,shc->thc", torch.softmax(sc.masked_fill(dead, float("-inf")), dim=-1), vv)
    return out


# ---------------------------------------------------------------- construction 1 under a window: a cumsum difference
def count_expected_window(rows, lens, W):
    """[n, heads, width] indicator rows -> [len(lens), heads, width] fp64: the mean of rows w0 .. L - 1 (L = 0: zeros)"""
    cs = torch.zeros(rows.shape[0] + 1, *rows.shape[1:], dtype=torch.float64)
    cs[1:] = rows.double().cumsum(0)
    out = torch.zeros(len(lens), *rows.shape[1:], dtype=torch.float64)
    for i, L in enumerate(int(x) for x in lens):
        if L > 0:
            w0 = first_key(L, W)
            out[i] = (cs[L] - cs[w0]) / (L - w0)
    return out


def gqa_count_want(case, Hq, W):
    """expected output of attn_exact.gqa_count_case under window W"""
    return count_expected_window(case["V"], case["lens"], W).repeat_interleave(Hq // case["V"].shape[1], dim=1)


def prefill_count_want(case, Hq, W):
    """expected output of attn_exact.prefill_count_case under window W: row i of a sequence is the mean of its rows i - W .. i"""
    v, cu = case["v"], case["cu"]
    want = torch.zeros(v.shape, dtype=torch.float64)
    for s0, s1 in zip(cu[:-1], cu[1:]):
        want[s0:s1] = count_expected_window(v[s0:s1], range(1, s1 - s0 + 1), W)
    return want.repeat_interleave(Hq // v.shape[1], dim=1)


def max_keys_per_position_channel_window(rows, lens, W, P):
    """the most permitted keys any position channel counts, over the given lengths (REL_COUNT needs <= 16)"""
    cs = torch.zeros(rows.shape[0] + 1, *rows.shape[1:])
    cs[1:] = rows.cumsum(0)
    return max((int((cs[L] - cs[first_key(L, W)])[..., :P].max()) for L in (int(x) for x in lens) if L > 0), default=0)


# ---------------------------------------------------------------- the two-level soft-cap case
# q is one-hot (amplitude 32, channel 0); even keys hold k_a there and odd keys k_b, so the scaled scores are s_a and s_b with
# |s_a| about 3 c; V rows are indicators of the two classes (channel 0: even keys, channel 1: odd keys).  Capped, the classes sit
# within a nat of each other; uncapped, class b has no weight at all -- a kernel that ignores the cap misses by ~0.4.
SOFTCAP_LEVELS = {5.0: (5.0, 3.0), 30.0: (-32.0, -22.0)}  # c -> (k_a, k_b): s = 32 k / sqrt(128) = (14.1, 8.5), (-90.5, -62.2)
SOFTCAP_LENGTHS = [1, 2, 17, 100, 130]


def gqa_softcap_case(Hq, Hkv, c, seed=0):
    k_a, k_b = SOFTCAP_LEVELS[c]
    n = max(SOFTCAP_LENGTHS)
    t = torch.arange(n)
    K = ax.small_ints((n, Hkv, 128), seed)
    K[:, :, 0] = torch.where(t % 2 == 0, k_a, k_b).view(n, 1)
    V = torch.zeros(n, Hkv, 128)
    V[t, :, t % 2] = 1.0
    q = torch.zeros(len(SOFTCAP_LENGTHS), 1, Hq, 128)
    q[:, :, :, 0] = ax.Q_AMP
    return dict(q=q.to(torch.bfloat16), K=K, V=V, lens=torch.tensor(SOFTCAP_LENGTHS, dtype=torch.int32), k_fill=ax.K_AMP, v_fill=1.0, c=c)


def gqa_softcap_want(case, Hq, W):
    """[bs, Hq, 128] fp64: the two class weights n_x e^{c tanh(s_x / c)} / sum, from the counts of even and odd keys in the window"""
    c = case["c"]
    k_a, k_b = SOFTCAP_LEVELS[c]
    e_a, e_b = (c * math.tanh(ax.Q_AMP * k * ax.GQA_SCALE / c) for k in (k_a, k_b))
    m = max(e_a, e_b)
    w_a, w_b = math.exp(e_a - m), math.exp(e_b - m)
    want = torch.zeros(len(case["lens"]), Hq, 128, dtype=torch.float64)
    for i, L in enumerate(int(x) for x in case["lens"]):
        w0 = first_key(L, W)
        n_a = len([t for t in range(w0, L) if t % 2 == 0])
        n_b = (L - w0) - n_a
        want[i, :, 0] = n_a * w_a / (n_a * w_a + n_b * w_b)
        want[i, :, 1] = n_b * w_b / (n_a * w_a + n_b * w_b)
    return want


# ---------------------------------------------------------------- tests/golden/attn_window.npz
# Inputs are recomputed here (tests.util.lattice), only the reference's outputs are stored.  K and V are multiples of 1/8 in
# [-1, 1]: exact in bf16 and, under any power-of-two row scale, in e4m3 -- so the fp8 cache holds the same rows.  q is large enough
# for the soft cap to matter (the generator asserts it).
FIX_HQ, FIX_HKV = 8, 2
FIX_LENGTHS = [1, 16, 17, 100, 130]   # attended lengths, the appended row included
FIX_WINDOWS = [-1, 0, 15, 16, 40]
FIX_CAPS = [0.0, 5.0]
FIX_SEQS = [1, 65, 130]
FIX_CACHE_LEN = 144
FIX_BAR = 1e-2


def fixture_key(kind, W, c):
    return f"{kind}_w{W}_c{c:g}".replace("-", "m")


def fixture_decode_inputs():
    """q [B, 1, Hq, 128]; contiguous caches [B, S, Hkv, 128] holding the rows before the append; the appended k / v [B, 1, Hkv, 128];
    cache_seqlens [B] = the lengths before the append"""
    B = len(FIX_LENGTHS)
    kc = lattice(B, FIX_CACHE_LEN, FIX_HKV, 128, mod=17, scale=8.0, salt=1)
    vc = lattice(B, FIX_CACHE_LEN, FIX_HKV, 128, mod=17, scale=8.0, salt=5)
    q = lattice(B, 1, FIX_HQ, 128, mod=89, scale=2.0, salt=11)
    k_new = lattice(B, 1, FIX_HKV, 128, mod=17, scale=8.0, salt=3)
    v_new = lattice(B, 1, FIX_HKV, 128, mod=17, scale=8.0, salt=9)
    return dict(q=q, k_cache=kc, v_cache=vc, k_new=k_new, v_new=v_new, cache_seqlens=torch.tensor(FIX_LENGTHS, dtype=torch.int64) - 1)


def fixture_decode_rows(inp):
    """the logical rows after the append, per sequence: K, V [B, S, Hkv, 128]"""
    K, V = inp["k_cache"].clone(), inp["v_cache"].clone()
    for b, L in enumerate(FIX_LENGTHS):
        K[b, L - 1], V[b, L - 1] = inp["k_new"][b, 0], inp["v_new"][b, 0]
    return K, V


def fixture_prefill_inputs():
    T = sum(FIX_SEQS)
    return dict(q=lattice(T, FIX_HQ, 128, mod=89, scale=2.0, salt=4), k=lattice(T, FIX_HKV, 128, mod=17, scale=8.0, salt=6),
                v=lattice(T, FIX_HKV, 128, mod=17, scale=8.0, salt=8), cu=ax.cu_of(FIX_SEQS))


def fixture_prefill_rows():
    """the rows of the prefill output the fixture keeps: both ends of every sequence, both sides of every window edge and of the
    kernel's 64-key tile edge"""
    keep = set()
    for s0, n in zip(ax.cu_of(FIX_SEQS)[:-1], FIX_SEQS):
        keep.update(s0 + i for i in (0, 1, 15, 16, 17, 40, 41, 42, 63, 64, 65, 100, 127, 128, n - 2, n - 1) if 0 <= i < n)
    return np.array(sorted(keep), dtype=np.int64)
