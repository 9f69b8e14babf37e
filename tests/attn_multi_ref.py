"""Multi-token GQA paged decode (chitu_hip_gqa_decode_multi: T <= 8 query tokens per sequence): the case builders and fixture
inputs shared by tests/test_gpu_gqa_multi.py (GPU), tests/test_gqa_multi_host.py (CPU) and tests/golden/gen_attn_multi.py (the
generator of tests/golden/attn_multi.npz, which runs the reference's RefAttnBackend._attention).  Builds on tests/attn_exact.py
and tests/attn_window_ref.py and leaves them alone.

Everything rests on one equivalence (the reference's bottom-right aligned causal mask, chitu/attn_backend.py:92-164): with
L = all keys of the sequence, the T new ones included, query (b, t) is the SINGLE-token decode of a row of length
L_t = L - T + t + 1 over the same keys (L_t <= 0: no visible key, zeros).  So a multi-token case is a single-token case of
tests/attn_exact.py / attn_window_ref.py built with the expanded lengths, ordered (b, t), whose q [bs * T, 1, Hq, 128] is
reshaped to [bs, T, Hq, 128]; the expected values are those builders' closed forms and fp64 attention, unchanged."""
import torch

from tests import attn_exact as ax
from tests import attn_window_ref as wr
from tests.util import lattice

MULTI_T = [2, 3, 4, 5, 8]
MULTI_HEADS = [(8, 2), (8, 1), (16, 1), (6, 2), (4, 4)]  # 4, 2, 1, 5 (15 of 16 columns) and 16 query tokens per tile
MULTI_SPLITS = [1, 2, 3, 5]
COUNT_N = 70


def expanded_lengths(totals, T):
    """[L_t for every (b, t)]: the single-token length of query t of a sequence of `totals[b]` keys"""
    return [max(int(L) - T + t + 1, 0) for L in totals for t in range(T)]


def tokens_per_tile(Hq, Hkv):
    return 16 // (Hq // Hkv)


def tile_split_edges(L, T, Hq, Hkv, splits, W=-1):
    """first key of every split of every tile of a sequence of L keys: the kernel's own arithmetic (csrc/gqa_decode_multi.hip)"""
    tpt, edges = tokens_per_tile(Hq, Hkv), set()
    for tok0 in range(0, T, tpt):
        tok1 = min(tok0 + tpt, T) - 1
        Lt = max(L - T + tok1 + 1, 0)
        f16 = wr.first_key(max(L - T + tok0 + 1, 0), W) >> 4 if W >= 0 else 0
        n16 = (Lt + 15) >> 4
        edges |= {16 * (f16 + (n16 - f16) * s // S) for S in splits for s in range(1, S)}
    return edges


# ---------------------------------------------------------------- construction 2: every query probes its own keys
def multi_dominant_case(n, T, Hq, Hkv, page, splits, W=-1):
    """Sequences of n keys.  Query t (L_t = n - T + t + 1 keys, the first one w0_t) probes, one key per (sequence, head of the group):
    its own last key L_t - 1, its first visible key w0_t (key 0 without a window), and both sides of every 16-key step, page and
    split edge inside [w0_t, L_t) -- amplitude 32 against 16: a lead of >= 45 nats, the answer is that key's V row.  Two more
    probes per query look PAST its range with amplitude 32 -- key L_t, the next draft token's own key, and key w0_t - 1 -- beside its
    own last key with amplitude 16 (a lead of 22.6 nats inside the range): the answer is row L_t - 1, and a kernel that admits the
    key outside returns that key's row instead.  Returns q [bs, T, Hq, 128], K, V, lens [bs] = n, want [bs * T, Hq, 128]."""
    G = Hq // Hkv
    edges = set(range(16, n, 16)) | set(range(page, n, page)) | tile_split_edges(n, T, Hq, Hkv, splits, W)
    per_t = []
    for t in range(T):
        Lt = n - T + t + 1
        w0 = wr.first_key(Lt, W)
        assert Lt >= 2
        inside = {Lt - 1, w0} | {x for e in edges for x in (e - 1, e) if w0 <= x < Lt}
        probes = [(x, None) for x in sorted(inside)]
        if Lt < n:
            probes.append((Lt - 1, Lt))
        if w0 >= 1:
            probes.append((Lt - 1, w0 - 1))
        per_t.append(probes)
    tokens = sorted({x for probes in per_t for pair in probes for x in pair if x is not None})
    assert len(tokens) <= 128, len(tokens)
    ch = {x: i for i, x in enumerate(tokens)}
    K = ax.small_ints((n, Hkv, 128), 5)
    K[:, :, : len(tokens)] = 0.0
    for x, i in ch.items():
        K[x, :, i] = ax.K_AMP
    V = ax.identity_rows(n, Hkv, 128)
    bs = max((len(p) + G - 1) // G for p in per_t)
    q = torch.zeros(bs, T, Hq, 128)
    want = torch.zeros(bs, T, Hq, 128, dtype=torch.float64)
    for b in range(bs):
        for t in range(T):
            for h in range(Hq):
                inside, outside = per_t[t][(b * G + h % G) % len(per_t[t])]
                if outside is None:
                    q[b, t, h, ch[inside]] = ax.Q_AMP
                else:
                    q[b, t, h, ch[outside]], q[b, t, h, ch[inside]] = ax.Q_AMP, ax.Q_AMP / 2
                want[b, t, h] = V[inside, h // G].double()
    assert ax.leak_bound(n, 15.0, ax.margin_nats(ax.Q_AMP / 2, ax.K_AMP, ax.GQA_SCALE)) < ax.ABS_DOMINANT
    return dict(q=q.to(torch.bfloat16), K=K, V=V, lens=torch.full((bs,), n, dtype=torch.int32), want=want.view(bs * T, Hq, 128),
                k_fill=ax.K_AMP, v_fill=15.0)


# ---------------------------------------------------------------- construction 3: the rescale vote of ANOTHER token's column
def multi_graded_case(n, T, Hq, Hkv, k_amps, tokens, probing_t, seed=0, q_amp=8.0):
    """Sequence (key, amplitude) of tokens x k_amps: ONLY query token `probing_t` steers to that key (channel = the sequence's index),
    which then leads its column by just under / just over kGqaDefer -- the wave-wide vote it casts or does not cast rescales every
    column of the tile.  The other query tokens hold small random values in channels 64 .. 127 (scores of a few nats against the
    random K rows), so their columns are the ones under test: running maxima that the step raises a little, or not at all.
    Random V.  want [bs * T, Hq, 128]: the fp64 attention on the expanded rows."""
    combos = [(x, a) for x in tokens for a in k_amps]
    assert len(combos) <= 64 and all(x <= n - T + probing_t for x in tokens)
    g = torch.Generator().manual_seed(seed)
    K = ax.small_ints((n, Hkv, 128), seed)
    K[:, :, : len(combos)] = 0.0
    q = torch.zeros(len(combos), T, Hq, 128)
    q[..., 64:] = torch.randint(-8, 9, (len(combos), T, Hq, 64), generator=g).float() / 4
    for i, (x, a) in enumerate(combos):
        K[x, :, i] = a
        q[i, probing_t] = 0.0
        q[i, probing_t, :, i] = q_amp
    V = torch.randn(n, Hkv, 128, generator=g).to(torch.bfloat16).float()
    lens = torch.full((len(combos),), n, dtype=torch.int32)
    want = wr.decode64_window(q.view(-1, Hq, 128), K, V, expanded_lengths(lens.tolist(), T), ax.GQA_SCALE)
    return dict(q=q.to(torch.bfloat16), K=K, V=V, lens=lens, want=want, k_fill=0.0, v_fill=0.0)


def multi_random_case(totals, T, Hq, Hkv, seed=0):
    """random q, K and V (bf16 values), ragged totals (totals below T included); no expected value: see multi_random_want"""
    n = max(max(totals), 1)
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(len(totals), T, Hq, 128, generator=g) * 0.5).to(torch.bfloat16)
    K = torch.randn(n, Hkv, 128, generator=g).to(torch.bfloat16).float()
    V = torch.randn(n, Hkv, 128, generator=g).to(torch.bfloat16).float()
    return dict(q=q, K=K, V=V, lens=torch.tensor(totals, dtype=torch.int32), k_fill=ax.K_AMP, v_fill=1.0)


def multi_random_want(case, W=-1, c=0.0):
    bs, T, Hq, _ = case["q"].shape
    return wr.decode64_window(case["q"].float().view(bs * T, Hq, 128), case["K"], case["V"], expanded_lengths(case["lens"].tolist(), T),
                              ax.GQA_SCALE, W, c)


# ---------------------------------------------------------------- tests/golden/attn_multi.npz
# The reference's RefAttnBackend._attention with causal=True on seqlen_q = T queries over a contiguous cache with a key padding
# mask.  Inputs are recomputed here (tests.util.lattice, the value sets of tests/attn_window_ref.py: exact in bf16 and in the fp8
# rows); only the reference's outputs are stored.
FIXM_HQ, FIXM_HKV = wr.FIX_HQ, wr.FIX_HKV
FIXM_T = [2, 4]
FIXM_WINDOWS = [-1, 0, 15]
FIXM_CAPS = [0.0, 5.0]
FIXM_CACHE_LEN = 112


def fixture_multi_lengths(T):
    """attended lengths, the T new rows included"""
    return [T, 16, 17, 100]


def fixture_multi_key(T, W, c):
    return f"t{T}_w{W}_c{c:g}".replace("-", "m")


def fixture_multi_inputs(T):
    """q [B, T, Hq, 128]; K, V [B, S, Hkv, 128] (all rows present: the fixture appends nothing); lens [B]"""
    B = len(fixture_multi_lengths(T))
    return dict(q=lattice(B, T, FIXM_HQ, 128, mod=89, scale=2.0, salt=11 + T),
                K=lattice(B, FIXM_CACHE_LEN, FIXM_HKV, 128, mod=17, scale=8.0, salt=1 + T),
                V=lattice(B, FIXM_CACHE_LEN, FIXM_HKV, 128, mod=17, scale=8.0, salt=5 + T),
                lens=torch.tensor(fixture_multi_lengths(T), dtype=torch.int32))
