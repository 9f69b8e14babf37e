"""Continued prefill over the paged K / V cache (chitu_hip_gqa_prefill_paged): the case builders shared by
tests/test_gpu_prefill_paged.py (GPU) and tests/test_prefill_paged_host.py (CPU).  Builds on tests/attn_exact.py and
tests/attn_window_ref.py and leaves them alone.

A case is a ragged batch: sequence s has L_s keys (logical rows K[s], V[s] in token order), the last n_s of them new; its n_s query
rows sit at positions P_s + i, P_s = L_s - n_s.  Everything rests on one equivalence (the bottom-right aligned causal mask): query
i of sequence s is the SINGLE-token decode of a row of length P_s + i + 1 over the same keys, so the fp64 expectation is
attn_exact.decode64 (attn_window_ref.decode64_window with a window or a cap) with those lengths, and the closed forms of
attn_exact's constructions carry over.  Expected values never come from a kernel."""
import torch

from tests import attn_exact as ax
from tests import attn_window_ref as wr

PREFIXES = [0, 1, 15, 16, 17, 63, 64, 65, 200]
NEWS = [1, 2, 31, 33, 129]
PAGES = [16, 64, 256, 48]  # 48: a multiple of 16 that is no power of two and does not divide the 64-key tile


def pairs():
    """every prefix once, the new lengths in turn: the 9 sequences of one ragged launch, every new length at least once (129 new
    rows behind prefix 17, 33 behind prefix 200)"""
    return [(P, NEWS[j % len(NEWS)]) for j, P in enumerate(PREFIXES)]


def query_lengths(P, n):
    """the single-token lengths of the n queries behind prefix P (a query before key 0 sees nothing)"""
    return [max(P + i + 1, 0) for i in range(n)]


def cu_q(case):
    return ax.cu_of(case["news"])


def expected64(case, scale=ax.GQA_SCALE, W=-1, c=0.0):
    """[T, Hq, 128] fp64: decode64 over the first P + i + 1 keys for each query (window / cap: decode64_window)"""
    out, cu = [], cu_q(case)
    for s, (P, n) in enumerate(zip(case["prefixes"], case["news"])):
        q = case["q"][cu[s] : cu[s + 1]].float()
        if W < 0 and c == 0.0:
            out.append(ax.decode64(q, case["K"][s], case["V"][s], query_lengths(P, n), scale))
        else:
            out.append(wr.decode64_window(q, case["K"][s], case["V"][s], query_lengths(P, n), scale, W, c))
    return torch.cat(out)


# ---------------------------------------------------------------- pages
def paginate(case, page, seed=0, k_fill=ax.K_AMP, v_fill=1.0, n_spare=2, extra=2, dead_before=None, poison_fill=None):
    """Scatter every sequence's logical rows into pages under a random block table.  Returns (k_cache, v_cache
    [pages, page, Hkv, 128] bf16, table [n_seq, width] int32, lens [n_seq] int32).  All sequences' pages are one random
    permutation of the pool, so a sequence's table is a random, non-contiguous, unordered set of pages.  Rows past L in a last
    page, the n_spare spare pages and -- dead_before[s] = the sequence's lowest visible key -- the pages wholly before it hold the
    fill (what a correct kernel never uses; poison_fill overrides both fills, e.g. NaN).  Table entries past ceil(L / page) name a
    spare page: a valid index of a page no sequence needs."""
    Ls = [max(P + n, 0) for P, n in zip(case["prefixes"], case["news"])]
    Hkv = case["K"][0].shape[1]
    need = [max(1, -(-L // page)) for L in Ls]
    total = sum(need) + n_spare
    perm = torch.randperm(total, generator=torch.Generator().manual_seed(seed)).tolist()
    kf, vf = (k_fill, v_fill) if poison_fill is None else (poison_fill, poison_fill)
    kc = torch.full((total, page, Hkv, 128), float(kf))
    vc = torch.full((total, page, Hkv, 128), float(vf))
    width = max(need) + extra
    spare = perm[sum(need) :]
    table = torch.zeros(len(Ls), width, dtype=torch.int32)
    at = 0
    for s, L in enumerate(Ls):
        ids = perm[at : at + need[s]]
        at += need[s]
        table[s, : need[s]] = torch.tensor(ids, dtype=torch.int32)
        table[s, need[s] :] = torch.tensor([spare[(s + j) % len(spare)] for j in range(width - need[s])], dtype=torch.int32)
        first = 0 if dead_before is None else max(0, int(dead_before[s])) // page
        for j, pid in enumerate(ids):
            if j < first:
                continue  # wholly before the lowest visible key: keeps the fill
            r0, r1 = j * page, min((j + 1) * page, L)
            kc[pid, : r1 - r0] = case["K"][s][r0:r1]
            vc[pid, : r1 - r0] = case["V"][s][r0:r1]
    return kc.to(torch.bfloat16), vc.to(torch.bfloat16), table, torch.tensor(Ls, dtype=torch.int32)


def lowest_visible(case, W):
    """per sequence: the lowest key any of its queries sees (0 without a window)"""
    return [0 if W < 0 else max(0, P - W) for P in case["prefixes"]]


# ---------------------------------------------------------------- construction 1: counting
def count_case(seq_pairs, Hq, Hkv, seed=0):
    """q = 0: query i of sequence s must be the mean of exactly its first P + i + 1 V rows (indicator rows, attn_exact.count_rows,
    other offsets per head and sequence).  want [T, Hq, 128] fp64 from the closed form n_d / n."""
    prefixes, news = [p for p, _ in seq_pairs], [n for _, n in seq_pairs]
    K, V, want = [], [], []
    for s, (P, n) in enumerate(seq_pairs):
        L = P + n
        v = ax.count_rows(L, [7 * h + 13 * s + 3 for h in range(Hkv)], 128, ax.P_GQA, ax.TILE)
        V.append(v)
        K.append(ax.small_ints((L, Hkv, 128), seed + s))
        want.append(ax.count_expected(v)[query_lengths(P, n)])
    q = torch.zeros(sum(news), Hq, 128)
    return dict(q=q, K=K, V=V, prefixes=prefixes, news=news, want=torch.cat(want).repeat_interleave(Hq // Hkv, dim=1))


def count_want_window(case, Hq, W):
    """count_case under window W: exactly min(W + 1, P + i + 1) keys, the last ones"""
    want = [wr.count_expected_window(v, query_lengths(P, n), W) for v, P, n in zip(case["V"], case["prefixes"], case["news"])]
    return torch.cat(want).repeat_interleave(Hq // case["V"][0].shape[1], dim=1)


def max_keys_per_position_channel(case, W=-1):
    """the most permitted keys any position channel counts over all queries (REL_COUNT needs <= 16)"""
    return max(wr.max_keys_per_position_channel_window(v, query_lengths(P, n), W, ax.P_GQA) if W >= 0
               else ax.max_keys_per_position_channel(v, ax.P_GQA) for v, P, n in zip(case["V"], case["prefixes"], case["news"]))


# ---------------------------------------------------------------- construction 2: dominant keys
def probes_of(P, n, i, page, W=-1):
    """[(inside, outside)] for query i (position p = P + i): the keys 0, P - 1, P and the first and last key of every page and
    every 64-key tile, where visible; every 4th query and each sequence's first two and last two also their own key p and, under a
    window, their first visible key (a channel per probed key, 128 channels: not every query can have its own two).  Every 8th
    query and each sequence's last-but-one also look one key PAST the causal edge (and one before the window) with the dominant
    amplitude, beside their own key p with half of it -- the answer is row p, a kernel that admits the key outside returns that
    key's row."""
    p = P + i
    w0 = 0 if W < 0 else max(0, p - W)
    own = i % 4 == 0 or i in (1, n - 2, n - 1)
    keys = {x for x in (0, P - 1, P) if w0 <= x <= p} | ({w0, p} if own else set())
    for step in (page, ax.TILE):
        for e in range(step, p + 1, step):
            keys |= {x for x in (e - 1, e) if w0 <= x <= p}
    out = [(x, None) for x in sorted(keys or {p})]
    if i % 8 == 0 or i == n - 2:
        if i + 1 < n:
            out.append((p, p + 1))
        if w0 >= 1:
            out.append((p, w0 - 1))
    return out


def dominant_case(seq_pairs, Hq, Hkv, page, W=-1):
    """Head h of query i of sequence s probes probes_of(...)[(i * Hq + h + s) % len]: one-hot q of amplitude 32 in the probed key's
    channel, that key 16 there, every other key 0: a lead of >= 45 nats, the output is the probed key's V row (identity rows
    spelling sequence, head, token).  Channels are given out per sequence to the keys some query probes (<= 128)."""
    prefixes, news = [p for p, _ in seq_pairs], [n for _, n in seq_pairs]
    G = Hq // Hkv
    K, V, qs, wants = [], [], [], []
    for s, (P, n) in enumerate(seq_pairs):
        L = P + n
        picks = {}
        for i in range(n):
            pr = probes_of(P, n, i, page, W)
            for h in range(Hq):
                picks[(i, h)] = pr[(i * Hq + h + s) % len(pr)]
        tokens = sorted({x for pair in picks.values() for x in pair if x is not None})
        if 0 <= W <= 125:  # no query scores two keys 128 apart (its window and the two keys outside span W + 3): channels repeat
            ch = {x: x % 128 for x in tokens}
        else:
            assert len(tokens) <= 128, (P, n, len(tokens))
            ch = {x: c for c, x in enumerate(tokens)}
        k = ax.small_ints((L, Hkv, 128), s)
        k[:, :, : max(ch.values()) + 1] = 0.0
        for x, c in ch.items():
            k[x, :, c] = ax.K_AMP
        v = ax.identity_rows(L, Hkv, 128, seq=s)
        q = torch.zeros(n, Hq, 128)
        want = torch.zeros(n, Hq, 128, dtype=torch.float64)
        for (i, h), (inside, outside) in picks.items():
            if outside is None:
                q[i, h, ch[inside]] = ax.Q_AMP
            else:
                q[i, h, ch[outside]], q[i, h, ch[inside]] = ax.Q_AMP, ax.Q_AMP / 2
            want[i, h] = v[inside, h // G].double()
        K.append(k), V.append(v), qs.append(q), wants.append(want)
    assert ax.leak_bound(max(P + n for P, n in seq_pairs), 15.0, ax.margin_nats(ax.Q_AMP / 2, ax.K_AMP, ax.GQA_SCALE)) < ax.ABS_DOMINANT
    return dict(q=torch.cat(qs), K=K, V=V, prefixes=prefixes, news=news, want=torch.cat(wants))


# ---------------------------------------------------------------- random data
def random_case(seq_pairs, Hq, Hkv, seed=0):
    """random q, K and V (bf16 values); no expected value: expected64"""
    g = torch.Generator().manual_seed(seed)
    prefixes, news = [p for p, _ in seq_pairs], [n for _, n in seq_pairs]
    q = (torch.randn(sum(news), Hq, 128, generator=g) * 0.5).to(torch.bfloat16).float()
    K = [torch.randn(max(P + n, 1), Hkv, 128, generator=g).to(torch.bfloat16).float() for P, n in seq_pairs]
    V = [torch.randn(max(P + n, 1), Hkv, 128, generator=g).to(torch.bfloat16).float() for P, n in seq_pairs]
    return dict(q=q, K=K, V=V, prefixes=prefixes, news=news)


def whole_sequence_case(L, Hq, Hkv, seed=0):
    """one sequence of L random rows with a query for every row: what the contiguous kernel takes (q, k, v [L, ., 128])"""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(L, Hq, 128, generator=g) * 0.5).to(torch.bfloat16)
    k = torch.randn(L, Hkv, 128, generator=g).to(torch.bfloat16)
    v = torch.randn(L, Hkv, 128, generator=g).to(torch.bfloat16)
    return q, k, v
