"""Input builders of the exact per-key attention tests (tests/test_gpu_attn_exact.py on the GPU, tests/test_attn_exact_host.py
through the oracles on the CPU).  Three constructions whose expected values have a closed form, so that ONE lost, doubled or
wrongly admitted key -- or one row fetched from the wrong page, head or sequence -- moves the result far outside the bar:

1. counting: q = 0, the softmax is uniform, the output is the mean of the V rows of exactly the permitted keys.  V rows are
   0/1 indicator rows: a position field (channel (t + c) mod P) in which no channel counts more than 16 keys, so one key more
   or less moves a channel by >= 1/17 of its value, and a block field (channel P + (t // block + c) mod P') that a block read
   from the wrong place moves by its full value.  c differs per KV head (and per sequence in prefill).  (A key that is admitted
   with a V row of zeros -- a score mask off by one in front of a staging step that zeroes rows past the end -- only shrinks every
   channel by n / (n + 1): counting sees that up to 62 keys, the probe of key n - 1 at every length.)
2. dominant key: q one-hot of amplitude 32, the probed key 16 in that channel, every other key 0 there: the probed key leads
   by 32 * 16 * scale >= 45 nats and the output is its V row.  V rows spell (sequence, KV head, token) in base-16 digits.
3. graded margin: construction 2 with the lead just under and just over a kernel's deferred-rescale constant, random V.

Every value is exact in bf16 and in both fp8 row formats (integers <= 16 beside a row maximum that gives a power-of-two scale).
Expected values come from the closed forms and from the fp64 attention below, never from a kernel."""
import math
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chitu_amd", "csrc")

# ---- the bars
# construction 1: the CPU oracle rounded to bf16 is within 2^-8 of n_d / n (one bf16 rounding; tests/test_attn_exact_host.py prints
# it); the kernels add at most one bf16 rounding of the split partials and one of the merge; a real error is >= 1/17 = 5.9 %.
REL_COUNT = 2.0 ** -6
# construction 2: the other keys leak n * max|V| * exp(-margin) ~ 1e-17 into an fp32 accumulator: a bound, not torch.equal
ABS_DOMINANT = 2.0 ** -20
MIN_MARGIN_NATS = 40.0
Q_AMP, K_AMP = 32.0, 16.0
GQA_SCALE = 128 ** -0.5
MLA_SCALE = 0.1352  # DeepSeek-V3's softmax scale (with its YaRN factor), the one the MLA suites use
P_GQA, P_MLA = 64, 256      # position-field widths: <= 16 keys per channel up to 1024 / 4096 keys
STEP_GQA, TILE = 16, 64     # the decode kernels' block sizes (gqa_decode_tile.h: 16-token steps; mla_decode_tile.h: kTile)
PREFILL_SEQS = [1, 2, 63, 64, 65, 127, 128, 129, 200]


def source_constant(file, name):
    """`constexpr <type> name = <number>` of a kernel source"""
    with open(os.path.join(CSRC, file)) as f:
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9.]+)f?\s*;", f.read())
    assert m, (file, name)
    return float(m.group(1))


# ---------------------------------------------------------------- fp64 attention (oracle/gqa.py and oracle/mla.py restated)
def decode64(q, K, V, lens, scale):
    """q [bs, Hq, D], K [n, Hkv, D], V [n, Hkv, Dv] (the logical rows, token order), lens [bs] -> [bs, Hq, Dv] fp64:
    softmax_t(scale * q . K[t, h // g]) . V[t, h // g] over t < lens[b]; an empty sequence gives zeros."""
    bs, Hq, _ = q.shape
    n, Hkv, _ = K.shape
    g = Hq // Hkv
    Kd, Vd = K.double().repeat_interleave(g, dim=1), V.double().repeat_interleave(g, dim=1)
    s = torch.einsum("bhd,nhd->bhn", q.double(), Kd) * scale
    dead = torch.arange(n).view(1, 1, n) >= torch.as_tensor(lens).view(bs, 1, 1)
    p = torch.softmax(s.masked_fill(dead, float("-inf")), dim=-1)
    return torch.einsum("bhn,nhc->bhc", torch.nan_to_num(p, nan=0.0), Vd)


def prefill64(q, k, v, cu, scale):
    """q [T, Hq, D], k [T, Hkv, D], v [T, Hkv, Dv], causal within each sequence of cu -> [T, Hq, Dv] fp64"""
    T, Hq, _ = q.shape
    g = Hq // k.shape[1]
    out = torch.zeros(T, Hq, v.shape[-1], dtype=torch.float64)
    for s0, s1 in zip(cu[:-1], cu[1:]):
        n = s1 - s0
        kk, vv = k[s0:s1].double().repeat_interleave(g, dim=1), v[s0:s1].double().repeat_interleave(g, dim=1)
        sc = torch.einsum("thd,shd->hts", q[s0:s1].double() * scale, kk)
        sc.masked_fill_(torch.triu(torch.ones(n, n, dtype=torch.bool), diagonal=1), float("-inf"))
        out[s0:s1] = torch.einsum("hts,shc->thc", torch.softmax(sc, dim=-1), vv)
    return out


# ---------------------------------------------------------------- rows
def count_rows(n, offsets, width, P, block):
    """[n, len(offsets), width] fp32 indicator rows: position field in channels [0, P), block field in [P, width)"""
    t = torch.arange(n)
    rows = torch.zeros(n, len(offsets), width)
    for i, c in enumerate(offsets):
        rows[t, i, (t + c) % P] = 1.0
        rows[t, i, P + (t // block + c) % (width - P)] = 1.0
    return rows


def count_expected(rows):
    """[n, heads, width] -> [n + 1, heads, width] fp64: entry L is the mean of the first L rows (n_d / n; L = 0: zeros)"""
    n = rows.shape[0]
    out = torch.zeros(n + 1, *rows.shape[1:], dtype=torch.float64)
    out[1:] = rows.double().cumsum(0) / torch.arange(1, n + 1, dtype=torch.float64).view(-1, 1, 1)
    return out


def max_keys_per_position_channel(rows, P):
    return int(rows[..., :P].sum(0).max())


def identity_rows(n, heads, width, seq=0):
    """[n, heads, width] fp32, values 0 .. 15: channels 0-3 the base-16 digits of the token, 4 the head, 5 the sequence, the
    others a mix of the three -- two rows of different (sequence, head, token) differ by >= 1 in some channel"""
    assert n <= 16 ** 4 and heads <= 16 and seq < 16
    t = torch.arange(n).view(n, 1, 1)
    h = torch.arange(heads).view(1, heads, 1)
    c = torch.arange(width).view(1, 1, width)
    v = (t * (2 * c + 1) + 5 * h + 3 * seq + c) % 16
    for d in range(4):
        v[:, :, d] = ((t // 16 ** d) % 16).view(n, 1)
    v[:, :, 4] = h.view(1, heads)
    v[:, :, 5] = seq
    return v.float()


def small_ints(shape, seed):
    """random integers in [-4, 4]: filler that is exact in bf16 and in e4m3 under any power-of-two scale a row of these tests gets"""
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed)).float()


def check_count(got, want):
    """The assertions of construction 1; returns the worst relative error of the non-zero channels."""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    zero = want == 0
    bad = (got != 0) & zero
    assert not bool(bad.any()), f"{int(bad.sum())} channels that no permitted key sets are not 0; first at {bad.nonzero()[0].tolist()}"
    if bool(zero.all()):
        return 0.0
    rel = ((got - want).abs() / want.masked_fill(zero, 1.0)).masked_fill(zero, 0.0)
    worst = float(rel.max())
    assert worst <= REL_COUNT, f"n_d / n missed by {worst:.4f} relative (bar {REL_COUNT}) at {(rel == rel.max()).nonzero()[0].tolist()}"
    return worst


def check_dominant(got, want):
    """The assertion of construction 2; returns the worst absolute error."""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    worst = float(err.max())
    assert worst <= ABS_DOMINANT, f"not the probed key's V row: off by {worst} at {(err == err.max()).nonzero()[0].tolist()}"
    return worst


def check_tied(got, want):
    """Prefill's construction 2 (the permitted keys congruent to the row tie): the bar of construction 1 on the fp64 mean"""
    got, want = got.detach().cpu().double(), want.double()
    err = (got - want).abs()
    over = err - (REL_COUNT * want.abs() + ABS_DOMINANT)
    assert float(over.max()) <= 0, f"off by {float(err.flatten()[over.argmax()])} at {(over == over.max()).nonzero()[0].tolist()}"
    live = want.abs() > ABS_DOMINANT
    return float((err[live] / want.abs()[live]).max())


# ---------------------------------------------------------------- pages
def paginate(rows, page, seed, spare_fill, n_spare=2):
    """Logical rows [n, ...] -> (cache [pages + n_spare, page, ...] with the pages shuffled, table [pages + 1] int32).  Rows past n
    up to the page end and the spare pages hold `spare_fill` everywhere (what a correct kernel never uses); the table's last
    entry names a spare page."""
    n = rows.shape[0]
    pages = max(1, (n + page - 1) // page)
    padded = torch.full((pages * page,) + tuple(rows.shape[1:]), float(spare_fill))
    padded[:n] = rows
    perm = torch.randperm(pages + n_spare, generator=torch.Generator().manual_seed(seed))
    cache = torch.full((pages + n_spare, page) + tuple(rows.shape[1:]), float(spare_fill))
    cache[perm[:pages]] = padded.view(pages, page, *rows.shape[1:])
    return cache.to(torch.bfloat16), perm[: pages + 1].to(torch.int32)


def split_edges(n, block, splits):
    """first token of every split of the decode kernels: block * (n_blocks * s // S), their formula"""
    nb = (n + block - 1) // block
    return sorted({block * (nb * s // S) for S in splits for s in range(1, S)})


def probe_tokens(n, block, page, splits):
    """keys 0 and n - 1, and both sides of every block (step / tile), page and split edge inside [0, n)"""
    edges = set(range(block, n, block)) | set(range(page, n, page)) | set(split_edges(n, block, splits))
    toks = {0, n - 1}
    for e in edges:
        if 0 < e < n:
            toks |= {e - 1, e}
    return sorted(toks)


# ---------------------------------------------------------------- GQA decode
def gqa_count_case(n_max, Hq, Hkv, seed=0, lengths=None, salt=0):
    """Batch row b attends to lengths[b] keys (default: every length 0 .. n_max), all rows over one table.  Returns q [bs, 1, Hq, 128],
    the logical K / V rows [n_max, Hkv, 128] (fp32 values), lens, want [bs, Hq, 128] fp64.  salt: another set of head offsets."""
    lens = torch.arange(n_max + 1) if lengths is None else torch.tensor(lengths)
    V = count_rows(n_max, [7 * h + 3 + 29 * salt for h in range(Hkv)], 128, P_GQA, STEP_GQA)
    K = small_ints((n_max, Hkv, 128), seed)
    want = count_expected(V)[lens].repeat_interleave(Hq // Hkv, dim=1)
    q = torch.zeros(len(lens), 1, Hq, 128, dtype=torch.bfloat16)
    return dict(q=q, K=K, V=V, lens=lens.to(torch.int32), want=want, k_fill=K_AMP, v_fill=1.0)


def gqa_dominant_case(n, Hq, Hkv, probes, seed=0, q_amp=Q_AMP, k_amp=K_AMP, seq=0):
    """Head i of a group in batch row b probes key probes[(b * G + i) % len]; probe p is steered through channel p.  All rows have
    length n.  want [rows, Hq, 128] = the probed keys' V rows."""
    G = Hq // Hkv
    assert len(probes) <= 128
    K = small_ints((n, Hkv, 128), seed)
    K[:, :, : len(probes)] = 0.0
    for i, t in enumerate(probes):
        K[t, :, i] = k_amp
    V = identity_rows(n, Hkv, 128, seq=seq)
    rows = (len(probes) + G - 1) // G
    q = torch.zeros(rows, 1, Hq, 128)
    want = torch.zeros(rows, Hq, 128, dtype=torch.float64)
    for b in range(rows):
        for h in range(Hq):
            i = (b * G + h % G) % len(probes)
            q[b, 0, h, i] = q_amp
            want[b, h] = V[probes[i], h // G].double()
    return dict(q=q.to(torch.bfloat16), K=K, V=V, lens=torch.full((rows,), n, dtype=torch.int32), want=want, k_fill=K_AMP, v_fill=15.0)


def graded_amplitudes(constant_nats, scale, q_amp=8.0):
    """bf16 key amplitudes whose lead q_amp * k * scale is ~4 % under / over `constant_nats`; returns ((k_lo, k_hi), (lead_lo, lead_hi))"""
    ks = [float(torch.tensor(constant_nats * f / (q_amp * scale)).to(torch.bfloat16)) for f in (0.96, 1.04)]
    return ks, [q_amp * k * scale for k in ks]


def gqa_graded_case(n, Hq, Hkv, k_amps, tokens, seed=0, q_amp=8.0):
    """Batch row (token, amplitude) of tokens x k_amps: every head steers to that row's channel; random V.  want: decode64."""
    K = small_ints((n, Hkv, 128), seed)
    combos = [(t, a) for t in tokens for a in k_amps]
    K[:, :, : len(combos)] = 0.0
    q = torch.zeros(len(combos), 1, Hq, 128)
    for i, (t, a) in enumerate(combos):
        K[t, :, i] = a
        q[i, 0, :, i] = q_amp
    V = torch.randn(n, Hkv, 128, generator=torch.Generator().manual_seed(seed + 1)).to(torch.bfloat16).float()
    lens = torch.full((len(combos),), n, dtype=torch.int32)
    want = decode64(q[:, 0], K, V, lens, GQA_SCALE)
    return dict(q=q.to(torch.bfloat16), K=K, V=V, lens=lens, want=want, k_fill=0.0, v_fill=0.0)


def gqa_pages(case, page, seed=0):
    """(k_cache, v_cache [pages, page, Hkv, 128] bf16, table [bs, pages + 1]) of a GQA decode case: both caches in the same shuffle"""
    kc, table = paginate(case["K"], page, seed, case["k_fill"])
    vc, _ = paginate(case["V"], page, seed, case["v_fill"])
    return kc, vc, table.view(1, -1).repeat(case["q"].shape[0], 1).contiguous()


# ---------------------------------------------------------------- MLA decode
def mla_rows(latent, rope):
    return torch.cat([latent, rope], dim=-1)


def mla_count_case(n_max, H, seed=0, lengths=None, salt=0):
    """Batch row b attends to lengths[b] keys (default: 0 .. n_max).  rows [n_max, 576]: latent = the indicator row, rope random
    (it cannot matter at q = 0)"""
    lens = torch.arange(n_max + 1) if lengths is None else torch.tensor(lengths)
    V = count_rows(n_max, [3 + 29 * salt], 512, P_MLA, TILE)[:, 0]
    rope = torch.randn(n_max, 64, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).float()
    want = count_expected(V.unsqueeze(1))[lens].expand(len(lens), H, 512)
    return dict(q_nope=torch.zeros(len(lens), H, 512, dtype=torch.bfloat16), q_pe=torch.zeros(len(lens), H, 64, dtype=torch.bfloat16),
                rows=mla_rows(V, rope), lens=lens.to(torch.int32), want=want, fill=1.0)


def mla_dominant_case(n, H, probes, q_amp=Q_AMP, k_amp=K_AMP, seq=0):
    """Head h of batch row b probes key probes[(b * H + h) % len] through rope channel p; q_nope = 0; latent = identity rows"""
    assert len(probes) <= 64
    latent = identity_rows(n, 1, 512, seq=seq)[:, 0]
    rope = torch.zeros(n, 64)
    for i, t in enumerate(probes):
        rope[t, i] = k_amp
    rows = (len(probes) + H - 1) // H
    q_pe = torch.zeros(rows, H, 64)
    want = torch.zeros(rows, H, 512, dtype=torch.float64)
    for b in range(rows):
        for h in range(H):
            i = (b * H + h) % len(probes)
            q_pe[b, h, i] = q_amp
            want[b, h] = latent[probes[i]].double()
    return dict(q_nope=torch.zeros(rows, H, 512, dtype=torch.bfloat16), q_pe=q_pe.to(torch.bfloat16), rows=mla_rows(latent, rope),
                lens=torch.full((rows,), n, dtype=torch.int32), want=want, fill=K_AMP)


def mla_graded_case(n, H, k_amps, tokens, seed=0, q_amp=8.0):
    combos = [(t, a) for t in tokens for a in k_amps]
    latent = torch.randn(n, 512, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).float()
    rope = torch.zeros(n, 64)
    q_pe = torch.zeros(len(combos), H, 64)
    for i, (t, a) in enumerate(combos):
        rope[t, i] = a
        q_pe[i, :, i] = q_amp
    rows = mla_rows(latent, rope)
    lens = torch.full((len(combos),), n, dtype=torch.int32)
    q_nope = torch.zeros(len(combos), H, 512)
    want = decode64(torch.cat([q_nope, q_pe], -1), rows.unsqueeze(1), latent.unsqueeze(1), lens, MLA_SCALE)
    return dict(q_nope=q_nope.to(torch.bfloat16), q_pe=q_pe.to(torch.bfloat16), rows=rows, lens=lens, want=want, fill=0.0)


def mla_pages(case, page, seed=0):
    """(cache [pages, page, 576] bf16, table [bs, pages + 1])"""
    cache, table = paginate(case["rows"], page, seed, case["fill"])
    return cache, table.view(1, -1).repeat(case["q_nope"].shape[0], 1).contiguous()


def mla_decode64(case):
    """the fp64 oracle on an MLA decode case"""
    q = torch.cat([case["q_nope"].float(), case["q_pe"].float()], -1)
    return decode64(q, case["rows"].unsqueeze(1), case["rows"][:, :512].unsqueeze(1), case["lens"], MLA_SCALE)


BIG_LENGTHS = [17, 130]


def big_gqa_cases(Hq, Hkv, page):
    """the sequences of the beyond-4-GiB tests: counting at 17 and 130 keys, then probes at 17 and 130 keys, each with its own rows"""
    return ([gqa_count_case(n, Hq, Hkv, seed=s, lengths=[n], salt=s + 1) for s, n in enumerate(BIG_LENGTHS)]
            + [gqa_dominant_case(n, Hq, Hkv, probe_tokens(n, STEP_GQA, page, [3]), seed=s, seq=s + 1) for s, n in enumerate(BIG_LENGTHS)])


def big_mla_cases(H, page):
    return ([mla_count_case(n, H, seed=s, lengths=[n], salt=s + 1) for s, n in enumerate(BIG_LENGTHS)]
            + [mla_dominant_case(n, H, probe_tokens(n, TILE, page, [3]), seq=s + 1) for s, n in enumerate(BIG_LENGTHS)])


LONG_N = 33000  # 516 tiles in one split: past mla_decode_tile.h's kMaxTilesLds, the page ids are then read from the table per tile
LONG_PROBES = [0, 63, 64, 16383, 16384, 32767, 32768, 32769, 32999]


# ---------------------------------------------------------------- prefill
def cu_of(seqs):
    cu = [0]
    for n in seqs:
        cu.append(cu[-1] + n)
    return cu


def prefill_count_case(seqs, Hq, Hkv, width, P, seed=0):
    """q = 0; row i of a sequence must be the counting value for i + 1 keys.  GQA: width 128, k random; MLA (Hkv = 1, width 512):
    k = [v | random rope].  Returns q [T, Hq, D], k [T, Hkv, D], v [T, Hkv, width] (fp32 values), cu, want [T, Hq, width]."""
    cu = cu_of(seqs)
    T = cu[-1]
    v = torch.zeros(T, Hkv, width)
    want = torch.zeros(T, Hkv, width, dtype=torch.float64)
    for s, (s0, s1) in enumerate(zip(cu[:-1], cu[1:])):
        v[s0:s1] = count_rows(s1 - s0, [7 * h + 13 * s + 3 for h in range(Hkv)], width, P, TILE)
        want[s0:s1] = count_expected(v[s0:s1])[1:]
    if width == 128:
        k = small_ints((T, Hkv, 128), seed)
    else:
        k = mla_rows(v, torch.randn(T, Hkv, 64, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).float())
    q = torch.zeros(T, Hq, k.shape[-1])
    return dict(q=q, k=k, v=v, cu=cu, want=want.repeat_interleave(Hq // Hkv, dim=1))


def prefill_dominant_case(seqs, Hq, Hkv, width):
    """q row i steers to channel i mod 128 (MLA: rope channel i mod 64), key s has 16 in channel s mod 128 (64): the permitted
    keys congruent to i tie, the diagonal key among them.  want: prefill64 (the mean of the tied keys' identity rows)."""
    cu = cu_of(seqs)
    T = cu[-1]
    mla = width == 512
    D, C, base = (576, 64, 512) if mla else (128, 128, 0)
    q, k, v = torch.zeros(T, Hq, D), torch.zeros(T, Hkv, D), torch.zeros(T, Hkv, width)
    for s, (s0, s1) in enumerate(zip(cu[:-1], cu[1:])):
        i = torch.arange(s1 - s0)
        q[s0 + i, :, base + i % C] = Q_AMP
        k[s0 + i, :, base + i % C] = K_AMP
        v[s0:s1] = identity_rows(s1 - s0, Hkv, width, seq=s)
    if mla:
        k[..., :512] = v
    scale = MLA_SCALE if mla else GQA_SCALE
    return dict(q=q, k=k, v=v, cu=cu, want=prefill64(q, k, v, cu, scale), scale=scale)


def prefill_graded_case(n, Hq, Hkv, width, k_amps, tokens, seed=0, q_amp=8.0):
    """One sequence of n tokens per (token, amplitude) pair of tokens x k_amps: EVERY head and query row of sequence c steers to
    channel c, and only that sequence's key `token` is set there.  The flash kernels decide the rescale by a wave-wide vote and a
    workgroup never spans two sequences, so all rows of a wave sit on the same side of the constant.  Random V.  want: prefill64."""
    mla = width == 512
    D, base = (576, 512) if mla else (128, 0)
    combos = [(t, a) for t in tokens for a in k_amps]
    cu = cu_of([n] * len(combos))
    T = cu[-1]
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(T, Hkv, width, generator=g).to(torch.bfloat16).float()
    k = torch.zeros(T, Hkv, D) if mla else small_ints((T, Hkv, D), seed + 1)
    k[:, :, base : base + len(combos)] = 0.0
    q = torch.zeros(T, Hq, D)
    for c, (t, a) in enumerate(combos):
        k[cu[c] + t, :, base + c] = a
        q[cu[c] : cu[c + 1], :, base + c] = q_amp
    if mla:
        k[..., :512] = v
    scale = MLA_SCALE if mla else GQA_SCALE
    return dict(q=q, k=k, v=v, cu=cu, want=prefill64(q, k, v, cu, scale), scale=scale, combos=combos, base=base)


def margin_nats(q_amp, k_amp, scale):
    return q_amp * k_amp * scale


def leak_bound(n, vmax, margin):
    """what the other n - 1 keys can add to the dominant key's row, absolute"""
    return n * vmax * math.exp(-margin)
