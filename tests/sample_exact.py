"""Exact inputs and expected values for the token sampler of csrc/sample.hip (no GPU needed).

The sampler is a selection: a wrong token leaves the model fluent, so the expectation has to be an equality.  This file holds
everything that equality needs and that can be checked on the CPU (tests/test_sample_exact_host.py); the device comparison
itself is tests/test_gpu_sample_exact.py.

  rows          PROBABILITY space with the row maximum exactly 1.0: then e = p / m = p bit for bit and any float pattern in
                (0, 1] can be placed as a weight.  Weights are 2^-a (fixed point exactly 2^(40-a)), Z and the kept mass S of
                the aimed cases are powers of two or short dyadic sums, so top_p and u are floats whose floor(top_p * Z) and
                floor(u * S) are the intended integers -- the builders assert those integers.
  expectations  oracle/sampling.py::kept_set_fixed_point through tests/spec_verify_ref.py (kept_weights, the inverse CDF and
                verify_row_from); the host test re-derives every draw with sample_fixed_point itself.  Closed forms where one
                exists (an all-equal row with top_k = K and u = (j + 0.5) / K gives token j; u on a cumulative boundary gives
                the token that starts there).
  reach         what each draw is meant to reach -- path (candidate list or radix descent), threshold level, the four clauses
                of `sufficient`, tau and its three 10-bit bins, keep_all, the tie quota, the segment / 256-element chunk / lane
                / quad slot of the drawn token.  cand_trace() and radix_trace() restate the kernel's control flow in numpy with
                those intermediates exposed; the host test holds them to oracle.sampling.sample_candidate_model (None = falls
                back) and sample_radix_model, and every record to the traces, so a case that stops reaching its edge fails on
                the CPU.
  clause 1      `n_kept < n_cand` is never true alone: a cut by top_k inside the list means n_cand > top_k (clause 2) and a cut
                by top_p means s_cand >= excl > p_rem (clause 3).  The records therefore hold all four clauses; "alone" exists
                for clauses 2, 3 and 4 only.
  one less      with the maximum weight 2^40 a float32 top_p cannot express p_rem = excl - 1 (43 significant bits); the
                "dropped" twin of an exact p_rem is the float just below, whose p_rem is 2^18 or 2^19 less (asserted < excl and
                >= the exclusive sum of the tie before).
  logits space  logits on the grid k / 8, |x| <= 16 (exact in fp32, bf16 and fp16): equal logits give bit-equal weights on the
                device and in numpy alike, distinct ones differ by >= 1/16 nat.  The device's __expf may differ from numpy's
                exp by a relative 2^-17 (argument rounding |x - m| * 2^-24 <= 2^-19, the instruction ~2^-23); a draw is
                admitted only with a margin of 2^-12 (32 times that) around every decision: every exclusive prefix sum at
                least 2^-12 * Z from top_p * Z, u * S at least 2^-12 * S from every kept cumulative boundary.  Each admitted
                case keeps a probability-space twin (the oracle's weights passed as probabilities).
  special       -inf / +inf / NaN of either sign / fp16 subnormals and +-65504, as bit patterns of each storage type.
"""

import dataclasses
import functools

import numpy as np

from oracle import sampling as osmp
from tests import spec_verify_ref as sv

F32 = np.float32
ONE_BELOW = float(np.nextafter(F32(1), F32(0)))  # the largest float32 below 1
FIX = 40
CAP = 1024
WAVES = 16
TKEYS = [(127 - 4 * (j + 1)) << 23 for j in range(5)]  # bits of 2^-4 .. 2^-20
MUST = (0, 3, 4, 255, 256, 1023, 1024, 4095, 4096)
MARGIN = 2.0 ** -12
U64_MAX = (1 << 64) - 1


def p2(a):
    return F32(2.0 ** -a)


def from_key(k):
    return np.array([k], dtype=np.uint32).view(F32)[0]


def key_of(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def spread(n, vocab, seed=0):
    """n distinct indices: the fixed edge indices first (0, 3, 4, 255, 256, 1023, 1024, 4095, 4096, vocab - 1), then one index in
    every wave of a row pass ((i // 256) % 16, vocabularies >= 4096), the rest from a seeded permutation."""
    must = [i for i in MUST if i < vocab - 1] + [vocab - 1]
    if vocab >= 4096:
        must += [256 * w + 16 * w + 9 for w in range(WAVES)]  # one per wave of a row pass
    perm = np.random.default_rng(seed).permutation(vocab).tolist()
    out = np.array(list(dict.fromkeys(must + perm))[:n], dtype=np.int64)
    if n >= 64 and vocab >= 4096:
        assert len(set(((out // 256) % WAVES).tolist())) == WAVES
    return out


def seg_len_of(vocab):
    return ((vocab + WAVES - 1) // WAVES + 255) // 256 * 256


def weights(row):
    """(keys int64: the float patterns of e = p / max, fix int64: floor(e * 2^40)) of a probability row"""
    _, e, fix = osmp._weights_fixed(row, 1.0, True)
    return e.view(np.uint32).astype(np.int64), fix.astype(np.int64)


def p_rem_of(top_p, z):
    """floor(top_p * Z) as the kernel and the oracle form it; None = no limit (top_p >= 1)"""
    if top_p >= 1.0:
        return None
    return int(np.floor(np.float64(max(F32(top_p), F32(0))) * np.float64(z)))


def top_p_exact(target, z):
    """the float32 top_p with floor(top_p * z) == target exactly (asserted)"""
    p = F32(target / z)
    assert p_rem_of(float(p), z) == target, (target, z)
    return float(p)


def top_p_between(lo, hi, z):
    """a float32 top_p with lo <= floor(top_p * z) < hi (asserted)"""
    p = F32((lo + hi) / 2 / z)
    assert lo <= p_rem_of(float(p), z) < hi, (lo, hi, z)
    return float(p)


def u_edges(excl, w, s):
    """(the smallest u whose target is >= excl, the largest u whose target is < excl + w): both ends of a token's CDF interval"""
    lo = sv.u_around(excl, s)[1] if excl > 0 else 0.0
    hi = sv.u_around(excl + w, s)[0]
    assert lo is not None and hi is not None and excl <= sv.target(lo, s) and sv.target(hi, s) < excl + w
    return lo, hi


# ---------------------------------------------------------------- the kernel's control flow, intermediates exposed
def cand_trace(row, top_k, top_p, cap=CAP):
    """sample_candidates of csrc/sample.hip up to the sufficiency rule: path, level, n_cand, n_kept, the four clauses"""
    keys, fix = weights(row)
    vocab, z = keys.size, int(fix.sum())
    counts = [int((keys >= t).sum()) for t in TKEYS]
    if top_k == 1:
        return dict(path="greedy")
    if z == 0 or counts[0] > cap:
        return dict(path="radix", level=None, clauses=None, over_cap=counts[0] > cap, counts=counts)
    level = max(j for j in range(5) if counts[j] <= cap)
    cand = np.nonzero(keys >= TKEYS[level])[0]
    cand = cand[np.lexsort((cand, -keys[cand]))]
    w = fix[cand]
    excl = np.cumsum(w) - w
    pr = p_rem_of(top_p, z)
    p_rem = U64_MAX if pr is None else pr
    k_eff = (1 << 32) - 1 if top_k <= 0 else int(top_k)
    kept = (np.arange(cand.size) < k_eff) & np.array([int(x) <= p_rem for x in excl], dtype=bool)
    n_cand, n_kept, s_cand = int(cand.size), int(kept.sum()), int(w.sum())
    clauses = (n_kept < n_cand, n_cand >= k_eff, s_cand > p_rem, n_cand == vocab)
    return dict(path="list" if any(clauses) else "radix", level=level, n_cand=n_cand, n_kept_list=n_kept, clauses=clauses,
                over_cap=False, counts=counts)


def radix_trace(row, top_k, top_p, u):
    """sample_radix_cut + the segment pass + the rescan: tau (the three levels' bins are its 10-bit fields), the tie quota, the
    segment, chunk, lane and quad slot of the drawn token"""
    keys, fix = weights(row)
    vocab, z = keys.size, int(fix.sum())
    if top_k == 1:
        return dict(path="greedy", token=osmp._argmax(row), n_kept=1)
    k_rem = (1 << 32) - 1 if top_k <= 0 else int(top_k)
    pr = p_rem_of(top_p, z)
    p_rem = U64_MAX if pr is None else pr
    uk, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    sums = np.zeros(uk.size, dtype=np.int64)
    np.add.at(sums, inv, fix)
    uk, cnt, sums = uk[::-1], cnt[::-1], sums[::-1]  # from the largest weight down, as the boundary walk
    c_incl, s_incl = np.cumsum(cnt), np.cumsum(sums)
    cond = (c_incl >= k_rem) | np.array([int(s) > p_rem for s in s_incl], dtype=bool)
    if not cond.any():
        keep_all, tau, e_tau, c_keep, c_above, s_kept, n_kept = True, 0, 0, (1 << 32) - 1, 0, z, vocab
    else:
        b = int(np.argmax(cond))
        keep_all, tau = False, int(uk[b])
        c_above, s_above = int(c_incl[b] - cnt[b]), int(s_incl[b] - sums[b])
        k_rem, p_rem = k_rem - c_above, p_rem - s_above
        e_tau = int(sums[b]) // int(cnt[b])
        c_p = min(p_rem // e_tau + 1, int(cnt[b])) if e_tau else int(cnt[b])
        c_keep = min(c_p, k_rem)
        s_kept, n_kept = s_above + c_keep * e_tau, c_above + c_keep
    out = dict(keep_all=keep_all, tau=tau, bins=(tau >> 20, (tau >> 10) & 1023, tau & 1023), c_keep=c_keep, e_tau=e_tau,
               n_kept=n_kept, s_kept=s_kept, z=z)
    if s_kept == 0:
        out.update(token=osmp._argmax(row), seg=None)
        return out
    target = sv.target(u, s_kept)
    tie = keys == tau
    rank = np.cumsum(tie) - tie
    wts = np.where(keys > tau, fix, 0)
    wts[tie & (rank < c_keep)] = e_tau
    tok = int(np.searchsorted(np.cumsum(wts), target, side="right"))
    seg_len = seg_len_of(vocab)
    seg = tok // seg_len
    within = tok - seg * seg_len
    out.update(token=tok, seg=seg, chunk=within // 256, lane=(within % 256) // 4, slot=tok % 4,
               ties_before_seg=int(tie[: seg * seg_len].sum()))
    return out


# ---------------------------------------------------------------- probability-space cases
@dataclasses.dataclass
class Case:
    """One probability row and its draws (top_k, top_p, u): a launch of len(draws) equal rows.  reach[i]: the record of draw i
    (keys of cand_trace / radix_trace); closed[i]: the closed-form (token, n_kept), entries or the whole list None."""
    name: str
    row: np.ndarray
    draws: list
    reach: list
    closed: list = None

    def __post_init__(self):
        self.row = np.ascontiguousarray(self.row, dtype=F32)
        assert float(self.row.max()) == 1.0 and float(self.row.min()) >= 0.0, self.name
        assert len(self.reach) == len(self.draws) and (self.closed is None or len(self.closed) == len(self.draws))
        self._kw = {}

    def kw(self, top_k, top_p):
        """spec_verify_ref.kept_weights of the row under (top_k, top_p), plus n_kept and Z"""
        key = (int(top_k), float(top_p))
        if key not in self._kw:
            kw = sv.kept_weights(self.row, 1.0, key[0], key[1], True)
            kw["z"] = int(weights(self.row)[1].sum())
            kw["n"] = 1 if kw["w"] is None else int(kw["mask"].sum())
            self._kw[key] = kw
        return self._kw[key]

    def expected(self):
        """[(token, n_kept, s_kept, z)] per draw"""
        out = []
        for k, p, u in self.draws:
            kw = self.kw(k, p)
            out.append((sv.verify_row_from(kw, -1, 0.0, u)[1], kw["n"], kw["S"], kw["z"]))
        return out


def u_for(case, top_k, top_p, token):
    """the uniform at the middle of `token`'s CDF interval under (top_k, top_p) (asserted to draw it)"""
    kw = case.kw(top_k, top_p)
    w = kw["w"].astype(np.int64)
    assert w[token] > 0, (case.name, token)
    excl = int(w[:token].sum())
    u = float(F32((excl + int(w[token]) / 2) / kw["S"]))
    assert sv.verify_row_from(kw, -1, 0.0, u)[1] == token
    return u


def _filled(vocab, fill):
    return np.full(vocab, fill, dtype=F32)


def a1_capacity():
    """N - 1 elements at (or one ulp below) the first threshold 2^-4, one at 1.0, the rest at 2^-30: counts[0] = N or 1"""
    cases = []
    for tag, v in (("at", p2(4)), ("below", from_key(0x3D7FFFFF))):
        for n in (1023, 1024, 1025):
            row = _filled(4099, p2(30))
            idx = spread(n, 4099, seed=n)
            row[idx] = v
            row[idx[n // 2]] = 1.0
            draws, reach = [], []
            for k, p in ((10, 1.0), (1024, 1.0), (1025, 1.0), (-1, 0.5)):
                for u in (0.3, ONE_BELOW):
                    draws.append((k, p, u))
                    if tag == "at":  # counts[0] = N: the list holds N entries at level 4 iff N <= 1024
                        path = "radix" if n == 1025 else ("list" if (k == 10 or p < 1 or k <= n) else "radix")
                        reach.append(dict(path=path, over_cap=n == 1025, **({} if n == 1025 else dict(level=4, n_cand=n))))
                    else:  # counts[0] = 1, every lower threshold counts N: level 4 with N entries, or level 0 with one
                        if n == 1025:
                            reach.append(dict(path="radix", level=0, n_cand=1, over_cap=False, clauses=(False,) * 4))
                        else:
                            reach.append(dict(path="list" if (k == 10 or p < 1 or k <= n) else "radix", level=4, n_cand=n))
            cases.append(Case(f"A1-{tag}-{n}", row, draws, reach))
    return cases


def a2_levels():
    """level j chosen: 1024 elements reach 2^-(4j+4) (one of them the 1.0), a 1025th reaches only the next threshold"""
    cases = []
    for j in range(5):
        row = _filled(4099, p2(30))
        idx = spread(1025, 4099, seed=20 + j)
        row[idx[:1024]] = p2(4 * j + 4)
        row[idx[7]] = 1.0
        if j < 4:
            row[idx[1024]] = p2(4 * j + 8)
        draws = [(500, 1.0, 0.3), (500, 1.0, ONE_BELOW), (-1, 0.5, 0.3), (-1, 0.5, 0.0)]
        reach = [dict(path="list", level=j, n_cand=1024, clauses=(True, True, False, False)),
                 dict(path="list", level=j, n_cand=1024, clauses=(True, True, False, False)),
                 dict(path="list", level=j, n_cand=1024, clauses=(True, False, True, False)),
                 dict(path="list", level=j, n_cand=1024, clauses=(True, False, True, False))]
        closed = [(None, 500), (None, 500), None, None]
        cases.append(Case(f"A2-level{j}", row, draws, reach, closed))
    return cases


def a3_clauses():
    """each clause of `sufficient` alone (2, 3, 4), clause 1 with 2 / with 3, and all four false: the fall-back's kept set then
    reaches below the threshold"""
    row = _filled(4099, p2(30))
    idx = spread(64, 4099, seed=31)
    row[idx] = p2(2)
    row[idx[5]] = 1.0
    keys, fix = weights(row)
    z, s_cand = int(fix.sum()), (1 << 40) + 63 * (1 << 38)
    p_mass = top_p_between(s_cand - (1 << 38), s_cand, z)  # the last candidate kept, the list's mass above p_rem
    p_none = ONE_BELOW  # Z * 2^-24 is a quarter of the mass below the threshold: the cut falls among the 2^-30 tokens
    assert s_cand < p_rem_of(p_none, z) < z - (1 << 10)
    draws = [(64, 1.0, 0.4), (-1, p_mass, 0.4), (65, 1.0, ONE_BELOW), (-1, p_none, ONE_BELOW), (-1, 1.0, 0.4), (30, 1.0, 0.4),
             (-1, 0.5, 0.4)]
    reach = [dict(path="list", level=4, n_cand=64, clauses=(False, True, False, False)),
             dict(path="list", level=4, n_cand=64, clauses=(False, False, True, False)),
             dict(path="radix", level=4, n_cand=64, clauses=(False, False, False, False)),
             dict(path="radix", level=4, n_cand=64, clauses=(False, False, False, False)),
             dict(path="radix", level=4, n_cand=64, clauses=(False, False, False, False), keep_all=True),
             dict(path="list", level=4, n_cand=64, clauses=(True, True, False, False)),
             dict(path="list", level=4, n_cand=64, clauses=(True, False, True, False))]
    closed = [(None, 64), (None, 64), (None, 65), None, (None, 4099), (None, 30), None]
    cases = [Case("A3-4099", row, draws, reach, closed)]
    assert cases[0].kw(65, 1.0)["mask"][fix == (1 << 10)].sum() == 1  # a token below every threshold is in the kept set
    assert cases[0].kw(-1, p_none)["n"] > 64
    for vocab in (5, 64, 65):  # the list is the whole row: clause 4 alone
        r = np.array([p2(i % 7) for i in range(vocab)], dtype=F32)
        r[vocab // 2] = 1.0
        r[0] = p2(3)
        draws = [(-1, 1.0, 0.0), (-1, 1.0, 0.6), (-1, 1.0, ONE_BELOW), (vocab + 1, 1.5, 0.6)]
        reach = [dict(path="list", n_cand=vocab, clauses=(False, False, False, True))] * 4
        cases.append(Case(f"A3-whole-{vocab}", r, draws, reach, [(None, vocab)] * 4))
    return cases


def a4_lengths():
    """list lengths around the bitonic sort's power-of-two padding (npow = 64 .. 1024 and its zero entries)"""
    cases = []
    for n in (1, 2, 63, 64, 65, 128, 129, 1024):
        row = _filled(4099, p2(30))
        idx = spread(n, 4099, seed=40 + n)
        row[idx] = p2(2)
        row[idx[n // 2]] = 1.0
        draws, reach, closed = [], [], []
        for u in (0.0, 0.37, ONE_BELOW):
            if n > 1:
                draws.append((n, 1.0, u))
                reach.append(dict(path="list", level=4, n_cand=n, clauses=(False, True, False, False)))
                closed.append((None, n))
            draws.append((-1, 0.5, u))
            reach.append(dict(path="list", level=4, n_cand=n, clauses=(n > 1, False, True, False)))
            closed.append(None)
        cases.append(Case(f"A4-len{n}", row, draws, reach, closed))
    return cases


def a5_ties_across_cut():
    """40 ties at 2^-3 over all waves, four 2^-1 and the 1.0 in front of them, everything else 0: Z = 2^43 exactly.  top_k ends
    the prefix after the 1st / 7th / 40th tie; top_p with p_rem exactly the exclusive sum in front of tie j (kept) and the
    float below (dropped).  The kept ties are the lowest indices."""
    row = _filled(4099, 0.0)
    idx = spread(45, 4099, seed=5)
    ties = np.sort(idx[:40])
    row[ties] = p2(3)
    row[idx[40:44]] = p2(1)
    row[idx[44]] = 1.0
    keys, fix = weights(row)
    z = int(fix.sum())
    assert z == 1 << 43
    case = Case("A5-ties", row, [(2, 1.0, 0.0)], [dict()])
    draws, reach, closed = [], [], []

    def add(k, p, n_ties):
        kw = case.kw(k, p)
        assert kw["n"] == 5 + n_ties and np.array_equal(np.nonzero(kw["mask"] & (fix == 1 << 37))[0], ties[:n_ties])
        us = [ONE_BELOW, 0.0] + ([u_for(case, k, p, int(ties[n_ties - 1]))] if n_ties else [])
        for u in us:
            draws.append((k, p, u))
            reach.append(dict(path="list", level=4, n_cand=45, tau=key_of(p2(3)) if n_ties else None, c_keep=n_ties if n_ties else None))
            closed.append((None, 5 + n_ties))

    for n_ties in (1, 7, 40):
        add(5 + n_ties, 1.0, n_ties)
    for j in (0, 6, 39):
        excl = 3 * (1 << 40) + j * (1 << 37)  # the 1.0, four 2^-1 and j ties in front of tie j
        p = top_p_exact(excl, z)
        add(-1, p, j + 1)
        below = float(np.nextafter(F32(p), F32(0)))
        pr = p_rem_of(below, z)
        assert excl - (1 << 37) <= pr < excl and excl - pr in (1 << 18, 1 << 19)
        add(-1, below, j)
    for r in reach:  # no tie kept: the descent stops at the 2^-1 tokens, another tau
        for f in ("tau", "c_keep"):
            if r[f] is None:
                del r[f]
    case.draws, case.reach, case.closed = draws, reach, closed
    return [case]


def a6_draw_edges():
    """five kept dyadic weights in an index order that is not the weight order, S = 2^41: u exactly on each cumulative boundary
    and the float just below it; u = 0, the largest float below 1, and the clamps 1.0, 2.0, -1.0"""
    row = _filled(4099, p2(30))
    idx = [3, 256, 1024, 4095, 4098]
    for i, a in zip(idx, (3, 0, 2, 3, 1)):
        row[i] = p2(a)
    case = Case("A6-edges", row, [(5, 1.0, 0.0)], [dict()])
    kw = case.kw(5, 1.0)
    assert kw["S"] == 1 << 41
    cum = np.cumsum(kw["w"].astype(np.int64)[idx])
    draws, closed = [], []
    for i in range(4):
        u = float(F32(int(cum[i]) / (1 << 41)))
        assert sv.target(u, 1 << 41) == int(cum[i])
        below = float(np.nextafter(F32(u), F32(0)))
        assert sv.target(below, 1 << 41) < int(cum[i])
        draws += [(5, 1.0, u), (5, 1.0, below)]
        closed += [(idx[i + 1], 5), (idx[i], 5)]
    for u, tok in ((0.0, idx[0]), (ONE_BELOW, idx[4]), (1.0, idx[4]), (2.0, idx[4]), (-1.0, idx[0])):
        draws.append((5, 1.0, u))
        closed.append((tok, 5))
    case.draws, case.closed = draws, closed
    case.reach = [dict(path="list", level=4, n_cand=5, clauses=(False, True, False, False))] * len(draws)
    return [case]


def b1_resolution():
    """pairs of weights whose patterns differ only in bits 0-9, 10-19, 20-29, and the pair ...3ff / ...400 (the last bin of one
    level-3 histogram, the first of the next), each separated once by top_k and once by top_p.  1100 elements at 2^-3: the list
    declines (counts[0] > 1024)."""
    base = 0x3E800000  # 0.25
    pairs = {"bits0-9": (base | 0x2AA, base | 0x155), "bits10-19": (base | (0x2AA << 10), base | (0x155 << 10)),
             "bits20-29": (0x3E800000, 0x3E700000), "3ff-400": (0x3E900400, 0x3E9003FF)}
    row = _filled(4099, p2(30))
    idx = spread(1109, 4099, seed=61)
    row[idx[:1100]] = p2(3)
    row[idx[1100]] = 1.0
    where = {}
    for n, (name, (hi, lo)) in enumerate(pairs.items()):
        a, b = sorted((int(idx[1101 + 2 * n]), int(idx[1102 + 2 * n])))
        row[b], row[a] = from_key(hi), from_key(lo)  # the larger weight at the HIGHER index: the order is by key, not by index
        where[name] = (b, a)
    keys, fix = weights(row)
    z = int(fix.sum())
    order = np.argsort(-keys, kind="stable")
    excl = np.cumsum(fix[order]) - fix[order]
    pos = {int(t): n for n, t in enumerate(order)}
    draws, reach, closed = [], [], []
    case = Case("B1-resolution", row, [(2, 1.0, 0.0)], [dict()])
    for name, (hi, lo) in pairs.items():
        i_hi, i_lo = where[name]
        assert pos[i_lo] == pos[i_hi] + 1
        k = pos[i_hi] + 1
        p = top_p_between(int(excl[pos[i_hi]]), int(excl[pos[i_lo]]), z)
        for kk, pp in ((k, 1.0), (-1, p)):
            kw = case.kw(kk, pp)
            assert kw["mask"][i_hi] and not kw["mask"][i_lo]
            for u in (u_for(case, kk, pp, i_hi), ONE_BELOW):
                draws.append((kk, pp, u))
                reach.append(dict(path="radix", over_cap=True, tau=hi, bins=(hi >> 20, (hi >> 10) & 1023, hi & 1023), c_keep=1))
                closed.append((None, k))
    case.draws, case.reach, case.closed = draws, reach, closed
    return [case]


def _b2_js(k, seg_len):
    """tie ranks worth drawing: both sides of every 256-element chunk edge (every segment edge is one), and the four quad slots
    of lanes 0 and 63 in the first chunk and in the chunk of the last kept tie"""
    js = set()
    for c in range(0, k + 256, 256):
        js.update((c - 1, c))
    for c in (0, (k - 1) // 256 * 256):
        js.update(range(c, c + 4))
        js.update(range(c + 252, c + 256))
    js.update((k - 1, k - 2, seg_len - 1, seg_len))
    return sorted(j for j in js if 0 <= j < k)


def b2_all_equal():
    """all-equal rows: top_k = K keeps the K lowest indices, u = (j + 0.5) / K draws token j"""
    cases = []
    for vocab in (256, 257, 4096, 4097, 8191):
        sl = seg_len_of(vocab)
        assert sl == {256: 256, 257: 256, 4096: 256, 4097: 512, 8191: 512}[vocab]
        row = _filled(vocab, 1.0)
        draws, reach, closed = [], [], []
        for last in (sl - 1, sl, sl + 1, 2 * sl, vocab - 1):
            k = last + 1
            if k > vocab or k == 1 or any(d[0] == k for d in draws):
                continue
            for j in _b2_js(k, sl):
                draws.append((k, 1.0, float(F32((j + 0.5) / k))))
                within = j - j // sl * sl
                reach.append(dict(path="list" if vocab <= CAP else "radix", tau=0x3F800000, c_keep=k, seg=j // sl, chunk=within // 256,
                                  lane=(within % 256) // 4, slot=j % 4, ties_before_seg=j // sl * sl))
                closed.append((j, k))
        cases.append(Case(f"B2-equal-{vocab}", row, draws, reach, closed))
    return cases


def _strict_positions(vocab):
    sl = seg_len_of(vocab)
    out = []
    for lo in range(0, vocab, sl):
        hi = min(lo + sl, vocab)
        out.append(sorted({lo, (lo + hi) // 2, hi - 1}))
    return sl, out


def b3_interleaved(vocab=4099, name="B3-interleaved"):
    """ties at 2^-2 everywhere, a 1.0 at the first, middle and last index of every segment; top_k lets the tie quota run out
    right before the middle token of segment 3 (a chunk edge).  Draws at the middle and at both ends of the CDF interval of:
    the last kept tie, the strict token right after it, the strict token at seg_end - 1, every strict token of every later
    segment (whose ties weigh nothing)."""
    sl, strict = _strict_positions(vocab)
    row = _filled(vocab, p2(2))
    flat = [i for s in strict for i in s]
    row[flat] = 1.0
    mid3 = strict[3][1]
    last_tie = mid3 - 1
    assert last_tie not in flat and (vocab != 4099 or (mid3 - 3 * sl) % 256 == 0)  # 4099: the quota ends at a chunk edge
    q = last_tie + 1 - sum(1 for i in flat if i <= last_tie)
    k = len(flat) + q
    case = Case(name, row, [(k, 1.0, 0.0)], [dict()])
    kw = case.kw(k, 1.0)
    w = kw["w"].astype(np.int64)
    assert kw["mask"][last_tie] and not kw["mask"][last_tie + 2] and w[last_tie + 2] == 0 and kw["n"] == k
    later = strict[4:] if vocab < 8192 else [strict[4], strict[-2], strict[-1]]
    aims = [last_tie, mid3, strict[3][2]] + [i for s in later for i in s]
    draws, reach, closed = [], [], []
    for t in aims:
        excl = int(w[:t].sum())
        for u in (u_for(case, k, 1.0, t),) + u_edges(excl, int(w[t]), kw["S"]):
            draws.append((k, 1.0, u))
            reach.append(dict(path="radix", over_cap=True, tau=key_of(p2(2)), c_keep=q, seg=t // sl, chunk=(t % sl) // 256))
            closed.append((t, k))
    for u, t in ((0.0, 0), (ONE_BELOW, flat[-1])):
        draws.append((k, 1.0, u))
        reach.append(dict(path="radix", seg=t // sl))
        closed.append((t, k))
    case.draws, case.reach, case.closed = draws, reach, closed
    return [case]


def b4_keep_all():
    """every spelling of "keep all": top_k in {-1, 0, vocab - 1, vocab, vocab + 1} x top_p in {largest float below 1, 1.0, 1.5}"""
    vocab = 4099
    row = np.array([p2((i * 7) % 12) for i in range(vocab)], dtype=F32)
    draws, reach, closed = [], [], []
    for k in (-1, 0, vocab - 1, vocab, vocab + 1):
        for p in (ONE_BELOW, 1.0, 1.5):
            for u in (0.41, ONE_BELOW):
                draws.append((k, p, u))
                unlimited = p >= 1 and k != vocab - 1
                reach.append(dict(path="radix", over_cap=True, keep_all=p >= 1 and k in (-1, 0, vocab + 1)))
                closed.append((None, vocab if unlimited else (vocab - 1 if p >= 1 else None)))
    return [Case("B4-keep-all", row, draws, reach, closed)]


def b5_zero_weights():
    """weights 2^-41 (positive key, fixed point 0) and 0.0: top_k reaches into them, they count in n_kept and are never drawn"""
    vocab = 4099
    row = _filled(vocab, 0.0)
    idx = spread(1251, vocab, seed=71)
    tiny = np.sort(idx[:50])  # index 0 and vocab - 1 among them
    row[idx[50:1250]] = p2(2)
    row[tiny] = p2(41)
    row[idx[1250]] = 1.0
    keys, fix = weights(row)
    assert (fix[tiny] == 0).all() and (keys[tiny] > 0).all() and tiny[0] == 0 and tiny[-1] == vocab - 1
    positive = np.nonzero(fix > 0)[0]
    draws, reach, closed = [], [], []
    for k, tau, c_keep in ((1201 + 20, key_of(p2(41)), 20), (1201 + 50 + 10, 0, 10), (1201 + 50, key_of(p2(41)), 50)):
        for u, t in ((0.0, int(positive[0])), (ONE_BELOW, int(positive[-1])), (1.0, int(positive[-1]))):
            draws.append((k, 1.0, u))
            reach.append(dict(path="radix", over_cap=True, tau=tau, c_keep=c_keep, e_tau=0))
            closed.append((t, k))
    return [Case("B5-zero-weights", row, draws, reach, closed)]


def b6_second_trip():
    """vocab 32773: the second trip of a row pass's outer loop (elements past 32768), a ragged tail of one element, an odd row
    stride.  B3's pattern, and a peaked row whose kept tokens include the ragged tail."""
    vocab = 32773
    cases = b3_interleaved(vocab, "B6-interleaved-32773")
    row = _filled(vocab, p2(30))
    idx = [0, 3, 255, 256, 4095, 4096, 16383, 16384, 32767, 32768, 32769, 32771, 32772]
    for n, i in enumerate(idx):
        row[i] = p2(1 + n % 6)
    row[32770] = 1.0
    case = Case("B6-peaked-32773", row, [(2, 1.0, 0.0)], [dict()])
    draws, reach, closed = [], [], []
    for k, p in ((14, 1.0), (9, 1.0), (-1, 0.9), (20, 1.0)):
        kw = case.kw(k, p)
        toks = np.nonzero(kw["w"])[0]
        for t in (int(toks[0]), int(toks[-1]), 32768 if kw["w"][32768] else int(toks[len(toks) // 2])):
            draws.append((k, p, u_for(case, k, p, t)))
            reach.append(dict(path="radix" if k == 20 else "list", level=4, n_cand=14))
            closed.append((t, None))
    case.draws, case.reach, case.closed = draws, reach, closed
    return cases + [case]


GROUPS = {"A1": a1_capacity, "A2": a2_levels, "A3": a3_clauses, "A4": a4_lengths, "A5": a5_ties_across_cut, "A6": a6_draw_edges,
          "B1": b1_resolution, "B2": b2_all_equal, "B3": b3_interleaved, "B4": b4_keep_all, "B5": b5_zero_weights,
          "B6": b6_second_trip}
VERIFY_GROUPS = ("A5", "B2", "B3")


@functools.lru_cache(maxsize=None)
def group(name):
    return GROUPS[name]()


# ---------------------------------------------------------------- C. verification rows
def verify_rows(case):
    """(top_ks, top_ps, drafts, uniforms [rows, 2], expected accepted, expected tokens, expected out) of the case as T = 2 sequences
    of chitu_hip_speculative_verify: row 0 carries a draft -- the last kept tie, the first dropped tie, a strict token, a token
    outside the kept set, a kept token a third of the way through the kept set -- with u_acc on both sides of w_d / S, row 1 is
    the bonus row (draft -1), which is the sampler's row."""
    keys, fix = weights(case.row)
    sl = seg_len_of(case.row.size)
    by_param = {}
    for k, p, u in case.draws:
        by_param.setdefault((k, p), []).append(u)
    drafted = []
    for (k, p), us in by_param.items():
        kw = case.kw(k, p)
        if kw["w"] is None:
            continue
        mask = kw["mask"]
        kept = np.nonzero(mask)[0]
        tau_w = fix[kept].min()
        picks = [int(kept[fix[kept] == tau_w].max())]
        dropped = np.nonzero(~mask & (fix == tau_w))[0]
        if dropped.size:
            picks.append(int(dropped.min()))
        strict = kept[fix[kept] > tau_w]
        if strict.size:
            picks.append(int(strict.max()))
        outside = np.nonzero(~mask & (fix != tau_w))[0]
        if outside.size:
            picks.append(int(outside[-1]))
        picks.append(int(kept[kept.size // 3]))
        n = 0
        for d in dict.fromkeys(picks):
            w_d = int(kw["w"][d])
            for ua in sv.u_around(w_d, kw["S"]):
                if ua is not None:
                    drafted.append((k, p, d, ua, us[n % len(us)]))
                    n += 1
            reject = sv.u_around(w_d, kw["S"])[1]
            if not w_d or reject is None:
                continue
            # a kept draft just rejected: the replacement is drawn from K without d -- aim it at both ends of the CDF interval
            # of d's kept neighbours and of the last kept token of d's segment (everything behind d moves up by w_d)
            w2 = kw["w"].astype(np.int64)
            w2[d] = 0
            nz = np.nonzero(w2)[0]
            after, before = nz[nz > d], nz[nz < d]
            in_seg = after[after < (d // sl + 1) * sl]
            for t in dict.fromkeys([int(a) for a in (after[:1].tolist() + in_seg[-1:].tolist() + before[-1:].tolist())]):
                for u_alt in u_edges(int(w2[:t].sum()), int(w2[t]), kw["S"] - w_d):
                    assert sv.verify_row_from(kw, d, reject, u_alt) == (False, t)
                    drafted.append((k, p, d, reject, u_alt))
    bonus = [(k, p, -1, 0.5, u) for k, p, u in case.draws if k != 1]
    rows = []
    for i in range(max(len(drafted), len(bonus))):
        rows += [drafted[i % len(drafted)], bonus[i % len(bonus)]]
    want = [sv.verify_row_from(case.kw(k, p), d, ua, u) for k, p, d, ua, u in rows]
    acc, tok = [int(a) for a, _ in want], [int(t) for _, t in want]
    return dict(top_ks=[r[0] for r in rows], top_ps=[r[1] for r in rows], drafts=[r[2] for r in rows],
                uniforms=[(r[3], r[4]) for r in rows], accepted=acc, tokens=tok, out=sv.sequences(acc, tok, 2),
                bonus_want=[sv.verify_row_from(case.kw(k, p), -1, 0.0, u)[1] for k, p, d, ua, u in rows[1::2]])


# ---------------------------------------------------------------- D. logits space
TEMPERATURES = (0.5, 0.7, 1.0, 1.3, 2.0)
LOGIT_VOCABS = (5, 257, 4099, 32773)


def logits_decisions(x, temperature, top_k, top_p):
    """(the smallest |excl - top_p * Z| / Z over every exclusive prefix sum of the descending order (inf for top_p >= 1), the kept
    cumulative boundaries in index order with 0 and S, S)"""
    _, e, fix = osmp._weights_fixed(x, temperature, False)
    keys, fix = e.view(np.uint32).astype(np.int64), fix.astype(np.int64)
    order = np.argsort(-keys, kind="stable")
    z = int(fix.sum())
    cut = np.inf
    if top_p < 1.0:
        excl = (np.cumsum(fix[order]) - fix[order]).astype(np.float64)
        cut = float(np.abs(excl - np.float64(F32(top_p)) * np.float64(z)).min() / z)
    mask, n, _, _ = osmp.kept_set_fixed_point(x, temperature, top_k, top_p)
    w = np.where(mask, fix, 0)
    s = int(w.sum())
    return cut, np.concatenate([[0], np.cumsum(w[mask])]).astype(np.float64), s


def logits_margins(x, temperature, top_k, top_p, u, decisions=None):
    """(the cut margin above, the smallest |u * S - c| / S over every kept cumulative boundary c)"""
    cut, bounds, s = decisions or logits_decisions(x, temperature, top_k, top_p)
    return cut, float(np.abs(bounds - np.float64(F32(u)) * np.float64(s)).min() / s)


@dataclasses.dataclass
class LogitsCase:
    """One row of grid logits (float32 values exact in bf16 and fp16), a temperature, its admitted draws (top_k, top_p, u) and
    their expected (token, n_kept)."""
    name: str
    x: np.ndarray
    temperature: float
    draws: list
    expected: list
    tried: int

    def twin(self):
        """the oracle's weights as a probability row: what the kernel must see in probs_mode to give the same answers"""
        return osmp._weights_fixed(self.x, self.temperature, False)[1]


@functools.lru_cache(maxsize=None)
def logits_cases():
    cases = []
    for vocab in LOGIT_VOCABS:
        for n, t in enumerate(TEMPERATURES):
            rng = np.random.default_rng(1000 * vocab + n)
            sigma = (3.0, 1.0, 5.0, 2.0, 0.25)[n]  # peaked, rounded to many ties, wide (fixed point 0 in the tail), flat
            x = np.clip(np.round(rng.normal(0, sigma, vocab) * 8) / 8, -16, 16).astype(F32)
            x[int(rng.integers(vocab))] = min(16.0, float(x.max()) + 0.5)
            assert np.array_equal(x * 8, np.round(x * 8)) and float(np.abs(x).max()) <= 16
            params = [(50, 0.9), (-1, 0.8), (7, 1.0), (-1, 1.0), (vocab, 0.95), (300, 0.5)]
            draws, expected, tried = [], [], 0
            for k, p in params:
                decisions = logits_decisions(x, t, k, p)
                for u in (0.11, 0.37, 0.5, 0.77, 0.93):
                    tried += 1
                    cut, draw = logits_margins(x, t, k, p, u, decisions)
                    if cut >= MARGIN and draw >= MARGIN and sum(1 for d in draws if d[:2] == (k, p)) < 2:
                        tok, n_kept, _ = osmp.sample_fixed_point(x, t, k, p, u)
                        draws.append((k, p, u))
                        expected.append((tok, n_kept))
            cases.append(LogitsCase(f"D-{vocab}-T{t}", x, t, draws, expected, tried))
    return cases


# ---------------------------------------------------------------- E. special values
FORMATS = {  # storage type -> (numpy bit type, +inf, -inf, NaN with a clear sign bit, NaN with the sign bit set)
    "float32": (np.uint32, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000),
    "bfloat16": (np.uint16, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0),
    "float16": (np.uint16, 0x7C00, 0xFC00, 0x7E00, 0xFE00),
}


def to_bits(x32, fmt):
    x32 = np.ascontiguousarray(x32, dtype=F32)
    if fmt == "float32":
        return x32.view(np.uint32).copy()
    if fmt == "bfloat16":
        b = (x32.view(np.uint32) >> 16).astype(np.uint16)
        assert np.array_equal(from_bits(b, fmt), x32)  # grid values are exact
        return b
    h = x32.astype(np.float16)
    assert np.array_equal(h.astype(F32), x32)
    return h.view(np.uint16).copy()


def from_bits(b, fmt):
    if fmt == "float32":
        return np.asarray(b, dtype=np.uint32).view(F32)
    if fmt == "bfloat16":
        return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F32)
    return np.asarray(b, dtype=np.uint16).view(np.float16).astype(F32)


@dataclasses.dataclass
class SpecialRow:
    """bits: the row in its storage type; grid: equal logits are bit-equal and distinct ones >= 1/8 apart, so a top_k cut is
    decided alike on the device and in numpy (otherwise only keep-all draws are compared)"""
    name: str
    bits: np.ndarray
    grid: bool = True


@functools.lru_cache(maxsize=None)
def special_rows(fmt):
    """the rows of section E in storage type `fmt`, all of vocabulary 1027 (a ragged tail of 3) except the padded 1024"""
    _, pinf, ninf, nan_pos, nan_neg = FORMATS[fmt]
    rng = np.random.default_rng(17)
    vocab = 1027
    base = (np.round(rng.uniform(-2, 2, vocab) * 8) / 8).astype(F32)
    base[400] = 2.5  # one clear maximum
    rows = []

    def poke(name, at, pattern, n=vocab, grid=True):
        b = to_bits(base[:n], fmt)
        b[list(at)] = pattern
        rows.append(SpecialRow(name, b, grid))

    poke("ninf-tail", range(1000, 1024), ninf, n=1024)
    poke("ninf-interior", [0, 3, 4, 255, 256, 400, 1026] + list(range(500, 521)), ninf)
    poke("one-finite", [i for i in range(vocab) if i != 777], ninf)
    poke("one-finite-tail", [i for i in range(vocab) if i != 1026], ninf)
    poke("all-ninf", range(vocab), ninf)
    poke("one-pinf", [600], pinf)
    poke("two-pinf", [300, 900], pinf)
    for tag, pat in (("nan", nan_pos), ("neg-nan", nan_neg)):
        for at in (0, 513, 1026):
            poke(f"{tag}-{at}", [at], pat)
    poke("neg-nan-beside-pinf", [100, 700], pinf)
    rows[-1].bits[50] = nan_neg
    if fmt == "float16":
        sub = rng.integers(1, 0x400, vocab).astype(np.uint16) | (rng.integers(0, 2, vocab).astype(np.uint16) << 15)
        sub[1026] = 0x03FF  # the largest subnormal, in the ragged tail
        rows.append(SpecialRow("subnormals", sub, grid=False))
        poke("65504-beside-pinf", [10, 900], 0x7BFF)
        rows[-1].bits[600] = pinf
        b = np.full(vocab, 0xFBFF, dtype=np.uint16)  # -65504 everywhere ...
        b[[0, 5, 1026]] = ninf  # ... beside -inf
        rows.append(SpecialRow("neg-65504-beside-ninf", b))
        poke("65504", [10, 900], 0x7BFF)
    return rows


SPECIAL_DRAWS = [(1.0, -1, 1.0, 0.0), (0.7, -1, 1.0, ONE_BELOW), (1.0, 0, 1.5, ONE_BELOW), (0.7, 50, 1.0, 0.0), (1.3, 50, 1.0, ONE_BELOW),
                 (0.7, 1, 1.0, 0.5)]  # (temperature, top_k, top_p, u); the last is a greedy row inside a sampling batch


def special_expected(row, fmt):
    """[(temperature, top_k, top_p, u, token, n_kept)] for the draws compared on this row"""
    x = from_bits(row.bits, fmt)
    out = []
    with np.errstate(all="ignore"):
        for t, k, p, u in SPECIAL_DRAWS:
            if k == 50 and not row.grid:
                continue
            tok, n, _ = osmp.sample_fixed_point(x, t, k, p, u)
            if k != 1 and u == ONE_BELOW:  # the draw is robust: the last weighted token owns more than 2^-20 of the mass
                mask, _, fix, _ = osmp.kept_set_fixed_point(x, t, k, p)
                s = int(np.where(mask, fix, 0).sum())
                assert s == 0 or int(fix[tok]) > s * 2.0 ** -20, (row.name, t, k)
            out.append((t, k, p, u, tok, n))
    return out
