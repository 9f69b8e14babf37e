"""Exact inputs and a float64 specification for the MoE routing kernels of gate.hip (no GPU needed).

The router is a selection: a wrong expert leaves the model fluent, so the expectation has to be an equality.  This file
holds everything that equality needs and that can be checked on the CPU (tests/test_route_exact_host.py); the device
comparison itself is tests/test_gpu_route_exact.py.

  spec()            the router restated in numpy: oracle/deepseek.py::gate_from_logits and oracle/mixtral.py::route plus the
                    tie rule of gate.hip (lower expert index first, lower group index first).  Sigmoid routers are bf16
                    pipelines and are computed in float32 with one bf16 rounding per torch op; softmax routers in float64.
  safe sigmoid      device expf may differ from the CPU's by an ulp, so sigmoid logits are drawn only from bf16 values whose
                    float64 sigmoid lies more than 2^-8 bf16-ulp from a rounding midpoint (SAFE): an fp32 evaluation error
                    of a few ulps is ~2^-14 bf16-ulp, so every faithful fp32 sigmoid rounds them alike.
  exact weights     the fp32 sum of the selected scores in rank order equals their float64 sum (asserted per case), so the
                    sum is exact in any order; division and scaling are single IEEE fp32 operations.
  softmax           logits on the grid k/16: scores of different logits differ by >= 6 % (asserted: >= 2^-6 relative, after
                    the bias and for the group scores too), equal logits give bit-identical scores; ids must be equal, a
                    weight must be a bf16 neighbour of the float64 value and the nearest one wherever that value lies more
                    than 2^-12 bf16-ulp from a midpoint (fp32 expf, sum and division: a few fp32 ulps = 2^-14 bf16-ulp).
  planes            the bf16 logit L = K ulp is delivered as S fp32 planes of integer multiples of q = ulp / 256 with a
                    different multiplier in every plane, summing to (256 K + d) q, 0 < |d| < 128: the sum is exact in fp32 in
                    any order, is NOT a bf16 value, rounds to L, and every plane alone is worth more than two bf16 ulps.
  dispatch()        a mirror of the launch predicate of gate_route_launch, to prove which kernel and sort a case reaches.
"""

import dataclasses
import functools

import numpy as np

from oracle import moe_align as oalign

SIGMOID, SOFTMAX, RENORM = "sigmoid", "softmax", "softmax_renorm"
SCORE_CODE = {SOFTMAX: 0, SIGMOID: 1, RENORM: 2}
ID_SENTINEL = -7
W_SENTINEL = 0x7FC1  # a quiet NaN no computation produces
F32 = np.float32


# ---------------------------------------------------------------- bf16 in numpy
def bf16_bits(x32):
    """float32 -> bf16 bit pattern, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x32, dtype=F32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) >> 16).astype(np.uint16)


def bits_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def r32(x32):
    """float32 -> the nearest bf16 value, as float32: one torch bf16 op's rounding."""
    return bits_f32(bf16_bits(x32))


def bf16_ulp64(v):
    """Spacing of the bf16 values in the binade of |v| (float64, normal v)."""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, e - 1 - 7)


def r64(v):
    """float64 -> the nearest bf16 value (ties to even) in ONE rounding, as float64."""
    u = bf16_ulp64(v)
    return np.rint(v / u) * u


def midpoint_distance(v):
    """Distance of float64 v from the nearest bf16 rounding midpoint, in bf16 ulps of v's binade (0 .. 0.5)."""
    n = np.abs(v) / bf16_ulp64(v)
    return np.abs(n - np.floor(n) - 0.5)


# ---------------------------------------------------------------- the safe sigmoid logit table
@functools.lru_cache(None)
def sigmoid_table():
    """All 65536 bf16 patterns as logits: (x float64, score float64, normal mask, safe mask)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = bits_f32(np.arange(65536, dtype=np.uint32).astype(np.uint16)).astype(np.float64)
        s = 1.0 / (1.0 + np.exp(-x))
    normal = np.isfinite(x) & (s >= 2.0 ** -126)
    safe = normal.copy()
    safe[normal] = midpoint_distance(s[normal]) > 2.0 ** -8
    return x, s, normal, safe


@functools.lru_cache(None)
def levels(lo=-6.0, hi=8.0):
    """The builders' alphabet: the distinct bf16 scores reachable from a safe logit in [lo, hi] with |x| >= 2^-6, ascending,
    and for each the safe logit of smallest magnitude that gives it.  Returns (scores float32, logits float32)."""
    x, s, _, safe = sigmoid_table()
    pick = safe & (x >= lo) & (x <= hi) & (np.abs(x) >= 2.0 ** -6)
    xs, sc = x[pick], r64(s[pick])
    order = np.lexsort((np.abs(xs), sc))
    xs, sc = xs[order], sc[order]
    first = np.r_[True, sc[1:] != sc[:-1]]
    return sc[first].astype(F32), xs[first].astype(F32)


def logit_for(p):
    """Target scores (any shape) -> (the nearest reachable bf16 score, its safe logit)."""
    sc, xs = levels()
    p = np.asarray(p, dtype=np.float64)
    i = np.clip(np.searchsorted(sc, p), 1, len(sc) - 1)
    i = np.where(np.abs(sc[i - 1] - p) <= np.abs(sc[i] - p), i - 1, i)
    return sc[i], xs[i]


def saturated_logits():
    """Safe logits in [8, 16] whose bf16 score is exactly 1."""
    x, s, _, safe = sigmoid_table()
    pick = safe & (x >= 8.0) & (x <= 16.0)
    assert (r64(s[pick]) == 1.0).all()
    return x[pick].astype(F32)


SOFTMAX_GRID = np.array([k / 16.0 for k in range(-128, 128) if k != 0], dtype=F32)  # bf16 values, 6.4 % apart in score


# ---------------------------------------------------------------- the case record
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str            # the builder
    E: int
    G: int = 1           # n_groups
    Kg: int = 1          # topk_groups
    topk: int = 8
    score: str = SIGMOID
    bias: bool = False
    S: int = 0           # fp32 split-K planes (0: bf16 logits)
    M: int = 3
    extra_n: int = 0     # always-on slots
    extra_id: int = -1
    alE: int = 0         # align_num_experts (0: chitu_hip_gate_route, no sort)
    block: int = 16
    ep: tuple = ()       # (rank, ranks): an expert-parallel expert_map over the routed experts
    scale: float = 2.5
    seed: int = 0

    @property
    def cols(self):
        return self.topk + (self.extra_n if self.extra_id >= 0 else 0)

    @property
    def gs(self):
        return self.E // self.G if self.G > 1 else 0


EXTRA_W = 0.75


# ---------------------------------------------------------------- the dispatch mirror (gate_route_launch)
def dispatch(c, generic=-1, ticket=-1, small_sort=-1):
    """(kernel, sort) the launcher picks for case c under the three debug options (-1: its own heuristic)."""
    threads = (max(c.E, c.alE) + 63) // 64 * 64
    sigmoid, gs = c.score == SIGMOID, c.gs
    fast = (sigmoid and gs in (0, 32, 64) and c.S <= 16 and (threads // 64) * c.topk <= 64
            and ((threads // 64) * c.topk) % 4 == 0 and c.G <= 32 and generic <= 0)
    small = (c.E <= c.alE and (c.extra_id < 0 or (c.extra_id >= c.E and c.extra_id + c.extra_n <= c.alE))
             and small_sort != 0)
    wg_sort = "wg_small" if small else "wg_general"
    if fast and c.alE > 0 and c.E == 256 and gs in (0, 32) and c.M <= 16 and c.extra_n <= 32 and ticket <= 0:
        return f"gate_route_align_wg_kernel<{gs}>", wg_sort
    if (not fast and c.alE > 0 and c.E <= 64 and not sigmoid and c.G <= 1 and c.M <= 16 and c.S <= 16 and c.topk <= 16
            and c.extra_n <= 32 and ticket <= 0 and generic <= 0):
        return "gate_route_align_wg_softmax_kernel", wg_sort
    sort = "none" if c.alE == 0 else "bs1_tail" if c.M == 1 else "ticket"
    if fast:
        return f"gate_route_fast_kernel<{gs}>", sort
    return f"gate_route_kernel<{1 if sigmoid else 0}>", sort


VARIANTS = {"default": {}, "gate_generic": dict(generic=1), "gate_ticket": dict(ticket=1), "gate_small_sort0": dict(small_sort=0)}
OPTIONS = {"default": {}, "gate_generic": {"gate_generic": 1}, "gate_ticket": {"gate_ticket": 1},
           "gate_small_sort0": {"gate_small_sort": 0}}


def variants(c):
    """The launch variants that reach another kernel or sort than the default for this case, the default first."""
    base = dispatch(c)
    return ["default"] + [v for v, kw in VARIANTS.items() if kw and dispatch(c, **kw) != base]


def small_declined(c):
    """The one-workgroup launch with the in-routing sort allowed, which the launcher still declines (always-on id outside
    [num_experts, align_num_experts))."""
    k, s = dispatch(c)
    return "align_wg" in k and s == "wg_general"


# ---------------------------------------------------------------- planes
def make_planes(logit, S, rng):
    """bf16 logits [M, E] (non-zero) -> fp32 planes [S + 2, M, E]: planes 0..S-1 as the module docstring says, two NaN planes
    behind them.  Every multiplier is asserted distinct per element and worth more than two bf16 ulps."""
    L = logit.astype(np.float64)
    assert (L != 0).all()
    ulp = bf16_ulp64(L)
    q = ulp / 256.0
    K = np.rint(L / ulp).astype(np.int64)  # 128 <= |K| <= 255
    d = rng.integers(1, 101, size=L.shape)
    d = np.where(rng.random(L.shape) < 0.4, -rng.integers(1, 61, size=L.shape), d)
    total = K * 256 + np.sign(K) * d  # rounds to K: |d| < 128, and d > -64 where |K| = 128 sits on a binade edge
    n = np.zeros((S,) + L.shape, dtype=np.int64)
    if S > 1:
        base = rng.permutation(np.arange(4, 4 + 2 * S))[: S - 1]  # distinct per plane
        sign = np.where(rng.random(S - 1) < 0.5, -1, 1)
        for s in range(S - 1):
            # (the odd low part makes every partial sum a non-bf16 value: a sum rounded plane by plane goes wrong)
            n[s] = sign[s] * ((base[s] * 8 + rng.integers(0, 8, size=L.shape)) * 512 + rng.integers(-255, 256, size=L.shape))
    n[S - 1] = total - n[: S - 1].sum(axis=0)
    # the last multiplier must be large and distinct too: where it is not, move a multiple of 1024 q between it and plane 0
    for it in range(16):
        if S == 1:
            break
        srt = np.sort(n, axis=0)
        bad = (np.abs(n) < 1024).any(axis=0) | (srt[1:] == srt[:-1]).any(axis=0)
        if not bad.any():
            break
        n[S - 1] += np.where(bad, 1024 * (37 + 2 * it), 0)
        n[0] -= np.where(bad, 1024 * (37 + 2 * it), 0)
    assert (n.sum(axis=0) == total).all() and np.abs(n).sum(axis=0).max() < 2 ** 24  # any partial sum, in any order, is an fp32 value
    if S > 1:
        srt = np.sort(n, axis=0)
        assert (np.abs(n) >= 1024).all() and (srt[1:] != srt[:-1]).all()
    planes = np.full((S + 2,) + L.shape, np.nan, dtype=F32)
    planes[:S] = (n * q).astype(F32)
    assert (planes[:S].astype(np.float64) == n * q).all()  # every plane is an fp32 value
    assert (r64(planes[:S].astype(np.float64).sum(axis=0)) == L).all()
    return planes


def sum_planes(planes, S, mut=()):
    """The routing kernels' logit: fp32 sum of planes 0..S-1 in plane order, rounded once to bf16 -- with the reference
    mutations of the host test."""
    use = [planes[s] for s in range(S)]
    if "drop_plane" in mut:
        use = use[:-1] if S > 1 else [np.zeros_like(use[0])]
    if "double_last" in mut:
        use = use + [use[-1]]
    a = np.zeros_like(planes[0])
    for p in use:
        a = (a + p).astype(F32)
        if "round_per_plane" in mut:
            a = r32(a)
    return a if "no_sum_round" in mut else r32(a)


# ---------------------------------------------------------------- the specification
def _order_desc(v, higher_index_wins=False):
    """argsort by (value descending, index ascending) along the last axis; -0 == +0."""
    if higher_index_wins:
        n = v.shape[-1]
        return n - 1 - np.argsort(-v[..., ::-1], axis=-1, kind="stable")
    return np.argsort(-v, axis=-1, kind="stable")


def spec(c, logit, bias, mut=(), keep_groups=None):
    """The router on bf16 logits [M, E] (float32 array of bf16 values), bias (float32 array of bf16 values, or None).

    Returns a dict: ids [M, topk] in rank order; w_bits [M, topk] uint16 (sigmoid) or w64 [M, topk] float64 (softmax);
    masked [M, E] selection scores after the group mask; gscore [M, G] or None; kept [M, Kg] group ids or None; cut_tie /
    group_tie [M] bool (an equality exactly at the top-k / topk_groups cut).  keep_groups [M, Kg] overrides the group choice
    (the host test follows torch.topk's unspecified choice among tied groups)."""
    M, E = logit.shape
    hi = "higher_index" in mut
    sig = c.score == SIGMOID
    if sig:
        orig = r64(1.0 / (1.0 + np.exp(-logit.astype(np.float64)))).astype(F32)
        sel = orig if bias is None else r32((orig + bias[None, :]).astype(F32))
    else:
        x = logit.astype(np.float64)
        ex = np.exp(x - x.max(axis=-1, keepdims=True))
        orig = ex / ex.sum(axis=-1, keepdims=True)
        sel = orig if bias is None else orig + bias[None, :].astype(np.float64)
    gscore = kept = None
    group_tie = np.zeros(M, bool)
    masked = sel
    if c.G > 1:
        grouped = sel.reshape(M, c.G, -1)
        top2 = np.sort(grouped, axis=-1)[..., -2:]
        if bias is None or "group_max" in mut:
            gscore = top2[..., 1]
        else:
            gscore = r32((top2[..., 1] + top2[..., 0]).astype(F32)) if sig else top2[..., 1] + top2[..., 0]
        gorder = _order_desc(gscore, hi)
        kept = gorder[:, : c.Kg] if keep_groups is None else keep_groups
        if c.Kg < c.G:
            rows = np.arange(M)
            group_tie = gscore[rows, gorder[:, c.Kg - 1]] == gscore[rows, gorder[:, c.Kg]]
        mask = np.zeros((M, c.G), bool)
        np.put_along_axis(mask, kept, True, axis=1)
        off = -np.inf if "mask_neginf" in mut else 0.0
        masked = np.where(mask[:, :, None], grouped, off).reshape(M, E).astype(sel.dtype)
    order = _order_desc(masked, hi)
    ids = order[:, : c.topk].astype(np.int64)
    rows = np.arange(M)
    cut_tie = (masked[rows, order[:, c.topk - 1]] == masked[rows, order[:, c.topk]]) if c.topk < E else np.zeros(M, bool)
    chosen = np.take_along_axis(orig, ids, axis=1)
    out = dict(ids=ids, masked=masked, gscore=gscore, kept=kept, cut_tie=cut_tie, group_tie=group_tie, orig=orig, sel=sel)
    if sig:
        s32 = np.cumsum(chosen, axis=1, dtype=F32)[:, -1]  # sequential fp32 adds in rank order
        out["sum_exact"] = bool((s32.astype(np.float64) == chosen.astype(np.float64).sum(axis=1)).all() and (s32 > 0).all())
        w = r32((chosen / r32(s32)[:, None]).astype(F32))
        out["w_bits"] = bf16_bits((w * F32(c.scale)).astype(F32))
    else:
        w = chosen
        if c.score == RENORM and "no_renorm" not in mut:
            w = w / w.sum(axis=1, keepdims=True)
        out["w64"] = w * float(F32(c.scale))
    return out


def softmax_weight_ok(w64, got_bits):
    """The softmax rule: (every weight is a bf16 neighbour of its float64 value AND the nearest one wherever that value lies
    more than 2^-12 bf16-ulp from a midpoint, the share of weights under the strict rule)."""
    u = bf16_ulp64(w64)
    lo, hi = np.floor(w64 / u) * u, np.ceil(w64 / u) * u
    got = bits_f32(got_bits).astype(np.float64)
    strict = midpoint_distance(w64) > 2.0 ** -12
    ok = ((got == lo) | (got == hi)) & (~strict | (got == r64(w64)))
    return ok, float(strict.mean())


def well_separated(v):
    """Every two entries of each row of v are bit-equal or at least 2^-6 apart, relative to the larger magnitude."""
    s = np.sort(v, axis=-1)
    a, b = s[..., :-1], s[..., 1:]
    return bool(((a == b) | (b - a >= 2.0 ** -6 * np.maximum(np.abs(a), np.abs(b)))).all())


# ---------------------------------------------------------------- builders: bf16 logits [M, E], bias [E] or None
def _bias_small(c, rng):
    return (rng.integers(-16, 17, size=c.E) * 2.0 ** -7).astype(F32) if c.bias else None


def _rand(c, rng):
    """Safe logits drawn with replacement (ties wherever they fall), bias in steps of 2^-7."""
    if c.score == SIGMOID:
        _, xs = levels()
        return xs[rng.integers(0, len(xs), size=(c.M, c.E))], _bias_small(c, rng)
    if c.E <= 64:  # a wide grid over few experts would leave one winner with everything: a window of the grid per token
        lo = rng.integers(0, len(SOFTMAX_GRID) - c.E, size=c.M)
        logit = np.stack([rng.permutation(SOFTMAX_GRID[l:l + c.E]) for l in lo])
    else:  # (256 experts on 255 grid values: one pair of equal logits per token)
        logit = np.stack([rng.permutation(SOFTMAX_GRID)[np.arange(c.E) % len(SOFTMAX_GRID)] for _ in range(c.M)])
    bias = None
    if c.bias:  # a few experts only: a bias under every score would push the small ones closer together than 2^-6 relative
        bias = np.zeros(c.E, dtype=F32)
        bias[rng.permutation(c.E)[:4]] = [0.5, 1.0, -0.5, 0.25]
    return logit, bias


def _rand_low(c, rng):
    """Sigmoid logits in [-6, -1] only (scores below 0.27, where one bf16 ulp of the logit moves the score by about one bf16
    ulp): the plane sweep's data, on which a logit that is off by one rounding shows in the selected weights."""
    assert c.score == SIGMOID
    x, _, _, safe = sigmoid_table()
    xs = x[safe & (x >= -6.0) & (x <= -1.0)].astype(F32)
    return xs[rng.integers(0, len(xs), size=(c.M, c.E))], _bias_small(c, rng)


def _few(c, rng):
    """Six levels only: ties in every group, at every cut, inside and across waves."""
    if c.score == SIGMOID:
        _, xs = levels()
        lv = xs[rng.choice(len(xs), size=6, replace=False)]
        bias = (rng.integers(0, 2, size=c.E) * 2.0 ** -4).astype(F32) if c.bias else None
    else:
        lv = rng.choice(SOFTMAX_GRID, size=6, replace=False)
        bias = None  # (a softmax bias would need the separation re-proved per draw; the biased softmax case is `rand`)
    logit = lv[rng.integers(0, 6, size=(c.M, c.E))]
    if c.G > 1 and c.score != SIGMOID:  # the last group repeats the first: a group-score tie of bit-equal fp32 sums
        rows = logit.reshape(c.M, c.G, -1)
        rows[:, -1] = rows[:, 0]
        logit = rows.reshape(c.M, c.E)
    return logit, bias


def _group_roles(c):
    """(a, b, tier1, low): the pair of groups at the topk_groups cut (a < b), the Kg - 1 groups above it, the rest below."""
    assert c.G >= c.Kg + 1 and c.topk == 2 * c.Kg
    a, b = (0 if c.G == 3 else 1), c.G - 1
    rest = [g for g in range(c.G) if g not in (a, b)]
    tier1 = rest[: c.Kg - 1] if c.G == 3 else rest[1: c.Kg]  # (group 0 stays below the cut where there is room)
    assert len(tier1) == c.Kg - 1
    return a, b, tier1, [g for g in rest if g not in tier1]


def _grouped_background(c, rng):
    return rng.uniform(0.05, 0.3, size=(c.M, c.G, c.E // c.G))


def _two_positions(c, rng):
    gs = c.E // c.G
    j = rng.permutation(gs)[:2]
    return int(j[0]), int(j[1])


def _group_tie_at_cut(c, rng):
    """Groups a < b hold identical rows, and their score is exactly the topk_groups-th: a stays, b is masked; both top
    experts of a are in the top-k."""
    a, b, tier1, low = _group_roles(c)
    p = _grouped_background(c, rng)
    for t in range(c.M):
        for i, g in enumerate(tier1):
            j1, j2 = _two_positions(c, rng)
            p[t, g, j1], p[t, g, j2] = 0.97 - 0.004 * i, 0.93 - 0.004 * i
        for i, g in enumerate(low):
            j1, j2 = _two_positions(c, rng)
            p[t, g, j1], p[t, g, j2] = 0.5 - 0.01 * i, 0.45
        j1, j2 = _two_positions(c, rng)
        p[t, a, j1], p[t, a, j2] = 0.85, 0.80
        p[t, b] = p[t, a]
    bias = None
    if c.bias:  # the same bias in every group, so the pair stays identical
        bias = np.tile((rng.integers(-4, 5, size=c.E // c.G) * 2.0 ** -7).astype(F32), c.G)
    return logit_for(p.reshape(c.M, c.E))[1], bias


def _group_max_twice(c, rng):
    """Group b's maximum appears twice (0.7 + 0.7 = 1.4) against group a's 0.8 + 0.55 at the cut: b stays only if the second
    maximum counts in full; by its maximum alone, a would."""
    a, b, tier1, low = _group_roles(c)
    p = _grouped_background(c, rng)
    for t in range(c.M):
        for i, g in enumerate(tier1):
            j1, j2 = _two_positions(c, rng)
            p[t, g, j1], p[t, g, j2] = 0.97 - 0.004 * i, 0.93 - 0.004 * i
        for i, g in enumerate(low):
            j1, j2 = _two_positions(c, rng)
            p[t, g, j1], p[t, g, j2] = 0.5 - 0.01 * i, 0.45
        j1, j2 = _two_positions(c, rng)
        p[t, b, j1], p[t, b, j2] = 0.7, 0.7
        j1, j2 = _two_positions(c, rng)
        p[t, a, j1], p[t, a, j2] = 0.8, 0.55
    return logit_for(p.reshape(c.M, c.E))[1], np.zeros(c.E, dtype=F32)


def _masked_zero(c, rng, exact_zero):
    """The last Kg groups stay, each with ONE positive biased score; their other experts are negative (bias -1) or, with
    exact_zero, exactly +0 (bias = -score).  The top-k then needs Kg more experts: the masked zeros of group 0, lowest
    index first, beat the negatives and -- by index -- the unmasked zeros."""
    assert c.G >= c.Kg + 1 and c.topk == 2 * c.Kg and c.bias
    gs = c.E // c.G
    p = _grouped_background(c, rng)
    sc, xs = logit_for(p.reshape(c.M, c.E))
    bias = np.full(c.E, -1.0, dtype=F32)
    for i, g in enumerate(range(c.G - c.Kg, c.G)):
        j = int(rng.integers(0, gs))
        if exact_zero:  # one row of scores for every token, so that bias = -score holds for all of them
            sc[:, g * gs:(g + 1) * gs], xs[:, g * gs:(g + 1) * gs] = sc[0, g * gs:(g + 1) * gs], xs[0, g * gs:(g + 1) * gs]
            bias[g * gs:(g + 1) * gs] = -sc[0, g * gs:(g + 1) * gs]
        hi_p = 0.96 - 0.01 * i - 0.002 * np.arange(c.M)
        sc[:, g * gs + j], xs[:, g * gs + j] = logit_for(hi_p)
        bias[g * gs + j] = 0.0
    return xs, bias


def _topk_ties(c, rng):
    """Ungrouped, one token per situation (those the shape has room for): four equal scores at the cut inside one wave;
    the same across waves (63 | 64 where there is a second wave); equal pairs at the top ranks far apart; all equal;
    saturated scores (exactly 1) for half the experts."""
    assert c.G == 1
    E, k = c.E, c.topk
    sc_all, _ = levels()
    rows = []

    def base():
        return rng.uniform(0.05, 0.3, size=E)

    def distinct_high(n):
        cand = sc_all[(sc_all > 0.62) & (sc_all < 0.99)]
        return rng.choice(cand, size=n, replace=False)

    if E >= k + 2 and k >= 2:
        for spread in (False, True):
            p = base()
            if spread and E > 64:
                tied = np.array([63, 64, E - 1, 1])
            elif spread:
                tied = np.array([0, E // 3, 2 * E // 3, E - 1])
            else:
                tied = rng.permutation(min(64, E))[:4]
            free = np.setdiff1d(np.arange(E), tied)
            p[rng.choice(free, size=k - 2, replace=False)] = distinct_high(k - 2)
            p[tied] = 0.6
            rows.append(logit_for(p)[1])
        p = base()
        pos = rng.permutation(E)[:k]
        vals = distinct_high(k)
        vals[1], vals[3 % k] = vals[0], vals[2 % k]
        p[pos] = vals
        rows.append(logit_for(p)[1])
    rows.append(np.full(E, logit_for(0.4)[1], dtype=F32))
    sat = saturated_logits()
    _, xs = levels()
    row = xs[rng.integers(0, len(xs), size=E)]
    half = rng.permutation(E)[: max(E // 2, 1)]
    row[half] = sat[rng.integers(0, len(sat), size=len(half))]
    rows.append(row)
    return np.stack(rows).astype(F32), None


BUILDERS = {
    "rand": _rand,
    "rand_low": _rand_low,
    "few": _few,
    "group_tie_at_cut": _group_tie_at_cut,
    "group_max_twice": _group_max_twice,
    "negative_vs_masked_zero": lambda c, rng: _masked_zero(c, rng, False),
    "unmasked_zero_vs_masked_zero": lambda c, rng: _masked_zero(c, rng, True),
    "topk_ties": _topk_ties,
}
NAMED = ("group_tie_at_cut", "group_max_twice", "negative_vs_masked_zero", "unmasked_zero_vs_masked_zero", "topk_ties")


def expert_map(c):
    if not c.ep:
        return None
    r, n = c.ep
    per = c.E // n
    m = np.full(max(c.E, c.alE), -1, dtype=np.int32)
    m[r * per:(r + 1) * per] = np.arange(per, dtype=np.int32)
    return m


def align_expect(c, ids_full, sorted_cap, expert_cap):
    """oracle.moe_align on the spec's ids [M, cols] at the capacities the launch is given.  Ids outside [0, alE) are dropped
    by the sort: they are handed to the oracle as one expert more, whose segment (the last) is cut off again."""
    flat = np.asarray(ids_full).reshape(-1)
    numel = flat.size
    clipped = np.where((flat >= 0) & (flat < c.alE), flat, c.alE)
    emap = expert_map(c)
    s, e, _, cum = oalign.moe_align_block_size(clipped, c.block, c.alE + 1, None)
    total = int(cum[c.alE])
    sorted_ids = np.full(sorted_cap, numel, dtype=np.int32)
    sorted_ids[:total] = s[:total]
    expert_ids = np.zeros(expert_cap, dtype=np.int32)
    expert_ids[: total // c.block] = e[: total // c.block]
    if emap is not None:
        expert_ids = emap[expert_ids]  # over the WHOLE array: unused blocks hold expert_map[0]
    return dict(sorted_ids=sorted_ids, expert_ids=expert_ids, num_post_pad=np.array([total], dtype=np.int32),
                cumsum=cum[: c.alE + 1].astype(np.int32))


@functools.lru_cache(None)
def build(c):
    """Inputs and expectation of case c (cached; treat as read-only).  Keys: logit [M, E] bf16 values, planes [S + 2, M, E]
    or None, bias or None, spec (see spec()), ids_full [M, cols], and for softmax strict_share."""
    for attempt in range(400):
        rng = np.random.default_rng([c.seed, attempt, c.E, c.M, c.S, c.topk])
        logit, bias = BUILDERS[c.kind](c, rng)
        logit = np.ascontiguousarray(logit, dtype=F32)
        assert logit.shape == (c.M, c.E), (c, logit.shape)
        assert (r32(logit) == logit).all() and (bias is None or (r32(bias) == bias).all())
        sp = spec(c, logit, bias)
        if c.score == SIGMOID:
            assert sp["sum_exact"], c
            break
        sep = well_separated(sp["sel"]) and (sp["gscore"] is None or well_separated(sp["gscore"]))
        _, share = softmax_weight_ok(sp["w64"], bf16_bits(sp["w64"].astype(F32)))
        if sep and share >= 0.95:
            sp["strict_share"] = share
            break
    else:
        raise AssertionError(f"no admissible draw for {c}")
    planes = make_planes(logit, c.S, rng) if c.S else None
    if planes is not None:
        assert (sum_planes(planes, c.S) == logit).all()
    ids_full = sp["ids"]
    if c.extra_id >= 0 and c.extra_n:
        extra = np.broadcast_to(c.extra_id + np.arange(c.extra_n, dtype=np.int64), (c.M, c.extra_n))
        ids_full = np.concatenate([ids_full, extra], axis=1)
    return dict(logit=logit, planes=planes, bias=bias, spec=sp, ids_full=ids_full)


# ---------------------------------------------------------------- the GPU case list
R1 = dict(E=256, G=8, Kg=4, topk=8)
FORMS = {  # one small shape per instantiation, for the plane sweep (three tokens: a wrong [S, M, E] stride shows)
    "generic1": dict(E=64, topk=6, bias=True),
    "generic0": dict(E=160, topk=6, score=SOFTMAX, scale=1.0),
    "fast0": dict(E=128, topk=6),
    "fast32": dict(E=160, G=5, Kg=2, topk=4, bias=True),
    "fast64": dict(E=192, G=3, Kg=2, topk=4, bias=True),
    "wg0": dict(E=256, topk=8, bias=True, alE=256),
    "wg32": dict(**R1, bias=True, alE=257, extra_n=1, extra_id=256),
    "wg_softmax": dict(E=64, topk=6, score=SOFTMAX, scale=1.0, alE=66, extra_n=2, extra_id=64),
}
PLANES = (0, 1, 2, 8, 9, 15, 16)


@functools.lru_cache(None)
def gpu_cases():
    cs = []

    def add(name, kind, **kw):
        cs.append(Case(name=name, kind=kind, seed=len(cs), **kw))

    # ---- sigmoid routing, no sort: every shape, random and dense-tie data, bf16 logits and planes
    shapes = {
        "r1_bias": dict(**R1, bias=True), "r1_nobias": dict(**R1), "e256_flat": dict(E=256, topk=8, bias=True),
        "e192_g64": dict(E=192, G=3, Kg=2, topk=4, bias=True), "e160_g32": dict(E=160, G=5, Kg=2, topk=4, bias=True),
        "e96_g32": dict(E=96, G=3, Kg=2, topk=4), "e128_top6": dict(E=128, topk=6), "e64_top6": dict(E=64, topk=6, bias=True),
        "e16_g4": dict(E=16, G=4, Kg=2, topk=4, bias=True), "e72_top4": dict(E=72, topk=4, bias=True),
        "e72_top3": dict(E=72, topk=3), "e10_top4": dict(E=10, topk=4), "e10_top3": dict(E=10, topk=3, bias=True),
        "e1024_top64": dict(E=1024, topk=64, M=2), "e8_topk_is_E": dict(E=8, topk=8),
    }
    for n, kw in shapes.items():
        add(f"{n}-rand", "rand", **kw)
        add(f"{n}-few-S2", "few", **{**kw, "S": 2, "M": kw.get("M", 3)})
    add("r1_bias-rand-M5-extra", "rand", **R1, bias=True, M=5, extra_n=1, extra_id=256)
    # ---- the named edges, on every grouped form (serial scan, groups of 32 and 64, the half-empty last wave)
    grouped = {"r1": R1, "e192_g64": dict(E=192, G=3, Kg=2, topk=4), "e160_g32": dict(E=160, G=5, Kg=2, topk=4),
               "e96_g32": dict(E=96, G=3, Kg=2, topk=4), "e16_g4": dict(E=16, G=4, Kg=2, topk=4)}
    for n, kw in grouped.items():
        add(f"{n}-group_tie_at_cut-bias", "group_tie_at_cut", **kw, bias=True)
        add(f"{n}-group_tie_at_cut-nobias", "group_tie_at_cut", **kw)
        add(f"{n}-group_max_twice", "group_max_twice", **kw, bias=True)
        add(f"{n}-negative_vs_masked_zero", "negative_vs_masked_zero", **kw, bias=True)
        add(f"{n}-unmasked_zero_vs_masked_zero", "unmasked_zero_vs_masked_zero", **kw, bias=True)
    for n, kw in {"e256": dict(E=256, topk=8), "e128": dict(E=128, topk=6), "e72": dict(E=72, topk=4), "e64": dict(E=64, topk=6),
                  "e10": dict(E=10, topk=4), "e8": dict(E=8, topk=8), "e1024": dict(E=1024, topk=64)}.items():
        add(f"{n}-topk_ties", "topk_ties", **{**kw, "M": 5 if kw["E"] >= kw["topk"] + 2 else 2})
    # ---- softmax routing, no sort
    soft = {
        "v2lite": dict(E=64, topk=6, score=SOFTMAX, scale=1.0, extra_n=2, extra_id=64),
        "mixtral": dict(E=8, topk=2, score=RENORM, scale=1.0),
        "e256_g4": dict(E=256, G=4, Kg=2, topk=8, score=SOFTMAX, scale=2.5),
        "e160": dict(E=160, topk=6, score=RENORM, scale=1.0),
        "e64_bias": dict(E=64, topk=6, score=SOFTMAX, bias=True, scale=1.0),
        "e256_g4_bias": dict(E=256, G=4, Kg=2, topk=8, score=SOFTMAX, bias=True, scale=1.0),
    }
    for n, kw in soft.items():
        add(f"soft-{n}-rand", "rand", **kw)
        if not kw.get("bias"):
            add(f"soft-{n}-few-S2", "few", **kw, S=2)
    # ---- the plane sweep on every instantiation; 17 and 24 planes are the generic kernel's alone
    for n, kw in FORMS.items():
        for S in PLANES:
            add(f"planes-{n}-S{S}", "rand" if kw.get("score", SIGMOID) != SIGMOID else "rand_low", **{"M": 3, **kw, "S": S})
    add("planes-r1-S17", "rand", **R1, bias=True, S=17)
    add("planes-r1-S24", "rand", **R1, bias=True, S=24, alE=257, extra_n=1, extra_id=256)
    add("planes-v2lite-S17", "rand", E=64, topk=6, score=SOFTMAX, scale=1.0, S=17, alE=66, extra_n=2, extra_id=64)
    add("planes-mixtral-S24", "rand", E=8, topk=2, score=RENORM, scale=1.0, S=24)
    # ---- route + align: tokens x block x expert map x always-on id
    r1a = dict(**R1, bias=True, alE=257, extra_n=1, extra_id=256)
    for M in (1, 2, 15, 16, 17, 40, 300):
        add(f"align-r1-M{M}-b16", "rand", **r1a, M=M, block=16, S=2 if M in (15, 300) else 0)
        add(f"align-r1-M{M}-b64-ep", "few", **{**r1a, "extra_n": 0, "extra_id": -1, "alE": 256}, M=M, block=64, ep=(2, 8))
    for M in (1, 2, 15, 16, 17, 40):
        add(f"align-e256_flat-M{M}", "rand", E=256, topk=8, alE=256, M=M, block=64)
        add(f"align-v2lite-M{M}", "rand", E=64, topk=6, score=SOFTMAX, scale=1.0, alE=66, extra_n=2, extra_id=64, M=M,
            block=16 if M % 2 else 64)
        add(f"align-mixtral-M{M}", "few", E=8, topk=2, score=RENORM, scale=1.0, alE=8, M=M, block=16, ep=(1, 2) if M % 2 else ())
    for M in (1, 16):
        add(f"align-r1-M{M}-extra_inside_routed", "rand", **{**r1a, "extra_id": 3, "alE": 256}, M=M)
        add(f"align-r1-M{M}-extra_past_table", "rand", **{**r1a, "extra_id": 300}, M=M)
        add(f"align-v2lite-M{M}-extra_past_table", "rand", E=64, topk=6, score=SOFTMAX, scale=1.0, alE=64, extra_n=2,
            extra_id=64, M=M)
        add(f"align-r1-M{M}-group_tie", "group_tie_at_cut", **r1a, M=M)
        add(f"align-r1-M{M}-unmasked_zero", "unmasked_zero_vs_masked_zero", **r1a, M=M)
    add("align-e256_flat-topk_ties", "topk_ties", E=256, topk=8, alE=256, M=5)
    for M in (1, 19):
        add(f"align-e192_g64-M{M}", "rand", E=192, G=3, Kg=2, topk=4, bias=True, alE=193, extra_n=1, extra_id=192, M=M, S=2 * (M == 1))
    add("align-e16_g4-M19", "rand", E=16, G=4, Kg=2, topk=4, bias=True, alE=17, extra_n=1, extra_id=16, M=19)
    add("align-soft-e160-M5", "rand", E=160, topk=6, score=RENORM, scale=1.0, alE=160, M=5, block=64)
    return tuple(cs)
