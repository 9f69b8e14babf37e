"""Builders and oracle of the paged-KV schedule tests (tests/test_kv_schedule_host.py on the CPU, tests/test_gpu_kv_schedule.py
with the real launches): what a serving loop does to ONE PagedKVCacheManager over time, with no model and no GEMM.

* PlainCache is the oracle: request -> list of row identities (incarnation, token position), one list for all layers (the
  identity of a cached row is (incarnation, layer, position)).  It knows nothing about pages.
* A schedule is a list of steps over the manager's public methods (Script builds them and tracks the lengths); coverage()
  derives from the lengths alone which paging events a schedule contains, and every schedule of SCHEDULES is asserted at import
  to contain all of COVERAGE_ITEMS.
* Driver runs a schedule against a manager, writes the rows (plain indexing here; the GPU suite overrides append / to_cache /
  from_cache with the project's launches) and checks after every manager call: page accounting, every device-visible buffer
  against values recomputed from PlainCache and the host block_table, and the cached rows (torch.equal) gathered through the
  device table.

Row values.  V (MLA: the latent part) is attn_exact.identity_rows with the digit 2 * incarnation + layer.  K (MLA: the rope
part) is a positional code in three one-hot fields, p % 16, p // 16 and (p + 8) // 16, each at attn_exact.K_AMP: two different
positions below 256 agree in at most two fields, so a query with Q_AMP on the three channels of p leads by Q_AMP * K_AMP * scale;
and p, p + 1 always share the second or the third field, which is what the forbidden-row probe needs (forbidden_q below).  Rows
that must never be read -- rejected drafts, and the `bait` the driver writes at position `len` of every request whose last page
has room -- carry the code of their own position at full amplitude and the V row of ANOTHER incarnation; rows dropped by rollback
and a dead request's rows in a reused page are attractive by themselves (full-amplitude code, another identity).  Every value is
an integer <= 16: exact in bf16 and in both fp8 row formats.  All margins are asserted below from the construction.

Limits.  At a length that is a multiple of the page the position `len` lies in a page the request does not own: no bait can be
written there, the table column is 0, and an over-read lands in page 0, row 0 -- the forbidden-row probe is then only as strong as
what page 0 happens to hold.  The tail of the length vectors behind the batch (a ring slot's older values) is never handed to a
kernel by the getters and is not checked.  coverage() infers page reuse from the free list being a queue; should that change, the
import-time assertion of that item means less, and Driver.reused (observed on the real block tables, asserted by both suites)
is the check that holds."""
import random
from dataclasses import dataclass

import torch

from tests import attn_exact as ax
from tests import test_gqa_kv_fp8_host as g8
from tests import test_mla_kv_fp8_host as m8

LAYERS, HOT, MAX_INCARNATIONS = 2, 6, 8
FORMATS = ("bf16", "fp8")
MULTI_T = (2, 5, 8)
assert MAX_INCARNATIONS * LAYERS <= 16, "identity_rows' sequence digit has 16 values"


@dataclass(frozen=True)
class Family:
    name: str
    page: int
    max_seq_len: int
    scale: float
    heads: int
    kv_heads: int
    width: int  # of a V row (MLA: the latent part)

    @property
    def max_blocks(self):
        return self.max_seq_len // self.page + 1

    @property
    def capacity(self):
        return self.max_blocks * self.page

    @property
    def num_blocks(self):
        return self.max_blocks * HOT


GQA = Family("gqa", 16, 64, ax.GQA_SCALE, 8, 2, 128)      # 5 pages per request, 80 positions, 30 pages
MLA = Family("mla", 64, 192, ax.MLA_SCALE, 16, 1, 512)    # 4 pages per request, 256 positions, 24 pages
FAMILIES = {"gqa": GQA, "mla": MLA}
assert all(f.max_blocks <= 9 and f.capacity <= 256 for f in FAMILIES.values())

# ---------------------------------------------------------------- the positional code and its margins
CODE_W, MAX_POS = 64, 256


def code_channels(p):
    return [p % 16, 16 + p // 16, 32 + (p + 8) // 16]


CODE = torch.zeros(MAX_POS + 1, CODE_W)  # row p: the K (rope) code of position p
for _p in range(MAX_POS + 1):
    if _p // 16 < 16:
        CODE[_p, code_channels(_p)] = ax.K_AMP
CODE[MAX_POS] = 0.0  # no such position: never written, never probed


def probe_q(p):
    """[64] query that picks position p: Q_AMP on its three code channels"""
    q = torch.zeros(CODE_W)
    q[code_channels(p)] = ax.Q_AMP
    return q


def forbidden_q(n):
    """[64] query of a sequence of n keys that would pick the FORBIDDEN position n if a kernel admitted it: Q_AMP on the code of
    n plus Q_AMP / 2 on the code of n - 1 (tests/test_gpu_attn_window.py, window_probe_case).  Among the permitted keys n - 1 leads."""
    q = torch.zeros(CODE_W)
    q[code_channels(n)] += ax.Q_AMP
    q[code_channels(n - 1)] += ax.Q_AMP / 2
    return q


def _assert_margins():
    for fam in FAMILIES.values():
        cap = fam.capacity
        keys = CODE[:cap]
        s = torch.stack([probe_q(p) for p in range(cap)]) @ keys.T * fam.scale  # [probe, key]
        own = s.diagonal().clone()
        s.fill_diagonal_(float("-inf"))
        margin = float((own - s.max(1).values).min())
        assert margin >= ax.MIN_MARGIN_NATS, (fam.name, margin)
        assert abs(margin - ax.margin_nats(ax.Q_AMP, ax.K_AMP, fam.scale)) < 1e-3
        assert ax.leak_bound(cap, 15.0, margin) < ax.ABS_DOMINANT
        worst, bait = float("inf"), float("inf")
        for n in range(1, cap):
            sc = CODE[: n + 1] @ forbidden_q(n) * fam.scale
            if n > 1:
                worst = min(worst, float(sc[n - 1] - sc[: n - 1].max()))
            bait = min(bait, float(sc[n] - sc[:n].max()))
        want = ax.margin_nats(ax.Q_AMP / 2, ax.K_AMP, fam.scale)
        assert worst >= want - 1e-3 and bait >= want - 1e-3, (fam.name, worst, bait, want)  # the bait would win if it were read
        assert ax.leak_bound(cap, 15.0, want) < ax.ABS_DOMINANT, (fam.name, ax.leak_bound(cap, 15.0, want))


_assert_margins()

# ---------------------------------------------------------------- rows
_IDENT = {}


def _ident(fam, digit):
    if (fam.name, digit) not in _IDENT:
        _IDENT[fam.name, digit] = ax.identity_rows(fam.capacity, fam.kv_heads, fam.width, seq=digit)
    return _IDENT[fam.name, digit]


def rows(fam, inc, layer, positions, v_inc=None):
    """The bf16 rows of identity (inc, layer, p) for p in positions.  GQA: (K [n, Hkv, 128], V [n, Hkv, 128]) -- K = the code in
    channels 0 .. 63, the identity's first 64 channels behind it (no query touches them; they make two requests' K rows differ).
    MLA: ([n, 576],) = [latent | code].  v_inc: the V (latent) part of ANOTHER incarnation -- a row nobody may read."""
    assert 0 <= inc < MAX_INCARNATIONS
    pos = torch.as_tensor(list(positions), dtype=torch.int64)
    own = _ident(fam, LAYERS * inc + layer)[pos]
    val = own if v_inc is None else _ident(fam, LAYERS * v_inc + layer)[pos]
    code = CODE[pos]
    if fam.name == "gqa":
        k = torch.cat([code.unsqueeze(1).expand(-1, fam.kv_heads, -1), own[:, :, :64]], dim=-1)
        return k.to(torch.bfloat16), val.to(torch.bfloat16)
    return (torch.cat([val[:, 0], code], dim=-1).to(torch.bfloat16),)


def values(fam, new):
    """the V part of rows(): what the attention returns for a picked key, [n, Hkv, width]"""
    return new[1] if fam.name == "gqa" else new[0][:, None, : fam.width]


class Lens:
    """what the manager reads of a prefill's VarLens"""

    def __init__(self, counts):
        self.cpu_lens = [int(c) for c in counts]
        self.cpu_prefix_lens = [0]
        for c in self.cpu_lens:
            self.cpu_prefix_lens.append(self.cpu_prefix_lens[-1] + c)


class PlainCache:
    """request -> [(incarnation, position), ...]: the rows a request holds, the same in every layer"""

    def __init__(self):
        self.rows, self.inc = {}, {}

    def admit(self, req, inc, n=0):
        assert req not in self.rows
        self.rows[req] = [(inc, p) for p in range(n)]

    def append(self, req, n=1):
        inc = self.incarnation(req)
        self.rows[req] += [(inc, p) for p in range(len(self.rows[req]), len(self.rows[req]) + n)]

    def drop(self, req, n):
        assert 0 <= n <= len(self.rows[req])
        del self.rows[req][len(self.rows[req]) - n:]

    def free(self, req):
        del self.rows[req]

    def length(self, req):
        return len(self.rows[req])

    def incarnation(self, req):
        return self.inc[req]


# ---------------------------------------------------------------- schedules
class Script:
    """Builds a schedule and tracks the lengths.  Steps:
    ("prefill", reqs, lens) ("register", req, 0) ("decode", reqs) ("multi", reqs, T, accepted) ("rollback", reqs, drops)
    ("continue", reqs, counts) ("free", req)"""

    def __init__(self, fam, rnd=None):
        self.fam, self.steps, self.len, self.rnd = fam, [], {}, rnd

    def prefill(self, reqs, lens):
        self.steps.append(("prefill", list(reqs), list(lens)))
        self.len.update(zip(reqs, lens))

    def register(self, req):
        self.steps.append(("register", req, 0))
        self.len[req] = 0

    def decode(self, reqs, times=1):
        for _ in range(times):
            assert all(self.len[r] + 1 <= self.fam.capacity for r in reqs)
            self.steps.append(("decode", list(reqs)))
            for r in reqs:
                self.len[r] += 1

    def multi(self, reqs, T, acc):
        assert all(self.len[r] + T <= self.fam.capacity and 1 <= a <= T for r, a in zip(reqs, acc))
        self.steps.append(("multi", list(reqs), T, list(acc)))
        for r, a in zip(reqs, acc):
            self.len[r] += a

    def rollback(self, reqs, drops):
        assert all(0 <= d <= self.len[r] for r, d in zip(reqs, drops))
        self.steps.append(("rollback", list(reqs), list(drops)))
        for r, d in zip(reqs, drops):
            self.len[r] -= d

    def cont(self, reqs, counts):
        assert all(c >= 1 and self.len[r] + c <= self.fam.capacity for r, c in zip(reqs, counts))
        self.steps.append(("continue", list(reqs), list(counts)))
        for r, c in zip(reqs, counts):
            self.len[r] += c

    def free(self, req):
        self.steps.append(("free", req))
        del self.len[req]

    def to(self, req, n):
        """bring a request to length n by a continued prefill or a rollback"""
        d = n - self.len[req]
        if d > 0:
            self.cont([req], [d])
        elif d < 0:
            self.rollback([req], [-d])

    def room(self, reqs, n):
        """make sure every request of reqs can grow by n"""
        for r in reqs:
            if self.len[r] + n > self.fam.capacity:
                self.to(r, self.fam.capacity - n - self.fam.page // 2)

    def noise(self, k):
        """k random valid steps over the live requests (random schedules only); admits and frees nobody"""
        rnd, fam = self.rnd, self.fam
        if rnd is None:
            return
        for _ in range(k):
            live = list(self.len)
            reqs = rnd.sample(live, rnd.randint(1, len(live)))
            kind = rnd.choice(["decode", "decode", "decode", "multi", "rollback", "continue"])
            if kind == "decode":
                reqs = [r for r in reqs if self.len[r] + 1 <= fam.capacity]
                if reqs:
                    self.decode(reqs)
            elif kind == "multi":
                T = rnd.choice(MULTI_T)
                reqs = [r for r in reqs if self.len[r] + T <= fam.capacity]
                if reqs:
                    self.multi(reqs, T, [rnd.randint(1, T) for _ in reqs])
            elif kind == "rollback":
                self.rollback(reqs, [rnd.randint(0, min(self.len[r], fam.page + 2)) for r in reqs])
            else:
                reqs = [r for r in reqs if self.len[r] + 1 <= fam.capacity]
                if reqs:
                    self.cont(reqs, [rnd.randint(1, min(fam.capacity - self.len[r], 2 * fam.page + 2)) for r in reqs])


def build_schedule(fam, T=5, seed=None):
    """The scripted life: every item of COVERAGE_ITEMS by construction, with multi-token steps of T tokens.  seed: the same life
    with random valid steps between its blocks (a seeded random schedule; the blocks re-establish the lengths they need)."""
    P = fam.page
    s = Script(fam, None if seed is None else random.Random(seed))
    s.prefill(["a", "b", "c"], [P - 1, 2 * P, P + 3])
    s.register("d")                              # registered at length 0 and decoded
    s.decode(["a", "b", "c", "d"], 14)           # one below a multiple (a), a multiple (b), the ring three times round
    s.decode(["d", "c", "b", "a"])               # the same requests in another order
    s.decode(["b", "a", "c", "d"])
    s.noise(8)
    s.free("a")                                  # a's pages go to whoever asks next, b / c / d stay live
    s.room(["b", "c", "d"], 4)
    s.decode(["b", "c", "d"])                    # the batch shrinks ...
    s.prefill(["e"], [2 * P - 2])
    s.decode(["b", "c", "d", "e"])               # ... and grows
    s.decode(["b", "c", "e"])
    s.prefill(["f"], [3])
    s.decode(["b", "c", "f"])                    # the same size with another set of requests
    s.noise(8)
    s.room(["b"], 2 * T + 8)
    s.to("b", s.len["b"] // P * P + 2)           # b stays off the page multiples, so that only d's pages change below
    s.to("d", P - 2)
    s.decode(["d", "b"])                         # the device table now holds [d, b]; d: P - 1
    s.multi(["d", "b"], T, [T, T])               # d takes a page and keeps it, nobody gives one back
    s.decode(["d", "b"])
    s.to("d", P - 1)
    s.multi(["d", "b"], T, [1, T])               # d takes a page and gives it back
    s.decode(["d", "b"])
    s.noise(8)
    s.room(["b"], 8)
    s.to("b", s.len["b"] // P * P + 5)
    s.to("d", P + 2)
    s.decode(["d", "b"])
    s.rollback(["d", "b"], [6, 0])               # d returns a page ...
    s.decode(["d", "b"])                         # ... and the same batch decodes on
    s.to("d", 4)
    s.rollback(["d", "b"], [1, 1])               # nobody returns a page
    s.decode(["d", "b"])
    s.cont(["d"], [2])                           # a continued prefill inside the last page: the device table stays valid
    s.decode(["d", "b"])
    s.noise(8)
    s.to("f", 4)
    s.decode(["f"])
    s.cont(["f"], [2 * P + 1])                   # a continued prefill that takes two pages
    s.decode(["f"])
    s.free("e")
    s.free("f")
    s.prefill(["g"], [fam.capacity - P - 2])
    for _ in range(4):                           # page traffic: a's and e's pages come round to g and h
        s.to("g", 3)
        s.to("g", fam.capacity - P - 2)
    s.noise(8)
    s.free("c")
    s.prefill(["h"], [fam.capacity - 3])
    s.decode(["h", "g", "d"], 3)                 # h up to its capacity
    s.rollback(["h"], [2 * P])
    s.decode(["g", "h", "d"])
    s.noise(8)
    return s.steps


def captured_stretch(fam):
    """A stretch of single-token steps at batch size 2 for a captured step, with the three events a graph must survive: a page
    crossing (a, at 3 * page), a change of membership in which the newcomer d gets pages the leaver b freed (fillers drain the
    free-list queue in front of them), and a reorder.  Returns (steps, index of the step that frees b, index of d's prefill)."""
    P = fam.page
    s = Script(fam)
    s.prefill(["a", "b"], [3 * P - 3, 3 * P + 2])
    s.decode(["a", "b"], 5)
    free_b = len(s.steps)
    s.free("b")
    front, fillers = fam.num_blocks - 8, []  # a and b hold 4 pages each
    while front > 0:
        fillers.append(f"z{len(fillers)}")
        s.prefill([fillers[-1]], [min(front, fam.max_blocks) * P])
        front -= min(front, fam.max_blocks)
    admit_d = len(s.steps)
    s.prefill(["d"], [P + 1])
    for z in fillers:
        s.free(z)
    s.decode(["a", "d"], 2)
    s.decode(["d", "a"], 2)
    s.decode(["a", "d"])
    return s.steps, free_b, admit_d


COVERAGE_ITEMS = (
    "page freed by one request and taken by another while others stay live",
    "single-token step at a multiple of the page",
    "single-token step one below a multiple of the page",
    "request registered at length 0 and decoded",
    "multi-token step takes a page and gives it back",
    "multi-token step takes a page and keeps it",
    "rollback returns a page, then a single-token step on the same batch",
    "rollback returns no page",
    "continued prefill inside the last page",
    "continued prefill takes two or more pages",
    "same batch size, different set of requests",
    "same set of requests in another order",
    "batch shrinks and grows",
    "3 * _STAGE_RING consecutive single-token steps",
)
from chitu_amd.cache_manager import _STAGE_RING as STAGE_RING  # noqa: E402


def coverage(schedule, fam):
    """The COVERAGE_ITEMS a schedule contains, from the lengths alone.  Page reuse is inferred: the manager's free list is a
    queue of num_blocks pages, so the pages a request frees have all been handed out again once num_blocks pages were taken
    after the free (the host suite checks on the real block tables that this happened)."""
    P = fam.page
    pages = lambda n: -(-n // P)
    cache, have = PlainCache(), set()
    L = cache.length
    taken_since_free, registered0, run = [], set(), 0
    last_single, after_rollback, sizes = None, None, []

    def took(n):
        for i in range(len(taken_since_free)):
            taken_since_free[i] += n
        if any(t >= fam.num_blocks for t in taken_since_free):
            have.add(COVERAGE_ITEMS[0])

    for st in schedule:
        kind = st[0]
        run = run + 1 if kind == "decode" else 0
        if run >= 3 * STAGE_RING:
            have.add(COVERAGE_ITEMS[13])
        if kind == "prefill":
            for r, n in zip(st[1], st[2]):
                cache.inc[r] = len(cache.inc)
                cache.admit(r, cache.inc[r], n)
                took(pages(n))
        elif kind == "register":
            cache.inc[st[1]] = len(cache.inc)
            cache.admit(st[1], cache.inc[st[1]], 0)
            registered0.add(st[1])
        elif kind == "decode":
            reqs = st[1]
            for r in reqs:
                if L(r) % P == 0:
                    took(1)
                    if L(r) > 0:
                        have.add(COVERAGE_ITEMS[1])
                if L(r) % P == P - 1:
                    have.add(COVERAGE_ITEMS[2])
                if L(r) == 0 and r in registered0:
                    have.add(COVERAGE_ITEMS[3])
            if after_rollback == reqs:
                have.add(COVERAGE_ITEMS[6])
            if last_single is not None:
                if len(last_single) == len(reqs) and set(last_single) != set(reqs):
                    have.add(COVERAGE_ITEMS[10])
                if set(last_single) == set(reqs) and last_single != reqs:
                    have.add(COVERAGE_ITEMS[11])
            sizes.append(len(reqs))
            last_single = reqs
            for r in reqs:
                cache.append(r)
        elif kind == "multi":
            _, reqs, T, acc = st
            for r, a in zip(reqs, acc):
                grown = pages(L(r) + T) - pages(L(r))
                took(grown)
                if grown and pages(L(r) + a) < pages(L(r) + T):
                    have.add(COVERAGE_ITEMS[4])
                if pages(L(r) + a) > pages(L(r)):
                    have.add(COVERAGE_ITEMS[5])
                cache.append(r, a)
        elif kind == "rollback":
            back = [pages(L(r)) - pages(L(r) - d) for r, d in zip(st[1], st[2])]
            if not any(back):
                have.add(COVERAGE_ITEMS[7])
            for r, d in zip(st[1], st[2]):
                cache.drop(r, d)
        elif kind == "continue":
            grown = [pages(L(r) + c) - pages(L(r)) for r, c in zip(st[1], st[2])]
            took(sum(grown))
            if not any(grown):
                have.add(COVERAGE_ITEMS[8])
            if max(grown) >= 2:
                have.add(COVERAGE_ITEMS[9])
            for r, c in zip(st[1], st[2]):
                cache.append(r, c)
        elif kind == "free":
            cache.free(st[1])
            if cache.rows:
                taken_since_free.append(0)
        after_rollback = st[1] if kind == "rollback" and any(back) else None
    if any(a > b for a, b in zip(sizes, sizes[1:])) and any(a < b for a, b in zip(sizes, sizes[1:])):
        have.add(COVERAGE_ITEMS[12])
    assert len(cache.inc) <= MAX_INCARNATIONS, "2 * incarnation + layer must fit identity_rows' 16-value digit"
    return have


SCHEDULES = {}  # (family, name) -> steps
for _fam in FAMILIES.values():
    for _T in MULTI_T:
        SCHEDULES[_fam.name, f"scripted-T{_T}"] = build_schedule(_fam, _T)
    for _seed in (1, 2):
        SCHEDULES[_fam.name, f"random-{_seed}"] = build_schedule(_fam, MULTI_T[_seed % 3], seed=_seed)
for (_f, _n), _steps in SCHEDULES.items():
    _missing = [i for i in COVERAGE_ITEMS if i not in coverage(_steps, FAMILIES[_f])]
    assert not _missing, (_f, _n, _missing)
    assert len(_steps) <= 200, (_f, _n, len(_steps))
SCHEDULE_NAMES = sorted({n for _, n in SCHEDULES})


# ---------------------------------------------------------------- the driver
class Driver:
    """Runs schedule steps against one PagedKVCacheManager and checks it against PlainCache after every manager call.  The
    writes are plain indexing (ops.append_to_paged_kv_cache's contract) and the manager's own scatters; a subclass replaces
    append / to_cache / from_cache by the launches and hooks its attention checks into attend_*."""

    def __init__(self, fam, fmt, device="cpu"):
        from chitu_amd import cache_manager as cm

        self.fam, self.fmt, self.cm, self.device = fam, fmt, cm, torch.device(device)
        kw = dict(num_hot_req=HOT, block_size=fam.page, max_seq_len=fam.max_seq_len, device=device)
        if fam.name == "gqa":
            shape, dtype = cm.gqa_kv_layout(fmt, fam.kv_heads)
            self.mgr = cm.PagedKVCacheManager(0, LAYERS, k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype, **kw)
        else:
            shape, dtype = cm.mla_kv_layout(fmt)
            self.mgr = cm.PagedKVCacheManager(0, LAYERS, kv_shape_per_sample=shape, dtype=dtype, **kw)
        assert (self.mgr.max_blocks_per_req, self.mgr.num_blocks) == (fam.max_blocks, fam.num_blocks)
        self.plain = PlainCache()
        self.step_no, self.reused, self.owners, self._expect = 0, False, {}, {}
        self.skipped_copies = 0

    # ---- what a subclass replaces
    def to_cache(self, t):
        """bf16 rows -> rows of the cache's dtype"""
        if self.fmt == "bf16":
            return t
        return g8.quant_ref(t) if self.fam.name == "gqa" else m8.quant_ref(t)

    def from_cache(self, t):
        if self.fmt == "bf16":
            return t
        return g8.dequant_ref(t) if self.fam.name == "gqa" else m8.dequant_ref(t)

    def append(self, layer, table, pos, new):
        """cache[table[i][pos[i] // page]][pos[i] % page] = new[i]"""
        P = self.fam.page
        p = pos.long()
        idx = table.long()[torch.arange(p.numel(), device=p.device), p // P] * P + p % P
        self.poke(layer, idx, new)

    def attend_single(self, layer, reqs):
        pass

    def attend_multi(self, layer, reqs, T, written):
        pass

    def attend_continue(self, layer, reqs, counts, written):
        pass

    # ---- plumbing
    def caches(self, layer):
        c = self.mgr.get_paged_kv_cache(layer)
        return c if isinstance(c, tuple) else (c,)

    def dev(self, new):
        return tuple(t.to(self.device) for t in new)

    def poke(self, layer, idx, new):
        for c, t in zip(self.caches(layer), new):
            c.view(-1, *c.shape[2:])[idx] = self.to_cache(t)

    def bait(self, reqs):
        """an attractive row at position len of every request whose last page has room: its own code, another incarnation's V"""
        P = self.fam.page
        hit = [r for r in reqs if self.plain.length(r) % P and self.plain.length(r) < self.fam.capacity]
        if not hit:
            return
        idx = torch.tensor([self.mgr.block_table[r][self.plain.length(r) // P] * P + self.plain.length(r) % P for r in hit],
                           device=self.device)
        for layer in range(LAYERS):
            new = [rows(self.fam, self.plain.incarnation(r), layer, [self.plain.length(r)],
                        v_inc=(self.plain.incarnation(r) + 1) % MAX_INCARNATIONS) for r in hit]
            self.poke(layer, idx, self.dev(tuple(torch.cat(t) for t in zip(*new))))

    def expected(self, inc, layer):
        """all rows of (inc, layer) on the device, bf16"""
        if (inc, layer) not in self._expect:
            self._expect[inc, layer] = self.dev(rows(self.fam, inc, layer, range(self.fam.capacity)))
        return self._expect[inc, layer]

    def new_rows(self, reqs, layer, starts, counts, good=None):
        """the rows of a step, request by request; good[b]: how many of request b's rows keep their own V (the others are drafts
        that will be rejected: another incarnation's V)"""
        out = []
        for b, (r, s, c) in enumerate(zip(reqs, starts, counts)):
            inc = self.plain.incarnation(r)
            g = c if good is None else good[b]
            out.append(rows(self.fam, inc, layer, range(s, s + g)))
            if g < c:
                out.append(rows(self.fam, inc, layer, range(s + g, s + c), v_inc=(inc + 1) % MAX_INCARNATIONS))
        return self.dev(tuple(torch.cat(t) for t in zip(*out)))

    # ---- checks
    def check_pages(self, what, pending=None):
        mgr, P = self.mgr, self.fam.page
        pending = pending or {}
        owned = [p for ids in mgr.block_table.values() for p in ids]
        free = list(mgr.free_blocks)
        assert len(set(owned)) == len(owned), f"{what}: a page is owned twice: {sorted(p for p in set(owned) if owned.count(p) > 1)}"
        assert len(set(free)) == len(free), f"{what}: a page is twice in the free list"
        assert not set(owned) & set(free), f"{what}: pages {sorted(set(owned) & set(free))} are owned and free"
        assert len(owned) + len(free) == mgr.num_blocks, f"{what}: {len(owned)} owned + {len(free)} free pages of {mgr.num_blocks}"
        assert all(0 <= p < mgr.num_blocks for p in owned + free)
        assert set(mgr.block_table) == set(self.plain.rows) == set(mgr.seq_lens), f"{what}: live requests differ from the oracle's"
        for r, ids in mgr.block_table.items():
            n = self.plain.length(r)
            assert mgr.seq_lens[r] == n, f"{what}: request {r!r} has length {mgr.seq_lens[r]}, the oracle {n}"
            want = -(-(n + pending.get(r, 0)) // P)
            assert len(ids) == want, f"{what}: request {r!r} owns {len(ids)} pages for {n} + {pending.get(r, 0)} rows, not {want}"
            for p in ids:  # page reuse across incarnations, observed
                inc = self.plain.incarnation(r)
                if self.owners.get(p, inc) != inc and len(mgr.block_table) > 1:
                    self.reused = True
                self.owners[p] = inc

    def want_table(self, reqs, repeat=1):
        t = torch.zeros(len(reqs) * repeat, self.mgr.max_blocks_per_req, dtype=torch.int32)
        for b, r in enumerate(reqs):
            ids = self.mgr.block_table[r]
            t[b * repeat : (b + 1) * repeat, : len(ids)] = torch.tensor(ids, dtype=torch.int32)
        return t

    def same(self, what, got, want):
        got = got.cpu()
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, tuple(got.shape), tuple(want.shape))
        assert torch.equal(got, want), f"{what} (step {self.step_no}): device {got.tolist()} != oracle {want.tolist()}"

    def check_rows(self, what, tables=None):
        """every live request's rows below its length, gathered through the device table where the step has one (tables:
        request -> device table row), else through the host block_table, against the oracle's: torch.equal"""
        P = self.fam.page
        for r in self.plain.rows:
            n = self.plain.length(r)
            if n == 0:
                continue
            if tables is not None and r in tables:
                row = tables[r].long()
            else:
                row = torch.tensor(self.mgr.block_table[r], dtype=torch.int64, device=self.device)
            pos = torch.arange(n, device=self.device)
            idx = row[pos // P] * P + pos % P
            for layer in range(LAYERS):
                want = self.expected(self.plain.incarnation(r), layer)
                for i, (c, w) in enumerate(zip(self.caches(layer), want)):
                    got = self.from_cache(c.view(-1, *c.shape[2:])[idx].contiguous())
                    if not torch.equal(got, w[:n]):
                        bad = (got != w[:n]).flatten(1).any(1).nonzero().flatten().tolist()
                        raise AssertionError(f"{what} (step {self.step_no}): request {r!r} layer {layer} cache {i}: rows {bad[:8]} of "
                                             f"{n} are not the oracle's")

    # ---- the steps
    def admit(self, req, n):
        assert len(self.plain.inc) < MAX_INCARNATIONS
        self.plain.inc[req] = len(self.plain.inc)
        self.plain.admit(req, self.plain.inc[req], n)

    def run(self, schedule):
        for st in schedule:
            self.step(st)

    def step(self, st):
        getattr(self, "do_" + st[0])(*st[1:])
        self.step_no += 1

    def do_prefill(self, reqs, lens):
        mgr, varlen = self.mgr, Lens(lens)
        for r, n in zip(reqs, lens):
            self.admit(r, n)
        for layer in range(LAYERS):
            new = self.new_rows(reqs, layer, [0] * len(reqs), lens)
            kv = [self.to_cache(t) for t in new]
            mgr.finalize_cache_bylayer_prefill(kv[0], kv[-1], reqs, varlen, layer)
            self.check_pages(f"finalize_cache_bylayer_prefill layer {layer}")
        mgr.finalize_cache_all_prefill(reqs, varlen)
        self.check_pages("finalize_cache_all_prefill")
        self.check_rows("prefill")
        self.bait(reqs)

    def do_register(self, req, n):
        self.admit(req, n)
        self.mgr.register_sequence(req, n)
        self.check_pages("register_sequence")

    def do_free(self, req):
        self.plain.free(req)
        self.mgr.finalize_cache_all_decode(req)
        self.check_pages("finalize_cache_all_decode")
        self.check_rows("after a request left")

    def check_single_buffers(self, reqs, what):
        mgr = self.mgr
        lens = torch.tensor([self.plain.length(r) for r in reqs], dtype=torch.int32)
        self.same(f"{what}: get_gpu_seq_lens_excl_this_decode", mgr.get_gpu_seq_lens_excl_this_decode(), lens)
        self.same(f"{what}: get_gpu_seq_lens_incl_this_decode", mgr.get_gpu_seq_lens_incl_this_decode(), lens + 1)
        self.same(f"{what}: get_gpu_block_table", mgr.get_gpu_block_table(), self.want_table(reqs))

    def do_decode(self, reqs):
        mgr = self.mgr
        mgr.prepare_cache_decode(reqs)
        self.check_pages("prepare_cache_decode")
        slot = mgr._stage_next["table"]
        mgr.prepare_block_table_for_decode(reqs)
        self.skipped_copies += mgr._stage_next["table"] == slot
        self.check_pages("prepare_block_table_for_decode", {r: 1 for r in reqs})
        self.check_single_buffers(reqs, "single-token step")
        starts = [self.plain.length(r) for r in reqs]
        written = []
        for layer in range(LAYERS):
            new = self.new_rows(reqs, layer, starts, [1] * len(reqs))
            written.append(new)
            self.write_single(layer, reqs, new)
        for r in reqs:
            self.plain.append(r)
        self.bait(reqs)
        for layer in range(LAYERS):
            self.attend_single(layer, reqs)
        mgr.finalize_cache_single_decode(reqs)
        self.check_pages("finalize_cache_single_decode")
        self.check_rows("single-token step", dict(zip(reqs, mgr.get_gpu_block_table())))

    def write_single(self, layer, reqs, new):
        self.append(layer, self.mgr.get_gpu_block_table(), self.mgr.get_gpu_seq_lens_excl_this_decode(), new)

    def do_multi(self, reqs, T, acc):
        mgr, n = self.mgr, len(reqs)
        mgr.prepare_block_table_for_decode_multi(reqs, T)
        self.check_pages("prepare_block_table_for_decode_multi", {r: T for r in reqs})
        starts = [self.plain.length(r) for r in reqs]
        row_lens = torch.tensor([s + t for s in starts for t in range(T)], dtype=torch.int32)
        self.same("multi-token step: get_gpu_multi_row_lens", mgr.get_gpu_multi_row_lens(), row_lens)
        self.same("multi-token step: get_gpu_multi_row_lens_incl", mgr.get_gpu_multi_row_lens_incl(), row_lens + 1)
        self.same("multi-token step: get_gpu_multi_seq_lens_incl", mgr.get_gpu_multi_seq_lens_incl(),
                  torch.tensor([s + T for s in starts], dtype=torch.int32))
        self.same("multi-token step: get_gpu_multi_block_table", mgr.get_gpu_multi_block_table(), self.want_table(reqs, T))
        written = []
        for layer in range(LAYERS):
            new = self.new_rows(reqs, layer, starts, [T] * n, good=acc)
            written.append(new)
            self.append(layer, mgr.get_gpu_multi_block_table(), mgr.get_gpu_multi_row_lens(), new)
        for layer in range(LAYERS):
            self.attend_multi(layer, reqs, T, written[layer])
        for r, a in zip(reqs, acc):
            self.plain.append(r, a)
        mgr.finalize_cache_multi_decode(reqs, acc)
        self.check_pages("finalize_cache_multi_decode")
        self.check_rows("multi-token step", dict(zip(reqs, mgr.get_gpu_multi_block_table()[::T])))

    def do_rollback(self, reqs, drops):
        for r, d in zip(reqs, drops):
            self.plain.drop(r, d)
        self.mgr.rollback(reqs, drops)
        self.check_pages("rollback")
        self.check_rows("rollback")

    def do_continue(self, reqs, counts):
        mgr = self.mgr
        mgr.prepare_cache_prefill_continue(reqs, Lens(counts))
        self.check_pages("prepare_cache_prefill_continue", dict(zip(reqs, counts)))
        starts = [self.plain.length(r) for r in reqs]
        self.same("continued prefill: get_continue_position_ids", mgr.get_continue_position_ids(),
                  torch.tensor([s + t for s, c in zip(starts, counts) for t in range(c)], dtype=torch.int64))
        self.same("continued prefill: get_gpu_continue_seq_lens_incl", mgr.get_gpu_continue_seq_lens_incl(),
                  torch.tensor([s + c for s, c in zip(starts, counts)], dtype=torch.int32))
        self.same("continued prefill: get_gpu_continue_block_table", mgr.get_gpu_continue_block_table(), self.want_table(reqs))
        written = []
        for layer in range(LAYERS):
            new = self.new_rows(reqs, layer, starts, counts)
            written.append(new)
            kv = [self.to_cache(t) for t in new]
            mgr.finalize_cache_bylayer_prefill_continue(kv[0], kv[-1], layer)
        tables = dict(zip(reqs, mgr.get_gpu_continue_block_table()))
        for r, c in zip(reqs, counts):
            self.plain.append(r, c)
        self.bait(reqs)
        for layer in range(LAYERS):
            self.attend_continue(layer, reqs, counts, written[layer])
        mgr.finalize_cache_all_prefill_continue(reqs)
        self.check_pages("finalize_cache_all_prefill_continue")
        self.check_rows("continued prefill", tables)


def single_probes(n, page):
    """the keys a single-token step probes in a sequence of n keys: key 0, the key just appended, the first key of the last page,
    the last key of the page before (key 0 where there is none) -- and None: the forbidden row at position n"""
    first = (n - 1) // page * page
    return [0, n - 1, first, max(first - 1, 0), None]
