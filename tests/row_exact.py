"""Builders and CPU oracles for the row kernels: norms, quantisers, RoPE, paged appends, gather, moe_sum, SiLU (no GPU needed).

The kernels of norm.hip / norm_common.h, quant.hip, kv.hip / mla_kv_row.h, the activation quantiser of w8a8_int8.hip and
moe_sum run between the GEMMs on every layer.  Each oracle here is a plain statement of one of them in which every rounding
is written out, on data for which no free choice of the kernel (summation order, FMA contraction) changes a bit:

  RMSNorm      rows of integers times one power of two per row: the sum of squares is exact in fp32 in any order (the
               builder asserts dim * max^2 < 2^24, it never measures).  mean = ss / dim, t = mean + eps, rr = 1/sqrt(t), each
               rounded to fp32, y = bf16((v rr) w).  The device rsqrtf is not correctly rounded: the oracle gives one
               expected row per candidate rr (the correctly rounded value and its RSQRT_RADIUS fp32 neighbours on each
               side) and a kernel's WHOLE row must equal one of them.
  quantisers   oracle/fp8.py (IEEE division, round-to-nearest-even) and quant_int8 here, on a table of adversarial groups.
  RoPE ...     fp32 statements of the kernel headers: products rounded separately, one add, one rounding to the type.
  SiLU         bf16(g / (1 + e)) in fp32 for every candidate e of expf(-g), then one bf16 rounding of the exact product.

tests/test_row_exact_host.py checks all of this on the CPU (against torch, float64 and wrong variants of each oracle);
tests/test_gpu_row_exact.py runs the kernels.  The shape lists of both live here.
"""

import functools

import numpy as np
import torch

from oracle import fp8 as ofp8
from tests.dense_exact import G, SENTINEL16, SENTINEL32, ints

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = {"f32": F32, "bf16": BF16, "f16": F16}
DT_CODE = {"bf16": 0, "f16": 1, "f32": 2}
CODE_SENTINEL = 0x7F  # pre-fill of fp8 code outputs (the e4m3fn NaN) ...
INT8_SENTINEL = 0x55  # ... and of int8 code outputs

# Candidate radii, in fp32 ulps around the correctly rounded value.  No accuracy table of the device library ships with the
# toolchain (neither the ISA text nor the device-library documentation is installed), so both start at the +-1 ulp that the
# HIP programming guide's table of device math functions states for rsqrtf and expf.
RSQRT_RADIUS = 1
EXPF_RADIUS = 1


# ---------------------------------------------------------------- guarded buffers
class Guarded:
    """A [rows, cols] output inside a [rows + 2 G, stride] buffer of sentinels: G guard rows on each side, stride - cols guard
    columns at the end of every row, the output itself pre-filled with the sentinel too.  `view` is what the kernel gets
    (row stride `stride`)."""

    def __init__(self, rows, cols, dtype, stride=None, device="cuda", sentinel=None):
        self.rows, self.cols, self.dtype, self.stride = rows, cols, dtype, stride or cols
        if dtype in (torch.uint8, torch.int8):
            self.raw, self.sentinel = torch.uint8, CODE_SENTINEL if sentinel is None else sentinel
        elif dtype == F32:
            self.raw, self.sentinel = torch.int32, SENTINEL32
        else:
            self.raw, self.sentinel = torch.int16, SENTINEL16
        self.full = torch.full((rows + 2 * G, self.stride), self.sentinel, dtype=self.raw, device=device)
        self.view = self.full[G:G + rows, :cols]

    def check(self, what, written=True):
        """Guards untouched; with written, no interior element still the sentinel (pass False for code outputs, whose every
        byte value is a legitimate code: there the comparison with the oracle is the check).  Returns the interior (CPU) in
        the output's own dtype."""
        got = self.full.cpu()
        outside = torch.ones_like(got, dtype=torch.bool)
        outside[G:G + self.rows, :self.cols] = False
        touched = ((got != self.sentinel) & outside).nonzero()
        assert len(touched) == 0, (f"{what}: stored outside the output, first (buffer row - G, col): "
                                   f"{[(int(r) - G, int(c)) for r, c in touched[:8]]}")
        inner = got[G:G + self.rows, :self.cols].contiguous()
        if written:
            left = (inner == self.sentinel).nonzero()
            assert len(left) == 0, f"{what}: {len(left)} output elements never written, first (row, col): {left[:8].tolist()}"
        return inner.view(self.dtype)

    def untouched(self, what):
        got = self.full.cpu()
        touched = (got != self.sentinel).nonzero()
        assert len(touched) == 0, f"{what}: output touched, first (buffer row - G, col): {[(int(r) - G, int(c)) for r, c in touched[:8]]}"


def bits(t):
    """Integer view of a tensor's bit patterns (NaN payloads included)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def canon_nan(t):
    """Bit view with every NaN mapped to one pattern: "NaN results compare as NaN"."""
    if t.dtype == torch.float8_e4m3fn or t.dtype == torch.uint8:
        b = t.contiguous().view(torch.uint8)
        return torch.where((b & 0x7F) == 0x7F, torch.full_like(b, 0x7F), b)
    b = bits(t).clone()
    if not t.is_floating_point():
        return b
    b[torch.isnan(t)] = {2: SENTINEL16, 4: SENTINEL32}[t.element_size()]
    return b


def assert_same(got, want, what, nan_ok=False):
    """Bit equality, every difference reported with its row and column."""
    g2, w2 = (canon_nan(got), canon_nan(want)) if nan_ok else (bits(got), bits(want))
    assert g2.shape == w2.shape, (what, g2.shape, w2.shape)
    if torch.equal(g2, w2):
        return
    g2, w2 = g2.reshape(-1, g2.shape[-1]), w2.reshape(-1, w2.shape[-1])
    bad = (g2 != w2).nonzero()
    gf, wf = got.reshape(g2.shape), want.reshape(w2.shape)
    raise AssertionError(f"{what}: {len(bad)} of {g2.numel()} elements differ in {len(set(bad[:, 0].tolist()))} rows; first (row, col, got, want): "
                         f"{[(int(r), int(c), float(gf[r, c].float()), float(wf[r, c].float())) for r, c in bad[:6]]}")


# ---------------------------------------------------------------- RMSNorm
EPS = 1e-6
ROW_EXPS = [-20, -10, 0, 10, 20]


def next_f32(x, direction):
    return torch.from_numpy(np.nextafter(x.numpy(), np.float32(direction)))


def rr_candidates(t, radius=RSQRT_RADIUS):
    """[2 radius + 1, rows] fp32: candidate 0 is 1/sqrt(t) from float64 rounded once; 2 k - 1 / 2 k are k ulps below / above."""
    rr = (1.0 / t.double().sqrt()).float()
    out, lo, hi = [rr], rr, rr
    for _ in range(radius):
        lo, hi = next_f32(lo, 0.0), next_f32(hi, np.inf)
        out += [lo, hi]
    return torch.stack(out)


def rms_t(v, dim=None, eps=EPS, ss=None):
    """t = fl(fl(ss / dim) + eps) of bf16 rows v [rows, dim]; ss exact (float64 of exactly representable squares)."""
    if ss is None:
        ss = (v.double() ** 2).sum(-1)
    ss32 = ss.float()
    assert torch.equal(ss32.double(), ss), "the sum of squares is not an fp32 number: the builder's bound is wrong"
    return ss32 / torch.tensor(float(dim or v.shape[-1]), dtype=F32) + torch.tensor(eps, dtype=F32)


def rms_rows(v, w, rr):
    """y = bf16((v rr) w): two fp32 roundings, one bf16 rounding.  rr [rows]."""
    return ((v.float() * rr[:, None]) * w.float()[None, :]).to(BF16)


def rms_oracle(v, w, eps=EPS, radius=RSQRT_RADIUS):
    """(t [rows], rr [C, rows], y [C, rows, dim] bf16)."""
    t = rms_t(v, eps=eps)
    rr = rr_candidates(t, radius)
    return t, rr, torch.stack([rms_rows(v, w, r) for r in rr])


def match_rows(got, t, rr, y, what):
    """Every row of got equals one candidate row as a whole; returns the candidate index per row.  A row that matches none is
    reported with its t, the candidates and its first differences from the central one."""
    gb, yb = bits(got), bits(y)
    hit = (gb[None] == yb).all(-1)  # [C, rows]
    idx = torch.where(hit.any(0), hit.float().argmax(0), torch.full((got.shape[0],), -1))
    for r in (idx < 0).nonzero().flatten().tolist():
        cols = (gb[r] != yb[0, r]).nonzero().flatten()[:4].tolist()
        raise AssertionError(
            f"{what}: row {r} equals no candidate row: t = {float(t[r])!r}, rr candidates {[float(c[r]) for c in rr]}; "
            f"{int((gb[r] != yb[0, r]).sum())} elements differ from the central row, first (col, got, want): "
            f"{[(c, float(got[r, c]), float(y[0, r, c])) for c in cols]}")
    return idx


def rms_limit(dim, terms=0):
    """Largest |integer| per input value such that the normalised row (x, or x + the sum of `terms` add rows) stays below
    the exactness bound dim * max^2 < 2^24 and inside bf16's 8 significant bits."""
    lim = 15
    while lim > 1 and (dim * (lim * (terms + 1)) ** 2 >= 2 ** 24 or lim * (terms + 1) > 255):
        lim -= 1
    assert dim * (lim * (terms + 1)) ** 2 < 2 ** 24 and lim * (terms + 1) <= 255, (dim, terms)
    return lim


@functools.lru_cache(maxsize=128)
def rms_case(rows, dim, terms=0, seed=0):
    """x [rows, dim] bf16 (integers -lim..lim times 2^e, e per row cycling through ROW_EXPS from a row-dependent start), `terms`
    add rows [rows, terms, dim] of the same kind and exponent, w [dim] random bf16 with full mantissas, and v = the row that
    is normalised: bf16(x + bf16(sum of the terms in order)) -- all exact, so v is simply the integer sum."""
    g = torch.Generator().manual_seed(1000003 * rows + 1009 * dim + 17 * terms + seed)
    lim = rms_limit(dim, terms)
    e = torch.tensor([ROW_EXPS[(r + dim + seed) % len(ROW_EXPS)] for r in range(rows)])
    scale = torch.ldexp(torch.ones(rows), e.to(torch.int32))[:, None]
    xi = ints(g, lim, rows, dim)
    x = (xi.float() * scale).to(BF16)
    assert torch.equal(x.double(), xi.double() * scale.double())
    w = (torch.randn(dim, generator=g) * 0.5 + torch.sign(torch.randn(dim, generator=g))).to(BF16)
    out = dict(x=x, w=w, e=e, lim=lim)
    vi = xi
    if terms:
        ai = ints(g, lim, rows, terms, dim)
        add = (ai.float() * scale[:, None]).to(BF16)
        assert torch.equal(add.double(), ai.double() * scale[:, None].double())
        si = ai.sum(1)
        out.update(add=add, add_sum=(si.float() * scale).to(BF16))
        vi = xi + si
    assert int(vi.abs().max()) <= 255 and dim * int(vi.abs().max()) ** 2 < 2 ** 24  # bf16-exact, ss exact in fp32
    out["v"] = (vi.float() * scale).to(BF16)
    assert torch.equal(out["v"].double(), vi.double() * scale.double())
    return out


def sum_terms_oracle(add):
    """bf16(in-order fp32 sum of add[:, k, :]): chitu_hip_moe_sum's arithmetic, stated as a loop."""
    acc = torch.zeros(add.shape[0], add.shape[2], dtype=F32)
    for k in range(add.shape[1]):
        acc = acc + add[:, k].float()
    return acc.to(BF16)


def residual_oracle(x, add_row):
    return (x.float() + add_row.float()).to(BF16)


# ---------------------------------------------------------------- quantisers
def quant_fp8(x, mode, eps=1e-10):
    """mode 0: act_quant_deepseek_v3, mode 1: per_token_group_quant_fp8 (oracle/fp8.py)."""
    return ofp8.act_quant_deepseek_v3(x) if mode == 0 else ofp8.per_token_group_quant_fp8(x, eps=eps)


def quant_int8(x):
    """s = max(max|x|, 1e-5) / 127 per row, q = clamp(rint(x / s), -128, 127), fp32 throughout, round-half-even.
    = oracle/w8a8.py::quant_act (the reference's quant_act, verbatim) on finite rows.  NaN: the reference propagates a NaN
    through max() into the scale and then casts NaN to int8, which is undefined; the kernels' rule is stated instead: the
    maximum drops NaN (fmaxf) and clamp(rint(NaN)) = fmin(fmax(NaN, -128), 127) = -128."""
    xf = x.float()
    a = xf.abs()
    amax = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(-1, keepdim=True)
    s = torch.clamp(amax, min=1e-5) / torch.tensor(127.0)
    q = torch.round(xf / s)
    q = torch.clamp(torch.where(torch.isnan(q), torch.full_like(q, -128.0), q), -128.0, 127.0)
    return q.to(torch.int8), s.view(-1)


def e4m3_values():
    """The 127 non-negative finite e4m3fn values, ascending (codes 0x00..0x7E)."""
    return torch.arange(0, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).float()


def e4m3_midpoints():
    v = e4m3_values().double()
    return (v[:-1] + v[1:]) / 2  # 126 of them


def _find_above_448():
    """A bf16 group maximum a with fl(a / fl(a / 448)) > 448: the scale rounds down, the quotient of the maximum itself
    lands one ulp above 448."""
    cand = torch.arange(0x3F80, 0x4100, dtype=torch.int16).view(BF16).float()
    q = cand / (cand / np.float32(448.0))
    hit = cand[q > 448.0]
    assert len(hit) > 0
    return float(hit[0])


KINDS_16 = ["tie+", "normal", "zero", "tie-", "tiny", "normal", "normal", "nan", "normal", "huge", "normal", "inf+",
            "above", "tie+k3", "inf-", "normal", "tie-k-2", "zero", "normal", "above"]


@functools.lru_cache(maxsize=8)
def quant_table(dt):
    """(x [n_groups, 128] in the dtype, kinds): the adversarial groups, four to a 64-lane wave so that several kinds share a
    wave.  f16 has no exponent range for a scale outside 2^+-60: there "tiny" and "huge" are the smallest normal and the
    largest maximum the type can hold."""
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(77)
    mids, rows = e4m3_midpoints(), []
    wide = dt != "f16"
    for i, kind in enumerate(KINDS_16):
        if kind.startswith("tie"):
            k = {"tie+": 0, "tie-": 0, "tie+k3": 3, "tie-k-2": -2}[kind]
            sign = -1.0 if kind[3] == "-" else 1.0
            row = torch.cat([torch.tensor([448.0, -448.0], dtype=torch.float64), sign * mids]) * 2.0 ** k
            row = row[torch.randperm(128, generator=g)]
        elif kind == "zero":
            row = torch.zeros(128, dtype=torch.float64)
        elif kind in ("tiny", "huge"):
            k = (-70 if kind == "tiny" else 70) if wide else (-14 if kind == "tiny" else 7)
            row = ints(g, 7, 128).double() * 64 * 2.0 ** k
            row[5] = 448.0 * 2.0 ** k
        elif kind == "above":
            row = ints(g, 100, 128).double() / 128
            row[17], row[90] = _find_above_448(), -_find_above_448()
        else:
            row = ints(g, 120, 128).double() * 2.0 ** [-9, -3, 2, -6][i % 4]
            if kind == "nan":
                row[33] = float("nan")
            if kind.startswith("inf"):
                row[70] = float("inf") if kind == "inf+" else float("-inf")
        t = row.to(dtype)
        ok = torch.isnan(row) | (t.double() == row)
        assert bool(ok.all()), (dt, kind)  # every value, the midpoints included, is exact in the input type
        rows.append(t)
    x = torch.stack(rows)
    for lo in range(0, len(KINDS_16), 4):  # the groups of one wave
        wave = KINDS_16[lo:lo + 4]
        assert len(set(wave)) >= 3 and "normal" in wave
    if wide:
        s = x.float().abs().nan_to_num(0.0, 0.0, 0.0).amax(-1) / 448.0
        assert float(s[KINDS_16.index("tiny")]) < 2.0 ** -60 and float(s[KINDS_16.index("huge")]) > 2.0 ** 60
    return x, KINDS_16


def quant_big(dt, rows=4104, cols=1024):
    """More than 32 768 groups (2048 workgroups x 16 groups): the table tiled over the whole tensor, so that the second
    iteration of the stride loop sees every kind again at other lanes."""
    x, _ = quant_table(dt)
    n = rows * cols // 128
    assert n > 32768
    reps = (n + x.shape[0] + 2) // (x.shape[0] + 3)
    pad = torch.cat([x, x[1:4]])  # 23 groups: the period is odd, the kinds walk through the lanes
    return pad.repeat(reps, 1)[:n].reshape(rows, cols).contiguous()


def int8_row(K, dt, k=0, seed=0, special=True):
    """One row for the int8 quantiser: maximum 127 2^k (scale exactly 2^k), the ties (n + 1/2) 2^k in both signs, random
    integers and halves elsewhere; special: one NaN (which clamps at -128, see quant_int8)."""
    g = torch.Generator().manual_seed(K * 31 + seed)
    row = (ints(g, 253, K).double() / 2) * 2.0 ** k  # multiples of 1/2 up to 126.5: every odd one is a tie
    if K >= 2:
        row[K - 1] = 127.0 * 2.0 ** k
        if special and K >= 7:
            row[K // 2] = float("nan")
    t = row.to(DTYPES[dt])
    assert bool((torch.isnan(row) | (t.double() == row)).all())
    return t


# ---------------------------------------------------------------- to_tile_major with chosen padding
def to_tile_major(q, s, code_pad=CODE_SENTINEL, scale_pad_bits=SENTINEL32):
    """Row-major codes [M, K] uint8 / scales [M, K/128] -> (codes [t 16, K] uint8, scale bits [t, K/128, 16] int32) of the
    tile-major layout X[m / 16][K / 16][m % 16][16 B], XS[m / 16][K / 128][m % 16]; the padding rows of the last tile hold
    the given fill (the sentinels: the kernel must leave them alone)."""
    M, K = q.shape
    t = (M + 15) // 16
    qp = torch.full((t * 16, K), code_pad, dtype=torch.uint8)
    qp[:M] = q.view(torch.uint8)
    sp = torch.full((t * 16, K // 128), scale_pad_bits, dtype=torch.int32)
    sp[:M] = bits(s.float())
    qt = qp.view(t, 16, K // 16, 16).permute(0, 2, 1, 3).contiguous().view(t * 16, K)
    st = sp.view(t, 16, K // 128).permute(0, 2, 1).contiguous()
    return qt, st


# ---------------------------------------------------------------- RoPE, appends, gather, moe_sum
def rope_oracle(x, cos, sin, layout):
    """x [bs, heads, d] of any float type, cos / sin [bs, d/2] fp32.  layout 0: pairs (2i, 2i+1); 1: (i, i + d/2).
    o0 = fl(fl(x0 c) - fl(x1 s)), o1 = fl(fl(x1 c) + fl(x0 s)), one rounding to x's type."""
    xf = x.float()
    half = x.shape[-1] // 2
    c, s = cos[:, None, :], sin[:, None, :]
    x0, x1 = (xf[..., 0::2], xf[..., 1::2]) if layout == 0 else (xf[..., :half], xf[..., half:])
    p, q, r, t = x0 * c, x1 * s, x1 * c, x0 * s
    o0, o1 = (p - q).to(x.dtype), (r + t).to(x.dtype)
    out = torch.empty_like(x)
    if layout == 0:
        out[..., 0::2], out[..., 1::2] = o0, o1
    else:
        out[..., :half], out[..., half:] = o0, o1
    return out


def rope_inputs(bs, heads, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(bs, heads, d, generator=g) * 3).to(dtype)
    ang = torch.rand(bs, d // 2, generator=g) * 6.2831853
    return x, torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()


def live_row(b, lens, table, page, pages_per_seq, num_pages):
    """The page row index sequence b appends to, or None when the guard of the append kernels drops it."""
    L = int(lens[b])
    if L < 0 or L // page >= pages_per_seq:
        return None
    p = int(table[b, L // page])
    if p < 0 or p >= num_pages:
        return None
    return p * page + L % page


def append_oracle(cache_rows, new_rows, lens, table, page, num_pages):
    """cache_rows [num_pages * page, ...] -> a copy with new_rows[b] at every live sequence's row."""
    out = cache_rows.clone()
    for b in range(len(lens)):
        r = live_row(b, lens, table, page, table.shape[1], num_pages)
        if r is not None:
            out[r] = new_rows[b]
    return out


def paged_batch(B, page, seed, bad=False):
    """(lens, table [B + 1, pages_per_seq] with one padding row, num_pages told to the kernel, pages allocated): valid
    sequences at the first and last slot of a page and across pages; bad: sequences 1, 3, 4, 6 (B >= 8) or 1 and 2 (B = 4,
    two variants by seed parity) carry a negative length, a position beyond the table, a page id == num_pages and a page id of
    -1.  The pages allocated exceed num_pages by G at the end, and the caller hands the kernel a pointer G pages into its
    allocation: a kernel without the guard writes a guard page, nothing else."""
    g = torch.Generator().manual_seed(seed)
    per = 3
    num_pages = B * per + 2
    perm = torch.randperm(num_pages, generator=g)
    table = torch.full((B + 1, per), 0, dtype=torch.int32)
    table[:B] = perm[: B * per].view(B, per).to(torch.int32)
    table[B] = perm[:per].to(torch.int32)  # the padding row repeats valid ids
    slots = [0, page - 1, page, 2 * page - 1, 2 * page, 3 * page - 1, 1, page + 1]
    lens = torch.tensor([slots[(b + seed) % len(slots)] for b in range(B)], dtype=torch.int32)
    kinds = {}
    if bad:
        where = [1, 3, 4, 6] if B >= 8 else ([1, 2] if seed % 2 == 0 else [0, 3])
        what = ["neg", "beyond", "page=num_pages", "page=-1"] if B >= 8 else (["neg", "page=num_pages"] if seed % 2 == 0 else ["beyond", "page=-1"])
        for b, k in zip(where, what):
            kinds[b] = k
            if k == "neg":
                lens[b] = -1 - (page if b % 2 else 0)  # -1 and -1 - page: L / page truncates to 0 and to -1
            elif k == "beyond":
                lens[b] = per * page  # first position past the table: the padding row / next sequence's entry would be read
            elif k == "page=num_pages":
                table[b, int(lens[b]) // page] = num_pages
            else:
                table[b, int(lens[b]) // page] = -1
    return lens, table, num_pages, num_pages + G, kinds


def moe_sum_oracle(c3):
    """c3 [tokens, topk, N] bf16 -> bf16(sum_k float(c3[:, k])) with k ascending."""
    return sum_terms_oracle(c3)


def embed_gather_oracle(tokens, table, vocab_start, positions, cos_t, sin_t):
    local = tokens - vocab_start
    mine = (local >= 0) & (local < table.shape[0])
    h = torch.where(mine[:, None], table[local.clamp(0, table.shape[0] - 1)], torch.zeros((), dtype=table.dtype))
    pos = positions.long().clamp(0, cos_t.shape[0] - 1)
    return h, cos_t[pos], sin_t[pos]


# ---------------------------------------------------------------- fp8 weight dequant
def dequant_oracle(codes, scales, out_dtype):
    """y = fl(float(code) * s[m / 128][n / 128]) rounded once to the output type (oracle/fp8.py, NaN codes stay NaN)."""
    return ofp8.weight_dequant_deepseek_v3(codes.view(torch.float8_e4m3fn), scales, out_dtype)


# ---------------------------------------------------------------- SiLU
def expf_candidates(g, radius=EXPF_RADIUS):
    """[C, ...] fp32 candidates for expf(-g): the correctly rounded value, then k ulps below / above.  Where the correctly
    rounded value is infinite the lower neighbour is FLT_MAX only if the true value is within an ulp of it; where it is 0 or
    subnormal the neighbours do not matter (1 + e == 1)."""
    x = (-g.double()).exp()
    c = x.float()
    out, lo, hi = [c], c, c
    fmax = torch.tensor(np.finfo(np.float32).max)
    for _ in range(radius):
        lo2 = next_f32(lo, 0.0)
        lo = torch.where(torch.isinf(lo) & (x > fmax.double() * (1 + 2.0 ** -23)), lo, lo2)
        hi = next_f32(hi, np.inf)
        out += [lo, hi]
    return torch.stack(out)


def silu_factor(g, e):
    """bf16(fl(g / fl(1 + e))), g bf16 as float, e fp32."""
    return (g / (torch.tensor(1.0) + e)).to(BF16)


def silu_oracle(gate, up, radius=EXPF_RADIUS):
    """gate [rows] bf16 (one gate value per row), up [rows, d] bf16 -> [C, rows, d] bf16: for every expf candidate the
    factor bf16(g / (1 + e)) and then the single bf16 rounding of its exact product with up (a product of two bf16 numbers
    is exact in fp32, so one fp32 multiply and one rounding state it)."""
    g = gate.float()
    out = []
    for e in expf_candidates(g, radius):
        s = silu_factor(g, e).float()
        out.append((s[:, None] * up.float()).to(BF16))
    return torch.stack(out)


SILU_UPS_FIXED = [0.0, -0.0, 2.0 ** -133, -(2.0 ** -130), 3.3895313892515355e38, -3.3895313892515355e38, 1.0, -1.0]


@functools.lru_cache(maxsize=2)
def silu_case(d=136):
    """x [65536, 2 d] bf16: row r's gate half holds the bf16 bit pattern r in every column, its up half the fixed values
    (+-0, two subnormals, +-the largest finite value, +-1) and random full-mantissa values."""
    gate = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)  # wraps: bit pattern r
    g = torch.Generator().manual_seed(5)
    up_row = torch.cat([torch.tensor(SILU_UPS_FIXED, dtype=torch.float64).to(BF16),
                        (torch.randn(d - len(SILU_UPS_FIXED), generator=g) * 4).to(BF16)])
    shift = torch.ldexp(torch.ones(65536), (torch.arange(65536) % 9 - 4).to(torch.int32))
    up = (up_row.float()[None, :] * shift[:, None]).to(BF16)
    up[:, :len(SILU_UPS_FIXED)] = up_row[:len(SILU_UPS_FIXED)]
    x = torch.cat([gate[:, None].expand(65536, d), up], 1).contiguous()
    return gate, up, x


def silu_match(got, want, what):
    """Every row of got [rows, d] equals, NaN as NaN, one candidate row as a whole (one gate per row: the factor the kernel
    used).  Returns the candidate index per row."""
    gb, wb = canon_nan(got), torch.stack([canon_nan(w) for w in want])
    hit = (gb[None] == wb).all(-1)
    idx = torch.where(hit.any(0), hit.float().argmax(0), torch.full((got.shape[0],), -1))
    bad = (idx < 0).nonzero().flatten()
    if len(bad):
        r = int(bad[0])
        cols = (gb[r] != wb[0, r]).nonzero().flatten()[:4].tolist()
        raise AssertionError(f"{what}: {len(bad)} rows equal no candidate, first row {r}: first (col, got, central want): "
                             f"{[(c, float(got[r, c]), float(want[0, r, c])) for c in cols]}")
    return idx


# ---------------------------------------------------------------- the shapes of the GPU tests
A_DIMS = [8, 16, 120, 128, 136, 1000, 2040, 2048, 2056, 4096, 4104, 6144, 6152, 7168, 8184, 8192]
A_QDIMS = [128, 256, 2048, 2176, 4096, 4224, 6144, 6272, 8192]
A_ROWS = [1, 3]
B_TERM_DIMS = [136, 8192]
B_TILE_ROWS = [1, 15, 16, 17, 33]
B_INT8_DIMS = [8, 1000, 4096, 8192]
E_VEC_K = [8, 2048, 2056, 16384]
E_SCALAR_K = [1, 7, 1001, 16392]
APPEND_ROW_BYTES = [2, 17, 30, 1152]
J_TOPK = [1, 2, 9, 16]
