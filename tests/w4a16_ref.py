"""Builders and CPU references of the W4A16 g128 exact tests (include/chitu_hip_ext9.h): the grid, the data and the
expectations.  No GPU, no kernel.

Data: x integers in [-8, 8] (bf16); codes u over 0..15 with 0 and 15 in every row (code 0 widens to the signed byte -128, the
sign-extension edge) and every code at each of the 8 nibble positions of a dword.  Two kinds of scales:

  pow2       powers of two, distinct among the four scales of every (row pair, K step) block and between the w1 and w3 halves
             of a w13, so that a scale taken from the wrong row, group or half changes the result.  The builder asserts
                 sum_k |x (u - 8) s| / min s < 2^24 for every output:
             every partial sum in any order is then a multiple of min s below 2^24 min s, an exact fp32 number, and the
             kernel's accumulator IS the real product.  Exponents -2..2 up to K = 2304, {1/2, 1, 2} beyond.
  quantiser  arbitrary fp32 scales, as quant_weight_w4a16 produces them.  No summation order is assumed (the header fixes
             none).  With v the fp64 value, G = K / 128 and P_g the exact group sums,
                 rho = (G + 9) 2^-24 sum_g |s_g P_g|
             bounds the accumulator's distance from v: G fused multiply-adds, one add of the even and odd accumulators and at
             most 8 adds of the wave reduce, each rounding once (relative 2^-24) a partial sum of at most sum |terms| (the
             adds of different waves' accumulators count once together: their partial sums are disjoint).  The fp32
             accumulator lies in [v - rho, v + rho], so between the smallest fp32 number not below v - rho and the largest
             not above v + rho; the output lies between their roundings.  (v itself is an fp64 sum of exact products: its
             own error, G 2^-53 of the same sum, is 2^-29 of rho.)

The SiLU expectations run tests/silu_ref.py's chain over the scaled accumulators (pow2) or over the ends of their interval
(quantiser)."""
import functools
import itertools

import torch

from tests import silu_ref
from tests.w8a16_ref import instantiations  # noqa: F401  (the plan walk is the W8A16 suite's)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
GROUP = 128
MS = (1, 2, 15, 16, 17, 32, 33)  # both token tiles, the second 32-row launch
KS = (128, 256, 384, 640, 1024, 1152, 2048, 2176)  # 1, 1, 2, 3, 4, 5, 8, 9 steps of 256: WK 1, 1, 2, 2, 4, 4, 8, 8
NS = (1, 16, 23, 24, 40)  # N of the linear, inter of SiLU: a single row, odd, a partial tile, more than one workgroup
GRID = tuple(dict.fromkeys(list(itertools.product(MS, (24,), KS)) + list(itertools.product((1, 17, 33), NS, (384, 1152)))))
K_RING = 10368  # 41 steps: every wave of 8 wraps the deepest ring
RING = ((1, 24, K_RING), (17, 24, K_RING))
TILED = (256, 64, 384)  # prefill-sized M: widen + the tiled bf16 GEMM; for SiLU inter = 32 over the same rows
F16_SHAPES = ((1, 24, 128), (17, 23, 384), (33, 24, 256))  # three grid shapes for the f16 store: short K keeps the 2 % cap
CAP = 0.02  # of the bf16 / f16 elements of one (entry, kind, output type) may have two admissible values

# what csrc/w4a16_gemm.hip instantiates: MT in {1, 2} x WK in {1, 2, 4, 8}; the depths are Int4Line::depth
ALL_LINEAR = {(mt, wk, 2 if mt == 2 else 4) for mt in (1, 2) for wk in (1, 2, 4, 8)}
ALL_SILU = {(mt, wk, 1 if mt == 2 else 2) for mt in (1, 2) for wk in (1, 2, 4, 8)}


# ---------------------------------------------------------------- data
def make_x(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (M, K), generator=g).to(BF16)


def make_u(rows, K, seed):
    """uint8 [rows, K] over 0..15: codes 0 and 15 in every row, and in row 0 code (d - p) % 16 at position p of dword d < 16,
    which puts every code at every nibble position"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 16, (rows, K), generator=g, dtype=torch.uint8)
    u[:, K - 1] = 15
    u[:, 0], u[:, 1] = 0, 15
    d, p = torch.arange(16).view(16, 1), torch.arange(8).view(1, 8)
    u[0, :GROUP] = ((d - p) % 16).to(torch.uint8).flatten()
    at = u.view(rows, K // 8, 8)
    assert all(sorted(set(at[:, :, q].flatten().tolist())) == list(range(16)) for q in range(8))
    assert bool((u == 0).any(dim=1).all()) and bool((u == 15).any(dim=1).all())
    return u


def pow2_scales(rows, K, halves=1):
    """fp32 [rows, K / 128], powers of two: exponents -2..2 up to K = 2304, -1..1 beyond"""
    n_rows, G = rows // halves, K // GROUP
    n, grp = torch.arange(n_rows).view(n_rows, 1), torch.arange(G).view(1, G)
    if K <= 2304:
        idx, m, shift = n + 2 * grp, 5, 3  # a row pair's 2 x 2 block reads 0, 2, 1, 3 (mod 5)
    else:
        # along the diagonal of a 2 x 2 block in odd blocks, across it in even ones (tests/test_gpu_w4a16.py::build's rule)
        idx, m, shift = torch.where((n // 2 + grp // 2) % 2 == 0, n + grp, n + 2 * grp), 3, 1
    e = torch.cat([(idx + h * shift) % m for h in range(halves)]) - m // 2
    s = torch.exp2(e.to(F32))
    blocks = s.view(halves, n_rows, G)
    for h in range(halves):
        b = blocks[h]
        if n_rows > 1:
            assert bool((b[0:-1:2] != b[1::2])[: n_rows // 2].all())  # the two rows of a pair, every group
        if G > 1:
            assert bool((b[:, 0:-1:2] != b[:, 1::2])[:, : G // 2].all())  # the two groups of a K step, every row
        if m == 5 and n_rows > 1 and G > 1:
            assert bool((b[0:-1:2, 0:-1:2] != b[1::2, 1::2]).all()) and bool((b[1::2, 0:-1:2] != b[0:-1:2, 1::2]).all())
    if halves == 2:
        assert bool((blocks[0] != blocks[1]).all())  # w1 against w3, slot for slot
    return s.contiguous()


def quantiser_scales(rows, K, seed):
    """arbitrary fp32 scales: quant_weight_w4a16's formula, max|w_group| / 7, over a random fp32 matrix.  (Over bf16 weights the
    scales are 8-bit numbers / 7 and with integer x one output in fourteen is a multiple of a short power of two, within 1e-9
    of an f16 / bf16 rounding tie: such a construction tests the tie, not the kernel.)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, K // GROUP, 8, generator=g) * 0.05
    return (w.abs().amax(dim=-1).clamp_(min=1e-5) / 7.0).contiguous()


# ---------------------------------------------------------------- the real product
def group_sums(x, u):
    """P[m][n][g] = sum_{k in g} x[m][k] (u[n][k] - 8), int64, exact"""
    M, K = x.shape
    xi = x.to(torch.float64).to(torch.int64).view(M, K // GROUP, GROUP)
    wi = (u.to(torch.int64) - 8).view(u.shape[0], K // GROUP, GROUP)
    return torch.einsum("mgk,ngk->mng", xi, wi)


def value_and_magnitude(x, u, s):
    """(v, sum_g |s_g P_g|) in fp64, [M, rows]"""
    t = group_sums(x, u).to(torch.float64) * s.to(torch.float64).unsqueeze(0)
    return t.sum(-1), t.abs().sum(-1)


def assert_exact(x, u, s):
    """the exactness condition of the pow2 kind; returns its largest left-hand side"""
    w = (u.to(torch.float64) - 8.0).abs() * s.to(torch.float64).repeat_interleave(GROUP, dim=1)
    worst = float((x.to(torch.float64).abs() @ w.t()).max() / float(s.min()))
    assert worst < 2.0 ** 24, worst
    return worst


def _f32_not_below(v):
    f = v.to(F32)
    return torch.where(f.to(torch.float64) < v, torch.nextafter(f, torch.full_like(f, float("inf"))), f)


def _f32_not_above(v):
    f = v.to(F32)
    return torch.where(f.to(torch.float64) > v, torch.nextafter(f, torch.full_like(f, float("-inf"))), f)


def accumulator_interval(x, u, s):
    """(lo, hi) fp32 [M, rows]: the ends of the fp32 numbers inside [v - rho, v + rho]"""
    v, mag = value_and_magnitude(x, u, s)
    rho = (x.shape[1] // GROUP + 9) * 2.0 ** -24 * mag
    return _f32_not_below(v - rho), _f32_not_above(v + rho)


def dequantised(u, s):
    """fp64 (u - 8) s"""
    return (u.to(torch.float64) - 8.0) * s.to(torch.float64).repeat_interleave(GROUP, dim=1)


def widened(u, s):
    """W' of the tiled contract: bf16(float(u - 8) * s), one fp32 multiply and one rounding"""
    return ((u.to(F32) - 8.0) * s.to(F32).repeat_interleave(GROUP, dim=1)).to(BF16)


# ---------------------------------------------------------------- cases
class Case:
    """One launch's inputs and what it must give.  rows = N (linear) or 2 inter (SiLU, u = [w1; w3], halves = 2).
    lo / hi: fp32 ends of the accumulator (equal for pow2: the exact value)."""

    def __init__(self, entry, kind, M, N, K, seed):
        self.entry, self.kind, self.M, self.N, self.K = entry, kind, M, N, K
        self.halves = 2 if entry == "silu" else 1
        rows = N * self.halves
        self.x, self.u = make_x(M, K, seed), make_u(rows, K, seed + 1)
        if kind == "pow2":
            self.s = pow2_scales(rows, K, self.halves)
            self.worst = assert_exact(self.x, self.u, self.s)
            v, _ = value_and_magnitude(self.x, self.u, self.s)
            self.lo = self.hi = v.to(F32)
            assert torch.equal(self.lo.to(torch.float64), v)
        else:
            self.s = quantiser_scales(rows, K, seed + 2)
            self.lo, self.hi = accumulator_interval(self.x, self.u, self.s)
            assert bool((self.lo <= self.hi).all())

    def packed(self):
        from chitu_amd.quantize.w4a16 import pack_w4a16

        return pack_w4a16(self.u, self.s, halves=self.halves)

    def linear_ends(self, dt):
        """(lo, hi) in the output type: equal wherever the output is determined"""
        return self.lo.to(dt), self.hi.to(dt)

    def silu_args(self):
        """(want, g_lo, u_lo, g_hi, u_hi) of silu_ref.check_silu; the hi ends are None for pow2"""
        n = self.N
        if self.kind == "pow2":
            return silu_ref.silu_mul(self.lo[:, :n], self.lo[:, n:]), self.lo[:, :n], self.lo[:, n:], None, None
        v, _ = value_and_magnitude(self.x, self.u, self.s)
        c = v.to(F32)
        return silu_ref.silu_mul(c[:, :n], c[:, n:]), self.lo[:, :n], self.lo[:, n:], self.hi[:, :n], self.hi[:, n:]

    def free(self, dt=BF16):
        """(elements with two admissible values, elements)"""
        if self.entry == "silu":
            _, g, u, gh, uh = self.silu_args()
            f = silu_ref.free_elements(silu_ref.silu_candidates(g, u, gh, uh))
        else:
            lo, hi = self.linear_ends(dt)
            f = lo != hi
        return int(f.sum()), f.numel()


@functools.lru_cache(maxsize=None)
def case(entry, kind, M, N, K):
    """built once per process and shared: nothing may modify a case"""
    return Case(entry, kind, M, N, K, seed=(M * 1000003 + N * 10007 + K * 31 + (7 if entry == "silu" else 0)) % (1 << 31))


def bf16_pool(entry, kind):
    return [case(entry, kind, *c) for c in GRID + RING]


def f16_pool(kind):
    return [case("linear", kind, *c) for c in F16_SHAPES]


def pooled_free(cases, dt=BF16):
    n_free = n_all = 0
    for c in cases:
        a, b = c.free(dt)
        n_free, n_all = n_free + a, n_all + b
    return n_free, n_all
