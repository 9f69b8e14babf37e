"""Builders and CPU references of the W8A16 tests (include/chitu_hip_ext6.h).

The integer specification: x has integer values in [-8, 8] (bf16), q is int8 over the full range with -127 and 127 in every row,
K <= 1088 -- every product and every partial sum is an integer below 8 * 127 * 1088 < 2^24, so fp32 accumulation is exact in
any order and the fp32 accumulator IS the int64 dot product.  The expected output is then one fp32 multiply by the row scale and
one rounding, evaluated here on the CPU: nothing about the kernel's summation order enters.
"""

import itertools

import torch

MS = (1, 2, 15, 16, 17, 32, 33)  # both token tiles, the second 32-row launch
NS = (16, 24, 40)  # a partial row tile
KS = (64, 128, 192, 512, 1088)  # every K split, the ring tail, the half-line tail
GRID = tuple(itertools.product(MS, NS, KS))
TILED_CASE = (256, 64, 256)  # prefill-sized M: the widen + tiled GEMM + scale_round form
K_MAX = 1088


def make_x(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (M, K), generator=g).to(torch.bfloat16)


def make_q(rows, K, seed):
    """int8 [rows, K] over [-127, 127] (and -128 once per row, which the widening must also get right) with both extremes of
    the quantiser's range in every row."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-127, 128, (rows, K), generator=g, dtype=torch.int16)
    q[:, 0], q[:, K - 1], q[:, K // 2] = -127, 127, -128
    return q.to(torch.int8)


def pow2_scales(rows):
    """2^-9 .. 2^-3, varied per row: acc * s is exact, so the whole chain down to the one bf16 rounding is exact arithmetic"""
    return torch.tensor([2.0 ** (-9 + (r * 5 + 3) % 7) for r in range(rows)], dtype=torch.float32)


def quantiser_scales(rows, seed):
    """arbitrary fp32 scales, as the quantiser produces them: max|w_row| / 127 of a random bf16 matrix row"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(rows, 64, generator=g) * 0.05).to(torch.bfloat16).float()
    return (w.abs().max(dim=-1)[0].clamp_(min=1e-5) / 127.0).contiguous()


def acc_int(x, q):
    """the exact accumulator, int64 [M, rows]"""
    a = x.to(torch.float64).to(torch.int64) @ q.to(torch.int64).t()
    assert int(a.abs().max()) < (1 << 24)
    return a


def expected_linear(x, q, s, out_dtype=torch.bfloat16):
    """(float32(acc) * s) rounded once to out_dtype: fp32 multiply (exact conversion of acc: |acc| < 2^24)"""
    return (acc_int(x, q).to(torch.float32) * s.view(1, -1)).to(out_dtype)


def expected_silu(x, q13, s):
    """h = bf16(bf16(silu(bf16(g))) * bf16(u)), g = acc_g * s[n], u = acc_u * s[inter + n], every step in fp32 -- the chain of
    bf16_gemm_silu_kernel restated: silu(g) = g / (1 + exp(-g)) in fp32."""
    inter = q13.shape[0] // 2
    a = acc_int(x, q13).to(torch.float32) * s.view(1, -1)
    g, u = a[:, :inter].to(torch.bfloat16).float(), a[:, inter:].to(torch.bfloat16).float()
    sg = (g / (1.0 + torch.exp(-g))).to(torch.bfloat16).float()
    return (sg * u).to(torch.bfloat16)


def instantiations(plan_fn, cases, silu):
    """every (MT, WK, ring) the launch plans of `cases` contain, and the forms"""
    seen, forms = set(), set()
    for (M, N, K) in cases:
        p = plan_fn(M, N, K, silu=silu)
        forms.add(p["form"])
        seen.update(p["launches"])
    return seen, forms


# what csrc/w8a16_gemm.hip instantiates: MT in {1, 2} x WK in {1, 2, 4, 8}; the ring depth follows MT
ALL_LINEAR = {(mt, wk, 2 if mt == 2 else 4) for mt in (1, 2) for wk in (1, 2, 4, 8)}
ALL_SILU = {(mt, wk, 2 if mt == 2 else 3) for mt in (1, 2) for wk in (1, 2, 4, 8)}
