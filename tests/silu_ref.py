"""The SiluAndMul rounding chain of the gate / up launches (csrc/stream_gemm.h::w8a16_silu_mul) on the CPU, over fp32
accumulators: the one statement the W8A16 and the W4A16 exact suites check their SiLU entries with.

    h = bf16( bf16(silu(bf16(g))) * bf16(u) ),  silu(g) = g / (1 + exp(-g)), every step in fp32

One step is not exactly specified on either side: exp(-g) goes through the device's expf and through the CPU's, each at most
1 ulp off (HIP's and glibc's documented bounds), so the two differ by at most 2 fp32 ulps = a factor within 1 -+ 2^-22.  The add
and the divide behind it are correctly rounded and monotone on both sides, so the device's silu lies between the chain evaluated
at exp * (1 - 2^-22) and at exp * (1 + 2^-22).

A caller that knows its accumulators only up to an interval [lo, hi] (fp32 numbers that enclose the device's value: an
arbitrary summation order under arbitrary fp32 scales) passes both ends.  bf16(g) is then one of bf16(g_lo), bf16(g_hi) when
those are equal or neighbours, and the admissible outputs are the chain at every corner (g end, u end, exp factor).  Where the
ends of g or of u lie further apart -- an accumulator that cancels to nearly zero, where bf16 numbers are dense -- the chain
is monotone in g (silu's only turning point, g = -1.2785, is asserted to be outside) and linear in u between two roundings, so
the output lies between the smallest and the largest corner."""
import torch

BF16 = torch.bfloat16
EXP_FACTORS = (1.0 - 2.0 ** -22, 1.0 + 2.0 ** -22)


def silu_mul(g_acc, u_acc, exp_factor=1.0):
    g, u = g_acc.to(torch.float32).to(BF16).float(), u_acc.to(torch.float32).to(BF16).float()
    e = torch.exp(-g) * torch.tensor(exp_factor, dtype=torch.float32)
    sg = (g / (1.0 + e)).to(BF16).float()
    return (sg * u).to(BF16)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _order(t):
    """bf16 -> an integer that counts bf16 numbers in order (-0 and +0 both 0)"""
    b = _bits(t.to(BF16)).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def silu_candidates(g_acc, u_acc, g_hi=None, u_hi=None):
    """the chain at every corner: 2 outputs for exact accumulators (the two exp factors), 8 for intervals"""
    return [silu_mul(g, u, f) for g in ((g_acc,) if g_hi is None else (g_acc, g_hi))
            for u in ((u_acc,) if u_hi is None else (u_acc, u_hi)) for f in EXP_FACTORS]


def free_elements(cands):
    """bool mask: the elements with more than one admissible output"""
    free = torch.zeros_like(cands[0], dtype=torch.bool)
    for c in cands[1:]:
        free |= _bits(c) != _bits(cands[0])
    return free


def check_silu(got, want, g_acc, u_acc, what, g_hi=None, u_hi=None):
    """got (bf16) must be the chain's output at one of the corners, and `want` (the caller's own statement of the chain at the
    centre) bit for bit wherever all corners agree.  Returns the count of elements with more than one admissible output."""
    cands = silu_candidates(g_acc, u_acc, g_hi, u_hi)
    gb, free = _bits(got), free_elements(cands)
    ok = torch.zeros_like(free)
    for c in cands:
        ok |= gb == _bits(c)
    if g_hi is not None:
        wide = ((_order(g_hi) - _order(g_acc)).abs() > 1) | ((_order(u_hi) - _order(u_acc)).abs() > 1)
        if bool(wide.any()):
            assert bool(((g_acc[wide] > -1.0) | (g_hi[wide] < -1.5)).all()), (what, "an interval of g around silu's turning point")
            vals = torch.stack([c.float() for c in cands])
            ok |= wide & (got.float() >= vals.min(0)[0]) & (got.float() <= vals.max(0)[0])
    assert bool(ok.all()), (what, (~ok).nonzero()[:4].tolist(), got[~ok][:4], cands[0][~ok][:4])
    assert bool((gb == _bits(want))[~free].all()), what  # off a boundary the CPU's fp32 chain is the answer, bit for bit
    return int(free.sum())
