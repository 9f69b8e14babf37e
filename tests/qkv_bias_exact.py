"""Builders and the CPU oracle of the q / k / v bias kernels (csrc/qkv_post_row16.hip), in the style of tests/qk_norm_exact.py.

One row of qkv = [hq | hkv | hkv] heads of 128 bf16, bias one bf16 row of the same layout.  For every head:
    y_i = bf16_rne(float(x_i) + float(b_i))                     one add, one rounding
    q and k heads: RoPE on y widened to fp32 (tests/row_exact.py::rope_oracle: products rounded separately, one rounding)
    v heads: y
    fp8 cache rows: tests/qk_norm_exact.py::fp8_rows of the rotated k head and of the v head y
The add is stated here in numpy float64 with an explicit round-to-nearest-even to bf16 (bf16_rne); the sum of two bf16
numbers of comparable magnitude is exact in float64 and in fp32 (asserted on the cases), so "one fp32 add, one rounding" leaves
the kernel no free choice.  The RoPE, page-row and fp8-row oracles are imported, not restated.

tests/test_qkv_bias_exact_host.py checks the oracle on the CPU; tests/test_gpu_qkv_bias.py runs the kernels.
"""

import functools

import numpy as np
import torch

from tests.qk_norm_exact import fp8_rows, rope_table  # noqa: F401
from tests.row_exact import BF16, append_oracle, bits, live_row, paged_batch, rope_oracle  # noqa: F401

D = 128
# (hq, hkv): Qwen2.5-7B at TP 4; two kv heads; a wave with idle head rows; Qwen2.5-7B unsharded -- 36 heads, three passes
# of the decode loop: the k heads fall in the second and the v heads in the third, on prefetched channels and bias chunks
SHAPES = [(7, 1), (4, 2), (1, 1), (28, 4)]
BATCHES = [1, 3, 5]
PAGE = 16
OLD_LENS = [0, 15, 16, 17]  # first slot of a page, its last, the next page's first and second
PREFILL_ROWS = [1, 5, 37]
POSITIONS = [0, 1, 5, 77, 300, 2, 1023, 16, 0, 48, 47]


def bf16_rne(a):
    """float64 array of values that are exact in fp32 -> bf16 (torch), round to nearest, ties to even, on the bit pattern."""
    a = np.asarray(a, dtype=np.float64)
    f = a.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), a), "the sum is not exact in fp32: the case leaves the add a choice"
    u = f.view(np.uint32).astype(np.uint64)
    assert not np.any((u & 0x7F800000) == 0x7F800000), "Inf / NaN"
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return torch.from_numpy(r.view(np.int16).copy()).view(BF16)


def add_bias(x, bias):
    """x [..., nh, 128] bf16 + bias [nh * 128] bf16 -> bf16, the statement above."""
    nh = x.shape[-2]
    s = x.double().numpy() + bias.double().view(nh, D).numpy()
    return bf16_rne(s).view(x.shape)


def bias_row(hq, hkv):
    """[(hq + 2 hkv) * 128] bf16 from (head, channel) alone: multiples of 1/16 in [-4, 4), another value in every channel of a
    head's 16-byte lane chunks and in the same channel of neighbouring heads (so a misindexed head or lane changes the result),
    of the activations' magnitude (so a dropped bias does)."""
    h = torch.arange(hq + 2 * hkv)[:, None]
    c = torch.arange(D)[None, :]
    b = ((h * 37 + c * 11 + (c // 8) * 5) % 128 - 64).float() / 16.0
    return b.to(BF16).reshape(-1)


@functools.lru_cache(maxsize=64)
def bias_case(bs, hq, hkv, seed=0):
    """x [bs, hq + 2 hkv, 128] bf16 random full-mantissa values of standard deviation 2 (2^-12 <= |x| < 16 or x = 0: x is a
    multiple of 2^-19, b of 2^-4, |x + b| < 2^5 -- at most 24 significant bits, exact in fp32), the bias row, cos / sin rows of the
    decoder's own table at POSITIONS (position 0 in every batch)."""
    g = torch.Generator().manual_seed(6151 * bs + 211 * hq + 13 * hkv + seed)
    x = (torch.randn(bs, hq + 2 * hkv, D, generator=g) * 2).clamp(-15, 15).to(BF16)
    x = torch.where(x.abs() < 2.0 ** -12, torch.zeros_like(x), x)
    pos = torch.tensor([POSITIONS[(b + (seed if b else 0)) % len(POSITIONS)] for b in range(bs)])
    cos_t, sin_t = rope_table()
    return dict(x=x.contiguous(), bias=bias_row(hq, hkv), pos=pos, cos=cos_t[pos].contiguous(), sin=sin_t[pos].contiguous(),
                hq=hq, hkv=hkv)


def bias_oracle(case, layout):
    """(y [bs, nh, 128] the biased row, q [bs, hq, 128], k [bs, hkv, 128], v [bs, hkv, 128]) bf16."""
    hq, hkv = case["hq"], case["hkv"]
    y = add_bias(case["x"], case["bias"])
    q = rope_oracle(y[:, :hq].contiguous(), case["cos"], case["sin"], layout)
    k = rope_oracle(y[:, hq:hq + hkv].contiguous(), case["cos"], case["sin"], layout)
    return y, q, k, y[:, hq + hkv:].contiguous()


def paged(bs, seed, bad=False):
    """tests/row_exact.py::paged_batch at page 16 with the old lengths of the valid rows replaced by OLD_LENS, walked through by
    (row + seed): (lens, table, num_pages, kinds)."""
    lens, table, num_pages, _, kinds = paged_batch(bs, PAGE, seed=seed, bad=bad)
    for b in range(bs):
        if b not in kinds:
            lens[b] = OLD_LENS[(b + seed) % len(OLD_LENS)]
    return lens, table, num_pages, kinds
