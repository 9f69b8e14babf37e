"""Builders and the CPU oracle of the partial-rotary entries (include/chitu_hip_ext7.h, csrc/qkv_post_row16.hip), on top of
tests/qkv_bias_exact.py.

One row of qkv = [hq | hkv | hkv] heads of 128 bf16, bias one bf16 row of the same layout, R the rotary width.  For every head:
    y_i = bf16_rne(float(x_i) + float(b_i))                     tests/qkv_bias_exact.py::add_bias
    q and k heads: tests/row_exact.py::rope_oracle(y[..., :R], cos, sin, 0) on the first R channels -- pairs (2 i, 2 i + 1),
        i < R / 2, by frequency i -- and y[..., R:] copied
    v heads: y
    fp8 cache rows: tests/qk_norm_exact.py::fp8_rows of the partly rotated k head and of the v head y
cos / sin are rows of the decoder's own table at rotary width R, precompute_freqs_cis(R, 1024, theta), at
tests/qkv_bias_exact.py's POSITIONS (theta is that file's, so that R = 128 is its case).  Nothing is restated here: the add, the
rotation, the page rows and the fp8 rows are imported.

tests/test_glm4_exact_host.py checks the oracle on the CPU; tests/test_gpu_glm4_exact.py runs the kernels.
"""

import functools

import torch  # noqa: F401

from tests.qkv_bias_exact import (BATCHES, D, OLD_LENS, PAGE, POSITIONS, PREFILL_ROWS, add_bias, append_oracle, bias_case,  # noqa: F401
                                  bias_row, bits, fp8_rows, live_row, paged)
from tests.row_exact import BF16, rope_oracle  # noqa: F401

# (hq, hkv): GLM-4-9B unsharded -- 36 heads, three passes of the decode loop, the k and v heads on prefetched chunks; TP 2; a
# wave with idle head rows; the model fixture's shape
SHAPES = [(32, 2), (16, 1), (1, 1), (4, 2)]
# GLM-4's width; one rotating lane (lane 0 alone); all but the last lane
WIDTHS = [64, 8, 120]
THETA = 1e6  # tests/qk_norm_exact.py::rope_table's


@functools.lru_cache(maxsize=8)
def rope_table(R, max_pos=1024, theta=THETA):
    """The decoder's own table at rotary width R (chitu_amd.llama.precompute_freqs_cis): cos / sin fp32 [max_pos, R / 2]."""
    from chitu_amd.llama import precompute_freqs_cis

    return precompute_freqs_cis(R, max_pos, theta)


def glm4_case(bs, hq, hkv, R, seed=0):
    """tests/qkv_bias_exact.py::bias_case (x, bias, positions) with cos / sin [bs, R / 2] of the table at width R.  At R = 128
    this is bias_case itself."""
    c = dict(bias_case(bs, hq, hkv, seed=seed))
    cos_t, sin_t = rope_table(R)
    c.update(cos=cos_t[c["pos"]].contiguous(), sin=sin_t[c["pos"]].contiguous(), R=R)
    return c


def rotate_partial(y, cos, sin):
    """y [bs, heads, 128] bf16, cos / sin [bs, R / 2]: the first R channels rotated as interleaved pairs, the rest copied."""
    R = 2 * cos.shape[-1]
    out = y.clone()
    out[..., :R] = rope_oracle(y[..., :R].contiguous(), cos, sin, 0)
    return out


def glm4_oracle(case):
    """(y [bs, nh, 128] the biased row, q [bs, hq, 128], k [bs, hkv, 128], v [bs, hkv, 128]) bf16."""
    hq, hkv = case["hq"], case["hkv"]
    y = add_bias(case["x"], case["bias"])
    q = rotate_partial(y[:, :hq].contiguous(), case["cos"], case["sin"])
    k = rotate_partial(y[:, hq:hq + hkv].contiguous(), case["cos"], case["sin"])
    return y, q, k, y[:, hq + hkv:].contiguous()
