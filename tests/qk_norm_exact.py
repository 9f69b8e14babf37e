"""Builders and the CPU oracle of the per-head QK-norm kernels (csrc/qkv_post_row16.hip), in the style of tests/row_exact.py, whose
helpers state the two halves: RMSNorm (rms_t, rr_candidates, rms_rows, match_rows) and RoPE (rope_oracle).

One head x of 128 bf16 channels, weight w [128] bf16, eps:
    ss = sum x_i^2 (fp32)      t = fl(fl(ss / 128) + eps)      rr = rsqrtf(t)      n_i = bf16(fl(fl(x_i rr) w_i))
    RoPE on n widened to fp32: o0 = bf16(fl(n0 c) - fl(n1 s)), o1 = bf16(fl(n1 c) + fl(n0 s))
The data leaves the kernel no free choice that changes a bit: heads are integers times one power of two per head with
128 * max^2 < 2^24 (asserted, never measured), so the sum of squares is exact in any order.  The device rsqrtf is not
correctly rounded: the oracle gives one expected head per candidate rr (the correctly rounded value and its RSQRT_RADIUS
fp32 neighbours), each carried through the bf16 rounding and the RoPE statement, and a kernel's WHOLE head must equal one.

tests/test_qk_norm_exact_host.py checks the oracle on the CPU; tests/test_gpu_qk_norm.py runs the kernels.
"""

import functools

import torch

from oracle import fp8 as ofp8
from tests.dense_exact import ints
from tests.row_exact import BF16, F32, RSQRT_RADIUS, Guarded, bits, match_rows, rms_rows, rms_t, rope_oracle, rr_candidates  # noqa: F401

D = 128
EPS = 1e-6
HEAD_EXPS = [-12, -3, 0, 4, 9]
LIM = 255  # bf16 holds every integer up to 256; 128 * 255^2 = 8 323 200 < 2^24
# (hq, hkv); (5, 1) and (3, 1) leave a wave's four-head group partly empty; (32, 8) is Qwen3-8B -- 48 heads, three passes of
# the decode loop, the k heads in the third: rotated from a prefetched chunk
SHAPES = [(8, 8), (8, 2), (8, 1), (5, 1), (3, 1), (32, 8)]
BATCHES = [1, 3, 17]
PAGES = [16, 48]
POSITIONS = [0, 1, 5, 77, 300, 2, 1023, 16, 0, 48, 47]


@functools.lru_cache(maxsize=1)
def rope_table(max_pos=1024, theta=1e6):
    """The decoder's own table (chitu_amd.llama.precompute_freqs_cis): cos / sin fp32 [max_pos, 64]."""
    from chitu_amd.llama import precompute_freqs_cis

    return precompute_freqs_cis(D, max_pos, theta)


def norm_weight(seed):
    """[128] bf16, +-2^k with k in -2 .. 2, sign and k mixed per channel."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-2, 3, (D,), generator=g)
    sign = torch.randint(0, 2, (D,), generator=g) * 2 - 1
    return (sign.float() * torch.ldexp(torch.ones(D), k.to(torch.int32))).to(BF16)


@functools.lru_cache(maxsize=64)
def qk_case(bs, hq, hkv, seed=0):
    """x [bs, hq + 2 hkv, 128] bf16: the q and k heads are integers -LIM .. LIM times 2^e, e per head cycling through HEAD_EXPS;
    the v heads are random full-mantissa values (they are copied or quantised, never normalised).  q_w, k_w: norm_weight.
    cos / sin: rows of the real table at POSITIONS (position 0 included in every batch)."""
    g = torch.Generator().manual_seed(7919 * bs + 131 * hq + 17 * hkv + seed)
    nqk = hq + hkv
    xi = ints(g, LIM, bs, nqk, D)
    assert D * int(xi.abs().max()) ** 2 < 2 ** 24 and int(xi.abs().max()) <= 256  # ss exact in fp32, values exact in bf16
    e = torch.tensor([[HEAD_EXPS[(b * nqk + h + seed) % len(HEAD_EXPS)] for h in range(nqk)] for b in range(bs)])
    scale = torch.ldexp(torch.ones(bs, nqk), e.to(torch.int32))[..., None]
    qk = (xi.float() * scale).to(BF16)
    assert torch.equal(qk.double(), xi.double() * scale.double())
    v = (torch.randn(bs, hkv, D, generator=g) * 3).to(BF16)
    pos = torch.tensor([POSITIONS[(b + (seed if b else 0)) % len(POSITIONS)] for b in range(bs)])
    assert int(pos[0]) == 0
    cos_t, sin_t = rope_table()
    return dict(x=torch.cat([qk, v], 1).contiguous(), q_w=norm_weight(seed + 1), k_w=norm_weight(seed + 2), pos=pos,
                cos=cos_t[pos].contiguous(), sin=sin_t[pos].contiguous(), hq=hq, hkv=hkv)


def head_candidates(x, w, cos, sin, layout, eps=EPS, radius=RSQRT_RADIUS):
    """x [bs, heads, 128] bf16, one weight w [128] for all of them, cos / sin [bs, 64] ->
    (t [bs * heads], rr [C, bs * heads], y [C, bs, heads, 128] bf16): the expected head per rr candidate."""
    bs, heads, _ = x.shape
    rows = x.reshape(bs * heads, D)
    t = rms_t(rows, dim=D, eps=eps)
    rr = rr_candidates(t, radius)
    y = torch.stack([rope_oracle(rms_rows(rows, w, r).view(bs, heads, D), cos, sin, layout) for r in rr])
    return t, rr, y


def qk_oracle(case, layout, eps=EPS):
    """(t, rr, y [C, bs, hq + hkv, 128]) of a qk_case: the q heads under q_w, the k heads under k_w."""
    hq, x = case["hq"], case["x"]
    tq, rq, yq = head_candidates(x[:, :hq], case["q_w"], case["cos"], case["sin"], layout, eps)
    tk, rk, yk = head_candidates(x[:, hq:hq + case["hkv"]], case["k_w"], case["cos"], case["sin"], layout, eps)
    return (tq, rq, yq), (tk, rk, yk)


def match_heads(got, cand, what):
    """got [bs, heads, 128] bf16 against head_candidates' triple: every head equals one candidate as a whole."""
    t, rr, y = cand
    return match_rows(got.reshape(-1, D), t, rr, y.reshape(y.shape[0], -1, D), what)


def fp8_rows(heads):
    """bf16 [..., 128] -> uint8 [..., 144]: the K / V cache row of every head as gqa_kv_fp8.hip states it -- 128 e4m3fn codes
    (oracle/fp8.py's round-to-nearest-even cast) of x * 2^-e | the fp32 scale 2^e | 12 zero bytes; e = the smallest integer with
    amax <= 448 * 2^e, clamped to >= -64 (amax == 0: -64).  The statement of tests/test_gqa_kv_fp8_host.py::quant_ref."""
    xf = heads.float()
    amax = xf.abs().amax(-1)
    m, ex = torch.frexp(amax / 448.0)  # amax / 448 = m 2^ex, m in [0.5, 1): <= 2^(ex - 1) only when m == 0.5
    e = ex - (m == 0.5).to(ex.dtype)
    e = torch.where(amax == 0, torch.full_like(e, -64), e).clamp(min=-64)
    out = torch.zeros(*heads.shape[:-1], 144, dtype=torch.uint8)
    out[..., :128] = ofp8.to_fp8(torch.ldexp(xf, -e.unsqueeze(-1))).view(torch.uint8)
    out[..., 128:132] = torch.ldexp(torch.ones_like(amax), e).contiguous().view(torch.uint8).view(*heads.shape[:-1], 4)
    return out


# ---------------------------------------------------------------- statements for the host test
def head_float64(x, w, cos, sin, layout, eps=EPS):
    """The same head in float64, the intermediate bf16 rounding kept: (n [bs, heads, 128] float64 values of bf16 numbers,
    o [bs, heads, 128] float64, unrounded)."""
    xd = x.double()
    rr = 1.0 / ((xd * xd).sum(-1, keepdim=True) / D + eps).sqrt()
    n = ((xd * rr) * w.double()).to(BF16).double()
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    n0, n1 = (n[..., 0::2], n[..., 1::2]) if layout == 0 else (n[..., :64], n[..., 64:])
    o = torch.empty_like(n)
    if layout == 0:
        o[..., 0::2], o[..., 1::2] = n0 * c - n1 * s, n1 * c + n0 * s
    else:
        o[..., :64], o[..., 64:] = n0 * c - n1 * s, n1 * c + n0 * s
    return n, o


def wrong_variants(x, w, cos, sin, layout, eps=EPS):
    """name -> [bs, heads, 128] bf16 of four plausible mis-statements, each with the correctly rounded rr."""
    bs, heads, _ = x.shape
    rows = x.reshape(-1, D)
    rr = rr_candidates(rms_t(rows, dim=D, eps=eps), 0)[0]
    out = {}
    # the weight multiplied in before rr is taken: the weighted head is what gets normalised
    xw = rows.float() * w.float()[None, :]
    ss = (xw.double() ** 2).sum(-1)
    rw = (1.0 / (ss / D + eps).sqrt()).float()
    out["weight applied before rr"] = rope_oracle((xw * rw[:, None]).to(BF16).view(bs, heads, D), cos, sin, layout)
    # RoPE on the fp32 normalised values, one rounding at the end
    n32 = ((rows.float() * rr[:, None]) * w.float()[None, :]).view(bs, heads, D)
    out["no intermediate bf16 rounding"] = rope_oracle(n32, cos, sin, layout).to(BF16)
    # RoPE first (rounded to bf16), then the norm
    r = rope_oracle(x, cos, sin, layout).reshape(-1, D)
    rr2 = (1.0 / ((r.double() ** 2).sum(-1) / D + eps).sqrt()).float()
    out["norm after RoPE"] = rms_rows(r, w, rr2).view(bs, heads, D)
    out["layouts swapped"] = rope_oracle(rms_rows(rows, w, rr).view(bs, heads, D), cos, sin, 1 - layout)
    return out
