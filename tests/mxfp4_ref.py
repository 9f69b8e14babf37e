"""Pure-torch statement of OCP MXFP4 (MX v1.0) and of the W4A8 fused MoE built on it.  TEST INFRASTRUCTURE ONLY.

Format: e2m1 elements (1 sign, 2 exponent, 1 mantissa bit; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6), two per byte with the
even k in the low nibble; one E8M0 scale byte per 32 consecutive k of a row, value 2^(byte - 127), 0xFF = NaN.
Scale bytes 2..252 are the specified range: every e2m1 x scale product is then a normal finite fp32 (and bf16) number.
Bytes 0, 1, 253 and 254 are UNSPECIFIED here (products may be subnormal or overflow bf16's rounding), 0xFF is NaN.

The quantiser is the OCP rule: shared exponent X = floor(log2(max|v| of the 32)) - 2 -- read off the fp32 exponent field, so a
subnormal maximum counts as 2^-127 --, scale byte = clamp(X + 127, 0, 254); elements = round-to-nearest-even of v / 2^X on the
e2m1 grid, saturated to +-6, sign = the value's sign bit.  AN ALL-ZERO BLOCK GETS SCALE BYTE 0 (and codes 0 / 8).

`fused_experts_mxfp4` is oracle.moe.fused_experts_fp8 with the weight operand exchanged (same rounding points, same loop,
same matmul shapes): tests/test_mxfp4_host.py asserts that the two agree bit for bit wherever MXFP4 weights are also
fp8-block weights, which keeps this file from drifting away from the pinned oracle.
"""

import torch
import torch.nn.functional as F

from oracle import fp8 as ofp8

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def unpack(packed: torch.Tensor) -> torch.Tensor:
    """uint8 [..., K/2] -> codes uint8 [..., K] (low nibble = even k)."""
    return torch.stack([packed & 15, packed >> 4], dim=-1).reshape(*packed.shape[:-1], packed.shape[-1] * 2)


def pack(codes: torch.Tensor) -> torch.Tensor:
    c = codes.to(torch.uint8).reshape(*codes.shape[:-1], codes.shape[-1] // 2, 2)
    return c[..., 0] | (c[..., 1] << 4)


def e2m1_value(codes: torch.Tensor) -> torch.Tensor:
    mag = E2M1[(codes & 7).long()]
    return torch.where((codes & 8) != 0, -mag, mag)


def scale_value(b: torch.Tensor) -> torch.Tensor:
    v = torch.ldexp(torch.ones(b.shape), b.to(torch.int32) - 127)
    return torch.where(b == 255, torch.full_like(v, float("nan")), v)


def dequant_f32(packed: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 [..., K] = e2m1 x 2^(byte - 127): exact for bytes 2..252."""
    K = packed.shape[-1] * 2
    v = e2m1_value(unpack(packed)).reshape(*packed.shape[:-1], K // 32, 32)
    out = torch.ldexp(v, (scales.to(torch.int32) - 127)[..., None].expand_as(v))
    out = torch.where((scales == 255)[..., None].expand_as(v), torch.full_like(out, float("nan")), out)
    return out.reshape(*packed.shape[:-1], K)


def dequant(packed, scales):
    return dequant_f32(packed, scales).to(torch.bfloat16)


def e2m1_code(q: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even onto the e2m1 grid, saturating; ties go to the code with an even mantissa bit."""
    a = q.abs()
    m = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
         + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    return m | (torch.signbit(q).to(torch.uint8) << 3)


def quant(v: torch.Tensor):
    """[..., K] float -> (packed uint8 [..., K/2], scales uint8 [..., K/32])."""
    K = v.shape[-1]
    b = v.float().reshape(*v.shape[:-1], K // 32, 32)
    amax = b.abs().amax(dim=-1)
    field = (amax.contiguous().view(torch.int32) >> 23) & 0xFF
    byte = (field - 2).clamp(0, 254)
    inv = torch.ldexp(torch.ones(byte.shape), 127 - byte)  # 2^-X, a normal number for every byte the rule can give (<= 253)
    codes = e2m1_code(b * inv[..., None])
    return pack(codes.reshape(*v.shape[:-1], K)), byte.to(torch.uint8)


def quant_from_fp8_block(w: torch.Tensor, scale: torch.Tensor):
    """e4m3 [..., R, K] + [128, 128] block scales [..., ceil(R/128), K/128]: quant(float(w) * scale)."""
    R, K = w.shape[-2], w.shape[-1]
    return quant(w.float() * ofp8._expand_block_scale(scale, R, K))


def gemm(a_q, a_s, w_packed, w_scales, out_dtype=torch.bfloat16, dot_dtype=torch.float32, w_f32=None):
    """oracle.fp8.fp8_gemm_deepseek_v3 with MXFP4 weights: acc += dot(a_kb, w_kb) * a_s[:, kb] per 128-block, the weights'
    own scales inside the dot.  dot_dtype=float64 evaluates the block dots in double (rounded to fp32 once).
    w_f32: dequant_f32(w_packed, w_scales) if the caller already has it."""
    K = a_q.shape[-1]
    a = a_q.float().reshape(-1, K)
    a_s = a_s.reshape(a.shape[0], -1)
    b = dequant_f32(w_packed, w_scales) if w_f32 is None else w_f32
    N = b.shape[0]
    acc = torch.zeros(a.shape[0], N, dtype=torch.float32)
    for kb in range(K // 128):
        sl = slice(kb * 128, (kb + 1) * 128)
        if dot_dtype == torch.float32:
            dot = ofp8.CAST["matmul"](a[:, sl], b[:, sl].T)
        else:
            dot = (a[:, sl].to(dot_dtype) @ b[:, sl].T.to(dot_dtype)).float()
        acc += dot * a_s[:, kb : kb + 1]
    return ofp8.to_out(acc, out_dtype).reshape(*a_q.shape[:-1], N)


def fused_experts_mxfp4(x, w1, w1_scale, w2, w2_scale, topk_weights, topk_ids, expert_map=None, dot_dtype=torch.float32,
                        reduce_topk=True):
    """x [M, K] bf16; w1 uint8 [E, 2I, K/2] + scales [E, 2I, K/32]; w2 uint8 [E, Nout, I/2] + scales [E, Nout, I/32]."""
    if expert_map is not None:
        local = torch.as_tensor(expert_map).long()[topk_ids.long()]
        keep = local >= 0
        return fused_experts_mxfp4(x, w1, w1_scale, w2, w2_scale, torch.where(keep, topk_weights, torch.zeros_like(topk_weights)),
                                   torch.where(keep, local, torch.zeros_like(local)), None, dot_dtype, reduce_topk)
    M, K = x.shape
    topk = topk_ids.shape[1]
    dt = x.dtype
    a1_q, a1_s = ofp8.per_token_group_quant_fp8(x)
    c1 = torch.empty(M, topk, w1.shape[1], dtype=dt)
    deq1, deq2 = {}, {}  # each expert dequantised once

    def deq(cache, w, s, e):
        if e not in cache:
            cache[e] = dequant_f32(w[e], s[e])
        return cache[e]

    for t in range(M):
        for j in range(topk):
            e = int(topk_ids[t, j])
            c1[t, j] = gemm(a1_q[t : t + 1], a1_s[t : t + 1], w1[e], w1_scale[e], dt, dot_dtype, deq(deq1, w1, w1_scale, e))[0]
    d = w1.shape[1] // 2
    c1 = c1.view(-1, w1.shape[1])
    c2 = F.silu(c1[..., :d]) * c1[..., d:]
    a2_q, a2_s = ofp8.per_token_group_quant_fp8(c2)
    c3 = torch.empty(M, topk, w2.shape[1], dtype=dt)
    for t in range(M):
        for j in range(topk):
            e = int(topk_ids[t, j])
            r = t * topk + j
            acc = gemm(a2_q[r : r + 1], a2_s[r : r + 1], w2[e], w2_scale[e], torch.float32, dot_dtype, deq(deq2, w2, w2_scale, e))[0]
            c3[t, j] = ofp8.to_out(acc * topk_weights[t, j].float(), dt)
    return c3.sum(dim=1) if reduce_topk else c3


# ---------------------------------------------------------------- inputs that are MXFP4 AND fp8-block weights at once
def fp8_twin_weights(E, R, K, gen, base_lo=117, base_hi=121):
    """Random MXFP4 weights [E, R, K] whose scale bytes lie within +-3 of a base per [128, 128] tile, and their exact fp8
    twin: w8 = e2m1 x 2^(byte - base) as e4m3 (magnitudes 2^-4 .. 48: inside e4m3's normal range, at most two significant
    bits) with fp32 block scale 2^(base - 127).  Returns (packed, scales, w8, block_scale)."""
    codes = torch.randint(0, 16, (E, R, K), generator=gen, dtype=torch.uint8)
    base = torch.randint(base_lo, base_hi + 1, (E, (R + 127) // 128, K // 128), generator=gen, dtype=torch.int32)
    delta = torch.randint(-3, 4, (E, R, K // 32), generator=gen, dtype=torch.int32)
    base_rows = base.repeat_interleave(128, dim=1)[:, :R].repeat_interleave(4, dim=2)  # [E, R, K/32]
    scales = (base_rows + delta).to(torch.uint8)
    rel = torch.ldexp(e2m1_value(codes).reshape(E, R, K // 32, 32), delta[..., None].expand(E, R, K // 32, 32)).reshape(E, R, K)
    w8 = rel.to(torch.float8_e4m3fn)
    assert torch.equal(w8.float(), rel), "the twin must be exactly representable in e4m3"
    return pack(codes), scales, w8, torch.ldexp(torch.ones(base.shape), base - 127)
