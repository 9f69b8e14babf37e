"""Builders and CPU expectations for the fused launches: the norm-prologue GEMMs, mla_q_proj and merge + W_UV (no GPU needed).

The fused entries (bf16_norm_gemm.hip, fp8_norm_gemm.hip, mla_q_proj.hip, the merge of absorb.hip) run an RMSNorm, a group
quantisation and a GEMM in one kernel.  The constructions of tests/dense_exact.py (integer operands, power-of-two scales: THE
matmul whatever the summation order) and tests/row_exact.py (rsqrt candidate rows) are chained here by one more: an activation
row that stays exact THROUGH the norm and the e4m3 group quantisation.

  the exact normalised row (norm_case)
      v, the row that is normalised (x, or x + add, or x + the in-order sum of the terms), holds exactly dim/4 non-zero entries
      per row, all +-c_r with c_r a power of two that changes from row to row: the mean square is c_r^2 / 4, its sum exact in fp32
      in ANY order (mla_q_proj sums in an order of its own; on this data the order cannot show).  rr = rsqrt(c_r^2 / 4 + eps) is
      2 / c_r (1 - d) with d ~ 2 eps / c_r^2 <= 2e-5 for c_r >= 1: far inside the half ulp of bf16 around (v rr) w = +-2 k 2^p
      for the norm weights w[i] = k_i 2^p[group] (k_i signed integers 1..6), so every rsqrt candidate within
      row_exact.RSQRT_RADIUS gives the SAME bf16 row (asserted with row_exact.rms_oracle, never assumed) and the expectation is
      one row.  Every 128-group has two special columns |k| = 7 and |k| = 14 of which a tier per (row, group) makes exactly one
      non-zero in v: the group's maximum is 14 2^p or 28 2^p, amax / 448 = 2^(p - 5 + tier) is a power of two that differs
      between neighbouring rows and neighbouring groups (p = 2 x a dense_exact.exps walk, tier = (row + group) % 2), and the
      codes are the integers 64 k / 32 k <= 448: dequantising them returns the row bit for bit (asserted).
  the full-mantissa family (ident_case)
      row_exact.rms_case rows (random norm weights with full mantissas, exact sum of squares) in front of an IDENTITY GEMM weight:
      every output element is one product, so the output is codes x scale of act_quant(one rsqrt candidate row), the whole row at
      once (row_exact.match_rows), or the candidate row itself for the bf16 entries.
  the merge workspace (merge_case)
      partial rows and LSE values laid out as chitu_hip_mla_decode(out = NULL) leaves them; live splits share one LSE (weight
      exp(0) = 1), empty splits have LSE = -inf and NaN rows, negligible splits have LSE = live - 200 (weight e^-200 ~ 1e-87,
      below the smallest fp32 subnormal: zero whatever the last bit of the device exp) and large finite rows.

tests/test_fused_exact_host.py checks all of this on the CPU; tests/test_gpu_fused_exact.py runs the kernels.  The shape lists of
both live here, with host mirrors of the launchers' choice of instantiation.
"""

import functools
import itertools

import torch

from oracle import fp8 as ofp8
from tests import dense_exact as dx
from tests import row_exact as rx

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ROW_C_EXPS = [0, 3, 1, 5, 2, 4]   # c_r = 2^e, >= 1 (large enough for eps <= 1e-5), neighbouring rows differ
EPS_LIST = [1e-6, 1e-5]
LSE_GAP = 200.0


# ---------------------------------------------------------------- the exact normalised row
def _split_terms(g, total, terms, rows, dim):
    """`terms` integer tensors [rows, dim] summing to `total` (|total| <= 248), each within 255."""
    lim = 0 if terms == 1 else max(1, 120 // (terms - 1))
    parts = [dx.ints(g, lim, rows, dim) for _ in range(terms - 1)]
    parts.append(total - sum(parts) if parts else total)
    out = torch.stack(parts, 1)  # [rows, terms, dim]
    assert int(out.abs().max()) <= 255 and torch.equal(out.sum(1), total)
    return out


@functools.lru_cache(maxsize=512)
def norm_case(rows, dim, terms=1, eps=rx.EPS, seed=0, mutate=None):
    """x [rows, dim], add [rows, terms, dim] (terms = 0: none, v = x), norm weight w [dim], v, the ONE expected normalised row y
    and, where dim % 128 == 0, its e4m3 codes and scales.  mutate (host tests only, the assertions about the mutated part are
    skipped): "w_chunk" = the norm weight of the next 8-element chunk, "drop_term" = the last term left out."""
    assert dim % 64 == 0
    g = torch.Generator().manual_seed(1000003 * rows + 1009 * dim + 17 * terms + seed + (7 if eps != rx.EPS else 0))
    ng, ngc, nb = dim // 128, (dim + 127) // 128, dim // 64
    p = 2 * dx.exps(g, 0, 2, ngc)                                                 # [ngc] in {0, 2, 4}
    tier = (torch.arange(rows)[:, None] + torch.arange(ngc)[None, :] + seed) % 2   # [rows, ngc]
    k = torch.randint(1, 7, (dim,), generator=g) * (torch.randint(0, 2, (dim,), generator=g) * 2 - 1)
    special = torch.zeros(dim, dtype=torch.bool)
    nz = torch.zeros(rows, dim, dtype=torch.bool)
    for gi in range(ng):
        c7, c14 = (torch.randperm(128, generator=g)[:2] + gi * 128).tolist()
        k[c7], k[c14] = 7 * torch.sign(k[c7]), 14 * torch.sign(k[c14])
        special[c7] = special[c14] = True
        nz[:, c7], nz[:, c14] = tier[:, gi] == 0, tier[:, gi] == 1
    # 16 non-zero entries in every 64-block of every row (dim / 4 in all), the specials counted
    score = torch.rand(rows, dim, generator=g)
    score[:, special] = 2.0
    need = 16 - nz.view(rows, nb, 64).sum(-1)
    rank = score.view(rows, nb, 64).argsort(-1).argsort(-1)
    nz = nz | (rank < need[:, :, None]).view(rows, dim)
    assert bool((nz.sum(1) == dim // 4).all()) and bool((nz.view(rows, nb, 64).sum(-1) == 16).all())
    vi = nz.long() * (torch.randint(0, 2, (rows, dim), generator=g) * 2 - 1)
    ce = torch.tensor([ROW_C_EXPS[(r + seed) % len(ROW_C_EXPS)] for r in range(rows)])
    c = dx.pow2(ce)[:, None].double()

    def units(i):
        t = (i.double() * (c if i.dim() == 2 else c[:, None])).to(BF16)
        assert torch.equal(t.double(), i.double() * (c if i.dim() == 2 else c[:, None]))  # bf16-exact integers times the row's unit
        return t

    out = dict(rows=rows, dim=dim, terms=terms, eps=eps, p=p, tier=tier, k=k, c_exp=ce)
    if terms:
        xi = dx.ints(g, 120, rows, dim)
        ai = _split_terms(g, vi - xi, terms, rows, dim)
        out.update(x=units(xi), add=units(ai))
        if mutate == "drop_term":
            vi = xi + ai[:, :-1].sum(1)
        v = rx.residual_oracle(out["x"], rx.sum_terms_oracle(out["add"][:, : terms - 1] if mutate == "drop_term" else out["add"]))
    else:
        out["x"] = v = units(vi)
    assert torch.equal(v.double(), vi.double() * c)  # the residual stream is exact: sum_out is simply the integer sum
    if mutate == "drop_term":
        return dict(v=v)  # (no longer a row of +-c_r: only the residual stream is looked at)
    w = (k.double() * dx.pow2(p).double().repeat_interleave(128)[:dim]).to(BF16)
    if mutate == "w_chunk":
        w = torch.roll(w, -8)
    t, rr, ys = rx.rms_oracle(v, w, eps=eps)
    if mutate is None:
        for cand in ys[1:]:
            assert torch.equal(rx.bits(cand), rx.bits(ys[0])), "an rsqrt candidate changes the row: c_r is too small for this eps"
        closed = (2.0 * vi.double() * w.double()[None, :]).to(BF16)
        assert torch.equal(ys[0].float() + 0.0, closed.float() + 0.0)  # y = +-2 k 2^p (the zeros carry the sign of v w)
    out.update(v=v, w=w, y=ys[0], t=t, rr=rr)
    if dim % 128 == 0:
        q, s = ofp8.act_quant_deepseek_v3(ys[0])
        out.update(codes=q, scales=s)
        if mutate is None:
            assert torch.equal(s, dx.pow2(p[None, :] + tier - 5)), "the group scales are not 2^(p - 5 + tier)"
            deq = (q.float() * s.repeat_interleave(128, 1)).to(BF16)
            assert torch.equal(rx.bits(deq), rx.bits(ys[0])), "dequant(codes, scales) != y"
            assert int(q.float().abs().max()) <= 448 and torch.equal(q.float(), q.float().round())
            for ax in (0, 1):
                n = s.shape[ax]
                if n > 1:
                    assert bool((s.narrow(ax, 0, n - 1) != s.narrow(ax, 1, n - 1)).all()), "neighbouring scales are equal"
    return out


def a_deq(nc, mutate=None):
    """The dequantised activation the fp8 GEMM sees, float64 [rows, dim]; mutations of the REFERENCE (host tests):
    "scale_row" / "scale_group" = the activation scale of the neighbouring row / group, "no_tier" = the tier ignored."""
    s = nc["scales"]
    if mutate == "scale_row":
        s = torch.roll(s, 1, 0)
    elif mutate == "scale_group":
        s = torch.roll(s, 1, 1)
    elif mutate == "no_tier":
        s = dx.pow2(nc["p"][None, :].expand_as(s) - 5)
    return nc["codes"].double() * s.double().repeat_interleave(128, 1)


# ---------------------------------------------------------------- GEMM weights (dense_exact's operands)
def fp8_weight(N, K, seed=0):
    """e4m3 integers -4..4 [N, K], power-of-two scales per [128, 128] block with neighbouring blocks different.  The exponent
    range is dense_exact's, two lower: y reaches 448 here, and every output has to stay inside f16."""
    lo, hi = (e - 2 for e in dx.range_for(K))
    g = torch.Generator().manual_seed(N * 1009 + K + 31 * seed + 5)
    w = dx.ints(g, 4, N, K)
    w_s = dx.pow2(dx.exps(g, lo, hi, (N + 127) // 128, K // 128))
    w_q = w.to(torch.float8_e4m3fn)
    assert torch.equal(w_q.double(), w.double())
    return dict(w_q=w_q, w_s=w_s, lo=lo)


def fp8_w_deq(wc, mutate=None):
    """float64 [N, K]; "w_scale_kb" = the weight scale of the neighbouring K block."""
    w_s = torch.roll(wc["w_s"], 1, 1) if mutate == "w_scale_kb" else wc["w_s"]
    N, K = wc["w_q"].shape
    return wc["w_q"].double() * w_s.double().repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)


def bf16_weight(N, K, seed=0, lo=None, hi=None):
    if lo is None:
        lo, hi = (e - 4 for e in dx.range_for(K))  # (four lower than dense_exact's: |y| <= 448 and f16 outputs)
    g = torch.Generator().manual_seed(N * 1009 + K + 31 * seed + 6)
    w = dx.ints(g, 8, N, K).double() * dx.pow2(dx.exps(g, lo, hi, N, 1)).double()
    w_q = w.to(BF16)
    assert torch.equal(w_q.double(), w)
    return dict(w_q=w_q, lo=lo)


def fp8_exact(nc, wc, mutate_a=None, mutate_w=None):
    """The float64 matmul of the dequantised operands, with the per-output exactness condition asserted (unit: the smallest
    y step 2 = 2^1 times the smallest weight scale)."""
    a, w = a_deq(nc, mutate_a), fp8_w_deq(wc, mutate_w)
    if mutate_a is None and mutate_w is None:
        assert torch.equal(a, nc["y"].double())
        dx._assert_exact(a, w, 1 + wc["lo"], f"fused fp8 {tuple(a.shape)} x {tuple(w.shape)}")
    return a @ w.T


def bf16_exact(nc, wc):
    a, w = nc["y"].double(), wc["w_q"].double()
    dx._assert_exact(a, w, 1 + wc["lo"], f"fused bf16 {tuple(a.shape)} x {tuple(w.shape)}")
    return a @ w.T


def silu_weight(inter, K, seed=0):
    """w13 [2 inter, K]: gate rows then up rows; scales chosen so that the gates (sums of ~K/4 products of |y| <= 448) stay of
    moderate size and SiLU sees its interesting range, as dense_exact.silu_case does for its own activations."""
    lo, hi = (-11, -9) if K <= 1024 else (-12, -10)
    return bf16_weight(2 * inter, K, seed, lo, hi)


def silu_expect(nc, wc, inter):
    """[C, M * inter, 1] candidates of bf16(bf16(silu(bf16(gate))) * bf16(up)), one row per output ELEMENT (every element has its
    own gate), for row_exact.silu_match."""
    exact = bf16_exact(nc, wc)
    gate, up = dx.expect(exact[:, :inter], BF16), dx.expect(exact[:, inter:], BF16)
    return rx.silu_oracle(gate.reshape(-1), up.reshape(-1, 1)), gate


# ---------------------------------------------------------------- the full-mantissa family
@functools.lru_cache(maxsize=64)
def ident_case(rows, dim, terms, seed=0):
    """row_exact.rms_case (its add rows as [rows, terms, dim]) with the candidate rows of its norm and, for dim % 128 == 0, the
    fp32 output of an identity fp8 GEMM behind act_quant of every candidate: codes x scale, one product per element (+ 0.0: the
    accumulator starts at +0, so a -0 code comes out as +0)."""
    c = rx.rms_case(rows, dim, terms, seed)
    t, rr, y = rx.rms_oracle(c["v"], c["w"])
    out = dict(c=c, t=t, rr=rr, y=y)
    if dim % 128 == 0:
        cand = []
        for yc in y:
            q, s = ofp8.act_quant_deepseek_v3(yc)
            cand.append(q.float() * s.repeat_interleave(128, 1) + 0.0)
        out["fp8_out"] = torch.stack(cand)
    out["bf16_out"] = torch.stack([yc.float() + 0.0 for yc in y])
    return out


def ident_fp8_weight(K):
    return torch.eye(K).to(torch.float8_e4m3fn), torch.ones((K + 127) // 128, K // 128)


# ---------------------------------------------------------------- host mirrors of the launchers' choice of instantiation
def fp8_norm_wk(N, K):
    """gemm_plan.h::fp8_norm_gemm_wk: 8, 4, or 0 = not served."""
    tiles, kb = (N + 15) // 16, K // 128
    t = max(1, min(kb, (1536 + tiles - 1) // tiles))
    wk = 1
    while wk * 2 <= t and wk < 8:
        wk *= 2
    if tiles * wk < 256 and N * K >= (24 << 20):
        return 0
    while wk > 1 and wk > kb:
        wk >>= 1
    return wk if wk >= 4 else 0


def fp8_norm_form(M, terms, N, K):
    """(WK, term registers, rows held) of chitu_hip_fp8_gemm_add_norm, or None where it answers CHITU_ERR_UNSUPPORTED."""
    if K % 128 or K > 8192 or terms > 16 or M > 2 or (M == 2 and terms != 1):
        return None
    wk = fp8_norm_wk(N, K)
    if wk == 0:
        return None
    return wk, (1 if M == 2 or terms == 1 else 10 if terms <= 10 else 16), M


def bf16_norm_form(M, N, K, deep=-1):
    """(WK, ring depth, MR) of chitu_hip_bf16_gemm_add_norm[_qkv_post], or None (CHITU_ERR_UNSUPPORTED)."""
    if not (1 <= M <= 4 and K % 64 == 0 and 512 <= K <= 8192 and M * K * 2 <= 48 * 1024):
        return None
    wk = dx.bf16_wk(N, K)
    if wk < 4:
        return None
    tiles, per_wave = (N + 15) // 16, (K // 64) // wk
    is_deep = per_wave <= 8 and (tiles <= 256 if deep < 0 else deep != 0)
    return wk, 8 if is_deep else 4, 1 if M == 1 else 2 if M == 2 else 4


def qproj_blocks(rank):
    """K blocks per wave of mla_q_proj_kernel (wave w takes range t = (w % 4) * 2 + w / 4 of 8)."""
    kb = rank // 128
    return [kb * (t + 1) // 8 - kb * t // 8 for t in [(w & 3) * 2 + (w >> 2) for w in range(8)]]


# ---------------------------------------------------------------- the merge workspace
@functools.lru_cache(maxsize=64)
def merge_case(B, H, S, seed=0, mutate=None):
    """part_o [B H, S, 512] bf16 and lse [B H, S] fp32 (the workspace is their concatenation, bytes), the merged rows
    [B, H, 512] (exact means, bf16-exact: asserted) and the live counts.  (b, h) number `dead` has no live split at all; the
    live splits sit at shuffled positions, one of them on the last or the first split.
    mutate (host tests): "skip_live" = the reference skips the last live split, "nan_through" = it does not mask the empty ones."""
    g = torch.Generator().manual_seed(B * 1000003 + H * 10007 + S * 101 + seed)
    BH = B * H
    counts = [n for n in (1, 2, 4, 8, 16) if n <= S]
    dead = (seed + 1) % BH if BH > 1 else -1
    e = dx.exps(g, -2, 2, B, H, 1).reshape(BH)
    part = torch.empty(BH, S, 512, dtype=BF16)
    lse = torch.empty(BH, S)
    merged = torch.zeros(BH, 512, dtype=torch.float64)
    live_n = torch.zeros(BH, dtype=torch.int64)
    for i in range(BH):
        n = 0 if i == dead else counts[(i + seed) % len(counts)]
        pos = torch.randperm(S, generator=g).tolist()
        edge = S - 1 if i % 2 == 0 else 0   # one live split sits on the last split (even b H + h) or the first: a loop one short sees it
        pos = [edge] + [q for q in pos if q != edge]
        base = float(torch.randint(-8, 9, (1,), generator=g)) * 0.375
        kinds = ["live"] * n + [("empty" if (j + i) % 2 == 0 or n == 0 else "tiny") for j in range(S - n)]
        rows_live = []
        for where, kind in zip(pos, kinds):
            if kind == "live":
                r = dx.ints(g, 8, 512).double() * 2.0 ** int(e[i])
                part[i, where], lse[i, where] = r.to(BF16), base
                rows_live.append(r)
            elif kind == "empty":
                part[i, where], lse[i, where] = float("nan"), float("-inf")
            else:
                part[i, where] = (dx.ints(g, 8, 512).float() * 2.0 ** 100).to(BF16)
                lse[i, where] = base - LSE_GAP
        live_n[i] = n
        if mutate == "skip_live" and n:
            rows_live = rows_live[:-1]
        if rows_live:
            merged[i] = sum(rows_live) / n
        if mutate == "nan_through" and "empty" in kinds:
            merged[i] = float("nan")
    if mutate is None:
        assert torch.equal(merged.to(BF16).double(), merged), "the merged rows do not fit bf16"
    return dict(part=part, lse=lse, merged=merged.view(B, H, 512), live=live_n, dead=dead, e=e.view(B, H))


def merge_workspace(mc):
    """The bytes chitu_hip_mla_decode(out = NULL) leaves: bf16 partial rows, then the fp32 LSE values."""
    return torch.cat([mc["part"].contiguous().view(torch.uint8).reshape(-1), mc["lse"].contiguous().view(torch.uint8).reshape(-1)])


def merge_expect(mc, ac):
    """(codes [B, H 128] e4m3, scales [B, H]) = act_quant_deepseek_v3(bf16(exact W_UV projection of the merged rows));
    ac = dense_exact.absorb_case(B, H, 128, 512, ...) for its weights and scales."""
    x, w = mc["merged"], ac["w_deq"]
    B, H, _ = x.shape
    if not bool(torch.isnan(x).any()):
        dx._assert_exact(x.transpose(0, 1), w, -2 - 4 - 2, f"merge + W_UV {B}x{H}")
    exact = torch.einsum("bhk,hnk->bhn", x, w)
    if bool(torch.isnan(exact).any()):
        return ofp8.act_quant_deepseek_v3(exact.float().to(BF16).reshape(B, H * 128).contiguous())
    return ofp8.act_quant_deepseek_v3(dx.expect(exact, BF16).reshape(B, H * 128).contiguous())


# ---------------------------------------------------------------- the shapes of the GPU tests
OUT3 = dx.OUT3
ALIAS = ["own", "x", "add"]

# A: chitu_hip_bf16_gemm_add_norm -- (M, N, K, terms, deep option, sum_out placement, second output type, (WK, ring, MR))
A_K = [512, 576, 1024, 4096, 8192]
A_N = [1, 16, 40, 136]
A_CASES = []
for _i, (_m, _k) in enumerate((m, k) for m, k in itertools.product([1, 2, 3, 4], A_K) if m * k <= 24576):
    _terms = 2 if _i % 3 == 1 else 1
    A_CASES.append((_m, A_N[(_i + _i // 4) % 4], _k, _terms, -1, ALIAS[_i % 3] if _terms == 1 else ALIAS[(_i // 3) % 2],
                    OUT3[1 + _i % 2], (8, 8 if _k <= 4096 else 4, 1 if _m == 1 else 2 if _m == 2 else 4)))
A_CASES += [
    (3, 4112, 1024, 1, -1, "own", "bf16", (8, 4, 4)),    # 257 tiles: the 4-deep ring by the tile rule
    (1, 4112, 4096, 2, -1, "x", "f16", (8, 4, 1)),       # ... with 8 blocks per wave
    (2, 8208, 512, 1, -1, "add", "bf16", (4, 4, 2)),     # 513 tiles x 8 waves > 4096: WK = 4
    (4, 8208, 512, 2, 1, "own", "f16", (4, 8, 4)),       # both ring depths at both WK through the bf16_gemm_deep option
    (1, 8208, 512, 1, 0, "x", "bf16", (4, 4, 1)),
    (3, 40, 1024, 2, 0, "own", "bf16", (8, 4, 4)),
    (2, 136, 4096, 1, 1, "add", "f16", (8, 8, 2)),
    (1, 16, 576, 1, 0, "own", "f16", (8, 4, 1)),
]

# B: chitu_hip_bf16_gemm_silu_add_norm -- (M, inter, K, sum_out placement, (WK, MR))
B_INTER = [8, 40, 136]
B_CASES = [(m, B_INTER[(i + i // 3) % 3], k, ALIAS[i % 3], (8, 1 if m == 1 else 2 if m == 2 else 4))
           for i, (m, k) in enumerate((m, k) for m, k in itertools.product([1, 2, 3, 4], A_K) if m * k <= 24576)] + [
    (1, 4112, 512, "own", (8, 1)), (3, 4112, 1024, "x", (8, 4))]

# C: chitu_hip_bf16_gemm_add_norm_qkv_post -- (q heads, kv heads, head_dim, K, M, page size, table variant)
C_HEADS = [(4, 4, 64), (8, 2, 128), (2, 1, 16)]
C_CASES = [(hq, hkv, d, k, m, [16, 48][i % 2], "valid" if m < 4 else ["valid", "out-of-table-0", "out-of-table-1"][(i // 3) % 3])
           for i, ((hq, hkv, d), k, m) in enumerate(itertools.product(C_HEADS, [512, 1024], [1, 2, 4]))]

# D: chitu_hip_fp8_gemm_add_norm -- (M, terms, N, K, second output type, (WK, term registers, MR))
D_MT = [(1, 1), (1, 2), (1, 9), (1, 10), (1, 11), (1, 16), (2, 1)]
D_K = [512, 640, 1024, 2048, 7168, 8192]
D_N = [16, 40, 136, 2112]
D_CASES = [(m, t, D_N[(i + j) % 4], k, OUT3[1 + (i + j) % 2],
            (4 if k < 1024 else 8, 1 if t == 1 else 10 if t <= 10 else 16, m))
           for i, (m, t) in enumerate(D_MT) for j, k in enumerate(D_K)] + [
    (1, 1, 3520, 1024, "bf16", (4, 1, 1)),    # 220 tiles: 193..384 tiles is WK = 4 by the tile rule, at K >= 1024
    (2, 1, 3520, 2048, "f16", (4, 1, 2)),
    (1, 16, 3520, 1024, "bf16", (4, 16, 1)),
    (1, 10, 3520, 2048, "f16", (4, 10, 1)),
]
D_REFUSED = [(2, 2, 136, 1024), (3, 1, 136, 1024), (1, 1, 136, 8320), (1, 1, 136, 256), (1, 1, 16400, 1024), (1, 17, 136, 1024)]
D_IDENT = [(1, 512, 1), (2, 1024, 1), (1, 2048, 3), (1, 640, 16)]   # (M, K = N, terms)
A_IDENT = [(1, 512, 1), (4, 1024, 1), (3, 576, 1), (2, 2048, 1)]    # (M, K = N, terms)

# E: chitu_hip_mla_q_proj -- (batch, q_lora_rank, N, second output type, out-of-table batch?)
E_BATCH = [1, 5, 16, 17, 32]
E_RANK = [128, 384, 896, 1024, 1152, 1536, 2048]
E_N = [1, 16, 40, 200, 1536]
E_CASES = [(b, r, E_N[(i + i // 5) % 5], OUT3[1 + i % 2], i % 3 == 1)
           for i, (r, b) in enumerate(itertools.product(E_RANK, E_BATCH))]
E_IDENT = [(5, 128), (16, 384), (17, 1024), (32, 1536), (3, 2048)]   # (batch, q_lora_rank = N)
E_REFUSED = [(33, 1536), (4, 2176), (4, 192)]

# F: chitu_hip_absorb_bmm_rope_kv_fp8 -- (B, H, N, K, scale strides, out-of-table batch?)
F_BH = [(1, 1), (16, 5), (17, 1), (1, 5), (16, 1), (17, 5)]
F_NK = [(16, 128), (128, 192), (512, 128), (16, 192), (128, 128), (512, 192)]
F_CASES = [(*F_BH[i % 6], *F_NK[(i + i // 6) % 6], ["w_uk", "w_uv", "distinct"][i % 3], i % 2 == 1 and F_BH[i % 6][0] >= 4)
           for i in range(12)]

# G: the merge -- (batch, heads, S, scale strides)
G_S = [2, 3, 16, 17, 64, 65, 130]
G_BH = [(1, 1), (15, 5), (16, 1), (17, 5), (1, 16), (16, 5), (17, 1)]
G_CASES = [(b, h, s, ["w_uv", "distinct"][(i + j) % 2]) for i, s in enumerate(G_S) for j, (b, h) in enumerate(G_BH)
           if (i + j) % 2 == 0 or s in (2, 17)] + [(15, 16, 3, "w_uv"), (2, 16, 65, "w_uv")]
