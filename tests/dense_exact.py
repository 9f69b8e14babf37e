"""Builders and exact references for the dense GEMM family on integer data (no GPU needed).

Operands are small integers (-4..4 in e4m3 / int8, -8..8 in bf16) and every scale is a power of two, so every product is a
multiple of one power of two u and, with sum_k |a w| / u < 2^24 for every output element (asserted by every builder, never
measured), every partial sum in any order is exactly representable in fp32: whatever the wave split, plane order or tile shape,
the fp32 accumulator holds THE matmul.  The expectation is that matmul in float64, rounded once (round-to-nearest-even) to the
output type.  Scale exponents are lo + (p[i] + q[j]) % R with p and q walks whose consecutive steps are non-zero mod R: the
scales of two neighbouring tokens, N blocks or K blocks always differ, so a scale read from the neighbour changes the result.

tests/test_dense_exact_host.py checks these constructions against the CPU references and against reference mutations;
tests/test_gpu_dense_exact.py runs the kernels on them.  The shape lists of both live here.
"""

import functools
import itertools

import torch

G = 4                    # guard rows on each side of an output
SENTINEL16 = 0x7FA5      # a bf16 / f16 NaN bit pattern (as the expert tests use)
SENTINEL32 = 0x7FC5A5A5  # an fp32 NaN bit pattern
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DT_CODE = {"bf16": 0, "f16": 1, "f32": 2}
F16_MAX = 65504.0


# ---------------------------------------------------------------- operands
def ints(g, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=g)


def _walk(g, n, R):
    """n residues mod R, consecutive ones different."""
    steps = torch.randint(1, R, (n,), generator=g)
    return torch.cumsum(steps, 0) % R


def exps(g, lo, hi, *shape):
    """Exponents in lo..hi, any two neighbours along any axis different."""
    R = hi - lo + 1
    assert R >= 3
    e = torch.zeros(shape, dtype=torch.int64)
    for ax, n in enumerate(shape):
        view = [1] * len(shape)
        view[ax] = n
        e = e + _walk(g, n, R).view(view)
    e = lo + e % R
    for ax, n in enumerate(shape):
        if n > 1:
            assert bool((e.narrow(ax, 0, n - 1) != e.narrow(ax, 1, n - 1)).all())
    return e


def pow2(e):
    return torch.ldexp(torch.ones(e.shape), e.to(torch.int32))


def _assert_exact(a_deq, w_deq, lo_sum, what, extra=None):
    """The exactness condition, per output element: sum_k |a w| (+ |extra|) in units of u = 2^lo_sum is below 2^24."""
    mag = a_deq.abs() @ w_deq.abs().transpose(-1, -2)
    if extra is not None:
        mag = mag + extra.abs()
    worst = float(mag.max()) / 2.0 ** lo_sum
    assert worst < 2 ** 24, f"{what}: sum |a w| / u = {worst:.3e} >= 2^24: narrow the exponent range of this case"


def expect(exact, dtype):
    """float64 -> dtype, rounded once: the value is an fp32 number (asserted), so the only rounding is fp32 -> dtype (RNE)."""
    f = exact.float()
    assert torch.equal(f.double(), exact)
    if dtype == torch.float16:
        assert float(exact.abs().max()) < F16_MAX
    return f.to(dtype)


def range_for(K):
    """Exponent range per side for a contraction length: the short ones take 2^-2..2^2, the long ones a narrower range."""
    return (-2, 2) if K <= 2048 else (-1, 1)


def fp8_case(M, N, K, lim=4):
    """e4m3 activations [M, K] with scales per (row, 128-group), e4m3 weights [N, K] with scales per [128, 128] block.
    lim: the integers are drawn from -lim..lim (the 2^20-long contraction takes -1..1 to stay below 2^24)."""
    return (_fp8_case if N * K > (1 << 22) else _fp8_case_cached)(M, N, K, lim)  # (the 25 MB cases are not kept)


def _fp8_case(M, N, K, lim):
    lo, hi = range_for(K)
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
    KB, NB = K // 128, (N + 127) // 128
    a, w = ints(g, lim, M, K), ints(g, lim, N, K)
    a_s, w_s = pow2(exps(g, lo, hi, M, KB)), pow2(exps(g, lo, hi, NB, KB))
    a_q, w_q = a.to(torch.float8_e4m3fn), w.to(torch.float8_e4m3fn)
    assert torch.equal(a_q.double(), a.double()) and torch.equal(w_q.double(), w.double())
    a_deq = a.double() * a_s.double().repeat_interleave(128, 1)
    w_deq = w.double() * w_s.double().repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)
    _assert_exact(a_deq, w_deq, 2 * lo, f"fp8 {M}x{N}x{K}")
    return dict(a_q=a_q, a_s=a_s, w_q=w_q, w_s=w_s, a_deq=a_deq, w_deq=w_deq, exact=a_deq @ w_deq.T, lo=lo, hi=hi)


_fp8_case_cached = functools.lru_cache(maxsize=64)(_fp8_case)


def soft_case(M, N, K, lim=4):
    """bf16 activations (a power of two per row folded in), e4m3 weights with [128, 128] block scales."""
    return (_soft_case if N * K > (1 << 22) else _soft_case_cached)(M, N, K, lim)


def _soft_case(M, N, K, lim):
    lo, hi = range_for(K)
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K + 1)
    KB, NB = K // 128, (N + 127) // 128
    a = ints(g, lim, M, K).double() * pow2(exps(g, lo, hi, M, 1)).double()
    w = ints(g, lim, N, K)
    w_s = pow2(exps(g, lo, hi, NB, KB))
    a_q, w_q = a.to(torch.bfloat16), w.to(torch.float8_e4m3fn)
    assert torch.equal(a_q.double(), a) and torch.equal(w_q.double(), w.double())
    w_deq = w.double() * w_s.double().repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)
    assert torch.equal(w_deq.to(torch.bfloat16).double(), w_deq)  # the kernel's bf16 weight is exact too
    _assert_exact(a, w_deq, 2 * lo, f"soft fp8 {M}x{N}x{K}")
    return dict(a_q=a_q, w_q=w_q, w_s=w_s, a_deq=a, w_deq=w_deq, exact=a @ w_deq.T, lo=lo, hi=hi)


_soft_case_cached = functools.lru_cache(maxsize=64)(_soft_case)


@functools.lru_cache(maxsize=64)
def bf16_case(M, N, K, lo=None, hi=None):
    """bf16 activations and weights: integers in -8..8 times a power of two per row."""
    if lo is None:
        lo, hi = range_for(K)
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K + 2)
    a = ints(g, 8, M, K).double() * pow2(exps(g, lo, hi, M, 1)).double()
    w = ints(g, 8, N, K).double() * pow2(exps(g, lo, hi, N, 1)).double()
    a_q, w_q = a.to(torch.bfloat16), w.to(torch.bfloat16)
    assert torch.equal(a_q.double(), a) and torch.equal(w_q.double(), w)
    _assert_exact(a, w, 2 * lo, f"bf16 {M}x{N}x{K}")
    return dict(a_q=a_q, w_q=w_q, a_deq=a, w_deq=w, exact=a @ w.T, lo=lo, hi=hi)


def silu_case(M, inter, K):
    """x [M, K] and w13 [2 inter, K] (gate rows, then up rows) with scales 2^-4..2^-2 on both sides: gate and up are exact
    multiples of 2^-8 of moderate size, so SiLU sees its whole interesting range."""
    return bf16_case(M, 2 * inter, K, -4, -2)


@functools.lru_cache(maxsize=64)
def int8_case(M, N, K):
    """int8 activations with a scale per row, int8 weights with a scale per output channel, an integer bias."""
    lo, hi = -2, 2
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K + 3)
    a, w = ints(g, 4, M, K), ints(g, 4, N, K)
    a_s, w_s = pow2(exps(g, lo, hi, M)), pow2(exps(g, lo, hi, N))
    bias = ints(g, 8, N).double()
    a_deq, w_deq = a.double() * a_s.double()[:, None], w.double() * w_s.double()[:, None]
    _assert_exact(a_deq, w_deq, 2 * lo, f"int8 {M}x{N}x{K}", extra=bias[None, :])
    return dict(a_q=a.to(torch.int8), a_s=a_s, w_q=w.to(torch.int8), w_s=w_s, bias=bias, a_deq=a_deq, w_deq=w_deq,
                exact=a_deq @ w_deq.T, lo=lo, hi=hi)


ABSORB_STRIDES = {   # name -> (stride_h, stride_n, stride_k) of the flat scale tensor; the first two are the model's
    "w_uk": (8, 1, 0),      # wkv_b's W_UK half transposed: the N blocks walk the scale row, one K block
    "w_uv": (8, 0, 1),      # the W_UV half: one N block, the K blocks walk the scale row
    "distinct": (23, 5, 1),
}
ABSORB_OFFSET = 3


@functools.lru_cache(maxsize=64)
def absorb_case(B, H, N, K, strides):
    """x [B, H, K] bf16 as a view of a wider tensor (q[..., :K]), w [H, N, K] e4m3 with a head stride above N K, the scales
    somewhere in a NaN-filled flat tensor: any index but the right one reads a NaN."""
    lo, hi = -2, 2
    sh, sn, sk = ABSORB_STRIDES[strides]
    g = torch.Generator().manual_seed(B * 1000003 + H * 10007 + N * 1009 + K + 4 + len(strides))
    NB, KB = (N + 127) // 128, (K + 127) // 128
    assert (sn == 0 or sn > (KB - 1) * sk) and sh > (NB - 1) * sn + (KB - 1) * sk
    wide = torch.zeros(B, H, K + 64, dtype=torch.bfloat16)
    wide[..., :K] = (ints(g, 8, B, H, K).double() * pow2(exps(g, lo, hi, B, H, 1)).double()).to(torch.bfloat16)
    wide[..., K:] = float("nan")
    x = wide[..., :K]
    w_store = torch.full((H, N * K + 48), 0x7F, dtype=torch.uint8)  # (0x7F: the e4m3fn NaN)
    w = ints(g, 4, H, N, K)
    w_store[:, : N * K] = w.to(torch.float8_e4m3fn).view(torch.uint8).reshape(H, N * K)
    e = exps(g, lo, hi, H, NB if sn else 1, KB if sk else 1)
    flat = torch.full((ABSORB_OFFSET + H * sh + 1,), float("nan"))
    s_full = torch.zeros(H, NB, KB, dtype=torch.float64)
    for h, nb, kb in itertools.product(range(H), range(NB), range(KB)):
        v = pow2(e[h, nb if sn else 0, kb if sk else 0])
        flat[ABSORB_OFFSET + h * sh + nb * sn + kb * sk] = v
        s_full[h, nb, kb] = v
    w_deq = w.double() * s_full.repeat_interleave(128, 1)[:, :N].repeat_interleave(128, 2)[:, :, :K]
    x_deq = x.double()
    _assert_exact(x_deq.transpose(0, 1), w_deq, 2 * lo, f"absorb {B}x{H}x{N}x{K}")
    exact = torch.einsum("bhk,hnk->bhn", x_deq, w_deq)
    return dict(x=x, w_store=w_store, w=w.to(torch.float8_e4m3fn), scale=flat, strides=(sh, sn, sk), x_deq=x_deq, w_deq=w_deq,
                exact=exact, lo=lo, hi=hi)


def rope_case(B, H, seed):
    """q_pe [B + 2 G, H, 64] bf16 integers (the rows of the first and last G tokens are guards), cos / sin [B, 32] drawn from
    the four exact rotations (1, 0), (0, 1), (-1, 0), (0, -1): the rotation is a signed permutation of each pair."""
    g = torch.Generator().manual_seed(seed)
    q = ints(g, 8, B + 2 * G, H, 64).to(torch.bfloat16)
    pick = torch.randint(0, 4, (B, 32), generator=g)
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[pick]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[pick]
    want = q.clone()
    x0, x1 = q[G:G + B, :, 0::2].float(), q[G:G + B, :, 1::2].float()
    c, s = cos[:, None, :], sin[:, None, :]
    want[G:G + B, :, 0::2] = (x0 * c - x1 * s).to(torch.bfloat16)
    want[G:G + B, :, 1::2] = (x1 * c + x0 * s).to(torch.bfloat16)
    return q, cos, sin, want


# ---------------------------------------------------------------- layouts and guarded outputs
def to_tile_major(q, s):
    """Row-major fp8 activations [M, K] / scales [M, K/128] -> the tile-major pair of fp8_gemm.hip:
    X[m / 16][K / 16][m % 16][16 B], XS[m / 16][K / 128][m % 16]; the inverse of ops.TiledQuant.to_row_major.  The rows that
    pad the last tile hold NaN codes and NaN scales (no kernel may use them)."""
    M, K = q.shape
    t = (M + 15) // 16
    qp = torch.full((t * 16, K), 0x7F, dtype=torch.uint8)
    qp[:M] = q.view(torch.uint8)
    sp = torch.full((t * 16, K // 128), float("nan"), dtype=torch.float32)
    sp[:M] = s
    qt = qp.view(t, 16, K // 16, 16).permute(0, 2, 1, 3).contiguous().view(t * 16, K).view(torch.float8_e4m3fn)
    st = sp.view(t, 16, K // 128).permute(0, 2, 1).contiguous()
    return qt, st


def guarded(rows, cols, dtype, planes=None, device="cuda"):
    """(whole buffer, interior view handed to the kernel): G sentinel rows, the output rows pre-filled with the same
    sentinel (an element the kernel never wrote is seen), G sentinel rows.  planes: the interior is [planes, rows, cols]
    and the guards are whole rows before plane 0 and after the last plane."""
    n = rows * (planes or 1)
    wide = dtype == torch.float32
    full = torch.full((n + 2 * G, cols), SENTINEL32 if wide else SENTINEL16, dtype=torch.int32 if wide else torch.int16,
                      device=device)
    inner = full[G:G + n].view(dtype)
    return full, (inner.view(planes, rows, cols) if planes else inner)


def check_guarded(full, dtype, what, planes=None):
    """After the launch: both guards untouched, no interior element still the sentinel; returns the interior on the CPU."""
    got = full.cpu()
    sentinel = SENTINEL32 if dtype == torch.float32 else SENTINEL16
    n = got.shape[0] - 2 * G
    for side, rows in (("before", got[:G]), ("after", got[G + n:])):
        touched = (rows != sentinel).nonzero()
        assert len(touched) == 0, f"{what}: stored into the guard rows {side} the output, first (row, col): {touched[:8].tolist()}"
    inner = got[G:G + n]
    unwritten = (inner == sentinel).nonzero()
    assert len(unwritten) == 0, f"{what}: {len(unwritten)} output elements never written, first (row, col): {unwritten[:8].tolist()}"
    inner = inner.view(dtype)
    return inner.view(planes, n // planes, inner.shape[1]) if planes else inner


def differs(got, want):
    """The comparison of the GPU tests: anything but torch.equal is a difference."""
    return not torch.equal(got, want)


def assert_equal(got, want, what):
    """torch.equal, and on failure the worst row and the first few positions."""
    if torch.equal(got, want):
        return
    g2, w2 = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    bad = ~((g2 == w2))
    rows = bad.sum(1)
    pos = bad.nonzero()[:6]
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result in {int((rows > 0).sum())} rows; worst row "
        f"{int(rows.argmax())} ({int(rows.max())} elements); first (row, col, got, want): "
        f"{[(int(r), int(c), float(g2[r, c]), float(w2[r, c])) for r, c in pos]}")


# ---------------------------------------------------------------- host mirrors of the launchers' plans
def plan_split(N, K):
    """gemm_plan.h::fp8_split_plan: (WK, S)."""
    tiles, kb = (N + 15) // 16, (K + 127) // 128
    t = max(1, min(kb, (1536 + tiles - 1) // tiles))
    wk = 1
    while wk * 2 <= t and wk < 8:
        wk *= 2
    s = 1
    if tiles * wk < 256 and N * K >= (24 << 20):
        s = min(8, (t + wk - 1) // wk)
        if s * wk > kb:
            s = kb // wk if kb // wk > 0 else 1
    return wk, s


def fp8_wk(N, K, forced=-1, S=1):
    """The WK chitu_hip_fp8_gemm_blockscale launches with (after its option and the KB clamp)."""
    wk = plan_split(N, K)[0] if forced < 0 else forced
    while wk > 1 and wk * S > K // 128:
        wk >>= 1
    return wk


def partials_ranges(K, S):
    """K ranges [k0, k1) of the planes of chitu_hip_fp8_gemm_blockscale_partials (tests/test_gpu_fp8.py's formula)."""
    KB = K // 128
    T = S * (8 if KB >= 8 * S else 4 if KB >= 4 * S else 2 if KB >= 2 * S else 1)
    return [((KB * (s * (T // S)) // T) * 128, (KB * ((s + 1) * (T // S)) // T) * 128) for s in range(S)]


def bf16_tiled_ranges(K, S):
    """64-wide K blocks of split s of the tiled bf16 GEMM: ceil(KB / S) blocks each, the last shares short or empty."""
    KB = K // 64
    per = (KB + S - 1) // S
    return [(min(s * per, KB) * 64, min((s + 1) * per, KB) * 64) for s in range(S)]


def bf16_stream_ranges(K, S):
    """K ranges of the planes of the streaming bf16 GEMM: wave t of S WK covers blocks [KB t / (S WK), KB (t + 1) / (S WK)),
    plane s the waves s WK .. (s + 1) WK - 1: [floor(KB s / S), floor(KB (s + 1) / S)) whatever WK."""
    KB = K // 64
    return [(KB * s // S * 64, KB * (s + 1) // S * 64) for s in range(S)]


# ---------------------------------------------------------------- the shapes of the GPU tests
def _cycle(ms, wks, ns, ks, dts, kblock):
    """Every (m, wk) pair once, at a K with at least wk blocks of kblock so that the launcher's `WK <= KB` clamp leaves the
    forced value alone: the pair that is asked for is the pair that is launched.  N, K and the output type cycle so that
    every (N, type) pair and every value occur."""
    out = []
    for i, (m, wk) in enumerate(itertools.product(ms, wks)):
        fits = [k for k in ks if k // kblock >= wk]
        out.append((m, ns[i % len(ns)], fits[(i + i // len(ks)) % len(fits)], wk, dts[(i // len(ns)) % len(dts)]))
    return out


def passes(M, rows):
    """Rows left at the start of each pass of a streaming launcher that takes `rows` token rows per pass."""
    return [M - mb for mb in range(0, M, rows)]


def fp8_tile_form(rem):
    """MT of a pass of the fp8 streaming GEMM (64 rows per pass) with rem rows left."""
    return 1 if rem <= 16 else 2 if rem <= 32 else 4


def bf16_tile_form(rem):
    """MT of a pass of the bf16 / SiLU / soft fp8 / int8 streaming GEMMs (32 rows per pass)."""
    return 1 if rem <= 16 else 2


def bf16_wk(N, K, forced=-1, S=1):
    """The WK chitu_hip_bf16_gemm (streaming) and chitu_hip_bf16_gemm_silu (S = 1, N = inter) launch with."""
    tiles, KB, wk = (N + 15) // 16, K // 64, 8
    while wk > 1 and (wk * S > KB or tiles * S * wk > 4096):
        wk >>= 1
    if forced >= 0:
        wk = forced
    while wk > 1 and wk * S > KB:
        wk >>= 1
    return wk


def bf16_deep(M, N, K, wk, S=1, deep=-1):
    """Does a pass with at most 16 rows left take the DEEP ring of the streaming bf16 GEMM?"""
    per_wave = (K // 64) // (wk * S)
    return wk == 8 and 4 < per_wave <= 8 and (((N + 15) // 16) * S <= 256 if deep < 0 else deep != 0)


OUT3 = ["f32", "bf16", "f16"]
WKS = [-1, 1, 2, 4, 8]
A_M = [1, 15, 16, 17, 32, 33, 64, 65, 127]
A_CASES = _cycle(A_M, WKS, [8, 129, 136, 272], [128, 384, 1024, 5120], OUT3, 128)            # (M, N, K, wk, dtype)
A_DEEP = [(m, n, 5120, wk, deep, dt) for (m, n, dt), wk, deep in
          itertools.product([(1, 272, "bf16"), (15, 129, "f32"), (16, 136, "f16")], [-1, 8], [0, 1])]
B_M = [1, 16, 17, 32, 33, 64, 65]   # (32: a second shape of the 32-row form, which of the issue's list only 17 takes)
B_CASES = _cycle(B_M, WKS, [8, 129, 136, 272], [128, 384, 1024, 5120], OUT3, 128)
B_DEEP = [(m, n, 5120, wk, deep, dt) for (m, n, dt), wk, deep in
          itertools.product([(1, 136, "f32"), (16, 129, "bf16")], [-1, 8], [0, 1])]
C_CASES = [(m, n, k, s) for i, (m, (k, s)) in enumerate(itertools.product([1, 17, 33, 70], [(384, 2), (384, 3), (2048, 2), (2048, 3), (2048, 16)]))
           for n in [[129, 136][i % 2]]]                                                   # (M, N, K, S), S <= KB
D_SHAPES = [(496, 50816, 4), (24, 1048576, 1)]                                             # (N, K, integer limit)
D_CASES = [(m, n, k, lim, dt) for (n, k, lim), (m, dt) in itertools.product(D_SHAPES, [(1, "f32"), (17, "bf16")])]
E_CASES = [(m, n, [128, 384, 1024][(p + t) % 3], tm, OUT3[(p + 2 * t) % 3])                # (M, N, K, fp8_tiled_tm, dtype):
           for p, (m, n) in enumerate([(128, 8), (129, 129), (191, 136), (257, 264), (128, 264), (257, 8)])
           for t, tm in enumerate([-1, 64, 128])]                                          # every K at every tile height
F_M = [1, 16, 17, 32, 33, 49, 255]
F_STREAM = _cycle(F_M, WKS, [8, 129, 130, 136, 272], [64, 192, 512, 2560], OUT3, 64)          # (M, N, K, wk, dtype)
F_DEEP = [(m, n, 2560, wk, deep, dt) for (m, n, dt), wk, deep in
          itertools.product([(1, 272, "bf16"), (16, 130, "f32")], [-1, 8], [0, 1])]
F_SPLIT_K = [512, 2560, 7680]   # 8, 40 and 120 blocks of 64
F_SPLIT = [(m, [8, 129, 130, 136][i % 4], fits[(i + i // 4) % len(fits)], s, wk)              # (M, N, K, S, wk), launched WK = wk
           for i, ((m, s), wk) in enumerate(itertools.product(itertools.product([1, 17, 33, 255], [3, 8]), [-1, 2, 4, 8]))
           for fits in [[k for k in F_SPLIT_K if k // 64 >= max(wk, 1) * s]]] + [
    (1, 136, 7680, 3, -1), (16, 130, 7680, 3, 8)]   # 120 blocks over 3 x 8 waves = 5 per wave: the DEEP ring at S > 1
F_TILED = [(m, n, k, s, tm, dt) for i, (((m, n), k), tm) in enumerate(itertools.product(
    itertools.product([(256, 136), (257, 264), (300, 8), (129, 1032)], [64, 320, 1024]), [64, 128]))
    for s, dt in [(1, OUT3[i % 3])]] + [
    (m, n, k, s, tm, "f32") for (m, n), (k, s), tm in itertools.product(
        [(257, 264), (300, 8)], [(320, 3), (320, 4), (1024, 3), (1024, 4)], [64, 128])]
G_M = [1, 16, 17, 33, 255, 32]   # 32 (last: the cases before it keep their shapes): one full two-tile launch, no row guarded
G_CASES = [(m, [8, 136, 1000][i % 3], fits[(i + i // 3) % len(fits)], wk) for i, (m, wk) in enumerate(itertools.product(G_M, WKS))
           for fits in [[k for k in [64, 512, 2560] if k // 64 >= wk]]]                    # (M, inter, K, wk), launched WK = wk
H_CASES = [(m, n, k, OUT3[(i + i // 6) % 3]) for i, (m, (n, k)) in enumerate(itertools.product(
    [1, 16, 17, 32, 33, 70], [(8, 128), (129, 384), (136, 640), (8, 1024), (129, 1024), (136, 384)]))]
I_BMM = [(b, h, n, k, st) for i, (b, (n, k)) in enumerate(itertools.product(
    [1, 16, 17, 33], [(8, 128), (128, 192), (136, 512), (512, 128), (512, 512), (136, 192)]))
    for h, st in [([1, 3][i % 2], ["w_uk", "w_uv", "distinct"][i % 3])]]
I_UV = [(b, h, k, st) for b, (h, k, st) in itertools.product([1, 16, 21], [(3, 512, "w_uv"), (1, 256, "distinct"), (3, 256, "w_uv")])]
J_SHAPES = [(40, 128), (40, 512), (1000, 384), (16400, 128), (16400, 256)]   # WK 1, 4, 2, 1 (KB = 1), 2
J_CASES = [(m, n, k, bias, dt) for i, (m, (n, k)) in enumerate(itertools.product([1, 16, 17, 33, 40], J_SHAPES))
           for bias, dt in [([None, "bf16", "f16", "f32"][(i + i // 5) % 4], OUT3[i % 3])]]   # (M, N, K, bias dtype, out dtype)


def fp8_shapes():
    """Every (M, N, K, lim) a fp8 builder is asked for by the GPU tests."""
    s = {(m, n, k, 4) for m, n, k, *_ in A_CASES + A_DEEP + B_CASES + B_DEEP + C_CASES + E_CASES}
    return sorted(s | {(m, n, k, lim) for m, n, k, lim, _ in D_CASES})
