"""The constructions of tests/dense_exact.py checked on the CPU: a construction the reference cannot pass is a bug in the test.

1. every builder at every shape tests/test_gpu_dense_exact.py uses: values exact in their storage type, the 2^24 bound, the
   f16 range where f16 is the output (the builders assert these themselves; here they are all run);
2. the project's CPU references return the float64 expectation exactly on these inputs;
3. the tile-major permutation inverts ops.TiledQuant.to_row_major;
4. sensitivity: six mutations of the reference's inputs each change the expectation in every case, under the very comparison
   the GPU tests make (torch.equal on the fp32 output, which every GPU case takes besides its own output type);
5. the host mirror of plan_split gives S > 1 exactly for the shapes of the in-library split, and the case lists cover every
   value and pair they promise;
6. csrc/gemm_plan.h, compiled by a host compiler into a stand-alone driver, gives the plans of these mirrors.
"""

import itertools
import os
import shutil
import subprocess

import pytest
import torch

from oracle import fp8 as ofp8
from oracle import w8a8 as ow
from tests import cpu_ops_shim as shim
from tests import dense_exact as dx
from tests import fused_exact as fx

FP8_SHAPES = dx.fp8_shapes()
SOFT_SHAPES = sorted({(m, n, k, 4) for m, n, k, _ in dx.H_CASES} | {(m, n, k, lim) for m, n, k, lim, _ in dx.D_CASES})
BF16_SHAPES = sorted({(m, n, k) for m, n, k, *_ in dx.F_STREAM + dx.F_DEEP + dx.F_SPLIT + dx.F_TILED})
SILU_SHAPES = sorted({(m, i, k) for m, i, k, _ in dx.G_CASES})
INT8_SHAPES = sorted({(m, n, k) for m, n, k, _, _ in dx.J_CASES})
ABSORB_SHAPES = sorted(set(dx.I_BMM) | {(b, h, 128, k, st) for b, h, k, st in dx.I_UV})


def _id(shape):
    return "-".join(str(v) for v in shape)


# ---------------------------------------------------------------- mutations of a reference's inputs
def _live_k(c):
    """The first k at which some activation and some weight are non-zero: zeroing it changes at least one product."""
    live = (c["a_deq"] != 0).any(0) & (c["w_deq"] != 0).any(0)
    return int(live.nonzero()[0])


def _mutations(c, a_scale=None, w_scale=None):
    """name -> the float64 matmul of the mutated inputs.  a_scale / w_scale: [M, KB] / [NB, KB] float64 scale tensors
    where the format has them (the scale mutations need them), with the unscaled integers in a_int / w_int."""
    a, w = c["a_deq"], c["w_deq"]
    M, K = a.shape
    N = w.shape[0]
    out = {}
    k = _live_k(c)
    a0 = a.clone()
    a0[:, k] = 0
    out["one k element zeroed"] = a0 @ w.T
    if M >= 2:
        out["row m from token m + 1"] = torch.cat([a[1:], a[-1:]]) @ w.T
    blk = 128
    out["last K block dropped"] = a[:, : K - min(blk, K)] @ w[:, : K - min(blk, K)].T if K > blk else torch.zeros(M, N, dtype=torch.float64)
    if a_scale is not None and M >= 2:
        s = a_scale.clone()
        s[[0, 1]] = s[[1, 0]]
        out["two adjacent tokens' scales swapped"] = (c["a_int"] * s.repeat_interleave(K // s.shape[1], 1)) @ w.T
    if w_scale is not None:
        NB, KB = w_scale.shape
        if KB >= 2:
            s = torch.cat([w_scale[:, 1:], w_scale[:, -1:]], 1)
            out["weight scale of K block kb from kb + 1"] = a @ (c["w_int"] * s.repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)[:, :K]).T
        if NB >= 2:
            s = torch.cat([w_scale[1:], w_scale[-1:]], 0)
            out["weight scale of N block nb from nb + 1"] = a @ (c["w_int"] * s.repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)[:, :K]).T
    return out


def _assert_sensitive(c, muts, what, dtype=torch.float32):
    want = dx.expect(c["exact"], dtype)
    for name, mutated in muts.items():
        assert dx.differs(mutated.float().to(dtype), want), f"{what}: the expectation survives '{name}': the inputs are too weak"


# ---------------------------------------------------------------- fp8 W8A8 (sections A to E)
@pytest.mark.parametrize("shape", FP8_SHAPES, ids=_id)
def test_fp8_builder_matches_the_oracle_and_every_mutation_changes_it(shape):
    M, N, K, lim = shape
    c = dx.fp8_case(M, N, K, lim)
    want = dx.expect(c["exact"], torch.float32)
    assert torch.equal(ofp8.fp8_gemm_deepseek_v3(c["a_q"], c["a_s"], c["w_q"], c["w_s"], torch.float32), want)
    assert torch.equal(shim.fp8_gemm_deepseek_v3(c["a_q"], c["a_s"], c["w_q"], c["w_s"]), dx.expect(c["exact"], torch.bfloat16))
    c = dict(c, a_int=c["a_q"].double(), w_int=c["w_q"].double())
    muts = _mutations(c, c["a_s"].double(), c["w_s"].double())
    assert len(muts) == 2 + 2 * (M >= 2) + (K > 128) + (N > 128)
    _assert_sensitive(c, muts, f"fp8 {shape}")


def test_fp8_cases_take_f16_only_inside_its_range():
    for m, n, k, *rest in dx.A_CASES + dx.A_DEEP + dx.B_CASES + dx.B_DEEP + dx.E_CASES:
        dx.expect(dx.fp8_case(m, n, k)["exact"], dx.DTYPES[rest[-1]])
    for m, n, k, dt in dx.H_CASES:
        dx.expect(dx.soft_case(m, n, k)["exact"], dx.DTYPES[dt])
    for m, n, k, *rest in dx.F_STREAM + dx.F_DEEP:
        dx.expect(dx.bf16_case(m, n, k)["exact"], dx.DTYPES[rest[-1]])
    for m, n, k, s, tm, dt in dx.F_TILED:
        dx.expect(dx.bf16_case(m, n, k)["exact"], dx.DTYPES[dt])
    for m, n, k, bias, dt in dx.J_CASES:
        c = dx.int8_case(m, n, k)
        dx.expect(c["exact"] + (0 if bias is None else c["bias"][None, :]), dx.DTYPES[dt])


@pytest.mark.parametrize("case", dx.C_CASES, ids=_id)
def test_fp8_partial_planes_are_exact_and_sum_to_the_gemm(case):
    M, N, K, S = case
    c = dx.fp8_case(M, N, K)
    ranges = dx.partials_ranges(K, S)
    assert ranges[0][0] == 0 and ranges[-1][1] == K and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert all(k1 > k0 for k0, k1 in ranges), "an empty plane: S <= KB must hold"
    planes = [c["a_deq"][:, k0:k1] @ c["w_deq"][:, k0:k1].T for k0, k1 in ranges]
    assert torch.equal(sum(planes), c["exact"])
    for (k0, k1), p in zip(ranges, planes):
        ref = ofp8.fp8_gemm_deepseek_v3(c["a_q"][:, k0:k1].contiguous(), c["a_s"][:, k0 // 128:k1 // 128].contiguous(),
                                        c["w_q"][:, k0:k1].contiguous(), c["w_s"][:, k0 // 128:k1 // 128].contiguous(), torch.float32)
        assert torch.equal(ref, dx.expect(p, torch.float32))


# ---------------------------------------------------------------- soft fp8 (sections H and D)
@pytest.mark.parametrize("shape", SOFT_SHAPES, ids=_id)
def test_soft_fp8_builder_matches_the_oracle_and_every_mutation_changes_it(shape):
    M, N, K, lim = shape
    c = dx.soft_case(M, N, K, lim)
    assert torch.equal(ofp8.soft_fp8_gemm_deepseek_v3(c["a_q"], c["w_q"], c["w_s"], torch.float32), dx.expect(c["exact"], torch.float32))
    c = dict(c, w_int=c["w_q"].double())
    muts = _mutations(c, None, c["w_s"].double())
    assert len(muts) == 2 + (M >= 2) + (K > 128) + (N > 128)
    _assert_sensitive(c, muts, f"soft fp8 {shape}")


# ---------------------------------------------------------------- bf16 (sections F and G)
@pytest.mark.parametrize("shape", BF16_SHAPES, ids=_id)
def test_bf16_builder_matches_linear_and_every_mutation_changes_it(shape):
    M, N, K = shape
    c = dx.bf16_case(M, N, K)
    assert torch.equal(torch.nn.functional.linear(c["a_q"].float(), c["w_q"].float()), dx.expect(c["exact"], torch.float32))
    assert torch.equal(shim.bf16_linear(c["a_q"], c["w_q"]), dx.expect(c["exact"], torch.bfloat16))
    muts = _mutations(c)
    muts["last K block dropped"] = c["a_deq"][:, : K - 64] @ c["w_deq"][:, : K - 64].T  # (this family's K block is 64 wide)
    _assert_sensitive(c, muts, f"bf16 {shape}")


@pytest.mark.parametrize("case", dx.F_SPLIT + [c[:5] for c in dx.F_TILED if c[3] > 1], ids=_id)
def test_bf16_split_ranges_tile_the_contraction(case):
    M, N, K, S = case[:4]
    for ranges in (dx.bf16_stream_ranges(K, S), dx.bf16_tiled_ranges(K, S)):
        assert ranges[0][0] == 0 and ranges[-1][1] == K and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert S <= K // 64
    if (K, S) == (320, 4):
        assert [(k1 - k0) // 64 for k0, k1 in dx.bf16_tiled_ranges(K, S)] == [2, 2, 1, 0]  # the empty share


@pytest.mark.parametrize("shape", SILU_SHAPES, ids=_id)
def test_silu_builder_is_exact_and_within_range(shape):
    M, inter, K = shape
    c = dx.silu_case(M, inter, K)
    h = dx.expect(c["exact"], torch.bfloat16)
    assert torch.equal(shim.bf16_linear(c["a_q"], c["w_q"]), h)
    assert torch.isfinite(shim.bf16_linear_silu(c["a_q"], c["w_q"]).float()).all()
    muts = _mutations(c)
    muts["last K block dropped"] = c["a_deq"][:, : K - 64] @ c["w_deq"][:, : K - 64].T  # (this family's K block is 64 wide)
    _assert_sensitive(c, muts, f"silu {shape}")


# ---------------------------------------------------------------- int8 (section J)
@pytest.mark.parametrize("shape", INT8_SHAPES, ids=_id)
def test_int8_builder_matches_the_oracle_and_every_mutation_changes_it(shape):
    M, N, K = shape
    c = dx.int8_case(M, N, K)
    for bias in (None, c["bias"].float()):
        want = dx.expect(c["exact"] + (0 if bias is None else c["bias"][None, :]), torch.float32)
        assert torch.equal(ow.w8a8_linear(c["a_q"], c["a_s"], c["w_q"], c["w_s"], bias, torch.float32), want)
    c = dict(c, a_int=c["a_q"].double(), w_int=c["w_q"].double())
    muts = _mutations(c)
    if M >= 2:
        s = c["a_s"].double().clone()
        s[[0, 1]] = s[[1, 0]]
        muts["two adjacent tokens' scales swapped"] = (c["a_int"] * s[:, None]) @ c["w_deq"].T
    s = torch.cat([c["w_s"][1:], c["w_s"][-1:]]).double()
    muts["channel scale n from n + 1"] = c["a_deq"] @ (c["w_int"] * s[:, None]).T
    _assert_sensitive(c, muts, f"int8 {shape}")


# ---------------------------------------------------------------- absorb (section I)
@pytest.mark.parametrize("shape", ABSORB_SHAPES, ids=_id)
def test_absorb_builder_matches_the_shim_and_every_mutation_changes_it(shape):
    B, H, N, K, st = shape
    c = dx.absorb_case(B, H, N, K, st)
    sh, sn, sk = c["strides"]
    want = dx.expect(c["exact"], torch.bfloat16)
    assert torch.equal(shim.absorb_bmm_fp8(c["x"], c["w"], c["scale"], dx.ABSORB_OFFSET, sh, sn, sk), want)
    assert not torch.isfinite(c["scale"][: dx.ABSORB_OFFSET]).any() and torch.isnan(c["scale"]).sum() > 0
    if N == 128 and sn == 0:
        q, s = shim.absorb_uv_quant_fp8(c["x"], c["w"], c["scale"], dx.ABSORB_OFFSET, sh, sk)
        q2, s2 = ofp8.act_quant_deepseek_v3(want.reshape(B, H * 128).contiguous())
        assert torch.equal(q.view(torch.uint8), q2.view(torch.uint8)) and torch.equal(s, s2) and torch.isfinite(s).all() and bool((s > 0).all())
    # the output is bf16 only: the mutations must show after that rounding
    x, w = c["x_deq"], c["w_deq"]
    live = ((x != 0).any(0) & (w != 0).any(1)).nonzero()[0]  # (h, k)
    x0 = x.clone()
    x0[:, live[0], live[1]] = 0
    muts = {"one k element zeroed": torch.einsum("bhk,hnk->bhn", x0, w),
            "last K block dropped": torch.einsum("bhk,hnk->bhn", x[..., : K - 64], w[..., : K - 64])}
    if B >= 2:
        muts["row m from token m + 1"] = torch.einsum("bhk,hnk->bhn", torch.cat([x[1:], x[-1:]]), w)
    if H >= 2:
        muts["head h from head h + 1's weights"] = torch.einsum("bhk,hnk->bhn", x, torch.cat([w[1:], w[-1:]]))
    for name, m in muts.items():
        assert dx.differs(m.float().to(torch.bfloat16), want), f"absorb {shape}: the expectation survives '{name}'"
    # a scale taken from any other index is a NaN or, for a neighbouring block, another power of two
    flat = c["scale"]
    for h, nb, kb in itertools.product(range(H), range((N + 127) // 128), range((K + 127) // 128)):
        i = dx.ABSORB_OFFSET + h * sh + nb * sn + kb * sk
        for j in {i + sn, i + sk, i + sh} - {i}:
            if j < flat.numel():
                assert not (flat[j] == flat[i]), (shape, h, nb, kb)


def test_rope_case_is_a_signed_permutation():
    q, cos, sin, want = dx.rope_case(17, 3, seed=1)
    assert bool(((cos == 0) != (sin == 0)).all()) and torch.equal(cos * cos + sin * sin, torch.ones_like(cos))
    G = dx.G
    assert torch.equal(want[:G], q[:G]) and torch.equal(want[-G:], q[-G:]) and not torch.equal(want, q)
    pairs_in = q[G:-G].float().view(17, 3, 32, 2).abs().sort(-1).values
    pairs_out = want[G:-G].float().view(17, 3, 32, 2).abs().sort(-1).values
    assert torch.equal(pairs_in, pairs_out)


# ---------------------------------------------------------------- layouts, guards
@pytest.mark.parametrize("M", dx.B_M)
def test_tile_major_permutation_inverts_to_row_major(M):
    from chitu_amd import ops

    K = 384
    c = dx.fp8_case(M, 136, K)
    qt, st = dx.to_tile_major(c["a_q"], c["a_s"])
    t = (M + 15) // 16
    assert tuple(qt.shape) == (t * 16, K) and tuple(st.shape) == (t, K // 128, 16)
    q, s = ops.TiledQuant(qt, st, M, K).to_row_major()
    assert torch.equal(q.view(torch.uint8), c["a_q"].view(torch.uint8)) and torch.equal(s, c["a_s"])
    # the stated layout, element by element: X[m / 16][K / 16][m % 16][16 B], XS[m / 16][K / 128][m % 16]
    flat = qt.view(torch.uint8).reshape(-1)
    for m, k in [(0, 0), (M - 1, K - 1), (M // 2, 17), (M - 1, 130)]:
        assert flat[(((m // 16) * (K // 16) + k // 16) * 16 + m % 16) * 16 + k % 16] == c["a_q"].view(torch.uint8)[m, k]
        assert st.reshape(-1)[((m // 16) * (K // 128) + k // 128) * 16 + m % 16] == c["a_s"][m, k // 128]
    if M % 16:
        assert torch.isnan(st[-1, :, M % 16:]).all()  # the padding rows of the last tile are poisoned


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_guarded_sees_unwritten_and_stray_elements(dt):
    dtype = dx.DTYPES[dt]
    full, inner = dx.guarded(5, 7, dtype, device="cpu")
    assert tuple(inner.shape) == (5, 7) and torch.isnan(inner.float()).all() and full.shape[0] == 5 + 2 * dx.G
    with pytest.raises(AssertionError, match="never written"):
        dx.check_guarded(full, dtype, "x")
    inner.fill_(1.0)
    assert torch.equal(dx.check_guarded(full, dtype, "x"), torch.ones(5, 7, dtype=dtype))
    for row in (dx.G - 1, dx.G + 5):
        full2 = full.clone()
        full2[row, 0] = 0
        with pytest.raises(AssertionError, match="guard rows"):
            dx.check_guarded(full2, dtype, "x")
    full, inner = dx.guarded(5, 7, dtype, planes=3, device="cpu")
    assert tuple(inner.shape) == (3, 5, 7) and full.shape[0] == 15 + 2 * dx.G
    inner.fill_(2.0)
    assert tuple(dx.check_guarded(full, dtype, "x", planes=3).shape) == (3, 5, 7)
    with pytest.raises(AssertionError, match="worst row 1"):
        dx.assert_equal(torch.tensor([[1.0, 2.0], [3.0, 4.0]]), torch.tensor([[1.0, 2.0], [0.0, 0.0]]), "x")


# ---------------------------------------------------------------- plans and coverage
def test_plan_split_mirror_and_the_shapes_that_take_the_in_library_split():
    from chitu_amd import ops

    assert dx.plan_split(496, 50816) == (8, 7) and dx.plan_split(24, 1048576) == (8, 8)
    d_shapes = {(n, k) for n, k, _ in dx.D_SHAPES}
    for m, n, k, _ in FP8_SHAPES + SOFT_SHAPES:
        wk, s = dx.plan_split(n, k)
        assert (s > 1) == ((n, k) in d_shapes), (n, k, wk, s)
    assert dx.plan_split(512, 7168) == (8, 1)  # the largest shape of the older tests: tiles * WK == 256
    # the mirror in ops (fp8_linear_add_norm_fits) agrees wherever it applies: it refuses exactly the split shapes
    for n, k in [(2112, 7168), (496, 7168), (3072, 1536), (16, 8192), (3200, 8192)]:
        wk, s = dx.plan_split(n, k)
        assert ops.fp8_linear_add_norm_fits(1, n, k) == (s == 1 and wk >= 4), (n, k)
    # the soft GEMM's plan takes WK 1, 2, 4 and 8 on the shapes of section H; the int8 launcher 1, 4, 2, 1 and 2 on section J
    # ((16400, 128) has one K block, which clamps the 1024-tile rule's WK = 2 to 1: (16400, 256) is there to reach it)
    assert {dx.plan_split(n, k)[0] for _, n, k, _ in dx.H_CASES} == {1, 2, 4, 8}
    wks = []
    for n, k in dx.J_SHAPES:
        tiles, wk = (n + 15) // 16, 0
        wk = 2 if tiles >= 1024 else 4 if tiles >= 384 else 8
        while wk > 1 and wk > k // 128:
            wk >>= 1
        wks.append(wk)
    assert wks == [1, 4, 2, 1, 2]


def test_case_lists_cover_every_value_and_pair():
    """The pairs are those that are LAUNCHED: the token-tile form of every pass of a case and the WK left after the launcher's
    option and its `WK <= KB` clamp, from the host mirrors of the launchers."""
    forms4, forms2, wks = [1, 2, 4], [1, 2], [1, 2, 4, 8]
    for cases, ms, ns, ks in ((dx.A_CASES, dx.A_M, [8, 129, 136, 272], [128, 384, 1024, 5120]),
                              (dx.B_CASES, dx.B_M, [8, 129, 136, 272], [128, 384, 1024, 5120]),
                              (dx.F_STREAM, dx.F_M, [8, 129, 130, 136, 272], [64, 192, 512, 2560])):
        assert {c[0] for c in cases} == set(ms) and {c[1] for c in cases} == set(ns) and {c[2] for c in cases} == set(ks)
        assert {(c[0], c[3]) for c in cases} == set(itertools.product(ms, dx.WKS))
        assert {(c[1], c[4]) for c in cases} == set(itertools.product(ns, dx.OUT3))
    assert set(dx.B_M) >= {1, 16, 17, 33, 64, 65}
    for cases in (dx.A_CASES, dx.B_CASES):
        assert all(wk < 0 or dx.fp8_wk(n, k, wk) == wk for _, n, k, wk, _ in cases), "a forced WK is clamped"
        launched = {(dx.fp8_tile_form(r), dx.fp8_wk(n, k, wk)) for m, n, k, wk, _ in cases for r in dx.passes(m, 64)}
        assert launched == set(itertools.product(forms4, wks)), sorted(launched)
        assert {dx.fp8_wk(n, k, -1) for _, n, k, wk, _ in cases if wk < 0} == {1, 2, 8}  # (the heuristic: 1, 3, 8 and 40 K blocks)
    assert any(m > 64 for m in dx.A_M) and any(m > 64 for m in dx.B_M)  # a second 64-row pass (m_base = 64)
    assert all(wk < 0 or dx.bf16_wk(n, k, wk) == wk for _, n, k, wk, _ in dx.F_STREAM)
    launched = {(dx.bf16_tile_form(r), dx.bf16_wk(n, k, wk)) for m, n, k, wk, _ in dx.F_STREAM for r in dx.passes(m, 32)}
    assert launched == set(itertools.product(forms2, wks)), sorted(launched)
    assert all(wk < 0 or dx.bf16_wk(i, k, wk) == wk for _, i, k, wk in dx.G_CASES)
    launched = {(dx.bf16_tile_form(r), dx.bf16_wk(i, k, wk)) for m, i, k, wk in dx.G_CASES for r in dx.passes(m, 32)}
    assert launched == set(itertools.product(forms2, wks)), sorted(launched)
    launched = {(dx.bf16_tile_form(r), dx.plan_split(n, k)[0]) for m, n, k, _ in dx.H_CASES for r in dx.passes(m, 32)}
    assert launched == set(itertools.product(forms2, wks)), sorted(launched)
    # the streaming split-K planes: both forms at launched WK 2, 4 and 8 under both plane counts, and the DEEP ring at S > 1
    assert all(wk < 0 or dx.bf16_wk(n, k, wk, s) == wk for _, n, k, s, wk in dx.F_SPLIT)
    launched = {(dx.bf16_tile_form(r), dx.bf16_wk(n, k, wk, s), s) for m, n, k, s, wk in dx.F_SPLIT for r in dx.passes(m, 32)}
    assert launched >= set(itertools.product(forms2, [2, 4, 8], [3, 8])), sorted(launched)
    assert any(dx.bf16_deep(m, n, k, dx.bf16_wk(n, k, wk, s), s) for m, n, k, s, wk in dx.F_SPLIT if m <= 16)
    for m, n, k, wk, deep, _ in dx.F_DEEP:
        assert m <= 16 and dx.bf16_deep(m, n, k, dx.bf16_wk(n, k, wk), 1, 1) and not dx.bf16_deep(m, n, k, dx.bf16_wk(n, k, wk), 1, 0)
    for m, n, k, wk, deep, _ in dx.A_DEEP + dx.B_DEEP:
        assert m <= 16 and dx.fp8_wk(n, k, wk) == 8 and 4 < (k // 128) // 8 <= 8
    assert {(c[2], c[3]) for c in dx.E_CASES} == set(itertools.product([128, 384, 1024], [-1, 64, 128]))
    assert {(c[1], c[4]) for c in dx.E_CASES} >= set(itertools.product([8, 136, 264], dx.OUT3))
    assert {c[0] for c in dx.E_CASES} == {128, 129, 191, 257} and {c[2] for c in dx.E_CASES} == {128, 384, 1024}
    assert {c[3] for c in dx.E_CASES} == {-1, 64, 128} and {c[1] for c in dx.E_CASES} == {8, 129, 136, 264}
    assert {(c[0], c[3]) for c in dx.C_CASES} >= set(itertools.product([1, 17, 33, 70], [2, 3, 16])) and {c[1] for c in dx.C_CASES} == {129, 136}
    assert all(s <= k // 128 for _, _, k, s in dx.C_CASES)
    assert {(c[0], c[3]) for c in dx.G_CASES} == set(itertools.product(dx.G_M, dx.WKS))
    assert {c[1] for c in dx.G_CASES} == {8, 136, 1000} and {c[2] for c in dx.G_CASES} == {64, 512, 2560}
    assert {c[0] for c in dx.H_CASES} == {1, 16, 17, 32, 33, 70} and {c[1] for c in dx.H_CASES} == {8, 129, 136}
    assert {c[2] for c in dx.H_CASES} == {128, 384, 640, 1024}
    assert {(c[1], c[3]) for c in dx.H_CASES} == set(itertools.product([8, 129, 136], dx.OUT3))
    assert {c[0] for c in dx.I_BMM} == {1, 16, 17, 33} and {c[1] for c in dx.I_BMM} == {1, 3}
    assert {c[2] for c in dx.I_BMM} == {8, 128, 136, 512} and {c[3] for c in dx.I_BMM} == {128, 192, 512}
    assert {c[4] for c in dx.I_BMM} == set(dx.ABSORB_STRIDES)
    assert {(c[0], c[2]) for c in dx.I_UV} == set(itertools.product([1, 16, 21], [512, 256]))
    assert {(c[1], c[2]) for c in dx.J_CASES} == set(dx.J_SHAPES) and {c[0] for c in dx.J_CASES} == {1, 16, 17, 33, 40}
    assert {c[3] for c in dx.J_CASES} == {None, "bf16", "f16", "f32"} and {c[4] for c in dx.J_CASES} == set(dx.OUT3)
    assert {(c[3], c[4]) for c in dx.F_TILED} == set(itertools.product([1, 3, 4], [64, 128]))
    assert {(c[0], c[1]) for c in dx.F_TILED} == {(256, 136), (257, 264), (300, 8), (129, 1032)}
    assert {(c[3], c[4]) for c in dx.F_SPLIT} == set(itertools.product([3, 8], [-1, 2, 4, 8])) and {c[0] for c in dx.F_SPLIT} == {1, 16, 17, 33, 255}


# ---------------------------------------------------------------- csrc/gemm_plan.h against the mirrors
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CXX = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("c++")
FORCED = [-1, 1, 2, 4, 8]
PLAN_DRIVER = r"""
#include <cstdio>
#include <initializer_list>
#include "gemm_plan.h"
using namespace chitu;
int main() {
    char mode;
    long a, b;
    auto show = [](int mb, auto mt, auto wk) { printf("%d:%d:%d ", mb, decltype(mt)::value, decltype(wk)::value); };
    while (scanf(" %c %ld %ld", &mode, &a, &b) == 3) {
        if (mode == 'w') {  // a rows under WK b: (m_base, MT, WK) of every pass, 32-row then 64-row passes
            stream_walk_m<32>(a, (int)b, show);
            printf("| ");
            stream_walk_m<64>(a, (int)b, show);
            printf("\n");
            continue;
        }
        const long N = a, K = b;
        const SplitPlan p = fp8_split_plan(N, K);
        printf("%d %d %d", p.WK, p.S, fp8_norm_gemm_wk(N, K));
        if (mode == 'p') {  // every other rule; a workspace that holds any split, then none
            for (long ws : {1l << 62, 0l})
                for (int forced : {-1, 1, 2, 4, 8}) {
                    const SplitPlan q = fp8_stream_plan(1, N, K, ws, forced);
                    printf(" %d %d %d %d", q.WK, q.S, (int)fp8_deep(q, K, -1), (int)fp8_deep(q, K, 0));
                }
            const SplitPlan q = fp8_plan_in_workspace(1, N, K, 0);
            printf(" %d %d", q.WK, q.S);
            for (int s : {2, 3, 16}) printf(" %d", fp8_partials_plan(K, s).WK);
            printf(" %d", w8a8_int8_wk(N, K));
            for (int s : {1, 3, 8}) printf(" %d", stream_wk((N + 15) / 16, K / 64, s));
        }
        printf("\n");
    }
}
"""


def _plan_grid():
    nk = {(c[1], c[2]) for c in dx.A_CASES + dx.B_CASES + dx.C_CASES + dx.H_CASES} | {(n, k) for n, k, _ in dx.D_SHAPES}
    nk |= set(dx.J_SHAPES) | {(c[2], c[3]) for c in fx.D_CASES} | {(c[2], c[3]) for c in fx.D_REFUSED if c[3] % 128 == 0}
    nk |= {(2112, 7168), (3072, 1536), (7168, 2048), (4608, 7168), (7168, 2304)}   # the DeepSeek shapes of tools/bench_kernels.py
    return sorted(nk)


def _int8_wk(N, K):
    """The rule behind dx.J_SHAPES' comment."""
    tiles = (N + 15) // 16
    wk = 2 if tiles >= 1024 else 4 if tiles >= 384 else 8
    while wk > 1 and wk > K // 128:
        wk >>= 1
    return wk


def _partials_wk(K, S):
    """The waves per plane inside dx.partials_ranges."""
    KB = K // 128
    return 8 if KB >= 8 * S else 4 if KB >= 4 * S else 2 if KB >= 2 * S else 1


@pytest.mark.skipif(not HOST_CXX or not os.path.exists(HOST_CXX), reason="needs a host C++ compiler")
def test_gemm_plan_header_gives_the_plans_of_the_mirrors(tmp_path):
    """gemm_plan.h is the one C++ statement of the launch rules; the mirrors of dense_exact / fused_exact and
    ops.fp8_linear_add_norm_fits stay independent statements, and here they are held against each other.  The sweep shows
    that the fused entry's refusal `fp8_split_plan gives S > 1` is the predicate it replaced, `tiles * WK < 256 and
    N * K >= 24 Mi`, over every K the entry admits (and that over K = 128 * 2^i, 50816, 28672 with under 300 tiles the
    predicate never holds with S == 1): fx.fp8_norm_wk still states the predicate."""
    from chitu_amd import ops

    (tmp_path / "driver.cpp").write_text(PLAN_DRIVER)
    res = subprocess.run([HOST_CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "chitu_amd", "csrc"),
                          str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    grid = _plan_grid()
    sweep = [(16 * t, k) for k in range(128, 8192 + 1, 128) for t in range(1, 4096 + 1)]
    wide = [(16 * t, k) for k in [128 << i for i in range(14)] + [50816, 28672] for t in range(1, 300)]
    ms = sorted({c[0] for c in dx.A_CASES + dx.B_CASES + dx.C_CASES + dx.H_CASES + dx.J_CASES} | set(range(1, 70)) | {255, 256})
    walks = [(m, wk) for m in ms for wk in (1, 2, 4, 8)]
    text = "".join(f"p {n} {k}\n" for n, k in grid) + "".join(f"n {n} {k}\n" for n, k in sweep + wide)
    text += "".join(f"w {m} {wk}\n" for m, wk in walks)
    res = subprocess.run([str(tmp_path / "driver")], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")
    assert len(lines) == len(grid) + len(sweep) + len(wide) + len(walks) + 1

    for (N, K), line in zip(grid, lines):
        got = [int(v) for v in line.split()]
        wk, s = dx.plan_split(N, K)
        want = [wk, s, fx.fp8_norm_wk(N, K)]
        for s_eff in (s, 1):
            for forced in FORCED:
                w = dx.fp8_wk(N, K, forced, s_eff)
                want += [w, s_eff, int(w == 8 and 4 < (K // 128) // (w * s_eff) <= 8), 0]
        want += [wk, 1] + [_partials_wk(K, sp) for sp in (2, 3, 16)] + [_int8_wk(N, K)]
        want += [dx.bf16_wk(N, K, -1, sp) for sp in (1, 3, 8)]
        assert got == want, (N, K, got, want)
    for n, k, _ in dx.D_SHAPES:
        assert dx.plan_split(n, k)[1] > 1   # the grid holds in-library splits
    assert [_int8_wk(n, k) for n, k in dx.J_SHAPES] == [1, 4, 2, 1, 2]
    for m, n, k, s in dx.C_CASES:
        assert (dx.partials_ranges(k, s)[1][0] // 128) == (k // 128) * _partials_wk(k, s) // (s * _partials_wk(k, s))

    refused_by_split = 0
    for (N, K), line in zip(sweep + wide, lines[len(grid):]):
        wk, s, norm_wk = (int(v) for v in line.split())
        assert (wk, s) == dx.plan_split(N, K) and norm_wk == fx.fp8_norm_wk(N, K), (N, K, line)
        predicate = ((N + 15) // 16) * wk < 256 and N * K >= (24 << 20)
        assert not (predicate and s == 1), (N, K)
        refused_by_split += predicate
        if K <= 8192:
            assert not predicate and ops.fp8_linear_add_norm_fits(1, N, K) == (norm_wk != 0), (N, K)
    assert refused_by_split > 0   # (outside the fused entry's K range the predicate does hold, always with S > 1)

    for (M, WK), line in zip(walks, lines[len(grid) + len(sweep) + len(wide):]):
        got32, got64 = ([tuple(int(v) for v in p.split(":")) for p in half.split()] for half in line.split("|"))
        assert got32 == [(M - r, dx.bf16_tile_form(r), WK) for r in dx.passes(M, 32)], (M, WK, got32)
        assert got64 == [(M - r, dx.fp8_tile_form(r), WK) for r in dx.passes(M, 64)], (M, WK, got64)
