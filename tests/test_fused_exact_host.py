"""CPU checks of tests/fused_exact.py: the builders' promises on every shape of the GPU lists, the expectation against the
composition of the existing CPU oracles, the host mirrors of the launchers' choice of instantiation, and reference mutations
that the case data must tell apart (each test states its count)."""

import numpy as np
import pytest
import torch

from oracle import fp8 as ofp8
from tests import dense_exact as dx
from tests import fused_exact as fx
from tests import row_exact as rx

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _fp8_norm_shapes():
    """Every (rows, dim, terms) a norm_case is asked for by sections D and E."""
    s = {(m, k, t) for m, t, _, k, _, _ in fx.D_CASES}
    return sorted(s | {(b, r, 0) for b, r, *_ in fx.E_CASES})


def _bf16_norm_shapes():
    return sorted({(m, k, t) for m, _, k, t, *_ in fx.A_CASES} | {(m, k, 1) for m, _, k, *_ in fx.B_CASES})


# ---------------------------------------------------------------- the exact normalised row
@pytest.mark.parametrize("eps", fx.EPS_LIST)
def test_norm_case_promises_hold_on_every_shape(eps):
    """The builder's own assertions (candidate collapse, power-of-two scales, dequant == y, neighbouring scales differ, exact
    operands) run for every shape of the lists and for the dims of the issue; here the rest: dim/4 entries +-c_r, the mean
    square c_r^2 / 4, and x / add / terms that sum to v in the kernels' order."""
    shapes = _fp8_norm_shapes() + _bf16_norm_shapes() + [(3, d, t) for d in (128, 512, 1536, 2048) for t in (0, 1, 2, 16)]
    for rows, dim, terms in shapes:
        c = fx.norm_case(rows, dim, terms, eps)
        v = c["v"].double()
        cr = torch.ldexp(torch.ones(rows), c["c_exp"].int()).double()
        assert bool(((v != 0).sum(1) == dim // 4).all()) and bool(((v == 0) | (v.abs() == cr[:, None])).all())
        assert torch.equal((v ** 2).mean(1), cr ** 2 / 4)
        if terms:
            assert c["add"].shape == (rows, terms, dim)
            assert torch.equal(rx.bits(rx.residual_oracle(c["x"], rx.sum_terms_oracle(c["add"]))), rx.bits(c["v"]))
            units = torch.cat([c["x"][:, None], c["add"]], 1).double() / cr[:, None, None]
            assert torch.equal(units, units.round()) and float(units.abs().max()) <= 255
        _, _, y = rx.rms_oracle(c["v"], c["w"], eps=eps)
        assert len(y) == 2 * rx.RSQRT_RADIUS + 1 and all(torch.equal(rx.bits(yc), rx.bits(c["y"])) for yc in y)
        if rows > 1:
            assert len(set(c["c_exp"][:2].tolist())) == 2
        if dim % 128 == 0:
            q, s = rx.quant_fp8(c["y"], 0)
            assert torch.equal(q.view(torch.uint8), c["codes"].view(torch.uint8)) and torch.equal(s, c["scales"])
            m, _ = np.frexp(s.numpy())
            assert bool((m == 0.5).all())


def test_rsqrt_candidates_collapse_with_a_wider_radius_too():
    """The margin is not one ulp wide: 64 candidates on each side still give the one row (d ~ 2e-5 against 2^-9)."""
    for eps in fx.EPS_LIST:
        c = fx.norm_case(4, 1536, 1, eps)
        _, rr, y = rx.rms_oracle(c["v"], c["w"], eps=eps, radius=64)
        assert len(set(rr[:, 0].tolist())) == 129 and all(torch.equal(rx.bits(yc), rx.bits(c["y"])) for yc in y)


# ---------------------------------------------------------------- expectation == composition of the existing oracles
def test_fp8_expectation_is_the_composition_of_the_oracles():
    """residual_oracle -> rms_oracle -> quant_fp8 -> float64 matmul -> expect, and oracle/fp8.py's own GEMM (fp32, another
    summation order) gives the same bits: the data is exact."""
    for m, t, n, k, dt, _ in fx.D_CASES:
        if n > 136 and k > 2048:
            continue  # (the 17 M-element weights are built by the builder test below)
        c, w = fx.norm_case(m, k, t), fx.fp8_weight(n, k)
        v = rx.residual_oracle(c["x"], rx.sum_terms_oracle(c["add"]))
        y = rx.rms_oracle(v, c["w"], eps=c["eps"])[2][0]
        q, s = rx.quant_fp8(y, 0)
        a = q.double() * s.double().repeat_interleave(128, 1)
        wd = ofp8.weight_dequant_deepseek_v3(w["w_q"], w["w_s"], F32).double()
        exact = a @ wd.T
        assert torch.equal(exact, fx.fp8_exact(c, w))
        for d in (F32, dx.DTYPES[dt]):
            want = dx.expect(exact, d)
            assert torch.equal(ofp8.fp8_gemm_deepseek_v3(q, s, w["w_q"], w["w_s"], d), want), (m, t, n, k, d)


def test_every_listed_case_builds_and_fits_every_output_type():
    n = 0
    for m, t, N, k, dt, _ in fx.D_CASES:
        exact = fx.fp8_exact(fx.norm_case(m, k, t), fx.fp8_weight(N, k))
        for d in (F32, BF16, F16):
            dx.expect(exact, d)
        n += 1
    for m, N, k, t, *_ in fx.A_CASES:
        exact = fx.bf16_exact(fx.norm_case(m, k, t), fx.bf16_weight(N, k))
        for d in (F32, BF16, F16):
            dx.expect(exact, d)
        n += 1
    for b, r, N, dt, _ in fx.E_CASES:
        exact = fx.fp8_exact(fx.norm_case(b, r, 0, fx.EPS_LIST[b % 2], seed=1), fx.fp8_weight(N, r))
        for d in (F32, BF16, F16):
            dx.expect(exact, d)
        n += 1
    for hq, hkv, d, k, m, _, _ in fx.C_CASES:
        dx.expect(fx.bf16_exact(fx.norm_case(m, k, 1), fx.bf16_weight((hq + 2 * hkv) * d, k)), BF16)
        n += 1
    for b, h, N, k, st, _ in fx.F_CASES:
        dx.expect(dx.absorb_case(b, h, N, k, st)["exact"], BF16)
        n += 1
    print(f"FUSEDEXACT host: {n} GEMM cases built, every exactness condition holds")


def test_silu_gates_cover_the_interesting_range():
    small = big = 0
    for m, inter, k, *_ in fx.B_CASES:
        if inter > 136:
            continue
        cand, gate = fx.silu_expect(fx.norm_case(m, k, 1), fx.silu_weight(inter, k), inter)
        g = gate.float().abs()
        small, big = small + int((g < 1).sum()), big + int((g > 8).sum())
        assert cand.shape == (2 * rx.EXPF_RADIUS + 1, m * inter, 1) and float(g.max()) < 88  # (no expf overflow: finite factors)
    assert small > 100 and big > 100, (small, big)


def test_identity_family_is_one_product_per_element():
    for rows, k, t in fx.D_IDENT + fx.A_IDENT:
        ic = fx.ident_case(rows, k, t)
        y = ic["y"]
        if k % 128 == 0:
            wq, ws = fx.ident_fp8_weight(k)
            for ci, yc in enumerate(y):
                q, s = rx.quant_fp8(yc, 0)
                assert torch.equal(ofp8.fp8_gemm_deepseek_v3(q, s, wq, ws, F32), ic["fp8_out"][ci])
        assert torch.equal(ic["bf16_out"][0], (y[0].float() @ torch.eye(k)))
        # the rows carry full mantissas: the e4m3 quantisation is NOT exact here, unlike norm_case's
        assert int((y[0].float().abs().view(torch.int32) & 0xFFFF0000 != 0).sum()) > 0


# ---------------------------------------------------------------- reference mutations
def test_reference_mutations_change_the_fp8_expectation():
    """Counts: with the lists as they are, 46 D cases: the neighbouring group's activation scale, the neighbouring K block's
    weight scale, the next chunk's norm weight and the ignored tier change all 46 (every case has >= 4 groups), the
    neighbouring row's activation scale all 7 two-row cases, a dropped term all 46 (sum_out)."""
    seen = dict(scale_group=0, scale_row=0, w_scale_kb=0, no_tier=0, w_chunk=0, drop_term=0)
    rows2 = 0
    for m, t, n, k, _, _ in fx.D_CASES:
        if n > 136 and k > 2048:
            n = 136  # (the same rows against a smaller weight: the mutations are of the activation side or per K block)
        c, w = fx.norm_case(m, k, t), fx.fp8_weight(n, k)
        base = fx.fp8_exact(c, w)
        seen["scale_group"] += not torch.equal(fx.fp8_exact(c, w, mutate_a="scale_group"), base)
        seen["no_tier"] += not torch.equal(fx.fp8_exact(c, w, mutate_a="no_tier"), base)
        seen["w_scale_kb"] += not torch.equal(fx.fp8_exact(c, w, mutate_w="w_scale_kb"), base)
        if m > 1:
            rows2 += 1
            seen["scale_row"] += not torch.equal(fx.fp8_exact(c, w, mutate_a="scale_row"), base)
        cw = fx.norm_case(m, k, t, mutate="w_chunk")
        seen["w_chunk"] += not torch.equal(rx.bits(cw["y"]), rx.bits(c["y"])) and not torch.equal(fx.fp8_exact(cw, w, mutate_a="w_chunk"), base)
        seen["drop_term"] += not torch.equal(rx.bits(fx.norm_case(m, k, t, mutate="drop_term")["v"]), rx.bits(c["v"]))
    total = len(fx.D_CASES)
    print(f"FUSEDEXACT host mutations: {seen} of {total} cases ({rows2} with two rows)")
    assert seen == dict(scale_group=total, scale_row=rows2, w_scale_kb=total, no_tier=total, w_chunk=total, drop_term=total)


def test_reference_mutations_change_the_bf16_expectation():
    changed = 0
    for m, n, k, t, *_ in fx.A_CASES:
        c, w = fx.norm_case(m, k, t), fx.bf16_weight(min(n, 136), k)
        cw = fx.norm_case(m, k, t, mutate="w_chunk")
        changed += not torch.equal(fx.bf16_exact(cw, w), fx.bf16_exact(c, w))
        assert not torch.equal(rx.bits(fx.norm_case(m, k, t, mutate="drop_term")["v"]), rx.bits(c["v"]))
    print(f"FUSEDEXACT host mutations: next chunk's norm weight changes {changed} of {len(fx.A_CASES)} bf16 cases")
    assert changed == len(fx.A_CASES)


# ---------------------------------------------------------------- the instantiation mirrors
def test_every_listed_shape_takes_the_intended_instantiation():
    from chitu_amd import ops

    for m, t, n, k, _, form in fx.D_CASES:
        assert fx.fp8_norm_form(m, t, n, k) == form, (m, t, n, k)
        assert ops.fp8_linear_add_norm_fits(m, n, k, t)
    for m, t, n, k in fx.D_REFUSED:
        assert fx.fp8_norm_form(m, t, n, k) is None and not ops.fp8_linear_add_norm_fits(m, n, k, t), (m, t, n, k)
    for m, k, _ in fx.D_IDENT:
        assert fx.fp8_norm_form(m, 1, k, k) is not None
    assert {f for *_, f in fx.D_CASES} >= {(wk, mt, mr) for wk in (4, 8) for mt, mr in ((1, 1), (10, 1), (16, 1), (1, 2))}
    for m, n, k, t, deep, _, _, form in fx.A_CASES:
        assert fx.bf16_norm_form(m, n, k, deep) == form, (m, n, k, deep)
        assert ops.bf16_add_norm_fits(m, n, k) and dx.bf16_wk(n, k) == form[0]
    forms = {f for *_, f in fx.A_CASES}
    assert {(wk, d) for wk, d, _ in forms} == {(4, 4), (4, 8), (8, 4), (8, 8)} and {mr for *_, mr in forms} == {1, 2, 4}
    for m, inter, k, _, (wk, mr) in fx.B_CASES:
        f = fx.bf16_norm_form(m, inter, k)
        assert f is not None and (f[0], f[2]) == (wk, mr) and ops.bf16_add_norm_fits(m, inter, k)
    for m, k, _ in fx.A_IDENT:
        assert fx.bf16_norm_form(m, k, k) is not None
    for hq, hkv, d, k, m, page, _ in fx.C_CASES:
        f = fx.bf16_norm_form(m, (hq + 2 * hkv) * d, k)
        assert f == (8, 8, 1 if m == 1 else 2 if m == 2 else 4) and ops.bf16_add_norm_fits(m, (hq + 2 * hkv) * d, k) and d % 16 == 0
    assert {c[5] for c in fx.C_CASES} == {16, 48} and {c[6] for c in fx.C_CASES} == {"valid", "out-of-table-0", "out-of-table-1"}
    assert {c[4] for c in fx.F_CASES} == set(dx.ABSORB_STRIDES) and any(c[5] for c in fx.F_CASES)
    assert not ops.bf16_add_norm_fits(4, 136, 8192) and not ops.bf16_add_norm_fits(5, 136, 512)
    # mla_q_proj: waves with 0, 1 and 2 K blocks
    want = {128: {0, 1}, 384: {0, 1}, 896: {0, 1}, 1024: {1}, 1152: {1, 2}, 1536: {1, 2}, 2048: {2}}
    for r in fx.E_RANK:
        b = fx.qproj_blocks(r)
        assert sum(b) == r // 128 and set(b) == want[r], (r, b)
        assert ops.mla_q_proj_fits(1, r) and ops.mla_q_proj_fits(32, r)
    for b, r in fx.E_REFUSED:
        assert not ops.mla_q_proj_fits(b, r)
    assert {b for b, *_ in fx.E_CASES} == set(fx.E_BATCH) and {n for _, _, n, *_ in fx.E_CASES} == set(fx.E_N)


# ---------------------------------------------------------------- the merge workspace
def test_negligible_splits_underflow_whatever_the_device_exp():
    """e^-200 against the smallest fp32 subnormal 2^-149, in float64: 60 orders of magnitude, where the device exp is off
    by an ulp or two."""
    assert np.exp(-np.float64(fx.LSE_GAP)) < 2.0 ** -149 * 1e-40
    assert np.float32(np.exp(-np.float64(fx.LSE_GAP))) == 0.0
    # and the large rows of those splits stay finite in bf16, so 0 x row is 0 even unmasked
    mc = fx.merge_case(2, 5, 17)
    tiny = (mc["lse"] < -100) & torch.isfinite(mc["lse"])
    assert int(tiny.sum()) > 0 and bool(torch.isfinite(mc["part"][tiny].float()).all())
    assert float(mc["part"][tiny].float().abs().max()) > 2.0 ** 100


def test_merge_cases_and_their_mutations():
    """Every G case: the merged row is the softmax-weighted sum in float64 (weights exp(lse - max)), the live counts are powers
    of two, one (b, h) is dead.  Mutations: skipping the last live split changes the expectation on all cases, letting an empty
    split's NaN through on all cases that hold one."""
    skip = nan = with_empty = 0
    for b, h, s, st in fx.G_CASES:
        mc = fx.merge_case(b, h, s)
        lse, part = mc["lse"].double(), mc["part"].double()
        wgt = torch.where(torch.isinf(lse), torch.zeros_like(lse), (lse - lse.max(1, keepdim=True).values).exp())
        wgt = torch.where(torch.isnan(wgt), torch.zeros_like(wgt), wgt)
        assert bool(((wgt == 1) | (wgt < 1e-80)).all())
        wgt = torch.where(wgt < 1e-80, torch.zeros_like(wgt), wgt)  # (float64 does not underflow at e^-200: fp32 does, see above)
        num = (torch.where(wgt[:, :, None] > 0, part, torch.zeros_like(part)) * wgt[:, :, None]).sum(1)
        ref = torch.where(wgt.sum(1, keepdim=True) > 0, num / wgt.sum(1, keepdim=True).clamp(min=1), torch.zeros_like(num))
        assert torch.equal(ref.view(b, h, 512), mc["merged"]) and torch.equal(wgt.sum(1).long(), mc["live"])
        assert set(mc["live"].tolist()) <= {0, 1, 2, 4, 8, 16} and (b * h == 1 or int(mc["live"][mc["dead"]]) == 0)
        ac = dx.absorb_case(b, h, 128, 512, st)
        q, sc = fx.merge_expect(mc, ac)
        if mc["dead"] >= 0:  # the dead (b, h): zeros -> amax 0 -> scale 0 -> 0 / 0: NaN codes, as the kernel's v / sc path gives
            bb, hh = divmod(mc["dead"], h)
            assert float(sc[bb, hh]) == 0.0 and bool(torch.isnan(q[bb, hh * 128:(hh + 1) * 128].float()).all())
        q2, s2 = fx.merge_expect(fx.merge_case(b, h, s, mutate="skip_live"), ac)
        skip += not (torch.equal(rx.canon_nan(q2), rx.canon_nan(q)) and torch.equal(s2, sc))
        has_empty = bool(torch.isinf(mc["lse"]).any())
        with_empty += has_empty
        q3, s3 = fx.merge_expect(fx.merge_case(b, h, s, mutate="nan_through"), ac)
        nan += not (torch.equal(rx.canon_nan(q3), rx.canon_nan(q)) and torch.equal(rx.bits(s3), rx.bits(sc)))
    total = len(fx.G_CASES)
    print(f"FUSEDEXACT host mutations: a live split skipped changes {skip} of {total} merge cases, an empty split's NaN let through "
          f"{nan} of the {with_empty} with an empty split")
    assert skip == total and nan == with_empty and with_empty >= total - 2
    assert {s for *_, s, _ in fx.G_CASES} == set(fx.G_S)
