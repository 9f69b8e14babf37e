"""CPU checks of tests/row_exact.py: every oracle against torch on the CPU or a float64 evaluation, every builder's promises,
and for every oracle at least one deliberately wrong variant that the case data must tell apart."""

import numpy as np
import pytest
import torch

from oracle import kv as okv
from oracle import w8a8 as ow8
from tests import dense_exact as dx
from tests import row_exact as rx

BF16, F32 = torch.bfloat16, torch.float32
HOST_DIMS = [8, 128, 1000, 2048, 2056, 7168, 8192]


# ---------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("dim", HOST_DIMS)
def test_rms_oracle_is_torch_and_tells_wrong_norms_apart(dim):
    c = rx.rms_case(40, dim)
    v, w = c["v"], c["w"]
    assert set(c["e"].tolist()) == set(rx.ROW_EXPS)
    t, rr, y = rx.rms_oracle(v, w)
    # torch on the CPU (fp32 math on the bf16 row, one rounding) is the central candidate on every row
    ref = torch.nn.functional.rms_norm(v.float(), (dim,), w.float(), rx.EPS).to(BF16)
    assert torch.equal(rx.bits(ref), rx.bits(y[0]))
    # float64: within one bf16 ulp of the exact value
    y64 = v.double() * (1.0 / ((v.double() ** 2).mean(-1, keepdim=True) + rx.EPS).sqrt()) * w.double()
    assert bool(((y[0].double() - y64).abs() <= y64.abs() * 2.0 ** -7).all())
    # the candidates are distinct numbers but rarely distinct rows
    assert bool((rr[1] < rr[0]).all()) and bool((rr[0] < rr[2]).all())
    idx = rx.match_rows(y[0], t, rr, y, "central")
    assert bool((idx == 0).all())

    def caught(wrong):
        """the wrong row equals NO candidate on at least one row"""
        hit = (rx.bits(wrong)[None] == rx.bits(y)).all(-1).any(0)
        return not bool(hit.all())

    ss = (v.double() ** 2).sum(-1)
    wrong_w = rx.rms_rows(v, torch.roll(w, 1), rr[0])                                        # a neighbour's weight
    wrong_div = rx.rms_rows(v, w, rx.rr_candidates(rx.rms_t(v, dim=dim + 8))[0])             # divide by dim + 8
    assert caught(wrong_w) and caught(wrong_div)
    if dim > 8:
        wrong_div2 = rx.rms_rows(v, w, rx.rr_candidates(rx.rms_t(v, dim=dim - 8))[0])        # divide by dim - 8
        ss_short = (v[:, :-8].double() ** 2).sum(-1)                                          # the last chunk left out of the sum
        wrong_ss = rx.rms_rows(v, w, rx.rr_candidates(rx.rms_t(v, dim=dim, ss=ss_short))[0])
        assert caught(wrong_div2) and caught(wrong_ss)
        with pytest.raises(AssertionError, match="equals no candidate"):
            rx.match_rows(wrong_ss, t, rr, y, "short sum")
    assert bool((ss < 2.0 ** 24 * torch.ldexp(torch.ones(40), 2 * c["e"].int()).double()).all())


def test_rms_candidates_cost_little_sharpness():
    rows = differ = 0
    for dim in HOST_DIMS:
        c = rx.rms_case(40, dim)
        _, _, y = rx.rms_oracle(c["v"], c["w"])
        rows += 40
        differ += int(((rx.bits(y[1]) != rx.bits(y[0])).any(-1) | (rx.bits(y[2]) != rx.bits(y[0])).any(-1)).sum())
    assert rows == 280 and differ <= rows // 10, differ  # one ulp of fp32 is 2^-16 of a bf16 ulp: the rows rarely move


@pytest.mark.parametrize("terms", [1, 2, 9, 16])
def test_residual_and_terms_are_exact_and_a_dropped_term_shows(terms):
    for dim in rx.B_TERM_DIMS:
        c = rx.rms_case(3, dim, terms)
        s = rx.sum_terms_oracle(c["add"])
        assert torch.equal(s.double(), c["add"].double().sum(1)) and torch.equal(rx.bits(s), rx.bits(c["add_sum"]))
        v = rx.residual_oracle(c["x"], s)
        assert torch.equal(rx.bits(v), rx.bits(c["v"])) and torch.equal(v.double(), c["x"].double() + c["add"].double().sum(1))
        assert not torch.equal(rx.sum_terms_oracle(c["add"][:, :-1]) if terms > 1 else torch.zeros_like(s), s)  # `k < terms - 1`
        assert dim * float((c["v"].double() / torch.ldexp(torch.ones(3), c["e"].int())[:, None].double()).abs().max()) ** 2 < 2 ** 24


# ---------------------------------------------------------------- fp8 quantisers
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_quant_table_ties_specials_and_the_nan_rule(dt):
    x, kinds = rx.quant_table(dt)
    vals = rx.e4m3_values()
    for mode in (0, 1):
        q, s = rx.quant_fp8(x, mode)
        code = q.view(torch.uint8)
        for gi, kind in enumerate(kinds):
            row, crow = x[gi].double(), code[gi]
            if kind.startswith("tie"):
                k = {"tie+": 0, "tie-": 0, "tie+k3": 3, "tie-k-2": -2}[kind]
                assert float(s[gi]) == 2.0 ** k
                quo = (row / 2.0 ** k).abs()
                for j in range(128):
                    lo = int((vals.double() <= quo[j]).sum()) - 1
                    if lo < 126 and float(quo[j]) == float(vals[lo] + vals[lo + 1]) / 2:  # a midpoint: the even code wins
                        want = lo if lo % 2 == 0 else lo + 1
                        assert int(crow[j]) & 0x7F == want, (kind, j)
                        away = lo + 1                                                   # round-half-away is told apart
                        if away != want:
                            assert int(crow[j]) & 0x7F != away
            elif kind == "zero":
                if mode == 0:
                    assert float(s[gi]) == 0.0 and bool(((crow & 0x7F) == 0x7F).all())
                else:
                    assert float(s[gi]) == float(np.float32(1e-10) / np.float32(448.0)) and bool((crow == 0).all())
            elif kind == "above":
                quo = x[gi].float() / s[gi]
                assert float(quo.max()) > 448.0 and int(crow[17]) == 0x7E and int(crow[90]) == 0xFE
            elif kind == "nan":
                assert torch.isfinite(s[gi]) and float(s[gi]) > 0
                assert int(crow[33]) == (0xFE if mode == 1 else int(crow[33]) | 0x7F)  # mode 1: -448; mode 0: a NaN code
                assert int(((crow & 0x7F) == 0x7F).sum()) == (0 if mode == 1 else 1)
            elif kind.startswith("inf"):
                assert torch.isinf(s[gi])
                assert int(crow[70]) == 0xFE if mode == 1 else int(crow[70]) & 0x7F == 0x7F  # inf / inf = NaN -> -448 under the clamp
                others = torch.cat([crow[:70], crow[71:]])
                assert bool(((others & 0x7F) == 0).all())
        # torch.clamp (the oracle before this rule was written down) keeps the NaN: told apart by the table
        xf = x.float()
        if mode == 1:
            naive = torch.clamp(xf / s[:, None], -448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
            assert not torch.equal(rx.canon_nan(naive), rx.canon_nan(code))
        # the neighbouring group's scale is told apart
        wrong = (xf / torch.roll(s, 1)[:, None])
        wrong = (torch.clamp(wrong, -448, 448) if mode == 1 else wrong).to(torch.float8_e4m3fn).view(torch.uint8)
        assert not torch.equal(rx.canon_nan(wrong), rx.canon_nan(code))
        # the finite normal groups: the code is a nearest e4m3 value of the fp32 quotient fl(x / s) (the reference divides
        # in fp32; the float64 quotient can sit on the other side of a midpoint that the fp32 one hits exactly)
        for gi, kind in enumerate(kinds):
            if kind == "normal":
                quo = (x[gi].float() / s[gi]).double()
                got = q[gi].float().double()
                allv = torch.cat([-vals.flip(0), vals]).double()
                near = (quo[:, None] - allv[None]).abs().min(1).values
                assert bool(((got - quo).abs() <= near + 1e-12).all())


def test_midpoints_are_exact_in_every_input_type():
    m = rx.e4m3_midpoints()
    assert len(m) == 126
    for dt in (torch.bfloat16, torch.float16):
        for k in (-2, 0, 3):
            assert torch.equal((m * 2.0 ** k).to(dt).double(), m * 2.0 ** k)


def test_quant_big_drives_a_second_stride_iteration():
    x = rx.quant_big("bf16")
    assert x.shape == (4104, 1024) and x.numel() // 128 > 2048 * 16
    assert x.numel() * 4 <= 40 << 20


# ---------------------------------------------------------------- int8 quantiser
@pytest.mark.parametrize("K", rx.E_VEC_K + rx.E_SCALAR_K)
def test_int8_oracle_is_the_reference_on_finite_rows_and_rounds_half_even(K):
    for dt in ("bf16", "f16", "f32"):
        for k in (0, -3, 4):
            row = rx.int8_row(K, dt, k, special=False)[None]
            q, s = rx.quant_int8(row)
            q_ref, s_ref = ow8.quant_act(row.float())
            assert torch.equal(q, q_ref) and torch.equal(s, s_ref)
            if K >= 2:
                assert float(s) == 2.0 ** k
                quo = row.double() / 2.0 ** k
                ties = (quo * 2) % 2 == 1
                if K >= 7:
                    assert bool(ties.any())
                assert bool((q.double()[ties] % 2 == 0).all())                     # half-even ...
                away = torch.sign(quo) * torch.floor(quo.abs() + 0.5)
                if bool(ties.any()):
                    assert not torch.equal(away, q.double())                       # ... and half-away is told apart
    zero = torch.zeros(1, K)
    q, s = rx.quant_int8(zero)
    assert float(s) == float(np.float32(1e-5) / np.float32(127.0)) and bool((q == 0).all())
    if K >= 7:
        q, s = rx.quant_int8(rx.int8_row(K, "bf16")[None])
        assert int(q[0, K // 2]) == -128 and float(s) == 1.0


# ---------------------------------------------------------------- RoPE
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("layout", [0, 1])
def test_rope_oracle_is_the_kv_oracle_and_close_to_float64(dt, layout):
    for d in (2, 128):
        x, cos, sin = rx.rope_inputs(5, 3, d, rx.DTYPES[dt], seed=d + layout)
        got = rx.rope_oracle(x, cos, sin, layout)
        ref, _ = okv.apply_rotary_pos_emb(x, x, cos, sin, "llama" if layout == 0 else "hf-llama")
        assert torch.equal(rx.bits(got), rx.bits(ref))
        xd, c, s = x.double(), cos.double()[:, None], sin.double()[:, None]
        x0, x1 = (xd[..., 0::2], xd[..., 1::2]) if layout == 0 else (xd[..., : d // 2], xd[..., d // 2:])
        g0, g1 = (got[..., 0::2], got[..., 1::2]) if layout == 0 else (got[..., : d // 2], got[..., d // 2:])
        ulp = {"f32": 2.0 ** -22, "bf16": 2.0 ** -7, "f16": 2.0 ** -10}[dt]
        bound = (x0.abs() + x1.abs()) * ulp
        assert bool(((g0.double() - (x0 * c - x1 * s)).abs() <= bound).all()) and bool(((g1.double() - (x1 * c + x0 * s)).abs() <= bound).all())
        if d > 2:
            assert not torch.equal(got, rx.rope_oracle(x, cos, sin, 1 - layout))      # the other layout (`2 i` for `i`)
            assert not torch.equal(got, rx.rope_oracle(x, torch.roll(cos, 1, 0), sin, layout))  # a neighbour's row


# ---------------------------------------------------------------- appends
def _unguarded_row(b, lens, table, page, per):
    """Where a kernel WITHOUT the guard would write (C arithmetic: / and % truncate towards zero)."""
    L = int(lens[b])
    pidx = int(L / page) if L >= 0 else -int(-L / page)
    rem = L - pidx * page
    flat = table.reshape(-1)
    return int(flat[b * per + pidx]) * page + rem


@pytest.mark.parametrize("B,seed", [(8, 0), (8, 3), (4, 0), (4, 1)])
@pytest.mark.parametrize("page", [4, 64])
def test_paged_batches_drop_the_bad_sequences_and_keep_a_broken_guard_inside_the_allocation(B, seed, page):
    lens, table, num_pages, alloc, kinds = rx.paged_batch(B, page, seed, bad=True)
    per = table.shape[1]
    assert table.shape[0] == B + 1 and alloc == num_pages + dx.G
    want = {8: {"neg", "beyond", "page=num_pages", "page=-1"}, 4: {"neg", "page=num_pages"} if seed % 2 == 0 else {"beyond", "page=-1"}}[B]
    assert set(kinds.values()) == want
    live = [rx.live_row(b, lens, table, page, per, num_pages) for b in range(B)]
    assert all((live[b] is None) == (b in kinds) for b in range(B))
    rows = [r for r in live if r is not None]
    assert len(set(rows)) == len(rows) and len(rows) == B - len(kinds)
    for b in kinds:  # the write of a guard-less kernel stays between the guard pages of the test's own allocation
        r = _unguarded_row(b, lens, table, page, per)
        assert -dx.G * page <= r < (num_pages + dx.G) * page, (b, kinds[b], r)
    good = rx.paged_batch(B, page, seed, bad=False)
    assert all(rx.live_row(b, good[0], good[1], page, per, num_pages) is not None for b in range(B))
    cache = torch.zeros(num_pages * page, 3)
    new = torch.arange(1, B + 1).float()[:, None].expand(B, 3)
    out = rx.append_oracle(cache, new, lens, table, page, num_pages)
    assert int((out != 0).any(-1).sum()) == B - len(kinds)
    # the sequence with a page id == num_pages is the one a kernel that lost `page < num_pages` would write: into the guard
    # pages after the cache, so a broken guard shows as a changed guard page
    over = [b for b, k in kinds.items() if k == "page=num_pages"]
    for b in over:
        assert num_pages * page <= _unguarded_row(b, lens, table, page, per) < (num_pages + dx.G) * page


# ---------------------------------------------------------------- gather, moe_sum, dequant
def test_gather_oracle_clamps_positions_and_zeroes_foreign_tokens():
    table = torch.arange(40).float().view(5, 8).to(BF16)
    cos_t, sin_t = torch.arange(12.0).view(4, 3), -torch.arange(12.0).view(4, 3)
    tokens = torch.tensor([9, 10, 14, 15, 12])
    h, c, s = rx.embed_gather_oracle(tokens, table, 10, torch.tensor([-1, 0, 3, 4, 2], dtype=torch.int32), cos_t, sin_t)
    assert bool((h[0] == 0).all()) and bool((h[3] == 0).all()) and torch.equal(h[1], table[0]) and torch.equal(h[2], table[4])
    assert torch.equal(c[0], cos_t[0]) and torch.equal(c[3], cos_t[3]) and torch.equal(s[4], sin_t[2])


@pytest.mark.parametrize("topk", rx.J_TOPK)
def test_moe_sum_oracle_is_the_float64_sum_on_integers(topk):
    g = torch.Generator().manual_seed(topk)
    c3 = (dx.ints(g, 7, 5, topk, 24).float() * 0.25).to(BF16)
    got = rx.moe_sum_oracle(c3)
    assert torch.equal(got.double(), c3.double().sum(1))
    if topk > 1:
        assert not torch.equal(got, rx.moe_sum_oracle(c3[:, :-1]))


def test_dequant_oracle_covers_every_code_and_overflows_f16():
    codes = torch.arange(256, dtype=torch.uint8).view(1, 256).repeat(2, 1)
    s = torch.tensor([[0.5, 4096.0]])
    for dt in (torch.float16, torch.float32):
        y = rx.dequant_oracle(codes, s, dt)
        want = codes.view(torch.float8_e4m3fn).double() * torch.tensor([0.5, 4096.0]).double().repeat_interleave(128)[None]
        fin = torch.isfinite(want)
        assert torch.equal(torch.isnan(y), torch.isnan(want))
        if dt == torch.float32:
            assert torch.equal(y.double()[fin], want[fin])
        else:
            assert bool(torch.isinf(y[0, 128 + 0x7E - 128 + 128 - 128:]).any())  # 448 * 4096 overflows f16
            small = fin & (want.abs() < 65504)
            assert torch.equal(y.double()[small], want[small].to(torch.float16).double())


def test_tile_major_is_the_dense_tests_layout_with_sentinel_padding():
    g = torch.Generator().manual_seed(1)
    for M in rx.B_TILE_ROWS:
        q = torch.randint(0, 0x7E, (M, 256), generator=g, dtype=torch.uint8)
        s = torch.rand(M, 2, generator=g)
        qt, st = rx.to_tile_major(q, s)
        qd, sd = dx.to_tile_major(q.view(torch.float8_e4m3fn), s)
        live = torch.zeros((M + 15) // 16 * 16, dtype=torch.bool)
        live[:M] = True
        lt = live.view(-1, 16)
        assert torch.equal(qt.view(-1, 16, 16, 16)[lt[:, None, :].expand(-1, 16, -1)], qd.view(torch.uint8).view(-1, 16, 16, 16)[lt[:, None, :].expand(-1, 16, -1)])
        assert torch.equal(st[lt[:, None, :].expand(-1, 2, -1)], rx.bits(sd)[lt[:, None, :].expand(-1, 2, -1)])
        assert bool((st[~lt[:, None, :].expand(-1, 2, -1)] == dx.SENTINEL32).all())
        assert bool((qt.view(-1, 16, 16, 16)[~lt[:, None, :].expand(-1, 16, -1)] == rx.CODE_SENTINEL).all())


# ---------------------------------------------------------------- SiLU
def test_silu_fp32_formula_is_torch_on_every_finite_gate_and_float64_alone_is_not():
    gate, up, x = rx.silu_case()
    assert x.shape == (65536, 272) and 65536 * (136 // 8) > 1048576 and x.numel() * 2 <= 40 << 20
    assert len(set(rx.bits(gate).tolist())) == 65536
    g = gate.float()
    fin = torch.isfinite(g)
    cands = rx.expf_candidates(g)
    central = rx.silu_factor(g, cands[0])
    ref = torch.nn.functional.silu(gate)
    assert int(fin.sum()) == 65280 and torch.equal(rx.bits(central[fin]), rx.bits(ref[fin]))
    f64 = (gate.double() / (1 + (-gate.double()).exp())).to(BF16)
    n64 = int((rx.bits(f64[fin]) != rx.bits(central[fin])).sum())
    assert 0 < n64 < 100, n64  # a float64-only reference would be wrong on these gates
    moved = sum(int((rx.canon_nan(rx.silu_factor(g, c)) != rx.canon_nan(central)).sum()) for c in cands[1:])
    assert moved < 65536 // 50, moved  # the candidates cost little sharpness


def test_silu_rows_pin_the_factor_and_wrong_products_are_caught():
    gate, up, _ = rx.silu_case()
    sel = torch.arange(0, 65536, 37)
    want = rx.silu_oracle(gate[sel], up[sel])
    idx = rx.silu_match(want[0], want, "central")
    assert bool((idx == 0).all())
    # the product rounded twice (through an fp32 silu that was never rounded to bf16) is told apart
    g = gate[sel].float()
    unrounded = ((g / (1 + rx.expf_candidates(g)[0]))[:, None] * up[sel].float()).to(BF16)
    with pytest.raises(AssertionError, match="equal no candidate"):
        rx.silu_match(unrounded, want, "factor never rounded to bf16")
    # the up values reach +-0, subnormals and the largest finite value in every row
    u = up[0].float()
    assert float(u[0]) == 0 and float(u[4]) > 3e38 and 0 < float(u[2]) < 2.0 ** -126


# ---------------------------------------------------------------- the guarded buffer itself
def test_guarded_buffer_reports_guard_writes_and_unwritten_elements():
    gb = rx.Guarded(3, 16, BF16, stride=24, device="cpu")
    with pytest.raises(AssertionError, match="never written"):
        gb.check("nothing written")
    gb.view.copy_(rx.bits(torch.ones(3, 16, dtype=BF16)))
    assert torch.equal(gb.check("ok"), torch.ones(3, 16, dtype=BF16))
    gb.full[dx.G + 1, 17] = 0
    with pytest.raises(AssertionError, match=r"stored outside the output.*\(1, 17\)"):
        gb.check("guard column")
    gb = rx.Guarded(2, 8, F32, device="cpu")
    gb.full[dx.G + 2, 0] = 0
    with pytest.raises(AssertionError, match=r"stored outside"):
        gb.check("row after")
