"""The tiled grouped GEMMs of bf16 experts (csrc/moe_bf16_tiled.hip, include/chitu_hip_ext3.h) and the tiled branch of
fused_experts on bf16 weights.

1. chitu_ext3_moe_gemm2_bf16_tiled on exact integer data: torch.equal against the integer matmul times the routed weight, the
   output between guard rows that must keep their sentinel bits.  I in {128, 384} (two and six 64-element K blocks: the ring's
   prologue is the whole loop / the ring wraps) x N in {128, 136, 640} (one tile; a clamped partial tile; five tiles, which
   the launcher walks four to a workgroup with a ragged last group of one).
2. chitu_ext3_moe_gemm1_silu_bf16_tiled, K in {128, 384} x I in {128, 384} (2 and 6 column tiles: fewer than / no multiple of
   the 8-XCD run), on two data sets: (a) positive activations and positive gate weights, so that every gate is >= 128, where
   fp32 SiLU is the identity whatever the device's expf (1 + e^-g rounds to 1 from g = 17.4 on): torch.equal against
   bf16(bf16(g) * bf16(u)) of the integer sums; (b) the data of tests/test_gpu_moe_routing.py's SiLU test (signed, gates of
   magnitude <= 48), held to that test's bar of 2^-7 per element.
   Both entries: block_m in {64, 128}, every tiled routing pattern of tests/test_gpu_moe_routing.py, the hottest expert on
   another rank (expert_map -1: zeros), routed weights as bf16 and as fp32.
3. fused_experts on bf16 weights with the tiled floor at 1, on every tiled pattern: poisoned allocations == unpoisoned; on
   integer data built so that h and the second GEMM stay exact, tiled == streaming == the CPU's integer arithmetic bit for
   bit; on random data against oracle.moe.fused_experts_bf16, whole tensor and row by row, at the bf16 family's bars.
4. The router at Qwen3-MoE's shapes (128 experts top 8, 16 experts top 4; renormalised softmax and plain softmax), separate
   and fused with moe_align, exact against tests/route_exact.py's CPU oracle.
"""

import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import moe as omoe
from tests import route_exact as rx
from tests.test_gpu_moe_routing import (E, G, PATTERN_NAMES, ROW_BAR, SENTINEL, TILED_PATTERNS, _exact, _ints, _pow2, hottest, n_blocks,
                                        pattern_ids, route)
from tests.util import assert_close, assert_close_elementwise, max_rel_to_peak, poisoned_allocations

pytestmark = pytest.mark.gpu

NAMES = PATTERN_NAMES["tiled"]
assert set(NAMES) == set(TILED_PATTERNS) | {"dups"}
for _name, (_M, _topk, _counts, _blocks) in TILED_PATTERNS.items():  # block counts at both tile heights, asserted by route()
    assert torch.equal(route(_counts, _M, _topk, _blocks), pattern_ids("tiled", _name)) and set(_blocks) == {64, 128}
ROUTED = torch.tensor([0.5, 2.0, 1.0, 4.0])


def _align(ids, block_m, remote):
    from chitu_amd import fused_moe

    emap = None
    if remote is not None:
        emap = torch.arange(E, dtype=torch.int32)
        emap[remote] = -1
        emap = emap.cuda()
    sorted_ids, expert_ids, npost = fused_moe.moe_align_block_size(ids.cuda(), block_m, E, emap)
    assert int(npost) == n_blocks(torch.bincount(ids.reshape(-1), minlength=E).tolist(), block_m) * block_m
    return sorted_ids, expert_ids, npost


def _guarded(numel, n_out):
    return torch.full((numel + 2 * G, n_out), SENTINEL, dtype=torch.int16, device="cuda")


def _read(full, numel, what):
    torch.cuda.synchronize()
    got = full.cpu()
    for side, rows in (("before", got[:G]), ("after", got[G + numel:])):
        touched = (rows != SENTINEL).nonzero()
        assert len(touched) == 0, f"{what}: stored into the guard rows {side} the output, first (row, col): {touched[:8].tolist()}"
    return got[G:G + numel].view(torch.bfloat16)


def launch_gemm1(a, w1, ids, I, K, block_m, remote=None):
    from chitu_amd import _lib
    from chitu_amd._lib import check, i32, i64, ptr, stream_ptr

    numel = ids.numel()
    sorted_ids, expert_ids, npost = _align(ids, block_m, remote)
    full = _guarded(numel, I)
    check(_lib.lib().chitu_ext3_moe_gemm1_silu_bf16_tiled(ptr(a), ptr(w1), ptr(sorted_ids), ptr(expert_ids), ptr(npost), ptr(full[G:]),
                                                          i64(numel), i32(ids.shape[1]), i64(I), i64(K),
                                                          i64(min(expert_ids.numel(), numel)), i32(block_m), stream_ptr()), "gemm1 tiled")
    return _read(full, numel, f"gemm1 bf16 tiled block_m={block_m}")


def launch_gemm2(h, w2, ids, wts, N, I, block_m, remote=None):
    from chitu_amd import _lib
    from chitu_amd._lib import check, float_dtype_code, i32, i64, ptr, stream_ptr

    numel = ids.numel()
    sorted_ids, expert_ids, npost = _align(ids, block_m, remote)
    full = _guarded(numel, N)
    check(_lib.lib().chitu_ext3_moe_gemm2_bf16_tiled(ptr(h), ptr(w2), ptr(sorted_ids), ptr(expert_ids), ptr(npost), ptr(wts),
                                                     i32(float_dtype_code(wts.dtype)), i32(1), ptr(full[G:]), i64(numel), i64(N), i64(I),
                                                     i64(min(expert_ids.numel(), numel)), i32(block_m), stream_ptr()), "gemm2 tiled")
    return _read(full, numel, f"gemm2 bf16 tiled block_m={block_m}")


def _bf16_ints(g, lo, hi, *shape):
    """Integers in -4..4 times a power of two 2^lo..2^hi per row, exact in bf16; (bf16 tensor, float64 values)."""
    t = _ints(g, *shape).float() * _pow2(g, lo, hi, *shape[:-1], 1)
    return t.to(torch.bfloat16), t.double()


def _assert_bits(got, expect, what):
    bad = (got.float() != expect.float()).nonzero()  # (+0 and -0 are the same result)
    assert len(bad) == 0, (f"{what}: {len(bad)} elements differ from the exact result, first (slot, n, got, want): "
                           f"{[(int(s), int(n), float(got[s, n]), float(expect[s, n])) for s, n in bad[:6]]}")


# ---------------------------------------------------------------- 1. GEMM2
@pytest.mark.parametrize("block_m", [64, 128])
@pytest.mark.parametrize("I,N", [(i, n) for i in (128, 384) for n in (128, 136, 640)])
def test_gemm2_entry_is_exact_on_integer_data_and_keeps_its_guard_rows(I, N, block_m):
    """h and W2 are integers in -4..4 times powers of two 2^-2..2^2 per row, routed weights from {0.5, 1, 2, 4}: every partial
    sum is a multiple of 2^-4 below 2^20, so the fp32 accumulator holds THE matmul whatever the order, and the output is that
    value times the routed weight rounded once to bf16."""
    g = torch.Generator().manual_seed(I + N)
    w2, w2d = _bf16_ints(g, -2, 2, E, N, I)
    w2 = w2.cuda()
    worst = 0
    for name in NAMES:
        ids = pattern_ids("tiled", name)
        M, topk = ids.shape
        numel = M * topk
        h, hd = _bf16_ints(g, -2, 2, numel, I)
        wts = ROUTED.repeat(numel)[:numel].view(M, topk)
        exact = _exact(hd, w2d, ids.reshape(-1), 1, -2, -2)
        want = (exact.float() * wts.float().view(-1, 1)).to(torch.bfloat16)
        assert float(exact.abs().max()) * 4 < 2 ** 24
        for remote in (None, hottest(ids)):
            expect = want.clone()
            if remote is not None:
                expect[ids.reshape(-1) == remote] = 0
            for dt in (torch.bfloat16, torch.float32):
                got = launch_gemm2(h.cuda(), w2, ids, wts.to(dt).cuda(), N, I, block_m, remote)
                _assert_bits(got, expect, f"gemm2 I={I} N={N} block_m={block_m} {name} remote={remote} {dt}")
                worst += 1
    print(f"BF16-TILED gemm2 I={I} N={N} block_m={block_m}: {worst} launches over {len(NAMES)} patterns exact, guard rows intact")


# ---------------------------------------------------------------- 2. GEMM1 + SiLU
@pytest.mark.parametrize("block_m", [64, 128])
@pytest.mark.parametrize("K,I", [(k, i) for k in (128, 384) for i in (128, 384)])
def test_gemm1_silu_entry_is_exact_where_silu_is_the_identity(K, I, block_m):
    """Activations in {1, 2}, gate weights in {1, 2}, up weights integers in -4..4: every gate is an integer in [K, 4K], where
    fp32 SiLU returns its argument (e^-g underflows against 1), every up an integer of magnitude <= 8K.  The entry's output is
    then bf16(bf16(g) * bf16(u)) with nothing left to the device's expf: torch.equal."""
    g = torch.Generator().manual_seed(K + I)
    gate = torch.randint(1, 3, (E, I, K), generator=g).float()
    up = _ints(g, E, I, K).float()
    w1 = torch.cat([gate, up], dim=1)
    w1_dev = w1.to(torch.bfloat16).cuda()
    n = 0
    for name in NAMES:
        ids = pattern_ids("tiled", name)
        M, topk = ids.shape
        x = torch.randint(1, 3, (M, K), generator=g).float()
        exact = _exact(x.double(), w1.double(), ids.reshape(-1), topk, 0, 0)
        gv, uv = exact[:, :I].float().to(torch.bfloat16).float(), exact[:, I:].float().to(torch.bfloat16).float()
        assert float(gv.min()) >= 128
        silu = torch.nn.functional.silu(gv)
        assert torch.equal(silu, gv)  # the CPU agrees that SiLU is the identity here
        want = (silu.to(torch.bfloat16).float() * uv).to(torch.bfloat16)
        for remote in (None, hottest(ids)):
            expect = want.clone()
            if remote is not None:
                expect[ids.reshape(-1) == remote] = 0
            got = launch_gemm1(x.to(torch.bfloat16).cuda(), w1_dev, ids, I, K, block_m, remote)
            _assert_bits(got, expect, f"gemm1 K={K} I={I} block_m={block_m} {name} remote={remote}")
            n += 1
    print(f"BF16-TILED gemm1+silu K={K} I={I} block_m={block_m}: {n} launches over {len(NAMES)} patterns exact, guard rows intact")


@pytest.mark.parametrize("block_m", [64, 128])
@pytest.mark.parametrize("K,I", [(k, i) for k in (128, 384) for i in (128, 384)])
def test_gemm1_silu_entry_on_signed_integer_data_within_two_bf16_ulps(K, I, block_m):
    """tests/test_gpu_moe_routing.py's SiLU data and bar: integers in -4..4 with scales 2^-4..2^-2 on both sides, gate and up
    exact multiples of 2^-8 of magnitude <= 48; reference h = bf16(bf16(silu(bf16(g))) * bf16(u)) in fp32 on the CPU; bar
    |h - ref| <= 2^-7 |ref| per element (SiLU's value may fall on the other side of a bf16 rounding boundary, that ulp is
    carried through the product, the final rounding adds one more).  The streaming entry on the same data is printed beside it."""
    from chitu_amd import _lib, fused_moe
    from chitu_amd._lib import check, i32, i64, ptr, stream_ptr

    g = torch.Generator().manual_seed(K + I + 1)
    w1, w1d = _bf16_ints(g, -4, -2, E, 2 * I, K)
    w1 = w1.cuda()
    for name in NAMES:
        ids = pattern_ids("tiled", name)
        M, topk = ids.shape
        numel = M * topk
        x, xd = _bf16_ints(g, -4, -2, M, K)
        exact = _exact(xd, w1d, ids.reshape(-1), topk, -4, -4)
        assert float(exact.abs().max()) <= 48.0
        gv, uv = exact[:, :I].float().to(torch.bfloat16).float(), exact[:, I:].float().to(torch.bfloat16).float()
        want = (torch.nn.functional.silu(gv).to(torch.bfloat16).float() * uv).to(torch.bfloat16)
        # the streaming entry (moe_align block 16) on the same problem
        s_sorted, s_experts, s_npost = fused_moe.moe_align_block_size(ids.cuda(), 16, E)
        streamed = torch.empty(numel, I, dtype=torch.bfloat16, device="cuda")
        check(_lib.lib().chitu_hip_moe_gemm_bf16(ptr(x.cuda()), i32(topk), ptr(w1), ptr(None), i32(0), ptr(s_sorted), ptr(s_experts),
                                                 ptr(s_npost), ptr(None), i32(0), i32(0), i32(1), ptr(streamed), i64(numel), i64(I), i64(K),
                                                 i64(min(s_experts.numel(), numel)), stream_ptr()), "streaming gemm1")
        for remote in (None, hottest(ids)):
            expect = want.clone()
            if remote is not None:
                expect[ids.reshape(-1) == remote] = 0
            got = launch_gemm1(x.cuda(), w1, ids, I, K, block_m, remote)
            assert torch.isfinite(got.float()).all()
            err, bar = (got.float() - expect.float()).abs(), 2.0 ** -7 * expect.float().abs()
            i = int((err - bar).argmax())
            s, n = divmod(i, I)
            vs_stream = int((got.float() != streamed.cpu().float()).sum()) if remote is None else -1
            print(f"BF16-TILED gemm1+silu signed K={K} I={I} block_m={block_m} {name} remote={remote}: {int((err != 0).sum())} of "
                  f"{err.numel()} differ from the CPU; worst slot {s} col {n} got {float(got[s, n])} want {float(expect[s, n])} = "
                  f"{float(err.flatten()[i] / bar.flatten()[i].clamp_min(1e-45)):.3f} of the bar; differ from the streaming entry: {vs_stream}")
            assert bool((err <= bar).all()), f"{int((err > bar).sum())} elements beyond 2^-7 of the reference"


# ---------------------------------------------------------------- 3. fused_experts
K4, I4 = 256, 128


@contextlib.contextmanager
def _block(monkeypatch, block_m):
    from chitu_amd import fused_moe

    with monkeypatch.context() as m:
        m.setattr(fused_moe, "_MOE_TILED_BLOCK_M", block_m)
        yield


def run_experts(monkeypatch, x, w1, w2, ids, wts, floor, block_m=128, remote=None, poisoned=False, reduce_topk=False):
    """fused_experts on bf16 weights; floor 1: the tiled form, 0: the streaming one -- checked against the C-ABI call log."""
    from chitu_amd import _lib, fused_moe

    kw = {}
    if remote is not None:
        emap = torch.arange(E, dtype=torch.int32)
        emap[remote] = -1
        kw.update(expert_map=emap.cuda(), global_num_experts=E)
    with _block(monkeypatch, block_m), (poisoned_allocations() if poisoned else contextlib.nullcontext()):
        _lib.call_log = []
        try:
            out = fused_moe.fused_experts(x.cuda(), w1, w2, wts.cuda(), ids.cuda(), reduce_topk=reduce_topk,
                                          bf16_tiled_min_tokens=floor, **kw).cpu()
            called = {n for n, _ in _lib.call_log if "gemm" in n}
        finally:
            _lib.call_log = None
    want = {"chitu_ext3_moe_gemm1_silu_bf16_tiled", "chitu_ext3_moe_gemm2_bf16_tiled"} if floor else {"chitu_hip_moe_gemm_bf16"}
    assert called == want, (floor, sorted(called))
    return out if reduce_topk else out.view(-1, x.shape[1])


@functools.lru_cache(maxsize=None)
def integer_case(name):
    """Data on which both GEMMs of both forms are exact: two non-zeros in {1, 2} per token, gate weights in {32, 64}, up and
    down weights integers in -4..4.  g = 32 (a + b) lies in [64, 256] where fp32 SiLU is the identity, |u| <= 16, so
    h = g u = 32 p with |p| <= 128 is a bf16 value, and the second GEMM sums multiples of 32 below 2^23."""
    ids = pattern_ids("tiled", name)
    M, topk = ids.shape
    g = torch.Generator().manual_seed(len(name) + M)
    x = torch.zeros(M, K4)
    cols = torch.stack([torch.randperm(K4, generator=g)[:2] for _ in range(M)])
    x.scatter_(1, cols, torch.randint(1, 3, (M, 2), generator=g).float())
    gate = 32.0 * torch.randint(1, 3, (E, I4, K4), generator=g).float()
    w1 = torch.cat([gate, _ints(g, E, I4, K4).float()], dim=1)
    w2 = _ints(g, E, K4, I4).float()
    wts = ROUTED.repeat(M * topk)[:M * topk].view(M, topk).to(torch.bfloat16)
    gu = _exact(x.double(), w1.double(), ids.reshape(-1), topk, 0, 0).float()
    gv, uv = gu[:, :I4], gu[:, I4:]
    assert float(gv.min()) >= 64 and torch.equal(torch.nn.functional.silu(gv), gv)
    h = (gv.to(torch.bfloat16).float() * uv.to(torch.bfloat16).float())
    assert torch.equal(h.to(torch.bfloat16).float(), h) and torch.equal(gv.to(torch.bfloat16).float(), gv)
    out = _exact(h.double(), w2.double(), ids.reshape(-1), 1, 5, 0)
    want = (out.float() * wts.float().view(-1, 1)).to(torch.bfloat16)
    return ids, x.to(torch.bfloat16), w1.to(torch.bfloat16), w2.to(torch.bfloat16), wts, want


@pytest.mark.parametrize("name", NAMES)
def test_fused_experts_tiled_is_the_streaming_form_bit_for_bit_on_integer_data(name, monkeypatch):
    ids, x, w1, w2, wts, want = integer_case(name)
    w1, w2 = w1.cuda(), w2.cuda()
    M, topk = ids.shape
    streamed = run_experts(monkeypatch, x, w1, w2, ids, wts, floor=0)
    _assert_bits(streamed, want, f"streaming {name}")
    for block_m in (128, 64):
        tiled = run_experts(monkeypatch, x, w1, w2, ids, wts, floor=1, block_m=block_m)
        _assert_bits(tiled, want, f"tiled {block_m} {name}")
        assert torch.equal(tiled, streamed), f"{name}: tiled (block_m {block_m}) != streaming"
        foul = run_experts(monkeypatch, x, w1, w2, ids, wts, floor=1, block_m=block_m, poisoned=True)
        assert torch.isfinite(foul.float()).all() and torch.equal(foul, tiled), f"{name}: poisoned != unpoisoned"
        summed = run_experts(monkeypatch, x, w1, w2, ids, wts, floor=1, block_m=block_m, reduce_topk=True)
        assert torch.equal(summed, tiled.view(M, topk, K4).float().sum(1).to(torch.bfloat16)), f"{name}: top-k sum"
        hot = hottest(ids)
        gone = ids.reshape(-1) == hot
        mapped = run_experts(monkeypatch, x, w1, w2, ids, wts, floor=1, block_m=block_m, remote=hot)
        assert bool((mapped[gone].float() == 0).all()) and torch.equal(mapped[~gone], tiled[~gone]), f"{name}: remote expert"
    print(f"BF16-TILED fused_experts integer data {name}: tiled 64 / 128 == streaming == CPU integer arithmetic, {ids.numel()} slots")


@functools.lru_cache(maxsize=None)
def random_case(name):
    """tests/test_gpu_moe.py::test_bf16_experts_vs_oracle's recipe on the pattern; the oracle per slot (top-1 on the flattened
    problem, routed weight folded in), computed once."""
    ids = pattern_ids("tiled", name)
    M, topk = ids.shape
    g = torch.Generator().manual_seed(M * 1000 + E + 5 + len(name))
    x = (torch.randn(M, K4, generator=g) * 0.5).to(torch.bfloat16)
    w1 = (torch.randn(E, 2 * I4, K4, generator=g) * K4 ** -0.5).to(torch.bfloat16)
    w2 = (torch.randn(E, K4, I4, generator=g) * I4 ** -0.5).to(torch.bfloat16)
    wts = (torch.rand(M, topk, generator=g) * 0.9 + 0.1).to(torch.bfloat16)
    per_slot = omoe.fused_experts_bf16(x.repeat_interleave(topk, 0), w1, w2, wts.reshape(-1, 1), ids.reshape(-1, 1))
    summed = omoe.fused_experts_bf16(x, w1, w2, wts, ids)
    return ids, x, w1, w2, wts, per_slot, summed


@pytest.mark.parametrize("name", NAMES)
def test_fused_experts_tiled_on_random_data_against_the_oracle(name, monkeypatch):
    """Bars: tests/test_gpu_moe.py::test_bf16_experts_vs_oracle's (assert_close at REL_TOL = 1e-2 of the peak plus
    assert_close_elementwise) on the summed and on the per-slot output, and the same 1e-2 ROW BY ROW: max |row - ref row| <
    1e-2 max |ref row| (a slot computed from the wrong token or expert is off by about its whole size).  A per-row bar cannot
    sit below 2^-7 = 7.8e-3: kernel and oracle sum in fp32 in different orders, so the final bf16 rounding of a row's peak
    element may fall on the other side, and one bf16 ulp is up to 2^-7 of the value (measured here: 6.94e-3 = 2^-7 / 1.125 on
    one row of "tail_only", 4.5e-3 and less elsewhere; tests/test_gpu_moe_routing.py's ROW_BAR for the streaming bf16 form,
    4.6e-3, is four times a measured value and below one ulp, so it is printed, not asserted)."""
    ids, x, w1, w2, wts, per_slot, summed = random_case(name)
    w1, w2 = w1.cuda(), w2.cuda()
    for block_m in (128, 64):
        what = f"bf16 tiled {block_m} {name}"
        out = run_experts(monkeypatch, x, w1, w2, ids, wts, floor=1, block_m=block_m)
        foul = run_experts(monkeypatch, x, w1, w2, ids, wts, floor=1, block_m=block_m, poisoned=True)
        assert torch.isfinite(foul.float()).all(), f"{what}: slot rows hold unwritten scratch"
        assert torch.equal(foul, out), f"{what}: poisoned != unpoisoned"
        total = run_experts(monkeypatch, x, w1, w2, ids, wts, floor=1, block_m=block_m, reduce_topk=True)
        rows = (out.float() - per_slot.float()).abs().amax(1) / per_slot.float().abs().amax(1)
        print(f"BF16-TILED fused_experts random {what}: per slot peak err {max_rel_to_peak(out, per_slot):.3e}, worst row "
              f"{float(rows.max()):.4e} (bar 1e-2; the streaming form's measured bar {ROW_BAR['bf16']:.4e}), summed peak err "
              f"{max_rel_to_peak(total, summed):.3e}")
        assert_close(out, per_slot, 1e-2, what=what)
        assert_close_elementwise(out, per_slot, what=what)
        assert_close(total, summed, 1e-2, what=what + " summed")
        assert_close_elementwise(total, summed, what=what + " summed")
        assert float(rows.max()) < 1e-2, (what, float(rows.max()), int(rows.argmax()))
        if block_m == 128:
            first = out
        else:
            assert torch.equal(out, first), f"{name}: block_m 64 != block_m 128"


def test_generic_bf16_calls_keep_the_streaming_form(monkeypatch):
    """No floor given: the module default (0 = never), whatever the size."""
    ids, x, w1, w2, wts, want = integer_case("edges")
    from chitu_amd import _lib, fused_moe

    _lib.call_log = []
    try:
        out = fused_moe.fused_experts(x.cuda(), w1.cuda(), w2.cuda(), wts.cuda(), ids.cuda(), reduce_topk=False).cpu()
        called = {n for n, _ in _lib.call_log if "gemm" in n}
    finally:
        _lib.call_log = None
    assert called == {"chitu_hip_moe_gemm_bf16"} and torch.equal(out.view(-1, K4), want)


# ---------------------------------------------------------------- 4. the router at Qwen3-MoE's shapes
@pytest.mark.parametrize("E_r,topk", [(128, 8), (16, 4)])
@pytest.mark.parametrize("score_func", ["softmax_renorm", "softmax"])
@pytest.mark.parametrize("fused_align", [False, True])
def test_router_at_qwen3_moe_shapes_is_exact_against_the_cpu_oracle(E_r, topk, score_func, fused_align):
    """bf16 logits drawn from route_exact's softmax grid (distinct per row, so the top-k is unique), delivered as one fp32
    plane: ids equal the oracle's; weights obey route_exact.softmax_weight_ok (a bf16 neighbour of the float64 value, the
    nearest one away from midpoints); with the align fused in, the sorted ids are moe_align's."""
    from chitu_amd import fused_moe, ops

    M = 37
    g = np.random.default_rng(E_r + topk)
    grid = rx.SOFTMAX_GRID
    logits = np.stack([g.choice(grid, size=E_r, replace=False) for _ in range(M)]).astype(np.float32)
    want = rx.spec(rx.Case("qwen3_moe", "grid", E_r, topk=topk, score=score_func, M=M, scale=1.0), logits, None)
    order, w64 = want["ids"], want["w64"]
    assert not want["cut_tie"].any()
    planes = torch.from_numpy(logits)[None].contiguous().cuda()
    gate = torch.zeros(E_r, 64, dtype=torch.bfloat16, device="cuda")  # not read: the logits are given
    align = (E_r, 16, None) if fused_align else None
    res = ops.gate_deepseek_v3(None, gate, None, 1, 1, topk, score_func, 1.0, align=align, logits_partials=planes)
    ids, w = res[1].cpu(), res[0].cpu()
    assert torch.equal(ids, torch.from_numpy(order)), "router ids differ from the CPU oracle"
    ok, share = rx.softmax_weight_ok(w64, rx.bf16_bits(w.float().numpy()))
    assert bool(np.all(ok)), f"{int((~ok).sum())} weights are no bf16 neighbour of the float64 value"
    if fused_align:
        s_ref, e_ref, n_ref = fused_moe.moe_align_block_size(res[1], 16, E_r)
        assert torch.equal(res[2][0], s_ref) and torch.equal(res[2][2], n_ref)
        nb = int(n_ref) // 16
        assert torch.equal(res[2][1][:nb], e_ref[:nb])
    print(f"QWEN3-MOE router E={E_r} top {topk} {score_func} fused_align={fused_align}: {M} rows exact, strict-rule share {share:.3f}")
