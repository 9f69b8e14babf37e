"""The grouped expert GEMMs under SKEWED routing, slot by slot, with poisoned scratch and guarded outputs.

The other MoE tests route every token through torch.randperm(E)[:topk], compare after the top-k sum against the tensor's peak
and reuse a warm workspace.  Here:
  1. `route(counts, M, topk)` builds ids with a prescribed number of slots per expert: one below / exactly / one above a block
     (16 for the streaming kernels, 64 and 128 for the tiled ones), idle experts, only-the-tail experts, hot experts, fewer /
     exactly / more than 8 m-blocks (the XCD remap of the tiled GEMM1), a token that lists one expert twice, top-1, and the
     hottest expert on another rank (expert_map -1: a multi-block zero fill).  Its self-checks run at import, without a GPU.
  2. every plain grouped GEMM entry of the C ABI on exact integer data (torch.equal against the integer matmul), its output
     between guard rows that must keep their sentinel bits: a store to row `numel` (the id of a padding slot) is seen;
  3. the SiLU-fused GEMM1 entries on the same data, every element within 2^-7 of the reference;
  4. fused_experts(reduce_topk=False) of every form on every pattern: inside tests.util.poisoned_allocations() == outside it,
     the bit identities between the forms, token permutation, the top-k sum, and the CPU oracles per slot -- whole tensor at
     the family's existing bar and ROW BY ROW (a slot computed from the wrong token or expert is wrong by its whole size).

Mutations tried by hand on the MI355X (other builds of the library, never committed) and what caught them here (the three
of the tiled kernels were made in csrc/moe_tiled.hip, before its tile walk and epilogue moved to csrc/moe_tiled_common.h):
  - csrc/moe_tiled_common.h, store_tile without `if (s >= numel) continue`: the guard rows of sections 2 and 3, all 14 cases of
    chitu_hip_moe_gemm2_fp8_tiled and chitu_hip_moe_gemm1_silu_fp8_tiled ("stored into the guard rows after the output").
    (Run against those two tests only: anywhere else the stray row lies outside the buffer.)
  - csrc/moe_tiled_common.h, `mt_valid = mt` for `mt + 1`: the exact tests of both tiled entries at block_m 128 (zeros in the last
    live 16-slot sub-tile) and the per-row bar of test_tiled_forms...[fp8-*] on all six patterns (worst row 0.76 .. 1.0).
    tests/test_gpu_moe.py sees this one too (test_prefill_tiled_expert_path_*).
  - csrc/moe_tiled_common.h, `C = nb >> 3` for `(nb + 7) >> 3`: the exact SiLU test of chitu_hip_moe_gemm1_silu_fp8_tiled (4 and 7
    blocks: nothing is computed) and test_tiled_forms...[fp8-*] on all six patterns ("poisoned != unpoisoned" or the per-row
    bar: every pattern has a block count that is no multiple of 8 at one of the two heights); of tests/test_gpu_moe.py only
    the 2048-token case notices (its other cases read the previous call's h).
  - csrc/moe.hip, moe_gemm2_q_kernel returning early for expert 7 (= E - 1 here): test_streaming_forms...[fp8-edges / top1 /
    dups], "17 (20) slot rows hold unwritten scratch" under poisoned_allocations().  tests/test_gpu_moe.py notices through its
    two- vs three-launch identity and wherever expert 7 is busy; its 8-expert oracle case [5-8-2-256-128] passes.
"""

import contextlib
import functools

import pytest
import torch

from oracle import moe as omoe
from oracle import w8a8 as ow
from tests import mxfp4_ref as mx
from tests.util import assert_close, assert_close_elementwise, max_rel_to_peak, poisoned_allocations

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. routing patterns (checked on the CPU, at import)
def n_blocks(counts, block_m):
    """moe_align's padded block count: every expert's segment is padded to whole blocks."""
    return sum((c + block_m - 1) // block_m for c in counts)


def route(counts, M, topk, blocks=None):
    """ids [M, topk] with exactly counts[e] slots on expert e.  The multiset of expert ids is laid out sorted by descending
    count (L) and token m takes L[m], L[M + m], ...: two of its entries lie M apart, an expert's run is at most max(counts)
    long, so no token lists an expert twice whenever max(counts) <= M.  blocks: {block_m: the padded block count the
    pattern is meant to give} -- asserted from the host formula sum(ceil(c / block_m))."""
    E = len(counts)
    assert sum(counts) == M * topk and max(counts) <= M, (counts, M, topk)
    order = sorted(range(E), key=lambda e: (-counts[e], e))
    L = torch.tensor([e for e in order for _ in range(counts[e])], dtype=torch.int64)
    ids = L.view(topk, M).t().contiguous()
    assert torch.bincount(ids.reshape(-1), minlength=E).tolist() == list(counts), counts
    assert all(len(set(row)) == topk for row in ids.tolist()), f"{counts}: a token lists an expert twice"
    for block_m, want in (blocks or {}).items():
        assert n_blocks(counts, block_m) == want, (counts, block_m, n_blocks(counts, block_m), want)
    return ids


E = 8
# name -> (M, topk, counts, {block_m: blocks}); "dups" is derived from "edges" below
STREAMING_PATTERNS = {  # 16-slot blocks
    "edges": (33, 2, [15, 16, 17, 1, 0, 0, 0, 17], {16: 7}),  # block - 1, block, block + 1, one slot, three idle, last busy
    "two_hot": (33, 2, [33, 0, 0, 0, 0, 33, 0, 0], {16: 6}),
    "top1": (33, 1, [15, 0, 1, 0, 0, 0, 0, 17], {16: 4}),
}
TILED_PATTERNS = {  # 64- and 128-slot blocks; 8 blocks is where the XCD remap of the tiled GEMM1 changes its shape
    "edges": (260, 2, [127, 128, 129, 1, 0, 65, 63, 7], {128: 8, 64: 12}),
    "single_slot_blocks": (260, 2, [129, 129, 129, 129, 1, 1, 1, 1], {128: 12, 64: 16}),
    "two_hot": (260, 2, [260, 0, 0, 260, 0, 0, 0, 0], {128: 6, 64: 10}),
    "tail_only": (260, 2, [0, 0, 0, 0, 0, 0, 260, 260], {128: 6, 64: 10}),
    "top1": (260, 1, [129, 0, 1, 0, 63, 3, 0, 64], {128: 6, 64: 7}),
}
PATTERNS = {"streaming": STREAMING_PATTERNS, "tiled": TILED_PATTERNS}
PATTERN_NAMES = {"streaming": sorted(STREAMING_PATTERNS) + ["dups"], "tiled": sorted(TILED_PATTERNS) + ["dups"]}


@functools.lru_cache(maxsize=None)
def pattern_ids(size, name):
    """ids [M, topk] of a pattern; "dups": the "edges" pattern with the second choice of every fourth token overwritten by its
    first -- that token lists one expert twice, and both slots are computed on their own."""
    if name == "dups":
        ids = pattern_ids(size, "edges").clone()
        ids[::4, 1] = ids[::4, 0]
        assert (ids[::4, 0] == ids[::4, 1]).all() and ids.shape[1] == 2
        return ids
    M, topk, counts, blocks = PATTERNS[size][name]
    return route(counts, M, topk, blocks)


def hottest(ids):
    return int(torch.bincount(ids.reshape(-1), minlength=E).argmax())


for _size, _names in PATTERN_NAMES.items():  # the self-checks of every pattern, GPU or not
    for _name in _names:
        _ids = pattern_ids(_size, _name)
        assert _ids.shape[0] * _ids.shape[1] >= (24 * E if _size == "tiled" else 1), "the tiled rule needs 24 slots per expert"
        assert torch.bincount(_ids.reshape(-1), minlength=E)[hottest(_ids)] > (128 if _size == "tiled" else 16), "remote = several blocks"


# ---------------------------------------------------------------- 2. + 3. the C-ABI entries on exact integer data
G = 4                 # guard rows on each side of the output
SENTINEL = 0x7FA5     # a bf16 NaN bit pattern: no result of finite data equals it
ABI_E = 4
ABI_ROUTES = {        # block_m -> (M, topk, counts): block - 1 .. block + 1 crossed, an idle expert, the hottest one first
    16: (21, 2, [17, 16, 0, 9], {16: 4}),
    64: (130, 2, [129, 65, 0, 66], {64: 7}),
    128: (130, 2, [129, 65, 0, 66], {128: 4}),
}
for _m, _t, _c, _b in ABI_ROUTES.values():
    route(_c, _m, _t, _b)
INT_CODES = torch.tensor([0, 2, 4, 5, 6, 10, 12, 13, 14], dtype=torch.uint8)  # e2m1 codes of 0, +-1, +-2, +-3, +-4


def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g)


def _pow2(g, lo, hi, *shape):
    return torch.ldexp(torch.ones(shape), torch.randint(lo, hi + 1, shape, generator=g).to(torch.int32))


def _acts(kind, rows, K, g, lo, hi):
    """Integer activations in -4..4 with power-of-two scales 2^lo..2^hi: q (what the entry reads), s (its scale tensor or
    None), deq (their exact values, float64)."""
    v = _ints(g, rows, K)
    if kind == "fp8":      # e4m3 + one fp32 scale per (row, 128-group)
        s = _pow2(g, lo, hi, rows, K // 128)
        return dict(q=v.to(torch.float8_e4m3fn), s=s, deq=v.double() * s.double().repeat_interleave(128, 1))
    if kind == "bf16":     # the scale of a row folded into its bf16 values (still exact)
        t = v.float() * _pow2(g, lo, hi, rows, 1)
        return dict(q=t.to(torch.bfloat16), s=None, deq=t.double())
    s = _pow2(g, lo, hi, rows)  # int8 + one fp32 scale per row
    return dict(q=v.to(torch.int8), s=s, deq=v.double() * s.double()[:, None])


def _weights(kind, rows, K, g, lo, hi):
    """[ABI_E, rows, K] integer weights in -4..4 with power-of-two scales, varied per block / row as the format allows."""
    v = _ints(g, ABI_E, rows, K)
    if kind == "fp8":      # [128, 128] block scales
        s = _pow2(g, lo, hi, ABI_E, (rows + 127) // 128, K // 128)
        full = s.double().repeat_interleave(128, 1)[:, :rows].repeat_interleave(128, 2)
        return dict(q=v.to(torch.float8_e4m3fn), s=s, deq=v.double() * full)
    if kind == "mxfp4":    # exact e2m1 codes, one E8M0 byte per (row, 32 k)
        codes = INT_CODES[torch.randint(0, len(INT_CODES), (ABI_E, rows, K), generator=g)]
        s = torch.randint(127 + lo, 127 + hi + 1, (ABI_E, rows, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
        q = mx.pack(codes)
        return dict(q=q, s=s, deq=mx.dequant_f32(q, s).double())
    if kind == "bf16":     # a power of two per row folded into the bf16 values
        t = v.float() * _pow2(g, lo, hi, ABI_E, rows, 1)
        return dict(q=t.to(torch.bfloat16), s=None, deq=t.double())
    s = _pow2(g, lo, hi, ABI_E, rows)  # int8, one fp32 scale per output channel
    return dict(q=v.to(torch.int8), s=s, deq=v.double() * s.double()[:, :, None])


def _exact(a_deq, w_deq, flat_ids, a_div, lo_a, lo_w):
    """The matmul of the exact values per slot, float64 [numel, rows]; every partial sum is an integer multiple of
    2^(lo_a + lo_w) and, in those units, below 2^24: fp32 holds it whatever the summation order."""
    K = a_deq.shape[1]
    assert float(a_deq.abs().max() * w_deq.abs().max() * K) / 2.0 ** (lo_a + lo_w) < 2 ** 24
    out = torch.zeros(flat_ids.numel(), w_deq.shape[1], dtype=torch.float64)
    for e in range(w_deq.shape[0]):
        sel = (flat_ids == e).nonzero().view(-1)
        out[sel] = a_deq[sel // a_div] @ w_deq[e].T
    return out


# name -> (C entry, activation format, weight format, activation row of a slot = slot / (topk or 1), moe_align block,
#          multiplies the routed weight, weight_kind of the bf16 entry)
PLAIN_ENTRIES = {
    "gemm1_fp8": ("chitu_hip_moe_gemm1_fp8", "fp8", "fp8", "topk", 16, False, None),
    "gemm2_fp8": ("chitu_hip_moe_gemm2_fp8", "fp8", "fp8", 1, 16, True, None),
    "gemm2_fp8_tiled_64": ("chitu_hip_moe_gemm2_fp8_tiled", "fp8", "fp8", 1, 64, True, None),
    "gemm2_fp8_tiled_128": ("chitu_hip_moe_gemm2_fp8_tiled", "fp8", "fp8", 1, 128, True, None),
    "gemm_mxfp4_a_div_topk": ("chitu_hip_moe_gemm_mxfp4", "fp8", "mxfp4", "topk", 16, False, None),
    "gemm_mxfp4_a_div_1": ("chitu_hip_moe_gemm_mxfp4", "fp8", "mxfp4", 1, 16, True, None),
    "gemm2_mxfp4_tiled_64": ("chitu_hip_moe_gemm2_mxfp4_tiled", "fp8", "mxfp4", 1, 64, True, None),
    "gemm2_mxfp4_tiled_128": ("chitu_hip_moe_gemm2_mxfp4_tiled", "fp8", "mxfp4", 1, 128, True, None),
    "gemm_bf16_kind_0": ("chitu_hip_moe_gemm_bf16", "bf16", "bf16", 1, 16, True, 0),
    "gemm_bf16_kind_1": ("chitu_hip_moe_gemm_bf16", "bf16", "fp8", 1, 16, True, 1),
    "i8_gemm2": ("chitu_hip_moe_i8_gemm2", "int8", "int8", 1, 16, True, None),
}
SILU_ENTRIES = {
    "gemm1_silu_fp8": ("chitu_hip_moe_gemm1_silu_fp8", "fp8", "fp8", "topk", 16, False, None),
    "gemm1_silu_fp8_tiled_64": ("chitu_hip_moe_gemm1_silu_fp8_tiled", "fp8", "fp8", "topk", 64, False, None),
    "gemm1_silu_fp8_tiled_128": ("chitu_hip_moe_gemm1_silu_fp8_tiled", "fp8", "fp8", "topk", 128, False, None),
    "gemm1_silu_mxfp4": ("chitu_hip_moe_gemm1_silu_mxfp4", "fp8", "mxfp4", "topk", 16, False, None),
    "gemm1_silu_mxfp4_tiled_64": ("chitu_hip_moe_gemm1_silu_mxfp4_tiled", "fp8", "mxfp4", "topk", 64, False, None),
    "gemm1_silu_mxfp4_tiled_128": ("chitu_hip_moe_gemm1_silu_mxfp4_tiled", "fp8", "mxfp4", "topk", 128, False, None),
    "i8_gemm1_silu": ("chitu_hip_moe_i8_gemm1_silu", "int8", "int8", "topk", 16, False, None),
    "gemm_bf16_silu_kind_0": ("chitu_hip_moe_gemm_bf16", "bf16", "bf16", "topk", 16, False, 0),
    "gemm_bf16_silu_kind_1": ("chitu_hip_moe_gemm_bf16", "bf16", "fp8", "topk", 16, False, 1),
}


def _launch(spec, A, W, ids, wts, n_out, K, silu, remote):
    """One launch of a grouped GEMM entry with the arguments the wrappers of chitu_amd.fused_moe pass: moe_align with the
    entry's own block size, max_mblocks = min(len(expert_ids), numel).  The output lies between G guard rows filled, like the
    output itself, with SENTINEL; the guards must come back untouched.  Returns the bf16 [numel, n_out] the entry wrote."""
    from chitu_amd import _lib, fused_moe
    from chitu_amd._lib import check, i32, i64, ptr, stream_ptr

    entry, _, _, a_div, block_m, routed, kind = spec
    M, topk = ids.shape
    numel = ids.numel()
    a_div = topk if a_div == "topk" else 1
    emap = None
    if remote is not None:
        emap = torch.arange(ABI_E, dtype=torch.int32)
        emap[remote] = -1
        emap = emap.cuda()
    sorted_ids, expert_ids, npost = fused_moe.moe_align_block_size(ids.cuda(), block_m, ABI_E, emap)
    assert int(npost) == n_blocks(torch.bincount(ids.reshape(-1), minlength=ABI_E).tolist(), block_m) * block_m
    mmb = min(expert_ids.numel(), numel)
    full = torch.full((numel + 2 * G, n_out), SENTINEL, dtype=torch.int16, device="cuda")
    out = full[G:]  # the entry is handed row G
    keep = [A["q"].cuda(), None if A["s"] is None else A["s"].float().cuda(), W["q"].cuda(),
            None if W["s"] is None else (W["s"] if W["s"].dtype == torch.uint8 else W["s"].float()).cuda(),
            wts.cuda() if routed else None]
    a, a_s, w, w_s, tw = (ptr(t) for t in keep)
    al = (ptr(sorted_ids), ptr(expert_ids), ptr(npost))
    rw = (tw, i32(0), i32(1 if routed else 0))  # routed weights are bf16 (dtype code 0)
    dims = (i64(numel), i64(n_out), i64(K), i64(mmb))
    st = stream_ptr()
    fn = getattr(_lib.lib(), entry)
    if entry == "chitu_hip_moe_gemm1_fp8":
        rc = fn(a, a_s, w, w_s, *al, ptr(out), i64(numel), i32(topk), i64(n_out), i64(K), i64(mmb), st)
    elif entry in ("chitu_hip_moe_gemm2_fp8", "chitu_hip_moe_i8_gemm2"):
        rc = fn(a, a_s, w, w_s, *al, *rw, ptr(out), *dims, st)
    elif entry in ("chitu_hip_moe_gemm2_fp8_tiled", "chitu_hip_moe_gemm2_mxfp4_tiled"):
        rc = fn(a, a_s, w, w_s, *al, *rw, ptr(out), *dims, i32(block_m), st)
    elif entry == "chitu_hip_moe_gemm_mxfp4":
        rc = fn(a, a_s, i32(a_div), w, w_s, *al, *rw, ptr(out), *dims, st)
    elif entry == "chitu_hip_moe_gemm_bf16":
        rc = fn(a, i32(a_div), w, w_s, i32(kind), *al, *rw, i32(1 if silu else 0), ptr(out), *dims, st)
    elif entry in ("chitu_hip_moe_gemm1_silu_fp8", "chitu_hip_moe_gemm1_silu_mxfp4", "chitu_hip_moe_i8_gemm1_silu"):
        rc = fn(a, a_s, w, w_s, *al, ptr(out), i64(numel), i32(topk), i64(n_out), i64(K), i64(mmb), st)
    elif entry in ("chitu_hip_moe_gemm1_silu_fp8_tiled", "chitu_hip_moe_gemm1_silu_mxfp4_tiled"):
        rc = fn(a, a_s, w, w_s, *al, ptr(out), i64(numel), i32(topk), i64(n_out), i64(K), i64(mmb), i32(block_m), st)
    else:
        raise KeyError(entry)
    check(rc, entry)
    torch.cuda.synchronize()
    got = full.cpu()
    for side, rows in (("before", got[:G]), ("after", got[G + numel:])):
        touched = (rows != SENTINEL).nonzero()
        assert len(touched) == 0, f"{entry}: stored into the guard rows {side} the output, first (row, col): {touched[:8].tolist()}"
    return got[G:G + numel].view(torch.bfloat16)


def _abi_case(spec, K, w_rows, seed, lo_a, hi_a, lo_w, hi_w):
    _, act, wt, a_div, block_m, _, _ = spec
    M, topk, counts, blocks = ABI_ROUTES[block_m]
    ids = route(counts, M, topk, blocks)
    g = torch.Generator().manual_seed(seed)
    A = _acts(act, M if a_div == "topk" else M * topk, K, g, lo_a, hi_a)
    W = _weights(wt, w_rows, K, g, lo_w, hi_w)
    wts = torch.tensor([0.5, 2.0, 1.0, 4.0]).repeat(M * topk)[: M * topk].view(M, topk).to(torch.bfloat16)
    exact = _exact(A["deq"], W["deq"], ids.reshape(-1), topk if a_div == "topk" else 1, lo_a, lo_w)
    return ids, A, W, wts, exact


@pytest.mark.parametrize("K,N", [(128, 128), (128, 200), (384, 128), (384, 200), (256, 1160)])
@pytest.mark.parametrize("name", sorted(PLAIN_ENTRIES))
def test_plain_grouped_gemm_entries_are_exact_on_integer_data_and_keep_their_guard_rows(name, K, N):
    """Activations and weights are integers in -4..4 (e4m3, exact e2m1 codes, bf16 or int8), every scale a power of two 2^-2..2^2
    varied per (row, group) / [128, 128] block / (row, 32 k) / row / channel, routed weights from {0.5, 1, 2, 4}: every product
    and partial sum is a multiple of 2^-4 below 2^20, so whatever the order of the sum the fp32 accumulator holds THE matmul,
    and the output is that value times the routed weight, rounded once to bf16 (the int8 entry rounds the scaled sum to bf16
    first and the product again: with a power-of-two weight the second rounding changes nothing, and the reference below does
    both).  torch.equal for every real slot row; N = 200 is no multiple of 128 nor of 16 (clamped tail rows of the weight
    tile); (K, N) = (256, 1160) is ten 128-row tiles of two K blocks each, which the tiled GEMM2 entries walk four to a
    workgroup (4, 4 and 2 tiles: the last group is partial, its last tile has 8 live rows); the G rows before and after
    the output keep their sentinel bits (a store to row numel, the id of a padding slot, would land in the first guard row
    after it).  Run once more with the hottest expert on another rank (expert_map -1):
    its slots, several blocks of them, come out as zeros and nothing else moves."""
    spec = PLAIN_ENTRIES[name]
    routed = spec[5]
    ids, A, W, wts, exact = _abi_case(spec, K, N, seed=K + N, lo_a=-2, hi_a=2, lo_w=-2, hi_w=2)
    want = exact.float() * (wts.float().view(-1, 1) if routed else 1.0)
    assert float(want.abs().max()) < 2 ** 24 and torch.equal(want.double(), exact * (wts.double().view(-1, 1) if routed else 1.0))
    if name == "i8_gemm2":  # bf16( bf16(sum x scales) x routed weight )
        want = exact.float().to(torch.bfloat16).float() * wts.float().view(-1, 1)
    want = want.to(torch.bfloat16)
    for remote in (None, 0):
        got = _launch(spec, A, W, ids, wts, N, K, silu=False, remote=remote)
        expect = want.clone()
        if remote is not None:
            expect[ids.reshape(-1) == remote] = 0
        bad = (got.view(torch.int16) != expect.view(torch.int16)).nonzero()
        bad = bad[(got.float() != expect.float())[bad[:, 0], bad[:, 1]]]  # (+0 and -0 are the same result)
        assert len(bad) == 0, (f"{name} K={K} N={N} remote={remote}: {len(bad)} elements differ from the exact result, first "
                               f"(slot, n, got, want): {[(int(s), int(n), float(got[s, n]), float(expect[s, n])) for s, n in bad[:6]]}")
        assert torch.equal(got, expect)


@pytest.mark.parametrize("K,I", [(128, 128), (384, 128), (384, 640)])
@pytest.mark.parametrize("name", sorted(SILU_ENTRIES))
def test_silu_fused_gemm1_entries_on_integer_data_within_two_bf16_ulps(name, K, I):
    """The data of the test above with scales 2^-4..2^-2 for activations and for weights: gate and up are exact multiples of
    2^-8 of magnitude <= 48 (asserted), so SiLU sees its whole interesting range and nothing underflows.  The entry's only freedom
    is the device expf (and the division) inside SiLU.  Reference, in fp32 on the CPU: h = bf16(bf16(silu(bf16(g))) * bf16(u)).
    Bar (derived, not measured): |h - ref| <= 2^-7 |ref| for every element -- SiLU's value may fall on the other side of a bf16
    rounding boundary (one ulp), that ulp is carried through the product, the final rounding adds one more.  The worst element
    is printed before the assertion.  Guard rows and remote expert as above.
    Measured on the MI355X: all nine entries return the reference's bits for every element of every case."""
    spec = SILU_ENTRIES[name]
    ids, A, W, wts, exact = _abi_case(spec, K, 2 * I, seed=K + I + 1, lo_a=-4, hi_a=-2, lo_w=-4, hi_w=-2)
    assert float(exact.abs().max()) <= 48.0
    gate, up = exact[:, :I].float().to(torch.bfloat16).float(), exact[:, I:].float().to(torch.bfloat16).float()
    want = (torch.nn.functional.silu(gate).to(torch.bfloat16).float() * up).to(torch.bfloat16)
    for remote in (None, 0):
        got = _launch(spec, A, W, ids, wts, I, K, silu=True, remote=remote)
        expect = want.clone()
        if remote is not None:
            expect[ids.reshape(-1) == remote] = 0
        assert torch.isfinite(got.float()).all()
        err, bar = (got.float() - expect.float()).abs(), 2.0 ** -7 * expect.float().abs()
        i = int((err - bar).argmax())
        s, n = divmod(i, I)
        print(f"{name} K={K} I={I} remote={remote}: {int((err != 0).sum())} of {err.numel()} differ; worst: slot {s} col {n} "
              f"g={float(gate[s, n])} u={float(up[s, n])} got {float(got[s, n])} want {float(expect[s, n])} = "
              f"{float(err.flatten()[i] / bar.flatten()[i].clamp_min(1e-45)):.3f} of the bar")
        assert bool((err <= bar).all()), f"{name}: {int((err > bar).sum())} elements beyond 2^-7 of the reference"


# ---------------------------------------------------------------- 4. fused_experts per slot
K4, I4, I_WIDE = 256, 128, 640
GEMM_ENTRIES = {v[0] for v in PLAIN_ENTRIES.values()} | {v[0] for v in SILU_ENTRIES.values()} | {
    "chitu_hip_moe_gemm2_quant_fp8", "chitu_hip_moe_gemm2_quant_mxfp4"}
EXPECTED_ENTRIES = {
    ("fp8", "two"): {"chitu_hip_moe_gemm1_silu_fp8", "chitu_hip_moe_gemm2_quant_fp8"},
    ("fp8", "three"): {"chitu_hip_moe_gemm1_fp8", "chitu_hip_moe_gemm2_fp8"},
    ("fp8", "tiled"): {"chitu_hip_moe_gemm1_silu_fp8_tiled", "chitu_hip_moe_gemm2_fp8_tiled"},
    ("mxfp4", "two"): {"chitu_hip_moe_gemm1_silu_mxfp4", "chitu_hip_moe_gemm2_quant_mxfp4"},
    ("mxfp4", "tiled"): {"chitu_hip_moe_gemm1_silu_mxfp4_tiled", "chitu_hip_moe_gemm2_mxfp4_tiled"},
    ("bf16", "two"): {"chitu_hip_moe_gemm_bf16"},
    ("soft_fp8", "two"): {"chitu_hip_moe_gemm_bf16"},
    ("int8", "two"): {"chitu_hip_moe_i8_gemm1_silu", "chitu_hip_moe_i8_gemm2"},
}


@functools.lru_cache(maxsize=None)
def family_weights(family, I):
    """Random expert weights as the family's own test file builds them (tests/test_gpu_moe.py::make_case,
    test_gpu_moe_mxfp4.py::twin_case, test_gpu_moe_int8.py::make_case), E experts, K4 -> 2I -> K4.  Built once, never changed."""
    g = torch.Generator().manual_seed(1000 + I + len(family))
    if family in ("fp8", "soft_fp8"):
        w1 = (torch.randn(E, 2 * I, K4, generator=g) * 0.5).to(torch.float8_e4m3fn)
        w2 = (torch.randn(E, K4, I, generator=g) * 0.5).to(torch.float8_e4m3fn)
        w1s = torch.rand(E, 2 * I // 128, K4 // 128, generator=g) * 0.02 + 0.01
        w2s = torch.rand(E, K4 // 128, I // 128, generator=g) * 0.02 + 0.01
        return dict(w1=w1, w2=w2, w1s=w1s, w2s=w2s)
    if family == "mxfp4":
        w1, w1s, _, _ = mx.fp8_twin_weights(E, 2 * I, K4, g)
        w2, w2s, _, _ = mx.fp8_twin_weights(E, K4, I, g)
        return dict(w1=w1, w2=w2, w1s=w1s, w2s=w2s)
    if family == "bf16":
        return dict(w1=(torch.randn(E, 2 * I, K4, generator=g) * K4 ** -0.5).to(torch.bfloat16),
                    w2=(torch.randn(E, K4, I, generator=g) * I ** -0.5).to(torch.bfloat16), w1s=None, w2s=None)
    assert family == "int8"
    w1, s1 = zip(*(ow.quant_weight(w) for w in torch.randn(E, 2 * I, K4, generator=g) * K4 ** -0.5))
    w2, s2 = zip(*(ow.quant_weight(w) for w in torch.randn(E, K4, I, generator=g) * I ** -0.5))
    return dict(w1=torch.stack(w1), w2=torch.stack(w2), w1s=torch.stack(s1), w2s=torch.stack(s2))


@functools.lru_cache(maxsize=None)
def tokens(M):
    return (torch.randn(M, K4, generator=torch.Generator().manual_seed(M)) * 0.5).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def slot_oracle(family, size, name, I=I4):
    """The family's CPU oracle on the flattened problem: token row of every slot, top-1, routed weight 1 -- its top-k sum is
    then the identity and it returns one row per slot, [numel, K4].  Computed once per (family, pattern)."""
    ids = pattern_ids(size, name)
    w = family_weights(family, I)
    x = tokens(ids.shape[0]).repeat_interleave(ids.shape[1], 0)
    flat, ones = ids.reshape(-1, 1), torch.ones(ids.numel(), 1, dtype=torch.bfloat16)
    if family == "fp8":
        return omoe.fused_experts_fp8(x, w["w1"], w["w2"], ones, flat, w["w1s"], w["w2s"])
    if family == "mxfp4":
        return mx.fused_experts_mxfp4(x, w["w1"], w["w1s"], w["w2"], w["w2s"], ones, flat)
    if family == "bf16":
        return omoe.fused_experts_bf16(x, w["w1"], w["w2"], ones, flat)
    if family == "soft_fp8":
        return omoe.fused_experts_soft_fp8(x, w["w1"], w["w2"], ones, flat, w["w1s"], w["w2s"])
    return ow.fused_experts_int8(x, w["w1"], w["w2"], ones, flat, w["w1s"], w["w2s"])


@functools.lru_cache(maxsize=None)
def _device_weights(family, I):
    return {k: None if v is None else v.cuda() for k, v in family_weights(family, I).items()}


@contextlib.contextmanager
def _form(monkeypatch, form):
    """form: "two" (streaming, SiLU fused into GEMM1), "three" (streaming, CHITU_MOE_FUSE_SILU=0), "tiled_64" / "tiled_128";
    a trailing "_wk1" switches the streaming kernels' K split off (debug_option moe_gemm1_wk = 1)."""
    from chitu_amd import fused_moe
    from chitu_amd._lib import debug_option

    wk1 = form.endswith("_wk1")
    base = form[:-4] if wk1 else form
    with monkeypatch.context() as m:
        if base.startswith("tiled"):
            m.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 128)
            m.setattr(fused_moe, "_MOE_MXFP4_TILED_MIN_TOKENS", 128)
            m.setattr(fused_moe, "_MOE_TILED_BLOCK_M", int(base.split("_")[1]))
        else:
            m.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 0)  # the tiled form off, whatever the token count
        m.setenv("CHITU_MOE_FUSE_SILU", "0" if base == "three" else "1")
        with (debug_option("moe_gemm1_wk", 1) if wk1 else contextlib.nullcontext()):
            yield


def run(monkeypatch, family, form, x, ids, I=I4, remote=None, reduce_topk=False, poisoned=False):
    """fused_experts of the family in the given form with every routed weight 1.0; returns the per-slot output [numel, K4]
    (reduce_topk=False) or the summed one [M, K4] on the CPU, and checks against the C-ABI call log that the call went
    through the form's grouped GEMM entries and no others.  remote: that expert lives on another rank (expert_map -1)."""
    from chitu_amd import _lib, fused_moe

    w = _device_weights(family, I)
    M, topk = ids.shape
    kw = dict(reduce_topk=reduce_topk)
    if remote is not None:
        emap = torch.arange(E, dtype=torch.int32)
        emap[remote] = -1
        kw.update(expert_map=emap.cuda(), global_num_experts=E)
    if family == "fp8":
        kw.update(use_fp8_w8a8=True, w1_scale=w["w1s"], w2_scale=w["w2s"], block_shape=[128, 128])
    elif family == "mxfp4":
        kw.update(use_mxfp4_w4a8=True, w1_scale=w["w1s"], w2_scale=w["w2s"])
    elif family == "soft_fp8":
        kw.update(use_fp8_w8a8=True, soft_fp8=True, w1_scale=w["w1s"], w2_scale=w["w2s"], block_shape=[128, 128])
    elif family == "int8":
        kw.update(use_int8_w8a8=True, w1_scale=w["w1s"], w2_scale=w["w2s"])
    args = (x.cuda(), w["w1"], w["w2"], torch.ones(M, topk, dtype=torch.bfloat16, device="cuda"), ids.cuda())
    with _form(monkeypatch, form), (poisoned_allocations() if poisoned else contextlib.nullcontext()):
        _lib.call_log = []
        try:
            out = fused_moe.fused_experts(*args, **kw).cpu()  # (a view of the workspace: copied before the next call)
            called = {n for n, _ in _lib.call_log} & GEMM_ENTRIES
        finally:
            _lib.call_log = None
    base = form[:-4] if form.endswith("_wk1") else form
    key = "tiled" if base.startswith("tiled") else "three" if (base == "three" or I > 512) and family == "fp8" else "two"
    assert called == EXPECTED_ENTRIES[family, key], (family, form, sorted(called))
    return out.view(-1, K4) if not reduce_topk else out


def _rel_mean(a, b):
    return ((a.float() - b.float()).abs().mean() / b.float().abs().mean()).item()


def _whole_tensor_bar(family, tiled, out, ref, what):
    """The bar of the family's existing oracle test, taken from its file and not loosened: tests/test_gpu_moe.py::test_vs_oracle
    (fp8: assert_close 1e-2, mean < 5e-3), ::test_bf16_experts_vs_oracle / ::test_soft_fp8_... (assert_close 1e-2 +
    assert_close_elementwise), test_gpu_moe_int8.py (assert_close 1e-2, mean < 5e-3), test_gpu_moe_mxfp4.py::_bars (the same),
    and for the tiled forms at hundreds of rows ::test_prefill_tiled_expert_path... / test_gpu_moe_mxfp4_tiled.py
    (assert_close 2e-2, mean < 5e-3)."""
    print(f"{what}: peak err {max_rel_to_peak(out, ref):.3e}, mean err {_rel_mean(out, ref):.3e}")
    assert_close(out, ref, 2e-2 if tiled else 1e-2, what=what)
    if family in ("bf16", "soft_fp8"):
        assert_close_elementwise(out, ref, what=what)
    else:
        assert _rel_mean(out, ref) < 5e-3, what


# Second bar, per slot row: max|out_row - ref_row| / max|ref_row|.  A slot computed from the wrong token or the wrong expert is
# off by about its whole size here (the experts are independent random matrices), however small its routed weight or however
# many good rows surround it.  MEASURED on the MI355X against the CPU oracle (never against another form of the kernels), worst
# row over all patterns (remote-expert runs included) and forms of the family; the bar is 4 x that (room for one e4m3 code of
# h flipping on a rounding boundary in a row whose own peak is small), capped at 0.1 (an order of magnitude below a wrong row).
#   family     measured worst row, per form                                                   worst        bar = 4 x worst
#   fp8        two- / three-launch 7.4074e-03, 640-wide 6.8408e-03, tiled 64 / 128 1.4387e-02  1.4387e-02   5.7548e-02
#   mxfp4      streaming 3.8168e-03, tiled 64 / 128 1.5385e-02                                  1.5385e-02   6.1540e-02
#   bf16       1.1521e-03                                                                       1.1521e-03   4.6084e-03
#   soft_fp8   2.6882e-03                                                                       2.6882e-03   1.0753e-02
#   int8       0 (integer dots, the oracle's order of the two scale products, the same bf16      0            0
#              and int8 codes everywhere: every slot row equals the oracle's bit for bit)
ROW_WORST = {"fp8": 1.4387e-02, "mxfp4": 1.5385e-02, "bf16": 1.1521e-03, "soft_fp8": 2.6882e-03, "int8": 0.0}
ROW_BAR = {family: min(4 * worst, 0.1) for family, worst in ROW_WORST.items()}


def _per_row_bar(family, out, ref, live, what):
    peaks = ref.float().abs().amax(1)[live]
    assert float(peaks.min()) > 0, f"{what}: the oracle has an all-zero row"
    rows = (out.float() - ref.float()).abs().amax(1)[live] / peaks
    print(f"{what}: worst row {float(rows.max()):.4e} (row {int(rows.argmax())} of {len(rows)}), bar {ROW_BAR[family]:.4e}")
    assert float(rows.max()) <= ROW_BAR[family], (what, float(rows.max()), int(rows.argmax()))


def _check_form(monkeypatch, family, form, size, name, I=I4):
    """Everything that holds for one form on one pattern; returns its per-slot output."""
    ids = pattern_ids(size, name)
    M, topk = ids.shape
    x = tokens(M)
    what = f"{family} {form} I={I} {size}/{name}"
    out = run(monkeypatch, family, form, x, ids, I)
    # poisoned scratch: a row that no launch of THIS call wrote reads back as NaN instead of the previous call's value
    foul = run(monkeypatch, family, form, x, ids, I, poisoned=True)
    assert torch.isfinite(foul.float()).all(), f"{what}: {int((~torch.isfinite(foul.float())).any(1).sum())} slot rows hold unwritten scratch"
    assert torch.equal(foul, out), f"{what}: poisoned != unpoisoned"
    # the CPU oracle: whole tensor, then row by row
    ref = slot_oracle(family, size, name, I)
    _whole_tensor_bar(family, form.startswith("tiled"), out, ref, what)
    _per_row_bar(family, out, ref, torch.ones(ids.numel(), dtype=torch.bool), what)
    # permuting the tokens permutes the slot rows
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(7))
    moved = run(monkeypatch, family, form, x[perm].contiguous(), ids[perm].contiguous(), I)
    assert torch.equal(moved.view(M, topk, K4), out.view(M, topk, K4)[perm]), f"{what}: token permutation"
    # the summed output is moe_sum's arithmetic of the per-slot output: fp32 sum over the top-k, rounded once
    assert torch.equal(run(monkeypatch, family, form, x, ids, I, reduce_topk=True), out.view(M, topk, K4).float().sum(1).to(torch.bfloat16)), f"{what}: top-k sum"
    # the hottest expert on another rank: its slots (several blocks) are exactly zero, every other slot keeps its bits
    hot = hottest(ids)
    gone = ids.reshape(-1) == hot
    mapped = run(monkeypatch, family, form, x, ids, I, remote=hot)
    mapped_foul = run(monkeypatch, family, form, x, ids, I, remote=hot, poisoned=True)
    assert torch.isfinite(mapped_foul.float()).all() and torch.equal(mapped_foul, mapped), f"{what}: remote expert, poisoned != unpoisoned"
    assert bool((mapped[gone].float() == 0).all()), f"{what}: slots of the remote expert are not zero"
    assert torch.equal(mapped[~gone], out[~gone]), f"{what}: a remote expert moved other slots"
    masked = ref.clone()
    masked[gone] = 0
    _whole_tensor_bar(family, form.startswith("tiled"), mapped, masked, what + " remote")
    _per_row_bar(family, mapped, masked, ~gone, what + " remote")
    return out


@pytest.mark.parametrize("name", PATTERN_NAMES["streaming"])
@pytest.mark.parametrize("family", ["fp8", "mxfp4", "bf16", "soft_fp8", "int8"])
def test_streaming_forms_per_slot_under_skewed_routing_and_poisoned_scratch(family, name, monkeypatch):
    """33 tokens, 16-slot blocks: every streaming form of the family on the pattern (see _check_form), and for fp8 the
    two-launch form == the three-launch form bit for bit (same K split), plus the three-launch form of 640-wide experts.
    Measured per-row values: see ROW_BAR."""
    out = _check_form(monkeypatch, family, "two", "streaming", name)
    if family == "fp8":
        three = _check_form(monkeypatch, family, "three", "streaming", name)
        assert_close(out, three, 4e-3, what="two- vs three-launch, each with its own K split")
        ids, x = pattern_ids("streaming", name), tokens(33)
        assert torch.equal(run(monkeypatch, family, "two_wk1", x, ids), run(monkeypatch, family, "three_wk1", x, ids)), "two-launch != three-launch"
        _check_form(monkeypatch, family, "two", "streaming", name, I=I_WIDE)  # I > 512: run() asserts the three-launch entries


@pytest.mark.parametrize("name", PATTERN_NAMES["tiled"])
@pytest.mark.parametrize("family", ["fp8", "mxfp4"])
def test_tiled_forms_per_slot_under_skewed_routing_and_poisoned_scratch(family, name, monkeypatch):
    """260 tokens: the tiled form at block heights 64 and 128 on the pattern (see _check_form); 64 == 128 bit for bit; for
    MXFP4 both == the streaming form without its K split.  Measured per-row values: see ROW_BAR."""
    ids = pattern_ids("tiled", name)
    from chitu_amd import fused_moe

    with _form(monkeypatch, "tiled_128"):
        assert fused_moe._takes_tiled(ids.shape[0], ids.numel(), E, I4, K4, None)
    t128 = _check_form(monkeypatch, family, "tiled_128", "tiled", name)
    t64 = _check_form(monkeypatch, family, "tiled_64", "tiled", name)
    assert torch.equal(t64, t128), f"{family}: block_m 64 != block_m 128"
    if family == "mxfp4":
        streamed = run(monkeypatch, family, "two_wk1", tokens(ids.shape[0]), ids)
        assert torch.equal(t128, streamed), "MXFP4 tiled != MXFP4 streaming without its K split"
