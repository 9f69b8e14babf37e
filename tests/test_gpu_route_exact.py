"""Every routing kernel of gate.hip against the float64 specification of tests/route_exact.py: equal ids, equal weight bits.

The C entries chitu_hip_gate_route and chitu_hip_gate_route_align are called directly on the inputs of tests/route_exact.py
(their CPU checks, the coverage proof and the reference mutations: tests/test_route_exact_host.py).  Ids and weights start
as sentinels (-7, bf16 bits 0x7fc1) with two guard rows after the last token; chitu_hip_gate_route gets two spare columns per
row, which must stay untouched.  Sigmoid routers: ids and weight bits equal the specification.  Softmax routers: ids equal;
every weight a bf16 neighbour of the float64 value and the nearest one wherever that lies more than 2^-12 bf16-ulp from a
midpoint.  The sort's outputs (sorted_token_ids and expert_ids with spare capacity behind the allocator's, num_tokens_post_pad,
cumsum) equal oracle.moe_align on the SPECIFICATION's ids, guard words behind every array untouched; every align case is
launched three times on one ticket word, which reads 0 afterwards.  Each case runs under every launch variant that the
dispatch mirror says reaches another kernel or sort (gate_generic, gate_ticket, gate_small_sort = 0).

Mutations tried by hand on the MI355X (other builds of the library, never committed; each run once; all of them change
computed values only) -- failures among the 407 runs here, and among the 46 older router tests (test_gate_route_on_identical_
logits, test_gate_end_to_end, test_gate_route_fast_path_equals_generic_kernel, test_route_and_align_in_one_launch_equals_the_
two_launches, test_in_routing_sort_equals_general_sort, the Mixtral router tests):
  - group-rank tie `g2 <= grp` in gate_route_kernel: 84 (81 on <1>, 3 on <0>; 29 of them named edges); older tests 7.
  - the same in gate_route_fast_kernel: 71 (24 named edges), e.g. r1_bias-rand "ids differ in 3 of 3 tokens; token 0: got
    [233, 167, 196, ...] want [233, 167, 5, 196, ...]"; older tests 17.
  - the same in gate_route_align_wg_kernel<32>: 38, under the in-routing and the general sort alike; older tests 6.
  - `key == k1 ? 0u : key` dropped in gate_route_align_wg_kernel<32> (top-2 = top-1 doubled): 26; older tests 6.
  - `bf16r` removed from the plane sum (all four kernels): 136, on every one of the eight instantiations (5 to 41 each);
    older tests 0 -- their split-K logits are randn sums, where one rounding more or less rarely moves a bf16 score.
  - score_key with `+ e` (and the matching decode): 151 on the five key-based instantiations; older tests 9.
  - `renorm` ignored in gate_route_align_wg_softmax_kernel: the 8 Mixtral runs that reach it (M 1, 2, 15, 16 x both sorts);
    older tests 3.
  - masked score `-0.f` for `0.f`: the 10 runs of the unmasked_zero_vs_masked_zero edge on the key-based kernels (fast<32>,
    fast<64>, wg<32>), where -0 orders below the unmasked +0; NOT on gate_route_kernel, which compares floats (-0 == +0: the
    same ids, an equivalent program -- torch's own `scores * mask` leaves -0 there too); older tests 0.
  - `min(i, S - 1)` -> `min(i, S)` in the three clamped plane loads: 0, and rightly: the extra load is discarded by
    `i < S ? v : 0`, so the values are the same; the mutant only reads one plane further, which is why the plane buffer here
    carries two NaN planes behind the S real ones.  Not run against the older tests, whose buffers end at plane S.
"""

import contextlib

import numpy as np
import pytest
import torch

from tests import route_exact as rx

pytestmark = pytest.mark.gpu

GUARD_ROWS, SPARE_COLS, SPARE_SORTED, SPARE_BLOCKS, GUARD_WORDS = 2, 2, 5, 3, 8
INT_SENTINEL = -77

RUNS = [(c, v) for c in rx.gpu_cases() for v in rx.variants(c)]


@contextlib.contextmanager
def _options(opts):
    from chitu_amd._lib import debug_option

    with contextlib.ExitStack() as stack:
        for name, value in opts.items():
            stack.enter_context(debug_option(name, value))
        yield


def _bf16_tensor(values32):
    bits = rx.bf16_bits(values32).view(np.int16)
    return torch.from_numpy(bits.copy()).view(torch.bfloat16).cuda()


def _int_buffer(n):
    return torch.full((n + GUARD_WORDS,), INT_SENTINEL, dtype=torch.int32, device="cuda")


def _check_routing(c, d, w_bits, ids, stride, what):
    sp = d["spec"]
    k, cols = c.topk, c.cols
    assert (ids[c.M:] == rx.ID_SENTINEL).all() and (w_bits[c.M:] == rx.W_SENTINEL).all(), f"{what}: guard rows written"
    assert (ids[: c.M, cols:] == rx.ID_SENTINEL).all() and (w_bits[: c.M, cols:] == rx.W_SENTINEL).all(), \
        f"{what}: columns beyond topk + extra written"
    got = ids[: c.M, :k]
    if not np.array_equal(got, sp["ids"]):
        t = int(np.nonzero((got != sp["ids"]).any(axis=1))[0][0])
        raise AssertionError(f"{what}: ids differ in {int((got != sp['ids']).any(axis=1).sum())} of {c.M} tokens; token {t}: "
                             f"got {got[t].tolist()} want {sp['ids'][t].tolist()}")
    if cols > k:
        assert np.array_equal(ids[: c.M, k:cols], d["ids_full"][:, k:]), f"{what}: always-on ids"
        want = rx.bf16_bits(np.full((c.M, cols - k), rx.EXTRA_W, dtype=np.float32))
        assert np.array_equal(w_bits[: c.M, k:cols], want), f"{what}: always-on weights"
    gw = w_bits[: c.M, :k]
    if c.score == rx.SIGMOID:
        if not np.array_equal(gw, sp["w_bits"]):
            t, j = (int(v[0]) for v in np.nonzero(gw != sp["w_bits"]))
            raise AssertionError(f"{what}: {int((gw != sp['w_bits']).sum())} weights differ; token {t} slot {j}: "
                                 f"got {int(gw[t, j]):#06x} want {int(sp['w_bits'][t, j]):#06x}")
    else:
        ok, _ = rx.softmax_weight_ok(sp["w64"], gw)
        if not ok.all():
            t, j = (int(v[0]) for v in np.nonzero(~ok))
            raise AssertionError(f"{what}: {int((~ok).sum())} weights outside the softmax rule; token {t} slot {j}: got "
                                 f"{float(rx.bits_f32(gw[t, j])):.8g} for {sp['w64'][t, j]:.12g}")


@pytest.mark.parametrize("case,variant", RUNS, ids=[f"{c.name}-{v}" for c, v in RUNS])
def test_routing_equals_the_specification(case, variant):
    from chitu_amd import _lib
    from chitu_amd._lib import check, f32, i32, i64, ptr, stream_ptr

    c, d = case, rx.build(case)
    kernel, sort = rx.dispatch(c, **rx.VARIANTS[variant])
    what = f"{c.name} [{variant}: {kernel}, sort {sort}]"
    lib = _lib.lib()
    logits = torch.from_numpy(d["planes"]).cuda() if c.S else _bf16_tensor(d["logit"])
    bias = _bf16_tensor(d["bias"]) if d["bias"] is not None else None
    align = c.alE > 0
    stride = c.cols + (0 if align else SPARE_COLS)
    rows = c.M + GUARD_ROWS
    head = (ptr(logits), i32(c.S), i64(c.M), i32(c.E), ptr(bias), i32(c.G), i32(c.Kg), i32(c.topk),
            i32(rx.SCORE_CODE[c.score]), f32(c.scale))

    def outputs():
        w = torch.full((rows, stride), rx.W_SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        ids = torch.full((rows, stride), rx.ID_SENTINEL, dtype=torch.int64, device="cuda")
        return w, ids

    def tail(w, ids):
        return ptr(w), ptr(ids), i32(stride), i32(c.extra_id), f32(rx.EXTRA_W), i32(c.extra_n)

    with _options(rx.OPTIONS[variant]):
        if not align:
            w, ids = outputs()
            check(lib.chitu_hip_gate_route(*head, *tail(w, ids), stream_ptr()), "gate_route")
            torch.cuda.synchronize()
            _check_routing(c, d, w.view(torch.int16).cpu().numpy().view(np.uint16), ids.cpu().numpy(), stride, what)
            return
        numel = c.M * c.cols
        cap = numel + c.alE * (c.block - 1) + SPARE_SORTED
        nblk = (cap + c.block - 1) // c.block + SPARE_BLOCKS
        want = rx.align_expect(c, d["ids_full"], cap, nblk)
        emap = rx.expert_map(c)
        emap_d = torch.from_numpy(emap).cuda() if emap is not None else None
        ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
        for launch in range(3):
            w, ids = outputs()
            bufs = dict(sorted_ids=_int_buffer(cap), expert_ids=_int_buffer(nblk), num_post_pad=_int_buffer(1),
                        cumsum=_int_buffer(c.alE + 1))
            rc = lib.chitu_hip_gate_route_align(*head, *tail(w, ids), i32(c.alE), i32(c.block), ptr(bufs["sorted_ids"]), i64(cap),
                                                ptr(bufs["expert_ids"]), i64(nblk), ptr(bufs["num_post_pad"]),
                                                ptr(bufs["cumsum"]), ptr(emap_d), ptr(ticket), stream_ptr())
            check(rc, "gate_route_align")
            torch.cuda.synchronize()
            tag = f"{what} launch {launch}"
            _check_routing(c, d, w.view(torch.int16).cpu().numpy().view(np.uint16), ids.cpu().numpy(), stride, tag)
            for name, buf in bufs.items():
                got = buf.cpu().numpy()
                n = want[name].size
                assert (got[n:] == INT_SENTINEL).all(), f"{tag}: {name} written past its capacity"
                if not np.array_equal(got[:n], want[name]):
                    i = int(np.nonzero(got[:n] != want[name])[0][0])
                    raise AssertionError(f"{tag}: {name} differs at {int((got[:n] != want[name]).sum())} of {n} places, first "
                                         f"[{i}]: got {int(got[i])} want {int(want[name][i])}")
            assert int(ticket.item()) == 0, f"{tag}: the ticket word is not back at 0"
