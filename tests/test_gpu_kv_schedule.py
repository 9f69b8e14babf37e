"""The schedules of tests/kv_schedule.py with the manager on the GPU and the project's real launches: every append goes through
ops.append_to_paged_kv_cache / append_gqa_kv_fp8 / append_mla_kv_fp8 (and, for GQA layer 1, through attn_with_kvcache's own
k= / v= append) on the manager's device tables and lengths, and after every step the attention kernels read the cache through
the manager's device buffers only and must return the closed-form row of every probe (attn_exact.check_dominant):

  single-token step   attn_with_kvcache / mla_decode: key 0, the key just appended, the first key of the last page, the last key of
                      the page before, and the forbidden row at position len (kv_schedule.forbidden_q), rotating over the heads
  multi-token step    attn_with_kvcache q [bs, T, ..] / mla_decode_multi ("multi" and "composed" on the expanded buffers): query
                      (b, t) probes its own key L0 + t (even heads) and the forbidden key L0 + t + 1, the next draft (odd heads)
  continued prefill   attn_varlen_with_kvcache (bf16 pages; it refuses the fp8 K / V cache) / mla_attn_varlen_with_kvcache

each with the default split count and a forced one.  The exact gather of the host suite runs after every step (fp8 caches through
gqa_kv_dequant_fp8 / mla_kv_dequant_fp8), and ops.mla_kv_gather reads the MLA caches a second time.

test_host_a_ring_ahead queues device work, then runs 3 * _STAGE_RING single-token and multi-token prepares without a
synchronise, snapshotting the device buffers on the stream after each.  With `ev.synchronize()` removed from _stage_slot the
later steps' host writes land in pinned slots whose copies have not run yet: the test catches it (its docstring has the message).
test_a_captured_step_replayed_across_a_schedule captures ONE step per family and cache format through graphs.capture_verified --
the append launch and the attention on the manager's static buffers, the new rows and the probe queries in static tensors -- and
replays it over kv_schedule.captured_stretch: a page crossing, a newcomer on the pages a leaver freed, a reorder.
Each test prints its worst error ("KV_SCHEDULE ...", pytest -s)."""
import pytest
import torch

from tests import attn_exact as ax
from tests import kv_schedule as ks

pytestmark = pytest.mark.gpu

FORCED_SPLITS = 3


def backend(H):
    from chitu_amd.attn_backend import HipAttnBackend

    return HipAttnBackend(local_n_heads=H)


class GpuDriver(ks.Driver):
    def __init__(self, fam, fmt):
        super().__init__(fam, fmt, device="cuda")
        from chitu_amd import ops

        self.ops, self.be, self.worst, self.probes = ops, backend(fam.heads), 0.0, 0
        self.gqa, self.fp8 = fam.name == "gqa", fmt == "fp8"

    # ---- the launches in place of plain indexing
    def to_cache(self, t):
        if not self.fp8:
            return t
        return self.ops.gqa_kv_quant_fp8(t.contiguous()) if self.gqa else self.ops.mla_kv_quant_fp8(t.contiguous())

    def from_cache(self, t):
        if not self.fp8:
            return t
        return self.ops.gqa_kv_dequant_fp8(t.contiguous()) if self.gqa else self.ops.mla_kv_dequant_fp8(t.contiguous())

    def append(self, layer, table, pos, new):
        c = self.caches(layer)
        assert int(table.max()) < self.mgr.num_blocks and int(table.min()) >= 0 and int(pos.max()) < self.fam.capacity
        if self.gqa and self.fp8:
            self.ops.append_gqa_kv_fp8(c[0], c[1], table, new[0], new[1], pos)
        elif self.gqa:
            self.ops.append_to_paged_kv_cache(c[0], table, new[0].contiguous(), pos)
            self.ops.append_to_paged_kv_cache(c[1], table, new[1].contiguous(), pos)
        elif self.fp8:
            self.ops.append_mla_kv_fp8(c[0], table, new[0], pos)
        else:
            self.ops.append_to_paged_kv_cache(c[0], table, new[0].contiguous(), pos)

    def write_single(self, layer, reqs, new):
        if self.gqa and layer == 1:  # the append of attn_with_kvcache itself
            mgr, c = self.mgr, self.caches(layer)
            table = mgr.get_gpu_block_table()
            assert int(table.max()) < mgr.num_blocks and int(table.min()) >= 0
            q = torch.zeros(len(reqs), 1, self.fam.heads, 128, dtype=torch.bfloat16, device="cuda")
            self.be.attn_with_kvcache(q, c[0], c[1], k=new[0].unsqueeze(1), v=new[1].unsqueeze(1),
                                      cache_seqlens=mgr.get_gpu_seq_lens_excl_this_decode(), block_table=table, softmax_scale=self.fam.scale)
        else:
            super().write_single(layer, reqs, new)

    # ---- probes
    def value(self, req, layer, p):
        """[heads, width] fp64: what every query head gets when it picks the oracle's row p of a request"""
        v = ks.values(self.fam, ks.rows(self.fam, self.plain.incarnation(req), layer, [p]))[0]
        return v.double().repeat_interleave(self.fam.heads // self.fam.kv_heads, dim=0)

    def forbidden(self, n):
        """the query that would pick position n; where the table has no such position, the probe of n - 1"""
        return ks.forbidden_q(n) if n < self.fam.capacity else ks.probe_q(n - 1)

    def check(self, got, want):
        self.worst = max(self.worst, ax.check_dominant(got, want))
        self.probes += want.shape[0] * want.shape[1]

    def single_queries(self, reqs, layer, lens):
        """([bs, H, 64] code queries, [bs, H, width] fp64 rows): request b of lens[b] keys, head h probes single_probes()[h + b + step]"""
        fam, H = self.fam, self.fam.heads
        qv = torch.zeros(len(reqs), H, ks.CODE_W)
        want = torch.zeros(len(reqs), H, fam.width, dtype=torch.float64)
        for b, (r, n) in enumerate(zip(reqs, lens)):
            probes = ks.single_probes(n, fam.page)
            for h in range(H):
                p = probes[(h + b + self.step_no) % len(probes)]
                qv[b, h] = self.forbidden(n) if p is None else ks.probe_q(p)
                want[b, h] = self.value(r, layer, n - 1 if p is None else p)[h]
        return qv, want

    def attend_single(self, layer, reqs):
        fam, mgr, H = self.fam, self.mgr, self.fam.heads
        qv, want = self.single_queries(reqs, layer, [self.plain.length(r) for r in reqs])
        lens, table, c = mgr.get_gpu_seq_lens_incl_this_decode(), mgr.get_gpu_block_table(), self.caches(layer)
        for splits in (None, FORCED_SPLITS):
            if self.gqa:
                q = torch.zeros(len(reqs), 1, H, 128)
                q[:, 0, :, : ks.CODE_W] = qv
                out = self.be.attn_with_kvcache(q.to(torch.bfloat16).cuda(), c[0], c[1], cache_seqlens=lens, block_table=table,
                                                softmax_scale=fam.scale, num_splits=splits)[:, 0]
            else:
                out = self.be.mla_decode(torch.zeros(len(reqs), H, 512, dtype=torch.bfloat16, device="cuda"), qv.to(torch.bfloat16).cuda(),
                                         c[0], lens, table, fam.scale, num_splits=splits)
            self.check(out, want)

    def pair_queries(self, reqs, starts, counts, written, layer):
        """one query row per new row (b, t) at position s + t: even heads pick that key, odd heads the forbidden key behind it;
        both must return the row written at s + t"""
        fam, H = self.fam, self.fam.heads
        vals = ks.values(fam, written).cpu().double().repeat_interleave(H // fam.kv_heads, dim=1)  # [rows, H, width]
        qv = torch.zeros(vals.shape[0], H, ks.CODE_W)
        i = 0
        for s, c in zip(starts, counts):
            for t in range(c):
                qv[i, 0::2] = ks.probe_q(s + t)
                qv[i, 1::2] = self.forbidden(s + t + 1)
                i += 1
        return qv, vals

    def attend_multi(self, layer, reqs, T, written):
        fam, mgr, H, n = self.fam, self.mgr, self.fam.heads, len(reqs)
        starts = [self.plain.length(r) for r in reqs]
        qv, want = self.pair_queries(reqs, starts, [T] * n, written, layer)
        lens, table, c = mgr.get_gpu_multi_seq_lens_incl(), mgr.get_gpu_multi_block_table()[::T], self.caches(layer)
        for splits in (None, FORCED_SPLITS):
            if self.gqa:
                q = torch.zeros(n * T, H, 128)
                q[:, :, : ks.CODE_W] = qv
                out = self.be.attn_with_kvcache(q.view(n, T, H, 128).to(torch.bfloat16).cuda(), c[0], c[1], cache_seqlens=lens,
                                                block_table=table, causal=True, softmax_scale=fam.scale, num_splits=splits)
                self.check(out.reshape(n * T, H, 128), want)
            else:
                qn = torch.zeros(n, T, H, 512, dtype=torch.bfloat16, device="cuda")
                qp = qv.view(n, T, H, ks.CODE_W).to(torch.bfloat16).cuda()
                out = self.be.mla_decode_multi(qn, qp, c[0], lens, table, fam.scale, num_splits=splits, kernel="multi")
                self.check(out.reshape(n * T, H, 512), want)
                out = self.be.mla_decode_multi(qn, qp, c[0], lens, table, fam.scale, num_splits=splits, kernel="composed",
                                               expanded=(mgr.get_gpu_multi_block_table(), mgr.get_gpu_multi_row_lens_incl()))
                self.check(out.reshape(n * T, H, 512), want)

    def attend_continue(self, layer, reqs, counts, written):
        fam, mgr, H = self.fam, self.mgr, self.fam.heads
        if self.gqa and self.fp8:
            return  # attn_varlen_with_kvcache reads bf16 pages only (it raises NotImplementedError on the fp8 K / V cache)
        starts = [self.plain.length(r) - c for r, c in zip(reqs, counts)]
        qv, want = self.pair_queries(reqs, starts, counts, written, layer)
        cu = torch.tensor(ks.Lens(counts).cpu_prefix_lens, dtype=torch.int32, device="cuda")
        lens, table, c = mgr.get_gpu_continue_seq_lens_incl(), mgr.get_gpu_continue_block_table(), self.caches(layer)
        if self.gqa:
            q = torch.zeros(qv.shape[0], H, 128)
            q[:, :, : ks.CODE_W] = qv
            out = self.be.attn_varlen_with_kvcache(q.to(torch.bfloat16).cuda(), c[0], c[1], cu, lens, table, max(counts), causal=True,
                                                   softmax_scale=fam.scale)
        else:
            q = torch.zeros(qv.shape[0], H, 576)
            q[:, :, 512:] = qv
            total = sum(self.plain.length(r) for r in reqs)
            out = self.be.mla_attn_varlen_with_kvcache(q.to(torch.bfloat16).cuda(), c[0], cu, lens, table, max(counts), total, fam.scale)
            # ops.mla_kv_gather as a second reader of the pages: the rows of the batch, contiguous
            cu_k = torch.tensor(ks.Lens([self.plain.length(r) for r in reqs]).cpu_prefix_lens, dtype=torch.int32, device="cuda")
            got = self.ops.mla_kv_gather(c[0], table, cu_k, total)
            rows = torch.cat([self.expected(self.plain.incarnation(r), layer)[0][: self.plain.length(r)] for r in reqs])
            assert torch.equal(got, rows), f"mla_kv_gather (step {self.step_no}): not the oracle's rows"
        self.check(out, want)


CASES = [(f, fmt, n) for f in ks.FAMILIES for fmt in ks.FORMATS for n in ks.SCHEDULE_NAMES]


@pytest.mark.parametrize("family,fmt,name", CASES, ids=["-".join(c) for c in CASES])
def test_schedule(family, fmt, name):
    d = GpuDriver(ks.FAMILIES[family], fmt)
    d.run(ks.SCHEDULES[family, name])
    assert d.reused and d.skipped_copies > 0 and d.probes > 0
    print(f"KV_SCHEDULE kernel {family} {fmt} {name}: {d.step_no} steps, {d.probes} probed heads, worst absolute error {d.worst:.3e}")


class CapturedDriver(GpuDriver):
    """layer 0 of every single-token step at batch size 2 runs as ONE captured graph: append + attention on the manager's static
    device buffers.  The graph is captured at the first such step and replayed at every later one; every output is checked."""
    BATCH = 2

    def __init__(self, fam, fmt):
        super().__init__(fam, fmt)
        H, n = fam.heads, self.BATCH
        self.graph, self.replays, self.out = None, 0, None
        self.s_new = self.dev(ks.rows(fam, 0, 0, [0] * n))  # static: the step's new rows
        self.s_q = torch.zeros((n, 1, H, 128) if self.gqa else (n, H, ks.CODE_W), dtype=torch.bfloat16, device="cuda")
        self.s_qn = torch.zeros(n, H, 512, dtype=torch.bfloat16, device="cuda")

    def captured_step(self):
        mgr, c, n = self.mgr, self.caches(0), self.BATCH
        table = mgr.gpu_block_table_buffer[:n]
        excl, incl = mgr.curr_seq_lens_gpu_excl_this_decode[:n], mgr.curr_seq_lens_gpu_incl_this_decode[:n]
        if self.gqa:  # the model's form: attn_with_kvcache appends k / v at excl, then attends to excl + 1 keys
            return self.be.attn_with_kvcache(self.s_q, c[0], c[1], k=self.s_new[0].unsqueeze(1), v=self.s_new[1].unsqueeze(1),
                                             cache_seqlens=excl, block_table=table, softmax_scale=self.fam.scale)[:, 0]
        if self.fp8:
            self.ops.append_mla_kv_fp8(c[0], table, self.s_new[0], excl)
        else:
            self.ops.append_to_paged_kv_cache(c[0], table, self.s_new[0], excl)
        return self.be.mla_decode(self.s_qn, self.s_q, c[0], incl, table, self.fam.scale)

    def write_single(self, layer, reqs, new):
        if layer != 0:
            return super().write_single(layer, reqs, new)
        from chitu_amd import graphs

        assert len(reqs) == self.BATCH  # do_decode has compared the device table and both length vectors with the oracle already
        P, lens = self.fam.page, [self.plain.length(r) + 1 for r in reqs]
        hit = [(r, n) for r, n in zip(reqs, lens) if n % P and n < self.fam.capacity]
        if hit:  # the bait behind the row this step appends, before the graph runs (Driver.bait writes it only afterwards)
            idx = torch.tensor([self.mgr.block_table[r][n // P] * P + n % P for r, n in hit], device="cuda")
            bait = [ks.rows(self.fam, self.plain.incarnation(r), 0, [n], v_inc=(self.plain.incarnation(r) + 1) % ks.MAX_INCARNATIONS)
                    for r, n in hit]
            self.poke(0, idx, self.dev(tuple(torch.cat(t) for t in zip(*bait))))
        qv, want = self.single_queries(reqs, 0, lens)
        for dst, src in zip(self.s_new, new):
            dst.copy_(src)
        if self.gqa:
            self.s_q[:, 0, :, : ks.CODE_W].copy_(qv.to(torch.bfloat16))
        else:
            self.s_q.copy_(qv.to(torch.bfloat16))
        if self.graph is None:
            self.graph, _, self.out = graphs.capture_verified(self.captured_step, None, "full", None,
                                                              what=f"kv schedule step {self.fam.name} {self.fmt}")
        else:
            self.graph.replay()
            self.replays += 1
        self.check(self.out, want)


@pytest.mark.parametrize("fmt", ks.FORMATS)
@pytest.mark.parametrize("family", list(ks.FAMILIES))
def test_a_captured_step_replayed_across_a_schedule(family, fmt):
    fam = ks.FAMILIES[family]
    steps, free_b, admit_d = ks.captured_stretch(fam)
    d = CapturedDriver(fam, fmt)
    for i, st in enumerate(steps):
        if i == free_b:
            freed = set(d.mgr.block_table["b"])
        d.step(st)
        if i == admit_d:
            assert freed & set(d.mgr.block_table["d"]), "the newcomer holds none of the pages the leaver freed"
    decodes = sum(st[0] == "decode" for st in steps)
    assert d.replays == decodes - 1 and d.replays >= 9
    print(f"KV_SCHEDULE captured step {family} {fmt}: 1 capture, {d.replays} replays over a page crossing, a swap onto freed pages and "
          f"a reorder, worst absolute error {d.worst:.3e}")


def test_host_a_ring_ahead():
    """The host prepares 3 * _STAGE_RING steps while the GPU is still busy with earlier work; every step's device buffers, copied
    on the stream right behind its prepare calls, must hold that step's values.  Mutation `ev.synchronize()` removed from
    _stage_slot, tried once on an MI355X: this test failed with "length vectors of step 0: device [[21, 8, 35], [22, 9, 36]] != oracle
    [[13, 0, 27], [14, 1, 28]]" -- step 0's copy carried step 8's lengths, the slot's third use.  That needs the host to finish its
    prepares within the ~80 ms of queued matmuls; on a much slower host the mutation would pass unnoticed, the test itself never fails
    for timing."""
    from chitu_amd import cache_manager as cm

    fam = ks.GQA
    steps, T, P = 3 * cm._STAGE_RING, 2, fam.page
    d = ks.Driver(fam, "bf16", device="cuda")
    mgr, reqs = d.mgr, ["a", "b", "c"]
    mgr.register_sequence("a", P - 3)
    mgr.register_sequence("b", 0)
    mgr.register_sequence("c", 2 * P - 5)
    n = len(reqs)
    snap_lens = torch.zeros(steps, 2, n, dtype=torch.int32, device="cuda")
    snap_table = torch.zeros(steps, n, mgr.max_blocks_per_req, dtype=torch.int32, device="cuda")
    snap_multi = torch.zeros(steps, 2 * n * T + n, dtype=torch.int32, device="cuda")
    snap_mtable = torch.zeros(steps, n * T, mgr.max_blocks_per_req, dtype=torch.int32, device="cuda")
    mgr._multi_buffers()
    a = torch.randn(8192, 8192, dtype=torch.bfloat16, device="cuda")
    a @ a  # the library's first call blocks the host: not part of the queue
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(96):  # tens of milliseconds of device work in front of the copies
        a @ a
    t1.record()
    seen, seen_multi = [], []  # what the oracle needs of every step; the tensors are built after the synchronise
    for i in range(steps):
        order = reqs if i % 2 == 0 else reqs[::-1]  # the rows change every step, so every step stages a table too
        mgr.prepare_cache_decode(order)
        mgr.prepare_block_table_for_decode(order)
        snap_lens[i].copy_(mgr._lens_dev[:, :n])
        snap_table[i].copy_(mgr.get_gpu_block_table())
        seen.append((order, [mgr.seq_lens[r] for r in order], [list(mgr.block_table[r]) for r in order]))
        mgr.finalize_cache_single_decode(order)
    for i in range(steps):
        order = reqs if i % 2 == 0 else reqs[::-1]
        mgr.prepare_block_table_for_decode_multi(order, T)
        snap_multi[i].copy_(mgr._multi_dev[: 2 * n * T + n])
        snap_mtable[i].copy_(mgr.get_gpu_multi_block_table())
        seen_multi.append((order, [mgr.seq_lens[r] for r in order], [list(mgr.block_table[r]) for r in order]))
        mgr.finalize_cache_multi_decode(order, [1 + (i + b) % T for b in range(n)])
    torch.cuda.synchronize()

    def table(pages, repeat):
        t = torch.zeros(n * repeat, mgr.max_blocks_per_req, dtype=torch.int32)
        for b, ids in enumerate(pages):
            t[b * repeat : (b + 1) * repeat, : len(ids)] = torch.tensor(ids, dtype=torch.int32)
        return t

    want_lens = [torch.tensor([lens, [x + 1 for x in lens]], dtype=torch.int32) for _, lens, _ in seen]
    want_table = [table(pages, 1) for _, _, pages in seen]
    want_multi, want_mtable = [], []
    for _, lens, pages in seen_multi:
        rows = torch.tensor([x + t for x in lens for t in range(T)], dtype=torch.int32)
        want_multi.append(torch.cat([rows, torch.tensor([x + T for x in lens], dtype=torch.int32), rows + 1]))
        want_mtable.append(table(pages, T))
    for name, got, want in (("length vectors", snap_lens, want_lens), ("block table", snap_table, want_table),
                            ("multi-token lengths", snap_multi, want_multi), ("multi-token block table", snap_mtable, want_mtable)):
        got = got.cpu()
        for i in range(steps):
            assert torch.equal(got[i], want[i]), f"{name} of step {i}: device {got[i].tolist()} != oracle {want[i].tolist()}"
    print(f"KV_SCHEDULE ring: {2 * steps} steps prepared, behind {t0.elapsed_time(t1):.1f} ms of queued device work, every snapshot equal")
