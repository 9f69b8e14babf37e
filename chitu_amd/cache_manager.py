"""Paged KV cache manager: host page allocator + persistent device buffers.

Mirrors chitu/cache_manager.py:12-225 (PagedKVCacheManager): same methods, same buffers
(`curr_seq_lens_gpu_{excl,incl}_this_decode`, `gpu_block_table_buffer`, `paged_kv_cache` /
`paged_k_cache`+`paged_v_cache`).  Differences, all host-side: the free list is a deque instead
of `list(set)[0]` (the reference's own TODO, :69), per-step H2D traffic is ONE small asynchronous copy from
pinned memory (the two length vectors; the block table travels only on the steps that change it) instead of
one blocking copy per request, and no Timers (their cuda syncs, global_vars.py:132,140, would serialise the
decode loop) -- so the host can prepare step t + 1 while the GPU runs step t.  Device memory layout is unchanged,
so the HIP kernels see exactly the reference's cache.
"""

from collections import deque
from logging import getLogger

import torch

logger = getLogger(__name__)
_BLOCK_SIZE = 512
_MAX_SEQ_LEN = 2048
_STAGE_RING = 4
MAX_DECODE_Q = 8  # query tokens per request of a multi-token decode step (attn_backend.GQA_MULTI_MAX_Q)


MLA_KV_CACHE_DTYPES = ("bf16", "fp8")


def mla_kv_layout(kv_cache_dtype, kv_lora_rank=512, rope=64):
    """(kv_shape_per_sample, dtype) of one cached MLA token, for PagedKVCacheManager(kv_shape_per_sample=..., dtype=...).
    "bf16": [kv_norm(kv_c) | rope(k_pe)] as bf16.  "fp8": byte rows -- kv_lora_rank e4m3 codes, one fp32 power-of-two scale
    per 128 latent channels, the rope part as bf16 (csrc/mla_kv_fp8.hip): 656 bytes for the 512 + 64 row, 0.569 of bf16's."""
    if kv_cache_dtype == "bf16":
        return (kv_lora_rank + rope,), torch.bfloat16
    if kv_cache_dtype == "fp8":
        assert kv_lora_rank % 128 == 0
        return (kv_lora_rank + 4 * (kv_lora_rank // 128) + 2 * rope,), torch.uint8
    raise ValueError(f"kv_cache_dtype must be one of {MLA_KV_CACHE_DTYPES}, got {kv_cache_dtype!r}")


GQA_KV_CACHE_DTYPES = ("bf16", "fp8")


def gqa_kv_layout(kv_cache_dtype, n_local_kv_heads, head_dim=128):
    """(shape_per_sample, dtype) of one cached GQA / MHA token, for PagedKVCacheManager(k_shape_per_sample=...,
    v_shape_per_sample=..., dtype=...) -- the same for K and for V.  "bf16": [Hkv, head_dim] bf16.  "fp8": byte rows [Hkv, 144] --
    128 e4m3 codes, one fp32 power-of-two scale per (token, head), 12 zero bytes (csrc/gqa_kv_fp8.hip): 0.5625 of bf16's."""
    if kv_cache_dtype == "bf16":
        return (n_local_kv_heads, head_dim), torch.bfloat16
    if kv_cache_dtype == "fp8":
        assert head_dim == 128, "the fp8 K / V cache rows are defined for head_dim 128"
        return (n_local_kv_heads, 144), torch.uint8
    raise ValueError(f"kv_cache_dtype must be one of {GQA_KV_CACHE_DTYPES}, got {kv_cache_dtype!r}")


class PagedKVCacheManager:
    def __init__(
        self,
        begin_layer_id,
        end_layer_id,
        num_hot_req=16,
        block_size=_BLOCK_SIZE,
        max_seq_len=_MAX_SEQ_LEN,
        device="cuda",
        *,
        k_shape_per_sample=None,
        v_shape_per_sample=None,
        kv_shape_per_sample=None,
        n_local_kv_heads=None,
        head_dim=None,
        dtype=None,
    ):
        self.max_blocks_per_req = max_seq_len // block_size + 1
        self.num_blocks = self.max_blocks_per_req * num_hot_req
        self.begin_layer_id = begin_layer_id
        self.end_layer_id = end_layer_id
        self.num_layers = end_layer_id - begin_layer_id
        self.k_shape_per_sample = (
            k_shape_per_sample if k_shape_per_sample is not None else (n_local_kv_heads, head_dim)
        )
        self.v_shape_per_sample = (
            v_shape_per_sample if v_shape_per_sample is not None else (n_local_kv_heads, head_dim)
        )
        self.kv_shape_per_sample = kv_shape_per_sample
        self.block_size = block_size
        self.max_seq_len = max_seq_len
        self.device = torch.device(device)
        self.gpu_block_table = None
        dtype = dtype or torch.get_default_dtype()

        self.seq_lens = {}
        self.block_table = {}  # req_id -> [block ids]
        self.curr_seq_lens = []
        # excl / incl live in one device allocation so that one copy refreshes both (same names and shapes as the reference's)
        self._lens_dev = torch.zeros(2, num_hot_req, dtype=torch.int32, device=self.device)
        self.curr_seq_lens_gpu_excl_this_decode = self._lens_dev[0]
        self.curr_seq_lens_gpu_incl_this_decode = self._lens_dev[1]
        self.gpu_block_table_buffer = torch.zeros(
            (num_hot_req, self.max_blocks_per_req), dtype=torch.int32, device=self.device
        )
        # Host staging: a small RING of pinned buffers + copy_(non_blocking=True).  A pageable copy_() returns only after
        # the runtime has staged the bytes, which waits for the stream -- the host then never runs ahead of the GPU.
        # From pinned memory the copy is just enqueued; a slot is rewritten _STAGE_RING steps later, after the event
        # recorded behind its copy has completed (it has, long since, unless the host is that far ahead).
        self._pinned = self.device.type == "cuda"
        self._host_lens = torch.zeros(_STAGE_RING, 2, num_hot_req, dtype=torch.int32, pin_memory=self._pinned)
        self._host_table = torch.zeros((_STAGE_RING, num_hot_req, self.max_blocks_per_req), dtype=torch.int32,
                                       pin_memory=self._pinned)
        self._lens_np, self._table_np = self._host_lens.numpy(), self._host_table.numpy()
        self._stage_events = {"lens": [None] * _STAGE_RING, "table": [None] * _STAGE_RING}
        self._stage_next = {"lens": 0, "table": 0}
        self._table_rows = None  # request ids whose rows the device table currently holds, in order (None = stale)
        self._multi_dev = self._multi_table_dev = None  # the multi-token step's buffers (_multi_buffers)
        self._multi_shape = (0, 1)
        self.free_blocks = deque(range(self.num_blocks))
        if self.kv_shape_per_sample is not None:
            self.paged_kv_cache = torch.zeros(
                (self.num_layers, self.num_blocks, block_size) + tuple(self.kv_shape_per_sample),
                device=device, dtype=dtype,
            )
        else:
            self.paged_k_cache = torch.zeros(
                (self.num_layers, self.num_blocks, block_size) + tuple(self.k_shape_per_sample),
                device=device, dtype=dtype,
            )
            self.paged_v_cache = torch.zeros(
                (self.num_layers, self.num_blocks, block_size) + tuple(self.v_shape_per_sample),
                device=device, dtype=dtype,
            )

    def get_block_size(self):
        return self.block_size

    # ---- prefill: write whole pages (chitu/cache_manager.py:93-142)
    def finalize_cache_bylayer_prefill(self, xk, xv, req_ids, varlen, layer_id):
        """Write the prompt tokens' rows of one layer into their pages (cache_manager.py:93-142).  The pages are taken and
        the destination row of every token is worked out once, at the first layer; each layer is then ONE scatter
        (index_copy_) per cache instead of a slice copy per page."""
        if layer_id == self.begin_layer_id:
            rows = []
            for idx, req_id in enumerate(req_ids):
                n_prepared = (varlen.cpu_lens[idx] + self.block_size - 1) // self.block_size
                self.seq_lens[req_id] = varlen.cpu_lens[idx]
                self.block_table[req_id] = [self.get_free_block() for _ in range(n_prepared)]
                self._table_rows = None
                n_tok = varlen.cpu_prefix_lens[idx + 1] - varlen.cpu_prefix_lens[idx]
                t = torch.arange(n_tok, dtype=torch.int64)
                blocks = torch.tensor(self.block_table[req_id], dtype=torch.int64)
                rows.append(blocks[t // self.block_size] * self.block_size + t % self.block_size)
            dev = (self.paged_kv_cache if self.kv_shape_per_sample is not None else self.paged_k_cache).device
            self._prefill_rows = (torch.cat(rows) if rows else torch.zeros(0, dtype=torch.int64)).to(dev)
        li = layer_id - self.begin_layer_id
        rows = self._prefill_rows
        if self.kv_shape_per_sample is not None:
            c = self.paged_kv_cache[li]
            c.view(-1, *c.shape[2:]).index_copy_(0, rows, xk[: rows.numel()].to(c.dtype))
        else:
            ck, cv = self.paged_k_cache[li], self.paged_v_cache[li]
            ck.view(-1, *ck.shape[2:]).index_copy_(0, rows, xk[: rows.numel()].to(ck.dtype))
            cv.view(-1, *cv.shape[2:]).index_copy_(0, rows, xv[: rows.numel()].to(cv.dtype))

    def register_sequence(self, req_id, length):
        """Allocate pages for a sequence of `length` cached tokens without writing data
        (synthetic benchmarks / tests; prefill normally does this)."""
        self.seq_lens[req_id] = length
        n = (length + self.block_size - 1) // self.block_size
        self.block_table[req_id] = [self.get_free_block() for _ in range(n)]
        self._table_rows = None

    def finalize_cache_all_prefill(self, req_ids, varlen):
        self.curr_varlens = None
        self.curr_req_ids = None

    def _stage_slot(self, kind):
        """Next pinned slot of a ring; waits for the copy that last read it (a no-op unless the host is a ring ahead)."""
        slot = self._stage_next[kind]
        self._stage_next[kind] = (slot + 1) % _STAGE_RING
        ev = self._stage_events[kind][slot]
        if ev is not None:
            ev.synchronize()
        return slot

    def _stage_done(self, kind, slot):
        if self._pinned:
            ev = torch.cuda.Event()
            ev.record()
            self._stage_events[kind][slot] = ev

    def prepare_cache_decode(self, req_ids):
        n = len(req_ids)
        seq_lens = [self.seq_lens[r] for r in req_ids]
        self.curr_seq_lens = seq_lens
        slot = self._stage_slot("lens")
        h = self._lens_np[slot]
        h[0, :n] = seq_lens
        h[1, :n] = h[0, :n] + 1
        # the live columns of both vectors: TWO contiguous row copies from the pinned slot (a strided [2, n] slice of a
        # [2, max] buffer is not one async memcpy for torch: it goes through a pageable temporary and a device copy kernel).
        # The tail keeps its old values: a ring slot's tail holds whatever step last used that slot.
        self._lens_dev[0, :n].copy_(self._host_lens[slot][0, :n], non_blocking=True)
        self._lens_dev[1, :n].copy_(self._host_lens[slot][1, :n], non_blocking=True)
        self._stage_done("lens", slot)

    def get_free_block(self):
        if not self.free_blocks:
            raise Exception("No more free blocks.")  # same behaviour as cache_manager.py:163-164
        return self.free_blocks.popleft()

    def get_gpu_block_table(self):
        return self.gpu_block_table

    def get_gpu_seq_lens_excl_this_decode(self):
        return self.curr_seq_lens_gpu_excl_this_decode[: len(self.curr_seq_lens)]

    def get_gpu_seq_lens_incl_this_decode(self):
        return self.curr_seq_lens_gpu_incl_this_decode[: len(self.curr_seq_lens)]

    def get_paged_kv_cache(self, layer_id):
        if self.kv_shape_per_sample is not None:
            return self.paged_kv_cache[layer_id - self.begin_layer_id]
        return (
            self.paged_k_cache[layer_id - self.begin_layer_id],
            self.paged_v_cache[layer_id - self.begin_layer_id],
        )

    def free_req_cache_blocks(self, req_id):
        for block in self.block_table[req_id]:
            self.free_blocks.append(block)
        del self.block_table[req_id]
        self._table_rows = None

    def prepare_block_table_for_decode(self, req_ids):
        """Make room for the token this decode step appends, then refresh the device table
        (chitu/cache_manager.py:196-209).  Page allocation stays on the host, outside the graph.  The table is copied
        only on the steps that change it (a request crossed a page boundary, or the batch's rows changed): in a
        steady decode that is one step in `block_size`."""
        n = len(req_ids)
        changed = self._table_rows is None or self._table_rows != list(req_ids)
        for req_id in req_ids:
            if self.seq_lens[req_id] % self.block_size == 0:
                self.block_table[req_id].append(self.get_free_block())
                changed = True
        if changed:
            slot = self._stage_slot("table")
            h = self._table_np[slot]
            h[:n] = 0
            for idx, req_id in enumerate(req_ids):
                ids = self.block_table[req_id]
                h[idx, : len(ids)] = ids
            self.gpu_block_table_buffer[:n].copy_(self._host_table[slot, :n], non_blocking=True)
            self._stage_done("table", slot)
            self._table_rows = list(req_ids)
        self.gpu_block_table = self.gpu_block_table_buffer[:n]

    # ---- multi-token decode steps (a speculative verify step: T query tokens per sequence, attn_with_kvcache's seqlen > 1)
    def _multi_buffers(self):
        """Persistent buffers of the multi-token step, made at its first use: a captured step replays on their addresses.
        Sized for MAX_DECODE_Q tokens per request, so one allocation serves every T."""
        if self._multi_dev is None:
            n, rows = self._lens_dev.shape[1], self._lens_dev.shape[1] * MAX_DECODE_Q
            # [row lengths (rows) | lengths incl. the T new tokens (n) | row lengths incl. the row itself (rows)] in one
            # allocation: one copy refreshes all three
            self._multi_dev = torch.zeros(2 * rows + n, dtype=torch.int32, device=self.device)
            self._multi_table_dev = torch.zeros((rows, self.max_blocks_per_req), dtype=torch.int32, device=self.device)
            self._multi_host = torch.zeros(_STAGE_RING, 2 * rows + n, dtype=torch.int32, pin_memory=self._pinned)
            self._multi_host_table = torch.zeros((_STAGE_RING, rows, self.max_blocks_per_req), dtype=torch.int32,
                                                 pin_memory=self._pinned)
            self._stage_events.update(multi=[None] * _STAGE_RING, multi_table=[None] * _STAGE_RING)
            self._stage_next.update(multi=0, multi_table=0)
        return self._multi_dev

    def prepare_block_table_for_decode_multi(self, req_ids, T):
        """Make room for the T tokens this step appends to every request and stage what the step reads, in persistent
        buffers of its own (the single-token step's buffers are not touched):
          get_gpu_multi_row_lens()      [n * T] the old length + t of expanded row (b, t): its RoPE and append position
          get_gpu_multi_seq_lens_incl() [n]     the old length + T: the keys the attention sees
          get_gpu_multi_row_lens_incl() [n * T] the old length + t + 1: the keys expanded row (b, t) sees, for an attention that
                                        takes the step as n * T single-token rows
          get_gpu_multi_block_table()   [n * T, max_blocks] request b's table in each of its T rows (the append kernels take one
                                        table row per appended row; the attention reads every T-th row)
        Pages beyond ceil(len / block_size) that a step takes and finalize_cache_multi_decode does not keep go back to the
        free list there."""
        assert 1 <= T <= MAX_DECODE_Q
        n = len(req_ids)
        assert n * MAX_DECODE_Q <= self._multi_buffers().numel()
        for req_id in req_ids:  # every request's capacity first: a refused step has taken no page
            if self.seq_lens[req_id] + T > self.max_blocks_per_req * self.block_size:
                raise Exception(f"request {req_id!r}: {self.seq_lens[req_id]} + {T} tokens do not fit its block table")
        for req_id in req_ids:
            while len(self.block_table[req_id]) * self.block_size < self.seq_lens[req_id] + T:
                self.block_table[req_id].append(self.get_free_block())
                self._table_rows = None  # the single-token step's device table no longer shows this request's pages
        lens = [self.seq_lens[r] for r in req_ids]
        slot = self._stage_slot("multi")
        h = self._multi_host[slot].numpy()
        rows = n * T
        for b, L0 in enumerate(lens):
            h[b * T : (b + 1) * T] = range(L0, L0 + T)
        h[rows : rows + n] = [L0 + T for L0 in lens]
        h[rows + n : 2 * rows + n] = h[:rows] + 1
        self._multi_dev[: 2 * rows + n].copy_(self._multi_host[slot][: 2 * rows + n], non_blocking=True)
        self._stage_done("multi", slot)
        slot = self._stage_slot("multi_table")
        ht = self._multi_host_table[slot].numpy()
        ht[:rows] = 0
        for b, req_id in enumerate(req_ids):
            ids = self.block_table[req_id]
            ht[b * T : (b + 1) * T, : len(ids)] = ids
        self._multi_table_dev[:rows].copy_(self._multi_host_table[slot, :rows], non_blocking=True)
        self._stage_done("multi_table", slot)
        self._multi_shape = (n, T)

    def get_gpu_multi_row_lens(self):
        n, T = self._multi_shape
        return self._multi_dev[: n * T]

    def get_gpu_multi_seq_lens_incl(self):
        n, T = self._multi_shape
        return self._multi_dev[n * T : n * T + n]

    def get_gpu_multi_row_lens_incl(self):
        n, T = self._multi_shape
        return self._multi_dev[n * T + n : 2 * n * T + n]

    def get_gpu_multi_block_table(self):
        n, T = self._multi_shape
        return self._multi_table_dev[: n * T]

    def finalize_cache_multi_decode(self, req_ids, n_accepted):
        """After a multi-token step of T tokens: request b keeps the first n_accepted[b] of them (1 <= n_accepted[b] <= T).  Its
        length advances by that, and the pages beyond ceil(length / block_size) go back to the free list -- the single-token
        methods' invariant.  The rejected rows stay behind the length as garbage: no kernel uses bytes past a length."""
        n, T = self._multi_shape
        assert len(req_ids) == n and len(n_accepted) == n
        for req_id, acc in zip(req_ids, n_accepted):
            acc = int(acc)
            assert 1 <= acc <= T, f"request {req_id!r}: {acc} accepted tokens of a step of {T}"
            self.seq_lens[req_id] += acc
            keep = (self.seq_lens[req_id] + self.block_size - 1) // self.block_size
            while len(self.block_table[req_id]) > keep:
                self.free_blocks.append(self.block_table[req_id].pop())
                self._table_rows = None
        self.curr_varlens = None
        self.curr_req_ids = None

    def rollback(self, req_ids, n_drop):
        """Give rows back: request b's length shrinks by n_drop[b] >= 0 and the pages beyond ceil(length / block_size) return to
        the free list (finalize_cache_multi_decode's invariant; `_table_rows` goes stale when a page left).  The rows are only
        forgotten -- they stay behind the length as garbage, and no kernel uses bytes past a length -- so dropping more rows than
        were decoded since prefill is allowed; dropping below 0 raises before anything changes.  A draft model's cache uses this
        to return to what the target accepted (sampling.ModelDrafter.settle)."""
        assert len(req_ids) == len(n_drop)
        drops = [int(d) for d in n_drop]
        for req_id, d in zip(req_ids, drops):
            if d < 0 or d > self.seq_lens[req_id]:
                raise ValueError(f"request {req_id!r}: cannot drop {d} of {self.seq_lens[req_id]} cached rows")
        for req_id, d in zip(req_ids, drops):
            self.seq_lens[req_id] -= d
            keep = (self.seq_lens[req_id] + self.block_size - 1) // self.block_size
            while len(self.block_table[req_id]) > keep:
                self.free_blocks.append(self.block_table[req_id].pop())
                self._table_rows = None

    # ---- continued / chunked prefill: n new tokens per request behind rows that are already cached
    def prepare_cache_prefill_continue(self, req_ids, varlen):
        """Make room for the varlen.cpu_lens[b] tokens a continued prefill appends to request b (already cached, any length) and
        stage what the step reads:
          get_continue_position_ids()        [T] int64  absolute position of every new token: its RoPE row
          get_gpu_continue_seq_lens_incl()   [n] int32  the old length + the new tokens: the keys the attention sees
          get_gpu_continue_block_table()     [n, max_blocks] int32
        and, for finalize_cache_bylayer_prefill_continue, the flat page row of every new token.  Every request's capacity and
        the free pages are checked before a page is taken from any (prepare_block_table_for_decode_multi's rule); each block
        table then grows to ceil((len + n) / block_size) pages -- finalize_cache_all_prefill_continue advances the lengths, so
        the single-token step's invariant holds again."""
        req_ids = list(req_ids)
        counts = [int(c) for c in varlen.cpu_lens]
        assert len(counts) == len(req_ids) and len(set(req_ids)) == len(req_ids)
        need = 0
        for req_id, c in zip(req_ids, counts):
            if req_id not in self.seq_lens:
                raise KeyError(f"request {req_id!r} is not cached: a continued prefill extends a sequence that prefill registered")
            assert c >= 1, f"request {req_id!r}: a continued prefill needs at least one new token"
            if self.seq_lens[req_id] + c > self.max_blocks_per_req * self.block_size:
                raise Exception(f"request {req_id!r}: {self.seq_lens[req_id]} + {c} tokens do not fit its block table")
            need += -(-(self.seq_lens[req_id] + c) // self.block_size) - len(self.block_table[req_id])
        if need > len(self.free_blocks):
            raise Exception(f"{need} more pages for {sum(counts)} tokens do not fit the {len(self.free_blocks)} free pages")
        rows, pos = [], []
        for req_id, c in zip(req_ids, counts):
            L0 = self.seq_lens[req_id]
            while len(self.block_table[req_id]) * self.block_size < L0 + c:
                self.block_table[req_id].append(self.get_free_block())
                self._table_rows = None  # the single-token step's device table no longer shows this request's pages
            t = torch.arange(L0, L0 + c, dtype=torch.int64)
            blocks = torch.tensor(self.block_table[req_id], dtype=torch.int64)
            rows.append(blocks[t // self.block_size] * self.block_size + t % self.block_size)
            pos.append(t)
        table = torch.zeros(len(req_ids), self.max_blocks_per_req, dtype=torch.int32)
        for b, req_id in enumerate(req_ids):
            table[b, : len(self.block_table[req_id])] = torch.tensor(self.block_table[req_id], dtype=torch.int32)
        lens = torch.tensor([self.seq_lens[r] + c for r, c in zip(req_ids, counts)], dtype=torch.int32)
        dev = self.device
        self._continue = dict(req_ids=req_ids, counts=counts, rows=torch.cat(rows).to(dev), positions=torch.cat(pos).to(dev),
                              table=table.to(dev), lens=lens.to(dev))

    def get_continue_position_ids(self):
        return self._continue["positions"]

    def get_gpu_continue_seq_lens_incl(self):
        return self._continue["lens"]

    def get_gpu_continue_block_table(self):
        return self._continue["table"]

    def finalize_cache_bylayer_prefill_continue(self, xk, xv, layer_id):
        """Write the new tokens' rows of one layer into their pages: one scatter (index_copy_) per cache, as
        finalize_cache_bylayer_prefill."""
        li = layer_id - self.begin_layer_id
        rows = self._continue["rows"]
        if self.kv_shape_per_sample is not None:
            c = self.paged_kv_cache[li]
            c.view(-1, *c.shape[2:]).index_copy_(0, rows, xk[: rows.numel()].to(c.dtype))
        else:
            ck, cv = self.paged_k_cache[li], self.paged_v_cache[li]
            ck.view(-1, *ck.shape[2:]).index_copy_(0, rows, xk[: rows.numel()].to(ck.dtype))
            cv.view(-1, *cv.shape[2:]).index_copy_(0, rows, xv[: rows.numel()].to(cv.dtype))

    def finalize_cache_all_prefill_continue(self, req_ids):
        """The continued prefill has run: the requests' lengths advance by their new tokens."""
        c = self._continue
        assert list(req_ids) == c["req_ids"]
        for req_id, n in zip(c["req_ids"], c["counts"]):
            self.seq_lens[req_id] += n
        self._continue = None
        self.curr_varlens = None
        self.curr_req_ids = None

    def finalize_cache_single_decode(self, req_ids):
        for req_id in req_ids:
            self.seq_lens[req_id] = self.seq_lens[req_id] + 1
        self.curr_varlens = None
        self.curr_req_ids = None

    def finalize_cache_all_decode(self, req_id):
        assert req_id in self.seq_lens
        assert req_id in self.block_table
        del self.seq_lens[req_id]
        self.free_req_cache_blocks(req_id)
        self.curr_varlens = None
        self.curr_req_ids = None
