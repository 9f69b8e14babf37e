"""Attention backend for gfx950 behind the reference's `AttnBackend` interface.

Reference (read-only): chitu/attn_backend.py -- interface AttnBackend:24-164,
TritonAttnBackend:687-774 (the MLA decode path the reference runs on non-NVIDIA devices),
FlashMLABackend:504-572 / FlashInferBackend:575-684 (graph-capturable third-party paths).
`HipAttnBackend` implements `prepare_metadata_for_decode`, `mla_attn_with_kvcache`,
`attn_with_kvcache(block_table=...)` and the MLA-prefill form of `attn_varlen_func` with hand-written HIP kernels; the host side only sizes
the KV split count from the batch (graph-static) and keeps a persistent scratch buffer.
"""

import os
from typing import Optional, Union

import torch

from . import _lib, workspace
from ._lib import check, f32, i32, i64, ptr, require_cuda, stream_ptr
from .ops import GQA_KV_FP8_ROW, MLA_KV_FP8_ROW, append_gqa_kv_fp8, append_mla_kv_fp8, append_to_paged_kv_cache

__all__ = ["AttnBackend", "HipAttnBackend"]


def is_fp8_mla_cache(kv_cache) -> bool:
    """A layer of the fp8 latent KV cache (uint8 [pages, page, 656], cache_manager.mla_kv_layout("fp8"))?"""
    return kv_cache.dtype == torch.uint8 and kv_cache.shape[-1] == MLA_KV_FP8_ROW


def is_fp8_gqa_cache(cache) -> bool:
    """A layer of the fp8 K or V cache (uint8 [pages, page, Hkv, 144], cache_manager.gqa_kv_layout("fp8"))?"""
    return cache.dtype == torch.uint8 and cache.dim() == 4 and cache.shape[-1] == GQA_KV_FP8_ROW


MLA_MULTI_MAX_Q = 8  # query tokens per sequence of chitu_hip_mla_decode_multi (csrc/mla_decode_tile.h: kMlaMultiMaxQ)
GQA_MULTI_MAX_Q = 8  # query tokens per sequence of chitu_hip_gqa_decode_multi (csrc/gqa_decode_multi.hip: kGqaMultiMaxQ)
# Upper bound of the KV splits of the GQA decode launch (graph-static: sized from the page table's width, not from the
# lengths).  32 by the sweep of round 4 (Llama-3-8B bs 1, ctx 1024: 64 -> 3.064, 32 -> 3.041, 16 -> 3.077, 8 -> 3.175 ms/step;
# from bs 4 on the CU-count term decides; profiles/r04_gqa_split_sweep.txt); CHITU_GQA_MAX_SPLITS overrides it for sweeps.
_GQA_MAX_SPLITS = int(os.environ.get("CHITU_GQA_MAX_SPLITS", "32"))
# single-wave workgroups per CU the split count aims for once batch * kv_heads decides (sweeps: CHITU_GQA_WAVES_PER_CU)
_GQA_WAVES_PER_CU = int(os.environ.get("CHITU_GQA_WAVES_PER_CU", "4"))


class AttnBackend:
    """Interface (chitu/attn_backend.py:24-164)."""

    def prepare_metadata_for_decode(self, *args, **kwargs):
        pass

    def attn_varlen_func(self, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0,
                         causal=False, window_size=(-1, -1), softcap=0.0, softmax_scale=None):
        raise NotImplementedError()

    def attn_with_kvcache(self, q, k_cache, v_cache, k=None, v=None, cache_seqlens=None, cache_leftpad=None,
                          block_table=None, causal=False, window_size=(-1, -1), softcap=0.0, softmax_scale=None):
        raise NotImplementedError()

    def mla_attn_with_kvcache(self, *args, **kwargs):
        raise NotImplementedError()


def _num_cus():
    try:
        return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    except Exception:
        return 256


def gqa_num_splits(batch: int, kv_heads: int, max_pages: int, page_size: int, window_left: int = -1) -> int:
    """KV splits attn_with_kvcache gives the GQA decode launch when the caller names none: graph-static (the page table's
    width, not the lengths), never more than 16-token steps, the cap above, and _GQA_WAVES_PER_CU workgroups per CU.
    window_left >= 0: a sequence walks at most the steps that overlap W + 1 keys ((W + 16) // 16 + 1 of them), so a short
    window is not cut into splits that have nothing to do."""
    max_steps = max(1, max_pages * page_size // 16)
    if window_left >= 0:
        max_steps = min(max_pages * page_size, window_left + 16) // 16 + 1
    return max(1, min(max_steps, _GQA_MAX_SPLITS, (_GQA_WAVES_PER_CU * _num_cus()) // max(1, batch * kv_heads)))


def choose_num_splits(batch: int, head_blocks: int, max_tiles: int, target_wgs: Optional[int] = None) -> int:
    """KV splits so that batch*head_blocks*splits workgroups fill the chip once (the decode kernel
    runs one 96 KB-LDS workgroup per CU), never more splits than 64-token tiles.  Depends only on
    graph-static quantities (batch, max context)."""
    import os

    if os.environ.get("CHITU_MLA_SPLITS"):
        return max(1, min(max_tiles, int(os.environ["CHITU_MLA_SPLITS"])))  # tuning knob
    if target_wgs is None:
        target_wgs = _num_cus()
    per = max(1, batch * head_blocks)
    s = max(1, min(max_tiles, (target_wgs + per - 1) // per))
    return min(s, 64)


# The multi-token MLA launch against the composition it replaces (chitu_hip_mla_decode on bs * T expanded rows), measured
# (profiles/mla_multi_sweep.json): the pair kernel reads the pages half as often but runs its two tile steps one
# after the other, so it wins only once the composition's workgroups more than fill the chip -- at bs * T * head_blocks *
# max_tiles = 4128 and 8256 tile steps it takes 0.76 - 0.89 of the composition's time, at 1088 the two tie, at 544 and below it
# is 1.08 - 1.5 x slower.  The crossover, in tile steps per CU of the composition (1088 / 256 CUs):
MLA_MULTI_MIN_TILE_STEPS_PER_CU = 4.25


def mla_multi_beats_composition(batch: int, q_len: int, heads: int, max_tiles: int) -> bool:
    """Graph-static routing rule of HipAttnBackend.mla_decode_multi (batch, T and the table's width: no lengths)."""
    return batch * q_len * ((heads + 15) // 16) * max_tiles >= MLA_MULTI_MIN_TILE_STEPS_PER_CU * _num_cus()


def window_and_cap(window_size, softcap, causal: bool):
    """(window_left, softcap) of the reference's window_size / softcap arguments (attn_backend.py:55-69) in the forms the GQA
    kernels implement: a left window W >= 0 (-1: none) whose effective right side is 0 -- given as 0, or implied by causal=True,
    which makes the reference set it to 0 (RefAttnBackend._attention, :333-334) -- and softcap >= 0.  (-1, -1) is no window.
    Anything else raises."""
    left, right = (int(w) for w in window_size)
    softcap = float(softcap)
    if not softcap >= 0.0:
        raise ValueError(f"softcap={softcap}: must be >= 0 (0.0 = off)")
    if left < -1 or right < -1:
        raise ValueError(f"window_size={window_size}: -1 means unlimited, anything below is not a window")
    if causal:
        right = 0
    if (left, right) == (-1, -1):
        return -1, softcap
    if right != 0:
        raise NotImplementedError(f"window_size={tuple(window_size)} with causal={causal}: only a left window (right side 0, given or "
                                  "implied by causal=True) is implemented")
    return left, softcap


_tickets = {}


def _fuse_tickets(device) -> torch.Tensor:
    """The arrival / departure words of chitu_hip_mla_decode_merge_uv_quant_fp8 (+ its sticky error word, the last one): zero
    at creation, left zero by every launch.  One buffer per (device, workspace namespace) for the life of the process --
    launches that share it must not overlap, and captured launches keep a valid address; created on the first EAGER call
    (decode() warms up eagerly before it captures)."""
    key = (torch.device(device).index or 0, workspace._namespace)
    t = _tickets.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mla_decode_merge_uv_quant must run once eagerly before graph capture")
        import ctypes

        n = ctypes.c_int64(0)
        check(_lib.lib().chitu_hip_mla_decode_tickets_bytes(ctypes.byref(n)), "mla_decode_tickets_bytes")
        t = _tickets[key] = torch.zeros(n.value // 4, dtype=torch.int32, device=device)
    return t


def fused_tail_timed_out(device) -> bool:
    """Did any fused MLA decode launch on this device give up waiting for a split (its 200 ms bound)?  Synchronises."""
    return any(int(t[-1].item()) != 0 for (dev, _), t in _tickets.items() if dev == (torch.device(device).index or 0))


class HipAttnBackend(AttnBackend):
    """MLA absorb-mode paged decode (+ GQA paged decode) on hand-written HIP kernels.

    Construction mirrors TritonAttnBackend (attn_backend.py:688-696) but takes the model
    dimensions explicitly instead of reading hydra globals.
    """

    def __init__(self, local_n_heads: int = 16, kv_lora_rank: int = 512, qk_rope_head_dim: int = 64,
                 qk_nope_head_dim: int = 128, max_seq_len: int = 4096):
        self.local_n_heads = local_n_heads
        self.kv_lora_rank = kv_lora_rank
        self.qk_rope_head_dim = qk_rope_head_dim
        self.qk_nope_head_dim = qk_nope_head_dim
        self.max_seq_len = max_seq_len
        self.block_size = None
        self.num_splits = None

    def prepare_metadata_for_decode(
        self,
        cache_seqlens_excl_this_decode,
        cache_seqlens_incl_this_decode,
        block_table,
        block_size,
        softmax_scale=None,
    ):
        """Runs OUTSIDE the captured graph (model.py:540 -> model_deepseek_v3.py:1339).  Unlike
        FlashInfer's prepare (attn_backend.py:620-637: Python loops with .item() syncs) this does
        no device work: the split count depends only on the batch size and the table width."""
        self.block_size = block_size
        bs = int(cache_seqlens_incl_this_decode.shape[0])
        max_tiles = max(1, (int(block_table.shape[1]) * int(block_size) + 63) // 64)
        self.num_splits = choose_num_splits(bs, (self.local_n_heads + 15) // 16, max_tiles)

    def mla_decode(self, q_nope, q_pe, kv_cache, cache_seqlens_incl, block_table, softmax_scale,
                   num_splits: Optional[int] = None, out: Optional[torch.Tensor] = None,
                   return_partials: bool = False):
        """softmax(scale * (q_nope.c + q_pe.k_pe)) . c over the paged latent cache; no append.

        return_partials=True (fused consumer, ops.mla_merge_absorb_uv_quant_fp8): when the KV range is
        split, skip the merge pass and return (workspace, num_splits) instead of the output; with a
        single split the output tensor is returned as usual.

        kv_cache uint8 [pages, page, 656] (the fp8 latent cache): chitu_hip_mla_decode_kv_fp8, same arguments, same
        workspace; the result is bit-identical to this call on ops.mla_kv_dequant_fp8(kv_cache)."""
        require_cuda(q_nope, q_pe, kv_cache, cache_seqlens_incl, block_table)
        assert kv_cache.ndim == 3 and kv_cache.is_contiguous()  # (num_blocks, block_size, dim)
        fp8_kv = is_fp8_mla_cache(kv_cache)
        assert (kv_cache.dtype == torch.bfloat16 or fp8_kv) and q_nope.dtype == torch.bfloat16 and q_pe.dtype == torch.bfloat16
        assert block_table.dtype == torch.int32 and cache_seqlens_incl.dtype == torch.int32
        assert block_table.stride(1) == 1 and cache_seqlens_incl.is_contiguous()
        B, H, C = q_nope.shape
        R = q_pe.shape[-1]
        assert fp8_kv or kv_cache.shape[-1] == C + R

        def ok(t):
            return t.stride(-1) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0

        if not ok(q_nope):
            q_nope = q_nope.contiguous()
        if not ok(q_pe):
            q_pe = q_pe.contiguous()
        if num_splits is None:
            max_tiles = max(1, (int(block_table.shape[1]) * int(kv_cache.shape[1]) + 63) // 64)
            num_splits = self.num_splits or choose_num_splits(B, (H + 15) // 16, max_tiles)
        partials = return_partials and num_splits > 1
        if out is None and not partials:
            out = torch.empty(B, H, C, dtype=torch.bfloat16, device=q_nope.device)
        need = B * H * num_splits * (C * 2 + 4) if num_splits > 1 else 0  # bf16 partial rows + fp32 LSE
        ws = workspace.get(max(need, 1), q_nope.device, "mla")
        entry = _lib.lib().chitu_hip_mla_decode_kv_fp8 if fp8_kv else _lib.lib().chitu_hip_mla_decode
        check(
            entry(
                ptr(q_nope), i64(q_nope.stride(0)), i64(q_nope.stride(1)), ptr(q_pe), i64(q_pe.stride(0)),
                i64(q_pe.stride(1)), ptr(kv_cache), i64(kv_cache.shape[0]), i32(kv_cache.shape[1]),
                ptr(block_table), i32(block_table.stride(0)), ptr(cache_seqlens_incl), f32(softmax_scale),
                ptr(None if partials else out), i32(B), i32(H), i32(C), i32(R), i32(num_splits), ptr(ws),
                i64(ws.numel()), stream_ptr(),
            ),
            "mla_decode_kv_fp8" if fp8_kv else "mla_decode",
        )
        return (ws, num_splits) if partials else out

    def mla_decode_multi(self, q_nope, q_pe, kv_cache, cache_seqlens_incl, block_table, softmax_scale,
                         num_splits: Optional[int] = None, out: Optional[torch.Tensor] = None,
                         return_partials: bool = False, kernel: Optional[str] = None, expanded=None):
        """mla_decode for T = q_nope.shape[1] <= 8 query tokens per sequence (chitu_hip_mla_decode_multi / _kv_fp8 by cache dtype,
        the kTok = 2 kernels of csrc/mla_decode.hip / mla_decode_kv_fp8.hip): q_nope [bs, T, H, 512], q_pe [bs, T, H, 64]; cache_seqlens_incl [bs] counts all keys, the T
        rows appended this step included; block_table [bs, stride], one row per sequence.  Query (b, t) sees the first
        L - T + t + 1 keys.  Returns [bs, T, H, 512], or with return_partials and more than one split (workspace, num_splits)
        with bs * T rows in (b, t) order: ops.mla_merge_absorb_uv_quant_fp8 consumes it with batch = bs * T.  One workgroup
        takes two query tokens, so the splits are sized for head_blocks * ceil(T / 2) workgroups per sequence (graph-static).

        kernel: "multi" = that launch; "composed" = the composition it replaces, mla_decode on the bs * T expanded rows (each
        table row T times, lengths L - T + t + 1: the same attention, row for row); None = by the measured rule
        mla_multi_beats_composition, T == 1 always the multi launch.  expanded = (table [bs * T, stride], lengths [bs * T]) of the
        expanded rows where the caller has them already (the cache manager's multi-token buffers); else they are built here."""
        require_cuda(q_nope, q_pe, kv_cache, cache_seqlens_incl, block_table)
        assert kv_cache.ndim == 3 and kv_cache.is_contiguous()
        fp8_kv = is_fp8_mla_cache(kv_cache)
        assert (kv_cache.dtype == torch.bfloat16 or fp8_kv) and q_nope.dtype == torch.bfloat16 and q_pe.dtype == torch.bfloat16
        assert block_table.dtype == torch.int32 and cache_seqlens_incl.dtype == torch.int32
        assert block_table.stride(1) == 1 and cache_seqlens_incl.is_contiguous()
        B, T, H, C = q_nope.shape
        R = q_pe.shape[-1]
        assert tuple(q_pe.shape[:3]) == (B, T, H) and (fp8_kv or kv_cache.shape[-1] == C + R)
        assert tuple(block_table.shape)[0] == B and cache_seqlens_incl.numel() == B
        if not 1 <= T <= MLA_MULTI_MAX_Q:
            raise ValueError(f"mla_decode_multi: {T} query tokens per sequence; 1 .. {MLA_MULTI_MAX_Q} are implemented")

        def ok(t):
            return t.stride(-1) == 1 and all(t.stride(d) % 8 == 0 for d in range(3)) and t.data_ptr() % 16 == 0

        if not ok(q_nope):
            q_nope = q_nope.contiguous()
        if not ok(q_pe):
            q_pe = q_pe.contiguous()
        max_tiles = max(1, (int(block_table.shape[1]) * int(kv_cache.shape[1]) + 63) // 64)
        if kernel is None:
            kernel = "multi" if T == 1 or mla_multi_beats_composition(B, T, H, max_tiles) else "composed"
        if kernel == "composed":
            if expanded is None:
                steps = torch.arange(1 - T, 1, dtype=torch.int32, device=q_nope.device)
                expanded = (block_table.repeat_interleave(T, dim=0), (cache_seqlens_incl.view(B, 1) + steps.view(1, T)).reshape(B * T))
            table_x, lens_x = expanded
            assert tuple(table_x.shape)[0] == B * T and lens_x.numel() == B * T
            if num_splits is None:
                num_splits = choose_num_splits(B * T, (H + 15) // 16, max_tiles)
            res = self.mla_decode(q_nope.reshape(B * T, H, C), q_pe.reshape(B * T, H, R), kv_cache, lens_x, table_x, softmax_scale,
                                  num_splits=num_splits, out=None if out is None else out.view(B * T, H, C), return_partials=return_partials)
            return res if isinstance(res, tuple) else res.view(B, T, H, C)
        assert kernel == "multi", kernel
        if num_splits is None:
            num_splits = choose_num_splits(B, ((H + 15) // 16) * ((T + 1) // 2), max_tiles)
        partials = return_partials and num_splits > 1
        if out is None and not partials:
            out = torch.empty(B, T, H, C, dtype=torch.bfloat16, device=q_nope.device)
        assert partials or (out.is_contiguous() and tuple(out.shape) == (B, T, H, C) and out.dtype == torch.bfloat16)
        need = B * T * H * num_splits * (C * 2 + 4) if num_splits > 1 else 0  # bf16 partial rows + fp32 LSE
        ws = workspace.get(max(need, 1), q_nope.device, "mla")
        name = "mla_decode_multi_kv_fp8" if fp8_kv else "mla_decode_multi"
        check(
            getattr(_lib.lib(), "chitu_hip_" + name)(
                ptr(q_nope), i64(q_nope.stride(0)), i64(q_nope.stride(1)), i64(q_nope.stride(2)), ptr(q_pe), i64(q_pe.stride(0)),
                i64(q_pe.stride(1)), i64(q_pe.stride(2)), ptr(kv_cache), i64(kv_cache.shape[0]), i32(kv_cache.shape[1]),
                ptr(block_table), i32(block_table.stride(0)), ptr(cache_seqlens_incl), f32(softmax_scale),
                ptr(None if partials else out), i32(B), i32(T), i32(H), i32(C), i32(R), i32(num_splits), ptr(ws),
                i64(ws.numel()), stream_ptr(),
            ),
            name,
        )
        return (ws, num_splits) if partials else out

    def mla_decode_merge_uv_quant(self, q_nope, q_pe, kv_cache, cache_seqlens_incl, block_table, softmax_scale, w_uv, scale,
                                  scale_offset, scale_stride_h, scale_stride_k, num_splits: Optional[int] = None,
                                  tile_major: bool = False):
        """mla_decode(return_partials=True) + ops.mla_merge_absorb_uv_quant_fp8 in ONE launch (round 6,
        chitu_hip_mla_decode_merge_uv_quant_fp8): every split workgroup waits for its sequence's other splits and finishes one
        head -- merge, o . W_UV^T (model_deepseek_v3.py:697), act_quant of wo's input.  Bit-identical to the two launches.
        Returns what the merge op returns, or None when the shape takes the two-launch form (one split, > 4096 groups, an
        fp8 latent cache -- the fused launch reads bf16 rows only)."""
        from . import ops

        require_cuda(q_nope, q_pe, kv_cache, cache_seqlens_incl, block_table, w_uv, scale)
        if is_fp8_mla_cache(kv_cache):
            return None
        assert kv_cache.ndim == 3 and kv_cache.is_contiguous() and kv_cache.dtype == torch.bfloat16
        assert q_nope.dtype == torch.bfloat16 and q_pe.dtype == torch.bfloat16
        assert block_table.dtype == torch.int32 and cache_seqlens_incl.dtype == torch.int32
        assert block_table.stride(1) == 1 and cache_seqlens_incl.is_contiguous()
        B, H, C = q_nope.shape
        R = q_pe.shape[-1]
        assert kv_cache.shape[-1] == C + R and C == 512
        assert w_uv.element_size() == 1 and scale.dtype == torch.float32 and w_uv.dim() == 3 and tuple(w_uv.shape) == (H, 128, C)
        assert w_uv.stride(2) == 1 and w_uv.stride(1) == C

        def ok(t):
            return t.stride(-1) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0

        if not ok(q_nope):
            q_nope = q_nope.contiguous()
        if not ok(q_pe):
            q_pe = q_pe.contiguous()
        if num_splits is None:
            max_tiles = max(1, (int(block_table.shape[1]) * int(kv_cache.shape[1]) + 63) // 64)
            num_splits = self.num_splits or choose_num_splits(B, (H + 15) // 16, max_tiles)
        if num_splits < 2 or B * ((H + 15) // 16) > 4096 or w_uv.data_ptr() % 16 != 0:
            return None
        ws = workspace.get(B * H * num_splits * (C * 2 + 4), q_nope.device, "mla")
        if tile_major:
            q, s = ops._tiled_buffers(B, H * 128, w_uv.device)
        else:
            q = torch.empty(B, H * 128, dtype=torch.float8_e4m3fn, device=w_uv.device)
            s = torch.empty(B, H, dtype=torch.float32, device=w_uv.device)
        check(
            _lib.lib().chitu_hip_mla_decode_merge_uv_quant_fp8(
                ptr(q_nope), i64(q_nope.stride(0)), i64(q_nope.stride(1)), ptr(q_pe), i64(q_pe.stride(0)), i64(q_pe.stride(1)),
                ptr(kv_cache), i64(kv_cache.shape[0]), i32(kv_cache.shape[1]), ptr(block_table), i32(block_table.stride(0)),
                ptr(cache_seqlens_incl), f32(softmax_scale), i32(B), i32(H), i32(C), i32(R), i32(num_splits), ptr(ws),
                i64(ws.numel()), ptr(w_uv), i64(w_uv.stride(0)), ptr(scale), i64(scale_offset), i64(scale_stride_h),
                i64(scale_stride_k), ptr(q), ptr(s), i32(1 if tile_major else 0), ptr(_fuse_tickets(q_nope.device)), stream_ptr(),
            ),
            "mla_decode_merge_uv_quant_fp8",
        )
        return (ops.TiledQuant(q, s, B, H * 128), None) if tile_major else (q, s)

    def mla_attn_with_kvcache(
        self,
        q_nope,
        q_pe,
        kv_cache,
        kv,
        cache_seqlens_excl_this_decode: Union[(int, torch.Tensor)],
        cache_seqlens_incl_this_decode: Union[(int, torch.Tensor)],
        block_table: torch.Tensor,
        causal=True,
        window_size=(-1, -1),  # -1 means infinite context window
        softcap=0.0,  # 0.0 means deactivated
        softmax_scale=None,
    ):
        """Same contract as TritonAttnBackend.mla_attn_with_kvcache (attn_backend.py:707-774):
        append this token's [kv_c | k_pe] row to its page, then attend over the sequence.
        Returns [B, 1, H, kv_lora_rank].  kv_cache uint8 [pages, page, 656] (the fp8 latent cache): the bf16 row `kv` is
        quantised as it is appended (ops.append_mla_kv_fp8) and the fp8 decode kernel reads the pages."""
        assert window_size == (-1, -1) and softcap == 0.0, "not used by the MLA decode path"
        if softmax_scale is None:
            # the reference's default here is accidentally a 1-tuple (attn_backend.py:756-758)
            softmax_scale = 1.0 / ((self.qk_rope_head_dim + self.qk_nope_head_dim) ** 0.5)
        if is_fp8_mla_cache(kv_cache):
            append_mla_kv_fp8(kv_cache, block_table, kv, cache_seqlens_excl_this_decode)
        else:
            append_to_paged_kv_cache(kv_cache, block_table, kv, cache_seqlens_excl_this_decode)
        B = q_nope.shape[0]
        o = self.mla_decode(q_nope, q_pe, kv_cache, cache_seqlens_incl_this_decode, block_table, float(softmax_scale))
        return o.view(B, 1, q_nope.shape[1], -1)

    # ------------------------------------------------------------------ MLA prefill (absorb mode, MQA 576/512)
    def attn_varlen_func(
        self,
        q,
        k,
        v,
        cu_seqlens_q,
        cu_seqlens_k,
        max_seqlen_q,
        max_seqlen_k,
        dropout_p=0.0,
        causal=False,
        window_size=(-1, -1),
        softcap=0.0,
        softmax_scale=None,
    ):
        """Causal varlen self-attention in the shape AttentionDeepSeekV3.prefill_forward calls it in
        absorb mode (model_deepseek_v3.py:589-599; interface attn_backend.py:39-90): MQA with
        q [T, H, C+R], k [T, 1, C+R] = [kv_norm(kv_c) | rope(k_pe)], v [T, 1, C] = the latent part of k
        (the MLA identity -- v is NOT read, k[..., :C] is used), cu_seqlens_q == cu_seqlens_k.

        chitu_hip_mla_prefill_flash (default): 128 Q rows (8 tokens x 16 heads) per workgroup against every 64-key tile,
        32x32x16 MFMA, Q in registers -- within the attention bar of the decode kernel, not bit for bit.
        CHITU_MLA_PREFILL=exact: chitu_hip_mla_prefill, the decode kernel's tile machinery with four query tokens per
        workgroup; per query token the arithmetic is the decode step's, so prefill and token-by-token decode agree bit
        for bit (3x slower at 2048 tokens; the cross-check).  CHITU_MLA_PREFILL=compose: the kernel-free composition
        (keys staged into 64-token pages, every query token run as one decode "sequence" over them) -- equal to "exact"
        bit for bit, KV re-read once per token.
        No host sync; not graph-captured (prefill never is, model.py:538-546)."""
        assert causal and dropout_p == 0.0
        T, H, Dq = q.shape
        C, R = self.kv_lora_rank, self.qk_rope_head_dim
        if Dq == 128 and k.dim() == 3 and k.shape[-1] == 128 and tuple(v.shape) == tuple(k.shape):
            # GQA / MHA, head_dim 128: window_size = (W, r) (causal: r is 0 whatever was given) and softcap >= 0 are implemented
            window_left, softcap = window_and_cap(window_size, softcap, causal)
            require_cuda(q, k, cu_seqlens_q, cu_seqlens_k)
            return self._gqa_varlen_causal(q, k, v, cu_seqlens_k, int(max_seqlen_k), softmax_scale, window_left, softcap)
        assert tuple(window_size) == (-1, -1) and softcap == 0.0, "not used by the MLA prefill path"
        require_cuda(q, k, cu_seqlens_q, cu_seqlens_k)
        assert Dq == C + R and tuple(k.shape) == (T, 1, Dq) and v.shape[0] == T and v.shape[-1] == C, \
            "only the MLA absorb-mode MQA shape (q/k 576, v 512) is implemented"
        assert cu_seqlens_q.shape == cu_seqlens_k.shape and max_seqlen_q == max_seqlen_k
        assert q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16
        if softmax_scale is None:
            softmax_scale = Dq ** -0.5
        if T == 0:
            return q.new_empty(0, H, C)
        dev = q.device
        mode = os.environ.get("CHITU_MLA_PREFILL", "flash")
        assert mode in ("flash", "exact", "compose"), mode
        if mode != "compose":
            kq = q if (q.stride(-1) == 1 and q.stride(0) % 8 == 0 and q.stride(1) % 8 == 0 and q.data_ptr() % 16 == 0) else q.contiguous()
            kk = k.reshape(T, Dq)
            if not (kk.stride(-1) == 1 and kk.stride(0) % 8 == 0 and kk.data_ptr() % 16 == 0):
                kk = kk.contiguous()
            cu32 = cu_seqlens_k.to(device=dev, dtype=torch.int32).contiguous()
            out = torch.empty(T, H, C, dtype=torch.bfloat16, device=dev)
            entry = _lib.lib().chitu_hip_mla_prefill_flash if mode == "flash" else _lib.lib().chitu_hip_mla_prefill
            check(
                entry(
                    ptr(kq), i64(kq.stride(0)), i64(kq.stride(1)), ptr(kk), i64(kk.stride(0)), ptr(cu32),
                    i32(cu32.numel() - 1), i32(int(max_seqlen_k)), f32(softmax_scale), ptr(out), i32(H), i32(C), i32(R),
                    stream_ptr(),
                ),
                "mla_prefill",
            )
            return out
        page = 64
        n_seq = cu_seqlens_k.numel() - 1
        cu = cu_seqlens_k.to(device=dev, dtype=torch.long)
        pos = torch.arange(T, device=dev)
        seq = torch.searchsorted(cu[1:].contiguous(), pos, right=True).clamp_(max=n_seq - 1)
        off = pos - cu[seq]
        pages_per = (cu[1:] - cu[:-1] + page - 1) // page
        base = torch.cumsum(pages_per, 0) - pages_per
        num_pages = T // page + n_seq + 1  # upper bound known on the host
        max_pages = max(1, (int(max_seqlen_k) + page - 1) // page)
        staged = torch.empty(num_pages, page, Dq, dtype=torch.bfloat16, device=dev)
        staged.view(-1, Dq).index_copy_(0, base[seq] * page + off, k.reshape(T, Dq))
        table = (base[seq].unsqueeze(1) + torch.arange(max_pages, device=dev)).clamp_(max=num_pages - 1).to(torch.int32)
        lens = (off + 1).to(torch.int32)
        out = torch.empty(T, H, C, dtype=torch.bfloat16, device=dev)
        step = 32768  # grid.y limit of one launch
        for t0 in range(0, T, step):
            t1 = min(T, t0 + step)
            self.mla_decode(q[t0:t1, :, :C], q[t0:t1, :, C:], staged, lens[t0:t1].contiguous(), table[t0:t1].contiguous(),
                            softmax_scale, num_splits=1, out=out[t0:t1])
        return out

    def _gqa_varlen_causal(self, q, k, v, cu_seqlens, max_seqlen, softmax_scale, window_left=-1, softcap=0.0):
        """Causal GQA / MHA prefill attention (Attention.prefill_forward, models/model.py:104-132), head_dim 128:
        q [T, Hq, 128], k / v [T, Hkv, 128].  Default: the flash kernel, chitu_hip_gqa_prefill at a group size G = Hq / Hkv that
        is a power of two and chitu_ext4_gqa_prefill (the same kernel, include/chitu_hip_ext4.h) at every other G <= 32.
        CHITU_GQA_PREFILL=compose (and shapes the kernel does not take; the decode kernel stops at G = 16): the round-2
        composition from the decode kernel -- keys / values staged once into 256-token pages, every query token one decode "sequence" of length pos + 1 over its own sequence's pages
        (chitu_hip_gqa_decode): exact causal attention with the decode numerics, KV re-read once per query token; kept
        as the cross-check.  window_left >= 0 (a token sees itself and the window_left before it) or softcap > 0:
        chitu_hip_gqa_prefill_window; the composition passes both on to the windowed decode launch.  No host sync either way."""
        T, Hq, D = q.shape
        Hkv = k.shape[1]
        if T == 0:
            return q.new_empty(0, Hq, D)
        dev = q.device
        G = Hq // Hkv
        if os.environ.get("CHITU_GQA_PREFILL", "flash") != "compose" and D == 128 and Hq % Hkv == 0 and G <= 32:
            # chitu_hip_gqa_prefill (csrc/gqa_prefill_flash.hip): 128 Q rows (128 / G tokens x G heads of one KV head) per
            # workgroup against 64-key K / V tiles; KV read once per 128 / G query tokens instead of once per token
            def ok(t):
                return t.stride(-1) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0

            qq, kk, vv = (t if ok(t) else t.contiguous() for t in (q, k, v))
            cu32 = cu_seqlens.to(device=dev, dtype=torch.int32).contiguous()
            out = torch.empty(T, Hq, D, dtype=torch.bfloat16, device=dev)
            if softmax_scale is None:
                softmax_scale = D ** -0.5
            args = (ptr(qq), i64(qq.stride(0)), i64(qq.stride(1)), ptr(kk), i64(kk.stride(0)), i64(kk.stride(1)), ptr(vv),
                    i64(vv.stride(0)), i64(vv.stride(1)), ptr(cu32), i32(cu32.numel() - 1), i32(int(max_seqlen)), f32(softmax_scale),
                    ptr(out), i32(Hq), i32(Hkv), i32(D))
            if (G & (G - 1)) != 0:
                check(_lib.lib().chitu_ext4_gqa_prefill(*args, i32(window_left), f32(softcap), stream_ptr()), "ext4_gqa_prefill")
            elif window_left >= 0 or softcap > 0.0:
                check(_lib.lib().chitu_hip_gqa_prefill_window(*args, i32(window_left), f32(softcap), stream_ptr()), "gqa_prefill_window")
            else:
                check(_lib.lib().chitu_hip_gqa_prefill(*args, stream_ptr()), "gqa_prefill")
            return out
        page = 256
        n_seq = cu_seqlens.numel() - 1
        cu = cu_seqlens.to(device=dev, dtype=torch.long)
        pos = torch.arange(T, device=dev)
        seq = torch.searchsorted(cu[1:].contiguous(), pos, right=True).clamp_(max=n_seq - 1)
        off = pos - cu[seq]
        pages_per = (cu[1:] - cu[:-1] + page - 1) // page
        base = torch.cumsum(pages_per, 0) - pages_per
        num_pages = T // page + n_seq + 1
        max_pages = max(1, (max_seqlen + page - 1) // page)
        dst = base[seq] * page + off
        k_pages = torch.zeros(num_pages, page, Hkv, D, dtype=torch.bfloat16, device=dev)
        v_pages = torch.zeros(num_pages, page, Hkv, D, dtype=torch.bfloat16, device=dev)
        k_pages.view(-1, Hkv, D).index_copy_(0, dst, k.reshape(T, Hkv, D))
        v_pages.view(-1, Hkv, D).index_copy_(0, dst, v.reshape(T, Hkv, D))
        table = (base[seq].unsqueeze(1) + torch.arange(max_pages, device=dev)).clamp_(max=num_pages - 1).to(torch.int32)
        lens = (off + 1).to(torch.int32)
        out = torch.empty(T, Hq, D, dtype=torch.bfloat16, device=dev)
        step = 16384
        for t0 in range(0, T, step):
            t1 = min(T, t0 + step)
            out[t0:t1] = self.attn_with_kvcache(q[t0:t1].unsqueeze(1), k_pages, v_pages, None, None, cache_seqlens=lens[t0:t1].contiguous(),
                                                block_table=table[t0:t1].contiguous(), window_size=(window_left, 0), softcap=softcap,
                                                softmax_scale=softmax_scale).view(t1 - t0, Hq, D)
        return out

    # ------------------------------------------------------------------ MLA continued prefill over the paged latent cache
    def mla_attn_varlen_with_kvcache(self, q, kv_cache, cu_seqlens_q, cache_seqlens, block_table, max_seqlen_q, total_keys,
                                     softmax_scale, gathered=None):
        """The MLA form of attn_varlen_with_kvcache (no reference counterpart): continued and chunked prefill in absorb mode.

        q [T, H, 576] bf16, sequence s owning rows cu_seqlens_q[s] .. cu_seqlens_q[s + 1]; kv_cache one layer of the latent
        cache, bf16 [pages, page, 576] or fp8 uint8 [pages, page, 656], with those rows' latent rows already written;
        cache_seqlens [n_seq] int32 counts ALL keys of a sequence, the new rows included; block_table [n_seq, max_pages] int32;
        max_seqlen_q bounds the launch; total_keys = sum(cache_seqlens), known to the host (no sync).  Query i of sequence s
        sits at position cache_seqlens[s] - n_s + i and sees the keys up to itself.  Returns [T, H, 512].

        Two launches: ops.mla_kv_gather copies (bf16) or widens (fp8) every sequence's rows out of the pages into `gathered`
        (bf16 [>= total_keys, 576]; allocated when None -- a model passes one buffer for all its layers), then
        chitu_ext2_mla_prefill_flash_continue runs the flash prefill kernel with separate query and key extents over it.
        With an fp8 cache the queries therefore attend over the QUANTISED rows, their own chunk's included."""
        from . import ops

        require_cuda(q, kv_cache, cu_seqlens_q, cache_seqlens, block_table)
        C, R = self.kv_lora_rank, self.qk_rope_head_dim
        assert (C, R) == (512, 64), "the flash prefill kernel is built for 512 + 64 rows"
        assert q.dim() == 3 and q.dtype == torch.bfloat16 and q.shape[-1] == C + R
        assert cache_seqlens.dtype == torch.int32 and cache_seqlens.dim() == 1
        T, H, _ = q.shape
        n_seq = cache_seqlens.numel()
        assert cu_seqlens_q.numel() == n_seq + 1 and block_table.shape[0] == n_seq
        if T == 0:
            return q.new_empty(0, H, C)
        dev = q.device
        cu_k = torch.zeros(n_seq + 1, dtype=torch.int32, device=dev)
        torch.cumsum(cache_seqlens, 0, dtype=torch.int32, out=cu_k[1:])
        gathered = ops.mla_kv_gather(kv_cache, block_table, cu_k, int(total_keys), out=gathered)
        if not (q.stride(-1) == 1 and q.stride(0) % 8 == 0 and q.stride(1) % 8 == 0 and q.data_ptr() % 16 == 0):
            q = q.contiguous()
        cu_q = cu_seqlens_q.to(device=dev, dtype=torch.int32).contiguous()
        out = torch.empty(T, H, C, dtype=torch.bfloat16, device=dev)
        check(
            _lib.lib().chitu_ext2_mla_prefill_flash_continue(
                ptr(q), i64(q.stride(0)), i64(q.stride(1)), ptr(gathered), i64(gathered.stride(0)), ptr(cu_q), ptr(cu_k), i32(n_seq),
                i32(int(max_seqlen_q)), f32(softmax_scale), ptr(out), i32(H), i32(C), i32(R), stream_ptr(),
            ),
            "mla_prefill_flash_continue",
        )
        return out

    # ------------------------------------------------------------------ GQA / MHA continued prefill over the paged cache
    def attn_varlen_with_kvcache(self, q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table, max_seqlen_q, causal=True,
                                 window_size=(-1, -1), softcap=0.0, softmax_scale=None):
        """The ragged form of attn_with_kvcache (no reference counterpart: attn_varlen_func's separate cu_seqlens_q with its keys
        in the pages, attn_with_kvcache at any seqlen_q): continued and chunked prefill.

        q [T, Hq, 128] bf16, sequence s owning rows cu_seqlens_q[s] .. cu_seqlens_q[s + 1]; k_cache / v_cache
        [pages, page_size, Hkv, 128] bf16 with those rows' K and V already written; cache_seqlens [n_seq] int32 counts ALL keys
        of a sequence, the new rows included; block_table [n_seq, max_pages] int32; max_seqlen_q bounds the launch.  Query i of
        sequence s sits at position cache_seqlens[s] - n_s + i and sees the keys up to itself (the causal mask aligned to the bottom
        right), within window_size = (W, 0) the last W + 1 of them; softcap as in attn_with_kvcache.  Returns [T, Hq, 128].
        One launch of chitu_hip_gqa_prefill_paged (csrc/gqa_prefill_flash.hip, kPaged; chitu_ext4_gqa_prefill_paged when
        G = Hq / Hkv is no power of two, any G <= 32): the pages are read once per 128 / G query tokens.  An fp8 cache raises
        NotImplementedError (the LDS-DMA cannot widen 144-byte rows), as does a mask that is not causal."""
        if is_fp8_gqa_cache(k_cache) or is_fp8_gqa_cache(v_cache):
            raise NotImplementedError("attn_varlen_with_kvcache reads bf16 K / V pages; the fp8 K / V cache is not implemented")
        window_left, softcap = window_and_cap(window_size, softcap, causal)
        if not causal and int(window_size[1]) != 0:
            raise NotImplementedError(f"causal=False with window_size={tuple(window_size)}: only the causal mask (causal=True, or a "
                                      "window whose right side is 0) is implemented")
        require_cuda(q, k_cache, v_cache, cu_seqlens_q, cache_seqlens, block_table)
        assert q.dim() == 3 and q.dtype == torch.bfloat16 and k_cache.dtype == torch.bfloat16 and v_cache.dtype == torch.bfloat16
        assert k_cache.dim() == 4 and k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape == v_cache.shape
        assert cache_seqlens.dtype == torch.int32 and cache_seqlens.is_contiguous()
        assert block_table.dtype == torch.int32 and block_table.dim() == 2 and block_table.stride(1) == 1
        T, Hq, D = q.shape
        Hkv = k_cache.shape[2]
        n_seq = cache_seqlens.numel()
        assert cu_seqlens_q.numel() == n_seq + 1 and block_table.shape[0] == n_seq and k_cache.shape[3] == D
        if T == 0:
            return q.new_empty(0, Hq, D)
        if softmax_scale is None:
            softmax_scale = D ** -0.5
        if not (q.stride(-1) == 1 and q.stride(0) % 8 == 0 and q.stride(1) % 8 == 0 and q.data_ptr() % 16 == 0):
            q = q.contiguous()
        cu32 = cu_seqlens_q.to(device=q.device, dtype=torch.int32).contiguous()
        out = torch.empty(T, Hq, D, dtype=torch.bfloat16, device=q.device)
        G = Hq // max(Hkv, 1)
        entry = _lib.lib().chitu_hip_gqa_prefill_paged if (G & (G - 1)) == 0 else _lib.lib().chitu_ext4_gqa_prefill_paged
        check(
            entry(
                ptr(q), i64(q.stride(0)), i64(q.stride(1)), ptr(k_cache), ptr(v_cache), i64(k_cache.shape[0]), i32(k_cache.shape[1]),
                i32(Hkv), ptr(block_table), i32(block_table.stride(0)), ptr(cu32), ptr(cache_seqlens), i32(n_seq),
                i32(int(max_seqlen_q)), f32(softmax_scale), ptr(out), i32(Hq), i32(D), i32(window_left), f32(softcap), stream_ptr(),
            ),
            "gqa_prefill_paged",
        )
        return out

    # ------------------------------------------------------------------ non-MLA (GQA / MHA) paged decode
    def attn_with_kvcache(
        self,
        q,
        k_cache,
        v_cache,
        k=None,
        v=None,
        cache_seqlens: Optional[Union[(int, torch.Tensor)]] = None,
        cache_leftpad: Optional[torch.Tensor] = None,
        block_table: Optional[torch.Tensor] = None,
        causal=False,
        window_size=(-1, -1),
        softcap=0.0,
        softmax_scale=None,
        num_splits: Optional[int] = None,
    ):
        """Paged single-token attention with in-place append, the contract of
        AttnBackend.attn_with_kvcache (chitu/attn_backend.py:92-164) as FlashAttnBackend implements
        it (:208-243): if k/v are given they are written at position cache_seqlens[b] of each
        sequence's pages, then q attends to cache_seqlens[b] + 1 tokens.

        q [bs, 1, Hq, 128]; k_cache / v_cache [pages, page_size, Hkv, 128]; k / v [bs, 1, Hkv, 128];
        cache_seqlens [bs] int32 (excluding this token); block_table [bs, max_pages] int32.
        Returns [bs, 1, Hq, 128].  (RefAttnBackend rejects block_table, :473 -- this is the paged path.)

        k_cache / v_cache uint8 [pages, page_size, Hkv, 144] (the fp8 K / V cache): k / v are quantised as they are appended
        (ops.append_gqa_kv_fp8, one launch for both) and chitu_hip_gqa_decode_kv_fp8 reads the pages -- same arguments, same
        workspace; the result is bit-identical to this call on ops.gqa_kv_dequant_fp8 of the caches.

        window_size = (W, 0) -- or (W, r) with causal=True, which makes the right side 0 -- and softcap >= 0 (the reference's
        semantics, :136-138 and RefAttnBackend._attention): the query sees the last W + 1 keys, the appended one included, and
        the score is softcap * tanh(scale * q.k / softcap).  chitu_hip_gqa_decode_window / _kv_fp8_window, taken only when a
        window or a cap is set; they read only the pages the window overlaps.  A right window on a non-causal call raises.

        q [bs, T, Hq, 128] with 1 < T <= 8 (the contract's seqlen > 1; a speculative verify step): k / v [bs, T, Hkv, 128] are
        written at cache_seqlens[b] .. + T - 1, then query t attends to the keys k <= cache_seqlens[b] + t (within the window:
        k >= cache_seqlens[b] + t - W) -- the causal mask aligned to the bottom right.  Needs causal=True or a window whose right
        side is 0 (anything else: NotImplementedError).  chitu_hip_gqa_decode_multi / _kv_fp8 (csrc/gqa_decode_multi.hip):
        16 // (Hq // Hkv) query tokens share one walk over the pages.  Returns [bs, T, Hq, 128].
        """
        assert block_table is not None, "HipAttnBackend.attn_with_kvcache is the paged path"
        assert cache_leftpad is None, "cache_leftpad is not implemented"
        window_left, softcap = window_and_cap(window_size, softcap, causal)
        assert q.dim() == 4 and 1 <= q.shape[1] <= GQA_MULTI_MAX_Q, f"decode: 1 .. {GQA_MULTI_MAX_Q} query tokens per sequence"
        if q.shape[1] > 1:
            if not causal and int(window_size[1]) != 0:
                raise NotImplementedError(f"{q.shape[1]} query tokens with causal=False and window_size={tuple(window_size)}: only the "
                                          "causal mask (causal=True, or a window whose right side is 0) is implemented")
            return self._attn_with_kvcache_multi(q, k_cache, v_cache, k, v, cache_seqlens, block_table, window_left, softcap,
                                                 softmax_scale, num_splits)
        require_cuda(q, k_cache, v_cache, cache_seqlens, block_table)
        fp8_kv = is_fp8_gqa_cache(k_cache)
        if fp8_kv:
            assert q.dtype == torch.bfloat16 and is_fp8_gqa_cache(v_cache) and q.shape[-1] == 128
        else:
            assert q.dtype == torch.bfloat16 and k_cache.dtype == torch.bfloat16 and v_cache.dtype == torch.bfloat16
        assert k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape == v_cache.shape
        assert cache_seqlens.dtype == torch.int32 and block_table.dtype == torch.int32 and block_table.stride(1) == 1
        bs, _, Hq, D = q.shape
        Hkv = k_cache.shape[2]
        if softmax_scale is None:
            softmax_scale = D ** -0.5
        seqlens = cache_seqlens
        if k is not None:
            assert v is not None
            if fp8_kv:
                append_gqa_kv_fp8(k_cache, v_cache, block_table, k, v, cache_seqlens)
            else:
                append_to_paged_kv_cache(k_cache, block_table, k.contiguous(), cache_seqlens)
                append_to_paged_kv_cache(v_cache, block_table, v.contiguous(), cache_seqlens)
            seqlens = cache_seqlens + 1
        q3 = q.view(bs, Hq, D)
        if not (q3.stride(-1) == 1 and q3.stride(0) % 8 == 0 and q3.stride(1) % 8 == 0 and q3.data_ptr() % 16 == 0):
            q3 = q3.contiguous()
        if num_splits is None:
            num_splits = gqa_num_splits(bs, Hkv, int(block_table.shape[1]), int(k_cache.shape[1]), window_left)
        out = torch.empty(bs, Hq, D, dtype=torch.bfloat16, device=q.device)
        need = bs * Hq * num_splits * (D + 1) * 4 if num_splits > 1 else 1
        ws = workspace.get(need, q.device, "gqa")
        name = "gqa_decode_kv_fp8" if fp8_kv else "gqa_decode"
        extra = ()
        if window_left >= 0 or softcap > 0.0:
            name, extra = name + "_window", (i32(window_left), f32(softcap))
        check(
            getattr(_lib.lib(), "chitu_hip_" + name)(
                ptr(q3), i64(q3.stride(0)), i64(q3.stride(1)), ptr(k_cache), ptr(v_cache), i64(k_cache.shape[0]),
                i32(k_cache.shape[1]), i32(Hkv), ptr(block_table), i32(block_table.stride(0)), ptr(seqlens),
                f32(softmax_scale), ptr(out), i32(bs), i32(Hq), i32(D), i32(num_splits), ptr(ws), i64(ws.numel()),
                *extra, stream_ptr(),
            ),
            name,
        )
        return out.view(bs, 1, Hq, D)

    def _attn_with_kvcache_multi(self, q, k_cache, v_cache, k, v, cache_seqlens, block_table, window_left, softcap, softmax_scale,
                                 num_splits):
        """attn_with_kvcache for q [bs, T, Hq, 128], T > 1.  The append runs the single-token append kernels on the bs * T
        expanded rows (row (b, t): table row b, position cache_seqlens[b] + t)."""
        require_cuda(q, k_cache, v_cache, cache_seqlens, block_table)
        fp8_kv = is_fp8_gqa_cache(k_cache)
        if fp8_kv:
            assert q.dtype == torch.bfloat16 and is_fp8_gqa_cache(v_cache) and q.shape[-1] == 128
        else:
            assert q.dtype == torch.bfloat16 and k_cache.dtype == torch.bfloat16 and v_cache.dtype == torch.bfloat16
        assert k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape == v_cache.shape
        assert cache_seqlens.dtype == torch.int32 and block_table.dtype == torch.int32 and block_table.stride(1) == 1
        bs, T, Hq, D = q.shape
        Hkv = k_cache.shape[2]
        if softmax_scale is None:
            softmax_scale = D ** -0.5
        seqlens = cache_seqlens
        if k is not None:
            assert v is not None and k.shape[:2] == (bs, T) and v.shape[:2] == (bs, T)
            rows_table = block_table.repeat_interleave(T, dim=0).contiguous()
            rows_lens = (cache_seqlens.view(bs, 1) + torch.arange(T, dtype=torch.int32, device=q.device)).view(bs * T)
            kr, vr = k.reshape(bs * T, Hkv, D), v.reshape(bs * T, Hkv, D)
            if fp8_kv:
                append_gqa_kv_fp8(k_cache, v_cache, rows_table, kr, vr, rows_lens)
            else:
                append_to_paged_kv_cache(k_cache, rows_table, kr.contiguous(), rows_lens)
                append_to_paged_kv_cache(v_cache, rows_table, vr.contiguous(), rows_lens)
            seqlens = cache_seqlens + T
        if not (q.stride(-1) == 1 and all(q.stride(i) % 8 == 0 for i in range(3)) and q.data_ptr() % 16 == 0):
            q = q.contiguous()
        if num_splits is None:
            tiles = -(-T // (16 // (Hq // Hkv)))  # workgroups per (sequence, kv head): 16 // G query tokens share one
            num_splits = gqa_num_splits(bs * tiles, Hkv, int(block_table.shape[1]), int(k_cache.shape[1]), window_left)
        out = torch.empty(bs, T, Hq, D, dtype=torch.bfloat16, device=q.device)
        need = bs * T * Hq * num_splits * (D + 1) * 4 if num_splits > 1 else 1
        ws = workspace.get(need, q.device, "gqa")
        name = "gqa_decode_multi_kv_fp8" if fp8_kv else "gqa_decode_multi"
        check(
            getattr(_lib.lib(), "chitu_hip_" + name)(
                ptr(q), i64(q.stride(0)), i64(q.stride(1)), i64(q.stride(2)), ptr(k_cache), ptr(v_cache), i64(k_cache.shape[0]),
                i32(k_cache.shape[1]), i32(Hkv), ptr(block_table), i32(block_table.stride(0)), ptr(seqlens),
                f32(softmax_scale), ptr(out), i32(bs), i32(T), i32(Hq), i32(D), i32(num_splits), ptr(ws), i64(ws.numel()),
                i32(window_left), f32(softcap), stream_ptr(),
            ),
            name,
        )
        return out
