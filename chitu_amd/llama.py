"""Llama-family (GQA / MHA, bf16) decode step on the gfx950 kernels -- BASELINE config 2
("Llama-3-8B bf16 TP=1 on one MI355X, paged KV, hipGraph decode").

Reference (read-only): chitu/models/model.py -- Attention:81-198 (decode_forward_paged:167-198),
FeedForward:201-214, TransformerBlock, Transformer.decode:538-622; models/model_llama.py (merged
wqkv / w13 layout of the original Meta checkpoints, rotary_type "llama" = interleaved pairs).

Per layer and step, 7 launches: add+RMSNorm, wqkv GEMM, [RoPE(q, k) + append K, V], paged GQA decode
(+ merge when the KV range is split), wo GEMM, add+RMSNorm, [w13 GEMM + SiluAndMul], w2 GEMM -- 4 at batch 1-2,
where both add+RMSNorm steps run as the prologue of the GEMM behind them and RoPE + the K / V append as the
epilogue of the qkv projection (bf16_norm_gemm.hip).
All GEMMs are the weight-streaming skinny bf16 kernel (bf16_gemm.hip); the whole step replays as one hipGraph.
"""

import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import ops
from . import tensor_parallel as tp
from .attn_backend import GQA_MULTI_MAX_Q, HipAttnBackend
from .cache_manager import PagedKVCacheManager, gqa_kv_layout
from .decoder import DecoderBase


@dataclass
class LlamaArgs:
    """Fields of chitu/config/models/Meta-Llama-3-8B-Instruct-original.yaml:6-14 (defaults = Llama-3-8B)."""

    dim: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    vocab_size: int = 128256
    ffn_dim: int = 14336
    norm_eps: float = 1e-5
    rope_theta: float = 500000.0
    kv_cache_dtype: str = "bf16"  # "fp8": 144-byte K / V rows per token and head (cache_manager.gqa_kv_layout), quantised as they are appended
    # a token attends to the last `sliding_window` positions, itself included (Hugging Face's rule kv_idx > q_idx - sliding_window;
    # Mistral-7B-v0.1: 4096); None: all of them.  Passed to the attention backend as window_size = (sliding_window - 1, 0).
    sliding_window: Optional[int] = None
    attn_softcap: float = 0.0  # > 0: scores are attn_softcap * tanh(score / attn_softcap) (the backend's softcap); 0.0: off
    # "w8a16": wqkv, wo, w13 and w2 of every layer are int8 with one fp32 scale per output row (quantize/w8a16.py); None: bf16
    quant: Optional[str] = None

    @property
    def head_dim(self):
        return self.dim // self.n_heads


def check_quant_supported(quant, who: str, dense: bool = True) -> None:
    """The `quant` field of the model args: None, or "w8a16" on the dense Llama-family decoders (Llama, Qwen2, Qwen3)."""
    if quant is None:
        return
    if quant != "w8a16":
        raise ValueError(f"{who}: quant={quant!r} is not supported (None or 'w8a16')")
    if not dense:
        raise ValueError(f"{who}: quant='w8a16' covers the dense Llama-family decoders; this model's linears have their own formats")


def precompute_freqs_cis(head_dim: int, max_pos: int, theta: float):
    """cos/sin [max_pos, head_dim/2] fp32 (models/model.py:81-88: precompute_freqs_cis; torch.polar like the
    reference so the table is bit-identical)."""
    freqs = 1.0 / (theta ** (torch.arange(0, head_dim, 2)[: head_dim // 2].float() / head_dim))
    ang = torch.outer(torch.arange(max_pos, dtype=torch.float32), freqs)
    cis = torch.polar(torch.ones_like(ang), ang)
    return cis.real.contiguous(), cis.imag.contiguous()


def _param(*shape, device=None):
    return torch.nn.Parameter(torch.empty(*shape, dtype=torch.bfloat16, device=device), requires_grad=False)


def _linear_weight(mod, name, n, k, quant, device):
    """mod.<name>: the [n, k] weight of a linear -- bf16, or with quant "w8a16" int8 plus the fp32 row scales mod.<name>_scale."""
    if quant == "w8a16":
        setattr(mod, name, torch.nn.Parameter(torch.empty(n, k, dtype=torch.int8, device=device), requires_grad=False))
        setattr(mod, name + "_scale", torch.nn.Parameter(torch.empty(n, dtype=torch.float32, device=device), requires_grad=False))
    else:
        setattr(mod, name, _param(n, k, device=device))


def _linear(mod, name, x):
    """x @ mod.<name>^T: the bf16 stream, or the W8A16 one when the weight is int8."""
    w = getattr(mod, name)
    if w.dtype == torch.int8:
        return ops.w8a16_linear(x, w, getattr(mod, name + "_scale"))
    return ops.bf16_linear(x, w)


# Decode batches up to this size run a layer's two residual-add + RMSNorm steps as the prologue of the GEMMs behind
# them, and RoPE + the K / V page append as the epilogue of the qkv projection (ops.bf16_linear_add_norm[_qkv_post] /
# bf16_linear_silu_add_norm: bit-identical, three launches fewer per layer).  Measured on Llama-3-8B (tools/llama_ab.py,
# profiles/r02_ab_llama_norm_prologue.txt): bs 1 3.45 -> 3.20 ms/step, bs 2 3.57 -> 3.44, bs 4 3.70 -> 3.84 (the
# four-row prologue costs more registers and LDS traffic than the launches it saves).  0 = off.
FUSE_NORM_MAX_BS = int(os.environ.get("CHITU_FUSE_NORM_MAX_BS", "2"))


def _fuses_norm(x, pending, n_out, two_terms_ok: bool = False, weight=None) -> bool:
    """pending must be a plain [bs, dim] tensor: not None (first layer), not a partial whose all-reduce the norm launch
    itself performs (tensor_parallel.PendingAllReduce, the in-graph xGMI form).  two_terms_ok: also [bs, 2, dim] (a top-2 MoE's
    un-summed outputs), for the prologue that takes them (ops.bf16_linear_add_norm).  weight: the matrix behind the norm; an int8
    one (W8A16) has no prologue form and takes the norm launch and the linear separately."""
    if weight is not None and weight.dtype == torch.int8:
        return False
    dims_ok = isinstance(pending, torch.Tensor) and (pending.dim() == 2 or (two_terms_ok and pending.dim() == 3 and pending.shape[1] == 2))
    return dims_ok and x.shape[0] <= FUSE_NORM_MAX_BS and ops.bf16_add_norm_fits(x.shape[0], n_out, x.shape[1])


class LlamaAttention(torch.nn.Module):
    def __init__(self, args, layer_id, cache, attn_backend, device=None, rotary_type="llama"):
        super().__init__()
        self.rotary_type = rotary_type  # "llama" (Meta original, interleaved) | "hf-llama" (half split) | "glm4" (partial interleaved)
        t = tp.get_tp_size()
        self.layer_id, self.cache, self.attn_backend = layer_id, cache, attn_backend
        self.hd = args.head_dim
        self.hq, self.hkv = args.n_heads // t, args.n_kv_heads // t
        self.fp8_kv = args.kv_cache_dtype == "fp8"
        if args.sliding_window is not None and args.sliding_window < 1:
            raise ValueError(f"sliding_window={args.sliding_window}: a token attends at least to itself (None = no window)")
        # launch constants of both attention calls: the captured decode graph holds them like any other scalar argument
        self.window_size = (-1, -1) if args.sliding_window is None else (args.sliding_window - 1, 0)
        self.softcap = float(args.attn_softcap)
        # merged [wq | wk | wv] rows (ColumnParallel: heads split across ranks), wo RowParallel
        quant = getattr(args, "quant", None)
        _linear_weight(self, "wqkv", (self.hq + 2 * self.hkv) * self.hd, args.dim, quant, device)
        _linear_weight(self, "wo", args.dim, self.hq * self.hd, quant, device)
        # Qwen3: an RMSNorm with a learned [head_dim] weight on every q head and every k head, after the projection and before
        # RoPE (replicated under TP: the weights are per channel, not per head)
        self.qk_norm = bool(getattr(args, "qk_norm", False))
        if self.qk_norm:
            assert self.hd == 128, "the head-norm launches are head_dim 128"
            self.q_norm = _param(self.hd, device=device)
            self.k_norm = _param(self.hd, device=device)
            self.qk_eps = args.norm_eps
        # Qwen2: a bias on the q / k / v projections, one merged row laid out like a row of wqkv's output (ColumnParallel like
        # wqkv: this rank's q heads, then k heads, then v heads).  It is added in the launch that rotates q and k and appends k and
        # v (decode) or in the prompt's one rotation launch (prefill), never as a launch of its own.
        self.qkv_bias = bool(getattr(args, "qkv_bias", False))
        if self.qkv_bias:
            if self.qk_norm:
                raise ValueError("qkv_bias together with qk_norm: no launch adds a bias in front of the head norm (no published model has both)")
            if self.hd != 128:
                raise ValueError(f"qkv_bias: the bias launches are head_dim 128, got {self.hd} (Qwen2.5-0.5B has 64)")
            self.bqkv = _param((self.hq + 2 * self.hkv) * self.hd, device=device)
        # GLM-4: interleaved pairs over the first rotary_dim channels of a head (the width of the decoder's cos / sin table), the
        # rest pass through.  Only the bias launches take a rotary width (include/chitu_hip_ext7.h).
        if rotary_type == "glm4":
            if self.qk_norm:
                raise ValueError("rotary_type 'glm4' with qk_norm: the head-norm launches rotate all 128 channels (no partial width)")
            if not self.qkv_bias:
                raise ValueError("rotary_type 'glm4' needs qkv_bias: the partial rotary width exists in the bias launches only "
                                 "(GLM-4-9B has a q / k / v bias)")

    def decode_forward_paged(self, x, cos, sin, q_len=1):
        """x = attn_norm(h) bf16 [bs, dim] -> wo(attention) before the all-reduce (model.py:167-198)."""
        return self.decode_from_qkv(_linear(self, "wqkv", x), cos, sin, q_len)

    def _row_tables(self, q_len):
        """(block table, old length) per row of the step: one row per sequence, or -- a multi-token step, q_len > 1 -- one per
        (sequence, token) in that order (PagedKVCacheManager.prepare_block_table_for_decode_multi)."""
        if q_len > 1:
            return self.cache.get_gpu_multi_block_table(), self.cache.get_gpu_multi_row_lens()
        return self.cache.get_gpu_block_table(), self.cache.get_gpu_seq_lens_excl_this_decode()

    def decode_from_qkv(self, qkv, cos, sin, q_len=1):
        """The merged projection's output [bs, (hq + 2 hkv) * hd] -> wo(attention) before the all-reduce."""
        bs = qkv.shape[0]
        qkv = qkv.view(bs, self.hq + 2 * self.hkv, self.hd)
        k_cache, v_cache = self.cache.get_paged_kv_cache(self.layer_id)
        # RoPE(q, k) + append of k and v to their pages: one launch (fp8 cache: with quantising stores)
        if self.qk_norm:  # the head norm in front of the rotation, same launch
            post, extra = "gqa_qkv_norm_post", (self.q_norm, self.k_norm, self.qk_eps)
        elif self.qkv_bias:  # the bias in front of the rotation, same launch
            post, extra = "gqa_qkv_bias_post", (self.bqkv,)
        else:
            post, extra = "gqa_qkv_post", ()
        q = getattr(ops, post + ("_kv_fp8" if self.fp8_kv else ""))(
            qkv, self.hq, self.hkv, cos, sin, k_cache, v_cache, *self._row_tables(q_len), *extra, rotary_type=self.rotary_type)
        return self.decode_from_q(q, q_len)

    def decode_from_q(self, q, q_len=1):
        """Rotated q heads [bs, hq, hd] (this token's k and v already in their pages) -> wo(attention).  q_len > 1: the rows are
        q_len consecutive tokens of bs / q_len sequences, all their k and v in the pages: one multi-token attention call."""
        bs = q.shape[0]
        k_cache, v_cache = self.cache.get_paged_kv_cache(self.layer_id)
        if q_len > 1:
            o = self.attn_backend.attn_with_kvcache(
                q.view(bs // q_len, q_len, self.hq, self.hd), k_cache, v_cache, None, None,
                cache_seqlens=self.cache.get_gpu_multi_seq_lens_incl(), block_table=self.cache.get_gpu_multi_block_table()[::q_len],
                causal=True, window_size=self.window_size, softcap=self.softcap)
            return _linear(self, "wo", o.view(bs, self.hq * self.hd))
        table = self.cache.get_gpu_block_table()
        o = self.attn_backend.attn_with_kvcache(
            q.unsqueeze(1), k_cache, v_cache, None, None,
            cache_seqlens=self.cache.get_gpu_seq_lens_incl_this_decode()[:bs], block_table=table[:bs],
            window_size=self.window_size, softcap=self.softcap)
        return _linear(self, "wo", o.view(bs, self.hq * self.hd))

    def decode_from_residual(self, x, pending, norm_weight, eps, cos, sin, q_len=1):
        """Small decode batches: residual add + attn_norm + wqkv projection [+ RoPE and the K / V page append when the
        rotary pairs are interleaved] in ONE launch.  Returns (x + pending, wo(attention) before the all-reduce).  The fused
        epilogue writes bf16 page rows: an fp8 cache takes the two-launch form of "hf-llama", and so does a model with a head norm
        or a qkv bias (the epilogue neither normalises nor adds one)."""
        if self.rotary_type == "llama" and not self.fp8_kv and not self.qk_norm and not self.qkv_bias:
            k_cache, v_cache = self.cache.get_paged_kv_cache(self.layer_id)
            x, qkv = ops.bf16_linear_add_norm_qkv_post(
                x, pending, norm_weight, eps, self.wqkv, self.hq, self.hkv, cos, sin, k_cache, v_cache, *self._row_tables(q_len))
            return x, self.decode_from_q(qkv[:, : self.hq], q_len)
        x, qkv = ops.bf16_linear_add_norm(x, pending, norm_weight, eps, self.wqkv)
        return x, self.decode_from_qkv(qkv, cos, sin, q_len)

    def _rotate(self, qkv, cos, sin):
        """Prefill: qkv [T, hq + 2 hkv, hd] -> (q, k, v) with RoPE on the q and k heads (behind the head norm or the bias, when the
        model has one) and v contiguous.  With a bias the three come out of ONE launch; otherwise the rotation and the copy of v
        are one each."""
        if self.qkv_bias:
            return ops.qkv_bias_rope(qkv, self.hq, self.hkv, self.bqkv, cos, sin, rotary_type=self.rotary_type)
        q, k = qkv[:, : self.hq], qkv[:, self.hq : self.hq + self.hkv]
        if self.qk_norm:
            q, k = ops.qk_norm_rope(q, k, self.q_norm, self.k_norm, self.qk_eps, cos, sin, rotary_type=self.rotary_type)
        else:
            q, k = ops.apply_rotary_pos_emb(q, k, cos, sin, rotary_type=self.rotary_type)
        return q, k, qkv[:, self.hq + self.hkv :].contiguous()

    def prefill_forward(self, x, cos, sin, varlens):
        """models/model.py:104-132: projections on all T prompt tokens, RoPE, page writes by the cache
        manager (cache_manager.py:93-142), causal GQA through attn_backend.attn_varlen_func.  varlens.continued (set by
        LlamaDecoder.prefill_continue): the rows extend cached sequences -- prefill_forward_paged."""
        if getattr(varlens, "continued", False):
            return self.prefill_forward_paged(x, cos, sin, varlens)
        T = x.shape[0]
        qkv = _linear(self, "wqkv", x).view(T, self.hq + 2 * self.hkv, self.hd)
        q, k, v = self._rotate(qkv, cos, sin)
        if self.fp8_kv:
            # the pages take the quantised rows (the same index_copy_ scatter, over byte rows); attention runs over the
            # unquantised ones, as the MLA prefill does
            self.cache.finalize_cache_bylayer_prefill(ops.gqa_kv_quant_fp8(k), ops.gqa_kv_quant_fp8(v), self.cache.curr_req_ids,
                                                      self.cache.curr_varlens, self.layer_id)
        else:
            self.cache.finalize_cache_bylayer_prefill(k, v, self.cache.curr_req_ids, self.cache.curr_varlens, self.layer_id)
        o = self.attn_backend.attn_varlen_func(q, k, v, varlens.prefix_lens, varlens.prefix_lens, varlens.max_len,
                                               varlens.max_len, causal=True, window_size=self.window_size, softcap=self.softcap)
        return _linear(self, "wo", o.reshape(T, self.hq * self.hd))

    def prefill_forward_paged(self, x, cos, sin, varlens):
        """prefill_forward for tokens behind rows that are already cached (PagedKVCacheManager.prepare_cache_prefill_continue has
        run): projections, RoPE at the absolute positions (cos / sin rows), the new K / V rows scattered into their pages, then ONE
        attention call over the pages -- every query sees the cached prefix and the new rows up to itself."""
        assert not self.fp8_kv, "continued prefill reads bf16 K / V pages"
        T = x.shape[0]
        qkv = _linear(self, "wqkv", x).view(T, self.hq + 2 * self.hkv, self.hd)
        q, k, v = self._rotate(qkv, cos, sin)
        self.cache.finalize_cache_bylayer_prefill_continue(k, v, self.layer_id)
        k_cache, v_cache = self.cache.get_paged_kv_cache(self.layer_id)
        o = self.attn_backend.attn_varlen_with_kvcache(
            q, k_cache, v_cache, varlens.prefix_lens, self.cache.get_gpu_continue_seq_lens_incl(),
            self.cache.get_gpu_continue_block_table(), varlens.max_len, causal=True, window_size=self.window_size, softcap=self.softcap)
        return _linear(self, "wo", o.reshape(T, self.hq * self.hd))


class LlamaFeedForward(torch.nn.Module):
    """w2(silu(w1 x) * w3 x) with w1 / w3 merged row-wise (model.py:201-214)."""

    def __init__(self, args: LlamaArgs, device=None):
        super().__init__()
        t = tp.get_tp_size()
        self.inter = args.ffn_dim // t
        quant = getattr(args, "quant", None)
        _linear_weight(self, "w13", 2 * self.inter, args.dim, quant, device)
        _linear_weight(self, "w2", args.dim, self.inter, quant, device)

    def forward(self, x):
        if self.w13.dtype == torch.int8:
            return _linear(self, "w2", ops.w8a16_linear_silu(x, self.w13, self.w13_scale))
        return ops.bf16_linear(ops.bf16_linear_silu(x, self.w13), self.w2)


class GqaBlock(torch.nn.Module):
    """A LlamaAttention behind attn_norm and an FFN behind ffn_norm; the residual adds are folded into the RMSNorm that consumes
    them.  The attention half is stated here once; a family names its FFN module and states the FFN half in forward()."""

    rotary_type = "llama"  # subclasses name the half-split ("hf-llama": Qwen, Mixtral) or the partial ("glm4") layout
    ffn_type = None  # the module behind ffn_norm: ffn_type(args, device)

    def __init__(self, layer_id, args, cache, attn_backend, device=None):
        super().__init__()
        self.attn = LlamaAttention(args, layer_id, cache, attn_backend, device, rotary_type=self.rotary_type)
        self.ffn = self.ffn_type(args, device)
        self.attn_norm = _param(args.dim, device=device)
        self.ffn_norm = _param(args.dim, device=device)
        self.eps = args.norm_eps

    def attn_part(self, x, pending, cos, sin, varlens, q_len, fuse=True, **fuses_norm_args):
        """(x, pending) -> (x + pending, the attention's output with its all-reduce deferred).  Small decode batches
        (_fuses_norm, with the block's own arguments; fuse=False: never): the add + attn_norm run as the prologue of the qkv
        projection, bit-identical, one launch less per layer.  varlens given = prefill."""
        if fuse and varlens is None and _fuses_norm(x, pending, self.attn.wqkv.shape[0], **fuses_norm_args):
            x, a = self.attn.decode_from_residual(x, pending, self.attn_norm, self.eps, cos, sin, q_len)
        else:
            x, hn = tp.add_norm(x, pending, self.attn_norm, self.eps)[:2]
            if varlens is None:
                a = self.attn.decode_forward_paged(hn, cos, sin, q_len)
            else:
                a = self.attn.prefill_forward(hn, cos, sin, varlens)
        return x, tp.defer_all_reduce(a)


class LlamaBlock(GqaBlock):
    ffn_type = LlamaFeedForward

    def forward(self, x, pending, cos, sin, varlens=None, q_len=1):
        """(x, pending) -> (x', pending'); varlens given = prefill; q_len > 1: the rows are q_len tokens per sequence
        (DecoderBase.decode_multi)."""
        x, a = self.attn_part(x, pending, cos, sin, varlens, q_len, weight=self.attn.wqkv)
        return self.ffn_part(x, a, varlens)

    def ffn_part(self, x, a, varlens):
        if varlens is None and _fuses_norm(x, a, self.ffn.inter, weight=self.ffn.w13):
            x, h = ops.bf16_linear_silu_add_norm(x, a, self.ffn_norm, self.eps, self.ffn.w13)
            return x, tp.defer_all_reduce(ops.bf16_linear(h, self.ffn.w2))
        x, hn = tp.add_norm(x, a, self.ffn_norm, self.eps)[:2]
        return x, tp.defer_all_reduce(self.ffn(hn))


class LlamaDecoder(DecoderBase):
    """DecoderBase over GQA blocks with bf16 (or W8A16) linears and a paged K / V cache (model.py:538-622)."""

    block_type = None  # subclasses (Mixtral) swap the block
    multi_max_q = GQA_MULTI_MAX_Q

    def __init__(self, args: LlamaArgs, cache: PagedKVCacheManager, attn_backend: HipAttnBackend,
                 max_position_embeddings: int = 4096, device="cuda"):
        super().__init__(args, cache, attn_backend, device)
        t = tp.get_tp_size()
        check_quant_supported(getattr(args, "quant", None), type(self).__name__)
        assert args.vocab_size % t == 0 and args.n_kv_heads % t == 0 and args.head_dim == 128, "gqa_decode: head_dim 128"
        # the cache this decoder was handed must have the format its args name (gqa_kv_layout raises on an unknown name)
        # in both modes: a bf16 cache of another row shape or dtype used to fail at the first attention assert, it fails here now.
        # cache None is a decoder that only holds weights (checkpoint loading and conversion build one); it never attends.
        kv_shape, kv_dtype = gqa_kv_layout(args.kv_cache_dtype, args.n_kv_heads // t, args.head_dim)
        if cache is not None:
            got = [(tuple(c.shape[3:]), c.dtype) for c in (cache.paged_k_cache, cache.paged_v_cache)]
            if not all(g == (tuple(kv_shape), kv_dtype) for g in got):
                raise ValueError(
                    f"kv_cache_dtype={args.kv_cache_dtype!r} needs K and V caches of {tuple(kv_shape)} x {kv_dtype} per token, got {got}: build "
                    "the cache with PagedKVCacheManager(k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype), "
                    "(shape, dtype) = cache_manager.gqa_kv_layout(kv_cache_dtype, n_local_kv_heads)")
        self.vocab_local = args.vocab_size // t
        self.vocab_start = tp.get_tp_rank() * self.vocab_local
        self.embed_weight = _param(self.vocab_local, args.dim, device=device)
        block = self.block_type or LlamaBlock
        self.layers = torch.nn.ModuleList(block(i, args, cache, attn_backend, device) for i in range(args.n_layers))
        self.norm = _param(args.dim, device=device)
        self.head_weight = _param(self.vocab_local, args.dim, device=device)
        # rotary_dim: the channels of a head that rotate (GLM-4: 64 of 128); every other model has no such field
        cos, sin = precompute_freqs_cis(getattr(args, "rotary_dim", args.head_dim), max_position_embeddings, args.rope_theta)
        self.cos_table, self.sin_table = cos.to(device), sin.to(device)

    def final_norm(self):
        return self.norm, self.args.norm_eps

    def check_step(self, kind, rows=0):
        """Chunked and continued prefill attend over bf16 K / V pages (LlamaAttention.prefill_forward_paged).  A multi-token step
        of more rows than the xGMI communicator holds is not refused: its collectives take the library path."""
        if kind != "multi-token decode" and self.args.kv_cache_dtype == "fp8":
            raise NotImplementedError(f"{kind} attends over bf16 K / V pages; kv_cache_dtype='fp8' is not implemented")


@torch.no_grad()
def init_synthetic_(model: torch.nn.Module, seed: int = 0):
    """bf16 weights randn / sqrt(fan_in) (unit-gain linears), norm weights 1, embeddings randn."""
    dev = next(model.parameters()).device
    gen = torch.Generator(device=dev).manual_seed(seed)
    for name, p in model.named_parameters():
        if name.endswith("norm"):
            p.data.fill_(1.0)
            continue
        std = 1.0 if name == "embed_weight" else p.shape[-1] ** -0.5
        flat = p.data.view(-1)
        for i in range(0, flat.numel(), 1 << 26):
            n = min(1 << 26, flat.numel() - i)
            flat[i : i + n].copy_((torch.randn(n, device=dev, generator=gen) * std).to(p.dtype))
    return model
