"""Qwen3-MoE models (Qwen3-30B-A3B, Qwen3-235B-A22B) on the Llama-family decode path.

A Qwen3-MoE block is a Qwen3 attention (per-head q / k RMSNorm, half-split RoPE, decoupled head_dim, no biases: LlamaAttention
with qk_norm, chitu_amd/qwen3.py) in front of a sparse MoE: a bf16 router over all experts -- softmax, top-k, renormalised when
norm_topk_prob -- and bf16 SwiGLU experts of width moe_intermediate_size, no shared expert.  The reference has no such model.
Router: ops.gate_deepseek_v3 with one group ("softmax_renorm", or "softmax" when norm_topk_prob is off).  Experts:
fused_moe.fused_experts on bf16 weights -- the 16-slot streaming GEMMs for decode, the tiled grouped GEMMs
(csrc/moe_bf16_tiled.hip) from TILED_MIN_TOKENS prompt tokens on.  Every rank holds all experts at 1 / tp of their width.
Everything else -- prefill, prefill_continue, decode, decode_multi, generate*, kv_cache_dtype="fp8", sliding_window, hipGraph
capture -- is LlamaDecoder's.
"""

import os
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from . import fused_moe, ops
from . import tensor_parallel as tp
from .deepseek_v3 import _route_align_enabled
from .llama import GqaBlock, LlamaDecoder, _param

# Prompt tokens from which the experts take the tiled grouped GEMMs (0 = never; fused_moe._takes_tiled's per-expert floor
# applies as well: 24 slots per expert, i.e. 384 tokens at 128 experts / top 8).  Measured on an MI355X at Qwen3-30B-A3B's shapes
# (E = 128, top 8, K = 2048, I = 768; tools/moe_bf16_ab.py, profiles/moe_bf16_tiled_ab.json), us per layer,
# streaming / tiled: 128 tokens 249 / 253, 256: 332 / 258, 384: 432 / 262, 512: 520 / 268, 1024: 878 / 288, 2048: 1561 / 388,
# 8192: 5639 / 985 -- 256 is the smallest measured count from which the tiled form wins at every larger one.
TILED_MIN_TOKENS = int(os.environ.get("CHITU_QWEN3_MOE_TILED_MIN_TOKENS", "256"))


@dataclass
class Qwen3MoeArgs:
    """Fields of a Hugging Face Qwen3MoeConfig under this package's names (defaults = Qwen3-30B-A3B)."""

    dim: int = 2048
    n_layers: int = 48
    n_heads: int = 32
    n_kv_heads: int = 4
    head_dim: int = 128
    vocab_size: int = 151936
    moe_inter_dim: int = 768  # moe_intermediate_size: the width of every expert
    num_experts: int = 128
    num_experts_per_tok: int = 8
    norm_topk_prob: bool = True
    norm_eps: float = 1e-6
    rope_theta: float = 1000000.0
    kv_cache_dtype: str = "bf16"  # "fp8": see LlamaArgs.kv_cache_dtype
    sliding_window: Optional[int] = None  # see LlamaArgs.sliding_window
    attn_softcap: float = 0.0  # see LlamaArgs.attn_softcap
    qk_norm: bool = True
    tie_word_embeddings: bool = False
    mlp_only_layers: List[int] = field(default_factory=list)  # dense layers: none in any published size, refused
    decoder_sparse_step: int = 1  # every layer is sparse in every published size; anything else is refused
    quant: Optional[str] = None  # the experts are bf16; LlamaArgs' "w8a16" (dense linears) is refused here

    def __post_init__(self):
        if self.quant is not None:
            raise ValueError(f"Qwen3MoeArgs: quant={self.quant!r} is not supported ('w8a16' covers the dense Llama-family decoders; "
                             "W8A16 experts are not built)")


def check_args(args: Qwen3MoeArgs, tp_size: int = 1) -> None:
    """What this path does not build is refused when the model is built, not when it first runs."""
    if list(args.mlp_only_layers):
        raise ValueError(f"mlp_only_layers={list(args.mlp_only_layers)}: dense layers inside a Qwen3-MoE model are not built")
    if args.decoder_sparse_step != 1:
        raise ValueError(f"decoder_sparse_step={args.decoder_sparse_step}: only models whose every layer is sparse (1) are built")
    if args.moe_inter_dim % tp_size != 0 or (args.moe_inter_dim // tp_size) % 128 != 0:
        raise ValueError(f"moe_inter_dim={args.moe_inter_dim} over {tp_size} ranks: the expert GEMMs need a rank's share of the "
                         "expert width to be a multiple of 128")


class Qwen3MoeSparseMoe(torch.nn.Module):
    """Router + bf16 experts.  gate [E, dim]; w13 [E, 2 I / tp, dim] (gate rows, then up rows: Hugging Face's fused
    gate_up_proj order); w2 [E, dim, I / tp]."""

    def __init__(self, args: Qwen3MoeArgs, device=None):
        super().__init__()
        t = tp.get_tp_size()
        check_args(args, t)
        self.E, self.topk, self.inter = args.num_experts, args.num_experts_per_tok, args.moe_inter_dim // t
        self.score_func = "softmax_renorm" if args.norm_topk_prob else "softmax"
        self.gate = _param(self.E, args.dim, device=device)
        self.w13 = _param(self.E, 2 * self.inter, args.dim, device=device)
        self.w2 = _param(self.E, args.dim, self.inter, device=device)
        self.tiled_min_tokens = TILED_MIN_TOKENS
        # test hook (eager launches only): a list collects (x, router_logits, ids, weights) of every call
        self.record_routing = None

    def forward(self, x, defer_sum: bool = False):
        """x: ffn_norm output bf16 [tokens, dim].  defer_sum: return the un-summed [tokens, topk, dim] expert outputs for a
        consumer that folds the top-k sum into its residual add."""
        # decode-sized batches: moe_align runs inside the routing launch, as in MixtralSparseMoe
        align = (self.E, fused_moe._MOE_BLOCK_M, None) if _route_align_enabled(x.shape[0]) else None
        partials = None
        if self.record_routing is not None:
            # the bf16 logits as one fp32 plane: the routing kernel's logit is the plane sum rounded to bf16, i.e. these values
            logits = ops.bf16_linear(x, self.gate)
            partials = logits.float().unsqueeze(0).contiguous()
        routed = ops.gate_deepseek_v3(x, self.gate, None, 1, 1, self.topk, self.score_func, 1.0, align=align,
                                      logits_partials=partials)
        if self.record_routing is not None:
            self.record_routing.append((x.clone(), logits.clone(), routed[1].clone(), routed[0].clone()))
        return fused_moe.fused_experts(x, self.w13, self.w2, routed[0], routed[1], inplace=True, global_num_experts=self.E,
                                       aligned=routed[2] if len(routed) > 2 else None, reduce_topk=not defer_sum,
                                       bf16_tiled_min_tokens=self.tiled_min_tokens)


class Qwen3MoeBlock(GqaBlock):
    rotary_type = "hf-llama"
    ffn_type = Qwen3MoeSparseMoe

    def forward(self, x, pending, cos, sin, varlens=None, q_len=1):
        # the prologue of the qkv projection takes a summed pending only: un-summed expert outputs go to the norm launch, which
        # sums up to 16 terms
        x, a = self.attn_part(x, pending, cos, sin, varlens, q_len)
        x, hn = tp.add_norm(x, a, self.ffn_norm, self.eps)[:2]
        # decode: the top-k sum moves into the next residual add whenever nothing else needs the summed tensor
        defer = varlens is None and x.is_cuda and tp.defers_topk_sum(hn.shape[0], hn.shape[1], self.ffn.topk)
        return x, tp.defer_all_reduce(self.ffn(hn, defer_sum=defer))


class Qwen3MoeDecoder(LlamaDecoder):
    """LlamaDecoder (embed, norm, head, hipGraph decode, prefill, generate) over Qwen3MoeBlocks."""

    block_type = Qwen3MoeBlock

    def __init__(self, args: Qwen3MoeArgs, cache, attn_backend, max_position_embeddings: int = 4096, device="cuda"):
        check_args(args, tp.get_tp_size())
        super().__init__(args, cache, attn_backend, max_position_embeddings, device)
