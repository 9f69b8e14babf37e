"""Qwen2 / Qwen2.5 dense models and the DeepSeek-R1 distillations onto them, on the Llama-family decode path.

The reference serves Qwen2-7B-Instruct, Qwen2-72B-Instruct and DeepSeek-R1-Distill-Qwen-14B as `type: hf-llama` with a bias
on the q / k / v projections (model_hf_llama.py:56, qkv_has_bias defaults to true).  Against a Llama "hf-llama" block that bias
is the one difference: LlamaAttention's qkv_bias branch owns one merged row `bqkv` [(hq + 2 hkv) * 128] (column-parallel like
wqkv; checkpoint.load_checkpoint_hf_llama merges q_proj.bias | k_proj.bias | v_proj.bias per rank) and adds it in the launch
that already rotates q and k and appends k and v on the decode path (ops.gqa_qkv_bias_post[_kv_fp8]), and in one launch over
the whole prompt in prefill (ops.qkv_bias_rope: bias, RoPE and the contiguous v -- one launch fewer than a Llama prefill
layer).  The sum is rounded to bf16 before the rotation (csrc/qkv_post_row16.hip states the arithmetic).  o_proj and the MLP have
no bias.  RoPE is half split ("hf-llama").

Published sizes that run: Qwen2 / Qwen2.5 1.5B, 3B, 7B, 14B, 32B, 72B and DeepSeek-R1-Distill-Qwen 7B / 14B / 32B -- all
head_dim 128, with G = n_heads / n_kv_heads = 6, 8, 7, 5, 5, 8 (the attention kernels take every G; prefill at a G that is
no power of two through include/chitu_hip_ext4.h).  The small sizes tie the output head to the embedding
(tie_word_embeddings: the loader fills the head from the embedding).  Qwen2 / Qwen2.5 0.5B does not run: its head_dim is 64
and LlamaAttention refuses it.  Not covered: rope scaling / YaRN (the long-context configurations) and `use_sliding_window`
layer patterns (max_window_layers: a window on some layers only; sliding_window here is LlamaArgs' -- every layer or none).
Everything else -- prefill, prefill_continue, chunked prefill, decode, decode_multi, generate*, kv_cache_dtype="fp8",
hipGraph capture -- is LlamaDecoder's.
"""

from dataclasses import dataclass
from typing import Optional

from .llama import LlamaBlock, LlamaDecoder


@dataclass
class Qwen2Args:
    """Fields of chitu/config/models/Qwen2-7B-Instruct.yaml under LlamaArgs' names (defaults = Qwen2-7B / Qwen2.5-7B)."""

    dim: int = 3584
    n_layers: int = 28
    n_heads: int = 28
    n_kv_heads: int = 4
    vocab_size: int = 152064
    ffn_dim: int = 18944
    norm_eps: float = 1e-6
    rope_theta: float = 1000000.0
    kv_cache_dtype: str = "bf16"
    sliding_window: Optional[int] = None
    attn_softcap: float = 0.0
    qkv_bias: bool = True
    tie_word_embeddings: bool = False
    quant: Optional[str] = None  # "w8a16": int8 wqkv / wo / w13 / w2 (LlamaArgs.quant); the reference's shipped W8A16 model is Qwen2-7B

    @property
    def head_dim(self):
        return self.dim // self.n_heads


class Qwen2Block(LlamaBlock):
    rotary_type = "hf-llama"


class Qwen2Decoder(LlamaDecoder):
    block_type = Qwen2Block
