"""Qwen3 dense models (0.6B, 1.7B, 4B, 8B, 14B, 32B) on the Llama-family decode path.

Against a Llama block a Qwen3 block differs in three things, none of which the reference has (it has no Qwen3 model):
  * an RMSNorm with a learned [head_dim] weight on every q head and every k head, after the projection and before RoPE --
    LlamaAttention's qk_norm branch: one launch with the rotation and the K / V page append on the decode path
    (ops.gqa_qkv_norm_post[_kv_fp8]), one launch over the whole prompt in prefill (ops.qk_norm_rope);
  * head_dim is a field of the config, not dim // n_heads (Qwen3-4B: dim 2560, 32 heads of 128);
  * the small sizes tie the output head to the embedding (tie_word_embeddings: checkpoint.load_checkpoint_hf_llama fills
    the head from the embedding; the decoder keeps two parameters).
RoPE is half split ("hf-llama") and there is no qkv bias.  G = n_heads / n_kv_heads is 2, 2, 4, 4, 5, 8: the attention
kernels take every G (prefill at a G that is no power of two through include/chitu_hip_ext4.h).  Everything else -- prefill,
prefill_continue, decode, decode_multi, generate*, kv_cache_dtype="fp8", sliding_window, hipGraph capture -- is LlamaDecoder's.
"""

from dataclasses import dataclass
from typing import Optional

from .llama import LlamaBlock, LlamaDecoder


@dataclass
class Qwen3Args:
    """Fields of a Hugging Face Qwen3Config under LlamaArgs' names (defaults = Qwen3-8B)."""

    dim: int = 4096
    n_layers: int = 36
    n_heads: int = 32
    n_kv_heads: int = 8
    head_dim: int = 128
    vocab_size: int = 151936
    ffn_dim: int = 12288
    norm_eps: float = 1e-6
    rope_theta: float = 1000000.0
    kv_cache_dtype: str = "bf16"
    sliding_window: Optional[int] = None
    attn_softcap: float = 0.0
    qk_norm: bool = True
    tie_word_embeddings: bool = False
    quant: Optional[str] = None  # "w8a16": int8 wqkv / wo / w13 / w2 (LlamaArgs.quant)


class Qwen3Block(LlamaBlock):
    rotary_type = "hf-llama"


class Qwen3Decoder(LlamaDecoder):
    block_type = Qwen3Block
