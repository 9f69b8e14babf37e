"""GLM-4-9B (glm-4-9b-chat) on the Llama-family decode path.

The reference serves glm-4-9b-chat as `type: hf-llama` with rotary_type "glm4" (backend.py:74-75).  Against a Qwen2 block -- a
q / k / v projection bias (LlamaAttention.bqkv), a SwiGLU MLP shipped merged, no other bias -- the rotation is the one
difference: only the first rotary_dim = 64 channels of every 128-channel head rotate, as interleaved (re, im) pairs over 32
frequencies (the decoder's cos / sin table is precompute_freqs_cis(64, ...): [positions, 32]); channels 64..127 pass through.
That is Hugging Face's modeling_glm.apply_rotary_pos_emb, the arithmetic the published weights were trained with, and NOT the
reference's torch branch (docs/design/4_parity.md records the difference).  The rotary width rides in the launches that already
add the bias: ops.gqa_qkv_bias_post[_kv_fp8] on the decode path and ops.qkv_bias_rope over the whole prompt, through
include/chitu_hip_ext7.h (csrc/qkv_post_row16.hip states the lane rule).

What runs: glm-4-9b-chat (32 / 2 heads, G = 16) at TP 1 and 2 only -- the 2 kv heads are not replicated over more ranks.  Both
checkpoint namings load: the ChatGLM remote-code names (`transformer.encoder.layers.N.self_attention.query_key_value` ...,
checkpoint.map_glm4_names) and Hugging Face's native GlmForCausalLM names (glm-4-9b-chat-hf).  Everything else -- prefill,
prefill_continue, chunked prefill, decode, decode_multi, generate*, kv_cache_dtype="fp8", quant="w8a16", hipGraph capture -- is
LlamaDecoder's.

What does not run: GLM-4-0414 (`Glm4ForCausalLM`, with its extra post-attention and post-MLP norms); the rope settings of
glm-4-9b-chat-1m beyond a different rope_theta; the vision model (glm-4v-9b).
"""

from dataclasses import dataclass
from typing import Optional

from .llama import LlamaBlock, LlamaDecoder


@dataclass
class Glm4Args:
    """Fields of chitu/config/models/glm-4-9b-chat.yaml under LlamaArgs' names (defaults = glm-4-9b-chat)."""

    dim: int = 4096
    n_layers: int = 40
    n_heads: int = 32
    n_kv_heads: int = 2
    vocab_size: int = 151552
    ffn_dim: int = 13696
    norm_eps: float = 1.5625e-07
    rope_theta: float = 5000000.0
    kv_cache_dtype: str = "bf16"
    sliding_window: Optional[int] = None
    attn_softcap: float = 0.0
    qkv_bias: bool = True
    rotary_dim: int = 64  # partial_rotary_factor 0.5 of head_dim 128: the channels of a head that rotate
    tie_word_embeddings: bool = False
    quant: Optional[str] = None  # "w8a16": int8 wqkv / wo / w13 / w2 (LlamaArgs.quant)

    @property
    def head_dim(self):
        return self.dim // self.n_heads


class Glm4Block(LlamaBlock):
    rotary_type = "glm4"


class Glm4Decoder(LlamaDecoder):
    block_type = Glm4Block
