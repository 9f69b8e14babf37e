"""The Qwen2 fixture (tests/golden/qwen2_hf.npz, made by tests/golden/gen_qwen2_hf.py from Hugging Face's Qwen2ForCausalLM), its
parameters regenerated from the seed, and a plain CPU restatement of this project's arithmetic for one sequence: tests/
qwen3_ref.py's, with the q / k / v bias added to the bf16 projection (one rounding, csrc/qkv_post_row16.hip's statement) in place of
the head norm.  The bar against the fixture is tests/qwen3_ref.py::check_logits.  No GPU needed."""

import ast

import torch
import torch.nn.functional as F

from tests.qwen3_ref import BF16, check_logits, logits_error, rms_norm, write_hf_dir  # noqa: F401
from tests.row_exact import rope_oracle
from tests.util import golden

SEED = 8644  # gen_qwen2_hf.py::SEED
LOGITS_BAR = 2e-2  # check_logits' bar on every row


def fixture():
    g = golden("qwen2_hf")
    return g, ast.literal_eval(str(g["cfg"][0]))


def qwen2_hf_params(g):
    """HF name -> bf16 tensor: gen_qwen2_hf.py::fill (keep in sync) -- sorted-name order, one CPU generator."""
    gen = torch.Generator().manual_seed(SEED)
    out = {}
    for name, shape in zip(g["names"].tolist(), g["shapes"].tolist()):
        shape = ast.literal_eval(shape)
        if name.endswith("norm.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=gen, dtype=torch.float32)
        elif name.startswith("model.embed_tokens"):
            t = torch.randn(shape, generator=gen, dtype=torch.float32)
        elif name.endswith(".bias"):
            t = 0.5 * torch.randn(shape, generator=gen, dtype=torch.float32)
        else:
            t = torch.randn(shape, generator=gen, dtype=torch.float32) * shape[-1] ** -0.5
        out[name] = t.to(BF16)
    return out


def qwen2_args(cfg, **over):
    from chitu_amd.qwen2 import Qwen2Args

    kw = dict(dim=cfg["hidden_size"], n_layers=cfg["num_hidden_layers"], n_heads=cfg["num_attention_heads"],
              n_kv_heads=cfg["num_key_value_heads"], vocab_size=cfg["vocab_size"], ffn_dim=cfg["intermediate_size"],
              norm_eps=cfg["rms_norm_eps"], rope_theta=cfg["rope_theta"], tie_word_embeddings=cfg["tie_word_embeddings"])
    kw.update(over)
    return Qwen2Args(**kw)


def module_params(hf, args):
    """HF names -> Qwen2Decoder parameter names through the product loader's own steps."""
    from chitu_amd.checkpoint import preprocess_hf_llama, to_llama_module_names

    return to_llama_module_names(preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim, head_dim=args.head_dim), qkv_bias=True)


def forward(p, tokens, args, max_pos=512, bias=True):
    """One sequence, all positions at once -> (fp32 logits [T, vocab], layer 0's k rows after bias + RoPE and its v rows after
    the bias, [T, hkv, 128] bf16 each).  bias=False: the same model with the bias dropped."""
    from chitu_amd.llama import precompute_freqs_cis

    T, hq, hkv, hd, eps = len(tokens), args.n_heads, args.n_kv_heads, args.head_dim, args.norm_eps
    cos_t, sin_t = precompute_freqs_cis(hd, max_pos, args.rope_theta)
    cos, sin = cos_t[:T].contiguous(), sin_t[:T].contiguous()
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    x = p["embed_weight"][torch.tensor(tokens)]
    k0 = v0 = None
    for i in range(args.n_layers):
        pre = f"layers.{i}."
        qkv = F.linear(rms_norm(x, p[pre + "attn_norm"], eps), p[pre + "attn.wqkv"])
        if bias:
            qkv = qkv + p[pre + "attn.bqkv"]  # bf16 + bf16: an fp32 add, one rounding
        qkv = qkv.view(T, hq + 2 * hkv, hd)
        q, k = rope_oracle(qkv[:, :hq], cos, sin, 1), rope_oracle(qkv[:, hq:hq + hkv], cos, sin, 1)
        v = qkv[:, hq + hkv:]
        if i == 0:
            k0, v0 = k, v
        kf, vf = (t.float().repeat_interleave(hq // hkv, dim=1) for t in (k, v))
        s = torch.einsum("thd,shd->hts", q.float(), kf) * hd ** -0.5
        s = s.masked_fill(~causal[None], float("-inf")).softmax(-1)
        o = torch.einsum("hts,shd->thd", s, vf).to(BF16)
        x = x + F.linear(o.reshape(T, hq * hd), p[pre + "attn.wo"])
        h13 = F.linear(rms_norm(x, p[pre + "ffn_norm"], eps), p[pre + "ffn.w13"])
        d = h13.shape[-1] // 2
        x = x + F.linear(F.silu(h13[:, :d]) * h13[:, d:], p[pre + "ffn.w2"])
    return F.linear(rms_norm(x, p["norm"], eps), p["head_weight"]).float(), k0, v0
