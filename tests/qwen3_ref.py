"""The Qwen3 fixture (tests/golden/qwen3_hf.npz, made by tests/golden/gen_qwen3_hf.py from Hugging Face's Qwen3ForCausalLM), its
parameters regenerated from the seed, and a plain CPU restatement of this project's arithmetic for one sequence: bf16
activations and linears, the head norm in fp32 with one rounding, RoPE from the decoder's fp32 table, causal GQA in fp32.
No GPU needed."""

import ast
import os

import torch
import torch.nn.functional as F

from tests.row_exact import rope_oracle
from tests.util import golden

BF16 = torch.bfloat16
SEED = 8642  # gen_qwen3_hf.py::SEED


def fixture():
    g = golden("qwen3_hf")
    return g, ast.literal_eval(str(g["cfg"][0]))


def qwen3_hf_params(g):
    """HF name -> bf16 tensor: gen_qwen3_hf.py::fill (keep in sync) -- sorted-name order, one CPU generator."""
    gen = torch.Generator().manual_seed(SEED)
    out = {}
    for name, shape in zip(g["names"].tolist(), g["shapes"].tolist()):
        shape = ast.literal_eval(shape)
        if name.endswith("norm.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=gen, dtype=torch.float32)
        elif name.startswith("model.embed_tokens"):
            t = torch.randn(shape, generator=gen, dtype=torch.float32)
        else:
            t = torch.randn(shape, generator=gen, dtype=torch.float32) * shape[-1] ** -0.5
        out[name] = t.to(BF16)
    return out


def qwen3_args(cfg, **over):
    from chitu_amd.qwen3 import Qwen3Args

    kw = dict(dim=cfg["hidden_size"], n_layers=cfg["num_hidden_layers"], n_heads=cfg["num_attention_heads"],
              n_kv_heads=cfg["num_key_value_heads"], head_dim=cfg["head_dim"], vocab_size=cfg["vocab_size"],
              ffn_dim=cfg["intermediate_size"], norm_eps=cfg["rms_norm_eps"], rope_theta=cfg["rope_theta"],
              tie_word_embeddings=cfg["tie_word_embeddings"])
    kw.update(over)
    return Qwen3Args(**kw)


def module_params(hf, args):
    """HF names -> Qwen3Decoder parameter names through the product loader's own steps."""
    from chitu_amd.checkpoint import preprocess_hf_llama, to_llama_module_names

    return to_llama_module_names(preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim, head_dim=args.head_dim))


def write_hf_dir(hf, path):
    """The parameters as a Hugging Face safetensors directory."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    save_file({k: v.contiguous() for k, v in hf.items()}, os.path.join(path, "model.safetensors"))
    return path


def rms_norm(x, w, eps):
    """fp32 statistics and products, one rounding to bf16 (norm.hip's statement)."""
    xf = x.float()
    rr = torch.rsqrt((xf * xf).mean(-1, keepdim=True) + eps)
    return ((xf * rr) * w.float()).to(BF16)


def forward(p, tokens, args, max_pos=512):
    """One sequence, all positions at once -> (fp32 logits [T, vocab], layer 0's k rows after norm + RoPE [T, hkv, 128] bf16)."""
    from chitu_amd.llama import precompute_freqs_cis

    T, hq, hkv, hd, eps = len(tokens), args.n_heads, args.n_kv_heads, args.head_dim, args.norm_eps
    cos_t, sin_t = precompute_freqs_cis(hd, max_pos, args.rope_theta)
    cos, sin = cos_t[:T].contiguous(), sin_t[:T].contiguous()
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    x = p["embed_weight"][torch.tensor(tokens)]
    k0 = None
    for i in range(args.n_layers):
        pre = f"layers.{i}."
        qkv = F.linear(rms_norm(x, p[pre + "attn_norm"], eps), p[pre + "attn.wqkv"]).view(T, hq + 2 * hkv, hd)
        q = rope_oracle(rms_norm(qkv[:, :hq], p[pre + "attn.q_norm"], eps), cos, sin, 1)
        k = rope_oracle(rms_norm(qkv[:, hq:hq + hkv], p[pre + "attn.k_norm"], eps), cos, sin, 1)
        v = qkv[:, hq + hkv:]
        if i == 0:
            k0 = k
        kf, vf = (t.float().repeat_interleave(hq // hkv, dim=1) for t in (k, v))
        s = torch.einsum("thd,shd->hts", q.float(), kf) * hd ** -0.5
        s = s.masked_fill(~causal[None], float("-inf")).softmax(-1)
        o = torch.einsum("hts,shd->thd", s, vf).to(BF16)
        x = x + F.linear(o.reshape(T, hq * hd), p[pre + "attn.wo"])
        h13 = F.linear(rms_norm(x, p[pre + "ffn_norm"], eps), p[pre + "ffn.w13"])
        d = h13.shape[-1] // 2
        x = x + F.linear(F.silu(h13[:, :d]) * h13[:, d:], p[pre + "ffn.w2"])
    return F.linear(rms_norm(x, p["norm"], eps), p["head_weight"]).float(), k0


def logits_error(mine, ref):
    """tests/test_llama_reference.py's statistic: per row max |mine - ref| / max |ref|; returns (worst, per row)."""
    per_row = (mine - ref).abs().amax(-1) / ref.abs().amax(-1)
    return per_row.max().item(), per_row


def check_logits(mine, g, what):
    """The bar of tests/test_llama_reference.py against the fp32 run: every row within 2e-2; the greedy token agrees on every
    step whose top-2 margin in the fixture exceeds twice the observed error, and on at least 31 of the 33 steps."""
    ref = torch.from_numpy(g["logits_fp32"])
    assert mine.shape == ref.shape, (mine.shape, ref.shape)
    err, per_row = logits_error(mine, ref)
    print(f"QWEN3 {what}: {err:.3e}")
    assert err < 2e-2, (what, err, (per_row >= 2e-2).nonzero().flatten().tolist())
    top2 = ref.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * err * ref.abs().amax(-1)
    agree = mine.argmax(-1) == torch.from_numpy(g["tokens"])
    assert bool(agree[clear].all()) and int(agree.sum()) >= 31, (what, int(clear.sum()), int(agree.sum()))
    return err, int(agree.sum())
