"""The GLM-4 fixture (tests/golden/glm4_hf.npz, made by tests/golden/gen_glm4_hf.py from Hugging Face's GlmForCausalLM), its
parameters regenerated from the seed, and a plain CPU restatement of this project's arithmetic for one sequence: tests/
qwen2_ref.py's, with tests/glm4_exact.py::rotate_partial -- interleaved pairs over the first rotary_dim channels, the rest passed
through -- as its rotation.  The bar against the fixture is tests/qwen3_ref.py::check_logits.  No GPU needed."""

import ast

import torch
import torch.nn.functional as F

from tests.glm4_exact import rotate_partial
from tests.qwen3_ref import BF16, check_logits, logits_error, rms_norm, write_hf_dir  # noqa: F401
from tests.row_exact import rope_oracle
from tests.util import golden

SEED = 8647  # gen_glm4_hf.py::SEED
LOGITS_BAR = 2e-2  # check_logits' bar on every row


def fixture():
    g = golden("glm4_hf")
    return g, ast.literal_eval(str(g["cfg"][0]))


def glm4_hf_params(g):
    """HF name (GlmForCausalLM's) -> bf16 tensor: gen_glm4_hf.py::fill (keep in sync) -- sorted-name order, one CPU generator."""
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


def chatglm_names(hf):
    """The same parameters under the key names of glm-4-9b-chat's remote-code files: q | k | v merged into query_key_value
    (weight and bias), gate | up already merged, plus the rotary module's inv_freq buffer the loader has to drop."""
    out = {"transformer.rotary_pos_emb.inv_freq": torch.zeros(32, dtype=BF16)}
    simple = {"model.embed_tokens.": "transformer.embedding.word_embeddings.", "model.norm.": "transformer.encoder.final_layernorm.",
              "lm_head.": "transformer.output_layer."}
    inner = {".self_attn.o_proj.": ".self_attention.dense.", ".mlp.gate_up_proj.": ".mlp.dense_h_to_4h.",
             ".mlp.down_proj.": ".mlp.dense_4h_to_h."}
    for k, v in hf.items():
        for a, b in simple.items():
            if k.startswith(a):
                out[b + k[len(a):]] = v
                break
        else:
            assert k.startswith("model.layers."), k
            k2 = "transformer.encoder.layers." + k[len("model.layers."):]
            if ".self_attn.q_proj." in k:
                kind = k.rsplit(".", 1)[1]
                parts = [hf[k.replace(".q_proj.", f".{x}_proj.")] for x in "qkv"]
                out[k2.replace(".self_attn.q_proj." + kind, ".self_attention.query_key_value." + kind)] = torch.cat(parts, dim=0)
            elif ".self_attn.k_proj." in k or ".self_attn.v_proj." in k:
                continue
            else:
                for a, b in inner.items():
                    k2 = k2.replace(a, b)
                out[k2] = v
    return out


def glm4_args(cfg, **over):
    from chitu_amd.glm4 import Glm4Args

    kw = dict(dim=cfg["hidden_size"], n_layers=cfg["num_hidden_layers"], n_heads=cfg["num_attention_heads"],
              n_kv_heads=cfg["num_key_value_heads"], vocab_size=cfg["vocab_size"], ffn_dim=cfg["intermediate_size"],
              norm_eps=cfg["rms_norm_eps"], rope_theta=cfg["rope_theta"], tie_word_embeddings=cfg["tie_word_embeddings"],
              rotary_dim=int(cfg["head_dim"] * cfg["partial_rotary_factor"]))
    kw.update(over)
    return Glm4Args(**kw)


def module_params(hf, args):
    """HF names -> Glm4Decoder parameter names through the product loader's own steps."""
    from chitu_amd.checkpoint import preprocess_hf_llama, to_llama_module_names

    return to_llama_module_names(preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim, head_dim=args.head_dim), qkv_bias=True)


def forward(p, tokens, args, max_pos=512, rotation="glm4"):
    """One sequence, all positions at once -> (fp32 logits [T, vocab], layer 0's k rows after bias + RoPE and its v rows after
    the bias, [T, hkv, 128] bf16 each).  rotation: "glm4" the model's; "none": the first rotary_dim channels pass through as well;
    "full": all 128 channels rotate as interleaved pairs (a table of width head_dim) -- two implementations the fixture has to
    tell from the model's."""
    from chitu_amd.llama import precompute_freqs_cis

    T, hq, hkv, hd, eps = len(tokens), args.n_heads, args.n_kv_heads, args.head_dim, args.norm_eps
    cos_t, sin_t = precompute_freqs_cis(hd if rotation == "full" else args.rotary_dim, max_pos, args.rope_theta)
    cos, sin = cos_t[:T].contiguous(), sin_t[:T].contiguous()
    rotate = {"glm4": lambda y: rotate_partial(y.contiguous(), cos, sin), "none": lambda y: y,
              "full": lambda y: rope_oracle(y.contiguous(), cos, sin, 0)}[rotation]
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    x = p["embed_weight"][torch.tensor(tokens)]
    k0 = v0 = None
    for i in range(args.n_layers):
        pre = f"layers.{i}."
        qkv = F.linear(rms_norm(x, p[pre + "attn_norm"], eps), p[pre + "attn.wqkv"])
        qkv = (qkv + p[pre + "attn.bqkv"]).view(T, hq + 2 * hkv, hd)  # bf16 + bf16: an fp32 add, one rounding
        q, k = rotate(qkv[:, :hq]), rotate(qkv[:, hq:hq + hkv])
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
