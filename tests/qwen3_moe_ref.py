"""The Qwen3-MoE fixture (tests/golden/qwen3_moe_hf.npz, made by tests/golden/gen_qwen3_moe_hf.py from Hugging Face's
Qwen3MoeForCausalLM), its parameters regenerated from the stored seed, the same parameters under the published per-expert
on-disk names, and an fp32 CPU restatement of the model for one sequence with an optional `route_ids` argument: the experts of
every (layer, token) are then the given ones, weighted by the restatement's own softmax over them -- the reference a bf16 run
can be held against, since near-tied experts flip under free routing.  No GPU needed."""

import ast
import os

import torch
import torch.nn.functional as F

from tests.qwen3_ref import logits_error
from tests.util import golden

BF16 = torch.bfloat16


def fixture():
    g = golden("qwen3_moe_hf")
    return g, ast.literal_eval(str(g["cfg"][0]))


def hf_params(g):
    """HF module name -> bf16 tensor: gen_qwen3_hf.py::fill with the fixture's seed -- sorted-name order, one CPU generator.
    The experts come fused, as the module holds them: mlp.experts.gate_up_proj [E, 2I, H], mlp.experts.down_proj [E, H, I]."""
    gen = torch.Generator().manual_seed(int(g["seed"][0]))
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


def on_disk_names(hf):
    """The published checkpoints' layout: mlp.experts.E.{gate,up,down}_proj.weight per expert (gate = the first I rows of the
    fused gate_up_proj, up = the rest); every other tensor under its module name."""
    out = {}
    for k, v in hf.items():
        if k.endswith(".mlp.experts.gate_up_proj"):
            pre, I = k[: -len("gate_up_proj")], v.shape[1] // 2
            for e in range(v.shape[0]):
                out[f"{pre}{e}.gate_proj.weight"] = v[e, :I].clone()
                out[f"{pre}{e}.up_proj.weight"] = v[e, I:].clone()
        elif k.endswith(".mlp.experts.down_proj"):
            pre = k[: -len("down_proj")]
            for e in range(v.shape[0]):
                out[f"{pre}{e}.down_proj.weight"] = v[e].clone()
        else:
            out[k] = v
    return out


def moe_args(cfg, **over):
    from chitu_amd.qwen3_moe import Qwen3MoeArgs

    kw = dict(dim=cfg["hidden_size"], n_layers=cfg["num_hidden_layers"], n_heads=cfg["num_attention_heads"],
              n_kv_heads=cfg["num_key_value_heads"], head_dim=cfg["head_dim"], vocab_size=cfg["vocab_size"],
              moe_inter_dim=cfg["moe_intermediate_size"], num_experts=cfg["num_experts"],
              num_experts_per_tok=cfg["num_experts_per_tok"], norm_topk_prob=cfg["norm_topk_prob"], norm_eps=cfg["rms_norm_eps"],
              rope_theta=cfg["rope_theta"], tie_word_embeddings=cfg["tie_word_embeddings"])
    kw.update(over)
    return Qwen3MoeArgs(**kw)


def module_params(hf, args, rank=0, world=1):
    """HF names -> Qwen3MoeDecoder parameter names through the product loader's own steps."""
    from chitu_amd.checkpoint import preprocess_hf_qwen3_moe

    return preprocess_hf_qwen3_moe(on_disk_names(hf), args, rank, world)


def write_hf_dir(hf, path):
    """The parameters as a Hugging Face safetensors directory under the on-disk names."""
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    save_file({k: v.contiguous() for k, v in on_disk_names(hf).items()}, os.path.join(path, "model.safetensors"))
    return path


def _rms(x, w, eps):
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w


def _rope(x, cos, sin):
    """Half split: x [T, h, d], cos / sin [T, d]."""
    d = x.shape[-1] // 2
    rot = torch.cat([-x[..., d:], x[..., :d]], dim=-1)
    return x * cos[:, None] + rot * sin[:, None]


def forward(hf, tokens, cfg, route_ids=None):
    """One sequence, all positions at once, fp32 throughout -> (logits [T, vocab], router logits [layers, T, E], router ids
    [layers, T, top_k]).  route_ids [layers, T, top_k] (any integer tensor): use these experts instead of the top-k."""
    p = {k: v.float() for k, v in hf.items()}
    T, hq, hkv, hd = len(tokens), cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    eps, top_k = cfg["rms_norm_eps"], cfg["num_experts_per_tok"]
    inv = 1.0 / cfg["rope_theta"] ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd)
    ang = torch.arange(T, dtype=torch.float32)[:, None] * inv[None]
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    x = p["model.embed_tokens.weight"][torch.tensor(tokens)]
    all_logits, all_ids = [], []
    for i in range(cfg["num_hidden_layers"]):
        pre = f"model.layers.{i}."
        h = _rms(x, p[pre + "input_layernorm.weight"], eps)
        q = F.linear(h, p[pre + "self_attn.q_proj.weight"]).view(T, hq, hd)
        k = F.linear(h, p[pre + "self_attn.k_proj.weight"]).view(T, hkv, hd)
        v = F.linear(h, p[pre + "self_attn.v_proj.weight"]).view(T, hkv, hd)
        q = _rope(_rms(q, p[pre + "self_attn.q_norm.weight"], eps), cos, sin)
        k = _rope(_rms(k, p[pre + "self_attn.k_norm.weight"], eps), cos, sin)
        kf, vf = k.repeat_interleave(hq // hkv, dim=1), v.repeat_interleave(hq // hkv, dim=1)
        s = torch.einsum("thd,shd->hts", q, kf) * hd ** -0.5
        s = s.masked_fill(~causal[None], float("-inf")).softmax(-1)
        o = torch.einsum("hts,shd->thd", s, vf).reshape(T, hq * hd)
        x = x + F.linear(o, p[pre + "self_attn.o_proj.weight"])
        h = _rms(x, p[pre + "post_attention_layernorm.weight"], eps)
        logits = F.linear(h, p[pre + "mlp.gate.weight"])
        probs = logits.softmax(-1)
        ids = probs.topk(top_k, -1).indices if route_ids is None else torch.as_tensor(route_ids[i]).long()
        w = probs.gather(-1, ids)
        if cfg["norm_topk_prob"]:
            w = w / w.sum(-1, keepdim=True)
        w13, w2 = p[pre + "mlp.experts.gate_up_proj"], p[pre + "mlp.experts.down_proj"]
        y = torch.zeros_like(x)
        for t in range(T):
            for j in range(top_k):
                e = int(ids[t, j])
                gu = w13[e] @ h[t]
                d = gu.shape[0] // 2
                y[t] += w[t, j] * (w2[e] @ (F.silu(gu[:d]) * gu[d:]))
        x = x + y
        all_logits.append(logits)
        all_ids.append(ids)
    out = F.linear(_rms(x, p["model.norm.weight"], eps), p["lm_head.weight"])
    return out, torch.stack(all_logits), torch.stack(all_ids)


def check_logits(mine, ref, what, tokens=None):
    """tests/qwen3_ref.py::check_logits' bar against fp32 logits `ref`: every row within 2e-2 of its peak; the greedy token
    agrees (with `tokens`, default ref's own arg-max) on every row whose top-2 margin in ref exceeds twice the observed error,
    and on all but at most two rows."""
    ref = torch.as_tensor(ref).float()
    assert mine.shape == ref.shape, (mine.shape, ref.shape)
    err, per_row = logits_error(mine.float(), ref)
    print(f"QWEN3-MOE {what}: {err:.3e}")
    assert err < 2e-2, (what, err, (per_row >= 2e-2).nonzero().flatten().tolist())
    top2 = ref.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * err * ref.abs().amax(-1)
    agree = mine.argmax(-1) == (ref.argmax(-1) if tokens is None else torch.as_tensor(tokens))
    assert bool(agree[clear].all()) and int(agree.sum()) >= ref.shape[0] - 2, (what, int(clear.sum()), int(agree.sum()))
    return err, int(agree.sum())
