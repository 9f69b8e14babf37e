"""Golden fixture for the GLM-4 dense path: Hugging Face's own GlmForCausalLM (transformers, CPU) at a test size -- 4 query heads
over 2 kv heads of 128, hidden 512, partial_rotary_factor 0.5 (the first 64 channels of a head rotate, as interleaved pairs), a
bias on the q / k / v projections and on nothing else, the MLP's gate | up shipped merged, an untied head.

Run on a CPU machine with transformers installed (nothing is downloaded):   python tests/golden/gen_glm4_hf.py
Writes tests/golden/glm4_hf.npz in tests/golden/gen_qwen2_hf.py's layout: the prompt, the 33 greedy tokens of the fp32 run, the
logits [33, vocab] of the prompt's last token and of 32 teacher-forced steps from an fp32 run and from a bf16 run of the same
model on the same tokens, the (name, shape) list of the parameters in sorted-name order, layer 0's k rows after bias + RoPE and its
v rows after the bias [39, 2, 128] from the fp32 run.  Parameter VALUES are not stored: tests/glm4_ref.py::glm4_hf_params
regenerates them from the same seed in the same order (`fill` below, keep in sync).

The seed is chosen so that a bf16 implementation can meet the project's bar: Hugging Face's own bf16 run picks the fp32 run's
token on all 33 rows (asserted below).
"""

import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = dict(hidden_size=512, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
           vocab_size=512, partial_rotary_factor=0.5, attention_bias=True, rms_norm_eps=1.5625e-07, rope_theta=5e6,
           tie_word_embeddings=False, pad_token_id=0)
PROMPT = [5, 17, 400, 33, 2, 41, 7]
NEW_TOKENS = 32
SEED = 8647


def fill(named, seed=SEED):
    """gen_qwen2_hf.py's recipe: sorted-name order, one CPU generator, every value rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    for n, p in named:
        if n.endswith("norm.weight"):
            t = 1.0 + 0.1 * torch.randn(p.shape, generator=g, dtype=torch.float32)
        elif n.startswith("model.embed_tokens"):
            t = torch.randn(p.shape, generator=g, dtype=torch.float32)
        elif n.endswith(".bias"):
            t = 0.5 * torch.randn(p.shape, generator=g, dtype=torch.float32)
        else:
            t = torch.randn(p.shape, generator=g, dtype=torch.float32) * p.shape[-1] ** -0.5
        p.data.copy_(t.to(torch.bfloat16).to(p.dtype))


def logits_error(mine, ref):
    per_row = (mine - ref).abs().amax(-1) / ref.abs().amax(-1)
    return per_row.max().item()


def main():
    import transformers.models.glm.modeling_glm as mg
    from transformers import GlmConfig, GlmForCausalLM

    cfg = GlmConfig(**CFG)
    cfg._attn_implementation = "eager"
    model = GlmForCausalLM(cfg).float().eval()
    named = sorted(model.named_parameters(), key=lambda kv: kv[0])
    assert sorted(n for n, _ in named if n.endswith(".bias")) == sorted(
        f"model.layers.{i}.self_attn.{x}_proj.bias" for i in range(CFG["num_hidden_layers"]) for x in "qkv")
    assert tuple(model.model.rotary_emb.inv_freq.shape) == (32,)  # 64 of the 128 channels rotate
    fill(named)

    k_rows, v_rows = [], []
    real_rope = mg.apply_rotary_pos_emb

    def recording_rope(q, k, cos, sin, *a, **kw):
        oq, ok = real_rope(q, k, cos, sin, *a, **kw)
        k_rows.append(ok.detach().clone())  # [1, hkv, T, 128], one call per layer in layer order
        return oq, ok

    mg.apply_rotary_pos_emb = recording_rope
    model.model.layers[0].self_attn.v_proj.register_forward_hook(lambda m, i, o: v_rows.append(o.detach().clone()))  # [1, T, hkv * 128]

    def logits_of(m, seq):
        with torch.inference_mode():
            return m(input_ids=torch.tensor([seq]), use_cache=False).logits[0].float()

    seq = list(PROMPT)
    toks = []
    for _ in range(NEW_TOKENS + 1):  # greedy, the whole sequence again every step (no cache: nothing but the model's forward)
        toks.append(int(logits_of(model, seq)[-1].argmax()))
        seq.append(toks[-1])
    fed = PROMPT + toks[:-1]  # teacher forcing: row i predicts the token after fed[i]
    k_rows.clear(), v_rows.clear()
    l32 = logits_of(model, fed)[len(PROMPT) - 1:]
    k0 = k_rows[0][0].transpose(0, 1).contiguous()  # layer 0: [T, hkv, 128]
    v0 = v_rows[0][0].view(len(fed), CFG["num_key_value_heads"], 128).contiguous()
    assert l32.argmax(-1).tolist() == toks

    model16 = model.to(torch.bfloat16)
    l16 = logits_of(model16, fed)[len(PROMPT) - 1:]
    agree = int((l16.argmax(-1) == l32.argmax(-1)).sum())
    top2 = l32.topk(2, -1).values
    margin = ((top2[:, 0] - top2[:, 1]) / l32.abs().amax(-1)).min().item()
    print("seed", SEED, "tokens", toks[:16], "...", "distinct", len(set(toks)), "bf16 greedy agreement", agree, "/", len(toks),
          f"bf16 vs fp32 {logits_error(l16, l32):.2e}, smallest top-2 margin {margin:.2e}")
    assert agree == len(toks) == 33
    np.savez_compressed(
        os.path.join(HERE, "glm4_hf.npz"), prompt=np.array(PROMPT), tokens=np.array(toks), logits_fp32=l32.numpy(),
        logits_bf16=l16.numpy(), names=np.array([n for n, _ in named]), shapes=np.array([str(tuple(p.shape)) for _, p in named]),
        k0_fp32=k0.float().numpy(), v0_fp32=v0.float().numpy(), cfg=np.array([repr(CFG)]))


if __name__ == "__main__":
    main()
