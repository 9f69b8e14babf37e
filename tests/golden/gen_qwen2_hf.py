"""Golden fixture for the Qwen2 dense path: Hugging Face's own Qwen2ForCausalLM (transformers, CPU) at a test size with
Qwen2.5-7B's head geometry at TP 4 -- 7 query heads over 1 kv head of 128 (G = 7, no power of two), hidden 896 -- a bias on the
q / k / v projections and on nothing else, half-split RoPE, an untied head.

Run on a CPU machine with transformers installed (nothing is downloaded):   python tests/golden/gen_qwen2_hf.py
Writes tests/golden/qwen2_hf.npz: the prompt, the 33 greedy tokens of the fp32 run, the logits [33, vocab] of the prompt's
last token and of 32 teacher-forced steps from an fp32 run and from a bf16 run of the same model on the same tokens, the
(name, shape) list of the parameters in sorted-name order, layer 0's k rows after bias + RoPE and its v rows after the bias
[39, 1, 128] from the fp32 run, and `no_bias_err`: the distance (tests/qwen3_ref.py::logits_error) of the same fp32 model
with every bias zeroed from the fp32 run -- what an implementation that dropped the bias would show.  Parameter VALUES are not
stored: tests/qwen2_ref.py::qwen2_hf_params regenerates them from the same seed in the same order (`fill` below, keep in sync).

The seed is chosen so that a bf16 implementation can meet the project's bar: Hugging Face's own bf16 run picks the fp32 run's
token on all 33 rows (asserted below).
"""

import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = dict(hidden_size=896, intermediate_size=512, num_hidden_layers=2, num_attention_heads=7, num_key_value_heads=1,
           vocab_size=512, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False, use_sliding_window=False)
PROMPT = [5, 17, 400, 33, 2, 41, 7]
NEW_TOKENS = 32
SEED = 8644


def fill(named, seed=SEED):
    """gen_qwen3_hf.py's recipe plus the biases: sorted-name order, one CPU generator, every value rounded to bf16."""
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
    import transformers.models.qwen2.modeling_qwen2 as mq
    from transformers import Qwen2Config, Qwen2ForCausalLM

    cfg = Qwen2Config(**CFG)
    cfg._attn_implementation = "eager"
    model = Qwen2ForCausalLM(cfg).float().eval()
    named = sorted(model.named_parameters(), key=lambda kv: kv[0])
    assert sorted(n for n, _ in named if n.endswith(".bias")) == sorted(
        f"model.layers.{i}.self_attn.{x}_proj.bias" for i in range(CFG["num_hidden_layers"]) for x in "qkv")
    fill(named)

    k_rows, v_rows = [], []
    real_rope = mq.apply_rotary_pos_emb

    def recording_rope(q, k, cos, sin, *a, **kw):
        oq, ok = real_rope(q, k, cos, sin, *a, **kw)
        k_rows.append(ok.detach().clone())  # [1, hkv, T, 128], one call per layer in layer order
        return oq, ok

    mq.apply_rotary_pos_emb = recording_rope
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

    biases = {n: p.data.clone() for n, p in named if n.endswith(".bias")}
    for n, p in named:
        if n in biases:
            p.data.zero_()
    no_bias_err = logits_error(logits_of(model, fed)[len(PROMPT) - 1:], l32)
    for n, p in named:
        if n in biases:
            p.data.copy_(biases[n])
    assert torch.equal(logits_of(model, fed)[len(PROMPT) - 1:], l32)

    model16 = model.to(torch.bfloat16)
    l16 = logits_of(model16, fed)[len(PROMPT) - 1:]
    agree = int((l16.argmax(-1) == l32.argmax(-1)).sum())
    top2 = l32.topk(2, -1).values
    margin = ((top2[:, 0] - top2[:, 1]) / l32.abs().amax(-1)).min().item()
    print("tokens", toks[:16], "...", "distinct", len(set(toks)), "bf16 greedy agreement", agree, "/", len(toks),
          f"bf16 vs fp32 {logits_error(l16, l32):.2e}, biases zeroed vs fp32 {no_bias_err:.2e}, smallest top-2 margin {margin:.2e}")
    assert agree == len(toks) == 33
    np.savez_compressed(
        os.path.join(HERE, "qwen2_hf.npz"), prompt=np.array(PROMPT), tokens=np.array(toks), logits_fp32=l32.numpy(),
        logits_bf16=l16.numpy(), names=np.array([n for n, _ in named]), shapes=np.array([str(tuple(p.shape)) for _, p in named]),
        k0_fp32=k0.float().numpy(), v0_fp32=v0.float().numpy(), no_bias_err=np.array([no_bias_err]), cfg=np.array([repr(CFG)]))


if __name__ == "__main__":
    main()
