"""Golden fixture for the Qwen3 dense path: Hugging Face's own Qwen3ForCausalLM (transformers, CPU) at a test size whose
hidden size is NOT n_heads * head_dim (256 vs 4 x 128: the decoupled head_dim of Qwen3-4B), GQA with G = 2, per-head
q_norm / k_norm, half-split RoPE, no biases, an untied head.

Run on a CPU machine with transformers installed (nothing is downloaded):   python tests/golden/gen_qwen3_hf.py
Writes tests/golden/qwen3_hf.npz: the prompt, the 33 greedy tokens of the fp32 run, the logits [33, vocab] of the prompt's
last token and of 32 teacher-forced steps from an fp32 run and from a bf16 run of the same model on the same tokens, the
(name, shape) list of the parameters in sorted-name order, and layer 0's k rows after norm + RoPE [39, 2, 128] from the
fp32 run.  Parameter VALUES are not stored: tests/qwen3_ref.py::qwen3_hf_params regenerates them from the same seed in
the same order (`fill` below, keep in sync).
"""

import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
           head_dim=128, vocab_size=512, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False, attention_bias=False)
PROMPT = [5, 17, 400, 33, 2, 41, 7]
NEW_TOKENS = 32
SEED = 8642


def fill(named, seed=SEED):
    """gen_ref_llama.py's recipe on HF names: sorted-name order, one CPU generator, every value rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    for n, p in named:
        if n.endswith("norm.weight"):
            t = 1.0 + 0.1 * torch.randn(p.shape, generator=g, dtype=torch.float32)
        elif n.startswith("model.embed_tokens"):
            t = torch.randn(p.shape, generator=g, dtype=torch.float32)
        else:
            t = torch.randn(p.shape, generator=g, dtype=torch.float32) * p.shape[-1] ** -0.5
        p.data.copy_(t.to(torch.bfloat16).to(p.dtype))


def main():
    import transformers.models.qwen3.modeling_qwen3 as mq
    from transformers import Qwen3Config, Qwen3ForCausalLM

    cfg = Qwen3Config(**CFG)
    cfg._attn_implementation = "eager"
    model = Qwen3ForCausalLM(cfg).float().eval()
    named = sorted(model.named_parameters(), key=lambda kv: kv[0])
    fill(named)

    k_rows = []
    real_rope = mq.apply_rotary_pos_emb

    def recording_rope(q, k, cos, sin, *a, **kw):
        oq, ok = real_rope(q, k, cos, sin, *a, **kw)
        k_rows.append(ok.detach().clone())  # [1, hkv, T, 128], one call per layer in layer order
        return oq, ok

    mq.apply_rotary_pos_emb = recording_rope

    def logits_of(m, seq):
        with torch.inference_mode():
            return m(input_ids=torch.tensor([seq]), use_cache=False).logits[0].float()

    seq = list(PROMPT)
    toks = []
    for _ in range(NEW_TOKENS + 1):  # greedy, the whole sequence again every step (no cache: nothing but the model's forward)
        toks.append(int(logits_of(model, seq)[-1].argmax()))
        seq.append(toks[-1])
    fed = PROMPT + toks[:-1]  # teacher forcing: row i predicts the token after fed[i]
    k_rows.clear()
    l32 = logits_of(model, fed)[len(PROMPT) - 1:]
    k0 = k_rows[0][0].transpose(0, 1).contiguous()  # layer 0: [T, hkv, 128]
    assert l32.argmax(-1).tolist() == toks
    model16 = model.to(torch.bfloat16)
    l16 = logits_of(model16, fed)[len(PROMPT) - 1:]
    np.savez_compressed(
        os.path.join(HERE, "qwen3_hf.npz"), prompt=np.array(PROMPT), tokens=np.array(toks), logits_fp32=l32.numpy(),
        logits_bf16=l16.numpy(), names=np.array([n for n, _ in named]), shapes=np.array([str(tuple(p.shape)) for _, p in named]),
        k0_fp32=k0.float().numpy(), cfg=np.array([repr(CFG)]))
    print("tokens", toks[:16], "...", "distinct", len(set(toks)), "bf16 greedy agreement",
          int((l16.argmax(-1) == l32.argmax(-1)).sum()), "/", len(toks))


if __name__ == "__main__":
    main()
