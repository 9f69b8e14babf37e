"""Golden fixture for the Qwen3-MoE path: Hugging Face's own Qwen3MoeForCausalLM (transformers, CPU) at a test size -- hidden
256, 16 experts of width 128, top 4 renormalised, 2 sparse layers, 4 / 2 heads of 128 (the decoupled head_dim), vocab 512.

Run on a CPU machine with transformers installed (nothing is downloaded):   python tests/golden/gen_qwen3_moe_hf.py
gen_qwen3_hf.py's recipe: its `fill`, its PROMPT, 32 new tokens.  Writes tests/golden/qwen3_moe_hf.npz: the prompt, the 33
greedy tokens of the fp32 run, the logits [33, vocab] of the prompt's last token and of 32 teacher-forced steps from the fp32
run, the (name, shape) list of the parameters in sorted-name order, the seed, and per layer the fp32 run's router ids
[2, 39, 4] and router logits [2, 39, 16] on the teacher-forced sequence.  Parameter VALUES are not stored:
tests/qwen3_moe_ref.py regenerates them from the seed in the same order.

logits_bf16_forced: HF's own bf16 run of the same model on the same tokens with each layer's routing FORCED to the fp32 run's
ids (Qwen3MoeTopKRouter.forward patched: its own softmax, the given ids instead of its top-k, its own renormalisation).  Under
free routing a bf16 run flips near-tied experts and lands 0.16 of the peak away from the fp32 run; with the ids forced it is
about 1e-2 away, which is what an end-to-end bar can be held against.

The seed is the first of SEEDS for which (a) the forced bf16 run is within 1.2e-2 of the fp32 run (tests/qwen3_ref.py's
logits_error: the reference alone keeps a 1.6x margin under the 2e-2 bar) and (b) the smallest gap between the 4th and 5th
largest fp32 router logit over every (layer, token) is at least 1e-3.  Both are asserted.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_qwen3_hf import NEW_TOKENS, PROMPT, fill  # noqa: E402

CFG = dict(hidden_size=256, intermediate_size=512, moe_intermediate_size=128, num_experts=16, num_experts_per_tok=4,
           norm_topk_prob=True, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128, vocab_size=512,
           rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False, attention_bias=False, decoder_sparse_step=1,
           mlp_only_layers=[])
SEEDS = (8642, 1, 2)
FORCED_BAR, GAP_BAR = 1.2e-2, 1e-3


def logits_error(mine, ref):  # tests/qwen3_ref.py::logits_error
    return ((mine - ref).abs().amax(-1) / ref.abs().amax(-1)).max().item()


def run(seed):
    import transformers.models.qwen3_moe.modeling_qwen3_moe as mq
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM

    cfg = Qwen3MoeConfig(**CFG)
    cfg._attn_implementation = "eager"
    model = Qwen3MoeForCausalLM(cfg).float().eval()
    named = sorted(model.named_parameters(), key=lambda kv: kv[0])
    fill(named, seed)

    top_k, n_layers = CFG["num_experts_per_tok"], CFG["num_hidden_layers"]
    recorded, forced = [], {"ids": None, "call": 0}
    real_forward = mq.Qwen3MoeTopKRouter.forward

    def router_forward(self, hidden_states):
        hidden_states = hidden_states.reshape(-1, self.hidden_dim)
        router_logits = torch.nn.functional.linear(hidden_states, self.weight)
        router_probs = torch.nn.functional.softmax(router_logits, dtype=torch.float, dim=-1)
        if forced["ids"] is None:
            router_top_value, router_indices = torch.topk(router_probs, self.top_k, dim=-1)
            recorded.append((router_logits.detach().float().clone(), router_indices.detach().clone()))
        else:  # one call per layer in layer order
            router_indices = forced["ids"][forced["call"] % n_layers]
            forced["call"] += 1
            router_top_value = router_probs.gather(-1, router_indices)
        if self.norm_topk_prob:
            router_top_value = router_top_value / router_top_value.sum(dim=-1, keepdim=True)
        return router_logits, router_top_value.to(router_logits.dtype), router_indices

    mq.Qwen3MoeTopKRouter.forward = router_forward
    try:
        def logits_of(m, seq):
            with torch.inference_mode():
                return m(input_ids=torch.tensor([seq]), use_cache=False).logits[0].float()

        seq, toks = list(PROMPT), []
        for _ in range(NEW_TOKENS + 1):  # greedy, the whole sequence again every step
            toks.append(int(logits_of(model, seq)[-1].argmax()))
            seq.append(toks[-1])
        fed = PROMPT + toks[:-1]  # teacher forcing: row i predicts the token after fed[i]
        recorded.clear()
        l32 = logits_of(model, fed)[len(PROMPT) - 1:]
        assert len(recorded) == n_layers and l32.argmax(-1).tolist() == toks
        r_logits = torch.stack([r[0] for r in recorded])  # [layers, T, E]
        r_ids = torch.stack([r[1] for r in recorded])  # [layers, T, top_k]
        srt = r_logits.sort(-1, descending=True).values
        gap = (srt[..., top_k - 1] - srt[..., top_k]).min().item()

        model16 = model.to(torch.bfloat16)
        free = logits_error(logits_of(model16, fed)[len(PROMPT) - 1:], l32)
        forced["ids"], forced["call"] = r_ids, 0
        l16 = logits_of(model16, fed)[len(PROMPT) - 1:]
        assert forced["call"] == n_layers
    finally:
        mq.Qwen3MoeTopKRouter.forward = real_forward
    err = logits_error(l16, l32)
    print(f"seed {seed}: bf16 vs fp32 free routing {free:.3e}, routing forced {err:.3e}, smallest 4th/5th logit gap {gap:.3e}, "
          f"distinct tokens {len(set(toks))}")
    return dict(named=named, toks=toks, l32=l32, l16=l16, r_logits=r_logits, r_ids=r_ids, err=err, gap=gap, free=free)


def main():
    for seed in SEEDS:
        r = run(seed)
        if r["err"] < FORCED_BAR and r["gap"] >= GAP_BAR:
            break
    else:
        raise AssertionError("no seed of SEEDS meets both conditions")
    assert r["err"] < FORCED_BAR and r["gap"] >= GAP_BAR
    named = r["named"]
    np.savez_compressed(
        os.path.join(HERE, "qwen3_moe_hf.npz"), prompt=np.array(PROMPT), tokens=np.array(r["toks"]), logits_fp32=r["l32"].numpy(),
        logits_bf16_forced=r["l16"].numpy(), names=np.array([n for n, _ in named]),
        shapes=np.array([str(tuple(p.shape)) for _, p in named]), router_ids=r["r_ids"].numpy().astype(np.int32),
        router_logits_fp32=r["r_logits"].numpy(), seed=np.array([seed]), cfg=np.array([repr(CFG)]),
        stats=np.array([r["free"], r["err"], r["gap"]]))
    print("wrote qwen3_moe_hf.npz with seed", seed)


if __name__ == "__main__":
    main()
