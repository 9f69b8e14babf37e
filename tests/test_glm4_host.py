"""The GLM-4 fixture (tests/golden/glm4_hf.npz: Hugging Face's GlmForCausalLM in fp32) against the CPU restatement of this project's
arithmetic (tests/glm4_ref.py), under tests/qwen3_ref.py::check_logits' bar of 2e-2 -- and against two rotations the fixture has to
tell from the model's: none at all, and all 128 channels.  No GPU."""

import torch

from tests import glm4_ref as g4
from tests.util import assert_close


def _run(rotation):
    g, cfg = g4.fixture()
    args = g4.glm4_args(cfg)
    p = g4.module_params(g4.glm4_hf_params(g), args)
    fed = g["prompt"].tolist() + g["tokens"].tolist()[:-1]
    logits, k0, v0 = g4.forward(p, fed, args, rotation=rotation)
    return g, logits[len(g["prompt"]) - 1:], k0, v0


def test_fixture_is_the_glm4_geometry():
    g, cfg = g4.fixture()
    assert (cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["partial_rotary_factor"]) == (4, 2, 128, 0.5)
    assert cfg["attention_bias"] and cfg["num_hidden_layers"] == 2 and cfg["hidden_size"] == 512
    names = g["names"].tolist()
    assert sorted(n for n in names if n.endswith(".bias")) == sorted(f"model.layers.{i}.self_attn.{x}_proj.bias" for i in range(2) for x in "qkv")
    assert "model.layers.0.mlp.gate_up_proj.weight" in names and not any("gate_proj" in n for n in names)  # shipped merged
    err, agree = g4.check_logits(torch.from_numpy(g["logits_bf16"]), g, "GLM4 HF bf16 vs HF fp32")
    assert agree == 33 and g["logits_fp32"].shape == (33, cfg["vocab_size"]) and g["k0_fp32"].shape == (39, 2, 128)


def test_cpu_restatement_reproduces_the_hf_fp32_run():
    g, logits, k0, v0 = _run("glm4")
    g4.check_logits(logits, g, "GLM4 CPU restatement vs HF fp32")
    assert_close(k0.float(), torch.from_numpy(g["k0_fp32"]), 1e-2, what="layer 0 k rows")
    assert_close(v0.float(), torch.from_numpy(g["v0_fp32"]), 1e-2, what="layer 0 v rows")


def test_fixture_tells_a_dropped_rotation_and_a_full_rotation_from_the_models():
    """The same restatement with the first 64 channels left unrotated, and with all 128 rotated, misses the logits bar."""
    for rotation in ("none", "full"):
        g, logits, _, _ = _run(rotation)
        err = g4.logits_error(logits, torch.from_numpy(g["logits_fp32"]))[0]
        print(f"GLM4 restatement with rotation={rotation!r} vs HF fp32: {err:.3e}")
        assert err > g4.LOGITS_BAR, rotation
