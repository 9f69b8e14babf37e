"""Qwen3-MoE, the parts that need no GPU: the third extension header against the library's exports, the host-side argument checks
of its two entries, the fp32 restatement (tests/qwen3_moe_ref.py) against Hugging Face's fp32 run (tests/golden/qwen3_moe_hf.npz),
the fixture's own forced-routing bf16 run against the bar the engine is held to, and the checkpoint loader on a tiny HF
directory under the published per-expert names at TP 1 and TP 2."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import qwen3_moe_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT3_HEADER = os.path.join(ROOT, "include", "chitu_hip_ext3.h")
ENTRIES = ("chitu_ext3_moe_gemm1_silu_bf16_tiled", "chitu_ext3_moe_gemm2_bf16_tiled")


def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


# ---------------------------------------------------------------- the header
def test_ext3_header_declares_exactly_the_exported_ext3_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(EXT3_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(chitu_ext3_\w+)\s*\(", src)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib().LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT\s+(chitu_ext3_\w+)", out)))
    assert declared == exported == sorted(ENTRIES)
    assert re.search(r"#define\s+CHITU_HIP_EXT3_VERSION\s+1\b", src) and '#include "chitu_hip.h"' in src
    assert not re.findall(r"\bint\s+(chitu_hip_\w+|chitu_ext_\w+|chitu_ext2_\w+)\s*\(", src)  # nothing of the frozen prefixes


# ---------------------------------------------------------------- host argument checks
I32, I64 = ctypes.c_int32, ctypes.c_int64


def _g1(p, numel, **over):
    a = dict(a=p, w1=p, sorted=p, experts=p, npost=p, h=p, numel=I64(numel), topk=I32(4), inter=I64(256), K=I64(384),
             max_mblocks=I64(8), block_m=I32(64), stream=None)
    a.update(over)
    return list(a.values())


def _g2(p, numel, **over):
    a = dict(h=p, w2=p, sorted=p, experts=p, npost=p, weights=p, weights_dtype=ctypes.c_int(0), mul=I32(1), out=p, numel=I64(numel),
             N=I64(136), inter=I64(256), max_mblocks=I64(8), block_m=I32(128), stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("numel", [0, 48])
def test_entries_check_their_arguments_on_the_host(numel):
    """Argument checks run before anything is launched and before the zero-size return: the pointers are host memory and are
    never dereferenced (with a launch these calls would return a HIP error or fault, not -1 / -2)."""
    lib = ctypes.CDLL(_lib().LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd, odd2 = ctypes.c_void_p(p.value + 8), ctypes.c_void_p(p.value + 2)
    g1, g2 = lib.chitu_ext3_moe_gemm1_silu_bf16_tiled, lib.chitu_ext3_moe_gemm2_bf16_tiled
    for name in ("a", "w1", "sorted", "experts", "npost", "h"):
        assert g1(*_g1(p, numel, **{name: None})) == -1, name
    for name in ("a", "w1", "h"):
        assert g1(*_g1(p, numel, **{name: odd})) == -1, name
    for name in ("sorted", "experts", "npost"):
        assert g1(*_g1(p, numel, **{name: odd2})) == -1, name
    for bad in (dict(block_m=I32(16)), dict(block_m=I32(96)), dict(block_m=I32(256)), dict(max_mblocks=I64(65536)),
                dict(max_mblocks=I64(-1)), dict(topk=I32(0))):
        assert g1(*_g1(p, numel, **bad)) == -1, bad
    assert g1(*_g1(p, -1)) == -1 and g2(*_g2(p, -1)) == -1
    for bad in (dict(K=I64(64)), dict(K=I64(192)), dict(K=I64(320)), dict(inter=I64(64)), dict(inter=I64(192))):
        assert g1(*_g1(p, numel, **bad)) == -2, bad
    for name in ("h", "w2", "sorted", "experts", "npost", "out", "weights"):
        assert g2(*_g2(p, numel, **{name: None})) == -1, name
    for name in ("h", "w2", "out"):
        assert g2(*_g2(p, numel, **{name: odd})) == -1, name
    assert g2(*_g2(p, numel, weights=ctypes.c_void_p(p.value + 1))) == -1
    assert g2(*_g2(p, numel, weights=odd2, weights_dtype=ctypes.c_int(2))) == -1
    for bad in (dict(block_m=I32(16)), dict(block_m=I32(0)), dict(max_mblocks=I64(65536)), dict(weights_dtype=ctypes.c_int(3))):
        assert g2(*_g2(p, numel, **bad)) == -1, bad
    for bad in (dict(inter=I64(64)), dict(inter=I64(320)), dict(N=I64(132)), dict(N=I64(7))):
        assert g2(*_g2(p, numel, **bad)) == -2, bad
    if numel == 0:  # nothing to do: 0 with nothing launched
        assert g1(*_g1(p, 0)) == 0 and g2(*_g2(p, 0)) == 0
        assert g2(*_g2(p, 0, weights=None, mul=I32(0))) == 0
    else:  # valid arguments, work to do, but no m-block to launch for
        assert g1(*_g1(p, numel, max_mblocks=I64(0))) == 0 and g2(*_g2(p, numel, max_mblocks=I64(0))) == 0


# ---------------------------------------------------------------- the restatement against Hugging Face's fp32 run
@pytest.fixture(scope="module")
def fx():
    g, cfg = mr.fixture()
    hf = mr.hf_params(g)
    fed = g["prompt"].tolist() + g["tokens"].tolist()[:-1]
    return g, cfg, hf, fed


def test_fixture_has_what_the_tests_read(fx):
    g, cfg, hf, fed = fx
    L, T, E, k = cfg["num_hidden_layers"], len(fed), cfg["num_experts"], cfg["num_experts_per_tok"]
    assert (L, T, E, k) == (2, 39, 16, 4)
    assert g["router_ids"].shape == (L, T, k) and g["router_logits_fp32"].shape == (L, T, E)
    assert g["logits_fp32"].shape == g["logits_bf16_forced"].shape == (33, cfg["vocab_size"])
    assert set(g["names"].tolist()) == set(hf) and f"model.layers.0.mlp.experts.gate_up_proj" in hf
    # the generator's two conditions, from the stored data
    srt = torch.from_numpy(g["router_logits_fp32"]).sort(-1, descending=True).values
    assert float((srt[..., k - 1] - srt[..., k]).min()) >= 1e-3
    err, _ = mr.logits_error(torch.from_numpy(g["logits_bf16_forced"]), torch.from_numpy(g["logits_fp32"]))
    assert err < 1.2e-2, err


def test_restatement_with_free_routing_reproduces_the_hf_fp32_run(fx):
    """Both sides are fp32 and only the summation order differs: 1e-4 of each row's peak sits two orders above fp32 noise and
    two below any bf16 effect.  The router's choices are the stored ones exactly."""
    g, cfg, hf, fed = fx
    logits, r_logits, r_ids = mr.forward(hf, fed, cfg)
    err, _ = mr.logits_error(logits[len(g["prompt"]) - 1:], torch.from_numpy(g["logits_fp32"]))
    r_err = float((r_logits - torch.from_numpy(g["router_logits_fp32"])).abs().max())
    print(f"QWEN3-MOE restatement vs HF fp32: logits {err:.3e}, router logits {r_err:.3e}")
    assert err < 1e-4, err
    assert torch.equal(r_ids.sort(-1).values, torch.from_numpy(g["router_ids"]).long().sort(-1).values)
    assert torch.equal(r_ids, torch.from_numpy(g["router_ids"]).long())


def test_restatement_with_the_stored_ids_forced_is_the_free_run(fx):
    g, cfg, hf, fed = fx
    free = mr.forward(hf, fed, cfg)[0]
    forced = mr.forward(hf, fed, cfg, route_ids=g["router_ids"])[0]
    assert torch.equal(free, forced)
    # ... and other ids give another function: the argument is not ignored
    other = (torch.from_numpy(g["router_ids"]).long() + 1) % cfg["num_experts"]
    assert not torch.equal(mr.forward(hf, fed, cfg, route_ids=other)[0], free)


def test_hf_bf16_run_with_forced_routing_meets_the_engines_bar(fx):
    g = fx[0]
    err, agree = mr.check_logits(torch.from_numpy(g["logits_bf16_forced"]), g["logits_fp32"], "HF bf16 (routing forced) vs HF fp32",
                                 tokens=g["tokens"])
    assert err < 1.2e-2 and agree >= 31


# ---------------------------------------------------------------- the loader
@pytest.mark.parametrize("world", [1, 2])
def test_loader_reads_the_per_expert_names_and_slices_by_width(fx, tmp_path, world):
    from chitu_amd.checkpoint import load_checkpoint_hf_qwen3_moe
    from chitu_amd.qwen3_moe import Qwen3MoeDecoder

    g, cfg, hf, _ = fx
    args = mr.moe_args(cfg)
    path = mr.write_hf_dir(hf, str(tmp_path / "qwen3_moe"))
    E, I, H = cfg["num_experts"], cfg["moe_intermediate_size"], cfg["hidden_size"]
    hd, hq, hkv = cfg["head_dim"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    if world == 2:  # a rank's share of the expert width must be a multiple of 128: a model with experts twice as wide
        args = mr.moe_args(cfg, moe_inter_dim=2 * I)
        wide = dict(hf)
        for k, v in hf.items():
            if k.endswith("gate_up_proj"):  # [E, 2I, H] -> [E, 4I, H]: gate rows twice as many, then up rows
                wide[k] = torch.cat([v[:, :I], v[:, :I] * 2, v[:, I:], v[:, I:] * 2], dim=1)
            elif k.endswith("experts.down_proj"):
                wide[k] = torch.cat([v, v * 2], dim=2)
        hf, I = wide, 2 * I
        path = mr.write_hf_dir(hf, str(tmp_path / "qwen3_moe_wide"))
    from safetensors.torch import load_file

    from chitu_amd.checkpoint import preprocess_hf_qwen3_moe

    on_disk = load_file(os.path.join(path, "model.safetensors"))
    assert f"model.layers.1.mlp.experts.{E - 1}.down_proj.weight" in on_disk and not any(k.endswith("gate_up_proj") for k in on_disk)
    for rank in range(world):
        st = preprocess_hf_qwen3_moe(on_disk, args, rank, world)
        Il = I // world
        for i in range(cfg["num_hidden_layers"]):
            gu, dn = hf[f"model.layers.{i}.mlp.experts.gate_up_proj"], hf[f"model.layers.{i}.mlp.experts.down_proj"]
            w13, w2 = st[f"layers.{i}.ffn.w13"], st[f"layers.{i}.ffn.w2"]
            assert w13.shape == (E, 2 * Il, H) and w2.shape == (E, H, Il) and w13.dtype == w2.dtype == torch.bfloat16
            assert torch.equal(w13[:, :Il], gu[:, rank * Il:(rank + 1) * Il])  # this rank's gate rows ...
            assert torch.equal(w13[:, Il:], gu[:, I + rank * Il:I + (rank + 1) * Il])  # ... then its up rows
            assert torch.equal(w2, dn[:, :, rank * Il:(rank + 1) * Il])
            assert torch.equal(st[f"layers.{i}.ffn.gate"], hf[f"model.layers.{i}.mlp.gate.weight"])  # the router stays whole
            q = hf[f"model.layers.{i}.self_attn.q_proj.weight"]
            ql = hq * hd // world
            assert torch.equal(st[f"layers.{i}.attn.wqkv"][:ql], q[rank * ql:(rank + 1) * ql])
            assert torch.equal(st[f"layers.{i}.attn.q_norm"], hf[f"model.layers.{i}.self_attn.q_norm.weight"])
            o = hf[f"model.layers.{i}.self_attn.o_proj.weight"]
            assert torch.equal(st[f"layers.{i}.attn.wo"], o[:, rank * ql:(rank + 1) * ql])
        V = cfg["vocab_size"] // world
        assert torch.equal(st["embed_weight"], hf["model.embed_tokens.weight"][rank * V:(rank + 1) * V])
        assert torch.equal(st["head_weight"], hf["lm_head.weight"][rank * V:(rank + 1) * V])
    if world == 1:  # the whole path into a decoder that only holds weights (cache None: it never attends)
        model = Qwen3MoeDecoder(args, None, None, max_position_embeddings=64, device="cpu")
        load_checkpoint_hf_qwen3_moe(model, path)
        want = mr.module_params(hf, args)
        params = dict(model.named_parameters())
        assert set(params) == set(want)
        for k, t in params.items():
            assert torch.equal(t, want[k]), k
        with pytest.raises(ValueError):  # 128 columns over two ranks: a rank's share is no multiple of 128
            load_checkpoint_hf_qwen3_moe(model, path, rank=0, world=2)
        # a file that lacks an expert is refused, not half loaded
        broken = {k: v for k, v in mr.on_disk_names(hf).items() if ".experts.3.up_proj." not in k}
        with pytest.raises(KeyError):
            from chitu_amd.checkpoint import preprocess_hf_qwen3_moe

            preprocess_hf_qwen3_moe(broken, args)


def test_what_is_not_built_is_refused():
    from chitu_amd.qwen3_moe import Qwen3MoeArgs, Qwen3MoeDecoder, check_args

    _, cfg = mr.fixture()
    check_args(mr.moe_args(cfg))
    check_args(Qwen3MoeArgs())  # Qwen3-30B-A3B: 768 = 6 x 128
    check_args(Qwen3MoeArgs(moe_inter_dim=1536), 4)  # Qwen3-235B-A22B at TP 4
    for bad, world in ((dict(moe_inter_dim=192), 1), (dict(moe_inter_dim=128), 2), (dict(moe_inter_dim=768), 4),
                       (dict(mlp_only_layers=[0]), 1), (dict(decoder_sparse_step=2), 1)):
        with pytest.raises(ValueError):
            check_args(mr.moe_args(cfg, **bad), world)
        if world == 1:
            with pytest.raises(ValueError):
                Qwen3MoeDecoder(mr.moe_args(cfg, **bad), None, None, max_position_embeddings=64, device="cpu")


def test_args_defaults_are_qwen3_30b_a3b():
    from chitu_amd.qwen3_moe import Qwen3MoeArgs

    a = Qwen3MoeArgs()
    assert (a.dim, a.n_layers, a.n_heads, a.n_kv_heads, a.head_dim, a.moe_inter_dim, a.num_experts, a.num_experts_per_tok) == \
        (2048, 48, 32, 4, 128, 768, 128, 8)
    assert a.norm_topk_prob and a.qk_norm and a.vocab_size == 151936 and a.norm_eps == 1e-6 and a.rope_theta == 1e6
    assert a.kv_cache_dtype == "bf16" and a.sliding_window is None and a.attn_softcap == 0.0 and not a.tie_word_embeddings


def test_generic_bf16_experts_keep_the_streaming_form_by_default():
    from chitu_amd import fused_moe

    assert fused_moe._MOE_BF16_TILED_MIN_TOKENS == 0 or "CHITU_MOE_BF16_TILED_MIN_TOKENS" in os.environ
    # the rule itself: floor 0 never takes the tiled form, a floor takes it from that many tokens on with enough slots per expert
    assert not fused_moe._takes_tiled(4096, 4096 * 8, 128, 768, 2048, None, min_tokens=0)
    assert fused_moe._takes_tiled(130, 520, 16, 128, 256, None, min_tokens=1)
    assert not fused_moe._takes_tiled(130, 520, 16, 128, 256, None, min_tokens=131)
    assert not fused_moe._takes_tiled(90, 360, 16, 128, 256, None, min_tokens=1)  # fewer than 24 slots per expert
