"""CPU checks of the q / k / v bias oracle (tests/qkv_bias_exact.py), of the new header and the entries' host checks, of the
loader's bias path, of LlamaAttention's constructor refusals, of the Qwen2 fixture, and of Qwen2Decoder's host-side wiring with
every HIP op swapped for an oracle.  No GPU."""

import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import qkv_bias_exact as bx
from tests import qwen2_ref as q2
from tests.row_exact import rope_oracle
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT5_HEADER = os.path.join(ROOT, "include", "chitu_hip_ext5.h")
ENTRIES = ["chitu_ext5_gqa_qkv_bias_post", "chitu_ext5_gqa_qkv_bias_post_kv_fp8", "chitu_ext5_qkv_bias_rope"]
BF16 = torch.bfloat16


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("hq,hkv", bx.SHAPES)
def test_oracle_is_the_existing_post_oracle_on_the_bf16_sum(hq, hkv, layout):
    """The numpy / float64 add with the explicit rounding equals torch's bf16 add bit for bit, so the oracle is
    gqa_qkv_post's (rope_oracle on q and k, v copied) applied to qkv + bias."""
    c = bx.bias_case(5, hq, hkv, seed=layout)
    y, q, k, v = bx.bias_oracle(c, layout)
    s = c["x"] + c["bias"].view(hq + 2 * hkv, bx.D)
    assert s.dtype == BF16 and torch.equal(bx.bits(y), bx.bits(s))
    assert torch.equal(bx.bits(q), bx.bits(rope_oracle(s[:, :hq].contiguous(), c["cos"], c["sin"], layout)))
    assert torch.equal(bx.bits(k), bx.bits(rope_oracle(s[:, hq:hq + hkv].contiguous(), c["cos"], c["sin"], layout)))
    assert torch.equal(bx.bits(v), bx.bits(s[:, hq + hkv:].contiguous()))
    # the rounding is a real one on these cases, and the bias matters
    assert int((y.double() != c["x"].double() + c["bias"].double().view(-1, bx.D)).sum()) > y.numel() // 4
    assert not torch.equal(q, rope_oracle(c["x"][:, :hq].contiguous(), c["cos"], c["sin"], layout))


def test_bf16_rne_rounds_ties_to_even_and_refuses_an_inexact_sum():
    import numpy as np

    ulp = 2.0 ** -7  # of a bf16 number in [1, 2)
    got = bx.bf16_rne(np.array([1 + ulp / 2, 1 + 3 * ulp / 2, 1 + ulp / 2 + 2.0 ** -20, -(1 + ulp / 2), 0.0, 3.0])).float().tolist()
    assert got == [1.0, 1 + 2 * ulp, 1 + ulp, -1.0, 0.0, 3.0]
    with pytest.raises(AssertionError):
        bx.bf16_rne(np.array([1.0 + 2.0 ** -30]))


def test_bias_values_tell_heads_and_lanes_apart_and_match_the_activations():
    for hq, hkv in bx.SHAPES:
        b = bx.bias_row(hq, hkv).float().view(hq + 2 * hkv, 16, 8)
        assert torch.equal(b.to(BF16).float(), b)
        for h in range(b.shape[0]):
            chunks = {tuple(b[h, l].tolist()) for l in range(16)}
            assert len(chunks) == 16 and all(len(set(ch)) == 8 for ch in chunks)  # every lane's chunk is its own; no channel repeats
            assert all(not torch.equal(b[h], b[o]) for o in range(b.shape[0]) if o != h)
            assert bool((b[h, :8] != b[h, 8:]).all())  # the half-split partner's chunk differs in every channel
        x = bx.bias_case(5, hq, hkv)["x"].float()
        assert 0.5 < float(b.std() / x.std()) < 2.0


def test_paged_batches_cover_the_four_old_lengths():
    seen = set()
    for hq, hkv in bx.SHAPES:
        for bs in bx.BATCHES:
            for layout in (0, 1):
                lens, table, num_pages, kinds = bx.paged(bs, seed=hq + hkv + layout + bs)
                assert not kinds and all(bx.live_row(b, lens, table, bx.PAGE, table.shape[1], num_pages) is not None for b in range(bs))
                seen |= set(lens.tolist())
    assert seen == set(bx.OLD_LENS)
    kinds = {}
    for seed in (0, 1):
        kinds.update({k: 1 for k in bx.paged(5, seed=seed, bad=True)[3].values()})
    assert sorted(kinds) == ["beyond", "neg", "page=-1", "page=num_pages"]


# ---------------------------------------------------------------- the header and the entries' host checks
def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_ext5_header_declares_exactly_the_exported_ext5_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(EXT5_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(chitu_ext5_\w+)\s*\(", src)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib().LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT\s+(chitu_ext5_\w+)", out)))
    assert declared == exported == sorted(ENTRIES)
    assert re.search(r"#define\s+CHITU_HIP_EXT5_VERSION\s+1\b", src) and '#include "chitu_hip.h"' in src
    assert not re.findall(r"\bint\s+(chitu_hip_\w+)\s*\(", src)  # nothing of the frozen prefix is declared here


def _post_args(p, head_dim=128, null=None):
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    a = [p, i64(36 * 128), i32(28), i32(4), i32(head_dim), p, p, i32(1), p, p, i64(4), i32(16), p, i32(2), p, i32(1), p, None]
    if null is not None:
        a[null] = None
    return a


def _rope_args(p, head_dim=128, null=None):
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    a = [p, i64(1024), i64(128), p, p, p, p, p, p, i64(1), i32(4), i32(2), i32(head_dim), i32(1), None]
    if null is not None:
        a[null] = None
    return a


def test_entries_refuse_other_head_dims_null_and_misaligned_pointers_on_the_host():
    """Argument checks run before anything is launched (the pointers are host memory and are never dereferenced; with a launch
    these calls would fault or return a HIP error, not -2 / -1)."""
    lib = ctypes.CDLL(_lib().LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    at = (ctypes.addressof(buf) + 15) & ~15
    p, odd = ctypes.c_void_p(at), ctypes.c_void_p(at + 8)
    for name in ENTRIES[:2]:
        fn = getattr(lib, name)
        assert fn(*_post_args(p, head_dim=64)) == -2, name
        for null in (0, 5, 6, 8, 9, 12, 14, 16):  # qkv, cos, sin, both caches, table, lengths, bias
            assert fn(*_post_args(p, null=null)) == -1, (name, null)
        for at_ in (0, 5, 6, 8, 9, 16):  # every 16-byte load or store base
            a = _post_args(p)
            a[at_] = odd
            assert fn(*a) == -1, (name, at_)
        a = _post_args(p)
        a[1] = ctypes.c_int64(35 * 128)  # a row stride shorter than the row
        assert fn(*a) == -2
        a = _post_args(p)
        a[15] = ctypes.c_int32(0)
        assert fn(*a) == 0  # zero rows: nothing is launched
    fn = lib.chitu_ext5_qkv_bias_rope
    assert fn(*_rope_args(p, head_dim=64)) == -2
    for null in (0, 3, 4, 5, 6, 7, 8):
        assert fn(*_rope_args(p, null=null)) == -1, null
        a = _rope_args(p)
        a[null] = odd
        assert fn(*a) == -1, null
    a = _rope_args(p)
    a[9] = ctypes.c_int64(0)
    assert fn(*a) == 0
    for at_, v in ((1, 1028), (2, 132)):  # strides that leave heads off 16-byte boundaries
        a = _rope_args(p)
        a[at_] = ctypes.c_int64(v)
        assert fn(*a) == -1


# ---------------------------------------------------------------- the loader
def _state_4_2(seed=3):
    """An HF-named state of one layer with 4 q / 2 kv heads of 128 over dim 512."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16)
    pre = "model.layers.0."
    return {"model.embed_tokens.weight": r(64, 512), "lm_head.weight": r(64, 512), "model.norm.weight": r(512),
            pre + "input_layernorm.weight": r(512), pre + "post_attention_layernorm.weight": r(512),
            pre + "self_attn.q_proj.weight": r(512, 512), pre + "self_attn.k_proj.weight": r(256, 512),
            pre + "self_attn.v_proj.weight": r(256, 512), pre + "self_attn.o_proj.weight": r(512, 512),
            pre + "self_attn.q_proj.bias": r(512), pre + "self_attn.k_proj.bias": r(256), pre + "self_attn.v_proj.bias": r(256),
            pre + "mlp.gate_proj.weight": r(128, 512), pre + "mlp.up_proj.weight": r(128, 512), pre + "mlp.down_proj.weight": r(512, 128)}


@pytest.mark.parametrize("world", [1, 2])
def test_loader_shards_the_bias_by_heads_like_wqkv(world):
    from chitu_amd.checkpoint import preprocess_hf_llama, to_llama_module_names

    hf = _state_4_2()
    hq, hkv = 4 // world, 2 // world
    per_rank = [to_llama_module_names(preprocess_hf_llama(hf, 4, 2, 512, rank, world), qkv_bias=True) for rank in range(world)]
    for st in per_rank:
        assert st["layers.0.attn.bqkv"].shape == ((hq + 2 * hkv) * 128,) and st["layers.0.attn.wqkv"].shape == ((hq + 2 * hkv) * 128, 512)
        assert not any(k.endswith(".bias") for k in st)
    for i, n in enumerate("qkv"):
        lo, hi = ((0, hq), (hq, hq + hkv), (hq + hkv, hq + 2 * hkv))[i]
        got = torch.cat([st["layers.0.attn.bqkv"].view(-1, 128)[lo:hi] for st in per_rank]).reshape(-1)
        assert torch.equal(got, hf[f"model.layers.0.self_attn.{n}_proj.bias"]), n
        got_w = torch.cat([st["layers.0.attn.wqkv"].view(-1, 128, 512)[lo:hi] for st in per_rank]).reshape(-1, 512)
        assert torch.equal(got_w, hf[f"model.layers.0.self_attn.{n}_proj.weight"]), n


def test_to_llama_module_names_refuses_every_other_bias():
    from chitu_amd.checkpoint import preprocess_hf_llama, to_llama_module_names

    hf = _state_4_2()
    st = preprocess_hf_llama(hf, 4, 2, 512)
    with pytest.raises(NotImplementedError):  # the default keeps refusing
        to_llama_module_names(st)
    assert "layers.0.attn.bqkv" in to_llama_module_names(st, qkv_bias=True)
    for extra in ("layers.0.self_attn.o_proj.bias", "layers.0.mlp.down_proj.bias", "lm_head.bias", "self_attn.qkv_proj.bias"):
        with pytest.raises(NotImplementedError):
            to_llama_module_names({**st, extra: torch.zeros(512, dtype=BF16)}, qkv_bias=True)


# ---------------------------------------------------------------- the constructor
def _attention(**over):
    from chitu_amd.llama import LlamaAttention
    from chitu_amd.qwen2 import Qwen2Args

    kw = dict(dim=512, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=64, ffn_dim=128)
    kw.update(over)
    return LlamaAttention(Qwen2Args(**kw), 0, None, None, device="cpu", rotary_type="hf-llama")


def test_constructor_owns_a_bias_only_with_the_flag_and_refuses_what_no_launch_covers():
    from chitu_amd.llama import LlamaArgs, LlamaAttention

    a = _attention()
    assert a.qkv_bias and a.bqkv.shape == (8 * 128,) and a.bqkv.dtype == BF16
    plain = LlamaAttention(LlamaArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=64, ffn_dim=128), 0, None, None, device="cpu")
    assert not plain.qkv_bias and [n for n, _ in plain.named_parameters()] == ["wqkv", "wo"]
    assert not _attention(qkv_bias=False).qkv_bias
    with pytest.raises(ValueError, match="head_dim"):
        _attention(dim=256)  # 4 heads of 64: Qwen2.5-0.5B's head_dim

    from chitu_amd.qwen3 import Qwen3Args

    both = Qwen3Args(dim=512, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=64, ffn_dim=128)
    both.qkv_bias = True
    with pytest.raises(ValueError, match="qk_norm"):
        LlamaAttention(both, 0, None, None, device="cpu", rotary_type="hf-llama")


def test_qwen2_defaults_are_the_7b_model():
    from chitu_amd.qwen2 import Qwen2Args, Qwen2Block, Qwen2Decoder

    a = Qwen2Args()
    assert (a.dim, a.n_layers, a.n_heads, a.n_kv_heads, a.vocab_size, a.ffn_dim, a.norm_eps, a.rope_theta, a.head_dim) == \
        (3584, 28, 28, 4, 152064, 18944, 1e-6, 1e6, 128)
    assert a.qkv_bias and not a.tie_word_embeddings and a.kv_cache_dtype == "bf16" and a.sliding_window is None and a.attn_softcap == 0.0
    assert Qwen2Block.rotary_type == "hf-llama" and Qwen2Decoder.block_type is Qwen2Block


# ---------------------------------------------------------------- the fixture
def test_fixture_is_sharp_enough_to_see_a_dropped_bias():
    """The stored distance of the bias-free model from the fp32 run exceeds ten times the logits bar; Hugging Face's own bf16
    run is inside the bar and picks the fp32 run's token on every row."""
    g, cfg = q2.fixture()
    assert float(g["no_bias_err"][0]) > 10 * q2.LOGITS_BAR
    assert cfg["num_attention_heads"] // cfg["num_key_value_heads"] == 7 and cfg["hidden_size"] // cfg["num_attention_heads"] == 128
    err, agree = q2.check_logits(torch.from_numpy(g["logits_bf16"]), g, "Qwen2 HF bf16 vs HF fp32")
    assert agree == 33
    names = g["names"].tolist()
    assert sorted(n for n in names if n.endswith(".bias")) == sorted(f"model.layers.{i}.self_attn.{x}_proj.bias" for i in range(2) for x in "qkv")


def test_cpu_restatement_reproduces_the_hf_fp32_run_and_misses_it_without_the_bias():
    g, cfg = q2.fixture()
    args = q2.qwen2_args(cfg)
    p = q2.module_params(q2.qwen2_hf_params(g), args)
    fed = g["prompt"].tolist() + g["tokens"].tolist()[:-1]
    logits, k0, v0 = q2.forward(p, fed, args)
    q2.check_logits(logits[len(g["prompt"]) - 1:], g, "Qwen2 CPU restatement vs HF fp32")
    assert_close(k0.float(), torch.from_numpy(g["k0_fp32"]), 1e-2, what="layer 0 k rows")
    assert_close(v0.float(), torch.from_numpy(g["v0_fp32"]), 1e-2, what="layer 0 v rows")
    dropped = q2.forward(p, fed, args, bias=False)[0][len(g["prompt"]) - 1:]
    err = q2.logits_error(dropped, torch.from_numpy(g["logits_fp32"]))[0]
    print(f"QWEN2 restatement without the bias vs HF fp32: {err:.3e} (fixture: {float(g['no_bias_err'][0]):.3e})")
    assert err > 10 * q2.LOGITS_BAR


# ---------------------------------------------------------------- the decoder's wiring on the CPU
def test_qwen2_decoder_wiring_on_the_cpu_reproduces_the_hf_fp32_run(tmp_path, monkeypatch):
    """Qwen2Decoder's host-side logic (the bias branches of LlamaAttention, the loader, the paged cache) with every HIP op
    swapped for the oracle (tests/cpu_ops_shim.py) and the two bias ops for a bf16 add in front of the oracle's rotation: prefill
    of the prompt, then 32 eager decode steps fed the fixture's tokens.  The kernels themselves are the GPU tests' business."""
    from chitu_amd import ops
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.checkpoint import load_checkpoint_hf_llama
    from chitu_amd.qwen2 import Qwen2Decoder
    from tests import cpu_ops_shim as shim

    shim.install_llama(monkeypatch.setattr)
    calls = {"prefill": 0, "decode": 0}

    def qkv_bias_rope(qkv, hq, hkv, bias, cos, sin, rotary_type="hf-llama"):
        calls["prefill"] += 1
        layout = 0 if rotary_type == "llama" else 1
        y = qkv + bias.view(hq + 2 * hkv, 128)
        return (rope_oracle(y[:, :hq].contiguous(), cos, sin, layout), rope_oracle(y[:, hq:hq + hkv].contiguous(), cos, sin, layout),
                y[:, hq + hkv:].contiguous())

    def gqa_qkv_bias_post(qkv, hq, hkv, cos, sin, k_cache, v_cache, table, lens, bias, rotary_type="llama"):
        calls["decode"] += 1
        q, k, v = qkv_bias_rope(qkv, hq, hkv, bias, cos, sin, rotary_type)
        calls["prefill"] -= 1
        page = k_cache.shape[1]
        for b in range(qkv.shape[0]):
            L = int(lens[b])
            k_cache[int(table[b][L // page])][L % page] = k[b]
            v_cache[int(table[b][L // page])][L % page] = v[b]
        return q

    monkeypatch.setattr(ops, "qkv_bias_rope", qkv_bias_rope)
    monkeypatch.setattr(ops, "gqa_qkv_bias_post", gqa_qkv_bias_post)
    monkeypatch.setattr(ops, "gqa_qkv_post", None)  # a Qwen2 block must not take the launches without the bias
    monkeypatch.setattr(ops, "apply_rotary_pos_emb", None)
    monkeypatch.setattr(ops, "bf16_linear_add_norm_qkv_post", None)
    g, cfg = q2.fixture()
    args = q2.qwen2_args(cfg)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=1, block_size=16, max_seq_len=64, device="cpu",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=BF16)
    model = Qwen2Decoder(args, cache, shim.CpuGqaBackend(), max_position_embeddings=64, device="cpu")
    load_checkpoint_hf_llama(model, q2.write_hf_dir(q2.qwen2_hf_params(g), str(tmp_path / "qwen2")))
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    rows = [model.prefill([prompt], ["r"]).float()]
    for step in range(32):
        cache.prepare_cache_decode(["r"])
        cache.prepare_block_table_for_decode(["r"])
        rows.append(model.decode(torch.tensor([toks[step]]), use_graph=False).float())
        cache.finalize_cache_single_decode(["r"])
    assert calls == {"prefill": args.n_layers, "decode": 32 * args.n_layers}
    q2.check_logits(torch.cat(rows), g, "Qwen2 CPU wiring vs HF fp32")
    pages = torch.tensor(cache.block_table["r"])
    assert_close(cache.paged_k_cache[0][pages].flatten(0, 1)[:39].float(), torch.from_numpy(g["k0_fp32"]), 1e-2, what="layer 0 K page rows")
    assert_close(cache.paged_v_cache[0][pages].flatten(0, 1)[:39].float(), torch.from_numpy(g["v0_fp32"]), 1e-2, what="layer 0 V page rows")
