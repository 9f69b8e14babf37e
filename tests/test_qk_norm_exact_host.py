"""Per-head QK-norm (Qwen3), the parts that need no GPU: the CPU oracle of tests/qk_norm_exact.py against a float64 statement
and against wrong variants of itself, the extension header against the library's exports, the entries' host-side argument
checks, the Qwen3 checkpoint loader, and the Hugging Face fixture against a CPU restatement of this project's arithmetic."""

import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import qk_norm_exact as qx
from tests import qwen3_ref as qr
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_HEADER = os.path.join(ROOT, "include", "chitu_hip_ext.h")
ENTRIES = ("chitu_ext_gqa_qkv_norm_post", "chitu_ext_gqa_qkv_norm_post_kv_fp8", "chitu_ext_qk_norm_rope")
CASES = [(bs, hq, hkv, layout) for bs in (1, 3) for hq, hkv in ((8, 2), (3, 1)) for layout in (0, 1)]


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("bs,hq,hkv,layout", CASES)
def test_oracle_against_a_float64_statement(bs, hq, hkv, layout):
    """The central candidate against float64 with the intermediate bf16 rounding kept.  fp32 against float64 moves rr by at most
    an ulp, which can move n across a bf16 rounding boundary: one bf16 ulp of n, 2^-7 |n|.  The rotation then adds the two
    products' fp32 roundings and its own bf16 rounding, 2^-8 (|n0| + |n1|) with room.  Bound per element: 2^-6 (|n0| + |n1|)."""
    c = qx.qk_case(bs, hq, hkv, seed=layout)
    for part, w in ((slice(0, hq), c["q_w"]), (slice(hq, hq + hkv), c["k_w"])):
        x = c["x"][:, part]
        _, _, y = qx.head_candidates(x, w, c["cos"], c["sin"], layout)
        n, o = qx.head_float64(x, w, c["cos"], c["sin"], layout)
        pair = (n[..., 0::2].abs() + n[..., 1::2].abs()).repeat_interleave(2, -1) if layout == 0 else \
            (n[..., :64].abs() + n[..., 64:].abs()).repeat(1, 1, 2)
        assert bool(((y[0].double() - o).abs() <= pair * 2.0 ** -6).all())
        if bs > 1:  # (a batch of one sits at position 0, where the rotation is the identity and o is a bf16 number already)
            assert float((y[0].double() - o).abs().max()) > 0  # the comparison is not vacuous: the last rounding is visible


def test_oracle_candidates_differ_from_each_other():
    """The neighbours of rr are not all absorbed by the bf16 rounding: some head tells them apart, so "equals one candidate"
    pins rr to +-RSQRT_RADIUS ulps on those heads."""
    c = qx.qk_case(17, 8, 8)
    _, _, y = qx.head_candidates(c["x"][:, :8], c["q_w"], c["cos"], c["sin"], 1)
    assert y.shape[0] == 2 * qx.RSQRT_RADIUS + 1
    assert any(not torch.equal(y[0], y[k]) for k in range(1, y.shape[0]))


def test_oracle_tells_every_wrong_variant_apart():
    """weight applied before rr, no intermediate bf16 rounding, norm after RoPE, layouts swapped: for each, at least one head of
    the cases equals NO candidate of the oracle."""
    told = {}
    for bs, hq, hkv, layout in CASES:
        c = qx.qk_case(bs, hq, hkv, seed=layout)
        x = c["x"][:, :hq]
        _, _, y = qx.head_candidates(x, c["q_w"], c["cos"], c["sin"], layout)
        yb = qx.bits(y).reshape(y.shape[0], -1, 128)
        for name, got in qx.wrong_variants(x, c["q_w"], c["cos"], c["sin"], layout).items():
            hit = (qx.bits(got).reshape(-1, 128)[None] == yb).all(-1).any(0)  # per head: equals some candidate
            told[name] = told.get(name, 0) + int((~hit).sum())
    assert set(told) == {"weight applied before rr", "no intermediate bf16 rounding", "norm after RoPE", "layouts swapped"}
    assert all(n > 0 for n in told.values()), told


def test_position_zero_leaves_the_normalised_head_alone():
    """cos = 1, sin = 0: the kernel's output at position 0 is the norm alone (every batch of the cases has such a row)."""
    c = qx.qk_case(3, 8, 2)
    assert int(c["pos"][0]) == 0 and bool((c["cos"][0] == 1).all()) and bool((c["sin"][0] == 0).all())
    t, rr, y = qx.head_candidates(c["x"][:1, :8], c["q_w"], c["cos"][:1], c["sin"][:1], 1)
    assert torch.equal(y[0], qx.rms_rows(c["x"][0, :8], c["q_w"], rr[0]).view(1, 8, 128))


def test_fp8_rows_are_the_statement_of_the_gqa_fp8_host_tests():
    from tests.test_gqa_kv_fp8_host import quant_ref

    x = (torch.randn(5, 3, 128, generator=torch.Generator().manual_seed(1)) * 7).to(torch.bfloat16)
    assert torch.equal(qx.fp8_rows(x), quant_ref(x))


# ---------------------------------------------------------------- the extension header and the entries' host checks
def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_extension_header_declares_exactly_the_exported_ext_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(EXT_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(chitu_ext_\w+)\s*\(", src)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib().LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT\s+(chitu_ext_\w+)", out)))
    assert declared == exported == sorted(ENTRIES)
    assert re.search(r"#define\s+CHITU_HIP_EXT_VERSION\s+1\b", src) and '#include "chitu_hip.h"' in src
    assert not re.findall(r"\bint\s+(chitu_hip_\w+)\s*\(", src)  # nothing of the frozen prefix is declared here


def _post_args(p, head_dim=128, null=None):
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    a = [p, i64(48 * 128), i32(32), i32(8), i32(head_dim), p, p, i32(1), p, p, i64(4), i32(16), p, i32(2), p, i32(1), p, p, f32(1e-6), None]
    if null is not None:
        a[null] = None
    return a


def _rope_args(p, head_dim=128, null=None):
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    a = [p, p, p, p, p, p, p, p, f32(1e-6), i64(1), i32(4), i32(2), i32(head_dim)] + [i64(1024), i64(128)] * 4 + [i32(1), None]
    if null is not None:
        a[null] = None
    return a


def test_entries_refuse_other_head_dims_and_null_pointers_on_the_host():
    """Argument checks run before anything is launched (the pointers are host memory and are never dereferenced; with a launch
    these calls would fault or return a HIP error, not -2 / -1)."""
    lib = ctypes.CDLL(_lib().LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    for name in ENTRIES[:2]:
        fn = getattr(lib, name)
        assert fn(*_post_args(p, head_dim=64)) == -2, name
        for null in (0, 5, 6, 8, 9, 12, 14, 16, 17):  # qkv, cos, sin, both caches, table, lengths, both weights
            assert fn(*_post_args(p, null=null)) == -1, (name, null)
        a = _post_args(p)
        a[15] = ctypes.c_int32(0)
        assert fn(*a) == 0  # zero rows: nothing is launched
    fn = lib.chitu_ext_qk_norm_rope
    assert fn(*_rope_args(p, head_dim=64)) == -2
    for null in range(8):
        assert fn(*_rope_args(p, null=null)) == -1, null
    a = _rope_args(p)
    a[9] = ctypes.c_int64(0)
    assert fn(*a) == 0
    a = _rope_args(p)
    a[13] = ctypes.c_int64(1028)  # a row stride that leaves heads off 16-byte boundaries
    assert fn(*a) == -1


# ---------------------------------------------------------------- the loader
def _tiny_state():
    g, cfg = qr.fixture()
    return g, cfg, qr.qwen3_hf_params(g)


def test_loader_keeps_head_norms_whole_and_splits_merged_qkv_by_head_dim():
    from chitu_amd.checkpoint import preprocess_hf_llama, to_llama_module_names

    _, cfg, hf = _tiny_state()
    hq, hkv, hd, dim = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["hidden_size"]
    assert dim // hq != hd  # the point of the fixture's shape
    merged = {}
    for k, v in hf.items():  # a file that ships qkv merged: TP has to split it by heads first
        if k.endswith("self_attn.q_proj.weight"):
            pre = k[: -len("q_proj.weight")]
            merged[pre + "qkv_proj.weight"] = torch.cat([v, hf[pre + "k_proj.weight"], hf[pre + "v_proj.weight"]], 0)
        elif not (k.endswith("self_attn.k_proj.weight") or k.endswith("self_attn.v_proj.weight")):
            merged[k] = v
    for state in (hf, merged):
        for rank in (0, 1):
            st = to_llama_module_names(preprocess_hf_llama(state, hq, hkv, dim, rank, 2, head_dim=hd))
            for i in range(cfg["num_hidden_layers"]):
                pre = f"model.layers.{i}.self_attn."
                assert torch.equal(st[f"layers.{i}.attn.q_norm"], hf[pre + "q_norm.weight"])
                assert torch.equal(st[f"layers.{i}.attn.k_norm"], hf[pre + "k_norm.weight"])
                q, k, v = (hf[pre + n + "_proj.weight"] for n in "qkv")
                want = torch.cat([q.chunk(2, 0)[rank], k.chunk(2, 0)[rank], v.chunk(2, 0)[rank]], 0)
                assert want.shape == ((hq + 2 * hkv) // 2 * hd, dim)
                assert torch.equal(st[f"layers.{i}.attn.wqkv"], want)
    with pytest.raises(RuntimeError):  # the derived quotient 256 // 4 = 64 cannot split 1024 merged rows
        preprocess_hf_llama(merged, hq, hkv, dim, 0, 2)
    one = to_llama_module_names(preprocess_hf_llama(hf, hq, hkv, dim))  # TP 1, no head_dim: what it always did
    assert torch.equal(one["layers.0.attn.wqkv"], torch.cat([hf["model.layers.0.self_attn." + n + "_proj.weight"] for n in "qkv"], 0))


def _cpu_decoder(cfg, **over):
    from chitu_amd.qwen3 import Qwen3Decoder

    return Qwen3Decoder(qr.qwen3_args(cfg, **over), None, None, max_position_embeddings=64, device="cpu")


def test_loader_fills_a_tied_head_from_the_embedding(tmp_path):
    from chitu_amd.checkpoint import load_checkpoint_hf_llama

    _, cfg, hf = _tiny_state()
    tied = {k: v for k, v in hf.items() if k != "lm_head.weight"}
    model = _cpu_decoder(cfg, tie_word_embeddings=True)
    load_checkpoint_hf_llama(model, qr.write_hf_dir(tied, str(tmp_path / "tied")))
    assert torch.equal(model.head_weight, hf["model.embed_tokens.weight"]) and torch.equal(model.embed_weight, model.head_weight)
    assert torch.equal(model.layers[1].attn.k_norm, hf["model.layers.1.self_attn.k_norm.weight"])
    assert model.layers[0].attn.rotary_type == "hf-llama" and model.layers[0].attn.wqkv.shape == (8 * 128, 256)
    untied = _cpu_decoder(cfg)
    with pytest.raises(KeyError):  # without the flag a missing head stays an error
        load_checkpoint_hf_llama(untied, str(tmp_path / "tied"))
    load_checkpoint_hf_llama(untied, qr.write_hf_dir(hf, str(tmp_path / "full")))
    assert torch.equal(untied.head_weight, hf["lm_head.weight"])


def test_loader_still_refuses_a_bias(tmp_path):
    from chitu_amd.checkpoint import load_checkpoint_hf_llama

    _, cfg, hf = _tiny_state()
    for n in "qkv":
        hf[f"model.layers.0.self_attn.{n}_proj.bias"] = torch.zeros(hf[f"model.layers.0.self_attn.{n}_proj.weight"].shape[0], dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        load_checkpoint_hf_llama(_cpu_decoder(cfg), qr.write_hf_dir(hf, str(tmp_path / "bias")))


def test_llama_args_without_the_flag_build_no_head_norm():
    from chitu_amd.llama import LlamaArgs, LlamaDecoder

    m = LlamaDecoder(LlamaArgs(dim=256, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=64, ffn_dim=128), None, None,
                     max_position_embeddings=16, device="cpu")
    assert not any("q_norm" in n or "k_norm" in n for n, _ in m.named_parameters()) and m.layers[0].attn.rotary_type == "llama"


# ---------------------------------------------------------------- the Hugging Face fixture
def test_hf_bf16_run_is_within_the_bar_of_its_fp32_run():
    """A bf16 implementation can meet the bar: Hugging Face's own does."""
    g, _ = qr.fixture()
    err, agree = qr.check_logits(torch.from_numpy(g["logits_bf16"]), g, "HF bf16 vs HF fp32")
    assert g["logits_fp32"].shape == (33, 512) and g["k0_fp32"].shape == (39, 2, 128)


def test_cpu_restatement_reproduces_the_hf_fp32_run():
    g, cfg, hf = _tiny_state()
    args = qr.qwen3_args(cfg)
    p = qr.module_params(hf, args)
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    logits, k0 = qr.forward(p, prompt + toks[:-1], args)
    assert_close(k0.float(), torch.from_numpy(g["k0_fp32"]), 1e-2, what="layer 0 k rows after norm + RoPE")
    qr.check_logits(logits[len(prompt) - 1:], g, "CPU restatement vs HF fp32")


# ---------------------------------------------------------------- the decoder's wiring on the CPU
def test_qwen3_decoder_wiring_on_the_cpu_reproduces_the_hf_fp32_run(tmp_path, monkeypatch):
    """Qwen3Decoder's host-side logic (the head-norm branches of LlamaAttention, the loader, the paged cache) with every HIP op
    swapped for the oracle (tests/cpu_ops_shim.py) and the two head-norm ops for the restatement of tests/qwen3_ref.py: prefill
    of the prompt, then 32 eager decode steps fed the fixture's tokens.  The kernels themselves are the GPU tests' business."""
    from chitu_amd import ops
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.checkpoint import load_checkpoint_hf_llama
    from chitu_amd.qwen3 import Qwen3Decoder
    from tests import cpu_ops_shim as shim
    from tests.row_exact import rope_oracle

    shim.install_llama(monkeypatch.setattr)

    def qk_norm_rope(q, k, q_w, k_w, eps, cos, sin, rotary_type="hf-llama"):
        layout = 0 if rotary_type == "llama" else 1
        return rope_oracle(qr.rms_norm(q, q_w, eps), cos, sin, layout), rope_oracle(qr.rms_norm(k, k_w, eps), cos, sin, layout)

    def gqa_qkv_norm_post(qkv, hq, hkv, cos, sin, k_cache, v_cache, table, lens, q_w, k_w, eps, rotary_type="llama"):
        q, k = qk_norm_rope(qkv[:, :hq], qkv[:, hq:hq + hkv], q_w, k_w, eps, cos, sin, rotary_type)
        page = k_cache.shape[1]
        for b in range(qkv.shape[0]):
            L = int(lens[b])
            k_cache[int(table[b][L // page])][L % page] = k[b]
            v_cache[int(table[b][L // page])][L % page] = qkv[b, hq + hkv:]
        return q

    monkeypatch.setattr(ops, "qk_norm_rope", qk_norm_rope)
    monkeypatch.setattr(ops, "gqa_qkv_norm_post", gqa_qkv_norm_post)
    monkeypatch.setattr(ops, "gqa_qkv_post", None)  # a Qwen3 block must not take the launches without the norm
    monkeypatch.setattr(ops, "apply_rotary_pos_emb", None)
    monkeypatch.setattr(ops, "bf16_linear_add_norm_qkv_post", None)
    g, cfg, hf = _tiny_state()
    args = qr.qwen3_args(cfg)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=1, block_size=16, max_seq_len=64, device="cpu",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=torch.bfloat16)
    model = Qwen3Decoder(args, cache, shim.CpuGqaBackend(), max_position_embeddings=64, device="cpu")
    load_checkpoint_hf_llama(model, qr.write_hf_dir(hf, str(tmp_path / "qwen3")))
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    rows = [model.prefill([prompt], ["r"]).float()]
    for step in range(32):
        cache.prepare_cache_decode(["r"])
        cache.prepare_block_table_for_decode(["r"])
        rows.append(model.decode(torch.tensor([toks[step]]), use_graph=False).float())
        cache.finalize_cache_single_decode(["r"])
    qr.check_logits(torch.cat(rows), g, "CPU wiring vs HF fp32")
    pages = torch.tensor(cache.block_table["r"])
    k_rows = cache.paged_k_cache[0][pages].flatten(0, 1)[:39].float()
    assert_close(k_rows, torch.from_numpy(g["k0_fp32"]), 1e-2, what="layer 0 K page rows")
