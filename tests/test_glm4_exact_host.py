"""CPU checks of the partial-rotary oracle (tests/glm4_exact.py) against tests/qkv_bias_exact.py's at the full width and against
Hugging Face's modeling_glm at GLM-4's, of the seventh extension header and its entries' host checks, of the loader's ChatGLM key
map, of LlamaAttention's constructor refusals, of Glm4Args' defaults, and of Glm4Decoder's host-side wiring with every HIP op
swapped for an oracle.  No GPU."""

import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import glm4_exact as gx
from tests import glm4_ref as g4
from tests import qkv_bias_exact as bx
from tests.util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT7_HEADER = os.path.join(ROOT, "include", "chitu_hip_ext7.h")
ENTRIES = ["chitu_ext7_gqa_qkv_bias_post", "chitu_ext7_gqa_qkv_bias_post_kv_fp8", "chitu_ext7_qkv_bias_rope", "chitu_ext7_rope"]
BF16 = torch.bfloat16


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("hq,hkv", gx.SHAPES)
def test_oracle_at_the_full_width_is_the_bias_oracle(hq, hkv):
    c = gx.glm4_case(5, hq, hkv, 128, seed=1)
    b = bx.bias_case(5, hq, hkv, seed=1)
    assert torch.equal(c["cos"], b["cos"]) and torch.equal(c["sin"], b["sin"]) and c["cos"].shape == (5, 64)
    for got, want in zip(gx.glm4_oracle(c), bx.bias_oracle(b, 0)):
        assert torch.equal(gx.bits(got), gx.bits(want))


@pytest.mark.parametrize("R", gx.WIDTHS)
def test_oracle_passes_the_channels_behind_the_width_through_and_rotates_the_rest(R):
    c = gx.glm4_case(5, 4, 2, R, seed=2)
    y, q, k, v = gx.glm4_oracle(c)
    assert c["cos"].shape == (5, R // 2)
    assert torch.equal(gx.bits(q[..., R:]), gx.bits(y[:, :4, R:])) and torch.equal(gx.bits(k[..., R:]), gx.bits(y[:, 4:6, R:]))
    assert torch.equal(gx.bits(v), gx.bits(y[:, 6:]))
    # row 0 is position 0: cos 1, sin 0.  Elsewhere the slow pairs at small positions turn by less than bf16 resolves, so
    # "most", not "all", of the rotating channels change -- and every lane chunk of 8 has one that does
    moved = gx.bits(q[1:, :, :R]) != gx.bits(y[1:, :4, :R])
    assert float(moved.float().mean()) > 0.5 and torch.equal(gx.bits(q[0]), gx.bits(y[0, :4]))
    assert bool(moved.view(4, 4, R // 8, 8).any(-1).any(0).all())


def test_oracle_is_hugging_faces_glm_rotation_to_one_bf16_ulp():
    """transformers' modeling_glm.apply_rotary_pos_emb in float64 on the same bf16 inputs and the same fp32 table values: the
    oracle's separately rounded fp32 products can move a result across a bf16 rounding boundary, no further."""
    mg = pytest.importorskip("transformers.models.glm.modeling_glm", reason="this transformers has no glm module")
    c = gx.glm4_case(5, 3, 2, 64, seed=3)
    y, q, k, _ = gx.glm4_oracle(c)
    cos64, sin64 = (torch.cat([t, t], dim=-1).double()[None] for t in (c["cos"], c["sin"]))  # [1, T, 64], as HF's rotary_emb lays it out
    yq, yk = (t.double().transpose(0, 1)[None] for t in (y[:, :3], y[:, 3:5]))  # [1, heads, T, 128]
    want_q, want_k = mg.apply_rotary_pos_emb(yq, yk, cos64, sin64)
    for got, want, name in ((q, want_q, "q"), (k, want_k, "k")):
        want = want[0].transpose(0, 1)
        mag = torch.maximum(got.double().abs(), want.abs()).clamp(min=2.0 ** -126)
        ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)  # spacing of bf16 numbers at that magnitude
        diff = (got.double() - want).abs()
        print(f"GLM4 oracle vs modeling_glm (float64), {name}: worst {float((diff / ulp).max()):.3f} bf16 ulp")
        assert bool((diff <= ulp).all()), name
        assert torch.equal(got[..., 64:].double(), want[..., 64:])  # the pass-through half exactly


# ---------------------------------------------------------------- the header and the entries' host checks
def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_ext7_header_declares_exactly_the_exported_ext7_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(EXT7_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(chitu_ext7_\w+)\s*\(", src)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib().LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT\s+(chitu_ext7_\w+)", out)))
    assert declared == exported == sorted(ENTRIES)
    assert re.search(r"#define\s+CHITU_HIP_EXT7_VERSION\s+1\b", src) and '#include "chitu_hip.h"' in src
    assert not re.findall(r"\bint\s+(chitu_hip_\w+|chitu_ext\d?_\w+)\s*\(", src.replace("chitu_ext7_", "chitu_seven_"))  # no earlier prefix
    # rotary_dim sits directly behind layout in every entry
    assert len(re.findall(r"int32_t\s+layout,\s*int32_t\s+rotary_dim,", src)) == 4


I32, I64 = ctypes.c_int32, ctypes.c_int64


def _post_args(p, R=64, layout=0, head_dim=128, batch=1):
    return [p, I64(36 * 128), I32(32), I32(2), I32(head_dim), p, p, I32(layout), I32(R), p, p, I64(4), I32(16), p, I32(2), p, I32(batch),
            p, None]


def _prefill_args(p, R=64, layout=0, head_dim=128, rows=1):
    return [p, I64(1024), I64(128), p, p, p, p, p, p, I64(rows), I32(4), I32(2), I32(head_dim), I32(layout), I32(R), None]


def _rope_args(p, R=64, layout=0, head_dim=128, dtype=0, batch=1):
    return [p, p, p, p, p, p, I32(dtype), I32(batch), I32(4), I32(2), I32(head_dim), I64(512), I64(128), I64(256), I64(128), I64(512),
            I64(128), I64(256), I64(128), I32(layout), I32(R), None]


@pytest.mark.parametrize("rows", [0, 1])
def test_entries_check_the_rotary_width_and_the_pointers_on_the_host(rows):
    """Argument checks run before anything is launched and before the zero-size return: the pointers are host memory and are
    never dereferenced (with a launch these calls would fault or return a HIP error, not -1 / -2)."""
    lib = ctypes.CDLL(_lib().LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    at = (ctypes.addressof(buf) + 15) & ~15
    p, odd = ctypes.c_void_p(at), ctypes.c_void_p(at + 8)
    forms = [(lib.chitu_ext7_gqa_qkv_bias_post, lambda **kw: _post_args(p, batch=rows, **kw), (5, 6)),
             (lib.chitu_ext7_gqa_qkv_bias_post_kv_fp8, lambda **kw: _post_args(p, batch=rows, **kw), (5, 6)),
             (lib.chitu_ext7_qkv_bias_rope, lambda **kw: _prefill_args(p, rows=rows, **kw), (4, 5)),
             (lib.chitu_ext7_rope, lambda **kw: _rope_args(p, batch=rows, **kw), (4, 5))]
    for fn, args, cos_sin in forms:
        for R in (12, 0, 136, -8, 4, 132):
            assert fn(*args(R=R)) == -1, (fn, R)
        assert fn(*args(R=64, layout=1)) == -2 and fn(*args(R=120, layout=1)) == -2
        assert fn(*args(R=64, layout=2)) == -1
        assert fn(*args(head_dim=64)) == -2
        for at_ in cos_sin:  # a cos / sin base off 16 bytes, and a missing one
            for bad in (odd, None):
                a = args()
                a[at_] = bad
                assert fn(*a) == -1, (fn, at_)
        if rows == 0:  # well-formed, nothing to do: nothing is launched at any width or layout
            assert fn(*args(R=64)) == 0 and fn(*args(R=8)) == 0 and fn(*args(R=128, layout=1)) == 0 and fn(*args(R=128, layout=0)) == 0
    assert lib.chitu_ext7_rope(*_rope_args(p, dtype=1, batch=rows)) == -2 and lib.chitu_ext7_rope(*_rope_args(p, dtype=2, batch=rows)) == -2
    a = _rope_args(p, batch=rows)
    a[12] = I64(132)  # a head stride that leaves heads off 16-byte boundaries
    assert lib.chitu_ext7_rope(*a) == -1


def test_ops_refuse_glm4_where_no_entry_takes_a_width():
    """The ValueError comes before any tensor is looked at."""
    from chitu_amd import ops

    t = torch.zeros(1)
    for call in (lambda: ops.qk_norm_rope(t, t, t, t, 1e-6, t, t, rotary_type="glm4"),
                 lambda: ops.gqa_qkv_norm_post(t, 1, 1, t, t, t, t, t, t, t, t, 1e-6, rotary_type="glm4"),
                 lambda: ops.gqa_qkv_norm_post_kv_fp8(t, 1, 1, t, t, t, t, t, t, t, t, 1e-6, rotary_type="glm4"),
                 lambda: ops.gqa_qkv_post(t, 1, 1, t, t, t, t, t, t, rotary_type="glm4"),
                 lambda: ops.gqa_qkv_post_kv_fp8(t, 1, 1, t, t, t, t, t, t, rotary_type="glm4"),
                 lambda: ops.gqa_qkv_bias_post(t, 1, 1, t, t, t, t, t, t, t, rotary_type="glm5"),
                 lambda: ops.qkv_bias_rope(t, 1, 1, t, t, t, rotary_type="glm5"),
                 lambda: ops.apply_rotary_pos_emb(t, t, t, t, rotary_type="glm5")):
        with pytest.raises(ValueError, match="Unknown rotary type"):
            call()


# ---------------------------------------------------------------- the constructor and the args
def _attention(rotary_type="glm4", **over):
    from chitu_amd.glm4 import Glm4Args
    from chitu_amd.llama import LlamaAttention

    kw = dict(dim=512, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=64, ffn_dim=128)
    kw.update(over)
    return LlamaAttention(Glm4Args(**kw), 0, None, None, device="cpu", rotary_type=rotary_type)


def test_constructor_takes_glm4_with_a_bias_and_refuses_it_without_one_or_with_a_head_norm():
    from chitu_amd.llama import LlamaAttention
    from chitu_amd.qwen3 import Qwen3Args

    a = _attention()
    assert a.rotary_type == "glm4" and a.qkv_bias and a.bqkv.shape == (8 * 128,)
    with pytest.raises(ValueError, match="needs qkv_bias"):
        _attention(qkv_bias=False)
    with pytest.raises(ValueError, match="qk_norm"):
        LlamaAttention(Qwen3Args(dim=512, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=64, ffn_dim=128), 0, None, None, device="cpu",
                       rotary_type="glm4")


def test_glm4_defaults_are_the_reference_yaml():
    """chitu/config/models/glm-4-9b-chat.yaml, typed here."""
    from chitu_amd.glm4 import Glm4Args, Glm4Block, Glm4Decoder

    a = Glm4Args()
    assert (a.dim, a.n_layers, a.n_heads, a.n_kv_heads, a.vocab_size, a.ffn_dim, a.norm_eps, a.rope_theta, a.head_dim) == \
        (4096, 40, 32, 2, 151552, 13696, 1.5625e-07, 5000000.0, 128)
    assert a.qkv_bias and a.rotary_dim == 64 and not a.tie_word_embeddings and a.kv_cache_dtype == "bf16" and a.quant is None
    assert a.sliding_window is None and a.attn_softcap == 0.0
    assert Glm4Block.rotary_type == "glm4" and Glm4Decoder.block_type is Glm4Block


def test_decoder_table_has_the_rotary_width_and_other_models_keep_theirs():
    from chitu_amd.glm4 import Glm4Decoder
    from chitu_amd.llama import precompute_freqs_cis
    from chitu_amd.qwen2 import Qwen2Decoder

    g, cfg = g4.fixture()
    m = Glm4Decoder(g4.glm4_args(cfg, n_layers=1), None, None, max_position_embeddings=32, device="cpu")
    cos, sin = precompute_freqs_cis(64, 32, cfg["rope_theta"])
    assert m.cos_table.shape == (32, 32) and torch.equal(m.cos_table, cos) and torch.equal(m.sin_table, sin)
    from tests import qwen2_ref as q2

    m2 = Qwen2Decoder(q2.qwen2_args(q2.fixture()[1], n_layers=1), None, None, max_position_embeddings=32, device="cpu")
    assert m2.cos_table.shape == (32, 64)


# ---------------------------------------------------------------- the loader
@pytest.mark.parametrize("world", [1, 2])
def test_chatglm_names_load_to_the_tensors_of_the_hf_native_names(world):
    from chitu_amd.checkpoint import map_glm4_names, preprocess_hf_llama, to_llama_module_names

    g, cfg = g4.fixture()
    hf = g4.glm4_hf_params(g)
    chat = g4.chatglm_names(hf)
    assert all(k.startswith("transformer.") for k in chat) and len(chat) == len(hf) - 4 * cfg["num_hidden_layers"] + 1
    mapped = map_glm4_names(chat)
    assert not any(k.startswith("transformer.") or "inv_freq" in k for k in mapped)
    for rank in range(world):
        steps = lambda st: to_llama_module_names(preprocess_hf_llama(st, 4, 2, 512, rank, world, head_dim=128), qkv_bias=True)
        a, b = steps(mapped), steps(hf)
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, rank)
        assert a["layers.0.attn.bqkv"].shape == ((4 + 2 * 2) * 128 // world,) and a["layers.0.ffn.w13"].shape == (1024 // world, 512)
    with pytest.raises(KeyError):
        map_glm4_names({"transformer.encoder.surprise.weight": torch.zeros(1)})


# ---------------------------------------------------------------- the decoder's wiring on the CPU
def test_glm4_decoder_wiring_on_the_cpu_reproduces_the_hf_fp32_run(tmp_path, monkeypatch):
    """Glm4Decoder's host-side logic (the glm4 branches of LlamaAttention, the table of width 64, the loader's key map, the paged
    cache) with every HIP op swapped for the oracle (tests/cpu_ops_shim.py) and the two bias ops for a bf16 add in front of
    tests/glm4_exact.py's rotation: prefill of the prompt from a ChatGLM-named directory, then 32 eager decode steps fed the
    fixture's tokens.  The kernels themselves are the GPU tests' business."""
    from chitu_amd import ops
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.checkpoint import load_checkpoint_hf_llama
    from chitu_amd.glm4 import Glm4Decoder
    from tests import cpu_ops_shim as shim

    shim.install_llama(monkeypatch.setattr)
    calls = {"prefill": 0, "decode": 0}

    def qkv_bias_rope(qkv, hq, hkv, bias, cos, sin, rotary_type="hf-llama"):
        assert rotary_type == "glm4" and cos.shape[-1] == 32
        calls["prefill"] += 1
        y = qkv + bias.view(hq + 2 * hkv, 128)
        return (gx.rotate_partial(y[:, :hq].contiguous(), cos, sin), gx.rotate_partial(y[:, hq:hq + hkv].contiguous(), cos, sin),
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
    monkeypatch.setattr(ops, "gqa_qkv_post", None)  # a GLM-4 block must not take the launches without the bias and the width
    monkeypatch.setattr(ops, "apply_rotary_pos_emb", None)
    monkeypatch.setattr(ops, "bf16_linear_add_norm_qkv_post", None)
    g, cfg = g4.fixture()
    args = g4.glm4_args(cfg)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=1, block_size=16, max_seq_len=64, device="cpu",
                                n_local_kv_heads=args.n_kv_heads, head_dim=args.head_dim, dtype=BF16)
    model = Glm4Decoder(args, cache, shim.CpuGqaBackend(), max_position_embeddings=64, device="cpu")
    load_checkpoint_hf_llama(model, g4.write_hf_dir(g4.chatglm_names(g4.glm4_hf_params(g)), str(tmp_path / "glm4")))
    prompt, toks = g["prompt"].tolist(), g["tokens"].tolist()
    rows = [model.prefill([prompt], ["r"]).float()]
    for step in range(32):
        cache.prepare_cache_decode(["r"])
        cache.prepare_block_table_for_decode(["r"])
        rows.append(model.decode(torch.tensor([toks[step]]), use_graph=False).float())
        cache.finalize_cache_single_decode(["r"])
    assert calls == {"prefill": args.n_layers, "decode": 32 * args.n_layers}
    g4.check_logits(torch.cat(rows), g, "GLM4 CPU wiring vs HF fp32")
    pages = torch.tensor(cache.block_table["r"])
    assert_close(cache.paged_k_cache[0][pages].flatten(0, 1)[:39].float(), torch.from_numpy(g["k0_fp32"]), 1e-2, what="layer 0 K page rows")
    assert_close(cache.paged_v_cache[0][pages].flatten(0, 1)[:39].float(), torch.from_numpy(g["v0_fp32"]), 1e-2, what="layer 0 V page rows")
