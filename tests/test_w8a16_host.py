"""W8A16 weight-only int8 linears, the parts that need no GPU: the sixth extension header against the library's exports, the
host-side argument checks of its entries, the quantiser against its formula, the Python surface, the launch-plan mirror over the
GPU test's shape list, and the checkpoint loader's per-rank quantisation."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from tests import w8a16_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT6_HEADER = os.path.join(ROOT, "include", "chitu_hip_ext6.h")
ENTRIES = ("chitu_ext6_w8a16_gemm", "chitu_ext6_w8a16_gemm_silu", "chitu_ext6_w8a16_scale_round", "chitu_ext6_w8a16_widen")


def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


# ---------------------------------------------------------------- the header
def test_ext6_header_declares_exactly_the_exported_ext6_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(EXT6_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(chitu_ext6_\w+)\s*\(", src)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib().LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT\s+(chitu_ext6_\w+)", out)))
    assert declared == exported == sorted(ENTRIES)
    assert re.search(r"#define\s+CHITU_HIP_EXT6_VERSION\s+1\b", src) and '#include "chitu_hip.h"' in src
    assert not re.findall(r"\bint\s+(chitu_hip_\w+|chitu_ext\d?_\w+)\s*\(", src.replace("chitu_ext6_", "chitu_six_"))  # no earlier prefix


# ---------------------------------------------------------------- host argument checks
I32, I64 = ctypes.c_int32, ctypes.c_int64


def _gemm_args(p, rows, **over):
    a = dict(x=p, w=p, scale=p, out=p, out_dtype=I32(0), M=I64(rows), N=I64(24), K=I64(192), stream=None)
    a.update(over)
    return list(a.values())


def _silu_args(p, rows, **over):
    a = dict(x=p, w=p, scale=p, out=p, M=I64(rows), inter=I64(24), K=I64(192), stream=None)
    a.update(over)
    return list(a.values())


def _widen_args(p, rows, **over):
    a = dict(w=p, out=p, N=I64(rows), K=I64(192), stream=None)
    a.update(over)
    return list(a.values())


def _round_args(p, rows, **over):
    a = dict(acc=p, scale=p, out=p, out_dtype=I32(0), M=I64(rows), N=I64(24), silu=I32(0), stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("rows", [0, 3])
def test_entries_check_their_arguments_on_the_host(rows):
    """Argument checks run before anything is launched and before the zero-size return: the pointers are host memory and are
    never dereferenced (with a launch these calls would return a HIP error or fault, not -1 / -2)."""
    lib = ctypes.CDLL(_lib().LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 8)
    gemm, silu, widen, rnd = (lib.chitu_ext6_w8a16_gemm, lib.chitu_ext6_w8a16_gemm_silu, lib.chitu_ext6_w8a16_widen,
                              lib.chitu_ext6_w8a16_scale_round)
    for name in ("x", "w", "scale", "out"):
        assert gemm(*_gemm_args(p, rows, **{name: None})) == -1, name
        assert gemm(*_gemm_args(p, rows, **{name: odd})) == -1, name
        assert silu(*_silu_args(p, rows, **{name: None})) == -1, name
        assert silu(*_silu_args(p, rows, **{name: odd})) == -1, name
    for bad in (dict(out_dtype=I32(3)), dict(out_dtype=I32(-1)), dict(M=I64(-1)), dict(N=I64(0)), dict(K=I64(0)), dict(K=I64(-64)),
                dict(N=I64(1 << 30)), dict(K=I64(1 << 30)), dict(M=I64(1 << 30))):
        assert gemm(*_gemm_args(p, rows, **bad)) == -1, bad
    for bad in (dict(M=I64(-1)), dict(inter=I64(0)), dict(K=I64(0)), dict(inter=I64(1 << 29)), dict(K=I64(1 << 30))):
        assert silu(*_silu_args(p, rows, **bad)) == -1, bad
    for k in (32, 96, 100, 191):  # K must be a multiple of 64
        assert gemm(*_gemm_args(p, rows, K=I64(k))) == -2 and silu(*_silu_args(p, rows, K=I64(k))) == -2, k
    for name in ("w", "out"):
        assert widen(*_widen_args(p, rows, **{name: None})) == -1 and widen(*_widen_args(p, rows, **{name: odd})) == -1, name
    for bad in (dict(N=I64(-1)), dict(K=I64(0)), dict(K=I64(1 << 30)), dict(N=I64(1 << 30))):
        assert widen(*_widen_args(p, rows, **bad)) == -1, bad
    assert widen(*_widen_args(p, rows, K=I64(24))) == -2
    for name in ("acc", "scale", "out"):
        assert rnd(*_round_args(p, rows, **{name: None})) == -1 and rnd(*_round_args(p, rows, **{name: odd})) == -1, name
    for bad in (dict(out_dtype=I32(3)), dict(silu=I32(2)), dict(silu=I32(1), out_dtype=I32(2)), dict(M=I64(-1)), dict(N=I64(0)),
                dict(N=I64(1 << 29))):
        assert rnd(*_round_args(p, rows, **bad)) == -1, bad
    if rows == 0:  # nothing to do: 0 with nothing launched, valid arguments otherwise
        assert gemm(*_gemm_args(p, 0)) == 0 and silu(*_silu_args(p, 0)) == 0 and widen(*_widen_args(p, 0)) == 0
        assert rnd(*_round_args(p, 0)) == 0 and rnd(*_round_args(p, 0, silu=I32(1))) == 0


# ---------------------------------------------------------------- the quantiser
def test_quant_weight_w8a16_against_its_formula():
    from chitu_amd.quantize import dequant_weight_w8a16, quant_weight_w8a16
    from chitu_amd.quantize.w8a8 import quant_weight

    g = torch.Generator().manual_seed(5)
    w = (torch.randn(37, 192, generator=g) * 0.07).to(torch.bfloat16)
    w[3] = 0  # a zero row: the clamp keeps the scale at 1e-5 / 127, the codes at 0
    w[5] = -w[5].abs() - 0.01  # a row whose maximum is negative: the scale comes from max |w|
    q, s = quant_weight_w8a16(w)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and tuple(q.shape) == (37, 192) and tuple(s.shape) == (37,)
    wf = w.float()
    s_ref = wf.abs().max(dim=-1)[0].clamp(min=1e-5) / 127.0
    q_ref = torch.clamp(torch.round(wf / s_ref.view(-1, 1)), -127, 127).to(torch.int8)
    assert torch.equal(s, s_ref) and torch.equal(q, q_ref)
    assert float(s[3]) == pytest.approx(1e-5 / 127.0, rel=1e-6) and int(q[3].abs().max()) == 0
    assert float(w[5].max()) < 0 and int(q[5].min()) == -127 and int(q[5].max()) < 0 and float(s[5]) == float(wf[5].abs().max() / 127.0)
    assert int(q.abs().max()) == 127 and bool((q.abs().max(dim=-1)[0][torch.arange(37) != 3] == 127).all())
    assert torch.equal(dequant_weight_w8a16(q, s), q.float() * s.view(-1, 1))
    # round-to-nearest: half a step per element.  The quantiser divides in fp32: w / s (at most 127 in magnitude) is off by at
    # most 127 * 2^-24 of a step before it is rounded to a code, which is all the slack there is; the product is taken in fp64.
    err = (q.double() * s.double().view(-1, 1) - wf.double()).abs()
    assert bool((err <= s.double().view(-1, 1) * (0.5 + 127 * 2.0 ** -24)).all())
    q8, s8 = quant_weight(wf)  # the W8A8 quantiser's formulas (no clamp there: the codes cannot leave [-127, 127] anyway)
    assert torch.equal(q8, q) and torch.equal(s8, s)


# ---------------------------------------------------------------- the Python surface
def test_signatures_of_the_new_functions_and_the_quant_field():
    from chitu_amd import ops, quantize
    from chitu_amd.deepseek_v3 import DeepSeekV3Args
    from chitu_amd.llama import LlamaArgs
    from chitu_amd.mixtral import MixtralArgs
    from chitu_amd.quantize import w8a16
    from chitu_amd.qwen2 import Qwen2Args
    from chitu_amd.qwen3 import Qwen3Args
    from chitu_amd.qwen3_moe import Qwen3MoeArgs

    def names(f):
        return list(inspect.signature(f).parameters)

    assert names(ops.w8a16_linear) == ["x", "q_weight", "scale", "out_dtype"]
    assert inspect.signature(ops.w8a16_linear).parameters["out_dtype"].default is None
    assert names(ops.w8a16_linear_silu) == ["x", "q_w13", "scale"]
    assert names(ops.w8a16_plan) == ["M", "N", "K", "silu"]
    assert names(w8a16.WeightOnlyLinear.__init__) == ["self", "in_features", "out_features", "bias", "name"]
    assert names(w8a16.quant_weight_w8a16) == ["w"] and names(w8a16.dequant_weight_w8a16) == ["q", "s"]
    assert names(w8a16.quantize_w8a16_) == ["decoder"] and names(w8a16.replace_with_w8a16)[0] == "model"
    for fn in ("WeightOnlyLinear", "quant_weight_w8a16", "dequant_weight_w8a16", "replace_with_w8a16", "quantize_w8a16_"):
        assert getattr(quantize, fn) is getattr(w8a16, fn)
    for cls in (LlamaArgs, Qwen2Args, Qwen3Args):
        assert cls().quant is None and cls(quant="w8a16").quant == "w8a16"
    for cls in (MixtralArgs, Qwen3MoeArgs, DeepSeekV3Args):
        assert cls().quant is None
        with pytest.raises(ValueError):
            cls(quant="w8a16")


def test_decoder_refuses_an_unknown_quant_and_builds_int8_parameters_for_w8a16():
    from chitu_amd.llama import LlamaArgs, LlamaDecoder

    small = dict(dim=256, n_layers=1, n_heads=2, n_kv_heads=1, vocab_size=64, ffn_dim=128)
    with pytest.raises(ValueError):
        LlamaDecoder(LlamaArgs(quant="w4a16", **small), None, None, max_position_embeddings=16, device="cpu")
    m = LlamaDecoder(LlamaArgs(quant="w8a16", **small), None, None, max_position_embeddings=16, device="cpu")
    p = dict(m.named_parameters())
    for name, shape in (("attn.wqkv", (512, 256)), ("attn.wo", (256, 256)), ("ffn.w13", (256, 256)), ("ffn.w2", (256, 128))):
        assert p[f"layers.0.{name}"].dtype == torch.int8 and tuple(p[f"layers.0.{name}"].shape) == shape
        assert p[f"layers.0.{name}_scale"].dtype == torch.float32 and tuple(p[f"layers.0.{name}_scale"].shape) == shape[:1]
    assert p["head_weight"].dtype == p["embed_weight"].dtype == p["layers.0.attn_norm"].dtype == torch.bfloat16


def test_quantize_w8a16_converts_a_decoder_in_place_and_leaves_the_rest():
    from chitu_amd.llama import LlamaArgs, LlamaDecoder, _fuses_norm, init_synthetic_
    from chitu_amd.quantize import quant_weight_w8a16, quantize_w8a16_

    m = LlamaDecoder(LlamaArgs(dim=256, n_layers=2, n_heads=2, n_kv_heads=1, vocab_size=64, ffn_dim=128), None, None,
                     max_position_embeddings=16, device="cpu")
    init_synthetic_(m, seed=1)
    before = {k: v.clone() for k, v in m.named_parameters()}
    assert quantize_w8a16_(m) is m and m.args.quant == "w8a16"
    after = dict(m.named_parameters())
    for k, v in before.items():
        if re.search(r"\.(wqkv|wo|w13|w2)$", k):
            q, s = quant_weight_w8a16(v)
            assert torch.equal(after[k], q) and torch.equal(after[k + "_scale"], s) and not after[k].requires_grad
        else:
            assert torch.equal(after[k], v) and after[k].dtype == torch.bfloat16
    assert len(after) == len(before) + 8
    x, pend = torch.zeros(1, 256, dtype=torch.bfloat16), torch.zeros(1, 256, dtype=torch.bfloat16)
    assert not _fuses_norm(x, pend, 512, weight=m.layers[0].attn.wqkv)  # int8 weights: no norm-prologue form
    assert _fuses_norm(x, pend, 512, weight=before["layers.0.attn.wqkv"]) == _fuses_norm(x, pend, 512)


def test_quant_dispatches_w8a16_replaces_linears_and_skips_the_head():
    from chitu_amd.quantize import WeightOnlyLinear, quant, quant_weight_w8a16

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.proj = torch.nn.Linear(128, 64, bias=False)
            self.block = torch.nn.Sequential(torch.nn.Linear(64, 32, bias=True), torch.nn.ReLU())
            self.odd = torch.nn.Linear(48, 8)  # in_features no multiple of 64: stays
            self.lm_head = torch.nn.Linear(64, 100, bias=False)
            self.head = torch.nn.Linear(64, 100, bias=False)

    m = Tiny()
    w = m.proj.weight.data.clone()
    assert quant(m, "w8a16") is m
    assert isinstance(m.proj, WeightOnlyLinear) and isinstance(m.block[0], WeightOnlyLinear)
    assert type(m.lm_head) is torch.nn.Linear and type(m.head) is torch.nn.Linear and type(m.odd) is torch.nn.Linear
    q, s = quant_weight_w8a16(w)
    assert torch.equal(m.proj.q_weight, q) and torch.equal(m.proj.q_scale_col, s) and m.proj.bias is None
    assert tuple(m.proj.q_weight.shape) == (64, 128) and m.block[0].bias is not None and m.proj.name == "proj"
    assert sorted(k for k, _ in m.proj.named_buffers()) == ["q_scale_col", "q_weight"]
    with pytest.raises(NotImplementedError):
        quant(m, "awq")


def test_fused_experts_still_refuses_w8a16():
    from chitu_amd import fused_moe

    assert "use_int8_w8a16" in inspect.signature(fused_moe.fused_experts).parameters
    x, w1, w2 = torch.zeros(2, 128, dtype=torch.bfloat16), torch.zeros(4, 256, 128, dtype=torch.bfloat16), torch.zeros(4, 128, 128, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):  # W8A16 experts are out of scope: refused before anything is looked at
        fused_moe.fused_experts(x, w1, w2, torch.ones(2, 2, dtype=torch.bfloat16), torch.zeros(2, 2, dtype=torch.int64), use_int8_w8a16=True)


# ---------------------------------------------------------------- the launch plan
def test_plan_mirror_covers_every_instantiation_over_the_gpu_grid():
    from chitu_amd import ops

    lin, forms = wr.instantiations(ops.w8a16_plan, wr.GRID, silu=False)
    assert lin == wr.ALL_LINEAR and forms == {"stream"}
    sil, forms = wr.instantiations(ops.w8a16_plan, wr.GRID, silu=True)
    assert sil == wr.ALL_SILU and forms == {"stream"}
    M, N, K = wr.TILED_CASE
    assert ops.w8a16_plan(M, N, K)["form"] == "tiled" and ops.w8a16_plan(M, N // 2, K, silu=True)["form"] == "tiled"
    # the K split: one wave per 128-element step up to 8, never an idle wave; the half-line tail is a step of its own
    assert [ops.w8a16_plan(1, 16, k)["launches"][0][1] for k in wr.KS] == [1, 1, 2, 4, 8]
    # M walked in 32-row launches: 16-row tail -> MT 1, anything longer -> MT 2
    assert [m for m, _, _ in ops.w8a16_plan(33, 16, 512)["launches"]] == [2, 1] and [m for m, _, _ in ops.w8a16_plan(17, 16, 512)["launches"]] == [2]
    # the grid bound of the bf16 stream: at most 4096 workgroup-waves (Llama-3-8B's w13: 1792 tiles -> 2 waves)
    assert ops.w8a16_plan(1, 28672, 4096)["launches"] == [(1, 2, 4)] and ops.w8a16_plan(1, 14336, 4096, silu=True)["launches"] == [(1, 4, 3)]
    assert ops.w8a16_plan(1, 3584, 2368)["launches"] == [(1, 8, 4)]  # Qwen2-7B's w2 at TP 8: K = 37 x 64, 18 lines and a half line
    # the token count of the tiled form: the measured rule, and never outside the bf16 GEMM's own (M >= 256, or M >= 128 with
    # >= 1024 rows), so that the GEMM over the widened weights is the compute-shaped one
    assert not ops.w8a16_tiled(127, 28672, 4096) and ops.w8a16_tiled(128, 6144, 4096) and not ops.w8a16_tiled(128, 6143, 4096)
    assert not ops.w8a16_tiled(191, 4096, 4096) and ops.w8a16_tiled(192, 1024, 4096) and not ops.w8a16_tiled(192, 1023, 4096)
    assert not ops.w8a16_tiled(255, 512, 4096) and ops.w8a16_tiled(256, 16, 64) and not ops.w8a16_tiled(256, 16, 1 << 23)
    for M in range(1, 300):
        for n in (16, 1023, 1024, 4096, 6144, 28672):
            assert not ops.w8a16_tiled(M, n, 4096) or M >= 256 or (M >= 128 and n >= 1024), (M, n)
    assert ops.w8a16_plan(0, 16, 64) == {"form": "none", "launches": []}


# ---------------------------------------------------------------- the loader
def _tiny_args(**kw):
    from chitu_amd.llama import LlamaArgs
    from tests.util import HF_LLAMA_TINY

    c = dict(HF_LLAMA_TINY, dim=512)
    return c, LlamaArgs(dim=c["dim"], n_layers=c["n_layers"], n_heads=c["n_heads"], n_kv_heads=c["n_kv_heads"], vocab_size=c["vocab_size"],
                        ffn_dim=c["ffn_dim"], **kw)


QUANTISED = re.compile(r"\.(wqkv|wo|w13|w2)$")


@pytest.mark.parametrize("world", [1, 2])
def test_loader_state_is_the_quantiser_of_each_ranks_shard_bit_for_bit(world):
    from chitu_amd import checkpoint as ck
    from chitu_amd.quantize import quant_weight_w8a16
    from tests.util import tiny_hf_llama_checkpoint

    c, args = _tiny_args(quant="w8a16")
    hf = tiny_hf_llama_checkpoint("llama", cfg=c)
    for rank in range(world):
        bf = ck.to_llama_module_names(ck.preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim, rank, world))
        st = ck.llama_to_w8a16(bf)
        n_q = 0
        for k, v in bf.items():
            if QUANTISED.search(k):
                q, s = quant_weight_w8a16(v)
                assert torch.equal(st[k], q) and torch.equal(st[k + "_scale"], s) and st[k].dtype == torch.int8, k
                n_q += 1
            else:
                assert st[k] is v, k
        assert n_q == 4 * c["n_layers"] and len(st) == len(bf) + n_q


def test_load_checkpoint_hf_llama_fills_a_w8a16_decoder(tmp_path):
    from safetensors.torch import save_file

    from chitu_amd import checkpoint as ck
    from chitu_amd.llama import LlamaDecoder
    from tests.util import tiny_hf_llama_checkpoint

    c, args = _tiny_args(quant="w8a16")
    hf = tiny_hf_llama_checkpoint("llama", cfg=c)
    save_file({k: v.contiguous() for k, v in hf.items()}, str(tmp_path / "model.safetensors"))
    model = LlamaDecoder(args, None, None, max_position_embeddings=64, device="cpu")
    ck.load_checkpoint_hf_llama(model, str(tmp_path))
    want = ck.llama_to_w8a16(ck.to_llama_module_names(ck.preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim)))
    got = dict(model.named_parameters())
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
    assert got["layers.1.ffn.w13"].dtype == torch.int8 and got["head_weight"].dtype == torch.bfloat16
