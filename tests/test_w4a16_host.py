"""W4A16 g128 on the host: the layout round trip, the quantiser against its formula, the GPTQ repacker, the decoder's parameters
and the header (include/chitu_hip_ext9.h)."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT9_HEADER = os.path.join(ROOT, "include", "chitu_hip_ext9.h")
ENTRIES = ("chitu_ext9_w4a16_gemm", "chitu_ext9_w4a16_gemm_silu", "chitu_ext9_w4a16_widen")
SMALL = dict(dim=256, n_layers=1, n_heads=2, n_kv_heads=1, vocab_size=64)


def test_ext9_header_declares_exactly_the_exported_ext9_symbols():
    from chitu_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(EXT9_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(chitu_ext9_\w+)\s*\(", src)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT\s+(chitu_ext9_\w+)", out)))
    assert declared == exported == sorted(ENTRIES)
    assert re.search(r"#define\s+CHITU_HIP_EXT9_VERSION\s+1\b", src) and '#include "chitu_hip.h"' in src
    assert not re.findall(r"\bint\s+(chitu_hip_\w+|chitu_ext\d?_\w+)\s*\(", src.replace("chitu_ext9_", "chitu_nine_"))  # no earlier prefix


@pytest.mark.parametrize("N,K,halves", [(16, 256, 1), (5, 384, 1), (6, 128, 2)])
def test_unpack_inverts_pack_over_all_codes(N, K, halves):
    from chitu_amd import ops
    from chitu_amd.quantize import pack_w4a16, unpack_w4a16

    u = (torch.arange(N * K) * 7 % 16).to(torch.uint8).view(N, K)  # every code at every position of a dword
    s = torch.rand(N, K // 128, generator=torch.Generator().manual_seed(1)) + 0.1
    packed, scales = pack_w4a16(u, s, halves=halves)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (N, K // 2) and tuple(scales.shape) == ops.w4a16_scale_shape(N, K, halves)
    got_u, got_s = unpack_w4a16(packed, scales, halves=halves)
    assert torch.equal(got_u, u) and torch.equal(got_s, s) and sorted(set(u.flatten().tolist())) == list(range(16))
    if halves == 1:
        again = unpack_w4a16(pack_w4a16(u, s))
        assert torch.equal(again[0], u) and torch.equal(again[1], s)
    # channel k: byte (k // 8) * 4 + k % 4, low nibble for k % 8 < 4, as u ^ 8
    k = 13
    assert int(packed[0, (k // 8) * 4 + k % 4]) >> 4 == int(u[0, k]) ^ 8


def test_quant_weight_w4a16_against_its_formula():
    from chitu_amd.quantize import dequant_weight_w4a16, quant_weight_w4a16

    w = (torch.randn(9, 384, generator=torch.Generator().manual_seed(2)) * 0.05).to(torch.bfloat16)
    w[0, :128] = 0  # an all-zero group: the clamped scale
    w[1, 128:256] = -w[1, 128:256].abs() - 0.01  # a group whose maximum is negative
    u, s = quant_weight_w4a16(w)
    grp = w.double().view(9, 3, 128)
    want_s = (grp.abs().amax(-1).to(torch.float32).clamp(min=1e-5) / 7.0)
    want_u = (torch.clamp(torch.round(w.float().view(9, 3, 128) / want_s.view(9, 3, 1)), -8, 7) + 8).to(torch.uint8).view(9, 384)
    assert u.dtype == torch.uint8 and s.dtype == torch.float32 and torch.equal(s, want_s) and torch.equal(u, want_u)
    assert float(s[0, 0]) == float(torch.tensor(1e-5) / 7.0) and bool((u[0, :128] == 8).all()) and int(u[1, 128:256].min()) == 1
    assert float((dequant_weight_w4a16(u, s) - w.float()).abs().max()) <= float(s.max()) / 2 + 1e-9
    with pytest.raises(ValueError):
        quant_weight_w4a16(torch.zeros(4, 192))


@pytest.mark.parametrize("stored_zero", [7, 8])
def test_from_gptq_repacks_both_zero_point_conventions_and_refuses_the_rest(stored_zero):
    from chitu_amd.quantize import from_gptq, unpack_w4a16

    N, K = 16, 256
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 16, (N, K), generator=g)
    s = (torch.rand(K // 128, N, generator=g) + 0.5).to(torch.float16)
    qweight = torch.zeros(K // 8, N, dtype=torch.int64)
    for i in range(8):
        qweight |= u.t()[i::8] << (4 * i)
    as_int32 = lambda t: ((t + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)  # noqa: E731  (the bit pattern, two's complement)
    qweight = as_int32(qweight)
    qzeros = as_int32(torch.full((K // 128, N // 8), sum(stored_zero << (4 * i) for i in range(8)), dtype=torch.int64))
    got_u, got_s = unpack_w4a16(from_gptq(qweight, qzeros, s, g_idx=torch.arange(K) // 128))
    assert torch.equal(got_u, u.to(torch.uint8)) and torch.equal(got_s, s.t().float())
    bad = qzeros.clone()
    bad[0, 0] = bad[0, 0] ^ 1
    with pytest.raises(ValueError, match="zero point"):
        from_gptq(qweight, bad, s)
    with pytest.raises(ValueError, match="act-order"):
        from_gptq(qweight, qzeros, s, g_idx=torch.arange(K).flip(0) // 128)


def test_decoder_builds_packed_parameters_and_refuses_a_k_off_the_group():
    from chitu_amd import ops, quantize
    from chitu_amd.llama import LlamaArgs, LlamaDecoder

    m = LlamaDecoder(LlamaArgs(quant="w4a16g128", ffn_dim=384, **SMALL), None, None, max_position_embeddings=16, device="cpu")
    a, f = m.layers[0].attn, m.layers[0].ffn
    shapes = {"wqkv": (a.wqkv, 512, 256, 1), "wo": (a.wo, 256, 256, 1), "w13": (f.w13, 768, 256, 2), "w2": (f.w2, 256, 384, 1)}
    for name, (w, n, k, halves) in shapes.items():
        scale = getattr(a if name in ("wqkv", "wo") else f, name + "_scale")
        assert w.dtype == torch.uint8 and tuple(w.shape) == (n, k // 2), name
        assert scale.dtype == torch.float32 and tuple(scale.shape) == ops.w4a16_scale_shape(n, k, halves) == (n // 2, (k + 255) // 256, 4), name
    quantised = {f"layers.0.{p}.{n}{x}" for p, n in (("attn", "wqkv"), ("attn", "wo"), ("ffn", "w13"), ("ffn", "w2")) for x in ("", "_scale")}
    assert all(p.dtype == torch.bfloat16 for k, p in m.named_parameters() if k not in quantised)
    with pytest.raises(ValueError, match="192"):  # w2's local K
        LlamaDecoder(LlamaArgs(quant="w4a16g128", ffn_dim=192, **SMALL), None, None, max_position_embeddings=16, device="cpu")
    with pytest.raises(ValueError):
        LlamaDecoder(LlamaArgs(quant="w4a16", ffn_dim=384, **SMALL), None, None, max_position_embeddings=16, device="cpu")
    lin = quantize.quant(torch.nn.Sequential(torch.nn.Linear(256, 8, bias=False)), "w4a16g128")[0]
    assert isinstance(lin, quantize.W4A16Linear) and tuple(lin.packed.shape) == (8, 128)
