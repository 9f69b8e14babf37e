"""Host tests (no GPU) of the MXFP4 W4A8 expert mode: the test-local format reference (tests/mxfp4_ref.py), its link to the
pinned fp8 oracle, the host-side argument checks of the new C entries, and the compiled kernels' ISA."""

import ctypes
import os
import re
import subprocess

import pytest
import torch

from oracle import moe as omoe
from tests import mxfp4_ref as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------- (a) the Python reference of the format
def test_every_code_round_trips_at_every_specified_scale():
    """All 16 codes x scale bytes 2..252 (every product a normal finite number): dequantise, quantise, same bytes back --
    except that a block's scale is chosen by its maximum, so each block here holds one code besides the 6 that fixes the
    exponent at the byte under test; and bf16 holds every value exactly."""
    codes = torch.arange(16, dtype=torch.uint8)
    bytes_ = torch.arange(2, 253, dtype=torch.uint8)
    blocks = torch.full((len(bytes_), 16, 32), 7, dtype=torch.uint8)  # 7 = +6: amax = 6 * 2^X -> floor(log2) - 2 = X
    blocks[:, :, 1::2] = codes[None, :, None]
    packed = mx.pack(blocks)
    scales = bytes_[:, None, None].expand(len(bytes_), 16, 1).contiguous()  # [rows, K/32 = 1]
    f32 = mx.dequant_f32(packed, scales)
    assert torch.isfinite(f32).all()
    tiny = torch.finfo(torch.float32).tiny
    assert ((f32 == 0) | (f32.abs() >= tiny)).all(), "every product is zero or a normal number"
    b16 = mx.dequant(packed, scales)
    assert torch.equal(b16.float(), f32), "bf16 holds e2m1 x 2^n exactly"
    expect = mx.e2m1_value(blocks) * mx.scale_value(scales)
    assert torch.equal(f32, expect.reshape(f32.shape))
    p2, s2 = mx.quant(f32)
    assert torch.equal(s2, scales)
    c2 = mx.unpack(p2).reshape(blocks.shape)
    same = (c2 == blocks) | ((blocks & 7) == 0) & ((c2 & 7) == 0)  # -0 keeps its sign bit: codes 0 and 8 both mean zero
    assert same.all()
    assert torch.equal(mx.unpack(mx.pack(blocks)).reshape(blocks.shape), blocks)
    assert torch.equal(mx.unpack(torch.tensor([0x21], dtype=torch.uint8)), torch.tensor([1, 2], dtype=torch.uint8)), "low nibble = even k"


def test_scale_byte_ff_is_nan_and_zero_block_gets_byte_zero():
    packed = mx.pack(torch.full((1, 32), 2, dtype=torch.uint8))
    assert torch.isnan(mx.dequant_f32(packed, torch.tensor([[255]], dtype=torch.uint8))).all()
    assert torch.isnan(mx.dequant(packed, torch.tensor([[255]], dtype=torch.uint8)).float()).all()
    p, s = mx.quant(torch.zeros(2, 64))
    assert int(s.max()) == 0 and int(p.max()) == 0


def test_quantiser_ties_and_saturation():
    """Round-to-nearest-even on the grid {0, .5, 1, 1.5, 2, 3, 4, 6}; the block maximum 4 puts X at 0 (scale byte 127)."""
    v = torch.zeros(1, 32)
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25, -2.5, 0.2500001, 0.7499999, 2.4999998, 2.5000002]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, -0.0, -2.0, 0.5, 0.5, 2.0, 3.0]
    v[0, : len(ties)] = torch.tensor(ties)
    v[0, 31] = 4.0
    p, s = mx.quant(v)
    assert int(s[0, 0]) == 127
    got = mx.dequant_f32(p, s)[0, : len(ties)]
    assert torch.equal(got, torch.tensor(want))
    # saturation: maximum 7.9 keeps X = 0 (floor(log2 7.9) = 2), and everything above 5 becomes 6
    v = torch.tensor([[7.9, -7.0, 5.0, 5.0000005, 6.1] + [0.0] * 27])
    p, s = mx.quant(v)
    assert int(s[0, 0]) == 127
    assert torch.equal(mx.dequant_f32(p, s)[0, :5], torch.tensor([6.0, -6.0, 4.0, 6.0, 6.0]))


# ---------------------------------------------------------------- (b) the link to the pinned oracle
@pytest.mark.parametrize("M,E,topk,K,I", [(5, 8, 2, 256, 128), (7, 4, 3, 384, 256)])
def test_local_reference_is_the_fp8_oracle_on_fp8_representable_weights(M, E, topk, K, I):
    g = torch.Generator().manual_seed(11 + M)
    w1p, w1s, w1_8, w1_bs = mx.fp8_twin_weights(E, 2 * I, K, g)
    w2p, w2s, w2_8, w2_bs = mx.fp8_twin_weights(E, K, I, g)
    # the premise: scale bytes within +-3 of the tile base, and the fp8 twin IS the MXFP4 tensor, bit for bit
    for p, s, w8, bs in ((w1p, w1s, w1_8, w1_bs), (w2p, w2s, w2_8, w2_bs)):
        R, C = w8.shape[1], w8.shape[2]
        base = (torch.log2(bs).to(torch.int32) + 127).repeat_interleave(128, 1)[:, :R].repeat_interleave(4, 2)
        assert ((s.to(torch.int32) - base).abs() <= 3).all()
        mag = w8.float().abs()
        assert float(mag[mag > 0].min()) >= 2.0 ** -4 and float(mag.max()) <= 48.0
        full = w8.float() * bs.repeat_interleave(128, 1)[:, :R].repeat_interleave(128, 2)[:, :, :C]
        assert torch.equal(mx.dequant_f32(p, s).view(torch.int32), full.view(torch.int32))
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(M)])
    wts = torch.rand(M, topk, generator=g).to(torch.bfloat16)
    ref = omoe.fused_experts_fp8(x, w1_8, w2_8, wts, ids, w1_bs, w2_bs)
    mine = mx.fused_experts_mxfp4(x, w1p, w1s, w2p, w2s, wts, ids)
    assert torch.equal(mine.view(torch.int16), ref.view(torch.int16))
    emap = torch.tensor([0, 1] + [-1] * (E - 2), dtype=torch.int32)
    ref = omoe.fused_experts_fp8(x, w1_8, w2_8, wts, ids, w1_bs, w2_bs, expert_map=emap)
    mine = mx.fused_experts_mxfp4(x, w1p, w1s, w2p, w2s, wts, ids, expert_map=emap)
    assert torch.equal(mine.view(torch.int16), ref.view(torch.int16))


def test_quant_from_fp8_block_is_quant_of_the_dequantised_tensor():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(3, 200, 256, generator=g) * 0.5).to(torch.float8_e4m3fn)
    s = torch.rand(3, 2, 2, generator=g) * 0.02 + 0.01
    p, sc = mx.quant_from_fp8_block(w, s)
    full = w.float() * s.repeat_interleave(128, 1)[:, :200].repeat_interleave(128, 2)
    p2, sc2 = mx.quant(full)
    assert torch.equal(p, p2) and torch.equal(sc, sc2)
    err = (mx.dequant_f32(p, sc) - full).abs().max() / full.abs().max()
    assert float(err) < 0.26  # half a step of the coarsest binade (4 .. 6 -> 1 of 8) is the format's bound


# ---------------------------------------------------------------- (c) ABI: host-side argument checks
def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_new_entries_refuse_bad_shapes_and_null_pointers_on_the_host():
    """Nothing is launched: the pointers are never dereferenced, so this needs no GPU."""
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    nul = ctypes.c_void_p(0)
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    BAD_ARG, UNSUPPORTED = -1, -2

    def g1(K, I, a=p, w=p):
        return lib.chitu_hip_moe_gemm1_silu_mxfp4(a, p, w, p, p, p, p, p, i64(8), i32(2), i64(I), i64(K), i64(8), None)

    def g2(I, N=256, h=p, s=p):
        return lib.chitu_hip_moe_gemm2_quant_mxfp4(h, p, s, p, p, p, p, i32(0), i32(1), p, i64(8), i64(N), i64(I), i64(8),
                                                   f32(1e-10), None)

    def gp(K, N=256, a=p, out=p):
        return lib.chitu_hip_moe_gemm_mxfp4(a, p, i32(1), p, p, p, p, p, p, i32(0), i32(1), out, i64(8), i64(N), i64(K), i64(8), None)

    for K in (127, 129, 64, 7168 + 32, 7168 + 64, 1):  # odd K, K not a multiple of 128
        assert g1(K, 256) == UNSUPPORTED, K
        assert gp(K) == UNSUPPORTED, K
    for I in (64, 192, 16, 257, 129):
        assert g1(256, I) == UNSUPPORTED, I
        assert g2(I) == UNSUPPORTED, I
        assert gp(I) == UNSUPPORTED, I
    assert g2(640) == UNSUPPORTED  # wider than 512: the three-launch form
    assert g1(256, 128, a=nul) == BAD_ARG and g1(256, 128, w=nul) == BAD_ARG
    assert g2(128, h=nul) == BAD_ARG and g2(128, s=nul) == BAD_ARG
    assert gp(256, a=nul) == BAD_ARG and gp(256, out=nul) == BAD_ARG
    # mul_routed_weight without the weights
    assert lib.chitu_hip_moe_gemm_mxfp4(p, p, i32(1), p, p, p, p, p, nul, i32(0), i32(1), p, i64(8), i64(16), i64(128), i64(8), None) == BAD_ARG
    q = lib.chitu_hip_quant_mxfp4
    assert q(p, i32(0), nul, i64(4), i64(48), i64(1), p, p, None) == UNSUPPORTED      # not whole 32-blocks
    assert q(p, i32(3), p, i64(4), i64(96), i64(4), p, p, None) == UNSUPPORTED        # fp8-block input: whole 128-blocks
    assert q(nul, i32(0), nul, i64(4), i64(64), i64(1), p, p, None) == BAD_ARG
    assert q(p, i32(3), nul, i64(4), i64(128), i64(4), p, p, None) == BAD_ARG         # block scales missing
    assert q(p, i32(4), nul, i64(4), i64(64), i64(1), p, p, None) == BAD_ARG
    d = lib.chitu_hip_dequant_mxfp4
    assert d(p, p, i64(4), i64(40), p, None) == UNSUPPORTED
    assert d(p, nul, i64(4), i64(64), p, None) == BAD_ARG and d(p, p, i64(4), i64(64), nul, None) == BAD_ARG
    # empty problems are accepted without a launch
    assert lib.chitu_hip_moe_gemm1_silu_mxfp4(p, p, p, p, p, p, p, p, i64(0), i32(2), i64(128), i64(256), i64(0), None) == 0
    assert q(p, i32(0), nul, i64(0), i64(64), i64(1), p, p, None) == 0


def test_python_surface_refuses_cpu_tensors_and_keeps_the_reference_signature():
    import inspect

    from chitu_amd import fused_moe
    from chitu_amd._lib import HipCallError
    from chitu_amd.quantize import mxfp4

    with pytest.raises(HipCallError):
        mxfp4.quant_mxfp4(torch.zeros(2, 64))
    with pytest.raises(HipCallError):
        mxfp4.dequant_mxfp4(torch.zeros(2, 32, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8))
    with pytest.raises(HipCallError):
        mxfp4.quant_mxfp4_from_fp8_block(torch.zeros(128, 128).to(torch.float8_e4m3fn), torch.ones(1, 1))
    for fn in (fused_moe.fused_experts, fused_moe.fused_experts_impl):
        par = inspect.signature(fn).parameters
        assert list(par)[-1] == "use_mxfp4_w4a8" and par["use_mxfp4_w4a8"].default is False
    x = torch.zeros(2, 256, dtype=torch.bfloat16)
    w1, w1s = torch.zeros(2, 256, 128, dtype=torch.uint8), torch.zeros(2, 256, 8, dtype=torch.uint8)
    w2, w2s = torch.zeros(2, 256, 64, dtype=torch.uint8), torch.zeros(2, 256, 4, dtype=torch.uint8)
    ids, wts = torch.zeros(2, 1, dtype=torch.int64), torch.ones(2, 1)
    with pytest.raises(HipCallError):  # no CPU fallback
        fused_moe.fused_experts(x, w1, w2, wts, ids, use_mxfp4_w4a8=True, w1_scale=w1s, w2_scale=w2s)
    with pytest.raises(AssertionError):  # its own shape checks: K/2 columns expected
        fused_moe.fused_experts(x, w1[:, :, :100].contiguous(), w2, wts, ids, use_mxfp4_w4a8=True, w1_scale=w1s, w2_scale=w2s)


# ---------------------------------------------------------------- (d) ISA
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_gemm_kernels_use_the_scaled_mfma_with_an_fp4_operand_and_do_not_spill(tmp_path):
    csrc = os.path.join(ROOT, "chitu_amd", "csrc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-S", "--cuda-device-only", os.path.join(csrc, "moe_mxfp4.hip"), "-o", str(tmp_path / "k.s")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    text = open(tmp_path / "k.s").read()
    # function bodies: "<name>: ; @<name>" ... ".Lfunc_end"
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN5chitu\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M)}
    gemms = [n for n in bodies if "moe_mx_gemm" in n]
    assert {k for n in gemms for k in ("gemm_kernel", "gemm1_silu", "gemm2_q") if k in n} == {"gemm_kernel", "gemm1_silu", "gemm2_q"}
    for n in gemms:
        mfma = re.findall(r"v_mfma_scale_f32_16x16x128_f8f6f4[^\n]*", bodies[n])
        assert mfma, n
        assert all("cbsz:4" in m or "blgp:4" in m for m in mfma), (n, mfma[:2])  # one operand is e2m1
        assert "scratch_" not in bodies[n], n
    # kernel descriptors and metadata: no private segment, no spilled registers
    private = dict(re.findall(r"\.amdhsa_kernel (\w+)\n(?:[^\n]*\n)*?\s+\.amdhsa_private_segment_fixed_size (\d+)", text))
    spills = {}
    for chunk in text.split("\n  - "):
        name, sp = re.search(r"\.name:\s+(\w+)", chunk), re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", chunk)
        if name and sp:
            spills[name.group(1)] = [int(v) for v in sp]
    for n in gemms:
        assert private.get(n) == "0", (n, private.get(n))
        assert spills.get(n) == [0, 0], (n, spills.get(n))
