"""FP8 K / V cache of the GQA / MHA paged decode, the parts that need no GPU: the CPU statement of the row format (the reference of
tests/test_gpu_gqa_kv_fp8.py) and its properties, the five C entries (header, ABI version, exports, host-side argument checks),
cache_manager.gqa_kv_layout and the args field.  (The decode kernel stores its widened V chunks at the LDS addresses the bf16
kernel stores them at -- same lane, same row, same 16-byte chunk -- so there is no new LDS traffic to put under the bank model.)"""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("chitu_hip_gqa_kv_quant_fp8", "chitu_hip_gqa_kv_dequant_fp8", "chitu_hip_gqa_kv_append_fp8",
           "chitu_hip_gqa_qkv_post_kv_fp8", "chitu_hip_gqa_decode_kv_fp8")
ROW = 144


# ---------------------------------------------------------------- the format on the CPU
def quant_ref(x):
    """bf16 [T, Hkv, 128] -> uint8 [T, Hkv, 144]: 128 e4m3fn codes | one fp32 power-of-two scale | 12 zero bytes.
    Per head: e = the smallest integer with amax <= 448 * 2^e, clamped to >= -64 (amax == 0: -64); code = RNE_e4m3(x * 2^-e)."""
    assert x.dtype == torch.bfloat16 and x.dim() == 3 and x.shape[2] == 128
    T, H, _ = x.shape
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, ex = torch.frexp(amax / 448.0)  # amax / 448 = m * 2^ex, m in [0.5, 1): <= 2^ex, and <= 2^(ex - 1) only when m == 0.5
    e = ex - (m == 0.5).to(ex.dtype)
    e = torch.where(amax == 0, torch.full_like(e, -64), e).clamp(min=-64)
    scale = torch.ldexp(torch.ones_like(amax), e)
    codes = torch.ldexp(xf, -e.unsqueeze(-1)).to(torch.float8_e4m3fn)
    out = torch.zeros(T, H, ROW, dtype=torch.uint8)
    out[:, :, :128] = codes.view(torch.uint8)
    out[:, :, 128:132] = scale.contiguous().view(torch.uint8).view(T, H, 4)
    return out


def row_parts(rows):
    """uint8 [..., 144] -> (codes as fp32 [..., 128], scales fp32 [...], pad bytes [..., 12])"""
    codes = rows[..., :128].contiguous().view(torch.float8_e4m3fn).float()
    scale = rows[..., 128:132].contiguous().view(torch.float32).squeeze(-1)
    return codes, scale, rows[..., 132:]


def dequant_ref(rows):
    """uint8 [..., 144] -> bf16 [..., 128]: code * scale (exact)"""
    codes, scale, _ = row_parts(rows)
    return (codes * scale.unsqueeze(-1)).to(torch.bfloat16)


EDGE_PEAKS = (448.0, 450.0, 896.0, 0.0, 1e-30)


def edge_rows():
    """One token whose five heads peak at 448, 450, 896, 0 and 1e-30: scales 1, 2, 2, 2^-64, 2^-64."""
    g = torch.Generator().manual_seed(5)
    x = torch.zeros(1, len(EDGE_PEAKS), 128)
    for h, peak in enumerate(EDGE_PEAKS):
        v = (torch.rand(128, generator=g) * 2 - 1) * peak * 0.9
        v[(7 * h + 3) % 128] = -peak if h & 1 else peak
        x[0, h] = v
    return x.to(torch.bfloat16)


def sample_rows(T, H, seed=0):
    """T x H heads whose magnitudes span 1e-6 ... 1e4"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(T, H, 1, generator=g) * 10 - 6)
    return (torch.randn(T, H, 128, generator=g) * mag).to(torch.bfloat16)


def test_reference_quantiser_properties():
    x = torch.cat([sample_rows(1024, 5), edge_rows()])
    rows = quant_ref(x)
    assert int(((rows[..., :128] & 0x7F) == 0x7F).sum()) == 0  # no NaN code
    codes, scale, pad = row_parts(rows)
    assert float(codes.abs().max()) <= 448.0
    assert int(pad.sum()) == 0
    # scales: exact powers of two, never below 2^-64
    sbits = scale.contiguous().view(torch.int32)
    assert int((sbits & 0x7FFFFF).abs().sum()) == 0 and bool((scale >= 2.0 ** -64).all())
    # the scale is the SMALLEST admissible one: every head that is not clamped has its largest code in [224, 448]
    amax = x.float().abs().amax(-1)
    live = amax > 448.0 * 2.0 ** -64
    assert bool((codes.abs().amax(-1)[live] >= 224.0).all())
    # dequantisation is exact in bf16
    prod = codes * scale.unsqueeze(-1)
    assert torch.equal(prod.to(torch.bfloat16).float(), prod)
    # the format's error: 2^-4 of the head's peak (half an e4m3 step at the top binade is 16 / 448 of it); a head below the scale
    # floor (the 1e-30 edge) flushes towards zero instead: its error is its own magnitude
    err = (prod - x.float()).abs().amax(-1)
    assert bool((err[live] <= amax[live] * 2.0 ** -4).all()) and bool((err[~live] <= amax[~live]).all())
    # dequantise . quantise . dequantise is a fixed point (in values: a head whose peak rounds down to 224 * 2^e re-quantises with
    # the next smaller scale and doubled codes)
    d = dequant_ref(rows)
    assert torch.equal(dequant_ref(quant_ref(d)).view(torch.int16), d.view(torch.int16))
    # the edges
    e_scale = row_parts(quant_ref(edge_rows()))[1]
    assert e_scale[0].tolist() == [1.0, 2.0, 2.0, 2.0 ** -64, 2.0 ** -64]


def test_gqa_kv_layout():
    from chitu_amd.cache_manager import gqa_kv_layout

    assert gqa_kv_layout("bf16", 8) == ((8, 128), torch.bfloat16)
    assert gqa_kv_layout("fp8", 8) == ((8, ROW), torch.uint8)
    assert gqa_kv_layout("fp8", 2, head_dim=128) == ((2, ROW), torch.uint8)
    with pytest.raises(ValueError):
        gqa_kv_layout("int4", 8)


def test_args_carry_the_cache_format_and_default_to_bf16():
    from chitu_amd import ops
    from chitu_amd.llama import LlamaArgs
    from chitu_amd.mixtral import MixtralArgs

    assert ops.GQA_KV_FP8_ROW == ROW
    for A in (LlamaArgs, MixtralArgs):
        assert A().kv_cache_dtype == "bf16" and A(kv_cache_dtype="fp8").kv_cache_dtype == "fp8"


def test_decoder_refuses_a_cache_of_the_other_format():
    """on CPU tensors: the check runs before anything touches a device"""
    from chitu_amd.cache_manager import PagedKVCacheManager, gqa_kv_layout
    from chitu_amd.llama import LlamaArgs, LlamaDecoder

    for args_fmt in ("bf16", "fp8"):
        for cache_fmt in ("bf16", "fp8"):
            shape, dtype = gqa_kv_layout(cache_fmt, 2)
            cache = PagedKVCacheManager(0, 1, num_hot_req=1, block_size=16, max_seq_len=32, device="cpu", k_shape_per_sample=shape,
                                        v_shape_per_sample=shape, dtype=dtype)
            args = LlamaArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=64, ffn_dim=128, kv_cache_dtype=args_fmt)
            if args_fmt == cache_fmt:
                LlamaDecoder(args, cache, None, max_position_embeddings=32, device="cpu")
            else:
                with pytest.raises(ValueError, match="gqa_kv_layout"):
                    LlamaDecoder(args, cache, None, max_position_embeddings=32, device="cpu")
    with pytest.raises(ValueError):
        LlamaDecoder(LlamaArgs(dim=512, n_layers=1, n_heads=4, n_kv_heads=2, vocab_size=64, ffn_dim=128, kv_cache_dtype="fp4"), None, None,
                     max_position_embeddings=32, device="cpu")


# ---------------------------------------------------------------- header, ABI, exports
def _header():
    return open(os.path.join(ROOT, "include", "chitu_hip.h")).read()


def _params(text, name):
    body = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1)
    return [" ".join(p.split()) for p in body.split(",")]


def test_entries_are_in_the_header_with_their_notes_and_abi_version_7():
    text = _header()
    assert int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)) >= 7
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert re.search(name + r"\s+new: no reference counterpart", text), name
    assert _params(text, "chitu_hip_gqa_decode_kv_fp8") == _params(text, "chitu_hip_gqa_decode")
    assert len(_params(text, "chitu_hip_gqa_qkv_post_kv_fp8")) == len(_params(text, "chitu_hip_gqa_qkv_post"))


def test_docs_agree_with_the_header_on_entry_count_and_abi_version():
    text = _header()
    n = len(re.findall(r"^int chitu_hip_\w+\s*\(", text, flags=re.M))
    version = re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{n} entry points, ABI version {version}" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in integ.splitlines() if l.startswith("| 6 → 7 |")]
    assert len(row) == 1 and all(name in row[0] for name in ENTRIES)


def _cdll():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_the_entries():
    lib = _cdll()
    assert all(hasattr(lib, name) for name in ENTRIES)


def test_ops_refuse_cpu_tensors():
    from chitu_amd import ops
    from chitu_amd._lib import HipCallError

    x = torch.zeros(2, 2, 128, dtype=torch.bfloat16)
    cache = torch.zeros(2, 16, 2, ROW, dtype=torch.uint8)
    table, lens = torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(HipCallError):
        ops.gqa_kv_quant_fp8(x)
    with pytest.raises(HipCallError):
        ops.gqa_kv_dequant_fp8(torch.zeros(2, 2, ROW, dtype=torch.uint8))
    with pytest.raises(HipCallError):
        ops.append_gqa_kv_fp8(cache, cache.clone(), table, x, x, lens)
    with pytest.raises(HipCallError):
        ops.gqa_qkv_post_kv_fp8(torch.zeros(2, 8, 128, dtype=torch.bfloat16), 4, 2, torch.zeros(2, 64), torch.zeros(2, 64), cache,
                                cache.clone(), table, lens)


def test_entries_check_their_arguments_on_the_host():
    """Nothing is launched: the pointers are never dereferenced, so this needs no GPU."""
    lib = _cdll()
    buf = ctypes.create_string_buffer(128)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd, nul = ctypes.c_void_p(base), ctypes.c_void_p(base + 8), ctypes.c_void_p(0)
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    BAD_ARG, UNSUPPORTED = -1, -2

    # the bf16 entry has the same parameter list (asserted with the header) and shares the checks: the same cases for both
    for entry in (lib.chitu_hip_gqa_decode_kv_fp8, lib.chitu_hip_gqa_decode):

        def decode(q=p, kc=p, vc=p, page=16, splits=1, hd=128, hq=32, hkv=8, ws=p, out=p, batch=0, qsb=4096, qsh=128, table=p, lens=p):
            return entry(q, i64(qsb), i64(qsh), kc, vc, i64(4), i32(page), i32(hkv), table, i32(4), lens, f32(0.1), out, i32(batch),
                         i32(hq), i32(hd), i32(splits), ws, i64(0), None)

        assert decode() == 0 and decode(page=256, splits=256) == 0  # batch 0: accepted, nothing launched
        for arg in ("q", "kc", "vc"):
            assert decode(**{arg: nul}) == BAD_ARG and decode(**{arg: odd}) == BAD_ARG, arg
        for arg in ("out", "table", "lens"):
            assert decode(**{arg: nul}) == BAD_ARG, arg
        assert decode(hd=64) == UNSUPPORTED and decode(hd=256) == UNSUPPORTED
        assert decode(hq=17, hkv=1) == UNSUPPORTED and decode(hq=16, hkv=1) == 0  # group <= 16
        assert decode(page=8) == UNSUPPORTED and decode(page=24) == UNSUPPORTED
        assert decode(splits=0) == BAD_ARG and decode(splits=257) == BAD_ARG
        assert decode(batch=1, splits=2, ws=nul) == BAD_ARG  # split partials need the workspace (and 0 bytes are too few)
        assert decode(batch=1, splits=2) == BAD_ARG
        assert decode(qsb=4100) == BAD_ARG and decode(qsh=132) == BAD_ARG  # strides: multiples of 8 elements

    def quant(src=p, ss=256, dst=p, ds=2 * ROW + 16, rows=0, heads=2):
        return lib.chitu_hip_gqa_kv_quant_fp8(src, i64(ss), dst, i64(ds), i64(rows), i32(heads), None)

    assert quant() == 0
    assert quant(src=odd) == BAD_ARG and quant(dst=odd) == BAD_ARG and quant(src=nul) == BAD_ARG and quant(dst=nul) == BAD_ARG
    assert quant(ss=255) == BAD_ARG and quant(ss=260) == BAD_ARG and quant(ds=ROW) == BAD_ARG and quant(ds=2 * ROW + 8) == BAD_ARG
    assert quant(heads=0) == BAD_ARG and quant(rows=-1) == BAD_ARG

    def dequant(src=p, ss=2 * ROW, dst=p, heads=2):
        return lib.chitu_hip_gqa_kv_dequant_fp8(src, i64(ss), dst, i64(0), i32(heads), None)

    assert dequant() == 0 and dequant(src=odd) == BAD_ARG and dequant(ss=2 * ROW - 16) == BAD_ARG and dequant(dst=nul) == BAD_ARG
    assert dequant(dst=odd) == BAD_ARG

    def append(k=p, ks=256, v=p, vs=256, kc=p, vc=p, page=1, pps=1, batch=0, heads=2):
        return lib.chitu_hip_gqa_kv_append_fp8(k, i64(ks), v, i64(vs), kc, vc, i64(4), i32(page), i32(heads), p, i32(pps), p, i32(batch), None)

    assert append() == 0 and append(page=7) == 0  # any page size >= 1
    assert append(page=0) == BAD_ARG and append(pps=0) == BAD_ARG and append(kc=odd) == BAD_ARG and append(vc=odd) == BAD_ARG
    assert append(ks=100) == BAD_ARG and append(vs=260) == BAD_ARG and append(k=nul) == BAD_ARG and append(v=odd) == BAD_ARG

    def post(qkv=p, rs=12 * 128, hd=128, layout=0, kc=p, vc=p, page=16, batch=0):
        return lib.chitu_hip_gqa_qkv_post_kv_fp8(qkv, i64(rs), i32(8), i32(2), i32(hd), p, p, i32(layout), kc, vc, i64(4), i32(page), p,
                                                 i32(1), p, i32(batch), None)

    assert post() == 0 and post(layout=1) == 0
    assert post(layout=2) == BAD_ARG and post(qkv=nul) == BAD_ARG and post(kc=odd) == BAD_ARG and post(vc=nul) == BAD_ARG
    assert post(hd=64) == UNSUPPORTED and post(rs=11 * 128) == UNSUPPORTED and post(rs=12 * 128 + 4) == UNSUPPORTED
