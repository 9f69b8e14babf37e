"""FP8 latent KV cache of the MLA paged decode, the parts that need no GPU: the CPU statement of the row format (the reference
of tests/test_gpu_mla_kv_fp8.py) and its properties, the four C entries (header, ABI version, exports, host-side argument
checks), cache_manager.mla_kv_layout, and the LDS traffic of the decode kernel's widening pass under the bank model of
tests/test_lds_layouts_host.py."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_lds_layouts_host import B128_GROUPS, ways

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("chitu_hip_mla_kv_quant_fp8", "chitu_hip_mla_kv_dequant_fp8", "chitu_hip_mla_kv_append_fp8", "chitu_hip_mla_decode_kv_fp8")
ROW = 656


# ---------------------------------------------------------------- the format on the CPU
def quant_ref(x):
    """bf16 [T, 576] -> uint8 [T, 656]: 512 e4m3fn codes | four fp32 power-of-two scales | the 64 rope values' bf16 bytes.
    Per 128-channel group: e = the smallest integer with amax <= 448 * 2^e, clamped to >= -64 (amax == 0: -64);
    code = RNE_e4m3(x * 2^-e)."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] == 576
    T = x.shape[0]
    lat = x[:, :512].float().view(T, 4, 128)
    amax = lat.abs().amax(-1)
    m, ex = torch.frexp(amax / 448.0)  # amax / 448 = m * 2^ex, m in [0.5, 1): <= 2^ex, and <= 2^(ex - 1) only when m == 0.5
    e = ex - (m == 0.5).to(ex.dtype)
    e = torch.where(amax == 0, torch.full_like(e, -64), e).clamp(min=-64)
    scale = torch.ldexp(torch.ones_like(amax), e)
    codes = torch.ldexp(lat, -e.unsqueeze(-1)).to(torch.float8_e4m3fn)
    out = torch.empty(T, ROW, dtype=torch.uint8)
    out[:, :512] = codes.view(torch.uint8).view(T, 512)
    out[:, 512:528] = scale.contiguous().view(torch.uint8).view(T, 16)
    out[:, 528:] = x[:, 512:].contiguous().view(torch.uint8).view(T, 128)
    return out


def row_parts(rows):
    """uint8 [T, 656] -> (codes as fp32 [T, 4, 128], scales fp32 [T, 4], rope bf16 [T, 64])"""
    T = rows.shape[0]
    codes = rows[:, :512].contiguous().view(torch.float8_e4m3fn).float().view(T, 4, 128)
    scale = rows[:, 512:528].contiguous().view(torch.float32).view(T, 4)
    rope = rows[:, 528:].contiguous().view(torch.bfloat16).view(T, 64)
    return codes, scale, rope


def dequant_ref(rows):
    """uint8 [T, 656] -> bf16 [T, 576]: code * scale (exact), the rope part as stored."""
    codes, scale, rope = row_parts(rows)
    lat = (codes * scale.unsqueeze(-1)).view(rows.shape[0], 512)
    return torch.cat([lat.to(torch.bfloat16), rope], dim=-1)


def edge_rows():
    """Two rows whose groups peak at 448, 450, 896, 0 and at 1e-30 (+ three ordinary groups): scales 1, 2, 2, 2^-64, 2^-64."""
    g = torch.Generator().manual_seed(5)
    x = torch.zeros(2, 576)
    for grp, peak in enumerate((448.0, 450.0, 896.0, 0.0)):
        v = (torch.rand(128, generator=g) * 2 - 1) * peak * 0.9
        v[(7 * grp + 3) % 128] = -peak if grp & 1 else peak
        x[0, grp * 128 : (grp + 1) * 128] = v
    x[1, :512] = torch.randn(512, generator=g)
    x[1, :128] = (torch.rand(128, generator=g) * 2 - 1) * 0.9e-30
    x[1, 5] = 1e-30
    x[:, 512:] = torch.randn(2, 64, generator=g)
    return x.to(torch.bfloat16)


def sample_rows(T, seed=0):
    """T rows whose magnitudes span 1e-6 ... 1e4 (per group), rope part N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(T, 4, 1, generator=g) * 10 - 6)
    lat = (torch.randn(T, 4, 128, generator=g) * mag).view(T, 512)
    return torch.cat([lat, torch.randn(T, 64, generator=g)], dim=-1).to(torch.bfloat16)


def test_reference_quantiser_properties():
    x = torch.cat([sample_rows(4096), edge_rows()])
    rows = quant_ref(x)
    T = x.shape[0]
    raw = rows[:, :512]
    assert int(((raw & 0x7F) == 0x7F).sum()) == 0  # no NaN code
    codes, scale, rope = row_parts(rows)
    assert float(codes.abs().max()) <= 448.0
    # scales: exact powers of two, never below 2^-64
    sbits = scale.contiguous().view(torch.int32)
    assert int((sbits & 0x7FFFFF).abs().sum()) == 0 and bool((scale >= 2.0 ** -64).all())
    # the scale is the SMALLEST admissible one: every group that is not clamped has its largest code in [224, 448]
    amax = x[:, :512].float().view(T, 4, 128).abs().amax(-1)
    live = amax > 448.0 * 2.0 ** -64
    assert bool((codes.abs().amax(-1)[live] >= 224.0).all())
    # dequantisation is exact in bf16
    prod = codes * scale.unsqueeze(-1)
    assert torch.equal(prod.to(torch.bfloat16).float(), prod)
    # the format's error: 2^-4 of the group's peak (half an e4m3 step at the top binade is 16 / 448 of it); a group below
    # the scale floor (peak < 448 * 2^-64, the 1e-30 edge) flushes towards zero instead: its error is its own magnitude
    err = (prod - x[:, :512].float().view(T, 4, 128)).abs().amax(-1)
    assert bool((err[live] <= amax[live] * 2.0 ** -4).all()) and bool((err[~live] <= amax[~live]).all())
    # the rope part is a copy
    assert torch.equal(rope.view(torch.int16), x[:, 512:].contiguous().view(torch.int16))
    # the edges
    e_scale = row_parts(quant_ref(edge_rows()))[1]
    assert e_scale[0].tolist() == [1.0, 2.0, 2.0, 2.0 ** -64] and float(e_scale[1, 0]) == 2.0 ** -64
    assert torch.equal(dequant_ref(rows)[:, 512:].view(torch.int16), x[:, 512:].contiguous().view(torch.int16))


def test_mla_kv_layout():
    from chitu_amd.cache_manager import mla_kv_layout

    assert mla_kv_layout("bf16") == ((576,), torch.bfloat16)
    assert mla_kv_layout("fp8") == ((656,), torch.uint8)
    assert mla_kv_layout("fp8", kv_lora_rank=512, rope=64) == ((ROW,), torch.uint8)
    with pytest.raises(ValueError):
        mla_kv_layout("int4")


def test_args_carry_the_cache_format_and_default_to_bf16():
    from chitu_amd.deepseek_v3 import DeepSeekV3Args

    assert DeepSeekV3Args().kv_cache_dtype == "bf16" and DeepSeekV3Args(kv_cache_dtype="fp8").kv_cache_dtype == "fp8"


# ---------------------------------------------------------------- header, ABI, exports
def _header():
    return open(os.path.join(ROOT, "include", "chitu_hip.h")).read()


def test_entries_are_in_the_header_with_their_notes_and_abi_version_6():
    text = _header()
    assert int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1)) >= 6
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert re.search(name + r"\s+new: no reference counterpart", text), name

    def params(name):
        body = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1)
        return [" ".join(p.split()) for p in body.split(",")]

    assert params("chitu_hip_mla_decode_kv_fp8") == params("chitu_hip_mla_decode")


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

    x = torch.zeros(2, 576, dtype=torch.bfloat16)
    with pytest.raises(HipCallError):
        ops.mla_kv_quant_fp8(x)
    with pytest.raises(HipCallError):
        ops.mla_kv_dequant_fp8(torch.zeros(2, ROW, dtype=torch.uint8))
    with pytest.raises(HipCallError):
        ops.append_mla_kv_fp8(torch.zeros(2, 4, ROW, dtype=torch.uint8), torch.zeros(2, 1, dtype=torch.int32), x,
                              torch.zeros(2, dtype=torch.int32))


def test_entries_check_their_arguments_on_the_host():
    """Nothing is launched: the pointers are never dereferenced, so this needs no GPU."""
    lib = _cdll()
    buf = ctypes.create_string_buffer(128)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd, nul = ctypes.c_void_p(base), ctypes.c_void_p(base + 8), ctypes.c_void_p(0)
    i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    BAD_ARG, UNSUPPORTED = -1, -2

    # the bf16 entry has the same parameter list (asserted with the header) and shares the checks: the same cases for both
    for entry in (lib.chitu_hip_mla_decode_kv_fp8, lib.chitu_hip_mla_decode):

        def decode(cache=p, page=64, splits=1, q=p, C=512, R=64, ws=p, out=p, batch=0):
            return entry(q, i64(576), i64(576), q, i64(64), i64(64), cache, i64(4), i32(page), p, i32(4), p,
                         f32(0.1), out, i32(batch), i32(16), i32(C), i32(R), i32(splits), ws, i64(0), None)

        assert decode() == 0  # batch 0: accepted, nothing launched
        for page in (32, 1, 96, 0):
            assert decode(page=page) == UNSUPPORTED, page
        assert decode(cache=odd) == BAD_ARG and decode(q=odd) == BAD_ARG and decode(cache=nul) == BAD_ARG
        assert decode(C=256) == UNSUPPORTED and decode(R=32) == UNSUPPORTED
        assert decode(splits=0) == BAD_ARG and decode(splits=257) == BAD_ARG
        assert decode(out=nul) == BAD_ARG  # no output and a single split: nothing to leave behind
        assert decode(batch=1, splits=2, ws=nul) == BAD_ARG  # split partials need the workspace

    def quant(src=p, ss=576, dst=p, ds=ROW + 16, rows=0):
        return lib.chitu_hip_mla_kv_quant_fp8(src, i64(ss), dst, i64(ds), i64(rows), None)

    assert quant() == 0
    assert quant(src=odd) == BAD_ARG and quant(dst=odd) == BAD_ARG and quant(src=nul) == BAD_ARG
    assert quant(ss=575) == BAD_ARG and quant(ss=580) == BAD_ARG and quant(ds=640) == BAD_ARG and quant(ds=ROW + 8) == BAD_ARG

    def dequant(src=p, ss=ROW, dst=p):
        return lib.chitu_hip_mla_kv_dequant_fp8(src, i64(ss), dst, i64(0), None)

    assert dequant() == 0 and dequant(src=odd) == BAD_ARG and dequant(ss=655) == BAD_ARG and dequant(dst=nul) == BAD_ARG

    def append(src=p, ss=576, cache=p, page=1, pps=1, batch=0):
        return lib.chitu_hip_mla_kv_append_fp8(src, i64(ss), cache, i64(4), i32(page), p, i32(pps), p, i32(batch), None)

    assert append() == 0 and append(page=7) == 0  # any page size >= 1
    assert append(page=0) == BAD_ARG and append(pps=0) == BAD_ARG and append(cache=odd) == BAD_ARG and append(ss=100) == BAD_ARG


# ---------------------------------------------------------------- the decode kernel's LDS traffic
def test_widening_pass_covers_the_tile_image_and_its_stores_do_not_conflict():
    """chitu_amd/csrc/mla_decode_kv_fp8.hip.  Staging buffer: [64 rows][41 chunks of 16 B], unswizzled; DMA piece n (41 of them),
    lane i -> staging chunk 64 n + i = (row q / 41, chunk q % 41).  Widening, codes: thread t, step i < 8: c = t + 256 i, row
    c >> 5, code chunk p = c & 31, one ds_read_b128, image chunks 2 p and 2 p + 1 stored at (chunk ^ swz(row)) of the
    [64][1152 B] image by two ds_write_b128, the lanes with bit 4 set storing the odd one first.  Rope: step i < 2: c = t + 256 i,
    row c >> 3, chunk p = c & 7 at byte 528 + 16 p of the staging row -> image chunk 64 + p.  The scales are read in place."""
    row_img = 1152

    def swz(r):
        return ((r >> 3) & 1) * 5 + ((r >> 1) & 1) * 2

    # the DMA covers the staging buffer exactly once
    assert sorted(64 * n + lane for n in range(41) for lane in range(64)) == list(range(64 * 41))
    written, read = set(), set()
    for step in range(8):
        for wave in range(4):
            first, second, rd = {}, {}, {}
            for lane in range(64):
                c = step * 256 + wave * 64 + lane
                r, p = c >> 5, c & 31
                odd_first = (lane >> 4) & 1
                rd[lane] = r * ROW + p * 16
                a, b = 2 * p + odd_first, 2 * p + 1 - odd_first
                first[lane], second[lane] = r * row_img + ((a ^ swz(r)) << 4), r * row_img + ((b ^ swz(r)) << 4)
                for chunk in (a, b):
                    assert (r, chunk ^ swz(r)) not in written
                    written.add((r, chunk ^ swz(r)))
                assert (r, p) not in read
                read.add((r, p))
            for grp in B128_GROUPS:  # the bulk of the pass: conflict-free on both sides
                assert ways([rd[lane] for lane in grp], 16) == 1, (step, wave)
                assert ways([first[lane] for lane in grp], 16) == 1 and ways([second[lane] for lane in grp], 16) == 1, (step, wave)
                # ... which the odd-first rule buys: all lanes storing their even chunk first is 2-way
                assert ways([second[lane] if (lane >> 4) & 1 else first[lane] for lane in grp], 16) == 2
    assert read == {(r, p) for r in range(64) for p in range(32)}
    for step in range(2):
        for wave in range(4):
            rd, wr = {}, {}
            for lane in range(64):
                c = step * 256 + wave * 64 + lane
                r, p = c >> 3, c & 7
                rd[lane] = r * ROW + 528 + p * 16
                wr[lane] = r * row_img + (((64 + p) ^ swz(r)) << 4)
                assert (r, (64 + p) ^ swz(r)) not in written
                written.add((r, (64 + p) ^ swz(r)))
            for grp in B128_GROUPS:  # 2 of the pass's 10 reads are 2-way (a group spans two staging rows); the stores are clean
                assert ways([rd[lane] for lane in grp], 16) == 2 and ways([wr[lane] for lane in grp], 16) == 1, (step, wave)
    # every chunk of the image is written exactly once per tile: 64 rows x 72 chunks
    assert written == {(r, c) for r in range(64) for c in range(72)}
    # LDS budget: image + two staging buffers + P + the softmax exchange + page ids, below the CU's 160 KB
    assert 64 * row_img + 2 * 64 * ROW + 16 * 72 * 2 + 2 * 64 * 4 + 512 * 4 == 162560 <= 160 * 1024
