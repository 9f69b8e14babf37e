"""Host tests (no GPU) of the prefill form of the MXFP4 experts (csrc/moe_mxfp4_tiled.hip): the dispatch rule that the fp8 and
the MXFP4 path share, the two C entries (header, ABI version, host-side argument checks), the LDS image of the weight tile under
the bank rules of gfx950, and the compiled kernel's K loop (no compiler wait where LDS-DMA requests are in flight)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------- dispatch
# (tokens, topk, E, I, Nout, aligned) -> tiled?   The rule: >= 128 tokens, >= 24 slots per expert on average, I % 128 == 0,
# Nout % 8 == 0, and no caller-supplied moe_align triple (that one comes from block 16).
DISPATCH = [
    ((127, 8, 32, 256, 7168, None), False),   # one token short
    ((128, 8, 32, 256, 7168, None), True),    # 1024 slots >= 24 * 32
    ((128, 8, 43, 256, 7168, None), False),   # numel = 1024, 24 * E = 1032: just below
    ((129, 8, 43, 256, 7168, None), True),    # numel = 1032 = 24 * E: at the bound
    ((128, 6, 32, 256, 7168, None), True),    # numel = 768 = 24 * 32
    ((128, 6, 33, 256, 7168, None), False),   # 768 < 792
    ((207, 5, 17, 256, 512, None), True),     # the tiny model's 200 + 7 token prefill (17 experts, top 4 + 1 shared)
    ((2048, 9, 257, 256, 7168, None), True),  # R1 at TP=8, a 2048-token prompt
    ((128, 9, 257, 256, 7168, None), False),  # ... a 128-token one: 4 slots per expert
    ((300, 2, 8, 192, 512, None), False),     # I no multiple of 128
    ((300, 2, 8, 640, 384, None), True),      # wide experts
    ((300, 2, 8, 128, 204, None), False),     # Nout % 8 != 0
    ((300, 2, 8, 128, 200, None), True),
    ((300, 2, 8, 128, 512, ("sorted", "experts", "npost")), False),  # caller-supplied triple: block 16, streaming
    ((0, 2, 8, 128, 512, None), False),
]


@pytest.mark.parametrize("case,want", DISPATCH)
def test_dispatch_predicate(case, want, monkeypatch):
    from chitu_amd import fused_moe

    monkeypatch.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 128)
    monkeypatch.setattr(fused_moe, "_MOE_TILED_MIN_PER_EXPERT", 24)
    tokens, topk, E, I, Nout, aligned = case
    assert fused_moe._takes_tiled(tokens, tokens * topk, E, I, Nout, aligned) is want


def test_dispatch_predicate_switch_and_default(monkeypatch):
    from chitu_amd import fused_moe

    if "CHITU_MOE_TILED_MIN_TOKENS" not in os.environ:
        assert fused_moe._MOE_TILED_MIN_TOKENS == 128 and fused_moe._MOE_TILED_MIN_PER_EXPERT == 24
    monkeypatch.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 0)  # CHITU_MOE_TILED_MIN_TOKENS=0: never
    assert fused_moe._takes_tiled(4096, 4096 * 8, 32, 256, 7168, None) is False
    monkeypatch.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 512)
    assert fused_moe._takes_tiled(511, 511 * 8, 32, 256, 7168, None) is False
    assert fused_moe._takes_tiled(512, 512 * 8, 32, 256, 7168, None) is True


def test_mxfp4_path_switches_over_at_its_own_token_count(monkeypatch):
    """Measured: at R1's shapes the tiled MXFP4 form first beats the streaming one at 512 tokens, so the MXFP4
    path passes its own threshold; everything else is the shared rule, and the fp8 switch at 0 switches both off."""
    from chitu_amd import fused_moe

    if "CHITU_MOE_MXFP4_TILED_MIN_TOKENS" not in os.environ:
        assert fused_moe._MOE_MXFP4_TILED_MIN_TOKENS == 512
    monkeypatch.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 128)
    monkeypatch.setattr(fused_moe, "_MOE_TILED_MIN_PER_EXPERT", 24)
    for tokens, want in ((127, False), (128, False), (511, False), (512, True), (2048, True)):
        assert fused_moe._takes_tiled(tokens, tokens * 8, 32, 256, 7168, None, min_tokens=512) is want, tokens
    assert fused_moe._takes_tiled(512, 512 * 9, 257, 256, 7168, None, min_tokens=512) is False   # 17.9 slots per expert
    assert fused_moe._takes_tiled(1024, 1024 * 9, 257, 256, 7168, None, min_tokens=512) is True
    assert fused_moe._takes_tiled(128, 128 * 8, 32, 256, 7168, None, min_tokens=128) is True
    assert fused_moe._takes_tiled(2048, 2048 * 8, 32, 256, 7168, None, min_tokens=0) is False
    assert fused_moe._takes_tiled(2048, 2048 * 8, 32, 256, 7168, ("s", "e", "n"), min_tokens=512) is False
    monkeypatch.setattr(fused_moe, "_MOE_TILED_MIN_TOKENS", 0)  # CHITU_MOE_TILED_MIN_TOKENS=0 keeps the streaming form
    assert fused_moe._takes_tiled(2048, 2048 * 8, 32, 256, 7168, None, min_tokens=512) is False


def test_both_paths_call_the_one_predicate():
    """The fp8 path and the MXFP4 path decide through _takes_tiled and nothing else."""
    import inspect

    from chitu_amd import fused_moe

    for fn, call in ((fused_moe.fused_experts_impl, "tiled = _takes_tiled(num_tokens, numel, global_num_experts, I, Nout, aligned)"),
                     (fused_moe._fused_experts_mxfp4, "tiled = _takes_tiled(num_tokens, numel, global_num_experts, I, Nout, aligned, "
                                                      "min_tokens=_MOE_MXFP4_TILED_MIN_TOKENS)")):
        src = inspect.getsource(fn)
        assert call in src, fn.__name__
        assert "_MOE_TILED_MIN_TOKENS" not in src and "_MOE_TILED_MIN_PER_EXPERT" not in src, fn.__name__


# ---------------------------------------------------------------- header and ABI
def test_new_entries_are_in_the_header_with_abi_version_5():
    text = open(os.path.join(ROOT, "include", "chitu_hip.h")).read()
    version = int(re.search(r"#define\s+CHITU_HIP_ABI_VERSION\s+(\d+)", text).group(1))
    assert version >= 5
    for name in ("chitu_hip_moe_gemm1_silu_mxfp4_tiled", "chitu_hip_moe_gemm2_mxfp4_tiled"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert re.search(name + r"\s+new: no reference counterpart; tiled form of", text), name
    # the argument lists are the fp8 tiled entries' with the weight and scale pointers exchanged
    def params(name):
        body = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1)
        return [" ".join(p.split()) for p in body.split(",")]

    for mx, f8 in (("chitu_hip_moe_gemm1_silu_mxfp4_tiled", "chitu_hip_moe_gemm1_silu_fp8_tiled"),
                   ("chitu_hip_moe_gemm2_mxfp4_tiled", "chitu_hip_moe_gemm2_fp8_tiled")):
        a, b = params(mx), params(f8)
        assert len(a) == len(b)
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        assert len(diff) == 2 and all(x.startswith("const void* w") for x, _ in diff), diff
        assert a[-2] == "int32_t block_m"


def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_new_entries_check_their_arguments_on_the_host():
    """Nothing is launched: the pointers are never dereferenced, so this needs no GPU."""
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    nul = ctypes.c_void_p(0)
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    BAD_ARG, UNSUPPORTED = -1, -2

    def g1(K, I, bm=128, numel=256, a=p, ws=p, mmb=4):
        return lib.chitu_hip_moe_gemm1_silu_mxfp4_tiled(a, p, p, ws, p, p, p, p, i64(numel), i32(2), i64(I), i64(K), i64(mmb), i32(bm), None)

    def g2(I, N=256, bm=128, numel=256, h=p, ws=p, mmb=4):
        return lib.chitu_hip_moe_gemm2_mxfp4_tiled(h, p, p, ws, p, p, p, p, i32(0), i32(1), p, i64(numel), i64(N), i64(I), i64(mmb),
                                                   i32(bm), None)

    for K in (127, 129, 64, 7168 + 32, 7168 + 64, 1):
        assert g1(K, 256) == UNSUPPORTED, K
    for I in (64, 192, 16, 257, 129):
        assert g1(256, I) == UNSUPPORTED, I
        assert g2(I) == UNSUPPORTED, I
    for bm in (16, 32, 0, 256, 96):
        assert g1(256, 128, bm=bm) == UNSUPPORTED and g2(128, bm=bm) == UNSUPPORTED, bm
    assert g2(128, N=204) == UNSUPPORTED  # N % 8
    # one expert's matrix beyond int32 byte offsets: 2I x K/2 and N x I/2 bytes
    assert g1(1 << 20, 2048) == UNSUPPORTED
    assert g2(1 << 16, N=1 << 16) == UNSUPPORTED
    # ... and the activation matrix
    assert g1(7168, 256, numel=(1 << 20) * 2) == UNSUPPORTED
    assert g1(256, 128, a=nul) == BAD_ARG and g1(256, 128, ws=nul) == BAD_ARG
    assert g2(128, h=nul) == BAD_ARG and g2(128, ws=nul) == BAD_ARG
    # zero work is accepted without a launch
    assert g1(256, 128, numel=0) == 0 and g1(256, 128, mmb=0) == 0
    assert g2(128, numel=0) == 0 and g2(128, mmb=0) == 0


# ---------------------------------------------------------------- the weight tile's LDS image
def test_weight_tile_image_is_conflict_free_and_the_dma_permutation_covers_it():
    """chitu_amd/csrc/moe_mxfp4_tiled.hip: [128 rows][64 B] unpadded, chunk c of row r at c ^ (-(r >> 2) & 3); lane (j, g) of a
    16-row MFMA tile reads chunk g of row j (mx_tile_frag_off) with ds_read_b128; a DMA piece n covers rows 16 n .. 16 n + 15, lane
    i -> row 16 n + (i >> 2), position i & 3, source chunk mx_tile_src_chunk(i).  Bank model: tests/test_lds_layouts_host.py."""
    from tests.test_lds_layouts_host import B128_GROUPS, ways

    for tile_row0 in range(0, 128, 16):
        for grp in B128_GROUPS:
            addrs = []
            for lane in grp:
                j, g = lane & 15, lane >> 4
                addrs.append(tile_row0 * 64 + j * 64 + ((g ^ ((-(j >> 2)) & 3)) << 4))
            assert ways(addrs, 16) == 1, tile_row0
    # the plain image is 2-way: what the permutation removes
    assert max(ways([(lane & 15) * 64 + (lane >> 4) * 16 for lane in grp], 16) for grp in B128_GROUPS) == 2
    for n in range(8):
        seen = set()
        for lane in range(64):
            r, pos = 16 * n + (lane >> 2), lane & 3
            src = (lane & 3) ^ ((-(lane >> 4)) & 3)
            assert src == pos ^ ((-(r >> 2)) & 3)  # the reader's formula and the source permutation agree
            seen.add((r, src))
        assert len(seen) == 64


# ---------------------------------------------------------------- the compiled K loop
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_no_compiler_wait_inside_the_dma_fed_loop(tmp_path):
    """tests/test_flash_asm_audit.py's audit on the new kernel: the loop fed by LDS-DMA holds no `s_waitcnt vmcnt` of the
    compiler's where a request is in flight (it would drain the tiles).  Every instantiation is read; each multiplies through
    the scaled fp4 MFMA."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_flash_asm

    csrc = os.path.join(ROOT, "chitu_amd", "csrc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-S", "--cuda-device-only", os.path.join(csrc, "moe_mxfp4_tiled.hip"), "-o", str(tmp_path / "k.s")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    seen, bad = check_flash_asm.audit_dma_loops(str(tmp_path / "k.s"), "moe_mx_gemm_tiled_kernel")
    assert len(seen) == 6 and not bad, (seen, bad)  # {GEMM1, GEMM2 x NREP 1 / 4} x TM {64, 128}
    assert "v_mfma_scale_f32_16x16x128_f8f6f4" in open(tmp_path / "k.s").read()
