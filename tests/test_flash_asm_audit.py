"""Host test (no GPU): the flash prefill kernel's gfx950 assembly keeps its accumulator in the AGPR file without spills.
The kernel pins 256 accumulator registers through asm operands and leaves hipcc a 256-VGPR allocation problem; a compiler
upgrade or an edit that tips it into spilling would still produce right answers, 3x slower -- this catches it at build time."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("src,kernel,literal", [("mla_prefill_flash.hip", "mla_prefill_flash_pipe_kernel", True)])
def test_flash_kernel_assembly_has_no_spills_and_no_accumulator_traffic(tmp_path, src, kernel, literal):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_flash_asm

    csrc = os.path.join(ROOT, "chitu_amd", "csrc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", str(tmp_path / "k.s")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    seen, bad = (check_flash_asm.audit_literal if literal else check_flash_asm.audit)(str(tmp_path / "k.s"), kernel)
    assert seen and not bad, bad


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("src,kernel", [("fp8_gemm_tiled.hip", "fp8_gemm_tiled_kernel"), ("bf16_gemm_tiled.hip", "bf16_gemm_tiled_kernel"),
                                        ("moe_tiled.hip", "moe_gemm_tiled_kernel"), ("gqa_prefill_flash.hip", "gqa_prefill_flash_kernel")])
def test_no_compiler_wait_inside_the_dma_fed_loops(tmp_path, src, kernel):
    """The loops fed by LDS-DMA hold no `s_waitcnt vmcnt` of the compiler's: it cannot see the DMA requests, its counter is
    in-order, so any such wait also drains the tiles in flight (check_flash_asm.audit_dma_loops).  (mla_decode.hip is not in
    the list: its tile loop keeps one compiler wait -- for the page-table fallback of splits above 32k tokens -- at the request
    point, right behind the kernel's own vmcnt(0) + barrier, where nothing is in flight; the compiler lays that loop out rotated
    and twice, which the audit's linear reading of the body cannot follow.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_flash_asm

    csrc = os.path.join(ROOT, "chitu_amd", "csrc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", str(tmp_path / "k.s")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    seen, bad = check_flash_asm.audit_dma_loops(str(tmp_path / "k.s"), kernel)
    assert seen and not bad, bad


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_asm_loads_of_mla_decode_are_untouched_until_their_wait(tmp_path):
    """mla_decode.hip requests seqlens and four page-table entries through inline-asm loads and waits for them in a LATER asm
    statement (so that they head the kernel); the compiler treats their outputs as defined at once.  Nothing may touch those
    registers in between (check_flash_asm.audit_async_asm_loads reads the compiled ISA of the three instantiations: one token,
    one token with the fused tail, two tokens)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_flash_asm

    csrc = os.path.join(ROOT, "chitu_amd", "csrc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-S", "--cuda-device-only", os.path.join(csrc, "mla_decode.hip"), "-o", str(tmp_path / "k.s")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    seen, bad = check_flash_asm.audit_async_asm_loads(str(tmp_path / "k.s"), "mla_decode_kernel")
    assert len(seen) == 3 and not bad, bad


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_mla_decode_kernels_fit_the_register_file_without_scratch(tmp_path):
    """The five MLA paged decode instantiations (mla_decode.hip: one token, one token with the fused tail, two tokens;
    mla_decode_kv_fp8.hip: one and two tokens) hold two tokens' Q fragments, accumulators and state in registers.  Their launch
    bound (256, 1) is one wave per SIMD, so up to the 512 unified registers the occupancy cannot change; above that, or with
    scratch or spills, the kernel is a different kernel.  Read from the code-object metadata of the compiled ISA."""
    import re

    csrc = os.path.join(ROOT, "chitu_amd", "csrc")
    found = {}
    for src in ("mla_decode.hip", "mla_decode_kv_fp8.hip"):
        out = tmp_path / (src + ".s")
        cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
               "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", str(out)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        for blk in re.split(r"\n  - \.agpr_count:", out.read_text())[1:]:
            name = re.search(r"\.name:\s*(\S+)", blk).group(1)
            if re.search(r"mla_decode(_kv_fp8)?_kernel", name):
                found[name] = {k: int(re.search(r"\." + k + r":\s*(\d+)", blk).group(1))
                               for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count")}
    assert len(found) == 5, sorted(found)
    for name, r in found.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["vgpr_count"] <= 512, (name, r)
