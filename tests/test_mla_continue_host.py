"""Continued MLA prefill (DeepSeek-V3), the parts that need no GPU: the second extension header against the library's exports,
the host-side argument checks of its two entries, the position map of the flash kernel's kCont instantiation restated in Python
(every live row stored once, no dead row stored, the LAST-block invariant), the signatures of the new Python methods, and the
compiled gfx950 assembly of both instantiations."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import mla_continue_ref as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT2_HEADER = os.path.join(ROOT, "include", "chitu_hip_ext2.h")
ENTRIES = ("chitu_ext2_mla_kv_gather", "chitu_ext2_mla_prefill_flash_continue")
HIPCC = "/opt/rocm/bin/hipcc"


def _lib():
    from chitu_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


# ---------------------------------------------------------------- the header
def test_ext2_header_declares_exactly_the_exported_ext2_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(EXT2_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(chitu_ext2_\w+)\s*\(", src)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib().LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r"\bT\s+(chitu_ext2_\w+)", out)))
    assert declared == exported == sorted(ENTRIES)
    assert re.search(r"#define\s+CHITU_HIP_EXT2_VERSION\s+1\b", src) and '#include "chitu_hip.h"' in src
    assert not re.findall(r"\bint\s+(chitu_hip_\w+|chitu_ext_\w+)\s*\(", src)  # nothing of the two frozen prefixes is declared here


# ---------------------------------------------------------------- host argument checks
I32, I64, F32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float


def _gather_args(p, n_seq, **over):
    a = dict(cache=p, fp8=I32(0), num_pages=I64(4), page_size=I32(16), table=p, table_stride=I32(2), cu=p, n_seq=I32(n_seq),
             total_rows=I64(5), out=p, out_stride=I64(576), rank=I32(512), rope=I32(64), stream=None)
    a.update(over)
    return list(a.values())


def _flash_args(p, n_seq, **over):
    a = dict(q=p, q_st=I64(16 * 576), q_sh=I64(576), kv=p, kv_st=I64(576), cu_q=p, cu_k=p, n_seq=I32(n_seq), max_q=I32(5),
             scale=F32(0.1352), out=p, heads=I32(16), rank=I32(512), rope=I32(64), stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("n_seq", [0, 3])
def test_entries_check_their_arguments_on_the_host(n_seq):
    """Argument checks run before anything is launched and before the zero-size return: the pointers are host memory and are
    never dereferenced (with a launch these calls would return a HIP error or fault, not -1 / -2)."""
    lib = ctypes.CDLL(_lib().LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 8)
    gather, flash = lib.chitu_ext2_mla_kv_gather, lib.chitu_ext2_mla_prefill_flash_continue
    for name in ("cache", "table", "cu", "out"):
        assert gather(*_gather_args(p, n_seq, **{name: None})) == -1, name
    for name in ("cache", "out"):
        assert gather(*_gather_args(p, n_seq, **{name: odd})) == -1, name
    for bad in (dict(out_stride=I64(575)), dict(out_stride=I64(580)), dict(out_stride=I64(568)), dict(page_size=I32(0)),
                dict(table_stride=I32(0)), dict(fp8=I32(2)), dict(total_rows=I64(-1)), dict(num_pages=I64(-1))):
        assert gather(*_gather_args(p, n_seq, **bad)) == -1, bad
    for bad in (dict(rank=I32(256)), dict(rope=I32(32))):
        assert gather(*_gather_args(p, n_seq, **bad)) == -2, bad
    for name in ("q", "kv", "cu_q", "cu_k", "out"):
        assert flash(*_flash_args(p, n_seq, **{name: None})) == -1, name
    for name in ("q", "kv", "out"):
        assert flash(*_flash_args(p, n_seq, **{name: odd})) == -1, name
    for bad in (dict(q_st=I64(16 * 576 + 4)), dict(q_sh=I64(580)), dict(kv_st=I64(577)), dict(heads=I32(0)), dict(max_q=I32(-1))):
        assert flash(*_flash_args(p, n_seq, **bad)) == -1, bad
    for bad in (dict(rank=I32(256)), dict(rope=I32(128))):
        assert flash(*_flash_args(p, n_seq, **bad)) == -2, bad
    # nothing to do: 0 with nothing launched (valid arguments otherwise; with n_seq = 3 only the zero size stops the launch)
    assert gather(*_gather_args(p, n_seq, total_rows=I64(0))) == 0
    assert flash(*_flash_args(p, n_seq, max_q=I32(0))) == 0
    if n_seq == 0:
        assert gather(*_gather_args(p, 0)) == 0 and flash(*_flash_args(p, 0)) == 0


# ---------------------------------------------------------------- the position map
PS, NS = range(0, 41), range(1, 21)


def test_position_map_stores_every_live_row_once_and_no_dead_row():
    bq = mc.kbq()
    assert bq == 8 and mc.KEY_BLOCK % bq == 0
    cu_q0 = 1000  # rows of other sequences lie on both sides
    for P in PS:
        for n in NS:
            L = P + n
            wgs = mc.position_map(cu_q0, n, L, mc.grid_x(n, bq), bq)
            stored = [row for wg in wgs for (_, _, _, row) in wg["stores"]]
            assert sorted(stored) == list(range(cu_q0, cu_q0 + n)), (P, n, stored)  # once each, none outside: no dead row
            assert max(a for wg in wgs for (_, _, a, _) in wg["stores"]) == L - 1  # the grid reaches the last row
            for wg in wgs:
                assert all(P <= a < L and row == cu_q0 + a - P for (_, _, a, row) in wg["stores"])
                assert all(cu_q0 <= r < cu_q0 + n for r in wg["q_rows"]), (P, n, wg)  # dead rows load a live row's Q
                seen = sorted((w, t) for (w, t, _, _) in wg["stores"])
                assert len(set(seen)) == len(seen) and all(w == t // mc.ROWS_PER_WAVE for w, t in seen)
            # one workgroup column fewer would not do for some (P, n): the + 1 of the host's grid is needed, and only there
            short = [row for wg in mc.position_map(cu_q0, n, L, mc.grid_x(n, bq) - 1, bq) for (_, _, _, row) in wg["stores"]]
            assert (len(short) < n) == (-(-(P % bq + n) // bq) > -(-n // bq)), (P, n)


def test_position_map_keeps_a_workgroups_live_queries_inside_one_key_block():
    """The invariant the kernel's mask rests on: key blocks 0 .. nb - 2 of a workgroup are unmasked, so every one of their keys
    must be permitted for every live query of the workgroup: 32 (nb - 1) - 1 <= the first live position.  It holds because the
    eight positions of a workgroup start at a multiple of 8 and so share a 32-key block."""
    bq = mc.kbq()
    broken = 0
    for P in PS:
        for n in NS:
            L = P + n
            for wg in mc.position_map(0, n, L, mc.grid_x(n, bq), bq):
                first, last = wg["p0"] + wg["t_lo"], wg["p0"] + wg["nq"] - 1
                assert first // mc.KEY_BLOCK == last // mc.KEY_BLOCK == wg["nb"] - 1, (P, n, wg)
                assert mc.KEY_BLOCK * (wg["nb"] - 1) - 1 <= first
            # the rejected layout (blocks start at the first new token) breaks it for some prefixes -- what the alignment is for
            for wg in mc.position_map(0, n, L, mc.grid_x(n, bq), bq, aligned=False):
                broken += mc.KEY_BLOCK * (wg["nb"] - 1) - 1 > wg["p0"] + wg["t_lo"]
    assert broken > 0


def test_position_map_with_more_queries_than_keys_stays_inside_the_sequence():
    """L < n is outside the contract; the map must still touch this sequence's rows only: the last L query rows are stored, the
    first n - L are neither stored nor loaded from below the sequence."""
    bq = mc.kbq()
    for L in range(0, 12):
        for n in range(L + 1, L + 12):
            wgs = mc.position_map(50, n, L, mc.grid_x(n, bq), bq)
            stored = sorted(row for wg in wgs for (_, _, _, row) in wg["stores"])
            assert stored == list(range(50 + n - L, 50 + n)), (L, n, stored)
            assert all(50 + n - L <= r < 50 + n for wg in wgs for r in wg["q_rows"])


def test_fp64_reference_with_an_offset_is_the_tail_of_the_whole_sequence_reference():
    from tests import attn_exact as ax

    g = torch.Generator().manual_seed(0)
    seqs, ns = [13, 40, 7], [5, 40, 1]
    cu = ax.cu_of(seqs)
    q = torch.randn(cu[-1], 3, 576, generator=g)
    kv = torch.randn(cu[-1], 576, generator=g)
    whole = ax.prefill64(q, kv.unsqueeze(1), kv[:, :512].unsqueeze(1), cu, ax.MLA_SCALE)
    qt, cu_q, idx = mc.tails(q, cu, ns)
    got = mc.prefill64_offset(qt, kv, cu_q, cu, ax.MLA_SCALE)
    assert float((got - whole[idx]).abs().max()) < 1e-12


# ---------------------------------------------------------------- the Python surface
def test_signatures_of_the_new_python_methods():
    from chitu_amd import ops
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.deepseek_v3 import AttentionDeepSeekV3, DeepSeekV3Decoder

    def names(f):
        return list(inspect.signature(f).parameters)

    assert names(ops.mla_kv_gather) == ["kv_cache", "block_table", "cu_seqlens_k", "total_rows", "out"]
    assert inspect.signature(ops.mla_kv_gather).parameters["out"].default is None
    assert names(HipAttnBackend.mla_attn_varlen_with_kvcache) == [
        "self", "q", "kv_cache", "cu_seqlens_q", "cache_seqlens", "block_table", "max_seqlen_q", "total_keys", "softmax_scale", "gathered"]
    assert inspect.signature(HipAttnBackend.mla_attn_varlen_with_kvcache).parameters["gathered"].default is None
    assert names(AttentionDeepSeekV3.prefill_forward_paged) == names(AttentionDeepSeekV3.prefill_forward)
    assert names(DeepSeekV3Decoder.prefill_continue) == ["self", "tokens", "req_ids"]
    assert names(DeepSeekV3Decoder.prefill) == ["self", "tokens", "req_ids", "chunk_size"]
    assert inspect.signature(DeepSeekV3Decoder.prefill).parameters["chunk_size"].default is None
    gen = inspect.signature(DeepSeekV3Decoder.generate).parameters
    assert "prefill_chunk_size" in gen and gen["prefill_chunk_size"].default is None


# ---------------------------------------------------------------- the assembly
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_both_instantiations_of_the_flash_kernel_keep_the_accumulator_in_the_agpr_file(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_flash_asm

    csrc = os.path.join(ROOT, "chitu_amd", "csrc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-S", "--cuda-device-only", os.path.join(csrc, "mla_prefill_flash.hip"), "-o", str(tmp_path / "k.s")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    seen, bad = check_flash_asm.audit_literal(str(tmp_path / "k.s"), "mla_prefill_flash_pipe_kernel")
    assert len(seen) == 2 and not bad, (seen, bad)
    assert sorted("ILb0E" in k for k in seen) == [False, True] and sum("ILb1E" in k for k in seen) == 1  # kCont = false and true
    text = (tmp_path / "k.s").read_text()
    found = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if "mla_prefill_flash_pipe_kernel" in name:
            found[name] = (int(re.match(r"\s*(\d+)", blk).group(1)), int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1)),
                           int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1)))
    assert len(found) == 2 and all(v == (256, 0, 0) for v in found.values()), found
