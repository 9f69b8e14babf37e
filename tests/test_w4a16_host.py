"""W4A16 g128 on the host: the layout round trip, the quantiser against its formula, the GPTQ repacker, the decoder's parameters
and the header (include/chitu_hip_ext9.h); the launch-plan mirror over the GPU test's grid and csrc/gemm_plan.h, the entries'
argument checks, the references of tests/w4a16_ref.py against themselves, and the loader's per-rank quantisation."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import w4a16_ref as w4

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


# ---------------------------------------------------------------- the launch plan
HOST_CXX = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("c++")
PRODUCTION = (((1, 14336, 4096), True, (1, 4, 2)), ((1, 4096, 14336), False, (1, 8, 4)), ((1, 6144, 4096), False, (1, 8, 4)))  # Llama-3-8B
WK_DRIVER = r"""
#include <cstdio>
#include "gemm_plan.h"
int main() {
    long tiles, steps;
    while (scanf("%ld %ld", &tiles, &steps) == 2) printf("%d\n", chitu::stream_wk(tiles, steps));
}
"""


def test_plan_mirror_covers_every_instantiation_over_the_gpu_grid():
    from chitu_amd import ops

    lin, forms = w4.instantiations(ops.w4a16_plan, w4.GRID + w4.RING, silu=False)
    assert lin == w4.ALL_LINEAR and forms == {"stream"} and len(lin) == 8
    sil, forms = w4.instantiations(ops.w4a16_plan, w4.GRID + w4.RING, silu=True)
    assert sil == w4.ALL_SILU and forms == {"stream"} and len(sil) == 8
    assert {c for c in w4.F16_SHAPES} <= set(w4.GRID)
    for silu in (False, True):  # the ring cases wrap the deepest ring on every wave
        for M, N, K in w4.RING:
            mt, wk, depth = ops.w4a16_plan(M, N, K, silu=silu)["launches"][0]
            assert wk == 8 and -(-K // 256) // wk > depth
    M, N, K = w4.TILED
    assert ops.w4a16_plan(M, N, K)["form"] == "tiled" and ops.w4a16_plan(M, N // 2, K, silu=True)["form"] == "tiled"
    # the K split over steps of 256 channels: one wave per step up to 8, never an idle wave; the half-line tail is a step
    assert [ops.w4a16_plan(1, 16, k)["launches"][0][1] for k in w4.KS] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert [-(-k // 256) for k in w4.KS] == [1, 1, 2, 3, 4, 5, 8, 9]
    assert [m for m, _, _ in ops.w4a16_plan(33, 16, 1024)["launches"]] == [2, 1] and [m for m, _, _ in ops.w4a16_plan(17, 16, 1024)["launches"]] == [2]
    for (M, N, K), silu, launch in PRODUCTION:
        assert ops.w4a16_plan(M, N, K, silu=silu)["launches"] == [launch], (M, N, K)
    for M in (1, 127, 128, 191, 192, 255, 256, 300):
        for n in (16, 1023, 1024, 4096, 6143, 6144, 28672):
            for K in (64, 4096, 1 << 23):
                assert ops.w4a16_tiled(M, n, K) == ops.w8a16_tiled(M, n, K), (M, n, K)
    assert ops.w4a16_tiled(128, 6144, 4096) and not ops.w4a16_tiled(127, 28672, 4096) and ops.w4a16_tiled(256, 16, 128)
    assert ops.w4a16_plan(0, 16, 128) == {"form": "none", "launches": []}


@pytest.mark.skipif(not HOST_CXX or not os.path.exists(HOST_CXX), reason="needs a host C++ compiler")
def test_gemm_plan_header_gives_the_mirrors_wave_count(tmp_path):
    """csrc/gemm_plan.h::stream_wk(tiles, ceil(K / 256)), what the entries call, against ops.w4a16_plan"""
    from chitu_amd import ops

    (tmp_path / "driver.cpp").write_text(WK_DRIVER)
    res = subprocess.run([HOST_CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "chitu_amd", "csrc"),
                          str(tmp_path / "driver.cpp"), "-o", str(tmp_path / "driver")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    shapes = [(M, N, K, silu) for (M, N, K) in w4.GRID + w4.RING for silu in (False, True)] + [(*c, s) for c, s, _ in PRODUCTION]
    text = "".join(f"{(N + 15) // 16} {(K + 255) // 256}\n" for _, N, K, _ in shapes)
    res = subprocess.run([str(tmp_path / "driver")], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in res.stdout.split()]
    assert len(got) == len(shapes)
    for (M, N, K, silu), wk in zip(shapes, got):
        assert {w for _, w, _ in ops.w4a16_plan(M, N, K, silu=silu)["launches"]} == {wk}, (M, N, K, silu, wk)


# ---------------------------------------------------------------- host argument checks
I32, I64 = ctypes.c_int32, ctypes.c_int64


def _gemm_args(p, rows, **over):
    a = dict(x=p, w=p, scale=p, out=p, out_dtype=I32(0), M=I64(rows), N=I64(24), K=I64(384), stream=None)
    a.update(over)
    return list(a.values())


def _silu_args(p, rows, **over):
    a = dict(x=p, w=p, scale=p, out=p, M=I64(rows), inter=I64(24), K=I64(384), stream=None)
    a.update(over)
    return list(a.values())


def _widen_args(p, rows, **over):
    a = dict(w=p, scale=p, out=p, N=I64(rows), K=I64(384), stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("rows", [0, 3])
def test_entries_check_their_arguments_on_the_host(rows):
    """Argument checks run before anything is launched and before the zero-size return: the pointers are host memory and are
    never dereferenced (with a launch these calls would return a HIP error or fault, not -1 / -2)."""
    from chitu_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 8)
    gemm, silu, widen = lib.chitu_ext9_w4a16_gemm, lib.chitu_ext9_w4a16_gemm_silu, lib.chitu_ext9_w4a16_widen
    for name in ("x", "w", "scale", "out"):
        for bad in (None, odd):
            assert gemm(*_gemm_args(p, rows, **{name: bad})) == -1, name
            assert silu(*_silu_args(p, rows, **{name: bad})) == -1, name
            if name != "x":
                assert widen(*_widen_args(p, rows, **{name: bad})) == -1, name
    for bad in (dict(out_dtype=I32(3)), dict(out_dtype=I32(-1)), dict(M=I64(-1)), dict(N=I64(0)), dict(N=I64(-1)), dict(K=I64(0)),
                dict(K=I64(-128)), dict(N=I64(1 << 30)), dict(K=I64(1 << 30)), dict(M=I64(1 << 30))):
        assert gemm(*_gemm_args(p, rows, **bad)) == -1, bad
    for bad in (dict(M=I64(-1)), dict(inter=I64(0)), dict(inter=I64(-1)), dict(K=I64(0)), dict(inter=I64(1 << 29)), dict(K=I64(1 << 30)),
                dict(M=I64(1 << 30))):
        assert silu(*_silu_args(p, rows, **bad)) == -1, bad
    for bad in (dict(N=I64(-1)), dict(K=I64(0)), dict(K=I64(1 << 30)), dict(N=I64(1 << 30))):
        assert widen(*_widen_args(p, rows, **bad)) == -1, bad
    for k in (64, 192, 320):  # K must be a multiple of the group
        assert gemm(*_gemm_args(p, rows, K=I64(k))) == -2 and silu(*_silu_args(p, rows, K=I64(k))) == -2, k
        assert widen(*_widen_args(p, rows, K=I64(k))) == -2, k
    if rows == 0:  # nothing to do: 0 with nothing launched, valid arguments otherwise
        assert gemm(*_gemm_args(p, 0)) == 0 and silu(*_silu_args(p, 0)) == 0 and widen(*_widen_args(p, 0)) == 0


# ---------------------------------------------------------------- the references against themselves
def test_exactness_holds_over_the_grid_and_the_cap_from_the_references_alone():
    for entry in ("linear", "silu"):
        pool = w4.bf16_pool(entry, "pow2") + [w4.case(entry, "pow2", w4.TILED[0], w4.TILED[1] // (2 if entry == "silu" else 1), w4.TILED[2])]
        assert all(c.worst < 2.0 ** 24 and torch.equal(c.lo, c.hi) for c in pool)  # (Case's own assertion, restated)
        for kind in ("pow2", "quantiser"):
            n, total = w4.pooled_free(w4.bf16_pool(entry, kind))
            print(f"W4A16REF {entry} {kind} bf16: {n} of {total} elements with two admissible values")
            assert total > 30000 and n <= w4.CAP * total and (kind == "quantiser" or entry == "silu" or n == 0)
    for kind in ("pow2", "quantiser"):
        n, total = w4.pooled_free(w4.f16_pool(kind), torch.float16)
        print(f"W4A16REF linear {kind} f16: {n} of {total} elements with two admissible values")
        assert n <= w4.CAP * total
    c = w4.case("linear", "quantiser", 33, 40, 1152)
    v, mag = w4.value_and_magnitude(c.x, c.u, c.s)
    rho = 18 * 2.0 ** -24 * mag  # G + 9 at K = 1152
    assert bool((c.lo.double() >= v - rho).all()) and bool((c.hi.double() <= v + rho).all()) and bool((c.lo <= v.float()).all())
    assert bool((torch.nextafter(c.lo, torch.full_like(c.lo, float("-inf"))).double() < v - rho).all())  # the tightest such ends
    assert bool((torch.nextafter(c.hi, torch.full_like(c.hi, float("inf"))).double() > v + rho).all())


@pytest.mark.parametrize("M,N,K", [(17, 23, 384), (33, 40, 1152), (17, 24, w4.K_RING)])
def test_every_mutation_moves_the_pow2_expectation(M, N, K):
    """What a kernel could get wrong must be visible in the expectation: a scale swapped with its pair neighbour (the other
    row, the other group of the step, the other half of w13), a dropped group, a code off by one, two nibbles exchanged."""
    for entry in ("linear", "silu"):
        c = w4.case(entry, "pow2", M, N, K)
        rows, G = c.u.shape[0], K // 128

        P = w4.group_sums(c.x, c.u).to(torch.float64)

        def moved(u, s, row=None):
            """per weight row (or for `row` alone): some token's accumulator moved"""
            if row is not None:
                v = (w4.group_sums(c.x, u[row:row + 1]).to(torch.float64) * s[row:row + 1].to(torch.float64).unsqueeze(0)).sum(-1)
                return (v.to(torch.float32) != c.lo[:, row:row + 1]).any()
            v = (P * s.to(torch.float64).unsqueeze(0)).sum(-1)
            return (v.to(torch.float32) != c.lo).any(dim=0)

        for r in range(rows):
            for g in range(G):
                if g ^ 1 < G:
                    s = c.s.clone()
                    s[r, g], s[r, g ^ 1] = c.s[r, g ^ 1], c.s[r, g]
                    assert bool(moved(c.u, s)[r]), ("group neighbour", r, g)
                mate = (r // N) * N + ((r % N) ^ 1)  # the other row of the pair, inside the same half
                if (r % N) ^ 1 < N:
                    s = c.s.clone()
                    s[r, g], s[mate, g] = c.s[mate, g], c.s[r, g]
                    assert bool(moved(c.u, s)[r]), ("row neighbour", r, g)
        if entry == "silu":
            s = torch.cat([c.s[N:], c.s[:N]])
            assert bool(moved(c.u, s).all()), "halves"
        for g in range(G):  # one group dropped
            s = c.s.clone()
            s[:, g] = 0
            assert bool(moved(c.u, s).all()), ("dropped group", g)
        gen = torch.Generator().manual_seed(K + N)
        for _ in range(32):
            r, k = int(torch.randint(0, rows, (1,), generator=gen)), int(torch.randint(0, K, (1,), generator=gen))
            u = c.u.clone()
            u[r, k] = u[r, k] + 1 if u[r, k] < 15 else 14
            assert bool(moved(u, c.s, r)), ("code", r, k)
            k2 = k ^ 4  # the other nibble of channel k's byte
            if c.u[r, k] != c.u[r, k2]:
                u = c.u.clone()
                u[r, k], u[r, k2] = c.u[r, k2], c.u[r, k]
                assert bool(moved(u, c.s, r)), ("nibbles", r, k)


# ---------------------------------------------------------------- the loader
def _tiny_args(ffn_dim=256, **kw):
    from chitu_amd.llama import LlamaArgs
    from tests.util import HF_LLAMA_TINY

    c = dict(HF_LLAMA_TINY, dim=512, ffn_dim=ffn_dim)  # every shard of two ranks keeps K % 128 == 0
    return c, LlamaArgs(dim=c["dim"], n_layers=c["n_layers"], n_heads=c["n_heads"], n_kv_heads=c["n_kv_heads"], vocab_size=c["vocab_size"],
                        ffn_dim=c["ffn_dim"], **kw)


QUANTISED = re.compile(r"\.(wqkv|wo|w13|w2)$")


@pytest.mark.parametrize("world", [1, 2])
def test_loader_state_is_the_quantiser_of_each_ranks_shard_bit_for_bit(world):
    from chitu_amd import checkpoint as ck
    from chitu_amd.quantize import pack_w4a16, quant_weight_w4a16
    from tests.util import tiny_hf_llama_checkpoint

    c, args = _tiny_args(quant="w4a16g128")
    hf = tiny_hf_llama_checkpoint("llama", cfg=c)
    for rank in range(world):
        bf = ck.to_llama_module_names(ck.preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim, rank, world))
        st = ck.llama_to_w4a16(bf)
        n_q = 0
        for k, v in bf.items():
            if QUANTISED.search(k):
                packed, scales = pack_w4a16(*quant_weight_w4a16(v), halves=2 if k.endswith("w13") else 1)
                assert st[k].dtype == torch.uint8 and torch.equal(st[k], packed) and torch.equal(st[k + "_scale"], scales), k
                assert v.shape[1] % 128 == 0 and tuple(packed.shape) == (v.shape[0], v.shape[1] // 2)
                n_q += 1
            else:
                assert st[k] is v, k
        assert n_q == 4 * c["n_layers"] and len(st) == len(bf) + n_q


def test_a_rank_whose_local_k_is_off_the_group_is_refused():
    from chitu_amd import checkpoint as ck
    from tests.util import tiny_hf_llama_checkpoint

    c, args = _tiny_args(ffn_dim=384)
    hf = tiny_hf_llama_checkpoint("llama", cfg=c)
    ck.llama_to_w4a16(ck.to_llama_module_names(ck.preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim, 0, 1)))
    with pytest.raises(ValueError, match="192"):  # w2 of one of two ranks
        ck.llama_to_w4a16(ck.to_llama_module_names(ck.preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim, 1, 2)))


def test_load_checkpoint_hf_llama_fills_a_w4a16_decoder(tmp_path):
    from safetensors.torch import save_file

    from chitu_amd import checkpoint as ck
    from chitu_amd.llama import LlamaDecoder
    from tests.util import tiny_hf_llama_checkpoint

    c, args = _tiny_args(quant="w4a16g128")
    hf = tiny_hf_llama_checkpoint("llama", cfg=c)
    save_file({k: v.contiguous() for k, v in hf.items()}, str(tmp_path / "model.safetensors"))
    model = LlamaDecoder(args, None, None, max_position_embeddings=64, device="cpu")
    ck.load_checkpoint_hf_llama(model, str(tmp_path))
    want = ck.llama_to_w4a16(ck.to_llama_module_names(ck.preprocess_hf_llama(hf, args.n_heads, args.n_kv_heads, args.dim)))
    got = dict(model.named_parameters())
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
    assert got["layers.1.ffn.w13"].dtype == torch.uint8 and got["layers.1.ffn.w13_scale"].dtype == torch.float32
    assert got["head_weight"].dtype == torch.bfloat16
