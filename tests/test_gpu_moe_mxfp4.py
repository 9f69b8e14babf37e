"""HIP fused MoE with MXFP4 experts (W4A8, csrc/moe_mxfp4.hip) on the MI355X: the scaled MFMA's lane map with exact data,
the quantiser / dequantiser bit for bit, fused_experts(use_mxfp4_w4a8=True) against the pinned fp8 oracle (on weights that are
both) and against tests/mxfp4_ref.py, against the fp8 HIP path, its options, a tiny DeepSeek-V3 with MXFP4 experts, the loader."""

import functools

import pytest
import torch

from oracle import moe as omoe
from tests import mxfp4_ref as mx
from tests.util import CKPT_TINY, assert_close, max_rel_to_peak, tiny_hf_checkpoint

pytestmark = pytest.mark.gpu

REL_TOL = 1e-2


# ---------------------------------------------------------------- lane map, exact integer data
def _plain_gemm(aq, a_s, a_div, w, ws, ids, E, wts=None):
    """chitu_hip_moe_gemm_mxfp4 on its own: out bf16 [numel, N], between guard rows that must stay untouched."""
    from chitu_amd import _lib, fused_moe
    from chitu_amd._lib import check, i32, i64, ptr, stream_ptr

    numel, N = ids.numel(), w.shape[1]
    K = aq.shape[1]
    sorted_ids, expert_ids, npost = fused_moe.moe_align_block_size(ids.cuda(), 16, E)
    guard = 4  # rows before and after the output, NaN like the output itself: a store to row numel (a padding slot's id) shows
    full = torch.full((numel + 2 * guard, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    out = full[guard:guard + numel]
    keep = [aq.cuda(), a_s.cuda(), w.cuda(), ws.cuda(), None if wts is None else wts.cuda()]
    check(_lib.lib().chitu_hip_moe_gemm_mxfp4(ptr(keep[0]), ptr(keep[1]), i32(a_div), ptr(keep[2]), ptr(keep[3]), ptr(sorted_ids),
                                              ptr(expert_ids), ptr(npost), ptr(keep[4]), i32(2), i32(0 if wts is None else 1),
                                              ptr(out), i64(numel), i64(N), i64(K), i64(min(expert_ids.numel(), numel)),
                                              stream_ptr()), "moe_gemm_mxfp4")
    torch.cuda.synchronize()
    assert torch.isnan(full[:guard]).all() and torch.isnan(full[guard + numel:]).all(), "moe_gemm_mxfp4 stored outside its output rows"
    return out.cpu()


@pytest.mark.parametrize("K,N", [(384, 40), (256, 16), (128, 24)])  # odd and even K-block counts, N no multiple of the tile
def test_lane_map_with_exact_integer_data(K, N):
    """Weights: e2m1 codes whose values are integers, every (row, 32-block) with its own power-of-two scale 2^0..2^3;
    activations: small integers as e4m3, unit group scales.  Every product and every partial sum is an integer below 2^24, so
    the fp32 result is THE integer matmul whatever the summation order.  (a) one-hot activations -- token k holds a single 1
    at k, so out[k, n] = W[n, k] exactly, also in bf16: pins which k and which scale byte every lane carries, asymmetrically;
    (b) dense integers against the exact matmul rounded once to bf16."""
    g = torch.Generator().manual_seed(K + N)
    E = 3
    int_codes = torch.tensor([0, 2, 4, 5, 6, 7, 10, 12, 13, 14, 15], dtype=torch.uint8)  # 0, +-1, +-2, +-3, +-4, +-6
    codes = int_codes[torch.randint(0, len(int_codes), (E, N, K), generator=g)]
    scales = torch.randint(127, 131, (E, N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    w = mx.pack(codes)
    wf = mx.dequant_f32(w, scales)  # [E, N, K] integers up to 48
    # (a) identity
    ids = (torch.arange(K) % E).view(K, 1)
    eye = torch.eye(K).to(torch.float8_e4m3fn)
    out = _plain_gemm(eye, torch.ones(K, K // 128), 1, w, scales, ids, E)
    want = torch.stack([wf[int(ids[k]), :, k] for k in range(K)])
    bad = (out.float() != want).nonzero()
    assert len(bad) == 0, f"out[k, n] != W[expert(k), n, k] at {len(bad)} places, first (k, n): {bad[:12].tolist()}"
    # (b) dense, several tokens per expert and more than one 16-slot tile for expert 0; topk 2 (a_div)
    M = 21
    x = torch.randint(-4, 5, (M, K), generator=g).float()
    ids = torch.stack([torch.randperm(E, generator=g)[:2] for _ in range(M)])
    ids[:18, 0], ids[:18, 1] = 0, 1 + (torch.arange(18) % 2)
    out = _plain_gemm(x.to(torch.float8_e4m3fn), torch.ones(M, K // 128), 2, w, scales, ids, E)
    exact = torch.stack([x[s // 2] @ wf[int(ids.view(-1)[s])].T for s in range(2 * M)])
    assert float(exact.abs().max()) < 2 ** 24
    assert torch.equal(out, exact.to(torch.bfloat16))
    # the routed weight multiplies the fp32 accumulator (powers of two: still exact)
    wts = torch.tensor([0.5, 2.0, 1.0, 4.0]).repeat(2 * M)[: 2 * M].view(M, 2)
    out = _plain_gemm(x.to(torch.float8_e4m3fn), torch.ones(M, K // 128), 2, w, scales, ids, E, wts=wts)
    assert torch.equal(out, (exact * wts.view(-1, 1)).to(torch.bfloat16))


# ---------------------------------------------------------------- quantiser / dequantiser
def _quant_inputs():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(37, 256, generator=g) * torch.logspace(-6, 4, 37).view(-1, 1)
    v[3] = 0.0                                   # zero blocks
    v[4, 32:64] = 0.0
    v[5, :8] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 4.0])  # ties under a block maximum of 4 (X = 0)
    v[5, 8:32] = 0.0
    v[6, :8] = torch.tensor([-0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -4.0])
    v[6, 8:32] = 0.0
    v[7, :6] = torch.tensor([7.9, -7.5, 6.5, 5.0000005, -5.0, 0.1])            # saturation: above 5 -> 6
    v[7, 6:32] = 0.0
    v[8, :32] = 1e-41                            # subnormal block maximum
    v[9, :32] = 3e38
    return v


def test_quantiser_and_dequantiser_are_bit_exact_against_the_reference():
    from chitu_amd.quantize import mxfp4

    v = _quant_inputs()
    for src in (v, v.to(torch.bfloat16), v.to(torch.float16).clamp(-6e4, 6e4)):
        p_ref, s_ref = mx.quant(src.float())
        p, s = mxfp4.quant_mxfp4(src.cuda())
        assert p.dtype == torch.uint8 and tuple(p.shape) == (37, 128) and tuple(s.shape) == (37, 8)
        assert torch.equal(s.cpu(), s_ref), src.dtype
        assert torch.equal(p.cpu(), p_ref), src.dtype
        ok = (s_ref >= 2) & (s_ref <= 252)  # the specified scale range
        d = mxfp4.dequant_mxfp4(p, s).cpu()
        d_ref = mx.dequant(p_ref, s_ref)
        sel = ok.repeat_interleave(32, dim=1)
        assert torch.equal(d.view(torch.int16)[sel], d_ref.view(torch.int16)[sel])
    assert int(s_ref[3].max()) == 0 and int(s_ref[4, 1]) == 0, "an all-zero block gets scale byte 0"
    # every code at every specified scale byte, and NaN for 0xFF
    codes = torch.arange(16, dtype=torch.uint8).repeat(2).view(1, 32).expand(251, 32)
    packed = mx.pack(codes).contiguous()
    sc = torch.arange(2, 253, dtype=torch.uint8).view(251, 1)
    d = mxfp4.dequant_mxfp4(packed.cuda(), sc.cuda()).cpu()
    assert torch.equal(d.view(torch.int16), mx.dequant(packed, sc).view(torch.int16))
    assert torch.isnan(mxfp4.dequant_mxfp4(packed[:1].cuda(), torch.tensor([[255]], dtype=torch.uint8).cuda()).float()).all()
    # leading dimensions pass through
    p3, s3 = mxfp4.quant_mxfp4(v.view(37, 2, 128)[:36].reshape(4, 9, 2, 128).cuda())
    assert tuple(p3.shape) == (4, 9, 2, 64) and tuple(s3.shape) == (4, 9, 2, 4)


def test_quantiser_from_fp8_block_scaled_weights():
    from chitu_amd.quantize import mxfp4

    g = torch.Generator().manual_seed(8)
    w = (torch.randn(3, 200, 384, generator=g) * 0.5).to(torch.float8_e4m3fn)  # 200 rows: a partial last row block
    w.view(torch.uint8)[0, 5, :32] = 0                                          # a zero block
    s = torch.rand(3, 2, 3, generator=g) * 0.02 + 0.01
    p, sc = mxfp4.quant_mxfp4_from_fp8_block(w.cuda(), s.cuda())
    p_ref, s_ref = mx.quant_from_fp8_block(w, s)
    assert torch.equal(sc.cpu(), s_ref) and torch.equal(p.cpu(), p_ref)
    p2, sc2 = mxfp4.quant_mxfp4_from_fp8_block(w[1].cuda(), s[1].cuda())       # a single matrix
    assert torch.equal(p2.cpu(), p_ref[1]) and torch.equal(sc2.cpu(), s_ref[1])


# ---------------------------------------------------------------- fused_experts vs the oracle
SHAPES = [
    (1, 32, 8, 7168, 256),    # R1 TP=8 per-expert shapes, bs=1
    (16, 32, 8, 7168, 256),   # bs=16 (several tokens per expert)
    (33, 16, 4, 512, 128),    # > one 16-slot tile per expert
    (5, 8, 2, 256, 128),      # fixture shape
    (7, 8, 3, 384, 640),      # I/128 = 5, K/128 = 3: the three-launch form, half steps in both GEMMs
    (4, 64, 6, 2048, 384),    # V2-Lite-like: 64 experts, top-6; three K blocks in GEMM2
    (16, 64, 8, 2048, 1408),  # DeepSeek-V2-Lite's expert width (11 K blocks)
    (5, 8, 2, 512, 2048),     # an expert-parallel rank's full-width R1 experts
    (40, 4, 2, 256, 1024),    # several 16-slot tiles per expert
]


@functools.lru_cache(maxsize=None)
def twin_case(M, E, topk, K, I, seed=None):
    """Inputs whose MXFP4 weights are at the same time fp8 block-scaled weights (tests/test_mxfp4_host.py proves the equality),
    and the pinned oracle's result on them.  Computed once per shape."""
    g = torch.Generator().manual_seed(M * 1000 + E if seed is None else seed)
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    w1p, w1s, w1_8, w1_bs = mx.fp8_twin_weights(E, 2 * I, K, g)
    w2p, w2s, w2_8, w2_bs = mx.fp8_twin_weights(E, K, I, g)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(M)])
    wts = torch.rand(M, topk, generator=g).to(torch.bfloat16)
    ref = omoe.fused_experts_fp8(x, w1_8, w2_8, wts, ids, w1_bs, w2_bs)
    return dict(x=x, w1=w1p, w1s=w1s, w2=w2p, w2s=w2s, w1_8=w1_8, w2_8=w2_8, w1_bs=w1_bs, w2_bs=w2_bs, ids=ids, wts=wts, ref=ref)


def run_mx(c, x=None, **kw):
    from chitu_amd import fused_moe

    xd = (c["x"] if x is None else x).cuda().clone()
    wts, ids = kw.pop("wts", c["wts"]), kw.pop("ids", c["ids"])
    w1, w1s, w2, w2s = (kw.pop(k, c[k]) for k in ("w1", "w1s", "w2", "w2s"))
    out = fused_moe.fused_experts(xd, w1.cuda(), w2.cuda(), wts.cuda(), ids.cuda(), use_mxfp4_w4a8=True,
                                  w1_scale=w1s.cuda(), w2_scale=w2s.cuda(), **kw)
    if kw.get("inplace"):
        assert out.data_ptr() == xd.data_ptr()
    return out.cpu()


def _bars(out, ref, what, outliers=0):
    print(f"{what}: peak err {max_rel_to_peak(out, ref):.3e}, mean err "
          f"{((out.float() - ref.float()).abs().mean() / ref.float().abs().mean()).item():.3e}")
    assert_close(out, ref, REL_TOL, what=what, outlier_frac=outliers / out.numel())
    assert ((out.float() - ref.float()).abs().mean() / ref.float().abs().mean()).item() < 5e-3


# Elements allowed outside the ELEMENT-WISE bar (they stay under the peak bar), per weight family and shape: none, except where
# the census on the MI355X (tools/moe_mxfp4_outliers.py, profiles/mxfp4_moe_outlier_census.txt, docs/design/4_parity.md) finds
# elements outside it whose SOLE cause is the documented one of tests/test_gpu_moe.py:83-91 -- h is re-quantised to fp8 between
# the two GEMMs, HIP's and the reference's fp32 sums over K differ in order, an h value lands on neighbouring e4m3 codes (one
# step = 6 %) and the outputs fed by it move: against the reference's GEMM2 evaluated on HIP's own h codes nothing is outside
# the bar.  The allowance is a count, bounded by that precedent's share 20 / 114 688 of the shape's elements (32 768 -> 5), not
# by what the kernels happen to give; the seeds leave zero elements between the reference's fp32 and fp64 evaluations.
ALLOWED = {("twin", 16, 64, 8, 2048, 1408): 32768 * 20 // 114688}


@pytest.mark.parametrize("M,E,topk,K,I", SHAPES)
def test_vs_the_fp8_oracle_on_fp8_representable_weights(M, E, topk, K, I):
    c = twin_case(M, E, topk, K, I)
    out = run_mx(c)
    _bars(out, c["ref"], f"mxfp4 experts, fp8-representable weights {M, E, topk, K, I}", ALLOWED.get(("twin", M, E, topk, K, I), 0))
    assert torch.equal(out, run_mx(c))  # no atomics: run to run identical


@functools.lru_cache(maxsize=None)
def free_case(M, E, topk, K, I):
    """Weights quantised freely from randn (any scale byte per block, no fp8 twin) and the local reference's result."""
    g = torch.Generator().manual_seed(M * 1000 + E + 3)
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    w1, w1s = mx.quant(torch.randn(E, 2 * I, K, generator=g) * 0.01)
    w2, w2s = mx.quant(torch.randn(E, K, I, generator=g) * 0.01)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(M)])
    wts = torch.rand(M, topk, generator=g).to(torch.bfloat16)
    ref = mx.fused_experts_mxfp4(x, w1, w1s, w2, w2s, wts, ids)
    return dict(x=x, w1=w1, w1s=w1s, w2=w2, w2s=w2s, ids=ids, wts=wts, ref=ref)


@pytest.mark.parametrize("M,E,topk,K,I", SHAPES)
def test_vs_the_local_reference_on_freely_quantised_weights(M, E, topk, K, I):
    c = free_case(M, E, topk, K, I)
    _bars(run_mx(c), c["ref"], f"mxfp4 experts, randn weights {M, E, topk, K, I}", ALLOWED.get(("free", M, E, topk, K, I), 0))


@pytest.mark.parametrize("M,E,topk,K,I", [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[4]])
def test_vs_the_fp8_hip_path_on_the_same_weights(M, E, topk, K, I):
    """The existing fp8 kernels on the fp8 twin: same values, same rounding points; the sum inside a 128-block is ordered
    differently (and the weights' scale is applied inside the block dot instead of after it: exact, powers of two)."""
    from chitu_amd import fused_moe

    c = twin_case(M, E, topk, K, I)
    f8 = fused_moe.fused_experts(c["x"].cuda().clone(), c["w1_8"].cuda(), c["w2_8"].cuda(), c["wts"].cuda(), c["ids"].cuda(),
                                 use_fp8_w8a8=True, w1_scale=c["w1_bs"].cuda(), w2_scale=c["w2_bs"].cuda(), block_shape=[128, 128]).cpu()
    _bars(run_mx(c), f8, f"mxfp4 vs fp8 HIP {M, E, topk, K, I}")


# ---------------------------------------------------------------- options
def test_option_combinations_against_the_plain_call():
    from chitu_amd import fused_moe, ops

    M, E, topk, K, I = 9, 8, 2, 256, 128
    c = twin_case(M, E, topk, K, I, seed=19)
    plain = run_mx(c)
    _bars(plain, c["ref"], "plain")
    # inplace
    assert torch.equal(run_mx(c, inplace=True), plain)
    # reduce_topk=False: the routed-weighted expert outputs; their fp32 sum rounded once is the plain output
    un = run_mx(c, reduce_topk=False)
    assert tuple(un.shape) == (M, topk, K) and torch.equal(un.float().sum(1).to(torch.bfloat16), plain)
    # a1_quant: the producer's per-128-group fp8 form of the tokens
    aq, as_ = fused_moe.per_token_group_quant_fp8(c["x"].cuda(), 128)
    assert torch.equal(run_mx(c, a1_quant=(aq, as_)), plain)
    # aligned: moe_align computed inside the routing launch (ops.gate_deepseek_v3(align=...)) -- here the ids come from it too
    g = torch.Generator().manual_seed(2)
    gate_w = (torch.randn(E, K, generator=g) * K ** -0.5).to(torch.bfloat16).cuda()
    routed = ops.gate_deepseek_v3(c["x"].cuda(), gate_w, None, 1, 1, topk, "sigmoid", 1.0, align=(E, 16, None))
    assert len(routed) == 3
    r_wts, r_ids = routed[0].cpu(), routed[1].cpu()
    with_align = run_mx(c, wts=r_wts, ids=r_ids, aligned=routed[2])
    assert torch.equal(with_align, run_mx(c, wts=r_wts, ids=r_ids))
    # expert_map with absent experts: this rank holds the first half; the others' slots contribute zeros
    h = E // 2
    emap = torch.full((E,), -1, dtype=torch.int32)
    emap[:h] = torch.arange(h, dtype=torch.int32)
    mapped = run_mx(c, w1=c["w1"][:h].contiguous(), w1s=c["w1s"][:h].contiguous(), w2=c["w2"][:h].contiguous(),
                    w2s=c["w2s"][:h].contiguous(), expert_map=emap.cuda(), global_num_experts=E)
    masked = torch.where(c["ids"] < h, c["wts"].float(), torch.zeros(())).to(c["wts"].dtype)
    assert torch.equal(mapped, run_mx(c, wts=masked)), "an absent expert = a zero routed weight"
    assert_close(mapped, omoe.fused_experts_fp8(c["x"], c["w1_8"], c["w2_8"], masked, c["ids"], c["w1_bs"], c["w2_bs"]), REL_TOL)
    # the same on the three-launch form (wide experts)
    cw = twin_case(7, 8, 3, 384, 640)
    mapped = run_mx(cw, w1=cw["w1"][:h].contiguous(), w1s=cw["w1s"][:h].contiguous(), w2=cw["w2"][:h].contiguous(),
                    w2s=cw["w2s"][:h].contiguous(), expert_map=emap.cuda(), global_num_experts=E)
    masked = torch.where(cw["ids"] < h, cw["wts"].float(), torch.zeros(())).to(cw["wts"].dtype)
    assert torch.equal(mapped, run_mx(cw, wts=masked))
    # zero tokens
    z = run_mx(c, x=c["x"][:0], wts=c["wts"][:0], ids=c["ids"][:0])
    assert tuple(z.shape) == (0, K)
    # the other 4-bit / weight-only modes still raise
    for bad in ({"use_int8_w8a16": True}, {"use_int4_w4a16": True}):
        with pytest.raises(NotImplementedError):
            fused_moe.fused_experts(c["x"].cuda(), c["w1_8"].cuda(), c["w2_8"].cuda(), c["wts"].cuda(), c["ids"].cuda(), **bad)


def test_k_split_variants_agree():
    """Every K-split width of GEMM1 (waves per workgroup) computes the same function up to the order of the fp32 sum."""
    from chitu_amd._lib import debug_option

    c = twin_case(16, 32, 8, 7168, 256)
    for wk in (1, 2, 4, 8):
        with debug_option("moe_gemm1_wk", wk):
            _bars(run_mx(c), c["ref"], f"WK={wk}", ALLOWED.get(("twin", 16, 32, 8, 7168, 256), 0))
    cw = twin_case(7, 8, 3, 384, 640)  # K = 3 blocks = 2 steps: the split is capped at 2 waves
    for wk in (1, 8):
        with debug_option("moe_gemm1_wk", wk):
            _bars(run_mx(cw), cw["ref"], f"wide, WK={wk}")


# ---------------------------------------------------------------- model
def tiny_args(**kw):
    """tests/test_gpu_deepseek.py::tiny_args, restated."""
    from chitu_amd.deepseek_v3 import DeepSeekV3Args

    return DeepSeekV3Args(
        vocab_size=1024, dim=512, inter_dim=1024, moe_inter_dim=256, n_layers=3, n_dense_layers=1, n_heads=16,
        n_routed_experts=16, n_shared_experts=1, n_activated_experts=4, n_expert_groups=4, n_limited_groups=2,
        q_lora_rank=256, gate_bias=True, **kw)


def _build(args, seed=0):
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager
    from chitu_amd.deepseek_v3 import DeepSeekV3Decoder, init_synthetic_

    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=2, block_size=64, max_seq_len=256, device="cuda",
                                kv_shape_per_sample=(576,), dtype=torch.bfloat16)
    model = DeepSeekV3Decoder(args, cache, HipAttnBackend(local_n_heads=16, max_seq_len=256), max_position_embeddings=256,
                              device="cuda")
    init_synthetic_(model, seed=seed)
    return model, cache


def _decode(model, cache, kv, use_graph):
    reqs = ["a", "b"]
    for r, n in zip(reqs, (70, 5)):
        cache.register_sequence(r, n)
    for r in reqs:
        for blk in cache.block_table[r]:
            cache.paged_kv_cache[:, blk] = kv.cuda()
    cache.prepare_cache_decode(reqs)
    cache.prepare_block_table_for_decode(reqs)
    model.prepare_decoding_attn()
    tokens = torch.tensor([5, 900], dtype=torch.int64, device="cuda")
    out = model.decode(tokens, use_graph=use_graph).clone()
    cache.finalize_cache_single_decode(reqs)
    for r in reqs:
        cache.finalize_cache_all_decode(r)
    return out


def test_tiny_model_with_mxfp4_experts_matches_its_fp8_twin_and_captures():
    from chitu_amd.deepseek_v3 import refresh_derived_layouts

    g = torch.Generator().manual_seed(4)
    kv = (torch.randn(3, 64, 576, generator=g) * 0.5).to(torch.bfloat16)
    m8, c8 = _build(tiny_args())
    m4, c4 = _build(tiny_args(expert_dtype="mxfp4"), seed=1)
    # synthetic MXFP4 experts: uint8 parameters, scale bytes in the narrow band, finite outputs
    ffn = m4.layers[1].ffn
    assert ffn.w1w3_weight.dtype == torch.uint8 and tuple(ffn.w1w3_weight.shape) == (17, 512, 256)
    assert tuple(ffn.w1w3_scale.shape) == (17, 512, 16) and tuple(ffn.w2_weight.shape) == (17, 512, 128) and tuple(ffn.w2_scale.shape) == (17, 512, 8)
    assert int(ffn.w1w3_scale.min()) >= 118 and int(ffn.w1w3_scale.max()) <= 120 and len(torch.unique(ffn.w2_weight)) == 256
    # an fp8 model initialises exactly as before: nothing is drawn for uint8 when there is none
    again, _ = _build(tiny_args())
    for (k, a), (_, b) in zip(m8.named_parameters(), again.named_parameters()):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
    del again
    # the twin: both models share every other parameter, and the experts are the same values in the two formats
    p8, p4 = dict(m8.named_parameters()), dict(m4.named_parameters())
    with torch.no_grad():
        for k in p8:
            if ".ffn.w1w3_" in k or ".ffn.w2_" in k:
                continue
            p4[k].copy_(p8[k])
        for i, layer in enumerate(m8.layers):
            if not layer.is_moe:
                continue
            for name, R, K in (("w1w3", 512, 512), ("w2", 512, 256)):
                packed, scales, w8, bs = mx.fp8_twin_weights(17, R, K, g)
                p4[f"layers.{i}.ffn.{name}_weight"].copy_(packed)
                p4[f"layers.{i}.ffn.{name}_scale"].copy_(scales)
                p8[f"layers.{i}.ffn.{name}_weight"].copy_(w8.cuda())
                p8[f"layers.{i}.ffn.{name}_scale"].copy_(bs)
    refresh_derived_layouts(m4)
    l8 = _decode(m8, c8, kv, use_graph=False)
    l4 = _decode(m4, c4, kv, use_graph=False)
    assert torch.isfinite(l4).all()
    print(f"tiny model, mxfp4 vs fp8 twin: {max_rel_to_peak(l4, l8):.3e} of the peak")
    assert_close(l4, l8, 6e-2, what="decode logits, MXFP4 experts vs their fp8 twin")
    g4 = _decode(m4, c4, kv, use_graph=True)  # graphs.capture_verified inside
    assert torch.equal(g4, l4), "the captured step equals the eager step bit for bit"


# ---------------------------------------------------------------- loader
def test_loader_converts_fp8_experts_and_round_trips_the_preprocessed_form(tmp_path):
    from safetensors.torch import save_file

    from chitu_amd import checkpoint as ck
    from chitu_amd.deepseek_v3 import DeepSeekV3Args, DeepSeekV3Decoder

    keys = ("vocab_size", "dim", "inter_dim", "moe_inter_dim", "n_layers", "n_dense_layers", "n_heads", "n_routed_experts",
            "n_shared_experts", "n_activated_experts", "n_expert_groups", "n_limited_groups", "route_scale", "score_func",
            "q_lora_rank", "kv_lora_rank", "qk_nope_head_dim", "qk_rope_head_dim", "v_head_dim", "rope_theta", "rope_factor")
    mk = lambda dt: DeepSeekV3Decoder(DeepSeekV3Args(**{k: CKPT_TINY[k] for k in keys}, gate_bias=True, shard_degree=1, expert_dtype=dt),
                                      None, None, max_position_embeddings=64, device="cuda")
    save_file({k: v.contiguous() for k, v in tiny_hf_checkpoint().items()}, str(tmp_path / "model-00001-of-00001.safetensors"))
    m8, m4 = mk("fp8"), mk("mxfp4")
    ck.load_checkpoint_deepseek_v3(m8, str(tmp_path))
    ck.load_checkpoint_deepseek_v3(m4, str(tmp_path))
    p8, p4 = dict(m8.named_parameters()), dict(m4.named_parameters())
    assert set(p8) == set(p4)
    n_conv = 0
    for k in p8:
        if ".ffn.w1w3_weight" in k or ".ffn.w2_weight" in k:
            s = k.replace("_weight", "_scale")
            packed, scales = mx.quant_from_fp8_block(p8[k].cpu(), p8[s].cpu())  # the reference's quantisation of the dequantised fp8
            assert p4[k].dtype == torch.uint8 and torch.equal(p4[k].cpu(), packed), k
            assert p4[s].dtype == torch.uint8 and torch.equal(p4[s].cpu(), scales), s
            n_conv += 1
        elif ".ffn.w1w3_scale" not in k and ".ffn.w2_scale" not in k:
            assert torch.equal(p4[k].view(torch.uint8), p8[k].view(torch.uint8)), k
    assert n_conv == 2
    ck.save_preprocessed(m4, str(tmp_path / "pre"), 0)
    again = mk("mxfp4")
    ck.load_checkpoint_deepseek_v3(again, str(tmp_path / "pre"), skip_preprocess=True)
    for (k, a), (k2, b) in zip(m4.named_parameters(), again.named_parameters()):
        assert k == k2 and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
