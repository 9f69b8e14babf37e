"""W4A16 g128 kernels (include/chitu_hip_ext9.h, csrc/w4a16_gemm.hip) on the GPU.

Exact: integer activations |x| <= 8, scales in {1/2, 1, 2}, codes over 0..15.  Every partial sum is a multiple of 1/2 below
256 K half-units, an exact fp32 number for K < 65536, so the fp64 product rounded once equals the kernel bit for bit.
Random: |out - ref| <= 2^-8 |ref| + K 2^-23 sum_k |x_k w_k| for every element -- twice the bf16 rounding bound plus twice the
fp32 accumulation bound, derived, not measured.
Model: the logits bar between a quantised model and its bf16 twin is tests/test_gpu_w8a16_model.py's LOGITS_BAR (3e-2 of the
peak, compare_with_whole's): the bound above does not carry through two layers of norms, softmax and SiLU."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
K_RING = 10368  # 41 K steps (40 lines and a half-line tail) on one tile: 8 waves of 5 or 6 steps, more than the ring of 4


def build(M, N, K, seed, exact=True, halves=1):
    """(x bf16 [M, K] on the GPU, packed, scales on the GPU, W fp64 [N, K] = (u - 8) * s, u, s)."""
    from chitu_amd.quantize.w4a16 import pack_w4a16

    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    u[:, 0], u[:, K - 1] = 0, 15
    n, grp = torch.arange(N).view(N, 1), torch.arange(K // 128).view(1, -1)
    if exact:
        x = torch.randint(-8, 9, (M, K), generator=g).to(BF16)
        # distinct across the neighbours of every 2 x 2 (row pair, K step) block: along the diagonal in odd blocks, across it in even ones
        s = torch.tensor([0.5, 1.0, 2.0])[torch.where((n // 2 + grp // 2) % 2 == 0, n + grp, n + 2 * grp) % 3]
    else:
        x = torch.randn(M, K, generator=g).to(BF16)
        s = torch.rand(N, K // 128, generator=g) * 0.02 + 1e-3
    packed, scales = pack_w4a16(u, s, halves=halves)
    W = (u.double() - 8.0) * s.double().repeat_interleave(128, dim=1)
    return x.cuda(), packed.cuda(), scales.cuda(), W, u, s


AXES = ([(17, 24, K) for K in (128, 256, 384, K_RING)] + [(1, 24, K_RING)] + [(17, N, 384) for N in (8, 16)]
        + [(M, 24, 384) for M in (1, 16, 33)])


@pytest.mark.parametrize("M,N,K", AXES)
def test_linear_is_the_fp64_product_rounded_once(M, N, K):
    from chitu_amd import ops

    if K == K_RING:
        mt, wk, depth = ops.w4a16_plan(M, N, K)["launches"][0]
        assert wk > 1 and -(-K // 256) // wk > depth, (mt, wk, depth)
    x, packed, scales, W, _, _ = build(M, N, K, seed=M * 1000 + N * 10 + K)
    ref = x.double().cpu() @ W.t()
    for dt in (BF16, F32):
        out = ops.w4a16_linear(x, packed, scales, out_dtype=dt).cpu()
        assert torch.equal(out, ref.to(F32).to(dt)), (dt, (out.double() - ref).abs().max())


@pytest.mark.parametrize("M,K", [(1, 384), (17, 384), (1, K_RING), (17, K_RING)])
def test_linear_silu_is_the_bf16_launch_on_the_dequantised_weights(M, K):
    from chitu_amd import ops

    x, packed, scales, W, _, _ = build(M, 48, K, seed=M + K, halves=2)
    assert torch.equal(W.to(BF16).double(), W)  # the dequantisation is exact: both launches run the same rounding chain
    out = ops.w4a16_linear_silu(x, packed, scales)
    assert tuple(out.shape) == (M, 24) and torch.equal(out, ops.bf16_linear_silu(x, W.to(BF16).cuda()))


def test_widen_and_the_tiled_form():
    from chitu_amd import ops

    _, packed, scales, _, u, s = build(1, 5, 384, seed=5, exact=False)
    want = ((u.float() - 8.0) * s.repeat_interleave(128, dim=1)).to(BF16)
    assert torch.equal(ops.w4a16_widen(packed, scales).cpu(), want)
    M, N, K = 128, 6144, 128  # the smallest M the plan sends to the tiled form
    assert ops.w4a16_plan(M, N, K)["form"] == "tiled" and ops.w4a16_plan(M - 1, N, K)["form"] == "stream"
    x, packed, scales, _, _, _ = build(M, N, K, seed=6, exact=False)
    assert torch.equal(ops.w4a16_linear(x, packed, scales), ops.bf16_linear(x, ops.w4a16_widen(packed, scales)))


@pytest.mark.parametrize("M,N,K", [(17, 24, 1152), (1, 40, K_RING)])
def test_random_inputs_within_the_derived_bound(M, N, K):
    from chitu_amd import ops

    x, packed, scales, W, _, _ = build(M, N, K, seed=K + M, exact=False)
    xd = x.double().cpu()
    ref, mag = xd @ W.t(), xd.abs() @ W.abs().t()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
    for dt in (BF16, F32):
        err = (ops.w4a16_linear(x, packed, scales, out_dtype=dt).double().cpu() - ref).abs()
        print(f"W4A16 random M={M} N={N} K={K} {dt}: max err / bound {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all())


def test_tiny_llama_graph_equals_eager_and_prefill_matches_the_bf16_twin():
    from chitu_amd.quantize import dequant_weight_w4a16, quantize_w4a16_, unpack_w4a16
    from chitu_amd.quantize.w4a16 import W4A16_WEIGHTS
    from tests.test_gpu_prefill_paged import prompts_of, release
    from tests.test_gpu_w8a16_model import LOGITS_BAR, _decoder
    from tests.util import assert_close

    mq, cq = _decoder("llama")
    mt, ct = _decoder("llama")
    quantize_w4a16_(mq)
    for lq, lt in zip(mq.layers, mt.layers):
        for part, name, halves in W4A16_WEIGHTS:
            packed, scales = getattr(getattr(lq, part), name), getattr(getattr(lq, part), name + "_scale")
            assert packed.dtype == torch.uint8 and scales.dtype == F32
            getattr(getattr(lt, part), name).data.copy_(dequant_weight_w4a16(*unpack_w4a16(packed, scales, halves=halves)).to(BF16))
    prompts = prompts_of(mq.args.vocab_size)
    ids = ["a0", "a1", "a2"]
    lq, lt = mq.prefill(prompts, ids), mt.prefill(prompts, ids)
    print(f"W4A16 model prefill logits vs the bf16 twin, of the peak: {assert_close(lq, lt, LOGITS_BAR, what='prefill'):.3e}")
    release(cq), release(ct)
    with_graph, without = mq.generate(prompts, 6, use_graph=True), mq.generate(prompts, 6, use_graph=False)
    assert torch.equal(with_graph, without) and tuple(with_graph.shape) == (3, 6)
