"""W4A16 g128 decoders on the GPU beyond the Llama twin of tests/test_gpu_w4a16.py: tiny Qwen2 (QKV bias), Qwen3 (head norm) and
GLM-4 (partial interleaved RoPE, bias) models of tests/test_gpu_w8a16_model.py's shape after quantize_w4a16_, against a bf16 twin
whose four linears per layer hold bf16(dequant(u, s)); one prefill long enough for the widen + tiled form; graph replay against
the eager step.  The bar is that module's LOGITS_BAR (3e-2 of the peak), nothing else."""
import gc

import pytest
import torch

from tests.test_gpu_prefill_paged import prompts_of, release, rows_of
from tests.test_gpu_w8a16_model import A, B, LOGITS_BAR, PAGE, SHAPE, _decoder, decode_step
from tests.util import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def models_are_gone_after_each_test():
    yield
    gc.collect()


def _decoder4(kind):
    if kind != "glm4":
        return _decoder(kind)
    from chitu_amd.attn_backend import HipAttnBackend
    from chitu_amd.cache_manager import PagedKVCacheManager, gqa_kv_layout
    from chitu_amd.glm4 import Glm4Args, Glm4Decoder
    from chitu_amd.llama import init_synthetic_

    args = Glm4Args(**SHAPE)
    shape, dtype = gqa_kv_layout("bf16", args.n_kv_heads)
    cache = PagedKVCacheManager(0, args.n_layers, num_hot_req=8, block_size=PAGE, max_seq_len=512, device="cuda",
                                k_shape_per_sample=shape, v_shape_per_sample=shape, dtype=dtype)
    model = Glm4Decoder(args, cache, HipAttnBackend(local_n_heads=args.n_heads, max_seq_len=512), max_position_embeddings=512, device="cuda")
    init_synthetic_(model, seed=0)
    return model, cache


def pair(kind):
    """(W4A16 model, its cache, bf16 twin, its cache): the same synthetic weights, the first quantised in place, the twin's four
    linears per layer overwritten with bf16(dequant) of the first's codes; everything else equal and bf16"""
    from chitu_amd.quantize import dequant_weight_w4a16, quantize_w4a16_, unpack_w4a16
    from chitu_amd.quantize.w4a16 import W4A16_WEIGHTS

    mq, cq = _decoder4(kind)
    mt, ct = _decoder4(kind)
    quantize_w4a16_(mq)
    assert mq.args.quant == "w4a16g128" and mt.args.quant is None
    for lq, lt in zip(mq.layers, mt.layers):
        for part, name, halves in W4A16_WEIGHTS:
            packed, scales = getattr(getattr(lq, part), name), getattr(getattr(lq, part), name + "_scale")
            assert packed.dtype == torch.uint8 and scales.dtype == torch.float32
            getattr(getattr(lt, part), name).data.copy_(dequant_weight_w4a16(*unpack_w4a16(packed, scales, halves=halves)).to(torch.bfloat16))
    names = tuple(n for _, n, _ in W4A16_WEIGHTS)
    for (kq, pq), (kt, pt) in zip(sorted((k, p) for k, p in mq.named_parameters() if p.dtype == torch.bfloat16),
                                  sorted((k, p) for k, p in mt.named_parameters() if not k.endswith(names))):
        assert kq == kt and torch.equal(pq, pt)  # the head, the embedding, the norms, the bias: bf16 and untouched
    return mq, cq, mt, ct


def prefill_and_four_steps_against_the_twin(kind, tag, prompt_lens=None):
    mq, cq, mt, ct = pair(kind)
    vocab = mq.args.vocab_size
    prompts = prompts_of(vocab) if prompt_lens is None else prompts_of(vocab, lens=prompt_lens)
    lq, lt = mq.prefill(prompts, A), mt.prefill(prompts, A)
    assert lq.dtype == torch.float32 and tuple(lq.shape) == (3, vocab) and bool(torch.isfinite(lq).all())
    print(f"W4A16MODEL {tag} prefill logits vs the bf16 twin, of the peak: {assert_close(lq, lt, LOGITS_BAR, what=(tag, 'prefill')):.3e}")
    g = torch.Generator().manual_seed(11)
    for step in range(4):
        tok = torch.randint(0, vocab, (3,), generator=g).cuda()
        dq, dt = decode_step(mq, cq, A, tok, False), decode_step(mt, ct, A, tok, False)
        print(f"W4A16MODEL {tag} decode step {step} logits vs the bf16 twin: {assert_close(dq, dt, LOGITS_BAR, what=(tag, 'decode', step)):.3e}")
    release(cq), release(ct)
    return mq, cq


def test_qwen2_with_its_bias_matches_the_twin():
    mq, _ = prefill_and_four_steps_against_the_twin("qwen2", "qwen2")
    assert mq.layers[0].attn.qkv_bias and mq.layers[0].attn.bqkv.dtype == torch.bfloat16 and mq.layers[0].attn.wqkv.dtype == torch.uint8


def test_qwen3_with_its_head_norm_matches_the_twin():
    mq, _ = prefill_and_four_steps_against_the_twin("qwen3", "qwen3")
    assert mq.layers[0].attn.qk_norm and mq.layers[0].attn.q_norm.dtype == torch.bfloat16 and mq.layers[0].attn.wqkv.dtype == torch.uint8


def test_glm4_with_its_partial_rope_matches_the_twin():
    mq, _ = prefill_and_four_steps_against_the_twin("glm4", "glm4")
    a = mq.layers[0].attn
    assert a.rotary_type == "glm4" and a.qkv_bias and a.bqkv.dtype == torch.bfloat16 and a.wqkv.dtype == torch.uint8


def test_a_prefill_long_enough_for_the_tiled_form_matches_the_twin():
    """265 prompt rows: every linear of the prefill takes the widen + tiled GEMM form"""
    from chitu_amd import ops

    rows = 150 + 70 + 45
    dim, ffn, qkv = SHAPE["dim"], SHAPE["ffn_dim"], (SHAPE["n_heads"] + 2 * SHAPE["n_kv_heads"]) * 128
    assert ops.w4a16_plan(rows, qkv, dim)["form"] == ops.w4a16_plan(rows, dim, dim)["form"] == "tiled"  # wqkv, wo
    assert ops.w4a16_plan(rows, ffn, dim, silu=True)["form"] == ops.w4a16_plan(rows, dim, ffn)["form"] == "tiled"  # w13, w2
    assert ops.w4a16_plan(3, qkv, dim)["form"] == "stream"  # the decode steps behind it
    mq, _ = prefill_and_four_steps_against_the_twin("llama", "llama-tiled-prefill", prompt_lens=(150, 70, 45))
    a, f = mq.layers[0].attn, mq.layers[0].ffn
    assert tuple(a.wqkv.shape) == (qkv, dim // 2) and tuple(a.wo.shape) == (dim, dim // 2)
    assert tuple(f.w13.shape) == (2 * ffn, dim // 2) and tuple(f.w2.shape) == (dim, ffn // 2)


def test_qwen3_decode_graph_is_the_eager_step_bit_for_bit():
    from chitu_amd.quantize import quantize_w4a16_

    mq, cq = _decoder("qwen3")
    quantize_w4a16_(mq)
    vocab = mq.args.vocab_size
    prompts = prompts_of(vocab)
    mq.prefill(prompts, A), mq.prefill(prompts, B)
    g = torch.Generator().manual_seed(12)
    for step in range(4):  # one capture, three replays
        tok = torch.randint(0, vocab, (3,), generator=g).cuda()
        eager, graph = decode_step(mq, cq, A, tok, False), decode_step(mq, cq, B, tok, True)
        assert torch.equal(eager, graph), step
    for a, b, p in zip(A, B, prompts):
        assert torch.equal(rows_of(cq, a, len(p) + 4), rows_of(cq, b, len(p) + 4))
    release(cq)
